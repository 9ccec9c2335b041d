"""The guard on reduce_q on the device: edt_partial_sum_stats_q, the scaled quantized consumes and the
transactional phase 1 against the CPU restatement (tests/reduce_q_guard_reference.py) bit for bit,
and the guarded schedule as N virtual ranks on one GPU against the unguarded run and the
restatement's composition."""
import numpy as np
import pytest
import torch

from tests import gather_q_reference as GQ
from tests import quant_reference as Q
from tests import reduce_q_guard_reference as RQ
from tests import sharded_guard_reference as G
from tests import sr_reference as S
from tests import stats_reference as R
from tests.virtual_schedules import bits, population

pytestmark = pytest.mark.gpu

F32, BF16 = torch.float32, torch.bfloat16
SIZES = [512, 1536, 66048]              # one tile; three; 65,536 + 512: the shard crosses a chunk boundary
FMTS = ["mxfp8", "mxfp4"]
OTHER = {"mxfp8": "mxfp4", "mxfp4": "mxfp8"}
SHAPES = [(37, 11), (5,), (1,), (40, 13), (129,), (31, 29), (57, 53)]    # 4,982: several buckets at world 2 and 4
CONFIGS = [(f, g, ef, rnd) for f in FMTS for g in (None, "other")
           for ef, rnd in ((True, "nearest"), (False, "nearest"), (False, "stochastic"))]
CID = [f"{f}-{'gather' if g else 'theta'}-{'ef' if ef else rnd}" for f, g, ef, rnd in CONFIGS]
EF = [(c, i) for c, i in zip(CONFIGS, CID) if c[2]]
SEED = 0x1234abcd
LR, MU, NEST = 0.7, 0.9, True


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a HIP device")
    return torch.device("cuda", 0)


def _ops():
    from evolutionarydistributedtraining_amd import ops
    return ops


def _kw(cfg):
    f, g, ef, rnd = cfg
    return dict(wire_format=f, gather_format=OTHER[f] if g else None, error_feedback=ef, rounding=rnd, seed=SEED)


def _pack(p, fmt):
    """One region of the fp32 array p (numpy) as a uint8 CPU tensor."""
    return torch.from_numpy(Q.pack(*Q.quantize(p, fmt), fmt, p.size))


# Values whose rank-ordered sum is finite in fp32 and rounds up to Inf in bf16: each is the largest
# element (448 / 6) of a block of its own scale, so it is on the grid: 1.75 (2^127 + 2^124 + 2^121 +
# 2^118) = 1.99951 * 2^127 and 1.5 (2^127 + 2^125 + ... + 2^119) = 1.99805 * 2^127, both between
# bf16's round-up threshold (2 - 2^-8) 2^127 and 2^128.
ROUND_UP = {"mxfp8": [np.ldexp(1.75, 127 - 3 * k) for k in range(4)],
            "mxfp4": [np.ldexp(1.5, 127 - 2 * k) for k in range(5)]}


def _partials(n, nacc, fmt, seed):
    """nacc fp32 partials of n elements (numpy) with what the statistics must handle planted, and
    the count of elements whose mean is not finite in (fp32, bf16)."""
    g = np.random.default_rng(seed)
    parts = [(g.standard_normal(n) * np.exp2(g.integers(-10, 2, n))).astype(np.float32) for _ in range(nacc)]
    for p in parts:
        p[64:128] = 0.0                                    # all-zero blocks on every rank: scale byte 0
    parts[0][96:128] = -0.0
    parts[nacc - 1][40] = np.nan                           # one NaN: its block of 32 ships with scale 255
    bad32 = bad16 = 32
    if nacc >= 8:                                          # the bf16 round-up, blocks 5 .. 9 of the last tile
        i = n - 512 + 5 * 32
        for k, v in enumerate(ROUND_UP[fmt]):
            for p in parts:
                p[i + 32 * k:i + 32 * k + 32] = 0.0
        for k, v in enumerate(ROUND_UP[fmt]):
            parts[k][i:i + 32] = 0.0
            parts[k][i + 7] = v
        bad16 += 1
    return parts, bad32, bad16


# ---- edt_partial_sum_stats_q -------------------------------------------------------------------

@pytest.mark.parametrize("nacc", [1, 2, 3, 4, 8])
@pytest.mark.parametrize("gdt", [F32, BF16], ids=["f32", "bf16"])
@pytest.mark.parametrize("fmt", FMTS)
def test_partial_sum_stats_q_bit_exact(dev, oracle, fmt, gdt, nacc):
    ops = _ops()
    for n in SIZES:
        parts, bad32, bad16 = _partials(n, nacc, fmt, seed=1000 * nacc + n)
        regions = [_pack(p, fmt) for p in parts]
        plan = ops.make_slerp_plan([0, n], dev)
        chunks = R.make_chunks([0, n])
        assert len(chunks) == (2 if n > 65536 else 1)
        want = RQ.mean_rows(regions, fmt, n, gdt, chunks, oracle)
        assert want[:, 1].sum() == (bad32 if gdt == F32 else bad16)          # the restatement counts the plants
        dregions = [r.to(dev) for r in regions]
        got = ops.partial_sum_stats_q(dregions, fmt, gdt, plan).cpu().numpy()
        assert R.same_bits(got, want), (n, np.argwhere(got != want)[:5])
        # the same rows as the fp32 statistics of the dequantized arrays
        deq = [d.to(dev) for d in RQ.dequantized(regions, fmt, n)]
        ref = ops.partial_sum_stats(deq, gdt, plan).cpu().numpy()
        assert R.same_bits(got, ref)
        for r, d in zip(regions, dregions):                                  # read only
            assert torch.equal(d.cpu(), r)


def test_partial_sum_stats_q_wrapper_refusals(dev):
    ops, L = _ops(), __import__("evolutionarydistributedtraining_amd._lib", fromlist=["EdtError"])
    n = 1024
    reg = torch.zeros(ops.q_region_bytes(n, "mxfp8"), dtype=torch.uint8, device=dev)
    plan = ops.make_slerp_plan([0, n], dev)
    assert not ops.partial_sum_stats_q([reg], "mxfp8", F32, plan).cpu().any()      # zero bytes: D = +0
    with pytest.raises(L.EdtError):
        ops.partial_sum_stats_q([reg], "mxfp4", F32, plan)                         # another format's size
    with pytest.raises(L.EdtError):
        ops.partial_sum_stats_q([reg], "mxfp8", F32, ops.make_slerp_plan([0, 4, n], dev))
    with pytest.raises(L.EdtError):
        ops.partial_sum_stats_q([], "mxfp8", F32, plan)


# ---- the scaled consumes -----------------------------------------------------------------------

def _consume_case(n, gdt, fmt, dev, seed, nacc=3):
    g = torch.Generator().manual_seed(seed)
    theta = (torch.randn(n, generator=g) * 0.5).to(gdt)
    mom = (torch.randn(n, generator=g) * 0.01).to(gdt)
    rg = np.random.default_rng(seed)
    regions = [_pack((rg.standard_normal(n) * 0.01).astype(np.float32), fmt) for _ in range(nacc)]
    res = torch.randn(n, generator=g) * 1e-4
    return theta, mom, regions, res


@pytest.mark.parametrize("gdt", [F32, BF16], ids=["f32", "bf16"])
@pytest.mark.parametrize("fmt", FMTS)
def test_scaled_consumes_at_one_are_the_plain_entries(dev, fmt, gdt):
    ops, n, fo = _ops(), 1536, OTHER[fmt]
    theta, mom, regions, res = _consume_case(n, gdt, fmt, dev, seed=5)
    dreg = [r.to(dev) for r in regions]
    hp = (True, LR, MU, NEST)

    def run(fn, *tail, **kw):
        th, m, r = theta.to(dev), mom.to(dev), res.to(dev)
        out = torch.zeros(ops.q_region_bytes(n, fo), dtype=torch.uint8, device=dev)
        fn(th, m, r, out, *tail, **kw)
        return [bits(th).cpu(), bits(m).cpu(), bits(r).cpu(), out.cpu()]
    a = run(lambda th, m, r, out: ops.sgd_apply_sum_q(th, dreg, fmt, m, *hp))
    b = run(lambda th, m, r, out: ops.sgd_apply_sum_q_scaled(th, dreg, fmt, m, *hp, 1.0))
    assert all(torch.equal(x, y) for x, y in zip(a, b)) and not torch.equal(a[0], bits(theta))
    a = run(lambda th, m, r, out: ops.sgd_delta_sum_q(th, dreg, fmt, m, *hp, out, fo, r))
    b = run(lambda th, m, r, out: ops.sgd_delta_sum_q_scaled(th, dreg, fmt, m, *hp, out, fo, 1.0, r))
    assert all(torch.equal(x, y) for x, y in zip(a, b)) and torch.equal(a[0], bits(theta)) and a[3].any()
    sr = dict(rounding="stochastic", seed=SEED, step=3, stream_id=5, elem_base=4096)
    a = run(lambda th, m, r, out: ops.sgd_delta_sum_q(th, dreg, fmt, m, *hp, out, fo, **sr))
    b = run(lambda th, m, r, out: ops.sgd_delta_sum_q_scaled(th, dreg, fmt, m, *hp, out, fo, 1.0, **sr))
    assert all(torch.equal(x, y) for x, y in zip(a, b)) and a[3].any()


@pytest.mark.parametrize("c", [0.5, 0.37])
@pytest.mark.parametrize("gdt", [F32, BF16], ids=["f32", "bf16"])
@pytest.mark.parametrize("fmt", FMTS)
def test_scaled_consumes_are_the_composition(dev, fmt, gdt, c):
    """dequantize -> edt_sgd_apply_sum_scaled on a clone; phase 2': the numpy update restatement on
    that clone's theta' - theta."""
    ops, n, fo = _ops(), 1536, OTHER[fmt]
    theta, mom, regions, res = _consume_case(n, gdt, fmt, dev, seed=11)
    dreg = [r.to(dev) for r in regions]
    deq = [d.to(dev) for d in RQ.dequantized(regions, fmt, n)]
    hp = (True, LR, MU, NEST)
    th_ref, m_ref = theta.to(dev), mom.to(dev)
    ops.sgd_apply_sum_scaled(th_ref, deq, m_ref, *hp, c)
    th, m = theta.to(dev), mom.to(dev)
    ops.sgd_apply_sum_q_scaled(th, dreg, fmt, m, *hp, c)
    assert torch.equal(bits(th), bits(th_ref)) and torch.equal(bits(m), bits(m_ref))
    plain = theta.to(dev)
    ops.sgd_apply_sum_q(plain, dreg, fmt, mom.to(dev), *hp)
    assert not torch.equal(bits(plain), bits(th))                                # the clip is seen
    # phase 2' with error feedback
    th, m, r = theta.to(dev), mom.to(dev), res.to(dev)
    out = torch.zeros(ops.q_region_bytes(n, fo), dtype=torch.uint8, device=dev)
    ops.sgd_delta_sum_q_scaled(th, dreg, fmt, m, *hp, out, fo, c, r)
    codes, scales, _, r_ref = GQ.delta_step(theta, th_ref.cpu(), res.numpy(), fo)
    assert torch.equal(bits(th).cpu(), bits(theta)) and torch.equal(bits(m), bits(m_ref))
    assert np.array_equal(out.cpu().numpy(), Q.pack(codes, scales, fo, n))
    assert np.array_equal(r.cpu().numpy().view(np.int32), r_ref.view(np.int32))
    # and with stochastic rounding
    th, m = theta.to(dev), mom.to(dev)
    ops.sgd_delta_sum_q_scaled(th, dreg, fmt, m, *hp, out, fo, c, rounding="stochastic", seed=SEED, step=2,
                               stream_id=3, elem_base=2048)
    with np.errstate(invalid="ignore"):
        u = (GQ._f32(th_ref.cpu()) - GQ._f32(theta)).astype(np.float32)
    codes, scales = S.sr_quantize(u, fo, SEED, 2, 3, 2048)
    assert torch.equal(bits(m), bits(m_ref)) and np.array_equal(out.cpu().numpy(), Q.pack(codes, scales, fo, n))


# ---- the transactional phase 1 -----------------------------------------------------------------

@pytest.mark.parametrize("K", [2, 3, 8])
@pytest.mark.parametrize("tdt,wdt", [(F32, BF16), (F32, F32), (BF16, BF16)], ids=["f32-bf16", "f32-f32", "bf16-bf16"])
@pytest.mark.parametrize("fmt", FMTS)
def test_delta_partial_q_residual_out(dev, fmt, tdt, wdt, K):
    ops, n, per = _ops(), 3072, 1536
    theta, workers = R.operands(n, K, tdt, wdt, seed=K)
    th, ws = theta.to(dev), [w.to(dev) for w in workers]
    res0 = torch.randn(n, generator=torch.Generator().manual_seed(1)) * 1e-4
    nb = n // per * ops.q_region_bytes(per, fmt)
    a_res, a_q = res0.to(dev), torch.zeros(nb, dtype=torch.uint8, device=dev)
    ops.delta_partial_q(th, ws, K, a_q, per, fmt, a_res)                          # in place
    b_in, b_out = res0.to(dev), torch.full((n,), 7.0, device=dev)
    b_q = torch.zeros(nb, dtype=torch.uint8, device=dev)
    ops.delta_partial_q(th, ws, K, b_q, per, fmt, b_in, residual_out=b_out)
    assert torch.equal(a_q, b_q) and torch.equal(bits(a_res), bits(b_out))
    assert torch.equal(bits(b_in).cpu(), bits(res0)) and not torch.equal(bits(b_out).cpu(), bits(res0))
    c_res, c_q = res0.to(dev), torch.zeros(nb, dtype=torch.uint8, device=dev)
    ops.delta_partial_q(th, ws, K, c_q, per, fmt, c_res, residual_out=c_res)      # the same buffer: in place
    assert torch.equal(a_q, c_q) and torch.equal(bits(a_res), bits(c_res))
    from evolutionarydistributedtraining_amd._lib import EdtError
    with pytest.raises(EdtError):
        ops.delta_partial_q(th, ws, K, b_q, per, fmt, None, residual_out=b_out)
    big = torch.zeros(2 * n, device=dev)                                          # overlapping, not the same
    with pytest.raises(EdtError):
        ops.delta_partial_q(th, ws, K, b_q, per, fmt, big[:n], residual_out=big[8:n + 8])


# ---- the schedules on virtual ranks ------------------------------------------------------------

def _run(dev, world, cfg, K=None, steps=2, **kw):
    K = K or 2 * world
    layout, theta, gens = population(SHAPES, F32, BF16, K, steps=steps)
    res = RQ.run_q(world, layout, F32, BF16, theta, gens, dev, bucket_elems=1024, **_kw(cfg), **kw)
    return layout, theta, gens, res


def _same_stats(res):
    for r in res[1:]:
        assert repr(r["stats"]) == repr(res[0]["stats"])


def test_constructor_accepts_the_guard(dev):
    """Fails without the feature: guard= with mode='reduce_q' was refused."""
    from evolutionarydistributedtraining_amd.diloco import OuterGuard
    _, _, _, res = _run(dev, 2, CONFIGS[0], steps=1, guard=OuterGuard(max_grad_norm=1.0, on_nonfinite="drop"))
    _same_stats(res)
    assert res[0]["errors"] == [None] and res[0]["stats"][0]["clip_coef"] is not None


@pytest.mark.parametrize("world", [2, 4])
@pytest.mark.parametrize("cfg", CONFIGS, ids=CID)
def test_finite_unclipped_guard_is_the_unguarded_step(dev, world, cfg):
    from evolutionarydistributedtraining_amd.diloco import OuterGuard
    layout, theta, gens, res = _run(dev, world, cfg, guard=OuterGuard(max_grad_norm=1e30))
    _, _, _, plain = _run(dev, world, cfg)
    assert len(res[0]["buckets"]) >= 2 and res[0]["n_pad"] > layout.total
    _same_stats(res)
    for r, p in zip(res, plain):
        assert r["errors"] == [None, None]
        for a, b in zip(r["steps"], p["steps"]):
            assert RQ.same_state(a, b)
        assert torch.equal(r["q_send"], p["q_send"]) and torch.equal(r["q_recv"], p["q_recv"])
    st = res[0]["stats"][-1]
    assert st["clip_coef"] == 1.0 and st["dropped"] == [] and st["nonfinite_mean"] == 0 and st["grad_norm"] > 0


@pytest.mark.parametrize("world", [2, 4])
@pytest.mark.parametrize("cfg", CONFIGS, ids=CID)
def test_raise_writes_nothing_and_the_next_step_works(dev, world, cfg):
    from evolutionarydistributedtraining_amd.diloco import NonFiniteWorkers, OuterGuard
    K, bad = 2 * world, 3
    layout, theta, gens, res = _run(dev, world, cfg, steps=3, guard=OuterGuard(), poison={1: [(bad, 17, float("nan"))]})
    _same_stats(res)
    for r in res:
        assert r["errors"][0] is None and r["errors"][2] is None
        err = r["errors"][1]
        assert isinstance(err, NonFiniteWorkers) and err.nonfinite == [int(k == bad) for k in range(K)]
        assert RQ.same_state(r["before"], r["after"]) and r["after"]["q_step"] == 1
    plain = RQ.run_q(world, layout, F32, BF16, theta, [gens[0], gens[2]], dev, bucket_elems=1024, **_kw(cfg))
    for r, p in zip(res, plain):
        assert RQ.same_state(r["steps"][-1], p["steps"][-1])


@pytest.mark.parametrize("world,K", [(2, 2), (4, 8)])              # (2, 2): K_local = 1, rank 1 is emptied
@pytest.mark.parametrize("cfg", CONFIGS, ids=CID)
def test_drop_is_the_composition_over_the_survivors(dev, oracle, world, K, cfg):
    from evolutionarydistributedtraining_amd.diloco import OuterGuard
    bad = K // world
    layout, theta, gens, res = _run(dev, world, cfg, K=K, guard=OuterGuard(on_nonfinite="drop"),
                                    poison={1: [(bad, 5, float("inf"))]})
    _same_stats(res)
    st = res[0]["stats"][1]
    assert st["dropped"] == [bad] and st["clip_coef"] == 1.0 and st["nonfinite_mean"] == 0
    n_pad, buckets = res[0]["n_pad"], res[0]["buckets"]
    state = RQ.state0(theta, n_pad, world, cfg)
    f_in, f_out = cfg[0], OTHER[cfg[0]] if cfg[1] else None
    RQ.compose(oracle, state, [G.padded(w, n_pad) for w in gens[0]], world, buckets, f_in, f_out, list(range(K)), 1.0,
               cfg[3], SEED)
    ws = [G.padded(w, n_pad) for w in gens[1]]
    ws[bad][5] = float("inf")
    s_mm, _ = RQ.compose(oracle, state, ws, world, buckets, f_in, f_out, [k for k in range(K) if k != bad], 1.0,
                         cfg[3], SEED)
    assert st["grad_norm"] == s_mm ** 0.5
    RQ.assert_is_state(res, state, cfg)
    if K // world == 1:
        assert not res[1]["q_send"].any()
        if cfg[2]:
            assert torch.equal(res[1]["steps"][1]["residual"], res[1]["steps"][0]["residual"])


@pytest.mark.parametrize("world", [2, 4])
@pytest.mark.parametrize("cfg", CONFIGS, ids=CID)
def test_clip_is_the_scaled_composition(dev, oracle, world, cfg):
    from evolutionarydistributedtraining_amd.diloco import OuterGuard, clip_coefficient
    K = 2 * world
    _, _, _, first = _run(dev, world, cfg, steps=1, guard=OuterGuard())
    norm = first[0]["stats"][0]["grad_norm"]
    layout, theta, gens, res = _run(dev, world, cfg, guard=OuterGuard(max_grad_norm=norm / 2))
    _same_stats(res)
    n_pad, buckets = res[0]["n_pad"], res[0]["buckets"]
    state = RQ.state0(theta, n_pad, world, cfg)
    f_in, f_out = cfg[0], OTHER[cfg[0]] if cfg[1] else None
    for g in range(2):
        st = res[0]["stats"][g]
        assert st["clip_coef"] == clip_coefficient(st["grad_norm"] ** 2, norm / 2) and st["clip_coef"] < 1.0
        s_mm, _ = RQ.compose(oracle, state, [G.padded(w, n_pad) for w in gens[g]], world, buckets, f_in, f_out,
                             list(range(K)), st["clip_coef"], cfg[3], SEED)
        assert st["grad_norm"] == s_mm ** 0.5
    RQ.assert_is_state(res, state, cfg)


BLOCK0 = 640                             # a block of 32 inside rank 1's shard of the first bucket


@pytest.mark.parametrize("world", [2, 4])
@pytest.mark.parametrize("cfg,cid", EF, ids=[i for _, i in EF])
def test_refusal_after_the_exchange_restores_the_residual(dev, world, cfg, cid):
    """Finite workers, but rank 1's p + r overflows in one block (a planted residual of 3.3e38 under
    positive deltas of about 1e38): scale byte 255, nonfinite_mean exactly 32 (the restatement's
    count: tests/test_reduce_q_guard_cpu.py), NonFiniteWorkers on every rank, every buffer as before."""
    from evolutionarydistributedtraining_amd.diloco import NonFiniteWorkers, OuterGuard
    K = 2 * world
    layout, theta, gens = population(SHAPES, F32, BF16, K, steps=3)
    for w in gens[1]:
        w[BLOCK0:BLOCK0 + 32] = (theta[BLOCK0:BLOCK0 + 32].float() + 1e38).to(w.dtype)
    saved = {}

    def prepare(sync, g):
        if g == 1 and sync.rank == 1:
            saved["r"] = sync.residual[BLOCK0:BLOCK0 + 32].clone()
            sync.residual[BLOCK0:BLOCK0 + 32] = 3.3e38
        if g == 2 and sync.rank == 1:
            sync.residual[BLOCK0:BLOCK0 + 32] = saved["r"]
    res = RQ.run_q(world, layout, F32, BF16, theta, gens, dev, bucket_elems=1024, guard=OuterGuard(), prepare=prepare,
                   **_kw(cfg))
    _same_stats(res)
    st = res[0]["stats"][1]
    assert st["nonfinite_mean"] == 32 and st["nonfinite"] == [0] * K
    for r in res:
        assert r["errors"][0] is None and r["errors"][2] is None
        assert isinstance(r["errors"][1], NonFiniteWorkers) and r["errors"][1].nonfinite_mean == 32
        assert RQ.same_state(r["before"], r["after"])
    assert res[1]["after"]["residual"][BLOCK0].item() == pytest.approx(3.3e38)
    plain = RQ.run_q(world, layout, F32, BF16, theta, [gens[0], gens[2]], dev, bucket_elems=1024, **_kw(cfg))
    for r, p in zip(res, plain):
        assert RQ.same_state(r["steps"][-1], p["steps"][-1])


@pytest.mark.parametrize("world", [2, 4])
@pytest.mark.parametrize("cfg", CONFIGS, ids=CID)
def test_guarded_broadcast_is_step_plus_copy(dev, world, cfg):
    from evolutionarydistributedtraining_amd.diloco import OuterGuard
    _, _, _, first = _run(dev, world, cfg, steps=1, guard=OuterGuard())
    guard = OuterGuard(max_grad_norm=first[0]["stats"][0]["grad_norm"] / 2)
    _, _, _, a = _run(dev, world, cfg, guard=guard, step_kw={"broadcast": True})
    _, _, _, b = _run(dev, world, cfg, guard=guard)
    for x, y in zip(a, b):
        sx, sy = x["steps"][-1], y["steps"][-1]
        want = dict(sy, workers=[sy["theta_buf"].to(BF16) for _ in sy["workers"]])
        assert RQ.same_state(sx, want)
