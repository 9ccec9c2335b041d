"""edt_partial_sum_stats, the scaled sharded SGD entries and ShardedOuterSync(guard=...) on the device:
the kernels against the CPU restatement (tests/sharded_guard_reference.py) bit for bit, and the
guarded schedules as N virtual ranks on one GPU (collectives.VirtualWorld) against the unguarded
run, the restatement's totals, the single-device guard's figures and the compositions."""
import numpy as np
import pytest
import torch

from tests import sharded_guard_reference as G
from tests import stats_reference as R
from tests.virtual_schedules import bits, population

pytestmark = pytest.mark.gpu

F32, BF16 = torch.float32, torch.bfloat16
SIZES = [1, 511, 513, 65536, 65537, 70518]
LAYOUT = [0, 5, 70006, 70518]          # chunk starts off 8, a segment longer than one chunk
SHAPES = [(37, 11), (5,), (1,), (40, 13), (129,)]          # 1,062 elements: no multiple of a unit
BIG = [(3, 9001), (70001,), (43007,)]                      # 140,011: a shard of world 2 crosses a chunk
MODES = [("reduce", "theta"), ("reduce_ordered", "theta"), ("exact", "theta"), ("exact", "workers")]
MID = ["reduce", "reduce_ordered", "exact-theta", "exact-workers"]
LR, MU, NEST = 0.7, 0.9, True


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a HIP device")
    return torch.device("cuda", 0)


def _ops():
    from evolutionarydistributedtraining_amd import ops
    return ops


def _partials(n, nacc, seed):
    gen = torch.Generator().manual_seed(seed)
    parts = [torch.randn(n, generator=gen) * 0.01 for _ in range(nacc)]
    for j, v in enumerate([0.0, -0.0, 1e-40, -1e-40]):     # signed zeros and subnormals
        if n > j:
            parts[j % nacc][j] = v
    return parts


def _check_rows(parts, gdt, offsets, dev, oracle, what, shift=False):
    ops = _ops()
    n = parts[0].numel()
    plan = ops.make_slerp_plan(list(offsets), dev)

    def put(p):
        buf = torch.empty(n + 4, dtype=F32, device=dev)
        v = buf[1:n + 1] if shift else buf[:n]
        v.copy_(p)
        assert (v.data_ptr() % 16 != 0) == shift
        return v
    got = ops.partial_sum_stats([put(p) for p in parts], gdt, plan).cpu().numpy()
    want = G.partial_sum_rows(parts, gdt, R.make_chunks(offsets), oracle)
    assert R.same_bits(got, want), (what, np.argwhere(got != want)[:5], got.shape)
    return got


# ---- edt_partial_sum_stats ---------------------------------------------------------------------

@pytest.mark.parametrize("nacc", [1, 2, 3, 8])
@pytest.mark.parametrize("gdt", [F32, BF16], ids=["f32", "bf16"])
def test_partial_sum_stats_bit_exact(dev, oracle, gdt, nacc):
    for n in SIZES:
        parts = _partials(n, nacc, seed=100 * nacc + n)
        _check_rows(parts, gdt, LAYOUT if n == LAYOUT[-1] else [0, n], dev, oracle, (n, nacc))


@pytest.mark.parametrize("gdt", [F32, BF16], ids=["f32", "bf16"])
def test_partial_sum_stats_off_alignment(dev, oracle, gdt):
    """Every pointer one float off a 16-byte boundary: scalar loads, the same bits."""
    for nacc in (1, 3):
        parts = _partials(LAYOUT[-1], nacc, seed=7 + nacc)
        a = _check_rows(parts, gdt, LAYOUT, dev, oracle, ("shift", nacc), shift=True)
        b = _check_rows(parts, gdt, LAYOUT, dev, oracle, ("aligned", nacc))
        assert R.same_bits(a, b)


@pytest.mark.parametrize("gdt", [F32, BF16], ids=["f32", "bf16"])
def test_partial_sum_stats_masks_what_is_not_finite(dev, oracle, gdt):
    n, nacc = LAYOUT[-1], 3
    parts = _partials(n, nacc, seed=31)
    clean = [p.clone() for p in parts]
    spots = {0: "nan", 511: "inf", 5 + 65536: "overflow", n - 1: "nan"}
    if gdt == BF16:
        spots[70000] = "round"          # finite in fp32, rounds up to Inf in bf16
    for i, kind in spots.items():
        for p in parts:
            p[i] = 0.0
        if kind == "nan":
            parts[1][i] = float("nan")
        elif kind == "inf":
            parts[2][i] = float("inf")
        elif kind == "overflow":
            parts[0][i], parts[1][i] = 3e38, 3e38          # each finite, the sum is not
        else:
            parts[0][i] = 3.4e38
        for p in clean:
            p[i] = 0.0
    got = _check_rows(parts, gdt, LAYOUT, dev, oracle, "masked")
    assert got[:, 1].sum() == len(spots)
    chunks = R.make_chunks(LAYOUT)
    assert got[:, 1].tolist() == [sum(1 for i in spots if a <= i < a + ln) for a, ln, _ in chunks]
    # the counted elements are absent from S_mm: the same sums as with zeros in their place
    zeroed = _check_rows(clean, gdt, LAYOUT, dev, oracle, "zeroed")
    assert R.same_bits(got[:, 0], zeroed[:, 0]) and zeroed[:, 1].sum() == 0


# ---- the scaled sharded SGD entries ------------------------------------------------------------

def _sgd_case(n, nacc, gdt, seed):
    gen = torch.Generator().manual_seed(seed)
    theta = (torch.randn(n, generator=gen) * 0.5).to(gdt)
    gens = [[torch.randn(n, generator=gen) * 0.01 for _ in range(nacc)] for _ in range(2)]
    return theta, gens


@pytest.mark.parametrize("nacc", [1, 3, 8])
@pytest.mark.parametrize("gdt", [F32, BF16], ids=["f32", "bf16"])
def test_scaled_sgd_at_one_is_the_unscaled_entry(dev, gdt, nacc):
    ops = _ops()
    for n in (1, 513, 70518):
        theta, gens = _sgd_case(n, nacc, gdt, seed=n + nacc)
        t = [theta.to(dev) for _ in range(4)]
        m = [torch.zeros(n, dtype=gdt, device=dev) for _ in range(4)]
        for g, parts in enumerate(gens):                   # the second generation carries the momentum
            ps = [p.to(dev) for p in parts]
            ops.sgd_apply_sum(t[0], ps, m[0], g > 0, LR, MU, NEST)
            ops.sgd_apply_sum_scaled(t[1], ps, m[1], g > 0, LR, MU, NEST, 1.0)
            ops.sgd_apply(t[2], ps[0], m[2], g > 0, LR, MU, NEST)
            ops.sgd_apply_scaled(t[3], ps[0], m[3], g > 0, LR, MU, NEST, 1.0)
            for a, b in ((0, 1), (2, 3)):
                assert torch.equal(bits(t[a]), bits(t[b])) and torch.equal(bits(m[a]), bits(m[b])), (n, g, a)


@pytest.mark.parametrize("c", [0.5, 0.3, 0.0])
@pytest.mark.parametrize("nacc", [1, 3, 8])
@pytest.mark.parametrize("gdt", [F32, BF16], ids=["f32", "bf16"])
def test_scaled_sgd_composition(dev, oracle, gdt, nacc, c):
    ops = _ops()
    for n in (1, 513, 70518):
        theta, gens = _sgd_case(n, nacc, gdt, seed=3 * n + nacc)
        ref_t, ref_m = theta.clone(), torch.zeros_like(theta)
        one_t, one_m = theta.clone(), torch.zeros_like(theta)
        sum_t, sum_m = theta.to(dev), torch.zeros(n, dtype=gdt, device=dev)
        app_t, app_m = theta.to(dev), torch.zeros(n, dtype=gdt, device=dev)
        for g, parts in enumerate(gens):
            G.sgd_apply_scaled(oracle, ref_t, G.partial_mean(parts, F32), ref_m, g > 0, LR, MU, NEST, c)
            G.sgd_apply_scaled(oracle, one_t, parts[0], one_m, g > 0, LR, MU, NEST, c)
            ops.sgd_apply_sum_scaled(sum_t, [p.to(dev) for p in parts], sum_m, g > 0, LR, MU, NEST, c)
            ops.sgd_apply_scaled(app_t, parts[0].to(dev), app_m, g > 0, LR, MU, NEST, c)
            assert torch.equal(bits(sum_t.cpu()), bits(ref_t)) and torch.equal(bits(sum_m.cpu()), bits(ref_m)), (n, g)
            assert torch.equal(bits(app_t.cpu()), bits(one_t)) and torch.equal(bits(app_m.cpu()), bits(one_m)), (n, g)


def test_scaled_sgd_refuses_a_bad_scale(dev):
    from evolutionarydistributedtraining_amd._lib import EdtError
    ops = _ops()
    n = 513
    theta, gens = _sgd_case(n, 2, F32, seed=5)
    t, m = theta.to(dev), torch.zeros(n, device=dev)
    ps = [p.to(dev) for p in gens[0]]
    for bad in (float("nan"), 1.5, -0.1, float("inf")):
        with pytest.raises(EdtError, match="grad_scale"):
            ops.sgd_apply_sum_scaled(t, ps, m, False, LR, MU, NEST, bad)
        with pytest.raises(EdtError, match="grad_scale"):
            ops.sgd_apply_scaled(t, ps[0], m, False, LR, MU, NEST, bad)
    assert torch.equal(bits(t.cpu()), bits(theta)) and not m.any()


def test_plain_sgd_refuses_a_wrong_dtype_momentum(dev):
    """The plain entries check the momentum as the scaled ones do: a bf16 momentum under an fp32
    theta is refused before anything is launched (the kernel would reinterpret its bytes)."""
    from evolutionarydistributedtraining_amd._lib import EdtError
    ops = _ops()
    n = 64
    theta, gens = _sgd_case(n, 2, F32, seed=11)
    t, m = theta.to(dev), torch.zeros(n, dtype=BF16, device=dev)
    ps = [p.to(dev) for p in gens[0]]
    with pytest.raises(EdtError, match="momentum must have theta's size and dtype"):
        ops.sgd_apply(t, ps[0], m, False, LR, 0.9, NEST)
    with pytest.raises(EdtError, match="momentum must have theta's size and dtype"):
        ops.sgd_apply_sum(t, ps, m, False, LR, 0.9, NEST)
    torch.cuda.synchronize()
    assert torch.equal(bits(t.cpu()), bits(theta)) and not m.any()


# ---- ShardedOuterSync(guard=...) on virtual ranks -----------------------------------------------

def _guard(**kw):
    from evolutionarydistributedtraining_amd.diloco import OuterGuard
    return OuterGuard(**kw)


def _single_device_stats(layout, tdt, wdt, theta, workers, dev):
    """(S_mm, S_kk) of the single-device guard: OuterSync(guard=...)'s figures before their square
    roots (the same pass over the same plan: checked against its last_stats)."""
    from evolutionarydistributedtraining_amd.diloco import OuterSync, stats_totals
    from evolutionarydistributedtraining_amd.params import ParamArena
    ops = _ops()
    rows = ops.delta_stats(theta, workers, ops.make_slerp_plan([0, layout.total], dev)).cpu().numpy()
    t = stats_totals(rows, len(workers))
    th = ParamArena(layout, tdt, dev, theta.clone())
    ws = [ParamArena(layout, wdt, dev, w.clone()) for w in workers]
    sync = OuterSync(th, ws, LR, MU, NEST, guard=_guard())
    sync.step()
    assert sync.last_stats["grad_norm"] == t["S_mm"] ** 0.5
    assert sync.last_stats["worker_norms"] == np.sqrt(t["S_kk"]).tolist()
    return t["S_mm"], t["S_kk"]


def _finite_case(dev, oracle, world, mode, broadcast, shapes, bucket_elems, tdt, wdt, K):
    layout, theta, gens = population(shapes, tdt, wdt, K, steps=2, device=dev)
    n = layout.total
    kw = dict(mode=mode, broadcast=broadcast, bucket_elems=bucket_elems)
    res = G.run_guarded(world, layout, tdt, wdt, theta, gens, dev, guard=_guard(max_grad_norm=1e9), **kw)
    plain = G.run_guarded(world, layout, tdt, wdt, theta, gens, dev, **kw)
    torch.cuda.synchronize()
    what = (world, mode, broadcast, tdt, K)
    assert res[0]["n_pad"] > n, what
    for r, p in zip(res, plain):
        assert repr(r["stats"]) == repr(res[0]["stats"]), what
        assert p["stats"] == [None, None]
        assert torch.equal(bits(r["theta_buf"]), bits(p["theta_buf"])), what
        assert torch.equal(bits(r["mom_shard"]), bits(p["mom_shard"])), what
        for a, b in zip(r["workers"], p["workers"]):
            assert torch.equal(bits(a), bits(b)), what
    n_pad = res[0]["n_pad"]
    th0 = G.padded(theta, n_pad)
    ws0 = [G.padded(w, n_pad) for w in gens[0]]
    st = res[0]["stats"][0]
    assert st["clip_coef"] == 1.0 and st["dropped"] == [] and st["nonfinite"] == [0] * K and st["nonfinite_mean"] == 0
    one_mm, one_kk = _single_device_stats(layout, tdt, wdt, theta, gens[0], dev)
    bound = 2 * n * 2.0 ** -53
    if mode == "exact":
        t = G.exact_stats(oracle, th0, ws0, world, bucket_elems)
        s_mm, s_kk = float(t[0]), t[1:K + 1]
        # m is element-wise the fused step's: only the fp64 summation order differs
        print("S_mm", what, s_mm, one_mm, abs(s_mm - one_mm) / s_mm, bound)
        assert abs(s_mm - one_mm) <= bound * s_mm, what
        assert (st["cos_to_mean"] is not None) == (K <= 8)
    else:
        s_mm, nfm, s_kk, nf, _ = G.reduce_stats(oracle, th0, ws0, world, bucket_elems)
        assert nfm == 0 and st["cos_to_mean"] is None
    assert st["grad_norm"] == s_mm ** 0.5, what
    assert st["worker_norms"] == np.sqrt(s_kk).tolist(), what
    for a, b in zip(s_kk, one_kk):
        assert abs(a - b) <= bound * a, what


@pytest.mark.parametrize("world", [2, 4])
@pytest.mark.parametrize("mode,broadcast", MODES, ids=MID)
def test_finite_unclipped_guard_is_the_unguarded_step(dev, oracle, world, mode, broadcast):
    for tdt, wdt in ((F32, BF16), (BF16, BF16)):
        for K in (4, 8):
            _finite_case(dev, oracle, world, mode, broadcast, SHAPES, 1024, tdt, wdt, K)


@pytest.mark.parametrize("mode,broadcast", MODES, ids=MID)
def test_a_shard_that_crosses_a_chunk(dev, oracle, mode, broadcast):
    _finite_case(dev, oracle, 2, mode, broadcast, BIG, 1 << 18, F32, BF16, 4)


@pytest.mark.parametrize("world", [2, 4])
@pytest.mark.parametrize("mode,broadcast", MODES, ids=MID)
def test_nan_worker_raises_on_every_rank(dev, world, mode, broadcast):
    from evolutionarydistributedtraining_amd.diloco import NonFiniteWorkers
    K = 8
    bad = K // world + 1 if world == 2 else K // world     # a worker of rank 1
    layout, theta, gens = population(SHAPES, F32, BF16, K, steps=3, device=dev)
    kw = dict(mode=mode, broadcast=broadcast, bucket_elems=1024)
    res = G.run_guarded(world, layout, F32, BF16, theta, gens, dev, guard=_guard(),
                        poison={1: [(bad, 17, float("nan"))]}, **kw)
    plain = G.run_guarded(world, layout, F32, BF16, theta, [gens[0], gens[2]], dev, **kw)
    torch.cuda.synchronize()
    for r, p in zip(res, plain):
        assert repr(r["stats"]) == repr(res[0]["stats"])
        assert r["errors"][0] is None and r["errors"][2] is None
        err = r["errors"][1]
        assert isinstance(err, NonFiniteWorkers) and err.nonfinite == [int(k == bad) for k in range(K)]
        assert G.same_buffers(r["before"], r["after"]) and r["before"]["has_momentum"] is True
        # the following finite step equals the unguarded one
        assert torch.equal(bits(r["theta_buf"]), bits(p["theta_buf"]))
        assert torch.equal(bits(r["mom_shard"]), bits(p["mom_shard"]))


@pytest.mark.parametrize("world,K", [(2, 4), (4, 4)])      # (4, 4): K_local = 1, rank 1 is emptied
@pytest.mark.parametrize("mode,broadcast", MODES, ids=MID)
def test_nan_worker_is_dropped(dev, oracle, world, K, mode, broadcast):
    ops = _ops()
    bad = K // world
    layout, theta, gens = population(SHAPES, F32, BF16, K, steps=1, device=dev)
    res = G.run_guarded(world, layout, F32, BF16, theta, gens, dev, mode=mode, broadcast=broadcast, bucket_elems=1024,
                        guard=_guard(on_nonfinite="drop"), poison={0: [(bad, 17, float("nan"))]})
    torch.cuda.synchronize()
    n, n_pad = layout.total, res[0]["n_pad"]
    survivors = [k for k in range(K) if k != bad]
    st = res[0]["stats"][0]
    assert st["dropped"] == [bad] and st["nonfinite"] == [int(k == bad) for k in range(K)]
    assert st["clip_coef"] == 1.0 and st["nonfinite_mean"] == 0
    if mode == "exact":
        th, mom = theta.clone(), torch.zeros_like(theta)
        ops.outer_step(th, [gens[0][k] for k in survivors], mom, False, LR, MU, NEST)
        th, mom = th.cpu(), mom.cpu()
    else:
        ws = [G.padded(w, n_pad) for w in gens[0]]
        ws[bad][17] = float("nan")
        th = G.padded(theta, n_pad)
        s_mm, _, _, _, parts = G.reduce_stats(oracle, th, ws, world, 1024, survivors)
        assert st["grad_norm"] == s_mm ** 0.5
        mom = torch.zeros_like(th)
        oracle.sgd_apply(th, G.partial_mean(parts, F32), mom, False, LR, MU, NEST)
    for r in res:
        assert repr(r["stats"]) == repr(res[0]["stats"])
        assert torch.equal(bits(r["theta"].cpu()), bits(th[:n]))
        assert torch.equal(bits(r["mom"][:n].cpu()), bits(mom[:n]))


@pytest.mark.parametrize("world", [2, 4])
@pytest.mark.parametrize("mode,broadcast", MODES, ids=MID)
def test_clipped_step_is_the_composition(dev, oracle, world, mode, broadcast):
    from evolutionarydistributedtraining_amd.diloco import clip_coefficient
    K = 8
    for tdt in (F32, BF16):
        layout, theta, gens = population(SHAPES, tdt, BF16, K, steps=1, device=dev)
        kw = dict(mode=mode, broadcast=broadcast, bucket_elems=1024)
        first = G.run_guarded(world, layout, tdt, BF16, theta, gens, dev, guard=_guard(), **kw)
        norm = first[0]["stats"][0]["grad_norm"]
        res = G.run_guarded(world, layout, tdt, BF16, theta, gens, dev, guard=_guard(max_grad_norm=norm / 2), **kw)
        torch.cuda.synchronize()
        st = res[0]["stats"][0]
        assert st["grad_norm"] == norm
        assert st["clip_coef"] == clip_coefficient(st["grad_norm"] ** 2, norm / 2) and 0.49 < st["clip_coef"] < 0.51
        n, n_pad = layout.total, res[0]["n_pad"]
        th = G.padded(theta, n_pad)
        ws = [G.padded(w, n_pad) for w in gens[0]]
        mom = torch.zeros_like(th)
        if mode == "exact":
            acc = R.deltas_and_mean(th, ws)[1].float()
        else:
            acc = G.partial_mean(G.reduce_partials(oracle, th, ws, world, list(range(K))), F32)
        G.sgd_apply_scaled(oracle, th, acc, mom, False, LR, MU, NEST, st["clip_coef"])
        for r in res:
            assert repr(r["stats"]) == repr(res[0]["stats"])
            assert torch.equal(bits(r["theta"].cpu()), bits(th[:n])), (tdt, "theta")
            assert torch.equal(bits(r["mom"].cpu()), bits(mom)), (tdt, "momentum")
            assert torch.equal(bits(r["theta"]), bits(res[0]["theta"]))          # the replicas agree
            if broadcast == "workers":
                for w in r["workers"]:
                    assert torch.equal(bits(w[:n].cpu()), bits(th[:n].to(BF16)))
