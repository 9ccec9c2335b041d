"""Stochastic rounding of the quantized exchange on the device (csrc/edt_quant.hip, the *_sr
entries): the packed bytes of edt_delta_partial_q_sr and edt_sgd_delta_sum_q_sr against the numpy
definition (tests/sr_reference.py: Philox4x32-10, the bumped scale, the (lo, f16, up) rule) bit for
bit, the counter discipline (global element index, seed, step, stream), unbiasedness with a
nearest-mode control, and ShardedOuterSync(rounding="stochastic") on virtual ranks against the
composition. The reference project quantizes nothing (EDT_LM/diloco.py:231-235, 302-308: checkpoints
over a shared disk)."""
import numpy as np
import pytest
import torch

from evolutionarydistributedtraining_amd import ops
from evolutionarydistributedtraining_amd._lib import EdtError
from tests import quant_reference as Q
from tests import sr_reference as S
from tests.virtual_schedules import bits, population

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
FMTS = ["mxfp8", "mxfp4"]
PAIRS = [(torch.float32, torch.float32), (torch.float32, torch.bfloat16), (torch.bfloat16, torch.bfloat16)]
MAXV = {"mxfp8": 448.0, "mxfp4": 6.0}
SEED = 0x0123456789abcdef
# (n, region_elems): one wave; two regions (the scale gather crosses a region); a wave count that is
# no multiple of the 4 waves of a workgroup
SHAPES_1 = [(512, 512), (1024, 512), (512 * 37, 512 * 37)]


def _np(t):
    return t.detach().cpu().numpy()


def _partial(theta, workers, k_total):
    acc = torch.empty(theta.numel(), dtype=torch.float32, device=DEV)
    ops.delta_partial(theta, workers, k_total, acc)
    return _np(acc)


def _packed(n, region, fmt):
    return torch.full((n // region * ops.q_region_bytes(region, fmt),), 0xAA, dtype=torch.uint8, device=DEV)


def _sr_bytes(p, fmt, region, seed=SEED, step=0, stream_id=0, elem_base=0):
    return Q.pack(*S.sr_quantize(p, fmt, seed, step, stream_id, elem_base), fmt, region)


@pytest.mark.parametrize("k_local,k_total", [(1, 1), (3, 3), (8, 8), (3, 24)])
@pytest.mark.parametrize("tdt,wdt", PAIRS)
@pytest.mark.parametrize("fmt", FMTS)
def test_phase1_bytes_equal_the_definition(fmt, tdt, wdt, k_local, k_total):
    """Random workers around theta (K_total 3 and 24: the exact-division path, 1 and 8: the
    reciprocal one, K_local = 8: the unrolled kernel) with a block where every worker equals theta
    (an all-zero partial) and one where a worker holds a NaN; the partial itself is
    edt_delta_partial's (bit-identical by the existing contract), the bytes are the definition's."""
    g = torch.Generator().manual_seed(11 * k_local + k_total)
    for n, region in SHAPES_1:
        theta = (torch.randn(n, generator=g) * 0.02).to(tdt)
        ws = [(theta.float() + torch.randn(n, generator=g) * torch.exp2(torch.randint(-14, -6, (n,), generator=g).float()))
              .to(wdt) for _ in range(k_local)]
        same = theta[64:96].bfloat16()               # exact in every dtype here: block 2's partial is zero
        theta[64:96] = same.to(tdt)
        for w in ws:
            w[64:96] = same.to(wdt)
        ws[-1][130] = float("nan")
        theta, ws = theta.to(DEV), [w.to(DEV) for w in ws]
        p = _partial(theta, ws, k_total)
        assert not p[64:96].any() and np.isnan(p[130]) and np.isfinite(p).sum() == n - 1
        for step, stream in ((0, 0), (3, 5)):
            packed = _packed(n, region, fmt)
            ops.delta_partial_q(theta, ws, k_total, packed, region, fmt, rounding="stochastic", seed=SEED, step=step,
                                stream_id=stream)
            want = _sr_bytes(p, fmt, region, step=step, stream_id=stream)
            assert np.array_equal(_np(packed), want), (n, region, step)
            codes, scales = Q.unpack(_np(packed), fmt, region)
            assert scales[2] == 0 and scales[4] == 255 and not codes[128:160].any()


def _special_blocks(fmt):
    """fp32 values placed by hand, 32 per block (theta = 0, one fp32 worker, K = 1: the partial is
    the worker itself). Returns (x padded to 1024, {name: block index})."""
    m, rng = MAXV[fmt], np.random.default_rng(5)
    top = 2 * 2.0 ** Q.FORMATS[fmt]["emax"]
    blocks, names = [], {}

    def add(name, blk):
        names[name] = len(blocks)
        blocks.append(np.asarray(blk, dtype=np.float32))

    def with_max(amax, s):
        b = rng.uniform(-0.97, 0.97, 32) * amax
        b[rng.integers(0, 32)] = -amax if s & 1 else amax
        return (b * 2.0 ** s).astype(np.float32)

    add("zero", np.zeros(32))
    add("negzero", np.full(32, -0.0))
    nan = rng.standard_normal(32)
    nan[7] = np.nan
    add("nan", nan)
    inf = rng.standard_normal(32)
    inf[31] = np.inf
    add("inf", inf)
    for i, (amax, s) in enumerate([(m * 1.001, 0), ((m + top) / 2, -9), (np.nextafter(np.float32(top), np.float32(0)), 5),
                                   (np.nextafter(np.float32(m), np.float32(np.inf)), -30)]):
        add(f"bump{i}", with_max(float(amax), s))
    for i, s in enumerate((0, -17, 20)):
        add(f"exact{i}", with_max(m, s))
    # the scale byte clamps to 0: normal fp32 values just above 2^-126
    add("clamp0", rng.uniform(1.0, 1.5, 32) * 2.0 ** -126 * np.where(rng.integers(0, 2, 32), 1, -1))
    # every value but the maximum lies below the smallest element subnormal (2^-9 / 2^-1 of the scale)
    tiny = rng.uniform(0.01, 0.99, 32) * 2.0 ** (-10 - Q.FORMATS[fmt]["emax"]) * np.where(rng.integers(0, 2, 32), 1, -1)
    tiny[11] = 1.0
    add("tiny", tiny)
    x = np.concatenate(blocks + [rng.standard_normal(1024 - 32 * len(blocks)).astype(np.float32) * 1e-3])
    return x.astype(np.float32), names


@pytest.mark.parametrize("fmt", FMTS)
def test_phase1_special_blocks(fmt):
    x, names = _special_blocks(fmt)
    n = x.size
    theta = torch.zeros(n, device=DEV)
    w = torch.from_numpy(x).to(DEV)
    p = _partial(theta, [w], 1)
    keep = np.isfinite(x)
    assert np.array_equal(p[keep].view(np.int32), (x[keep] + np.float32(0)).view(np.int32))     # -0 + 0 = +0: the partial's zero
    for region in (512, 1024):
        packed = _packed(n, region, fmt)
        ops.delta_partial_q(theta, [w], 1, packed, region, fmt, rounding="stochastic", seed=SEED, step=2, stream_id=1)
        assert np.array_equal(_np(packed), _sr_bytes(p, fmt, region, step=2, stream_id=1)), region
        codes, scales = Q.unpack(_np(packed), fmt, region)
        near = Q.quantize(p, fmt)[1]
        sb = lambda name: int(scales[names[name]])
        assert sb("zero") == 0 and sb("negzero") == 0 and sb("nan") == 255 and sb("inf") == 255 and sb("clamp0") == 0
        for name, b in names.items():
            if name.startswith("bump"):
                assert sb(name) == int(near[b]) + 1, name
            elif name.startswith("exact"):
                assert sb(name) == int(near[b]), name
        d = Q.dequantize(codes, scales, fmt)
        fin = ~np.isnan(d)
        assert (np.abs(d[fin] - p[fin]) < S.grid_step(p, fmt)[fin]).all()
        assert np.isnan(d).sum() == 64
        # nothing saturated: every block maximum is met or passed only by rounding, never clamped below
        for name, b in names.items():
            if name.startswith(("bump", "exact")):
                blk, dq = np.abs(p[32 * b:32 * b + 32]), np.abs(d[32 * b:32 * b + 32])
                assert dq.max() >= blk.max() - S.grid_step(p, fmt)[32 * b + int(blk.argmax())], name
                if name.startswith("exact"):
                    assert dq[int(blk.argmax())] == blk.max(), name


FMT_PAIRS = [(a, b) for a in FMTS for b in FMTS]


def _regions(rng, n, nacc, fmt):
    out = []
    for _ in range(nacc):
        a = (rng.standard_normal(n) * 1e-3).astype(np.float32)
        out.append(torch.from_numpy(Q.pack(*Q.quantize(a, fmt), fmt, n)).to(DEV))
    return out


@pytest.mark.parametrize("tdt", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("nacc", [1, 2, 8])
@pytest.mark.parametrize("fmt_in,fmt_out", FMT_PAIRS)
def test_phase2_momentum_theta_and_bytes(tdt, nacc, fmt_in, fmt_out):
    """The momentum equals edt_sgd_apply_sum_q's on a clone, theta is not written, and packed_out is
    the definition applied to u = f32(theta') - f32(theta) (theta' the clone's), at the shard's
    elem_base, over two chained calls per momentum setting."""
    rng = np.random.default_rng(100 * nacc + len(fmt_in))
    g = torch.Generator().manual_seed(7 + nacc)
    for n, base in ((512, 0), (37 * 512, 8 * 1000003)):
        regions = _regions(rng, n, nacc, fmt_in)
        theta = (torch.randn(n, generator=g) * 0.02).to(tdt).to(DEV)
        theta0 = theta.clone()
        mom0 = (torch.randn(n, generator=g) * 1e-3).to(tdt).to(DEV)
        for nesterov, has, mu in [(True, True, 0.9), (True, False, 0.9), (False, True, 0.9), (False, False, 0.9),
                                  (False, False, 0.0)]:
            mom = mom0.clone() if mu else None
            packed = torch.empty(ops.q_region_bytes(n, fmt_out), dtype=torch.uint8, device=DEV)
            for call in range(2):
                th_ref = theta.clone()
                mom_ref = None if mom is None else mom.clone()
                carried = bool(mu) and (has or call > 0)
                ops.sgd_apply_sum_q(th_ref, regions, fmt_in, mom_ref, carried, 0.7, mu, nesterov)
                packed.fill_(0xAA)
                ops.sgd_delta_sum_q(theta, regions, fmt_in, mom, carried, 0.7, mu, nesterov, packed, fmt_out,
                                    rounding="stochastic", seed=SEED, step=call, stream_id=3, elem_base=base)
                tag = (n, nesterov, has, mu, call)
                assert torch.equal(bits(theta), bits(theta0)), tag
                assert not torch.equal(bits(th_ref), bits(theta0)), tag
                if mom is not None:
                    assert torch.equal(bits(mom), bits(mom_ref)), tag
                u = (_np(th_ref.float()) - _np(theta.float())).astype(np.float32)
                want = _sr_bytes(u, fmt_out, n, step=call, stream_id=3, elem_base=base)
                assert np.array_equal(_np(packed), want), tag


def _one_worker(x):
    return torch.zeros(x.size, device=DEV), [torch.from_numpy(x).to(DEV)]


def _q(x, fmt, region=None, **kw):
    theta, ws = _one_worker(x)
    region = region or x.size
    packed = _packed(x.size, region, fmt)
    ops.delta_partial_q(theta, ws, 1, packed, region, fmt, **kw)
    return _np(packed)


@pytest.mark.parametrize("fmt", FMTS)
def test_counter_discipline(fmt):
    rng = np.random.default_rng(9)
    x = (rng.standard_normal(4096) * np.exp2(rng.integers(-10, 2, 4096))).astype(np.float32)
    kw = dict(rounding="stochastic", seed=SEED, step=4, stream_id=6)
    whole = _q(x, fmt, region=2048, **kw)
    halves = np.concatenate([_q(x[:2048], fmt, **kw, elem_base=0), _q(x[2048:], fmt, **kw, elem_base=2048)])
    assert np.array_equal(whole, halves)
    assert not np.array_equal(_q(x[2048:], fmt, **kw, elem_base=0), _q(x[2048:], fmt, **kw, elem_base=2048))
    assert np.array_equal(whole, _q(x, fmt, region=2048, **kw))                 # the same triple: the same bytes
    assert np.array_equal(whole, _sr_bytes(x, fmt, 2048, step=4, stream_id=6))
    codes0, scales0 = Q.unpack(whole, fmt, 2048)
    for change in ({"seed": SEED + 1}, {"seed": SEED ^ (1 << 40)}, {"step": 5}, {"stream_id": 7}):
        other = _q(x, fmt, region=2048, **{**kw, **change})
        codes, scales = Q.unpack(other, fmt, 2048)
        assert np.array_equal(scales, scales0) and not np.array_equal(codes, codes0), change
        assert np.array_equal(other, _sr_bytes(x, fmt, 2048, **{"seed": SEED, "step": 4, "stream_id": 6, **change}))
    # an element index past 2^32 groups reaches the counter's second word
    far = 8 * ((1 << 32) + 5)
    assert np.array_equal(_q(x[:512], fmt, **kw, elem_base=far), _sr_bytes(x[:512], fmt, 512, step=4, stream_id=6, elem_base=far))


@pytest.mark.parametrize("fmt", FMTS)
@pytest.mark.parametrize("tdt,wdt", PAIRS)
def test_nearest_mode_is_untouched(fmt, tdt, wdt):
    g = torch.Generator().manual_seed(3)
    n = 512 * 5
    theta = (torch.randn(n, generator=g) * 0.02).to(tdt).to(DEV)
    ws = [(theta.float().cpu() + torch.randn(n, generator=g) * 1e-3).to(wdt).to(DEV) for _ in range(3)]
    a, b, c = _packed(n, 512, fmt), _packed(n, 512, fmt), _packed(n, 512, fmt)
    ops.delta_partial_q(theta, ws, 3, a, 512, fmt)
    ops.delta_partial_q(theta, ws, 3, b, 512, fmt, rounding="nearest")
    ops.delta_partial_q(theta, ws, 3, c, 512, fmt, rounding="nearest", seed=9, step=9, stream_id=9)   # ignored
    assert torch.equal(a, b) and torch.equal(a, c)
    assert np.array_equal(_np(a), Q.pack(*Q.quantize(_partial(theta, ws, 3), fmt), fmt, 512))
    res = torch.zeros(n, device=DEV)
    d, e = _packed(n, 512, fmt), _packed(n, 512, fmt)
    ops.delta_partial_q(theta, ws, 3, d, 512, fmt, res)
    res2 = torch.zeros(n, device=DEV)
    ops.delta_partial_q(theta, ws, 3, e, 512, fmt, res2, rounding="nearest")
    assert torch.equal(d, e) and torch.equal(bits(res), bits(res2)) and torch.equal(d, a)


@pytest.mark.parametrize("fmt", FMTS)
def test_unbiased_where_nearest_is_not(fmt):
    """x = N(0,1) * 2^U{-12..3} (fixed), one worker, theta = 0, K = 1: the partial is x. Over steps
    0..255 of one seed the mean of D(Q_sr(x)) lies within 0.2 grid steps (q 2^e at the element) of x
    for every element: each error lies inside one grid step, so by Hoeffding the chance that any of
    4096 elements leaves +-0.2 steps is <= 4096 * 2 exp(-2 * 256 * 0.2^2) ~ 1e-5 (the numpy
    definition gives 0.123 / 0.086 on these inputs: tests/test_sr_cpu.py). Control: nearest
    rounding, whose mean is its single error, misses the same bound for at least a quarter of the
    elements, so the test can see a biased quantizer."""
    x = S.unbiased_inputs()
    n = x.size
    theta, ws = _one_worker(x)
    packed = _packed(n, n, fmt)
    step_sr = S.grid_step(x, fmt)
    acc = np.zeros(n)
    for step in range(256):
        ops.delta_partial_q(theta, ws, 1, packed, n, fmt, rounding="stochastic", seed=S.UNBIASED_SEED, step=step)
        d = Q.dequantize(*Q.unpack(_np(packed), fmt, n), fmt)
        assert (np.abs(d - x) < step_sr).all(), step                          # one of the two neighbours
        acc += d
    worst = (np.abs(acc / 256 - x) / step_sr).max()
    print("stochastic: max |mean - x| / grid step", fmt, worst)
    assert worst <= 0.2
    ops.delta_partial_q(theta, ws, 1, packed, n, fmt, rounding="nearest")
    codes, scales = Q.unpack(_np(packed), fmt, n)
    miss = np.abs(Q.dequantize(codes, scales, fmt) - x) / S.grid_step(x, fmt, scales) > 0.2
    print("nearest: fraction of elements outside 0.2 grid steps", fmt, miss.mean())
    assert miss.mean() >= 0.25


LAYOUT = [(37, 11), (5,), (1,), (64, 33), (129,), (300,), (7, 401)]           # 5,761 elements


def _device_fns():
    def sgd_sum(new, ds, mom, has, lr, mu, nesterov):
        ops.sgd_apply_sum(new, ds, mom, has, lr, mu, nesterov)

    return _partial, sgd_sum


@pytest.mark.parametrize("world,units", [(2, 2), (4, 1), (8, 1)])
@pytest.mark.parametrize("fmt_in,fmt_out", [("mxfp8", None), ("mxfp4", "mxfp8"), ("mxfp8", "mxfp4")])
@pytest.mark.parametrize("tdt,wdt", [(torch.float32, torch.bfloat16), (torch.bfloat16, torch.bfloat16)])
def test_stochastic_schedule_on_virtual_ranks(world, units, fmt_in, fmt_out, tdt, wdt):
    layout, theta, gens = population(LAYOUT, tdt, wdt, 8, steps=3, device=DEV)
    bucket = world * 512 * units
    res = S.run_schedule(world, layout, tdt, wdt, theta, gens, None, fmt_in, fmt_out, SEED, bucket)
    torch.cuda.synchronize()
    n_pad, buckets = res[0]["n_pad"], res[0]["buckets"]
    assert len(buckets) >= 2 and n_pad > layout.total and res[0]["q_step"] == 3 and not res[0]["has_residual"]
    for r in res:
        for a, b in zip(r["steps"], res[0]["steps"]):
            assert torch.equal(bits(a["theta"]), bits(b["theta"]))
    th, mom = S.compose(*_device_fns(), theta, gens, world, n_pad, buckets, fmt_in, fmt_out, SEED)
    torch.cuda.synchronize()
    assert torch.equal(bits(res[0]["steps"][-1]["theta"]), bits(th))
    assert not torch.equal(bits(th[:layout.total]), bits(theta))
    own = S.owners(buckets, world, n_pad)
    for r in range(world):
        idx = torch.from_numpy(np.flatnonzero(own == r)).to(DEV)
        assert torch.equal(bits(res[r]["steps"][-1]["mom"]), bits(mom[idx])), r
    # a second sync that restores theta, the momentum and q_step = 1 replays steps 1-2 bit for bit
    state = [r["steps"][0] for r in res]
    again = S.run_schedule(world, layout, tdt, wdt, theta, gens[1:], None, fmt_in, fmt_out, SEED, bucket, first_step=1,
                           state=state)
    torch.cuda.synchronize()
    for r in range(world):
        assert again[r]["q_step"] == 3
        for a, b in zip(again[r]["steps"], res[r]["steps"][1:]):
            assert torch.equal(bits(a["theta"]), bits(b["theta"])) and torch.equal(bits(a["mom"]), bits(b["mom"]))


def test_bad_arguments_raise_and_start_no_kernel():
    n = 1024
    theta = torch.zeros(n, device=DEV)
    ws = [torch.ones(n, device=DEV)]
    mom = torch.zeros(n, device=DEV)
    res = torch.zeros(n, device=DEV)
    out8 = torch.full((ops.q_region_bytes(n, "mxfp8"),), 0xAA, dtype=torch.uint8, device=DEV)
    reg8 = torch.zeros(ops.q_region_bytes(n, "mxfp8"), dtype=torch.uint8, device=DEV)
    sr = dict(rounding="stochastic", seed=1, step=2, stream_id=3)

    def part(**kw):
        ops.delta_partial_q(theta, ws, 1, out8, n, "mxfp8", **{**sr, **kw})

    def delta(**kw):
        ops.sgd_delta_sum_q(theta, [reg8], "mxfp8", mom, True, 0.7, 0.9, True, out8, "mxfp8", **{**sr, **kw})

    bad_calls = [
        lambda: part(residual=res),                      # stochastic rounding takes no residual
        lambda: delta(residual=res),
        lambda: part(rounding="up"),
        lambda: delta(rounding="truncate"),
        lambda: part(elem_base=4),
        lambda: part(elem_base=-8),
        lambda: delta(elem_base=12),
        lambda: part(seed=-1),
        lambda: part(seed=1 << 64),
        lambda: delta(step=-1),
        lambda: part(stream_id=1 << 32),
        lambda: ops.delta_partial_q(theta, ws, 1, out8, n, "int8", **sr),
        lambda: ops.delta_partial_q(theta, ws, 1, out8, 500, "mxfp8", **sr),
        lambda: ops.delta_partial_q(theta, ws, 1, out8[:-16], n, "mxfp8", **sr),
        lambda: ops.delta_partial_q(theta, ws, 1, out8.cpu(), n, "mxfp8", **sr),
        lambda: ops.sgd_delta_sum_q(theta, [reg8], "mxfp8", mom, True, 0.7, 0.9, True, out8, "fp4", **sr),
        lambda: ops.sgd_delta_sum_q(theta[:1000], [reg8], "mxfp8", mom, True, 0.7, 0.9, True, out8, "mxfp8", **sr),
    ]
    for i, call in enumerate(bad_calls):
        with pytest.raises(EdtError):
            call()
            pytest.fail(f"call {i} was accepted")
    torch.cuda.synchronize()
    assert (out8 == 0xAA).all() and not mom.any()                     # no kernel ran
    part()
    delta()
    torch.cuda.synchronize()
    assert not (out8 == 0xAA).all()
