"""The quantized partial exchange on the device (csrc/edt_quant.hip): edt_delta_partial_q's bytes
against the numpy restatement of the wire format (tests/quant_reference.py) applied to
the existing edt_delta_partial's fp32 partial, edt_sgd_apply_sum_q against the existing
edt_sgd_apply_sum on the dequantized arrays, and the reduce_q schedule of ShardedOuterSync on
virtual ranks against that composition — all bit for bit. The reference has no such path (its
workers exchange checkpoints on disk, EDT_LM/diloco.py:231-235)."""
import numpy as np
import pytest
import torch

from evolutionarydistributedtraining_amd import ops
from evolutionarydistributedtraining_amd._lib import EdtError
from evolutionarydistributedtraining_amd.collectives import VirtualWorld
from tests import quant_reference as Q
from tests.virtual_schedules import bits, population

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
FMTS = ["mxfp8", "mxfp4"]
PAIRS = [(torch.float32, torch.float32), (torch.float32, torch.bfloat16), (torch.bfloat16, torch.bfloat16)]
# odd tensor sizes (292,187 elements), as tests/test_gpu_virtual_ranks.py
SHAPES = [(37, 11), (5,), (1,), (256, 513), (129,), (3, 9001), (1001,), (2, 77)]


def _np(t):
    return t.detach().cpu().numpy()


def _partial(theta, workers, k_total):
    acc = torch.empty(theta.numel(), dtype=torch.float32, device=DEV)
    ops.delta_partial(theta, workers, k_total, acc)
    return _np(acc)


def _same_bits(a, b):
    return np.array_equal(np.asarray(a).view(np.int32), np.asarray(b).view(np.int32))


@pytest.mark.parametrize("tdt,wdt", PAIRS)
@pytest.mark.parametrize("fmt", FMTS)
@pytest.mark.parametrize("k_local,k_total", [(1, 8), (3, 6), (8, 8)])
def test_quantizer_matches_numpy_bit_for_bit(tdt, wdt, fmt, k_local, k_total):
    """packed == pack(Q(p)) with p from edt_delta_partial; with a residual, p' = p + r and the
    stored residual too, over two chained calls."""
    g = torch.Generator().manual_seed(11 + k_local)
    for n in (512, 2048, 37 * 512):
        theta = (torch.randn(n, generator=g) * 0.02).to(tdt).to(DEV)
        workers = [(theta.float().cpu() + torch.randn(n, generator=g) * 1e-3).to(wdt).to(DEV) for _ in range(k_local)]
        p = _partial(theta, workers, k_total)
        for region in sorted({512, n}):
            packed = torch.full((n // region * ops.q_region_bytes(region, fmt),), 0xAA, dtype=torch.uint8, device=DEV)
            ops.delta_partial_q(theta, workers, k_total, packed, region, fmt)
            assert np.array_equal(_np(packed), Q.pack(*Q.quantize(p, fmt), fmt, region)), (n, region)
            r = (torch.randn(n, generator=g) * 1e-4).numpy()
            res = torch.from_numpy(r).to(DEV)
            for call in range(2):
                packed.fill_(0x55)
                ops.delta_partial_q(theta, workers, k_total, packed, region, fmt, residual=res)
                codes, scales, _, r = Q.ef_step(p, r, fmt)
                assert np.array_equal(_np(packed), Q.pack(codes, scales, fmt, region)), (n, region, call)
                assert _same_bits(_np(res), r), (n, region, call)


def _crafted():
    """Blocks of 32, (name, values); then padded with ordinary blocks to a multiple of 512."""
    rng = np.random.default_rng(5)
    small = lambda: rng.uniform(-1, 1, 32).astype(np.float32)
    out = [("zeros", np.zeros(32, dtype=np.float32)), ("minus zeros", np.full(32, -0.0, dtype=np.float32))]
    for k in (-20, 0, 5, 100, -100):
        b = small() * np.float32(2.0 ** k) * np.float32(0.99)
        b[7] = 2.0 ** k
        out.append((f"amax 2^{k}", b))
        b = b.copy()
        b[7] = -np.nextafter(np.float32(2.0 ** (k + 1)), np.float32(0))
        b[8] = 1.99 * 2.0 ** k
        out.append((f"amax just below 2^{k + 1}", b))
    b = small() * np.float32(2.0 ** -20)
    b[3] = 1.0
    out.append(("one element 2^20 times the rest", b))
    out.append(("near 1e-30", small() * np.float32(1e-30)))
    for s in (1.0, 2.0 ** -30):
        t8 = np.array([256, 17, -17, 19, -19, 8.5, -8.5, 9.5, -9.5, 2.0 ** -10, -(2.0 ** -10), 3 * 2.0 ** -10,
                       464, -464, 240, -208, 1.0625, -1.1875], dtype=np.float64) * s
        t4 = np.array([4, 0.25, -0.25, 0.75, -0.75, 1.25, -1.25, 1.75, -1.75, 2.5, -2.5, 3.5, -3.5], dtype=np.float64) * s
        for name, t in (("E4M3 ties", t8), ("E2M1 ties", t4), ("E2M1 ties, amax 7", np.append(t4 * 1.0, [7 * s, 5 * s, -5 * s]))):
            b = np.zeros(32, dtype=np.float32)
            b[:len(t)] = t
            out.append((f"{name} x {s}", b))
    for name, v in (("NaN", np.nan), ("Inf", np.inf), ("-Inf", -np.inf)):
        b = small()
        b[13] = v
        out.append((name, b))
    out.append(("largest finite", np.where(np.arange(32) % 2, -1.0, 1.0).astype(np.float32) * np.finfo(np.float32).max))
    sub = (small() * np.float32(1e-38)).astype(np.float32)         # fp32 subnormals and tiny normals
    sub[0] = 1e-40
    out.append(("subnormal", sub))
    while len(out) % 16:
        out.append(("ordinary", small()))
    return out


@pytest.mark.parametrize("fmt", FMTS)
def test_crafted_blocks(fmt):
    """theta = 0, one fp32 worker, k_total = 1: the partial is the input (0 + -0 = +0 aside, so the
    quantizer's input is read back from edt_delta_partial). Every block but the subnormal one bit
    for bit; that one finite and within one grid step."""
    blocks = _crafted()
    x = np.concatenate([b for _, b in blocks])
    n = x.size
    theta = torch.zeros(n, dtype=torch.float32, device=DEV)
    w = [torch.from_numpy(x).to(DEV)]
    p = _partial(theta, w, 1)
    plain = np.isfinite(x) & ((np.abs(x) >= np.finfo(np.float32).tiny) | ((x == 0) & ~np.signbit(x)))
    assert _same_bits(p[plain], x[plain])
    packed = torch.empty(ops.q_region_bytes(n, fmt), dtype=torch.uint8, device=DEV)
    res = torch.zeros(n, dtype=torch.float32, device=DEV)
    ops.delta_partial_q(theta, w, 1, packed, n, fmt, residual=res)
    codes, scales = Q.unpack(_np(packed), fmt, n)
    want_c, want_s, want_d, want_r = Q.ef_step(p, np.zeros(n, dtype=np.float32), fmt)
    got_d = Q.dequantize(codes, scales, fmt)
    f = Q.FORMATS[fmt]
    for i, (name, b) in enumerate(blocks):
        sl = slice(32 * i, 32 * i + 32)
        if name == "subnormal":
            assert scales[i] == 0 and np.isfinite(got_d[sl]).all(), name
            step = 2.0 ** (f["emax"] - f["mbits"] - 127)
            assert (np.abs(got_d[sl].astype(np.float64) - b.astype(np.float64)) <= step).all(), name
            assert np.isfinite(_np(res)[sl]).all()
            continue
        assert scales[i] == want_s[i], (name, scales[i], want_s[i])
        assert np.array_equal(codes[sl], want_c[sl]), name
        if name in ("NaN", "Inf", "-Inf"):
            assert scales[i] == 255 and np.isnan(got_d[sl]).all() and np.isnan(_np(res)[sl]).all(), name
        else:
            assert np.isfinite(got_d[sl]).all(), name
            assert _same_bits(_np(res)[sl], want_r[sl]), name
    # pinned outcomes, independent of the restatement: the saturating neighbours of a power of two
    i = [name for name, _ in blocks].index("amax just below 2^1")
    d = got_d[32 * i:32 * i + 32]
    top = {"mxfp8": 448 * 2.0 ** -8, "mxfp4": 6 * 2.0 ** -2}[fmt]
    assert d[7] == -top and d[8] == top


@pytest.mark.parametrize("tdt", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("fmt", FMTS)
@pytest.mark.parametrize("nacc", [1, 2, 8])
def test_phase2_equals_sgd_apply_sum_on_dequantized_partials(tdt, fmt, nacc):
    n = 9 * 512
    rng = np.random.default_rng(nacc)
    g = torch.Generator().manual_seed(3)
    nb = Q.FORMATS[fmt]["bits"]
    regions, deq = [], []
    for r in range(nacc):
        if r % 2 == 0:                 # quantized data
            a = (rng.standard_normal(n) * 1e-3).astype(np.float32)
            a[64:96] = 0
            a[96:128] *= np.float32(2.0 ** -100)
            codes, scales = Q.quantize(a, fmt)
        else:                          # any valid code under any scale, tiny scales included
            codes = rng.integers(0, 1 << nb, n).astype(np.uint8)
            if fmt == "mxfp8":
                codes[(codes & 0x7f) == 0x7f] = 0x7e
            scales = rng.integers(100, 128, n // 32).astype(np.uint8)
            scales[:6] = [0, 1, 40, 62, 63, 64]
        regions.append(torch.from_numpy(Q.pack(codes, scales, fmt, n)).to(DEV))
        deq.append(torch.from_numpy(Q.dequantize(codes, scales, fmt)).to(DEV))
    theta0 = (torch.randn(n, generator=g) * 0.02).to(tdt).to(DEV)
    mom0 = (torch.randn(n, generator=g) * 1e-3).to(tdt).to(DEV)
    for nesterov in (True, False):
        for has in (True, False):
            th_q, mom_q, th_f, mom_f = theta0.clone(), mom0.clone(), theta0.clone(), mom0.clone()
            ops.sgd_apply_sum_q(th_q, regions, fmt, mom_q, has, 0.7, 0.9, nesterov)
            ops.sgd_apply_sum(th_f, deq, mom_f, has, 0.7, 0.9, nesterov)
            torch.cuda.synchronize()
            assert torch.equal(bits(th_q), bits(th_f)), (nesterov, has)
            assert torch.equal(bits(mom_q), bits(mom_f)), (nesterov, has)
            assert not torch.equal(bits(th_q), bits(theta0))
    th_q, th_f = theta0.clone(), theta0.clone()                    # no momentum at all
    ops.sgd_apply_sum_q(th_q, regions, fmt, None, False, 0.7, 0.0, False)
    ops.sgd_apply_sum(th_f, deq, None, False, 0.7, 0.0, False)
    assert torch.equal(bits(th_q), bits(th_f))


def _composition(theta0, gens, world, n_pad, fmt, ef, lr=0.7, mu=0.9, nesterov=True):
    """ops.delta_partial per rank -> numpy Q / D with the rank's residual -> ops.sgd_apply_sum, over
    the whole padded arena (no buckets, regions or packing)."""
    n = theta0.numel()
    th = torch.zeros(n_pad, dtype=theta0.dtype, device=DEV)
    th[:n] = theta0
    mom = torch.zeros_like(th)
    res = [np.zeros(n_pad, dtype=np.float32) if ef else None for _ in range(world)]
    for i, ws in enumerate(gens):
        K = len(ws)
        kl = K // world
        ds = []
        for r in range(world):
            pads = []
            for w in ws[r * kl:(r + 1) * kl]:
                pw = torch.zeros(n_pad, dtype=w.dtype, device=DEV)
                pw[:n] = w
                pads.append(pw)
            _, _, d, res[r] = Q.ef_step(_partial(th, pads, K), res[r], fmt)
            ds.append(torch.from_numpy(d).to(DEV))
        ops.sgd_apply_sum(th, ds, mom, i > 0, lr, mu, nesterov)
    torch.cuda.synchronize()
    return th, mom, res


@pytest.mark.parametrize("world,units", [(2, 37), (4, 37), (8, 17)])
@pytest.mark.parametrize("fmt", FMTS)
@pytest.mark.parametrize("ef", [True, False])
@pytest.mark.parametrize("tdt,wdt", PAIRS)
def test_reduce_q_schedule_on_virtual_ranks(world, units, fmt, ef, tdt, wdt):
    from evolutionarydistributedtraining_amd.distributed import ShardedOuterSync
    layout, theta, gens = population(SHAPES, tdt, wdt, 8, steps=3, device=DEV)
    k_local = 8 // world

    def body(comm):
        s = ShardedOuterSync(layout, tdt, wdt, k_local, DEV, mode="reduce_q", wire_format=fmt, error_feedback=ef,
                             bucket_elems=world * 512 * units, comm=comm)
        s.theta.flat.copy_(theta)
        for ws in gens:
            for j, a in enumerate(s.workers):
                a.flat.copy_(ws[comm.rank * k_local + j])
            s.step()
        return {"theta": s.theta_buf.clone(), "mom": comm.all_gather_object(s.mom_shard.clone()),
                "residual": None if s.residual is None else s.residual.clone(), "buckets": s.buckets,
                "n_pad": s.n_pad, "wire": s.wire_bytes()}

    res = VirtualWorld(world).run(body)
    torch.cuda.synchronize()
    n_pad, buckets = res[0]["n_pad"], res[0]["buckets"]
    sizes = {e - b for b, e in buckets}
    assert len(buckets) >= 3 and n_pad > layout.total and len(sizes) == 2            # ragged last bucket
    for r in res:
        assert torch.equal(bits(r["theta"]), bits(res[0]["theta"]))
    th, mom_ref, resid = _composition(theta, gens, world, n_pad, fmt, ef)
    assert torch.equal(bits(res[0]["theta"]), bits(th))
    mom = torch.empty(n_pad, dtype=tdt, device=DEV)
    off = [0] * world
    for b, e in buckets:
        per = (e - b) // world
        for r in range(world):
            mom[b + r * per:b + (r + 1) * per] = res[0]["mom"][r][off[r]:off[r] + per]
            off[r] += per
    assert torch.equal(bits(mom), bits(mom_ref))
    for r in range(world):
        if ef:
            assert _same_bits(_np(res[r]["residual"]), resid[r]), r
        else:
            assert res[r]["residual"] is None
    q = {"mxfp8": 1 + 1 / 32, "mxfp4": 1 / 2 + 1 / 32}[fmt]
    assert res[0]["wire"] == int((world - 1) / world * n_pad * (q + theta.element_size()))


@pytest.mark.parametrize("fmt", FMTS)
def test_error_feedback_identity_on_the_device(fmt):
    """Per element sum_t D(q_t) + r_T = sum_t p_t within T * 2 * 2^-24 * max|p'|: two fp32
    roundings per step (p' = p + r, r = p' - D(q))."""
    n, T, K = 8 * 512, 4, 4
    g = torch.Generator().manual_seed(17)
    theta = (torch.randn(n, generator=g) * 0.02).to(DEV)
    res = torch.zeros(n, dtype=torch.float32, device=DEV)
    packed = torch.empty(ops.q_region_bytes(n, fmt), dtype=torch.uint8, device=DEV)
    sent, true, peak = np.zeros(n), np.zeros(n), 0.0
    for t in range(T):
        workers = [(theta.cpu() + torch.randn(n, generator=g) * 1e-3 * (t + 1)).bfloat16().to(DEV) for _ in range(K)]
        p = _partial(theta, workers, K)
        peak = max(peak, float(np.abs(p + _np(res)).max()))
        ops.delta_partial_q(theta, workers, K, packed, n, fmt, residual=res)
        sent += Q.dequantize(*Q.unpack(_np(packed), fmt, n), fmt)
        true += p
    r = _np(res).astype(np.float64)
    assert np.abs(r).max() > 0
    assert np.abs(sent + r - true).max() <= T * 2 * 2.0 ** -24 * peak


def test_wrappers_validate_their_arguments():
    n = 1024
    theta = torch.zeros(n, device=DEV)
    ws = [torch.zeros(n, dtype=torch.bfloat16, device=DEV)]
    good = torch.zeros(ops.q_region_bytes(n, "mxfp8"), dtype=torch.uint8, device=DEV)
    ops.delta_partial_q(theta, ws, 1, good, n, "mxfp8")
    bad_calls = [
        lambda: ops.delta_partial_q(theta, ws, 1, good.to(torch.int8), n, "mxfp8"),                 # dtype
        lambda: ops.delta_partial_q(theta, ws, 1, good[:-16], n, "mxfp8"),                           # size
        lambda: ops.delta_partial_q(theta, ws, 1, good, n, "mxfp4"),                                 # size for fmt
        lambda: ops.delta_partial_q(theta, ws, 1, good, 500, "mxfp8"),                               # region
        lambda: ops.delta_partial_q(theta, ws, 1, good, 1536, "mxfp8"),                              # n % region
        lambda: ops.delta_partial_q(theta, ws, 1, good, n, "int8"),                                  # fmt
        lambda: ops.delta_partial_q(theta, ws, 1, good.cpu(), n, "mxfp8"),                           # device
        lambda: ops.delta_partial_q(theta, ws, 1, good, n, "mxfp8", residual=torch.zeros(n, dtype=torch.float16, device=DEV)),
        lambda: ops.delta_partial_q(theta, ws, 1, good, n, "mxfp8", residual=torch.zeros(n - 1, device=DEV)),
        lambda: ops.delta_partial_q(theta, [ws[0][:512]], 1, good, n, "mxfp8"),                      # worker size
        lambda: ops.delta_partial_q(theta.double(), ws, 1, good, n, "mxfp8"),                        # theta dtype
        lambda: ops.sgd_apply_sum_q(theta, [good.to(torch.int8)], "mxfp8", None, False, 0.7, 0.0, False),
        lambda: ops.sgd_apply_sum_q(theta, [good[:-16]], "mxfp8", None, False, 0.7, 0.0, False),
        lambda: ops.sgd_apply_sum_q(theta, [], "mxfp8", None, False, 0.7, 0.0, False),
        lambda: ops.sgd_apply_sum_q(theta, [good.cpu()], "mxfp8", None, False, 0.7, 0.0, False),
        lambda: ops.sgd_apply_sum_q(theta, [good], "fp8", None, False, 0.7, 0.0, False),
        lambda: ops.sgd_apply_sum_q(theta[:1000], [good], "mxfp8", None, False, 0.7, 0.0, False),
        lambda: ops.sgd_apply_sum_q(theta, [good], "mxfp8", torch.zeros(n, dtype=torch.bfloat16, device=DEV), True, 0.7,
                                    0.9, True),
        lambda: ops.q_region_bytes(500, "mxfp8"),
    ]
    for i, call in enumerate(bad_calls):
        with pytest.raises(EdtError):
            call()
            pytest.fail(f"call {i} was accepted")
    assert ops.q_region_bytes(512, "mxfp8") == 528 and ops.q_region_bytes(512, "mxfp4") == 272
