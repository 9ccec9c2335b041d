"""The quantized partial exchange without a GPU: the numpy restatement of the wire format
(tests/quant_reference.py) pinned by hand-written vectors, the host-side validation of
the three C-ABI entries, and the reduce_q schedule of ShardedOuterSync on virtual ranks with a
numpy stand-in for the kernels (the kernels= seam). The reference has no wire format (its workers
exchange checkpoints on disk, EDT_LM/diloco.py:231-235); the GPU form is tests/test_gpu_quant.py."""
import ctypes

import numpy as np
import pytest
import torch

from tests import quant_reference as Q
from tests.virtual_schedules import bits, population

FMTS = ["mxfp8", "mxfp4"]
EMAX = {"mxfp8": 8, "mxfp4": 2}
MAXV = {"mxfp8": 448.0, "mxfp4": 6.0}


def _block(vals, fill=0.0):
    b = np.full(32, fill, dtype=np.float32)
    b[:len(vals)] = vals
    return b


@pytest.mark.parametrize("fmt", FMTS)
def test_every_code_round_trips(fmt):
    """Every finite element code (both signs; E4M3's 0x7f / 0xff are NaN and never produced) at
    scale 2^0 and at a scale far from it quantizes back to itself."""
    nb = Q.FORMATS[fmt]["bits"]
    codes = np.array([c for c in range(1 << nb) if np.isfinite(Q.magnitude_table(fmt)[c & ((1 << (nb - 1)) - 1)])],
                     dtype=np.uint8)
    top = (1 << (nb - 1)) - (2 if fmt == "mxfp8" else 1)           # the largest finite magnitude code
    assert Q.magnitude_table(fmt)[top] == MAXV[fmt]
    for sb in (127, 127 - 40, 127 + 60):
        for lo in range(0, len(codes), 31):
            blk = np.full(32, top, dtype=np.uint8)                 # amax pinned: the block's scale is sb
            part = codes[lo:lo + 31]
            blk[1:1 + len(part)] = part
            v = Q.dequantize(blk, np.array([sb], dtype=np.uint8), fmt)
            c2, s2 = Q.quantize(v, fmt)
            assert s2[0] == sb
            assert np.array_equal(c2, blk)
    if fmt == "mxfp8":
        assert np.isnan(Q.dequantize(np.full(32, 0x7f, dtype=np.uint8), np.array([127], dtype=np.uint8), fmt)).all()
        assert list(Q.finite_grid(fmt)[[1, 7, 8, 126]]) == [2.0 ** -9, 7 * 2.0 ** -9, 2.0 ** -6, 448.0]
    else:
        assert list(Q.finite_grid(fmt)) == [0, 0.5, 1, 1.5, 2, 3, 4, 6]


@pytest.mark.parametrize("fmt", FMTS)
@pytest.mark.parametrize("k", [-20, 0, 13])
def test_saturation(fmt, k):
    """amax = 1.99 * 2^k: e = k - emax, the scaled value 1.99 * 2^emax (509.4 / 7.96) is past the
    largest element and saturates to it."""
    blk = _block([1.99 * 2.0 ** k, -1.99 * 2.0 ** k, 2.0 ** k])
    codes, sb = Q.quantize(blk, fmt)
    assert sb[0] == k - EMAX[fmt] + 127
    d = Q.dequantize(codes, sb, fmt)
    assert d[0] == MAXV[fmt] * 2.0 ** (k - EMAX[fmt]) and d[1] == -d[0] and d[2] == np.float32(2.0 ** k)
    assert np.isfinite(d).all()


def test_ties_to_even_and_signs():
    # E4M3 at scale 2^0 (amax 256 = 2^8): grid step 2 in [16, 32), 1 in [8, 16), 2^-9 below 2^-6
    blk = _block([256, 17, 19, -17, -19, 8.5, 9.5, 2.0 ** -10, 3 * 2.0 ** -10, -(2.0 ** -10)])
    codes, sb = Q.quantize(blk, "mxfp8")
    d = Q.dequantize(codes, sb, "mxfp8")
    assert sb[0] == 127
    assert list(d[:10]) == [256, 16, 20, -16, -20, 8, 10, 0, 2.0 ** -8, 0]
    assert np.signbit(d[9]) and codes[9] == 0x80                   # rounds to zero, sign kept
    # E2M1 at scale 2^0 (amax 4): ties 0.25 -> 0, 0.75 -> 1, 1.25 -> 1, 1.75 -> 2, 2.5 -> 2, 3.5 -> 4, 5 -> 4
    blk = _block([4, 0.25, 0.75, 1.25, 1.75, 2.5, 3.5, -2.5, -3.5, -0.25])
    codes, sb = Q.quantize(blk, "mxfp4")
    d = Q.dequantize(codes, sb, "mxfp4")
    assert sb[0] == 127
    assert list(d[:10]) == [4, 0, 1, 1, 2, 2, 4, -2, -4, 0] and np.signbit(d[9]) and codes[9] == 0x8
    codes, sb = Q.quantize(_block([7.9, 5.0, -5.0]), "mxfp4")     # amax in [4, 8): e = 0; 5 ties to 4 (even code)
    assert list(Q.dequantize(codes, sb, "mxfp4")[:3]) == [6, 4, -4]


@pytest.mark.parametrize("fmt", FMTS)
def test_zero_blocks_and_scale_clamps(fmt):
    nb = Q.FORMATS[fmt]["bits"]
    codes, sb = Q.quantize(np.zeros(32, dtype=np.float32), fmt)
    assert sb[0] == 0 and not codes.any()
    neg = _block([-0.0] * 5)
    codes, sb = Q.quantize(neg, fmt)
    assert sb[0] == 0 and list(codes[:6]) == [1 << (nb - 1)] * 5 + [0]          # -0 keeps its sign
    d = Q.dequantize(codes, sb, fmt)
    assert not d.any() and np.signbit(d[:5]).all() and not np.signbit(d[5:]).any()
    # the low clamp: amax = 2^-125 gives e = -125 - emax < -127, stored as byte 0 (e = -127)
    blk = _block([2.0 ** -125, -(2.0 ** -126)])
    codes, sb = Q.quantize(blk, fmt)
    assert sb[0] == 0
    d = Q.dequantize(codes, sb, fmt)
    assert d[0] == np.float32(2.0 ** -125) and d[1] == np.float32(-(2.0 ** -126))     # 4 and 2 on both grids
    # the high clamp is 254; an fp32 amax reaches at most 127 - emax + 127
    assert list(Q.scale_byte([-200, -128, -127, 0, 127, 128, 300])) == [0, 0, 0, 127, 254, 254, 254]
    big = np.float32(np.finfo(np.float32).max)
    codes, sb = Q.quantize(_block([big]), fmt)
    assert sb[0] == 254 - EMAX[fmt]
    assert np.isfinite(Q.dequantize(codes, sb, fmt)).all()


@pytest.mark.parametrize("fmt", FMTS)
@pytest.mark.parametrize("poison", [np.nan, np.inf, -np.inf])
def test_non_finite_block_is_never_hidden(fmt, poison):
    p = np.linspace(-1, 1, 64).astype(np.float32)
    p[40] = poison
    codes, sb = Q.quantize(p, fmt)
    assert sb[1] == 255 and sb[0] != 255 and not codes[32:].any()
    d = Q.dequantize(codes, sb, fmt)
    assert np.isnan(d[32:]).all() and np.isfinite(d[:32]).all()


@pytest.mark.parametrize("fmt", FMTS)
def test_pack_layout(fmt):
    rng = np.random.default_rng(0)
    p = rng.standard_normal(1024).astype(np.float32)
    codes, sb = Q.quantize(p, fmt)
    packed = Q.pack(codes, sb, fmt, 512)
    rb = Q.region_bytes(512, fmt)
    assert rb == {"mxfp8": 512 + 16, "mxfp4": 256 + 16}[fmt] and packed.size == 2 * rb and rb % 16 == 0
    pay = rb - 16
    assert np.array_equal(packed[rb + pay:2 * rb], sb[16:])        # region 1: scales after its payload
    if fmt == "mxfp8":
        assert np.array_equal(packed[rb:rb + pay], codes[512:])
    else:
        assert packed[rb] == codes[512] | (codes[513] << 4)        # element 2i low nibble, 2i + 1 high
    c2, s2 = Q.unpack(packed, fmt, 512)
    assert np.array_equal(c2, codes) and np.array_equal(s2, sb)


@pytest.mark.parametrize("fmt", FMTS)
def test_error_feedback_identity(fmt):
    """sum_t D(q_t) + r_T = sum_t p_t up to two fp32 roundings per step."""
    rng = np.random.default_rng(1)
    T, n = 5, 2048
    r = np.zeros(n, dtype=np.float32)
    sent, true, peak = np.zeros(n), np.zeros(n), 0.0
    for _ in range(T):
        p = (rng.standard_normal(n) * 1e-3).astype(np.float32)
        peak = max(peak, float(np.abs(p + r).max()))
        _, _, d, r = Q.ef_step(p, r, fmt)
        sent += d
        true += p
    assert np.abs(sent + r - true).max() <= T * 2 * 2.0 ** -24 * peak


# ---------------------------------------------------------------------------------------------
# host-side validation of the C ABI (no GPU: every call fails before any HIP call)

@pytest.fixture(scope="module")
def lib():
    if torch.cuda.is_available():
        pytest.skip("host-pointer validation: CPU-only (a device run would launch on host addresses)")
    from evolutionarydistributedtraining_amd import _lib
    return _lib.load_library()


_host = (ctypes.c_uint8 * 4096)()
_P = ctypes.c_void_p


def _fake(i):
    return _P(ctypes.addressof(_host) // 64 * 64 + 64 * (i + 1))     # 16-byte aligned, never dereferenced


def test_abi_validation_of_the_quant_entries(lib):
    ws = (_P * 2)(_fake(1), _fake(2))

    def partial(n=1024, region=512, fmt=0, K=2, gdt=0, wdt=1):
        return lib.edt_delta_partial_q(_fake(0), gdt, ws, wdt, K, 8, n, region, fmt, None, _fake(3), None)

    def err():
        return lib.edt_last_error().decode()

    assert partial(region=500) < 0 and "multiple of 512" in err()
    assert partial(region=0) < 0 and "multiple of 512" in err()
    assert partial(n=1536, region=1024) < 0 and "whole number of regions" in err()
    assert partial(fmt=2) < 0 and "wire format" in err()
    assert partial(fmt=-1) < 0 and "wire format" in err()
    assert partial(K=0) < 0 and "worker count" in err()
    assert partial(K=65) < 0 and "worker count" in err()
    assert partial(gdt=1, wdt=0) < 0 and "dtype" in err()
    regs = (_P * 2)(_fake(4), _fake(5))

    def apply(n=512, fmt=0, nacc=2, gdt=0):
        return lib.edt_sgd_apply_sum_q(_fake(0), gdt, regs, nacc, fmt, _fake(6), 1, n, 0.7, 0.9, 1, None)

    assert apply(n=500) < 0 and "multiple of 512" in err()
    assert apply(fmt=7) < 0 and "wire format" in err()
    assert apply(nacc=0) < 0 and "partial count" in err()
    assert apply(nacc=65) < 0 and "partial count" in err()
    assert apply(gdt=3) < 0 and "dtype" in err()
    assert lib.edt_q_region_bytes(512, 0) == 528 and lib.edt_q_region_bytes(512, 1) == 272
    assert lib.edt_q_region_bytes(1 << 26, 0) == (1 << 26) + (1 << 21)
    assert lib.edt_q_region_bytes(500, 0) == 0 and lib.edt_q_region_bytes(512, 2) == 0
    assert lib.edt_abi_version() == 6


# ---------------------------------------------------------------------------------------------
# the schedule through the kernels= seam, on CPU tensors

SHAPES = [(37, 11), (5,), (1,), (64, 33), (129,), (300,), (7, 401)]


def _hand_reference(oracle, theta0, gens, world, n_pad, fmt, ef, lr=0.7, mu=0.9, nesterov=True):
    """reduce_q composed by hand over the whole padded arena, with no buckets, regions or packing:
    per rank the oracle's fp32 partial, Q/D with the rank's residual, the D's summed in rank
    order, the oracle's SGD. Blocks of 32 start at multiples of 32 of the arena either way."""
    n = theta0.numel()
    th = torch.zeros(n_pad, dtype=theta0.dtype)
    th[:n] = theta0
    mom = torch.zeros_like(th)
    res = [np.zeros(n_pad, dtype=np.float32) if ef else None for _ in range(world)]
    for i, ws in enumerate(gens):
        K = len(ws)
        kl = K // world
        total = None
        for r in range(world):
            pad = [torch.zeros(n_pad, dtype=w.dtype) for w in ws[r * kl:(r + 1) * kl]]
            for dst, w in zip(pad, ws[r * kl:(r + 1) * kl]):
                dst[:n] = w
            acc = torch.zeros(n_pad, dtype=torch.float32)
            oracle.delta_partial(th, pad, K, acc, False)
            _, _, d, res[r] = Q.ef_step(acc.numpy(), res[r], fmt)
            d = torch.from_numpy(d)
            total = d if total is None else total.add_(d)
        oracle.sgd_apply(th, total, mom, i > 0, lr, mu, nesterov)
    return th, mom, res


def _run_reduce_q(world, layout, tdt, wdt, theta0, gens, kernels, fmt, ef, bucket_elems):
    from evolutionarydistributedtraining_amd.collectives import VirtualWorld
    from evolutionarydistributedtraining_amd.distributed import ShardedOuterSync
    k_local = len(gens[0]) // world

    def body(comm):
        s = ShardedOuterSync(layout, tdt, wdt, k_local, theta0.device, mode="reduce_q", wire_format=fmt,
                             error_feedback=ef, bucket_elems=bucket_elems, kernels=kernels, comm=comm)
        s.theta.flat.copy_(theta0)
        for ws in gens:
            for j, a in enumerate(s.workers):
                a.flat.copy_(ws[comm.rank * k_local + j])
            s.step()
        return {"theta": s.theta_buf.clone(), "mom": comm.all_gather_object(s.mom_shard.clone()),
                "residual": None if s.residual is None else s.residual.clone(), "buckets": s.buckets,
                "n_pad": s.n_pad, "wire": s.wire_bytes(), "mode": (s.mode, s.broadcast),
                "kernel_bytes": s.kernel_bytes()}

    res = VirtualWorld(world).run(body)
    r0 = res[0]
    mom = torch.empty(r0["n_pad"], dtype=tdt, device=theta0.device)
    off = [0] * world
    for b, e in r0["buckets"]:
        per = (e - b) // world
        for r in range(world):
            mom[b + r * per:b + (r + 1) * per] = r0["mom"][r][off[r]:off[r] + per]
            off[r] += per
    return res, mom


@pytest.mark.parametrize("world", [2, 3])
@pytest.mark.parametrize("fmt", FMTS)
@pytest.mark.parametrize("tdt,wdt", [(torch.float32, torch.bfloat16), (torch.bfloat16, torch.bfloat16)])
def test_reduce_q_schedule_through_the_kernels_seam(oracle, world, fmt, tdt, wdt):
    layout, theta, gens = population(SHAPES, tdt, wdt, 6, steps=3)
    res, mom = _run_reduce_q(world, layout, tdt, wdt, theta, gens, Q.NumpyQuantKernels(oracle), fmt, True,
                             bucket_elems=world * 512)
    n_pad = res[0]["n_pad"]
    assert len(res[0]["buckets"]) >= 3 and n_pad > layout.total and n_pad % (world * 512) == 0
    assert res[0]["mode"] == ("reduce_q", "theta")
    for r in res:
        assert torch.equal(bits(r["theta"]), bits(res[0]["theta"]))
    th, mom_ref, resid = _hand_reference(oracle, theta, gens, world, n_pad, fmt, True)
    assert torch.equal(bits(res[0]["theta"]), bits(th))
    assert torch.equal(bits(mom), bits(mom_ref))
    for r in range(world):
        assert np.array_equal(res[r]["residual"].numpy().view(np.int32), resid[r].view(np.int32))
        assert np.abs(resid[r]).max() > 0
    bg = theta.element_size()
    q = {"mxfp8": 1 + 1 / 32, "mxfp4": 1 / 2 + 1 / 32}[fmt]
    assert res[0]["wire"] == int((world - 1) / world * n_pad * (q + bg))
    shard = n_pad // world
    k_local, wb = 6 // world, gens[0][0].element_size()
    assert res[0]["kernel_bytes"] == int(n_pad * (k_local * wb + bg + 8 + q) + shard * (4 * bg + world * q))


def test_reduce_q_is_opt_in_and_auto_is_unchanged():
    """mode="auto" picks what the module docstring lists (K = 8), and reduce_q only comes when asked
    for, with broadcast="theta"."""
    from evolutionarydistributedtraining_amd.collectives import VirtualWorld
    from evolutionarydistributedtraining_amd.distributed import ShardedOuterSync
    from evolutionarydistributedtraining_amd.params import ParamLayout
    layout = ParamLayout([(1000,)])
    want = {(torch.bfloat16, 2): ("reduce_ordered", "theta"), (torch.bfloat16, 4): ("exact", "workers"),
            (torch.bfloat16, 8): ("exact", "workers"), (torch.float32, 2): ("reduce_ordered", "theta"),
            (torch.float32, 4): ("reduce_ordered", "theta"), (torch.float32, 8): ("exact", "workers")}
    for (wdt, world), expect in want.items():
        s = ShardedOuterSync(layout, torch.float32, wdt, 8 // world, "cpu", kernels=object(),
                             comm=VirtualWorld(world).comm(0))
        assert (s.mode, s.broadcast) == expect, (wdt, world)
        assert not hasattr(s, "residual")
    comm = VirtualWorld(2).comm(0)
    with pytest.raises(ValueError):
        ShardedOuterSync(layout, torch.float32, torch.bfloat16, 4, "cpu", mode="reduce_q", broadcast="workers",
                         kernels=object(), comm=comm)
    with pytest.raises(ValueError):
        ShardedOuterSync(layout, torch.float32, torch.bfloat16, 4, "cpu", mode="reduce_q", wire_format="int8",
                         kernels=object(), comm=comm)
    s = ShardedOuterSync(layout, torch.float32, torch.bfloat16, 4, "cpu", mode="reduce_q", wire_format="mxfp4",
                         error_feedback=False, kernels=object(), comm=comm)
    assert (s.mode, s.broadcast, s.residual) == ("reduce_q", "theta", None) and s.n_pad == 1024
    assert s.q_send.dtype == torch.uint8 and s.q_send.numel() == s.q_recv.numel() == 1024 // 2 + 1024 // 32
