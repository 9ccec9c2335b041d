"""The quantized gather of the reduce_q schedule on the device (csrc/edt_quant.hip):
edt_sgd_delta_sum_q (phase 2') against the existing edt_sgd_apply_sum_q on a clone plus the numpy
quantizer (tests/gather_q_reference.py), edt_apply_delta_q (phase 3) against torch's
fp32 add and rounding on the dequantized array, and the schedule of ShardedOuterSync with
gather_format on virtual ranks against that composition — all bit for bit. The reference has no
such path (its workers exchange checkpoints on disk, EDT_LM/diloco.py:231-235, 302-308)."""
import numpy as np
import pytest
import torch

from evolutionarydistributedtraining_amd import ops
from evolutionarydistributedtraining_amd._lib import EdtError
from evolutionarydistributedtraining_amd.collectives import VirtualWorld
from tests import gather_q_reference as G
from tests import quant_reference as Q
from tests.virtual_schedules import bits, population

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
FMTS = ["mxfp8", "mxfp4"]
PAIRS = [(torch.float32, torch.float32), (torch.float32, torch.bfloat16), (torch.bfloat16, torch.bfloat16)]
FMT_PAIRS = [("mxfp8", "mxfp8"), ("mxfp4", "mxfp8"), ("mxfp8", "mxfp4")]
# one wave, one full block, an odd tile count that leaves a partial block in the grid-stride loop
SIZES = (512, 2048, 37 * 512)
# odd tensor sizes (292,187 elements), as tests/test_gpu_quant.py
SHAPES = [(37, 11), (5,), (1,), (256, 513), (129,), (3, 9001), (1001,), (2, 77)]
QB = {"mxfp8": 1 + 1 / 32, "mxfp4": 1 / 2 + 1 / 32}


def _np(t):
    return t.detach().cpu().numpy()


def _same_bits(a, b):
    return np.array_equal(np.asarray(a).view(np.int32), np.asarray(b).view(np.int32))


def _regions(rng, n, nacc, fmt):
    """nacc packed regions of n elements: quantized partials ~ 1e-3."""
    out = []
    for _ in range(nacc):
        a = (rng.standard_normal(n) * 1e-3).astype(np.float32)
        out.append(torch.from_numpy(Q.pack(*Q.quantize(a, fmt), fmt, n)).to(DEV))
    return out


@pytest.mark.parametrize("tdt", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("nacc", [1, 2, 8])
@pytest.mark.parametrize("fmt_in", FMTS)
@pytest.mark.parametrize("fmt_out", FMTS)
def test_phase2_momentum_update_and_residual_bit_for_bit(tdt, nacc, fmt_in, fmt_out):
    """The momentum equals edt_sgd_apply_sum_q's on a clone, theta is not written, and packed_out /
    the residual equal delta_step(theta, the clone's theta', r, fmt_out) over two chained calls from a
    non-zero residual (the second call starts from the first one's momentum and residual); then
    once without a residual."""
    rng = np.random.default_rng(100 * nacc + len(fmt_in))
    g = torch.Generator().manual_seed(7 + nacc)
    for n in SIZES:
        regions = _regions(rng, n, nacc, fmt_in)
        theta = (torch.randn(n, generator=g) * 0.02).to(tdt).to(DEV)
        theta0 = theta.clone()
        mom0 = (torch.randn(n, generator=g) * 1e-3).to(tdt).to(DEV)
        for nesterov, has, mu in [(True, True, 0.9), (True, False, 0.9), (False, True, 0.9), (False, False, 0.9),
                                  (False, False, 0.0)]:
            mom = mom0.clone() if mu else None
            r = (torch.randn(n, generator=g) * 1e-5).numpy()
            res = torch.from_numpy(r).to(DEV)
            packed = torch.empty(ops.q_region_bytes(n, fmt_out), dtype=torch.uint8, device=DEV)
            for call in range(3):
                ef = call < 2
                th_ref = theta.clone()
                mom_ref = None if mom is None else mom.clone()
                ops.sgd_apply_sum_q(th_ref, regions, fmt_in, mom_ref, has, 0.7, mu, nesterov)
                packed.fill_(0xAA)
                ops.sgd_delta_sum_q(theta, regions, fmt_in, mom, has, 0.7, mu, nesterov, packed, fmt_out,
                                    res if ef else None)
                tag = (n, nesterov, has, mu, call)
                assert torch.equal(bits(theta), bits(theta0)), tag
                assert not torch.equal(bits(th_ref), bits(theta0)), tag
                if mom is not None:
                    assert torch.equal(bits(mom), bits(mom_ref)), tag
                codes, scales, _, r_new = G.delta_step(theta, th_ref, r if ef else None, fmt_out)
                assert np.array_equal(_np(packed), Q.pack(codes, scales, fmt_out, n)), tag
                if ef:
                    r = r_new
                    assert np.abs(r).max() > 0
                assert _same_bits(_np(res), r), tag


@pytest.mark.parametrize("tdt", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("fmt", FMTS)
def test_phase3_adds_the_dequantized_update(tdt, fmt):
    """theta after edt_apply_delta_q == (theta.float() + D).to(dtype) for any valid codes under any
    scale (bytes 0, 1, 62-64 and 127 included), with regions of 512 and of n elements; a block
    with scale byte 255 makes exactly its 32 elements NaN; theta's neighbours keep their bytes."""
    rng = np.random.default_rng(3)
    g = torch.Generator().manual_seed(5)
    nb = Q.FORMATS[fmt]["bits"]
    guard = 64
    for n in SIZES:
        codes = rng.integers(0, 1 << nb, n).astype(np.uint8)
        if fmt == "mxfp8":
            codes[(codes & 0x7f) == 0x7f] = 0x7e
        scales = rng.integers(100, 128, n // 32).astype(np.uint8)
        scales[:6] = [0, 1, 62, 63, 64, 127]
        for poison in (False, True):
            if poison:
                scales[9] = 255
            d = Q.dequantize(codes, scales, fmt)
            for region in sorted({512, n}):
                buf = torch.full((n + 2 * guard,), 123.0, dtype=tdt, device=DEV)
                theta = buf[guard:guard + n]
                theta.copy_((torch.randn(n, generator=g) * 0.02).to(tdt))
                want = G.apply_delta(theta, d)
                packed = torch.from_numpy(Q.pack(codes, scales, fmt, region)).to(DEV)
                ops.apply_delta_q(theta, packed, region, fmt)
                tag = (n, region, poison)
                nan = torch.isnan(theta)
                if poison:
                    assert nan[9 * 32:10 * 32].all() and int(nan.sum()) == 32, tag
                    assert torch.equal(torch.isnan(want), nan), tag
                else:
                    assert not nan.any(), tag
                assert torch.equal(bits(theta)[~nan], bits(want)[~nan]), tag
                assert not torch.equal(bits(theta), bits(buf.new_full((n,), 123.0))), tag
                assert (buf[:guard] == 123.0).all() and (buf[guard + n:] == 123.0).all(), tag
                assert np.array_equal(_np(packed), Q.pack(codes, scales, fmt, region)), tag


def _partial(theta, workers, k_total):
    acc = torch.empty(theta.numel(), dtype=torch.float32, device=DEV)
    ops.delta_partial(theta, workers, k_total, acc)
    return _np(acc)


def _composition(theta0, gens, world, n_pad, fmt_in, fmt_out, ef, lr=0.7, mu=0.9, nesterov=True):
    """ops.delta_partial per rank -> numpy Q / D with the rank's residual -> ops.sgd_apply_sum on a
    copy of theta -> numpy Q / D of the update with the owners' residual (one array over the arena:
    every element has one owner) -> torch's fp32 add and rounding. No buckets, regions or packing."""
    n = theta0.numel()
    th = torch.zeros(n_pad, dtype=theta0.dtype, device=DEV)
    th[:n] = theta0
    mom = torch.zeros_like(th)
    res = [np.zeros(n_pad, dtype=np.float32) if ef else None for _ in range(world)]
    res_g = np.zeros(n_pad, dtype=np.float32) if ef else None
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
            _, _, d, res[r] = Q.ef_step(_partial(th, pads, K), res[r], fmt_in)
            ds.append(torch.from_numpy(d).to(DEV))
        new = th.clone()
        ops.sgd_apply_sum(new, ds, mom, i > 0, lr, mu, nesterov)
        _, _, d, res_g = G.delta_step(th, new, res_g, fmt_out)
        th = G.apply_delta(th, d)
    torch.cuda.synchronize()
    return th, mom, res, res_g


@pytest.mark.parametrize("world,units", [(2, 37), (4, 37), (8, 17)])
@pytest.mark.parametrize("fmt_in,fmt_out", FMT_PAIRS)
@pytest.mark.parametrize("ef", [True, False])
@pytest.mark.parametrize("tdt,wdt", PAIRS)
def test_gather_q_schedule_on_virtual_ranks(world, units, fmt_in, fmt_out, ef, tdt, wdt):
    from evolutionarydistributedtraining_amd.distributed import ShardedOuterSync
    layout, theta, gens = population(SHAPES, tdt, wdt, 8, steps=3, device=DEV)
    k_local = 8 // world

    def body(comm):
        s = ShardedOuterSync(layout, tdt, wdt, k_local, DEV, mode="reduce_q", wire_format=fmt_in, error_feedback=ef,
                             bucket_elems=world * 512 * units, comm=comm, gather_format=fmt_out)
        s.theta.flat.copy_(theta)
        for ws in gens:
            for j, a in enumerate(s.workers):
                a.flat.copy_(ws[comm.rank * k_local + j])
            s.step()
        return {"theta": s.theta_buf.clone(), "mom": s.mom_shard.clone(),
                "residual": None if s.residual is None else s.residual.clone(),
                "residual_g": None if s.residual_g is None else s.residual_g.clone(), "buckets": s.buckets,
                "n_pad": s.n_pad, "wire": s.wire_bytes()}

    res = VirtualWorld(world).run(body)
    torch.cuda.synchronize()
    n_pad, buckets = res[0]["n_pad"], res[0]["buckets"]
    sizes = {e - b for b, e in buckets}
    assert len(buckets) >= 3 and n_pad > layout.total and len(sizes) == 2            # ragged last bucket
    for r in res:
        assert torch.equal(bits(r["theta"]), bits(res[0]["theta"]))
    th, mom_ref, resid, resid_g = _composition(theta, gens, world, n_pad, fmt_in, fmt_out, ef)
    assert torch.equal(bits(res[0]["theta"]), bits(th))
    for r in range(world):
        # this rank's shards in bucket order: how mom_shard and residual_g are laid out
        own = np.concatenate([np.arange(b + r * ((e - b) // world), b + (r + 1) * ((e - b) // world))
                              for b, e in buckets])
        assert torch.equal(bits(res[r]["mom"]), bits(mom_ref[torch.from_numpy(own).to(DEV)])), r
        if ef:
            assert _same_bits(_np(res[r]["residual"]), resid[r]), r
            assert _same_bits(_np(res[r]["residual_g"]), resid_g[own]), r
        else:
            assert res[r]["residual"] is None and res[r]["residual_g"] is None
    if ef:
        assert np.abs(resid_g).max() > 0
    assert res[0]["wire"] == int((world - 1) / world * n_pad * (QB[fmt_in] + QB[fmt_out]))


@pytest.mark.parametrize("fmt", FMTS)
def test_update_error_feedback_identity_on_the_device(fmt):
    """fp32 theta, T = 4 steps of phase 2' + phase 3 on one shard: per element
    theta_T - theta_0 + r_T = sum_t u_t, u_t = fl(theta'_t - theta_t) being the update that phase 2'
    quantizes (theta'_t from edt_sgd_apply_sum_q on a clone). Per step three fp32 roundings separate
    the two sides: u' = fl(u + r) and r' = fl(u' - D(q)), each within 2^-24 |u'| (|r'| <= |u'| here:
    D(q) rounds u' on a grid that holds 0), and theta <- fl(theta + D(q)) within half an ulp of the
    new theta, <= 2^-24 |theta|. With r_0 = 0 the exact recurrences telescope, so
    |theta_T - theta_0 + r_T - sum u_t| <= T (2 * 2^-24 max|u'| + 2^-24 max|theta|)."""
    n, T, nacc = 8 * 512, 4, 4
    rng = np.random.default_rng(23)
    g = torch.Generator().manual_seed(17)
    theta = (torch.randn(n, generator=g) * 0.02).to(DEV)
    theta0 = _np(theta).astype(np.float64)
    mom = torch.zeros(n, device=DEV)
    res = torch.zeros(n, dtype=torch.float32, device=DEV)
    packed = torch.empty(ops.q_region_bytes(n, fmt), dtype=torch.uint8, device=DEV)
    true, peak_u, peak_t = np.zeros(n), 0.0, float(np.abs(theta0).max())
    for t in range(T):
        regions = _regions(rng, n, nacc, "mxfp8")
        new = theta.clone()
        ops.sgd_apply_sum_q(new, regions, "mxfp8", mom.clone(), t > 0, 0.7, 0.9, True)
        u = _np(new) - _np(theta)                                   # fp32 subtract
        peak_u = max(peak_u, float(np.abs(u + _np(res)).max()))
        ops.sgd_delta_sum_q(theta, regions, "mxfp8", mom, t > 0, 0.7, 0.9, True, packed, fmt, res)
        ops.apply_delta_q(theta, packed, n, fmt)
        true += u
        peak_t = max(peak_t, float(np.abs(_np(theta)).max()))
    r = _np(res).astype(np.float64)
    assert np.abs(r).max() > 0
    err = np.abs(_np(theta).astype(np.float64) - theta0 + r - true).max()
    assert err <= T * (2 * 2.0 ** -24 * peak_u + 2.0 ** -24 * peak_t)


def test_wrappers_validate_their_arguments():
    n = 1024
    theta = torch.zeros(n, device=DEV)
    mom = torch.zeros(n, device=DEV)
    reg8 = torch.zeros(ops.q_region_bytes(n, "mxfp8"), dtype=torch.uint8, device=DEV)
    reg4 = torch.zeros(ops.q_region_bytes(n, "mxfp4"), dtype=torch.uint8, device=DEV)
    res = torch.zeros(n, device=DEV)

    def delta(theta=theta, regions=(reg8,), fin="mxfp8", mom=mom, out=reg4, fout="mxfp4", res=res):
        ops.sgd_delta_sum_q(theta, list(regions), fin, mom, True, 0.7, 0.9, True, out, fout, res)

    def apply(theta=theta, packed=reg8, region=n, fmt="mxfp8"):
        ops.apply_delta_q(theta, packed, region, fmt)

    delta()
    apply()
    apply(packed=torch.zeros(2 * ops.q_region_bytes(512, "mxfp4"), dtype=torch.uint8, device=DEV), region=512, fmt="mxfp4")
    bad_calls = [
        lambda: delta(theta=theta.double()),                                         # dtype
        lambda: delta(theta=theta[:1000]),                                           # size: n % 512
        lambda: delta(regions=()),                                                   # no regions
        lambda: delta(regions=(reg8, reg4)),                                         # region size for fmt_in
        lambda: delta(regions=(reg8.to(torch.int8),)),                               # region dtype
        lambda: delta(regions=(reg8.cpu(),)),                                        # device
        lambda: delta(fin="int8"),                                                   # format
        lambda: delta(fout="fp4"),                                                   # format
        lambda: delta(out=reg8),                                                     # packed_out size for fmt_out
        lambda: delta(out=reg4.to(torch.int8)),                                      # packed_out dtype
        lambda: delta(out=reg4.cpu()),                                               # device
        lambda: delta(mom=mom.bfloat16()),                                           # momentum dtype
        lambda: delta(mom=mom[:512]),                                                # momentum size
        lambda: delta(res=res.half()),                                               # residual dtype
        lambda: delta(res=res[:-1]),                                                 # residual size
        lambda: delta(res=res.cpu()),                                                # device
        lambda: apply(theta=theta.double()),                                         # dtype
        lambda: apply(theta=theta.cpu()),                                            # device
        lambda: apply(packed=reg8.to(torch.int8)),                                   # dtype
        lambda: apply(packed=reg8[:-16]),                                            # size
        lambda: apply(packed=reg4),                                                  # size for fmt
        lambda: apply(packed=reg8.cpu()),                                            # device
        lambda: apply(fmt="int8"),                                                   # format
        lambda: apply(region=500),                                                   # region % 512
        lambda: apply(region=0),                                                     # region
        lambda: apply(theta=torch.zeros(1536, device=DEV), region=1024),             # n % region
    ]
    for i, call in enumerate(bad_calls):
        with pytest.raises(EdtError):
            call()
            pytest.fail(f"call {i} was accepted")
