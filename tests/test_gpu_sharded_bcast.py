"""The new theta handed to the local workers in the sharded step's own pass, on the device:
edt_apply_delta_q_bcast (phase 3 fused with the broadcast) against edt_apply_delta_q on a clone
followed by torch's copy_ per destination, edt_broadcast_theta against copy_, and
ShardedOuterSync.step(broadcast=True) on virtual ranks against step() on an identically built sync —
all bit for bit (NaN elements excepted: NaN in theta and every worker, payload unspecified). The
reference ends every outer step by saving the new base into each worker directory
(EDT_LM/diloco.py:302-308), from which the bf16 workers load it rounded."""
import functools

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
# (n, region_elems): one wave; regions that straddle the 2,048-element workgroup tile; one region
PHASE3_SHAPES = [(512, 512), (4608, 1536), (4608, 4608)]
GUARD = 64                      # elements on either side: 128 or 256 bytes, so the views stay 16-byte aligned
FILL = 77.0


def _np(t):
    return t.detach().cpu().numpy()


def _guarded(n, dt, off=0):
    """(buffer, view of n elements inside it, `off` elements past the aligned start)."""
    buf = torch.full((n + 2 * GUARD + off,), FILL, dtype=dt, device=DEV)
    return buf, buf[GUARD + off:GUARD + off + n]


def _guards_intact(buf, n, off=0):
    return bool((buf[:GUARD + off] == FILL).all() and (buf[GUARD + off + n:] == FILL).all())


def _copy_of(theta, wdt):
    return torch.empty(theta.numel(), dtype=wdt, device=DEV).copy_(theta)


# ---------------------------------------------------------------------------------------------
# phase 3 fused with the broadcast

@pytest.mark.parametrize("nbcast", [1, 3])
@pytest.mark.parametrize("fmt", FMTS)
@pytest.mark.parametrize("tdt,wdt", PAIRS)
def test_fused_phase3_equals_phase3_then_copy(tdt, wdt, fmt, nbcast):
    """Codes and scales as tests/test_gpu_gather_q.py::test_phase3_adds_the_dequantized_update builds
    them (scale bytes 0, 1, 62-64 and 127; once with a scale-255 block): theta equals the plain
    entry's on a clone bit for bit, every destination equals copy_ from that theta wherever theta is
    not NaN, the NaN masks agree and count 32 (poisoned) or 0, guards and `packed` keep their bytes."""
    rng = np.random.default_rng(3)
    g = torch.Generator().manual_seed(5)
    nb = Q.FORMATS[fmt]["bits"]
    for n, region in PHASE3_SHAPES:
        codes = rng.integers(0, 1 << nb, n).astype(np.uint8)
        if fmt == "mxfp8":
            codes[(codes & 0x7f) == 0x7f] = 0x7e
        scales = rng.integers(100, 128, n // 32).astype(np.uint8)
        scales[:6] = [0, 1, 62, 63, 64, 127]
        for poison in (False, True):
            if poison:
                scales[9] = 255
            want_packed = Q.pack(codes, scales, fmt, region)
            packed = torch.from_numpy(want_packed).to(DEV)
            tbuf, theta = _guarded(n, tdt)
            theta.copy_((torch.randn(n, generator=g) * 0.02).to(tdt))
            plain = theta.clone()
            ops.apply_delta_q(plain, packed, region, fmt)
            dsts = [_guarded(n, wdt) for _ in range(nbcast)]
            ops.apply_delta_q(theta, packed, region, fmt, broadcast=[d for _, d in dsts])
            tag = (n, region, poison)
            assert torch.equal(bits(theta), bits(plain)), tag
            assert not torch.equal(bits(theta), bits(tbuf.new_full((n,), FILL))), tag
            nan = torch.isnan(theta)
            assert int(nan.sum()) == (32 if poison else 0), tag
            if poison:
                assert nan[9 * 32:10 * 32].all(), tag
            want = _copy_of(plain, wdt)
            for dbuf, d in dsts:
                assert torch.equal(torch.isnan(d), nan), tag
                assert torch.equal(bits(d)[~nan], bits(want)[~nan]), tag
                assert _guards_intact(dbuf, n), tag
            assert _guards_intact(tbuf, n), tag
            assert np.array_equal(_np(packed), want_packed), tag


@pytest.mark.parametrize("fmt", FMTS)
@pytest.mark.parametrize("tdt,wdt", PAIRS)
def test_a_destination_may_be_a_worker_the_caller_just_used(tdt, wdt, fmt):
    """The schedule's own use: the tensors phase 1 read as workers are phase 3's destinations (the
    same tensor objects, not aliased with theta)."""
    n, region, K = 4608, 1536, 3
    g = torch.Generator().manual_seed(11)
    theta = (torch.randn(n, generator=g) * 0.02).to(tdt).to(DEV)
    workers = [(theta.float().cpu() + torch.randn(n, generator=g) * 1e-3).to(wdt).to(DEV) for _ in range(K)]
    packed = torch.empty(n // region * ops.q_region_bytes(region, fmt), dtype=torch.uint8, device=DEV)
    ops.delta_partial_q(theta, workers, K, packed, region, fmt)
    before = [w.clone() for w in workers]
    plain = theta.clone()
    ops.apply_delta_q(plain, packed, region, fmt)
    ops.apply_delta_q(theta, packed, region, fmt, broadcast=workers)
    assert torch.equal(bits(theta), bits(plain)) and not torch.isnan(theta).any()
    want = _copy_of(plain, wdt)
    for w, w0 in zip(workers, before):
        assert torch.equal(bits(w), bits(want)) and not torch.equal(bits(w), bits(w0))


# ---------------------------------------------------------------------------------------------
# the broadcast alone

SIZES = (1, 7, 8, 2047, 2048, 2049, 40961)
# values whose rounding to bf16 is a tie (to even: down, up), overflows to inf, is exact, or is an
# fp32 subnormal (bf16 has fp32's exponent range); signed zeros and infinities
SPECIAL = [1.00390625, 1.01171875, -1.00390625, 3.3895314e38, -3.3895314e38, float("inf"), float("-inf"), 0.0, -0.0,
           1e-40, -3e-39, 65280.0]


def _theta_values(n, tdt, g):
    x = torch.randn(n, generator=g) * 0.02
    k = min(n, len(SPECIAL))
    x[:k] = torch.tensor(SPECIAL[:k])
    return x.to(tdt)


@pytest.mark.parametrize("nbcast", [1, 2, 5])
@pytest.mark.parametrize("tdt,wdt", PAIRS)
def test_broadcast_theta_equals_copy(tdt, wdt, nbcast):
    """Every size (below, at and past the 8-element vector and the 2,048-element tile; many blocks)
    with every operand aligned, with theta one element off a 16-byte boundary, and with the last
    destination one element off: bit-equal to copy_, guards and theta untouched."""
    g = torch.Generator().manual_seed(23)
    for n in SIZES:
        vals = _theta_values(n, tdt, g).to(DEV)
        want = _copy_of(vals, wdt)
        for toff, doff in ((0, 0), (1, 0), (0, 1)):
            tbuf, theta = _guarded(n, tdt, toff)
            theta.copy_(vals)
            offs = [0] * (nbcast - 1) + [doff]
            dsts = [_guarded(n, wdt, o) for o in offs]
            ops.broadcast_theta(theta, [d for _, d in dsts])
            tag = (n, toff, doff)
            for (dbuf, d), o in zip(dsts, offs):
                assert torch.equal(bits(d), bits(want)), tag
                assert _guards_intact(dbuf, n, o), tag
            assert torch.equal(bits(theta), bits(vals)) and _guards_intact(tbuf, n, toff), tag


def test_broadcast_theta_takes_65_destinations_in_chunks():
    n = 2049
    theta = _theta_values(n, torch.float32, torch.Generator().manual_seed(3)).to(DEV)
    outs = [torch.full((n,), FILL, dtype=torch.bfloat16, device=DEV) for _ in range(65)]
    ops.broadcast_theta(theta, outs)
    want = _copy_of(theta, torch.bfloat16)
    assert all(torch.equal(bits(o), bits(want)) for o in outs)


# ---------------------------------------------------------------------------------------------
# the schedules on virtual ranks

SHAPES = [(37, 11), (5,), (1,), (256, 513), (129,), (3, 9001), (1001,), (2, 77)]     # tests/test_gpu_gather_q.py's
MODES = {
    "reduce": {"mode": "reduce"},
    "reduce_ordered": {"mode": "reduce_ordered"},
    "reduce_q": {"mode": "reduce_q"},
    "reduce_q+gather": {"mode": "reduce_q", "gather_format": "mxfp8"},
    "reduce_q+gather+sr": {"mode": "reduce_q", "gather_format": "mxfp8", "rounding": "stochastic",
                           "error_feedback": False, "seed": 0x5eed},
    "exact": {"mode": "exact"},
}


@functools.lru_cache(maxsize=None)
def _population(tdt, wdt):
    return population(SHAPES, tdt, wdt, 8, steps=3, device=DEV)


def _drive(world, kw, tdt, wdt, bcast):
    """`world` virtual ranks, 3 steps with fresh workers each; per rank and step what the sync holds."""
    from evolutionarydistributedtraining_amd.distributed import ShardedOuterSync
    layout, theta, gens = _population(tdt, wdt)
    k_local = 8 // world

    def body(comm):
        s = ShardedOuterSync(layout, tdt, wdt, k_local, DEV, bucket_elems=world * 512 * 37, comm=comm,
                             broadcast="theta", **kw)
        s.theta.flat.copy_(theta)
        steps = []
        for ws in gens:
            for j, w in enumerate(s.worker_bufs):
                w[:layout.total].copy_(ws[comm.rank * k_local + j])
                w[layout.total:].zero_()
            loaded = [w.clone() for w in s.worker_bufs]
            s.step(broadcast=True) if bcast else s.step()
            state = {"theta": s.theta_buf, "mom": s.mom_shard, "residual": getattr(s, "residual", None),
                     "residual_g": getattr(s, "residual_g", None), "q_send": getattr(s, "q_send", None),
                     "q_recv": getattr(s, "q_recv", None), "u_recv": getattr(s, "u_recv", None)}
            steps.append({"state": {k: None if v is None else v.clone() for k, v in state.items()},
                          "q_step": s.q_step, "has_momentum": s.has_momentum, "loaded": loaded,
                          "workers": [w.clone() for w in s.worker_bufs]})
        return {"steps": steps, "buckets": s.buckets, "n_pad": s.n_pad, "wire": s.wire_bytes()}

    res = VirtualWorld(world).run(body)
    torch.cuda.synchronize()
    return layout, res


@pytest.mark.parametrize("world", [2, 4])
@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("tdt,wdt", PAIRS)
def test_step_broadcast_refreshes_the_workers_and_changes_nothing_else(world, mode, tdt, wdt):
    layout, plain = _drive(world, MODES[mode], tdt, wdt, False)
    _, bc = _drive(world, MODES[mode], tdt, wdt, True)
    buckets, n_pad = bc[0]["buckets"], bc[0]["n_pad"]
    assert len(buckets) >= 3 and n_pad > layout.total and len({e - b for b, e in buckets}) == 2   # ragged last bucket
    for r in range(world):
        assert plain[r]["wire"] == bc[r]["wire"]
        for i, (a, b) in enumerate(zip(plain[r]["steps"], bc[r]["steps"])):
            tag = (r, i)
            assert a["q_step"] == b["q_step"] == i + 1 and a["has_momentum"] and b["has_momentum"], tag
            for key, x in a["state"].items():
                y = b["state"][key]
                assert (x is None) == (y is None), (tag, key)
                if x is not None:
                    assert torch.equal(x.view(torch.uint8), y.view(torch.uint8)), (tag, key)
            theta = b["state"]["theta"]
            assert theta.numel() == n_pad and not torch.isnan(theta).any(), tag
            want = theta.to(wdt)
            for w, w0 in zip(b["workers"], b["loaded"]):
                assert w.numel() == n_pad and torch.equal(bits(w), bits(want)), tag
                assert not torch.equal(bits(w), bits(w0)), tag
            for w, w0 in zip(a["workers"], a["loaded"]):
                assert torch.equal(bits(w), bits(w0)), tag


def test_exact_workers_accepts_the_flag_and_does_what_it_did():
    from evolutionarydistributedtraining_amd.distributed import ShardedOuterSync
    tdt, wdt, world = torch.float32, torch.bfloat16, 2
    layout, theta, gens = _population(tdt, wdt)

    def run(bcast):
        def body(comm):
            s = ShardedOuterSync(layout, tdt, wdt, 4, DEV, mode="exact", broadcast="workers",
                                 bucket_elems=world * 512 * 37, comm=comm)
            s.theta.flat.copy_(theta)
            for j, a in enumerate(s.workers):
                a.flat.copy_(gens[0][comm.rank * 4 + j])
            s.step(broadcast=True) if bcast else s.step()
            return [w.clone() for w in s.worker_bufs], s.gather_theta().clone(), s.kernel_bytes(), s.kernel_bytes(True)
        return VirtualWorld(world).run(body)

    for (wa, ta, ka, _), (wb, tb, kb, kbt) in zip(run(False), run(True)):
        assert torch.equal(bits(ta), bits(tb)) and ka == kb == kbt
        for x, y in zip(wa, wb):
            assert torch.equal(bits(x), bits(y)) and torch.equal(bits(x[:layout.total]), bits(tb.to(wdt)))


# ---------------------------------------------------------------------------------------------
# the wrappers

def test_wrappers_validate_their_arguments():
    """Past 64 destinations apply_delta_q chunks: the fused launch takes the first 64 and
    broadcast_theta the rest (both store round_w of the same theta)."""
    n = 1024
    theta = torch.zeros(n, device=DEV)
    tb = torch.zeros(n, dtype=torch.bfloat16, device=DEV)
    reg = torch.zeros(ops.q_region_bytes(n, "mxfp8"), dtype=torch.uint8, device=DEV)
    w32 = [torch.zeros(n, device=DEV) for _ in range(2)]
    w16 = [torch.zeros(n, dtype=torch.bfloat16, device=DEV) for _ in range(2)]
    both = torch.zeros(2 * n, device=DEV)

    def apply(theta=theta, outs=w16):
        ops.apply_delta_q(theta, reg, n, "mxfp8", broadcast=outs)

    def bcast(theta=theta, outs=w16):
        ops.broadcast_theta(theta, outs)

    for ok in (apply, bcast):
        ok()
        ok(outs=w32)
        ok(theta=tb)
        ok(theta=both[:n], outs=[both[n:]])                       # adjacent, not overlapping
    apply(outs=[])                                                # the plain entry
    apply(outs=None)
    bcast(outs=[])                                                # nothing to do
    for fn in (apply, bcast):
        bad_calls = [
            lambda: fn(theta=tb, outs=w32),                       # dtype pair: bf16 theta, fp32 workers
            lambda: fn(outs=[w16[0], w32[0]]),                    # dtype mix
            lambda: fn(outs=[w16[0].half()]),                     # dtype
            lambda: fn(outs=[w16[0][:-8]]),                       # length
            lambda: fn(outs=[w16[0], tb[:512]]),                  # length
            lambda: fn(outs=[theta]),                             # theta itself
            lambda: fn(theta=both[:n], outs=[both[n - 8:2 * n - 8]]),   # overlapping theta's tail
            lambda: fn(outs=[w16[0].cpu()]),                      # device
            lambda: fn(theta=theta.cpu()),                        # device
            lambda: fn(outs=[torch.zeros(2 * n, dtype=torch.bfloat16, device=DEV)[::2]]),   # not contiguous
        ]
        for i, call in enumerate(bad_calls):
            with pytest.raises(EdtError):
                call()
                pytest.fail(f"{fn.__name__} call {i} was accepted")
    rb = reg.numel()                                              # a destination over `packed`'s last 16 bytes
    raw = torch.zeros(rb + 2 * n, dtype=torch.uint8, device=DEV)
    with pytest.raises(EdtError, match="overlaps packed"):
        ops.apply_delta_q(theta, raw[:rb], n, "mxfp8", broadcast=[raw[rb - 16:rb - 16 + 2 * n].view(torch.bfloat16)])
    ops.apply_delta_q(theta, raw[:rb], n, "mxfp8", broadcast=[raw[rb:].view(torch.bfloat16)])     # adjacent
    # 65 destinations: chunked, every one written
    g = torch.Generator().manual_seed(2)
    th = (torch.randn(n, generator=g) * 0.02).to(DEV)
    outs = [torch.full((n,), FILL, dtype=torch.bfloat16, device=DEV) for _ in range(65)]
    codes = np.random.default_rng(1).integers(0, 0x7e, n).astype(np.uint8)
    packed = torch.from_numpy(Q.pack(codes, np.full(n // 32, 110, dtype=np.uint8), "mxfp8", n)).to(DEV)
    plain = th.clone()
    ops.apply_delta_q(plain, packed, n, "mxfp8")
    ops.apply_delta_q(th, packed, n, "mxfp8", broadcast=outs)
    want = _copy_of(plain, torch.bfloat16)
    assert torch.equal(bits(th), bits(plain)) and not torch.equal(bits(th), bits(torch.zeros_like(th)))
    assert all(torch.equal(bits(o), bits(want)) for o in outs)
