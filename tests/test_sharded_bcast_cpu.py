"""ShardedOuterSync.step(broadcast=True) without a GPU: every schedule on virtual ranks through the
kernels= seam with the oracle stand-ins (which lack the two new kernels, so the step takes its
copy_ fallback), the host-side validation of edt_apply_delta_q_bcast and edt_broadcast_theta, and
kernel_bytes(broadcast=True). The reference ends every outer step by saving the new base into each
worker directory (EDT_LM/diloco.py:302-308); the GPU form is tests/test_gpu_sharded_bcast.py."""
import ctypes

import pytest
import torch

from tests import gather_q_reference as G
from tests import sr_reference as S
from tests.oracle_kernels import OracleKernels
from tests.test_gather_q_cpu import QB, SHAPES, _fake
from tests.virtual_schedules import bits, population

_P = ctypes.c_void_p
K_TOTAL = 6
PAIRS = [(torch.float32, torch.bfloat16), (torch.bfloat16, torch.bfloat16), (torch.float32, torch.float32)]
# name -> (the stand-in kernels of the schedule, its options)
MODES = {
    "reduce": (OracleKernels, {"mode": "reduce"}),
    "reduce_ordered": (OracleKernels, {"mode": "reduce_ordered"}),
    "reduce_q": (G.NumpyGatherKernels, {"mode": "reduce_q"}),
    "reduce_q+gather": (G.NumpyGatherKernels, {"mode": "reduce_q", "gather_format": "mxfp8"}),
    "reduce_q+gather+sr": (S.NumpySrKernels, {"mode": "reduce_q", "gather_format": "mxfp8", "rounding": "stochastic",
                                              "error_feedback": False, "seed": 0x5eed}),
    "exact": (OracleKernels, {"mode": "exact"}),
}


def _drive(oracle, world, mode, tdt, wdt, bcast, steps=3):
    from evolutionarydistributedtraining_amd.collectives import VirtualWorld
    from evolutionarydistributedtraining_amd.distributed import ShardedOuterSync
    layout, theta, gens = population(SHAPES, tdt, wdt, K_TOTAL, steps=steps)
    make, kw = MODES[mode]
    k_local = K_TOTAL // world

    def body(comm):
        kernels = make(oracle)
        assert not hasattr(kernels, "broadcast_theta")             # the fallback is what runs here
        s = ShardedOuterSync(layout, tdt, wdt, k_local, "cpu", bucket_elems=world * 512, kernels=kernels, comm=comm,
                             broadcast="theta", **kw)
        s.theta.flat.copy_(theta)
        out = []
        for ws in gens:
            for j, w in enumerate(s.worker_bufs):
                w[:layout.total].copy_(ws[comm.rank * k_local + j])
                w[layout.total:].zero_()
            loaded = [w.clone() for w in s.worker_bufs]
            s.step(broadcast=True) if bcast else s.step()
            state = {"theta": s.theta_buf, "mom": s.mom_shard, "residual": getattr(s, "residual", None),
                     "residual_g": getattr(s, "residual_g", None), "q_send": getattr(s, "q_send", None),
                     "q_recv": getattr(s, "q_recv", None), "u_recv": getattr(s, "u_recv", None)}
            out.append({"state": {k: None if v is None else v.clone() for k, v in state.items()}, "q_step": s.q_step,
                        "loaded": loaded, "workers": [w.clone() for w in s.worker_bufs]})
        return {"steps": out, "buckets": s.buckets, "n_pad": s.n_pad, "wire": s.wire_bytes(), "sync": s}

    return layout, VirtualWorld(world).run(body)


@pytest.mark.parametrize("world", [2, 3])
@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("tdt,wdt", PAIRS[:2])
def test_step_broadcast_through_the_kernels_seam(oracle, world, mode, tdt, wdt):
    """Two identically built syncs, one stepping with broadcast=True: theta, the momentum, the
    residuals, the packed buffers and q_step agree bit for bit on every rank after every step; every
    worker arena of the second equals theta_buf.to(wdt) over all of n_pad; the first one's workers
    are untouched."""
    layout, plain = _drive(oracle, world, mode, tdt, wdt, False)
    _, bc = _drive(oracle, world, mode, tdt, wdt, True)
    buckets, n_pad = bc[0]["buckets"], bc[0]["n_pad"]
    assert len(buckets) >= 3 and n_pad > layout.total
    for r in range(world):
        assert plain[r]["wire"] == bc[r]["wire"]
        for i, (a, b) in enumerate(zip(plain[r]["steps"], bc[r]["steps"])):
            tag = (r, i)
            assert a["q_step"] == b["q_step"] == i + 1, tag
            for key, x in a["state"].items():
                y = b["state"][key]
                assert (x is None) == (y is None), (tag, key)
                if x is not None:
                    assert torch.equal(x.view(torch.uint8), y.view(torch.uint8)), (tag, key)
            want = b["state"]["theta"].to(wdt)
            for w, w0 in zip(b["workers"], b["loaded"]):
                assert w.numel() == n_pad and torch.equal(bits(w), bits(want)), tag
                assert not torch.equal(bits(w), bits(w0)), tag
            for w, w0 in zip(a["workers"], a["loaded"]):
                assert torch.equal(bits(w), bits(w0)), tag


def test_exact_workers_accepts_the_flag(oracle):
    """broadcast="workers" already refreshes the arenas: step(broadcast=True) is accepted and leaves
    what step() leaves."""
    from tests.virtual_schedules import run_sharded
    from evolutionarydistributedtraining_amd.collectives import VirtualWorld
    from evolutionarydistributedtraining_amd.distributed import ShardedOuterSync
    tdt, wdt = torch.float32, torch.bfloat16
    layout, theta, gens = population(SHAPES, tdt, wdt, 4, steps=1)
    ref = run_sharded(2, layout, tdt, wdt, theta, gens, "cpu", kernels=OracleKernels(oracle), mode="exact",
                      broadcast="workers", bucket_elems=1024)

    def body(comm):
        s = ShardedOuterSync(layout, tdt, wdt, 2, "cpu", mode="exact", broadcast="workers", bucket_elems=1024,
                             kernels=OracleKernels(oracle), comm=comm)
        s.theta.flat.copy_(theta)
        for j, a in enumerate(s.workers):
            a.flat.copy_(gens[0][comm.rank * 2 + j])
        s.step(broadcast=True)
        assert s.kernel_bytes(broadcast=True) == s.kernel_bytes()
        return [w.flat.clone() for w in s.workers]

    for got, want in zip(VirtualWorld(2).run(body), ref):
        for x, y in zip(got, want["workers"]):
            assert torch.equal(bits(x), bits(y))


@pytest.mark.parametrize("world", [1, 2, 8])
@pytest.mark.parametrize("tdt,wdt", PAIRS)
def test_kernel_bytes_gains_the_refresh(world, tdt, wdt):
    """+ n_pad * K_local * b_w where phase 3 carries the stores; + n_pad * (b_g + K_local * b_w)
    where edt_broadcast_theta reads theta once more; wire_bytes() has no such argument."""
    from evolutionarydistributedtraining_amd.collectives import VirtualWorld
    from evolutionarydistributedtraining_amd.distributed import ShardedOuterSync
    from evolutionarydistributedtraining_amd.params import ParamLayout
    k_local = 8 // world
    bg, bw = torch.empty(0, dtype=tdt).element_size(), torch.empty(0, dtype=wdt).element_size()
    for name, (_, kw) in MODES.items():
        s = ShardedOuterSync(ParamLayout([(5000,), (37,)]), tdt, wdt, k_local, "cpu", kernels=object(),
                             comm=VirtualWorld(world).comm(0), broadcast="theta", **kw)
        extra = s.kernel_bytes(broadcast=True) - s.kernel_bytes()
        fused = "gather" in name
        assert extra == s.n_pad * (k_local * bw + (0 if fused else bg)), name
        assert s.kernel_bytes(broadcast=False) == s.kernel_bytes(), name
    s = ShardedOuterSync(ParamLayout([(5000,)]), tdt, wdt, k_local, "cpu", kernels=object(),
                         comm=VirtualWorld(world).comm(0), mode="reduce_q", wire_format="mxfp4", gather_format="mxfp8")
    assert s.wire_bytes() == int((world - 1) / world * s.n_pad * (QB["mxfp4"] + QB["mxfp8"]))


# ---------------------------------------------------------------------------------------------
# host-side validation of the C ABI (no GPU: every call fails before any HIP call)

@pytest.fixture(scope="module")
def lib():
    if torch.cuda.is_available():
        pytest.skip("host-pointer validation: CPU-only (a device run would launch on host addresses)")
    from evolutionarydistributedtraining_amd import _lib
    return _lib.load_library()


def test_abi_validation_of_the_broadcast_entries(lib):
    # _fake(i): the i-th 64-byte slot of a host array, never dereferenced. With n = 512: theta (fp32)
    # is slots [0, 32), packed (mxfp8, 528 bytes) [34, 42.25), the bf16 destinations [44, 60) and [60, 76)
    far = (_P * 2)(_fake(44), _fake(60))

    def err():
        return lib.edt_last_error().decode()

    def apply(n=512, region=512, fmt=0, gdt=0, wdt=1, theta=_fake(0), packed=_fake(34), bcast=far, nb=2):
        return lib.edt_apply_delta_q_bcast(theta, gdt, packed, n, region, fmt, bcast, wdt, nb, None)

    # edt_apply_delta_q's checks
    assert apply(region=500) < 0 and "multiple of 512" in err()
    assert apply(region=0) < 0 and "multiple of 512" in err()
    assert apply(n=1536, region=1024) < 0 and "whole number of regions" in err()
    assert apply(fmt=2) < 0 and "wire format" in err()
    assert apply(gdt=2) < 0 and "dtype" in err()
    assert apply(theta=None) < 0 and "theta_g is null" in err()
    assert apply(packed=None) < 0 and "packed is null" in err()
    assert apply(theta=_fake(0, 8)) < 0 and "16-byte aligned" in err()
    assert apply(packed=_fake(34, 4)) < 0 and "16-byte aligned" in err()
    # and the broadcast's
    assert apply(gdt=1, wdt=0) < 0 and "dtype pair" in err()
    assert apply(wdt=2) < 0 and "dtype pair" in err()
    assert apply(nb=-1) < 0 and "broadcast count" in err()
    assert apply(nb=65) < 0 and "broadcast count" in err()
    assert apply(bcast=None) < 0 and "bcast is null" in err()
    assert apply(bcast=(_P * 2)(_fake(44), None)) < 0 and "bcast[1] is null" in err()
    assert apply(bcast=(_P * 2)(_fake(44), _fake(60, 8))) < 0 and "16-byte aligned" in err()
    assert apply(theta=_fake(43)) < 0 and "bcast[0] overlaps theta_g" in err()
    assert apply(bcast=(_P * 2)(_fake(44), _fake(31))) < 0 and "bcast[1] overlaps theta_g" in err()
    assert apply(packed=_fake(59)) < 0 and "bcast[0] overlaps packed" in err()
    assert apply(packed=_fake(61)) < 0 and "bcast[1] overlaps packed" in err()
    assert apply(n=0) == 0                                           # nothing to do, nothing launched
    assert apply(n=0, nb=0, bcast=None) == 0
    assert apply(nb=0, region=500) < 0 and "multiple of 512" in err()      # nbcast = 0: the plain entry's checks

    # n = 8: theta is 32 bytes of its slot, a bf16 destination 16 bytes of its own
    dst = (_P * 2)(_fake(2), _fake(3))
    null = (_P * 2)(_fake(2), None)

    def bcast(n=8, gdt=0, wdt=1, theta=_fake(0), out=dst, nb=2):
        return lib.edt_broadcast_theta(theta, gdt, n, out, wdt, nb, None)

    assert bcast(gdt=1, wdt=0) < 0 and "dtype pair" in err()
    assert bcast(gdt=3) < 0 and "dtype pair" in err()
    assert bcast(nb=-1) < 0 and "broadcast count" in err()
    assert bcast(nb=65) < 0 and "broadcast count" in err()
    assert bcast(theta=None) < 0 and "theta_g is null" in err()
    assert bcast(out=None) < 0 and "bcast is null" in err()
    assert bcast(out=null) < 0 and "bcast[1] is null" in err()
    assert bcast(theta=_fake(3)) < 0 and "bcast[1] overlaps theta_g" in err()
    assert bcast(n=64, theta=_fake(1)) < 0 and "bcast[0] overlaps theta_g" in err()      # 256 B of theta reach slot 2
    assert bcast(n=0) == 0 and bcast(nb=0, out=None) == 0 and bcast(n=0, theta=None) == 0
    assert lib.edt_abi_version() == 6
