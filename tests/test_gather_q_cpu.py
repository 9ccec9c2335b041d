"""The quantized gather of the reduce_q schedule without a GPU: the host-side validation of the two
new C-ABI entries (edt_sgd_delta_sum_q, edt_apply_delta_q), the schedule of ShardedOuterSync with
gather_format on virtual ranks through the kernels= seam (tests/gather_q_reference.py on top of
tests/quant_reference.py), and the option handling. The reference has no wire format (its workers
exchange checkpoints on disk, EDT_LM/diloco.py:231-235, 302-308); the GPU form is
tests/test_gpu_gather_q.py."""
import ctypes

import numpy as np
import pytest
import torch

from tests import gather_q_reference as G
from tests import quant_reference as Q
from tests.virtual_schedules import bits, population

QB = {"mxfp8": 1 + 1 / 32, "mxfp4": 1 / 2 + 1 / 32}


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


def _fake(i, skew=0):
    return _P(ctypes.addressof(_host) // 64 * 64 + 64 * (i + 1) + skew)     # never dereferenced


def test_abi_validation_of_the_gather_entries(lib):
    regs = (_P * 2)(_fake(1), _fake(2))
    odd = (_P * 2)(_fake(1), _fake(2, 8))
    null = (_P * 2)(_fake(1), None)

    def err():
        return lib.edt_last_error().decode()

    def delta(n=512, fin=0, fout=0, nacc=2, gdt=0, theta=_fake(0), regions=regs, mom=_fake(3), res=_fake(4),
              out=_fake(5), mu=0.9):
        return lib.edt_sgd_delta_sum_q(theta, gdt, regions, nacc, fin, mom, 1, n, 0.7, mu, 1, res, out, fout, None)

    assert delta(fin=2) < 0 and "wire format" in err()
    assert delta(fout=-1) < 0 and "wire format" in err()
    assert delta(fin=1, fout=7) < 0 and "wire format 7" in err()
    assert delta(nacc=0) < 0 and "partial count" in err()
    assert delta(nacc=65) < 0 and "partial count" in err()
    assert delta(n=500) < 0 and "multiple of 512" in err()
    assert delta(gdt=3) < 0 and "dtype" in err()
    assert delta(theta=None) < 0 and "null" in err()
    assert delta(regions=None) < 0 and "null" in err()
    assert delta(regions=null) < 0 and "regions[1] is null" in err()
    assert delta(out=None) < 0 and "packed_out is null" in err()
    assert delta(mom=None) < 0 and "momentum buffer is null" in err()
    for kw in ({"theta": _fake(0, 8)}, {"regions": odd}, {"mom": _fake(3, 4)}, {"res": _fake(4, 8)}, {"out": _fake(5, 8)}):
        assert delta(**kw) < 0 and "16-byte aligned" in err(), kw
    assert delta(n=0) == 0                                           # nothing to do, nothing launched

    def apply(n=1024, region=512, fmt=0, gdt=0, theta=_fake(0), packed=_fake(1)):
        return lib.edt_apply_delta_q(theta, gdt, packed, n, region, fmt, None)

    assert apply(region=500) < 0 and "multiple of 512" in err()
    assert apply(region=0) < 0 and "multiple of 512" in err()
    assert apply(n=1536, region=1024) < 0 and "whole number of regions" in err()
    assert apply(fmt=2) < 0 and "wire format" in err()
    assert apply(gdt=2) < 0 and "dtype" in err()
    assert apply(theta=None) < 0 and "null" in err()
    assert apply(packed=None) < 0 and "null" in err()
    assert apply(theta=_fake(0, 8)) < 0 and "16-byte aligned" in err()
    assert apply(packed=_fake(1, 4)) < 0 and "16-byte aligned" in err()
    assert apply(n=0) == 0
    assert lib.edt_abi_version() == 6


# ---------------------------------------------------------------------------------------------
# the schedule through the kernels= seam, on CPU tensors

SHAPES = [(37, 11), (5,), (1,), (64, 33), (129,), (300,), (7, 401)]


def _owner_layout(buckets, world, n_pad):
    """For the sharded state (momentum, residual_g): per rank the arena indices of its shards in
    bucket order — the order they lie in mom_shard / residual_g."""
    idx = [[] for _ in range(world)]
    for b, e in buckets:
        per = (e - b) // world
        for r in range(world):
            idx[r].append(np.arange(b + r * per, b + (r + 1) * per))
    return [np.concatenate(i) for i in idx]


def _hand_reference(oracle, theta0, gens, world, n_pad, fmt_in, fmt_out, ef, lr=0.7, mu=0.9, nesterov=True):
    """reduce_q with the quantized gather composed by hand over the whole padded arena, with no
    buckets, regions or packing: per rank the oracle's fp32 partial, Q/D with the rank's residual,
    the D's summed in rank order, the oracle's SGD on a copy of theta; then the update over the
    whole arena, Q/D with the owners' residual (one array: every element has one owner), and
    theta + D rounded. Blocks of 32 start at multiples of 32 of the arena either way."""
    n = theta0.numel()
    th = torch.zeros(n_pad, dtype=theta0.dtype)
    th[:n] = theta0
    mom = torch.zeros_like(th)
    res = [np.zeros(n_pad, dtype=np.float32) if ef else None for _ in range(world)]
    res_g = np.zeros(n_pad, dtype=np.float32) if ef else None
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
            _, _, d, res[r] = Q.ef_step(acc.numpy(), res[r], fmt_in)
            d = torch.from_numpy(d)
            total = d if total is None else total.add_(d)
        new = th.clone()
        oracle.sgd_apply(new, total, mom, i > 0, lr, mu, nesterov)
        _, _, d, res_g = G.delta_step(th, new, res_g, fmt_out)
        th = G.apply_delta(th, d)
    return th, mom, res, res_g


def _run(world, layout, tdt, wdt, theta0, gens, kernels, fmt_in, fmt_out, ef, bucket_elems):
    from evolutionarydistributedtraining_amd.collectives import VirtualWorld
    from evolutionarydistributedtraining_amd.distributed import ShardedOuterSync
    k_local = len(gens[0]) // world

    def body(comm):
        s = ShardedOuterSync(layout, tdt, wdt, k_local, theta0.device, mode="reduce_q", wire_format=fmt_in,
                             error_feedback=ef, bucket_elems=bucket_elems, kernels=kernels, comm=comm,
                             gather_format=fmt_out)
        s.theta.flat.copy_(theta0)
        for ws in gens:
            for j, a in enumerate(s.workers):
                a.flat.copy_(ws[comm.rank * k_local + j])
            s.step()
        return {"theta": s.theta_buf.clone(), "mom": s.mom_shard.clone(),
                "residual": None if s.residual is None else s.residual.clone(),
                "residual_g": None if s.residual_g is None else s.residual_g.clone(), "buckets": s.buckets,
                "n_pad": s.n_pad, "wire": s.wire_bytes(), "mode": (s.mode, s.broadcast),
                "kernel_bytes": s.kernel_bytes(), "u_recv": s.u_recv.numel()}

    return VirtualWorld(world).run(body)


@pytest.mark.parametrize("world", [2, 3])
@pytest.mark.parametrize("fmt_in,fmt_out", [("mxfp8", "mxfp8"), ("mxfp4", "mxfp8"), ("mxfp8", "mxfp4")])
@pytest.mark.parametrize("tdt,wdt", [(torch.float32, torch.bfloat16), (torch.bfloat16, torch.bfloat16)])
def test_gather_q_schedule_through_the_kernels_seam(oracle, world, fmt_in, fmt_out, tdt, wdt):
    layout, theta, gens = population(SHAPES, tdt, wdt, 6, steps=3)
    res = _run(world, layout, tdt, wdt, theta, gens, G.NumpyGatherKernels(oracle), fmt_in, fmt_out, True,
               bucket_elems=world * 512)
    n_pad, buckets = res[0]["n_pad"], res[0]["buckets"]
    assert len(buckets) >= 3 and n_pad > layout.total and n_pad % (world * 512) == 0
    assert res[0]["mode"] == ("reduce_q", "theta")
    for r in res:
        assert torch.equal(bits(r["theta"]), bits(res[0]["theta"]))
    th, mom_ref, resid, resid_g = _hand_reference(oracle, theta, gens, world, n_pad, fmt_in, fmt_out, True)
    assert torch.equal(bits(res[0]["theta"]), bits(th))
    assert not torch.equal(bits(th[:layout.total]), bits(theta))
    own = _owner_layout(buckets, world, n_pad)
    for r in range(world):
        assert torch.equal(bits(res[r]["mom"]), bits(mom_ref[torch.from_numpy(own[r])])), r
        assert np.array_equal(res[r]["residual"].numpy().view(np.int32), resid[r].view(np.int32)), r
        assert np.array_equal(res[r]["residual_g"].numpy().view(np.int32), resid_g[own[r]].view(np.int32)), r
        assert np.abs(resid[r]).max() > 0
    assert np.abs(resid_g).max() > 0
    bg, wb = theta.element_size(), gens[0][0].element_size()
    qi, qo = QB[fmt_in], QB[fmt_out]
    assert res[0]["wire"] == int((world - 1) / world * n_pad * (qi + qo))
    assert res[0]["u_recv"] == int(n_pad * qo)
    shard, k_local = n_pad // world, 6 // world
    # phase 1: theta, the workers and the residual read, the residual and N regions written;
    # phase 2': theta, the momentum, N regions and the residual read, the momentum, the residual and
    # one region written; phase 3: theta read and written, N regions read
    want = (n_pad * (k_local * wb + bg + 8 + qi)
            + shard * (bg + 2 * bg + 8 + world * qi + qo)
            + n_pad * (2 * bg + qo))
    assert res[0]["kernel_bytes"] == int(want)


def test_gather_format_is_opt_in_and_everything_else_is_unchanged():
    from evolutionarydistributedtraining_amd.collectives import VirtualWorld
    from evolutionarydistributedtraining_amd.distributed import ShardedOuterSync
    from evolutionarydistributedtraining_amd.params import ParamLayout
    layout = ParamLayout([(1000,)])
    comm = VirtualWorld(2).comm(0)

    def make(**kw):
        return ShardedOuterSync(layout, torch.float32, torch.bfloat16, 4, "cpu", kernels=object(), comm=comm, **kw)

    for mode in ("reduce", "reduce_ordered", "exact", "auto"):
        with pytest.raises(ValueError):
            make(mode=mode, gather_format="mxfp8")
    for bad in ("int8", "fp8", ""):
        with pytest.raises(ValueError):
            make(mode="reduce_q", gather_format=bad)
    # auto picks what it picks today (the module docstring's table at K = 8)
    want = {(torch.bfloat16, 2): ("reduce_ordered", "theta"), (torch.bfloat16, 4): ("exact", "workers"),
            (torch.bfloat16, 8): ("exact", "workers"), (torch.float32, 2): ("reduce_ordered", "theta"),
            (torch.float32, 4): ("reduce_ordered", "theta"), (torch.float32, 8): ("exact", "workers")}
    for (wdt, world), expect in want.items():
        s = ShardedOuterSync(layout, torch.float32, wdt, 8 // world, "cpu", kernels=object(),
                             comm=VirtualWorld(world).comm(0))
        assert (s.mode, s.broadcast) == expect, (wdt, world)
        assert not hasattr(s, "u_recv") and not hasattr(s, "residual_g")
    s = make(mode="reduce_q")
    assert not hasattr(s, "u_recv") and not hasattr(s, "residual_g") and s.gather_format is None
    assert s.wire_bytes() == int(0.5 * 1024 * (QB["mxfp8"] + 4))
    s = make(mode="reduce_q", wire_format="mxfp4", gather_format="mxfp8")
    assert (s.mode, s.broadcast, s.n_pad) == ("reduce_q", "theta", 1024)
    assert s.u_recv.dtype == torch.uint8 and s.u_recv.numel() == 1024 + 32 and s.q_send.numel() == 512 + 32
    assert s.residual_g.dtype == torch.float32 and s.residual_g.numel() == s.mom_shard.numel() == 512
    assert s.wire_bytes() == int(0.5 * 1024 * (QB["mxfp4"] + QB["mxfp8"]))
    s = make(mode="reduce_q", gather_format="mxfp4", error_feedback=False)
    assert s.residual is None and s.residual_g is None and s.u_recv.numel() == 512 + 32
    s = make(mode="reduce_q", gather_format="mxfp8", momentum=0.0, nesterov=False)
    assert s.mom_shard is None and s.residual_g.numel() == 512
