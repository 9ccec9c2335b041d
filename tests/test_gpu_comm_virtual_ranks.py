"""The C sharded outer-step schedules of csrc/edt_comm.cpp (edt_outer_step_sharded, _ordered, _exact)
and its collectives at world sizes above one, on one GPU.

RCCL refuses two ranks on one device, so the ranks are host threads over
tests/c_abi/_build/libedt_comm_virtual.so: the unmodified edt_comm.cpp linked with an in-process
stand-in for the RCCL calls it makes (tests/c_abi/vrccl.hip), bound through comm.Comm(lib=...).
Each rank has its own torch stream, theta copy, workers, momentum shard and workspaces. Every
assertion on data is bit for bit. Nothing here says anything about real RCCL.
"""
import ctypes
import os
import re
import subprocess
import time

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
C_ABI = os.path.join(ROOT, "tests", "c_abi")
VLIB_PATH = os.path.join(C_ABI, "_build", "libedt_comm_virtual.so")

CONTROL = {"edt_vrccl_set_wait_bound", "edt_vrccl_wait_bound", "edt_vrccl_break_world", "edt_vrccl_live_worlds",
           "edt_vrccl_staged_moves", "edt_vrccl_arrivals", "edt_vrccl_last_error"}
ERR_ARG, ERR_ABORTED = -1, -4
LR, MU = 0.7, 0.9
F32, BF16 = torch.float32, torch.bfloat16


def test_virtual_library_exports_and_dependencies():
    """The library's dynamic symbol table defines include/edt_comm.h's entry points and the
    stand-in's control functions and nothing else (no nccl* name: the process has the real librccl
    mapped through torch), every nccl* call is bound inside it, and librccl is no dependency."""
    from evolutionarydistributedtraining_amd import comm
    subprocess.run(["make", "-s", "-C", C_ABI], check=True)
    defined = subprocess.run(["nm", "-D", "--defined-only", VLIB_PATH], capture_output=True, text=True, check=True).stdout
    names = {ln.split()[-1].split("@")[0] for ln in defined.splitlines() if ln.strip()}
    abi = {n for n, _, _ in comm.SIGNATURES}
    assert names == abi | CONTROL, names ^ (abi | CONTROL)
    assert all(re.match(r"edt_comm_|edt_outer_step_sharded|edt_vrccl_", n) for n in names)
    undefined = subprocess.run(["nm", "-D", "--undefined-only", VLIB_PATH], capture_output=True, text=True,
                               check=True).stdout
    assert "nccl" not in undefined.lower(), undefined
    dyn = subprocess.run(["readelf", "-d", VLIB_PATH], capture_output=True, text=True, check=True).stdout
    needed = re.findall(r"\(NEEDED\).*\[(.+?)\]", dyn)
    assert any(n.startswith("libedt_sync.so") for n in needed) and any(n.startswith("libamdhip64") for n in needed)
    assert not any("rccl" in n or "nccl" in n for n in needed), needed


# ------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def vlib(dev):
    """The virtual library with edt_comm.h's entry points typed, plus the control functions."""
    from evolutionarydistributedtraining_amd.comm import load_comm_library
    lib = load_comm_library(VLIB_PATH)
    lib.edt_vrccl_set_wait_bound.restype, lib.edt_vrccl_set_wait_bound.argtypes = ctypes.c_double, [ctypes.c_double]
    lib.edt_vrccl_wait_bound.restype, lib.edt_vrccl_wait_bound.argtypes = ctypes.c_double, []
    lib.edt_vrccl_break_world.restype, lib.edt_vrccl_break_world.argtypes = ctypes.c_int, [ctypes.c_char_p]
    lib.edt_vrccl_live_worlds.restype, lib.edt_vrccl_live_worlds.argtypes = ctypes.c_int, []
    lib.edt_vrccl_staged_moves.restype, lib.edt_vrccl_staged_moves.argtypes = ctypes.c_ulonglong, []
    lib.edt_vrccl_arrivals.restype, lib.edt_vrccl_arrivals.argtypes = ctypes.c_ulonglong, []
    lib.edt_vrccl_last_error.restype, lib.edt_vrccl_last_error.argtypes = ctypes.c_char_p, []
    assert lib.edt_vrccl_wait_bound() == 30.0
    yield lib
    assert lib.edt_vrccl_live_worlds() == 0


@pytest.fixture(scope="module")
def streams(dev):
    """One caller's stream per rank, so no rank's work is ordered against another's by accident."""
    return [torch.cuda.Stream(device=dev) for _ in range(8)]


def run_world(vlib, streams, dev, world, body, wait=True):
    """body(comm, rank) on `world` rank threads (collectives.VirtualWorld.run), each under its own
    stream, then edt_comm_wait (which must return 0) and close. A rank's exception breaks the
    world, so its peers return at once instead of waiting; the earliest one is re-raised here. The
    inputs were written on the default stream: it is drained first, and the whole device afterwards."""
    from evolutionarydistributedtraining_amd.collectives import VirtualWorld
    from evolutionarydistributedtraining_amd.comm import Comm
    uid = Comm.unique_id(vlib)
    torch.cuda.synchronize()
    errors = []

    def rank_fn(vc):
        c = None
        try:
            c = Comm(uid, world, vc.rank, lib=vlib)
            assert (c.rank, c.size) == (vc.rank, world)
            assert (vlib.edt_comm_rank(c._h), vlib.edt_comm_size(c._h)) == (vc.rank, world)
            with torch.cuda.stream(streams[vc.rank % len(streams)]):
                out = body(c, vc.rank)
                if wait:
                    c.wait(dev, timeout_s=60.0)
            return out
        except BaseException as e:
            errors.append(e)                       # list.append is atomic: in order of failure
            vlib.edt_vrccl_break_world(uid)
            raise
        finally:
            if c is not None:
                c.close()

    try:
        return VirtualWorld(world).run(rank_fn)
    except BaseException:
        if errors:
            raise errors[0]
        raise
    finally:
        torch.cuda.synchronize()


def same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.view(torch.uint8), b.view(torch.uint8))


def rand(gen, n, dtype, dev):
    """Values over ~12 binades, so a sum's bits depend on its order."""
    x = torch.randn(n, generator=gen, device=dev) * torch.exp2(torch.randint(-6, 7, (n,), generator=gen, device=dev).float())
    return x.to(dtype)


def left_fold(parts):
    s = parts[0].clone()
    for p in parts[1:]:
        s = s + p                                  # one fp32 add per rank, ranks in order
    return s


COUNT = 1007        # per rank: odd, four blocks of the fold kernel with a partial last one


# ------------------------------------------------------------------------------------------
# the stand-in against plain tensor indexing
@pytest.mark.gpu
@pytest.mark.parametrize("inplace", [False, True])
@pytest.mark.parametrize("world", [2, 3, 4])
def test_virtual_reduce_scatter(vlib, streams, dev, world, inplace):
    """recv[0, count) = left fold over ranks of send[rank * count, +count), bit for bit; in place
    when recv == send + rank * count (only that slice of send is written)."""
    g = torch.Generator(device=dev).manual_seed(10 + world)
    sends = [rand(g, world * COUNT, F32, dev) for _ in range(world)]
    orig = [s.clone() for s in sends]
    recvs = [s[r * COUNT:(r + 1) * COUNT] if inplace else torch.full((COUNT,), float("nan"), device=dev)
             for r, s in enumerate(sends)]
    want = [left_fold([o[r * COUNT:(r + 1) * COUNT] for o in orig]) for r in range(world)]
    if world > 2:       # the inputs do tell a left fold from a right one
        assert not same_bits(want[0], left_fold([o[:COUNT] for o in reversed(orig)]))
    run_world(vlib, streams, dev, world, lambda c, r: c.reduce_scatter_f32(sends[r], recvs[r]))
    for r in range(world):
        assert same_bits(recvs[r], want[r]), r
        keep = torch.ones(world * COUNT, dtype=torch.bool, device=dev)
        if inplace:
            keep[r * COUNT:(r + 1) * COUNT] = False
        assert same_bits(sends[r][keep], orig[r][keep]), r


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", [F32, BF16])
@pytest.mark.parametrize("inplace", [False, True])
@pytest.mark.parametrize("world", [2, 3, 4])
def test_virtual_all_gather(vlib, streams, dev, world, inplace, dtype):
    """recv[r * count, +count) = rank r's send[0, count); in place when send == recv + rank * count."""
    g = torch.Generator(device=dev).manual_seed(20 + world)
    src = [rand(g, COUNT, dtype, dev) for _ in range(world)]
    recvs = [torch.full((world * COUNT,), float("nan"), dtype=dtype, device=dev) for _ in range(world)]
    sends = []
    for r in range(world):
        if inplace:
            recvs[r][r * COUNT:(r + 1) * COUNT] = src[r]
            sends.append(recvs[r][r * COUNT:(r + 1) * COUNT])
        else:
            sends.append(src[r].clone())
    run_world(vlib, streams, dev, world, lambda c, r: c.all_gather(sends[r], recvs[r]))
    want = torch.cat(src)
    for r in range(world):
        assert same_bits(recvs[r], want), r
        assert same_bits(sends[r], src[r]), r


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", [F32, BF16])
@pytest.mark.parametrize("world", [2, 3, 4])
def test_virtual_all_to_all(vlib, streams, dev, world, dtype):
    """recv[r * count, +count) = rank r's send[this rank * count, +count)."""
    g = torch.Generator(device=dev).manual_seed(30 + world)
    sends = [rand(g, world * COUNT, dtype, dev) for _ in range(world)]
    orig = [s.clone() for s in sends]
    recvs = [torch.full((world * COUNT,), float("nan"), dtype=dtype, device=dev) for _ in range(world)]
    run_world(vlib, streams, dev, world, lambda c, r: c.all_to_all(sends[r], recvs[r]))
    for q in range(world):
        want = torch.cat([orig[r][q * COUNT:(q + 1) * COUNT] for r in range(world)])
        assert same_bits(recvs[q], want), q
        assert same_bits(sends[q], orig[q]), q


@pytest.mark.gpu
def test_virtual_all_to_all_stages_crossing_buffers(vlib, streams, dev):
    """World 2, each rank receiving into the other rank's send buffer: the destinations overlap the
    sources across ranks, so the stand-in goes through its temporary and still gives the exchange."""
    g = torch.Generator(device=dev).manual_seed(39)
    bufs = [rand(g, 2 * COUNT, F32, dev) for _ in range(2)]
    orig = [b.clone() for b in bufs]
    before = vlib.edt_vrccl_staged_moves()
    run_world(vlib, streams, dev, 2, lambda c, r: c.all_to_all(bufs[r], bufs[1 - r]))
    assert vlib.edt_vrccl_staged_moves() > before
    for q in range(2):          # rank q received into bufs[1 - q]
        want = torch.cat([orig[r][q * COUNT:(q + 1) * COUNT] for r in range(2)])
        assert same_bits(bufs[1 - q], want), q


@pytest.mark.gpu
@pytest.mark.parametrize("world", [2, 3, 4])
def test_virtual_exchange(vlib, streams, dev, world):
    """edt_comm_exchange over one pattern: a ring over ranks 0 .. world-2 (at world 2 that ring is
    rank 0's self-send), a self-send on rank 0, the last rank only receiving, and two operations of
    different sizes between the same pair (rank 0 to the last rank), matched in order."""
    g = torch.Generator(device=dev).manual_seed(40 + world)
    last, ring = world - 1, world - 1
    a = [rand(g, 501, BF16, dev) for r in range(ring)]                        # rank r -> rank (r + 1) % ring
    b = [torch.zeros(501, dtype=BF16, device=dev) for r in range(ring)]
    self_src, self_dst = rand(g, 333, F32, dev), torch.zeros(333, device=dev)
    x1, x2 = rand(g, 100, F32, dev), rand(g, 37, F32, dev)
    y1, y2 = torch.zeros(100, device=dev), torch.zeros(37, device=dev)

    def body(c, r):
        ops = []
        if r < ring:
            ops.append(((r + 1) % ring, a[r], (r - 1) % ring, b[r]))
        if r == 0:
            ops += [(0, self_src, 0, self_dst), (last, x1, -1, None), (last, x2, -1, None)]
        if r == last:
            ops += [(-1, None, 0, y1), (-1, None, 0, y2)]
        c.exchange(ops)

    run_world(vlib, streams, dev, world, body)
    for r in range(ring):
        assert same_bits(b[r], a[(r - 1) % ring]), r
    assert same_bits(self_dst, self_src)
    assert same_bits(y1, x1) and same_bits(y2, x2)


@pytest.mark.gpu
def test_virtual_refuses_unmatched_and_duplicate(vlib, streams, dev):
    """A receive with no matching send, a send with no matching receive and a rank joining twice
    are errors on every rank, at once (no wait runs out)."""
    from evolutionarydistributedtraining_amd import _lib as L
    from evolutionarydistributedtraining_amd.collectives import VirtualWorld
    from evolutionarydistributedtraining_amd.comm import Comm
    s, t = torch.ones(8, device=dev), torch.zeros(8, device=dev)
    t0 = time.monotonic()
    for ops0, match in (([(-1, None, 1, t)], "sends it nothing"), ([(1, s, -1, None)], "does not receive it")):
        def body(c, r, ops0=ops0):
            c.exchange(ops0 if r == 0 else [(1, s, 1, t)])     # rank 1 takes part with a self-send only

        with pytest.raises(L.EdtError, match=match):
            run_world(vlib, streams, dev, 2, body)
    uid = Comm.unique_id(vlib)
    with pytest.raises(L.EdtError, match="joined twice"):
        VirtualWorld(2).run(lambda vc: Comm(uid, 2, 0, lib=vlib).close())
    assert time.monotonic() - t0 < vlib.edt_vrccl_wait_bound()


# ------------------------------------------------------------------------------------------
# the three schedules against the single-GPU kernels and the oracle
def buckets_of(world, n_pad, bucket_elems):
    """[b, e) per bucket as include/edt_comm.h states it: bucket_elems rounded down to a multiple of
    world x 64, at least one such unit, at most n_pad."""
    unit = world * 64
    bucket = min(max(bucket_elems // unit * unit, unit), n_pad)
    return [(b, min(b + bucket, n_pad)) for b in range(0, n_pad, bucket)]


def bucket_sizes(world):
    return [world * 640, world * 640 + 63, 1, 1 << 26]


_population_cache, _reference_cache = {}, {}


def population(dev, world, k_local, gdt, wdt):
    """theta and the K_total workers (global worker k = rank * K_local + j), zero in the pad."""
    key = (world, k_local, gdt, wdt)
    if key not in _population_cache:
        n_pad = world * 64 * 37
        n = n_pad - 29
        g = torch.Generator(device=dev).manual_seed(1000 * world + k_local)
        theta = torch.zeros(n_pad, dtype=gdt, device=dev)
        theta[:n] = (torch.randn(n, generator=g, device=dev) * 0.02).to(gdt)
        workers = []
        for _ in range(world * k_local):
            w = torch.zeros(n_pad, dtype=wdt, device=dev)
            w[:n] = (theta[:n].float() + torch.randn(n, generator=g, device=dev) * 1e-3).to(wdt)
            workers.append(w)
        _population_cache[key] = (n, n_pad, theta, workers)
    return _population_cache[key]


def reference(oracle, dev, schedule, world, k_local, gdt, wdt, mu, nesterov):
    """Three steps (has_momentum False, True, True) of what the schedule must equal, computed once
    per configuration and left unchanged: the same for every bucket size.
      exact    ops.outer_step over all K_total workers on the whole padded arena, itself equal to
               oracle.outer_step on the CPU
      ordered  per-rank ops.delta_partial (k_total = K_total), ops.sgd_apply_sum in rank order
      reduce   per-rank ops.delta_partial, the stand-in's left fold formed with torch fp32 adds,
               ops.sgd_apply"""
    from evolutionarydistributedtraining_amd import ops
    key = (schedule, world, k_local, gdt, wdt, mu, nesterov)
    if key not in _reference_cache:
        n, n_pad, theta0, workers = population(dev, world, k_local, gdt, wdt)
        th = theta0.clone()
        mom = torch.zeros(n_pad, dtype=gdt, device=dev) if mu != 0 else None
        for has in (False, True, True):
            if schedule == "exact":
                ops.outer_step(th, workers, mom, has, LR, mu, nesterov)
                continue
            parts = [torch.full((n_pad,), float("nan"), device=dev) for _ in range(world)]
            for r in range(world):
                ops.delta_partial(th, workers[r * k_local:(r + 1) * k_local], world * k_local, parts[r])
            if schedule == "ordered":
                ops.sgd_apply_sum(th, parts, mom, has, LR, mu, nesterov)
            else:
                ops.sgd_apply(th, left_fold(parts), mom, has, LR, mu, nesterov)
        torch.cuda.synchronize()
        if schedule == "exact":
            cth, cmom = theta0.cpu(), (torch.zeros(n_pad, dtype=gdt) if mu != 0 else None)
            cw = [w.cpu() for w in workers]
            for has in (False, True, True):
                oracle.outer_step(cth, cw, cmom, has, LR, mu, nesterov)
            assert same_bits(th.cpu(), cth)
            assert mom is None or same_bits(mom.cpu(), cmom)
        assert not same_bits(th, theta0)
        _reference_cache[key] = (th, mom)
    return _reference_cache[key]


def run_schedule(vlib, streams, dev, schedule, world, k_local, gdt, wdt, bucket_elems, mu=MU, nesterov=True):
    """Three steps of one schedule on `world` ranks from the population's inputs: theta per rank
    and the momentum put together again from the ranks' shards (buckets in order, each rank's shard
    the run of its per-element pieces). Workspaces start as NaN; nothing is written behind a shard."""
    n, n_pad, theta0, workers = population(dev, world, k_local, gdt, wdt)
    thetas = [theta0.clone() for _ in range(world)]
    local = [[workers[r * k_local + j].clone() for j in range(k_local)] for r in range(world)]
    # each momentum shard is the head of a NaN-filled buffer: a step that runs past its shard shows
    guards = [torch.full((n_pad,), float("nan"), dtype=gdt, device=dev) for _ in range(world)]
    shards = [None] * world
    if mu != 0:
        shards = [g[:n_pad // world] for g in guards]
        for sh in shards:
            sh.zero_()
    acc = [torch.full((n_pad,), float("nan"), device=dev) for _ in range(world)]
    recv = [torch.full((n_pad,), float("nan"), device=dev) for _ in range(world)]
    recv_w = [[torch.full((n_pad,), float("nan"), dtype=wdt, device=dev) for _ in range(k_local)] for _ in range(world)]

    def body(c, r):
        for has in (False, True, True):
            if schedule == "exact":
                c.outer_step_sharded_exact(thetas[r], local[r], shards[r], has, LR, mu, nesterov, recv_w[r],
                                           bucket_elems=bucket_elems)
            elif schedule == "ordered":
                c.outer_step_sharded_ordered(thetas[r], local[r], shards[r], has, LR, mu, nesterov, acc[r], recv[r],
                                             bucket_elems=bucket_elems)
            else:
                c.outer_step_sharded(thetas[r], local[r], shards[r], has, LR, mu, nesterov, acc[r],
                                     bucket_elems=bucket_elems)

    run_world(vlib, streams, dev, world, body)
    for r in range(world):          # the workers are inputs only
        for j in range(k_local):
            assert same_bits(local[r][j], workers[r * k_local + j]), (r, j)
    for r in range(world):
        assert torch.isnan(guards[r][n_pad // world if mu != 0 else 0:]).all(), f"rank {r} wrote past its momentum shard"
    if mu == 0:
        return thetas, None
    mom = torch.full((n_pad,), float("nan"), dtype=gdt, device=dev)
    off = 0
    for b, e in buckets_of(world, n_pad, bucket_elems):
        per = (e - b) // world
        for r in range(world):
            mom[b + r * per:b + (r + 1) * per] = shards[r][off:off + per]
        off += per
    assert off == n_pad // world
    return thetas, mom


def check_schedule(vlib, streams, dev, oracle, schedule, world, k_local, gdt, wdt, bucket_elems, mu=MU, nesterov=True):
    n, n_pad, _, _ = population(dev, world, k_local, gdt, wdt)
    ref_t, ref_m = reference(oracle, dev, schedule, world, k_local, gdt, wdt, mu, nesterov)
    first = run_schedule(vlib, streams, dev, schedule, world, k_local, gdt, wdt, bucket_elems, mu, nesterov)
    again = run_schedule(vlib, streams, dev, schedule, world, k_local, gdt, wdt, bucket_elems, mu, nesterov)
    for thetas, mom in (first, again):
        for r in range(world):
            assert same_bits(thetas[r], ref_t), f"theta of rank {r}"
            assert not thetas[r][n:].any(), f"pad of rank {r}"
        assert (mom is None and ref_m is None) or same_bits(mom, ref_m), "momentum"
    for r in range(world):          # the same case twice gives the same bits (a race would differ)
        assert same_bits(first[0][r], again[0][r])
    assert first[1] is None or same_bits(first[1], again[1])


def _bucket_layouts():
    """The four bucket sizes at world 3 give: 3 full buckets + a ragged one of 7 units, the same,
    37 buckets of one unit, one bucket."""
    n_pad = 3 * 64 * 37
    got = [buckets_of(3, n_pad, be) for be in bucket_sizes(3)]
    assert [len(x) for x in got] == [4, 4, 37, 1] and got[0] == got[1]
    assert [e - b for b, e in got[0]] == [1920, 1920, 1920, 7 * 192]


_bucket_layouts()

DTYPE_PAIRS = [(F32, F32), (F32, BF16), (BF16, BF16)]
SCHEDULES = ["reduce", "ordered", "exact"]
CASES = [(w, k, b) for w, k in ((2, 1), (2, 3), (3, 2)) for b in range(4)] + [(4, 2, 0), (8, 1, 0)]


def _dt_id(p):
    return "-".join("f32" if d == F32 else "bf16" for d in p)


@pytest.mark.gpu
@pytest.mark.parametrize("schedule", SCHEDULES)
@pytest.mark.parametrize("dtypes", DTYPE_PAIRS, ids=_dt_id)
@pytest.mark.parametrize("world,k_local,bucket", CASES, ids=lambda v: str(v))
def test_c_schedule_virtual_ranks(vlib, streams, dev, oracle, world, k_local, bucket, dtypes, schedule):
    """Three Nesterov steps (lr 0.7, mu 0.9; has_momentum False, True, True) of each C schedule
    over `world` ranks and every bucket layout equal its reference bit for bit: theta on every
    rank, the momentum reassembled from the shards, a zero pad, the same bits on a second run."""
    check_schedule(vlib, streams, dev, oracle, schedule, world, k_local, *dtypes, bucket_sizes(world)[bucket])


@pytest.mark.gpu
@pytest.mark.parametrize("schedule", SCHEDULES)
@pytest.mark.parametrize("mu,nesterov", [(MU, False), (0.0, False)], ids=["plain-momentum", "mu0-null-shard"])
def test_c_schedule_virtual_ranks_scalars(vlib, streams, dev, oracle, schedule, mu, nesterov):
    """Without Nesterov, and with mu = 0 and a null momentum shard (world 3, K_local 2, ragged buckets)."""
    check_schedule(vlib, streams, dev, oracle, schedule, 3, 2, F32, BF16, bucket_sizes(3)[0], mu, nesterov)


# ------------------------------------------------------------------------------------------
# limits and refusals at world sizes above one
@pytest.mark.gpu
def test_c_exact_schedule_64_workers(vlib, streams, dev, oracle):
    """K_local x nranks == 64 (8 x 8), the most the fused step takes: equal to it."""
    check_schedule(vlib, streams, dev, oracle, "exact", 8, 8, F32, BF16, bucket_sizes(8)[0])


def refused(vlib, streams, dev, world, call):
    """call(comm, rank, theta) must fail with EDT_COMM_ERR_ARG on every rank, before any collective
    (no rank enters a rendezvous) and with theta untouched; returns the messages."""
    from evolutionarydistributedtraining_amd import _lib as L
    n_pad = call.n_pad
    g = torch.Generator(device=dev).manual_seed(77)
    theta0 = torch.randn(n_pad, generator=g, device=dev) * 0.02
    thetas = [theta0.clone() for _ in range(world)]
    before = vlib.edt_vrccl_arrivals()

    def body(c, r):
        with pytest.raises(L.EdtError) as ei:
            call(c, r, thetas[r])
        assert f"({ERR_ARG})" in str(ei.value), str(ei.value)
        return str(ei.value)

    msgs = run_world(vlib, streams, dev, world, body)
    assert vlib.edt_vrccl_arrivals() == before
    for r in range(world):
        assert same_bits(thetas[r], theta0), r
    return msgs


def _step_call(dev, schedule, n_pad, k_local, alias_recv=False):
    ws = [torch.zeros(n_pad, device=dev) for _ in range(k_local)]
    mom, acc, recv = torch.zeros(n_pad, device=dev), torch.zeros(n_pad, device=dev), torch.zeros(n_pad, device=dev)

    def call(c, r, theta):
        if schedule == "exact":
            c.outer_step_sharded_exact(theta, ws, mom, False, LR, MU, True, ws)
        elif schedule == "ordered":
            c.outer_step_sharded_ordered(theta, ws, mom, False, LR, MU, True, acc, acc if alias_recv else recv)
        else:
            c.outer_step_sharded(theta, ws, mom, False, LR, MU, True, acc)

    call.n_pad = n_pad
    return call


@pytest.mark.gpu
def test_c_exact_schedule_refuses_65_workers(vlib, streams, dev):
    """K_local x nranks == 65 (world 5 x 13) is refused on every rank before any collective."""
    msgs = refused(vlib, streams, dev, 5, _step_call(dev, "exact", 5 * 64 * 2, 13))
    assert all("at most 64 workers" in m for m in msgs), msgs


@pytest.mark.gpu
@pytest.mark.parametrize("schedule", SCHEDULES)
def test_c_schedule_refuses_bad_n_pad(vlib, streams, dev, schedule):
    """World 3, n_pad a multiple of 64 but not of 3 x 64: refused on every rank before any collective."""
    msgs = refused(vlib, streams, dev, 3, _step_call(dev, schedule, 64 * 4, 2))
    assert all("not a multiple of nranks x 64" in m for m in msgs), msgs


@pytest.mark.gpu
def test_c_ordered_schedule_refuses_recv_aliasing_acc(vlib, streams, dev):
    msgs = refused(vlib, streams, dev, 2, _step_call(dev, "ordered", 2 * 64 * 3, 2, alias_recv=True))
    assert all("alias" in m for m in msgs), msgs


@pytest.mark.gpu
def test_c_abort_world2(vlib, streams, dev):
    """Rank 1 aborts before the step. With the stand-in's bound at 2 s, rank 0's step returns a
    negative code with a message within that bound (it never waits the bound out: the abort breaks
    the world), rank 1's later calls return EDT_COMM_ERR_ABORTED, both handles close (run_world
    closes them) and the device is sound afterwards."""
    from evolutionarydistributedtraining_amd import _lib as L
    n_pad = 2 * 64 * 5
    g = torch.Generator(device=dev).manual_seed(5)
    theta0 = torch.randn(n_pad, generator=g, device=dev) * 0.02
    thetas = [theta0.clone() for _ in range(2)]
    ws = [[theta0 + 1e-3 for _ in range(2)] for _ in range(2)]
    moms = [torch.zeros(n_pad // 2, device=dev) for _ in range(2)]
    accs = [torch.zeros(n_pad, device=dev) for _ in range(2)]

    def step(c, r):
        return vlib.edt_outer_step_sharded(c._h, L.ptr(thetas[r]), 0, L.ptr_array(ws[r]), 0, 2, L.ptr(moms[r]), 0, n_pad,
                                           1 << 26, LR, MU, 1, L.ptr(accs[r]), L.stream_ptr(dev))

    def body(c, r):
        if r == 1:
            c.abort()
            assert step(c, r) == ERR_ABORTED and b"aborted" in vlib.edt_comm_last_error()
            assert vlib.edt_comm_poll(c._h) == ERR_ABORTED
            assert vlib.edt_comm_reduce_scatter_f32(c._h, L.ptr(accs[r]), L.ptr(accs[r]), n_pad // 2,
                                                    L.stream_ptr(dev)) == ERR_ABORTED
            return None
        t0 = time.monotonic()
        rc = step(c, r)
        return rc, vlib.edt_comm_last_error().decode(), time.monotonic() - t0

    old = vlib.edt_vrccl_set_wait_bound(2.0)
    try:
        assert old == 30.0
        rc, msg, took = run_world(vlib, streams, dev, 2, body, wait=False)[0]
    finally:
        vlib.edt_vrccl_set_wait_bound(old)
    assert rc < 0 and "rank 1 aborted" in msg, (rc, msg)
    assert took < 2.0, took
    for r in range(2):          # the owned shard is stepped only after the reduce-scatter, which never ran
        assert same_bits(thetas[r], theta0), r
    assert same_bits(theta0 + 0.0, theta0)      # the device still computes
