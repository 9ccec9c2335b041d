"""ShardedFragmentSync without a GPU: FragmentPlan.pieces, the schedule on virtual ranks (and gloo)
through the kernels= seam with the oracle stand-ins (tests/fragment_shard_reference.py), the
checkpoint bridge, every refusal, and the host-side validation of the three piece-list ABI entries.
The GPU form, with the HIP kernels, is tests/test_gpu_sharded_fragment.py."""
import ctypes
import os
import random

import pytest
import torch

from evolutionarydistributedtraining_amd import EdtError, FragmentPlan, OuterState, ShardedFragmentSync
from evolutionarydistributedtraining_amd.collectives import VirtualWorld
from tests import fragment_shard_reference as R
from tests.fragment_shard_reference import bits

_P = ctypes.c_void_p
_U64 = ctypes.c_uint64


# ---------------------------------------------------------------------------------------------
# fragment space

@pytest.mark.parametrize("name", ["strided", "explicit"])
def test_pieces_tile_the_range_and_map_like_snapshot_views(name):
    lay = R.layout()
    plan = R.plans(lay)[name]
    rng = random.Random(3)
    arena = torch.arange(lay.total)
    for p in range(len(plan)):
        F = plan.numel(p)
        snap = torch.cat(plan.views(p, arena))                   # fragment space -> arena element
        assert torch.equal(torch.cat(plan.snapshot_views(p, snap)), snap)
        ranges = [(0, F), (0, F + 200), (F, F + 64), (F + 1, F + 2), (3, 3)]
        ranges += [tuple(sorted((rng.randrange(F + 130), rng.randrange(F + 130)))) for _ in range(200)]
        for lo, hi in ranges:
            pc = plan.pieces(p, lo, hi)
            at = lo
            for a, f, n in pc:
                assert n > 0 and f == at, (p, lo, hi)            # in order, no gap, no empty piece
                assert torch.equal(arena[a:a + n], snap[f:f + n]), (p, lo, hi)
                at += n
            assert at == max(lo, min(hi, F)), (p, lo, hi)        # exactly [lo, min(hi, F)): none beyond F
            # cut only at the range's bounds and at run ends
            assert len(pc) <= len(plan.runs(p))
    assert plan.pieces(0, 0, 0) == []


# ---------------------------------------------------------------------------------------------
# the schedule on virtual ranks

def _maker(lay, plan, tdt, wdt, k_local, oracle, bucket, mu=0.9, nesterov=True, made=None):
    def make(comm):
        s = ShardedFragmentSync(lay, plan, tdt, wdt, k_local, "cpu", 0.7, mu, nesterov, bucket_elems=bucket,
                                kernels=R.PieceOracleKernels(oracle), comm=comm)
        if made is not None:
            made[comm.rank] = s
        return s
    return make


@pytest.mark.parametrize("world", [2, 3])
@pytest.mark.parametrize("name", ["strided", "explicit"])
@pytest.mark.parametrize("tdt,wdt", R.REGIMES)
def test_schedule_equals_the_composition(oracle, world, name, tdt, wdt):
    """Two round robins (mix 0.5 and 1.0, with and without snapshots): R.drive checks theta, the
    gathered momentum and every worker against the one-process composition after every step on
    every rank, and the canaries outside the fragment. K_total 4 at world 2, 3 (true division) at 3."""
    lay = R.layout()
    plan = R.plans(lay)[name]
    k_local = 2 if world == 2 else 1
    theta, workers = R.population(lay, tdt, wdt, k_local * world)
    syncs, ref = R.drive(VirtualWorld(world), _maker(lay, plan, tdt, wdt, k_local, oracle, R.bucket_elems(world, name)),
                         plan, theta, workers, R.OracleArith(oracle))
    assert max(len(b) for b in syncs[0].buckets) >= 3
    assert any(fp > plan.numel(p) for p, fp in enumerate(syncs[0].f_pad))            # pad elements exist
    for r, s in enumerate(syncs):
        assert torch.equal(bits(s.theta.flat), bits(syncs[0].theta.flat))             # replicas identical
        assert s.fragment_has_momentum == [True] * len(plan) and s.fragment_steps == [2] * len(plan)
        assert s.steps == 2 * len(plan)
        for p in range(len(plan)):                  # the momentum's pad elements are never written
            for _, _, s0, s1, off in s._owned(p):
                pad = max(0, s1 - max(s0, plan.numel(p)))
                assert pad == 0 or not s.mom[p][off + (s1 - s0) - pad:off + (s1 - s0)].any()


def test_without_momentum_and_without_merge(oracle):
    lay = R.layout()
    plan = R.plans(lay)["explicit"]
    tdt, wdt = torch.float32, torch.bfloat16
    theta, workers = R.population(lay, tdt, wdt, 4)
    syncs, _ = R.drive(VirtualWorld(2), _maker(lay, plan, tdt, wdt, 2, oracle, 384, mu=0.0, nesterov=False), plan,
                       theta, workers, R.OracleArith(oracle), mu=0.0, nesterov=False)
    assert syncs[0].mom is None and syncs[0].fragment_has_momentum == [False] * len(plan)

    def body(comm):
        s = _maker(lay, plan, tdt, wdt, 2, oracle, 384)(comm)
        s.theta.flat.copy_(theta)
        for a, w in zip(s.workers, workers[comm.rank * 2:]):
            a.flat.copy_(w)
        before = [a.flat.clone() for a in s.workers]
        s.step_fragment(1, 0.5, merge=False)
        assert all(torch.equal(bits(a.flat), bits(b)) for a, b in zip(s.workers, before))
        return s.theta.flat.clone()

    got = VirtualWorld(2).run(body)
    ref = R.ShardRun(plan, theta, [workers[:2], workers[2:]], R.OracleArith(oracle), 0.7, 0.9, True)
    ref.step(1, 0.5, merge=False)
    assert torch.equal(bits(got[0]), bits(ref.theta)) and torch.equal(bits(got[1]), bits(ref.theta))


def test_checkpoint_bridge_continues_bit_for_bit(oracle, tmp_path):
    """gather_state -> OuterState.save -> load -> load_state on a fresh sync: the next steps equal an
    uninterrupted run's; a partly stepped state saves only whole fragments' buffers."""
    lay = R.layout()
    plan = R.plans(lay)["explicit"]
    tdt, wdt, world, k_local = torch.float32, torch.bfloat16, 2, 2
    theta, workers = R.population(lay, tdt, wdt, 4)
    first, rest = [(0, 0.5, False), (2, 1.0, False)], [(1, 0.5, False), (0, 0.5, False), (2, 0.5, False)]
    path = str(tmp_path / "outer_optim.pt")
    make = _maker(lay, plan, tdt, wdt, k_local, oracle, 384)

    def load(s, comm):
        s.theta.flat.copy_(theta)
        for a, w in zip(s.workers, workers[comm.rank * k_local:]):
            a.flat.copy_(w)

    def run(s, steps):
        for p, mix, _ in steps:
            s.step_fragment(p, mix)

    def whole(comm):
        s = make(comm)
        load(s, comm)
        run(s, first + rest)
        return s.theta.flat.clone(), s.gather_state().momentum.clone(), [a.flat.clone() for a in s.workers]

    def resumed(comm):
        s = make(comm)
        load(s, comm)
        run(s, first)
        st = s.gather_state()
        assert st.fragment_has_momentum == [True, False, True] and st.fragments is plan and not st.has_momentum
        assert st.steps == 2 and st.fragment_steps == [1, 0, 1]
        if comm.rank == 0:
            st.save(path, lay)
        comm.barrier()
        sd = torch.load(path, map_location="cpu", weights_only=True)
        assert sorted(sd["state"]) == sorted(plan.tensors(0) + plan.tensors(2))       # whole fragments only
        s2 = make(comm)
        s2.theta.flat.copy_(s.theta.flat)
        for a, b in zip(s2.workers, s.workers):
            a.flat.copy_(b.flat)
        s2.load_state(OuterState.load(path, lay, tdt, "cpu", fragments=plan))
        assert s2.fragment_has_momentum == [True, False, True]
        run(s2, rest)
        return s2.theta.flat.clone(), s2.gather_state().momentum.clone(), [a.flat.clone() for a in s2.workers]

    a, b = VirtualWorld(world).run(whole), VirtualWorld(world).run(resumed)
    for r in range(world):
        assert torch.equal(bits(a[r][0]), bits(b[r][0])) and torch.equal(bits(a[r][1]), bits(b[r][1]))
        for x, y in zip(a[r][2], b[r][2]):
            assert torch.equal(bits(x), bits(y))
    # what a single-process fragment-wise state would write: the same keys and buffers
    sd = torch.load(path, map_location="cpu", weights_only=True)
    assert sd["param_groups"][0]["lr"] == 0.7 and sd["param_groups"][0]["nesterov"] is True


class _CountingComm:
    """A world of one whose collectives count themselves: a refusal must come before any."""
    world, rank, inplace = 1, 0, True

    def __init__(self, world=1):
        self.world, self.issued = world, 0

    def all_to_all(self, out, inp, async_op=False):
        self.issued += 1
        raise AssertionError("a collective was issued")

    all_gather = all_to_all


def test_refusals_come_before_any_collective(oracle):
    lay = R.layout()
    plan = R.plans(lay)["strided"]
    tdt, wdt = torch.float32, torch.bfloat16
    kern = R.PieceOracleKernels(oracle)

    def build(comm=None, k_local=2, kernels=kern, lr=0.7, mu=0.9, nesterov=True, plan=plan):
        return ShardedFragmentSync(lay, plan, tdt, wdt, k_local, "cpu", lr, mu, nesterov, bucket_elems=512,
                                   kernels=kernels, comm=comm or _CountingComm())

    with pytest.raises(EdtError, match="64 workers"):
        build(_CountingComm(world=8), k_local=9)
    with pytest.raises(EdtError, match="64 workers"):
        build(k_local=0)
    with pytest.raises(EdtError, match="theta_scatter_mix_list"):
        from tests.oracle_kernels import OracleKernels
        build(kernels=OracleKernels(oracle))
    with pytest.raises(ValueError, match="Nesterov"):
        build(mu=0.0, nesterov=True)
    with pytest.raises(ValueError, match="learning rate"):
        build(lr=-1.0)
    with pytest.raises(ValueError, match="momentum value"):
        build(mu=-0.5, nesterov=False)
    other = R.ParamLayout([(n + 1,) for n in R.NUMELS], list(R.NAMES))
    with pytest.raises(EdtError, match="does not match the layout"):
        build(plan=FragmentPlan.strided(other, 2))
    comm = _CountingComm()
    s = build(comm)
    n = plan.numel(0)
    good = [torch.zeros(n, dtype=wdt) for _ in range(2)]
    for bad_p in (-1, len(plan)):
        with pytest.raises(EdtError, match="out of range"):
            s.step_fragment(bad_p)
        with pytest.raises(EdtError, match="out of range"):
            s.capture_fragment(bad_p)
    for mix in (0.0, -0.1, 1.5, float("nan")):
        with pytest.raises(EdtError, match="mix"):
            s.step_fragment(0, mix)
    for snaps in (good[:1], [torch.zeros(n + 1, dtype=wdt)] * 2, [torch.zeros(n, dtype=torch.float32)] * 2,
                  good + good[:1]):
        with pytest.raises(EdtError, match="snapshots"):
            s.step_fragment(0, 1.0, snapshots=snaps)
    assert comm.issued == 0 and kern.calls == [] and s.steps == 0


def test_accounting():
    lay = R.layout()
    plan = R.plans(lay)["strided"]
    for world, (tdt, wdt) in [(1, R.REGIMES[0]), (2, R.REGIMES[1]), (4, R.REGIMES[2])]:
        k_local = 8 // world
        s = ShardedFragmentSync(lay, plan, tdt, wdt, k_local, "cpu", kernels=R.PieceOracleKernels(None),
                                comm=VirtualWorld(world).comm(0), bucket_elems=world * 64 * 5)
        bg, bw = torch.empty(0, dtype=tdt).element_size(), torch.empty(0, dtype=wdt).element_size()
        whole = 0
        for p in range(len(plan)):
            F, fp = plan.numel(p), s.f_pad[p]
            assert fp % (world * 64) == 0 and 0 <= fp - F < world * 64
            assert s.wire_bytes(p) == int((world - 1) / world * fp * (4 + bg))
            own = s._owned_elems(p)
            assert (own == F) if world == 1 else (0 < own < F)
            p1, p2 = F * (k_local * bw + bg + 4), own * (world * 4 + 4 * bg)
            assert s.kernel_bytes(p, merge=False) == p1 + p2 + F * 2 * bg
            assert s.kernel_bytes(p) == p1 + p2 + F * (2 * bg + k_local * bw)
            assert s.kernel_bytes(p, mix=0.5) == p1 + p2 + F * (2 * bg + 2 * k_local * bw)
            whole += s.wire_bytes(p)
        # a round robin moves what one whole reduce_ordered step moves, up to the fragments' padding
        unit = world * 64
        n_pad = -(-lay.total // unit) * unit
        assert 0 <= whole - int((world - 1) / world * n_pad * (4 + bg)) <= len(plan) * unit * (4 + bg)


# ---------------------------------------------------------------------------------------------
# gloo, world 2 (the launcher idiom of tests/test_distributed_cpu.py)

def _gloo_worker(rank, port, outdir):
    import torch.distributed as dist

    from oracle import oracle
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=2)
    lay = R.layout()
    plan = R.plans(lay)["explicit"]
    tdt, wdt = torch.float32, torch.bfloat16
    theta, workers = R.population(lay, tdt, wdt, 4)
    s = ShardedFragmentSync(lay, plan, tdt, wdt, 2, "cpu", bucket_elems=384, kernels=R.PieceOracleKernels(oracle))
    assert not s.inplace
    s.theta.flat.copy_(theta)
    for a, w in zip(s.workers, workers[rank * 2:]):
        a.flat.copy_(w)
    for p, mix, _ in R.schedule_steps(len(plan)):
        s.step_fragment(p, mix)
    torch.save({"theta": s.theta.flat.clone(), "mom": s.gather_state().momentum.clone(),
                "workers": [a.flat.clone() for a in s.workers]}, os.path.join(outdir, f"rank{rank}.pt"))
    dist.barrier()
    dist.destroy_process_group()


@pytest.mark.slow
def test_schedule_over_gloo_world2(oracle, tmp_path):
    import torch.multiprocessing as mp

    from tests.test_distributed_cpu import _free_port
    mp.start_processes(_gloo_worker, args=(_free_port(), str(tmp_path)), nprocs=2, join=True, start_method="spawn")
    res = [torch.load(tmp_path / f"rank{r}.pt", weights_only=True) for r in range(2)]
    lay = R.layout()
    plan = R.plans(lay)["explicit"]
    theta, workers = R.population(lay, torch.float32, torch.bfloat16, 4)
    ref = R.ShardRun(plan, theta, [workers[:2], workers[2:]], R.OracleArith(oracle), 0.7, 0.9, True)
    for p, mix, _ in R.schedule_steps(len(plan)):
        ref.step(p, mix)
    for r in range(2):
        assert torch.equal(bits(res[r]["theta"]), bits(ref.theta)) and torch.equal(bits(res[r]["mom"]), bits(ref.mom))
        for x, y in zip(res[r]["workers"], ref.workers[r]):
            assert torch.equal(bits(x), bits(y))


# ---------------------------------------------------------------------------------------------
# host-side validation of the C ABI (no GPU: every call fails before any HIP call)

@pytest.fixture(scope="module")
def lib():
    if torch.cuda.is_available():
        pytest.skip("host-pointer validation: CPU-only (a device run would launch on host addresses)")
    from evolutionarydistributedtraining_amd import _lib
    return _lib.load_library()


_host = (ctypes.c_uint8 * 8192)()


def _fake(i, skew=0):
    return _P(ctypes.addressof(_host) // 64 * 64 + 64 * (i + 1) + skew)     # never dereferenced


def _arr(*ptrs):
    return (_P * len(ptrs))(*ptrs)


def test_abi_validation_of_the_piece_list_entries(lib):
    def err():
        return lib.edt_last_error().decode()

    T = 2
    numel = (_U64 * T)(8, 8)                         # fp32: 32 bytes of a 64-byte slot each
    ws = _fake(100)
    big = 1 << 20
    assert lib.edt_abi_version() == 6
    assert lib.edt_delta_partial_list_workspace_bytes(T, 3) == (2 * T + 1 + (2 + 3) * T) * 8
    assert lib.edt_sgd_sum_list_to_workspace_bytes(T, 2) == (2 * T + 1 + (3 + 2) * T) * 8
    assert lib.edt_theta_scatter_mix_list_workspace_bytes(T, 0) == (2 * T + 1 + 2 * T) * 8
    assert lib.edt_delta_partial_list_workspace_bytes(-1, 1) == 0 and lib.edt_sgd_sum_list_to_workspace_bytes(1, 0) == 0

    th, acc, w = _arr(_fake(0), _fake(1)), _arr(_fake(2), _fake(3)), _arr(_fake(4), _fake(5), _fake(6), _fake(7))

    def partial(gdt=0, wdt=0, K=2, Kt=4, theta=th, workers=w, accs=acc, n=numel, T=T, wsp=ws, wsb=big):
        return lib.edt_delta_partial_list(theta, gdt, workers, wdt, K, Kt, accs, n, T, wsp, wsb, None)

    assert partial(gdt=1, wdt=0) < 0 and "dtype pair" in err()
    assert partial(K=0) < 0 and "worker count" in err()
    assert partial(K=65) < 0 and "worker count" in err()
    assert partial(Kt=0) < 0 and "total worker count" in err()
    assert partial(T=-1) < 0 and "piece count" in err()
    assert partial(T=0) == 0
    assert partial(theta=None) < 0 and "null piece table" in err()
    assert partial(accs=None) < 0 and "null piece table" in err()
    assert partial(n=None) < 0 and "null piece table" in err()
    assert partial(wsp=None) < 0 and "workspace" in err()
    assert partial(wsb=8) < 0 and "workspace of" in err()
    assert partial(wsp=_fake(100, 4)) < 0 and "8-byte aligned" in err()
    assert partial(theta=_arr(_fake(0), None)) < 0 and "theta_t[1] is null" in err()
    assert partial(accs=_arr(None, _fake(3))) < 0 and "acc_t[0] is null" in err()
    assert partial(workers=_arr(_fake(4), _fake(5), _fake(6), None)) < 0 and "theta_k[1][1] is null" in err()
    assert partial(n=(_U64 * T)(0, 0), theta=_arr(None, None)) == 0              # empty pieces: nothing read

    parts, mom, out = _arr(_fake(4), _fake(5), _fake(6), _fake(7)), _arr(_fake(8), _fake(9)), _arr(_fake(10), _fake(11))

    def sgd(gdt=0, nacc=2, theta=th, p=parts, m=mom, o=out, mu=0.9, n=numel, T=T, wsp=ws, wsb=big):
        return lib.edt_sgd_sum_list_to(theta, gdt, p, nacc, m, 1, o, n, T, 0.7, mu, 1, wsp, wsb, None)

    assert sgd(gdt=2) < 0 and "dtype" in err()
    assert sgd(nacc=0) < 0 and "partial count" in err()
    assert sgd(nacc=65) < 0 and "partial count" in err()
    assert sgd(T=-1) < 0 and "piece count" in err()
    assert sgd(T=0) == 0
    assert sgd(p=None) < 0 and "null piece table" in err()
    assert sgd(o=None) < 0 and "null piece table" in err()
    assert sgd(m=None) < 0 and "momentum table is null" in err()
    assert sgd(m=_arr(_fake(8), None)) < 0 and "momentum_t[1] is null" in err()
    assert sgd(p=_arr(_fake(4), _fake(5), None, _fake(7))) < 0 and "parts[1][0] is null" in err()
    assert sgd(o=_arr(None, _fake(11))) < 0 and "out_t[0] is null" in err()
    assert sgd(wsb=16) < 0 and "workspace of" in err()

    src, live = _arr(_fake(12), _fake(13)), _arr(_fake(14), _fake(15), _fake(16), _fake(17))

    def scatter(gdt=0, wdt=0, nmix=2, mix=0.5, theta=th, s=src, l=live, n=numel, T=T, wsp=ws, wsb=big):
        return lib.edt_theta_scatter_mix_list(theta, gdt, s, l, wdt, nmix, mix, n, T, wsp, wsb, None)

    assert scatter(gdt=1, wdt=0) < 0 and "dtype pair" in err()
    for mix in (0.0, -0.5, 1.0000001, float("nan"), float("inf")):
        assert scatter(mix=mix) < 0 and "outside (0, 1]" in err()
    assert scatter(nmix=-1) < 0 and "destination count" in err()
    assert scatter(nmix=65) < 0 and "destination count" in err()
    assert scatter(T=-1) < 0 and "piece count" in err()
    assert scatter(T=0) == 0
    assert scatter(theta=None) < 0 and "null piece table" in err()
    assert scatter(s=None) < 0 and "null piece table" in err()
    assert scatter(l=None) < 0 and "live is null" in err()
    assert scatter(s=_arr(_fake(12), None)) < 0 and "src_t[1] is null" in err()
    assert scatter(l=_arr(_fake(14), _fake(15), None, _fake(17))) < 0 and "live[1][0] is null" in err()
    assert scatter(wsb=16) < 0 and "workspace of" in err()
    overlap = "overlaps another operand"
    assert scatter(l=_arr(_fake(14), _fake(15), _fake(16), _fake(0))) < 0 and overlap in err()        # a destination on theta
    assert scatter(l=_arr(_fake(14), _fake(15), _fake(16), _fake(12, 16))) < 0 and overlap in err()   # inside src
    assert scatter(l=_arr(_fake(14), _fake(15), _fake(14, 28), _fake(17))) < 0 and overlap in err()   # one another, by 4 bytes
    assert scatter(theta=_arr(_fake(0), _fake(13))) < 0 and overlap in err()                          # theta on src
    assert scatter(theta=_arr(_fake(0), _fake(0, 16))) < 0 and overlap in err()                       # theta on theta
    assert scatter(nmix=0, l=None, theta=_arr(_fake(0), _fake(12))) < 0 and overlap in err()
