"""The sharded fragment step on the device: the three piece-list kernels against their non-list
siblings on packed copies of the same pieces, the schedule with the HIP kernels on virtual ranks of
one GPU against the composition of those siblings (tests/fragment_shard_reference.py), and the
cross-checks that tie ShardedFragmentSync to OuterSync.step_fragment and to ShardedOuterSync — all
bit for bit. The CPU form of the schedule tests is tests/test_sharded_fragment_cpu.py."""
import pytest
import torch

from evolutionarydistributedtraining_amd import (EdtError, FragmentPlan, OuterSync, ParamArena, ShardedFragmentSync,
                                                 ops)
from evolutionarydistributedtraining_amd.collectives import VirtualWorld
from evolutionarydistributedtraining_amd.distributed import ShardedOuterSync
from tests import fragment_shard_reference as R
from tests.fragment_shard_reference import bits

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
FILL = 77.0
GUARD = 64
# (numel, elements past a 16-byte boundary). Aligned: a run shorter than 8 (scalar tail only), one
# longer than a 2,048-element tile with a tail, one of two 4,096-element chunks and 8 more, 7. Off a
# boundary (the scalar body): 64, 1,000, 2,048 and one longer than a chunk. And an empty piece.
PIECES = [(5, 0), (4099, 0), (64, 1), (0, 0), (1000, 3), (8200, 0), (7, 0), (2048, 5), (4100, 2)]


class Pieces:
    """One operand of a piece-list call: a FILL-ed buffer and its pieces, each with guard bands."""

    def __init__(self, dtype, values=None):
        at, self.spans = GUARD, []
        for n, skew in PIECES:
            self.spans.append((at + skew, n))
            at = -(-(at + skew + n + GUARD) // 64) * 64
        self.buf = torch.full((at,), FILL, dtype=dtype, device=DEV)
        self.views = [self.buf[a:a + n] for a, n in self.spans]
        self.mask = torch.zeros(at, dtype=torch.bool, device=DEV)
        for a, n in self.spans:
            self.mask[a:a + n] = True
        if values is not None:
            self.set(values)

    def set(self, packed):
        self.buf[self.mask] = packed.to(self.buf.dtype)

    def packed(self):
        return self.buf[self.mask].clone()

    def guards_intact(self):
        return bool((self.buf[~self.mask] == FILL).all())


TOTAL = sum(n for n, _ in PIECES)


def _rand(g, scale=0.02):
    return torch.randn(TOTAL, generator=g) * scale


def test_the_pieces_take_both_bodies():
    x = Pieces(torch.bfloat16)
    al = [v.data_ptr() % 16 == 0 for v in x.views]
    assert al == [s == 0 for _, s in PIECES] and x.guards_intact()


# ---------------------------------------------------------------------------------------------
# 1. phase 1

@pytest.mark.parametrize("K", [1, 2, 3, 8])
@pytest.mark.parametrize("tdt,wdt", R.REGIMES)
def test_delta_partial_list_equals_delta_partial_on_packed_copies(tdt, wdt, K):
    g = torch.Generator().manual_seed(K)
    base = _rand(g)
    theta = Pieces(tdt, base.to(DEV))
    workers = [Pieces(wdt, (base + _rand(g, 1e-3)).to(DEV)) for _ in range(K)]
    for k_total in (K, 3 * K):                       # the multiply (powers of two) and the true division
        acc = Pieces(torch.float32)
        ops.delta_partial_list(theta.views, [w.views for w in workers], k_total, acc.views)
        want = torch.empty(TOTAL, dtype=torch.float32, device=DEV)
        ops.delta_partial(theta.packed(), [w.packed() for w in workers], k_total, want)
        assert torch.equal(bits(acc.packed()), bits(want)), k_total
        assert want.abs().max() > 0
        assert acc.guards_intact() and theta.guards_intact() and all(w.guards_intact() for w in workers)
        assert torch.equal(bits(theta.packed()), bits(base.to(tdt).to(DEV)))


# ---------------------------------------------------------------------------------------------
# 2. phase 2

@pytest.mark.parametrize("nacc", [1, 2, 3, 4])
@pytest.mark.parametrize("tdt", [torch.float32, torch.bfloat16])
def test_sgd_sum_list_to_equals_sgd_apply_sum_on_packed_copies(tdt, nacc):
    g = torch.Generator().manual_seed(10 + nacc)
    theta0 = _rand(g).to(tdt).to(DEV)
    parts0 = [_rand(g, 1e-3).to(DEV) for _ in range(nacc)]
    mom0 = _rand(g, 1e-3).to(tdt).to(DEV)
    for has, mu, nesterov in [(False, 0.9, True), (True, 0.9, True), (True, 0.9, False), (False, 0.9, False),
                              (False, 0.0, False)]:
        theta, out = Pieces(tdt, theta0), Pieces(tdt)
        parts = [Pieces(torch.float32, q) for q in parts0]
        mom = Pieces(tdt, mom0) if mu else None
        ops.sgd_sum_list_to(theta.views, [q.views for q in parts], mom.views if mom else None, has, 0.7, mu, nesterov,
                            out.views)
        want_t, want_m = theta0.clone(), mom0.clone() if mu else None
        ops.sgd_apply_sum(want_t, [q.clone() for q in parts0], want_m, has, 0.7, mu, nesterov)
        tag = (has, mu, nesterov)
        assert torch.equal(bits(out.packed()), bits(want_t)), tag
        assert not torch.equal(bits(want_t), bits(theta0)), tag
        assert torch.equal(bits(theta.packed()), bits(theta0)), tag                 # theta is only read
        if mu:
            assert torch.equal(bits(mom.packed()), bits(want_m)), tag
            assert mom.guards_intact(), tag
        assert out.guards_intact() and theta.guards_intact() and all(q.guards_intact() for q in parts), tag
        for q, q0 in zip(parts, parts0):
            assert torch.equal(bits(q.packed()), bits(q0)), tag
    with pytest.raises(EdtError, match="momentum tensors are required"):
        ops.sgd_sum_list_to(theta.views, [q.views for q in parts], None, False, 0.7, 0.9, True, out.views)


# ---------------------------------------------------------------------------------------------
# 3. phase 3

@pytest.mark.parametrize("nmix", [0, 1, 3])
@pytest.mark.parametrize("tdt,wdt", R.REGIMES)
def test_theta_scatter_mix_list_equals_copy_and_lerp(tdt, wdt, nmix):
    g = torch.Generator().manual_seed(20 + nmix)
    src0 = _rand(g).to(tdt).to(DEV)
    live0 = [(src0.float().cpu() + _rand(g, 1e-3)).to(wdt).to(DEV) for _ in range(nmix)]
    for mix in (0.25, 0.5, 1.0):
        src, theta = Pieces(tdt, src0), Pieces(tdt)
        live = [Pieces(wdt, l) for l in live0]
        if mix == 1.0:
            for l in live:                           # the overwrite does not read the destination
                l.set(torch.full((TOTAL,), float("nan"), device=DEV))
        ops.theta_scatter_mix_list(theta.views, src.views, [l.views for l in live], mix)
        assert torch.equal(bits(theta.packed()), bits(src0)), mix
        assert torch.equal(bits(src.packed()), bits(src0)) and src.guards_intact() and theta.guards_intact(), mix
        v = src0.to(wdt)
        for l, l0 in zip(live, live0):
            want = v if mix == 1.0 else ops.lerp(mix, l0, v)
            got = l.packed()
            assert not torch.isnan(got).any(), mix
            assert torch.equal(bits(got), bits(want)), mix
            assert l.guards_intact(), mix


@pytest.mark.parametrize("mix", [0.25, 1.0])
@pytest.mark.parametrize("tdt,wdt", R.REGIMES)
def test_the_two_merge_texts_agree(tdt, wdt, mix):
    """What edt_outer_step_list_mix leaves in its destinations equals what phase 3 leaves in its own
    from the same new theta: the fused list kernels' merge and this unit's are one rule."""
    g = torch.Generator().manual_seed(31)
    K = 3
    base = _rand(g)
    theta = Pieces(tdt, base.to(DEV))
    mom = Pieces(tdt, _rand(g, 1e-3).to(DEV))
    deltas = [Pieces(wdt, (base + _rand(g, 1e-3)).to(DEV)) for _ in range(K)]
    live0 = [(base + _rand(g, 2e-3)).to(wdt).to(DEV) for _ in range(K)]
    fused = [Pieces(wdt, l) for l in live0]
    ops.outer_step_list_mix(theta.views, [d.views for d in deltas], mom.views, True, 0.7, 0.9, True,
                            [l.views for l in fused], mix)
    new_theta = theta.packed()
    assert not torch.equal(bits(new_theta), bits(base.to(tdt).to(DEV)))
    src, out = Pieces(tdt, new_theta), Pieces(tdt)
    mine = [Pieces(wdt, l) for l in live0]
    ops.theta_scatter_mix_list(out.views, src.views, [l.views for l in mine], mix)
    for a, b in zip(mine, fused):
        assert torch.equal(bits(a.packed()), bits(b.packed()))
    assert torch.equal(bits(out.packed()), bits(new_theta))


def test_phase3_refuses_overlap_and_bad_mix():
    theta, src, live = Pieces(torch.float32), Pieces(torch.float32, torch.zeros(TOTAL, device=DEV)), Pieces(torch.bfloat16)
    for mix in (0.0, 1.5, float("nan")):
        with pytest.raises(EdtError, match="mix"):
            ops.theta_scatter_mix_list(theta.views, src.views, [live.views], mix)
    with pytest.raises(EdtError, match="overlaps"):
        ops.theta_scatter_mix_list(theta.views, theta.views, [live.views], 0.5)
    with pytest.raises(EdtError, match="overlaps"):
        ops.theta_scatter_mix_list(theta.views, src.views, [live.views, live.views], 0.5)
    assert theta.guards_intact() and bool((theta.packed() == FILL).all()) and bool((live.packed() == FILL).all())


# ---------------------------------------------------------------------------------------------
# 4. the schedule with the HIP kernels on virtual ranks of one GPU

class GpuArith:
    """The composition's arithmetic from the existing non-list kernels, on packed copies."""

    def partial(self, theta, deltas, k_total, acc):
        ops.delta_partial(theta, deltas, k_total, acc, False)

    def sgd_sum(self, theta, parts, mom, has, lr, mu, nesterov):
        ops.sgd_apply_sum(theta, parts, mom, has, lr, mu, nesterov)

    def merge(self, live, theta_new, mix):
        if mix == 1.0:
            live.copy_(theta_new)
        else:
            ops.lerp(mix, live.clone(), theta_new.to(live.dtype), out=live)


def _make(lay, plan, tdt, wdt, k_local, bucket):
    def make(comm):
        return ShardedFragmentSync(lay, plan, tdt, wdt, k_local, DEV, 0.7, 0.9, True, bucket_elems=bucket, comm=comm)
    return make


@pytest.mark.parametrize("world", [2, 4])
@pytest.mark.parametrize("name", ["strided", "explicit"])
@pytest.mark.parametrize("tdt,wdt", R.REGIMES)
def test_schedule_on_virtual_ranks_equals_the_composition(world, name, tdt, wdt):
    """R.drive: two round robins (mix 0.5 and 1.0, with and without snapshots); theta, the gathered
    momentum and every worker bit for bit on every rank after every step, NaN canaries everywhere
    outside the stepped fragment."""
    lay = R.layout()
    plan = R.plans(lay)[name]
    k_local = 2
    theta, workers = R.population(lay, tdt, wdt, k_local * world, device=DEV)
    syncs, _ = R.drive(VirtualWorld(world), _make(lay, plan, tdt, wdt, k_local, R.bucket_elems(world, name)), plan, theta,
                       workers, GpuArith())
    assert syncs[0].kernels is ops and max(len(b) for b in syncs[0].buckets) >= 3
    for s in syncs[1:]:
        assert torch.equal(bits(s.theta.flat), bits(syncs[0].theta.flat))


# ---------------------------------------------------------------------------------------------
# 5. cross-checks

@pytest.mark.parametrize("wdt", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("name", ["strided", "explicit"])
def test_world1_fp32_theta_equals_outer_sync_step_fragment(name, wdt):
    """With fp32 theta the fp32 partial sum is the fused kernel's chain, so at world 1 the sharded
    fragment step is OuterSync.step_fragment bit for bit: theta, momentum, workers."""
    lay = R.layout()
    plan = R.plans(lay)[name]
    tdt, K = torch.float32, 3
    theta, workers = R.population(lay, tdt, wdt, K, device=DEV)
    s = ShardedFragmentSync(lay, plan, tdt, wdt, K, DEV, 0.7, 0.9, True, bucket_elems=R.bucket_elems(1, name),
                            comm=VirtualWorld(1).comm(0))
    o = OuterSync(ParamArena(lay, tdt, DEV, theta.clone()), [ParamArena(lay, wdt, DEV, w.clone()) for w in workers],
                  0.7, 0.9, True, fragments=plan)
    s.theta.flat.copy_(theta)
    for a, w in zip(s.workers, workers):
        a.flat.copy_(w)
    seed = 0
    for p, mix, snap in R.schedule_steps(len(plan)):
        snaps = s.capture_fragment(p) if snap else None
        snaps_o = o.capture_fragment(p) if snap else None
        for a, b in zip(s.workers, o.workers):
            seed += 1
            a.flat.copy_(R.drift(a.flat, seed))
            b.flat.copy_(a.flat)
        s.step_fragment(p, mix, snaps)
        o.step_fragment(p, mix, snaps_o)
        tag = (p, mix, snap)
        assert torch.equal(bits(s.theta.flat), bits(o.theta.flat)), tag
        assert torch.equal(bits(s.gather_state().momentum), bits(o.state.momentum)), tag
        for a, b in zip(s.workers, o.workers):
            assert torch.equal(bits(a.flat), bits(b.flat)), tag
    assert s.fragment_has_momentum == o.state.fragment_has_momentum and s.fragment_steps == o.state.fragment_steps
    assert not torch.equal(bits(s.theta.flat), bits(theta))


@pytest.mark.parametrize("tdt,wdt", R.REGIMES)
def test_one_fragment_mix1_world2_equals_the_whole_sharded_step(tdt, wdt):
    """A one-fragment plan at mix 1.0 is ShardedOuterSync(mode="reduce_ordered").step(broadcast=True)
    over [0, n): theta, the momentum and the workers, two steps."""
    lay = R.layout()
    plan = FragmentPlan(lay, [list(range(len(lay)))])
    world, k_local, n, bucket = 2, 2, lay.total, 4608
    theta, workers = R.population(lay, tdt, wdt, k_local * world, device=DEV)
    gens = [workers, [R.drift(w, 50 + i) for i, w in enumerate(workers)]]

    def body(comm):
        f = ShardedFragmentSync(lay, plan, tdt, wdt, k_local, DEV, 0.7, 0.9, True, bucket_elems=bucket, comm=comm)
        w = ShardedOuterSync(lay, tdt, wdt, k_local, DEV, 0.7, 0.9, True, mode="reduce_ordered", bucket_elems=bucket,
                             comm=comm)
        assert f.buckets[0] == w.buckets and len(w.buckets) >= 3 and f.f_pad[0] == w.n_pad > n
        f.theta.flat.copy_(theta)
        w.theta.flat.copy_(theta)
        for gen in gens:
            for j in range(k_local):
                f.workers[j].flat.copy_(gen[comm.rank * k_local + j])
                w.workers[j].flat.copy_(gen[comm.rank * k_local + j])
            f.step_fragment(0, 1.0)
            w.step(broadcast=True)
            assert torch.equal(bits(f.theta.flat), bits(w.theta.flat))
            for _, _, s0, s1, off in f._owned(0):      # the owned shards' real elements (the whole step also
                real = max(0, min(s1, n) - s0)         # steps its padding, the fragment step never writes it)
                assert torch.equal(bits(f.mom[0][off:off + real]), bits(w.mom_shard[off:off + real]))
            for a, b in zip(f.workers, w.workers):
                assert torch.equal(bits(a.flat), bits(b.flat))
        return f.theta.flat.clone()

    got = VirtualWorld(world).run(body, devices=[DEV] * world)
    assert torch.equal(bits(got[0]), bits(got[1])) and not torch.equal(bits(got[0]), bits(theta))
