"""The quantized sharded fragment step on the device (csrc/edt_fragment_q.hip): the two fragment-space
kernels against the existing FLAT quantized kernels on packed, zero-padded copies (every packed
byte, every residual element, the new theta, the momentum), their independence of the pieces'
alignment, the schedule with the HIP kernels on virtual ranks of one GPU against the composition of
the flat kernels (tests/fragment_q_reference.py), the zero-delta identity with the fp32 step, and the
argument errors — all bit for bit. The CPU form is tests/test_sharded_fragment_q_cpu.py."""
import numpy as np
import pytest
import torch

from evolutionarydistributedtraining_amd import EdtError, FragmentPlan, ParamLayout, ShardedFragmentSync, ops
from evolutionarydistributedtraining_amd.collectives import VirtualWorld
from tests import fragment_q_reference as FQ
from tests import fragment_shard_reference as R
from tests import quant_reference as Q
from tests.fragment_shard_reference import bits

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
WORLD = 4
GUARD = 32                      # elements around an arena / a compact buffer: NaN canaries
NAN = float("nan")


def guarded(n, dtype, skew=0, fill=NAN):
    """(buffer, view): n elements at GUARD + skew elements into a canary-filled buffer; skew 0 starts
    the view on a 16-byte boundary (GUARD elements are 64 or 128 bytes)."""
    buf = torch.full((n + 2 * GUARD + 8,), fill, dtype=dtype, device=DEV)
    return buf, buf[GUARD + skew:GUARD + skew + n]


def guards_intact(buf, view):
    lo = (view.data_ptr() - buf.data_ptr()) // buf.element_size()
    return bool(torch.isnan(buf[:lo]).all()) and bool(torch.isnan(buf[lo + view.numel():]).all())


def padded(plan, p, flat, fp):
    out = torch.zeros(fp, dtype=flat.dtype, device=flat.device)
    out[:plan.numel(p)] = R.pack(plan, p, flat)
    return out


def cut(buf, pieces, arena):
    return [buf[a:a + n] if arena else buf[f:f + n] for a, f, n in pieces]


def arena_population(lay, tdt, wdt, K, seed, skew=0):
    """theta and K workers in guarded arenas (values independent of skew)."""
    theta0, workers0 = R.population(lay, tdt, wdt, K, seed=seed)
    tb, theta = guarded(lay.total, tdt, skew)
    theta.copy_(theta0)
    ws = []
    for w0 in workers0:
        wb, w = guarded(lay.total, wdt, skew)
        w.copy_(w0)
        ws.append((wb, w))
    return (tb, theta), ws


def phase1_ranges(plan, p, name):
    """The whole padded fragment as regions of 512, and (a range that starts inside the fragment) its
    second bucket as the schedule cuts it."""
    fp = FQ.f_pad(plan, p, WORLD)
    out = [(0, fp, 512)]
    bucket = FQ.bucket_elems(WORLD, name)
    if fp > bucket:
        out.append((bucket, min(2 * bucket, fp), (min(2 * bucket, fp) - bucket) // WORLD))
    return out


# ---------------------------------------------------------------------------------------------
# 1. phase 1 against the flat kernel

@pytest.mark.parametrize("k_local,k_total", [(1, 3), (1, 4), (3, 3), (3, 4)])
@pytest.mark.parametrize("tdt,wdt", R.REGIMES)
@pytest.mark.parametrize("fmt", FQ.FORMATS)
def test_delta_partial_q_frag_equals_delta_partial_q_on_padded_copies(fmt, tdt, wdt, k_local, k_total):
    """Every packed byte and every residual element, with and without error feedback, from the live
    arenas and from snapshots, over whole fragments and over a bucket inside one; one worker element
    is Inf and one, in another block, NaN (the scale-255 rule)."""
    lay = R.layout()
    vec = gather = 0
    for name, plan in R.plans(lay).items():
        (tb, theta), ws = arena_population(lay, tdt, wdt, k_local, seed=k_local + k_total)
        for p in range(len(plan)):
            (a0, _), (a1, n1) = plan.runs(p)[0], plan.runs(p)[-1]
            ws[0][1][a0 + 1] = float("inf")                              # block 0 of the fragment
            ws[-1][1][a1 + n1 - 1] = NAN                                 # its last block (may straddle the padding)
        keep = [tb.clone()] + [wb.clone() for wb, _ in ws]
        for p in range(len(plan)):
            F = plan.numel(p)
            snaps = [R.pack(plan, p, w) for _, w in ws]
            for lo, hi, region in phase1_ranges(plan, p, name):
                n = hi - lo
                pc = plan.pieces(p, lo, hi)
                starts = [f for _, f, _ in pc]
                th_flat = padded(plan, p, theta, FQ.f_pad(plan, p, WORLD))[lo:hi].clone()
                ws_flat = [padded(plan, p, w, FQ.f_pad(plan, p, WORLD))[lo:hi].clone() for _, w in ws]
                nb = n // region * ops.q_region_bytes(region, fmt)
                res0 = (torch.randn(n, generator=torch.Generator().manual_seed(p)) * 1e-5).to(DEV)
                res0[max(0, F - lo):] = 0                                # the padding's residual is zero
                for ef in (False, True):
                    want = torch.full((nb,), 0xAA, dtype=torch.uint8, device=DEV)
                    want_r = res0.clone() if ef else None
                    ops.delta_partial_q(th_flat, ws_flat, k_total, want, region, fmt, want_r)
                    for live in (True, False):
                        deltas = [cut(w, pc, True) for _, w in ws] if live else [cut(s, pc, False) for s in snaps]
                        pb, packed = guarded(nb, torch.uint8, fill=0xAA)
                        rb, res = guarded(n, torch.float32)
                        res.copy_(res0)
                        ops.delta_partial_q_frag(cut(theta, pc, True), deltas, k_total, starts, lo, packed, region, fmt,
                                                 res if ef else None)
                        tag = (name, p, lo, hi, ef, live)
                        assert torch.equal(packed, want), tag
                        assert bool((pb[:GUARD] == 0xAA).all()) and bool((pb[GUARD + nb:] == 0xAA).all()), tag
                        assert torch.equal(bits(res), bits(want_r if ef else res0)) and guards_intact(rb, res), tag
                sc =Q.unpack(want.cpu().numpy(), fmt, region)[1]
                if lo == 0:
                    assert sc[0] == 255 and (sc == 255).sum() >= 2 and (sc != 255).any(), (name, p)
                v, g = FQ.lane_paths(pc, lo, hi, [(theta.data_ptr(), theta.element_size(), True)] +
                                     [(w.data_ptr(), w.element_size(), True) for _, w in ws])
                vec, gather = vec + v, gather + g
        for k, b in zip(keep, [tb] + [wb for wb, _ in ws]):              # the arenas are only read
            assert torch.equal(bits(k), bits(b))
    assert vec > 0 and gather > 0


# ---------------------------------------------------------------------------------------------
# 2. phase 2 against the flat kernel

def _regions(n, nacc, fmt, seed):
    """nacc packed regions of n elements: random partials through the numpy encoder."""
    g = np.random.default_rng(seed)
    out = []
    for _ in range(nacc):
        codes, scales = Q.quantize((g.standard_normal(n) * 1e-3).astype(np.float32), fmt)
        out.append(torch.from_numpy(Q.pack(codes, scales, fmt, n)).to(DEV))
    return out


@pytest.mark.parametrize("nacc", [1, 2, 4])
@pytest.mark.parametrize("tdt", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("fmt", FQ.FORMATS)
def test_sgd_sum_q_frag_to_equals_sgd_apply_sum_q_on_padded_copies(fmt, tdt, nacc):
    """Every owned shard of every fragment at world 4 (whole, partly padding, all padding): the
    output and the momentum against the flat kernel on a packed copy; theta itself, the momentum's
    padding and everything around the compact buffers untouched (NaN canaries); the output's padding
    zeroed. First step, carried momentum (Nesterov and not), no momentum."""
    lay = R.layout()
    seen = set()
    for name, plan in R.plans(lay).items():
        (tb, theta), _ = arena_population(lay, tdt, tdt, 1, seed=nacc)
        keep = tb.clone()
        bucket = FQ.bucket_elems(WORLD, name)
        for p in range(len(plan)):
            F, fp = plan.numel(p), FQ.f_pad(plan, p, WORLD)
            th_pad = padded(plan, p, theta, fp)
            shards = [(b + r * (min(b + bucket, fp) - b) // WORLD, b + (r + 1) * (min(b + bucket, fp) - b) // WORLD)
                      for b in range(0, fp, bucket) for r in range(WORLD)]
            for s0, s1 in shards[:WORLD] + shards[-WORLD:]:              # the first and the last bucket's
                n, real = s1 - s0, max(0, min(s1, F) - s0)
                seen.add("whole" if real == n else "part" if real else "none")
                pc = plan.pieces(p, s0, s1)
                regions = _regions(n, nacc, fmt, seed=s0 + nacc)
                mom0 = (torch.randn(n, generator=torch.Generator().manual_seed(s0)) * 1e-3).to(tdt).to(DEV)
                for has, mu, nesterov in [(False, 0.9, True), (True, 0.9, True), (True, 0.9, False), (False, 0.0, False)]:
                    want_t, want_m = th_pad[s0:s1].clone(), mom0.clone() if mu else None
                    ops.sgd_apply_sum_q(want_t, regions, fmt, want_m, has, 0.7, mu, nesterov)
                    ob, out = guarded(n, tdt)
                    mb, mom = guarded(n, tdt)
                    mom[:real] = mom0[:real]                             # its padding keeps the canary
                    ops.sgd_sum_q_frag_to(cut(theta, pc, True), [f for _, f, _ in pc], s0, regions, fmt,
                                          mom if mu else None, has, 0.7, mu, nesterov, out)
                    tag = (name, p, s0, s1, has, mu, nesterov)
                    assert torch.equal(bits(out[:real]), bits(want_t[:real])), tag
                    assert not bits(out[real:]).any() and guards_intact(ob, out), tag          # zeroed, +0
                    if mu:
                        assert torch.equal(bits(mom[:real]), bits(want_m[:real])), tag
                    else:
                        assert torch.equal(bits(mom[:real]), bits(mom0[:real])), tag
                    assert bool(torch.isnan(mom[real:]).all()) and guards_intact(mb, mom), tag
                    if real:
                        assert not torch.equal(bits(out[:real]), bits(th_pad[s0:s0 + real])), tag
        assert torch.equal(bits(keep), bits(tb))                         # theta is only read
    assert seen == {"whole", "part", "none"}
    with pytest.raises(EdtError, match="momentum buffer is required"):
        ops.sgd_sum_q_frag_to(cut(theta, pc, True), [f for _, f, _ in pc], s0, regions, fmt, None, False, 0.7, 0.9, True,
                              out)


# ---------------------------------------------------------------------------------------------
# 3. alignment independence

ALIGNED_NUMELS = [8, 4104, 64, 0, 1000, 8200, 16, 2048]         # multiples of 8: every piece 16-byte aligned


@pytest.mark.parametrize("tdt,wdt", R.REGIMES)
@pytest.mark.parametrize("fmt", FQ.FORMATS)
def test_the_bytes_do_not_depend_on_alignment(fmt, tdt, wdt):
    """The same fragment from arenas placed so that every piece is 16-byte aligned (every covered
    lane takes the vector loads) and from arenas one element further (every lane gathers): the
    same packed bytes and residual, the same new theta and momentum."""
    lay = ParamLayout([(n,) for n in ALIGNED_NUMELS], list(R.NAMES))
    plan = FragmentPlan(lay, [[0, 5, 6], [1, 3, 7], [2, 4]])
    K, k_total = 2, 4
    for p in range(len(plan)):
        fp = FQ.f_pad(plan, p, WORLD)
        pc = plan.pieces(p, 0, fp)
        starts = [f for _, f, _ in pc]
        nb = fp // 512 * ops.q_region_bytes(512, fmt)
        regions = _regions(fp, 2, fmt, seed=p)
        got = []
        for skew in (0, 1):
            (_, theta), ws = arena_population(lay, tdt, wdt, K, seed=5, skew=skew)
            v, g = FQ.lane_paths(pc, 0, fp, [(theta.data_ptr(), theta.element_size(), True)] +
                                 [(w.data_ptr(), w.element_size(), True) for _, w in ws])
            assert (v == plan.numel(p) // 8 and v > 0) if skew == 0 else v == 0
            packed = torch.zeros(nb, dtype=torch.uint8, device=DEV)
            res = torch.zeros(fp, dtype=torch.float32, device=DEV)
            ops.delta_partial_q_frag(cut(theta, pc, True), [cut(w, pc, True) for _, w in ws], k_total, starts, 0, packed,
                                     512, fmt, res)
            out = torch.full((fp,), NAN, dtype=tdt, device=DEV)
            mom = torch.zeros(fp, dtype=tdt, device=DEV)
            ops.sgd_sum_q_frag_to(cut(theta, pc, True), starts, 0, regions, fmt, mom, False, 0.7, 0.9, True, out)
            got.append((packed, res, out, mom))
        assert torch.equal(got[0][0], got[1][0]) and got[0][0].any()
        for a, b in zip(got[0][1:], got[1][1:]):
            assert torch.equal(bits(a), bits(b))
        assert got[0][1].any()


# ---------------------------------------------------------------------------------------------
# 4. the schedule with the HIP kernels on virtual ranks of one GPU

class GpuArith:
    """The composition's merge from the existing kernels, on packed copies."""

    def merge(self, live, theta_new, mix):
        if mix == 1.0:
            live.copy_(theta_new)
        else:
            ops.lerp(mix, live.clone(), theta_new.to(live.dtype), out=live)


def _make(lay, plan, tdt, wdt, k_local, bucket, fmt, ef=True):
    def make(comm):
        return ShardedFragmentSync(lay, plan, tdt, wdt, k_local, DEV, 0.7, 0.9, True, bucket_elems=bucket, comm=comm,
                                   wire_format=fmt, error_feedback=ef)
    return make


@pytest.mark.parametrize("world,name,fmt,regime", [(w, name, fmt, i % 3) for i, (w, name, fmt) in enumerate(
    (w, name, fmt) for w in (2, 4) for name in ("strided", "explicit") for fmt in FQ.FORMATS)])
def test_schedule_on_virtual_ranks_equals_the_composition(world, name, fmt, regime):
    """FQ.drive_q with `ops` as the composition's arithmetic — the existing flat HIP kernels
    (edt_delta_partial_q, edt_sgd_apply_sum_q) on packed, padded copies: two round robins (mix 0.5 and
    1.0, snapshots alternating); theta, the gathered momentum, every worker and every rank's
    residuals bit for bit after every step, NaN canaries everywhere else. Error feedback on."""
    lay = R.layout()
    plan = R.plans(lay)[name]
    tdt, wdt = R.REGIMES[regime]
    k_local = 2
    theta, workers = R.population(lay, tdt, wdt, k_local * world, device=DEV)
    syncs, ref = FQ.drive_q(VirtualWorld(world), _make(lay, plan, tdt, wdt, k_local, FQ.bucket_elems(world, name), fmt),
                            plan, theta, workers, ops, GpuArith(), fmt)
    assert syncs[0].kernels is ops and max(len(b) for b in syncs[0].buckets) >= 3
    for s in syncs[1:]:
        assert torch.equal(bits(s.theta.flat), bits(syncs[0].theta.flat))
    assert any(r.any() for rs in ref.residual for r in rs) and not torch.equal(bits(ref.theta), bits(theta))


# ---------------------------------------------------------------------------------------------
# 5. zero delta: the quantized step is the fp32 step

@pytest.mark.parametrize("tdt,wdt", [R.REGIMES[0], R.REGIMES[2]])
@pytest.mark.parametrize("fmt", FQ.FORMATS)
def test_zero_delta_equals_the_fp32_step(fmt, tdt, wdt):
    """With every worker equal to theta every partial is +0, which the wire format carries exactly:
    theta, the momentum and the workers after quantized steps equal the fp32 ShardedFragmentSync's on
    the same layout, and the residuals stay zero."""
    lay = R.layout()
    plan = R.plans(lay)["explicit"]
    world, k_local = 2, 2
    theta, _ = R.population(lay, tdt, wdt, 1, device=DEV)

    def body(comm):
        kw = dict(bucket_elems=FQ.bucket_elems(world, "explicit"), comm=comm)
        q = ShardedFragmentSync(lay, plan, tdt, wdt, k_local, DEV, 0.7, 0.9, True, wire_format=fmt, **kw)
        f = ShardedFragmentSync(lay, plan, tdt, wdt, k_local, DEV, 0.7, 0.9, True, **kw)
        for s in (q, f):
            s.theta.flat.copy_(theta)
        for p, mix, _ in R.schedule_steps(len(plan)):
            for s in (q, f):
                for a in s.workers:
                    a.flat.copy_(s.theta.flat)                           # every delta is zero
                s.step_fragment(p, mix)
            assert torch.equal(bits(q.theta.flat), bits(f.theta.flat)), (p, mix)
            assert torch.equal(bits(q.gather_state().momentum), bits(f.gather_state().momentum)), (p, mix)
            for a, b in zip(q.workers, f.workers):
                assert torch.equal(bits(a.flat), bits(b.flat)), (p, mix)
        assert not any(r.any() for r in q.residual)
        return q.theta.flat.clone()

    got = VirtualWorld(world).run(body, devices=[DEV] * world)
    assert torch.equal(bits(got[0]), bits(got[1])) and torch.equal(bits(got[0]), bits(theta))


# ---------------------------------------------------------------------------------------------
# 6. argument errors: EdtError, nothing launched

def test_argument_errors_launch_nothing():
    lay = R.layout()
    plan = R.plans(lay)["explicit"]
    p, fmt = 0, "mxfp8"
    fp = FQ.f_pad(plan, p, WORLD)
    pc = plan.pieces(p, 0, fp)
    starts = [f for _, f, _ in pc]
    assert len(pc) == 2
    (_, theta), ws = arena_population(lay, torch.float32, torch.bfloat16, 2, seed=1)
    th, wk = cut(theta, pc, True), [cut(w, pc, True) for _, w in ws]
    nb = fp // 512 * ops.q_region_bytes(512, fmt)
    big = torch.full((nb + 64,), 0xAA, dtype=torch.uint8, device=DEV)
    packed = big[:nb]
    res = torch.full((fp + 8,), 7.0, device=DEV)
    out = torch.full((fp,), 7.0, device=DEV)
    mom = torch.full((fp + 8,), 7.0, device=DEV)
    regs = _regions(fp, 2, fmt, seed=0)
    ok1 = dict(thetas=th, workers=wk, k_total=4, starts=starts, lo=0, packed=packed, region_elems=512, fmt=fmt,
               residual=res[:fp])
    ok2 = dict(thetas=th, starts=starts, lo=0, regions=regs, fmt=fmt, momentum=mom[:fp], has_momentum=True, lr=0.7,
               momentum_coef=0.9, nesterov=True, out=out)
    bad1 = [dict(fmt="int8"), dict(region_elems=500), dict(packed=packed.to(torch.int8)), dict(packed=packed[:-16]),
            dict(packed=big[8:nb + 8]),                                          # off a 16-byte boundary
            dict(residual=res[:fp - 1]), dict(residual=res[:fp].double()), dict(residual=res[1:fp + 1]),
            dict(starts=starts[::-1]), dict(starts=[0, starts[1] - 1]),          # unsorted; overlapping
            dict(starts=[0, fp - 3]), dict(starts=starts[:-1]),                  # leaving the range; one too few dict(lo=64), dict(workers=[]), dict(workers=[wk[0][:-1]]),
            dict(packed=packed.cpu()), dict(k_total=0), dict(thetas=[t.double() for t in th])]
    for kw in bad1:
        with pytest.raises(EdtError):
            ops.delta_partial_q_frag(**{**ok1, **kw})
    bad2 = [dict(fmt="fp8"), dict(regions=[]), dict(regions=[regs[0][:-16]]), dict(regions=[regs[0].to(torch.int8)]),
            dict(momentum=None), dict(momentum=mom[:fp].to(torch.bfloat16)), dict(momentum=mom[1:fp + 1]),
            dict(out=out[:fp - 512]), dict(out=out.to(torch.bfloat16)), dict(starts=starts[::-1]), dict(lo=8),
            dict(regions=[regs[0].cpu()]), dict(thetas=th[:-1])]
    for kw in bad2:
        with pytest.raises(EdtError):
            ops.sgd_sum_q_frag_to(**{**ok2, **kw})
    torch.cuda.synchronize()
    assert bool((big == 0xAA).all()) and bool((res == 7.0).all()) and bool((out == 7.0).all()) and bool((mom == 7.0).all())
    ops.delta_partial_q_frag(**ok1)                                              # and the good calls do run
    ops.sgd_sum_q_frag_to(**ok2)
    assert not bool((packed == 0xAA).all()) and not bool((out == 7.0).all())
