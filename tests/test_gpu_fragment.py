"""The fragment-wise outer step and its fused worker merge (edt_outer_step_list_mix,
OuterSync.step_fragment, diloco.outer_step_fragment) on an MI355X.

Bar, everywhere: bit for bit. The step against `ops.outer_step_list` on clones of the same runs;
the merge against the CPU restatement (tests/fragment_reference.py) and against the device
composition `ops.broadcast_theta` -> `ops.lerp`. Every operand of the kernel cases lives in one
buffer of sentinel NaNs with gaps around its runs, and the whole buffer is compared, so a store
past a run's edge fails the test.
"""
import pytest
import torch

from tests import fragment_reference as ref
from tests.golden_data import bits

pytestmark = pytest.mark.gpu

F32, BF16 = torch.float32, torch.bfloat16
REGIMES = [(F32, F32), (F32, BF16), (BF16, BF16)]
# empty, below a vector, tail only, one vector, vector + tail, tile edges (2048 = 256 threads x 8),
# exactly one list chunk (4096), a second chunk of one element, two chunks with a ragged tail
SIZES = [0, 1, 7, 8, 15, 513, 2048, 2049, 4096, 4097, 8200]
HYPERS = [(False, 0.7, 0.9, True), (True, 0.7, 0.9, True), (False, 0.5, 0.8, False), (True, 0.5, 0.8, False)]
MIXES = [1.0, 0.5, 0.3, 2.0 ** -24]
GAP = 8
SENTINEL = {F32: 0x7FC0BEEF, BF16: 0x7FED}
INT = {F32: torch.int32, BF16: torch.int16}


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def ops():
    from evolutionarydistributedtraining_amd import ops as o
    return o


def eq(a, b):
    return a.dtype == b.dtype and torch.equal(bits(a.cpu()), bits(b.cpu()))


class Buf:
    """One operand: its runs (CPU tensors) laid into one device buffer of sentinels, each run on a
    16-byte boundary plus `shift` bytes, at least GAP elements apart."""

    def __init__(self, runs, dev, shift=0):
        dt = runs[0].dtype
        es = 2 if dt == BF16 else 4
        al, sh = 16 // es, shift // es
        pos, spans = GAP, []
        for r in runs:
            s = -(-pos // al) * al + sh
            spans.append((s, s + r.numel()))
            pos = s + r.numel() + GAP
        self.dt, self.spans, self.runs0 = dt, spans, [r.clone() for r in runs]
        self.host0 = self.image(runs, pos + GAP)
        self.buf = self.host0.to(dev).view(dt)
        assert self.buf.data_ptr() % 16 == 0
        self.views = [self.buf[a:b] for a, b in spans]
        assert all(v.data_ptr() % 16 == shift for v in self.views if v.numel())

    def image(self, runs, total=None):
        img = torch.full((total or self.host0.numel(),), SENTINEL[runs[0].dtype], dtype=INT[runs[0].dtype])
        for (a, b), r in zip(self.spans, runs):
            img[a:b] = bits(r)
        return img

    def reset(self):
        self.buf.copy_(self.host0.view(self.dt))

    def holds(self, runs):
        """The whole buffer: `runs` inside the spans (None: the initial values), sentinels outside."""
        want = self.host0 if runs is None else self.image(runs)
        return torch.equal(self.buf.view(INT[self.dt]).cpu(), want)


def plant(theta, workers, mom, live):
    """Values where the rounding rules bite, in the 513-element run: signed zeros, subnormals, and a
    theta that a carried momentum pushes past the largest bf16 (the merge then sees an Inf)."""
    r = SIZES.index(513)
    gdt, wdt = theta[r].dtype, workers[0][r].dtype
    theta[r][:6] = torch.tensor([0.0, -0.0, 1e-40, -1e-40, 3.389e38, 0.0]).to(gdt)
    mom[r][:6] = torch.tensor([0.0, -0.0, 0.0, 1e-40, -2e36, -0.0]).to(gdt)
    for k, w in enumerate(workers):
        w[r][:6] = torch.tensor([-0.0, -0.0, -1e-40 if k % 2 else 1e-40, -1e-40, 3.3895e38, 0.0]).to(wdt)
    for l in live:
        l[r][:6] = torch.tensor([-0.0, 0.0, 1e-40, -1e-40, 1.0, -0.0]).to(wdt)


def make_runs(gdt, wdt, K, nextra, seed):
    g = torch.Generator().manual_seed(seed)
    rnd = lambda n, s, dt: (torch.randn(n, generator=g) * s).to(dt)
    theta = [rnd(n, 0.02, gdt) for n in SIZES]
    workers = [[(t.float() + torch.randn(t.numel(), generator=g) * 1e-3).to(wdt) for t in theta] for _ in range(K)]
    mom = [rnd(n, 1e-3, gdt) for n in SIZES]
    extra = [[(t.float() + torch.randn(t.numel(), generator=g) * 3e-3).to(wdt) for t in theta] for _ in range(nextra)]
    plant(theta, workers, mom, extra)
    return theta, workers, mom, extra


class Operands:
    """Two device copies (the fused call's and the composition's) of theta, momentum, K workers
    and K + 2 further destination buffers, with the CPU values beside them."""

    def __init__(self, dev, gdt, wdt, K, seed, shift=0):
        self.K = K
        self.theta, self.workers, self.mom, self.extra = make_runs(gdt, wdt, K, K + 2, seed)
        mk = lambda runs: Buf(runs, dev, shift)
        self.sets = [dict(theta=mk(self.theta), mom=mk(self.mom), w=[mk(w) for w in self.workers],
                          x=[mk(x) for x in self.extra]) for _ in range(2)]

    def reset(self):
        for s in self.sets:
            for b in [s["theta"], s["mom"], *s["w"], *s["x"]]:
                b.reset()

    def live(self, config):
        """(which buffers are destinations: ("w", k) or ("x", k)) for a configuration."""
        K = self.K
        if config == "alias":
            return [("w", k) for k in range(K)]
        if config == "distinct":
            return [("x", k) for k in range(K)]
        if config == "more":                      # nmix > K: the workers themselves and two more
            return [("w", k) for k in range(K)] + [("x", 0), ("x", 1)]
        return [("x", k) for k in range(max(1, K - 1))]     # "fewer": nmix < K (K = 1: one)


def run_case(ops, c, hypers=HYPERS, mixes=MIXES, configs=("alias", "distinct", "more", "fewer")):
    A, B = c.sets
    for has, lr, mu, nest in hypers:
        th_ref, mo_ref, _ = ref.mix_reference(c.theta, c.workers, c.mom, has, lr, mu, nest, None, 1.0)
        for mix in mixes:
            for config in configs:
                c.reset()
                sel = c.live(config)
                pick = lambda S: [S[kind][k].views for kind, k in sel]
                ops.outer_step_list_mix(A["theta"].views, [w.views for w in A["w"]], A["mom"].views, has, lr, mu, nest,
                                        pick(A), mix)
                # the composition on the second copy: the list step, then broadcast_theta -> lerp per run
                ops.outer_step_list(B["theta"].views, [w.views for w in B["w"]], B["mom"].views, has, lr, mu, nest)
                for r, th in enumerate(B["theta"].views):
                    if th.numel() == 0:
                        continue
                    dst = [l[r] for l in pick(B)]
                    if mix == 1.0:
                        for d in dst:
                            d.copy_(th)
                    else:
                        v = torch.empty(th.numel(), dtype=dst[0].dtype, device=th.device)
                        ops.broadcast_theta(th, [v])
                        for d in dst:
                            ops.lerp(mix, d, v, out=d)
                what = f"has={has} lr={lr} mu={mu} nesterov={nest} mix={mix} {config}"
                # the step: the list step's bits, and the oracle's
                assert A["theta"].holds(th_ref) and B["theta"].holds(th_ref), f"theta: {what}"
                assert A["mom"].holds(mo_ref) and B["mom"].holds(mo_ref), f"momentum: {what}"
                # the merge: the restatement's bits and the composition's; everything else untouched
                cpu = {("w", k): c.workers[k] for k in range(c.K)}
                cpu.update({("x", k): c.extra[k] for k in range(len(c.extra))})
                for key, runs in cpu.items():
                    want = [ref.merge_reference(l, t, mix) for l, t in zip(runs, th_ref)] if key in sel else None
                    for S, name in ((A, "fused"), (B, "composition")):
                        assert S[key[0]][key[1]].holds(want), f"{name} {key}: {what}"


@pytest.mark.parametrize("K", [1, 2, 3, 4, 8, 9])
@pytest.mark.parametrize("gdt,wdt", REGIMES)
def test_mix_matrix(dev, ops, gdt, wdt, K):
    """Every compile-time K body and the generic one, the three regimes, fresh and carried
    momentum, Nesterov on and off, the four mixes, and the four destination configurations."""
    run_case(ops, Operands(dev, gdt, wdt, K, seed=100 + K))


def test_bf16_round_up_reaches_the_merge(dev, ops):
    """The planted theta really rounds up to Inf in bf16 under a carried momentum: the case above
    compares an Inf, not a finite value."""
    c = Operands(dev, F32, BF16, 2, seed=7)
    th, _, live = ref.mix_reference(c.theta, c.workers, c.mom, True, 0.7, 0.9, True, c.workers, 0.5)
    r = SIZES.index(513)
    assert torch.isfinite(th[r][4]) and torch.isinf(live[0][r][4])


@pytest.mark.parametrize("gdt,wdt", REGIMES)
def test_mix_unaligned_runs(dev, ops, gdt, wdt):
    """Every run of every operand 4 bytes off a 16-byte boundary: the scalar body."""
    run_case(ops, Operands(dev, gdt, wdt, 3, seed=31, shift=4), hypers=HYPERS[1:3], mixes=[1.0, 0.3])


@pytest.mark.parametrize("gdt,wdt", REGIMES)
def test_overwrite_ignores_the_destination(dev, ops, gdt, wdt):
    """mix == 1.0: destinations planted with NaN, +-Inf and -0 come out as copy_ of theta_new."""
    c = Operands(dev, gdt, wdt, 3, seed=11)
    A = c.sets[0]
    junk = torch.tensor([float("nan"), float("inf"), float("-inf"), -0.0]).to(wdt).to(dev)
    for kind, cnt in (("w", 3), ("x", 2)):
        for k in range(cnt):
            for v in A[kind][k].views:
                v[:] = junk.repeat(v.numel() // 4 + 1)[:v.numel()]
    has, lr, mu, nest = HYPERS[1]
    th_ref, mo_ref, _ = ref.mix_reference(c.theta, c.workers, c.mom, has, lr, mu, nest, None, 1.0)
    # deltas from clean snapshots (the second copy's workers), destinations all planted
    B = c.sets[1]
    live = [w.views for w in A["w"]] + [A["x"][0].views, A["x"][1].views]
    ops.outer_step_list_mix(A["theta"].views, [w.views for w in B["w"]], A["mom"].views, has, lr, mu, nest, live, 1.0)
    assert A["theta"].holds(th_ref) and A["mom"].holds(mo_ref)
    want = [t.to(wdt) for t in th_ref]
    for b in [*A["w"], A["x"][0], A["x"][1]]:
        assert b.holds(want)
        for v, t in zip(b.views, A["theta"].views):
            assert eq(v, torch.empty_like(v).copy_(t))
    assert all(w.holds(None) for w in B["w"])


def test_refusals_launch_nothing(dev, ops):
    from evolutionarydistributedtraining_amd import EdtError
    c = Operands(dev, F32, BF16, 3, seed=3)
    A, B = c.sets
    th, ws, mo = A["theta"].views, [w.views for w in A["w"]], A["mom"].views
    good = [x.views for x in A["x"][:3]]
    args = (True, 0.7, 0.9, True)

    def refused(live, mix, workers=ws):
        with pytest.raises(EdtError):
            ops.outer_step_list_mix(th, workers, mo, *args, live, mix)
        torch.cuda.synchronize()
        for b in [A["theta"], A["mom"], *A["w"], *A["x"]]:
            assert b.holds(None)

    for mix in (0.0, 1.5, float("nan"), -0.25):
        refused(good, mix)
    r = SIZES.index(4097)
    part = [list(v) for v in good]                       # a destination partially overlapping a worker run
    part[0][r] = A["w"][1].buf[A["w"][1].spans[r][0] + 8:A["w"][1].spans[r][0] + 8 + 4097]
    refused(part, 0.5)
    cross = [ws[1], ws[0], ws[2]]                        # live[0] is workers[1]: not the allowed alias
    refused(cross, 0.5)
    twice = [good[0], good[0]]                           # two destinations in one buffer
    refused(twice, 0.5)
    on_theta = [good[0], th]                             # wrong dtype (and theta itself)
    refused(on_theta, 0.5)
    wrong_dt = [[v.float() for v in good[0]]]
    refused(wrong_dt, 0.5)
    short = [[v[:max(0, v.numel() - 1)] for v in good[0]]]
    refused(short, 0.5)
    refused([], 0.5)
    refused(good, 0.5, workers=[ws[k % 3] for k in range(65)])      # K > 64
    # and the same operands are accepted once the fault is gone
    ops.outer_step_list_mix(th, ws, mo, *args, good, 0.5)
    ops.outer_step_list_mix(th, ws, mo, *args, ws, 0.5)


# ------------------------------------------------------------------------------------------
# OuterSync.step_fragment

def small_layout():
    from evolutionarydistributedtraining_amd import ParamLayout
    names, shapes = ["model.embed_tokens.weight"], [(77,)]
    for b in range(5):
        names += [f"model.layers.{b}.attn.weight", f"model.layers.{b}.mlp.weight", f"model.layers.{b}.norm.weight"]
        shapes += [(13, 5), (4099 if b == 2 else 129,), (7,)]
    names += ["model.norm.weight", "lm_head.weight"]
    shapes += [(7,), (77,)]
    return ParamLayout(shapes, names)


def population(lay, gdt, wdt, K, seed):
    g = torch.Generator().manual_seed(seed)
    theta = (torch.randn(lay.total, generator=g) * 0.02).to(gdt)
    workers = [(theta.float() + torch.randn(lay.total, generator=g) * 1e-3).to(wdt) for _ in range(K)]
    return theta, workers


def make_sync(dev, lay, theta, workers, **kw):
    from evolutionarydistributedtraining_amd import OuterSync, ParamArena
    th = ParamArena(lay, theta.dtype, dev, flat=theta.to(dev))
    ws = [ParamArena(lay, w.dtype, dev, flat=w.to(dev)) for w in workers]
    return OuterSync(th, ws, lr=0.7, momentum=0.9, nesterov=True, **kw)


@pytest.mark.parametrize("gdt,wdt", REGIMES)
def test_step_fragment_whole_run(dev, gdt, wdt):
    """P = 3 strided fragments, 7 fragment steps round robin, mix = 0.5: after every step theta,
    the momentum and the worker arenas equal the restatement driven by the same plan; in
    particular a fragment's first step takes buf = grad for itself only, and what lies outside the
    fragment keeps its bits."""
    from evolutionarydistributedtraining_amd import FragmentPlan
    lay = small_layout()
    plan = FragmentPlan.strided(lay, 3)
    theta, workers = population(lay, gdt, wdt, 3, seed=21)
    sync = make_sync(dev, lay, theta, workers, fragments=plan)
    run = ref.FragmentRun(plan, theta, workers, 0.7, 0.9, True)
    g = torch.Generator().manual_seed(22)
    for s in range(7):
        p = s % 3
        inside = torch.zeros(lay.total, dtype=torch.bool)
        for a, n in plan.runs(p):
            inside[a:a + n] = True
        before = [sync.theta.flat.clone(), sync.state.buffer_for(sync.theta.flat).clone()] + [w.flat.clone() for w in sync.workers]
        sync.step_fragment(p, mix=0.5)
        run.step(p, mix=0.5)
        after = [sync.theta.flat, sync.state.momentum] + [w.flat for w in sync.workers]
        for b, a in zip(before, after):
            assert eq(b[~inside.to(dev)], a[~inside.to(dev)]), f"step {s}: outside the fragment"
        assert eq(sync.theta.flat, run.theta), f"step {s}: theta"
        assert eq(sync.state.momentum, run.mom), f"step {s}: momentum"
        for k in range(3):
            assert eq(sync.workers[k].flat, run.workers[k]), f"step {s}: worker {k}"
        assert sync.state.fragment_has_momentum == run.has and sync.state.steps == s + 1
        assert sync.state.has_momentum == (s >= 2)
        # an inner loop: every worker trains on
        for k in range(3):
            d = (torch.randn(lay.total, generator=g) * 1e-3)
            run.workers[k] = (run.workers[k].float() + d).to(wdt)
            sync.workers[k].flat.copy_(run.workers[k])
    assert sync.state.fragment_steps == [3, 2, 2]


@pytest.mark.parametrize("gdt,wdt", REGIMES)
def test_one_fragment_overwrite_is_the_broadcast_step(dev, gdt, wdt):
    """P = 1 and mix = 1.0: a fragment step equals OuterSync.step(broadcast=True) on clones, fresh
    and carried."""
    from evolutionarydistributedtraining_amd import FragmentPlan
    lay = small_layout()
    theta, workers = population(lay, gdt, wdt, 4, seed=41)
    a = make_sync(dev, lay, theta, workers, fragments=FragmentPlan.sequential(lay, 1))
    b = make_sync(dev, lay, theta, workers)
    for s in range(2):
        a.step_fragment(0, mix=1.0)
        b.step(broadcast=True)
        assert eq(a.theta.flat, b.theta.flat) and eq(a.state.momentum, b.state.momentum)
        for wa, wb in zip(a.workers, b.workers):
            assert eq(wa.flat, wb.flat)
        assert a.state.has_momentum and b.state.has_momentum
        for k, (wa, wb) in enumerate(zip(a.workers, b.workers)):
            wa.flat.add_(1e-3 * (k + 1))
            wb.flat.copy_(wa.flat)


def test_snapshots(dev):
    """Capture, perturb the live workers, step: the deltas are the snapshots', the merge targets the
    perturbed live values; merge=False leaves the workers alone."""
    from evolutionarydistributedtraining_amd import EdtError, FragmentPlan
    lay = small_layout()
    plan = FragmentPlan.strided(lay, 2)
    theta, workers = population(lay, F32, BF16, 3, seed=51)
    sync = make_sync(dev, lay, theta, workers, fragments=plan)
    run = ref.FragmentRun(plan, theta, workers, 0.7, 0.9, True)
    snaps = sync.capture_fragment(1)
    assert all(s.numel() == plan.numel(1) and s.dtype == BF16 for s in snaps)
    cpu_snaps = [torch.cat([w[a:a + n] for a, n in plan.runs(1)]) for w in workers]
    assert all(eq(s, c) for s, c in zip(snaps, cpu_snaps))
    g = torch.Generator().manual_seed(52)
    for k in range(3):
        run.workers[k] = (run.workers[k].float() + torch.randn(lay.total, generator=g) * 2e-3).to(BF16)
        sync.workers[k].flat.copy_(run.workers[k])
    sync.step_fragment(1, mix=0.3, snapshots=snaps)
    run.step(1, mix=0.3, snapshots=cpu_snaps)
    assert eq(sync.theta.flat, run.theta) and eq(sync.state.momentum, run.mom)
    assert all(eq(sync.workers[k].flat, run.workers[k]) for k in range(3))
    assert all(eq(s, c) for s, c in zip(snaps, cpu_snaps))
    sync.capture_fragment(0, out=[torch.empty(plan.numel(0), dtype=BF16, device=dev) for _ in range(3)])
    sync.step_fragment(0, merge=False)
    run.step(0, merge=False)
    assert eq(sync.theta.flat, run.theta) and eq(sync.state.momentum, run.mom)
    assert all(eq(sync.workers[k].flat, run.workers[k]) for k in range(3))
    with pytest.raises(EdtError):
        sync.step_fragment(1, snapshots=snaps[:2])
    with pytest.raises(EdtError):
        sync.step_fragment(1, snapshots=[s[:-1] for s in snaps])
    with pytest.raises(EdtError):
        sync.place_arenas()
    with pytest.raises(EdtError):
        make_sync(dev, lay, theta, workers, fragments=plan, cpu_tails=(32, 8))
    with pytest.raises(EdtError):
        make_sync(dev, lay, theta, [workers[k % 3] for k in range(65)], fragments=plan)


def _guarded(dev, guard, seed=61, K=3, regime=(F32, F32)):
    from evolutionarydistributedtraining_amd import FragmentPlan
    lay = small_layout()
    plan = FragmentPlan.strided(lay, 3)
    theta, workers = population(lay, *regime, K, seed=seed)
    return lay, plan, theta, workers


def test_guard_raise_and_other_fragment(dev):
    from evolutionarydistributedtraining_amd.diloco import NonFiniteWorkers, OuterGuard
    lay, plan, theta, workers = _guarded(dev, None)
    a0, _ = plan.runs(1)[0]
    workers[1][a0 + 3] = float("nan")                     # in fragment 1, worker 1
    sync = make_sync(dev, lay, theta, workers, fragments=plan, guard=OuterGuard(on_nonfinite="raise"))
    run = ref.FragmentRun(plan, theta, workers, 0.7, 0.9, True)
    before = [sync.theta.flat.clone()] + [w.flat.clone() for w in sync.workers]
    with pytest.raises(NonFiniteWorkers):
        sync.step_fragment(1, mix=0.5)
    assert eq(sync.theta.flat, before[0]) and all(eq(w.flat, b) for w, b in zip(sync.workers, before[1:]))
    assert sync.state.momentum is None or not sync.state.momentum.any()
    assert sync.state.steps == 0 and sync.state.fragment_has_momentum == [False] * 3
    # the NaN lies in another fragment: fragment 0 steps as if it were not there
    sync.step_fragment(0, mix=0.5)
    run.step(0, mix=0.5)
    assert eq(sync.theta.flat, run.theta) and eq(sync.state.momentum, run.mom)
    assert all(eq(sync.workers[k].flat, run.workers[k]) for k in range(3))
    assert sync.last_stats["dropped"] == [] and sync.last_stats["clip_coef"] == 1.0


def test_guard_drop_merges_into_the_dropped_worker(dev):
    from evolutionarydistributedtraining_amd.diloco import OuterGuard
    lay, plan, theta, workers = _guarded(dev, None)
    a0, _ = plan.runs(1)[0]
    workers[1][a0 + 3] = float("nan")
    sync = make_sync(dev, lay, theta, workers, fragments=plan, guard=OuterGuard(on_nonfinite="drop"))
    sync.step_fragment(1, mix=0.5)
    assert sync.last_stats["dropped"] == [1]
    # the restatement: the deltas of workers 0 and 2, every worker a destination
    th, mo = theta.clone(), torch.zeros_like(theta)
    ws = [w.clone() for w in workers]
    for a, n in plan.runs(1):
        ref.step_run(th[a:a + n], [workers[0][a:a + n].clone(), workers[2][a:a + n].clone()], mo[a:a + n], False, 0.7, 0.9, True)
        for w in ws:
            w[a:a + n] = ref.merge_reference(w[a:a + n], th[a:a + n], 0.5)
    assert eq(sync.theta.flat, th) and eq(sync.state.momentum, mo)
    assert all(eq(sync.workers[k].flat, ws[k]) for k in range(3))
    assert torch.isnan(sync.workers[1].flat[a0 + 3]) and torch.isfinite(sync.workers[1].flat[a0 + 2])


@pytest.mark.parametrize("mix", [0.5, 1.0])
def test_guard_clip_is_the_scaled_composition(dev, ops, mix):
    from evolutionarydistributedtraining_amd.diloco import OuterGuard
    lay, plan, theta, workers = _guarded(dev, None, regime=(F32, BF16))
    sync = make_sync(dev, lay, theta, workers, fragments=plan, guard=OuterGuard(max_grad_norm=1e-3))
    th = theta.to(dev)
    mo = torch.zeros_like(th)
    ws = [w.to(dev) for w in workers]
    sync.step_fragment(2, mix=mix)
    clip = sync.last_stats["clip_coef"]
    assert 0.0 < clip < 1.0
    ops.outer_step_list_scaled(plan.views(2, th), [plan.views(2, w) for w in ws], plan.views(2, mo), False, 0.7, 0.9,
                               True, clip)
    for r, t in enumerate(plan.views(2, th)):
        v = torch.empty(t.numel(), dtype=BF16, device=dev)
        ops.broadcast_theta(t, [v])
        for w in ws:
            d = plan.views(2, w)[r]
            if mix == 1.0:
                d.copy_(v)
            else:
                ops.lerp(mix, d, v, out=d)
    assert eq(sync.theta.flat, th) and eq(sync.state.momentum, mo)
    assert all(eq(sync.workers[k].flat, ws[k]) for k in range(3))
    assert not eq(sync.theta.flat, theta.to(dev))


def test_drop_in_equals_the_arena_form(dev):
    """outer_step_fragment over separately allocated tensors equals step_fragment on packed clones
    (every size a multiple of 8, the documented index rule), with snapshots and distinct live lists."""
    from evolutionarydistributedtraining_amd import FragmentPlan, ParamLayout, outer_step_fragment
    names = ["embed.weight"] + [f"layers.{b}.{x}.weight" for b in range(4) for x in ("attn", "mlp")] + ["head.weight"]
    lay = ParamLayout([(64,)] + [(8, 9), (4104,)] * 4 + [(64,)], names)
    plan = FragmentPlan.strided(lay, 2)
    theta, workers = population(lay, F32, BF16, 2, seed=71)
    sync = make_sync(dev, lay, theta, workers, fragments=plan)
    split = lambda flat: [v.clone().to(dev) for v in lay.views(flat)]
    base, wl = split(theta), [split(w) for w in workers]
    state = None
    for s, p in enumerate((1, 0, 1)):
        snaps = sync.capture_fragment(p)
        snap_l = [[wl[k][i].clone() for i in plan.tensors(p)] for k in range(2)]
        for k in range(2):
            sync.workers[k].flat.add_(1e-3)
            for t in wl[k]:
                t.add_(1e-3)
        sync.step_fragment(p, mix=0.3, snapshots=snaps)
        state = outer_step_fragment(base, wl, state, plan, p, mix=0.3, snapshot_params=snap_l, lr=0.7, momentum=0.9,
                                    nesterov=True)
        cat = lambda ts: torch.cat([t.reshape(-1) for t in ts])
        assert eq(cat(base), sync.theta.flat) and eq(state.momentum, sync.state.momentum), f"step {s}"
        for k in range(2):
            assert eq(cat(wl[k]), sync.workers[k].flat), f"step {s}: worker {k}"
    assert state.fragment_steps == [1, 2] and state.has_momentum
