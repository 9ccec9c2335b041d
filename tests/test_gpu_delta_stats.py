"""edt_delta_stats, edt_outer_step_scaled and OuterSync(guard=...) on the device, against the CPU
restatement (tests/stats_reference.py): the statistics' rows and counts bit for bit, their
coherence with the fused step, the masking of what is not finite, the scaled step against its
composition, and the guarded step's policies."""
import numpy as np
import pytest
import torch

from tests import stats_reference as R

pytestmark = pytest.mark.gpu

F32, BF16 = torch.float32, torch.bfloat16
REGIMES = [(F32, F32), (F32, BF16), (BF16, BF16)]
RID = ["f32-f32", "f32-bf16", "bf16-bf16"]
SIZES = [1, 7, 8, 511, 512, 513, 65536, 65537]
LAYOUT = [0, 5, 70006, 70518]          # odd first segment, chunk starts off 8, a segment > one chunk


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a HIP device")
    return torch.device("cuda", 0)


def _ops():
    from evolutionarydistributedtraining_amd import ops
    return ops


def _gpu_rows(theta, workers, offsets, dev):
    ops = _ops()
    plan = ops.make_slerp_plan(list(offsets), dev)
    rows = ops.delta_stats(theta.to(dev), [w.to(dev) for w in workers], plan)
    return rows.cpu().numpy(), plan


def _check(theta, workers, offsets, dev, oracle, what):
    got, plan = _gpu_rows(theta, workers, offsets, dev)
    chunks = R.make_chunks(offsets)
    assert (plan.chunks_host == chunks).all()
    want, _ = R.stats_rows(theta, workers, chunks, oracle)
    K = len(workers)
    if K > 8:
        assert (got[:, K + 1:2 * K + 1] == 0).all(), what
    assert R.same_bits(got, want), (what, np.argwhere(got != want)[:5], got.shape)


@pytest.mark.parametrize("K", [1, 2, 3, 8, 9, 64])
@pytest.mark.parametrize("gdt,wdt", REGIMES, ids=RID)
def test_rows_bit_exact(dev, oracle, gdt, wdt, K):
    for n in SIZES:
        theta, workers = R.operands(n, K, gdt, wdt, seed=1000 + n + K)
        _check(theta, workers, [0, n], dev, oracle, (n, K))


@pytest.mark.parametrize("K", [3, 8, 9])
@pytest.mark.parametrize("gdt,wdt", REGIMES, ids=RID)
def test_three_segments(dev, oracle, gdt, wdt, K):
    theta, workers = R.operands(LAYOUT[-1], K, gdt, wdt, seed=7 + K)
    _check(theta, workers, LAYOUT, dev, oracle, ("layout", K))


@pytest.mark.parametrize("K", [3, 9])
@pytest.mark.parametrize("gdt,wdt", REGIMES, ids=RID)
def test_offset_view_takes_scalar_path(dev, oracle, gdt, wdt, K):
    ops = _ops()
    n = 70518
    theta, workers = R.operands(n, K, gdt, wdt, seed=99 + K)
    plan = ops.make_slerp_plan(LAYOUT, dev)
    want, _ = R.stats_rows(theta, workers, R.make_chunks(LAYOUT), oracle)
    # theta off a 16-byte boundary, then one worker, then all
    for shift_theta, shifted in ((True, ()), (False, (K - 1,)), (True, tuple(range(K)))):
        def put(t, shift):
            buf = torch.empty(n + 1, dtype=t.dtype, device=dev)
            v = buf[1:] if shift else buf[:n]
            v.copy_(t)
            assert (v.data_ptr() % 16 != 0) == shift
            return v
        th = put(theta, shift_theta)
        ws = [put(w, k in shifted) for k, w in enumerate(workers)]
        got = ops.delta_stats(th, ws, plan).cpu().numpy()
        assert R.same_bits(got, want), (shift_theta, shifted)


@pytest.mark.parametrize("K", [3, 8])
@pytest.mark.parametrize("gdt", [F32, BF16], ids=["f32", "bf16"])
def test_coherent_with_the_step(dev, oracle, gdt, K):
    """theta = 0, lr = 1, mu = 0: the fused step's new theta is m, and the arena total of S_mm is
    the canonical sum of theta'^2."""
    ops = _ops()
    from evolutionarydistributedtraining_amd.diloco import stats_totals
    n = LAYOUT[-1]
    _, workers = R.operands(n, K, gdt, BF16 if gdt == BF16 else F32, seed=5 + K)
    theta = torch.zeros(n, dtype=gdt)
    got, plan = _gpu_rows(theta, workers, LAYOUT, dev)
    th = theta.to(dev)
    ops.outer_step(th, [w.to(dev) for w in workers], None, False, 1.0, 0.0, False)
    _, m = R.deltas_and_mean(theta, workers)
    assert torch.equal(th.cpu().float(), m.float())           # as values: 0 - (-0) is +0 in the step
    sq = oracle.canonical_chunk_sums(th.cpu(), th.cpu(), R.make_chunks(LAYOUT))[:, 0]
    assert R.same_bits(got[:, 0], sq)
    assert stats_totals(got, K)["S_mm"] == float(np.cumsum(sq)[-1])


@pytest.mark.parametrize("gdt,wdt", REGIMES, ids=RID)
def test_masking(dev, oracle, gdt, wdt):
    K, n = 3, LAYOUT[-1]
    theta, workers = R.operands(n, K, gdt, wdt, seed=31)
    chunks = R.make_chunks(LAYOUT)
    spots = [0, n - 1, 511, 512, 5 + 65535, 5 + 65536]       # first, last, tile edge, chunk edge
    vals = [float("nan"), float("inf"), float("-inf")]
    for j, i in enumerate(spots):
        workers[1][i] = vals[j % 3]
    got, _ = _gpu_rows(theta, workers, LAYOUT, dev)
    want, _ = R.stats_rows(theta, workers, chunks, oracle)
    assert R.same_bits(got, want)
    nf = got[:, 2 * K + 2:].sum(axis=0)
    assert nf.tolist() == [0, len(spots), 0]
    assert got[:, 2 * K + 1].sum() == len(spots)             # an Inf or NaN delta makes the mean one
    per_chunk = [sum(1 for i in spots if a <= i < a + ln) for a, ln, _ in chunks]
    assert got[:, 2 * K + 3].tolist() == per_chunk
    # theta holding a NaN flags every worker at that element
    theta2, workers2 = R.operands(n, K, gdt, wdt, seed=32)
    theta2[70005] = float("nan")
    got2, _ = _gpu_rows(theta2, workers2, LAYOUT, dev)
    want2, _ = R.stats_rows(theta2, workers2, chunks, oracle)
    assert R.same_bits(got2, want2)
    assert got2[:, 2 * K + 2:].sum(axis=0).tolist() == [1, 1, 1] and got2[:, 2 * K + 1].sum() == 1


def _bits(t):
    return t.cpu().view(torch.int16 if t.dtype == BF16 else torch.int32)


@pytest.mark.parametrize("K", [1, 3, 8, 33])
@pytest.mark.parametrize("gdt,wdt", REGIMES, ids=RID)
def test_scaled_step_composition(dev, oracle, gdt, wdt, K):
    ops = _ops()
    lr, mu, nesterov = 0.7, 0.9, True
    for n in (1, 513, 100003):
        for c in (0.0, 0.37, 1.0):
            theta, _ = R.operands(n, K, gdt, wdt, seed=n + K)
            ref_t, ref_m = theta.clone(), torch.zeros_like(theta)
            plain_t, plain_m = theta.to(dev), torch.zeros(n, dtype=gdt, device=dev)
            dev_t, dev_m = theta.to(dev), torch.zeros(n, dtype=gdt, device=dev)
            for gen in range(2):                       # the second generation carries the momentum
                _, workers = R.operands(n, K, gdt, wdt, seed=10 * n + K + gen)
                workers = [(ref_t.float() + (w.float() - theta.float())).to(wdt) for w in workers]
                _, m = R.deltas_and_mean(ref_t, workers)
                if gdt == F32:                         # fp32 master: the oracle's partial sum is m itself
                    acc = torch.zeros(n, dtype=F32)
                    oracle.delta_partial(ref_t, workers, K, acc)
                    assert torch.equal(acc, m)
                scaled = (m.float() * torch.tensor(c, dtype=F32)).to(gdt)
                oracle.sgd_apply(ref_t, scaled.float().contiguous(), ref_m, gen > 0, lr, mu, nesterov)
                ws = [w.to(dev) for w in workers]
                ops.outer_step_scaled(dev_t, ws, dev_m, gen > 0, lr, mu, nesterov, c)
                assert torch.equal(_bits(dev_t), _bits(ref_t)), (n, c, gen, "theta")
                assert torch.equal(_bits(dev_m), _bits(ref_m)), (n, c, gen, "momentum")
                if c == 1.0:
                    ops.outer_step(plain_t, ws, plain_m, gen > 0, lr, mu, nesterov)
                    assert torch.equal(_bits(dev_t), _bits(plain_t)) and torch.equal(_bits(dev_m), _bits(plain_m))


def test_scaled_step_honours_tail_bits(dev):
    ops = _ops()
    n, K = 100003, 3
    theta, workers = R.operands(n, K, BF16, BF16, seed=77)
    gen = torch.Generator().manual_seed(3)
    tail = torch.randint(0, 256, ((n + 7) // 8,), dtype=torch.uint8, generator=gen).to(dev)
    ws = [w.to(dev) for w in workers]
    a_t, a_m = theta.to(dev), (torch.randn(n, generator=gen) * 0.01).to(BF16).to(dev)
    b_t, b_m = a_t.clone(), a_m.clone()
    c_t, c_m = a_t.clone(), a_m.clone()
    ops.outer_step(a_t, ws, a_m, True, 0.7, 0.9, True, tail_bits=tail)
    ops.outer_step_scaled(b_t, ws, b_m, True, 0.7, 0.9, True, 1.0, tail_bits=tail)
    ops.outer_step(c_t, ws, c_m, True, 0.7, 0.9, True)
    assert torch.equal(_bits(a_t), _bits(b_t)) and torch.equal(_bits(a_m), _bits(b_m))
    assert not torch.equal(_bits(a_t), _bits(c_t))          # the tail bits changed something


# ---- OuterSync(guard=...) ---------------------------------------------------------------------

def _sync(dev, K, gdt=F32, wdt=F32, seed=0, shapes=((5,), (70001,), (512,)), **kw):
    from evolutionarydistributedtraining_amd.diloco import OuterSync
    from evolutionarydistributedtraining_amd.params import ParamArena, ParamLayout
    layout = ParamLayout([torch.Size(s) for s in shapes])
    theta, workers = R.operands(layout.total, K, gdt, wdt, seed=seed)
    th = ParamArena(layout, gdt, dev, theta.to(dev))
    ws = [ParamArena(layout, wdt, dev, w.to(dev)) for w in workers]
    return OuterSync(th, ws, **kw), theta, workers


def test_guard_unclipped_is_the_plain_step(dev):
    from evolutionarydistributedtraining_amd.diloco import OuterGuard
    for gdt, wdt in REGIMES:
        a, _, _ = _sync(dev, 8, gdt, wdt, seed=4)
        b, _, _ = _sync(dev, 8, gdt, wdt, seed=4, guard=OuterGuard(max_grad_norm=1e9, per_tensor=True))
        for _ in range(2):
            a.step()
            b.step()
        assert torch.equal(_bits(a.theta.flat), _bits(b.theta.flat))
        assert torch.equal(_bits(a.state.momentum), _bits(b.state.momentum))
        st = b.last_stats
        assert st["clip_coef"] == 1.0 and st["dropped"] == [] and len(st["worker_norms"]) == 8
        assert len(st["cos_to_mean"]) == 8 and len(st["per_tensor"]) == 3 and st["grad_norm"] > 0


def test_guard_clips_to_max_norm(dev):
    from evolutionarydistributedtraining_amd.diloco import OuterGuard
    max_norm = 0.05
    s, theta, _ = _sync(dev, 3, seed=8, lr=1.0, momentum=0.0, nesterov=False,
                        guard=OuterGuard(max_grad_norm=max_norm))
    s.step()
    st = s.last_stats
    assert st["grad_norm"] > max_norm and 0 < st["clip_coef"] < 1
    applied = (s.theta.flat.cpu().double() - theta.double())
    # theta' - theta is the clipped gradient up to the fp32 rounding of theta' (half an ulp of each
    # element of theta, |theta| < 4: 2^-22 per element at the most, root-sum-squared over n)
    slack = (2.0 ** -22) * (theta.numel() ** 0.5)
    assert float(applied.norm()) <= max_norm + slack
    assert float(applied.norm()) >= 0.9 * max_norm


def test_guard_raise_leaves_state_untouched(dev):
    from evolutionarydistributedtraining_amd.diloco import NonFiniteWorkers, OuterGuard
    s, _, _ = _sync(dev, 3, seed=9, guard=OuterGuard())
    s.step()                                                    # a momentum to protect
    t0, m0 = s.theta.flat.clone(), s.state.momentum.clone()
    s.workers[2].flat[17] = float("inf")
    with pytest.raises(NonFiniteWorkers) as e:
        s.step()
    assert e.value.nonfinite == [0, 0, 1] and e.value.nonfinite_mean == 1
    assert torch.equal(_bits(s.theta.flat), _bits(t0)) and torch.equal(_bits(s.state.momentum), _bits(m0))
    assert s.state.steps == 1


def test_guard_drop_steps_over_survivors_and_broadcasts(dev):
    from evolutionarydistributedtraining_amd.diloco import NonFiniteWorkers, OuterGuard, OuterSync
    for max_norm in (None, 0.05):                               # the fused and the scaled form
        g = OuterGuard(on_nonfinite="drop", max_grad_norm=max_norm)
        s, _, _ = _sync(dev, 4, F32, BF16, seed=11, guard=g)
        s.workers[1].flat[3] = float("nan")
        ref = OuterSync(type(s.theta)(s.theta.layout, F32, dev, s.theta.flat.clone()),
                        [type(w)(w.layout, BF16, dev, w.flat.clone()) for k, w in enumerate(s.workers) if k != 1],
                        guard=OuterGuard(max_grad_norm=max_norm))
        s.step(broadcast=True)
        ref.step()
        assert s.last_stats["dropped"] == [1] and s.last_stats["nonfinite"] == [0, 1, 0, 0]
        assert s.last_stats["grad_norm"] == ref.last_stats["grad_norm"]
        assert (s.last_stats["clip_coef"] < 1) == (max_norm is not None)
        assert torch.equal(_bits(s.theta.flat), _bits(ref.theta.flat))
        assert torch.equal(_bits(s.state.momentum), _bits(ref.state.momentum))
        want = s.theta.flat.to(BF16)
        for w in s.workers:                                     # the dropped one rejoins too
            assert torch.equal(_bits(w.flat), _bits(want))
    s, _, _ = _sync(dev, 3, seed=12, guard=OuterGuard(on_nonfinite="drop", min_workers=3))
    s.workers[0].flat[0] = float("-inf")
    t0 = s.theta.flat.clone()
    with pytest.raises(NonFiniteWorkers):
        s.step()
    assert torch.equal(_bits(s.theta.flat), _bits(t0))


def test_guard_refuses_more_than_64_workers(dev):
    from evolutionarydistributedtraining_amd._lib import EdtError
    from evolutionarydistributedtraining_amd.diloco import OuterGuard
    with pytest.raises(EdtError):
        _sync(dev, 65, shapes=((64,),), guard=OuterGuard())


def test_drop_in_outer_step_with_guard_packs_lists(dev):
    from evolutionarydistributedtraining_amd.diloco import OuterGuard, outer_step
    gen = torch.Generator().manual_seed(2)
    base = [torch.randn(s, generator=gen).to(dev) for s in ((3, 5), (700,))]
    workers = [[b + 0.01 * torch.randn(b.shape, generator=gen).to(dev) for b in base] for _ in range(3)]
    base2 = [b.clone() for b in base]
    st = outer_step(base, workers, guard=OuterGuard(max_grad_norm=1e9))
    st2 = outer_step(base2, workers)
    assert st.last_stats["clip_coef"] == 1.0 and st2.last_stats is None
    for a, b in zip(base, base2):
        assert torch.equal(a, b)
