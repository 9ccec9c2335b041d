"""The guard over separate tensors on the device: edt_delta_stats_list against the per-tensor CPU
restatement (tests/stats_reference.py) bit for bit — every K body, mixed alignment, masking — and
against the arena form; edt_outer_step_list_scaled against the flat scaled step on packed clones;
and diloco.outer_step(guard=...) on lists that are not arena views, which must neither pack nor,
on a refusal, write anything."""
import functools

import numpy as np
import pytest
import torch

from tests import stats_reference as R

pytestmark = pytest.mark.gpu

F32, BF16 = torch.float32, torch.bfloat16
REGIMES = [(F32, F32), (F32, BF16), (BF16, BF16)]
RID = ["f32-f32", "f32-bf16", "bf16-bf16"]
# empty | below one vector | a tail only | one vector | vector + tail | a tile + 1 | exactly one
# chunk | a second chunk of one element | two chunks with a ragged tail
SIZES = [0, 1, 7, 8, 15, 513, 65536, 65537, 70001]
SIZES8 = [8, 512, 65536, 65544, 70000]          # every size a multiple of 8


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a HIP device")
    return torch.device("cuda", 0)


def _ops():
    from evolutionarydistributedtraining_amd import ops
    return ops


def _bits(t):
    return t.cpu().view(torch.int16 if t.dtype == BF16 else torch.int32)


def _offsets(sizes):
    return [0] + np.cumsum(sizes).tolist()


@functools.lru_cache(maxsize=None)
def _population(gdt, wdt, K, seed, sizes=tuple(SIZES)):
    """(thetas[T], workers[K][T]) on the CPU, stats_reference.operands per tensor. Shared and never
    written: a test that plants values clones first."""
    thetas, workers = [], [[] for _ in range(K)]
    for t, n in enumerate(sizes):
        th, ws = R.operands(n, K, gdt, wdt, seed=seed + 17 * t)
        thetas.append(th)
        for k in range(K):
            workers[k].append(ws[k])
    return thetas, workers


def _list_chunks(sizes):
    """The relative per-tensor table: tensor t's one-segment table with segment index t."""
    return np.concatenate([R.make_chunks([0, n]) + [0, 0, t] for t, n in enumerate(sizes) if n]).reshape(-1, 3)


def _restate(thetas, workers, oracle):
    """The restatement: stats_rows per tensor as an arena of one segment, concatenated in tensor
    order. Returns (rows, first-row index per tensor [T + 1])."""
    rows, first = [], [0]
    for t, th in enumerate(thetas):
        if th.numel():
            r, _ = R.stats_rows(th, [w[t] for w in workers], R.make_chunks([0, th.numel()]), oracle)
            rows.append(r)
        first.append(first[-1] + (len(rows[-1]) if th.numel() else 0))
    return np.concatenate(rows), first


_WANT = {}


def _want(oracle, gdt, wdt, K, seed, sizes=tuple(SIZES)):
    key = (gdt, wdt, K, seed, sizes)
    if key not in _WANT:
        _WANT[key] = _restate(*_population(gdt, wdt, K, seed, sizes), oracle)
    return _WANT[key]


def _to(dev, thetas, workers, off_theta=(), off_worker=None):
    """Device copies. off_theta: tensor indices of theta placed off a 16-byte boundary (a view at
    element 1 of a larger buffer); off_worker: {k: tensor indices} for the workers."""
    def put(t, shift):
        buf = torch.empty(t.numel() + 1, dtype=t.dtype, device=dev)
        v = buf[1:] if shift else buf[:t.numel()]
        v.copy_(t)
        if t.numel():
            assert (v.data_ptr() % 16 != 0) == shift
        return v
    off_worker = off_worker or {}
    return ([put(t, i in off_theta) for i, t in enumerate(thetas)],
            [[put(t, i in off_worker.get(k, ())) for i, t in enumerate(w)] for k, w in enumerate(workers)])


def _plan(dev, sizes):
    return _ops().make_slerp_plan(_offsets(sizes), dev, relative=True)


def _gpu_rows(dev, thetas, workers, **off):
    th, ws = _to(dev, thetas, workers, **off)
    return _ops().delta_stats_list(th, ws, _plan(dev, [t.numel() for t in thetas])).cpu().numpy()


# ---- 1. rows against the per-tensor restatement ---------------------------------------------------

@pytest.mark.parametrize("K", [1, 2, 3, 8, 9, 64])
@pytest.mark.parametrize("gdt,wdt", REGIMES, ids=RID)
def test_rows_equal_the_per_tensor_restatement(dev, oracle, gdt, wdt, K):
    thetas, workers = _population(gdt, wdt, K, 500 + K)
    want, _ = _want(oracle, gdt, wdt, K, 500 + K)
    plan = _plan(dev, SIZES)
    assert plan.relative and plan.nseg == len(SIZES)
    assert (plan.chunks_host == _list_chunks(SIZES)).all()
    got = _gpu_rows(dev, thetas, workers)
    assert got.shape == (plan.nchunks, 3 * K + 2)
    if K > 8:
        assert (got[:, K + 1:2 * K + 1] == 0).all()
    assert R.same_bits(got, want), np.argwhere(got != want)[:5]


# ---- 2. mixed alignment ---------------------------------------------------------------------------

@pytest.mark.parametrize("K", [3, 9])
@pytest.mark.parametrize("gdt,wdt", REGIMES, ids=RID)
def test_mixed_alignment_gives_the_same_bits(dev, oracle, gdt, wdt, K):
    thetas, workers = _population(gdt, wdt, K, 900 + K)
    want, _ = _want(oracle, gdt, wdt, K, 900 + K)
    aligned = _gpu_rows(dev, thetas, workers)
    assert R.same_bits(aligned, want)
    every = tuple(range(len(SIZES)))
    for off in (dict(off_theta=(5,)), dict(off_worker={K - 1: (3, 8)}),
                dict(off_theta=every, off_worker={k: every for k in range(K)})):
        got = _gpu_rows(dev, thetas, workers, **off)
        assert R.same_bits(got, aligned), (off, np.argwhere(got != aligned)[:5])


# ---- 3. masking and counts ------------------------------------------------------------------------

@pytest.mark.parametrize("gdt,wdt", REGIMES, ids=RID)
def test_masking_and_counts_per_tensor(dev, oracle, gdt, wdt):
    K = 3
    thetas, workers = _population(gdt, wdt, K, 40)
    thetas = [t.clone() for t in thetas]
    workers = [[t.clone() for t in w] for w in workers]
    workers[1][5][0] = float("nan")                 # the first element of a tensor
    workers[1][8][SIZES[8] - 1] = float("inf")      # the last element of another
    workers[1][7][65536] = float("-inf")            # the lone element of a second chunk
    thetas[6][100] = 3e38                           # finite operands whose delta overflows theta's dtype
    workers[0][6][100] = -3e38
    want, first = _restate(thetas, workers, oracle)
    got = _gpu_rows(dev, thetas, workers)
    assert R.same_bits(got, want), np.argwhere(got != want)[:5]
    per_tensor = np.asarray([got[a:b, 2 * K + 1:].sum(axis=0) for a, b in zip(first[:-1], first[1:])])
    expect = np.zeros((len(SIZES), K + 1))          # columns: the mean, then the K workers
    expect[5, [0, 2]] = 1
    expect[8, [0, 2]] = 1
    expect[7, [0, 2]] = 1
    expect[6, [0, 1]] = 1
    assert (per_tensor == expect).all(), per_tensor
    assert got[first[7] + 1, 2 * K + 3] == 1 and got[first[7], 2 * K + 3] == 0   # the second chunk's own row


# ---- 4. against the arena form --------------------------------------------------------------------

@pytest.mark.parametrize("gdt,wdt", REGIMES, ids=RID)
def test_sizes_of_multiples_of_8_equal_the_packed_arena(dev, gdt, wdt):
    ops = _ops()
    K = 3
    thetas, workers = _population(gdt, wdt, K, 60, tuple(SIZES8))
    got = _gpu_rows(dev, thetas, workers)
    aplan = ops.make_slerp_plan(_offsets(SIZES8), dev)
    arena = ops.delta_stats(torch.cat(thetas).to(dev), [torch.cat(w).to(dev) for w in workers], aplan).cpu().numpy()
    assert R.same_bits(got, arena), np.argwhere(got != arena)[:5]


@pytest.mark.parametrize("gdt,wdt", REGIMES, ids=RID)
def test_ragged_sizes_agree_with_the_arena_in_total(dev, gdt, wdt):
    """Ragged sizes put the arena's chunk starts off 8, so its lanes hold other elements: the same
    products summed in another fp64 order. DESIGN §3's bound, per column: 2 n 2^-53 relative."""
    ops = _ops()
    K = 3
    thetas, workers = _population(gdt, wdt, K, 500 + K)
    got = _gpu_rows(dev, thetas, workers)
    aplan = ops.make_slerp_plan(_offsets(SIZES), dev)
    arena = ops.delta_stats(torch.cat(thetas).to(dev), [torch.cat(w).to(dev) for w in workers], aplan).cpu().numpy()
    n = sum(SIZES)
    a, b = np.cumsum(got, axis=0)[-1], np.cumsum(arena, axis=0)[-1]
    rel = np.abs(a - b)[:2 * K + 1] / np.abs(b)[:2 * K + 1]            # the sums (the counts are 0)
    print("largest relative difference of a column total:", rel.max(), "bound", 2 * n * 2.0 ** -53,
          "columns differing:", int((a != b).sum()))
    assert (np.abs(a - b) <= 2 * n * 2.0 ** -53 * np.abs(b)).all(), rel
    assert (a[2 * K + 1:] == 0).all() and (b[2 * K + 1:] == 0).all()


# ---- 5. the scaled list step ----------------------------------------------------------------------

def _fresh_workers(gdt, wdt, K, seed, base):
    """Workers around the current theta `base` (CPU list), as a new generation trains them."""
    thetas0, workers = _population(gdt, wdt, K, seed)
    return [[(b.float() + (w.float() - t0.float())).to(wdt) for b, w, t0 in zip(base, wk, thetas0)] for wk in workers]


@pytest.mark.parametrize("nesterov", [True, False], ids=["nesterov", "plain"])
@pytest.mark.parametrize("K", [1, 3, 8, 33])
@pytest.mark.parametrize("gdt,wdt", REGIMES, ids=RID)
def test_scaled_list_step_equals_the_flat_scaled_step(dev, gdt, wdt, K, nesterov):
    ops = _ops()
    lr, mu = 0.7, 0.9
    thetas, _ = _population(gdt, wdt, K, 200 + K)
    for c in (0.37, 1.0):
        l_t = [t.to(dev) for t in thetas]
        l_m = [torch.zeros_like(t) for t in l_t]
        f_t, f_m = torch.cat(l_t), torch.cat(l_m)
        p_t, p_m = [t.clone() for t in l_t], [t.clone() for t in l_m]
        for gen in range(2):                            # fresh, then carried momentum
            ws = _fresh_workers(gdt, wdt, K, 300 + K + gen, [t.cpu() for t in l_t])
            ws = [[t.to(dev) for t in w] for w in ws]
            ops.outer_step_list_scaled(l_t, ws, l_m, gen > 0, lr, mu, nesterov, c)
            ops.outer_step_scaled(f_t, [torch.cat(w) for w in ws], f_m, gen > 0, lr, mu, nesterov, c)
            assert torch.equal(_bits(torch.cat(l_t)), _bits(f_t)), (c, gen, "theta")
            assert torch.equal(_bits(torch.cat(l_m)), _bits(f_m)), (c, gen, "momentum")
            if c == 1.0:
                ops.outer_step_list(p_t, ws, p_m, gen > 0, lr, mu, nesterov)
                assert torch.equal(_bits(torch.cat(l_t)), _bits(torch.cat(p_t)))
                assert torch.equal(_bits(torch.cat(l_m)), _bits(torch.cat(p_m)))


def test_scaled_list_step_honours_tail_masks(dev):
    from evolutionarydistributedtraining_amd.diloco import _tail_bits
    ops = _ops()
    K = 3
    thetas, workers = _population(BF16, BF16, K, 77)
    tails = _tail_bits((32, 8), SIZES, dev, per_tensor=True)
    arena_mask = _tail_bits((32, 8), SIZES, dev)
    gen = torch.Generator().manual_seed(5)
    l_t = [t.to(dev) for t in thetas]
    l_m = [(torch.randn(t.numel(), generator=gen) * 0.01).to(BF16).to(dev) for t in thetas]
    ws = [[t.to(dev) for t in w] for w in workers]
    f_t, f_m = torch.cat(l_t), torch.cat(l_m)
    n_t, n_m = [t.clone() for t in l_t], [t.clone() for t in l_m]
    ops.outer_step_list_scaled(l_t, ws, l_m, True, 0.7, 0.9, True, 0.37, tails=tails)
    ops.outer_step_scaled(f_t, [torch.cat(w) for w in ws], f_m, True, 0.7, 0.9, True, 0.37, tail_bits=arena_mask)
    ops.outer_step_list_scaled(n_t, ws, n_m, True, 0.7, 0.9, True, 0.37)
    assert torch.equal(_bits(torch.cat(l_t)), _bits(f_t)) and torch.equal(_bits(torch.cat(l_m)), _bits(f_m))
    assert not torch.equal(_bits(torch.cat(l_t)), _bits(torch.cat(n_t)))     # the masks changed something


def test_scaled_list_step_refuses_scales_outside_0_1(dev):
    from evolutionarydistributedtraining_amd._lib import EdtError
    ops = _ops()
    thetas, workers = _population(F32, F32, 3, 200 + 3)
    l_t = [t.to(dev) for t in thetas]
    ws = [[t.to(dev) for t in w] for w in workers]
    before = [t.clone() for t in l_t]
    for bad in (-0.1, 1.5, float("nan"), float("inf")):
        with pytest.raises(EdtError):
            ops.outer_step_list_scaled(l_t, ws, None, False, 0.7, 0.0, False, bad)
    for a, b in zip(l_t, before):
        assert torch.equal(_bits(a), _bits(b))


# ---- 6.-9. diloco.outer_step(guard=...) on separate tensors ---------------------------------------

@pytest.fixture()
def no_packing(monkeypatch):
    from evolutionarydistributedtraining_amd import diloco

    def refuse(*a, **k):
        raise AssertionError("a guarded step over separate tensors must not pack")
    monkeypatch.setattr(diloco, "pack", refuse)
    monkeypatch.setattr(diloco, "unpack_", refuse)


def _device_lists(dev, gdt, wdt, K, seed):
    thetas, workers = _population(gdt, wdt, K, seed)
    return [t.to(dev) for t in thetas], [[t.to(dev) for t in w] for w in workers]


@pytest.mark.parametrize("gdt,wdt", REGIMES, ids=RID)
def test_guarded_drop_in_step_runs_on_the_lists(dev, no_packing, gdt, wdt):
    from evolutionarydistributedtraining_amd import diloco
    ops = _ops()
    K, n = 3, sum(SIZES)
    base, ws = _device_lists(dev, gdt, wdt, K, 700)
    plain = [t.clone() for t in base]
    # unclipped: the unguarded list step, bit for bit, over two generations
    st = st2 = None
    for gen in range(2):
        st = diloco.outer_step(base, ws, st, guard=diloco.OuterGuard(max_grad_norm=1e9))
        st2 = diloco.outer_step(plain, ws, st2)
        assert st.last_stats["clip_coef"] == 1.0 and st.last_stats["dropped"] == []
        assert torch.equal(_bits(torch.cat(base)), _bits(torch.cat(plain)))
        assert torch.equal(_bits(st.momentum), _bits(st2.momentum))
    # clipped to half the measured norm: the flat scaled step on packed clones with the very clip_coef
    base, ws = _device_lists(dev, gdt, wdt, K, 700)
    f_t, f_ws = torch.cat(base), [torch.cat(w) for w in ws]
    probe = diloco.outer_step([t.clone() for t in base], ws, guard=diloco.OuterGuard(max_grad_norm=1e9))
    norm = probe.last_stats["grad_norm"]
    assert norm > 0
    st = diloco.outer_step(base, ws, guard=diloco.OuterGuard(max_grad_norm=norm / 2))
    clip = st.last_stats["clip_coef"]
    assert 0.49 < clip <= 0.5 and st.last_stats["grad_norm"] == norm
    f_m = torch.zeros_like(f_t)
    ops.outer_step_scaled(f_t, f_ws, f_m, False, 0.7, 0.9, True, clip)
    assert torch.equal(_bits(torch.cat(base)), _bits(f_t)) and torch.equal(_bits(st.momentum), _bits(f_m))
    # the arena guard on packed clones measures the same norm up to the fp64 summation order
    from evolutionarydistributedtraining_amd.params import ParamArena, ParamLayout
    layout = ParamLayout([torch.Size((s,)) for s in SIZES])
    a_t, a_ws = torch.cat(_device_lists(dev, gdt, wdt, K, 700)[0]), f_ws
    sync = diloco.OuterSync(ParamArena(layout, gdt, dev, a_t), [ParamArena(layout, wdt, dev, w) for w in a_ws],
                            guard=diloco.OuterGuard(max_grad_norm=norm / 2))
    sync.step()
    arena_norm = sync.last_stats["grad_norm"]
    # |dS_mm| <= 2 n 2^-53 S_mm. Through the square root the relative bound halves
    # (|dx| = |dS| / (x + x')), and each of the two norms carries one rounding of its own (2^-53).
    print("grad_norm list", norm, "arena", arena_norm, "relative", abs(norm - arena_norm) / arena_norm)
    assert abs(norm - arena_norm) <= (n + 3) * 2.0 ** -53 * arena_norm


def test_policies_on_lists(dev, no_packing):
    from evolutionarydistributedtraining_amd import diloco
    K = 4
    base, ws = _device_lists(dev, F32, BF16, K, 800)
    st = diloco.outer_step(base, ws, guard=diloco.OuterGuard())            # a momentum to protect
    t0, m0 = [t.clone() for t in base], st.momentum.clone()
    ws[2][5][17] = float("inf")
    ws[2][8][70000] = float("nan")
    # raise: names the worker and its counts, nothing touched
    with pytest.raises(diloco.NonFiniteWorkers) as e:
        diloco.outer_step(base, ws, st, guard=diloco.OuterGuard())
    assert e.value.nonfinite == [0, 0, 2, 0] and e.value.nonfinite_mean == 2 and e.value.survivors == [0, 1, 3]
    assert all(torch.equal(_bits(a), _bits(b)) for a, b in zip(base, t0))
    assert torch.equal(_bits(st.momentum), _bits(m0)) and st.has_momentum and st.steps == 1
    # min_workers is honoured after a drop
    with pytest.raises(diloco.NonFiniteWorkers):
        diloco.outer_step(base, ws, st, guard=diloco.OuterGuard(on_nonfinite="drop", min_workers=4))
    assert all(torch.equal(_bits(a), _bits(b)) for a, b in zip(base, t0)) and torch.equal(_bits(st.momentum), _bits(m0))
    # ignore: only reports (on clones: the step itself is poisoned, as the policy says)
    ign = diloco.outer_step([t.clone() for t in base], ws, guard=diloco.OuterGuard(on_nonfinite="ignore"))
    assert ign.last_stats["nonfinite"] == [0, 0, 2, 0] and ign.last_stats["clip_coef"] == 1.0
    assert ign.last_stats["dropped"] == []
    # drop: the unguarded list step over the survivors
    ref_t = [t.clone() for t in base]
    ref = diloco.OuterState()
    ref.momentum, ref.has_momentum, ref.steps = m0.clone(), True, 1
    diloco.outer_step(base, ws, st, guard=diloco.OuterGuard(on_nonfinite="drop", min_workers=3))
    diloco.outer_step(ref_t, [ws[0], ws[1], ws[3]], ref)
    assert st.last_stats["dropped"] == [2] and st.last_stats["nonfinite"] == [0, 0, 2, 0]
    assert st.last_stats["nonfinite_mean"] == 0 and st.last_stats["clip_coef"] == 1.0
    assert torch.equal(_bits(torch.cat(base)), _bits(torch.cat(ref_t)))
    assert torch.equal(_bits(st.momentum), _bits(ref.momentum)) and st.steps == 2


def test_per_tensor_report(dev, oracle, no_packing):
    from evolutionarydistributedtraining_amd import diloco, guard
    K = 3
    thetas, workers = _population(F32, F32, K, 500 + K)
    want, first = _want(oracle, F32, F32, K, 500 + K)
    base, ws = _device_lists(dev, F32, F32, K, 500 + K)
    st = diloco.outer_step(base, ws, guard=diloco.OuterGuard(per_tensor=True))
    per = st.last_stats["per_tensor"]
    assert len(per) == len(SIZES)
    assert per[0]["grad_norm"] == 0.0 and per[0]["worker_norms"] == [0.0] * K and per[0]["nonfinite"] == [0] * K
    for t, (a, b) in enumerate(zip(first[:-1], first[1:])):
        expect = guard.report(guard.stats_totals(want[a:b], K))
        assert {k: v for k, v in per[t].items() if k != "cos_to_mean"} == \
            {k: v for k, v in expect.items() if k != "cos_to_mean"}, t
        assert np.array_equal(per[t]["cos_to_mean"], expect["cos_to_mean"], equal_nan=True), t
    assert st.last_stats["grad_norm"] == guard.report(guard.stats_totals(want, K))["grad_norm"]


def test_guard_on_lists_refuses_more_than_64_workers(dev):
    from evolutionarydistributedtraining_amd import diloco
    from evolutionarydistributedtraining_amd._lib import EdtError
    base = [torch.zeros(8, device=dev), torch.zeros(3, device=dev)]
    ws = [[torch.zeros(8, device=dev), torch.zeros(3, device=dev)] for _ in range(65)]
    with pytest.raises(EdtError):
        diloco.outer_step(base, ws, guard=diloco.OuterGuard())
    diloco.outer_step(base, ws)                         # unguarded: packed and chained, as before
