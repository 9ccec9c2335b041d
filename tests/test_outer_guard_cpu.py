"""The guarded outer step's host side, without a device: guard_decision on synthetic totals, the
clip coefficient's formula and float32 cast, the totals' summation order, the CPU restatement of
the statistics against a plain float64 sum, the C ABI's validation of edt_delta_stats and
edt_outer_step_scaled, and the guard= plumbing of the sync classes."""
import ctypes

import numpy as np
import pytest
import torch

from tests import stats_reference as R

P = ctypes.c_void_p
F32, BF16 = 0, 1


def _totals(nf, nfm=0, s_mm=4.0):
    K = len(nf)
    return {"S_mm": s_mm, "S_kk": np.ones(K), "S_km": np.ones(K) if K <= 8 else None,
            "nonfinite": np.asarray(nf, dtype=np.int64), "nonfinite_mean": nfm}


def test_guard_decision_policies():
    from evolutionarydistributedtraining_amd.diloco import NonFiniteWorkers, OuterGuard, guard_decision
    from evolutionarydistributedtraining_amd._lib import EdtError
    assert issubclass(NonFiniteWorkers, EdtError)
    assert guard_decision(_totals([0, 0, 0]), OuterGuard()) == ([0, 1, 2], 1.0)
    with pytest.raises(NonFiniteWorkers) as e:
        guard_decision(_totals([0, 3, 0], 3), OuterGuard())
    assert e.value.nonfinite == [0, 3, 0] and e.value.nonfinite_mean == 3 and e.value.survivors == [0, 2]
    with pytest.raises(NonFiniteWorkers):                       # finite workers, overflowed mean
        guard_decision(_totals([0, 0], 1), OuterGuard())
    drop = OuterGuard(on_nonfinite="drop", max_grad_norm=1.0)
    assert guard_decision(_totals([0, 3, 0], 3), drop) == ([0, 2], None)     # measured again by the caller
    assert guard_decision(_totals([0, 0]), drop) == ([0, 1], float(np.float32(1.0 / (2.0 + 1e-6))))
    with pytest.raises(NonFiniteWorkers):                       # a non-finite mean over finite survivors
        guard_decision(_totals([0, 0], 2), drop)
    with pytest.raises(NonFiniteWorkers):
        guard_decision(_totals([1, 0, 5]), OuterGuard(on_nonfinite="drop", min_workers=2))
    assert guard_decision(_totals([1, 0, 5]), OuterGuard(on_nonfinite="drop", min_workers=1)) == ([1], None)
    with pytest.raises(NonFiniteWorkers):                       # min_workers holds under every policy
        guard_decision(_totals([0, 0]), OuterGuard(on_nonfinite="ignore", min_workers=3))
    assert guard_decision(_totals([1, 0], 1), OuterGuard(on_nonfinite="ignore")) == ([0, 1], 1.0)
    for bad in (dict(on_nonfinite="skip"), dict(max_grad_norm=0.0), dict(max_grad_norm=float("nan")),
                dict(min_workers=0)):
        with pytest.raises(ValueError):
            OuterGuard(**bad)


def test_clip_coefficient_formula_and_cast():
    from evolutionarydistributedtraining_amd.diloco import OuterGuard, clip_coefficient, guard_decision
    assert clip_coefficient(123.0, None) == 1.0
    for s_mm, mx in ((9.0, 1.0), (2.0, 0.3), (1e-20, 1.0), (0.0, 5.0), (1.0, 1.0), (3.7e9, 0.01)):
        want = np.float32(min(1.0, mx / (np.sqrt(np.float64(s_mm)) + 1e-6)))
        got = clip_coefficient(s_mm, mx)
        assert got == float(want) and np.float32(got) == want
        assert guard_decision(_totals([0], s_mm=s_mm), OuterGuard(max_grad_norm=mx))[1] == got
    # the 1.0 shortcut: a norm below the bound, and one so close above it that float32 rounds to 1
    assert clip_coefficient(0.25, 1.0) == 1.0
    assert clip_coefficient(1.0, 1.0 + 1e-6 - 1e-9) == 1.0     # 1 - 1e-9 in float64, 1.0f as cast
    assert clip_coefficient(1.0, 1.0) < 1.0                     # 1 / (1 + 1e-6), torch's formula
    assert clip_coefficient(9.0, 1.0) == float(np.float32(1.0 / (3.0 + 1e-6)))


def test_totals_are_sequential_in_chunk_order():
    from evolutionarydistributedtraining_amd.diloco import stats_totals
    K = 2
    rng = np.random.default_rng(0)
    rows = rng.standard_normal((5000, 3 * K + 2)) * 10.0 ** rng.integers(-8, 8, (5000, 1))
    rows[:, 2 * K + 1:] = rng.integers(0, 3, (5000, K + 1))
    t = stats_totals(rows, K, first=np.asarray([0, 10, 10, 5000]))
    seq = 0.0
    for x in rows[:, 0]:
        seq += x
    assert t["S_mm"] == seq
    assert t["nonfinite"].tolist() == rows[:, 2 * K + 2:].sum(axis=0).astype(int).tolist()
    assert [s["S_mm"] for s in t["segments"]][1] == 0.0 and len(t["segments"]) == 3
    seg0 = 0.0
    for x in rows[:10, 1]:
        seg0 += x
    assert t["segments"][0]["S_kk"][0] == seg0
    assert stats_totals(np.zeros((3, 3 * 9 + 2)), 9)["S_km"] is None


# Measured on this restatement at n = 70,518 (three segments, K = 3, the three dtype regimes): the
# largest relative difference between a canonical-order total and numpy's float64 sum of the same
# products was 1.7e-16 (under one ulp of fp64; both sum exact products in fp64 and differ in order only).
# The gate is a small multiple of it.
RESTATEMENT_REL_TOL = 8 * 1.7e-16


@pytest.mark.parametrize("gdt,wdt", [(torch.float32, torch.float32), (torch.float32, torch.bfloat16),
                                     (torch.bfloat16, torch.bfloat16)])
def test_restatement_against_plain_float64_sum(oracle, gdt, wdt):
    offsets = [0, 5, 70006, 70518]
    K = 3
    theta, workers = R.operands(offsets[-1], K, gdt, wdt, seed=21)
    rows, m = R.stats_rows(theta, workers, R.make_chunks(offsets), oracle)
    tot = np.cumsum(rows, axis=0)[-1]
    ds, _ = R.deltas_and_mean(theta, workers)
    md = m.double().numpy()
    worst = 0.0
    for k, d in enumerate(ds):
        dd = d.double().numpy()
        for got, want in ((tot[1 + k], np.sum(dd * dd)), (tot[1 + K + k], np.sum(dd * md)), (tot[0], np.sum(md * md))):
            worst = max(worst, abs(got - want) / abs(want))
    print("largest relative difference:", worst)
    assert worst <= RESTATEMENT_REL_TOL
    assert (rows[:, 2 * K + 1:] == 0).all()


# ---- C ABI validation ---------------------------------------------------------------------------

@pytest.fixture(scope="module")
def lib():
    from evolutionarydistributedtraining_amd import _lib
    return _lib.load_library()


_host = (ctypes.c_uint8 * 8192)()
_base = ctypes.addressof(_host)


def fake(i):
    return P(_base + 64 * (i + 1))            # distinct, 16-byte aligned, never dereferenced


def arr(ptrs):
    return (P * max(1, len(ptrs)))(*ptrs)


def _rejects(lib, rc, needle):
    msg = lib.edt_last_error().decode()
    assert rc < 0 and needle in msg, (rc, msg)


def test_abi_version_is_unchanged(lib):
    assert lib.edt_abi_version() == 6


def test_delta_stats_validation(lib):
    ws = arr([fake(2), fake(3), fake(4)])
    call = lib.edt_delta_stats
    _rejects(lib, call(fake(0), BF16, ws, F32, 3, 100, fake(9), 1, fake(10), None), "dtype pair")
    _rejects(lib, call(fake(0), 7, ws, F32, 3, 100, fake(9), 1, fake(10), None), "dtype pair")
    _rejects(lib, call(fake(0), F32, ws, F32, 0, 100, fake(9), 1, fake(10), None), "out of range")
    _rejects(lib, call(fake(0), F32, ws, F32, 65, 100, fake(9), 1, fake(10), None), "out of range")
    _rejects(lib, call(fake(0), F32, ws, F32, 3, 100, fake(9), -1, fake(10), None), "negative")
    _rejects(lib, call(fake(0), F32, None, F32, 3, 100, fake(9), 1, fake(10), None), "theta_k is null")
    _rejects(lib, call(None, F32, ws, F32, 3, 100, fake(9), 1, fake(10), None), "theta_g is null")
    _rejects(lib, call(fake(0), F32, arr([fake(2), None, fake(4)]), F32, 3, 100, fake(9), 1, fake(10), None),
             "theta_k[1] is null")
    _rejects(lib, call(fake(0), F32, ws, F32, 3, 100, None, 1, fake(10), None), "null chunk table")
    _rejects(lib, call(fake(0), F32, ws, F32, 3, 100, fake(9), 1, None, None), "null chunk table")
    assert call(None, F32, ws, F32, 3, 0, None, 0, None, None) == 0          # n = 0: nothing to do
    assert call(fake(0), F32, ws, F32, 3, 0, fake(9), 1, fake(10), None) == 0
    assert lib.edt_delta_stats_doubles(8, 10) == 10 * 26 * 33
    assert lib.edt_delta_stats_doubles(64, 1) == 194 * 33
    assert lib.edt_delta_stats_doubles(0, 10) == 0 and lib.edt_delta_stats_doubles(65, 10) == 0
    assert lib.edt_delta_stats_doubles(3, -1) == 0


def test_outer_step_scaled_validation(lib):
    ws = arr([fake(2), fake(3), fake(4)])
    call = lib.edt_outer_step_scaled

    def go(theta=fake(0), gdt=F32, w=ws, wdt=BF16, K=3, mom=fake(1), n=100, scale=0.5):
        return call(theta, gdt, w, wdt, K, mom, 1, n, 0.7, 0.9, 1, None, scale, None)

    _rejects(lib, go(gdt=BF16, wdt=F32), "dtype pair")
    _rejects(lib, go(K=0), "out of range")
    _rejects(lib, go(K=65), "out of range")
    for bad in (-0.25, 1.5, float("nan"), float("inf"), -float("inf")):
        _rejects(lib, go(scale=bad), "grad_scale")
    _rejects(lib, go(theta=None), "theta_g is null")
    _rejects(lib, go(w=None), "theta_k is null")
    _rejects(lib, go(w=arr([fake(2), fake(3), None])), "theta_k[2] is null")
    _rejects(lib, go(mom=None), "momentum buffer is null")
    assert go(n=0) == 0 and go(n=0, scale=0.0) == 0 and go(n=0, scale=1.0) == 0


# ---- guard= plumbing ------------------------------------------------------------------------------

def test_sync_classes_take_a_guard():
    from evolutionarydistributedtraining_amd._lib import EdtError
    from evolutionarydistributedtraining_amd.diloco import DirOuterSync, OuterGuard, OuterState, OuterSync
    from evolutionarydistributedtraining_amd.params import ParamArena, ParamLayout
    g = OuterGuard(max_grad_norm=2.0, on_nonfinite="drop", min_workers=2, per_tensor=True)
    assert (g.max_grad_norm, g.on_nonfinite, g.min_workers, g.per_tensor) == (2.0, "drop", 2, True)
    d = DirOuterSync(device="cpu", guard=g)
    assert d.guard is g and d.last_stats is None
    assert DirOuterSync(device="cpu").guard is None
    with pytest.raises(TypeError):
        DirOuterSync(device="cpu", guard="raise")
    layout = ParamLayout([torch.Size((4,))])
    arena = lambda: ParamArena(layout, torch.float32, "cpu")
    s = OuterSync(arena(), [arena() for _ in range(2)], guard=g)
    assert s.guard is g and s.last_stats is None
    with pytest.raises(EdtError):
        OuterSync(arena(), [arena() for _ in range(65)], guard=g)
    OuterSync(arena(), [arena() for _ in range(65)])           # unguarded: the chained form, as before
    assert OuterState().last_stats is None
