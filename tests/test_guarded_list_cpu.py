"""The tensor-list guard without a device: the C ABI's validation of edt_delta_stats_list,
edt_delta_stats_list_workspace_bytes and edt_outer_step_list_scaled (pointers that are never
dereferenced), and diloco's list-guard dispatch driven with the three ops replaced by recorders
whose rows come from the CPU restatement (tests/stats_reference.py)."""
import ctypes

import numpy as np
import pytest
import torch

from tests import stats_reference as R

P = ctypes.c_void_p
U64 = ctypes.c_uint64
F32, BF16 = 0, 1

_host = (ctypes.c_uint8 * 8192)()
_base = ctypes.addressof(_host)


def fake(i, off=0):
    return P(_base + 64 * (i + 1) + off)      # distinct, 16-byte aligned (off = 0), never dereferenced


def arr(ptrs):
    return (P * max(1, len(ptrs)))(*ptrs)


def u64(vals):
    return (U64 * max(1, len(vals)))(*vals)


@pytest.fixture(scope="module")
def lib():
    from evolutionarydistributedtraining_amd import _lib
    return _lib.load_library()


def _rejects(lib, rc, needle):
    msg = lib.edt_last_error().decode()
    assert rc < 0 and needle in msg, (rc, msg)


def test_abi_version_is_unchanged(lib):
    assert lib.edt_abi_version() == 6


def test_workspace_query(lib):
    q = lib.edt_delta_stats_list_workspace_bytes
    assert q(0, 3) == 0 and q(-1, 3) == 0 and q(5, 0) == 0 and q(5, 65) == 0
    for T, K in ((1, 1), (9, 3), (292, 8), (292, 64)):
        assert q(T, K) >= 8 * T * (K + 1)                  # every pointer of the table
        assert q(T + 1, K) - q(T, K) == q(1, K)            # linear in T ...
        assert q(T, K) > q(T, K - 1) if K > 1 else True    # ... and growing with K
    assert q(292, 8) - q(292, 7) == 8 * 292                # one pointer per tensor and worker


def test_delta_stats_list_validation(lib):
    T, K = 2, 3
    th, ws, numel = arr([fake(0), fake(1)]), arr([fake(2 + i) for i in range(K * T)]), u64([100, 7])
    need = lib.edt_delta_stats_list_workspace_bytes(T, K)

    def go(theta=th, gdt=F32, w=ws, wdt=BF16, K=K, numel=numel, T=T, chunks=fake(20), nchunks=2, out=fake(21),
           wsp=fake(22), nbytes=need):
        return lib.edt_delta_stats_list(theta, gdt, w, wdt, K, numel, T, chunks, nchunks, out, wsp, nbytes, None)

    _rejects(lib, go(gdt=BF16, wdt=F32), "dtype pair")
    _rejects(lib, go(gdt=7), "dtype pair")
    _rejects(lib, go(K=0), "out of range")
    _rejects(lib, go(K=65), "out of range")
    _rejects(lib, go(T=-1), "tensor count")
    _rejects(lib, go(nchunks=-1), "negative")
    _rejects(lib, go(theta=None), "null tensor table")
    _rejects(lib, go(w=None), "null tensor table")
    _rejects(lib, go(numel=None), "null tensor table")
    _rejects(lib, go(chunks=None), "null chunk table")
    _rejects(lib, go(out=None), "null chunk table")
    _rejects(lib, go(out=fake(21, 4)), "8-byte aligned")
    _rejects(lib, go(wsp=None), "workspace")
    _rejects(lib, go(nbytes=need - 1), "workspace")
    _rejects(lib, go(wsp=fake(22, 4)), "workspace must be 8-byte aligned")
    _rejects(lib, go(theta=arr([fake(0), None])), "theta_t[1] is null")
    bad = [fake(2 + i) for i in range(K * T)]
    bad[1 * T + 0] = None
    _rejects(lib, go(w=arr(bad)), "theta_k[1][0] is null")
    assert go(T=0, theta=None, w=None, numel=None) == 0                   # nothing to do
    assert go(nchunks=0, chunks=None, out=None, wsp=None, nbytes=0) == 0


def test_outer_step_list_scaled_validation(lib):
    T, K = 2, 3
    th, mo = arr([fake(0), fake(1)]), arr([fake(30), fake(31)])
    ws, numel = arr([fake(2 + i) for i in range(K * T)]), u64([100, 7])
    need = lib.edt_outer_list_workspace_bytes(T, K)

    def go(theta=th, gdt=F32, w=ws, wdt=BF16, K=K, mom=mo, numel=numel, T=T, bits=None, offs=None, scale=0.5,
           wsp=fake(22), nbytes=need):
        return lib.edt_outer_step_list_scaled(theta, gdt, w, wdt, K, mom, 1, numel, T, 0.7, 0.9, 1, bits, offs, scale,
                                              wsp, nbytes, None)

    _rejects(lib, go(gdt=BF16, wdt=F32), "dtype pair")
    _rejects(lib, go(K=0), "out of range")
    _rejects(lib, go(K=65), "out of range")
    _rejects(lib, go(T=-1), "tensor count")
    for bad in (-0.1, 1.5, float("nan"), float("inf")):
        _rejects(lib, go(scale=bad), "grad_scale")
        _rejects(lib, go(scale=bad, T=0), "grad_scale")                   # checked before anything else
    _rejects(lib, go(theta=None), "null tensor table")
    _rejects(lib, go(w=None), "null tensor table")
    _rejects(lib, go(numel=None), "null tensor table")
    _rejects(lib, go(mom=None), "momentum table is null")
    _rejects(lib, go(wsp=None), "workspace")
    _rejects(lib, go(nbytes=need - 8), "workspace")
    _rejects(lib, go(bits=fake(23), offs=u64([0, 13])), "bf16 master")    # tail bits with an fp32 master
    _rejects(lib, go(gdt=BF16, bits=fake(23), offs=None), "byte offsets")
    assert go(T=0) == 0 and go(T=0, scale=0.0) == 0 and go(T=0, scale=1.0) == 0


# ---- diloco's list-guard dispatch -----------------------------------------------------------------

SIZES = [0, 1, 7, 8, 15, 513]
K = 3


class Recorder:
    """Stands in for ops.delta_stats_list / outer_step_list / outer_step_list_scaled: the rows are the
    restatement's, per tensor, concatenated in tensor order; the steps only record their call."""

    def __init__(self, oracle):
        self.oracle = oracle
        self.calls = []

    def delta_stats_list(self, thetas, workers, plan):
        assert plan.relative and plan.nseg == len(thetas)
        rows = []
        for t, th in enumerate(thetas):
            if th.numel():
                r, _ = R.stats_rows(th, [w[t] for w in workers], R.make_chunks([0, th.numel()]), self.oracle)
                rows.append(r)
        self.calls.append(("stats", len(workers), [id(w) for w in workers]))
        return torch.from_numpy(np.concatenate(rows))

    def outer_step_list(self, thetas, workers, moms, has, lr, mu, nesterov, tails=None):
        self.calls.append(("plain", len(workers), [id(w) for w in workers]))

    def outer_step_list_scaled(self, thetas, workers, moms, has, lr, mu, nesterov, scale, tails=None):
        self.calls.append(("scaled", len(workers), [id(w) for w in workers], scale))


@pytest.fixture()
def rec(oracle, monkeypatch):
    from evolutionarydistributedtraining_amd import diloco, ops
    r = Recorder(oracle)
    for name in ("delta_stats_list", "outer_step_list", "outer_step_list_scaled"):
        monkeypatch.setattr(ops, name, getattr(r, name))

    def no_pack(*a, **k):
        raise AssertionError("the guarded list step must not pack")
    monkeypatch.setattr(diloco, "pack", no_pack)
    monkeypatch.setattr(diloco, "unpack_", no_pack)
    return r


def _lists(seed=3):
    thetas, workers = [], [[] for _ in range(K)]
    for t, n in enumerate(SIZES):
        th, ws = R.operands(n, K, torch.float32, torch.float32, seed=seed + t)
        thetas.append(th)
        for k in range(K):
            workers[k].append(ws[k])
    return thetas, workers


def _s_mm(oracle, thetas, workers):
    from evolutionarydistributedtraining_amd.diloco import stats_totals
    rows = Recorder(oracle).delta_stats_list(thetas, workers, type("P", (), {"relative": True, "nseg": len(thetas)}))
    return stats_totals(rows.numpy(), len(workers))["S_mm"]


def test_dispatch_plain_at_clip_one(rec):
    from evolutionarydistributedtraining_amd import diloco
    thetas, workers = _lists()
    st = diloco.OuterState()
    diloco._step_list(thetas, workers, st, 0.7, 0.9, True, guard=diloco.OuterGuard(max_grad_norm=1e9, per_tensor=True))
    assert [c[0] for c in rec.calls] == ["stats", "plain"]
    assert rec.calls[1][2] == [id(w) for w in workers]
    rep = st.last_stats
    assert rep["clip_coef"] == 1.0 and rep["dropped"] == [] and st.has_momentum and st.steps == 1
    assert len(rep["per_tensor"]) == len(SIZES)
    assert rep["per_tensor"][0]["grad_norm"] == 0.0 and rep["per_tensor"][0]["nonfinite"] == [0] * K


def test_dispatch_scaled_below_one(rec, oracle):
    from evolutionarydistributedtraining_amd import diloco
    thetas, workers = _lists()
    norm = _s_mm(oracle, thetas, workers) ** 0.5
    st = diloco.OuterState()
    diloco._step_list(thetas, workers, st, 0.7, 0.9, True, guard=diloco.OuterGuard(max_grad_norm=norm / 2))
    assert [c[0] for c in rec.calls] == ["stats", "scaled"]
    clip = rec.calls[1][3]
    assert clip == st.last_stats["clip_coef"] == diloco.clip_coefficient(norm * norm, norm / 2) and 0.49 < clip < 0.5
    assert st.last_stats["grad_norm"] == norm


def test_dispatch_drop_passes_the_survivors(rec, oracle):
    from evolutionarydistributedtraining_amd import diloco
    thetas, workers = _lists()
    workers[1][5][200] = float("nan")
    st = diloco.OuterState()
    diloco._step_list(thetas, workers, st, 0.7, 0.9, True, guard=diloco.OuterGuard(on_nonfinite="drop"))
    kinds = [c[0] for c in rec.calls]
    assert kinds == ["stats", "stats", "plain"]
    survivors = [id(workers[0]), id(workers[2])]
    assert rec.calls[0][1] == K and rec.calls[1][2] == survivors and rec.calls[2][2] == survivors
    rep = st.last_stats
    assert rep["dropped"] == [1] and rep["nonfinite"] == [0, 1, 0] and rep["clip_coef"] == 1.0
    assert rep["grad_norm"] == _s_mm(oracle, thetas, [workers[0], workers[2]]) ** 0.5
    assert np.isnan(rep["cos_to_mean"][1]) and not np.isnan(rep["cos_to_mean"][0])


def test_dispatch_nothing_after_a_raise(rec):
    from evolutionarydistributedtraining_amd import diloco
    thetas, workers = _lists()
    workers[2][3][7] = float("inf")
    st = diloco.OuterState()
    with pytest.raises(diloco.NonFiniteWorkers) as e:
        diloco._step_list(thetas, workers, st, 0.7, 0.9, True, guard=diloco.OuterGuard())
    assert e.value.nonfinite == [0, 0, 1] and e.value.survivors == [0, 1]
    assert [c[0] for c in rec.calls] == ["stats"]
    assert st.momentum is None and not st.has_momentum and st.steps == 0
    with pytest.raises(diloco.NonFiniteWorkers):                # min_workers after a drop
        diloco._step_list(thetas, workers, st, 0.7, 0.9, True,
                          guard=diloco.OuterGuard(on_nonfinite="drop", min_workers=3))
    assert [c[0] for c in rec.calls] == ["stats", "stats"] and st.momentum is None


def test_dispatch_refuses_more_than_64_workers(rec):
    from evolutionarydistributedtraining_amd import diloco
    from evolutionarydistributedtraining_amd._lib import EdtError
    thetas, workers = _lists()
    with pytest.raises(EdtError):
        diloco._step_list(thetas, [workers[0]] * 65, diloco.OuterState(), 0.7, 0.9, True, guard=diloco.OuterGuard())
    assert rec.calls == []


def test_plan_is_cached_by_sizes_and_device(rec):
    from evolutionarydistributedtraining_amd import diloco
    thetas, workers = _lists()
    st = diloco.OuterState()
    p1 = diloco._stats_list_plan(st, thetas)
    assert diloco._stats_list_plan(st, thetas) is p1 and p1.relative and p1.nseg == len(SIZES)
    assert p1.seg_numel.tolist() == SIZES
    want = np.concatenate([R.make_chunks([0, n]) + [0, 0, t] for t, n in enumerate(SIZES) if n])
    assert (p1.chunks_host == want).all()
    assert diloco._stats_list_plan(st, thetas[:-1]) is not p1
