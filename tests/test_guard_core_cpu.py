"""The guard's host-side core (guard.py) and how ShardedOuterSync uses it: the names diloco
re-exports, the totals and the re-measurement merge as pure functions, a guarded step's decision as a
value that no later step can see, and the one table of kernel entries. No device: the sharded steps
run on virtual ranks with the oracle-backed stand-in kernels of tests/test_sharded_guard_cpu.py."""
import numpy as np
import pytest
import torch

from evolutionarydistributedtraining_amd import diloco, guard
from evolutionarydistributedtraining_amd import distributed as D
from evolutionarydistributedtraining_amd._lib import EdtError
from evolutionarydistributedtraining_amd.collectives import VirtualWorld
from evolutionarydistributedtraining_amd.params import ParamLayout
from tests.test_sharded_guard_cpu import GuardOracleKernels, SumKernels

F32, BF16 = torch.float32, torch.bfloat16
CPU = torch.device("cpu")


@pytest.mark.parametrize("name", ["OuterGuard", "NonFiniteWorkers", "guard_decision", "stats_totals",
                                  "clip_coefficient"])
def test_diloco_reexports_the_moved_names(name):
    assert getattr(diloco, name) is getattr(guard, name)


@pytest.mark.parametrize("K", [3, 9])
def test_totals_from_row_is_stats_totals(K):
    W = 3 * K + 2
    rows = np.random.default_rng(K).standard_normal((7, W)) * 1e3
    rows[:, 2 * K + 1:] = np.abs(rows[:, 2 * K + 1:]).round()            # the count columns
    got = guard.totals_from_row(guard.sequential_total(rows, W), K)
    want = guard.stats_totals(rows, K)
    assert list(got) == list(want) == ["S_mm", "S_kk", "S_km", "nonfinite_mean", "nonfinite"]
    for key in got:
        if got[key] is None:
            assert want[key] is None and key == "S_km" and K > 8
        else:
            assert np.array_equal(np.asarray(got[key]), np.asarray(want[key])), key
            assert np.asarray(got[key]).dtype == np.asarray(want[key]).dtype
    assert (got["S_km"] is None) == (K > 8)
    # the fixed order: one running sum down the rows, not numpy's pairwise sum
    run = np.zeros(W)
    for r in rows:
        run = run + r
    assert np.array_equal(guard.sequential_total(rows, W), run)


def test_sequential_total_of_no_rows():
    for width in (2, 11):
        t = guard.sequential_total(np.zeros((0, width)), width)
        assert t.shape == (width,) and t.dtype == np.float64 and not t.any()
        assert guard.sequential_total([], width).shape == (width,)


def test_fold_remeasured():
    K, survivors = 4, [0, 2]
    first = {"grad_norm": 9.0, "worker_norms": [1.0, 2.0, 3.0, 4.0], "cos_to_mean": [0.1, 0.2, 0.3, 0.4],
             "nonfinite": [0, 5, 0, 1], "nonfinite_mean": 6, "clip_coef": None, "dropped": []}
    again = {"grad_norm": 2.5, "worker_norms": [1.5, 3.5], "cos_to_mean": [0.75, -0.25], "nonfinite": [0, 0],
             "nonfinite_mean": 0}
    rep = dict(first)
    assert guard.fold_remeasured(rep, again, survivors, K) is None
    assert rep["grad_norm"] == 2.5 and rep["nonfinite_mean"] == 0
    cos = rep["cos_to_mean"]
    assert np.isnan(cos[1]) and np.isnan(cos[3]) and cos[0] == 0.75 and cos[2] == -0.25 and len(cos) == K
    for key in ("worker_norms", "nonfinite", "clip_coef", "dropped"):
        assert rep[key] == first[key]
    # no cosines in the second report (above 8 workers): the first report's stay
    rep = dict(first)
    guard.fold_remeasured(rep, dict(again, cos_to_mean=None), survivors, K)
    assert rep["cos_to_mean"] == first["cos_to_mean"] and rep["grad_norm"] == 2.5 and rep["nonfinite_mean"] == 0
    assert rep["worker_norms"] == first["worker_norms"] and rep["nonfinite"] == first["nonfinite"]


# ---- no decision outlives its step ---------------------------------------------------------------

STEP_ENTRIES = {"sgd_apply", "sgd_apply_sum", "outer_step"}
STEP_ENTRIES |= {D._entry(name, 0.5)[0] for name in STEP_ENTRIES}


class Logged:
    """A kernels object that records (entry name, positional arguments) of every call, and raises
    instead of running the `fail_at`-th step entry (1-based) when that is set."""

    def __init__(self, inner):
        self.inner, self.log, self.fail_at = inner, [], None

    def __getattr__(self, name):
        fn = getattr(self.inner, name)                     # a missing entry stays missing (hasattr)

        def call(*args, **kw):
            self.log.append((name, args))
            if self.fail_at is not None and name in STEP_ENTRIES:
                self.fail_at -= 1
                if self.fail_at == 0:
                    self.fail_at = None
                    raise RuntimeError("injected kernel failure")
            return fn(*args, **kw)
        return call


def _three_steps(oracle, mode, kernels, policy):
    """Steps (a) guarded and clipped, (b) guarded with the second bucket's consume failing, (c)
    unguarded, on 2 virtual ranks; returns per rank the three logs, the errors of (b) and last_stats
    after (a)."""
    world, k_local = 2, 2
    layout = ParamLayout([(200,)])
    g = torch.Generator().manual_seed(5)
    theta0 = torch.randn(200, generator=g) * 0.02
    workers0 = [(theta0 + torch.randn(200, generator=g) * 1e-3).to(BF16) for _ in range(world * k_local)]
    if policy == "drop":
        workers0[1][7] = float("nan")                      # global worker 1: rank 0's second

    def body(comm):
        k = Logged(kernels(oracle))
        sync = D.ShardedOuterSync(layout, F32, BF16, k_local, CPU, mode=mode, broadcast="theta", bucket_elems=128,
                                  kernels=k, comm=comm, guard=guard.OuterGuard(max_grad_norm=1e-6, on_nonfinite=policy))
        assert sync.n_pad == 256 and sync.buckets == [(0, 128), (128, 256)]
        attrs = set(vars(sync))
        sync.theta.flat.copy_(theta0)
        for j, arena in enumerate(sync.workers):
            arena.flat.copy_(workers0[comm.rank * k_local + j])
        out = {"logs": []}
        sync.step()                                        # (a)
        out["stats"] = dict(sync.last_stats)
        out["logs"].append(list(k.log))
        del k.log[:]
        k.fail_at = 2                                      # (b)
        with pytest.raises(RuntimeError, match="injected kernel failure"):
            sync.step()
        out["logs"].append(list(k.log))
        del k.log[:]
        sync.guard = None                                  # (c)
        sync.step()
        out["logs"].append(list(k.log))
        assert set(vars(sync)) == attrs                    # a step leaves no new attribute behind
        assert not any(isinstance(x, D._Verdict) for x in vars(sync).values())
        return out

    return VirtualWorld(world).run(body)


@pytest.mark.parametrize("policy", ["raise", "drop"])
@pytest.mark.parametrize("mode,kernels", [("reduce", GuardOracleKernels), ("reduce_ordered", GuardOracleKernels),
                                          ("reduce_ordered", SumKernels), ("exact", GuardOracleKernels)],
                         ids=["reduce", "reduce_ordered", "reduce_ordered-sum", "exact"])
def test_no_decision_outlives_its_step(oracle, mode, kernels, policy):
    plain = "outer_step" if mode == "exact" else "sgd_apply_sum" if kernels is SumKernels else "sgd_apply"
    scaled = D._entry(plain, 0.5)[0]
    assert scaled == plain + "_scaled" and D._entry(plain, 1.0) == (plain, ())
    dropped = [1] if policy == "drop" else []
    for rank, r in enumerate(_three_steps(oracle, mode, kernels, policy)):
        a, b, c = r["logs"]
        steps = lambda log: [(name, args) for name, args in log if name in STEP_ENTRIES]
        assert 0.0 < r["stats"]["clip_coef"] < 1.0 and r["stats"]["dropped"] == dropped
        # (a): the scaled entry for both buckets, with the coefficient the report states
        assert [name for name, _ in steps(a)] == [scaled, scaled]
        assert all(args[7] == r["stats"]["clip_coef"] for _, args in steps(a))
        # (b): the first bucket's consume ran, the second's raised
        assert [name for name, _ in steps(b)] == [scaled, scaled]
        # (c): plain entries only, every worker, the full divisor
        assert [name for name, _ in steps(c)] == [plain, plain]
        assert not [name for name, _ in c if name.endswith("_scaled") or name.endswith("_stats")]
        for log, gone in ((a, dropped), (b, dropped), (c, [])):
            if mode == "exact":
                assert [len(args[1]) for _, args in steps(log)] == [4 - len(gone)] * 2
            else:
                phase1 = [(len(args[1]), args[2]) for name, args in log if name == "delta_partial"]
                mine = 2 - len([k for k in gone if k // 2 == rank])
                assert phase1 == [(mine, 4 - len(gone))] * 2


# ---- the kernel-name table -----------------------------------------------------------------------

def _without(base, missing):
    class Hidden(base):
        def __getattribute__(self, name):
            if name == missing:
                raise AttributeError(name)
            return super().__getattribute__(name)
    return Hidden


@pytest.mark.parametrize("kernels", [GuardOracleKernels, SumKernels], ids=["no-sum", "sum"])
@pytest.mark.parametrize("mode", ["reduce", "reduce_ordered", "exact"])
def test_check_guard_needs_the_entry_the_step_would_launch(oracle, mode, kernels):
    plain = {"reduce": "sgd_apply", "exact": "outer_step",
             "reduce_ordered": "sgd_apply_sum" if kernels is SumKernels else "sgd_apply"}[mode]
    needed = D._entry(plain, 0.5)[0]
    layout, comm = ParamLayout([(200,)]), VirtualWorld(1).comm(0)
    mk = lambda k: D.ShardedOuterSync(layout, F32, BF16, 2, CPU, mode=mode, broadcast="theta", kernels=k, comm=comm,
                                      guard=guard.OuterGuard())
    with pytest.raises(EdtError, match=rf"lacks \['{needed}'\]"):
        mk(_without(kernels, needed)(oracle))
    # exactly that one: a scaled entry this schedule never launches may be missing
    for other in sorted({"sgd_apply_scaled", "sgd_apply_sum_scaled", "outer_step_scaled"} - {needed}):
        assert mk(_without(kernels, other)(oracle)).guard is not None
