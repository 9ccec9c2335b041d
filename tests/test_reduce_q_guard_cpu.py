"""ShardedOuterSync(mode="reduce_q", guard=OuterGuard) on virtual ranks with the numpy stand-ins as
the kernels (tests/reduce_q_guard_reference.py): screening before phase 1, the zero-send rule, the
transactional residual, the statistics of the dequantized mean, the clip — and the argument checks
of the new C ABI entries, which need no device."""
import ctypes

import numpy as np
import pytest
import torch

from evolutionarydistributedtraining_amd._lib import EdtError
from evolutionarydistributedtraining_amd.collectives import VirtualWorld
from evolutionarydistributedtraining_amd.diloco import NonFiniteWorkers, OuterGuard, clip_coefficient
from evolutionarydistributedtraining_amd.distributed import ShardedOuterSync
from tests import reduce_q_guard_reference as RQ
from tests import sharded_guard_reference as G
from tests import sr_reference as S
from tests.virtual_schedules import population

F32, BF16 = torch.float32, torch.bfloat16
CPU = torch.device("cpu")
SHAPES = [(37, 11), (5,), (1,), (40, 13), (129,), (31, 29)]      # 1,961 elements: two buckets at world 2 and 3
OTHER = {"mxfp8": "mxfp4", "mxfp4": "mxfp8"}
# (wire format, gather format, error feedback, rounding)
CONFIGS = [(f, g, ef, rnd) for f in ("mxfp8", "mxfp4") for g in (None, "other")
           for ef, rnd in ((True, "nearest"), (False, "nearest"), (False, "stochastic"))]
CID = [f"{f}-{'gather' if g else 'theta'}-{'ef' if ef else rnd}" for f, g, ef, rnd in CONFIGS]
EF_CONFIGS = [c for c in CONFIGS if c[2]]
SEED = 0x1234abcd


def _kw(cfg):
    f, g, ef, rnd = cfg
    return dict(wire_format=f, gather_format=OTHER[f] if g else None, error_feedback=ef, rounding=rnd, seed=SEED)


def _run(oracle, world, cfg, K=None, steps=2, **kw):
    K = K or 2 * world
    layout, theta, gens = population(SHAPES, F32, BF16, K, steps=steps)
    res = RQ.run_q(world, layout, F32, BF16, theta, gens, CPU, kernels=RQ.NumpyGuardQKernels(oracle), bucket_elems=1024,
                   **_kw(cfg), **kw)
    return layout, theta, gens, res


def _same_stats(res):
    for r in res[1:]:
        assert repr(r["stats"]) == repr(res[0]["stats"])      # NaN-safe, exact floats


# ---- the C ABI ---------------------------------------------------------------------------------

NEW_SYMBOLS = ("edt_partial_sum_stats_q", "edt_sgd_apply_sum_q_scaled", "edt_sgd_delta_sum_q_scaled",
               "edt_sgd_delta_sum_q_sr_scaled", "edt_delta_partial_q_to")


def test_abi_has_the_new_symbols():
    """Fails without the feature: the entries do not exist."""
    from evolutionarydistributedtraining_amd import _lib
    lib = _lib.load_library()
    assert lib.edt_abi_version() == 6 == _lib.EDT_ABI_VERSION
    for name in NEW_SYMBOLS:
        assert getattr(lib, name) is not None and any(s[0] == name for s in _lib.SIGNATURES)


def test_abi_validation():
    """Every refusal is EDT_ERR_ARG before anything is launched (host memory stands in for the
    device pointers: a refused call never touches them)."""
    from evolutionarydistributedtraining_amd import _lib
    lib = _lib.load_library()
    ERR = _lib.EDT_ERR_ARG if hasattr(_lib, "EDT_ERR_ARG") else -1
    buf = (ctypes.c_uint8 * 8192)()
    base = (ctypes.addressof(buf) + 15) // 16 * 16
    P = ctypes.c_void_p

    def tab(*ptrs):
        return (P * len(ptrs))(*ptrs)
    n = 512
    ok_regions = tab(base, base + 1024)
    # edt_partial_sum_stats_q(regions, nacc, fmt, gdt, n, chunk_desc, nchunks, out, stream)
    stats = lib.edt_partial_sum_stats_q
    assert stats(ok_regions, 2, 7, 0, n, base, 1, base + 2048, None) == ERR           # fmt
    assert stats(ok_regions, 2, 0, 9, n, base, 1, base + 2048, None) == ERR           # gdt
    assert stats(ok_regions, 2, 0, 0, n + 8, base, 1, base + 2048, None) == ERR       # n % 512
    assert stats(ok_regions, 0, 0, 0, n, base, 1, base + 2048, None) == ERR           # nacc
    assert stats(tab(*[base] * 65), 65, 0, 0, n, base, 1, base + 2048, None) == ERR
    assert stats(None, 2, 0, 0, n, base, 1, base + 2048, None) == ERR                 # null table
    assert stats(tab(base, None), 2, 0, 0, n, base, 1, base + 2048, None) == ERR      # null region
    assert stats(tab(base, base + 1028), 2, 0, 0, n, base, 1, base + 2048, None) == ERR   # misaligned region
    assert stats(ok_regions, 2, 0, 0, n, None, 1, base + 2048, None) == ERR           # null chunk table
    assert stats(ok_regions, 2, 0, 0, n, base, 1, None, None) == ERR                  # null out
    assert stats(ok_regions, 2, 0, 0, n, base, 1, base + 2052, None) == ERR           # out off 8 bytes
    assert stats(ok_regions, 2, 0, 0, n, base, -1, base + 2048, None) == ERR
    assert stats(ok_regions, 2, 0, 0, 0, base, 1, base + 2048, None) == 0             # nothing to do
    # the scaled consumes: (theta, gdt, regions, nacc, fmt, mom, has, n, lr, mu, nesterov, ...)
    head = (P(base + 4096), 0, ok_regions, 2, 0, None, 0, n, 0.7, 0.0, 0)
    apply_ = lib.edt_sgd_apply_sum_q_scaled
    for bad in (float("nan"), float("inf"), -0.5, 1.5):
        assert apply_(*head, bad, None) == ERR
        assert lib.edt_sgd_delta_sum_q_scaled(*head, None, P(base + 6144), 0, bad, None) == ERR
        assert lib.edt_sgd_delta_sum_q_sr_scaled(*head, P(base + 6144), 0, 1, 0, 0, 0, bad, None) == ERR
    assert apply_(P(base + 4096), 0, ok_regions, 2, 5, None, 0, n, 0.7, 0.0, 0, 0.5, None) == ERR       # fmt
    assert apply_(P(base + 4096), 0, ok_regions, 2, 0, None, 0, n + 32, 0.7, 0.0, 0, 0.5, None) == ERR  # n % 512
    assert apply_(None, 0, ok_regions, 2, 0, None, 0, n, 0.7, 0.0, 0, 0.5, None) == ERR                  # null theta
    assert apply_(P(base + 4100), 0, ok_regions, 2, 0, None, 0, n, 0.7, 0.0, 0, 0.5, None) == ERR        # misaligned
    assert apply_(P(base + 4096), 0, ok_regions, 0, 0, None, 0, n, 0.7, 0.0, 0, 0.5, None) == ERR        # nacc
    assert apply_(P(base + 4096), 0, tab(*[base] * 65), 65, 0, None, 0, n, 0.7, 0.0, 0, 0.5, None) == ERR
    assert lib.edt_sgd_delta_sum_q_scaled(*head, None, None, 0, 0.5, None) == ERR                      # null packed_out
    assert lib.edt_sgd_delta_sum_q_scaled(*head, None, P(base + 6148), 0, 0.5, None) == ERR            # misaligned
    assert lib.edt_sgd_delta_sum_q_scaled(*head, None, P(base + 6144), 3, 0.5, None) == ERR            # fmt_out
    assert lib.edt_sgd_delta_sum_q_sr_scaled(*head, P(base + 6144), 0, 1, 0, 0, 4, 0.5, None) == ERR   # elem_base % 8
    # edt_delta_partial_q_to(theta, gdt, theta_k, wdt, K_local, K_total, n, region_elems, fmt, in, out, packed, stream)
    to = lib.edt_delta_partial_q_to
    th, wk, rin, rout, pk = base, tab(base + 2048), P(base + 4096), P(base + 6144), P(base + 1024)
    assert to(th, 0, wk, 0, 1, 1, n, n, 9, rin, rout, pk, None) == ERR                # fmt
    assert to(th, 0, wk, 0, 1, 1, n, 500, 0, rin, rout, pk, None) == ERR              # region_elems % 512
    assert to(th, 0, wk, 0, 1, 1, n + 512, 1024, 0, rin, rout, pk, None) == ERR       # n % region_elems
    assert to(th, 0, wk, 0, 1, 1, n, n, 0, None, rout, pk, None) == ERR               # null residual_in
    assert to(th, 0, wk, 0, 1, 1, n, n, 0, rin, None, pk, None) == ERR                # null residual_out
    assert to(th, 0, wk, 0, 1, 1, n, n, 0, rin, P(base + 6148), pk, None) == ERR      # misaligned
    assert to(th, 0, wk, 0, 1, 1, n, n, 0, rin, P(base + 4096 + 16), pk, None) == ERR     # overlap, not equal
    assert to(th, 0, wk, 0, 1, 1, n, n, 0, rin, rout, None, None) == ERR              # null packed
    assert to(th, 0, wk, 0, 0, 1, n, n, 0, rin, rout, pk, None) == ERR                # K_local
    assert to(None, 0, wk, 0, 1, 1, n, n, 0, rin, rout, pk, None) == ERR              # null theta
    assert to(th, 0, wk, 0, 1, 1, 0, n, 0, rin, rout, pk, None) == 0                  # nothing to do


# ---- the constructor ---------------------------------------------------------------------------

def test_constructor_accepts_the_guard(oracle):
    """Fails without the feature: guard= with mode='reduce_q' was a ValueError."""
    layout, _, _ = population(SHAPES, F32, BF16, 2, steps=1)
    comm = VirtualWorld(1).comm(0)
    k = RQ.NumpyGuardQKernels(oracle)
    mk = lambda **kw: ShardedOuterSync(layout, F32, BF16, kw.pop("k_local", 2), CPU, comm=comm, mode="reduce_q", **kw)
    sync = mk(kernels=k, guard=OuterGuard(max_grad_norm=1.0, on_nonfinite="drop"))
    assert sync.last_stats is None and sync._residual_next is not None
    assert sync._residual_next.shape == sync.residual.shape and sync._residual_next.dtype == F32
    shard = sync.n_pad // sync.world
    assert sync.guard_bytes() == sync.n_pad * (2 * 2 + 4) + sync.world * (shard + shard // 32)
    # the second residual buffer exists only with a guard and error feedback
    assert mk(kernels=k)._residual_next is None and mk(kernels=k).guard_bytes() == 0
    assert mk(kernels=k, guard=OuterGuard(), error_feedback=False)._residual_next is None
    # what stays refused
    with pytest.raises(ValueError, match="per_tensor"):
        mk(kernels=k, guard=OuterGuard(per_tensor=True))
    with pytest.raises(EdtError, match="64"):
        mk(kernels=k, k_local=65, guard=OuterGuard())
    # stand-ins without the new names: an EdtError that is still the ValueError it used to be
    for lacking, gf in ((S.NumpySrKernels(oracle), None), (S.NumpySrKernels(oracle), "mxfp8")):
        with pytest.raises(ValueError, match="reduce_q") as info:
            mk(kernels=lacking, guard=OuterGuard(), gather_format=gf)
        assert isinstance(info.value, EdtError)
        assert ("sgd_delta_sum_q_scaled" if gf else "sgd_apply_sum_q_scaled") in str(info.value)


def test_unguarded_sync_looks_up_no_new_name(oracle):
    new = {"partial_sum_stats_q", "sgd_apply_sum_q_scaled", "sgd_delta_sum_q_scaled", "delta_stats",
           "make_slerp_plan", "partial_sum_stats"}

    class Strict(S.NumpySrKernels):
        def __getattr__(self, name):
            assert name not in new, f"looked up {name} without a guard"
            raise AttributeError(name)

        def delta_partial_q(self, *a, **kw):
            assert "residual_out" not in kw
            return super().delta_partial_q(*a, **kw)
    layout, theta, gens = population(SHAPES, F32, BF16, 2, steps=1)
    for cfg in CONFIGS:
        sync = ShardedOuterSync(layout, F32, BF16, 2, CPU, comm=VirtualWorld(1).comm(0), mode="reduce_q",
                                kernels=Strict(oracle), **_kw(cfg))
        for w, src in zip(sync.workers, gens[0]):
            w.flat.copy_(src)
        sync.step()
        assert sync.last_stats is None and sync.guard_bytes() == 0 and sync._residual_next is None


# ---- the schedule ------------------------------------------------------------------------------

@pytest.mark.parametrize("world", [2, 3])
@pytest.mark.parametrize("cfg", CONFIGS, ids=CID)
def test_finite_unclipped_guard_is_the_unguarded_step(oracle, world, cfg):
    layout, theta, gens, res = _run(oracle, world, cfg, guard=OuterGuard(max_grad_norm=1e30))
    _, _, _, plain = _run(oracle, world, cfg)
    assert len(res[0]["buckets"]) == 2 and res[0]["n_pad"] > layout.total
    _same_stats(res)
    for r, p in zip(res, plain):
        assert r["errors"] == [None, None]
        for a, b in zip(r["steps"], p["steps"]):
            assert RQ.same_state(a, b)
        assert torch.equal(r["q_send"], p["q_send"]) and torch.equal(r["q_recv"], p["q_recv"])
        assert r["steps"][-1]["q_step"] == 2
    st = res[0]["stats"][-1]
    K = 2 * world
    assert st["clip_coef"] == 1.0 and st["dropped"] == [] and st["nonfinite"] == [0] * K
    assert st["grad_norm"] > 0 and st["nonfinite_mean"] == 0 and st["cos_to_mean"] is None
    n_pad = res[0]["n_pad"]
    q = n_pad * (8 if cfg[0] == "mxfp8" else 4) // 8 + n_pad // 32
    assert res[0]["guard_bytes"] == n_pad * (2 * 2 + 4) + q          # world regions of a shard each


@pytest.mark.parametrize("world", [2, 3])
@pytest.mark.parametrize("cfg", CONFIGS, ids=CID)
def test_raise_writes_nothing_and_the_next_step_works(oracle, world, cfg):
    K, bad = 2 * world, 2 + 1                                      # a worker of rank 1
    layout, theta, gens, res = _run(oracle, world, cfg, steps=3, guard=OuterGuard(),
                                    poison={1: [(bad, 17, float("nan"))]})
    _same_stats(res)
    for r in res:
        assert r["errors"][0] is None and r["errors"][2] is None
        err = r["errors"][1]
        assert isinstance(err, NonFiniteWorkers) and err.nonfinite == [int(k == bad) for k in range(K)]
        assert repr(err) == repr(res[0]["errors"][1])
        assert RQ.same_state(r["before"], r["after"]) and r["after"]["q_step"] == 1
    # generations 0 and 2 alone, unguarded: the refused step changed nothing (q_step included)
    plain = RQ.run_q(world, layout, F32, BF16, theta, [gens[0], gens[2]], CPU, kernels=S.NumpySrKernels(oracle),
                     bucket_elems=1024, **_kw(cfg))
    for r, p in zip(res, plain):
        assert RQ.same_state(r["steps"][-1], p["steps"][-1])


@pytest.mark.parametrize("world,K", [(2, 4), (3, 3)])              # (3, 3): K_local = 1, rank 1 is emptied
@pytest.mark.parametrize("cfg", CONFIGS, ids=CID)
def test_drop_is_the_composition_over_the_survivors(oracle, world, K, cfg):
    bad = K // world                                               # rank 1's first worker
    layout, theta, gens, res = _run(oracle, world, cfg, K=K, guard=OuterGuard(on_nonfinite="drop"),
                                    poison={1: [(bad, 5, float("inf"))]})
    _same_stats(res)
    st = res[0]["stats"][1]
    assert st["dropped"] == [bad] and st["nonfinite"] == [int(k == bad) for k in range(K)]
    assert st["clip_coef"] == 1.0 and st["nonfinite_mean"] == 0
    n_pad, buckets = res[0]["n_pad"], res[0]["buckets"]
    state = RQ.state0(theta, n_pad, world, cfg)
    f_in, f_out = cfg[0], OTHER[cfg[0]] if cfg[1] else None
    RQ.compose(oracle, state, [G.padded(w, n_pad) for w in gens[0]], world, buckets, f_in, f_out, list(range(K)), 1.0,
               cfg[3], SEED)
    ws = [G.padded(w, n_pad) for w in gens[1]]
    ws[bad][5] = float("inf")
    s_mm, nfm = RQ.compose(oracle, state, ws, world, buckets, f_in, f_out, [k for k in range(K) if k != bad], 1.0,
                           cfg[3], SEED)
    assert st["grad_norm"] == s_mm ** 0.5 and nfm == 0
    RQ.assert_is_state(res, state, cfg)
    if K // world == 1:                                            # the emptied rank sent zero, kept its residual
        r1 = res[1]
        assert not r1["q_send"].any()
        for (b, e), (qb, qe) in zip(buckets, r1["q_bytes"]):
            per = (e - b) // world
            assert np.array_equal(r1["q_send"][qb:qe].numpy(), np.tile(RQ.zero_region(per, f_in), world))
        if cfg[2]:
            assert torch.equal(r1["steps"][1]["residual"], r1["steps"][0]["residual"])
            assert r1["steps"][0]["residual"].any()


@pytest.mark.parametrize("world", [2, 3])
@pytest.mark.parametrize("cfg", CONFIGS, ids=CID)
def test_clip_is_the_scaled_composition(oracle, world, cfg):
    K = 2 * world
    _, _, _, first = _run(oracle, world, cfg, steps=1, guard=OuterGuard())
    norm = first[0]["stats"][0]["grad_norm"]
    layout, theta, gens, res = _run(oracle, world, cfg, guard=OuterGuard(max_grad_norm=norm / 2))
    _same_stats(res)
    n_pad, buckets = res[0]["n_pad"], res[0]["buckets"]
    state = RQ.state0(theta, n_pad, world, cfg)
    f_in, f_out = cfg[0], OTHER[cfg[0]] if cfg[1] else None
    for g in range(2):
        st = res[0]["stats"][g]
        assert st["clip_coef"] == clip_coefficient(st["grad_norm"] ** 2, norm / 2) and st["clip_coef"] < 1.0
        s_mm, _ = RQ.compose(oracle, state, [G.padded(w, n_pad) for w in gens[g]], world, buckets, f_in, f_out,
                             list(range(K)), st["clip_coef"], cfg[3], SEED)
        assert st["grad_norm"] == s_mm ** 0.5
    assert res[0]["stats"][0]["grad_norm"] == norm and 0.49 < res[0]["stats"][0]["clip_coef"] < 0.51
    RQ.assert_is_state(res, state, cfg)


BLOCK0 = 640                                                       # a block of 32 inside rank 1's shard at world 2 and 3


def _plant(theta, gens, g):
    """Finite workers whose partial overflows against a planted residual: positive deltas of about
    1e38 in one block of 32 of every worker of generation g."""
    for w in gens[g]:
        w[BLOCK0:BLOCK0 + 32] = (theta[BLOCK0:BLOCK0 + 32].float() + 1e38).to(w.dtype)


@pytest.mark.parametrize("policy", ["raise", "drop"])
@pytest.mark.parametrize("world", [2, 3])
@pytest.mark.parametrize("cfg", EF_CONFIGS, ids=[i for i, c in zip(CID, CONFIGS) if c[2]])
def test_refusal_after_the_exchange_restores_the_residual(oracle, world, cfg, policy):
    """Every worker is finite, but rank 1's p + r overflows in one block: it ships with scale byte
    255, the mean has exactly 32 non-finite elements, and the step refuses on every rank with the
    residual as it was."""
    K = 2 * world
    layout, theta, gens = population(SHAPES, F32, BF16, K, steps=3)
    _plant(theta, gens, 1)
    saved = {}

    def prepare(sync, g):
        if g == 1 and sync.rank == 1:
            saved["r"] = sync.residual[BLOCK0:BLOCK0 + 32].clone()
            sync.residual[BLOCK0:BLOCK0 + 32] = 3.3e38
        if g == 2 and sync.rank == 1:                              # the operator repairs what they planted
            sync.residual[BLOCK0:BLOCK0 + 32] = saved["r"]
    # the restatement first: the planted step's mean counts exactly the block
    n_pad, buckets = (2048, [(0, 1024), (1024, 2048)]) if world == 2 else (3072, [(0, 1536), (1536, 3072)])
    assert any(b + (e - b) // world <= BLOCK0 < b + 2 * (e - b) // world for b, e in buckets)   # rank 1 owns it
    state = RQ.state0(theta, n_pad, world, cfg)
    f_in, f_out = cfg[0], OTHER[cfg[0]] if cfg[1] else None
    RQ.compose(oracle, state, [G.padded(w, n_pad) for w in gens[0]], world, buckets, f_in, f_out, list(range(K)), 1.0)
    trial = {k: (v.clone() if isinstance(v, torch.Tensor) else [x.clone() for x in v] if isinstance(v, list) else v)
             for k, v in state.items()}
    trial["residual"][1][BLOCK0:BLOCK0 + 32] = 3.3e38
    _, nfm = RQ.compose(oracle, trial, [G.padded(w, n_pad) for w in gens[1]], world, buckets, f_in, f_out,
                        list(range(K)), 1.0)
    assert nfm == 32
    res = RQ.run_q(world, layout, F32, BF16, theta, gens, CPU, kernels=RQ.NumpyGuardQKernels(oracle),
                   bucket_elems=1024, guard=OuterGuard(on_nonfinite=policy), prepare=prepare, **_kw(cfg))
    assert res[0]["n_pad"] == n_pad and res[0]["buckets"] == buckets
    _same_stats(res)
    st = res[0]["stats"][1]
    assert st["nonfinite_mean"] == 32 and st["nonfinite"] == [0] * K and st["dropped"] == []
    for r in res:
        err = r["errors"][1]
        assert r["errors"][0] is None and r["errors"][2] is None
        assert isinstance(err, NonFiniteWorkers) and err.nonfinite_mean == 32 and err.nonfinite == [0] * K
        assert RQ.same_state(r["before"], r["after"])
    assert res[1]["after"]["residual"][BLOCK0] == 3.3e38
    # generations 0 and 2 alone, unguarded
    plain = RQ.run_q(world, layout, F32, BF16, theta, [gens[0], gens[2]], CPU, kernels=S.NumpySrKernels(oracle),
                     bucket_elems=1024, **_kw(cfg))
    for r, p in zip(res, plain):
        assert RQ.same_state(r["steps"][-1], p["steps"][-1])
