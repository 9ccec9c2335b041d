"""The task-vector merges without a GPU: the two references against each other on the dyadic inputs (the GPU
test's float64 bound holds for the reference itself), plan routing, coefficients, the ABI's and ops' refusals."""
import ctypes

import numpy as np
import pytest
import torch

from evolutionarydistributedtraining_amd import EdtError, _lib, merge, ops
from tests import task_merge_reference as R

SIZES = R.SIZES


@pytest.mark.parametrize("normalize", [True, False])
@pytest.mark.parametrize("method", sorted(R.METHODS))
@pytest.mark.parametrize("K", [1, 3, 9])
def test_references_agree_on_dyadic_inputs(method, normalize, K):
    bases, models = R.dyadic_inputs(K, SIZES)
    w, c, drop = R.coefficients([[2.0 ** ((k + t) % 3 - 1) for t in range(len(SIZES))] for k in range(K)],
                                R.densities(method, K, len(SIZES), dyadic=True))
    keep = R.keep_masks(SIZES, drop, seed=7, step=3)
    for t, (B, M) in enumerate(zip(bases, models)):
        ref, sign64, lq = R.merge_f64(B, M, w[:, t], c[:, t], keep[t], 0.75, R.METHODS[method][0], normalize)
        for bf16 in (False, True):
            got, sign32 = R.merge_f32(B, M, w[:, t], c[:, t], keep[t], 0.75, R.METHODS[method][0], normalize, bf16)
            assert np.array_equal(sign32, sign64)
            assert np.all(np.abs(got - ref) <= R.bound(B, lq, ref, bf16))


def test_plan_routes_weight_and_density_per_key():
    cfg = {"merge_method": "dare_ties", "base_model": "B",
           "models": [{"model": "B"},
                      {"model": "M0", "parameters": {"weight": [{"filter": "self_attn", "value": [0, 1]}, {"value": 0.5}],
                                                     "density": [{"filter": "mlp", "value": [1.0, 0.5, 0.25]}]}},
                      {"model": "M1", "parameters": {"weight": 0.25, "density": 0.5}}],
           "parameters": {"normalize": False, "lambda": 0.5}}
    keys = ["embed.weight", "layers.0.self_attn.q.weight", "layers.1.self_attn.q.weight", "layers.1.mlp.up.weight",
            "layers.2.mlp.up.weight", "layers.3.mlp.up.weight", "layers.2.norm.weight"]
    assert merge.task_merge_plan(keys, 3, cfg) == [
        ("embed.weight", [0.5, 0.25], [1.0, 0.5]),
        ("layers.0.self_attn.q.weight", [0.0, 0.25], [1.0, 0.5]),
        ("layers.1.self_attn.q.weight", [0.5, 0.25], [1.0, 0.5]),
        ("layers.1.mlp.up.weight", [0.5, 0.25], [0.5, 0.5]),
        ("layers.2.mlp.up.weight", [0.5, 0.25], [0.25, 0.5]),          # layers.3: beyond num_layers, skipped
        ("layers.2.norm.weight", [0.5, 0.25], [1.0, 0.5])]
    assert merge.task_merge_settings(cfg) == {"consensus": True, "normalize": False, "lam": 0.5}
    cfg["merge_method"] = "task_arithmetic"                            # every density is 1
    assert all(d == [1.0, 1.0] for _, _, d in merge.task_merge_plan(keys, 3, cfg))
    with pytest.raises(EdtError, match="merge_method"):
        merge.task_merge_plan(keys, 3, dict(cfg, merge_method="slerp"))


def test_coefficients():
    w, c, drop = ops.task_merge_coefficients([0.5, 3.0], [[1.0, 0.5, 0.9], [0.25, 1e-9, 1.0]], 2, 3)
    assert drop.tolist() == [[0, 32768, 6554], [49152, 65535, 0]] and drop.dtype == np.uint32
    assert w.tolist() == [[0.5] * 3, [3.0] * 3] and w.dtype == c.dtype == np.float32
    want = [[0.5, 1.0, np.float32(0.5 / (1 - 6554 / 65536))], [12.0, np.float32(3.0 * 65536), 3.0]]
    assert c.tolist() == want
    for got, ref in zip((w, c, drop), R.coefficients(w, [[1.0, 0.5, 0.9], [0.25, 1e-9, 1.0]])):
        assert np.array_equal(got, ref)
    assert ops.task_merge_coefficients(2.0, 1.0, 3, 2)[1].tolist() == [[2.0, 2.0]] * 3
    bad = [(1.0, d, "density") for d in (0.0, -0.5, 1.5, float("nan"))] + [(w, 1.0, "finite") for w in (float("inf"), float("nan"), 1e39)]
    for w, d, msg in bad + [(3e38, 0.5, "finite"), ([1.0, 2.0, 3.0], 1.0, "weights")]:      # 3e38 / 0.5 overflows fp32
        with pytest.raises(EdtError, match=msg):
            ops.task_merge_coefficients(w, d, 2, 3)


def test_ops_refusals_before_the_device():
    b = torch.zeros(8)                                         # refused before any tensor is looked at
    for bases, models, kw, msg in (([], [], {}, "no models"), ([], [[]] * 65, {}, "at most"),
                                   ([b], [[b]], dict(densities=0.0), "density"), ([b], [[b]], dict(weights=[1.0, 2.0]), "weights"),
                                   ([b], [[b]], dict(lam=float("inf")), "lam")):
        with pytest.raises(EdtError, match=msg):
            ops.task_merge_list(bases, models, **{"weights": 1.0, **kw})


def _call(lib, K=2, T=2, gdt=0, wdt=0, odt=0, base=(0x1000, 0x2000), models=(0x3000, 0x4000, 0x5000, 0x6000),
          outs=(0x7000, 0x8000), numel=(8, 5), w=None, c=None, drop=None, lam=1.0, ws=0x100000, ws_bytes=None,
          tables=True):
    P, n = ctypes.c_void_p, max(1, K * T)
    arr = lambda xs: (P * max(1, len(xs)))(*xs)
    f32 = lambda xs: (ctypes.c_float * n)(*(xs if xs is not None else [1.0] * n))
    need = lib.edt_task_merge_list_workspace_bytes(T, K)
    return lib.edt_task_merge_list(arr(base) if tables else None, gdt, arr(models), wdt, K,
                                   None if outs is None else arr(outs), odt, (ctypes.c_uint64 * max(1, len(numel)))(*numel), T,
                                   f32(w), f32(c), (ctypes.c_uint32 * n)(*(drop or [0] * n)), lam, 1, 1, 0, 0, P(ws),
                                   need if ws_bytes is None else ws_bytes, None)


@pytest.mark.parametrize("kw,msg", [
    (dict(gdt=1, wdt=0), "dtype pair"), (dict(odt=2), "output dtype"), (dict(K=0), "out of range"),
    (dict(K=65), "out of range"), (dict(T=-1), "tensor count"), (dict(lam=float("nan")), "lambda"),
    (dict(lam=1e39), "lambda"), (dict(outs=None, odt=1), "in-place"), (dict(tables=False), "null tensor table"),
    (dict(base=(0x1000, 0)), r"base_t\[1\] is null"), (dict(models=(0x3000, 0x4000, 0, 0x6000)), r"model_k\[1\]\[0\] is null"),
    (dict(outs=(0, 0x8000)), r"out_t\[0\] is null"), (dict(w=[1.0, float("inf"), 1.0, 1.0]), "not finite"),
    (dict(c=[1.0, 1.0, float("nan"), 1.0]), "not finite"), (dict(drop=[0, 0, 65536, 0]), "65535"),
    (dict(ws=0), "workspace"), (dict(ws_bytes=8), "workspace"), (dict(ws=0x100004), "8-byte aligned"),
    (dict(outs=(0x1010, 0x8000)), "overlaps"),                 # out[0] inside base[0], not exactly it
    (dict(outs=(0x3000, 0x8000)), "overlaps"),                 # out[0] is a model
    (dict(outs=(0x1000, 0x2000), odt=1, gdt=0, wdt=1), "overlaps"),      # exact alias in another dtype
    (dict(outs=None, base=(0x1000, 0x1010)), "overlaps"),      # in place, two base tensors overlap
])
def test_abi_refusals(kw, msg):
    import re
    lib = _lib.load_library()
    assert _call(lib, **kw) == -1 and re.search(msg, lib.edt_last_error().decode()), lib.edt_last_error()
    assert _call(lib, T=0, numel=()) == 0 and _call(lib, numel=(0, 0), base=(0, 0)) == 0      # nothing to read
