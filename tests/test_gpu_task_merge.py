"""ops.task_merge_list on the GPU against tests/task_merge_reference.py, over one tensor list whose sizes hit
every path: empty, sub-vector, tile edge, chunk edge, chunk + 1, a view offset by one element (the scalar body)."""
import numpy as np
import pytest
import torch

from evolutionarydistributedtraining_amd import EdtError, merge, ops
from tests import task_merge_reference as R

pytestmark = pytest.mark.gpu

SIZES = R.SIZES
T = len(SIZES)
F32, BF16 = torch.float32, torch.bfloat16
DEV = torch.device("cuda:0")
SEED, STEP, LAM = 0x1234567890abcdef, 5, 0.75


def lay(arrays, dtype, offset_all=False):
    """One allocation per tensor; the last tensor (with offset_all: every one) is a view one element into its own."""
    out = []
    for t, a in enumerate(arrays):
        off = int(offset_all or t == len(arrays) - 1)
        buf = torch.empty(a.size + off, dtype=dtype, device=DEV)
        buf[off:].copy_(torch.from_numpy(a).to(dtype))
        out.append(buf[off:])
    return out


widened = lambda ts: [t.float().cpu().numpy() for t in ts]
bits = lambda ts: [t.cpu().view(torch.int16 if t.dtype == BF16 else torch.int32) for t in ts]


@pytest.mark.parametrize("K", [1, 3, 8, 9])
@pytest.mark.parametrize("gdt,wdt,odt", [(F32, F32, F32), (BF16, BF16, BF16), (F32, BF16, F32)])
@pytest.mark.parametrize("normalize", [True, False])
@pytest.mark.parametrize("method", sorted(R.METHODS))
def test_task_merge(method, normalize, gdt, wdt, odt, K):
    consensus = R.METHODS[method][0]
    bf16_out = odt == BF16

    def run(bases, models, weights, dens, inplace=False, offset_all=False):
        b = lay(bases, gdt, offset_all)
        m = [lay(list(mk), wdt, offset_all) for mk in zip(*models)]
        o = None if inplace else lay([np.zeros(n, dtype=np.float32) for n in SIZES], odt, offset_all)
        ops.task_merge_list(b, m, o, weights=weights, densities=dens, lam=LAM, consensus=consensus, normalize=normalize,
                            seed=SEED, step=STEP)
        return b if inplace else o, b, m

    # 1. bit for bit against the float32 restatement, out= and in place; 2. the same bits re-laid unaligned
    weights = [[0.3 + 0.2 * ((k + 2 * t) % 4) for t in range(T)] for k in range(K)]
    dens = R.densities(method, K, T)
    w, c, drop = R.coefficients(weights, dens)
    keep = R.keep_masks(SIZES, drop, SEED, STEP)
    bases, models = R.normal_inputs(K, SIZES)
    out, b, m = run(bases, models, weights, dens)
    bw, mw = widened(b), [widened(mk) for mk in m]
    want = [R.merge_f32(bw[t], np.stack([mk[t] for mk in mw]).reshape(K, -1), w[:, t], c[:, t], keep[t], LAM, consensus,
                        normalize, bf16_out)[0] for t in range(T)]
    want_bits = bits([torch.from_numpy(x).to(odt) for x in want])
    assert all(torch.equal(g, x) for g, x in zip(bits(out), want_bits))
    assert all(torch.equal(g, x) for g, x in zip(bits(run(bases, models, weights, dens, inplace=True)[0]), want_bits))
    assert all(torch.equal(g, x) for g, x in zip(bits(run(bases, models, weights, dens, offset_all=True)[0]), want_bits))

    # 3. against float64 on dyadic inputs: exact sums, the election cannot differ, three roundings
    weights = [[2.0 ** ((k + t) % 3 - 1) for t in range(T)] for k in range(K)]
    dens = R.densities(method, K, T, dyadic=True)
    w, c, drop = R.coefficients(weights, dens)
    keep = R.keep_masks(SIZES, drop, SEED, STEP)
    bases, models = R.dyadic_inputs(K, SIZES)
    out = run(bases, models, weights, dens)[0]
    for t in range(T):
        ref, _, lq = R.merge_f64(bases[t], models[t], w[:, t], c[:, t], keep[t], LAM, consensus, normalize)
        err = np.abs(out[t].float().cpu().numpy().astype(np.float64) - ref)
        assert np.all(err <= R.bound(bases[t], lq, ref, bf16_out)), (t, err.max())


def test_long_list_searches_the_global_table():
    """8200 tensors of 8 elements (every other base view off a 16-byte boundary) pack like one tensor of 65,600."""
    n, K = 8200 * 8, 2
    bases, models = R.normal_inputs(K, [n])
    w, c, drop = R.coefficients([[0.5], [1.5]], [[0.5], [0.5]])
    want = R.merge_f32(bases[0], models[0], w[:, 0], c[:, 0], R.keep_masks([n], drop, SEED, STEP)[0], LAM, True, True)[0]
    b = torch.zeros(2 * n)                                      # tensor t at 16 t (+ 1 for odd t)
    starts = [16 * t + (t & 1) for t in range(8200)]
    for t, s in enumerate(starts):
        b[s:s + 8] = torch.from_numpy(bases[0][8 * t:8 * t + 8])
    b = b.to(DEV)
    m = [torch.from_numpy(models[0][k]).to(DEV) for k in range(K)]
    out = torch.empty(n, device=DEV)
    ops.task_merge_list([b[s:s + 8] for s in starts], [[mk[8 * t:8 * t + 8] for t in range(8200)] for mk in m],
                        [out[8 * t:8 * t + 8] for t in range(8200)], weights=[0.5, 1.5], densities=0.5, lam=LAM,
                        consensus=True, seed=SEED, step=STEP)
    assert torch.equal(out.cpu().view(torch.int32), torch.from_numpy(want).view(torch.int32))


def tiny(seed):
    torch.manual_seed(seed)
    blk = lambda: torch.nn.ModuleDict({"self_attn": torch.nn.Linear(8, 8, bias=False), "mlp": torch.nn.Linear(8, 13, bias=False)})
    return torch.nn.ModuleDict({"embed": torch.nn.Embedding(5, 8), "layers": torch.nn.ModuleList([blk(), blk()])}).to(DEV)


@pytest.mark.parametrize("inplace", [True, False])
def test_models_into_matches_list_call(inplace):
    cfg = {"merge_method": "dare_ties", "base_model": "B", "parameters": {"normalize": True, "lambda": 0.5},
           "models": [{"model": "B"}] + [
               {"model": f"M{k}", "parameters": {
                   "weight": [{"filter": "self_attn", "value": [0.25, 1.0 + k]}, {"filter": "mlp", "value": [1.0, 0.5]},
                              {"value": 0.5}],
                   "density": [{"filter": "mlp", "value": [0.5, 1.0]}, {"value": 0.75}]}} for k in range(3)]}
    base = tiny(0)
    models = [tiny(1 + k) for k in range(3)]
    target = base if inplace else tiny(9)
    plan = merge.task_merge_plan(list(base.state_dict()), 2, cfg)
    assert [k for k, _, _ in plan] == list(base.state_dict()) and plan[1][1] == [0.25, 0.25, 0.25] and plan[4][2] == [1.0] * 3
    bases = [base.state_dict()[k].clone() for k, _, _ in plan]
    outs = [torch.empty_like(b) for b in bases]
    ops.task_merge_list(bases, [[m.state_dict()[k] for k, _, _ in plan] for m in models], outs,
                        weights=[[w[j] for _, w, _ in plan] for j in range(3)],
                        densities=[[d[j] for _, _, d in plan] for j in range(3)], lam=0.5, consensus=True, seed=3, step=1)
    merge.task_merge_models_into_(target, base, models, cfg, 2, seed=3, step=1)
    assert all(torch.equal(target.state_dict()[k], o) for (k, _, _), o in zip(plan, outs))
    with pytest.raises(EdtError, match="overlaps"):            # an output inside another operand
        ops.task_merge_list(bases[:1], [[outs[0]]], [outs[0]], weights=1.0)
