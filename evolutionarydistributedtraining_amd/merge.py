"""Model-level crossover math shared by the RL / EVOMERGE / LM surfaces.

The reference merges two state dicts key by key in Python, each key a numpy SLERP on the CPU
(EDT_RL/crossover.py:84-135, EDT_EVOMERGE/train/crossover.py:104-146). Here the per-key t values
are computed on the host exactly as the reference does, and the whole merge is three launches
(chunk sums, per-segment coefficients, blend) with one segment per key: over the parents' own
device tensors (ops.slerp_list, results optionally written straight into the target model), or
over two flat HBM arenas the parents are packed into when they are not on the device
(ops.slerp_arena).
"""
from __future__ import annotations

import numbers
import threading

import numpy as np
import torch

from . import ops
from ._lib import EdtError


# ------------------------------------------------------------------------------------------
# host-side scalar logic (bit-identical python-float arithmetic to the reference)

def lerp(t, v0, v1):
    """(1 - t) * v0 + t * v1 (EDT_RL/crossover.py:46-47, EDT_LM/train/crossover.py:50-51).

    Python numbers: plain float arithmetic (as interpolate_t uses it). torch tensors: one fused
    launch with torch's rounding in the tensors' dtype (output on the inputs' device). numpy
    arrays: float32 math as numpy does it, computed on the GPU, returned as numpy."""
    if isinstance(v0, numbers.Number) and isinstance(v1, numbers.Number):
        return (1 - t) * v0 + t * v1
    if isinstance(v0, np.ndarray) or isinstance(v1, np.ndarray):
        a = torch.from_numpy(np.ascontiguousarray(v0, dtype=np.float32))
        b = torch.from_numpy(np.ascontiguousarray(v1, dtype=np.float32))
        return lerp(t, a, b).numpy()
    dev = _compute_device(v0)
    a = v0.detach().to(dev).contiguous()
    b = v1.detach().to(device=dev, dtype=a.dtype).contiguous()
    out = ops.lerp(float(t), a.reshape(-1), b.reshape(-1)).view(a.shape)
    return out if v0.is_cuda else out.cpu()


def maybe_torch(v, is_torch):
    """numpy -> torch when the caller passed torch (EDT_LM/train/crossover.py:54-57; host helper
    of the reference's numpy SLERP, kept for callers that import it)."""
    if is_torch:
        return torch.from_numpy(v)
    return v


def normalize(v, eps):
    """v / ||v|| when the norm exceeds eps (EDT_LM/train/crossover.py:60-64; host helper on numpy
    arrays — the device SLERP forms the norms inside its stats pass)."""
    norm_v = np.linalg.norm(v)
    if norm_v > eps:
        v = v / norm_v
    return v


class LazyTensorLoader:
    """A model's state dict fetched once, on first use, then served per key on `device`
    (EDT_LM/train/crossover.py:87-102, EDT_EVOMERGE/train/crossover.py:86-101)."""

    def __init__(self, model, device="cpu"):
        self.model = model
        self.state_dict = None
        self.lock = threading.Lock()
        self.device = device

    def get_tensor(self, key):
        with self.lock:
            if self.state_dict is None:
                self.state_dict = self.model.state_dict()
            return self.state_dict[key].to(self.device)

    def flush(self):
        with self.lock:
            self.state_dict = None


def interpolate_t(layer_idx, num_layers, t_curve):
    """Piecewise-linear t over the layer index (EDT_RL/crossover.py:70-81)."""
    if layer_idx < 0:
        return t_curve[0]
    if layer_idx >= num_layers - 1:
        return t_curve[-1]
    position = layer_idx / (num_layers - 1) * (len(t_curve) - 1)
    lo = int(position)
    hi = min(lo + 1, len(t_curve) - 1)
    return lerp(position - lo, t_curve[lo], t_curve[hi])


def parse_t_parameters(merge_config_dict: dict):
    """{filter: curve} and the global t of a MergeKit-style config (EDT_RL/crossover.py:99-100)."""
    ts = merge_config_dict["parameters"]["t"]
    param_t = {p["filter"]: p["value"] for p in ts if "filter" in p}
    global_t = next((p["value"] for p in ts if "filter" not in p), 0.5)
    return param_t, global_t


def t_for_key(key: str, num_layers: int, param_t: dict, global_t):
    """The reference's key routing (EDT_RL/crossover.py:108-122): the t for `key`, or None when
    the key is skipped (a layer index beyond num_layers)."""
    if "layer" in key:
        layer_idx = int(key.split(".")[1])
        if layer_idx >= num_layers:
            return None
        if "self_attn" in key and "self_attn" in param_t:
            return interpolate_t(layer_idx, num_layers, param_t["self_attn"])
        if "mlp" in key and "mlp" in param_t:
            return interpolate_t(layer_idx, num_layers, param_t["mlp"])
        return global_t
    return global_t


_plan_memo: dict = {}


def merge_plan(keys, num_layers: int, merge_config_dict: dict):
    """[(key, t)] for the keys the merge covers (cached per (keys, num_layers, config))."""
    import json
    memo = (tuple(keys), num_layers, json.dumps(merge_config_dict, sort_keys=True, default=str))
    got = _plan_memo.get(memo)
    if got is None:
        if len(_plan_memo) > 16:
            _plan_memo.clear()
        got = _plan_memo[memo] = _merge_plan(keys, num_layers, merge_config_dict)
    return list(got)


def _merge_plan(keys, num_layers: int, merge_config_dict: dict):
    """[(key, t)] in state-dict order, skipped keys removed."""
    param_t, global_t = parse_t_parameters(merge_config_dict)
    out = []
    for k in keys:
        t = t_for_key(k, num_layers, param_t, global_t)
        if t is not None:
            out.append((k, float(t)))
    return out


# ------------------------------------------------------------------------------------------
# device-side merges

def _compute_device(*tensors) -> torch.device:
    for t in tensors:
        if isinstance(t, torch.Tensor) and t.is_cuda:
            return t.device
    if not torch.cuda.is_available():
        raise EdtError("no HIP device visible: the crossover kernels run on MI355X only")
    return torch.device("cuda", torch.cuda.current_device())


_plans: dict = {}

# The SLERP branch-decision mode of every merge below (and so of the rl / evomerge surfaces):
# None = the kernels' fp64 dot; an ops.RefDot = the reference host's own fp32 dot,
# bit for bit, on the segments it flags (set_reference_dot).
_ref_dot = None


def set_reference_dot(ref=None):
    """Decide the SLERP branch as the reference host does (ops.RefDot(threads, band)), or from the
    accurate fp64 dot (None, the default). Returns the previous setting."""
    global _ref_dot
    prev, _ref_dot = _ref_dot, ref
    return prev


def _plan_for(offsets, device, relative=False):
    key = (tuple(offsets), str(device), relative)
    plan = _plans.get(key)
    if plan is None:
        if len(_plans) > 8:
            _plans.clear()
        plan = _plans[key] = ops.make_slerp_plan(list(offsets), device, relative=relative)
    return plan


def _listable(tensors, dev) -> bool:
    """Device tensors the tensor-list kernels can address directly."""
    return all(isinstance(t, torch.Tensor) and t.device == dev and t.is_contiguous()
               and t.data_ptr() % 16 == 0 for t in tensors)


def _writes_are_safe(pairs, outs) -> bool:
    """out[i] may alias its own inputs exactly (the blend is element-wise, after every sum);
    any other overlap of an output with an input or another output is unsafe (ops.writes_safe)."""
    ts = [t for (a, b), o in zip(pairs, outs) for t in (a, b, o)]
    st = np.fromiter((t.data_ptr() for t in ts), dtype=np.int64, count=len(ts))
    nb = np.fromiter((t.numel() * t.element_size() for t in ts), dtype=np.int64, count=len(ts))
    return ops.writes_safe(st, nb)


def slerp_tensors(pairs, ts, out_dtype=torch.float32, device=None, dot_threshold=0.9995,
                  eps=1e-8, out=None) -> list[torch.Tensor]:
    """SLERP of each (v0, v1) pair with its own t, all in ONE multi-tensor pass.

    Inputs are upcast to float32 exactly like the reference's `.float().numpy()` when the two
    parents' dtypes differ; results are float32 (the reference returns float32) or `out_dtype`
    (rounded to nearest even, as load_state_dict into a bf16 model does). `out`: optional list of
    destination tensors (e.g. the target model's parameters, which may be the first parent's
    own tensors), written in place.

    Parents already on the device are read where they lie (edt_slerp_merge_list); anything
    else is first packed into two flat arenas (edt_slerp_merge)."""
    pairs = list(pairs)
    if not pairs:
        return []
    dev = device or _compute_device(*[t for p in pairs for t in p])
    in_dt = pairs[0][0].dtype
    if any(a.dtype != in_dt or b.dtype != in_dt for a, b in pairs) or in_dt not in (torch.float32, torch.bfloat16):
        in_dt = torch.float32
    offsets = [0]
    for a, b in pairs:
        if a.shape != b.shape:
            raise EdtError(f"parents disagree on a tensor shape: {tuple(a.shape)} vs {tuple(b.shape)}")
        offsets.append(offsets[-1] + a.numel())
    if out is not None:
        out = list(out)
        if len(out) != len(pairs) or any(o.shape != a.shape for o, (a, _) in zip(out, pairs)):
            raise EdtError("out must hold one tensor per pair, shaped like the parents")
        dts = {o.dtype for o in out}
        out_dtype = out[0].dtype if len(dts) == 1 else torch.float32   # mixed: round once, in copy_
    tt = torch.tensor([float(t) for t in ts], dtype=torch.float64).to(dev)
    if all(a.dtype == in_dt and b.dtype == in_dt for a, b in pairs) and _listable([t for p in pairs for t in p], dev):
        outs = out
        if outs is None:
            outs = [torch.empty(a.shape, dtype=out_dtype, device=dev) for a, _ in pairs]
        if _listable(outs, dev) and all(o.dtype == out_dtype for o in outs) and _writes_are_safe(pairs, outs):
            plan = _plan_for(offsets, dev, relative=True)
            # the tensors as they are (the C ABI reads data pointers: no autograd, no detach needed);
            # sizes and dtypes were checked above, so the binding skips its own per-tensor pass
            ops.SlerpListBinding(plan, [a for a, _ in pairs], [b for _, b in pairs], outs, checked=True).merge(
                tt, dot_threshold, eps, ref_dot=_ref_dot)
            return outs
    total = offsets[-1]
    v0 = torch.empty(total, dtype=in_dt, device=dev)
    v1 = torch.empty(total, dtype=in_dt, device=dev)
    for (a, b), s, e in zip(pairs, offsets[:-1], offsets[1:]):
        v0[s:e].copy_(a.detach().reshape(-1))
        v1[s:e].copy_(b.detach().reshape(-1))
    res = torch.empty(total, dtype=out_dtype, device=dev)
    plan = _plan_for(offsets, dev)
    ops.slerp_arena(plan, v0, v1, res, tt, dot_threshold, eps, ref_dot=_ref_dot)
    views = [res[s:e].view(a.shape) for (a, _), s, e in zip(pairs, offsets[:-1], offsets[1:])]
    if out is None:
        return views
    with torch.no_grad():
        for o, v in zip(out, views):
            o.copy_(v)
    return out


def slerp(t, v0, v1, DOT_THRESHOLD=0.9995, eps=1e-8):
    """SLERP of one tensor pair (EDT_RL/crossover.py:11-43): float32 result, on the inputs'
    device (CPU in, CPU out; numpy in, numpy out)."""
    as_numpy = isinstance(v0, np.ndarray) and isinstance(v1, np.ndarray)
    a = torch.from_numpy(np.ascontiguousarray(v0)) if isinstance(v0, np.ndarray) else v0
    b = torch.from_numpy(np.ascontiguousarray(v1)) if isinstance(v1, np.ndarray) else v1
    res = slerp_tensors([(a, b)], [t], dot_threshold=DOT_THRESHOLD, eps=eps)[0]
    if as_numpy:
        return res.cpu().numpy()
    on_device = (isinstance(v0, torch.Tensor) and v0.is_cuda) or (isinstance(v1, torch.Tensor) and v1.is_cuda)
    return res if on_device else res.cpu()


def slerp_state_dicts(sd1: dict, sd2: dict, plan, out_dtype=torch.float32, device=None,
                      dot_threshold=0.9995, eps=1e-8, out: dict | None = None) -> dict:
    """Merged state dict {key: tensor} for plan = [(key, t)] (see merge_plan). `out`: a state
    dict to write the results into (e.g. the target model's, == load_state_dict of the merge)."""
    keys = [k for k, _ in plan]
    res = slerp_tensors([(sd1[k], sd2[k]) for k in keys], [t for _, t in plan], out_dtype, device,
                        dot_threshold, eps, out=None if out is None else [out[k] for k in keys])
    return dict(zip(keys, res))


def _padded_offsets(ns):
    """Element offsets of tensors of sizes `ns` packed with every start on a 16-byte boundary
    (a multiple of 8 elements: the tensor-list kernels' alignment), and the total size."""
    ns = np.asarray(ns, dtype=np.int64)
    padded = (ns + 7) // 8 * 8
    offs = np.zeros(len(ns), dtype=np.int64)
    if len(ns):
        np.cumsum(padded[:-1], out=offs[1:])
    return offs, max(int(padded.sum()), 8)


def fresh_outputs(like, dtype, device) -> list[torch.Tensor]:
    """Tensors shaped like `like`, carved from ONE new buffer with every start on a 16-byte
    boundary: a merge's output apart from both parents, so it can take the single-pass form
    (ops.slerp_list) instead of the two-pass in-place one (the layout _rebind_merge writes)."""
    offs, total = _padded_offsets([t.numel() for t in like])
    buf = torch.empty(total, dtype=dtype, device=device)
    return [buf.as_strided(t.shape, _contig_strides(t.shape), a) for a, t in zip(offs.tolist(), like)]


def _contig_strides(shape):
    st, acc = [], 1
    for d in reversed(shape):
        st.append(acc)
        acc *= d
    return tuple(reversed(st))


def _spans(ts):
    st = np.fromiter((t.data_ptr() for t in ts), dtype=np.int64, count=len(ts))
    nb = np.fromiter((t.numel() * t.element_size() for t in ts), dtype=np.int64, count=len(ts))
    keep = nb > 0
    return st[keep], st[keep] + nb[keep]


def _overlaps_any(outs, ins) -> bool:
    """Some output byte span overlaps some input byte span (numpy: inputs sorted, running end)."""
    a_in, e_in = _spans(ins)
    a_out, e_out = _spans(outs)
    if a_in.size == 0 or a_out.size == 0:
        return False
    o = np.argsort(a_in, kind="stable")
    a_in, far = a_in[o], np.maximum.accumulate(e_in[o])
    i = np.searchsorted(a_in, e_out, side="left")               # input spans starting before e
    return bool(np.any((i > 0) & (far[np.maximum(i - 1, 0)] > a_out)))


class _NeedsStateDict(Exception):
    pass


def module_tensors(module: torch.nn.Module) -> dict:
    """module.state_dict()'s {key: tensor} — for a module whose state is its parameters (no
    persistent buffers, no state-dict hooks, no extra state), read in one walk of the module tree
    in state_dict's own key order (a module's parameters, then its children), without state_dict's
    per-module generator chain and per-tensor detach (the kernels take data pointers)."""
    out = {}
    base_extra = torch.nn.Module.get_extra_state

    def walk(m, pre):
        if m._state_dict_hooks or m._state_dict_pre_hooks or type(m).get_extra_state is not base_extra:
            raise _NeedsStateDict
        if m._buffers:
            for n, b in m._buffers.items():
                if b is not None and n not in m._non_persistent_buffers_set:
                    raise _NeedsStateDict
        for n, p in m._parameters.items():
            if p is not None:
                out[pre + n] = p
        for n, c in m._modules.items():
            if c is not None:
                walk(c, pre + n + ".")

    try:
        walk(module, "")
    except _NeedsStateDict:
        return module.state_dict()
    return out


def _pair_pointers(pairs, dev):
    """One pass over device-resident parent pairs: (v0 addresses, v1 addresses, sizes, dtype) as
    numpy arrays when the tensor-list kernels can address every tensor where it lies (one dtype,
    fp32 / bf16, on `dev`, contiguous, 16-byte aligned); None otherwise. Unequal shapes raise as
    slerp_tensors does."""
    if not pairs:
        return None
    dt = pairs[0][0].dtype
    if dt not in (torch.float32, torch.bfloat16):
        return None
    idx = dev.index if dev.index is not None else torch.cuda.current_device()
    p0, p1, ns = [], [], []
    for a, b in pairs:
        if a.dtype != dt or b.dtype != dt or not (a.is_cuda and b.is_cuda):
            return None
        if a.shape != b.shape:
            raise EdtError(f"parents disagree on a tensor shape: {tuple(a.shape)} vs {tuple(b.shape)}")
        if a.get_device() != idx or b.get_device() != idx or not (a.is_contiguous() and b.is_contiguous()):
            return None
        p0.append(a.data_ptr())
        p1.append(b.data_ptr())
        ns.append(a.numel())
    p0 = np.array(p0, dtype=np.uint64)
    p1 = np.array(p1, dtype=np.uint64)
    if np.any((p0 | p1) % np.uint64(16)):
        return None
    return p0, p1, np.array(ns, dtype=np.int64), dt


def _rebind_merge(params, keys, outs, sd1, sd2, plan, out_dtype, dev, dot_threshold, eps, bound=None) -> bool:
    """slerp_into_module_'s single-pass form, when it applies: the children written to ONE fresh
    buffer (16-byte aligned starts, addresses computed before any view of it exists), the merge
    launched, and only then — while the device runs it — the views carved and the parameters
    re-pointed at them. False (nothing done) when the form does not apply: a parent not addressable
    in place, an output dtype other than the merge's (a mixed-dtype module keeps its tensors), or
    outputs apart from both parents (written in place in one pass already). `bound` (a dict, the
    surface cache): receives what a repeat of this merge needs (_Bound)."""
    if any(o.dtype != out_dtype for o in outs):
        return False
    pairs = [(sd1[k], sd2[k]) for k in keys]
    meta = _pair_pointers(pairs, dev)
    if meta is None:
        return False
    p0, p1, ns, in_dt = meta
    if not all(o is a for o, (a, _) in zip(outs, pairs)):      # all: the reference's case, target == model_1
        if not (all(o.device == dev for o in outs) and _overlaps_any(outs, [t for p in pairs for t in p])):
            return False
    offs, total = _padded_offsets(ns)
    buf = torch.empty(total, dtype=out_dtype, device=dev)
    esz = buf.element_size()
    po = np.uint64(buf.data_ptr()) + offs.astype(np.uint64) * np.uint64(esz)
    offsets = [0]
    offsets.extend(np.cumsum(ns).tolist())
    splan = _plan_for(offsets, dev, relative=True)
    tt = torch.tensor([t for _, t in plan], dtype=torch.float64).to(dev)
    ops.SlerpListBinding.from_pointers(splan, p0, p1, po, in_dt, out_dtype, dev, keep=(buf, pairs)).merge(
        tt, dot_threshold, eps, ref_dot=_ref_dot)
    cur = torch.cuda.current_stream(dev)
    with torch.no_grad():                                        # overlaps the kernels
        for k, o, a in zip(keys, outs, offs.tolist()):
            # the parameter's old storage may be its last reference: the caching allocator must
            # not hand the block out again before the merge queued on this stream has read it
            # (it may have been allocated on another stream than the one the merge runs on)
            params[k].data.record_stream(cur)
            params[k].data = buf.as_strided(o.shape, _contig_strides(o.shape), a)
    if bound is not None:
        done = torch.cuda.Event()
        done.record(cur)                         # the launch that read the held memory
        bound.update(done=done)
        bound.update(keys=keys, ts=[t for _, t in plan], tt=tt, splan=splan, ns=ns, offs=offs, total=total,
                     in_dt=in_dt, out_dt=out_dtype, p0=po, p1=p1, buf=buf, shapes=[o.shape for o in outs],
                     hold2=[b.data for _, b in pairs],
                     ends=(params[keys[0]], params[keys[-1]], pairs[0][1], pairs[-1][1]))
    return True


def slerp_into_module_(module: torch.nn.Module, sd1: dict, sd2: dict, plan, out_dtype, device=None,
                       dot_threshold=0.9995, eps=1e-8, params: dict | None = None, bound: dict | None = None) -> None:
    """== module.load_state_dict(SLERP of sd1 / sd2 per plan) (EDT_EVOMERGE/train/crossover.py:142),
    in the fewest passes over HBM. When the module's own tensors are a parent's (the reference
    merges into model_1 itself) and everything is device-resident, the children are written to a
    FRESH buffer by the single-pass form and the module's parameters are then re-pointed at it
    (param.data = view, _rebind_merge): the same values as writing into the parent's tensors —
    which would force the two-pass form, whose blend re-reads both parents after every sum — in one
    pass over the parents (7B lineage: ~7 ms against ~11 ms). The parent's old storage is released
    once nothing else refers to it. Otherwise the merge writes into the module's tensors in place."""
    keys = [k for k, _ in plan]
    params = params if params is not None else dict(module.named_parameters(remove_duplicate=False))
    if all(k in params for k in keys):
        tsd, outs = None, [params[k] for k in keys]          # no state_dict walk: the parameters
    else:
        tsd = module.state_dict()
        outs = [tsd[k] for k in keys]
    dev = device or _compute_device(*[t for k in keys for t in (sd1[k], sd2[k])])
    if tsd is None and dev.type == "cuda" and keys and _rebind_merge(
            params, keys, outs, sd1, sd2, plan, out_dtype, dev, dot_threshold, eps, bound):
        return
    slerp_state_dicts(sd1, sd2, plan, out_dtype=out_dtype, device=device, dot_threshold=dot_threshold,
                      eps=eps, out=tsd if tsd is not None else dict(zip(keys, outs)))


class _Bound:
    """What merge_models_into_ needs to repeat a merge of model_2 into model_1 without host work
    before the launch (VERDICT r4 Next 3): the key plan and its device t, the chunk plan, the
    parents' addresses and sizes, the packing of the fresh output buffer — and strong references
    to the memory those addresses point at (model_1's tensors are views of `buf`, the previous
    merge's output; `hold2`: model_2's tensors), so a launch over the cached addresses only ever
    reads live memory of the recorded sizes, whatever the modules did meanwhile. Whether the
    modules still hold exactly these tensors is checked while the device runs the merge
    (_bound_merge); the entry dies with either module (weak references)."""

    def __init__(self, key, model_1, model_2, dev, rec):
        import weakref
        self.key, self.dev = key, dev
        drop = lambda _r, key=key, cache=_bound_cache, evict=_evict: evict(cache, key)   # safe at exit
        self.r1, self.r2 = weakref.ref(model_1, drop), weakref.ref(model_2, drop)
        for k, v in rec.items():
            setattr(self, k, v)
        self.all_keys = list(rec["all_keys"])
        self.offs_bytes = self.offs.astype(np.uint64) * np.uint64(torch.empty(0, dtype=self.out_dt).element_size())
        self.offs_list = self.offs.tolist()
        self.strides = [_contig_strides(s) for s in self.shapes]


_bound_cache: dict = {}


def _evict(cache: dict, key) -> None:
    """Drop a cached binding once the last launch that read its held memory (`done`, an event on
    the stream that launch ran on, whatever the device) has finished: the held tensors may be the
    last references to a parent's storage, which must not be reused while a merge reads it."""
    b = cache.pop(key, None)
    ev = getattr(b, "done", None)
    if ev is not None:
        try:
            ev.synchronize()
        except Exception:        # noqa: BLE001 - interpreter shutdown: the runtime may be gone
            pass


def clear_merge_cache() -> None:
    """Drop merge_models_into_'s cached bindings (and the references they hold)."""
    if _bound_cache and torch.cuda.is_available():
        torch.cuda.synchronize()                 # merges in flight may still read the held memory
    _bound_cache.clear()


def _bound_key(target, model_1, model_2, merge_config_dict, num_layers, dev):
    import json
    return (id(target), id(model_1), id(model_2), num_layers, str(dev),
            json.dumps(merge_config_dict, sort_keys=True, default=str))


def _bound_merge(b: _Bound, model_1, model_2) -> bool:
    """The cached merge: a fresh output buffer, the binding over the cached addresses, the launch —
    then, while the device runs it, the check that the modules still hold exactly the bound
    tensors (the walk, keys, Parameters, addresses, sizes, dtypes: what the uncached path reads
    before its launch) and the re-pointing of model_1's parameters at the new buffer. False
    (nothing re-pointed, the entry dropped, the output discarded) when anything changed: the
    caller merges the uncached way. A module whose first or last merged tensor moved (a reload, a
    re-pointing) is caught before the launch, so that case costs no wasted merge."""
    f1, l1, f2, l2 = b.ends
    if (f1.data_ptr() != int(b.p0[0]) or l1.data_ptr() != int(b.p0[-1]) or f2.data_ptr() != int(b.p1[0])
            or l2.data_ptr() != int(b.p1[-1])):
        _evict(_bound_cache, b.key)
        return False
    buf = torch.empty(b.total, dtype=b.out_dt, device=b.dev)
    po = np.uint64(buf.data_ptr()) + b.offs_bytes
    ops.SlerpListBinding.from_checked(b.splan, b.p0, b.p1, po, b.in_dt, b.out_dt, b.dev,
                                      keep=(buf, b.buf, b.hold2)).merge(b.tt, ref_dot=_ref_dot)
    cur = torch.cuda.current_stream(b.dev)
    sd1 = module_tensors(model_1)
    sd2 = module_tensors(model_2)
    ok = isinstance(sd1, dict) and list(sd1.keys()) == b.all_keys and all(
        isinstance(sd1[k], torch.nn.Parameter) for k in b.keys)
    if ok:
        pairs = [(sd1[k], sd2.get(k)) for k in b.keys]
        ok = all(y is not None for _, y in pairs)
    if ok:
        meta = _pair_pointers(pairs, b.dev)
        ok = (meta is not None and meta[3] == b.in_dt and np.array_equal(meta[0], b.p0)
              and np.array_equal(meta[1], b.p1) and np.array_equal(meta[2], b.ns)
              and [a.shape for a, _ in pairs] == b.shapes and next(model_1.parameters()).dtype == b.out_dt)
    b.done = torch.cuda.Event()
    b.done.record(cur)
    if not ok:
        _evict(_bound_cache, b.key)              # the launch read the held memory: let it finish
        return False
    with torch.no_grad():                        # overlaps the kernels
        for k, shp, st, off in zip(b.keys, b.shapes, b.strides, b.offs_list):
            p = sd1[k]
            p.data.record_stream(cur)
            p.data = buf.as_strided(shp, st, off)
    b.p0, b.buf = po, buf
    return True


def merge_models_into_(target: torch.nn.Module, model_1: torch.nn.Module, model_2: torch.nn.Module,
                       merge_config_dict: dict, num_layers: int, device=None) -> None:
    """EDT_EVOMERGE/train/crossover.py:114-142 without the save: the SLERP of model_1 / model_2's
    state (the key plan of merge_config_dict over num_layers) loaded into `target` (which may be
    model_1 itself, as the reference passes it): slerp_into_module_ when the keys match, else
    load_state_dict of the merged dict (which reports the mismatch as the reference's does).

    Merging into model_1 again with the same model_2 and config (a resident population's next
    generation) repeats the previous call's binding (_Bound): no module walk, key plan, per-tensor
    check, t upload or chunk-plan lookup before the launch — those checks run while the device
    merges, and a module that changed in between falls back to the uncached merge."""
    dev = torch.device(device) if device not in (None, "cpu") else None
    key = None
    if target is model_1 and model_2 is not model_1:
        key = _bound_key(target, model_1, model_2, merge_config_dict, num_layers, dev)
        b = _bound_cache.get(key)
        if b is not None and b.r1() is model_1 and b.r2() is model_2 and _bound_merge(b, model_1, model_2):
            return
    sd1 = module_tensors(model_1)
    sd2 = sd1 if model_2 is model_1 else module_tensors(model_2)
    plan = merge_plan(list(sd1.keys()), num_layers, merge_config_dict)
    out_dtype = next(target.parameters()).dtype
    tparams = sd1 if target is model_1 and isinstance(sd1, dict) else None
    tkeys = set(tparams) if tparams is not None else set(module_tensors(target))
    if tkeys == {k for k, _ in plan}:
        is_params = tparams is not None and all(isinstance(v, torch.nn.Parameter) for v in tparams.values())
        rec = {} if key is not None and is_params else None
        slerp_into_module_(target, sd1, sd2, plan, out_dtype, device=dev, params=tparams if is_params else None,
                           bound=rec)
        if rec:                                   # the single-pass rebind ran: remember it
            rec["all_keys"] = list(sd1.keys())
            if len(_bound_cache) >= 4:               # the oldest binding goes, once its last merge
                _evict(_bound_cache, next(iter(_bound_cache)))      # (any stream, any device) is done
            _bound_cache[key] = _Bound(key, model_1, model_2, rec["tt"].device, rec)
    else:
        target.load_state_dict(slerp_state_dicts(sd1, sd2, plan, out_dtype=out_dtype, device=dev))


# ------------------------------------------------------------------------------------------
# task-vector merges of K models of one base (MergeKit's task_arithmetic / dare_linear / dare_ties)

# merge_method -> (sign consensus, density used)
TASK_MERGE_METHODS = {"task_arithmetic": (False, False), "dare_linear": (False, True), "dare_ties": (True, True)}


def _routed_parameter(name: str, value, default):
    """A MergeKit parameter that is a scalar or a [{filter, value}] list, as t_for_key's arguments:
    ({filter: curve}, global value). A filtered scalar is a one-point curve."""
    if value is None:
        return {}, default
    if isinstance(value, numbers.Number):
        return {}, value
    if not (isinstance(value, (list, tuple)) and all(isinstance(p, dict) and "value" in p for p in value)):
        raise EdtError(f"{name}: a scalar or a [{{filter, value}}] list")
    curves = {p["filter"]: list(p["value"]) if isinstance(p["value"], (list, tuple)) else [p["value"]]
              for p in value if "filter" in p}
    return curves, next((p["value"] for p in value if "filter" not in p), default)


def task_merge_settings(merge_config_dict: dict) -> dict:
    """The per-call settings of a task-merge config: consensus (from merge_method), normalize and lam
    (top-level parameters; MergeKit's defaults, normalize on and lambda 1)."""
    method = merge_config_dict.get("merge_method")
    if method not in TASK_MERGE_METHODS:
        raise EdtError(f"merge_method {method!r}: one of {sorted(TASK_MERGE_METHODS)}")
    top = merge_config_dict.get("parameters") or {}
    return {"consensus": TASK_MERGE_METHODS[method][0], "normalize": bool(top.get("normalize", True)),
            "lam": float(top.get("lambda", 1.0))}


def task_merge_plan(keys, num_layers: int, merge_config_dict: dict):
    """[(key, [weight per model], [density per model])] for the keys a task-merge config covers:
    every model's `weight` and `density` (a scalar or a [{filter, value}] list, default 1) routed per
    key exactly as SLERP's t is (t_for_key / interpolate_t: self_attn / mlp curves over the layer
    index, the unfiltered value elsewhere, keys of layers beyond num_layers skipped). task_arithmetic
    takes every density as 1. The models are `models`' entries other than `base_model`, in order."""
    task_merge_settings(merge_config_dict)                  # refuses an unknown merge_method
    uses_density = TASK_MERGE_METHODS[merge_config_dict["merge_method"]][1]
    base = merge_config_dict.get("base_model")
    entries = [m for m in merge_config_dict.get("models", []) if m.get("model") != base or base is None]
    if not entries:
        raise EdtError("a task merge needs at least one model besides base_model")
    routed = []
    for m in entries:
        p = m.get("parameters") or {}
        routed.append((_routed_parameter("weight", p.get("weight"), 1.0),
                       _routed_parameter("density", p.get("density") if uses_density else None, 1.0)))
    out = []
    for k in keys:
        ws = [t_for_key(k, num_layers, *w) for w, _ in routed]
        if ws[0] is None:                                   # a layer beyond num_layers: skipped, as SLERP's plan does
            continue
        out.append((k, [float(x) for x in ws], [float(t_for_key(k, num_layers, *d)) for _, d in routed]))
    return out


_TASK_PAIRS = {(torch.float32, torch.float32), (torch.float32, torch.bfloat16), (torch.bfloat16, torch.bfloat16)}


def task_merge_tensors(bases, models, weights, densities=1.0, *, outs=None, out_dtype=None, device=None, lam=1.0,
                       consensus=False, normalize=True, seed=0, step=0) -> list[torch.Tensor]:
    """Task-vector merge of models[k][t] relative to bases[t] in ONE multi-tensor pass
    (ops.task_merge_list): the merged tensors, on the device, shaped like the bases. weights,
    densities: a scalar, [K] or [K][T]. Device tensors are read where they lie; anything else (CPU
    tensors, other dtypes than fp32 / bf16, a base / model dtype pair the kernel lacks: those are
    widened to fp32) is copied to the device tensor by tensor first. outs: destinations written in
    place (outs[t] may be bases[t] itself: the in-place form); out_dtype (without outs): fp32 or
    bf16, default the bases' dtype."""
    bases = list(bases)
    models = [list(m) for m in models]
    if not bases:
        return []
    if any(len(m) != len(bases) for m in models):
        raise EdtError("every model needs one tensor per base tensor")
    for m in models:
        for b, x in zip(bases, m):
            if x.shape != b.shape:
                raise EdtError(f"a model disagrees with the base on a tensor shape: {tuple(x.shape)} vs {tuple(b.shape)}")
    dev = device or _compute_device(*bases, *[x for m in models for x in m])
    gdts, wdts = {b.dtype for b in bases}, {x.dtype for m in models for x in m}
    gdt, wdt = (next(iter(gdts)), next(iter(wdts))) if len(gdts) == 1 and len(wdts) == 1 else (None, None)
    if (gdt, wdt) not in _TASK_PAIRS:
        gdt = wdt = torch.float32

    def resident(x, dt):
        x = x.detach()
        return x if x.device == dev and x.dtype == dt and x.is_contiguous() else x.to(device=dev, dtype=dt).contiguous()

    b_dev = [resident(b, gdt) for b in bases]
    m_dev = [[resident(x, wdt) for x in m] for m in models]
    if outs is not None:
        outs = list(outs)
        if len(outs) != len(bases) or any(o.shape != b.shape for o, b in zip(outs, bases)):
            raise EdtError("outs must hold one tensor per base tensor, shaped like it")
        odts = {o.dtype for o in outs}
        out_dtype = next(iter(odts)) if len(odts) == 1 else torch.float32      # mixed: round once, in copy_
    elif out_dtype is None:
        out_dtype = gdt
    if out_dtype not in (torch.float32, torch.bfloat16):
        out_dtype = torch.float32
    direct = outs is not None and all(o.device == dev and o.dtype == out_dtype and o.is_contiguous() for o in outs)
    res = [o.detach() for o in outs] if direct else [torch.empty(b.shape, dtype=out_dtype, device=dev) for b in bases]
    ops.task_merge_list(b_dev, m_dev, res, weights=weights, densities=densities, lam=lam, consensus=consensus,
                        normalize=normalize, seed=seed, step=step)
    if outs is None:
        return res
    if not direct:
        with torch.no_grad():
            for o, r in zip(outs, res):
                o.copy_(r)
    return outs


def task_merge_state_dicts(base_sd: dict, sds, plan, *, out: dict | None = None, out_dtype=None, device=None, lam=1.0,
                           consensus=False, normalize=True, seed=0, step=0) -> dict:
    """Merged state dict {key: tensor} for plan = [(key, weights, densities)] (task_merge_plan) of the
    models' state dicts `sds` relative to base_sd. out: a state dict to write the results into (it may
    be base_sd itself: in place). CPU tensors go to the device tensor by tensor; there is no arena form."""
    keys = [k for k, _, _ in plan]
    K = len(sds)
    if any(len(w) != K or len(d) != K for _, w, d in plan):
        raise EdtError("the plan holds one weight and one density per model")
    weights = [[w[k] for _, w, _ in plan] for k in range(K)]
    densities = [[d[k] for _, _, d in plan] for k in range(K)]
    res = task_merge_tensors([base_sd[k] for k in keys], [[sd[k] for k in keys] for sd in sds], weights, densities,
                             outs=None if out is None else [out[k] for k in keys], out_dtype=out_dtype, device=device,
                             lam=lam, consensus=consensus, normalize=normalize, seed=seed, step=step)
    return dict(zip(keys, res))


def task_merge_models_into_(target: torch.nn.Module, base_model: torch.nn.Module, models, merge_config_dict: dict,
                            num_layers: int, seed: int = 0, step: int = 0, device=None) -> None:
    """The task-vector merge of `models` relative to base_model that merge_config_dict describes
    (task_merge_plan, task_merge_settings), loaded into `target`: base_model itself (its tensors are
    rewritten in place, one pass) or another module with the same keys (written where its tensors
    lie). When the plan skips keys of the target the merged dict goes through load_state_dict, which
    reports the mismatch. seed / step pick DARE's random bits."""
    dev = torch.device(device) if device not in (None, "cpu") else None
    base_sd = module_tensors(base_model)
    sds = [module_tensors(m) for m in models]
    plan = task_merge_plan(list(base_sd.keys()), num_layers, merge_config_dict)
    settings = task_merge_settings(merge_config_dict)
    tsd = base_sd if target is base_model else module_tensors(target)
    out_dtype = next(target.parameters()).dtype
    if set(tsd) == {k for k, _, _ in plan}:
        task_merge_state_dicts(base_sd, sds, plan, out=tsd, device=dev, seed=seed, step=step, **settings)
    else:
        target.load_state_dict(task_merge_state_dicts(base_sd, sds, plan, out_dtype=out_dtype, device=dev, seed=seed,
                                                      step=step, **settings))


def uniform_dna_crossover(dna1, dna2):
    """Per gene, parent 1's value if np.random.rand() > 0.5 else parent 2's, with numpy's global
    RNG (EDT_LM/train/crossover.py:318-321, EDT_RL/crossover.py:167-170)."""
    assert len(dna1) == len(dna2), "DNA lengths must be the same for uniform crossover."
    from_first = [np.random.rand() > 0.5 for _ in dna1]     # one draw per gene, in gene order
    return [a if f else b for a, b, f in zip(dna1, dna2, from_first)]


def rl_t_per_segment(keys, num_layers: int | None = None):
    """The t of every key under run_slerp_merge's config (EDT_RL/crossover.py:146-164: the
    self_attn / mlp layer curves, global 0.5) routed as EDT_RL/crossover.py:108-122 routes it
    (t_for_key); num_layers defaults to 1 + the largest layer index among the keys. Skipped keys
    (a layer beyond num_layers) get the global t."""
    if num_layers is None:
        idx = [int(k.split(".")[1]) for k in keys if "layer" in k]
        num_layers = 1 + max(idx) if idx else 0
    param_t = {"self_attn": [0, 0.5, 0.3, 0.7, 1], "mlp": [1, 0.5, 0.7, 0.3, 0]}
    ts = []
    for k in keys:
        v = t_for_key(k, num_layers, param_t, 0.5)
        ts.append(0.5 if v is None else float(v))
    return ts
