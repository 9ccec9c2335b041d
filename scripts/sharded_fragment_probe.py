"""Probe: the sharded fragment step on one GPU — 1.3B layout, fp32 theta, K = 8 fp32 workers,
FragmentPlan.strided P = 4, world 1 (a loopback communicator: the collectives are device copies of
the compact buffers, nothing moves between devices, no link time can be measured here).

  kernels  the three piece-list kernels over one whole fragment's pieces, each alternating with its
           non-list sibling(s) on packed copies of the same bytes, every launch between HIP events:
             edt_delta_partial_list       / edt_delta_partial
             edt_sgd_sum_list_to          / edt_sgd_apply_sum
             edt_theta_scatter_mix_list   / edt_broadcast_theta (+ one edt_lerp per worker below mix 1)
  step     a whole step_fragment (host wall time around the call + synchronize) against
           ShardedOuterSync(mode="reduce_ordered").step(broadcast=True) over the whole arena: what a
           multi-GPU user who wants fragments runs without this class.
  wire     wire_bytes(p) against the whole step's, at N = 2, 4, 8: computed from byte counts,
           UNMEASURED on a multi-GPU node.

    python scripts/sharded_fragment_probe.py --out profiles/sharded_fragment_probe.json
"""
from __future__ import annotations

import argparse
import gc
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

PEAK_BYTES_PER_MS = 8e9         # 8 TB/s
K = 8


def summary(ms, nbytes):
    med = statistics.median(ms)
    return {"median_ms": round(med, 4), "min_ms": round(min(ms), 4), "max_ms": round(max(ms), 4), "bytes": nbytes,
            "fraction_of_8TBps": round(nbytes / med / PEAK_BYTES_PER_MS, 4)}


def timed(fns, rounds):
    """The callables alternating for `rounds` rounds after two warm-up ones, each between HIP
    events -> one list of milliseconds per callable."""
    ms = [[] for _ in fns]
    for i in range(rounds + 2):
        evs = [torch.cuda.Event(enable_timing=True) for _ in range(len(fns) + 1)]
        evs[0].record()
        for f, e in zip(fns, evs[1:]):
            f()
            e.record()
        torch.cuda.synchronize()
        if i >= 2:
            for j in range(len(fns)):
                ms[j].append(evs[j].elapsed_time(evs[j + 1]))
    return ms


def fill(sync, dev):
    g = torch.Generator(device=dev).manual_seed(0)
    theta = sync.theta.flat if hasattr(sync.theta, "flat") else sync.theta
    theta.normal_(0, 0.02, generator=g)
    for w in sync.workers:
        w.flat.copy_(theta)
        w.flat.add_(torch.randn(theta.numel(), device=dev, generator=g).mul_(1e-3))


def kernels_and_step(layout, plan, p, rounds, dev):
    from evolutionarydistributedtraining_amd import ShardedFragmentSync, ops
    from evolutionarydistributedtraining_amd.collectives import VirtualWorld
    s = ShardedFragmentSync(layout, plan, torch.float32, torch.float32, K, dev, comm=VirtualWorld(1).comm(0))
    fill(s, dev)
    F = plan.numel(p)
    pc = plan.pieces(p, 0, F)
    arena = lambda buf: [buf[a:a + n] for a, _, n in pc]
    frag = lambda buf: [buf[f:f + n] for _, f, n in pc]
    pack = lambda buf: torch.cat(arena(buf))
    th, ws = arena(s.theta.flat), [arena(w.flat) for w in s.workers]
    th_p, ws_p = pack(s.theta.flat), [pack(w.flat) for w in s.workers]
    acc_p, mom_p = torch.zeros(F, device=dev), torch.zeros(F, device=dev)
    out = {"fragment": p, "fragment_elems": F, "pieces": len(pc), "aligned_pieces": sum(
        all(t.data_ptr() % 16 == 0 for t in (a, b)) for a, b in zip(th, frag(s.send)))}
    # phase 1 and phase 2 and their siblings
    b1 = F * (K * 4 + 4 + 4)
    b2 = F * (4 + 4 + 4 + 8)
    ms = timed([lambda: ops.delta_partial_list(th, ws, K, frag(s.send)),
                lambda: ops.delta_partial(th_p, ws_p, K, acc_p),
                lambda: ops.sgd_sum_list_to(th, [frag(s.send)], frag(s.mom[p]), True, 0.7, 0.9, True, frag(s.gathered)),
                lambda: ops.sgd_apply_sum(th_p, [acc_p], mom_p, True, 0.7, 0.9, True)], rounds)
    out["delta_partial_list"], out["delta_partial"] = summary(ms[0], b1), summary(ms[1], b1)
    out["sgd_sum_list_to"], out["sgd_apply_sum"] = summary(ms[2], b2), summary(ms[3], b2)
    del acc_p, mom_p
    # phase 3 below mix 1 (every destination read and rewritten) and at mix 1 (the overwrite)
    v = torch.empty(F, device=dev)

    def sibling_blend():
        ops.broadcast_theta(th_p, [v])
        for w in ws_p:
            ops.lerp(0.5, w, v, out=w)

    ms = timed([lambda: ops.theta_scatter_mix_list(th, frag(s.gathered), ws, 0.5), sibling_blend,
                lambda: ops.theta_scatter_mix_list(th, frag(s.gathered), ws, 1.0),
                lambda: ops.broadcast_theta(th_p, ws_p)], rounds)
    out["theta_scatter_mix_list_mix0.5"] = summary(ms[0], F * (4 + 4 + 2 * K * 4))
    out["broadcast_theta_plus_lerp_mix0.5"] = summary(ms[1], F * (4 + 4) + K * F * 12)
    out["theta_scatter_mix_list_mix1"] = summary(ms[2], F * (4 + 4 + K * 4))
    out["broadcast_theta_mix1"] = summary(ms[3], F * (4 + K * 4))
    for a, b in (("delta_partial_list", "delta_partial"), ("sgd_sum_list_to", "sgd_apply_sum"),
                 ("theta_scatter_mix_list_mix0.5", "broadcast_theta_plus_lerp_mix0.5"),
                 ("theta_scatter_mix_list_mix1", "broadcast_theta_mix1")):
        out[a]["over_sibling"] = round(out[a]["median_ms"] / out[b]["median_ms"], 4)
    del th_p, ws_p, v
    gc.collect()
    torch.cuda.empty_cache()
    # the whole fragment step, every fragment once per round
    fill(s, dev)
    step_ms = {q: [] for q in range(len(plan))}
    for i in range(rounds + 2):
        for q in range(len(plan)):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            s.step_fragment(q, 0.5)
            torch.cuda.synchronize()
            if i >= 2:
                step_ms[q].append((time.perf_counter() - t0) * 1e3)
    steps = [dict(summary(step_ms[q], s.kernel_bytes(q, True, 0.5)), fragment=q, fragment_elems=plan.numel(q),
                  buckets=len(s.buckets[q])) for q in range(len(plan))]
    del s, th, ws
    gc.collect()
    torch.cuda.empty_cache()
    return out, steps


def whole_step(layout, rounds, dev):
    from evolutionarydistributedtraining_amd.collectives import VirtualWorld
    from evolutionarydistributedtraining_amd.distributed import ShardedOuterSync
    s = ShardedOuterSync(layout, torch.float32, torch.float32, K, dev, mode="reduce_ordered", broadcast="theta",
                         comm=VirtualWorld(1).comm(0))
    fill(s, dev)
    ms = []
    for i in range(rounds + 2):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        s.step(broadcast=True)
        torch.cuda.synchronize()
        if i >= 2:
            ms.append((time.perf_counter() - t0) * 1e3)
    out = dict(summary(ms, s.kernel_bytes(broadcast=True)), buckets=len(s.buckets))
    del s
    gc.collect()
    torch.cuda.empty_cache()
    return out


def wire(layout, plan):
    """Byte counts only: a fragment step's wire bytes against the whole reduce_ordered step's."""
    rows = []
    for world in (2, 4, 8):
        unit = world * 64
        f = (world - 1) / world
        whole = int(f * (-(-layout.total // unit) * unit) * 8)
        frags = [int(f * (-(-plan.numel(p) // unit) * unit) * 8) for p in range(len(plan))]
        rows.append({"world": world, "whole_step_bytes": whole, "fragment_step_bytes": frags,
                     "peak_ratio": round(max(frags) / whole, 4)})
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--layout", default="gpt_1p3b")
    ap.add_argument("--fragments", type=int, default=4)
    ap.add_argument("--fragment", type=int, default=1)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sharded_fragment_probe.json"))
    a = ap.parse_args()
    from evolutionarydistributedtraining_amd import FragmentPlan, _lib as L
    from evolutionarydistributedtraining_amd.layouts import LAYOUTS
    dev = torch.device("cuda:0")
    layout = LAYOUTS[a.layout]()
    plan = FragmentPlan.strided(layout, a.fragments)
    kernels, steps = kernels_and_step(layout, plan, a.fragment, a.rounds, dev)
    print(json.dumps(kernels), flush=True)
    print(json.dumps(steps), flush=True)
    whole = whole_step(layout, a.rounds, dev)
    print(json.dumps(whole), flush=True)
    res = {"probe": "sharded_fragment_probe", "layout": a.layout, "elements": layout.total, "K": K, "theta": "f32",
           "workers": "f32", "plan": f"strided P={a.fragments}", "world": 1, "rounds": a.rounds,
           "device": torch.cuda.get_device_name(0), "library_sha256": L.library_sha256(),
           "note": "one GPU, world 1: the collectives are device copies, nothing moves between devices. Kernel times "
                   "are HIP events; step times are host wall time around the call + synchronize, mix 0.5. The wire "
                   "rows are byte counts, unmeasured on a multi-GPU node.",
           "kernels": kernels, "step_fragment": steps, "whole_step_broadcast": whole, "wire_bytes": wire(layout, plan)}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
