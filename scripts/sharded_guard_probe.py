"""Probe: what ShardedOuterSync(guard=OuterGuard) costs on one GPU — 1.3B layout, fp32 theta, K = 8
bf16 workers, as rank 0 of 1 and of 8 behind a loopback communicator (every peer's partial or
worker slice of the owned shard is a copy of this rank's own, so the kernels see the N-rank step's
shapes, buffers and bytes; nothing is measured of the links, and no multi-GPU link time can be
measured here).

  kernel   edt_partial_sum_stats against its yardstick edt_sgd_apply_sum on the same shard and the
           same partials, alternating in this process for --rounds rounds, each launch between HIP
           events: the statistics pass reads a subset of the yardstick's bytes and writes none.
  step     a guarded step against an unguarded one per schedule (reduce, reduce_ordered, exact),
           alternating on one object (guard on / off), host wall time around step() + synchronize:
           a guarded step has host syncs, so device events alone would miss its cost.

    python scripts/sharded_guard_probe.py --out profiles/sharded_guard_probe.json
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


def loopback(world: int):
    from evolutionarydistributedtraining_amd.collectives import Collectives, _Done

    class Loopback(Collectives):
        """Rank 0 of `world` with no peers: an all-to-all delivers this rank's own first region from
        every source, a reduce-scatter and an all-gather leave the owned shard in place, and every
        peer's host object is this rank's own."""
        inplace = True

        def __init__(self):
            self.world, self.rank = world, 0

        def all_to_all(self, out, inp, async_op=False):
            out.view(world, -1).copy_(inp.view(world, -1)[0].expand(world, -1))
            return _Done()

        def reduce_scatter(self, out, inp, async_op=False):
            return _Done()

        def all_gather(self, out, inp, async_op=False):
            return _Done()

        def all_gather_object(self, obj):
            return [obj] * world

    return Loopback()


def summary(ms):
    return {"median_ms": round(statistics.median(ms), 4), "min_ms": round(min(ms), 4), "max_ms": round(max(ms), 4)}


def make_sync(layout, world, mode, dev, guard):
    from evolutionarydistributedtraining_amd.distributed import ShardedOuterSync
    s = ShardedOuterSync(layout, torch.float32, torch.bfloat16, 8 // world, dev, mode=mode, broadcast="theta",
                         comm=loopback(world), guard=guard)
    g = torch.Generator(device=dev).manual_seed(0)
    s.theta_buf.normal_(0, 0.02, generator=g)
    for w in s.worker_bufs:
        w.copy_(s.theta_buf)
        w.add_(torch.randn(s.n_pad, device=dev, generator=g).mul_(1e-3))
    return s


def kernel_pair(layout, world, rounds, dev):
    """edt_partial_sum_stats / edt_sgd_apply_sum alternating on rank 0's shard of the whole arena
    (one bucket) and its `world` partials."""
    from evolutionarydistributedtraining_amd import ops
    unit = world * 64
    n_pad = -(-layout.total // unit) * unit
    shard = n_pad // world
    g = torch.Generator(device=dev).manual_seed(1)
    theta = torch.empty(shard, device=dev).normal_(0, 0.02, generator=g)
    mom = torch.zeros(shard, device=dev)
    parts = [torch.empty(shard, device=dev).normal_(0, 1e-4, generator=g) for _ in range(world)]
    plan = ops.make_slerp_plan([0, shard], dev)
    ev = lambda: torch.cuda.Event(enable_timing=True)
    stats_ms, sgd_ms = [], []
    for i in range(rounds + 2):                                 # two warm-up rounds
        a, b, c = ev(), ev(), ev()
        a.record()
        ops.partial_sum_stats(parts, torch.float32, plan)
        b.record()
        ops.sgd_apply_sum(theta, parts, mom, True, 0.7, 0.9, True)
        c.record()
        torch.cuda.synchronize()
        if i >= 2:
            stats_ms.append(a.elapsed_time(b))
            sgd_ms.append(b.elapsed_time(c))
    stats_bytes = shard * 4 * world
    sgd_bytes = shard * (4 * world + 16)
    out = {"world": world, "nacc": world, "shard_elems": shard, "chunks": plan.nchunks,
           "partial_sum_stats": dict(summary(stats_ms), bytes=stats_bytes,
                                     fraction_of_8TBps=round(stats_bytes / statistics.median(stats_ms) / PEAK_BYTES_PER_MS, 4)),
           "sgd_apply_sum": dict(summary(sgd_ms), bytes=sgd_bytes,
                                 fraction_of_8TBps=round(sgd_bytes / statistics.median(sgd_ms) / PEAK_BYTES_PER_MS, 4))}
    out["stats_over_yardstick"] = round(statistics.median(stats_ms) / statistics.median(sgd_ms), 4)
    out["stats_exceeds_yardstick"] = statistics.median(stats_ms) > statistics.median(sgd_ms)
    del theta, mom, parts
    gc.collect()
    torch.cuda.empty_cache()
    return out


def step_pair(layout, world, mode, rounds, dev):
    """A guarded and an unguarded step alternating on one object."""
    from evolutionarydistributedtraining_amd.diloco import OuterGuard
    guard = OuterGuard(max_grad_norm=1e9)
    s = make_sync(layout, world, mode, dev, guard)
    ms = {"guarded": [], "unguarded": []}
    for i in range(rounds + 2):
        for name, g in (("unguarded", None), ("guarded", guard)):
            s.guard = g
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            s.step()
            torch.cuda.synchronize()
            if i >= 2:
                ms[name].append((time.perf_counter() - t0) * 1e3)
    s.guard = guard
    gb, kb = s.guard_bytes(), s.kernel_bytes()
    gm, um = statistics.median(ms["guarded"]), statistics.median(ms["unguarded"])
    out = {"world": world, "mode": mode, "buckets": len(s.buckets), "guarded": summary(ms["guarded"]),
           "unguarded": summary(ms["unguarded"]), "guard_ms": round(gm - um, 4), "guard_bytes": gb, "kernel_bytes": kb,
           "guard_fraction_of_8TBps": round(gb / max(gm - um, 1e-9) / PEAK_BYTES_PER_MS, 4),
           "grad_norm": s.last_stats["grad_norm"], "clip_coef": s.last_stats["clip_coef"]}
    del s
    gc.collect()
    torch.cuda.empty_cache()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=10)
    ap.add_argument("--layout", default="gpt_1p3b")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sharded_guard_probe.json"))
    a = ap.parse_args()
    from evolutionarydistributedtraining_amd import _lib as L
    from evolutionarydistributedtraining_amd.layouts import LAYOUTS
    dev = torch.device("cuda:0")
    layout = LAYOUTS[a.layout]()
    kernels, steps = [], []
    for world in (1, 8):
        kernels.append(kernel_pair(layout, world, a.rounds, dev))
        print(json.dumps(kernels[-1]), flush=True)
    for world in (1, 8):
        for mode in ("reduce", "reduce_ordered", "exact"):
            steps.append(step_pair(layout, world, mode, a.rounds, dev))
            print(json.dumps(steps[-1]), flush=True)
    res = {"probe": "sharded_guard_probe", "layout": a.layout, "elements": layout.total, "K": 8, "theta": "f32",
           "workers": "bf16", "rounds": a.rounds, "device": torch.cuda.get_device_name(0),
           "library_sha256": L.library_sha256(),
           "note": "one GPU, loopback communicator: local kernels and host syncs only; no multi-GPU link time can be "
                   "measured here. Kernel times are HIP events, step times host wall time around step() + synchronize.",
           "kernels": kernels, "steps": steps}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
