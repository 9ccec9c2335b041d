"""Probe: handing the new theta to the local workers inside the sharded step's own pass
(ShardedOuterSync.step(broadcast=True)) against the copies it replaces, on one GPU, 1.3B layout,
fp32 theta, the loopback communicator of scripts/reduce_q_probe.py and 20 buckets.

Groups: ranks 1 / 8 (K_local 8 / 1) x bf16 / fp32 workers. In each, on the buckets, buffers and
packed bytes of one reduce_q step with gather_format=mxfp8 (u_recv holds the real blocks that step
left), one pass over the 20 buckets of
  fused    (a) edt_apply_delta_q, then K_local `w.copy_(theta)` per bucket — the only way to refresh
               the workers before this entry existed: the yardstick
           (b) edt_apply_delta_q_bcast
  replica  (a) K_local `w.copy_(theta)` per bucket
           (b) edt_broadcast_theta
is timed between two HIP events: the median of --steps passes after --warmup. (a) and (b) alternate
in this process on the same operands for --rounds rounds; the median of the rounds and their range
are reported beside the ratio of algorithmic bytes. Local kernels only: nothing is measured of the
links, and no multi-GPU node has run the schedule.

    python scripts/sharded_bcast_probe.py --out profiles/sharded_bcast_probe.json
"""
from __future__ import annotations

import argparse
import gc
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))

Q8 = 1 + 1 / 32                 # mxfp8 bytes per element


def timed(fn, steps, warmup):
    ms = []
    for i in range(warmup + steps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        if i >= warmup:
            ms.append(a.elapsed_time(b))
    return statistics.median(ms)


def summary(rows):
    return {"ms": round(statistics.median(rows), 4), "min_ms": round(min(rows), 4), "max_ms": round(max(rows), 4),
            "rounds_ms": [round(r, 4) for r in rows]}


def group(layout, wdt, world, a, dev):
    from evolutionarydistributedtraining_amd import ops
    from evolutionarydistributedtraining_amd.distributed import ShardedOuterSync
    from reduce_q_probe import loopback
    k_local, gf = 8 // world, "mxfp8"
    s = ShardedOuterSync(layout, torch.float32, wdt, k_local, dev, mode="reduce_q", broadcast="theta",
                         comm=loopback(world), error_feedback=False, gather_format=gf)
    g = torch.Generator(device=dev).manual_seed(0)
    s.theta_buf.normal_(0, 0.02, generator=g)
    for w in s.worker_bufs:
        w.copy_(s.theta_buf)
        w.add_(torch.randn(s.n_pad, device=dev, generator=g).mul_(1e-3))
    s.step()                    # u_recv now holds every owner's real blocks
    torch.cuda.synchronize()
    th, ws = s.theta_buf, s.worker_bufs
    cuts = [(b, e, s.u_recv[s._q_bytes(b, gf):s._q_bytes(e, gf)], (e - b) // world) for b, e in s.buckets]

    def copies(b, e):
        for w in ws:
            w[b:e].copy_(th[b:e])

    def fused_a():
        for b, e, u, region in cuts:
            ops.apply_delta_q(th[b:e], u, region, gf)
            copies(b, e)

    def fused_b():
        for b, e, u, region in cuts:
            ops.apply_delta_q(th[b:e], u, region, gf, broadcast=[w[b:e] for w in ws])

    def replica_a():
        for b, e, _, _ in cuts:
            copies(b, e)

    def replica_b():
        for b, e, _, _ in cuts:
            ops.broadcast_theta(th[b:e], [w[b:e] for w in ws])

    def phase3():
        for b, e, u, region in cuts:
            ops.apply_delta_q(th[b:e], u, region, gf)

    rows = {k: [] for k in ("phase3_alone", "fused_a", "fused_b", "replica_a", "replica_b")}
    fns = {"phase3_alone": phase3, "fused_a": fused_a, "fused_b": fused_b, "replica_a": replica_a,
           "replica_b": replica_b}
    for _ in range(a.rounds):
        for k, fn in fns.items():
            rows[k].append(timed(fn, a.steps, a.warmup))
    bg, bw, K = 4, ws[0].element_size(), k_local
    out = {"world": world, "workers": "bf16" if wdt == torch.bfloat16 else "f32", "theta": "f32", "k_local": K,
           "buckets": len(cuts), "n_pad": s.n_pad, **{k: summary(v) for k, v in rows.items()}}
    for kind, num, den in (("fused", 2 * bg + Q8 + K * bw, 2 * bg + Q8 + K * (bg + bw)),
                           ("replica", bg + K * bw, K * (bg + bw))):
        ra, rb = out[kind + "_a"], out[kind + "_b"]
        out[kind + "_ratio_measured"] = round(rb["ms"] / ra["ms"], 4)
        out[kind + "_ratio_bytes"] = round(num / den, 4)
        out[kind + "_bytes_per_elem"] = {"a": den, "b": num}
        # (b) is no slower than (a) outside the runs' own range
        out[kind + "_b_not_slower"] = rb["min_ms"] <= ra["max_ms"]
    del s, th, ws, cuts
    gc.collect()
    torch.cuda.empty_cache()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--layout", default="gpt_1p3b")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sharded_bcast_probe.json"))
    a = ap.parse_args()
    from evolutionarydistributedtraining_amd import _lib as L
    from evolutionarydistributedtraining_amd.layouts import LAYOUTS
    dev = torch.device("cuda:0")
    layout = LAYOUTS[a.layout]()
    groups = []
    for world in (1, 8):
        for wdt in (torch.bfloat16, torch.float32):
            groups.append(group(layout, wdt, world, a, dev))
            print(json.dumps(groups[-1]), flush=True)
    res = {"probe": "sharded_bcast_probe", "layout": a.layout, "elements": layout.total, "steps": a.steps,
           "warmup": a.warmup, "rounds": a.rounds, "gather_format": "mxfp8", "device": torch.cuda.get_device_name(0),
           "library_sha256": L.library_sha256(),
           "note": "one GPU, loopback communicator, local kernels only: one pass over the step's buckets between two "
                   "HIP events, median of `steps` passes, then the median and range of `rounds` alternating rounds; "
                   "(a) is phase 3 + K_local copy_ (fused) or K_local copy_ (replica), (b) the new entry; ratios are "
                   "b / a; nothing is measured of the links and no multi-GPU node has run the schedule",
           "groups": groups}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
