"""Times the task-vector merge kernel (edt_task_merge_list) against its byte floor, (K * b_w + b_g + b_out)
bytes per element, with the tensor-list outer step (edt_outer_step_list, no momentum: K * b_w + 2 * b_g,
the same operand count) beside it on the same tensors. One device, HIP events, the cells alternated in one
process on the same operands; median over rounds x repeats and the min - max of the round medians.

Cells: task_arithmetic (no random bits), dare_linear and dare_ties at density 0.5 (one Philox call per
lane and model), each written to a separate child; outer_step_list with lr = 0.

    python scripts/task_merge_probe.py --out profiles/task_merge_probe.json [--layout gpt_1p3b] [--models 8]
"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

HBM_PEAK = 8.0e12          # bytes / s, MI355X


def timed(fn, dev, cover):
    """fn's device time: the start event is queued behind a few large copies, so the host side of fn (the
    per-tensor checks and the table of some hundred tensors, a millisecond or two) runs while the device
    is busy and the events bracket the table upload and the kernel only."""
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    for _ in range(4):
        cover[0].copy_(cover[1])
    a.record()
    fn()
    b.record()
    torch.cuda.synchronize(dev)
    return a.elapsed_time(b)


def summary(rounds, nbytes):
    per_round = [statistics.median(r) for r in rounds]
    med = statistics.median([t for r in rounds for t in r])
    return {"median_ms": round(med, 4), "min_ms": round(min(per_round), 4), "max_ms": round(max(per_round), 4),
            "bytes": nbytes, "floor_ms_at_8TBs": round(nbytes / HBM_PEAK * 1e3, 4),
            "fraction_of_8TBs": round(nbytes / (med * 1e-3) / HBM_PEAK, 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--layout", default="gpt_1p3b")
    ap.add_argument("--models", type=int, default=8)
    ap.add_argument("--dtype", default="bf16", choices=["bf16", "f32"])
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    from evolutionarydistributedtraining_amd import _lib, ops
    from evolutionarydistributedtraining_amd.layouts import LAYOUTS
    dev = torch.device("cuda", 0)
    lay = LAYOUTS[a.layout]()
    K, n = a.models, lay.total
    dt = torch.bfloat16 if a.dtype == "bf16" else torch.float32
    base = (torch.randn(n, device=dev, dtype=torch.float32) * 0.02).to(dt)
    arenas = []
    for _ in range(K):
        w = torch.randn(n, device=dev, dtype=torch.float32)
        w.mul_(1e-3).add_(base)
        arenas.append(w.to(dt))
        del w
    child = torch.empty(n, device=dev, dtype=dt)
    cover = (torch.empty(n, device=dev, dtype=dt), base)
    bs, ms, cs = lay.views(base), [lay.views(w) for w in arenas], lay.views(child)
    b = base.element_size()
    merge_bytes, step_bytes = n * (K * b + 2 * b), n * (K * b + 2 * b)
    weights = [1.0 / K] * K
    runs = {
        "task_arithmetic": lambda: ops.task_merge_list(bs, ms, cs, weights=weights),
        "dare_linear": lambda: ops.task_merge_list(bs, ms, cs, weights=weights, densities=0.5, seed=1),
        "dare_ties": lambda: ops.task_merge_list(bs, ms, cs, weights=weights, densities=0.5, consensus=True, seed=1),
        "ties_no_drop": lambda: ops.task_merge_list(bs, ms, cs, weights=weights, consensus=True),
        "outer_step_list": lambda: ops.outer_step_list(bs, ms, None, False, 0.0, 0.0, False),
    }
    nbytes = {k: step_bytes if k == "outer_step_list" else merge_bytes for k in runs}
    times = {k: [] for k in runs}
    for _ in range(a.warmup):
        for fn in runs.values():
            fn()
    for _ in range(a.rounds):
        cur = {k: [] for k in runs}
        for _ in range(a.repeats):
            for k, fn in runs.items():
                cur[k].append(timed(fn, dev, cover))
        for k in runs:
            times[k].append(cur[k])
    report = {"device": torch.cuda.get_device_name(dev), "layout": a.layout, "n": n, "tensors": len(lay), "models": K,
              "dtype": a.dtype, "rounds": a.rounds, "repeats": a.repeats, "library_sha256": _lib.library_sha256(),
              "command": "python scripts/task_merge_probe.py " + " ".join(sys.argv[1:]),
              "cells": {k: summary(times[k], nbytes[k]) for k in runs}}
    ref = report["cells"]["outer_step_list"]["median_ms"]
    for k in runs:
        report["cells"][k]["over_outer_step_list"] = round(report["cells"][k]["median_ms"] / ref, 4)
    print(json.dumps(report))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(json.dumps(report, indent=1) + "\n")


if __name__ == "__main__":
    main()
