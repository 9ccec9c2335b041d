"""Times the fragment step with its fused worker merge (edt_outer_step_list_mix) against the
composition it replaces, on one device: edt_outer_step_list on the fragment's runs, then per run
edt_broadcast_theta into a scratch buffer and K x edt_lerp into the workers. HIP events, the two
alternated in one process on the same operands (so drift hits both alike), with the plain list step
on the same runs beside them as the ceiling's yardstick.

One fragment of a model layout cut into P strided fragments, fp32 master with fp32 and with bf16
workers, the merge destinations aliasing the delta workers (the live arenas) and distinct from them
(snapshots as the delta workers).

    python scripts/fragment_mix_probe.py --out profiles/fragment_mix_probe.json [--layout gpt_1p3b] [--fragments 4]
"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

HBM_PEAK = 8.0e12          # bytes / s, MI355X


def timed(fn, dev):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    torch.cuda.synchronize(dev)
    return a.elapsed_time(b)


def summary(rounds, nbytes):
    """rounds: per round, the times of that round's repeats. Median over everything, and the
    min - max of the per-round medians."""
    per_round = [statistics.median(r) for r in rounds]
    med = statistics.median([t for r in rounds for t in r])
    return {"median_ms": round(med, 4), "round_medians_ms": [round(x, 4) for x in per_round],
            "min_ms": round(min(per_round), 4), "max_ms": round(max(per_round), 4), "bytes": nbytes,
            "fraction_of_8TBs": round(nbytes / (med * 1e-3) / HBM_PEAK, 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--layout", default="gpt_1p3b")
    ap.add_argument("--fragments", type=int, default=4)
    ap.add_argument("--fragment", type=int, default=1)
    ap.add_argument("--workers", type=int, default=8)
    ap.add_argument("--mix", type=float, default=0.5)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    from evolutionarydistributedtraining_amd import FragmentPlan, _lib, ops
    from evolutionarydistributedtraining_amd.layouts import LAYOUTS
    dev = torch.device("cuda", 0)
    lay = LAYOUTS[a.layout]()
    plan = FragmentPlan.strided(lay, a.fragments)
    p, K, mix = a.fragment, a.workers, a.mix
    n = plan.numel(p)
    report = {"device": torch.cuda.get_device_name(dev), "layout": a.layout, "fragments": a.fragments, "fragment": p,
              "runs": len(plan.runs(p)), "n": n, "workers": K, "mix": mix, "rounds": a.rounds, "repeats": a.repeats,
              "library_sha256": _lib.library_sha256(), "cells": {}}
    for name, gdt, wdt in (("f32_f32", torch.float32, torch.float32), ("f32_bf16", torch.float32, torch.bfloat16)):
        theta = torch.randn(lay.total, device=dev, dtype=gdt) * 0.5
        mom = torch.zeros(lay.total, device=dev, dtype=gdt)
        arenas = []
        for _ in range(K):
            w = torch.randn(lay.total, device=dev, dtype=torch.float32)
            w.mul_(0.02).add_(theta)
            arenas.append(w.to(wdt))
            del w
        snaps = [torch.cat(plan.views(p, w)) for w in arenas]
        scratch = torch.empty(n, device=dev, dtype=wdt)
        th, mo = plan.views(p, theta), plan.views(p, mom)
        live = [plan.views(p, w) for w in arenas]
        snap_v = [plan.snapshot_views(p, s) for s in snaps]
        sc = plan.snapshot_views(p, scratch)
        bg, bw = theta.element_size(), arenas[0].element_size()
        step = (True, 0.0, 0.9, True)          # lr = 0: theta stays where it is, every round streams the same operands

        def composition(deltas):
            ops.outer_step_list(th, deltas, mo, *step)
            for r, t in enumerate(th):
                ops.broadcast_theta(t, [sc[r]])
                for l in live:
                    ops.lerp(mix, l[r], sc[r], out=l[r])

        for cell, deltas in (("aliased", live), ("distinct", snap_v)):
            fused_bytes = n * (K * bw + (K * bw if cell == "distinct" else 0) + K * bw + 4 * bg)
            comp_bytes = n * ((K * bw + 4 * bg) + (bg + bw) + K * 3 * bw)
            runs = {"fused": lambda d=deltas: ops.outer_step_list_mix(th, d, mo, *step, live, mix),
                    "composition": lambda d=deltas: composition(d),
                    "outer_step_list": lambda d=deltas: ops.outer_step_list(th, d, mo, *step)}
            nbytes = {"fused": fused_bytes, "composition": comp_bytes, "outer_step_list": n * (K * bw + 4 * bg)}
            ms = {k: [] for k in runs}
            for _ in range(a.warmup):
                for fn in runs.values():
                    fn()
            for _ in range(a.rounds):
                cur = {k: [] for k in runs}
                for _ in range(a.repeats):
                    for k, fn in runs.items():
                        cur[k].append(timed(fn, dev))
                for k in runs:
                    ms[k].append(cur[k])
            out = {k: summary(ms[k], nbytes[k]) for k in runs}
            out["fused_over_composition"] = round(out["fused"]["median_ms"] / out["composition"]["median_ms"], 4)
            out["bytes_predict"] = round(fused_bytes / comp_bytes, 4)
            report["cells"][f"{name}/{cell}"] = out
        del theta, mom, arenas, snaps, scratch, th, mo, live, snap_v, sc
        torch.cuda.empty_cache()
    print(json.dumps(report))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(json.dumps(report, indent=1) + "\n")


if __name__ == "__main__":
    main()
