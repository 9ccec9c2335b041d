"""Times the guarded step's two kernels against the kernels they should match, on one device:
edt_delta_stats against edt_delta_partial (the same K b_w + b_g bytes read per element; the partial
writes 4 B per element more) and edt_outer_step_scaled against edt_outer_step (the same bytes).
HIP events, the pairs alternated in one process on the same operands, so drift hits both alike.

    python scripts/delta_stats_probe.py --out profiles/delta_stats_probe.json [--n 1300000000] [--workers 8]
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


def summary(ms, nbytes):
    med = statistics.median(ms)
    return {"median_ms": round(med, 4), "min_ms": round(min(ms), 4), "max_ms": round(max(ms), 4),
            "bytes": nbytes, "fraction_of_8TBs": round(nbytes / (med * 1e-3) / HBM_PEAK, 4)}


def main():
    from evolutionarydistributedtraining_amd import _lib, ops
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1_300_000_000)
    ap.add_argument("--workers", type=int, default=8)
    ap.add_argument("--rounds", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    n, K = a.n, a.workers
    report = {"device": torch.cuda.get_device_name(dev), "n": n, "workers": K, "rounds": a.rounds,
              "library_sha256": _lib.library_sha256(), "regimes": {}}
    plan = ops.make_slerp_plan([0, n], dev)
    for name, gdt, wdt in (("f32_f32", torch.float32, torch.float32), ("f32_bf16", torch.float32, torch.bfloat16)):
        theta = torch.randn(n, device=dev, dtype=gdt) * 0.5
        ws = []
        for _ in range(K):
            w = torch.randn(n, device=dev, dtype=torch.float32)
            w.mul_(0.02).add_(theta)
            ws.append(w.to(wdt))
            del w
        mom = torch.zeros(n, device=dev, dtype=gdt)
        acc = torch.empty(n, device=dev, dtype=torch.float32)
        bg, bw = theta.element_size(), ws[0].element_size()
        read = n * (K * bw + bg)
        step_bytes = n * (K * bw + 4 * bg)
        runs = {
            "delta_stats": lambda: ops.delta_stats(theta, ws, plan),
            "delta_partial": lambda: ops.delta_partial(theta, ws, K, acc),
            # lr = 0: theta stays where it is, every round streams the same operands
            "outer_step_scaled": lambda: ops.outer_step_scaled(theta, ws, mom, True, 0.0, 0.9, True, 0.37),
            "outer_step": lambda: ops.outer_step(theta, ws, mom, True, 0.0, 0.9, True),
        }
        ms = {k: [] for k in runs}
        for r in range(a.warmup + a.rounds):
            for k, fn in runs.items():
                t = timed(fn, dev)
                if r >= a.warmup:
                    ms[k].append(t)
        report["regimes"][name] = {
            "delta_stats": summary(ms["delta_stats"], read),
            "delta_partial": summary(ms["delta_partial"], read + 4 * n),
            "outer_step_scaled": summary(ms["outer_step_scaled"], step_bytes),
            "outer_step": summary(ms["outer_step"], step_bytes),
        }
        del theta, ws, mom, acc
        ops.release_scratch()
        torch.cuda.empty_cache()
    line = json.dumps(report)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(json.dumps(report, indent=1) + "\n")


if __name__ == "__main__":
    main()
