"""Times the guarded step's two kernels against the kernels they should match, on one device:
edt_delta_stats against edt_delta_partial (the same K b_w + b_g bytes read per element; the partial
writes 4 B per element more) and edt_outer_step_scaled against edt_outer_step (the same bytes).
HIP events, the pairs alternated in one process on the same operands, so drift hits both alike.

    python scripts/delta_stats_probe.py --out profiles/delta_stats_probe.json [--n 1300000000] [--workers 8]

--list: the tensor-list form on a model layout (separate tensors, as list(model.parameters())):
(a) edt_delta_stats on packed copies, (b) edt_delta_stats_list on the separate tensors, alternated,
and (c) the guarded drop-in diloco.outer_step end to end with its peak allocation above the
operands. --tree PATH runs (c) alone on the package of another checkout (the parent commit, built
there), so both sides of the comparison come from the same script.

    python scripts/delta_stats_probe.py --list --out profiles/delta_stats_list_probe.json [--layout gpt_1p3b]
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


def separate_tensors(numels, K, gdt, wdt, dev):
    """theta and K workers as separately allocated tensors (not views of one arena)."""
    thetas = [torch.randn(n, device=dev, dtype=gdt) * 0.5 for n in numels]
    workers = [[(torch.randn(n, device=dev, dtype=torch.float32) * 0.02 + t.float()).to(wdt) for n, t in zip(numels, thetas)]
               for _ in range(K)]
    return thetas, workers


def list_mode(a):
    if a.tree:
        sys.path.insert(0, os.path.abspath(a.tree))
    from evolutionarydistributedtraining_amd import _lib, diloco, ops
    from evolutionarydistributedtraining_amd.layouts import LAYOUTS
    import time
    dev = torch.device("cuda", 0)
    numels = list(LAYOUTS[a.layout]().numels)
    n, K, T = sum(numels), a.workers, len(numels)
    report = {"device": torch.cuda.get_device_name(dev), "layout": a.layout, "tensors": T, "n": n, "workers": K,
              "rounds": a.rounds, "library_sha256": _lib.library_sha256(),
              "tree": a.tree or ".", "regimes": {}}
    for name, gdt, wdt in (("f32_f32", torch.float32, torch.float32), ("f32_bf16", torch.float32, torch.bfloat16)):
        thetas, workers = separate_tensors(numels, K, gdt, wdt, dev)
        bg, bw = thetas[0].element_size(), workers[0][0].element_size()
        read = n * (K * bw + bg)
        out = {}
        if not a.tree:                                        # (a) and (b), alternated
            offs = [0]
            for m in numels:
                offs.append(offs[-1] + m)
            theta, ws = diloco.pack(thetas), [diloco.pack(w) for w in workers]
            aplan, lplan = ops.make_slerp_plan(offs, dev), ops.make_slerp_plan(offs, dev, relative=True)
            runs = {"delta_stats_arena_packed": lambda: ops.delta_stats(theta, ws, aplan),
                    "delta_stats_list": lambda: ops.delta_stats_list(thetas, workers, lplan)}
            ms = {k: [] for k in runs}
            for r in range(a.warmup + a.rounds):
                for k, fn in runs.items():
                    t = timed(fn, dev)
                    if r >= a.warmup:
                        ms[k].append(t)
            out = {k: summary(v, read) for k, v in ms.items()}
            out["list_over_arena"] = round(out["delta_stats_list"]["median_ms"] /
                                           out["delta_stats_arena_packed"]["median_ms"], 4)
            del theta, ws
            ops.release_scratch()
            torch.cuda.empty_cache()
        # (c) the guarded drop-in step end to end (lr = 0: theta stays where it is)
        guard = diloco.OuterGuard(max_grad_norm=1e-3)        # far below the norm: the clipped step runs
        state, wall = None, []
        torch.cuda.synchronize(dev)
        operands = torch.cuda.memory_allocated(dev)
        for r in range(a.warmup + a.rounds):
            if r == a.warmup:
                torch.cuda.synchronize(dev)
                torch.cuda.reset_peak_memory_stats(dev)
            t0 = time.perf_counter()
            state = diloco.outer_step(thetas, workers, state, lr=0.0, guard=guard)
            torch.cuda.synchronize(dev)
            if r >= a.warmup:
                wall.append((time.perf_counter() - t0) * 1e3)
        peak = torch.cuda.max_memory_allocated(dev)
        out["guarded_outer_step"] = {"median_ms": round(statistics.median(wall), 3), "min_ms": round(min(wall), 3),
                                     "max_ms": round(max(wall), 3), "clip_coef": state.last_stats["clip_coef"],
                                     "operand_bytes": operands, "peak_bytes": peak,
                                     "peak_over_operands": round(peak / operands, 4)}
        report["regimes"][name] = out
        del thetas, workers, state
        ops.release_scratch()
        torch.cuda.empty_cache()
    return report


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--list", action="store_true", help="the tensor-list form on --layout")
    ap.add_argument("--layout", default="gpt_1p3b")
    ap.add_argument("--tree", default=None, help="with --list: run the end-to-end step of the package in this checkout")
    ap.add_argument("--n", type=int, default=1_300_000_000)
    ap.add_argument("--workers", type=int, default=8)
    ap.add_argument("--rounds", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.list:
        return emit(list_mode(a), a.out)
    from evolutionarydistributedtraining_amd import _lib, ops
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
    emit(report, a.out)


def emit(report, out):
    print(json.dumps(report))
    if out:
        os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
        with open(out, "w") as f:
            f.write(json.dumps(report, indent=1) + "\n")


if __name__ == "__main__":
    main()
