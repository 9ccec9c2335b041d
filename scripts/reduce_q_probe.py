"""Probe: the local kernels of one sharded outer step with fp32 partials (reduce_ordered, the
baseline) against block-quantized partials (reduce_q: mxfp8 / mxfp4, error feedback on / off), on
one GPU, 1.3B layout, K = 8, fp32 theta, bf16 and fp32 workers, at world 1 and as rank 0 of 8.

One process, one rank: the communicator is a loopback (every peer's partial of the owned shard is
a copy of this rank's own), so the kernels see the shapes, buffers and bytes of the N-rank step
and nothing is measured of the links — the wire bytes of reduce_q are computed, not measured.
Every kernel is bracketed by HIP events through ShardedOuterSync's kernel_events seam; a step's
phase 1 is the sum of its edt_delta_partial(_q) launches, phase 2 of its edt_sgd_apply_sum(_q)
launches; medians over --steps steps after --warmup. The baseline runs three times per group
(first, middle, last), and its spread is recorded beside the numbers it judges.

    python scripts/reduce_q_probe.py --out profiles/reduce_q_probe.json

--gather-format mxfp8|mxfp4 probes the quantized gather instead (reduce_q with gather_format): per
group and error-feedback setting, plain reduce_q and the gather form alternate in this process on
the same operands (plain, gather, plain, gather, plain), each kernel timed — phase 1
(edt_delta_partial_q), phase 2 / 2' (edt_sgd_apply_sum_q / edt_sgd_delta_sum_q) and phase 3
(edt_apply_delta_q) — and the result goes to profiles/gather_q_probe.json. The loopback's uint8
all-gather fills every slot with this rank's own region, so phase 3 reads real blocks.

    python scripts/reduce_q_probe.py --gather-format mxfp8

--rounding stochastic probes stochastic rounding instead (reduce_q with rounding="stochastic"): per
group — world 1 / 8 x bf16 / fp32 workers x mxfp8 / mxfp4 partials, with --gather-format also the
quantized gather in that format — error feedback off (the floor), error feedback on (what
stochastic rounding replaces) and stochastic rounding alternate in this process on the same operands
(off, on, sr, off, on, sr), each kernel timed by HIP events; the ratios sr / off and sr / on are
formed within the run. The result is merged into profiles/sr_probe.json under the gather format.

    python scripts/reduce_q_probe.py --rounding stochastic [--gather-format mxfp8]
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

PEAK_BYTES_PER_MS = 8e9         # 8 TB/s


def loopback(world: int):
    from evolutionarydistributedtraining_amd.collectives import Collectives, _Done

    class Loopback(Collectives):
        """Rank 0 of `world` with no peers: an all-to-all delivers this rank's own region for its
        shard from every source, an all-gather leaves the owned shard in place."""
        inplace = True

        def __init__(self):
            self.world, self.rank = world, 0

        def all_to_all(self, out, inp, async_op=False):
            out.view(world, -1).copy_(inp.view(world, -1)[0].expand(world, -1))
            return _Done()

        def all_gather(self, out, inp, async_op=False):
            if out.dtype == torch.uint8 and world > 1:       # the quantized gather: every owner's region
                out.view(world, -1)[1:].copy_(inp.expand(world - 1, -1))
            return _Done()

    return Loopback()


def measure(layout, wdt, world, mode, fmt, ef, steps, warmup, dev, seed=0, gather=None, rounding="nearest"):
    from evolutionarydistributedtraining_amd.distributed import ShardedOuterSync
    k_local = 8 // world
    s = ShardedOuterSync(layout, torch.float32, wdt, k_local, dev, mode=mode, broadcast="theta", comm=loopback(world),
                         **({"wire_format": fmt, "error_feedback": ef} if mode == "reduce_q" else {}),
                         **({"gather_format": gather} if gather else {}),
                         **({"rounding": rounding, "seed": 0x5eed} if rounding != "nearest" else {}))
    g = torch.Generator(device=dev).manual_seed(seed)
    s.theta_buf.normal_(0, 0.02, generator=g)
    for w in s.worker_bufs:
        w.copy_(s.theta_buf)
        w.add_(torch.randn(s.n_pad, device=dev, generator=g).mul_(1e-3))
    nb = len(s.buckets)
    if gather:
        return measure_gather(s, nb, fmt, ef, gather, steps, warmup)
    p1, p2 = [], []
    for i in range(warmup + steps):
        s.kernel_events = []
        s.step()
        torch.cuda.synchronize()
        ms = [a.elapsed_time(b) for a, b in s.kernel_events]
        assert len(ms) == 2 * nb
        if i >= warmup:
            p1.append(sum(ms[:nb]))
            p2.append(sum(ms[nb:]))
    tot = [a + b for a, b in zip(p1, p2)]
    kb = s.kernel_bytes()
    out = {"mode": mode, "wire_format": fmt, "error_feedback": ef, "buckets": nb, "n_pad": s.n_pad,
           "phase1_ms": round(statistics.median(p1), 4), "phase2_ms": round(statistics.median(p2), 4),
           "ms": round(statistics.median(tot), 4), "kernel_bytes": kb,
           "fraction_of_8TBps": round(kb / statistics.median(tot) / PEAK_BYTES_PER_MS, 4),
           "wire_bytes_computed": s.wire_bytes()}
    del s
    gc.collect()
    torch.cuda.empty_cache()
    return out


def measure_gather(s, nb, fmt, ef, gather, steps, warmup):
    """The gather form's three phases per kernel, with each phase's algorithmic bytes."""
    p1, p2, p3 = [], [], []
    for i in range(warmup + steps):
        s.kernel_events = []
        s.step()
        torch.cuda.synchronize()
        ms = [a.elapsed_time(b) for a, b in s.kernel_events]
        assert len(ms) == 3 * nb
        if i >= warmup:
            p1.append(sum(ms[:nb]))
            p2.append(sum(ms[nb:2 * nb]))
            p3.append(sum(ms[2 * nb:]))
    tot = [a + b + c for a, b, c in zip(p1, p2, p3)]
    shard = s.n_pad // s.world
    e8 = 8 if ef else 0
    b2 = shard * (4 + 8 + e8) + s.world * s._q_bytes(shard) + s._q_bytes(shard, gather)
    b3 = s.n_pad * 8 + s._q_bytes(s.n_pad, gather)
    kb = s.kernel_bytes()
    m2, m3 = statistics.median(p2), statistics.median(p3)
    out = {"mode": "reduce_q", "wire_format": fmt, "gather_format": gather, "error_feedback": ef, "buckets": nb,
           "n_pad": s.n_pad, "phase1_ms": round(statistics.median(p1), 4), "phase2_ms": round(m2, 4),
           "phase3_ms": round(m3, 4), "ms": round(statistics.median(tot), 4), "kernel_bytes": kb,
           "phase2_bytes": b2, "phase3_bytes": b3,
           "phase2_fraction_of_8TBps": round(b2 / m2 / PEAK_BYTES_PER_MS, 4),
           "phase3_fraction_of_8TBps": round(b3 / m3 / PEAK_BYTES_PER_MS, 4),
           "fraction_of_8TBps": round(kb / statistics.median(tot) / PEAK_BYTES_PER_MS, 4),
           "wire_bytes_computed": s.wire_bytes()}
    del s
    gc.collect()
    torch.cuda.empty_cache()
    return out


def gather_main(a, layout, dev):
    from evolutionarydistributedtraining_amd import _lib as L
    gf, fmt = a.gather_format, "mxfp8"
    groups = []
    for world in (1, 8):
        for name, wdt in (("bf16", torch.bfloat16), ("f32", torch.float32)):
            for ef in (False, True):
                run = lambda g=None: measure(layout, wdt, world, "reduce_q", fmt, ef, a.steps, a.warmup, dev, gather=g)
                runs = [run(), run(gf), run(), run(gf), run()]
                plain, gath = runs[0::2], runs[1::2]
                med = lambda rows, key: round(statistics.median(r[key] for r in rows), 4)
                shard = plain[0]["n_pad"] // world
                b2_plain = shard * (8 + 8) + world * (shard + shard // 32)
                p2 = med(plain, "phase2_ms")
                # what phase 2' + phase 3 would cost if their bytes moved at the rate the same run's
                # plain phase 2 achieves, against what they took
                at_rate = (gath[0]["phase2_bytes"] + gath[0]["phase3_bytes"]) / (b2_plain / p2)
                took = med(gath, "phase2_ms") + med(gath, "phase3_ms")
                grp = {"world": world, "workers": name, "theta": "f32", "k_local": 8 // world, "error_feedback": ef,
                       "reduce_q": dict(plain[1], phase1_ms=med(plain, "phase1_ms"), phase2_ms=p2, ms=med(plain, "ms"),
                                        repeats_phase2_ms=[r["phase2_ms"] for r in plain],
                                        repeats_ms=[r["ms"] for r in plain], phase2_bytes=b2_plain,
                                        phase2_fraction_of_8TBps=round(b2_plain / p2 / PEAK_BYTES_PER_MS, 4),
                                        spread_ms=round(max(r["ms"] for r in plain) - min(r["ms"] for r in plain), 4)),
                       "gather_q": dict(gath[0], phase1_ms=med(gath, "phase1_ms"), phase2_ms=med(gath, "phase2_ms"),
                                        phase3_ms=med(gath, "phase3_ms"), ms=med(gath, "ms"),
                                        repeats_ms=[r["ms"] for r in gath]),
                       "phase2p_plus_phase3_ms": round(took, 4),
                       "same_bytes_at_plain_phase2_rate_ms": round(at_rate, 4),
                       "ratio_to_plain_phase2_rate": round(took / at_rate, 4),
                       "extra_local_ms_over_reduce_q": round(med(gath, "ms") - med(plain, "ms"), 4)}
                groups.append(grp)
                print(json.dumps(grp), flush=True)
    res = {"probe": "gather_q_probe", "layout": a.layout, "elements": layout.total, "K": 8, "steps": a.steps,
           "warmup": a.warmup, "wire_format": fmt, "gather_format": gf, "device": torch.cuda.get_device_name(0),
           "library_sha256": L.library_sha256(),
           "note": "local kernels only, one GPU, loopback communicator; wire_bytes_computed follow from the byte "
                   "counts and were not measured on a multi-GPU node", "groups": groups}
    out = a.out or os.path.join(ROOT, "profiles", "gather_q_probe.json")
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


def sr_main(a, layout, dev):
    """Stochastic rounding against error feedback off and on, per group, interleaved in one process."""
    from evolutionarydistributedtraining_amd import _lib as L
    gf = a.gather_format
    phases = ("phase1_ms", "phase2_ms") + (("phase3_ms",) if gf else ()) + ("ms",)
    groups = []
    for world in (1, 8):
        for name, wdt in (("bf16", torch.bfloat16), ("f32", torch.float32)):
            for fmt in ("mxfp8", "mxfp4"):
                run = lambda ef, rnd="nearest": measure(layout, wdt, world, "reduce_q", fmt, ef, a.steps, a.warmup, dev,
                                                        gather=gf, rounding=rnd)
                rows = {"ef_off": [], "ef_on": [], "sr": []}
                for _ in range(a.rounds):
                    rows["ef_off"].append(run(False))
                    rows["ef_on"].append(run(True))
                    rows["sr"].append(run(False, "stochastic"))
                grp = {"world": world, "workers": name, "theta": "f32", "k_local": 8 // world, "wire_format": fmt,
                       "gather_format": gf}
                for key, rs in rows.items():
                    grp[key] = {ph: round(statistics.median(r[ph] for r in rs), 4) for ph in phases}
                    grp[key]["repeats_ms"] = [r["ms"] for r in rs]
                    grp[key]["repeats_phase1_ms"] = [r["phase1_ms"] for r in rs]
                    grp[key]["kernel_bytes"] = rs[0]["kernel_bytes"]
                for ph in phases:
                    tag = "total" if ph == "ms" else ph[:-3]
                    grp[f"sr_over_ef_off_{tag}"] = round(grp["sr"][ph] / grp["ef_off"][ph], 4)
                    grp[f"sr_over_ef_on_{tag}"] = round(grp["sr"][ph] / grp["ef_on"][ph], 4)
                grp["sr_not_slower_than_ef_on"] = grp["sr"]["ms"] <= grp["ef_on"]["ms"]
                groups.append(grp)
                print(json.dumps(grp), flush=True)
    out = a.out or os.path.join(ROOT, "profiles", "sr_probe.json")
    try:
        with open(out) as f:
            res = json.load(f)
        assert res.get("probe") == "sr_probe"
    except (OSError, ValueError, AssertionError):
        res = {"probe": "sr_probe", "runs": {}}
    res.update({"layout": a.layout, "elements": layout.total, "K": 8, "device": torch.cuda.get_device_name(0),
                "note": "local kernels only, one GPU, loopback communicator, HIP-event times per kernel: medians over "
                        "`steps` steps, then over `rounds` alternating runs; ef_off is the floor, ef_on what stochastic "
                        "rounding replaces; nothing is measured of the links"})
    res["runs"]["gather_" + (gf or "none")] = {"steps": a.steps, "warmup": a.warmup, "rounds": a.rounds,
                                               "library_sha256": L.library_sha256(), "groups": groups}
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--layout", default="gpt_1p3b")
    ap.add_argument("--out", default=None, help="default: profiles/reduce_q_probe.json (gather_q_probe.json "
                                                "with --gather-format)")
    ap.add_argument("--gather-format", choices=("mxfp8", "mxfp4"), default=None,
                    help="probe the quantized gather next to plain reduce_q instead")
    ap.add_argument("--rounding", choices=("nearest", "stochastic"), default="nearest",
                    help="stochastic: probe stochastic rounding against error feedback off / on (profiles/sr_probe.json)")
    ap.add_argument("--rounds", type=int, default=3, help="--rounding stochastic: alternating runs per setting")
    a = ap.parse_args()
    from evolutionarydistributedtraining_amd import _lib as L
    from evolutionarydistributedtraining_amd.layouts import LAYOUTS
    dev = torch.device("cuda:0")
    layout = LAYOUTS[a.layout]()
    if a.rounding == "stochastic":
        return sr_main(a, layout, dev)
    if a.gather_format:
        return gather_main(a, layout, dev)
    a.out = a.out or os.path.join(ROOT, "profiles", "reduce_q_probe.json")
    groups = []
    for world in (1, 8):
        for name, wdt in (("bf16", torch.bfloat16), ("f32", torch.float32)):
            run = lambda mode, fmt=None, ef=None: measure(layout, wdt, world, mode, fmt, ef, a.steps, a.warmup, dev)
            base = [run("reduce_ordered")]
            rows = [run("reduce_q", "mxfp8", False), run("reduce_q", "mxfp8", True)]
            base.append(run("reduce_ordered"))
            rows += [run("reduce_q", "mxfp4", False), run("reduce_q", "mxfp4", True)]
            base.append(run("reduce_ordered"))
            b1 = [b["phase1_ms"] for b in base]
            bt = [b["ms"] for b in base]
            grp = {"world": world, "workers": name, "theta": "f32", "k_local": 8 // world,
                   "baseline": dict(base[1], repeats_phase1_ms=b1, repeats_ms=bt,
                                    phase1_ms=round(statistics.median(b1), 4), ms=round(statistics.median(bt), 4),
                                    spread_phase1_ms=round(max(b1) - min(b1), 4), spread_ms=round(max(bt) - min(bt), 4)),
                   "reduce_q": rows}
            # the merge condition: phase 1 without error feedback is not slower than edt_delta_partial
            # on the same operands by more than the baseline's own spread
            grp["phase1_not_slower"] = {r["wire_format"]: r["phase1_ms"] <= grp["baseline"]["phase1_ms"]
                                        + grp["baseline"]["spread_phase1_ms"]
                                        for r in rows if not r["error_feedback"]}
            groups.append(grp)
            print(json.dumps(grp), flush=True)
    res = {"probe": "reduce_q_probe", "layout": a.layout, "elements": layout.total, "K": 8, "steps": a.steps,
           "warmup": a.warmup, "device": torch.cuda.get_device_name(0), "library_sha256": L.library_sha256(),
           "note": "local kernels only, one GPU, loopback communicator; wire_bytes_computed follow from the byte "
                   "counts and were not measured on a multi-GPU node", "groups": groups}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
