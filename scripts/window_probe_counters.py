"""Memory-side counters of scripts/native/window_probe.hip at two residency caps, one rocprofv3
--pmc pass per small counter group and nothing else traced. The groups hold the L2's memory-side
read/write request, busy and stall counters; `rocprofv3 --list-avail` decides which of them exist
on the device. The probe launches its caps round-robin, so the dispatches of window_step_kernel
alternate between the caps in the order given (the trace's LDS_Block_Size column shows the static
size only, 0 for every cap, so the order is what tells them apart); per counter and cap the median
over the launches after the warm-up pair is recorded.

    python scripts/window_probe_counters.py PROBE_BINARY OUT.json [--caps 0,1] [--workdir DIR]
"""
import argparse
import csv
import glob
import json
import os
import statistics
import subprocess
import sys

GROUPS = [
    ["TCC_EA0_RDREQ_sum", "TCC_EA0_RDREQ_DRAM_CREDIT_STALL_sum", "GRBM_GUI_ACTIVE"],
    ["TCC_EA0_WRREQ_sum", "TCC_EA0_WRREQ_STALL_sum", "TCC_EA0_WRREQ_DRAM_CREDIT_STALL_sum"],
    ["TCC_BUSY_sum", "TCC_TAG_STALL_sum"],
    ["TCC_EA0_RDREQ_LEVEL_sum", "TCC_EA0_WRREQ_LEVEL_sum"],
    ["TCP_PENDING_STALL_CYCLES_sum", "TCP_TCC_READ_REQ_LATENCY_sum", "TCP_TCC_READ_REQ_sum"],
]
# a fault, an abort or a time limit: nothing more is started on the device
FATAL = {124, 137, 134, 139, -6, -9, -11}
LAUNCHES = 3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("probe")
    ap.add_argument("out")
    ap.add_argument("--caps", default="0,1")
    ap.add_argument("--workdir", default="bench_out/window_pmc")
    a = ap.parse_args()
    caps = [int(c) for c in a.caps.split(",")]
    os.makedirs(a.workdir, exist_ok=True)
    avail = subprocess.run(["rocprofv3", "--list-avail"], capture_output=True, text=True, timeout=120)
    listing = avail.stdout + avail.stderr
    rec = {"probe": os.path.basename(a.probe), "caps": caps, "launches_per_cap": LAUNCHES, "counters": {}, "unavailable": [],
           "failed_passes": []}
    for gi, group in enumerate(GROUPS):
        have = [c for c in group if c in listing]
        rec["unavailable"] += [c for c in group if c not in have]
        if not have:
            continue
        d = os.path.join(a.workdir, f"g{gi}")
        cmd = ["timeout", "-k", "10", "180", "rocprofv3", "--pmc", *have, "--output-format", "csv", "-d", d, "-o", "pmc", "--",
               a.probe, "--draws", "1", "--rounds", "1", "--launches", str(LAUNCHES), "--caps", a.caps]
        r = subprocess.run(cmd, capture_output=True, text=True)
        if r.returncode != 0:
            rec["failed_passes"].append({"counters": have, "status": r.returncode, "stderr_tail": r.stderr[-400:]})
            if r.returncode in FATAL:
                break
            continue
        rows = []
        for path in glob.glob(os.path.join(d, "**", "*counter_collection.csv"), recursive=True):
            with open(path) as f:
                rows += [x for x in csv.DictReader(f) if "window_step_kernel" in x.get("Kernel_Name", "")]
        for c in have:
            mine = sorted((x for x in rows if x["Counter_Name"] == c), key=lambda x: int(x["Dispatch_Id"]))
            per_cap = {}
            for i, cap in enumerate(caps):
                vals = [float(x["Counter_Value"]) for x in mine[len(caps) + i::len(caps)]]     # after the warm-up pair
                per_cap[str(cap)] = {"median": statistics.median(vals) if vals else None, "launches": len(vals)}
            rec["counters"][c] = per_cap
    if not rec["counters"]:
        rec["note"] = "no memory-side counter could be collected on this device: the timings stand alone"
    with open(a.out, "w") as f:
        json.dump(rec, f, indent=1)
    print(json.dumps(rec))
    return 0 if not any(p["status"] in FATAL for p in rec["failed_passes"]) else 1


if __name__ == "__main__":
    sys.exit(main())
