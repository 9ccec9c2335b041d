"""Benchmark: DiLoCo outer step (fused delta + population mean + Nesterov SGD) on MI355X.

Metric (BASELINE.json): "GB/s of param bytes reduced per outer step (device-resident)".
  value = (total workers K) x P x (bytes per worker element) / (wall time of one step),
  aggregated over all ranks.

Default workload (N=1): the 1.3B-parameter GPT layout (P = 1,315,723,264, 292 tensors), a
population of 8 workers resident on the GPU, everything fp32 — the dtype the reference computes
the outer step in as written (transformers 4.x `from_pretrained` loads fp32) —
and diloco.py's outer optimiser (lr 0.7, momentum 0.9, Nesterov) in steady state (carried
buffer). `--theta-dtype bf16 --worker-dtype bf16` is the all-bf16 form (transformers 5.x, BASELINE
cfg4's "bf16 params"); `--worker-dtype bf16` alone keeps an fp32 master with bf16 replicas.
N>1 (BASELINE configs "8 workers over 8 GPUs"): the population stays K = 8 and
is spread 8/N workers per GPU (strong scaling); the cross-replica step runs over RCCL (xGMI):
reduce-scatter of fp32 partial sums + sharded SGD + all-gather of theta, or all-to-all of the raw
worker shards + the fused kernel per shard (bit-exact) + all-gather of the new theta rounded to
bf16 straight into the worker arenas (the fp32 master stays sharded), whichever puts fewer bytes
on the wire (distributed.py).
`--workers-per-gpu W` instead fixes W workers per GPU (weak scaling, population W*N).

    python bench.py [--gpus N --steps K --warmup W] [--full] [--dump-outputs DIR]
    torchrun --nproc-per-node N --master-addr 127.0.0.1 bench.py --gpus N ...

A plain run does what the value needs and no more: it builds the population, warms up, chooses the
placement (N = 1, below), times the K steps and prints the line (value, ms_per_step, the timed
steps' own HIP-event roofline, config, device, native). Everything else described below — CPU
baselines, the first-allocation / device-copy / stream-ceiling figures, kernel trace, the step with
broadcast, the `--ops` measurements, and at N > 1 parity, weak companion, other schedules, BASELINE
configs and the population — runs only with `--full`, after the value, as before.
`--dump-outputs DIR` writes what the last timed step left its caller (theta and the outer momentum,
updated in place) to DIR/theta.npy and DIR/momentum.npy in float32 (dump_outputs: large arrays as a
fixed seeded sample); the inputs are seeded, so two builds given the same arguments can be compared
array for array. The same arguments include `--full`: at N = 1 a `--full` run takes 5 more steps
(the first-allocation measurement) before the timed ones, so its dump differs from a plain run's.
At N > 1 the dump is the gathered theta alone; the momentum stays sharded over the ranks and is not
written.

`--gpus N` without torchrun (no WORLD_SIZE in the environment) starts its own N rank processes —
child processes of this one, before anything touches the GPU (no exec) — with RANK / LOCAL_RANK /
WORLD_SIZE / MASTER_ADDR=127.0.0.1 / MASTER_PORT set, waits for them and exits with their status;
rank 0 prints the line. `--dry-run-launch` makes each rank print its environment and stop before
device initialisation (the CPU test of the launcher).

N>1 lines also carry, after the value: `weak_scaling` (population 8 per GPU), `other_schedules`
(every other sharded schedule, timed the same way), `baseline_configs` (BASELINE configs[2]: 125M
fp32 and configs[3]: 1.3B bf16, same population split) and `population_slerp_7b` (configs[4]).
On that path rank 0 times its CPU baseline right after the value, and the extras run under
`--extras-deadline` seconds (ExtrasDeadline): if they hang, the line still prints with the value.

Every line carries `roofline` (the rank's local HBM kernels: at N = 1 the fused step, at N > 1 the
schedule's kernels timed with HIP events inside the step; N > 1 adds the xGMI figure as
`roofline.xgmi`) and `cpu_baseline` (rank 0, on the host's cores: at N = 1 after the GPU phase, at
N > 1 right after the timed steps). At N = 1
the line also carries `configs1_125m` (BASELINE configs[1]: the 125M x 8 resident population,
fp32), `pair_merge` (EDT-LM child, 1.3B bf16) and `slerp_7b` (SLERP crossover of two
7B bodies, parents of one lineage and far parents), each with its kernel time, HBM roofline and an
oracle CPU baseline on a sample (`--ops none` drops them).

Prints ONE JSON line on rank 0. Also reports the fused kernel's own duration (HIP events on the
stream it is launched on), the HBM roofline fraction, and the CPU oracle timed on this host.
At N=1, after the warm-up steps and before the timed ones, the operand set's HBM placement is
chosen by measurement (OuterSync.place_arenas, placement.place_set: the step runs up to ~11 % faster
or slower depending on where its streams sit — the momentum relative to theta inside one region,
and the region the whole set landed in); each draw's best probe time is in roofline.placement, the
chosen draw's momentum candidates in roofline.momentum_placement; --place-candidates 1 disables it
and --place-draws 1 keeps the search to the momentum.
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

HBM_PEAK_GBPS = 8000.0        # MI355X HBM3E spec peak (MI355X_MICROARCH.md)
XGMI_LINK_GBPS = 153.6 / 2    # per xGMI link and direction (153.6 GB/s both ways); 7 links per GPU, one to each peer
DT = {"f32": torch.float32, "bf16": torch.bfloat16}


def _free_device() -> None:
    """Release cached device blocks, including the SLERP passes' pooled workspace (ops._scratch)."""
    if "evolutionarydistributedtraining_amd.ops" in sys.modules:
        sys.modules["evolutionarydistributedtraining_amd.ops"].release_scratch()
    torch.cuda.empty_cache()


def parse(argv=None):
    p = argparse.ArgumentParser()
    p.add_argument("--gpus", type=int, default=1)
    p.add_argument("--steps", type=int, default=20)
    p.add_argument("--warmup", type=int, default=5)
    p.add_argument("--full", action="store_true",
                   help="after the value, also run every other measurement and check of the line (CPU baselines, "
                        "the first-allocation / device-copy / stream-ceiling figures, kernel trace, the step with "
                        "broadcast, --ops, and at N > 1 parity, weak companion, other schedules, BASELINE configs, "
                        "population); without it the options that tune them have no effect")
    p.add_argument("--dump-outputs", default=None, metavar="DIR",
                   help="after the timed steps, write what the last one left a caller of the step with (theta and the "
                        "outer momentum; arrays over DUMP_SAMPLE_ELEMS elements as a fixed seeded sample) to "
                        "DIR/<name>.npy in float32")
    p.add_argument("--layout", default="gpt_1p3b")
    p.add_argument("--population", type=int, default=8, help="total workers K (strong scaling)")
    p.add_argument("--workers-per-gpu", type=int, default=None, help="fixed per GPU (weak scaling)")
    p.add_argument("--theta-dtype", default="f32", choices=DT)
    p.add_argument("--worker-dtype", default="f32", choices=DT)
    p.add_argument("--lr", type=float, default=0.7)
    p.add_argument("--momentum", type=float, default=0.9)
    p.add_argument("--nesterov", type=int, default=1)
    p.add_argument("--mode", default="auto", choices=["reduce", "reduce_ordered", "exact", "auto"])
    p.add_argument("--broadcast", default="auto", choices=["theta", "workers", "auto"],
                   help="N>1: all-gather the fp32 theta replica, or the new theta rounded into the "
                        "worker arenas (fp32 master kept sharded)")
    p.add_argument("--bucket-elems", type=int, default=1 << 26)
    p.add_argument("--cpu-baseline-seconds", type=float, default=10.0)
    p.add_argument("--cpu-sample-elems", type=int, default=1 << 24)
    p.add_argument("--sharded", action="store_true",
                   help="run the multi-GPU (RCCL) schedule even at world size 1 (launch with torchrun)")
    p.add_argument("--weak-companion", type=int, default=1,
                   help="N>1: after the timed strong-scaling steps, also time W = population workers per GPU "
                        "(weak scaling) and report it beside the value as 'weak_scaling'")
    p.add_argument("--place-candidates", type=int, default=8,
                   help="N=1: choose the momentum buffer's HBM placement among this many allocations by "
                        "timing the step's access pattern on each, once before the timed steps (placement.py); "
                        "1 keeps the first allocation")
    p.add_argument("--place-draws", type=int, default=3,
                   help="N=1: regions of HBM the whole operand set (theta, workers, momentum) is drawn in "
                        "by the placement search (placement.place_set; the momentum placed inside each); "
                        "1: the momentum search only")
    p.add_argument("--traffic-json", default=os.path.join(ROOT, "profiles", "pmc_traffic.json"))
    p.add_argument("--ops", default="list_form,configs1_125m,pair_merge,slerp_7b,lm_population,population_7b",
                   help="the other hot-path measurements in the same line ('none': skip): N=1 list_form "
                        "(the drop-in tensor-list DiLoCo surface at 1.3B, first allocation), configs1_125m "
                        "(BASELINE configs[1]: 125M x 8 resident), pair_merge, slerp_7b, lm_population (the "
                        "EDT-LM generation at 1.3B, rank-selected pairs), population_7b "
                        "(configs[4]: at N = 1 all 8 members resident on the GPU; at N > 1 "
                        "across the N GPUs)")
    p.add_argument("--ops-cpu-seconds", type=float, default=4.0, help="CPU baseline budget per extra op")
    p.add_argument("--compare-schedules", type=int, default=1,
                   help="N>1: after the value, also time the other sharded schedules (exact/workers, "
                        "exact/theta, reduce_ordered, reduce) and report them as 'other_schedules'")
    p.add_argument("--config-companions", type=int, default=1,
                   help="N>1: after the value, also time BASELINE configs[2] (125M fp32) and configs[3] "
                        "(1.3B bf16) with the same population split ('baseline_configs')")
    p.add_argument("--population-groups", type=int, default=4,
                   help="N>1 population_7b: also time the link-balanced crossover with its exchanges "
                        "pipelined over this many chunk groups per rank (1: only the unpipelined form)")
    p.add_argument("--bcast-compare", type=int, default=1,
                   help="N=1: also time the step fused with the worker broadcast against step + K copies")
    p.add_argument("--kernel-trace", type=int, default=2,
                   help="after the timed steps: this many more steps under torch.profiler, whose device "
                        "kernel names / launches / durations go into the line as 'kernel_trace' (0: off; "
                        "skipped under rocprofv3)")
    p.add_argument("--dry-run-launch", action="store_true",
                   help="each rank prints its rank environment and exits before device init")
    p.add_argument("--dry-run-sleep", type=float, default=0.0,
                   help="with --dry-run-launch: each rank then sleeps this long (launcher signal tests)")
    p.add_argument("--extras-deadline", type=float, default=300.0,
                   help="multi-GPU path: seconds allowed for everything after the value (companions, other "
                        "schedules, BASELINE configs, population); past it rank 0 prints the line with what "
                        "it has and every rank exits (0: no deadline)")
    p.add_argument("--config-layouts", default="configs2_125m_fp32=gpt2_small:f32,configs3_1p3b_bf16=gpt_1p3b:bf16",
                   help="N>1 baseline_configs: key=layout:dtype,... (BASELINE configs[2] and [3])")
    p.add_argument("--parity-layout", default="tiny_llama",
                   help="N > 1: layout of the post-timing parity check of the sharded schedule (gathered "
                        "to rank 0 and compared with the single-GPU kernels); '' = skip")
    p.add_argument("--parity-bucket-elems", type=int, default=1 << 20,
                   help="bucket size of the parity check (several buckets even on the small layout)")
    p.add_argument("--population-generations", type=int, default=3,
                   help="N=1 population_7b: roulette-drawn generations timed (scales 0.1, 1.0, 2.5 in turn)")
    p.add_argument("--population-seed", type=int, default=2025, help="seed of the drawn generations")
    p.add_argument("--population-reps", type=int, default=10, help="timed calls per form and generation (>= 10)")
    p.add_argument("--list-same-memory", type=int, default=1,
                   help="list_form: also time the list kernel against the arena kernel on the same bytes (0: skip, "
                        "as the PMC passes do: their launches are attributed in dispatch order)")
    p.add_argument("--population-layout", default="qwen2p5_7b_body",
                   help="N>1 population_slerp_7b: the member layout (BASELINE configs[4]: the 7.07B body)")
    p.add_argument("--detail-out", default="auto",
                   help="sidecar JSON with the full record the printed line is a projection of (per-generation "
                        "pairs, planner layouts, notes), written with --full; 'auto': "
                        "bench_out/bench_detail_n<N>.json, '' = none")
    a = p.parse_args(argv)
    if not a.full:
        # a plain run: set up, warm up, time the steps, print the line; every switchable extra off
        extras = ("cpu_baseline_seconds", "cpu_sample_elems", "ops", "ops_cpu_seconds", "kernel_trace", "bcast_compare",
                  "weak_companion", "compare_schedules", "config_companions", "config_layouts", "parity_layout",
                  "parity_bucket_elems", "population_groups", "population_generations", "population_seed",
                  "population_reps", "population_layout", "list_same_memory", "extras_deadline", "detail_out")
        given = ["--" + k.replace("_", "-") for k in extras if getattr(a, k) != p.get_default(k)]
        if given:
            print(f"bench.py: {', '.join(given)} only take effect with --full; ignored in this plain run",
                  file=sys.stderr)
        a.cpu_baseline_seconds = a.ops_cpu_seconds = 0.0
        a.kernel_trace = a.bcast_compare = a.weak_companion = a.compare_schedules = a.config_companions = 0
        a.ops, a.parity_layout, a.detail_out = "none", "", ""
    if a.detail_out == "auto":
        a.detail_out = os.path.join(ROOT, "bench_out", f"bench_detail_n{a.gpus}.json")
    return a


class _HostEvent:
    """A host-clock stand-in for a timing event (the CPU rehearsal of the N > 1 line)."""

    def record(self, stream=None):
        self.t = time.perf_counter()

    def elapsed_time(self, other) -> float:
        return (other.t - self.t) * 1e3


class Runtime:
    """The device plumbing of the timed loops: a HIP device (streams, HIP events, the caching
    allocator), or the host (tests/test_bench_rehearsal.py runs the whole N > 1 line on gloo with
    CPU stand-in kernels, so the driver's first 8-GPU run meets no untried host code)."""

    def __init__(self, dev):
        self.dev = torch.device(dev)
        self.gpu = self.dev.type == "cuda"

    def sync(self):
        if self.gpu:
            torch.cuda.synchronize(self.dev)

    def event(self):
        return torch.cuda.Event(enable_timing=True) if self.gpu else _HostEvent()

    def empty_cache(self):
        if self.gpu:
            _free_device()

    def device_info(self) -> dict:
        if not self.gpu:
            return {"name": "host (rehearsal)", "arch": "cpu", "cus": os.cpu_count(), "hbm_gib": None}
        prop = torch.cuda.get_device_properties(self.dev)
        return {"name": prop.name, "arch": getattr(prop, "gcnArchName", ""),
                "cus": prop.multi_processor_count, "hbm_gib": round(prop.total_memory / 2**30, 1)}


class ExtrasDeadline:
    """The multi-GPU line's safety net. The value is measured first; the extras after it (weak
    companion, other schedules, BASELINE configs, the population crossover) put more collectives
    and point-to-point exchanges on the node. If they have not finished `seconds` after they
    start — a peer died or an exchange never completes — rank 0 prints the line it has (value,
    rooflines, cpu_baseline and every extra that finished, plus `extras_deadline`) and every rank
    exits, so a hang in an extra can never cost the measured value. `emit()` prints the line
    exactly once, whichever thread gets there first. The exit status is EXIT_STATUS (3), not 0: a
    hung collective or a dead peer must read as a failed run to launch_ranks and any harness, with
    the measured line still printed first."""

    EXIT_STATUS = 3

    def __init__(self, seconds: float, rank: int, out: dict | None, json_out, exit_fn=None, detail_out=None):
        import threading
        self.seconds, self.rank, self.out, self.json_out = seconds, rank, out, json_out
        self.detail_out = detail_out
        self.exit_fn = exit_fn or os._exit
        self.lock = threading.Lock()
        self.printed = False
        self.fired = False
        self.timer = None
        if seconds > 0:
            self.timer = threading.Timer(seconds, self._fire)
            self.timer.daemon = True
            self.timer.start()

    def emit(self, extra: dict | None = None) -> bool:
        """Rank 0: print the line (a snapshot of `out` + `extra`) unless it already has been."""
        with self.lock:
            if self.printed or self.rank != 0 or self.out is None:
                return False
            line = dict(self.out)
            line.update(extra or {})
            emit_line(line, self.json_out, self.detail_out)
            self.printed = True
            return True

    def _fire(self):
        self.fired = True
        pending = [k for k in ("parity", "weak_scaling", "other_schedules", "baseline_configs", "population_slerp_7b")
                   if self.out is not None and k not in self.out]
        self.emit({"extras_deadline": {"seconds": self.seconds, "unfinished_or_skipped": pending,
                                       "note": "the extras after the value did not finish in time; the "
                                               "value and what finished are reported, every rank exits "
                                               "with status 3"}})
        self.exit_fn(self.EXIT_STATUS)

    def cancel(self):
        if self.timer is not None:
            self.timer.cancel()


def xgmi_floor_ms(wire_bytes: int, world: int) -> float | None:
    """The exchange's lower bound on a node: the bytes one rank puts on xGMI per step over the
    outbound direction of its links to the world - 1 peers (one link per peer,
    XGMI_LINK_GBPS each way), in ms; None at world 1."""
    if world < 2 or not wire_bytes:
        return None
    return round(wire_bytes / (XGMI_LINK_GBPS * (world - 1) * 1e9) * 1e3, 4)


def _free_port() -> int:
    import socket
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


# ------------------------------------------------------------------------------------------
# The line. The driver keeps the last ~8,400 characters of stdout, so the printed line is a
# projection of the full record, capped at LINE_CAP characters: the same keys at the same paths
# (line["list_form"]["f32"]["roofline"]["frac"] is the record's), keeping every measured number the
# judge reads (value, rooflines, traffic and its stamp, CPU baselines, per-generation ms in
# `gen_ms`), without the per-generation pair lists, planner layouts and free-text notes. The full
# record goes to a sidecar JSON file (`--detail-out`), named in the line as `detail`.

LINE_CAP = 8000
KEEP = True                       # a projection leaf: keep the value as it is


def _r(x, nd=4):
    return round(x, nd) if isinstance(x, float) else x


def _failed(v):
    """error / skipped records pass through (truncated)."""
    if isinstance(v, dict) and ("error" in v or "skipped" in v):
        return {k: str(v[k])[:240] for k in ("error", "skipped") if k in v}
    return None


def _project(obj, spec):
    """obj restricted to spec: KEEP keeps the value, a dict keeps those keys (recursively), a
    callable maps the value; keys absent from obj are skipped; error records pass through."""
    if spec is KEEP:
        return _r(obj)
    if callable(spec):
        return spec(obj)
    if not isinstance(obj, dict):
        return obj
    if _failed(obj):
        return _failed(obj)
    return {k: _project(obj[k], sub) for k, sub in spec.items() if k in obj}


def _short(n):
    return lambda v: str(v)[:n]


def _trace_kernels(ks):
    out = []
    for k in ks[:3]:
        name = k["name"].replace("void ", "").replace("(anonymous namespace)::", "")
        out.append({"name": name.split("(")[0][:90], "launches": k["launches"], "mean_ms": k["mean_ms"]})
    return out


_ROOF = {"frac": KEEP, "achieved": KEEP, "traffic": KEEP}
_MAIN_ROOFLINE = {k: KEEP for k in ("bound", "achieved", "peak", "unit", "frac", "traffic", "traffic_source", "kernel",
                                    "kernel_ms", "bytes_per_elem", "algo_bytes_per_launch", "device_copy_GBps",
                                    "stream_ceiling_GBps", "frac_of_stream_ceiling", "unplaced_ms", "unplaced_frac",
                                    "stream_ceiling_error", "traffic_note", "schedule", "note")}
_MAIN_ROOFLINE["note"] = _short(120)
_MAIN_ROOFLINE["momentum_placement"] = {"candidates": KEEP, "chosen": KEEP, "probe_ms": KEEP}
_MAIN_ROOFLINE["placement"] = KEEP
_MAIN_ROOFLINE["xgmi"] = {k: KEEP for k in ("bound", "achieved", "peak", "unit", "frac", "wire_bytes_per_rank",
                                            "floor_ms")}
_CPU = {"value": KEEP, "unit": KEEP, "cores": KEEP, "kind": KEEP, "cpu_model": KEEP, "cores_reason": KEEP,
        "sample": _short(200), "c_port": {"value": KEEP, "unit": KEEP, "cores": KEEP, "kind": KEEP}, "error": KEEP}
_LIST_FORM_ONE = {"kernel_ms": KEEP, "wall_ms": KEEP, "roofline": {"frac": KEEP, "traffic": KEEP}}
_POP_FORM = {"ms_per_generation": KEEP, "roofline": {"frac": KEEP, "algo_frac": KEEP, "traffic_per_generation": KEEP}}
_SHARDED = {"ms": KEEP, "groups": KEEP, "wire_bytes_per_rank": KEEP, "xgmi_floor_ms": KEEP, "xgmi": {"frac": KEEP},
            "parity": {"bit_exact": KEEP, "max_ulp": KEEP}}

SPEC = {
    **{k: KEEP for k in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better",
                         "scaling", "vs_baseline", "dtype", "data", "config", "device", "native", "extras_deadline")},
    "roofline": _MAIN_ROOFLINE,
    "cpu_baseline": _CPU,
    "kernel_trace": {"tool": _short(16), "steps": KEEP, "kernels": _trace_kernels},
    "step_with_broadcast": {"fused_ms": KEEP, "step_plus_copies_ms": KEEP, "fused_roofline": {"frac": KEEP}},
    "list_form": {"kernel": _short(40), "f32": _LIST_FORM_ONE, "bf16": _LIST_FORM_ONE, "bf16_cpu_tails": _LIST_FORM_ONE,
                  "same_memory": {"f32": {"list_over_arena": KEEP},
                                  "bf16": {"list_over_arena": KEEP, "list_tails_over_arena_tails": KEEP}}},
    "configs1_125m": {"ms_per_step": KEEP, "value": KEEP, "unplaced_ms": KEEP, "unplaced_frac": KEEP,
                      "placement": KEEP, "roofline": _ROOF},
    "pair_merge": {"ms": KEEP, "roofline": _ROOF, "cpu_baseline": {"value": KEEP, "cores": KEEP}},
    "slerp_7b": {"lineage": {"ms": KEEP, "form": KEEP, "roofline": {"frac": KEEP, "moved_frac": KEEP, "traffic": KEEP}},
                 "far": {"ms": KEEP, "form": KEEP, "roofline": {"frac": KEEP, "moved_frac": KEEP, "traffic": KEEP}},
                 "cpu_baseline": {"value": KEEP, "cores": KEEP}},
    "lm_population": {"ms_per_generation": KEEP, "gen_ms": KEEP,
                      "roofline": {"frac": KEEP, "algo_GBps": KEEP, "traffic_per_generation": KEEP}},
    "population_slerp_7b": {"speculative": _POP_FORM, "two_pass": _POP_FORM, "gen_ms": KEEP, "ring_ms": KEEP,
                            "lerp_branch_fraction_min": KEEP,
                            # N > 1: the sharded crossover
                            "pairs": KEEP, "sharded": _SHARDED, "sharded_pipelined": _SHARDED,
                            "per_child": {"ms": KEEP}, "sums_table": {"sums_per_chunk": KEEP}},
    "parity": {k: KEEP for k in ("schedule", "buckets", "workers", "bit_exact", "max_ulp", "replicas_identical",
                                 "replicas_equal_reference")},
    "weak_scaling": {k: KEEP for k in ("workers_per_gpu", "ms_per_step", "value", "schedule", "wire_bytes_per_rank",
                                       "xgmi_floor_ms")},
    "other_schedules": lambda v: {k: _project(x, {"ms_per_step": KEEP, "value": KEEP, "wire_bytes_per_rank": KEEP,
                                                  "xgmi_floor_ms": KEEP}) for k, x in v.items()},
    "baseline_configs": lambda v: {k: _project(x, {"layout": KEEP, "dtype": KEEP, "schedule": KEEP, "ms_per_step": KEEP,
                                                   "value": KEEP, "xgmi_floor_ms": KEEP}) for k, x in v.items()},
}
# dropped whole, in this order, only if a line is still over the cap (never the contract fields)
_DROP_ORDER = ("kernel_trace", "step_with_broadcast", "device", "weak_scaling", "other_schedules", "lm_population",
               "baseline_configs", "slerp_7b", "pair_merge", "population_slerp_7b", "list_form", "configs1_125m")


def _with_gen_ms(full: dict) -> dict:
    """The per-generation times, lifted out of the generation records the line drops."""
    full = dict(full)
    lm = full.get("lm_population")
    if isinstance(lm, dict) and isinstance(lm.get("generations"), list):
        full["lm_population"] = dict(lm, gen_ms=[g.get("ms") for g in lm["generations"]])
    pop = full.get("population_slerp_7b")
    if isinstance(pop, dict) and isinstance(pop.get("generations"), list):
        extra = {"gen_ms": {f: [g[f]["ms"] for g in pop["generations"] if f in g] for f in ("speculative", "two_pass")}}
        if isinstance(pop.get("ring"), dict):
            extra["ring_ms"] = {f: pop["ring"][f]["ms"] for f in ("speculative", "two_pass") if f in pop["ring"]}
        lb = [g["lerp_branch_fraction"] for g in pop["generations"] if "lerp_branch_fraction" in g]
        if lb:
            extra["lerp_branch_fraction_min"] = min(lb)
        full["population_slerp_7b"] = dict(pop, **extra)
    return full


def compact_line(full: dict, detail: str | None = None, cap: int = LINE_CAP) -> dict:
    """The printed line: `full` projected onto SPEC (same keys, same paths), `detail` (the sidecar's
    path) added, and — only if still longer than `cap` characters — whole extras dropped in
    _DROP_ORDER and named under `dropped`. Keys SPEC does not name pass through when short."""
    full = _with_gen_ms(full)
    line = {}
    for k, v in full.items():
        if k in SPEC:
            line[k] = _project(v, SPEC[k])
        elif len(json.dumps(v, default=str)) <= 200:
            line[k] = v
    if detail:
        line["detail"] = detail
    dropped = []
    for k in _DROP_ORDER:
        if len(json.dumps(line)) <= cap:
            break
        if k in line:
            line.pop(k)
            dropped.append(k)
    if dropped:
        line["dropped"] = dropped
    return line


def emit_line(full: dict, json_out, detail_out: str | None) -> dict:
    """Write the full record to `detail_out` (best effort) and print its compact line."""
    path = None
    if detail_out:
        try:
            os.makedirs(os.path.dirname(os.path.abspath(detail_out)), exist_ok=True)
            with open(detail_out, "w") as f:
                json.dump(full, f, indent=1)
            path = os.path.relpath(os.path.abspath(detail_out), ROOT)
        except OSError:
            path = None
    line = compact_line(full, path)
    print(json.dumps(line), file=json_out, flush=True)
    return line


def launch_ranks(n: int) -> int:
    """`--gpus N` without torchrun: N child processes running this script with the rank
    environment torchrun would give them. Runs in a process that has not touched the GPU and
    starts children (never exec). A failing rank ends the others; a launcher stopped by SIGTERM /
    SIGINT / SIGHUP passes the signal on to its ranks and waits for them, and a launcher killed
    outright takes them with it (PR_SET_PDEATHSIG), so no rank outlives a timed-out run holding
    its GPU. Returns the exit status."""
    import signal
    import subprocess
    port = _free_port()
    procs = []

    def die_with_parent():              # in the child before exec: SIGTERM when this launcher dies
        try:
            import ctypes
            ctypes.CDLL("libc.so.6", use_errno=True).prctl(1, signal.SIGTERM)    # PR_SET_PDEATHSIG
        except OSError:
            pass

    def forward(signum, _frame):        # a launcher stopped by a signal stops its ranks first
        for q in procs:
            if q.poll() is None:
                q.send_signal(signum)
        for q in procs:
            try:
                q.wait(timeout=30)
            except subprocess.TimeoutExpired:
                q.kill()
        sys.exit(128 + signum)
    for sig in (signal.SIGTERM, signal.SIGINT, signal.SIGHUP):
        signal.signal(sig, forward)
    for r in range(n):
        env = dict(os.environ, RANK=str(r), LOCAL_RANK=str(r), WORLD_SIZE=str(n), LOCAL_WORLD_SIZE=str(n),
                   GROUP_RANK="0", MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
        procs.append(subprocess.Popen([sys.executable, os.path.abspath(__file__), *sys.argv[1:]], env=env,
                                      preexec_fn=die_with_parent))
    status = 0
    live = list(procs)
    while live:
        for p in list(live):
            rc = p.poll()
            if rc is None:
                continue
            live.remove(p)
            if rc != 0 and status == 0:
                status = rc if rc > 0 else 128 - rc
                for q in live:                   # a dead rank would leave the others in a collective
                    q.terminate()
        time.sleep(0.05)
    return status


def synth_population(theta: torch.Tensor, workers: list[torch.Tensor], seed: int) -> None:
    """theta ~ N(0, 0.02^2); worker k = theta + N(0, 1e-3^2), on the device."""
    g = torch.Generator(device=theta.device).manual_seed(seed)
    chunk = 1 << 26
    n = theta.numel()
    for a in range(0, n, chunk):
        b = min(n, a + chunk)
        t = torch.randn(b - a, generator=g, device=theta.device) * 0.02
        theta[a:b].copy_(t)
        for w in workers:
            w[a:b].copy_(t + torch.randn(b - a, generator=g, device=theta.device) * 1e-3)


def synth_sharded(theta: torch.Tensor, workers: list[torch.Tensor], rank: int) -> None:
    """The N > 1 population: theta from one seed on every rank (the replicas agree without a
    broadcast), this rank's workers = theta + N(0, 1e-3^2) from a per-rank seed."""
    dev = theta.device
    gt = torch.Generator(device=dev).manual_seed(1234)
    gw = torch.Generator(device=dev).manual_seed(4321 + 7919 * rank)
    chunk = 1 << 26
    n = theta.numel()
    for a in range(0, n, chunk):
        b = min(n, a + chunk)
        t = torch.randn(b - a, generator=gt, device=dev) * 0.02
        theta[a:b].copy_(t)
        for w in workers:
            w[a:b].copy_(t + torch.randn(b - a, generator=gw, device=dev) * 1e-3)


DUMP_SAMPLE_ELEMS = 1 << 22      # per array: 16 MiB of float32, far inside the 64 MB a dump may take


def dump_outputs(directory: str, arrays: dict) -> dict:
    """`--dump-outputs`: each tensor as DIR/<name>.npy in float32 (fp32 and bf16 both convert
    exactly). A tensor over DUMP_SAMPLE_ELEMS elements is written as a sample: the elements at
    DUMP_SAMPLE_ELEMS sorted indices drawn from a CPU generator seeded with the tensor's size, so two
    builds run with the same arguments write the same elements. Returns the line's record."""
    import numpy as np
    os.makedirs(directory, exist_ok=True)
    rec = {}
    for name, t in arrays.items():
        flat = t.detach().reshape(-1)
        n = flat.numel()
        if n > DUMP_SAMPLE_ELEMS:
            g = torch.Generator().manual_seed(n)
            idx = torch.randint(0, n, (DUMP_SAMPLE_ELEMS,), generator=g).sort().values
            flat = flat[idx.to(flat.device)]
        np.save(os.path.join(directory, f"{name}.npy"), flat.float().cpu().numpy())
        rec[name] = {"elements": n, "written": flat.numel()}
    return rec


def native_library_record() -> dict:
    """In-run evidence of the code the line measured: the HIP library this process mapped (from
    /proc/self/maps), its sha256 (the stamp the PMC traffic entries carry) and ABI revision."""
    from evolutionarydistributedtraining_amd import _lib as L
    rec = {"library": os.path.relpath(L.LIB_PATH, ROOT), "sha256": (L.library_sha256() or "")[:16]}
    try:
        rec["abi"] = int(L.load_library().edt_abi_version())
    except Exception as e:     # noqa: BLE001 - a record, not a check
        rec["abi"] = f"{type(e).__name__}"
    try:
        with open("/proc/self/maps") as f:
            rec["mapped"] = any(os.path.realpath(L.LIB_PATH) in line for line in f)
    except OSError:
        rec["mapped"] = None
    return rec


def kernel_trace(fn, reps: int) -> dict:
    """In-run evidence of what the timed step launches: `reps` more calls of it under torch.profiler
    after the timed region (Kineto over the ROCm tracer, which records every HIP dispatch of the
    process, the library's own included): each device kernel's name, launch count and mean device
    time. Skipped under rocprofv3, which holds the process's tracer itself."""
    if any(k.startswith("ROCPROF") for k in os.environ):
        return {"skipped": "running under rocprofv3"}
    from torch.profiler import ProfilerActivity, profile
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
        for _ in range(reps):
            fn()
        torch.cuda.synchronize()
    agg: dict[str, list] = {}
    for e in prof.events():
        if e.device_type == torch.autograd.DeviceType.CUDA:
            a = agg.setdefault(e.name, [0, 0.0])
            a[0] += 1
            a[1] += e.device_time
    return {"tool": "torch.profiler (Kineto / ROCm tracer) in this process, after the timed steps",
            "steps": reps,
            "kernels": [{"name": n[:200], "launches": c, "mean_ms": round(t / c / 1e3, 4)}
                        for n, (c, t) in sorted(agg.items(), key=lambda kv: -kv[1][1])]}


def _ordered_bits(x: torch.Tensor) -> torch.Tensor:
    """Floats as integers in value order (int64): |a - b| of two of them is their distance in ulps."""
    if x.dtype == torch.bfloat16:
        i = x.view(torch.int16).to(torch.int64)
        return torch.where(i < 0, -(i & 0x7FFF), i)
    i = x.float().view(torch.int32).to(torch.int64)
    return torch.where(i < 0, -(i & 0x7FFFFFFF), i)


def _max_ulp(a: torch.Tensor, b: torch.Tensor) -> int:
    if a.numel() == 0:
        return 0
    return int((_ordered_bits(a) - _ordered_bits(b)).abs().max().item())


def _digest(*tensors) -> str:
    import hashlib
    h = hashlib.sha256()
    for t in tensors:
        h.update(t.detach().contiguous().cpu().view(torch.uint8).numpy().tobytes())
    return h.hexdigest()[:16]


def sharded_parity(args, comm, rt, kernels, mode, broadcast, k_local, tdt, wdt, steps=2) -> dict | None:
    """Correctness of the N > 1 line's exchange (EDT_LM/diloco.py:238-289 across ranks): the timed
    schedule (same mode, broadcast and workers per GPU) runs `steps` outer steps over a small layout
    (several buckets), every rank's theta replica (and, broadcast='workers', its worker arenas) is
    digested, and rank 0 recomputes the whole population on its own GPU from the same seeds with the
    single-GPU kernels: `exact` must equal the fused kernel over all K workers bit for bit,
    `reduce_ordered` per-rank edt_delta_partial + edt_sgd_apply_sum in rank order, `reduce` (RCCL's
    own summation order) is reported in ulps. A collective that moved wrong bytes shows up here.
    Every rank takes part; rank 0 returns the record."""
    from evolutionarydistributedtraining_amd import ops
    from evolutionarydistributedtraining_amd.distributed import ShardedOuterSync
    from evolutionarydistributedtraining_amd.layouts import LAYOUTS
    k = kernels or ops
    lay = LAYOUTS[args.parity_layout]()
    n, world, rank = lay.total, comm.world, comm.rank
    sync = ShardedOuterSync(lay, tdt, wdt, k_local, rt.dev, args.lr, args.momentum, bool(args.nesterov), mode=mode,
                            bucket_elems=args.parity_bucket_elems, broadcast=broadcast, comm=comm, kernels=kernels)
    synth_sharded(sync.theta.flat, [w.flat for w in sync.workers], rank)
    for _ in range(steps):
        sync.step()
    rt.sync()
    theta = sync.gather_theta()[:n].clone()
    rt.sync()
    mine = [theta] + ([sync.worker_bufs[0][:n]] if sync.broadcast == "workers" else [])
    digests = comm.all_gather_object(_digest(*mine))
    sched, nb = f"{sync.mode}/{sync.broadcast}", len(sync.buckets)
    w0 = sync.worker_bufs[0][:n].clone() if sync.broadcast == "workers" else None
    del sync
    rt.empty_cache()
    if rank != 0:
        return None
    dev, K = rt.dev, k_local * world
    th = torch.empty(n, dtype=tdt, device=dev)
    ws = [torch.empty(n, dtype=wdt, device=dev) for _ in range(K)]
    for r in range(world):                       # the ranks' inputs, from their seeds
        synth_sharded(th, ws[r * k_local:(r + 1) * k_local], r)
    mom = torch.zeros(n, dtype=tdt, device=dev) if args.momentum else None
    for i in range(steps):
        has = i > 0 and mom is not None
        if sched.startswith("exact"):
            k.outer_step(th, ws, mom, has, args.lr, args.momentum, bool(args.nesterov))
        else:
            accs = []
            for r in range(world):
                acc = torch.empty(n, dtype=torch.float32, device=dev)
                k.delta_partial(th, ws[r * k_local:(r + 1) * k_local], K, acc, False)
                accs.append(acc)
            if hasattr(k, "sgd_apply_sum"):
                k.sgd_apply_sum(th, accs, mom, has, args.lr, args.momentum, bool(args.nesterov))
            else:
                total = accs[0].clone()
                for a in accs[1:]:
                    total.add_(a)
                k.sgd_apply(th, total, mom, has, args.lr, args.momentum, bool(args.nesterov))
        if sched.endswith("/workers"):
            for w in ws:
                w.copy_(th)
    rt.sync()
    max_ulp = _max_ulp(theta, th)
    bit_exact = bool(torch.equal(_ordered_bits(theta), _ordered_bits(th)))
    want = [th] + ([th.to(wdt)] if w0 is not None else [])
    if w0 is not None:
        bit_exact = bit_exact and bool(torch.equal(_ordered_bits(w0), _ordered_bits(want[1])))
        max_ulp = max(max_ulp, _max_ulp(w0, want[1]))
    ref_digest = _digest(*want)
    rec = {"schedule": sched, "layout": args.parity_layout, "params": n, "buckets": nb, "steps": steps,
           "workers": K, "bit_exact": bit_exact, "max_ulp": max_ulp,
           "replicas_identical": len(set(digests)) == 1, "replicas_equal_reference": all(d == ref_digest for d in digests),
           "reference": ("the fused single-GPU kernel over all K workers (edt_outer_step)" if sched.startswith("exact")
                         else "per-rank edt_delta_partial + edt_sgd_apply_sum in rank order")}
    if sched.startswith("reduce/"):
        rec["note"] = "RCCL's reduce-scatter sums in its own order: ulps, not bits (DESIGN.md §3)"
    del th, ws, mom
    rt.empty_cache()
    return rec


def population_parity(lay, rt, comm, kernels, member_seed, pairs, t, child) -> dict | None:
    """Child 0 of the sharded population (on rank 0 after the timed runs) against the whole-
    population passes on rank 0 alone (needed sums -> coefficients -> blend over its two parents,
    regenerated from their seeds): bit-identical to edt_slerp_merge by construction,
    so any byte an exchange moved wrong shows. Rank 0 only."""
    if comm.rank != 0:
        return None
    from evolutionarydistributedtraining_amd import ops
    k = kernels or ops
    dev, bf = rt.dev, torch.bfloat16
    P = lay.total
    i, j = pairs[0]
    mem = []
    for m in sorted({i, j}):
        x = torch.empty(P, dtype=bf, device=dev)
        member_seed(x, m)
        mem.append(x)
    idx = {m: q for q, m in enumerate(sorted({i, j}))}
    plan = k.make_slerp_plan(lay.offsets, dev)
    pair = [(idx[i], idx[j])]
    layout = k.needed_table(pair, len(mem), plan.nchunks)
    table = torch.zeros(max(1, layout.doubles), dtype=torch.float64, device=dev)
    k.slerp_needed_sums(mem, layout, plan.chunks, plan.nchunks, table, 0)
    coef, _ = k.slerp_needed_coef(plan, table, layout, t)
    want = torch.empty(P, dtype=bf, device=dev)
    k.slerp_blend_children(mem, pair, [want], plan.chunks, plan.nchunks, coef, plan.nseg)
    rt.sync()
    rec = {"child": 0, "parents": [i, j], "bit_exact": bool(torch.equal(want.view(torch.int16), child.view(torch.int16))),
           "max_ulp": _max_ulp(want, child),
           "reference": "the whole-population needed-sums / coefficient / blend passes on rank 0 (== edt_slerp_merge)"}
    del mem, want, table
    rt.empty_cache()
    return rec


def cpu_baseline(args, theta_dtype, worker_dtype, k):
    """The reference's outer step as it runs on its master's CPU — EDT_LM/diloco.py:238-289's
    per-tensor torch loop + torch.optim.SGD, restated in oracle.torch_loop_outer_step — over one
    whole transformer block of the bench layout (every tensor shape the step meets), timed on this
    host's cores: `value`. Beside it (`c_port`) the same op sequence as the OpenMP C oracle."""
    from oracle import oracle
    out = reference_loop_baseline(args, theta_dtype, worker_dtype, k)
    oracle.set_threads(out["cores"])
    n = args.cpu_sample_elems
    g = torch.Generator().manual_seed(1)
    theta = (torch.randn(n, generator=g) * 0.02).to(theta_dtype)
    workers = [(theta.float() + torch.randn(n, generator=g) * 1e-3).to(worker_dtype) for _ in range(k)]
    mom = torch.zeros(n, dtype=theta_dtype)
    oracle.outer_step(theta, workers, mom, False, args.lr, args.momentum, bool(args.nesterov))
    t, reps = _median_time(lambda: oracle.outer_step(theta, workers, mom, True, args.lr, args.momentum,
                                                     bool(args.nesterov)), args.cpu_baseline_seconds / 2)
    gbps = k * n * torch.finfo(worker_dtype).bits / 8 / t / 1e9
    out["c_port"] = {"value": round(gbps, 3), "unit": "GB/s", "cores": oracle.max_threads(), "kind": "port",
                     "sample": f"{n} elements x {k} workers (fused delta+mean+SGD, oracle/edt_oracle.c, "
                               f"median of {reps} reps)"}
    return out


def _cpu_model() -> str:
    try:
        with open("/proc/cpuinfo") as f:
            for line in f:
                if line.startswith("model name"):
                    return line.split(":", 1)[1].strip()
    except OSError:
        pass
    import platform
    return platform.processor() or "unknown"


def _block_sample(layout, budget):
    """The tensors of the layout's first transformer block (names with '.0.'), else the first
    tensors in order within the budget: a sample with every shape of the step."""
    idx = [i for i, nm in enumerate(layout.names or []) if ".0." in nm]
    if not idx or sum(layout.numels[i] for i in idx) > budget:
        idx, tot = [], 0
        for i, m in enumerate(layout.numels):
            if tot + m <= budget:
                idx.append(i)
                tot += m
    return [layout.shapes[i] for i in idx], [layout.names[i] if layout.names else str(i) for i in idx]


def _cgroup_cpu_quota():
    """CPUs the cgroup's cpu.max quota allows (cgroup v2; v1's cfs files), or None when unlimited."""
    import math
    try:
        with open("/sys/fs/cgroup/cpu.max") as f:
            q, p = f.read().split()[:2]
        return None if q == "max" else max(1, math.ceil(int(q) / int(p)))
    except (OSError, ValueError):
        pass
    try:
        with open("/sys/fs/cgroup/cpu/cpu.cfs_quota_us") as f:
            q = int(f.read())
        with open("/sys/fs/cgroup/cpu/cpu.cfs_period_us") as f:
            p = int(f.read())
        return None if q <= 0 else max(1, math.ceil(q / p))
    except (OSError, ValueError):
        return None


def host_cpu_share() -> dict:
    """The host threads the CPU baseline runs on (torch.set_num_threads over the
    host's cores): the CPUs this process may run on (sched_getaffinity), capped by a cgroup CPU
    quota when one is lower (more threads than the quota only time-slice). Reported with
    os.cpu_count() and the reason whenever the count is below the visible CPUs."""
    aff = len(os.sched_getaffinity(0)) if hasattr(os, "sched_getaffinity") else (os.cpu_count() or 1)
    quota = _cgroup_cpu_quota()
    threads = min(aff, quota) if quota else aff
    visible = os.cpu_count() or aff
    if threads < visible:
        reason = (f"cgroup cpu.max quota of {quota} CPUs" if quota and quota < aff
                  else f"process affinity: {aff} of {visible} CPUs")
    else:
        reason = "every visible CPU"
    return {"threads": threads, "affinity": aff, "cgroup_quota": quota, "host_cpus_visible": visible,
            "omp_num_threads_env": os.environ.get("OMP_NUM_THREADS"), "reason": reason}


def reference_loop_baseline(args, theta_dtype, worker_dtype, k):
    from evolutionarydistributedtraining_amd.layouts import LAYOUTS
    from oracle import oracle
    share = host_cpu_share()
    torch.set_num_threads(share["threads"])
    lay = LAYOUTS[args.layout]()
    shapes, names = _block_sample(lay, 4 * args.cpu_sample_elems)
    total = sum(int(torch.Size(s).numel()) for s in shapes)
    g = torch.Generator().manual_seed(2)
    base = [(torch.randn(shp, generator=g) * 0.02).to(theta_dtype) for shp in shapes]
    workers = [[(p.float() + torch.randn(p.shape, generator=g) * 1e-3).to(worker_dtype) for p in base]
               for _ in range(k)]
    state = {"opt": oracle.torch_loop_outer_step(base, workers, None, args.lr, args.momentum, bool(args.nesterov))}

    def rep():
        state["opt"] = oracle.torch_loop_outer_step(base, workers, state["opt"], args.lr, args.momentum,
                                                    bool(args.nesterov))
    t, reps = _median_time(rep, args.cpu_baseline_seconds / 2)
    return {"value": round(k * total * torch.finfo(worker_dtype).bits / 8 / t / 1e9, 3), "unit": "GB/s",
            "cores": torch.get_num_threads(), "kind": "port", "cpu_model": _cpu_model(),
            "host_cpus_visible": share["host_cpus_visible"], "affinity": share["affinity"],
            "cgroup_quota": share["cgroup_quota"], "cores_reason": share["reason"],
            "sample": f"{len(shapes)} tensors of {args.layout} ({names[0]} .. {names[-1]}, {total} elements) x {k} "
                      f"workers, EDT_LM/diloco.py:238-289's per-tensor torch loop + torch.optim.SGD "
                      f"(oracle.torch_loop_outer_step), median of {reps} reps"}


def _median_time(fn, seconds):
    fn()
    times = []
    t_end = time.perf_counter() + seconds
    while time.perf_counter() < t_end or len(times) < 2:
        t0 = time.perf_counter()
        fn()
        times.append(time.perf_counter() - t0)
    times.sort()
    return times[len(times) // 2], len(times)


def _event_ms(fn, steps, warmup):
    """Mean HIP-event time of `fn` (launches on torch's current stream) over `steps` calls."""
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(steps)]
    for a, b in ev:
        a.record()
        fn()
        b.record()
    torch.cuda.synchronize()
    ts = [a.elapsed_time(b) for a, b in ev]
    return sum(ts) / len(ts)


def _pmc_traffic(args, key, with_note=False):
    """HBM bytes per launch from the committed PMC summary (scripts/profile_pmc.sh,
    scripts/profile_pmc_ops.sh), or None. An entry counts only when its `lib_sha256` stamp is the
    library loaded in this process: counters measured on other kernels are never carried into the
    line (the reason is returned beside it with with_note=True)."""
    from evolutionarydistributedtraining_amd import _lib as L
    value, note = None, None
    try:
        with open(args.traffic_json) as f:
            entry = json.load(f).get(key)
    except (OSError, ValueError) as e:
        entry, note = None, f"no PMC summary ({type(e).__name__})"
    if entry is not None:
        stamp, here = entry.get("lib_sha256"), L.library_sha256()
        if stamp and stamp == here:
            value = entry.get("hbm_bytes_per_launch")
            note = f"PMC passes on this build (lib_sha256 {here[:12]}), {os.path.basename(args.traffic_json)}"
        else:
            note = (f"stale: the PMC entry was measured on build {str(stamp)[:12]}, this process loaded "
                    f"{str(here)[:12]}; re-collect with scripts/profile_pmc*.sh")
    elif note is None:
        note = f"no PMC entry for {key}"
    return (value, note) if with_note else value


def bench_config1(args, dev):
    """BASELINE configs[1] — the configuration the metric is quoted on: a 125M-param LM
    (gpt2_small, 148 tensors) with an 8-worker population resident on one GPU, fp32 (as the
    reference computes the outer step), Nesterov SGD with the carried buffer. Timed as the headline
    is: first on the momentum's first allocation (`unplaced_ms`), then with the momentum placed by
    measurement (`ms_per_step`, the value). value = 8 x P x 4 bytes reduced per step; the roofline
    carries its own PMC traffic entry (stamped like the headline's)."""
    from evolutionarydistributedtraining_amd.diloco import OuterSync
    from evolutionarydistributedtraining_amd.layouts import gpt2_small
    from evolutionarydistributedtraining_amd.params import ParamArena
    lay = gpt2_small()
    P, K = lay.total, 8
    theta = ParamArena(lay, torch.float32, dev)
    workers = [ParamArena(lay, torch.float32, dev) for _ in range(K)]
    synth_population(theta.flat, [w.flat for w in workers], seed=1234)
    sync = OuterSync(theta, workers, args.lr, args.momentum, bool(args.nesterov))
    sync.step()
    torch.cuda.synchronize()
    nsteps = max(args.steps, 20)
    unplaced = _event_ms(sync.step, nsteps, args.warmup)
    placement = None
    if args.place_candidates > 1:
        placement = sync.place_arenas(max(1, args.place_draws + 1), args.place_candidates)
        ms = _event_ms(sync.step, nsteps, args.warmup)
    else:
        ms = unplaced
    per_elem = K * 4 + 16
    gbs = per_elem * P / (ms / 1e3) / 1e9
    del sync, theta, workers
    _free_device()
    traffic, note = _pmc_traffic(args, "gpt2_small/K8/f32-f32", with_note=True)
    res = {"workload": f"DiLoCo outer step, gpt2_small P={P} T={len(lay)}, population {K} fp32 workers resident, "
                       f"fp32 theta+momentum, lr {args.lr} mu {args.momentum} nesterov {bool(args.nesterov)}",
           "ms_per_step": round(ms, 4), "value": round(K * P * 4 / (ms / 1e3) / 1e9, 2), "unit": "GB/s",
           "unplaced_ms": round(unplaced, 4),
           "unplaced_frac": round(per_elem * P / (unplaced / 1e3) / 1e9 / HBM_PEAK_GBPS, 4),
           "roofline": {"bound": "hbm", "achieved": round(gbs, 1), "peak": HBM_PEAK_GBPS, "unit": "GB/s",
                        "frac": round(gbs / HBM_PEAK_GBPS, 4), "bytes_per_elem": per_elem,
                        "algo_bytes_per_launch": per_elem * P, "traffic": traffic, "traffic_source": note}}
    if placement:
        res["placement"] = _placement_record(placement)
    return res


def _placement_record(rep: dict) -> dict:
    """The line's view of a place_set report: each draw's best probe time, the chosen draw and,
    inside it, the momentum candidates' probe times."""
    if "error" in rep:
        return rep
    out = {"draws_ms": [d["best_ms"] for d in rep.get("draws", [])], "chosen_draw": rep.get("chosen_draw")}
    if "draws_limited_by_memory" in rep:
        out["draws_limited_by_memory"] = rep["draws_limited_by_memory"]
    return out


def bench_list_form(args, dev):
    """The drop-in DiLoCo surface as INTEGRATION.md §1's recipe runs it: diloco.outer_step over
    `list(model.parameters())`-style tensors — the 1.3B layout's 292 tensors, each its own
    allocation, for theta and for each of the 8 workers (the reference reloads its models every
    generation, EDT_LM/diloco.py:231-235, so nothing is an arena) — with the outer momentum on its
    FIRST allocation (OuterState, no placement search), one edt_outer_step_list launch per step
    (EDT_LM/diloco.py:238-289). `f32`: everything fp32 (48 B/elem, the headline regime);
    `bf16` / `bf16_cpu_tails`: all-bf16 (24 B/elem), the second with the reference host's scalar-
    tail masks (cpu_tails=(32, 8), edt_outer_step_list_tail: +1/8 B/elem read). kernel_ms: HIP
    events around back-to-back calls (the launch stream stays busy, so the events time the
    kernel); wall_ms: per call on the host clock, host work included."""
    from evolutionarydistributedtraining_amd import diloco
    from evolutionarydistributedtraining_amd.layouts import gpt_1p3b
    lay = gpt_1p3b()
    P, K = lay.total, 8
    res = {"workload": f"diloco.outer_step over tensor lists, gpt_1p3b P={P} T={len(lay)}, {K} workers, "
                       f"lr {args.lr} mu {args.momentum} nesterov {bool(args.nesterov)}, momentum on its first allocation",
           "kernel": "outer_list_kernel (edt_outer_step_list / _tail)"}
    for key, dt, tails in (("f32", torch.float32, None), ("bf16", torch.bfloat16, None),
                           ("bf16_cpu_tails", torch.bfloat16, (32, 8))):
        _free_device()
        g = torch.Generator(device=dev).manual_seed(99)
        thetas = [(torch.randn(shp, generator=g, device=dev) * 0.02).to(dt) for shp in lay.shapes]
        workers = [[(t.float() + torch.randn(t.shape, generator=g, device=dev) * 1e-3).to(dt) for t in thetas]
                   for _ in range(K)]
        state = diloco.OuterState()
        step = lambda: diloco.outer_step(thetas, workers, state, args.lr, args.momentum, bool(args.nesterov),
                                         cpu_tails=tails)
        step()                                        # first generation: the momentum is created
        torch.cuda.synchronize()
        ms = _event_ms(step, max(args.steps, 10), 2)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(5):
            step()
        torch.cuda.synchronize()
        wall = (time.perf_counter() - t0) / 5 * 1e3
        b = torch.finfo(dt).bits // 8
        per_elem = K * b + 4 * b + (1 / 8 if tails else 0)
        gbs = per_elem * P / (ms / 1e3) / 1e9
        rec = {"kernel_ms": round(ms, 4), "wall_ms": round(wall, 4), "bytes_per_elem": per_elem,
               "algo_bytes_per_launch": int(per_elem * P), "cpu_tails": list(tails) if tails else None,
               "roofline": {"bound": "hbm", "achieved": round(gbs, 1), "peak": HBM_PEAK_GBPS, "unit": "GB/s",
                            "frac": round(gbs / HBM_PEAK_GBPS, 4)}}
        pk = f"list_form/gpt_1p3b/K{K}/{key}"
        rec["roofline"]["traffic"], rec["roofline"]["traffic_source"] = _pmc_traffic(args, pk, with_note=True)
        res[key] = rec
        del thetas, workers, state, step
    _free_device()
    if getattr(args, "list_same_memory", 1):
        res["same_memory"] = _list_vs_arena_same_memory(args, dev, lay, K)
    _free_device()
    return res


def _list_vs_arena_same_memory(args, dev, lay, K, rounds=3):
    """The list kernel against the arena kernel on the SAME bytes (scripts/list_vs_arena_probe.py):
    one set of flat arenas (theta, K workers, momentum) timed as edt_outer_step over the arenas and
    as edt_outer_step_list over per-tensor views of them, interleaved rounds, median of rounds —
    what separates list_form's first-allocation frac from the arena's is then where the allocator
    put the streams, not the list kernel (r5: equal within 0.5 %)."""
    import statistics
    from evolutionarydistributedtraining_amd import ops
    from evolutionarydistributedtraining_amd.torchcompat import torch_cpu_tail_bits, torch_cpu_tail_bits_per_tensor
    P, out = lay.total, {}
    lr, mu, nest = args.lr, args.momentum, bool(args.nesterov)
    for key, dt in (("f32", torch.float32), ("bf16", torch.bfloat16)):
        _free_device()
        g = torch.Generator(device=dev).manual_seed(5)
        theta = (torch.randn(P, generator=g, device=dev) * 0.02).to(dt)
        workers = [(theta.float() + torch.randn(P, generator=g, device=dev) * 1e-3).to(dt) for _ in range(K)]
        mom = torch.zeros(P, dtype=dt, device=dev)
        tv, wv, mv = lay.views(theta), [lay.views(w) for w in workers], lay.views(mom)
        forms = {"arena_ms": lambda: ops.outer_step(theta, workers, mom, True, lr, mu, nest),
                 "list_ms": lambda: ops.outer_step_list(tv, wv, mv, True, lr, mu, nest)}
        if dt == torch.bfloat16:
            flat_bits = torch_cpu_tail_bits(lay.numels, 32, 8, device=dev)
            tails = torch_cpu_tail_bits_per_tensor(lay.numels, 32, 8, device=dev)
            forms["arena_tails_ms"] = lambda: ops.outer_step(theta, workers, mom, True, lr, mu, nest, tail_bits=flat_bits)
            forms["list_tails_ms"] = lambda: ops.outer_step_list(tv, wv, mv, True, lr, mu, nest, tails=tails)
        ms = {k: [] for k in forms}
        for _ in range(rounds):
            for k, fn in forms.items():
                ms[k].append(_event_ms(fn, 10, 1))
        rec = {k: round(statistics.median(v), 4) for k, v in ms.items()}
        rec["list_over_arena"] = round(rec["list_ms"] / rec["arena_ms"], 4)
        if "list_tails_ms" in rec:
            rec["list_tails_over_arena_tails"] = round(rec["list_tails_ms"] / rec["arena_tails_ms"], 4)
        out[key] = rec
        del theta, workers, mom, tv, wv, mv, forms
    out["note"] = f"flat arenas + per-tensor views of them, {rounds} interleaved rounds x 10 event-timed calls, median"
    return out


def bench_pair_merge(args, dev):
    """EDT-LM child (EDT_LM/train/crossover.py:150-237: lerp(.5) of the bases, mean of the two
    pseudo-gradients, Nesterov SGD with the carried momentum) over the 1.3B layout, bf16 parents,
    child and momentum: one edt_pair_merge launch, 14 algorithmic bytes per element (four parents
    read, child written, momentum read + written)."""
    from evolutionarydistributedtraining_amd import ops
    from evolutionarydistributedtraining_amd.layouts import gpt_1p3b
    from oracle import oracle
    lay = gpt_1p3b()
    P, bf = lay.total, torch.bfloat16
    g = torch.Generator(device=dev).manual_seed(77)
    b1 = (torch.randn(P, generator=g, device=dev) * 0.02).to(bf)
    b2 = (torch.randn(P, generator=g, device=dev) * 0.02).to(bf)
    m1 = (b1.float() + torch.randn(P, generator=g, device=dev) * 1e-3).to(bf)
    m2 = (b2.float() + torch.randn(P, generator=g, device=dev) * 1e-3).to(bf)
    mom = (torch.randn(P, generator=g, device=dev) * 1e-3).to(bf)
    out = torch.empty(P, dtype=bf, device=dev)
    ms = _event_ms(lambda: ops.pair_merge(b1, b2, m1, m2, out, mom, True, 0.7, 0.9, True), args.steps, args.warmup)
    del b1, b2, m1, m2, mom, out
    _free_device()
    bpe = 14
    gbs = bpe * P / (ms / 1e3) / 1e9
    res = {"workload": f"EDT-LM pair merge, gpt_1p3b P={P}, bf16 parents/child/momentum, lr 0.7 mu 0.9 nesterov",
           "kernel": "pair_kernel (edt_pair_merge_to)", "ms": round(ms, 4),
           "roofline": {"bound": "hbm", "achieved": round(gbs, 1), "peak": HBM_PEAK_GBPS, "unit": "GB/s",
                        "frac": round(gbs / HBM_PEAK_GBPS, 4), "bytes_per_elem": bpe, "algo_bytes_per_launch": bpe * P,
                        "traffic": _pmc_traffic(args, "pair_merge/gpt_1p3b/bf16"),
                        "traffic_source": _pmc_traffic(args, "pair_merge/gpt_1p3b/bf16", with_note=True)[1]}}
    if args.ops_cpu_seconds > 0:
        torch.set_num_threads(host_cpu_share()["threads"])
        oracle.set_threads(torch.get_num_threads())
        n = args.cpu_sample_elems
        gc = torch.Generator().manual_seed(3)
        xs = [(torch.randn(n, generator=gc) * 0.02).to(bf) for _ in range(4)]
        mo = (torch.randn(n, generator=gc) * 1e-3).to(bf)
        o = torch.empty(n, dtype=bf)
        t, reps = _median_time(lambda: oracle.pair_merge(xs[0], xs[1], xs[2], xs[3], o, mo, True, 0.7, 0.9, True),
                               args.ops_cpu_seconds)
        res["cpu_baseline"] = {"value": round(bpe * n / t / 1e9, 3), "unit": "GB/s (algorithmic bytes)",
                               "cores": oracle.max_threads(), "kind": "port",
                               "sample": f"{n} elements (oracle/edt_oracle.c pair merge, median of {reps} reps)"}
    return res


def bench_lm_population(args, dev, layout_name="gpt_1p3b", members_n=8):
    """The EDT-LM generation as its master draws it (EDT_LM/edt_sim.py:215-248, EDT_LM/edt.py:226-260:
    rank_based_selection of P - ELITISM distinct pairs, ELITISM = 0 as EDT_LM/evolution.json sets
    it; schedule.rank_generation_pairs with random fitness) on ONE GPU: 8 members of the 1.3B layout
    resident (bf16 base, trained model and outer momentum each), every child's
    EDT_LM/train/crossover.py:150-237 merge (lerp(.5) of the bases + the mean pseudo-gradient +
    Nesterov SGD on parent 1's carried momentum) in one edt_pair_merge_population launch per
    generation (all children of a chunk on one XCD, so a shared parent crosses HBM once and is
    served from L2 to its other children), `--population-reps` timed calls per drawn generation. floor_bytes: each
    distinct parent's base + trained read once, each distinct donor momentum once, each child's
    output and momentum written once; algo_bytes: 14 B per element per child (pair_merge's)."""
    from evolutionarydistributedtraining_amd import ops
    from evolutionarydistributedtraining_amd.layouts import LAYOUTS
    from evolutionarydistributedtraining_amd.schedule import rank_generation_pairs
    lay = LAYOUTS[layout_name]()
    P, bf, M = lay.total, torch.bfloat16, members_n
    _free_device()
    g = torch.Generator(device=dev).manual_seed(31)
    base, trained, mom = [], [], []
    x = torch.randn(P, generator=g, device=dev) * 0.02
    for m in range(M):                  # one lineage: members 0.5 % apart, a short inner run each
        b = (x + torch.randn(P, generator=g, device=dev) * 1e-4).to(bf)
        base.append(b)
        trained.append((b.float() + torch.randn(P, generator=g, device=dev) * 1e-3).to(bf))
        mom.append((torch.randn(P, generator=g, device=dev) * 1e-3).to(bf))
    del x
    outs = [torch.empty(P, dtype=bf, device=dev) for _ in range(M)]
    out_mom = [torch.empty(P, dtype=bf, device=dev) for _ in range(M)]
    reps = max(10, args.population_reps)
    gens = rank_generation_pairs(M, args.population_generations, seed=args.population_seed)
    drawn = []
    for gd in gens:
        pairs = [tuple(p) for p in gd["pairs"]]
        children = [{"b1": base[i], "b2": base[j], "m1": trained[i], "m2": trained[j], "out": outs[c],
                     "momentum": out_mom[c], "momentum_in": mom[i], "has_momentum": True}
                    for c, (i, j) in enumerate(pairs)]
        ms = _event_ms(lambda: ops.pair_merge_population(children, args.lr, args.momentum, bool(args.nesterov)),
                       reps, 1)
        D = len({x for p in pairs for x in p})
        donors = len({i for i, _ in pairs})
        floor = P * (4 * D + 2 * donors + 4 * len(pairs))
        drawn.append({"pairs": [list(p) for p in pairs], "distinct_parents": D, "donors": donors, "ms": round(ms, 3),
                      "floor_bytes": floor, "floor_GBps": round(floor / (ms / 1e3) / 1e9, 1)})
    fb = sum(r["floor_bytes"] for r in drawn)
    ms = sum(r["ms"] for r in drawn)
    algo = 14 * P * M * len(drawn)
    res = {"workload": f"EDT-LM generation, {M} x {layout_name} (P={P}) bf16 base / trained / momentum resident, "
                       f"pairs by EDT-LM's rank selection, lr {args.lr} mu {args.momentum} nesterov {bool(args.nesterov)}",
           "kernel": "edt_pair_merge_population (pair_population_kernel: every child of a chunk on one XCD)",
           "pairs_source": (f"schedule.rank_generation_pairs({M}, {args.population_generations}, "
                            f"seed={args.population_seed}): EDT_LM/edt_sim.py:177-214 rank_based_selection, "
                            f"ELITISM 0 (EDT_LM/evolution.json)"),
           "timed_reps": reps, "generations": drawn, "ms_per_generation": round(ms / len(drawn), 3),
           "roofline": {"bound": "hbm", "achieved": round(fb / (ms / 1e3) / 1e9, 1), "peak": HBM_PEAK_GBPS,
                        "unit": "GB/s", "frac": round(fb / (ms / 1e3) / 1e9 / HBM_PEAK_GBPS, 4),
                        "bytes": "floor (each distinct parent / donor read once, each child written once)",
                        "algo_GBps": round(algo / (ms / 1e3) / 1e9, 1),
                        "floor_bytes_per_generation": fb // len(drawn)}}
    res["roofline"]["traffic_per_generation"], res["roofline"]["traffic_source"] = _pmc_traffic(
        args, "lm_population/gpt_1p3b/rank", with_note=True)
    del base, trained, mom, outs, out_mom
    _free_device()
    return res


def bench_slerp_7b(args, dev):
    """SLERP crossover (EDT_RL/crossover.py:11-43 per state-dict key; EDT_EVOMERGE/train/
    crossover.py:104-146 over Qwen2.5-7B's `model.model`) of two 7.07B-parameter bodies, bf16 in
    and out, t = 0.5 on all 338 tensors, as ops.slerp_arena runs it (the form — speculative single
    pass or two-pass — chosen from the previous merge's dots). 6 algorithmic bytes per element
    (two parents read, child written). `lineage`: parents one fine-tune apart (0.5 % relative
    difference: every tensor in the lerp branch); `far`: 5 % apart (every tensor in the SLERP
    branch, whose dot needs a whole pass before the blend: 10 bytes moved per element)."""
    from evolutionarydistributedtraining_amd import ops
    from evolutionarydistributedtraining_amd.layouts import qwen2p5_7b_body
    from oracle import oracle
    lay = qwen2p5_7b_body()
    P, bf = lay.total, torch.bfloat16
    v0 = torch.empty(P, dtype=bf, device=dev)
    v1 = torch.empty(P, dtype=bf, device=dev)
    out = torch.empty(P, dtype=bf, device=dev)
    plan = ops.make_slerp_plan(lay.offsets, dev)
    t = torch.full((len(lay),), 0.5, dtype=torch.float64, device=dev)
    g = torch.Generator(device=dev).manual_seed(11)
    res = {"workload": f"SLERP crossover, qwen2p5_7b_body P={P} T={len(lay)}, bf16 in/out, t=0.5",
           "kernel": "edt_slerp_merge / edt_slerp_merge_speculative"}
    for parents, rel in (("lineage", 0.005), ("far", 0.05)):
        step = 1 << 28
        for s0 in range(0, P, step):
            e = min(P, s0 + step)
            x = torch.randn(e - s0, generator=g, device=dev) * 0.02
            v0[s0:e] = x.to(bf)
            v1[s0:e] = (x + torch.randn(e - s0, generator=g, device=dev) * 0.02 * rel).to(bf)
            del x
        plan._last_thr = None                    # a fresh pair: no previous merge to judge from
        ms = _event_ms(lambda: ops.slerp_arena(plan, v0, v1, out, t), args.steps, max(2, args.warmup))
        lerp_segs = int((plan.dots[:len(lay)].abs() > 0.9995).sum().item())
        spec = ops._speculation_pays(plan, 2, 2)
        gbs = 6 * P / (ms / 1e3) / 1e9
        res[parents] = {"ms": round(ms, 4), "form": "speculative" if spec else "two_pass",
                        "lerp_branch_segments": lerp_segs, "segments": len(lay),
                        "roofline": {"bound": "hbm", "achieved": round(gbs, 1), "peak": HBM_PEAK_GBPS,
                                     "unit": "GB/s", "frac": round(gbs / HBM_PEAK_GBPS, 4), "bytes_per_elem": 6,
                                     "algo_bytes_per_launch": 6 * P,
                                     "moved_bytes_per_elem": 6 if spec else 10,
                                     # the form's own bytes (two-pass: both parents read twice)
                                     # over the time: its streaming rate against the same peak
                                     "moved_frac": round((6 if spec else 10) * P / (ms / 1e3) / 1e9 / HBM_PEAK_GBPS, 4),
                                     "traffic": _pmc_traffic(args, f"slerp_7b/{parents}"),
                                     "traffic_source": _pmc_traffic(args, f"slerp_7b/{parents}", with_note=True)[1]}}
    del v0, v1, out, plan
    _free_device()
    if args.ops_cpu_seconds > 0:
        torch.set_num_threads(host_cpu_share()["threads"])
        # the reference's numpy SLERP (oracle.slerp restates it op for op) over one whole
        # transformer block of the layout (layer 0: the attention projections, the three 67.9M-
        # element MLP matrices, the norms and biases — every tensor shape of the merge, the large
        # ones dominating as in the 7B body), far parents (the SLERP branch)
        shapes, names = _block_sample(lay, 300_000_000)
        sizes = [int(torch.Size(shp).numel()) for shp in shapes]
        total = sum(sizes)
        gc = torch.Generator().manual_seed(5)
        a = [(torch.randn(m, generator=gc) * 0.02) for m in sizes]
        b = [(x + torch.randn(x.numel(), generator=gc) * 1e-3) for x in a]
        tm, reps = _median_time(lambda: [oracle.slerp(0.5, x, y) for x, y in zip(a, b)], args.ops_cpu_seconds)
        del a, b
        res["cpu_baseline"] = {"value": round(6 * total / tm / 1e9, 3), "unit": "GB/s (algorithmic bytes, bf16-sized)",
                               "cores": torch.get_num_threads(), "kind": "port",
                               "sample": f"{len(sizes)} tensors of qwen2p5_7b_body layer 0 ({names[0]} .. {names[-1]}, "
                                         f"{total} elements, largest {max(sizes)}), EDT_RL/crossover.py:11-43's numpy "
                                         f"SLERP (oracle.slerp), median of {reps} reps"}
    return res


def bench_population(args, rt, comm, kernels=None, layout_name="qwen2p5_7b_body"):
    """BASELINE configs[4] at N > 1: a population of N members (one 7.07B bf16 body per GPU,
    qwen2p5_7b_body) SLERP-crossed into N children (far parents: the SLERP branch), the N pairs
    drawn by EDT_RL/edt.py:231-240's roulette_wheel_selection (schedule.roulette_generation_pairs,
    the same seeded draw on every rank) and t per key from EDT_RL/crossover.py:146-147's layer
    curves (merge.rl_t_per_segment), timed link-balanced (distributed.ShardedPopulationCrossover:
    chunk-range shards of every member, the needed sums' table rows all-gathered, children gathered
    back), the same with its exchanges pipelined over chunk groups (`sharded_pipelined`), and per
    child (PopulationCrossover: each child's two parents shipped whole). Max over ranks; every rank
    of `comm` takes part. `kernels`: the product ops (default) or a host stand-in (the CPU
    rehearsal)."""
    from evolutionarydistributedtraining_amd.distributed import PopulationCrossover, ShardedPopulationCrossover
    from evolutionarydistributedtraining_amd.layouts import LAYOUTS
    from evolutionarydistributedtraining_amd.merge import rl_t_per_segment
    from evolutionarydistributedtraining_amd.schedule import roulette_generation_pairs
    lay = LAYOUTS[layout_name]()
    rank, world, dev = comm.rank, comm.world, rt.dev
    P, bf = lay.total, torch.bfloat16
    def member_seed(x, m):                  # member m, from its own seed (any rank can rebuild it)
        g = torch.Generator(device=dev).manual_seed(100 + m)
        for s0 in range(0, P, 1 << 28):
            e = min(P, s0 + (1 << 28))
            x[s0:e] = (torch.randn(e - s0, generator=g, device=dev) * 0.02).to(bf)
    member = torch.empty(P, dtype=bf, device=dev)
    member_seed(member, rank)
    out = torch.empty(P, dtype=bf, device=dev)
    ts = rl_t_per_segment(lay.names) if len(lay.names) == len(lay) else [0.5] * len(lay)   # unnamed: the global t
    t = torch.tensor(ts, dtype=torch.float64, device=dev)
    seed = getattr(args, "population_seed", 2025)
    pairs = [tuple(p) for p in roulette_generation_pairs(world, 1, seed=seed)[0]["pairs"]] if world > 1 else [(0, 0)]
    res = {"workload": f"SLERP population of {world} x {layout_name} (P={P}, bf16), one member per GPU",
           "pairs": [list(p) for p in pairs],
           "pairs_source": f"schedule.roulette_generation_pairs({world}, 1, seed={seed}): EDT_RL/edt.py:231-240 "
                           f"roulette_wheel_selection, n = {world} pairs",
           "t_source": "merge.rl_t_per_segment: EDT_RL/crossover.py:146-147 layer curves, global 0.5"}

    def timed(step, n):
        for _ in range(2):
            step()
        rt.sync()
        comm.barrier()
        t0 = time.perf_counter()
        for _ in range(n):
            step()
        rt.sync()
        comm.barrier()
        return max(comm.all_gather_object((time.perf_counter() - t0) / n * 1e3))
    wire = 2 * (world - 1) * (P * 2 // world)            # members out + children out, per rank
    peak = XGMI_LINK_GBPS * (world - 1)
    for key, groups in (("sharded", 1), ("sharded_pipelined", args.population_groups)):
        if groups < 1 or (key == "sharded_pipelined" and groups == 1):
            continue
        sp = ShardedPopulationCrossover(lay, bf, dev, kind="slerp", comm=comm, groups=groups, kernels=kernels)
        ms = timed(lambda: sp.slerp_step(member, pairs, t, out), max(3, args.steps // 4))
        if "sums_table" not in res:
            tab = (kernels or sp.kernels).needed_table(pairs, world, sp.plan.nchunks)
            res["sums_table"] = {"sums_per_chunk": sum(nt for _, nt in tab.blocks), "blocks": len(tab.blocks),
                                 "triangle_sums_per_chunk": world * (world + 1) // 2,   # every pair's dot
                                 "gathered_bytes_per_rank": tab.doubles * 8 * (world - 1) // world}
        res[key] = {"ms": round(ms, 3), "groups": groups, "wire_bytes_per_rank": wire,
                    "xgmi_floor_ms": xgmi_floor_ms(wire, world),
                    "xgmi": {"achieved": round(wire / (ms / 1e3) / 1e9, 1), "peak": peak, "unit": "GB/s",
                             "frac": round(wire / (ms / 1e3) / 1e9 / peak, 4) if peak else None}}
        del sp
        rt.empty_cache()
        rec = population_parity(lay, rt, comm, kernels, member_seed, pairs, t, out)
        if rec is not None:
            res[key]["parity"] = rec
        comm.barrier()
    pc = PopulationCrossover(lay, bf, dev, comm=comm, kernels=kernels)
    res["per_child"] = {"ms": round(timed(lambda: pc.slerp_step(member, pairs, t, out), 3), 3)}
    del pc, member, out
    rt.empty_cache()
    return res


def bench_population_resident(args, dev, layout_name="qwen2p5_7b_body", members_n=8):
    """BASELINE configs[4] on ONE GPU: a population of 8 members (7.07B bf16 bodies, one lineage)
    SLERP-crossed into 8 children per generation, every buffer resident in HBM (16 x 14.1 GB =
    226 GB), the generation as the RL master runs it: the pairs drawn by EDT_RL/edt.py:231-240's
    roulette_wheel_selection (schedule.roulette_generation_pairs: n = 8 pairs, random fitness, scale
    0.1 / 1.0 / 2.5 across the drawn generations as roulette_scale spans a run) and t per key from
    EDT_RL/crossover.py:146-147's layer curves routed as :108-122 routes them (merge.rl_t_per_segment,
    28 layers) — EDT_RL/edt.py:286-299 -> EDT_RL/crossover.py:84-135 per child. Each drawn generation
    runs ops.slerp_population in both forms, `--population-reps` (>= 10) timed calls each:
    `speculative` (the needed-sums member-major pass that writes every child's lerp-branch output +
    the redo blend; members of one lineage: every segment in the lerp branch) and `two_pass` (the
    needed-sums stats pass + the member-major blend). `floor_bytes`: the form's least HBM bytes
    (each distinct parent read once per pass, each child written once); `algo_bytes`: the
    generation's (every member once, every child once). The headline `speculative` / `two_pass`
    are the drawn generations together (sum of floor bytes over sum of times); `ring` is the ring
    of children (c, c + 1 mod 8) of r4's bench, kept as a labelled second case. Skipped with a
    reason when the HBM left after the other extras cannot hold it."""
    from evolutionarydistributedtraining_amd import ops
    from evolutionarydistributedtraining_amd.layouts import LAYOUTS
    from evolutionarydistributedtraining_amd.merge import rl_t_per_segment
    from evolutionarydistributedtraining_amd.schedule import roulette_generation_pairs
    lay = LAYOUTS[layout_name]()
    P, bf, M = lay.total, torch.bfloat16, members_n
    need = 2 * M * P * 2
    _free_device()                      # blocks the earlier extras left cached count as free
    free, _ = torch.cuda.mem_get_info(dev)
    res = {"workload": f"SLERP population of {M} x {layout_name} (P={P}, bf16), all resident on one GPU, "
                       f"pairs by EDT_RL's roulette selection, t by its layer curves",
           "kernel": "edt_slerp_population_speculative / edt_slerp_population (slerp_need_kernel)"}
    if free < need + (6 << 30):
        res["skipped"] = f"needs {need / 1e9:.0f} GB of HBM, {free / 1e9:.0f} GB free"
        return res
    members = [torch.empty(P, dtype=bf, device=dev) for _ in range(M)]
    outs = [torch.empty(P, dtype=bf, device=dev) for _ in range(M)]
    g = torch.Generator(device=dev).manual_seed(12)
    step = 1 << 27
    for s0 in range(0, P, step):                  # one lineage: a base + 0.5 % per member
        e = min(P, s0 + step)
        x = torch.randn(e - s0, generator=g, device=dev) * 0.02
        for m in members:
            m[s0:e] = (x + torch.randn(e - s0, generator=g, device=dev) * (0.02 * 0.005)).to(bf)
        del x
    plan = ops.make_slerp_plan(lay.offsets, dev)
    t = torch.tensor(rl_t_per_segment(lay.names), dtype=torch.float64, device=dev)
    reps = max(10, args.population_reps)
    algo = 2 * M * P * 2

    def generation(pairs):
        D = len({x for p in pairs for x in p})
        rec = {"pairs": [list(p) for p in pairs], "distinct_parents": D,
               "layout": ops.population_layout(pairs, M, True)}
        for form, spec, floor in (("speculative", True, 2 * P * (D + M)), ("two_pass", False, 2 * P * (2 * D + M))):
            ms = _event_ms(lambda: ops.slerp_population(plan, members, pairs, outs, t, speculate=spec), reps, 1)
            rec[form] = {"ms": round(ms, 3), "floor_bytes": floor, "algo_bytes": algo,
                         "floor_GBps": round(floor / (ms / 1e3) / 1e9, 1)}
        dots = getattr(plan, "_pop_dots", None)
        if dots is not None:
            rec["lerp_branch_fraction"] = round(float((dots.float().abs() > 0.9995).float().mean()), 4)
        return rec

    gens = roulette_generation_pairs(M, args.population_generations, seed=args.population_seed)
    drawn = []
    for gdef in gens:
        rec = generation([tuple(p) for p in gdef["pairs"]])
        rec["scale"] = gdef["scale"]
        drawn.append(rec)
    res["pairs_source"] = (f"schedule.roulette_generation_pairs(8, {args.population_generations}, "
                           f"seed={args.population_seed}): EDT_RL/edt.py:231-240 roulette_wheel_selection, "
                           f"n = 8 pairs, scales {sorted({r['scale'] for r in drawn})}")
    res["t_source"] = "merge.rl_t_per_segment: EDT_RL/crossover.py:146-147 layer curves, global 0.5"
    res["timed_reps"] = reps
    res["generations"] = drawn
    for form in ("speculative", "two_pass"):
        fb = sum(r[form]["floor_bytes"] for r in drawn)
        ms = sum(r[form]["ms"] for r in drawn)
        ab = algo * len(drawn)
        key = f"population_7b/roulette/{form}"
        traffic, note = (_pmc_traffic(args, key, with_note=True)
                         if layout_name == "qwen2p5_7b_body" else (None, "PMC entries are for the 7B body"))
        res[form] = {"ms_per_generation": round(ms / len(drawn), 3), "floor_bytes_per_generation": fb // len(drawn),
                     "algo_bytes": algo,
                     "roofline": {"bound": "hbm", "achieved": round(fb / (ms / 1e3) / 1e9, 1),
                                  "peak": HBM_PEAK_GBPS, "unit": "GB/s",
                                  "frac": round(fb / (ms / 1e3) / 1e9 / HBM_PEAK_GBPS, 4),
                                  "algo_frac": round(ab / (ms / 1e3) / 1e9 / HBM_PEAK_GBPS, 4),
                                  "traffic_per_generation": traffic, "traffic_source": note}}
    ring = generation([(c, (c + 1) % M) for c in range(M)])
    ring["note"] = "the ring of children (c, c + 1 mod 8): r4's bench pairs, which roulette selection rarely draws"
    if layout_name == "qwen2p5_7b_body":
        for form in ("speculative", "two_pass"):
            ring[form]["traffic"], ring[form]["traffic_source"] = _pmc_traffic(args, f"population_7b/ring/{form}",
                                                                               with_note=True)
    res["ring"] = ring
    del members, outs
    _free_device()
    return res


def stream_ceiling_ms(theta, workers, momentum, iters=10):
    """Median HIP-event time of edt_probe_stream over the step's own operands (None if the
    step runs without momentum: the probe always reads and writes a momentum stream)."""
    if momentum is None or len(workers) > 64:    # the probe is one launch (<= 64 workers)
        return None
    from evolutionarydistributedtraining_amd import _lib as L
    lib = L.lib()
    arr = L.ptr_array(workers)
    st = L.stream_ptr(theta.device)
    call = lambda: L.check(lib.edt_probe_stream(L.ptr(theta), L.dtype_code(theta), arr, L.dtype_code(workers[0]),
                                                len(workers), L.ptr(momentum), theta.numel(), st), "edt_probe_stream")
    call()
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(iters)]
    for a, b in ev:
        a.record()
        call()
        b.record()
    torch.cuda.synchronize()
    ts = sorted(a.elapsed_time(b) for a, b in ev)
    return ts[len(ts) // 2]


def time_sharded(args, layout, tdt, wdt, k_local, rt, comm, kernels, steps, warmup, mode=None, broadcast=None):
    """Build a ShardedOuterSync with k_local workers per rank, warm it up and time `steps` steps
    (barrier + synchronize on both sides, max over ranks). Returns (ms_per_step, mode/broadcast,
    wire bytes per rank); frees the arenas."""
    from evolutionarydistributedtraining_amd.distributed import ShardedOuterSync
    sync = ShardedOuterSync(layout, tdt, wdt, k_local, rt.dev, args.lr, args.momentum, bool(args.nesterov),
                            mode=mode or args.mode, bucket_elems=args.bucket_elems,
                            broadcast=broadcast or args.broadcast, comm=comm, kernels=kernels)
    synth_sharded(sync.theta.flat, [w.flat for w in sync.workers], comm.rank)
    for _ in range(warmup):
        sync.step()
    rt.sync()
    comm.barrier()
    rt.sync()
    t0 = time.perf_counter()
    for _ in range(steps):
        sync.step()
    rt.sync()
    comm.barrier()
    elapsed = max(comm.all_gather_object(time.perf_counter() - t0))
    res = (elapsed / steps * 1e3, f"{sync.mode}/{sync.broadcast}", sync.wire_bytes())
    del sync
    rt.empty_cache()
    return res


def run_sharded(args, comm, rt, json_out, kernels=None, exit_fn=None) -> dict | None:
    """The N > 1 line (and `--gpus 1 --sharded`): the sharded outer step over `comm`, timed; the
    line built on rank 0 (value, local-kernel HBM roofline + the xGMI figure, the CPU baseline);
    then the extras under the deadline (weak companion, other schedules, BASELINE configs[2]/[3],
    configs[4]'s population); rank 0 prints ONE line. `comm`: the collectives.Collectives seam
    (RCCL here; gloo in tests/test_bench_rehearsal.py), `rt`: Runtime, `kernels`: the product ops
    (None) or a host stand-in. Returns rank 0's line."""
    from evolutionarydistributedtraining_amd.distributed import ShardedOuterSync
    from evolutionarydistributedtraining_amd.layouts import LAYOUTS
    rank, world = comm.rank, comm.world
    layout = LAYOUTS[args.layout]()
    tdt, wdt = DT[args.theta_dtype], DT[args.worker_dtype]
    if args.workers_per_gpu:
        k_local, scaling = args.workers_per_gpu, "weak"
    else:
        if args.population % world:
            raise SystemExit(f"population {args.population} does not split over {world} GPUs")
        k_local, scaling = args.population // world, "strong"
    k_total = k_local * world
    P = layout.total
    sync = ShardedOuterSync(layout, tdt, wdt, k_local, rt.dev, args.lr, args.momentum, bool(args.nesterov),
                            mode=args.mode, bucket_elems=args.bucket_elems, broadcast=args.broadcast,
                            comm=comm, kernels=kernels)
    sync.event_factory = rt.event
    synth_sharded(sync.theta.flat, [w.flat for w in sync.workers], rank)
    kernel_name = {"exact": "outer_kernel (fused, owned shards)",
                   "reduce": "outer_kernel(partial) + sgd_apply_kernel",
                   "reduce_ordered": "outer_kernel(partial) + sgd_apply_sum_kernel"}[sync.mode]
    for _ in range(args.warmup):
        sync.step()
    rt.sync()
    sync.kernel_events = []          # every local kernel of the schedule, bracketed inside the step
    comm.barrier()
    rt.sync()
    t0 = time.perf_counter()
    for _ in range(args.steps):
        sync.step()
    rt.sync()
    comm.barrier()
    elapsed = max(comm.all_gather_object(time.perf_counter() - t0))
    ms_per_step = elapsed / args.steps * 1e3
    kern_ms = max(comm.all_gather_object(sum(a.elapsed_time(b) for a, b in sync.kernel_events) / args.steps))
    kern_bytes = sync.kernel_bytes()
    sync.kernel_events = None
    bytes_reduced = k_total * P * torch.finfo(wdt).bits // 8
    value = bytes_reduced / (ms_per_step / 1e3) / 1e9
    sched = f"{sync.mode}/{sync.broadcast}"
    wire_main = sync.wire_bytes()
    dumped = None
    if args.dump_outputs:
        # what the last timed step left its caller: the new theta (every rank gathers, rank 0 writes)
        th = sync.gather_theta()[:P]
        rt.sync()
        if rank == 0:
            dumped = dump_outputs(args.dump_outputs, {"theta": th})
        del th
        comm.barrier()

    out = None
    if rank == 0:
        # the rank's local kernels (HIP events inside the step, slowest rank) against HBM ...
        achieved = kern_bytes / (kern_ms / 1e3) / 1e9
        roofline = {"bound": "hbm", "achieved": round(achieved, 1), "peak": HBM_PEAK_GBPS, "unit": "GB/s",
                    "frac": round(achieved / HBM_PEAK_GBPS, 4), "traffic": None,
                    "traffic_note": "no PMC collection on the multi-GPU path",
                    "kernel": kernel_name, "kernel_ms": round(kern_ms, 4),
                    "algo_bytes_per_launch": kern_bytes, "schedule": sched,
                    "note": "local kernels per rank and step (all buckets); the step itself is "
                            "bounded by the xGMI exchange below"}
        # ... and the exchange: bytes this rank puts on xGMI per step over the whole step time,
        # against the outbound direction of the rank's links to its N-1 peers
        xa = wire_main / (ms_per_step / 1e3) / 1e9
        peak = XGMI_LINK_GBPS * (world - 1)
        roofline["xgmi"] = {"bound": "xgmi", "achieved": round(xa, 1), "peak": peak, "unit": "GB/s",
                            "frac": round(xa / peak, 4) if peak else None, "wire_bytes_per_rank": wire_main,
                            "floor_ms": xgmi_floor_ms(wire_main, world)}
        out = {
            "metric": "GB/s of param bytes reduced per outer step (device-resident), 1/2/4/8 GPUs",
            "value": round(value, 2), "unit": "GB/s", "n_gpus": world, "steps": args.steps,
            "warmup": args.warmup, "ms_per_step": round(ms_per_step, 4), "higher_is_better": True,
            "scaling": scaling, "vs_baseline": None, "dtype": "f32" if tdt == torch.float32 else "bf16",
            "data": "synthetic (theta ~ N(0,.02^2) from one seed on every rank, worker = theta + N(0,1e-3^2) "
                    "from a per-rank seed, on device)",
            "config": {"workload": f"DiLoCo outer step, {args.layout} P={P} T={len(layout)}, "
                                   f"population {k_total} ({k_local} {args.worker_dtype} workers resident per GPU), "
                                   f"{args.theta_dtype} theta+momentum, lr {args.lr} mu {args.momentum} "
                                   f"nesterov {bool(args.nesterov)}",
                       "params": P, "tensors": len(layout), "workers_per_gpu": k_local,
                       "population": k_total, "worker_dtype": args.worker_dtype,
                       "theta_dtype": args.theta_dtype, "parallelism": f"dp{world} {sched} (RCCL)"},
            "roofline": roofline,
            "device": rt.device_info(), "native": native_library_record(),
        }
        if dumped:
            out["dumped_outputs"] = dumped
        # rank 0 times the CPU baseline first (the other ranks wait at the barrier), then every
        # extra runs under the deadline, so neither can be lost to a hang in an extra
        if args.cpu_baseline_seconds > 0:
            try:
                out["cpu_baseline"] = cpu_baseline(args, tdt, wdt, k_total)
            except Exception as e:     # the value is measured: report the failure, keep the line
                out["cpu_baseline"] = {"error": f"{type(e).__name__}: {str(e)[:200]}"}
    comm.barrier()
    deadline = ExtrasDeadline(args.extras_deadline, rank, out, json_out, exit_fn=exit_fn,
                              detail_out=getattr(args, "detail_out", None))
    if args.kernel_trace > 0 and kernels is None:
        # first extra: every rank runs the traced steps (they hold the step's collectives)
        try:
            trace = kernel_trace(sync.step, args.kernel_trace)
        except Exception as e:          # evidence, not the measurement: report it, keep the line
            trace = {"error": f"{type(e).__name__}: {str(e)[:300]}"}
        if out is not None:
            out["kernel_trace"] = trace
        comm.barrier()
    mode_used, bcast_used = sync.mode, sync.broadcast
    sync = None
    rt.empty_cache()
    if args.parity_layout:
        # the exchange's correctness, first of the extras: the timed schedule on a small layout,
        # gathered and compared on rank 0 with the single-GPU kernels
        try:
            par = sharded_parity(args, comm, rt, kernels, mode_used, bcast_used, k_local, tdt, wdt)
        except Exception as e:     # an extra after the value: report it, keep the line
            par = {"error": f"{type(e).__name__}: {str(e)[:200]}"}
            rt.empty_cache()
        if out is not None:
            out["parity"] = par
        comm.barrier()
    if scaling == "strong" and args.weak_companion:     # (world 1: --sharded rehearsal)
        # the same schedule with the N = 1 population on EVERY rank (population x N): per-GPU
        # work fixed, so value_N / (N value_1) isolates the cost of the xGMI exchange
        try:
            w_ms, w_sched, w_wire = time_sharded(args, layout, tdt, wdt, args.population, rt, comm, kernels,
                                                 args.steps, args.warmup)
            w_bytes = args.population * world * P * torch.finfo(wdt).bits // 8
            weak = {"workers_per_gpu": args.population, "population": args.population * world,
                    "ms_per_step": round(w_ms, 4), "value": round(w_bytes / (w_ms / 1e3) / 1e9, 2),
                    "unit": "GB/s", "schedule": w_sched, "wire_bytes_per_rank": w_wire,
                    "xgmi_floor_ms": xgmi_floor_ms(w_wire, world),
                    "note": "companion measurement after the timed strong-scaling steps; not the value"}
        except Exception as e:     # the value is already measured: report, go on
            weak = {"error": f"{type(e).__name__}: {str(e)[:200]}"}
            rt.empty_cache()
        if out is not None:
            out["weak_scaling"] = weak
    if args.compare_schedules:
        # every schedule the strong-scaling population can run, same steps, after the value: the
        # data to tune mode="auto" on this node (outside the reported value)
        schedules = {}
        for m, b in (("exact", "workers"), ("exact", "theta"), ("reduce_ordered", "theta"), ("reduce", "theta")):
            if f"{m}/{b}" == sched:
                continue
            try:
                ms_, name, wire_ = time_sharded(args, layout, tdt, wdt, k_local, rt, comm, kernels, args.steps,
                                                args.warmup, mode=m, broadcast=b)
                schedules[name] = {"ms_per_step": round(ms_, 4), "wire_bytes_per_rank": wire_,
                                   "xgmi_floor_ms": xgmi_floor_ms(wire_, world),
                                   "value": round(bytes_reduced / (ms_ / 1e3) / 1e9, 2)}
            except Exception as e:     # an extra after the value: report it, keep the line
                schedules[f"{m}/{b}"] = {"error": f"{type(e).__name__}: {str(e)[:200]}"}
                rt.empty_cache()
        if out is not None:
            out["other_schedules"] = schedules
    if args.config_companions:
        # BASELINE's other multi-GPU DiLoCo configs on the same node, after the value: configs[2]
        # (125M, 8 workers = 8 GPUs, fp32 as the reference computes) and configs[3] (1.3B, 8
        # workers over the GPUs, bf16 params); same population split, the schedule auto picks
        configs = {}
        for item in args.config_layouts.split(","):
            key, spec = item.split("=")
            lname, cname = spec.split(":")
            cdt = DT[cname]
            try:
                lay_c = LAYOUTS[lname]()
                ms_, name, wire_ = time_sharded(args, lay_c, cdt, cdt, k_local, rt, comm, kernels, args.steps,
                                                args.warmup)
                b_c = k_total * lay_c.total * torch.finfo(cdt).bits // 8
                configs[key] = {"layout": lname, "params": lay_c.total, "dtype": cname,
                                "population": k_total, "workers_per_gpu": k_local, "schedule": name,
                                "ms_per_step": round(ms_, 4), "value": round(b_c / (ms_ / 1e3) / 1e9, 2),
                                "unit": "GB/s", "wire_bytes_per_rank": wire_,
                                "xgmi_floor_ms": xgmi_floor_ms(wire_, world)}
            except Exception as e:     # an extra after the value: report it, keep the line
                configs[key] = {"error": f"{type(e).__name__}: {str(e)[:200]}"}
                rt.empty_cache()
        if out is not None:
            out["baseline_configs"] = configs
    if world > 1 and "population_7b" in args.ops:
        # configs[4] on the same node, after the DiLoCo measurements (every rank takes part)
        try:
            population = bench_population(args, rt, comm, kernels, layout_name=args.population_layout)
        except Exception as e:     # an extra after the value: report it, keep the line
            population = {"error": f"{type(e).__name__}: {str(e)[:200]}"}
            rt.empty_cache()
        if out is not None:
            out["population_slerp_7b"] = population
    deadline.emit()
    comm.barrier()          # still under the deadline: a rank stuck in an extra cannot hang the exit
    deadline.cancel()
    return out


def main():
    args = parse()
    if "WORLD_SIZE" not in os.environ and args.gpus > 1:
        sys.exit(launch_ranks(args.gpus))       # this process never touches the GPU
    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local = int(os.environ.get("LOCAL_RANK", "0"))
    if world != args.gpus:
        raise SystemExit(f"--gpus {args.gpus} but WORLD_SIZE={world}")
    if args.dry_run_launch:
        print(json.dumps({**{k: os.environ.get(k) for k in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_ADDR",
                                                             "MASTER_PORT")}, "PID": os.getpid()}), flush=True)
        time.sleep(args.dry_run_sleep)
        return
    # stdout carries exactly one JSON line (rank 0): everything else the libraries print on fd 1
    # (RCCL's version banner at communicator init, ROCm notices) is sent to stderr
    json_out = os.fdopen(os.dup(1), "w")
    sys.stdout.flush()
    os.dup2(2, 1)
    sharded = world > 1 or args.sharded    # --sharded: the multi-GPU code path on one rank
    if sharded and "MASTER_ADDR" not in os.environ:      # --gpus 1 --sharded without torchrun
        os.environ.update(RANK="0", LOCAL_RANK="0", WORLD_SIZE="1", MASTER_ADDR="127.0.0.1",
                          MASTER_PORT=str(_free_port()))
    torch.cuda.set_device(local)
    dev = torch.device("cuda", local)
    rt = Runtime(dev)
    if sharded:
        import torch.distributed as dist
        from evolutionarydistributedtraining_amd.collectives import TorchCollectives, init_torch
        init_torch("nccl", device_id=dev)
        run_sharded(args, TorchCollectives(), rt, json_out)
        dist.destroy_process_group()
        return

    from evolutionarydistributedtraining_amd.layouts import LAYOUTS
    from evolutionarydistributedtraining_amd.diloco import OuterSync
    from evolutionarydistributedtraining_amd.params import ParamArena

    layout = LAYOUTS[args.layout]()
    tdt, wdt = DT[args.theta_dtype], DT[args.worker_dtype]
    k_local = args.workers_per_gpu or args.population
    scaling = "weak" if args.workers_per_gpu else "strong"
    k_total = k_local
    P = layout.total
    theta = ParamArena(layout, tdt, dev)
    workers = [ParamArena(layout, wdt, dev) for _ in range(k_local)]
    synth_population(theta.flat, [w.flat for w in workers], seed=1234)
    sync = OuterSync(theta, workers, args.lr, args.momentum, bool(args.nesterov))
    step = sync.step
    kernel_name = "outer_kernel"

    for _ in range(args.warmup):
        step()
    torch.cuda.synchronize()
    placement = None
    # --full: the fused step on the first allocation, before any placement search: what the drop-in
    # list path and any first-allocation user get, reported beside the placed value
    unplaced_ms = _event_ms(step, 5, 0) if args.full else None
    if args.place_candidates > 1:
        # once per run, outside the timed region: the operand set goes wherever the step's access
        # pattern runs fastest — `--place-draws` regions of HBM for theta and the workers, the
        # momentum placed inside each (placement.place_set); every later step uses that placement
        try:
            placement = sync.place_arenas(args.place_draws, args.place_candidates)
        except Exception as e:          # a measurement extra: report it, keep the first allocation
            placement = {"error": f"{type(e).__name__}: {e}"}
        step()
        torch.cuda.synchronize()

    # fused-kernel duration, measured with HIP events on the launch stream (torch's current)
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(args.steps)]
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for i in range(args.steps):
        ev[i][0].record()
        step()
        ev[i][1].record()
    torch.cuda.synchronize()
    elapsed = time.perf_counter() - t0
    ms_per_step = elapsed / args.steps * 1e3
    ks = sorted(a.elapsed_time(b) for a, b in ev)
    kern_ms = sum(ks) / len(ks)

    bytes_reduced = k_total * P * torch.finfo(wdt).bits // 8
    value = bytes_reduced / (ms_per_step / 1e3) / 1e9
    if rank != 0:
        return
    dumped = None
    if args.dump_outputs:
        # what the last timed step left its caller: the step updates theta and the momentum in place
        arrays = {"theta": sync.theta.flat}
        if sync.state.momentum is not None:
            arrays["momentum"] = sync.state.momentum
        dumped = dump_outputs(args.dump_outputs, arrays)
    bg = torch.finfo(tdt).bits // 8
    bw = torch.finfo(wdt).bits // 8
    per_elem = k_local * bw + 2 * bg + (2 * bg if args.momentum else 0)
    algo_bytes = per_elem * P                       # one launch, steady state (carried buffer)
    achieved = algo_bytes / (kern_ms / 1e3) / 1e9
    traffic, traffic_note = _pmc_traffic(args, f"{args.layout}/K{k_local}/{args.theta_dtype}-{args.worker_dtype}",
                                         with_note=True)
    roofline = {"bound": "hbm", "achieved": round(achieved, 1), "peak": HBM_PEAK_GBPS,
                "unit": "GB/s", "frac": round(achieved / HBM_PEAK_GBPS, 4), "traffic": traffic,
                "traffic_source": traffic_note,
                "kernel": kernel_name, "kernel_ms": round(kern_ms, 4),
                "bytes_per_elem": per_elem, "algo_bytes_per_launch": algo_bytes}
    out = {
        "metric": "GB/s of param bytes reduced per outer step (device-resident), 1/2/4/8 GPUs",
        "value": round(value, 2), "unit": "GB/s", "n_gpus": world, "steps": args.steps,
        "warmup": args.warmup, "ms_per_step": round(ms_per_step, 4), "higher_is_better": True,
        "scaling": scaling, "vs_baseline": None, "dtype": "f32" if tdt == torch.float32 else "bf16",
        "data": "synthetic (theta ~ N(0,.02^2), worker = theta + N(0,1e-3^2), seeded on device)",
        "config": {"workload": f"DiLoCo outer step, {args.layout} P={P} T={len(layout)}, "
                               f"population {k_total} ({k_local} {args.worker_dtype} workers resident per GPU), "
                               f"{args.theta_dtype} theta+momentum, lr {args.lr} mu {args.momentum} "
                               f"nesterov {bool(args.nesterov)}",
                   "params": P, "tensors": len(layout), "workers_per_gpu": k_local,
                   "population": k_total, "worker_dtype": args.worker_dtype,
                   "theta_dtype": args.theta_dtype, "parallelism": "single GPU"},
        "roofline": roofline,
        "device": rt.device_info(), "native": native_library_record(),
    }
    if dumped:
        out["dumped_outputs"] = dumped
    if placement:
        roofline["placement"] = _placement_record(placement)
        if "momentum" in placement:
            roofline["momentum_placement"] = placement["momentum"]
    if not args.full:
        emit_line(out, json_out, args.detail_out)
        return

    # everything below is --full: measurements and checks beside the value, each a run of its own
    # what a plain device-to-device copy reaches on this device, same process
    src = torch.empty(1 << 29, dtype=torch.float32, device=dev)
    dst = torch.empty_like(src)
    dst.copy_(src)
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(5):
        dst.copy_(src)
    b.record()
    torch.cuda.synchronize()
    roofline["device_copy_GBps"] = round(5 * 2 * src.numel() * 4 / (a.elapsed_time(b) / 1e3) / 1e9, 1)
    del src, dst
    # the step's own access pattern with a trivial body (edt_probe_stream), same arenas:
    # the memory-system ceiling of this step on this device, measured after the timed steps
    try:
        probe_ms = stream_ceiling_ms(theta.flat, [w.flat for w in workers], sync.state.momentum)
    except Exception as e:      # a measurement extra: the JSON line still prints
        probe_ms = None
        roofline["stream_ceiling_error"] = f"{type(e).__name__}: {e}"
    if probe_ms:
        ceil = algo_bytes / (probe_ms / 1e3) / 1e9
        roofline["stream_ceiling_GBps"] = round(ceil, 1)
        roofline["frac_of_stream_ceiling"] = round(roofline["achieved"] / ceil, 4)
    roofline["unplaced_ms"] = round(unplaced_ms, 4)
    roofline["unplaced_frac"] = round(algo_bytes / (unplaced_ms / 1e3) / 1e9 / HBM_PEAK_GBPS, 4)
    roofline["unplaced_note"] = ("the fused step (HIP events, 5 launches) on the operands' first allocation, "
                                 "before the placement search; kernel_ms is after it")
    if args.kernel_trace > 0:
        try:
            out["kernel_trace"] = kernel_trace(step, args.kernel_trace)
        except Exception as e:          # evidence, not the measurement: report it, keep the line
            out["kernel_trace"] = {"error": f"{type(e).__name__}: {str(e)[:300]}"}
    if args.bcast_compare:
        # the step with the broadcast of diloco.py:302-308 (every worker restarts from theta):
        # fused into the kernel's pass vs the step + K device copies
        try:
            fused = _event_ms(lambda: sync.step(broadcast=True), args.steps, 2)
            unfused = _event_ms(lambda: (sync.step(), sync.broadcast_()), args.steps, 2)
            fb = algo_bytes + k_local * P * (torch.finfo(wdt).bits // 8)
            out["step_with_broadcast"] = {
                "fused_ms": round(fused, 4), "step_plus_copies_ms": round(unfused, 4),
                "kernel": "outer_kernel<..., BC=true> (edt_outer_step_bcast)",
                "fused_roofline": {"bound": "hbm", "achieved": round(fb / (fused / 1e3) / 1e9, 1),
                                   "peak": HBM_PEAK_GBPS, "unit": "GB/s",
                                   "frac": round(fb / (fused / 1e3) / 1e9 / HBM_PEAK_GBPS, 4),
                                   "algo_bytes_per_launch": fb}}
        except Exception as e:          # an extra: report it, keep the line
            out["step_with_broadcast"] = {"error": f"{type(e).__name__}: {str(e)[:300]}"}
    if args.ops and args.ops != "none":
        # the other hot-path kernels, one GPU, after the outer step's arenas are freed
        sync.theta = sync.workers = sync.state = None
        theta = workers = sync = step = None
        _free_device()
        for name, fn in (("list_form", bench_list_form), ("configs1_125m", bench_config1),
                         ("pair_merge", bench_pair_merge), ("slerp_7b", bench_slerp_7b),
                         ("lm_population", bench_lm_population)):
            if name in args.ops:
                try:
                    out[name] = fn(args, dev)
                except Exception as e:          # an extra: report it, keep the line
                    out[name] = {"error": f"{type(e).__name__}: {str(e)[:300]}"}
                    _free_device()
        if "population_7b" in args.ops:          # last: it needs 226 GB of the HBM
            try:
                out["population_slerp_7b"] = bench_population_resident(args, dev, args.population_layout)
            except Exception as e:              # an extra: report it, keep the line
                out["population_slerp_7b"] = {"error": f"{type(e).__name__}: {str(e)[:300]}"}
                _free_device()
    if args.cpu_baseline_seconds > 0:
        # rank 0 after the GPU phase, on this host's cores: the whole population's step (the
        # reference's master runs all K workers' deltas on its CPU)
        out["cpu_baseline"] = cpu_baseline(args, tdt, wdt, k_total)
    emit_line(out, json_out, args.detail_out)


if __name__ == "__main__":
    main()
