"""DiLoCo outer step across GPUs: one process per GPU, RCCL over xGMI (torch.distributed "nccl").

The reference has no collectives: its "gather" is K x `from_pretrained` of the workers'
checkpoints on a shared disk and its "broadcast" is K x `save_pretrained` (EDT_LM/diloco.py:
231-235, 302-308). Here the population is resident in HBM across the node and the cross-replica
mean is a real exchange step. Three schedules and one opt-in fourth, all bucketed so RCCL traffic
on the comm stream overlaps the HBM-bound kernels on the compute stream:

  mode="reduce"          each rank fuses its local workers into an fp32 partial sum
                         (edt_delta_partial), reduce-scatter(sum, fp32) -> SGD on the owned shard
                         (momentum sharded 1/N, edt_sgd_apply) -> all-gather of theta. Wire bytes
                         per rank and step: (N-1)/N * P * (4 + b_g). The cross-rank sum is RCCL's
                         (its order depends on the algorithm RCCL picks); within DESIGN §3's bound of
                         the reference's sequential order.
  mode="reduce_ordered"  the same partials, an all-to-all of them instead of the reduce-scatter,
                         then edt_sgd_apply_sum: the owned shard's N partials summed in rank order
                         + SGD. Same wire bytes as reduce; one fixed summation order whatever RCCL
                         does (reproducible run to run, bit-exact with the oracle's split).
  mode="reduce_q"        opt-in, never chosen by "auto": reduce_ordered with the partials block-quantized
                         on the wire (wire_format="mxfp8" | "mxfp4": OCP MX blocks of 32 elements with
                         one E8M0 scale byte). edt_delta_partial_q forms the fp32 partial
                         in registers and writes only the packed regions [dest rank][payload | scales];
                         the all-to-all moves uint8; edt_sgd_apply_sum_q dequantizes the owned shard's
                         N regions, sums them in rank order and steps. Wire bytes: (N-1)/N * P *
                         (q + b_g), q = 1 + 1/32 (mxfp8) or 1/2 + 1/32 (mxfp4) — computed from the
                         byte counts, not measured on a multi-GPU node. error_feedback=True carries
                         each rank's quantization error into its next step (`residual`, fp32, per
                         rank: r = p' - D(Q(p')), p' = p + r_prev). Only with broadcast="theta".
    gather_format="mxfp8" | "mxfp4" (reduce_q only, opt-in) quantizes the other half of the
                         exchange: the owner runs edt_sgd_delta_sum_q instead — the same sum and SGD
                         update, the same momentum bits, but theta is left alone and the update
                         u = theta' - theta is written as one more packed region, straight into this
                         rank's slot of `u_recv` ([src rank][payload | scales]); a uint8 all-gather
                         replaces the all-gather of theta, and as each bucket lands
                         edt_apply_delta_q adds the dequantized updates to theta — the same kernel
                         on the same bytes on every rank, so the replicas stay bit-identical.
                         error_feedback also keeps `residual_g` (fp32, sharded like the momentum:
                         u' = u + r_g, r_g = u' - D(Q(u'))). Wire bytes: (N-1)/N * P * (q_in + q_out)
                         — 2.0625 B/elem with mxfp8 both ways whatever theta's dtype; computed from
                         the byte counts, not measured on a multi-GPU node.
    rounding="stochastic" (reduce_q only, opt-in, instead of error feedback) makes both encoders
                         round each element to one of its two grid neighbours with the probability
                         of its distance (Philox4x32-10 bits from `seed`, the step counter
                         `q_step`, a stream per rank and encoder, and the element's index in the
                         arena): unbiased in expectation, no residual buffers, no extra HBM bytes.
                         The decoders and the bytes' layout are unchanged.
  mode="exact"           all-to-all of the raw worker shards to their owners, then the single-GPU
                         fused kernel on each shard (the reference's worker order, bit-exact),
                         all-gather of theta. Wire bytes: (N-1)/N * P * (K_local * b_w + b_g).
  broadcast              what the all-gather delivers to every rank. "theta": the full master
                         replica (theta's dtype). "workers" (exact mode only): the new theta rounded
                         to the worker dtype, straight into every local worker arena — the start of
                         the next inner loop, which is all the reference ships to the workers
                         (diloco.py:302-308 saves the base to every worker dir; the bf16 workers load
                         it rounded). The fp32 master then stays sharded (`gather_theta()` assembles
                         it on demand, e.g. for a checkpoint). Wire bytes: (N-1)/N * P * (K_local + 1) * b_w.
  step(broadcast=True)   hands the new theta to the local workers in the step's own pass, for every
                         schedule that keeps the theta replica: when the step's work completes each
                         local worker arena over [0, n_pad) holds round_w(theta_new) (RNE, what
                         `w.copy_(theta)` leaves), and theta, the momentum, the residuals, the packed
                         buffers and q_step are bit-identical to step(). reduce_q with gather_format
                         fuses it into phase 3 (edt_apply_delta_q_bcast: the pass already holds the
                         new theta in registers, + K_local * b_w bytes per element); the others run
                         one edt_broadcast_theta per bucket as its all-gather lands (theta read
                         once, + b_g + K_local * b_w), overlapping the later buckets' gathers.
                         With broadcast="workers" the step already does it and the flag changes
                         nothing. NaN elements (a scale-255 block) are NaN in theta and in every
                         worker; their payload bits are not specified.
  guard=OuterGuard       (every schedule; opt-in) measures, screens and clips the step
                         across the ranks before theta is touched: every rank forms the
                         same float64 totals in one fixed order (its buckets and chunks in order, then
                         the ranks in rank order after an all_gather_object) and takes the same
                         guard.guard_decision. The reduce schedules screen the local workers before
                         the exchange (edt_delta_stats: S_kk and the non-finite counts) and measure
                         the mean on the owned shards after it (edt_partial_sum_stats), clipping with
                         edt_sgd_apply(_sum)_scaled; exact runs edt_delta_stats on the received slices
                         and clips with edt_outer_step_scaled. A refusal leaves theta, the momentum and
                         the worker arenas as they were on every rank, with every collective waited for.
                         reduce_q screens the same way before phase 1; a rank left without a worker
                         launches no phase 1, sends zero bytes (every block +0) and keeps its residual;
                         the mean is measured as it will be applied — the dequantized rank-ordered sum,
                         quantization error and residuals included (edt_partial_sum_stats_q) — and
                         clipped by edt_sgd_apply_sum_q_scaled / edt_sgd_delta_sum_q(_sr)_scaled. With
                         error feedback phase 1 writes the new residual into a second buffer
                         (edt_delta_partial_q_to; + 4 B per element of memory per rank, no extra
                         traffic) and the two are swapped only once the step is decided, so a refusal
                         also leaves `residual`, `residual_g` and `q_step` as they were.
  mode="auto" / broadcast="auto" (defaults) pick the combination with the fewest wire bytes,
  ties to exact, then reduce_ordered: at K = 8 bf16 workers, fp32 theta: N = 2 reduce_ordered/theta
  (8 B/elem), N = 4 and 8 exact/workers (6 and 4 B/elem); all fp32: N = 2 and 4 reduce_ordered,
  N = 8 exact.

Every rank holds 1/N of the momentum and owns contiguous shards of every bucket.
"""
from __future__ import annotations

import math
from typing import NamedTuple

import numpy as np
import torch

from . import ops as _ops
from ._lib import EdtError
from .collectives import Collectives, TorchCollectives
from .diloco import check_sgd_hparams
from .guard import (NonFiniteWorkers, OuterGuard, fold_remeasured, guard_decision, report, sequential_total,
                    totals_from_row)
from .params import ParamArena, ParamLayout
from .tracing import trange, traced


def _timing_event():
    return torch.cuda.Event(enable_timing=True)


_Q_BITS = {"mxfp8": 8, "mxfp4": 4}       # element bits of the reduce_q wire formats


class _Verdict(NamedTuple):
    """What the guard decided for one step, handed to the phases that act on it and kept nowhere."""
    local: list | None         # this rank's surviving local workers (None: all of them)
    divisor: int | None        # how many workers phase 1 divides by (None: k_total)
    survivors: list | None     # exact: the surviving global workers (None: all of them)
    clip: float                # the factor on the mean pseudo-gradient; 1.0: the plain entries


_NO_GUARD = _Verdict(None, None, None, 1.0)      # every worker, unclipped: what an unguarded step passes


class GuardKernelsMissing(EdtError, ValueError):
    """guard= with mode='reduce_q' on kernels that lack what that schedule's guard needs. Also a
    ValueError: before those kernels existed the constructor refused the combination with one."""


def _scaled(name: str) -> str:
    return name + "_scaled"


def _entry(name: str, clip: float):
    """The kernels' entry of a step and its trailing arguments: `name` itself at exactly 1.0, else
    its scaled form with the coefficient."""
    return (name, ()) if clip == 1.0 else (_scaled(name), (clip,))


class ShardedOuterSync:
    def __init__(self, layout: ParamLayout, theta_dtype: torch.dtype, worker_dtype: torch.dtype,
                 k_local: int, device, lr: float = 0.7, momentum: float = 0.9, nesterov: bool = True,
                 mode: str = "auto", bucket_elems: int = 1 << 26, group=None, kernels=None,
                 broadcast: str = "auto", comm: Collectives | None = None,
                 cpu_tails: tuple[int, int] | None = None, wire_format: str = "mxfp8",
                 error_feedback: bool = True, gather_format: str | None = None, rounding: str = "nearest",
                 seed: int = 0, guard=None):
        """guard: a guard.OuterGuard — every step is measured, screened and clipped across the ranks
        before theta is touched (`_guarded`, `last_stats`); None: nothing changes.
        mode="reduce_q": `wire_format` picks the element format of the quantized partials and
        `error_feedback` keeps `self.residual` — this rank's fp32 quantization error (n_pad
        elements), added to the next step's partial before it is quantized. The residual is per
        rank (each rank quantizes its own partial) and is not part of theta or the momentum: a
        restart without it loses at most one step's quantization error. `gather_format` (reduce_q
        only) ships the owners' quantized updates instead of theta (module docstring); with
        error_feedback it keeps `self.residual_g`, the owner's fp32 error of that quantization
        (sharded like the momentum), under the same restart rule. `rounding="stochastic"` (reduce_q
        with error_feedback=False only) rounds stochastically instead and keeps no residual: its
        whole state is `seed` and the public integer `q_step`, which starts at 0, numbers the
        current step's random bits and is incremented at the end of step(). q_step is settable: a
        restart that restores it (with theta, the momentum and the same seed) replays the same
        bits, so the run continues bit for bit."""
        if (mode not in ("reduce", "reduce_ordered", "reduce_q", "exact", "auto")
                or broadcast not in ("theta", "workers", "auto")):
            raise ValueError((mode, broadcast))
        if mode.startswith("reduce") and broadcast == "workers":
            raise ValueError("the reduce schedules need the full theta replica (broadcast='theta')")
        if mode == "reduce_q" and wire_format not in _Q_BITS:
            raise ValueError(f"wire_format {wire_format!r}: 'mxfp8' or 'mxfp4'")
        if gather_format is not None:
            if mode != "reduce_q":
                raise ValueError("gather_format quantizes the gather of mode='reduce_q' only")
            if gather_format not in _Q_BITS:
                raise ValueError(f"gather_format {gather_format!r}: None, 'mxfp8' or 'mxfp4'")
        if rounding not in ("nearest", "stochastic"):
            raise ValueError(f"rounding {rounding!r}: 'nearest' or 'stochastic'")
        if rounding == "stochastic":
            if mode != "reduce_q":
                raise ValueError(f"rounding='stochastic' needs mode='reduce_q' (the quantizing schedule), not mode={mode!r}")
            if error_feedback:
                raise ValueError("rounding='stochastic' needs error_feedback=False: it replaces the residual")
            if not 0 <= int(seed) < 1 << 64:
                raise ValueError(f"seed {seed!r}: an unsigned 64-bit integer")
        check_sgd_hparams(lr, momentum, nesterov)
        # the communicator seam: torch.distributed (RCCL / gloo) by default, or N virtual ranks
        # on one device (collectives.VirtualWorld)
        self.comm = comm or TorchCollectives(group)
        self.world = self.comm.world
        self.rank = self.comm.rank
        wb = torch.empty(0, dtype=worker_dtype).element_size()
        gb = torch.empty(0, dtype=theta_dtype).element_size()
        cands = {("reduce", "theta"): 4 + gb, ("reduce_ordered", "theta"): 4 + gb,
                 ("exact", "theta"): k_local * wb + gb, ("exact", "workers"): (k_local + 1) * wb}
        cands = {key: v for key, v in cands.items()
                 if mode in ("auto", key[0]) and broadcast in ("auto", key[1])}
        if mode == "reduce_q":                         # opt-in only: never a candidate of "auto"
            cands = {("reduce_q", "theta"): _Q_BITS[wire_format] / 8 + 1 / 32 + gb}
        # fewest wire bytes per element; ties go to the bit-exact schedule, then to the one whose
        # cross-rank sum has a fixed order (reduce_ordered) over RCCL's own (reduce)
        pref = {"exact": 0, "reduce_ordered": 1, "reduce": 2, "reduce_q": 3}
        mode, broadcast = min(cands, key=lambda key: (cands[key], pref[key[0]], key[1] != "workers"))
        self.kernels = kernels or _ops
        self.mode = mode
        self.broadcast = broadcast
        self.layout = layout
        self.lr, self.momentum, self.nesterov = lr, momentum, nesterov
        self.k_local = k_local
        self.k_total = k_local * self.world
        self.rounding, self.seed = rounding, int(seed)
        self.q_step = 0                # stochastic rounding: the step counter of the random bits
        self.guard = guard
        self.last_stats = None         # the last guarded step's report, identical on every rank
        self._guard_plans = {}
        self.gather_format = gather_format
        if guard is not None:
            self._check_guard()
        n = layout.total
        # buckets: multiples of world * 64 elements so every shard is 16-byte aligned (reduce_q:
        # world * 512, so every shard is a whole region of the wire format)
        unit = self.world * (512 if mode == "reduce_q" else 64)
        bucket = max(unit, bucket_elems // unit * unit)
        self.n = n
        self.n_pad = math.ceil(n / unit) * unit
        self.bucket = min(bucket, self.n_pad)
        self.buckets = [(b, min(b + self.bucket, self.n_pad)) for b in range(0, self.n_pad, self.bucket)]
        self.theta_buf = torch.zeros(self.n_pad, dtype=theta_dtype, device=device)
        self.theta = ParamArena(layout, theta_dtype, device, self.theta_buf[:n])
        self.worker_bufs = [torch.zeros(self.n_pad, dtype=worker_dtype, device=device) for _ in range(k_local)]
        self.workers = [ParamArena(layout, worker_dtype, device, w[:n]) for w in self.worker_bufs]
        shard_total = sum((e - b) // self.world for b, e in self.buckets)
        self.mom_shard = torch.zeros(shard_total, dtype=theta_dtype, device=device) if momentum else None
        self.has_momentum = False
        # RCCL (and the virtual ranks) reduce/gather in place; gloo gets separate buffers
        self.inplace = self.comm.inplace
        self.kernel_events = None      # a list: (start, end) HIP events around every local kernel
        self.event_factory = _timing_event   # bench.py's host rehearsal swaps in host-clock events
        # (Vec::size(), threads) of the reference's host: exact mode reproduces its bf16 scalar tails
        # (diloco.outer_step's cpu_tails; the reduce mode reassociates the sum anyway)
        self.tail_bits = None
        if cpu_tails is not None and mode == "exact" and self.kernels is _ops:
            from .torchcompat import torch_cpu_tail_bits
            self.tail_bits = torch_cpu_tail_bits(list(layout.numels) + [self.n_pad - n], vec_elems=cpu_tails[0],
                                                 num_threads=cpu_tails[1], device=device)
        if mode == "reduce":
            self.acc = torch.zeros(self.n_pad, dtype=torch.float32, device=device)
            self.acc_shard = None if self.inplace else torch.empty(shard_total, dtype=torch.float32, device=device)
        elif mode == "reduce_ordered":
            # partials laid out [dest rank][shard] per bucket, received as [src rank][shard]
            self.acc = torch.zeros(self.n_pad, dtype=torch.float32, device=device)
            self.acc_recv = torch.zeros(self.n_pad, dtype=torch.float32, device=device)
        elif mode == "reduce_q":
            # per bucket `world` regions of one shard each, [dest rank][payload | scales], received
            # as [src rank][payload | scales]; a bucket starts at byte _q_bytes(b) of both buffers
            self.wire_format = wire_format
            self.q_send = torch.zeros(self._q_bytes(self.n_pad), dtype=torch.uint8, device=device)
            self.q_recv = torch.zeros(self._q_bytes(self.n_pad), dtype=torch.uint8, device=device)
            self.residual = torch.zeros(self.n_pad, dtype=torch.float32, device=device) if error_feedback else None
            # a guarded step with error feedback writes the new residual here and swaps the two
            # once the step is decided (`_commit_residual`): a refusal leaves `residual` as it was
            self._residual_next = (torch.zeros(self.n_pad, dtype=torch.float32, device=device)
                                   if error_feedback and guard is not None else None)
            self._residual_pending = False
            if gather_format is not None:
                # the owners' updates of a bucket, [src rank][payload | scales], from byte
                # _q_bytes(b, gather_format); this rank writes its own slot, the all-gather the rest
                self.u_recv = torch.zeros(self._q_bytes(self.n_pad, gather_format), dtype=torch.uint8, device=device)
                self.residual_g = (torch.zeros(shard_total, dtype=torch.float32, device=device)
                                   if error_feedback else None)
        else:
            # recv[j][b:e] viewed [src rank][per]: local worker j of every rank, this rank's shard
            self.recv = [torch.empty(self.n_pad, dtype=worker_dtype, device=device) for _ in range(k_local)]

    # ---------------------------------------------------------------------------------------
    def _shard(self, b, e):
        per = (e - b) // self.world
        return b + self.rank * per, b + (self.rank + 1) * per

    def _q_bytes(self, elems: int, fmt: str | None = None) -> int:
        """Packed bytes of `elems` elements (a multiple of 512) in this sync's wire format (or in
        `fmt`): the payload and one scale byte per 32 elements. Linear in elems, so it is also the
        byte offset of element offset `elems` in the send / receive buffers."""
        return elems * _Q_BITS[fmt or self.wire_format] // 8 + elems // 32

    def _launch(self, fn, *args, **kw):
        """A local kernel, bracketed by timing events on its launch stream when
        `kernel_events` is a list (bench.py: the per-rank HBM roofline at N > 1)."""
        if self.kernel_events is None:
            return fn(*args, **kw)
        a, b = self.event_factory(), self.event_factory()
        a.record()
        got = fn(*args, **kw)
        b.record()
        self.kernel_events.append((a, b))
        return got

    def _check_guard(self):
        """The constructor's refusals of guard=: each says what is missing."""
        if not isinstance(self.guard, OuterGuard):
            raise TypeError("guard must be an OuterGuard")
        if self.guard.per_tensor:
            raise ValueError("guard.per_tensor is not available on the sharded step: shards cut tensors, so no "
                             "rank holds a tensor's rows")
        if self.k_total > 64:
            raise EdtError(f"a guarded step takes at most 64 workers in all, not {self.k_total}")
        k = self.kernels
        measure = {"exact": [], "reduce_q": ["partial_sum_stats_q"]}.get(self.mode, ["partial_sum_stats"])
        need = ["make_slerp_plan", "delta_stats"] + measure
        need.append(_scaled(self._step_name()))
        missing = [m for m in need if not hasattr(k, m)]
        if missing:
            err = GuardKernelsMissing if self.mode == "reduce_q" else EdtError
            raise err(f"guard= with mode={self.mode!r} needs kernels that provide {need}; "
                      f"{type(k).__name__ if not hasattr(k, '__name__') else k.__name__} lacks {missing}")

    def _step_name(self) -> str:
        """The entry that steps an owned shard in this schedule, before `_entry` picks its plain or
        scaled form. Without sgd_apply_sum (stand-in kernels) reduce_ordered sums in torch."""
        if self.mode == "exact":
            return "outer_step"
        if self.mode == "reduce_q":           # phase 2, or phase 2' of the quantized gather
            return "sgd_apply_sum_q" if self.gather_format is None else "sgd_delta_sum_q"
        if self.mode == "reduce_ordered" and hasattr(self.kernels, "sgd_apply_sum"):
            return "sgd_apply_sum"
        return "sgd_apply"

    def guard_bytes(self) -> int:
        """Algorithmic HBM bytes the guard adds to one step on this rank (no drop; kernel_bytes()
        keeps its meaning). Reduce schedules: edt_delta_stats over the local arenas (theta and the
        K_local workers, whole arena) and edt_partial_sum_stats over the owned shards' partials (N
        of them, reduce: the one reduced shard; reduce_q: edt_partial_sum_stats_q over the N packed
        regions, q bytes per element each); exact: edt_delta_stats over the owned shards with all K
        received slices. The shadow residual of reduce_q adds memory, no traffic. 0 without a guard."""
        if self.guard is None:
            return 0
        wb = self.worker_bufs[0].element_size()
        gb = self.theta_buf.element_size()
        shard = self.n_pad // self.world
        if self.mode == "exact":
            return shard * (self.k_total * wb + gb)
        if self.mode == "reduce_q":
            return self.n_pad * (self.k_local * wb + gb) + self.world * self._q_bytes(shard)
        nacc = self.world if self.mode == "reduce_ordered" else 1
        return self.n_pad * (self.k_local * wb + gb) + shard * 4 * nacc

    def kernel_bytes(self, broadcast: bool = False) -> int:
        """Algorithmic HBM bytes of one step's local kernels on this rank (steady state:
        momentum read + written). exact: the fused kernel over the owned shards with all K
        workers; reduce: the partial over the whole arena + the SGD over the owned shards.
        broadcast: of step(broadcast=True) — the K_local worker arenas written (fused into phase 3
        of the quantized gather), and theta read once more where edt_broadcast_theta does it."""
        if broadcast and self.broadcast != "workers":
            wb = self.worker_bufs[0].element_size()
            fused = self.mode == "reduce_q" and self.gather_format is not None
            return self.kernel_bytes() + self.n_pad * (self.k_local * wb
                                                       + (0 if fused else self.theta_buf.element_size()))
        wb = self.worker_bufs[0].element_size()
        gb = self.theta_buf.element_size()
        shard = self.n_pad // self.world
        mom = 2 * gb if self.momentum else 0
        if self.mode == "exact":
            return shard * (self.k_total * wb + 2 * gb + mom)
        if self.mode == "reduce_ordered":
            return self.n_pad * (self.k_local * wb + gb + 4) + shard * (4 * self.world + 2 * gb + mom)
        if self.mode == "reduce_q":
            # phase 1 writes q instead of 4 B per element (+ the residual read and written with
            # error feedback); phase 2 reads N x q instead of N x 4 B per owned element
            ef = 8 if self.residual is not None else 0
            p1 = self.n_pad * (self.k_local * wb + gb + ef) + self._q_bytes(self.n_pad)
            if self.gather_format is not None:
                # phase 2' reads theta, the momentum and N regions, writes the momentum and one
                # region (+ its residual read and written); phase 3 reads and writes theta over the
                # whole arena and reads every owner's region
                gf = self.gather_format
                return (p1 + shard * (gb + mom + ef) + self.world * self._q_bytes(shard) + self._q_bytes(shard, gf)
                        + self.n_pad * 2 * gb + self._q_bytes(self.n_pad, gf))
            return p1 + shard * (2 * gb + mom) + self.world * self._q_bytes(shard)
        return self.n_pad * (self.k_local * wb + gb + 4) + shard * (4 + 2 * gb + mom)

    @traced("edt/ShardedOuterSync.step")
    def step(self, broadcast: bool = False) -> None:
        """One outer step; returns when the work is enqueued (stream-ordered, async).
        broadcast=True: every local worker arena over [0, n_pad) also holds the new theta rounded
        to the worker dtype when the step's work completes (module docstring); theta, the momentum,
        the residuals and q_step are what step() leaves."""
        with trange(f"edt/sharded.{self.mode}/{self.broadcast}"):
            self._step_body(broadcast)
        self.q_step += 1

    def _sr(self, encoder: int, elem_base: int) -> dict:
        """The stochastic-rounding keywords of one encoder launch (none in nearest mode, so stand-in
        kernels without them keep working): stream 2 * rank for phase 1, 2 * rank + 1 for phase 2';
        elem_base is the launch's first element in the arena."""
        if self.rounding != "stochastic":
            return {}
        return {"rounding": "stochastic", "seed": self.seed, "step": self.q_step,
                "stream_id": 2 * self.rank + encoder, "elem_base": elem_base}

    def _step_body(self, broadcast: bool = False) -> None:
        """The driver every schedule shares. Per bucket, `_produce_<mode>` launches the bucket's
        local work (if any) and issues its collectives, all buckets before the first wait, so the
        traffic of bucket i overlaps the kernels of bucket i + 1. Then, per bucket in order, its
        handles are waited for and `_consume_<mode>` steps the owned shard [s0, s1) — `mom` is its
        slice `sl` of the sharded momentum — and returns the handle of the bucket's gather.

        broadcast (step(broadcast=True)): as each bucket's gather lands, its slice of every local
        worker arena is overwritten with round_w(theta_new) on the compute stream — fused into
        phase 3 where that pass exists, else by one edt_broadcast_theta per bucket while later
        buckets' gathers are still in flight. The arenas are the step's inputs, so the hazards are:
        the reduce schedules read them in phase 1 only, and phase 1 of every bucket is enqueued
        above before any destination store, on the same stream; exact mode's all-to-alls read them
        on the communicator's stream, and a bucket's all-to-all handles are waited for (before its
        consume, hence before its gather is issued and waited for) before its arena slice is
        written. broadcast="workers" already leaves the arenas so: nothing is added."""
        refresh = broadcast and self.broadcast != "workers"
        produce = getattr(self, "_produce_" + self.mode)
        consume = getattr(self, "_consume_" + self.mode)
        if self.guard is not None:
            # measured, screened and clipped first (_guarded): every exchange is waited for before
            # the decision, so nothing below runs on a step the guard refuses
            gathers = self._guarded(produce, consume)
        else:
            works = [produce(b, e, _NO_GUARD) for b, e in self.buckets]
            gathers = []
            for owned, ws in zip(self._owned(), works):
                for w in ws:
                    w.wait()
                gathers.append(consume(*owned, _NO_GUARD))
        if self.mode == "reduce_q" and self.gather_format is not None:
            # phase 3: as each bucket's updates land, every rank adds the same D(q) to its replica
            gf = self.gather_format
            fused = refresh and hasattr(self.kernels, "broadcast_theta")
            for (b, e), g in zip(self.buckets, gathers):
                g.wait()
                self._launch(self.kernels.apply_delta_q, self.theta_buf[b:e],
                             self.u_recv[self._q_bytes(b, gf):self._q_bytes(e, gf)], (e - b) // self.world, gf,
                             **({"broadcast": [w[b:e] for w in self.worker_bufs]} if fused else {}))
                if refresh and not fused:
                    self._refresh_workers(b, e)
        elif refresh:
            for (b, e), g in zip(self.buckets, gathers):
                g.wait()
                self._refresh_workers(b, e)
        for g in gathers:
            g.wait()
        if self.broadcast == "workers":
            for w in self.worker_bufs[1:]:          # every local worker starts from the same theta
                w.copy_(self.worker_bufs[0])
        if self.momentum:
            self.has_momentum = True

    def _owned(self):
        """Per bucket (b, e), the owned shard [s0, s1) and its slice `sl` of the sharded momentum
        (`mom`, or None)."""
        mom_off = 0
        for b, e in self.buckets:
            s0, s1 = self._shard(b, e)
            sl = slice(mom_off, mom_off + (s1 - s0))
            yield b, e, s0, s1, (None if self.mom_shard is None else self.mom_shard[sl]), sl
            mom_off = sl.stop

    # ---- the guarded step (guard=OuterGuard) -----------------------------------------------
    # One rule: every rank forms the same float64 totals from the same numbers in the same order —
    # per rank its buckets in order and their chunks in order (cumsum), then the ranks in rank order
    # after an all_gather_object of the per-rank totals, never an all-reduce in the library's own
    # order — and calls the same pure guard.guard_decision on them. So every rank steps, or every
    # rank raises the same exception, with every issued collective waited for.

    def _stats_plan(self, n):
        plan = self._guard_plans.get(n)
        if plan is None:
            plan = self._guard_plans[n] = self.kernels.make_slerp_plan([0, n], self.theta_buf.device)
        return plan

    def _rank_totals(self, rows: list, width: int):
        """rows: this rank's per-bucket row blocks (device, consumed before the next statistics
        call reuses the workspace: cloned as they come). One host sync; the totals of every column
        over this rank's chunks in order, then over the ranks in rank order."""
        mine = sequential_total(torch.cat([r.reshape(-1, width) for r in rows]).cpu().numpy(), width)
        return sequential_total(self.comm.all_gather_object(mine.tolist()), width)

    def _exchange(self, produce, v: _Verdict) -> None:
        """Every bucket's produce, then every handle waited for: nothing is in flight afterwards."""
        for ws in [produce(b, e, v) for b, e in self.buckets]:
            for w in ws:
                w.wait()

    def _screen(self, totals: dict) -> list:
        """A step's first statistics, recorded and screened (may refuse) -> the surviving workers."""
        self.last_stats = dict(report(totals), clip_coef=None, dropped=[])
        return list(guard_decision(totals, self.guard)[0])

    def _verdict(self, survivors: list, clip: float) -> _Verdict:
        if len(survivors) == self.k_total:
            return _NO_GUARD._replace(clip=clip)
        lo = self.rank * self.k_local
        return _Verdict([k - lo for k in survivors if lo <= k < lo + self.k_local], len(survivors), survivors, clip)

    def _guarded(self, produce, consume):
        """The tail both schedule families share. Each family returns the totals over all workers,
        the totals of what will be applied and the survivors, with every exchange waited for."""
        totals, final, survivors = (self._guard_exact if self.mode == "exact" else self._guard_reduce)(produce)
        rep = self.last_stats
        rep["dropped"] = [k for k in range(self.k_total) if k not in survivors]
        try:
            _, clip = guard_decision(final, self.guard)
        except NonFiniteWorkers as err:         # the survivors' view -> every worker's counts
            raise NonFiniteWorkers(str(err), totals["nonfinite"], final["nonfinite_mean"], survivors) from None
        if clip is None:                        # cannot happen: every survivor was finite
            raise EdtError("the survivors' statistics flagged a worker")
        rep["clip_coef"] = clip
        self._commit_residual()                 # the step is decided: nothing below refuses
        v = self._verdict(survivors, clip)
        return [consume(*owned, v) for owned in self._owned()]

    def _commit_residual(self):
        """reduce_q with error feedback: a guarded phase 1 wrote the new residual into the second
        buffer; the step has been decided, so the two swap. Per rank: a rank that launched no
        phase 1 (no surviving worker) keeps its residual."""
        if self.mode == "reduce_q" and self._residual_pending:
            self.residual, self._residual_next = self._residual_next, self.residual
            self._residual_pending = False

    def _guard_reduce(self, produce):
        """Reduce schedules. Before any exchange, edt_delta_stats over the local workers and the
        whole arena gives every worker's S_kk and non-finite count (its local-mean columns are
        ignored: the mean is not known where the deltas are); gathered, global worker index
        rank * K_local + j; the policy screens the workers with nothing in flight. Then phase 1 over
        the survivors and every exchange, and the mean's statistics from what the owners hold
        (reduce_q: of the dequantized regions, the value phase 2 applies)."""
        kl, K = self.k_local, self.k_total
        if self.mode == "reduce_q":
            self._residual_pending = False      # a refused step's second buffer is simply overwritten
        rows = torch.as_tensor(self._launch(self.kernels.delta_stats, self.theta_buf, list(self.worker_bufs),
                                            self._stats_plan(self.n_pad)))
        t = sequential_total(rows.cpu().numpy(), 3 * kl + 2)                     # host sync 1 of 2
        cols = _ops.stats_columns(kl)
        every = self.comm.all_gather_object((t[cols["S_kk"]].tolist(), t[cols["nonfinite"]].tolist()))
        row, cols = np.zeros(3 * K + 2), _ops.stats_columns(K)
        row[cols["S_kk"]] = [x for skk, _ in every for x in skk]
        row[cols["nonfinite"]] = [x for _, nf in every for x in nf]
        # the mean's columns stay zero until the exchange, and no schedule here forms S_km
        totals = dict(totals_from_row(row, K), S_km=None)
        survivors = self._screen(totals)
        self._exchange(produce, self._verdict(survivors, 1.0))
        rows = []
        for b, e, s0, s1, _, _ in self._owned():
            if self.mode == "reduce_q":
                got = self._launch(self.kernels.partial_sum_stats_q, self._q_regions(b, e), self.wire_format,
                                   self.theta_buf.dtype, self._stats_plan(s1 - s0))
            else:
                parts = ([self._acc_out(b, e)] if self.mode == "reduce"
                         else list(self.acc_recv[b:e].view(self.world, s1 - s0)))
                got = self._launch(self.kernels.partial_sum_stats, parts, self.theta_buf.dtype,
                                   self._stats_plan(s1 - s0))
            rows.append(torch.as_tensor(got).clone())
        t = self._rank_totals(rows, 2)                                           # host sync 2 of 2
        totals["S_mm"], totals["nonfinite_mean"] = float(t[0]), int(t[1])
        self.last_stats.update(report(totals))
        return totals, dict(totals, nonfinite=[int(totals["nonfinite"][k]) for k in survivors]), survivors

    def _guard_exact(self, produce):
        """exact: every all-to-all first, then edt_delta_stats on the received slices; after a drop
        the survivors are measured again, as diloco._guard_pass does."""
        self._exchange(produce, _NO_GUARD)
        totals = final = self._measure_exact(list(range(self.k_total)))
        survivors = self._screen(totals)
        if len(survivors) < self.k_total:
            final = self._measure_exact(survivors)
            fold_remeasured(self.last_stats, report(final), survivors, self.k_total)
        return totals, final, survivors

    def _measure_exact(self, idx):
        """exact: edt_delta_stats on every owned shard with the received slices of workers `idx`
        (all the all-to-alls have been waited for) -> the totals over every rank's shards."""
        K = len(idx)
        rows = []
        for b, e, s0, s1, _, _ in self._owned():
            shards = self._received(b, e)
            rows.append(torch.as_tensor(self._launch(self.kernels.delta_stats, self.theta_buf[s0:s1],
                                                     [shards[i] for i in idx], self._stats_plan(s1 - s0))).clone())
        return totals_from_row(self._rank_totals(rows, 3 * K + 2), K)

    def _received(self, b, e):
        """exact: the owned shard's slice of every worker as the all-to-alls of bucket [b, e) left
        it, in the reference's worker order (global worker k = src * K_local + j)."""
        rv = [r[b:e].view(self.world, (e - b) // self.world) for r in self.recv]
        return [rv[j][src] for src in range(self.world) for j in range(self.k_local)]

    def _refresh_workers(self, b, e):
        """Bucket [b, e) of every local worker arena <- round_w(theta) (torch copy_: RNE), theta
        read once (edt_broadcast_theta); its gather has been waited for."""
        dst = [w[b:e] for w in self.worker_bufs]
        if hasattr(self.kernels, "broadcast_theta"):
            self._launch(self.kernels.broadcast_theta, self.theta_buf[b:e], dst)
            return
        for d in dst:                        # stand-in kernels (CPU tests): the same copies in torch
            d.copy_(self.theta_buf[b:e])

    def _partial(self, b, e, v: _Verdict):
        """Phase 1 of the fp32 reduce schedules: the local workers' partial sum of bucket [b, e).
        After a guarded drop (`v.local`): over this rank's surviving workers, divided by the number
        of survivors in all; a rank with none contributes a zero partial."""
        workers, k_total = self.worker_bufs, self.k_total
        if v.local is not None:
            workers, k_total = [self.worker_bufs[j] for j in v.local], v.divisor
            if not workers:
                self.acc[b:e].zero_()
                return
        self._launch(self.kernels.delta_partial, self.theta_buf[b:e], [w[b:e] for w in workers],
                     k_total, self.acc[b:e], False)

    # reduce: reduce-scatter each bucket's partial as soon as it is ready; SGD on the owned shard
    def _produce_reduce(self, b, e, v):
        self._partial(b, e, v)
        return [self.comm.reduce_scatter(self._acc_out(b, e), self.acc[b:e], async_op=True)]

    def _consume_reduce(self, b, e, s0, s1, mom, sl, v):
        name, scale = _entry(self._step_name(), v.clip)
        self._launch(getattr(self.kernels, name), self.theta_buf[s0:s1], self._acc_out(b, e), mom, self.has_momentum,
                     self.lr, self.momentum, self.nesterov, *scale)
        return self._gather(b, e, s0, s1)

    # reduce_ordered: the partial of bucket [b, e) is laid out [dest rank][shard]; the all-to-all
    # delivers it as [src rank][shard], and the owned shard's N partials are summed in rank order
    def _produce_reduce_ordered(self, b, e, v):
        self._partial(b, e, v)
        return [self.comm.all_to_all(self.acc_recv[b:e], self.acc[b:e], async_op=True)]

    def _consume_reduce_ordered(self, b, e, s0, s1, mom, sl, v):
        self._launch(self._sgd_sum, self.theta_buf[s0:s1], list(self.acc_recv[b:e].view(self.world, s1 - s0)), mom,
                     v.clip)
        return self._gather(b, e, s0, s1)

    # reduce_q: reduce_ordered with quantized partials: phase 1 writes bucket [b, e) as `world`
    # packed regions [dest rank][payload | scales] (the fp32 partial stays in registers), the
    # all-to-all moves the bytes; phase 2 dequantizes the owned shard's N regions
    # A guarded step (`v` from the screening): phase 1 over this rank's survivors, divided by the
    # number of survivors in all; a rank with none launches nothing, sends the wire format's zero
    # (scale byte 0, codes 0: D = +0 everywhere) and keeps its residual; with error feedback the new
    # residual goes to the second buffer until `_commit_residual`
    def _produce_reduce_q(self, b, e, v):
        qb, qe = self._q_bytes(b), self._q_bytes(e)
        workers, k_total = self.worker_bufs, self.k_total
        if v.local is not None:
            workers, k_total = [self.worker_bufs[j] for j in v.local], v.divisor
        if not workers:
            self.q_send[qb:qe].zero_()
        else:
            kw = self._sr(0, b)
            if self.guard is not None and self.residual is not None:
                if self._residual_next is None:
                    raise EdtError("guard= on reduce_q with error feedback must be given to the constructor "
                                   "(it allocates the second residual buffer)")
                kw["residual_out"] = self._residual_next[b:e]
                self._residual_pending = True
            self._launch(self.kernels.delta_partial_q, self.theta_buf[b:e], [w[b:e] for w in workers],
                         k_total, self.q_send[qb:qe], (e - b) // self.world, self.wire_format,
                         None if self.residual is None else self.residual[b:e], **kw)
        return [self.comm.all_to_all(self.q_recv[qb:qe], self.q_send[qb:qe], async_op=True)]

    def _q_regions(self, b, e):
        """The owned shard's `world` received regions of bucket [b, e), in rank order."""
        per = (e - b) // self.world
        return list(self.q_recv[self._q_bytes(b):self._q_bytes(e)].view(self.world, self._q_bytes(per)))

    def _consume_reduce_q(self, b, e, s0, s1, mom, sl, v):
        k, per = self.kernels, s1 - s0
        regions = self._q_regions(b, e)
        name, scale = _entry(self._step_name(), v.clip)
        if self.gather_format is None:
            self._launch(getattr(k, name), self.theta_buf[s0:s1], regions, self.wire_format, mom,
                         self.has_momentum, self.lr, self.momentum, self.nesterov, *scale)
            return self._gather(b, e, s0, s1)
        # phase 2': the quantized update of the owned shard into this rank's slot of u_recv (theta
        # untouched), then the all-gather of the packed bytes
        gf = self.gather_format
        ub, ur = self._q_bytes(b, gf), self._q_bytes(per, gf)
        slot = self.u_recv[ub + self.rank * ur:ub + (self.rank + 1) * ur]
        res_g = None if self.residual_g is None else self.residual_g[sl]
        self._launch(getattr(k, name), self.theta_buf[s0:s1], regions, self.wire_format, mom,
                     self.has_momentum, self.lr, self.momentum, self.nesterov, slot, gf, *scale, res_g,
                     **self._sr(1, s0))
        src = slot if self.inplace else slot.clone()
        return self.comm.all_gather(self.u_recv[ub:self._q_bytes(e, gf)], src, async_op=True)

    # exact: every bucket's all-to-all straight from the worker arenas (a worker's bucket [b, e) is
    # already laid out [dest rank][per]), one collective per local worker; as each bucket lands,
    # the single-GPU fused step on the owned shard
    def _produce_exact(self, b, e, v):
        return [self.comm.all_to_all(self.recv[j][b:e], wb[b:e], async_op=True)
                for j, wb in enumerate(self.worker_bufs)]

    def _consume_exact(self, b, e, s0, s1, mom, sl, v):
        k = self.kernels
        shards = self._received(b, e)
        if v.survivors is not None:        # a guarded step: the workers the guard kept
            shards = [shards[i] for i in v.survivors]
        name, scale = _entry(self._step_name(), v.clip)
        # shards start at multiples of 64: whole bytes of the tail mask
        tail = {} if self.tail_bits is None else {"tail_bits": self.tail_bits[s0 // 8:(s1 + 7) // 8]}
        # broadcast="workers": the plain HIP kernel also stores the new shard, rounded to the worker
        # dtype, into local worker 0's arena (its bucket has been sent) — the rounding copy fused
        # into the step; the scaled and the tail forms have no fused broadcast
        fused = self.broadcast == "workers" and k is _ops and not scale and not tail
        self._launch(getattr(k, name), self.theta_buf[s0:s1], shards, mom, self.has_momentum, self.lr,
                     self.momentum, self.nesterov, *scale, *([[self.worker_bufs[0][s0:s1]]] if fused else []), **tail)
        if self.broadcast == "workers":
            return self._gather_to_workers(b, e, s0, s1, rounded=fused)
        return self._gather(b, e, s0, s1)

    def _sgd_sum(self, theta, parts, mom, clip):
        """SGD from the shard's per-rank partials, summed in rank order."""
        step = self._step_name()
        name, scale = _entry(step, clip)
        if step == "sgd_apply":
            total = parts[0].clone()         # stand-in kernels (CPU tests): the same order in torch
            for p in parts[1:]:
                total.add_(p)
            parts = total
        getattr(self.kernels, name)(theta, parts, mom, self.has_momentum, self.lr, self.momentum, self.nesterov, *scale)

    def _acc_out(self, b, e):
        """Reduce-scatter destination for bucket [b, e): this rank's slice of the acc buffer
        (in place, as RCCL allows: recv == send + rank * count); a separate slice elsewhere."""
        s0, s1 = self._shard(b, e)
        if self.inplace:
            return self.acc[s0:s1]
        off = sum((e2 - b2) // self.world for b2, e2 in self.buckets if b2 < b)
        return self.acc_shard[off:off + (s1 - s0)]

    def _gather(self, b, e, s0, s1):
        """All-gather the updated shards of bucket [b, e) into every rank's theta replica."""
        src = self.theta_buf[s0:s1] if self.inplace else self.theta_buf[s0:s1].clone()
        return self.comm.all_gather(self.theta_buf[b:e], src, async_op=True)

    def _gather_to_workers(self, b, e, s0, s1, rounded=False):
        """The new theta shard of bucket [b, e), rounded to the worker dtype (torch copy_: RNE;
        rounded=True: the kernel already stored it), all-gathered into local worker 0's arena
        (its bucket was consumed by the all-to-all)."""
        w0 = self.worker_bufs[0]
        if not rounded:
            w0[s0:s1].copy_(self.theta_buf[s0:s1])
        src = w0[s0:s1] if self.inplace else w0[s0:s1].clone()
        return self.comm.all_gather(w0[b:e], src, async_op=True)

    def gather_theta(self) -> torch.Tensor:
        """The full master theta on every rank (with broadcast="workers" it is kept sharded;
        this assembles it, e.g. for a checkpoint). Returns the flat theta (length P)."""
        if self.broadcast == "workers":
            for b, e in self.buckets:
                s0, s1 = self._shard(b, e)
                src = self.theta_buf[s0:s1] if self.inplace else self.theta_buf[s0:s1].clone()
                self.comm.all_gather(self.theta_buf[b:e], src)
        return self.theta.flat

    # ---------------------------------------------------------------------------------------
    def bytes_reduced(self) -> int:
        """Metric bytes of one step on this rank: K_local x P x bytes per worker element."""
        return self.k_local * self.n * self.worker_bufs[0].element_size()

    def wire_bytes(self) -> int:
        """Bytes this rank sends over xGMI per step (ring/all-to-all lower bound)."""
        f = (self.world - 1) / self.world
        bg = self.theta_buf.element_size()
        wb = self.worker_bufs[0].element_size()
        if self.mode == "reduce_q" and self.gather_format is not None:     # packed both ways
            return int(f * (self._q_bytes(self.n_pad) + self._q_bytes(self.n_pad, self.gather_format)))
        if self.mode == "reduce_q":        # the packed partials + theta: (N-1)/N * P * (q + b_g)
            return int(f * (self._q_bytes(self.n_pad) + self.n_pad * bg))
        if self.mode.startswith("reduce"):
            return int(f * self.n_pad * (4 + bg))
        return int(f * self.n_pad * (self.k_local * wb + (wb if self.broadcast == "workers" else bg)))


class PopulationCrossover:
    """EDT / SLERP children across GPUs: one population member per rank (member r on rank r,
    child c built on rank c). The only exchange is point-to-point: a grouped batch of RCCL
    send/recv delivers each child's parents to its rank (schedule.exchange_plan: one transfer per
    (member, destination), each over the direct xGMI link between the two GPUs); the merge itself
    is the single-GPU kernel, with no collective.

    The reference does this through the shared disk: every worker loads both parents' checkpoint
    directories (EDT_LM/train/crossover.py:255-258, EDT_EVOMERGE/train/crossover.py:167-168), and
    the RL master merges pairs one after another in one process (EDT_RL/edt.py:286-299)."""

    def __init__(self, layout: ParamLayout, dtype: torch.dtype, device, group=None, kernels=None,
                 comm: Collectives | None = None):
        self.comm = comm or TorchCollectives(group)
        self.world = self.comm.world
        self.rank = self.comm.rank
        self.kernels = kernels or _ops
        self.layout = layout
        self.device = device
        self.dtype = dtype
        self._bufs = {}
        self._plan = None

    def _buf(self, key, dtype=None):
        if key not in self._bufs:
            self._bufs[key] = torch.empty(self.layout.total, dtype=dtype or self.dtype, device=self.device)
        return self._bufs[key]

    def _exchange(self, pairs, payload, like=None):
        """payload(member, dst) -> tensors this rank ships for its member to the rank building
        child dst; like(src_member) -> the tensors this rank receives for that parent (shapes and
        dtypes; default: what this rank would ship for its own member). Returns the parents'
        tensor lists for this rank's child: ([...] of parent 1, [...] of parent 2)."""
        from .schedule import exchange_plan
        n = self.world
        if len(pairs) != n:
            raise ValueError(f"{len(pairs)} children for {n} ranks: one child per rank")
        plan = exchange_plan(pairs, list(range(n)), list(range(n)))
        mine = plan[self.rank]
        ops_ = []
        for m, dst in mine["send"]:
            for t in payload(m, dst):
                ops_.append(("send", t, dst))
        i, j = pairs[self.rank]
        got = {}
        for m, src in mine["recv"]:
            shapes = like(m) if like is not None else payload(self.rank, self.rank)
            bufs = [self._buf(("recv", m == i, k), t.dtype) for k, t in enumerate(shapes)]
            for b in bufs:
                ops_.append(("recv", b, src))
            got[m] = bufs
        self.comm.p2p(ops_)
        par1 = payload(i, self.rank) if i == self.rank else got[i]
        par2 = payload(j, self.rank) if j == self.rank else got[j]
        return par1, par2

    @traced("edt/PopulationCrossover.slerp_step")
    def slerp_step(self, member: torch.Tensor, pairs, t: torch.Tensor, out: torch.Tensor,
                   dot_threshold: float = 0.9995, eps: float = 1e-8) -> None:
        """SLERP child of pairs[rank] into `out` (EDT_RL/crossover.py:84-135 per Policy/Value;
        EDT_EVOMERGE/train/crossover.py:104-146). member: this rank's flat parameters."""
        (p1,), (p2,) = self._exchange(pairs, lambda m, dst: [member])
        if self._plan is None:
            self._plan = self.kernels.make_slerp_plan(self.layout.offsets, self.device)
        self.kernels.slerp_arena(self._plan, p1, p2, out, t, dot_threshold, eps)

    def pair_merge_step(self, base: torch.Tensor, trained: torch.Tensor, momentum: torch.Tensor | None,
                        pairs, out: torch.Tensor, out_momentum: torch.Tensor | None, lr: float = 0.7,
                        mu: float = 0.9, nesterov: bool = True, has_momentum: bool = True,
                        generation: int = 0) -> None:
        """EDT-LM child of pairs[rank] (EDT_LM/train/crossover.py:150-237): both parents ship
        (base, trained); the child inherits parent 1's outer momentum when parent 1 has one, else
        parent 2's (:183-227), and only that donor ships it. Which members have a momentum
        (`momentum is not None and has_momentum` on their rank) is agreed first, so every rank
        knows every message; a child with no donor past generation 0 raises NotImplementedError
        on every rank, as the reference's crossover does (:226-227)."""
        flags = self.comm.all_gather_object(bool(has_momentum and momentum is not None))
        donors = [i if flags[i] else (j if flags[j] else None) for i, j in pairs]
        if mu != 0 and generation > 0 and any(d is None for d in donors):
            raise NotImplementedError("Merging outer optimizer states not implemented for this case.")
        donor = donors[self.rank]
        if donor is not None and out_momentum is None:
            raise ValueError("the child inherits an outer momentum: pass out_momentum")

        def payload(m, dst):
            return [base, trained] + ([momentum] if donors[dst] == m else [])

        def like(m):
            return [base, trained] + ([out_momentum] if donor == m else [])
        par1, par2 = self._exchange(pairs, payload, like)
        if donor is not None:
            out_momentum.copy_((par1 if donor == pairs[self.rank][0] else par2)[2])
        self.kernels.pair_merge(par1[0], par2[0], par1[1], par2[1], out, out_momentum,
                                donor is not None, lr, mu, nesterov)


class ShardedPopulationCrossover:
    """A generation of a population of P = world members (one per GPU: BASELINE configs[4], the
    EDT-RL / EVOMERGE population of 8 SLERP-crossed on 7B bodies across 8 GPUs; or the EDT-LM pair
    merges), link-balanced. PopulationCrossover ships each child's two parents whole to the child's
    rank — two full members over at most two of the GPU's seven xGMI links. Here every rank owns a
    parameter-index shard instead (a contiguous range of whole SLERP chunks, ~1/N of the layout):

      1. members -> shards: rank r sends rank s the slice of its member in s's range (grouped p2p,
         every link busy: (N-1)/N of a member out and in per rank);
      2. SLERP: per chunk of the rank's range the sums the generation needs — each distinct
         parent's norm and each distinct dot its children use, per connected component of the
         pair graph (edt_slerp_needed_sums: edt_slerp_population's needed-sums pass, r5; a
         component's row is its D norms, D ring-dot and <= 4 chord slots, against the Gram
         triangle's 36 at N = 8) — the table rows all-gathered
         (nchunks x those sums doubles: 12-16 MB at 7B for a roulette-drawn generation, against ~31 MB
         for the triangle), then every child's coefficients (edt_slerp_needed_coef) — each chunk's
         sums come from the same kernel in the same order wherever the chunk lives, so every child
         is bit-identical to edt_slerp_merge on its two parents; then the rank's range of every
         child (edt_slerp_blend_children).
         EDT-LM: the rank's range of every child (edt_pair_merge_population), nothing to gather;
      3. child shards -> children: the range of child c goes to rank c.

    Wire bytes per rank and generation: (N-1)/N x (member + child) (+ the donor momenta for
    EDT-LM), spread over all N-1 links, against up to two whole members over one or two links.
    Reference: EDT_RL/edt.py:286-299 (the master merges pair after pair), EDT_EVOMERGE/edt.py:262-280.
    A rank's range starts at a multiple of 8 elements below its first chunk (<= 7 elements shared
    with the previous rank), so every chunk keeps its vector alignment and hence its sums.

    groups > 1 (SLERP): every rank's range is cut into that many groups of whole chunks and the
    exchanges run per group, all of a phase's groups in flight at once: the Gram pass of group g
    starts as soon as g's member slices have landed (while later groups are still on the links),
    and group g of the children leaves as soon as its blend is done (while later groups blend).
    Same bytes, same kernels on the same chunks: the children are bit-identical to groups = 1."""

    def __init__(self, layout: ParamLayout, dtype: torch.dtype, device, kind: str = "slerp",
                 out_dtype: torch.dtype | None = None, comm: Collectives | None = None, group=None,
                 kernels=None, chunk_elems: int = 1 << 16, groups: int = 1):
        if kind not in ("slerp", "sgd"):
            raise ValueError(kind)
        self.comm = comm or TorchCollectives(group)
        self.world, self.rank = self.comm.world, self.comm.rank
        if self.world > 8 and kind == "slerp":
            raise ValueError("the Gram pass takes at most 8 members (one per rank)")
        if self.world > 16:
            raise ValueError("at most 16 children per launch")
        self.kind, self.layout, self.device = kind, layout, torch.device(device)
        self.dtype, self.out_dtype = dtype, out_dtype or dtype
        self.kernels = kernels or _ops
        self.plan = self.kernels.make_slerp_plan(layout.offsets, self.device, chunk_elems=chunk_elems)
        host = np.asarray(self.plan.chunks_host, dtype=np.int64).reshape(-1, 3)
        n, N = layout.total, self.world
        starts = host[:, 0] if len(host) else np.zeros(0, dtype=np.int64)
        cuts = [0] + [int(np.searchsorted(starts, (r * n) // N, side="left")) for r in range(1, N)] + [len(host)]
        self.ranges = []           # per rank: (first chunk, end chunk, base, start, end) in elements
        for r in range(N):
            c0, c1 = cuts[r], max(cuts[r], cuts[r + 1])
            if c1 > c0:
                start, end = int(host[c0, 0]), int(host[c1 - 1, 0] + host[c1 - 1, 1])
            else:
                start = end = int(host[c0, 0]) if c0 < len(host) else n
            self.ranges.append((c0, c1, start // 8 * 8, start, end))
        if groups < 1:
            raise ValueError(groups)
        # per rank: its chunk range in `groups` contiguous groups (fewer when it has fewer chunks),
        # each (first chunk, end chunk, lo, hi) with [lo, hi) the elements a group carries: the
        # first group from the rank's aligned base, the others from their first chunk's start
        self.granges = []
        for r in range(N):
            a, b, rbase = self.ranges[r][0], self.ranges[r][1], self.ranges[r][2]
            G = min(groups, b - a)
            gl = []
            for g in range(G):
                g0, g1 = a + (b - a) * g // G, a + (b - a) * (g + 1) // G
                lo = rbase if g == 0 else int(host[g0, 0])
                gl.append((g0, g1, lo, int(host[g1 - 1, 0] + host[g1 - 1, 1])))
            self.granges.append(gl)
        self.groups = groups
        c0, c1, base, start, end = self.ranges[self.rank]
        self.nloc = c1 - c0
        self.base, self.start, self.end = base, start, end
        loc = host[c0:c1].copy()
        loc[:, 0] -= base
        self.local_chunks = torch.from_numpy(loc).to(self.device) if self.device.type == "cuda" else torch.from_numpy(loc)
        L = end - base
        self._shard_len = max(L, 8)     # no closure over self: the buffers go with the object
        self._bufs = {}

    def _buf(self, key, dt):
        if key not in self._bufs:
            self._bufs[key] = torch.empty(self._shard_len, dtype=dt, device=self.device)
        return self._bufs[key]

    def _scatter(self, tensors, tag):
        """Every rank's tensors -> this rank's range of each: {tag, j: buffer of rank j's tensor}."""
        ops_, got = [], {}
        L = self.end - self.base
        for s in range(self.world):
            _, _, b, _, e = self.ranges[s]
            if s != self.rank and e > b:
                for i, t in enumerate(tensors):
                    ops_.append(("send", t[b:e], s))
        for j in range(self.world):
            bufs = [self._buf((tag, i, j), t.dtype) for i, t in enumerate(tensors)]
            got[j] = [bb[:L] for bb in bufs]
            if j == self.rank:
                for bb, t in zip(got[j], tensors):
                    bb.copy_(t[self.base:self.end])
            elif L > 0:
                ops_.extend(("recv", bb, j) for bb in got[j])
        self.comm.p2p(ops_)
        return got

    def _gather_children(self, shards, outs):
        """Child q's range from every rank into outs (this rank's child): shards[q] = this rank's
        range of child q (buffers of base..end); outs = this rank's child tensors."""
        ops_ = []
        off = self.start - self.base
        for q in range(self.world):
            for sh, out in zip(shards[q], outs):
                if q == self.rank:
                    out[self.start:self.end].copy_(sh[off:self.end - self.base])
                elif self.end > self.start:
                    ops_.append(("send", sh[off:self.end - self.base], q))
        for j in range(self.world):
            _, _, _, st, en = self.ranges[j]
            if j != self.rank and en > st:
                ops_.extend(("recv", out[st:en], j) for out in outs)
        self.comm.p2p(ops_)

    def _scatter_groups(self, member, tag):
        """_scatter of one tensor, one grouped exchange per chunk group, all issued at once.
        Returns (buffers per rank j, one handle per group)."""
        L = self.end - self.base
        got = {j: self._buf((tag, 0, j), member.dtype)[:L] for j in range(self.world)}
        mine = self.granges[self.rank]
        handles = []
        for g in range(self.groups):
            ops_ = []
            for s_ in range(self.world):
                if s_ != self.rank and g < len(self.granges[s_]):
                    _, _, lo, hi = self.granges[s_][g]
                    ops_.append(("send", member[lo:hi], s_))
            if g < len(mine):
                _, _, lo, hi = mine[g]
                ops_.extend(("recv", got[j][lo - self.base:hi - self.base], j)
                            for j in range(self.world) if j != self.rank)
            handles.append(self.comm.p2p(ops_, async_op=True))
        got[self.rank].copy_(member[self.base:self.end])
        return got, handles

    def _gather_group(self, g, outs, out):
        """Group g of this rank's range of every child q to rank q, and group g of every other
        rank's range of this rank's child into `out` (issued, not waited)."""
        ops_ = []
        mine = self.granges[self.rank]
        if g < len(mine):
            _, _, lo, hi = mine[g]
            lo = max(lo, self.start)
            for q in range(self.world):
                if q == self.rank:
                    out[lo:hi].copy_(outs[q][lo - self.base:hi - self.base])
                else:
                    ops_.append(("send", outs[q][lo - self.base:hi - self.base], q))
        for j in range(self.world):
            if j != self.rank and g < len(self.granges[j]):
                _, _, lo, hi = self.granges[j][g]
                lo = max(lo, self.ranges[j][3])
                ops_.append(("recv", out[lo:hi], j))
        return self.comm.p2p(ops_, async_op=True)

    def _reference_dots(self, members, pairs, t, dots, dot_threshold, eps, ref):
        """Reference-dot mode of the sharded generation (ops.RefDot): the reference's fp32 dot of
        every flagged (child, segment) — the BLAS sdot chains and numpy's pairwise sum run over the
        WHOLE segment in order, so each segment is computed by the rank that holds its first chunk:
        from its own shards when the segment ends in its range, else after the later ranks send it
        the rest of that segment of the parents it needs (only segments that straddle a range
        boundary: at most N - 1). The values are all-gathered (host objects) and every rank forms
        the reference's coefficients of every child from them (ops.reference_coefficients): the
        children equal the reference's merges bit for bit with band < 0. Returns (coef [Q, nseg, 2],
        dots [Q, nseg]) on the device."""
        ref.check_host()
        k, N, Q = self.kernels, self.world, len(pairs)
        plan, nseg = self.plan, self.plan.nseg
        host = np.asarray(plan.chunks_host, dtype=np.int64).reshape(-1, 3)
        first = np.searchsorted(host[:, 2], np.arange(nseg + 1), side="left") if len(host) \
            else np.zeros(nseg + 1, dtype=np.int64)
        d = dots[:Q, :nseg].detach().cpu().numpy().astype(np.float32)
        if ref.band < 0:
            flag = np.ones((Q, nseg), dtype=bool)
        else:                               # refdot_flag_kernel's test, in fp32
            flag = np.abs(np.abs(d) - np.float32(dot_threshold)) <= np.float32(ref.band)
        flag &= (first[1:] > first[:-1])[None, :]          # segments with elements
        owner = np.full(nseg, -1, dtype=np.int64)
        for r in range(N):
            a, b = self.ranges[r][:2]
            owner[(first[:-1] >= a) & (first[:-1] < b)] = r
        c0, c1 = self.ranges[self.rank][:2]
        dt = members[0].dtype
        # 1. the rest of each straddling flagged segment to its owner (same op order on every rank)
        ops_, bufs = [], {}
        for s in range(nseg):
            r = int(owner[s])
            if r < 0 or not flag[:, s].any() or first[s + 1] <= self.ranges[r][1]:
                continue
            need = sorted({int(x) for q in range(Q) if flag[q, s] for x in pairs[q]})
            seg_lo = int(host[first[s], 0])
            seg_hi = int(host[first[s + 1] - 1, 0] + host[first[s + 1] - 1, 1])
            if r == self.rank:
                own_hi = int(host[c1 - 1, 0] + host[c1 - 1, 1])
                for m in need:
                    buf = bufs[(s, m)] = torch.empty(seg_hi - seg_lo, dtype=dt, device=self.device)
                    buf[:own_hi - seg_lo].copy_(members[m][seg_lo - self.base:own_hi - self.base])
            for j in range(N):
                if j == r:
                    continue
                ja, jb, jbase = self.ranges[j][:3]
                lo, hi = max(int(first[s]), ja), min(int(first[s + 1]), jb)
                if hi <= lo:
                    continue
                elo, ehi = int(host[lo, 0]), int(host[hi - 1, 0] + host[hi - 1, 1])
                for m in need:
                    if j == self.rank:
                        ops_.append(("send", members[m][elo - jbase:ehi - jbase], r))
                    elif r == self.rank:
                        ops_.append(("recv", bufs[(s, m)][elo - seg_lo:ehi - seg_lo], j))
        if ops_:
            self.comm.p2p(ops_)
        # 2. this rank's segments: whole ones from its shards (one pass per child), straddling ones
        #    from the assembled buffers
        mine = owner == self.rank
        whole = mine & (first[1:] <= c1)
        sf = torch.from_numpy(np.clip(first - c0, 0, max(0, c1 - c0)).astype(np.int32)).to(self.device)
        found = []
        for q, (i, j) in enumerate(pairs):
            fq = flag[q] & whole
            if fq.any():
                val = k.slerp_refdot(members[i], members[j], self.local_chunks, sf, nseg, plan.chunk_elems,
                                     torch.from_numpy(fq.astype(np.int32)).to(self.device), ref, eps)
                vh = val[:nseg].cpu().numpy()
                found.extend((q, int(s), float(vh[s])) for s in np.nonzero(fq)[0])
        for s in sorted({s for (s, _) in bufs}):
            seg_len = int(host[first[s + 1] - 1, 0] + host[first[s + 1] - 1, 1] - host[first[s], 0])
            ce = plan.chunk_elems
            rows = np.asarray([(x, min(ce, seg_len - x), 0) for x in range(0, seg_len, ce)], dtype=np.int64)
            ch = torch.from_numpy(rows).to(self.device)
            sf1 = torch.tensor([0, len(rows)], dtype=torch.int32).to(self.device)
            one = torch.ones(1, dtype=torch.int32).to(self.device)
            for q, (i, j) in enumerate(pairs):
                if flag[q, s]:
                    val = k.slerp_refdot(bufs[(s, i)], bufs[(s, j)], ch, sf1, 1, ce, one, ref, eps)
                    found.append((q, int(s), float(val[:1].cpu().numpy()[0])))
        # 3. every rank: all values, then the reference's coefficients of every child
        final = d.copy()
        for part in self.comm.all_gather_object(found):
            for q, s, v in part:
                final[q, s] = np.float32(v)
        from .ops import reference_coefficients
        coef = reference_coefficients(final, t[:nseg].detach().cpu().numpy(), dot_threshold)
        return torch.from_numpy(coef).to(self.device), torch.from_numpy(final).to(self.device)

    @traced("edt/ShardedPopulationCrossover.slerp_step")
    def slerp_step(self, member: torch.Tensor, pairs, t: torch.Tensor, out: torch.Tensor,
                   dot_threshold: float = 0.9995, eps: float = 1e-8, ref_dot=None) -> torch.Tensor:
        """Child pairs[rank] into `out`; returns the per-segment dots of every child [N, nseg].
        ref_dot (ops.RefDot): the reference-dot mode (_reference_dots; the groups > 1 pipeline is
        not used in that mode: the coefficients need every rank's values first)."""
        if len(pairs) != self.world:
            raise ValueError(f"{len(pairs)} children for {self.world} ranks")
        k, N = self.kernels, self.world
        layout = k.needed_table(pairs, N, self.plan.nchunks)
        table = self._bufs.get("needed")
        if table is None or table.numel() < max(1, layout.doubles):
            table = self._bufs["needed"] = torch.empty(max(1, layout.doubles), dtype=torch.float64, device=self.device)
        c0, c1 = self.ranges[self.rank][:2]
        mine = self.granges[self.rank]
        if self.groups > 1 and ref_dot is None:
            sh, handles = self._scatter_groups(member, "m")
            members = [sh[j] for j in range(N)]
            for g, h in enumerate(handles):
                h.wait()
                if g < len(mine):
                    g0, g1 = mine[g][0] - c0, mine[g][1] - c0
                    k.slerp_needed_sums(members, layout, self.local_chunks[g0:g1], g1 - g0, table, c0 + g0)
        else:
            sh = self._scatter([member], "m")
            members = [sh[j][0] for j in range(N)]
            if self.nloc:
                k.slerp_needed_sums(members, layout, self.local_chunks, self.nloc, table, c0)
        ops_ = []                       # all-gather of the table rows: every rank's chunk range, per block
        for b in range(len(layout.blocks)):
            for s in range(N):
                if s != self.rank and self.nloc:
                    ops_.append(("send", layout.rows(table, b, c0, c1), s))
            for j in range(N):
                ja, jb = self.ranges[j][:2]
                if j != self.rank and jb > ja:
                    ops_.append(("recv", layout.rows(table, b, ja, jb), j))
        self.comm.p2p(ops_)
        coef, dots = k.slerp_needed_coef(self.plan, table, layout, t, dot_threshold, eps)
        if ref_dot is not None:
            coef, dots = self._reference_dots(members, pairs, t, dots, dot_threshold, eps, ref_dot)
        outs = [self._buf(("c", q), self.out_dtype)[:self.end - self.base] for q in range(N)]
        if self.groups > 1 and ref_dot is None:
            handles = []
            for g in range(self.groups):
                if g < len(mine):
                    g0, g1 = mine[g][0] - c0, mine[g][1] - c0
                    k.slerp_blend_children(members, pairs, outs, self.local_chunks[g0:g1], g1 - g0, coef,
                                           self.plan.nseg)
                handles.append(self._gather_group(g, outs, out))
            for h in handles:
                h.wait()
            return dots
        if self.nloc:
            k.slerp_blend_children(members, pairs, outs, self.local_chunks, self.nloc, coef, self.plan.nseg)
        self._gather_children([[o] for o in outs], [out])
        return dots

    def pair_merge_step(self, base: torch.Tensor, trained: torch.Tensor, momentum: torch.Tensor | None,
                        pairs, out: torch.Tensor, out_momentum: torch.Tensor | None, lr: float = 0.7,
                        mu: float = 0.9, nesterov: bool = True, has_momentum: bool = True,
                        generation: int = 0) -> None:
        """EDT-LM child pairs[rank] into out / out_momentum (EDT_LM/train/crossover.py:150-237;
        donor = parent 1 when it has an outer momentum, else parent 2, as PopulationCrossover)."""
        if len(pairs) != self.world:
            raise ValueError(f"{len(pairs)} children for {self.world} ranks")
        # each rank's momentum flag and the dtypes its momentum buffers would travel in: every rank
        # sizes its p2p buffers from its own send list, so a dtype that differs across ranks would
        # post sends and receives of different byte counts — refused on every rank instead
        has = bool(has_momentum and momentum is not None)
        mdt = str(out_momentum.dtype) if out_momentum is not None else None
        info = self.comm.all_gather_object((has, mdt, str(momentum.dtype) if has else None))
        flags = [f for f, _, _ in info]
        donors = [i if flags[i] else (j if flags[j] else None) for i, j in pairs]
        if mu != 0 and generation > 0 and any(d is None for d in donors):
            raise NotImplementedError("Merging outer optimizer states not implemented for this case.")
        send_mom = any(d is not None for d in donors)      # some child inherits a buffer
        if send_mom and any(m is None for _, m, _ in info):     # on every rank, not just the one missing it
            raise ValueError("the child inherits an outer momentum: pass out_momentum on every rank")
        if send_mom and (len({m for _, m, _ in info}) != 1 or any(d not in (None, info[0][1]) for _, _, d in info)):
            raise EdtError(f"outer momentum dtypes differ across ranks or from the child's: {info}")
        with_mom = out_momentum is not None                # children write one (mu != 0)
        stand_in = (lambda: torch.zeros_like(base, dtype=out_momentum.dtype)) if send_mom else None
        send = [base, trained] + ([momentum if has else stand_in()] if send_mom else [])
        sh = self._scatter(send, "p")
        L = self.end - self.base
        children = []
        outs = [[self._buf(("c", q), self.out_dtype)[:L]] + ([self._buf(("cm", q), out_momentum.dtype)[:L]]
                                                             if with_mom else []) for q in range(self.world)]
        for q, (i, j) in enumerate(pairs):
            d = donors[q]
            children.append({"b1": sh[i][0], "b2": sh[j][0], "m1": sh[i][1], "m2": sh[j][1], "out": outs[q][0],
                             "momentum": outs[q][1] if with_mom else None,
                             "momentum_in": sh[d][2] if d is not None else None, "has_momentum": d is not None})
        if L > 0:
            self.kernels.pair_merge_population(children, lr, mu, nesterov)
        self._gather_children(outs, [out] + ([out_momentum] if with_mom else []))
