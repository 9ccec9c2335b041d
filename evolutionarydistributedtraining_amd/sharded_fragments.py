"""Streaming DiLoCo across ranks: the fragment-wise outer step, sharded, with the worker merge fused.

`OuterSync.step_fragment` steps one fragment of a `FragmentPlan` per outer step on one process.
`ShardedFragmentSync` does it across N ranks, so that only the stepped fragment — 1/P of the
parameters — crosses the links per outer step. One schedule, `ShardedOuterSync`'s reduce_ordered
(a fixed rank-order sum), run in FRAGMENT SPACE: fragment p's runs laid back to back, the layout of
its snapshots (`FragmentPlan.snapshot_views`).

  F_p = plan.numel(p), F_pad = F_p rounded up to a multiple of world * 64; fragment space is cut into
  buckets by ShardedOuterSync's rule (multiples of world * 64, at most bucket_elems) and rank r owns
  the r-th slice of every bucket, per = (e - b) / world elements. A shard's bounds cut runs in the
  middle, so every kernel runs over the PIECES of a fragment-space range (`FragmentPlan.pieces`):
  views into the arenas at the pieces' arena offsets, views into the compact buffers at their
  fragment-space offsets. Nothing is packed.

  phase 1  per bucket: edt_delta_partial_list over the bucket's pieces — the local workers' fp32
           partial (from the live arenas, or from fragment-space snapshots) into the compact send
           buffer, which in fragment-space order IS the [dest rank][per] layout — then an all-to-all
           of the compact partial. All buckets are produced before the first wait.
  phase 2  per bucket, once its all-to-all has landed: edt_sgd_sum_list_to over the owned shard's
           pieces — the N received partials summed in rank order, torch's SGD update with the owned
           slice of the fragment's momentum; theta is only read, the new theta goes into this rank's
           slot of the compact gather buffer — then an all-gather of the compact theta.
  phase 3  as each gather lands: edt_theta_scatter_mix_list over the bucket's pieces — the gathered
           theta into theta's pieces and, with merge=True, into every local worker arena's pieces as
           w <- lerp(mix, w, theta_new) in the worker dtype (Streaming DiLoCo's alpha is 1 - mix).
           The same kernel runs on the same bytes on every rank: the replicas stay bit-identical.

Per rank: a full theta replica, K_local worker arenas (unpadded), and per fragment 1/N of its
momentum in fragment space (F_pad / N elements; the pad elements are never written). Nothing outside
fragment p is read or written by its step.

Quantized exchange (wire_format="mxfp8" | "mxfp4": Streaming DiLoCo's low-precision outer gradients).
The partial crosses the links as OCP MX regions (ShardedOuterSync's reduce_q wire format, DESIGN §3:
1.03 / 0.53 B per element instead of 4) with error feedback:

  The unit of fragment space is world * 512 instead of world * 64, so every rank's region of every
  bucket is whole 512-element waves; F_pad, the buckets and the momentum shards follow from it.
  `send` / `recv` are uint8: a bucket [b, e) holds `world` regions of (e - b) / world elements,
  [dest rank][payload | scales], at byte b * (bits / 8 + 1 / 32).
  phase 1  per bucket: edt_delta_partial_q_frag over the bucket's pieces — the same fp32 partial,
           gathered through the piece table in fragment space, + residual[p], quantized in registers
           (the fp32 partial never reaches HBM), the new residual stored — then the all-to-all of
           the packed bytes. All buckets before the first wait, as above.
  phase 2  edt_sgd_sum_q_frag_to over the owned shard: the N received regions dequantized and
           summed in rank order, the same SGD update; the new theta into the gather buffer (zero on
           the padding). The all-gather of theta in theta's dtype and phase 3 are unchanged.
  residual[p] (error_feedback=True): F_pad fp32 elements per fragment on this rank, in fragment
  space, zero at the start; what the quantization of this rank's partial lost and adds back at the
  fragment's next step. It is NOT checkpointed, by ShardedOuterSync.residual's rule: a restart
  loses at most one step's quantization error per fragment.

Not here, and not planned by this module: guard= (the statistics, screening and clip of
ShardedOuterSync), a quantized gather of theta' for fragments, stochastic rounding, cpu_tails, the
exact and reduce schedules, the C schedules of edt_comm.cpp, and bucket sizes tuned for xGMI.
"""
from __future__ import annotations

import math

import torch

from . import ops as _ops
from ._lib import EDT_MAX_WORKERS, EdtError
from .collectives import Collectives, TorchCollectives
from .diloco import OuterState, check_sgd_hparams
from .fragments import FragmentPlan
from .params import ParamArena, ParamLayout
from .tracing import traced

KERNEL_NAMES = ("delta_partial_list", "sgd_sum_list_to", "theta_scatter_mix_list")
# with a wire format, phases 1 and 2 are these two instead; phase 3 stays theta_scatter_mix_list
Q_KERNEL_NAMES = ("delta_partial_q_frag", "sgd_sum_q_frag_to", "theta_scatter_mix_list")
WIRE_BITS = {"mxfp8": 8, "mxfp4": 4}


class ShardedFragmentSync:
    def __init__(self, layout: ParamLayout, plan: FragmentPlan, theta_dtype: torch.dtype, worker_dtype: torch.dtype,
                 k_local: int, device, lr: float = 0.7, momentum: float = 0.9, nesterov: bool = True,
                 bucket_elems: int = 1 << 26, group=None, kernels=None, comm: Collectives | None = None,
                 wire_format: str | None = None, error_feedback: bool = True):
        check_sgd_hparams(lr, momentum, nesterov)
        if plan.layout.numels != layout.numels:
            raise EdtError("the fragment plan does not match the layout")
        if wire_format is not None and wire_format not in WIRE_BITS:
            raise EdtError(f"unknown wire format {wire_format!r}: None, 'mxfp8' or 'mxfp4'")
        self.wire_format = wire_format
        self.kernels = kernels or _ops
        names = KERNEL_NAMES if wire_format is None else Q_KERNEL_NAMES
        missing = [m for m in names if not hasattr(self.kernels, m)]
        if missing:
            raise EdtError(f"the sharded fragment step needs kernels that provide {list(names)}; "
                           f"{getattr(self.kernels, '__name__', type(self.kernels).__name__)} lacks {missing}")
        # the communicator seam: torch.distributed (RCCL / gloo) by default, or N virtual ranks on
        # one device (collectives.VirtualWorld)
        self.comm = comm or TorchCollectives(group)
        self.world, self.rank = self.comm.world, self.comm.rank
        if k_local < 1 or k_local * self.world > EDT_MAX_WORKERS:
            raise EdtError(f"a sharded fragment step takes 1 to {EDT_MAX_WORKERS} workers in all, not "
                           f"{k_local} x {self.world}")
        self.layout, self.plan = layout, plan
        self.lr, self.momentum, self.nesterov = lr, momentum, nesterov
        self.k_local, self.k_total = k_local, k_local * self.world
        self.inplace = self.comm.inplace
        self.theta = ParamArena(layout, theta_dtype, device, torch.zeros(layout.total, dtype=theta_dtype, device=device))
        self.workers = [ParamArena(layout, worker_dtype, device, torch.zeros(layout.total, dtype=worker_dtype, device=device))
                        for _ in range(k_local)]
        # fragment space: buckets of multiples of world * 64 elements, so every shard starts on a
        # 16-byte boundary of the compact buffers; with a wire format world * 512, so every rank's
        # region is whole 512-element waves of the quantizing kernels
        unit = self.world * (64 if wire_format is None else 512)
        bucket = max(unit, bucket_elems // unit * unit)
        self.f_pad = [math.ceil(plan.numel(p) / unit) * unit for p in range(len(plan))]
        self.buckets = [[(b, min(b + bucket, fp)) for b in range(0, fp, bucket)] for fp in self.f_pad]
        self.mom = ([torch.zeros(fp // self.world, dtype=theta_dtype, device=device) for fp in self.f_pad]
                    if momentum else None)
        # compact exchange buffers in fragment space, sized for the largest fragment: a bucket [b, e)
        # of `send` is [dest rank][per], of `recv` and `gathered` [src rank][per]
        top = max(self.f_pad)
        if wire_format is None:
            self.send = torch.zeros(top, dtype=torch.float32, device=device)
            self.recv = torch.zeros(top, dtype=torch.float32, device=device)
            self.residual = None
        else:
            # packed: a bucket's `world` regions back to back start at byte _qbytes(b)
            self.send = torch.zeros(self._qbytes(top), dtype=torch.uint8, device=device)
            self.recv = torch.zeros(self._qbytes(top), dtype=torch.uint8, device=device)
            # error feedback: per fragment, this rank's quantization error in fragment space (the
            # padding stays zero); not checkpointed (module docstring)
            self.residual = ([torch.zeros(fp, dtype=torch.float32, device=device) for fp in self.f_pad]
                             if error_feedback else None)
        self.gathered = torch.zeros(top, dtype=theta_dtype, device=device)
        # OuterState's per-fragment semantics: a fragment's first step takes buf = grad
        self.fragment_has_momentum = [False] * len(plan)
        self.fragment_steps = [0] * len(plan)
        self.steps = 0

    # ---------------------------------------------------------------------------------------
    def _shard(self, b: int, e: int) -> tuple[int, int]:
        per = (e - b) // self.world
        return b + self.rank * per, b + (self.rank + 1) * per

    def _owned(self, p: int):
        """Per bucket (b, e) of fragment p: the owned shard [s0, s1) of fragment space and where
        its momentum starts in mom[p]."""
        off = 0
        for b, e in self.buckets[p]:
            s0, s1 = self._shard(b, e)
            yield b, e, s0, s1, off
            off += s1 - s0

    def _qbytes(self, elems: int) -> int:
        """Packed bytes of `elems` elements (a multiple of 512) as whole regions: payload + one scale
        byte per 32 — linear in the elements, so also the byte offset of fragment-space element
        `elems` in `send` / `recv`."""
        return elems * WIRE_BITS[self.wire_format] // 8 + elems // 32

    def _check_fragment(self, p: int) -> None:
        if not 0 <= p < len(self.plan):
            raise EdtError(f"fragment {p} out of range [0, {len(self.plan)})")

    def capture_fragment(self, p: int, out: list[torch.Tensor] | None = None) -> list[torch.Tensor]:
        """Snapshots of fragment p of every local worker arena for a later `step_fragment(p,
        snapshots=...)`: K_local flat buffers of the fragment's size in the workers' dtype, its runs
        back to back (`OuterSync.capture_fragment`'s layout). out: buffers to reuse."""
        self._check_fragment(p)
        n = self.plan.numel(p)
        if out is None:
            out = [torch.empty(n, dtype=w.flat.dtype, device=w.flat.device) for w in self.workers]
        self._check_snapshots(p, out)
        for o, w in zip(out, self.workers):
            for dst, src in zip(self.plan.snapshot_views(p, o), self.plan.views(p, w.flat)):
                dst.copy_(src)
        return out

    def _check_snapshots(self, p: int, snapshots) -> None:
        n, wdt = self.plan.numel(p), self.workers[0].flat.dtype
        if len(snapshots) != len(self.workers) or any(s.numel() != n or s.dtype != wdt or s.dim() != 1
                                                      for s in snapshots):
            raise EdtError("snapshots: one flat buffer of the fragment's size and the workers' dtype per worker")

    @traced("edt/ShardedFragmentSync.step_fragment")
    def step_fragment(self, p: int, mix: float = 1.0, snapshots: list[torch.Tensor] | None = None,
                      merge: bool = True) -> None:
        """One outer step of fragment p alone across the ranks; returns when the work is enqueued.
        snapshots: K_local fragment-space buffers (`capture_fragment(p)`) the pseudo-gradient is taken
        from; None: the live worker arenas. merge=True: every local worker's fragment becomes
        lerp(mix, w, theta_new) in the worker dtype (mix = 1 overwrites); merge=False steps theta
        and the momentum only. Every refusal comes before any collective is issued.

        Stream hazards: phase 1 of every bucket is enqueued before any phase-3 store into the arenas
        it read, on the same stream; every collective is waited for before its buffers are consumed,
        and all of them before this returns, so the next step may reuse the compact buffers."""
        self._check_fragment(p)
        mix = float(mix)
        if not 0.0 < mix <= 1.0:                    # NaN fails both comparisons
            raise EdtError(f"mix {mix} outside (0, 1]")
        if snapshots is not None:
            self._check_snapshots(p, snapshots)
        k, plan = self.kernels, self.plan
        theta = self.theta.flat
        has = self.fragment_has_momentum[p] if self.momentum != 0 else False

        def cut(buf, pieces, arena):
            """The pieces' views of `buf`: at their arena offsets, or at their fragment-space ones."""
            return [buf[a:a + n] if arena else buf[f:f + n] for a, f, n in pieces]

        fmt = self.wire_format
        works = []
        for b, e in self.buckets[p]:                # phase 1: every bucket before the first wait
            pc = plan.pieces(p, b, e)
            deltas = ([cut(w.flat, pc, True) for w in self.workers] if snapshots is None
                      else [cut(s, pc, False) for s in snapshots])
            if fmt is not None:
                # a bucket that is all padding is still quantized: its regions are sent like any other
                q0, q1 = self._qbytes(b), self._qbytes(e)
                k.delta_partial_q_frag(cut(theta, pc, True), deltas, self.k_total, [f for _, f, _ in pc], b,
                                       self.send[q0:q1], (e - b) // self.world, fmt,
                                       None if self.residual is None else self.residual[p][b:e])
                works.append(self.comm.all_to_all(self.recv[q0:q1], self.send[q0:q1], async_op=True))
                continue
            if pc:
                k.delta_partial_list(cut(theta, pc, True), deltas, self.k_total, cut(self.send, pc, False))
            works.append(self.comm.all_to_all(self.recv[b:e], self.send[b:e], async_op=True))
        gathers = []
        for (b, e, s0, s1, moff), w in zip(self._owned(p), works):      # phase 2 on the owned shard
            w.wait()
            pc = plan.pieces(p, s0, s1)
            per = s1 - s0
            if fmt is not None:
                q0, rb = self._qbytes(b), self._qbytes(per)
                regions = [self.recv[q0 + r * rb:q0 + (r + 1) * rb] for r in range(self.world)]
                k.sgd_sum_q_frag_to(cut(theta, pc, True), [f for _, f, _ in pc], s0, regions, fmt,
                                    None if self.mom is None else self.mom[p][moff:moff + per], has, self.lr,
                                    self.momentum, self.nesterov, self.gathered[s0:s1])
            elif pc:
                parts = [[self.recv[b + r * per + f - s0:b + r * per + f - s0 + n] for _, f, n in pc]
                         for r in range(self.world)]
                moms = None if self.mom is None else [self.mom[p][moff + f - s0:moff + f - s0 + n] for _, f, n in pc]
                k.sgd_sum_list_to(cut(theta, pc, True), parts, moms, has, self.lr, self.momentum, self.nesterov,
                                  cut(self.gathered, pc, False))
            src = self.gathered[s0:s1] if self.inplace else self.gathered[s0:s1].clone()
            gathers.append(self.comm.all_gather(self.gathered[b:e], src, async_op=True))
        for (b, e), g in zip(self.buckets[p], gathers):                  # phase 3 as each gather lands
            g.wait()
            pc = plan.pieces(p, b, e)
            if pc:
                live = [cut(w.flat, pc, True) for w in self.workers] if merge else []
                k.theta_scatter_mix_list(cut(theta, pc, True), cut(self.gathered, pc, False), live, mix)
        if self.momentum != 0:
            self.fragment_has_momentum[p] = True
        self.fragment_steps[p] += 1
        self.steps += 1

    # ---------------------------------------------------------------------------------------
    def _owned_elems(self, p: int) -> int:
        return sum(n for _, _, s0, s1, _ in self._owned(p) for _, _, n in self.plan.pieces(p, s0, s1))

    def wire_bytes(self, p: int) -> int:
        """Bytes this rank sends per step of fragment p (all-to-all / all-gather lower bound):
        (N - 1) / N * F_pad * (4 + b_g) — the fp32 partials out, theta's dtype back. With a wire
        format the partial costs bits / 8 + 1 / 32 bytes per element instead of 4 (F_pad is then a
        multiple of world * 512). Computed from byte counts, not measured on a multi-GPU node."""
        f = (self.world - 1) / self.world
        return int(f * self.f_pad[p] * (self._partial_bytes() + self.theta.flat.element_size()))

    def _partial_bytes(self) -> float:
        """Bytes per element of the partial as it is exchanged: 4 (fp32), or the payload plus one
        scale byte per 32 elements."""
        return 4 if self.wire_format is None else WIRE_BITS[self.wire_format] / 8 + 1 / 32

    def kernel_bytes(self, p: int, merge: bool = True, mix: float = 1.0) -> int:
        """Algorithmic HBM bytes of the three kernels of one step of fragment p on this rank, steady
        state (the fragment's momentum carried), F = F_p, O = this rank's owned elements of it:
          phase 1  F * (K_local * b_w  the workers' pieces read
                        + b_g          theta's pieces read
                        + 4)           the fp32 partial written
          phase 2  O * (N * 4          the N received partials read
                        + b_g          theta's pieces read
                        + b_g          the new theta written to the gather buffer
                        + 2 * b_g)     the momentum read and written (0 without momentum)
          phase 3  F * (b_g            the gathered theta read
                        + b_g          theta's pieces written
                        + K_local * b_w                 the workers' pieces written (merge)
                        + K_local * b_w)                and read first (merge with mix < 1)
        With a wire format, q = bits / 8 + 1 / 32: phase 1 writes q instead of 4, plus 8 with error
        feedback (the residual read and written); phase 2 reads N * q instead of N * 4."""
        F, O = self.plan.numel(p), self._owned_elems(p)
        bg, bw = self.theta.flat.element_size(), self.workers[0].flat.element_size()
        q = self._partial_bytes()
        p1 = F * (self.k_local * bw + bg + q + (8 if self.residual is not None else 0))
        p2 = O * (self.world * q + 2 * bg + (2 * bg if self.momentum else 0))
        p3 = F * (2 * bg + (self.k_local * bw * (1 if mix == 1.0 else 2) if merge else 0))
        return int(p1 + p2 + p3)

    # ---------------------------------------------------------------------------------------
    # checkpoint bridge (cold path)

    def gather_state(self) -> OuterState:
        """The whole outer-optimiser state on every rank, as a single-process fragment-wise run
        would hold it: the momentum shards all-gathered into one flat arena-order buffer (zeros
        where a fragment has not stepped), the per-fragment flags and counters, the plan attached —
        `OuterState.save(path, layout)` then writes what `OuterSync`'s state would. Collective:
        every rank calls it."""
        st = OuterState()
        st.hparams = dict(lr=self.lr, momentum=self.momentum, nesterov=self.nesterov)
        st.fragments = self.plan
        st.fragment_has_momentum = list(self.fragment_has_momentum)
        st.fragment_steps = list(self.fragment_steps)
        st.steps = self.steps
        st.has_momentum = self.momentum != 0 and all(self.fragment_has_momentum)
        if self.mom is None:
            return st
        flat = torch.zeros(self.layout.total, dtype=self.theta.flat.dtype, device=self.theta.flat.device)
        for p in range(len(self.plan)):
            full = torch.zeros(self.f_pad[p], dtype=flat.dtype, device=flat.device)
            for b, e, s0, s1, off in self._owned(p):
                full[s0:s1].copy_(self.mom[p][off:off + s1 - s0])
                self.comm.all_gather(full[b:e], full[s0:s1] if self.inplace else full[s0:s1].clone())
            for a, f, n in self.plan.pieces(p, 0, self.f_pad[p]):
                flat[a:a + n].copy_(full[f:f + n])
        st.momentum = flat
        return st

    def load_state(self, state: OuterState) -> None:
        """Scatter an `OuterState` (from `gather_state`, or `OuterState.load(..., fragments=plan)`)
        back: every rank keeps its shards of each fragment's momentum, the flags and the counters.
        A state that has stepped as a whole carries its momentum into every fragment."""
        P = len(self.plan)
        flags = state.fragment_has_momentum
        if flags is None:
            flags = [bool(state.has_momentum)] * P
        if len(flags) != P:
            raise EdtError("the state's fragments do not match the plan")
        if self.mom is not None and any(flags):
            if state.momentum is None or state.momentum.numel() != self.layout.total:
                raise EdtError("outer-optimizer state does not match the parameter count")
            src = state.momentum.to(dtype=self.theta.flat.dtype, device=self.theta.flat.device)
            for p in range(P):
                full = torch.zeros(self.f_pad[p], dtype=src.dtype, device=src.device)
                for a, f, n in self.plan.pieces(p, 0, self.f_pad[p]):
                    full[f:f + n].copy_(src[a:a + n])
                for _, _, s0, s1, off in self._owned(p):
                    self.mom[p][off:off + s1 - s0].copy_(full[s0:s1])
        elif self.mom is not None:
            for m in self.mom:
                m.zero_()
        self.fragment_has_momentum = [bool(f) and self.momentum != 0 for f in flags]
        self.fragment_steps = list(state.fragment_steps) if state.fragment_steps is not None else [0] * P
        self.steps = int(state.steps)
