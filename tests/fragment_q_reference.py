"""The quantized sharded fragment step (ShardedFragmentSync with wire_format=) restated in one
process, and what its CPU and GPU tests share. Built on tests/fragment_shard_reference.py (the layout,
the plans, the populations, pack / unpack) and tests/quant_reference.py (the wire format in numpy).

`QShardRun` is the composition the schedule must equal bit for bit: per rank the partial of its local
workers over the PACKED, ZERO-PADDED fragment (fragment space up to F_pad, a multiple of world * 512),
quantized with the rank's residual of that fragment (error feedback); the dequantized partials summed
in rank order, one SGD step on the packed theta and momentum, unpacked; then the merge per worker. Its
quantized arithmetic is handed in as an object with the two FLAT entries' names (`delta_partial_q`,
`sgd_apply_sum_q`): `quant_reference.NumpyQuantKernels` on the CPU, `ops` itself — the existing flat
HIP kernels — on the GPU. Blocks of 32 never straddle a region (every bound is a multiple of 512), so
the codes do not depend on how fragment space is cut into regions: the composition uses one region.
`PieceQuantKernels` is the kernels= stand-in for the two fragment-space entries.
"""
from __future__ import annotations

import math

import torch

from tests import fragment_shard_reference as R
from tests import quant_reference as Q
from tests.fragment_shard_reference import bits

FORMATS = ["mxfp8", "mxfp4"]


def unit(world: int) -> int:
    return world * 512


def bucket_elems(world: int, plan_name: str) -> int:
    """explicit: one unit, so every larger fragment has many buckets; strided: two units, so the larger
    fragment has 3 or more buckets and its last one is shorter (another region size)."""
    return unit(world) * (1 if plan_name == "explicit" else 2)


def f_pad(plan, p: int, world: int) -> int:
    return math.ceil(plan.numel(p) / unit(world)) * unit(world)


def lane_paths(pieces, lo: int, hi: int, operands) -> tuple[int, int]:
    """How many lanes of the range [lo, hi) of fragment space take the vector loads and how many
    gather, by the kernels' rule: a lane's 8 elements (at a multiple of 8) lie inside one piece and
    every arena operand's address for them is 16-byte aligned. pieces: FragmentPlan.pieces' (arena
    offset, fragment-space offset, numel); operands: (base address in bytes, element size, True: the
    operand is indexed by arena offset, False: by fragment-space offset) per arena operand."""
    vec = 0
    for i in range(lo, hi, 8):
        hit = next(((a, f) for a, f, n in pieces if f <= i and i + 8 <= f + n), None)
        if hit is not None and all((base + (hit[0] + i - hit[1] if arena else i) * size) % 16 == 0
                                   for base, size, arena in operands):
            vec += 1
    return vec, (hi - lo) // 8 - vec


class PieceQuantKernels(R.PieceOracleKernels):
    """kernels= stand-in for ShardedFragmentSync with a wire format: the two fragment-space entries
    in numpy — the oracle's partial and SGD per piece, quant_reference's ef_step / pack / unpack /
    dequantize between them, over the padded range — and PieceOracleKernels' phase 3."""

    def delta_partial_q_frag(self, thetas, workers, k_total, starts, lo, packed, region_elems, fmt, residual=None):
        self.calls.append("delta_partial_q_frag")
        n = packed.numel() // Q.region_bytes(region_elems, fmt) * region_elems
        acc = torch.zeros(n, dtype=torch.float32)                # what no piece covers: +0
        for t, th in enumerate(thetas):
            f = starts[t] - lo
            self.a.partial(th, [w[t] for w in workers], k_total, acc[f:f + th.numel()])
        codes, scales, _, new = Q.ef_step(acc.numpy(), None if residual is None else residual.numpy(), fmt)
        if residual is not None:
            residual.copy_(torch.from_numpy(new))
        packed.copy_(torch.from_numpy(Q.pack(codes, scales, fmt, region_elems)))

    def sgd_sum_q_frag_to(self, thetas, starts, lo, regions, fmt, momentum, has, lr, mu, nesterov, out):
        self.calls.append("sgd_sum_q_frag_to")
        n = out.numel()
        total = None
        for reg in regions:
            d = torch.from_numpy(Q.dequantize(*Q.unpack(reg.numpy(), fmt, n), fmt))
            total = d if total is None else total.add_(d)
        out.zero_()                                              # the padding's slots are zeroed
        for t, th in enumerate(thetas):
            f, m = starts[t] - lo, th.numel()
            new = th.clone()                                     # theta is only read
            self.a.o.sgd_apply(new, total[f:f + m].clone(), None if momentum is None else momentum[f:f + m], has, lr, mu,
                               nesterov)
            out[f:f + m].copy_(new)


class QShardRun(R.ShardRun):
    """The single-process composition. workers[r][j]: rank r's local worker j (arena-sized); qk: the
    flat quantized entries (delta_partial_q, sgd_apply_sum_q); arith: merge (R.OracleArith / GpuArith)."""

    def __init__(self, plan, theta, workers, qk, arith, lr, mu, nesterov, fmt, error_feedback=True):
        super().__init__(plan, theta, workers, arith, lr, mu, nesterov)
        self.qk, self.fmt = qk, fmt
        world = len(workers)
        self.f_pad = [f_pad(plan, p, world) for p in range(len(plan))]
        self.residual = ([[torch.zeros(fp, dtype=torch.float32, device=theta.device) for fp in self.f_pad]
                          for _ in range(world)] if error_feedback else None)

    def step(self, p, mix=1.0, snapshots=None, merge=True):
        plan, fp, F = self.plan, self.f_pad[p], self.plan.numel(p)

        def pad(x):
            out = torch.zeros(fp, dtype=x.dtype, device=x.device)
            out[:x.numel()] = x
            return out

        if fp:
            th = pad(R.pack(plan, p, self.theta))
            k_total = sum(len(ws) for ws in self.workers)
            regions = []
            for r, ws in enumerate(self.workers):
                deltas = [pad(R.pack(plan, p, w)) for w in ws] if snapshots is None else [pad(s) for s in snapshots[r]]
                packed = torch.zeros(Q.region_bytes(fp, self.fmt), dtype=torch.uint8, device=th.device)
                self.qk.delta_partial_q(th, deltas, k_total, packed, fp, self.fmt,
                                        None if self.residual is None else self.residual[r][p])
                regions.append(packed)
            mom = pad(R.pack(plan, p, self.mom)) if self.mu != 0 else None
            self.qk.sgd_apply_sum_q(th, regions, self.fmt, mom, self.has[p], self.lr, self.mu, self.nesterov)
            R.unpack_(plan, p, self.theta, th[:F])
            if mom is not None:
                R.unpack_(plan, p, self.mom, mom[:F])
            if merge:
                for ws in self.workers:
                    for w in ws:
                        live = R.pack(plan, p, w)
                        self.arith.merge(live, th[:F], mix)
                        R.unpack_(plan, p, w, live)
        if self.mu != 0:
            self.has[p] = True


def drive_q(vw, make_sync, plan, theta0, workers0, qk, arith, fmt, error_feedback=True, lr=0.7, mu=0.9, nesterov=True,
            steps=None):
    """fragment_shard_reference.drive for the quantized step: runs `steps` (default: schedule_steps)
    on the virtual world and on QShardRun, checking after every step and on every rank, bit for bit:
    theta, the gathered momentum and every local worker against the composition; every fragment's
    residual on this rank against the composition's for that rank, its padding still zero; and —
    through NaN canaries in every element outside the stepped fragment of theta and the workers, in
    the other fragments' momentum and in the stepped fragment's momentum padding — that nothing else
    was touched. Returns the syncs (rank order) and the composition."""
    world = vw.world
    k_local = len(workers0) // world
    per_rank = [workers0[r * k_local:(r + 1) * k_local] for r in range(world)]
    steps = steps if steps is not None else R.schedule_steps(len(plan))
    ref = QShardRun(plan, theta0, per_rank, qk, arith, lr, mu, nesterov, fmt, error_feedback)
    want, seed = [], 1000
    for p, mix, snap in steps:
        snaps = [[R.pack(plan, p, w) for w in ws] for ws in ref.workers] if snap else None
        for ws in ref.workers:                       # the workers train on after the snapshot
            for j in range(len(ws)):
                seed += 1
                ws[j] = R.drift(ws[j], seed)
        loaded = [[w.clone() for w in ws] for ws in ref.workers]
        ref.step(p, mix, snaps)
        want.append({"loaded": loaded, "snaps": snaps, "theta": ref.theta.clone(), "mom": ref.mom.clone(),
                     "workers": [[w.clone() for w in ws] for ws in ref.workers],
                     "residual": None if ref.residual is None else [[x.clone() for x in rs] for rs in ref.residual]})

    def body(comm):
        s = make_sync(comm)
        r = comm.rank
        assert s.f_pad == ref.f_pad and (s.residual is None) == (not error_feedback)
        s.theta.flat.copy_(theta0)
        nan = float("nan")
        for (p, mix, snap), w in zip(steps, want):
            for a, src in zip(s.workers, w["loaded"][r]):
                a.flat.copy_(src)
            snaps = None if w["snaps"] is None else [x.clone() for x in w["snaps"][r]]
            out = ~R.inside(plan, p, theta0.device)
            keep_theta, keep_w = s.theta.flat.clone(), [a.flat.clone() for a in s.workers]
            s.theta.flat[out] = nan
            for a in s.workers:
                a.flat[out] = nan
            keep_mom, pads = None, []
            if s.mom is not None:
                keep_mom = [m.clone() for m in s.mom]
                for q, m in enumerate(s.mom):
                    if q != p:
                        m.fill_(nan)
                for _, _, s0, s1, off in s._owned(p):            # the stepped fragment's momentum padding
                    real = max(0, min(s1, plan.numel(p)) - s0)
                    pads.append((off + real, off + s1 - s0))
                    s.mom[p][off + real:off + s1 - s0] = nan
            canary = (s.theta.flat.clone(), [a.flat.clone() for a in s.workers])
            s.step_fragment(p, mix, snaps)
            tag = (r, p, mix, snap)
            assert torch.equal(bits(s.theta.flat)[out], bits(canary[0])[out]), tag
            for a, c in zip(s.workers, canary[1]):
                assert torch.equal(bits(a.flat)[out], bits(c)[out]), tag
            s.theta.flat[out] = keep_theta[out]
            for a, k in zip(s.workers, keep_w):
                a.flat[out] = k[out]
            if s.mom is not None:
                for q, (m, k) in enumerate(zip(s.mom, keep_mom)):
                    if q != p:
                        assert bool(torch.isnan(m).all()), tag
                        m.copy_(k)
                for lo, hi in pads:
                    assert bool(torch.isnan(s.mom[p][lo:hi]).all()), tag
                    s.mom[p][lo:hi] = keep_mom[p][lo:hi]
            assert torch.equal(bits(s.theta.flat), bits(w["theta"])), tag
            for a, x in zip(s.workers, w["workers"][r]):
                assert torch.equal(bits(a.flat), bits(x)), tag
            st = s.gather_state()
            if mu != 0:
                assert torch.equal(bits(st.momentum), bits(w["mom"])), tag
            else:
                assert st.momentum is None
            if error_feedback:
                for q, (mine, ref_q) in enumerate(zip(s.residual, w["residual"][r])):
                    assert torch.equal(bits(mine), bits(ref_q)), (tag, q)
                    assert not mine[plan.numel(q):].any(), (tag, q)              # the padding stays zero
        return s

    return vw.run(body), ref
