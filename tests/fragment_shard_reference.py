"""The sharded fragment step (sharded_fragments.ShardedFragmentSync) restated in one process, and what
its CPU and GPU tests share.

`ShardRun` is the composition the schedule must equal bit for bit: per rank the partial of its local
workers over the PACKED fragment (fragment space: the runs back to back), the partials summed in rank
order, one SGD step on the packed theta and momentum, unpacked; then the merge per worker. Its
arithmetic is handed in: `OracleArith` (the CPU oracle: tests/oracle_kernels.py's partial and
rank-ordered SGD, torch lerp / copy_) for the CPU tests, the existing non-list HIP kernels on packed
copies for the GPU tests. `PieceOracleKernels` is the kernels= stand-in: the three piece-list names,
per piece, with the same oracle arithmetic.
"""
from __future__ import annotations

import torch

from evolutionarydistributedtraining_amd.fragments import FragmentPlan
from evolutionarydistributedtraining_amd.params import ParamLayout

# a run shorter than 8 elements, sizes off a multiple of 8 (later pieces are not 16-byte aligned), a
# run longer than a 4,096-element chunk and a 2,048-element tile, an empty tensor
NUMELS = [5, 4099, 64, 0, 1000, 8200, 7, 2048]
NAMES = ["layers.0.a", "layers.1.a", "layers.2.a", "layers.2.b", "layers.3.a", "layers.4.a", "layers.5.a",
         "layers.6.a"]
REGIMES = [(torch.float32, torch.float32), (torch.float32, torch.bfloat16), (torch.bfloat16, torch.bfloat16)]


def layout() -> ParamLayout:
    return ParamLayout([(n,) for n in NUMELS], list(NAMES))


def plans(lay: ParamLayout) -> dict:
    """strided: layers alternate between two fragments; explicit: non-adjacent tensors share one."""
    return {"strided": FragmentPlan.strided(lay, 2), "explicit": FragmentPlan(lay, [[0, 5, 6], [1, 3, 7], [2, 4]])}


def bucket_elems(world: int, plan_name: str) -> int:
    """world * 64 * k. strided: 4,608, so a bucket holds a piece longer than a chunk and the larger
    fragment still has 3 buckets; explicit: 384 (two units at world 3), so its smallest fragment
    (1,064 elements) has 3 buckets and shard bounds cut every run."""
    unit = world * 64
    target = 4608 if plan_name == "strided" else 384
    return max(unit, target // unit * unit)


def bits(t: torch.Tensor) -> torch.Tensor:
    return t.view(torch.int32) if t.dtype == torch.float32 else t.view(torch.int16)


def pack(plan: FragmentPlan, p: int, flat: torch.Tensor) -> torch.Tensor:
    vs = plan.views(p, flat)
    return torch.cat(vs) if vs else flat[:0].clone()


def unpack_(plan: FragmentPlan, p: int, flat: torch.Tensor, packed: torch.Tensor) -> None:
    for dst, src in zip(plan.views(p, flat), plan.snapshot_views(p, packed)):
        dst.copy_(src)


def inside(plan: FragmentPlan, p: int, device="cpu") -> torch.Tensor:
    """Boolean mask over the arena: the elements of fragment p."""
    m = torch.zeros(plan.layout.total, dtype=torch.bool, device=device)
    for a, n in plan.runs(p):
        m[a:a + n] = True
    return m


class OracleArith:
    """The composition's arithmetic on the CPU."""

    def __init__(self, oracle):
        self.o = oracle

    def partial(self, theta, deltas, k_total, acc):
        self.o.delta_partial(theta, deltas, k_total, acc, False)

    def sgd_sum(self, theta, parts, mom, has, lr, mu, nesterov):
        total = parts[0].clone()
        for q in parts[1:]:
            total.add_(q)
        self.o.sgd_apply(theta, total, mom, has, lr, mu, nesterov)

    def merge(self, live, theta_new, mix):
        """torch's own: copy_ at mix 1.0, else lerp towards theta_new in the worker dtype."""
        if mix == 1.0:
            live.copy_(theta_new)
        else:
            live.copy_(torch.lerp(live, theta_new.to(live.dtype), mix))


class PieceOracleKernels:
    """kernels= stand-in for ShardedFragmentSync: the three piece-list entries, piece by piece."""

    def __init__(self, oracle):
        self.a = OracleArith(oracle)
        self.calls = []

    def delta_partial_list(self, thetas, workers, k_total, accs):
        self.calls.append("delta_partial_list")
        for t, th in enumerate(thetas):
            self.a.partial(th, [w[t] for w in workers], k_total, accs[t])

    def sgd_sum_list_to(self, thetas, parts, momenta, has, lr, mu, nesterov, outs):
        self.calls.append("sgd_sum_list_to")
        for t, th in enumerate(thetas):
            new = th.clone()                                     # theta is only read
            self.a.sgd_sum(new, [q[t] for q in parts], None if momenta is None else momenta[t], has, lr, mu, nesterov)
            outs[t].copy_(new)

    def theta_scatter_mix_list(self, thetas, srcs, live, mix):
        self.calls.append("theta_scatter_mix_list")
        for t, th in enumerate(thetas):
            th.copy_(srcs[t])
            for l in live:
                self.a.merge(l[t], srcs[t], mix)


class ShardRun:
    """The single-process composition. workers[r][j]: rank r's local worker j (arena-sized)."""

    def __init__(self, plan, theta, workers, arith, lr, mu, nesterov):
        self.plan, self.arith, self.lr, self.mu, self.nesterov = plan, arith, lr, mu, nesterov
        self.theta = theta.clone()
        self.workers = [[w.clone() for w in ws] for ws in workers]
        self.mom = torch.zeros_like(self.theta)
        self.has = [False] * len(plan)

    def step(self, p, mix=1.0, snapshots=None, merge=True):
        """snapshots[r][j]: rank r's fragment-space snapshot of its worker j (None: the live arenas)."""
        plan = self.plan
        th = pack(plan, p, self.theta)
        if th.numel():
            k_total = sum(len(ws) for ws in self.workers)
            parts = []
            for r, ws in enumerate(self.workers):
                deltas = [pack(plan, p, w) for w in ws] if snapshots is None else [s.clone() for s in snapshots[r]]
                acc = torch.zeros(th.numel(), dtype=torch.float32, device=th.device)
                self.arith.partial(th, deltas, k_total, acc)
                parts.append(acc)
            mom = pack(plan, p, self.mom) if self.mu != 0 else None
            self.arith.sgd_sum(th, parts, mom, self.has[p], self.lr, self.mu, self.nesterov)
            unpack_(plan, p, self.theta, th)
            if mom is not None:
                unpack_(plan, p, self.mom, mom)
            if merge:
                for ws in self.workers:
                    for w in ws:
                        live = pack(plan, p, w)
                        self.arith.merge(live, th, mix)
                        unpack_(plan, p, w, live)
        if self.mu != 0:
            self.has[p] = True


def population(lay, tdt, wdt, k_total, seed=7, device="cpu"):
    g = torch.Generator().manual_seed(seed)
    theta = (torch.randn(lay.total, generator=g) * 0.02).to(tdt)
    workers = [(theta.float() + torch.randn(lay.total, generator=g) * 1e-3).to(wdt).to(device) for _ in range(k_total)]
    return theta.to(device), workers


def drift(w: torch.Tensor, seed: int) -> torch.Tensor:
    """What an inner loop leaves: w moved a little, deterministically (in w's dtype)."""
    g = torch.Generator().manual_seed(seed)
    return (w.float().cpu() + torch.randn(w.numel(), generator=g) * 1e-3).to(w.dtype).to(w.device)


def schedule_steps(P: int) -> list[tuple[int, float, bool]]:
    """Two round robins over the fragments as (p, mix, from snapshots): mix 0.5 then 1.0, snapshots
    on alternating steps."""
    return [(p, 0.5 if rnd == 0 else 1.0, (rnd + p) % 2 == 0) for rnd in range(2) for p in range(P)]


def drive(vw, make_sync, plan, theta0, workers0, arith, lr=0.7, mu=0.9, nesterov=True, steps=None):
    """Runs `steps` (default: schedule_steps) on the virtual world `vw` and on ShardRun, checking after
    every step and on every rank, bit for bit: theta and the gathered momentum against the
    composition, every local worker against it, and — through NaN canaries planted in every element
    outside the stepped fragment of theta, the workers and the other fragments' momentum — that
    nothing else was touched. make_sync(comm) builds the rank's ShardedFragmentSync. Returns the
    syncs (rank order) and the composition."""
    world = vw.world
    k_local = len(workers0) // world
    per_rank = [workers0[r * k_local:(r + 1) * k_local] for r in range(world)]
    steps = steps if steps is not None else schedule_steps(len(plan))
    # the composition first: the states every rank must show after each step, and the snapshots
    ref = ShardRun(plan, theta0, per_rank, arith, lr, mu, nesterov)
    want, seed = [], 1000
    for p, mix, snap in steps:
        snaps = None
        if snap:
            snaps = [[pack(plan, p, w) for w in ws] for ws in ref.workers]
        for ws in ref.workers:                       # the workers train on after the snapshot
            for j in range(len(ws)):
                seed += 1
                ws[j] = drift(ws[j], seed)
        loaded = [[w.clone() for w in ws] for ws in ref.workers]
        ref.step(p, mix, snaps)
        want.append({"loaded": loaded, "snaps": snaps, "theta": ref.theta.clone(), "mom": ref.mom.clone(),
                     "workers": [[w.clone() for w in ws] for ws in ref.workers]})

    def body(comm):
        s = make_sync(comm)
        r = comm.rank
        s.theta.flat.copy_(theta0)
        nan = float("nan")
        for (p, mix, snap), w in zip(steps, want):
            for a, src in zip(s.workers, w["loaded"][r]):
                a.flat.copy_(src)
            snaps = None if w["snaps"] is None else [x.clone() for x in w["snaps"][r]]
            out = ~inside(plan, p, theta0.device)
            keep_theta, keep_w = s.theta.flat.clone(), [a.flat.clone() for a in s.workers]
            s.theta.flat[out] = nan
            for a in s.workers:
                a.flat[out] = nan
            keep_mom = None
            if s.mom is not None:
                keep_mom = [m.clone() for m in s.mom]
                for q, m in enumerate(s.mom):
                    if q != p:
                        m.fill_(nan)
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
            assert torch.equal(bits(s.theta.flat), bits(w["theta"])), tag
            for a, x in zip(s.workers, w["workers"][r]):
                assert torch.equal(bits(a.flat), bits(x)), tag
            st = s.gather_state()
            if mu != 0:
                assert torch.equal(bits(st.momentum), bits(w["mom"])), tag
            else:
                assert st.momentum is None
        return s

    return vw.run(body), ref
