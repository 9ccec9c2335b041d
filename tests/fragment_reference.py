"""The fragment-wise outer step with its fused worker merge, restated on the CPU.

The step of a run is the oracle's outer step on that run alone. The merge is three torch CPU ops in
the worker dtype with Python-float coefficients, `(1.0 - t) * live + t * theta_new.to(wdt)`; t == 1.0
is the overwrite (`theta_new.to(wdt)`, the destination not read). tests/test_fragment_cpu.py pins the
merge against the oracle's `lerp`, the restatement `ops.lerp` is tested against."""
import torch

from oracle import oracle


def merge_reference(live: torch.Tensor, theta_new: torch.Tensor, t: float) -> torch.Tensor:
    v = theta_new.to(live.dtype)
    if t == 1.0:
        return v
    return (1.0 - t) * live + t * v


def step_run(theta, deltas, mom, has, lr, mu, nesterov) -> None:
    """The oracle's outer step on one run, in place on theta and mom (CPU tensors; mom None when
    mu == 0)."""
    if theta.numel():
        oracle.outer_step(theta, deltas, mom if mu != 0 else None, has, lr, mu, nesterov)


def mix_reference(thetas, deltas, moms, has, lr, mu, nesterov, live, t):
    """`ops.outer_step_list_mix` on CPU clones: returns (thetas, moms, live) after the call.
    deltas: K lists of R runs; live: nmix lists of R runs, or None (no merge); a destination that is
    the same object as a delta run is read before it is overwritten, as on the device."""
    th = [x.clone() for x in thetas]
    mo = [x.clone() for x in moms] if moms is not None else None
    for r in range(len(th)):
        step_run(th[r], [d[r].contiguous() for d in deltas], mo[r] if mo is not None else None, has, lr, mu, nesterov)
    out = None
    if live is not None:
        out = [[merge_reference(l[r], th[r], t) for r in range(len(th))] for l in live]
    return th, mo, out


class FragmentRun:
    """A whole fragment-wise run on CPU arenas, driven by the same FragmentPlan as OuterSync's:
    theta, the momentum (zeros until a fragment's first step writes it) and K worker arenas."""

    def __init__(self, plan, theta, workers, lr, mu, nesterov):
        self.plan, self.lr, self.mu, self.nesterov = plan, lr, mu, nesterov
        self.theta = theta.clone()
        self.workers = [w.clone() for w in workers]
        self.mom = torch.zeros_like(self.theta)
        self.has = [False] * len(plan)

    def step(self, p, mix=1.0, snapshots=None, merge=True):
        for r, (a, n) in enumerate(self.plan.runs(p)):
            th, mo = self.theta[a:a + n], self.mom[a:a + n]
            if snapshots is None:
                deltas = [w[a:a + n].clone() for w in self.workers]
            else:
                off = sum(m for _, m in self.plan.runs(p)[:r])
                deltas = [s[off:off + n].clone() for s in snapshots]
            step_run(th, deltas, mo, self.has[p], self.lr, self.mu, self.nesterov)
            if merge:
                for w in self.workers:
                    w[a:a + n] = merge_reference(w[a:a + n], th, mix)
        if self.mu != 0:
            self.has[p] = True
