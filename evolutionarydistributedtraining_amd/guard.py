"""The outer guard's host side: the policy, the totals, the decision and the report, as
pure functions of host numbers (numpy, no device work). `diloco._guard_pass` (arenas),
`diloco._guard_pass_list` (separate tensors) and `distributed.ShardedOuterSync._guarded` launch the statistics kernels and bring their rows to the
host; what they conclude from them is here, once. Totals are float64 sums in one fixed order
(`sequential_total`), so every rank reaches the same decision."""
from __future__ import annotations

import numpy as np

from ._lib import EdtError
from .ops import stats_columns


class OuterGuard:
    """Protection of theta and the outer momentum (opt-in, `guard=` of OuterSync, DirOuterSync,
    ShardedOuterSync and outer_step): before the step, one read-only pass (`ops.delta_stats`)
    measures the pseudo-gradient the step would apply — its norm, every worker's delta norm and
    cosine to the mean, and what is not finite — and `guard_decision` screens the workers and clips.

    max_grad_norm: clip the mean pseudo-gradient to this 2-norm (torch's clip_grad_norm_ formula
    over the fp64 norm); None: no clipping.
    on_nonfinite: "raise" (a NaN / Inf delta or mean raises NonFiniteWorkers, theta and the momentum
    untouched), "drop" (the flagged workers are left out: a true mean over the survivors, measured
    again) or "ignore" (report only).
    min_workers: fewer workers (after a drop: survivors) than this raises.
    per_tensor: last_stats also carries the figures per parameter tensor."""

    POLICIES = ("raise", "drop", "ignore")

    def __init__(self, max_grad_norm: float | None = None, on_nonfinite: str = "raise", min_workers: int = 1,
                 per_tensor: bool = False):
        if on_nonfinite not in self.POLICIES:
            raise ValueError(f"on_nonfinite must be one of {self.POLICIES}, got {on_nonfinite!r}")
        if max_grad_norm is not None and not (float(max_grad_norm) > 0.0):
            raise ValueError(f"max_grad_norm must be positive, got {max_grad_norm}")
        if int(min_workers) < 1:
            raise ValueError(f"min_workers must be at least 1, got {min_workers}")
        self.max_grad_norm = None if max_grad_norm is None else float(max_grad_norm)
        self.on_nonfinite = on_nonfinite
        self.min_workers = int(min_workers)
        self.per_tensor = bool(per_tensor)


class NonFiniteWorkers(EdtError):
    """The guard refused the step. nonfinite[k]: worker k's count of non-finite delta elements;
    nonfinite_mean: the mean's; survivors: the workers that were not flagged."""

    def __init__(self, message: str, nonfinite, nonfinite_mean: int, survivors):
        super().__init__(message)
        self.nonfinite = [int(c) for c in nonfinite]
        self.nonfinite_mean = int(nonfinite_mean)
        self.survivors = list(survivors)


def sequential_total(rows, width: int):
    """The float64 total of every column of `rows` ([n, width]), summed sequentially in row order
    (cumsum, not numpy's pairwise sum: one fixed function of the rows); zeros for no rows."""
    rows = np.asarray(rows, dtype=np.float64).reshape(-1, width)
    return np.cumsum(rows, axis=0)[-1] if len(rows) else np.zeros(width)


def totals_from_row(t, K: int) -> dict:
    """The totals dictionary from one total vector of 3 K + 2 doubles (`ops.stats_columns`). S_km
    is None above 8 workers (the pass does not form it)."""
    cols = stats_columns(K)
    return {"S_mm": float(t[0]), "S_kk": t[cols["S_kk"]].copy(),
            "S_km": t[cols["S_km"]].copy() if K <= 8 else None,
            "nonfinite_mean": int(t[2 * K + 1]), "nonfinite": t[cols["nonfinite"]].astype(np.int64)}


def stats_totals(rows, K: int, first=None) -> dict:
    """Totals of `ops.delta_stats` rows (host float64 [nchunks, 3 K + 2]) in float64, summed
    sequentially in chunk order. first: per-segment first-chunk indices [nseg + 1] -> the same
    totals per segment under "segments"."""
    W = 3 * K + 2
    rows = np.asarray(rows, dtype=np.float64).reshape(-1, W)
    out = totals_from_row(sequential_total(rows, W), K)
    if first is not None:
        out["segments"] = [totals_from_row(sequential_total(rows[int(a):int(b)], W), K)
                           for a, b in zip(first[:-1], first[1:])]
    return out


def clip_coefficient(s_mm: float, max_grad_norm: float | None) -> float:
    """min(1, max_norm / (norm + 1e-6)) over the fp64 norm sqrt(S_mm), evaluated in Python float64
    and cast to float32 (what the kernel multiplies by): torch.nn.utils.clip_grad_norm_'s formula."""
    if max_grad_norm is None:
        return 1.0
    return float(np.float32(min(1.0, float(max_grad_norm) / (float(s_mm) ** 0.5 + 1e-6))))


def guard_decision(totals: dict, guard: OuterGuard):
    """(survivors, clip_coef) from the totals of one statistics pass: a pure function, no device.
    survivors: indices of the workers the step averages. clip_coef: the float32 factor on the mean
    pseudo-gradient (1.0: the plain step runs) — None when workers were dropped, since the norm of
    what is applied is then that of a second pass over the survivors. Raises NonFiniteWorkers as
    the policy says, and whenever fewer than min_workers would take part."""
    nf = [int(c) for c in totals["nonfinite"]]
    nfm = int(totals["nonfinite_mean"])
    K = len(nf)
    everyone = list(range(K))
    flagged = [k for k in everyone if nf[k] > 0]
    survivors = [k for k in everyone if nf[k] == 0]
    if K < guard.min_workers:
        raise NonFiniteWorkers(f"{K} workers, min_workers = {guard.min_workers}", nf, nfm, everyone)
    if guard.on_nonfinite == "raise" and (flagged or nfm):
        raise NonFiniteWorkers(f"non-finite pseudo-gradient: workers {flagged} (counts {nf}), mean {nfm}",
                               nf, nfm, survivors)
    if guard.on_nonfinite == "drop":
        if len(survivors) < guard.min_workers:
            raise NonFiniteWorkers(f"{len(survivors)} finite workers left of {K}, min_workers = "
                                   f"{guard.min_workers} (counts {nf})", nf, nfm, survivors)
        if flagged:
            return survivors, None
        if nfm:
            raise NonFiniteWorkers(f"the mean of finite workers is not finite at {nfm} elements", nf, nfm, survivors)
    return everyone, clip_coefficient(totals["S_mm"], guard.max_grad_norm)


def report(totals: dict) -> dict:
    """What last_stats says of one statistics pass: the norms, the cosines and the counts."""
    with np.errstate(divide="ignore", invalid="ignore"):
        cos = None if totals["S_km"] is None else \
            (totals["S_km"] / np.sqrt(totals["S_kk"] * totals["S_mm"])).tolist()
    return {"grad_norm": float(totals["S_mm"]) ** 0.5, "worker_norms": np.sqrt(totals["S_kk"]).tolist(),
            "cos_to_mean": cos, "nonfinite": [int(c) for c in totals["nonfinite"]],
            "nonfinite_mean": int(totals["nonfinite_mean"])}


def fold_remeasured(rep: dict, again: dict, survivors, K: int) -> None:
    """After a drop: `rep` (the report over all K workers) takes the norm and the mean's count of what
    is applied from `again` (the report over the survivors, measured again) and their cosines at the
    survivors' indices, NaN at the dropped ones. Its per-worker norms and counts stay."""
    rep["grad_norm"], rep["nonfinite_mean"] = again["grad_norm"], again["nonfinite_mean"]
    if again["cos_to_mean"] is not None:
        cos = [float("nan")] * K
        for j, k in enumerate(survivors):
            cos[k] = again["cos_to_mean"][j]
        rep["cos_to_mean"] = cos
