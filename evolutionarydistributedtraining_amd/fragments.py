"""Fragments of a parameter layout for the fragment-wise outer step (Streaming DiLoCo).

The parameters are cut into P fragments; each outer step synchronises one of them
(`OuterSync.step_fragment`, `diloco.outer_step_fragment`). A `FragmentPlan` only says which tensors
of a `ParamLayout` belong to which fragment and where they lie in an arena: it holds no tensors and
needs no device.
"""
from __future__ import annotations

import re

import torch

from .params import ParamLayout


def _first_int(name: str):
    m = re.search(r"\d+", name)
    return int(m.group()) if m else None


class FragmentPlan:
    """`fragments`: P lists of tensor indices into `layout` that together partition
    range(len(layout)) (every tensor in exactly one fragment; a fragment may be empty)."""

    def __init__(self, layout: ParamLayout, fragments):
        self.layout = layout
        self.fragments = [sorted(int(i) for i in f) for f in fragments]
        if not self.fragments:
            raise ValueError("a plan needs at least one fragment")
        seen = sorted(i for f in self.fragments for i in f)
        if seen != list(range(len(layout))):
            raise ValueError("the fragments must partition the layout's tensors: every index of "
                             f"range({len(layout)}) exactly once")
        self._runs = [self._coalesce(f) for f in self.fragments]

    def __len__(self) -> int:
        return len(self.fragments)

    def _coalesce(self, idx) -> list[tuple[int, int]]:
        runs: list[tuple[int, int]] = []
        for i in idx:                                   # arena order; empty tensors join no run
            off, n = self.layout.offsets[i], self.layout.numels[i]
            if n == 0:
                continue
            if runs and runs[-1][0] + runs[-1][1] == off:
                runs[-1] = (runs[-1][0], runs[-1][1] + n)
            else:
                runs.append((off, n))
        return runs

    @classmethod
    def sequential(cls, layout: ParamLayout, P: int) -> "FragmentPlan":
        """Contiguous tensor ranges, balanced greedily by element count: fragment p is closed at the
        tensor where the running total comes closest to (p + 1) / P of the whole."""
        if P < 1:
            raise ValueError("P must be at least 1")
        frags: list[list[int]] = [[] for _ in range(P)]
        total, done, p = layout.total, 0, 0
        for i, n in enumerate(layout.numels):
            target = total * (p + 1) / P
            if p < P - 1 and frags[p] and abs(done + n - target) > abs(done - target):
                p += 1
            frags[p].append(i)
            done += n
        return cls(layout, frags)

    @classmethod
    def strided(cls, layout: ParamLayout, P: int, block_of=None) -> "FragmentPlan":
        """Fragments strided over the model's blocks: block_of(name) is a tensor's block id
        (default: the first integer in its name, `layers.12.…` -> 12; None where there is none). The
        tensors without one that come before the first numbered tensor form one block ahead of the
        numbered ones, the remaining ones one block behind them. The distinct blocks in that order
        are b = 0, 1, …, and block b goes to fragment b % P."""
        if P < 1:
            raise ValueError("P must be at least 1")
        if len(layout.names) != len(layout):
            raise ValueError("a strided plan needs the layout's tensor names")
        block_of = block_of or _first_int
        ids = [block_of(n) for n in layout.names]
        first = next((i for i, b in enumerate(ids) if b is not None), len(ids))
        keys = [(1, b) if b is not None else ((0, 0) if i < first else (2, 0)) for i, b in enumerate(ids)]
        order = {k: b for b, k in enumerate(sorted(set(keys)))}
        frags: list[list[int]] = [[] for _ in range(P)]
        for i, k in enumerate(keys):
            frags[order[k] % P].append(i)
        return cls(layout, frags)

    def tensors(self, p: int) -> list[int]:
        return self.fragments[p]

    def fragment_of(self, i: int) -> int:
        return next(p for p, f in enumerate(self.fragments) if i in f)

    def numel(self, p: int) -> int:
        return sum(n for _, n in self._runs[p])

    def runs(self, p: int) -> list[tuple[int, int]]:
        """The fragment's tensors in arena order, adjacent ones coalesced: (offset, numel) runs."""
        return list(self._runs[p])

    def pieces(self, p: int, lo: int, hi: int) -> list[tuple[int, int, int]]:
        """Fragment space is fragment p's runs laid back to back (the layout of its snapshots). The
        sub-runs covered by the fragment-space range [lo, hi), in that order, as (arena offset,
        fragment-space offset, numel): runs are cut at the range's bounds, empty pieces are left
        out, and the part of the range at or beyond numel(p) (the padding of a sharded fragment)
        has none."""
        out, off = [], 0
        for a, n in self._runs[p]:
            s, e = max(lo, off), min(hi, off + n)
            if s < e:
                out.append((a + s - off, s, e - s))
            off += n
        return out

    def views(self, p: int, flat: torch.Tensor) -> list[torch.Tensor]:
        """The run views of a flat buffer laid out by the plan's layout."""
        if flat.numel() != self.layout.total:
            raise ValueError("the buffer does not match the plan's layout")
        return [flat[a:a + n] for a, n in self._runs[p]]

    def snapshot_views(self, p: int, snap: torch.Tensor) -> list[torch.Tensor]:
        """The run views of a snapshot of fragment p: its runs back to back (`capture_fragment`)."""
        if snap.numel() != self.numel(p):
            raise ValueError("the snapshot does not match the fragment's size")
        out, off = [], 0
        for _, n in self._runs[p]:
            out.append(snap[off:off + n])
            off += n
        return out
