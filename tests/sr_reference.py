"""numpy restatement of the stochastic rounding mode of the quantized exchange (EDT_ROUND_STOCHASTIC:
DESIGN §3, include/edt_sync.h), written from the definition, not from the kernel. The wire format,
the grids, pack and dequantize are tests/quant_reference.py's, unchanged; what is restated here is

  random bits  Philox4x32 with PHILOX_ROUNDS rounds (the header's EDT_PHILOX_ROUNDS), key = the two
               words of the seed, counter = (g lo, g hi, step, stream), g = global element index / 8;
               element 8g + j takes bits 16 (j % 2) .. 16 (j % 2) + 15 of output word j / 2
  scale        e = floor(log2(amax)) - emax, + 1 when amax 2^-e exceeds the largest element;
               byte = clamp(e + 127, 0, 254); an all-zero block stores 0
  element      a = |v| 2^-e, k = max(floor(log2 a), EMIN), q = 2^(k - MB), t = a / q, lo = floor(t),
               f16 = floor((t - lo) 2^16), up = (r16 < f16): the element is (lo + up) q, sign kept
  non-finite   block: scale byte 255, codes 0

in float64, where every step above is exact for fp32 inputs. There is no reference-project code
behind this mode (the reference ships checkpoints over a disk and quantizes nothing)."""
from __future__ import annotations

import os
import re

import numpy as np

from tests import gather_q_reference as G
from tests import quant_reference as Q

_HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "edt_sync.h")
with open(_HEADER) as _f:
    PHILOX_ROUNDS = int(re.search(r"^#define\s+EDT_PHILOX_ROUNDS\s+(\d+)", _f.read(), re.M).group(1))

M0, M1 = 0xD2511F53, 0xCD9E8D57
W0, W1 = 0x9E3779B9, 0xBB67AE85
_MASK = np.uint64(0xffffffff)


def philox4x32(counter, key, rounds: int = PHILOX_ROUNDS) -> np.ndarray:
    """counter [..., 4], key [..., 2] (broadcast against each other), 32-bit words -> output [..., 4] uint32."""
    c = np.asarray(counter, dtype=np.uint64) & _MASK
    k = np.asarray(key, dtype=np.uint64) & _MASK
    c0, c1, c2, c3 = (c[..., i] for i in range(4))
    k0, k1 = k[..., 0], k[..., 1]
    for _ in range(rounds):
        p0, p1 = np.uint64(M0) * c0, np.uint64(M1) * c2              # < 2^64: exact in uint64
        c0, c1, c2, c3 = (p1 >> np.uint64(32)) ^ c1 ^ k0, p1 & _MASK, (p0 >> np.uint64(32)) ^ c3 ^ k1, p0 & _MASK
        k0, k1 = (k0 + np.uint64(W0)) & _MASK, (k1 + np.uint64(W1)) & _MASK
    return np.stack(np.broadcast_arrays(c0, c1, c2, c3), axis=-1).astype(np.uint32)


def random_bits(seed: int, step: int, stream_id: int, n: int, elem_base: int = 0) -> np.ndarray:
    """r16 (uint32 in [0, 2^16)) of the global elements elem_base .. elem_base + n - 1 (both multiples of 8)."""
    assert n % 8 == 0 and elem_base % 8 == 0
    g = np.arange(elem_base // 8, (elem_base + n) // 8, dtype=np.uint64)
    ctr = np.stack([g & _MASK, g >> np.uint64(32), np.full_like(g, step & 0xffffffff), np.full_like(g, stream_id)], axis=-1)
    w = philox4x32(ctr, np.array([seed & 0xffffffff, (seed >> 32) & 0xffffffff], dtype=np.uint64))
    lo, hi = w & np.uint32(0xffff), w >> np.uint32(16)                # element j: word j / 2, half j % 2
    return np.stack([lo, hi], axis=-1).reshape(-1).astype(np.uint32)


def _fmt(fmt):
    f = Q.FORMATS[fmt]
    return f, 1 - f["bias"], float(Q.finite_grid(fmt)[-1])            # EMIN = 1 - bias (E4M3: -6, E2M1: 0)


def scale_exponent(blk: np.ndarray, fmt: str):
    """Per block of 32 (rows of blk, float32): (bad, scale byte, the exponent applied, bumped?)."""
    f, _, maxv = _fmt(fmt)
    bad = ~np.isfinite(blk).all(axis=1)
    amax = np.where(bad, 0.0, np.abs(np.where(np.isfinite(blk), blk, 0)).max(axis=1).astype(np.float64))
    zero = amax == 0
    _, ex = np.frexp(np.where(zero, 1.0, amax))                       # floor(log2 amax) = ex - 1
    e = ex.astype(np.int64) - 1 - f["emax"]
    bump = np.ldexp(amax, (-e).astype(np.int32)) > maxv               # amax 2^-e exceeds the largest element
    e = e + bump
    sb = np.where(zero, 0, Q.scale_byte(e)).astype(np.uint8)
    sb = np.where(bad, 255, sb).astype(np.uint8)
    return bad, sb, np.where(bad, 0, sb.astype(np.int64) - 127), bump & ~zero & ~bad


def quantize_sr(p: np.ndarray, fmt: str, r16: np.ndarray):
    """p float32 [n], n % 32 == 0, r16 [n] the elements' random bits -> (codes uint8 [n], scale bytes
    uint8 [n / 32]): the definition above, step by step."""
    f, emin, maxv = _fmt(fmt)
    mb = f["mbits"]
    p = np.ascontiguousarray(p, dtype=np.float32)
    assert p.size % Q.BLOCK == 0 and np.size(r16) == p.size
    blk = p.reshape(-1, Q.BLOCK)
    bad, sb, e_used, _ = scale_exponent(blk, fmt)
    a = np.ldexp(np.abs(np.where(bad[:, None], 0.0, blk)).astype(np.float64), (-e_used)[:, None].astype(np.int32))
    _, ex = np.frexp(np.where(a == 0, 1.0, a))
    k = np.maximum(np.where(a == 0, emin, ex.astype(np.int64) - 1), emin)
    t = np.ldexp(a, (mb - k).astype(np.int32))                        # a / q, q = 2^(k - MB): exact
    lo = np.floor(t)
    f16 = np.floor((t - lo) * 65536.0)
    up = np.asarray(r16, dtype=np.float64).reshape(blk.shape) < f16
    val = np.minimum(np.ldexp(lo + up, (k - mb).astype(np.int32)), maxv)       # saturates only at the 254 clamp
    grid = Q.finite_grid(fmt)
    code = np.searchsorted(grid, val)
    assert np.array_equal(grid[code], val), "the result is a grid point by construction"
    sign = np.signbit(blk).astype(np.uint8) << (f["bits"] - 1)
    code = np.where(bad[:, None], 0, code.astype(np.uint8) | sign).astype(np.uint8)
    return code.reshape(-1), sb


def grid_step(p: np.ndarray, fmt: str, scales: np.ndarray | None = None) -> np.ndarray:
    """q 2^e at every element (float64): the distance of the element's two grid neighbours under its
    block's scale — the stochastic encoder's, or the one in `scales` (the bytes an encoder wrote, e.g.
    the nearest one's, which never bumps). NaN inside a non-finite block."""
    f, emin, _ = _fmt(fmt)
    blk = np.ascontiguousarray(p, dtype=np.float32).reshape(-1, Q.BLOCK)
    bad, _, e_used, _ = scale_exponent(blk, fmt)
    if scales is not None:
        e_used = np.where(bad, 0, np.asarray(scales, dtype=np.int64) - 127)
    a = np.ldexp(np.abs(np.where(bad[:, None], 0.0, blk)).astype(np.float64), (-e_used)[:, None].astype(np.int32))
    _, ex = np.frexp(np.where(a == 0, 1.0, a))
    k = np.maximum(np.where(a == 0, emin, ex.astype(np.int64) - 1), emin)
    step = np.ldexp(1.0, (k - f["mbits"] + e_used[:, None]).astype(np.int32))
    return np.where(bad[:, None], np.nan, step).reshape(-1)


def sr_quantize(p: np.ndarray, fmt: str, seed: int, step: int, stream_id: int, elem_base: int = 0):
    """quantize_sr with the bits of (seed, step, stream_id) at global elements elem_base + i."""
    return quantize_sr(p, fmt, random_bits(seed, step, stream_id, np.size(p), elem_base))


UNBIASED_SEED = 0x5eed5eed5eed5eed


def unbiased_inputs(n: int = 4096) -> np.ndarray:
    """The fixed inputs of the unbiasedness tests: N(0, 1) * 2^U{-12..3}, numpy seed 0."""
    g = np.random.default_rng(0)
    return (g.standard_normal(n) * np.exp2(g.integers(-12, 4, n))).astype(np.float32)


def owners(buckets, world: int, n_pad: int) -> np.ndarray:
    """The rank that owns each arena element under ShardedOuterSync's buckets."""
    own = np.empty(n_pad, dtype=np.int64)
    for b, e in buckets:
        per = (e - b) // world
        for r in range(world):
            own[b + r * per:b + (r + 1) * per] = r
    return own


def update_sr(theta_old, theta_new, fmt: str, seed: int, step: int, own: np.ndarray):
    """Phase 2' over the whole arena: u = f32(theta') - f32(theta) quantized by each element's owner
    r on stream 2 r + 1 at the element's arena index. A block has one owner and its scale does not
    depend on the stream, so the owners' codes assemble by selection. Returns D(q)."""
    with np.errstate(invalid="ignore"):
        u = (G._f32(theta_new) - G._f32(theta_old)).astype(np.float32)
    codes, scales = None, None
    for r in np.unique(own):
        c, s = sr_quantize(u, fmt, seed, step, 2 * int(r) + 1)
        codes = c if codes is None else np.where(own == r, c, codes)
        scales = s
    return Q.dequantize(codes, scales, fmt)


def compose(partial, sgd_sum, theta0, gens, world, n_pad, buckets, fmt_in, fmt_out, seed, lr=0.7, mu=0.9,
            nesterov=True, first_step=0, mom=None):
    """reduce_q with stochastic rounding composed by hand over the whole padded arena, with no
    regions, packing or per-bucket calls: per rank r the fp32 partial (partial(theta, workers, K) ->
    numpy), quantized on stream 2 r at step first_step + i; the D's summed in rank order and the SGD
    step by sgd_sum(theta, [D_0 ..], momentum, has_momentum, lr, mu, nesterov) (in place); without
    fmt_out that is the new theta, with it the update is quantized by its owners (update_sr) and
    added. mom: the carried momentum (then the first step has one). Returns (theta, momentum)."""
    import torch
    n = theta0.numel()
    th = torch.zeros(n_pad, dtype=theta0.dtype, device=theta0.device)
    th[:n] = theta0
    has = mom is not None
    mom = torch.zeros_like(th) if mom is None else mom.clone()
    own = owners(buckets, world, n_pad)
    for i, ws in enumerate(gens):
        K = len(ws)
        kl = K // world
        ds = []
        for r in range(world):
            pads = []
            for w in ws[r * kl:(r + 1) * kl]:
                pw = torch.zeros(n_pad, dtype=w.dtype, device=th.device)
                pw[:n] = w
                pads.append(pw)
            codes, scales = sr_quantize(partial(th, pads, K), fmt_in, seed, first_step + i, 2 * r)
            ds.append(torch.from_numpy(Q.dequantize(codes, scales, fmt_in)).to(th.device))
        new = th.clone()
        sgd_sum(new, ds, mom, has or i > 0, lr, mu, nesterov)
        if fmt_out is None:
            th = new
        else:
            th = G.apply_delta(th, update_sr(th, new, fmt_out, seed, first_step + i, own))
    return th, mom


class NumpySrKernels(G.NumpyGatherKernels):
    """NumpyGatherKernels whose two encoders take the rounding keywords (ShardedOuterSync's kernels=
    seam on CPU tensors): nearest is the parent class's, stochastic is sr_quantize."""

    def delta_partial_q(self, theta, workers, k_total, packed, region_elems, fmt, residual=None, rounding="nearest",
                        seed=0, step=0, stream_id=0, elem_base=0):
        if rounding == "nearest":
            return super().delta_partial_q(theta, workers, k_total, packed, region_elems, fmt, residual)
        import torch
        assert rounding == "stochastic" and residual is None and elem_base % 8 == 0
        acc = torch.zeros(theta.numel(), dtype=torch.float32)
        self.o.delta_partial(theta, workers, k_total, acc, False)
        codes, scales = sr_quantize(acc.numpy(), fmt, seed, step, stream_id, elem_base)
        packed.copy_(torch.from_numpy(Q.pack(codes, scales, fmt, region_elems)))

    def sgd_delta_sum_q(self, theta, regions, fmt_in, momentum, has_momentum, lr, mu, nesterov, packed_out, fmt_out,
                        residual=None, rounding="nearest", seed=0, step=0, stream_id=0, elem_base=0):
        if rounding == "nearest":
            return super().sgd_delta_sum_q(theta, regions, fmt_in, momentum, has_momentum, lr, mu, nesterov,
                                           packed_out, fmt_out, residual)
        import torch
        assert rounding == "stochastic" and residual is None and elem_base % 8 == 0
        new = theta.clone()
        self.sgd_apply_sum_q(new, regions, fmt_in, momentum, has_momentum, lr, mu, nesterov)
        with np.errstate(invalid="ignore"):
            u = (G._f32(new) - G._f32(theta)).astype(np.float32)
        codes, scales = sr_quantize(u, fmt_out, seed, step, stream_id, elem_base)
        packed_out.copy_(torch.from_numpy(Q.pack(codes, scales, fmt_out, theta.numel())))


def run_schedule(world, layout, tdt, wdt, theta0, gens, kernels, fmt_in, fmt_out, seed, bucket_elems,
                 rounding="stochastic", first_step=0, state=None):
    """ShardedOuterSync(mode="reduce_q", error_feedback=False, rounding=...) on `world` virtual ranks
    (kernels None: the HIP kernels), one step per generation of `gens`. state (per rank {"theta",
    "mom"}) restarts from a saved step with q_step = first_step. Returns per rank the theta replica
    and the momentum shard after every step, the buckets, n_pad and the final q_step."""
    from evolutionarydistributedtraining_amd.collectives import VirtualWorld
    from evolutionarydistributedtraining_amd.distributed import ShardedOuterSync
    k_local = len(gens[0]) // world

    def body(comm):
        s = ShardedOuterSync(layout, tdt, wdt, k_local, theta0.device, mode="reduce_q", wire_format=fmt_in,
                             error_feedback=False, bucket_elems=bucket_elems, kernels=kernels, comm=comm,
                             gather_format=fmt_out, rounding=rounding, seed=seed)
        s.theta.flat.copy_(theta0)
        if state is not None:
            s.theta_buf.copy_(state[comm.rank]["theta"])
            s.mom_shard.copy_(state[comm.rank]["mom"])
            s.has_momentum = True
            s.q_step = first_step
        out = []
        for ws in gens:
            for j, a in enumerate(s.workers):
                a.flat.copy_(ws[comm.rank * k_local + j])
            s.step()
            out.append({"theta": s.theta_buf.clone(), "mom": s.mom_shard.clone()})
        return {"steps": out, "buckets": s.buckets, "n_pad": s.n_pad, "q_step": s.q_step,
                "has_residual": s.residual is not None or getattr(s, "residual_g", None) is not None}

    return VirtualWorld(world).run(body)
