"""numpy restatement of the quantized partial exchange's wire format (include/edt_sync.h),
written from the format's definition, not from the kernel: the element grids are enumerated from
the OCP encodings and rounding is a nearest-neighbour search on the grid in float64.

  block     32 consecutive fp32 elements share one E8M0 scale byte (bias 127)
  scale     e = floor(log2(amax)) - emax (emax 8 for E4M3, 2 for E2M1); byte = clamp(e + 127, 0, 254);
            an all-zero block stores byte 0
  elements  v * 2^-e rounded to nearest-even onto the grid, saturating (448 / 6), sign kept
  non-finite block: scale byte 255, element codes 0; dequantizes to NaN everywhere
  packing   mxfp8 one byte per element; mxfp4 element 2i in the low nibble, 2i + 1 in the high one;
            a region of R elements is R * bits / 8 payload bytes, then R / 32 scale bytes
  D(q) = elem * 2^e
"""
from __future__ import annotations

import numpy as np

BLOCK = 32
FORMATS = {"mxfp8": {"bits": 8, "mbits": 3, "bias": 7, "emax": 8},
           "mxfp4": {"bits": 4, "mbits": 1, "bias": 1, "emax": 2}}


def magnitude_table(fmt: str) -> np.ndarray:
    """Value of every magnitude code 0 .. 2^(bits-1) - 1 (float64); OCP E4M3's 0x7f is NaN."""
    f = FORMATS[fmt]
    mb, bias = f["mbits"], f["bias"]
    out = np.empty(1 << (f["bits"] - 1), dtype=np.float64)
    for c in range(len(out)):
        E, m = c >> mb, c & ((1 << mb) - 1)
        out[c] = m * 2.0 ** (1 - bias - mb) if E == 0 else (1 + m / (1 << mb)) * 2.0 ** (E - bias)
    if fmt == "mxfp8":
        out[0x7f] = np.nan
    return out


def finite_grid(fmt: str) -> np.ndarray:
    t = magnitude_table(fmt)
    return t[np.isfinite(t)]                 # ascending; index == magnitude code


def round_to_grid(a: np.ndarray, fmt: str) -> np.ndarray:
    """Magnitude codes of |values| a (float64, finite, >= 0): nearest grid point, ties to the even
    code, saturating at the largest finite one."""
    g = finite_grid(fmt)
    hi = np.clip(np.searchsorted(g, a, side="left"), 1, len(g) - 1)      # g[hi-1] <= a <= g[hi] inside the grid
    lo = hi - 1
    dl, dh = a - g[lo], g[hi] - a
    pick_hi = (dh < dl) | ((dh == dl) & (hi % 2 == 0))
    code = np.where(pick_hi, hi, lo)
    return np.where(a >= g[-1], len(g) - 1, code).astype(np.uint8)


def scale_byte(e) -> np.ndarray:
    return np.clip(np.asarray(e, dtype=np.int64) + 127, 0, 254).astype(np.uint8)


def quantize(p: np.ndarray, fmt: str):
    """p: float32, a multiple of 32 elements -> (codes uint8 [n] with the sign in bit bits-1,
    scale bytes uint8 [n / 32])."""
    f = FORMATS[fmt]
    p = np.ascontiguousarray(p, dtype=np.float32)
    assert p.size % BLOCK == 0
    blk = p.reshape(-1, BLOCK)
    bad = ~np.isfinite(blk).all(axis=1)
    amax = np.where(bad, 0.0, np.abs(np.where(np.isfinite(blk), blk, 0)).max(axis=1).astype(np.float64))
    zero = amax == 0
    _, ex = np.frexp(np.where(zero, 1.0, amax))          # amax = m 2^ex, m in [0.5, 1): floor(log2) = ex - 1
    e = ex.astype(np.int64) - 1 - f["emax"]
    sb = np.where(zero, 0, scale_byte(e)).astype(np.uint8)
    e_used = sb.astype(np.int64) - 127                   # the clamped exponent is the one applied
    scaled = np.ldexp(np.where(bad[:, None], 0.0, blk).astype(np.float64), (-e_used)[:, None].astype(np.int32))
    code = round_to_grid(np.abs(scaled), fmt)
    sign = np.signbit(blk).astype(np.uint8) << (f["bits"] - 1)
    code = np.where(bad[:, None], 0, code | sign).astype(np.uint8)
    sb = np.where(bad, 255, sb).astype(np.uint8)
    return code.reshape(-1), sb


def dequantize(codes: np.ndarray, scales: np.ndarray, fmt: str) -> np.ndarray:
    """D(q): float32 [n]; scale byte 255 -> NaN for the whole block."""
    f = FORMATS[fmt]
    codes = np.asarray(codes, dtype=np.uint8).reshape(-1, BLOCK)
    scales = np.asarray(scales, dtype=np.uint8)
    mag = magnitude_table(fmt)[codes & ((1 << (f["bits"] - 1)) - 1)]
    val = np.where(codes >> (f["bits"] - 1), -mag, mag)
    with np.errstate(invalid="ignore"):
        out = np.ldexp(val, (scales.astype(np.int32) - 127)[:, None])
    out = np.where((scales == 255)[:, None], np.nan, out)
    return out.astype(np.float32).reshape(-1)


def region_bytes(region_elems: int, fmt: str) -> int:
    assert region_elems % 512 == 0
    return region_elems * FORMATS[fmt]["bits"] // 8 + region_elems // BLOCK


def pack(codes: np.ndarray, scales: np.ndarray, fmt: str, region_elems: int) -> np.ndarray:
    """Regions back to back, each its payload then its scale bytes."""
    n = codes.size
    assert n % region_elems == 0 and region_elems % 512 == 0
    out = []
    for r in range(n // region_elems):
        c = codes[r * region_elems:(r + 1) * region_elems]
        if fmt == "mxfp4":
            c = (c[0::2] | (c[1::2] << 4)).astype(np.uint8)
        out += [c, scales[r * region_elems // BLOCK:(r + 1) * region_elems // BLOCK]]
    return np.concatenate(out).astype(np.uint8) if out else np.zeros(0, dtype=np.uint8)


def unpack(packed: np.ndarray, fmt: str, region_elems: int):
    """Inverse of pack: (codes [n], scales [n / 32])."""
    rb = region_bytes(region_elems, fmt)
    packed = np.asarray(packed, dtype=np.uint8)
    assert packed.size % rb == 0
    pay = region_elems * FORMATS[fmt]["bits"] // 8
    codes, scales = [], []
    for r in range(packed.size // rb):
        reg = packed[r * rb:(r + 1) * rb]
        c = reg[:pay]
        if fmt == "mxfp4":
            c = np.stack([c & 0xf, c >> 4], axis=1).reshape(-1)
        codes.append(c)
        scales.append(reg[pay:])
    return np.concatenate(codes), np.concatenate(scales)


def ef_step(p: np.ndarray, residual: np.ndarray | None, fmt: str):
    """One quantization with error feedback: p' = p + r (one fp32 add), q = Q(p'), r' = p' - D(q)
    (one fp32 subtract). residual None: no feedback. Returns (codes, scales, D(q), r' or None)."""
    p = np.asarray(p, dtype=np.float32)
    if residual is not None:
        p = (p + np.asarray(residual, dtype=np.float32)).astype(np.float32)
    codes, scales = quantize(p, fmt)
    d = dequantize(codes, scales, fmt)
    with np.errstate(invalid="ignore"):
        new = None if residual is None else (p - d).astype(np.float32)
    return codes, scales, d, new


class NumpyQuantKernels:
    """Stand-in for ops on CPU tensors (ShardedOuterSync's kernels= seam): the oracle's partial and
    SGD, this module's quantizer between them."""

    def __init__(self, oracle):
        self.o = oracle

    def delta_partial_q(self, theta, workers, k_total, packed, region_elems, fmt, residual=None):
        import torch
        acc = torch.zeros(theta.numel(), dtype=torch.float32)
        self.o.delta_partial(theta, workers, k_total, acc, False)
        codes, scales, _, new = ef_step(acc.numpy(), None if residual is None else residual.numpy(), fmt)
        if residual is not None:
            residual.copy_(torch.from_numpy(new))
        packed.copy_(torch.from_numpy(pack(codes, scales, fmt, region_elems)))

    def sgd_apply_sum_q(self, theta, regions, fmt, momentum, has_momentum, lr, mu, nesterov):
        import torch
        total = None
        for reg in regions:
            d = torch.from_numpy(dequantize(*unpack(reg.numpy(), fmt, theta.numel()), fmt))
            total = d if total is None else total.add_(d)
        self.o.sgd_apply(theta, total, momentum, has_momentum, lr, mu, nesterov)
