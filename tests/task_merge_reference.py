"""numpy restatement of the task-vector merge contract (include/edt_sync.h, DESIGN §3: task_arithmetic /
dare_linear / dare_ties), written from the definition, not from the kernel: `merge_f32` op by op in
float32 (numpy rounds every element-wise operation on its own, no FMA), `merge_f64` the same formulas
in float64 with the same mask and the same fp32 coefficients. The random bits are
tests/sr_reference.random_bits. Beside them, the inputs the CPU and GPU tests share."""
import numpy as np

from tests import sr_reference as SR

# empty, sub-vector, tile edge, chunk edge, chunk + 1; the last one the tests lay out one element off alignment
SIZES = [1, 7, 8, 0, 2047, 2059, 4096, 4097, 13]
# method -> (consensus, density: a number for every (k, t), or "mix": per model and tensor, d = 1 included)
METHODS = {"task_arithmetic": (False, 1.0), "dare_linear": (False, 0.5), "dare_ties": (True, 0.5),
           "dare_ties_mix": (True, "mix")}


def densities(method: str, K: int, T: int, dyadic: bool = False):
    d = METHODS[method][1]
    mix = (1.0, 0.5) if dyadic else (1.0, 0.5, 0.25, 0.9)
    return [[mix[(k + t) % len(mix)] if d == "mix" else d for t in range(T)] for k in range(K)]


def coefficients(weights, dens):
    """(w f32, c f32, drop16) [K, T] from the contract's formulas."""
    w = np.asarray(weights, dtype=np.float64).astype(np.float32)
    drop = np.clip(np.rint((1.0 - np.asarray(dens, dtype=np.float64)) * 65536.0), 0, 65535).astype(np.uint32)
    return w, (w.astype(np.float64) / (1.0 - drop / 65536.0)).astype(np.float32), drop


def keep_masks(sizes, drop16, seed: int, step: int):
    """Per tensor the [K, n] mask r16 >= drop16[k][t], bits of element base_t + i (starts padded to 8)."""
    out, base = [], 0
    for t, n in enumerate(sizes):
        pad = (n + 7) // 8 * 8
        out.append(np.stack([SR.random_bits(seed, step, k, pad, base)[:n] >= drop16[k][t] for k in range(len(drop16))]))
        base += pad
    return out


def round_bf16(x: np.ndarray) -> np.ndarray:
    u = np.ascontiguousarray(x, dtype=np.float32).view(np.uint32).astype(np.uint64)
    return ((u + 0x7fff + ((u >> 16) & 1)) & 0xffff0000).astype(np.uint32).view(np.float32)


def _merge(f, B, M, w, c, keep, lam, consensus, normalize):
    B = B.astype(f)
    A, P, N, WP, WN = (np.zeros(B.shape, dtype=f) for _ in range(5))
    WA, zero = f(0), f(0)
    for k in range(len(M)):
        delta = M[k].astype(f) - B
        tau = np.where(keep[k], f(c[k]) * delta, zero)
        A = A + tau
        P, N = P + np.where(tau > 0, tau, zero), N + np.where(tau < 0, tau, zero)
        WP, WN = WP + np.where(tau > 0, f(w[k]), zero), WN + np.where(tau < 0, f(w[k]), zero)
        WA = WA + f(w[k])
    if consensus:
        num = np.where(A > 0, P, np.where(A < 0, N, A))
        den = np.where(A > 0, WP, np.where(A < 0, WN, f(1)))
    else:
        num, den = A, np.full(B.shape, WA, dtype=f)
    q = num / np.where(np.abs(den) < f(np.float32(1e-8)), f(1), den) if normalize else num
    return B + f(np.float32(lam)) * q, np.sign(A).astype(np.int8), q


def merge_f32(B, M, w, c, keep, lam, consensus, normalize, bf16_out=False):
    """One tensor: B [n], M [K, n] float32 (bf16 widened), w / c [K], keep [K, n] -> (out, the sign of A)."""
    with np.errstate(all="ignore"):
        out, sign, _ = _merge(np.float32, B, M, w, c, keep, lam, consensus, normalize)
    return (round_bf16(out) if bf16_out else out), sign


def merge_f64(B, M, w, c, keep, lam, consensus, normalize):
    """The same in float64, unrounded -> (out, the sign of A, lambda * q)."""
    out, sign, q = _merge(np.float64, B, M, w, c, keep, lam, consensus, normalize)
    return out, sign, float(np.float32(lam)) * q


def bound(B, lq, ref, bf16_out):
    """|out - ref| allowed on the dyadic inputs: three roundings (div, mul, add); bf16 out: + half a bf16 ulp."""
    b = 2.0 ** -23 * (np.abs(B.astype(np.float64)) + 2 * np.abs(lq))
    if bf16_out:
        b = b + np.where(ref == 0, 0.0, 2.0 ** (np.floor(np.log2(np.abs(np.where(ref == 0, 1.0, ref)))) - 8))
    return b


def normal_inputs(K: int, sizes, seed: int = 0):
    """Random normal base, small task vectors; where a model equals the base (tau = 0) the value is bf16-exact."""
    g = np.random.default_rng(seed)
    bases, models = [], []
    for n in sizes:
        b = (g.standard_normal(n) * 0.02).astype(np.float32)
        same = g.random((K, n)) < 0.25
        b = np.where(same.any(axis=0), round_bf16(b), b)
        m = b + (g.standard_normal((K, n)) * 1e-3).astype(np.float32)
        bases.append(b)
        models.append(np.where(same, b, m).astype(np.float32))
    return bases, models


def dyadic_inputs(K: int, sizes, seed: int = 1):
    """Base and deltas integer multiples of 2^-6, exact in bf16 too: with power-of-two weights every sum is exact."""
    g = np.random.default_rng(seed)
    bases = [(g.integers(-100, 101, n) / 64.0).astype(np.float32) for n in sizes]
    models = [(b + g.integers(-28, 29, (K, b.size)) / 64.0).astype(np.float32) for b in bases]
    return bases, models
