// edt_mx.h — the one text of the quantized exchange's wire format (edt_quant.hip's header comment
// holds the format's definition): the element formats' parameters; the decoder — a magnitude code's
// value and ld_q, a lane's 8 elements of a packed region as fp32; the encoder — quant_store, a wave's
// 512 values to codes and scale bytes, with region_of's addressing; and the host checks of a format
// and a region size. Every kernel that reads or writes packed regions runs this text: the quantized
// steps (edt_quant.hip), the statistics of the mean they apply (edt_stats.hip,
// edt_partial_sum_stats_q) and the sharded fragment step's quantized phases (edt_fragment_q.hip),
// whose bit-for-bit agreement rests on it.
#pragma once

#include "edt_common.h"

namespace {

// element formats: mantissa bits, smallest normal exponent, exponent bias, largest magnitude, emax
template <int FMT> struct QFmt;
template <> struct QFmt<EDT_MXFP8> {
    static constexpr int MB = 3, EMIN = -6, BIAS = 7, EMAX = 8, BITS = 8;
    static constexpr float MAXV = 448.f;
};
template <> struct QFmt<EDT_MXFP4> {
    static constexpr int MB = 1, EMIN = 0, BIAS = 1, EMAX = 2, BITS = 4;
    static constexpr float MAXV = 6.f;
};

__device__ __forceinline__ float pow2f(int e) { return __uint_as_float((uint32_t)(e + 127) << 23); }   // -126 <= e <= 127

// magnitude code -> value
template <int FMT>
__device__ __forceinline__ float q_decode(uint32_t c) {
    using F = QFmt<FMT>;
    if (FMT == EDT_MXFP8 && c == 0x7fu) return __builtin_nanf("");                  // OCP E4M3's NaN
    if (c < (1u << F::MB)) return (float)c * pow2f(F::EMIN - F::MB);
    return __uint_as_float((c + ((uint32_t)(127 - F::BIAS) << F::MB)) << (23 - F::MB));
}

// the packed regions a kernel sums in rank order (one per rank; each [payload | scales])
struct QRegions {
    const uint8_t* p[EDT_MAX_WORKERS];
};

// D(q) of the 8 elements at i (a multiple of 8) of a region of n elements
template <int FMT>
__device__ __forceinline__ void ld_q(const uint8_t* region, uint64_t n, uint64_t i, float (&x)[kVec]) {
    using F = QFmt<FMT>;
    uint32_t code[kVec];
    if constexpr (FMT == EDT_MXFP8) {
        const u32x2 v = *reinterpret_cast<const u32x2*>(region + i);
#pragma unroll
        for (int j = 0; j < 4; ++j) { code[j] = (v.x >> (8 * j)) & 0xffu; code[4 + j] = (v.y >> (8 * j)) & 0xffu; }
    } else {
        const uint32_t v = *reinterpret_cast<const uint32_t*>(region + (i >> 1));
#pragma unroll
        for (int j = 0; j < kVec; ++j) code[j] = (v >> (4 * j)) & 0xfu;
    }
    const uint32_t sb = region[n * F::BITS / 8 + (i >> 5)];
    const int e = (int)sb - 127;                         // elem * 2^e as two exact factors
    const float f0 = pow2f(e < -64 ? -64 : e), f1 = pow2f(e < -64 ? e + 64 : 0);
#pragma unroll
    for (int j = 0; j < kVec; ++j) {
        const uint32_t sign = (code[j] >> (F::BITS - 1)) << 31;
        const float mag = q_decode<FMT>(code[j] & ((1u << (F::BITS - 1)) - 1u)) * f0 * f1;
        x[j] = sb == 255u ? __builtin_nanf("") : __uint_as_float(__float_as_uint(mag) | sign);
    }
}

// ---------------------------------------------------------------------------------------
// the encoder

// stochastic rounding: the Philox key (the seed) and what of the counter is the same for a whole call
struct QSr {
    uint32_t key0, key1;     // seed, low and high word
    uint32_t step;           // counter word 2
    uint32_t stream;         // counter word 3
    uint64_t group_base;     // elem_base / 8: the call's first group of 8 elements
};

constexpr int kPhiloxRounds = EDT_PHILOX_ROUNDS;

// Philox4x32 (Salmon et al., SC'11), kPhiloxRounds rounds: counter c, key (k0, k1) -> c
__device__ __forceinline__ void philox4x32(uint32_t (&c)[4], uint32_t k0, uint32_t k1) {
#pragma unroll
    for (int r = 0; r < kPhiloxRounds; ++r) {
        const uint64_t p0 = (uint64_t)0xD2511F53u * c[0], p1 = (uint64_t)0xCD9E8D57u * c[2];
        const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c[1] ^ k0, n2 = (uint32_t)(p0 >> 32) ^ c[3] ^ k1;
        c[0] = n0;
        c[1] = (uint32_t)p1;
        c[2] = n2;
        c[3] = (uint32_t)p0;
        k0 += 0x9E3779B9u;
        k1 += 0xBB67AE85u;
    }
}

// |x| (finite, < 2^(EMAX + 1)) rounded to nearest-even onto the element grid and saturated:
// adding 2^23 q, q the grid step at |x|, makes the fp32 adder round at q.
template <int FMT>
__device__ __forceinline__ float q_round(float a) {
    using F = QFmt<FMT>;
    int k = (int)(__float_as_uint(a) >> 23) - 127;
    k = k < F::EMIN ? F::EMIN : k;
    const float magic = pow2f(k - F::MB + 23);
    const float r = (a + magic) - magic;
    return r > F::MAXV ? F::MAXV : r;
}

// the magnitude code of a grid value r (q_round's result)
template <int FMT>
__device__ __forceinline__ uint32_t q_code(float r) {
    using F = QFmt<FMT>;
    if (r < pow2f(F::EMIN)) return (uint32_t)(r * pow2f(F::MB - F::EMIN));       // zero and subnormals
    return (__float_as_uint(r) >> (23 - F::MB)) - ((uint32_t)(127 - F::BIAS) << F::MB);
}

// The quantize-and-store tail shared by phase 1 and phase 2': the 8 values v at element `off` of the
// region at `base` (off a multiple of 8; the wave's 64 lanes cover 512 consecutive elements of one
// region) become codes under their block's scale; with EF the residual v - D(q) goes to res[i].
// RND = EDT_ROUND_STOCHASTIC (never with EF): the bumped scale and the Philox draw of group
// sr.group_base + i / 8 (i: the element's index inside the call) pick the grid neighbour.
template <int FMT, bool EF, int RND = EDT_ROUND_NEAREST>
__device__ __forceinline__ void quant_store(const float (&acc)[kVec], float* res, uint64_t i, uint8_t* base,
                                            uint64_t off, uint64_t payload_bytes, const QSr& sr = QSr{}) {
    using F = QFmt<FMT>;
    constexpr int N = kVec;
    static_assert(!(EF && RND == EDT_ROUND_STOCHASTIC), "stochastic rounding takes no residual");
    // block amax over the bit patterns of |v| (monotone for finite values; NaN / Inf compare highest)
    uint32_t m = 0;
#pragma unroll
    for (int j = 0; j < N; ++j) {
        const uint32_t u = __float_as_uint(acc[j]) & 0x7fffffffu;
        m = u > m ? u : m;
    }
    uint32_t o = (uint32_t)__shfl_xor((int)m, 1);
    m = o > m ? o : m;
    o = (uint32_t)__shfl_xor((int)m, 2);
    m = o > m ? o : m;
    const bool bad = m >= 0x7f800000u;
    int sb = (int)(m >> 23) - F::EMAX;                   // e + 127
    if constexpr (RND == EDT_ROUND_STOCHASTIC)           // amax * 2^-e > MAXV: the mantissa decides
        sb += (m & 0x7fffffu) > (__float_as_uint(F::MAXV) & 0x7fffffu) ? 1 : 0;
    sb = sb < 0 ? 0 : sb;
    if (bad) sb = 255;
    // v * 2^-e = v * 2^(127 - sb): one exact multiply; back by 2^e as two exact factors, since
    // 2^-127 (scale byte 0) is no normal fp32
    const int up = bad ? 0 : 127 - sb;                   // -125 .. 127
    const float su = pow2f(up);
    const float d0 = pow2f(up > 64 ? -64 : -up), d1 = pow2f(up > 64 ? 64 - up : 0);
    uint32_t code[N];
    float deq[N];
    if constexpr (RND == EDT_ROUND_STOCHASTIC) {
        const uint64_t g = sr.group_base + (i >> 3);
        uint32_t w[4] = {(uint32_t)g, (uint32_t)(g >> 32), sr.step, sr.stream};
        philox4x32(w, sr.key0, sr.key1);
#pragma unroll
        for (int j = 0; j < N; ++j) {
            const uint32_t nr = j & 1 ? ~w[j >> 1] >> 16 : ~w[j >> 1] & 0xffffu;     // 0xffff - r16
            const uint32_t sign = __float_as_uint(acc[j]) & 0x80000000u;
            float ax = __uint_as_float(__float_as_uint(acc[j]) & 0x7fffffffu) * su;
            ax = bad ? 0.f : ax;
            uint32_t kb = __float_as_uint(ax) >> 23;                                  // k + 127
            kb = kb < (uint32_t)(F::EMIN + 127) ? (uint32_t)(F::EMIN + 127) : kb;
            // floor(t 2^16), t = a 2^(MB - k) < 2^(MB + 1): exact product, truncating convert
            const uint32_t fx = (uint32_t)(ax * __uint_as_float(((uint32_t)(2 * 127 + F::MB + 16) - kb) << 23));
            const uint32_t mag = ((kb - (uint32_t)(F::EMIN + 127)) << F::MB) + ((fx + nr) >> 16);
            code[j] = bad ? 0u : (mag | (sign >> (32 - F::BITS)));
        }
    } else {
#pragma unroll
        for (int j = 0; j < N; ++j) {
            const uint32_t sign = __float_as_uint(acc[j]) & 0x80000000u;
            const float ax = __uint_as_float(__float_as_uint(acc[j]) & 0x7fffffffu) * su;
            const float r = q_round<FMT>(bad ? 0.f : ax);
            code[j] = bad ? 0u : (q_code<FMT>(r) | (sign >> (32 - F::BITS)));
            deq[j] = bad ? __builtin_nanf("") : __uint_as_float(__float_as_uint(r * d0 * d1) | sign);   // D(q)
        }
    }
    if constexpr (EF) {
        float r[N];
#pragma unroll
        for (int j = 0; j < N; ++j) r[j] = acc[j] - deq[j];          // r = p' - D(q)
        st<EDT_F32, N, false>(res, i, r);
    }
    if constexpr (FMT == EDT_MXFP8) {
        u32x2 v;
        v.x = code[0] | (code[1] << 8) | (code[2] << 16) | (code[3] << 24);
        v.y = code[4] | (code[5] << 8) | (code[6] << 16) | (code[7] << 24);
        *reinterpret_cast<u32x2*>(base + off) = v;
    } else {
        uint32_t v = 0;
#pragma unroll
        for (int j = 0; j < N; ++j) v |= code[j] << (4 * j);
        *reinterpret_cast<uint32_t*>(base + (off >> 1)) = v;
    }
    // the wave's 16 scale bytes: lanes 4b .. 4b+3 hold block b's; each group of 16 lanes gathers
    // its four into one dword by an or-butterfly, and its first lane stores it
    const unsigned lane = threadIdx.x & 63u;
    uint32_t sw = (uint32_t)sb << (8 * ((lane >> 2) & 3u));
    sw |= (uint32_t)__shfl_xor((int)sw, 4);
    sw |= (uint32_t)__shfl_xor((int)sw, 8);
    if ((lane & 15u) == 0) *reinterpret_cast<uint32_t*>(base + payload_bytes + (off >> 5)) = sw;
}

// Addresses: tile = 512 elements = one wave, and a region is a whole number of tiles. The region
// that element i (of a buffer of regions back to back) lies in, and i's offset inside that region.
struct RegionOf {
    uint64_t reg, off;
};
__device__ __forceinline__ RegionOf region_of(uint64_t i, uint64_t tiles_per_region) {
    const uint64_t tile = i >> 9;
    uint64_t reg;
    if ((tile | tiles_per_region) >> 32) reg = tile / tiles_per_region;
    else reg = (uint32_t)tile / (uint32_t)tiles_per_region;
    return {reg, i - reg * (tiles_per_region << 9)};
}

// ---------------------------------------------------------------------------------------
// host checks of a format and of a buffer of regions (same codes, same messages for every entry)

inline int fmt_bits(int fmt) { return fmt == EDT_MXFP8 ? 8 : fmt == EDT_MXFP4 ? 4 : 0; }

inline int check_fmt(int fmt) {
    if (!fmt_bits(fmt)) return fail(EDT_ERR_ARG, "unknown wire format %d (EDT_MXFP8 or EDT_MXFP4)", fmt);
    return EDT_OK;
}

inline int check_regions(uint64_t n, uint64_t region_elems) {
    if (region_elems == 0 || region_elems % 512)
        return fail(EDT_ERR_ARG, "region_elems %llu is not a positive multiple of 512", (unsigned long long)region_elems);
    if (n % region_elems)
        return fail(EDT_ERR_ARG, "n = %llu is not a whole number of regions of %llu elements", (unsigned long long)n,
                    (unsigned long long)region_elems);
    return EDT_OK;
}

}  // namespace
