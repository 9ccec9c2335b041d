// edt_mx.h — the decoder of the quantized exchange's wire format (edt_quant.hip holds the format's
// definition and its encoders): the element formats' parameters, a magnitude code's value, and
// ld_q, a lane's 8 elements of a packed region as fp32. One text for every kernel that reads
// packed regions: the quantized steps (edt_quant.hip) and the statistics of the mean they apply
// (edt_stats.hip, edt_partial_sum_stats_q), whose bit-for-bit agreement rests on it.
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

}  // namespace
