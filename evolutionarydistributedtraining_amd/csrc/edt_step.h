// edt_step.h — the one text of the outer step's pieces that the fused kernels (edt_outer.hip) and
// the quantized sharded kernels (edt_quant.hip) both run: a worker's delta added to the sum, the
// rank-ordered sum of partials and the SGD step from it, the two grid-stride drivers, and the host
// checks the sharded entries share (the runtime-code -> compile-time-tag dispatch is edt_common.h's,
// with every unit's). Their bit-for-bit agreement across the fp32 and the quantized schedules rests
// on this file: a variant of the step is written here once.
#pragma once

#include "edt_common.h"

namespace {

// ---------------------------------------------------------------------------------------
// grid-stride drivers

// Vector body + scalar tail: f(Int<kVec>, i) over the whole groups of 8 elements of [0, n), then
// f(Int<1>, i) over the < 8 elements left (N == kVec); N == 1: f(Int<1>, i) over every element
// (operands that are not all 16-byte aligned).
template <int N, class F>
__device__ __forceinline__ void for_vec_tail(uint64_t n, F&& f) {
    const uint64_t stride = (uint64_t)gridDim.x * kBlock;
    const uint64_t tid = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
    if constexpr (N == kVec) {
        const uint64_t nv = n / kVec;
        for (uint64_t v = tid; v < nv; v += stride) f(Int<kVec>{}, v * kVec);
        const uint64_t t = nv * kVec + tid;      // scalar tail (< 8 elements)
        if (t < n) f(Int<1>{}, t);
    } else {
        for (uint64_t e = tid; e < n; e += stride) f(Int<1>{}, e);
    }
}

// Whole waves only: f(i) for every group of 8 elements of [0, n). The quantizing kernels shuffle
// across the 4 lanes of a block and the 16 lanes of a scale dword, so no lane of a wave may leave
// the loop alone: n % 512 == 0 (the entries check it), hence a wave is in or out as a whole.
template <class F>
__device__ __forceinline__ void for_whole_waves(uint64_t n, F&& f) {
    const uint64_t stride = (uint64_t)gridDim.x * kBlock;
    const uint64_t nv = n / kVec;
    for (uint64_t v = (uint64_t)blockIdx.x * kBlock + threadIdx.x; v < nv; v += stride) f(v * kVec);
}

// ---------------------------------------------------------------------------------------
// the step's shared bodies

// acc += round(round(w_k - g) / K_total) for worker k of the launch, each op in the precision of
// GDT (EDT_LM/diloco.py:243-246): w_k is a.wp(k)'s N elements at i, g the base. a: the launch's
// argument block (wp, kdiv, kinv). DIV = 1: true division by a.kdiv (torch CPU `delta /
// num_models`); DIV = 0: multiply by a.kinv = 1/K_total, bit-identical when K_total is a power of
// two. ROUND_ACC: acc is kept in GDT (rounded after every add); without it the rounded quotients
// are summed in fp32 (the sharded partials).
// The loop over k (KC unrolled, else `unroll 4`) stays with the two callers: a loop counter declared
// in an inlined callee is promoted to a register before the caller's acc, the loop's phi order
// flips, and the generic-K kernels' register allocation moves with it (spills, lost occupancy).
// raw: at most one float[N], which receives w_k as loaded (the fused merge's aliased form blends
// into the value the delta used without loading it again); without it nothing is emitted.
template <int GDT, int WDT, int DIV, int N, int H2, bool ROUND_ACC, class A, class... R>
__device__ __forceinline__ void add_delta(const A& a, int k, const float (&g)[N], float (&acc)[N], uint64_t i,
                                          R&... raw) {
    static_assert(sizeof...(R) <= 1, "at most one copy of the worker's values");
    float w[N];
    ld<WDT, N, nt_worker_loads<WDT, H2>(), H2>(a.wp(k), i, w);
    if constexpr (sizeof...(R) == 1) {
#pragma unroll
        for (int j = 0; j < N; ++j) ((raw[j] = w[j]), ...);
    }
#pragma unroll
    for (int j = 0; j < N; ++j) w[j] = w[j] - g[j];              // trained - base
    rnd<GDT>(w);
    if constexpr (DIV) {
#pragma unroll
        for (int j = 0; j < N; ++j) w[j] = w[j] / a.kdiv;        // delta / num_models
    } else {
#pragma unroll
        for (int j = 0; j < N; ++j) w[j] = w[j] * a.kinv;
    }
    rnd<GDT>(w);
#pragma unroll
    for (int j = 0; j < N; ++j) acc[j] = acc[j] + w[j];          // acc += delta / K
    if constexpr (ROUND_ACC) rnd<GDT>(acc);
}

// add_delta's two halves on values already loaded, for the statistics pass (edt_stats.hip), which
// sums the delta itself and the mean: delta_of is d_k = round(w_k - g) in place, mean_add the rest
// of the chain (d is kept). add_delta keeps its own text: routing it through these two moved the
// register allocation of the quantized partial kernels (the sensitivity noted above); the two
// texts are held together by the test that the fused step's theta equals the statistics' mean.
template <int GDT, int N>
__device__ __forceinline__ void delta_of(float (&w)[N], const float (&g)[N]) {
#pragma unroll
    for (int j = 0; j < N; ++j) w[j] = w[j] - g[j];
    rnd<GDT>(w);
}

template <int GDT, int DIV, bool ROUND_ACC, int N, class A>
__device__ __forceinline__ void mean_add(const A& a, const float (&d)[N], float (&acc)[N]) {
    float w[N];
    if constexpr (DIV) {
#pragma unroll
        for (int j = 0; j < N; ++j) w[j] = d[j] / a.kdiv;
    } else {
#pragma unroll
        for (int j = 0; j < N; ++j) w[j] = d[j] * a.kinv;
    }
    rnd<GDT>(w);
#pragma unroll
    for (int j = 0; j < N; ++j) acc[j] = acc[j] + w[j];
    if constexpr (ROUND_ACC) rnd<GDT>(acc);
}

// a = ((p_0 + p_1) + ...) + p_{np-1} in fp32: the per-rank partials of one shard summed in rank
// order (one fixed order whatever the collective library does). ld_rank(r, x) loads rank r's N
// values: an fp32 ld, or ld_q of a packed region.
template <int N, class LD>
__device__ __forceinline__ void rank_sum(int np, float (&a)[N], LD&& ld_rank) {
    ld_rank(0, a);
    for (int r = 1; r < np; ++r) {
        float x[N];
        ld_rank(r, x);
#pragma unroll
        for (int j = 0; j < N; ++j) a[j] = a[j] + x[j];
    }
}

// The sharded step's phase 2 for the N elements at i: grad = -round_g(rank_sum), then torch's SGD
// step. g0 = theta as loaded, g = theta after the step (in registers: the caller stores g, or the
// update g - g0); the momentum is updated in place. SC: grad = round_g((-a) * grad_scale), the clipped
// form (outer_elems' SC branch: one fp32 multiply, rounded); without it grad_scale is not read.
template <int GDT, int N, bool SC = false, class LD>
__device__ __forceinline__ void sgd_from_sum(const void* theta, void* mom, uint64_t i, const SgdScalars& s, int np,
                                             LD&& ld_rank, float (&g0)[N], float (&g)[N], float grad_scale = 1.f) {
    float a[N], grad[N], b_in[N];
    ld<GDT, N>(theta, i, g0);
    ld_momentum<GDT, N>(mom, i, s, b_in);
    rank_sum(np, a, ld_rank);
    rnd<GDT>(a);
#pragma unroll
    for (int j = 0; j < N; ++j) { grad[j] = -a[j]; g[j] = g0[j]; }   // p.grad = -avg_delta
    if constexpr (SC) {
#pragma unroll
        for (int j = 0; j < N; ++j) grad[j] = grad[j] * grad_scale;
        rnd<GDT>(grad);
    }
    sgd_update<GDT, N>(g, grad, mom, i, s, b_in);
}

// The destinations of a broadcast fused into a pass over theta (edt_apply_delta_q_bcast,
// edt_broadcast_theta): n worker arenas of one dtype. NoBcast is what a kernel without the
// broadcast takes in its place (no bytes).
struct BcastDst {
    void* p[EDT_MAX_WORKERS];
    int n;
};
struct NoBcast {};

// x (the N values just written to theta at i, in registers) rounded to WDT (RNE, torch copy_) into
// every destination: the stores of outer_elems' BC branch, under the same EDT_NT_STORES policy.
template <int WDT, int N>
__device__ __forceinline__ void st_bcast(const BcastDst& d, uint64_t i, const float (&x)[N]) {
#pragma unroll 4
    for (int k = 0; k < d.n; ++k) st<WDT, N, (EDT_NT_STORES != 0)>(d.p[k], i, x);
}

// ---------------------------------------------------------------------------------------
// host validation shared by the sharded entries (same codes, same messages)

inline int check_master_dtype(int gdt) {
    if (gdt != EDT_F32 && gdt != EDT_BF16) return fail(EDT_ERR_ARG, "unsupported dtype");
    return EDT_OK;
}

inline int check_partial_count(int nacc) {
    if (nacc < 1 || nacc > EDT_MAX_WORKERS)
        return fail(EDT_ERR_ARG, "partial count %d out of range [1, %d]", nacc, EDT_MAX_WORKERS);
    return EDT_OK;
}

// the clip coefficient of the scaled entries: finite, in [0, 1] (NaN fails both comparisons)
inline int check_grad_scale(float grad_scale) {
    if (!(grad_scale >= 0.f && grad_scale <= 1.f))
        return fail(EDT_ERR_ARG, "grad_scale %g outside [0, 1]", (double)grad_scale);
    return EDT_OK;
}

// the SGD scalars of a shard's step (n != 0), refusing a missing momentum buffer
inline int shard_sgd(SgdScalars& s, int gdt, double lr, double momentum_coef, int has_momentum, int nesterov,
                     const void* momentum) {
    s = make_sgd(gdt, lr, momentum_coef, has_momentum, nesterov);
    if (s.use_momentum && !momentum) return fail(EDT_ERR_ARG, "momentum buffer is null");
    return EDT_OK;
}

// dst[0 .. count) = src[0 .. count), each checked non-null ("<name>[r] is null"); `aligned` is
// and-ed with their 16-byte alignment
template <class T, class U>
int fill_table(T (&dst)[EDT_MAX_WORKERS], const U* const* src, int count, const char* name, bool& aligned) {
    for (int r = 0; r < count; ++r) {
        if (!src[r]) return fail(EDT_ERR_ARG, "%s[%d] is null", name, r);
        dst[r] = static_cast<T>(src[r]);
        aligned = aligned && aligned16(src[r]);
    }
    return EDT_OK;
}

inline int check_bcast_count(int nbcast) {
    if (nbcast < 0 || nbcast > EDT_MAX_WORKERS)
        return fail(EDT_ERR_ARG, "broadcast count %d out of range [0, %d]", nbcast, EDT_MAX_WORKERS);
    return EDT_OK;
}

// d = bcast[0 .. nbcast) (nbcast >= 1, n != 0 elements of wdt each): each checked non-null and
// clear of theta_g's theta_bytes ("bcast[k] overlaps theta_g", as edt_outer_step_bcast reports it)
// and of `packed`'s packed_bytes (packed may be null: no such operand); `aligned` is and-ed with
// their 16-byte alignment
inline int fill_bcast(BcastDst& d, void* const* bcast, int nbcast, uint64_t n, int wdt, const void* theta_g,
                      uint64_t theta_bytes, const void* packed, uint64_t packed_bytes, bool& aligned) {
    memset(&d, 0, sizeof(d));
    if (!bcast) return fail(EDT_ERR_ARG, "bcast is null");
    const uint64_t bytes = n * (wdt == EDT_BF16 ? 2 : 4);
    for (int k = 0; k < nbcast; ++k) {
        if (!bcast[k]) return fail(EDT_ERR_ARG, "bcast[%d] is null", k);
        if (bytes_overlap(bcast[k], bytes, theta_g, theta_bytes)) return fail(EDT_ERR_ARG, "bcast[%d] overlaps theta_g", k);
        if (bytes_overlap(bcast[k], bytes, packed, packed_bytes)) return fail(EDT_ERR_ARG, "bcast[%d] overlaps packed", k);
        d.p[k] = bcast[k];
        aligned = aligned && aligned16(bcast[k]);
    }
    d.n = nbcast;
    return EDT_OK;
}

}  // namespace
