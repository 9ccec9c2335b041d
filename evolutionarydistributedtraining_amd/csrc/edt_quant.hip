// edt_quant.hip — the block-quantized partial exchange of the sharded outer step (the "reduce_q"
// schedule of distributed.ShardedOuterSync): phase 1 forms each rank's fp32 pseudo-gradient partial
// (edt_delta_partial's, by the same code: edt_step.h) and writes it as OCP MX blocks — MXFP8 (E4M3
// elements) or MXFP4 (E2M1 elements), 32 elements per E8M0 scale byte — without the fp32 partial ever
// reaching HBM; phase 2 dequantizes the owned shard's N regions, sums them in rank order and runs
// the SGD step (edt_sgd_apply_sum's, by the same code). With the quantized gather (gather_format) the
// owner runs phase 2' instead: the same step, but theta is left alone and the update theta' - theta
// is written as one more region (sharded error feedback); phase 3 then adds the dequantized updates
// of a whole bucket to theta on every rank. The reference ships checkpoints over a shared disk
// (EDT_LM/diloco.py:231-235) and has no wire format; this one is defined here and in DESIGN.md §3.
//
// Wire format (the definition; tests/quant_reference.py restates it in numpy)
//   block     32 consecutive elements of a rank's fp32 partial share one E8M0 scale byte (bias 127)
//   scale     e = floor(log2(amax)) - emax, emax = 8 (E4M3) / 2 (E2M1); byte = clamp(e + 127, 0, 254);
//             an all-zero block (+-0) stores byte 0
//   elements  v * 2^-e rounded to nearest-even onto the element grid, saturating at +-448 / +-6
//             (never NaN); the sign is kept, -0 and values that round to zero included
//   non-finite  a block holding any NaN or +-Inf stores scale byte 255 and elements of code 0; every
//             element of it dequantizes to NaN
//   packing   MXFP8: one byte per element; MXFP4: element 2i in the low nibble, 2i+1 in the high
//             nibble. A region of R elements (R % 512 == 0) is R*bits/8 payload bytes, then R/32
//             scale bytes: both start 16-byte aligned
//   D(q)      elem * 2^e, exact in fp32
//   fp32 subnormal inputs are outside the bit-exact contract (finite, within one grid step).
//
// Stochastic rounding (EDT_ROUND_STOCHASTIC, the *_sr entries; tests/sr_reference.py restates it):
// blocks, packing, layout, the non-finite rule and D(q) as above; the encoder differs in
//   scale     e as above, then e + 1 when amax * 2^-e exceeds the element maximum (448 / 6), so no
//             finite element saturates; byte = clamp(e + 127, 0, 254)
//   elements  a = |v| 2^-e, k = max(floor(log2 a), EMIN), q = 2^(k - MB), t = a / q, lo = floor(t),
//             f16 = floor((t - lo) 2^16): the element is (lo + up) q, up = (r16 < f16); the sign is kept
//   r16       Philox4x32-10 (kPhiloxRounds) keyed by the 64-bit seed at counter (g lo, g hi, step,
//             stream), g = global element index / 8 — the lane's 8 elements; element 8g + j takes bits
//             16 (j % 2) .. + 15 of output word j / 2
// Here floor(t 2^16) = lo 2^16 + f16 is one exact fp32 multiply and a truncating convert, and adding
// 0xffff - r16 to it carries into bit 16 exactly when r16 < f16; the magnitude code is then
// ((k - EMIN) << MB) + lo + up for normal and subnormal elements alike (EMIN + BIAS = 1 in both formats).
//
// Mapping: a thread owns 8 consecutive elements (one 16-byte load per bf16 operand, two per fp32
// operand), so 4 adjacent lanes hold a block: the block amax is a two-step xor butterfly, a wave
// covers 512 elements = 16 blocks, and sizes are multiples of 512 so every wave is whole. Payload
// leaves as one 8-byte (MXFP8) or 4-byte (MXFP4) store per lane, contiguous across the wave; the
// 16 scale bytes of a wave are gathered across lanes into four dwords stored by lanes 0/16/32/48.
#include "edt_mx.h"
#include "edt_step.h"

namespace {

struct QWorkers {
    const void* p[EDT_MAX_WORKERS];
};

struct QPartialArgs {
    const void* theta;
    float* residual;         // error feedback (EF): read, added, rewritten (the _to kernel: read only)
    uint8_t* packed;         // [region][payload | scales]
    uint64_t n;
    uint64_t tiles_per_region;   // region_elems / 512
    uint64_t region_bytes;
    uint64_t payload_bytes;      // of one region
    int K;
    float kdiv;
    float kinv;
    QWorkers w;
    __device__ __forceinline__ const void* wp(int k) const { return w.p[k]; }
};

// edt_delta_partial_q_to's block: the new residual goes to a second buffer. It trails, so the
// in-place kernels keep their argument block.
struct QPartialArgsTo : QPartialArgs {
    float* residual_out;
};

// QSr, quant_store (the encoder) and region_of: edt_mx.h, shared with edt_fragment_q.hip

// Phase 1 for the 8 elements at i (a multiple of 8; the wave's 64 lanes cover 512 consecutive ones):
// edt_delta_partial's partial (add_delta per worker, the rounded quotients summed in fp32), quantized.
// res_out: where the new residual goes (EF): a.residual itself, or the _to kernel's second buffer.
template <int GDT, int WDT, int KC, int DIV, int FMT, bool EF, int RND = EDT_ROUND_NEAREST>
__device__ __forceinline__ void partial_q_elems(const QPartialArgs& a, float* res_out, uint64_t i,
                                                const QSr& sr = QSr{}) {
    constexpr int N = kVec;
    float g[N], acc[N];
    ld<GDT, N, (EDT_NT_RMW != 0)>(a.theta, i, g);
#pragma unroll
    for (int j = 0; j < N; ++j) acc[j] = 0.f;
    const int K = KC > 0 ? KC : a.K;
    auto body = [&](int k) { add_delta<GDT, WDT, DIV, N, 4, false>(a, k, g, acc, i); };   // the fp32 partial
    if constexpr (KC > 0) {
#pragma unroll
        for (int k = 0; k < KC; ++k) body(k);
    } else {
#pragma unroll 4
        for (int k = 0; k < K; ++k) body(k);
    }
    if constexpr (EF) {
        float r[N];
        ld<EDT_F32, N>(a.residual, i, r);
#pragma unroll
        for (int j = 0; j < N; ++j) acc[j] = acc[j] + r[j];          // p' = p + r
    }
    const RegionOf r = region_of(i, a.tiles_per_region);
    quant_store<FMT, EF, RND>(acc, res_out, i, a.packed + r.reg * a.region_bytes, r.off, a.payload_bytes, sr);
}

template <int GDT, int WDT, int KC, int DIV, int FMT, bool EF>
__global__ __launch_bounds__(kBlock, EDT_MIN_WAVES) void delta_partial_q_kernel(QPartialArgs a) {
    for_whole_waves(a.n, [&](uint64_t i) { partial_q_elems<GDT, WDT, KC, DIV, FMT, EF>(a, a.residual, i); });
}

// the transactional phase 1 (edt_delta_partial_q_to): the same body with error feedback, the
// residual read from a.residual and the new one written to a.residual_out (another buffer)
template <int GDT, int WDT, int KC, int DIV, int FMT>
__global__ __launch_bounds__(kBlock, EDT_MIN_WAVES) void delta_partial_q_to_kernel(QPartialArgsTo a) {
    for_whole_waves(a.n, [&](uint64_t i) { partial_q_elems<GDT, WDT, KC, DIV, FMT, true>(a, a.residual_out, i); });
}

// phase 1 with stochastic rounding: the same partial, no residual, the draw of each lane's group
template <int GDT, int WDT, int KC, int DIV, int FMT>
__global__ __launch_bounds__(kBlock, EDT_MIN_WAVES) void delta_partial_q_sr_kernel(QPartialArgs a, QSr sr) {
    for_whole_waves(a.n, [&](uint64_t i) {
        partial_q_elems<GDT, WDT, KC, DIV, FMT, false, EDT_ROUND_STOCHASTIC>(a, nullptr, i, sr);
    });
}

// ---------------------------------------------------------------------------------------
// phase 2

// QRegions and ld_q, a region's decoder: edt_mx.h (shared with the statistics pass)

// edt_sgd_apply_sum's step (sgd_from_sum) with every rank's partial dequantized from its region.
// SC (the *_scaled entries, here and in phase 2'): grad = round_g((-sum) * grad_scale); the clip
// coefficient is a trailing argument only the SC instantiations have (`scale` is one float with SC,
// nothing without), so the unscaled kernels keep their argument block, as edt_outer.hip's do.
template <int GDT, int FMT, bool SC = false, class... S>
__global__ __launch_bounds__(kBlock) void sgd_apply_sum_q_kernel(void* theta, QRegions P, int np, void* mom,
                                                                 uint64_t n, SgdScalars s, S... scale) {
    static_assert(sizeof...(S) == (SC ? 1 : 0), "one grad_scale with SC, none without");
    for_whole_waves(n, [&](uint64_t i) {
        float g0[kVec], g[kVec];
        sgd_from_sum<GDT, kVec, SC>(theta, mom, i, s, np, [&](int r, float (&x)[kVec]) { ld_q<FMT>(P.p[r], n, i, x); },
                                    g0, g, scale...);
        st<GDT, kVec>(theta, i, g);
    });
}

// phase 2': sgd_apply_sum_q_kernel's step on the owned shard, but theta stays as it is: the update
// u = theta' - theta (+ the owner's residual with EF) leaves as one region of FOUT blocks, rounded
// to nearest (with or without EF) or stochastically (RND, no residual)
template <int GDT, int FIN, int FOUT, bool EF, int RND, bool SC = false, class... S>
__device__ __forceinline__ void delta_sum_q_body(const void* theta, const QRegions& P, int np, void* mom, uint64_t n,
                                                 const SgdScalars& s, float* residual, uint8_t* packed_out,
                                                 const QSr& sr, S... scale) {
    const uint64_t payload = n / 8 * QFmt<FOUT>::BITS;
    for_whole_waves(n, [&](uint64_t i) {
        float g0[kVec], g[kVec], u[kVec];
        sgd_from_sum<GDT, kVec, SC>(theta, mom, i, s, np, [&](int r, float (&x)[kVec]) { ld_q<FIN>(P.p[r], n, i, x); },
                                    g0, g, scale...);
#pragma unroll
        for (int j = 0; j < kVec; ++j) u[j] = g[j] - g0[j];               // u = theta' - theta
        if constexpr (EF) {
            float r[kVec];
            ld<EDT_F32, kVec>(residual, i, r);
#pragma unroll
            for (int j = 0; j < kVec; ++j) u[j] = u[j] + r[j];            // u' = u + r_g
        }
        quant_store<FOUT, EF, RND>(u, residual, i, packed_out, i, payload, sr);
    });
}

template <int GDT, int FIN, int FOUT, bool EF, bool SC = false, class... S>
__global__ __launch_bounds__(kBlock) void sgd_delta_sum_q_kernel(const void* theta, QRegions P, int np, void* mom,
                                                                 uint64_t n, SgdScalars s, float* residual,
                                                                 uint8_t* packed_out, S... scale) {
    static_assert(sizeof...(S) == (SC ? 1 : 0), "one grad_scale with SC, none without");
    delta_sum_q_body<GDT, FIN, FOUT, EF, EDT_ROUND_NEAREST, SC>(theta, P, np, mom, n, s, residual, packed_out, QSr{},
                                                                scale...);
}

template <int GDT, int FIN, int FOUT, bool SC = false, class... S>
__global__ __launch_bounds__(kBlock) void sgd_delta_sum_q_sr_kernel(const void* theta, QRegions P, int np, void* mom,
                                                                    uint64_t n, SgdScalars s, uint8_t* packed_out,
                                                                    QSr sr, S... scale) {
    static_assert(sizeof...(S) == (SC ? 1 : 0), "one grad_scale with SC, none without");
    delta_sum_q_body<GDT, FIN, FOUT, false, EDT_ROUND_STOCHASTIC, SC>(theta, P, np, mom, n, s, nullptr, packed_out, sr,
                                                                      scale...);
}

// phase 3: theta <- round_g(theta + D(q)) over a bucket of n / region_elems regions back to back.
// BC (edt_apply_delta_q_bcast): the value written to theta also goes, rounded to WDT, to every
// destination of bc — the local workers' refresh in the pass that already holds the new theta in
// registers. A destination element is written by the thread that wrote theta's, and nothing here
// reads a destination.
template <int GDT, int FMT, int WDT = GDT, bool BC = false>
__global__ __launch_bounds__(kBlock) void apply_delta_q_kernel(void* theta, const uint8_t* packed, uint64_t n,
                                                               uint64_t tiles_per_region, uint64_t region_bytes,
                                                               std::conditional_t<BC, BcastDst, NoBcast> bc) {
    for_whole_waves(n, [&](uint64_t i) {
        const RegionOf r = region_of(i, tiles_per_region);
        float g[kVec], d[kVec];
        ld<GDT, kVec>(theta, i, g);
        ld_q<FMT>(packed + r.reg * region_bytes, tiles_per_region << 9, r.off, d);
#pragma unroll
        for (int j = 0; j < kVec; ++j) g[j] = g[j] + d[j];
        rnd<GDT>(g);
        st<GDT, kVec>(theta, i, g);
        if constexpr (BC) st_bcast<WDT, kVec>(bc, i, g);
    });
}

// ---------------------------------------------------------------------------------------
// launch helpers (sr: the stochastic-rounding kernel; else nearest, with error feedback when there
// is a residual)

// residual_out: the _to kernel (error feedback into a second buffer); null: in place
int launch_partial_q(int gdt, int wdt, int fmt, const QPartialArgs& a, const QSr* sr, bool div_exact, hipStream_t s,
                     float* residual_out = nullptr) {
    const unsigned g = grid_for(a.n, true);
    return with_pair(gdt, wdt, [&](auto G, auto W) {
        return with_fmt(fmt, [&](auto F) {
            return with_kc_div<KC_QUANT>(a.K, div_exact, [&](auto KC, auto DIV) {
                constexpr int GDT = decltype(G)::value, WDT = decltype(W)::value, FMT = decltype(F)::value;
                constexpr int KCV = decltype(KC)::value, DIVV = decltype(DIV)::value;
                if (residual_out) {
                    QPartialArgsTo to;
                    static_cast<QPartialArgs&>(to) = a;
                    to.residual_out = residual_out;
                    delta_partial_q_to_kernel<GDT, WDT, KCV, DIVV, FMT><<<g, kBlock, 0, s>>>(to);
                    return check_launch("delta_partial_q_to_kernel");
                }
                if (sr) {
                    delta_partial_q_sr_kernel<GDT, WDT, KCV, DIVV, FMT><<<g, kBlock, 0, s>>>(a, *sr);
                    return check_launch("delta_partial_q_sr_kernel");
                }
                return with_bool(a.residual != nullptr, [&](auto EF) {
                    delta_partial_q_kernel<GDT, WDT, KCV, DIVV, FMT, decltype(EF)::value><<<g, kBlock, 0, s>>>(a);
                    return check_launch("delta_partial_q_kernel");
                });
            });
        });
    });
}

// scale: the scaled entries' clip coefficient (the SC instantiations); null: the plain kernels
int launch_delta_sum_q(int gdt, int fmt_in, int fmt_out, const void* theta, const QRegions& P, int np, void* mom,
                       uint64_t n, const SgdScalars& sc, float* residual, uint8_t* out, const QSr* sr,
                       const float* scale, hipStream_t s) {
    const unsigned g = grid_for(n, true);
    return with_dtype(gdt, [&](auto G) {
        return with_fmt(fmt_in, [&](auto FI) {
            return with_fmt(fmt_out, [&](auto FO) {
                constexpr int GDT = decltype(G)::value, FIN = decltype(FI)::value, FOUT = decltype(FO)::value;
                if (sr) {
                    if (scale)
                        sgd_delta_sum_q_sr_kernel<GDT, FIN, FOUT, true>
                            <<<g, kBlock, 0, s>>>(theta, P, np, mom, n, sc, out, *sr, *scale);
                    else
                        sgd_delta_sum_q_sr_kernel<GDT, FIN, FOUT><<<g, kBlock, 0, s>>>(theta, P, np, mom, n, sc, out, *sr);
                    return check_launch("sgd_delta_sum_q_sr_kernel");
                }
                return with_bool(residual != nullptr, [&](auto EF) {
                    if (scale)
                        sgd_delta_sum_q_kernel<GDT, FIN, FOUT, decltype(EF)::value, true>
                            <<<g, kBlock, 0, s>>>(theta, P, np, mom, n, sc, residual, out, *scale);
                    else
                        sgd_delta_sum_q_kernel<GDT, FIN, FOUT, decltype(EF)::value>
                            <<<g, kBlock, 0, s>>>(theta, P, np, mom, n, sc, residual, out);
                    return check_launch("sgd_delta_sum_q_kernel");
                });
            });
        });
    });
}

inline QSr make_sr(uint64_t seed, uint64_t step, uint32_t stream_id, uint64_t elem_base) {
    QSr sr;
    sr.key0 = (uint32_t)seed;
    sr.key1 = (uint32_t)(seed >> 32);
    sr.step = (uint32_t)step;
    sr.stream = stream_id;
    sr.group_base = elem_base / 8;
    return sr;
}

// ---------------------------------------------------------------------------------------
// argument checks the entries share

// check_fmt, check_regions: edt_mx.h

int check_one_region(uint64_t n) {
    if (n % 512) return fail(EDT_ERR_ARG, "n = %llu is not a multiple of 512 (one region)", (unsigned long long)n);
    return EDT_OK;
}

int check_elem_base(uint64_t elem_base) {
    if (elem_base % 8)
        return fail(EDT_ERR_ARG, "elem_base %llu is not a multiple of 8 (one lane's group of elements)",
                    (unsigned long long)elem_base);
    return EDT_OK;
}

}  // namespace

extern "C" {

uint64_t edt_q_region_bytes(uint64_t region_elems, int fmt) {
    const int bits = fmt_bits(fmt);
    if (!bits || region_elems % 512) return 0;
    return region_elems / 8 * bits + region_elems / 32;
}

// edt_delta_partial_q (sr null), edt_delta_partial_q_sr and edt_delta_partial_q_to (residual_out:
// another buffer than residual): one validation, one argument block
static int delta_partial_q_impl(const void* theta_g, int gdt, const void* const* theta_k, int wdt, int K_local,
                                int K_total, uint64_t n, uint64_t region_elems, int fmt, float* residual, void* packed,
                                const QSr* sr, uint64_t elem_base, void* stream, float* residual_out = nullptr) {
    g_err[0] = 0;
    if (!valid_pair(gdt, wdt)) return fail(EDT_ERR_ARG, "unsupported dtype pair (gdt/wdt)");
    if (int rc = check_fmt(fmt)) return rc;
    if (K_local < 1 || K_local > EDT_MAX_WORKERS)
        return fail(EDT_ERR_ARG, "worker count %d out of range [1, %d]", K_local, EDT_MAX_WORKERS);
    if (K_total < 1) return fail(EDT_ERR_ARG, "total worker count %d < 1", K_total);
    if (int rc = check_regions(n, region_elems)) return rc;
    if (int rc = check_elem_base(elem_base)) return rc;
    if (!theta_k) return fail(EDT_ERR_ARG, "theta_k is null");
    if (n == 0) return EDT_OK;
    if (!theta_g) return fail(EDT_ERR_ARG, "theta_g is null");
    if (!packed) return fail(EDT_ERR_ARG, "packed is null");
    QPartialArgs a;
    memset(&a, 0, sizeof(a));
    bool al = aligned16(theta_g) && aligned16(packed) && aligned16(residual) && aligned16(residual_out);
    if (int rc = fill_table(a.w.p, theta_k, K_local, "theta_k", al)) return rc;
    if (!al) return fail(EDT_ERR_ARG, "the quantized partial needs 16-byte aligned operands");
    a.theta = theta_g;
    a.residual = residual;
    a.packed = static_cast<uint8_t*>(packed);
    a.n = n;
    a.tiles_per_region = region_elems / 512;
    a.region_bytes = edt_q_region_bytes(region_elems, fmt);
    a.payload_bytes = region_elems / 8 * fmt_bits(fmt);
    a.K = K_local;
    a.kdiv = (float)K_total;
    a.kinv = 1.0f / (float)K_total;
    return launch_partial_q(gdt, wdt, fmt, a, sr, !is_pow2(K_total), (hipStream_t)stream, residual_out);
}

int edt_delta_partial_q(const void* theta_g, int gdt, const void* const* theta_k, int wdt, int K_local,
                        int K_total, uint64_t n, uint64_t region_elems, int fmt, float* residual, void* packed,
                        void* stream) {
    return delta_partial_q_impl(theta_g, gdt, theta_k, wdt, K_local, K_total, n, region_elems, fmt, residual, packed,
                                nullptr, 0, stream);
}

int edt_delta_partial_q_to(const void* theta_g, int gdt, const void* const* theta_k, int wdt, int K_local,
                           int K_total, uint64_t n, uint64_t region_elems, int fmt, const float* residual_in,
                           float* residual_out, void* packed, void* stream) {
    g_err[0] = 0;
    if (n != 0 && (!residual_in || !residual_out))
        return fail(EDT_ERR_ARG, "residual_in / residual_out is null (without error feedback: edt_delta_partial_q)");
    float* in = const_cast<float*>(residual_in);       // the _to kernel only reads it
    if (residual_in == residual_out)                    // in place: edt_delta_partial_q itself
        return delta_partial_q_impl(theta_g, gdt, theta_k, wdt, K_local, K_total, n, region_elems, fmt, in, packed,
                                    nullptr, 0, stream);
    if (bytes_overlap(residual_in, n * sizeof(float), residual_out, n * sizeof(float)))
        return fail(EDT_ERR_ARG, "residual_out overlaps residual_in (the same buffer, or clear of it)");
    return delta_partial_q_impl(theta_g, gdt, theta_k, wdt, K_local, K_total, n, region_elems, fmt, in, packed,
                                nullptr, 0, stream, residual_out);
}

int edt_delta_partial_q_sr(const void* theta_g, int gdt, const void* const* theta_k, int wdt, int K_local,
                           int K_total, uint64_t n, uint64_t region_elems, int fmt, void* packed, uint64_t seed,
                           uint64_t step, uint32_t stream_id, uint64_t elem_base, void* stream) {
    const QSr sr = make_sr(seed, step, stream_id, elem_base);
    return delta_partial_q_impl(theta_g, gdt, theta_k, wdt, K_local, K_total, n, region_elems, fmt, nullptr, packed,
                                &sr, elem_base, stream);
}

// edt_sgd_apply_sum_q (scale null) and edt_sgd_apply_sum_q_scaled (the clip coefficient is checked
// first, so a refused call writes nothing)
static int sgd_apply_sum_q_impl(void* theta_g, int gdt, const void* const* regions, int nacc, int fmt, void* momentum,
                                int has_momentum, uint64_t n, double lr, double momentum_coef, int nesterov,
                                const float* scale, void* stream) {
    g_err[0] = 0;
    if (int rc = check_master_dtype(gdt)) return rc;
    if (int rc = check_fmt(fmt)) return rc;
    if (scale)
        if (int rc = check_grad_scale(*scale)) return rc;
    if (int rc = check_partial_count(nacc)) return rc;
    if (int rc = check_one_region(n)) return rc;
    if (n == 0) return EDT_OK;
    if (!theta_g || !regions) return fail(EDT_ERR_ARG, "null buffer");
    SgdScalars s;
    if (int rc = shard_sgd(s, gdt, lr, momentum_coef, has_momentum, nesterov, momentum)) return rc;
    QRegions P;
    memset(&P, 0, sizeof(P));
    bool al = aligned16(theta_g) && (!s.use_momentum || aligned16(momentum));
    if (int rc = fill_table(P.p, regions, nacc, "regions", al)) return rc;
    if (!al) return fail(EDT_ERR_ARG, "the quantized sum needs 16-byte aligned operands");
    const unsigned g = grid_for(n, true);
    hipStream_t st = (hipStream_t)stream;
    return with_dtype(gdt, [&](auto G) {
        return with_fmt(fmt, [&](auto F) {
            if (scale)
                sgd_apply_sum_q_kernel<decltype(G)::value, decltype(F)::value, true>
                    <<<g, kBlock, 0, st>>>(theta_g, P, nacc, momentum, n, s, *scale);
            else
                sgd_apply_sum_q_kernel<decltype(G)::value, decltype(F)::value>
                    <<<g, kBlock, 0, st>>>(theta_g, P, nacc, momentum, n, s);
            return check_launch("sgd_apply_sum_q_kernel");
        });
    });
}

int edt_sgd_apply_sum_q(void* theta_g, int gdt, const void* const* regions, int nacc, int fmt, void* momentum,
                        int has_momentum, uint64_t n, double lr, double momentum_coef, int nesterov, void* stream) {
    return sgd_apply_sum_q_impl(theta_g, gdt, regions, nacc, fmt, momentum, has_momentum, n, lr, momentum_coef, nesterov,
                                nullptr, stream);
}

int edt_sgd_apply_sum_q_scaled(void* theta_g, int gdt, const void* const* regions, int nacc, int fmt, void* momentum,
                               int has_momentum, uint64_t n, double lr, double momentum_coef, int nesterov,
                               float grad_scale, void* stream) {
    return sgd_apply_sum_q_impl(theta_g, gdt, regions, nacc, fmt, momentum, has_momentum, n, lr, momentum_coef, nesterov,
                                &grad_scale, stream);
}

// edt_sgd_delta_sum_q (sr null) and edt_sgd_delta_sum_q_sr; scale: their scaled forms' coefficient
static int sgd_delta_sum_q_impl(const void* theta_g, int gdt, const void* const* regions, int nacc, int fmt_in,
                                void* momentum, int has_momentum, uint64_t n, double lr, double momentum_coef,
                                int nesterov, float* residual, void* packed_out, int fmt_out, const QSr* sr,
                                uint64_t elem_base, void* stream, const float* scale = nullptr) {
    g_err[0] = 0;
    if (int rc = check_master_dtype(gdt)) return rc;
    if (scale)
        if (int rc = check_grad_scale(*scale)) return rc;
    if (int rc = check_fmt(fmt_in)) return rc;
    if (int rc = check_fmt(fmt_out)) return rc;
    if (int rc = check_partial_count(nacc)) return rc;
    if (int rc = check_one_region(n)) return rc;
    if (int rc = check_elem_base(elem_base)) return rc;
    if (n == 0) return EDT_OK;
    if (!theta_g || !regions) return fail(EDT_ERR_ARG, "null buffer");
    if (!packed_out) return fail(EDT_ERR_ARG, "packed_out is null");
    SgdScalars s;
    if (int rc = shard_sgd(s, gdt, lr, momentum_coef, has_momentum, nesterov, momentum)) return rc;
    QRegions P;
    memset(&P, 0, sizeof(P));
    bool al = aligned16(theta_g) && (!s.use_momentum || aligned16(momentum)) && aligned16(residual) && aligned16(packed_out);
    if (int rc = fill_table(P.p, regions, nacc, "regions", al)) return rc;
    if (!al) return fail(EDT_ERR_ARG, "the quantized update needs 16-byte aligned operands");
    return launch_delta_sum_q(gdt, fmt_in, fmt_out, theta_g, P, nacc, momentum, n, s, residual,
                              static_cast<uint8_t*>(packed_out), sr, scale, (hipStream_t)stream);
}

int edt_sgd_delta_sum_q(const void* theta_g, int gdt, const void* const* regions, int nacc, int fmt_in, void* momentum,
                        int has_momentum, uint64_t n, double lr, double momentum_coef, int nesterov, float* residual,
                        void* packed_out, int fmt_out, void* stream) {
    return sgd_delta_sum_q_impl(theta_g, gdt, regions, nacc, fmt_in, momentum, has_momentum, n, lr, momentum_coef,
                                nesterov, residual, packed_out, fmt_out, nullptr, 0, stream);
}

int edt_sgd_delta_sum_q_sr(const void* theta_g, int gdt, const void* const* regions, int nacc, int fmt_in,
                           void* momentum, int has_momentum, uint64_t n, double lr, double momentum_coef, int nesterov,
                           void* packed_out, int fmt_out, uint64_t seed, uint64_t step, uint32_t stream_id,
                           uint64_t elem_base, void* stream) {
    const QSr sr = make_sr(seed, step, stream_id, elem_base);
    return sgd_delta_sum_q_impl(theta_g, gdt, regions, nacc, fmt_in, momentum, has_momentum, n, lr, momentum_coef,
                                nesterov, nullptr, packed_out, fmt_out, &sr, elem_base, stream);
}

int edt_sgd_delta_sum_q_scaled(const void* theta_g, int gdt, const void* const* regions, int nacc, int fmt_in,
                               void* momentum, int has_momentum, uint64_t n, double lr, double momentum_coef,
                               int nesterov, float* residual, void* packed_out, int fmt_out, float grad_scale,
                               void* stream) {
    return sgd_delta_sum_q_impl(theta_g, gdt, regions, nacc, fmt_in, momentum, has_momentum, n, lr, momentum_coef,
                                nesterov, residual, packed_out, fmt_out, nullptr, 0, stream, &grad_scale);
}

int edt_sgd_delta_sum_q_sr_scaled(const void* theta_g, int gdt, const void* const* regions, int nacc, int fmt_in,
                                  void* momentum, int has_momentum, uint64_t n, double lr, double momentum_coef,
                                  int nesterov, void* packed_out, int fmt_out, uint64_t seed, uint64_t step,
                                  uint32_t stream_id, uint64_t elem_base, float grad_scale, void* stream) {
    const QSr sr = make_sr(seed, step, stream_id, elem_base);
    return sgd_delta_sum_q_impl(theta_g, gdt, regions, nacc, fmt_in, momentum, has_momentum, n, lr, momentum_coef,
                                nesterov, nullptr, packed_out, fmt_out, &sr, elem_base, stream, &grad_scale);
}

// edt_apply_delta_q (nbcast = 0: bcast and wdt unused) and edt_apply_delta_q_bcast: one validation
static int apply_delta_q_impl(void* theta_g, int gdt, const void* packed, uint64_t n, uint64_t region_elems, int fmt,
                              void* const* bcast, int wdt, int nbcast, void* stream) {
    if (int rc = check_master_dtype(gdt)) return rc;
    if (int rc = check_fmt(fmt)) return rc;
    if (int rc = check_regions(n, region_elems)) return rc;
    if (n == 0) return EDT_OK;
    if (!theta_g) return fail(EDT_ERR_ARG, "theta_g is null");
    if (!packed) return fail(EDT_ERR_ARG, "packed is null");
    const uint64_t tpr = region_elems / 512, rb = edt_q_region_bytes(region_elems, fmt);
    bool al = aligned16(theta_g) && aligned16(packed);
    BcastDst bc;
    if (nbcast > 0)
        if (int rc = fill_bcast(bc, bcast, nbcast, n, wdt, theta_g, n * (gdt == EDT_BF16 ? 2 : 4), packed,
                                n / region_elems * rb, al))
            return rc;
    if (!al) return fail(EDT_ERR_ARG, "the quantized update needs 16-byte aligned operands");
    const unsigned g = grid_for(n, true);
    hipStream_t st = (hipStream_t)stream;
    const uint8_t* q = static_cast<const uint8_t*>(packed);
    if (nbcast > 0)
        return with_pair(gdt, wdt, [&](auto G, auto W) {
            return with_fmt(fmt, [&](auto F) {
                apply_delta_q_kernel<decltype(G)::value, decltype(F)::value, decltype(W)::value, true>
                    <<<g, kBlock, 0, st>>>(theta_g, q, n, tpr, rb, bc);
                return check_launch("apply_delta_q_kernel");
            });
        });
    return with_dtype(gdt, [&](auto G) {
        return with_fmt(fmt, [&](auto F) {
            apply_delta_q_kernel<decltype(G)::value, decltype(F)::value>
                <<<g, kBlock, 0, st>>>(theta_g, q, n, tpr, rb, NoBcast{});
            return check_launch("apply_delta_q_kernel");
        });
    });
}

int edt_apply_delta_q(void* theta_g, int gdt, const void* packed, uint64_t n, uint64_t region_elems, int fmt,
                      void* stream) {
    g_err[0] = 0;
    return apply_delta_q_impl(theta_g, gdt, packed, n, region_elems, fmt, nullptr, gdt, 0, stream);
}

int edt_apply_delta_q_bcast(void* theta_g, int gdt, const void* packed, uint64_t n, uint64_t region_elems, int fmt,
                            void* const* bcast, int wdt, int nbcast, void* stream) {
    g_err[0] = 0;
    if (!valid_pair(gdt, wdt)) return fail(EDT_ERR_ARG, "unsupported dtype pair (gdt/wdt)");
    if (int rc = check_bcast_count(nbcast)) return rc;
    return apply_delta_q_impl(theta_g, gdt, packed, n, region_elems, fmt, bcast, wdt, nbcast, stream);
}

}  // extern "C"
