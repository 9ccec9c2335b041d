// edt_fragment_q.hip — the sharded fragment step's two quantized phases (Streaming DiLoCo across
// ranks with low-precision outer gradients, sharded_fragments.py with wire_format=), with their C
// ABI entries (include/edt_sync.h):
//   edt_delta_partial_q_frag   phase 1: the local workers' fp32 partial of a fragment-space range,
//                              gathered through the piece table and written as MX regions; the fp32
//                              partial never reaches HBM
//   edt_sgd_sum_q_frag_to      phase 2: the owned shard's received regions dequantized and summed in
//                              rank order, the SGD step; theta is gathered through the piece table
//                              and only read, the new theta goes to a compact fragment-space buffer
// Phase 3 is edt_theta_scatter_mix_list (edt_fragment.hip), unchanged.
//
// Both kernels are indexed in FRAGMENT SPACE, relative to the range's start: a wave covers 512
// consecutive elements — 16 whole blocks, so edt_mx.h's quant_store (the cross-lane amax, the scale
// bytes' gather) applies as it does in edt_quant.hip — and a lane covers 8. The compact operands
// (residual, packed, momentum, out) are indexed directly. The arena operands come through the piece
// table: sorted, disjoint pieces of the range, each with its end, its start and one pointer per
// arena operand, REBASED on the host by the piece's start so that base[i] is element i of the
// range wherever the piece lies. Elements no piece covers are the padding beyond the fragment's
// size: they read as +0 (theta and every worker), so their partial is +0, and nothing of theirs is
// stored to an arena or to the momentum.
//
// Piece lookup: one search per wave, then a linear advance per lane. The piece ends (8 B each) are
// staged in LDS (up to kListLdsMaxPieces, edt_table.h's limit; longer tables are searched in
// global memory); a wave binary-searches the first piece that ends beyond its first element — the
// same addresses in every lane, so the LDS reads broadcast and the branches are uniform — and each
// lane steps forward from there to the piece of its own first element. With real tensors (pieces
// far longer than 512 elements) that is zero or one step; a per-lane search would pay log2(T)
// divergent LDS reads in every lane to save it.
//
// A lane whose 8 elements lie inside one piece all of whose rebased pointers are 16-byte aligned
// takes the vector loads (ld<.., 8>), and runs add_delta / sgd_from_sum exactly as edt_quant.hip's
// flat kernels do. Any other lane gathers: element by element, each from the piece that holds it
// (advancing through tiny and empty pieces), through the same templates at N = 1, as
// edt_fragment.hip's scalar body does. Every value is formed by the same operations in either
// path, so the bits do not depend on the path, on alignment or on how the pieces are cut. The two
// paths rejoin before quant_store's shuffles.
#include "edt_mx.h"
#include "edt_step.h"
#include "edt_table.h"

namespace {

using namespace edt_table;      // kVecFlag: the start[t] bit of a piece whose pointers allow vector loads

// The device table of a launch, 8-byte words: end[T] | start[T] | the pointer columns, rows x T,
// row-major. end and start are relative to the range's first element; end is non-decreasing.
struct FragTable {
    const uint64_t* end;        // T: where piece t ends
    const uint64_t* start;      // T: kVecFlag | where piece t starts
    const uint64_t* cols;       // rebased pointers
    uint64_t T;
    template <class P = void>
    __device__ __forceinline__ P* at(uint64_t row, uint64_t t) const {
        return reinterpret_cast<P*>(static_cast<uintptr_t>(cols[row * T + t]));
    }
};

// the piece ends, in LDS when they fit (every thread of the workgroup calls this once, first)
template <bool LDS>
__device__ __forceinline__ const uint64_t* stage_ends(const FragTable& L) {
    extern __shared__ uint64_t s_end[];
    if constexpr (LDS) {
        for (uint64_t t = threadIdx.x; t < L.T; t += kBlock) s_end[t] = L.end[t];
        __syncthreads();
        return s_end;
    } else {
        return L.end;
    }
}

__device__ __forceinline__ uint64_t wave_uniform(uint64_t x) {
    const uint32_t lo = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)x);
    const uint32_t hi = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)(x >> 32));
    return ((uint64_t)hi << 32) | lo;
}

// The first piece that ends beyond element i's wave (uniform: one search per wave), advanced to the
// first that ends beyond i itself; T: none. Whole waves only (for_whole_waves): lane 0 is active.
__device__ __forceinline__ uint64_t piece_from(const uint64_t* end, uint64_t T, uint64_t i) {
    const uint64_t w0 = wave_uniform(i & ~511ull);
    uint64_t lo = 0, hi = T;
    while (lo < hi) {
        const uint64_t mid = (lo + hi) >> 1;
        if (end[mid] > w0) hi = mid;
        else lo = mid + 1;
    }
    while (lo < T && end[lo] <= i) ++lo;
    return lo;
}

// t (the first piece ending beyond e, from a piece at or before it) and whether it covers e
__device__ __forceinline__ bool covers(const FragTable& L, const uint64_t* end, uint64_t& t, uint64_t e) {
    while (t < L.T && end[t] <= e) ++t;
    return t < L.T && (L.start[t] & ~kVecFlag) <= e;
}

// whether the 8 elements at i lie inside piece t (from piece_from) and may be loaded as vectors
__device__ __forceinline__ bool vector_lane(const FragTable& L, const uint64_t* end, uint64_t t, uint64_t i) {
    if (t >= L.T) return false;
    const uint64_t sf = L.start[t];
    return (sf & kVecFlag) && (sf & ~kVecFlag) <= i && i + kVec <= end[t];
}

// ---------------------------------------------------------------------------------------
// phase 1: edt_delta_partial_list's partial (add_delta per local worker, the rounded quotients
// summed in fp32), edt_delta_partial_q's error feedback and quantization (quant_store).
// columns: theta (row 0) | w (rows 1 .. 1 + K)

struct FragWorkers {                // what add_delta reads of a launch's argument block
    const uint64_t* w;              // the worker rows of the table
    uint64_t T, t;
    float kdiv, kinv;
    __device__ __forceinline__ const void* wp(int k) const {
        return reinterpret_cast<const void*>(static_cast<uintptr_t>(w[(uint64_t)k * T + t]));
    }
};

struct QFragPartial {
    float* residual;             // error feedback (EF): n floats, read, added, rewritten
    uint8_t* packed;             // [region][payload | scales]
    uint64_t n;
    uint64_t tiles_per_region;   // region_elems / 512
    uint64_t region_bytes;
    uint64_t payload_bytes;      // of one region
    int K;
    float kdiv, kinv;
};

template <int GDT, int WDT, int KC, int DIV, int FMT, bool EF, bool LDS>
__global__ __launch_bounds__(kBlock, EDT_MIN_WAVES) void delta_partial_q_frag_kernel(FragTable L, QFragPartial a) {
    const uint64_t* end = stage_ends<LDS>(L);
    const int K = KC > 0 ? KC : a.K;
    for_whole_waves(a.n, [&](uint64_t i) {
        constexpr int N = kVec;
        uint64_t t = piece_from(end, L.T, i);
        float acc[N];
        if (vector_lane(L, end, t, i)) {
            const FragWorkers A = {L.cols + L.T, L.T, t, a.kdiv, a.kinv};
            float g[N];
            ld<GDT, N, (EDT_NT_RMW != 0)>(L.at<const void>(0, t), i, g);
#pragma unroll
            for (int j = 0; j < N; ++j) acc[j] = 0.f;
            if constexpr (KC > 0) {
#pragma unroll
                for (int k = 0; k < KC; ++k) add_delta<GDT, WDT, DIV, N, 4, false>(A, k, g, acc, i);
            } else {
#pragma unroll 4
                for (int k = 0; k < K; ++k) add_delta<GDT, WDT, DIV, N, 4, false>(A, k, g, acc, i);
            }
        } else {
#pragma unroll
            for (int j = 0; j < N; ++j) {
                const uint64_t e = i + j;
                float a1[1] = {0.f};                              // no piece: the padding's +0
                if (covers(L, end, t, e)) {
                    const FragWorkers A = {L.cols + L.T, L.T, t, a.kdiv, a.kinv};
                    float g1[1];
                    ld<GDT, 1, (EDT_NT_RMW != 0)>(L.at<const void>(0, t), e, g1);
#pragma unroll 1
                    for (int k = 0; k < K; ++k) add_delta<GDT, WDT, DIV, 1, 4, false>(A, k, g1, a1, e);
                }
                acc[j] = a1[0];
            }
        }
        if constexpr (EF) {
            float r[N];
            ld<EDT_F32, N>(a.residual, i, r);
#pragma unroll
            for (int j = 0; j < N; ++j) acc[j] = acc[j] + r[j];          // p' = p + r
        }
        const RegionOf r = region_of(i, a.tiles_per_region);
        quant_store<FMT, EF>(acc, a.residual, i, a.packed + r.reg * a.region_bytes, r.off, a.payload_bytes);
    });
}

// ---------------------------------------------------------------------------------------
// phase 2: edt_sgd_apply_sum_q's step (sgd_from_sum over ld_q) on the owned shard; theta through
// the piece table (read only), the momentum and the new theta compact. A padding element's output
// slot is ZEROED (every lane stores its 8 outputs as one vector); its momentum is not written.
// columns: theta (row 0)

template <int GDT, int FMT, bool LDS>
__global__ __launch_bounds__(kBlock) void sgd_sum_q_frag_to_kernel(FragTable L, QRegions P, int np, void* mom, void* out,
                                                                   uint64_t n, SgdScalars s) {
    const uint64_t* end = stage_ends<LDS>(L);
    for_whole_waves(n, [&](uint64_t i) {
        constexpr int N = kVec;
        uint64_t t = piece_from(end, L.T, i);
        float g[N];
        if (vector_lane(L, end, t, i)) {
            float g0[N];
            sgd_from_sum<GDT, N>(L.at<const void>(0, t), mom, i, s, np,
                                 [&](int r, float (&x)[N]) { ld_q<FMT>(P.p[r], n, i, x); }, g0, g);
        } else {
            float sum[N];                                         // the 8 rank-ordered sums, decoded once
            rank_sum(np, sum, [&](int r, float (&x)[N]) { ld_q<FMT>(P.p[r], n, i, x); });
#pragma unroll
            for (int j = 0; j < N; ++j) {
                const uint64_t e = i + j;
                float g0[1], g1[1] = {0.f};                       // no piece: the slot is zeroed
                if (covers(L, end, t, e))
                    sgd_from_sum<GDT, 1>(L.at<const void>(0, t), mom, e, s, 1,
                                         [&](int, float (&x)[1]) { x[0] = sum[j]; }, g0, g1);
                g[j] = g1[0];
            }
        }
        st<GDT, N>(out, i, g);
    });
}

// ---------------------------------------------------------------------------------------
// host side: the table is edt_table.h's range layout

// The launch's view of the uploaded table. T == 0 (a range that is all padding): no table.
FragTable frag_table(const void* workspace, int T) {
    const uint64_t* d = static_cast<const uint64_t*>(workspace);
    return {d, d + T, d + 2 * (uint64_t)T, (uint64_t)T};
}

int check_range(uint64_t lo, uint64_t n) {
    if (lo % 512) return fail(EDT_ERR_ARG, "range start %llu is not a multiple of 512", (unsigned long long)lo);
    if (n > ~0ull - lo) return fail(EDT_ERR_ARG, "range too large");
    return EDT_OK;
}

}  // namespace

extern "C" {

uint64_t edt_delta_partial_q_frag_workspace_bytes(int T, int K_local) {
    if (T < 0 || K_local < 1) return 0;
    return range_table_words(T, 1 + K_local) * sizeof(uint64_t);
}

uint64_t edt_sgd_sum_q_frag_to_workspace_bytes(int T) {
    if (T < 0) return 0;
    return range_table_words(T, 1) * sizeof(uint64_t);
}

int edt_delta_partial_q_frag(const void* const* theta_t, int gdt, const void* const* theta_k, int wdt, int K_local,
                             int K_total, const uint64_t* start, const uint64_t* numel, int T, uint64_t lo, uint64_t n,
                             uint64_t region_elems, int fmt, float* residual, void* packed, void* workspace,
                             uint64_t workspace_bytes, void* stream) {
    g_err[0] = 0;
    if (!valid_pair(gdt, wdt)) return fail(EDT_ERR_ARG, "unsupported dtype pair (gdt/wdt)");
    if (int rc = check_fmt(fmt)) return rc;
    if (K_local < 1 || K_local > EDT_MAX_WORKERS)
        return fail(EDT_ERR_ARG, "worker count %d out of range [1, %d]", K_local, EDT_MAX_WORKERS);
    if (K_total < 1) return fail(EDT_ERR_ARG, "total worker count %d < 1", K_total);
    if (T < 0) return fail(EDT_ERR_ARG, "piece count %d < 0", T);
    if (int rc = check_regions(n, region_elems)) return rc;
    if (int rc = check_range(lo, n)) return rc;
    if (n == 0) return EDT_OK;
    if (T > 0 && (!theta_t || !theta_k || !start || !numel)) return fail(EDT_ERR_ARG, "null piece table");
    if (!packed) return fail(EDT_ERR_ARG, "packed is null");
    if (!aligned16(packed) || !aligned16(residual))
        return fail(EDT_ERR_ARG, "the quantized partial needs 16-byte aligned compact buffers (packed, residual)");
    if (int rc = check_workspace(workspace, workspace_bytes, edt_delta_partial_q_frag_workspace_bytes(T, K_local)))
        return rc;
    const uint64_t bg = gdt == EDT_BF16 ? 2 : 4, bw = wdt == EDT_BF16 ? 2 : 4;
    const Column cols[] = {{theta_t, 1, "theta_t", bg}, {theta_k, K_local, "theta_k", bw}};
    thread_local std::vector<uint64_t> h;
    if (!fill_range_table(h, start, numel, T, lo, n, cols, 2, last_error())) return EDT_ERR_ARG;
    hipStream_t st = (hipStream_t)stream;
    if (int rc = upload_table(h, workspace, st, "piece")) return rc;
    const FragTable L = frag_table(workspace, T);
    QFragPartial a;
    a.residual = residual;
    a.packed = static_cast<uint8_t*>(packed);
    a.n = n;
    a.tiles_per_region = region_elems / 512;
    a.region_bytes = edt_q_region_bytes(region_elems, fmt);
    a.payload_bytes = region_elems / 8 * fmt_bits(fmt);
    a.K = K_local;
    a.kdiv = (float)K_total;
    a.kinv = 1.0f / (float)K_total;
    const ListLaunch ll = list_launch((uint64_t)T, grid_for(n, true), (uint64_t)T);
    return with_pair(gdt, wdt, [&](auto G, auto W) {
        return with_fmt(fmt, [&](auto F) {
            return with_kc_div<KC_QUANT>(K_local, !is_pow2(K_total), [&](auto KC, auto DIV) {
                return with_bool(residual != nullptr, [&](auto EF) {
                    return with_bool(ll.lds, [&](auto LDS) {
                        delta_partial_q_frag_kernel<decltype(G)::value, decltype(W)::value, decltype(KC)::value,
                                                    decltype(DIV)::value, decltype(F)::value, decltype(EF)::value,
                                                    decltype(LDS)::value><<<ll.grid, kBlock, ll.shm, st>>>(L, a);
                        return check_launch("delta_partial_q_frag_kernel");
                    });
                });
            });
        });
    });
}

int edt_sgd_sum_q_frag_to(const void* const* theta_t, int gdt, const uint64_t* start, const uint64_t* numel, int T,
                          uint64_t lo, uint64_t n, const void* const* regions, int nacc, int fmt, void* momentum,
                          int has_momentum, void* out, double lr, double momentum_coef, int nesterov, void* workspace,
                          uint64_t workspace_bytes, void* stream) {
    g_err[0] = 0;
    if (int rc = check_master_dtype(gdt)) return rc;
    if (int rc = check_fmt(fmt)) return rc;
    if (int rc = check_partial_count(nacc)) return rc;
    if (T < 0) return fail(EDT_ERR_ARG, "piece count %d < 0", T);
    if (n % 512) return fail(EDT_ERR_ARG, "n = %llu is not a multiple of 512 (one region)", (unsigned long long)n);
    if (int rc = check_range(lo, n)) return rc;
    if (n == 0) return EDT_OK;
    if (T > 0 && (!theta_t || !start || !numel)) return fail(EDT_ERR_ARG, "null piece table");
    if (!regions) return fail(EDT_ERR_ARG, "regions is null");
    if (!out) return fail(EDT_ERR_ARG, "out is null");
    SgdScalars s;
    if (int rc = shard_sgd(s, gdt, lr, momentum_coef, has_momentum, nesterov, momentum)) return rc;
    QRegions P;
    memset(&P, 0, sizeof(P));
    bool al = aligned16(out) && (!s.use_momentum || aligned16(momentum));
    if (int rc = fill_table(P.p, regions, nacc, "regions", al)) return rc;
    if (!al)
        return fail(EDT_ERR_ARG, "the quantized sum needs 16-byte aligned compact buffers (regions, momentum, out)");
    if (int rc = check_workspace(workspace, workspace_bytes, edt_sgd_sum_q_frag_to_workspace_bytes(T))) return rc;
    const Column cols[] = {{theta_t, 1, "theta_t", gdt == EDT_BF16 ? 2u : 4u}};
    thread_local std::vector<uint64_t> h;
    if (!fill_range_table(h, start, numel, T, lo, n, cols, 1, last_error())) return EDT_ERR_ARG;
    hipStream_t st = (hipStream_t)stream;
    if (int rc = upload_table(h, workspace, st, "piece")) return rc;
    const FragTable L = frag_table(workspace, T);
    const ListLaunch ll = list_launch((uint64_t)T, grid_for(n, true), (uint64_t)T);
    void* mom = s.use_momentum ? momentum : nullptr;
    return with_dtype(gdt, [&](auto G) {
        return with_fmt(fmt, [&](auto F) {
            return with_bool(ll.lds, [&](auto LDS) {
                sgd_sum_q_frag_to_kernel<decltype(G)::value, decltype(F)::value, decltype(LDS)::value>
                    <<<ll.grid, kBlock, ll.shm, st>>>(L, P, nacc, mom, out, n, s);
                return check_launch("sgd_sum_q_frag_to_kernel");
            });
        });
    });
}

}  // extern "C"
