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
// staged in LDS (up to kListLdsMaxPieces, edt_fragment.hip's limit; longer tables are searched in
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

namespace {

constexpr uint64_t kVecFlag = 1ull << 63;                // start[t] bit: the piece's pointers allow vector loads
constexpr uint64_t kListLdsMaxPieces = 8191;             // edt_fragment.hip's: at most 64 KiB of LDS

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
// host side: the table and the checks the two entries share

// One pointer column of an entry: rows x T host pointers, row-major, to elements of elem_bytes.
struct FragColumn {
    const void* const* p;
    int rows;
    uint64_t elem_bytes;
    const char* name;
};

uint64_t frag_table_words(int T, int rows) { return (uint64_t)(2 + rows) * (uint64_t)T; }

// Fills h from the pieces of the range [lo, lo + n): sorted, disjoint and inside it (empty pieces
// anywhere in it), every pointer of a non-empty piece non-null; the pointers rebased by the piece's
// start, the piece's vector flag from the rebased pointers' 16-byte alignment.
int fill_frag_table(std::vector<uint64_t>& h, const uint64_t* start, const uint64_t* numel, int T, uint64_t lo,
                    uint64_t n, const FragColumn* cols, int ncols) {
    int rows = 0;
    for (int c = 0; c < ncols; ++c) rows += cols[c].rows;
    h.assign(frag_table_words(T, rows), 0);
    uint64_t* end = h.data();
    uint64_t* sflag = end + T;
    uint64_t* out = sflag + T;
    uint64_t prev = lo;                                  // where the piece before ends
    for (int t = 0; t < T; ++t) {
        const uint64_t s = start[t], m = numel[t];
        if (s < prev)
            return fail(EDT_ERR_ARG, "piece %d starts before the range or before the end of piece %d: sorted, disjoint pieces",
                        t, t - 1);
        if (s - lo > n || m > n - (s - lo)) return fail(EDT_ERR_ARG, "piece %d leaves the range", t);
        bool vec = true;
        uint64_t row = 0;
        for (int c = 0; c < ncols; ++c) {
            for (int r = 0; r < cols[c].rows; ++r, ++row) {
                const void* p = cols[c].p[(uint64_t)r * T + t];
                if (!m) continue;                        // an empty piece's pointers are not read
                if (!p)
                    return cols[c].rows > 1 ? fail(EDT_ERR_ARG, "%s[%d][%d] is null", cols[c].name, r, t)
                                            : fail(EDT_ERR_ARG, "%s[%d] is null", cols[c].name, t);
                const uint64_t base = reinterpret_cast<uintptr_t>(p) - (s - lo) * cols[c].elem_bytes;
                vec = vec && (base & 15u) == 0;
                out[row * T + t] = base;
            }
        }
        prev = s + m;
        end[t] = prev - lo;
        sflag[t] = (s - lo) | (vec && m ? kVecFlag : 0);
    }
    return EDT_OK;
}

int check_range(uint64_t lo, uint64_t n) {
    if (lo % 512) return fail(EDT_ERR_ARG, "range start %llu is not a multiple of 512", (unsigned long long)lo);
    if (n > ~0ull - lo) return fail(EDT_ERR_ARG, "range too large");
    return EDT_OK;
}

int check_frag_workspace(const void* workspace, uint64_t workspace_bytes, uint64_t need) {
    if (!need) return EDT_OK;
    if (!workspace || workspace_bytes < need)
        return fail(EDT_ERR_ARG, "workspace of %llu bytes needed", (unsigned long long)need);
    if (reinterpret_cast<uintptr_t>(workspace) & 7u) return fail(EDT_ERR_ARG, "workspace must be 8-byte aligned");
    return EDT_OK;
}

// The table uploaded by a stream-ordered copy (pageable source, overwritten by this thread's next
// call: the runtime has read it when hipMemcpyAsync returns, as the _list entries rely on) and the
// launch's view of it. T == 0 (a range that is all padding): no table, nothing copied.
int upload_frag_table(FragTable& L, const std::vector<uint64_t>& h, void* workspace, int T, hipStream_t st) {
    if (T > 0) {
        hipError_t e = hipMemcpyAsync(workspace, h.data(), h.size() * sizeof(uint64_t), hipMemcpyHostToDevice, st);
        if (e != hipSuccess) return fail(EDT_ERR_LAUNCH, "piece table upload failed: %s", hipGetErrorString(e));
    }
    const uint64_t* d = static_cast<const uint64_t*>(workspace);
    L.end = d;
    L.start = d + T;
    L.cols = d + 2 * (uint64_t)T;
    L.T = (uint64_t)T;
    return EDT_OK;
}

bool ends_in_lds(int T) { return (uint64_t)T <= kListLdsMaxPieces; }

}  // namespace

extern "C" {

uint64_t edt_delta_partial_q_frag_workspace_bytes(int T, int K_local) {
    if (T < 0 || K_local < 1) return 0;
    return frag_table_words(T, 1 + K_local) * sizeof(uint64_t);
}

uint64_t edt_sgd_sum_q_frag_to_workspace_bytes(int T) {
    if (T < 0) return 0;
    return frag_table_words(T, 1) * sizeof(uint64_t);
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
    if (int rc = check_frag_workspace(workspace, workspace_bytes, edt_delta_partial_q_frag_workspace_bytes(T, K_local)))
        return rc;
    const uint64_t bg = gdt == EDT_BF16 ? 2 : 4, bw = wdt == EDT_BF16 ? 2 : 4;
    const FragColumn cols[] = {{theta_t, 1, bg, "theta_t"}, {theta_k, K_local, bw, "theta_k"}};
    thread_local std::vector<uint64_t> h;
    if (int rc = fill_frag_table(h, start, numel, T, lo, n, cols, 2)) return rc;
    FragTable L;
    hipStream_t st = (hipStream_t)stream;
    if (int rc = upload_frag_table(L, h, workspace, T, st)) return rc;
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
    const unsigned g = grid_for(n, true);
    const bool lds = ends_in_lds(T);
    const size_t shm = lds ? (size_t)T * sizeof(uint64_t) : 0;
    return with_pair(gdt, wdt, [&](auto G, auto W) {
        return with_fmt(fmt, [&](auto F) {
            return with_kc_div<KC_QUANT>(K_local, !is_pow2(K_total), [&](auto KC, auto DIV) {
                return with_bool(residual != nullptr, [&](auto EF) {
                    return with_bool(lds, [&](auto LDS) {
                        delta_partial_q_frag_kernel<decltype(G)::value, decltype(W)::value, decltype(KC)::value,
                                                    decltype(DIV)::value, decltype(F)::value, decltype(EF)::value,
                                                    decltype(LDS)::value><<<g, kBlock, shm, st>>>(L, a);
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
    if (int rc = check_frag_workspace(workspace, workspace_bytes, edt_sgd_sum_q_frag_to_workspace_bytes(T))) return rc;
    const FragColumn cols[] = {{theta_t, 1, gdt == EDT_BF16 ? 2u : 4u, "theta_t"}};
    thread_local std::vector<uint64_t> h;
    if (int rc = fill_frag_table(h, start, numel, T, lo, n, cols, 1)) return rc;
    FragTable L;
    hipStream_t st = (hipStream_t)stream;
    if (int rc = upload_frag_table(L, h, workspace, T, st)) return rc;
    const unsigned g = grid_for(n, true);
    const bool lds = ends_in_lds(T);
    const size_t shm = lds ? (size_t)T * sizeof(uint64_t) : 0;
    void* mom = s.use_momentum ? momentum : nullptr;
    return with_dtype(gdt, [&](auto G) {
        return with_fmt(fmt, [&](auto F) {
            return with_bool(lds, [&](auto LDS) {
                sgd_sum_q_frag_to_kernel<decltype(G)::value, decltype(F)::value, decltype(LDS)::value>
                    <<<g, kBlock, shm, st>>>(L, P, nacc, mom, out, n, s);
                return check_launch("sgd_sum_q_frag_to_kernel");
            });
        });
    });
}

}  // extern "C"
