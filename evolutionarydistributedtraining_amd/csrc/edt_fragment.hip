// edt_fragment.hip — the sharded fragment step's three kernels over piece lists (Streaming DiLoCo
// across ranks, sharded_fragments.py), with their C ABI entries (include/edt_sync.h):
//   edt_delta_partial_list       phase 1: the local workers' fp32 partial of a bucket's pieces
//   edt_sgd_sum_list_to          phase 2: rank-ordered sum + SGD on the owned shard's pieces, the new
//                                theta stored elsewhere (theta itself is only read)
//   edt_theta_scatter_mix_list   phase 3: the gathered theta into theta's pieces and, merged, into
//                                every local worker's
// A piece is one contiguous stretch of every operand: a view into an arena at the piece's arena
// offset, or into a compact fragment-space buffer. The list machinery is outer_list_kernel's
// (edt_outer.hip), restated here so that unit's instantiations cannot move: a device table uploaded
// by a stream-ordered copy, chunks of kListChunk elements that never cross a piece, the chunk
// prefix sums searched in LDS, the vector body for pieces whose pointers are all 16-byte aligned
// and the scalar body otherwise (a piece may start at any element of a run: unaligned pieces are the
// normal case), tile and lane mapping following the element's index inside its piece. Every result
// is element-wise, so it does not depend on how the pieces are cut. The arithmetic is edt_step.h's
// (add_delta, sgd_from_sum) and edt_common.h's (lerp_held).
#include "edt_step.h"

#include <algorithm>

namespace {

// outer_list_kernel's chunking (edt_outer.hip): the same rule, the same constants
#ifndef EDT_LIST_ITERS
#define EDT_LIST_ITERS 2
#endif
constexpr uint64_t kListChunk = (uint64_t)kBlock * kVec * EDT_LIST_ITERS;   // 4096 elements
constexpr uint64_t kVecFlag = 1ull << 63;                                  // numel[t] bit: vector body ok
constexpr uint64_t kListLdsMaxPieces = 8191;                               // (T + 1) x 8 B <= 64 KiB of LDS

// The device table of a launch, 8-byte words: prefix[T + 1] | numel[T] | the kernel's pointer columns,
// each rows x T words, row-major (cols + (first row of the column + r) * T + t).
struct PieceList {
    const uint64_t* prefix;     // T + 1 chunk prefix sums
    const uint64_t* numel;      // T, kVecFlag | numel
    const uint64_t* cols;       // the pointer columns
    uint64_t T;
    uint64_t chunks;            // prefix[T]
    template <class P = void>
    __device__ __forceinline__ P* at(uint64_t row, uint64_t t) const {
        return reinterpret_cast<P*>(static_cast<uintptr_t>(cols[row * T + t]));
    }
};

// The piece of chunk b (the last t with prefix[t] <= b; uniform across the workgroup) and the
// chunk's element range [c0, c1) inside it.
__device__ __forceinline__ uint64_t piece_of(const PieceList& L, const uint64_t* prefix, uint64_t b, uint64_t& nf,
                                             uint64_t& c0, uint64_t& c1) {
    uint64_t lo = 0, hi = L.T;
    while (hi - lo > 1) {
        const uint64_t mid = (lo + hi) >> 1;
        if (prefix[mid] <= b) lo = mid;
        else hi = mid;
    }
    nf = L.numel[lo];
    const uint64_t n = nf & ~kVecFlag;
    c0 = (b - prefix[lo]) * kListChunk;
    c1 = c0 + kListChunk < n ? c0 + kListChunk : n;
    return lo;
}

// f(Int<N>, Int<H2>, i) over the chunk [c0, c1) of a piece, as outer_list_chunk walks it. SPLIT and
// an aligned piece: tiles of kBlock x 8 elements in split-halves order, then a scalar tail; an aligned
// piece otherwise: 8 consecutive elements per thread and a scalar tail of < 8; an unaligned piece:
// one element per thread. c0 is a multiple of kListChunk, so every vector access is 16-byte aligned.
template <bool SPLIT, class F>
__device__ __forceinline__ void for_chunk(uint64_t nf, uint64_t c0, uint64_t c1, F&& f) {
    if (nf & kVecFlag) {
        if constexpr (SPLIT) {
            constexpr uint64_t tile = (uint64_t)kBlock * kVec;
            const uint64_t vend = c0 + (c1 - c0) / tile * tile;
            for (uint64_t i = c0 + 4ull * threadIdx.x; i < vend; i += tile) f(Int<kVec>{}, Int<4 * kBlock>{}, i);
            for (uint64_t i = vend + threadIdx.x; i < c1; i += kBlock) f(Int<1>{}, Int<4>{}, i);
        } else {
            const uint64_t vend = c0 + (c1 - c0) / kVec * kVec;
            for (uint64_t i = c0 + (uint64_t)threadIdx.x * kVec; i < vend; i += (uint64_t)kBlock * kVec)
                f(Int<kVec>{}, Int<4>{}, i);
            const uint64_t i = vend + threadIdx.x;
            if (i < c1) f(Int<1>{}, Int<4>{}, i);
        }
    } else {
        for (uint64_t i = c0 + threadIdx.x; i < c1; i += kBlock) f(Int<1>{}, Int<4>{}, i);
    }
}

// The grid-stride loop over chunks with the prefix sums staged in LDS (LDS = false, very long
// lists: the global table is searched): body(t, nf, c0, c1) per chunk.
template <bool LDS, class F>
__device__ __forceinline__ void for_pieces(const PieceList& L, F&& body) {
    extern __shared__ uint64_t s_prefix[];
    const uint64_t* prefix = L.prefix;
    if constexpr (LDS) {
        for (uint64_t i = threadIdx.x; i <= L.T; i += kBlock) s_prefix[i] = L.prefix[i];
        __syncthreads();
        prefix = s_prefix;
    }
    for (uint64_t b = blockIdx.x; b < L.chunks; b += gridDim.x) {
        uint64_t nf, c0, c1;
        const uint64_t t = piece_of(L, prefix, b, nf, c0, c1);
        body(t, nf, c0, c1);
    }
}

// ---------------------------------------------------------------------------------------
// phase 1: acc_t[i] = sum_k round_g(round_g(f32(w_k,t[i]) - f32(theta_t[i])) / K_total), the sum in
// fp32, local workers in order — add_delta<..., ROUND_ACC = false>, the body edt_delta_partial runs.
// columns: theta (row 0) | acc (row 1) | w (rows 2 .. 2 + K)

struct PartialPiece {               // what add_delta reads of a launch's argument block
    const uint64_t* w;              // the worker rows of the table
    uint64_t T, t;
    float kdiv, kinv;
    __device__ __forceinline__ const void* wp(int k) const {
        return reinterpret_cast<const void*>(static_cast<uintptr_t>(w[(uint64_t)k * T + t]));
    }
};

template <int GDT, int WDT, int KC, int DIV, bool LDS>
__global__ __launch_bounds__(kBlock, EDT_MIN_WAVES) void delta_partial_list_kernel(PieceList L, int Krt, float kdiv,
                                                                                    float kinv) {
    for_pieces<LDS>(L, [&](uint64_t t, uint64_t nf, uint64_t c0, uint64_t c1) {
        const PartialPiece a = {L.cols + 2 * L.T, L.T, t, kdiv, kinv};
        const void* theta = L.at<const void>(0, t);
        float* out = L.at<float>(1, t);
        const int K = KC > 0 ? KC : Krt;
        for_chunk<split_halves<GDT, WDT>()>(nf, c0, c1, [&](auto VN, auto VH, uint64_t i) {
            constexpr int N = decltype(VN)::value, H2 = decltype(VH)::value;
            float g[N], acc[N];
            ld<GDT, N, (EDT_NT_RMW != 0), H2>(theta, i, g);
#pragma unroll
            for (int j = 0; j < N; ++j) acc[j] = 0.f;
            if constexpr (KC > 0) {
#pragma unroll
                for (int k = 0; k < KC; ++k) add_delta<GDT, WDT, DIV, N, H2, false>(a, k, g, acc, i);
            } else {
#pragma unroll 4
                for (int k = 0; k < K; ++k) add_delta<GDT, WDT, DIV, N, H2, false>(a, k, g, acc, i);
            }
            st<EDT_F32, N, (EDT_NT_STORES != 0), H2>(out, i, acc);
        });
    });
}

// ---------------------------------------------------------------------------------------
// phase 2: a = round_g(((p_0 + p_1) + ...) + p_{N-1}) in rank order, grad = -a, torch's SGD update
// with the piece's momentum (in place) — sgd_from_sum, unchanged. theta is only read; the new theta
// goes to out_t (theta's dtype), as edt_sgd_delta_sum_q leaves theta alone.
// columns: theta (row 0) | mom (row 1) | out (row 2) | parts (rows 3 .. 3 + np)

template <int GDT, bool LDS>
__global__ __launch_bounds__(kBlock) void sgd_sum_list_to_kernel(PieceList L, int np, SgdScalars s) {
    for_pieces<LDS>(L, [&](uint64_t t, uint64_t nf, uint64_t c0, uint64_t c1) {
        const void* theta = L.at<const void>(0, t);
        void* mom = s.use_momentum ? L.at<void>(1, t) : nullptr;
        void* out = L.at<void>(2, t);
        for_chunk<false>(nf, c0, c1, [&](auto VN, auto, uint64_t i) {
            constexpr int M = decltype(VN)::value;
            float g0[M], g[M];
            sgd_from_sum<GDT, M>(theta, mom, i, s, np,
                                 [&](int r, float (&x)[M]) { ld<EDT_F32, M>(L.at<const float>(3 + (uint64_t)r, t), i, x); },
                                 g0, g);
            st<GDT, M>(out, i, g);
        });
    });
}

// ---------------------------------------------------------------------------------------
// phase 3: theta_t[i] <- src_t[i] (theta's dtype, the bits as they are), and with v = round_w(src)
// every destination live_j,t[i] <- round_w(round_w(c0 * live) + round_w(c1 * v)) — the merge of
// outer_elems' MX branch (edt_outer.hip), kept as a second text so that the fused list kernels'
// code does not move; tests/test_gpu_sharded_fragment.py holds the two together bit for bit. COPY
// (mix == 1): v is stored, the destination is not read.
// columns: src (row 0) | theta (row 1) | live (rows 2 .. 2 + nmix)

// x, whose values are exact in DT, stored bit for bit (st<BF16> would convert, which may quiet a
// signalling NaN: an all-gather of theta moves bits, so this does too)
template <int DT, int N, bool NT, int H2>
__device__ __forceinline__ void st_exact(void* __restrict__ p, uint64_t i, const float (&x)[N]) {
    if constexpr (DT == EDT_F32) {
        st<EDT_F32, N, NT, H2>(p, i, x);
    } else {
        static_assert(N == 1 || (N == 8 && H2 == 4), "bf16 pieces take the 8-consecutive or the scalar body");
        uint16_t* q = static_cast<uint16_t*>(p) + i;
        auto pk = [](float lo, float hi) { return (__float_as_uint(lo) >> 16) | (__float_as_uint(hi) & 0xffff0000u); };
        if constexpr (N == 8) {
            u32x4 w;
            w.x = pk(x[0], x[1]); w.y = pk(x[2], x[3]);
            w.z = pk(x[4], x[5]); w.w = pk(x[6], x[7]);
            vstore<u32x4, NT>(reinterpret_cast<u32x4*>(q), w);
        } else {
            q[0] = uint16_t(__float_as_uint(x[0]) >> 16);
        }
    }
}

template <int GDT, int WDT, bool COPY, bool LDS>
__global__ __launch_bounds__(kBlock) void theta_scatter_mix_list_kernel(PieceList L, int nmix, float c0, float c1) {
    for_pieces<LDS>(L, [&](uint64_t t, uint64_t nf, uint64_t b0, uint64_t b1) {
        const void* src = L.at<const void>(0, t);
        void* theta = L.at<void>(1, t);
        for_chunk<split_halves<GDT, WDT>()>(nf, b0, b1, [&](auto VN, auto VH, uint64_t i) {
            constexpr int N = decltype(VN)::value, H2 = decltype(VH)::value;
            constexpr bool NT = EDT_NT_STORES != 0;
            float g[N];
            ld<GDT, N, false, H2>(src, i, g);
            st_exact<GDT, N, NT, H2>(theta, i, g);
            rnd<WDT>(g);
            if constexpr (COPY) {
#pragma unroll 4
                for (int j = 0; j < nmix; ++j) st<WDT, N, NT, H2>(L.at<void>(2 + (uint64_t)j, t), i, g);
            } else {
                float y[N];                                          // round_w(c1 * v): one for every destination
#pragma unroll
                for (int j = 0; j < N; ++j) y[j] = c1 * g[j];
                rnd<WDT>(y);
#pragma unroll 4
                for (int j = 0; j < nmix; ++j) {
                    void* d = L.at<void>(2 + (uint64_t)j, t);
                    float x[N];
                    ld<WDT, N, false, H2>(d, i, x);
                    lerp_held<WDT, N>(x, y, c0);
                    st<WDT, N, NT, H2>(d, i, x);
                }
            }
        });
    });
}

// ---------------------------------------------------------------------------------------
// host side: the table and the checks the three entries share

// One pointer column of an entry: rows x T host pointers, row-major; p == nullptr: an operand the
// call does not use (zeros in the table, not read by the kernel).
struct Column {
    const void* const* p;
    int rows;
    const char* name;
};

uint64_t table_words(int T, int rows) { return (uint64_t)(2 + rows) * (uint64_t)T + 1; }

// Fills h (table_words(T, all rows) words) from numel and the columns: every pointer of a non-empty
// piece checked non-null ("<name>[t] is null", "<name>[r][t] is null" for a column of several rows),
// the piece's vector flag from their 16-byte alignment, the chunk prefix sums. chunks = prefix[T].
int fill_pieces(std::vector<uint64_t>& h, const uint64_t* numel, int T, const Column* cols, int ncols, uint64_t& chunks) {
    int rows = 0;
    for (int c = 0; c < ncols; ++c) rows += cols[c].rows;
    h.assign(table_words(T, rows), 0);
    uint64_t* prefix = h.data();
    uint64_t* nflag = prefix + T + 1;
    uint64_t* out = nflag + T;
    for (int t = 0; t < T; ++t) {
        const uint64_t n = numel[t];
        if (n >= kVecFlag) return fail(EDT_ERR_ARG, "piece %d too large", t);
        bool vec = true;
        uint64_t row = 0;
        for (int c = 0; c < ncols; ++c) {
            for (int r = 0; r < cols[c].rows; ++r, ++row) {
                if (!cols[c].p) continue;
                const void* p = cols[c].p[(uint64_t)r * T + t];
                if (n && !p)
                    return cols[c].rows > 1 ? fail(EDT_ERR_ARG, "%s[%d][%d] is null", cols[c].name, r, t)
                                            : fail(EDT_ERR_ARG, "%s[%d] is null", cols[c].name, t);
                vec = vec && aligned16(p);
                out[row * T + t] = reinterpret_cast<uintptr_t>(p);
            }
        }
        prefix[t + 1] = prefix[t] + (n + kListChunk - 1) / kListChunk;
        nflag[t] = n | (vec ? kVecFlag : 0);
    }
    chunks = prefix[T];
    if (chunks > 0x7fffffffull) return fail(EDT_ERR_ARG, "too many elements for one launch");
    return EDT_OK;
}

int check_workspace(const void* workspace, uint64_t workspace_bytes, uint64_t need) {
    if (!workspace || workspace_bytes < need)
        return fail(EDT_ERR_ARG, "workspace of %llu bytes needed", (unsigned long long)need);
    if (reinterpret_cast<uintptr_t>(workspace) & 7u) return fail(EDT_ERR_ARG, "workspace must be 8-byte aligned");
    return EDT_OK;
}

// The table uploaded by a stream-ordered copy (pageable source, overwritten by this thread's next
// call: the runtime has read it when hipMemcpyAsync returns, as edt_outer_step_list relies on) and
// the launch's view of it.
int upload_table(PieceList& L, const std::vector<uint64_t>& h, void* workspace, int T, uint64_t chunks, hipStream_t st) {
    hipError_t e = hipMemcpyAsync(workspace, h.data(), h.size() * sizeof(uint64_t), hipMemcpyHostToDevice, st);
    if (e != hipSuccess) return fail(EDT_ERR_LAUNCH, "piece table upload failed: %s", hipGetErrorString(e));
    const uint64_t* d = static_cast<const uint64_t*>(workspace);
    L.prefix = d;
    L.numel = d + T + 1;
    L.cols = d + 2 * (uint64_t)T + 1;
    L.T = (uint64_t)T;
    L.chunks = chunks;
    return EDT_OK;
}

struct ListLaunch {
    unsigned grid;
    size_t shm;
    bool lds;
};
ListLaunch list_launch(int T, uint64_t chunks) {
    const bool lds = (uint64_t)T <= kListLdsMaxPieces;
    return {chunks > kMaxBlocks ? (unsigned)kMaxBlocks : (unsigned)chunks, lds ? (size_t)(T + 1) * sizeof(uint64_t) : 0,
            lds};
}

int check_piece_count(int T) {
    if (T < 0) return fail(EDT_ERR_ARG, "piece count %d < 0", T);
    return EDT_OK;
}

// Phase 3's aliasing rule over its non-empty pieces: theta's pieces and the destinations are
// written, src is read; a written range may overlap nothing. One sort of the byte ranges, then a
// sweep (as edt_outer_step_list_mix's check).
int check_scatter_ranges(const void* const* src_t, void* const* theta_t, int gdt, void* const* live, int wdt, int nmix,
                         const uint64_t* numel, int T) {
    struct Range {
        uintptr_t lo, hi;
        int written;
    };
    const uint64_t bg = gdt == EDT_BF16 ? 2 : 4, bw = wdt == EDT_BF16 ? 2 : 4;
    thread_local std::vector<Range> rs;
    rs.clear();
    auto push = [&](const void* p, uint64_t bytes, int written) {
        const uintptr_t lo = reinterpret_cast<uintptr_t>(p);
        rs.push_back({lo, lo + bytes, written});
    };
    for (int t = 0; t < T; ++t) {
        const uint64_t n = numel[t];
        if (!n) continue;
        push(src_t[t], n * bg, 0);
        push(theta_t[t], n * bg, 1);
        for (int j = 0; j < nmix; ++j) push(live[(uint64_t)j * T + t], n * bw, 1);
    }
    std::sort(rs.begin(), rs.end(), [](const Range& a, const Range& b) { return a.lo < b.lo; });
    uintptr_t end_any = 0, end_written = 0;      // furthest end so far: of any range, of a written one
    for (const Range& r : rs) {
        if (r.lo < (r.written ? end_any : end_written))
            return fail(EDT_ERR_ARG, "a piece of theta or a merge destination overlaps another operand");
        if (r.hi > end_any) end_any = r.hi;
        if (r.written && r.hi > end_written) end_written = r.hi;
    }
    return EDT_OK;
}

}  // namespace

extern "C" {

uint64_t edt_delta_partial_list_workspace_bytes(int T, int K_local) {
    if (T < 0 || K_local < 1) return 0;
    return table_words(T, 2 + K_local) * sizeof(uint64_t);
}

uint64_t edt_sgd_sum_list_to_workspace_bytes(int T, int nacc) {
    if (T < 0 || nacc < 1) return 0;
    return table_words(T, 3 + nacc) * sizeof(uint64_t);
}

uint64_t edt_theta_scatter_mix_list_workspace_bytes(int T, int nmix) {
    if (T < 0 || nmix < 0) return 0;
    return table_words(T, 2 + nmix) * sizeof(uint64_t);
}

int edt_delta_partial_list(const void* const* theta_t, int gdt, const void* const* theta_k, int wdt, int K_local,
                           int K_total, float* const* acc_t, const uint64_t* numel, int T, void* workspace,
                           uint64_t workspace_bytes, void* stream) {
    g_err[0] = 0;
    if (!valid_pair(gdt, wdt)) return fail(EDT_ERR_ARG, "unsupported dtype pair (gdt/wdt)");
    if (K_local < 1 || K_local > EDT_MAX_WORKERS)
        return fail(EDT_ERR_ARG, "worker count %d out of range [1, %d]", K_local, EDT_MAX_WORKERS);
    if (K_total < 1) return fail(EDT_ERR_ARG, "total worker count %d < 1", K_total);
    if (int rc = check_piece_count(T)) return rc;
    if (T == 0) return EDT_OK;
    if (!theta_t || !theta_k || !acc_t || !numel) return fail(EDT_ERR_ARG, "null piece table");
    if (int rc = check_workspace(workspace, workspace_bytes, edt_delta_partial_list_workspace_bytes(T, K_local))) return rc;
    const Column cols[] = {{theta_t, 1, "theta_t"},
                           {reinterpret_cast<const void* const*>(acc_t), 1, "acc_t"},
                           {theta_k, K_local, "theta_k"}};
    thread_local std::vector<uint64_t> h;
    uint64_t chunks;
    if (int rc = fill_pieces(h, numel, T, cols, 3, chunks)) return rc;
    if (chunks == 0) return EDT_OK;
    PieceList L;
    hipStream_t st = (hipStream_t)stream;
    if (int rc = upload_table(L, h, workspace, T, chunks, st)) return rc;
    const ListLaunch ll = list_launch(T, chunks);
    const float kdiv = (float)K_total, kinv = 1.0f / (float)K_total;
    return with_pair(gdt, wdt, [&](auto G, auto W) {
        return with_kc_div<KC_FUSED>(K_local, !is_pow2(K_total), [&](auto KC, auto DIV) {
            return with_bool(ll.lds, [&](auto LDS) {
                delta_partial_list_kernel<decltype(G)::value, decltype(W)::value, decltype(KC)::value, decltype(DIV)::value,
                                          decltype(LDS)::value><<<ll.grid, kBlock, ll.shm, st>>>(L, K_local, kdiv, kinv);
                return check_launch("delta_partial_list_kernel");
            });
        });
    });
}

int edt_sgd_sum_list_to(const void* const* theta_t, int gdt, const float* const* parts, int nacc,
                        void* const* momentum_t, int has_momentum, void* const* out_t, const uint64_t* numel, int T,
                        double lr, double momentum_coef, int nesterov, void* workspace, uint64_t workspace_bytes,
                        void* stream) {
    g_err[0] = 0;
    int rc = check_master_dtype(gdt);
    if (!rc) rc = check_partial_count(nacc);
    if (!rc) rc = check_piece_count(T);
    if (rc) return rc;
    if (T == 0) return EDT_OK;
    if (!theta_t || !parts || !out_t || !numel) return fail(EDT_ERR_ARG, "null piece table");
    const SgdScalars s = make_sgd(gdt, lr, momentum_coef, has_momentum, nesterov);
    if (s.use_momentum && !momentum_t) return fail(EDT_ERR_ARG, "momentum table is null");
    if ((rc = check_workspace(workspace, workspace_bytes, edt_sgd_sum_list_to_workspace_bytes(T, nacc)))) return rc;
    const Column cols[] = {{theta_t, 1, "theta_t"},
                           {s.use_momentum ? reinterpret_cast<const void* const*>(momentum_t) : nullptr, 1, "momentum_t"},
                           {reinterpret_cast<const void* const*>(out_t), 1, "out_t"},
                           {reinterpret_cast<const void* const*>(parts), nacc, "parts"}};
    thread_local std::vector<uint64_t> h;
    uint64_t chunks;
    if ((rc = fill_pieces(h, numel, T, cols, 4, chunks))) return rc;
    if (chunks == 0) return EDT_OK;
    PieceList L;
    hipStream_t st = (hipStream_t)stream;
    if ((rc = upload_table(L, h, workspace, T, chunks, st))) return rc;
    const ListLaunch ll = list_launch(T, chunks);
    return with_dtype(gdt, [&](auto G) {
        return with_bool(ll.lds, [&](auto LDS) {
            sgd_sum_list_to_kernel<decltype(G)::value, decltype(LDS)::value><<<ll.grid, kBlock, ll.shm, st>>>(L, nacc, s);
            return check_launch("sgd_sum_list_to_kernel");
        });
    });
}

int edt_theta_scatter_mix_list(void* const* theta_t, int gdt, const void* const* src_t, void* const* live, int wdt,
                               int nmix, double mix, const uint64_t* numel, int T, void* workspace,
                               uint64_t workspace_bytes, void* stream) {
    g_err[0] = 0;
    if (!valid_pair(gdt, wdt)) return fail(EDT_ERR_ARG, "unsupported dtype pair (gdt/wdt)");
    if (!(mix > 0.0 && mix <= 1.0))                 // NaN fails both comparisons
        return fail(EDT_ERR_ARG, "mix %g outside (0, 1]", mix);
    if (nmix < 0 || nmix > EDT_MAX_WORKERS)
        return fail(EDT_ERR_ARG, "merge destination count %d out of range [0, %d]", nmix, EDT_MAX_WORKERS);
    if (int rc = check_piece_count(T)) return rc;
    if (T == 0) return EDT_OK;
    if (!theta_t || !src_t || !numel) return fail(EDT_ERR_ARG, "null piece table");
    if (nmix && !live) return fail(EDT_ERR_ARG, "live is null");
    if (int rc = check_workspace(workspace, workspace_bytes, edt_theta_scatter_mix_list_workspace_bytes(T, nmix))) return rc;
    const Column cols[] = {{src_t, 1, "src_t"},
                           {reinterpret_cast<const void* const*>(theta_t), 1, "theta_t"},
                           {reinterpret_cast<const void* const*>(live), nmix, "live"}};
    thread_local std::vector<uint64_t> h;
    uint64_t chunks;
    if (int rc = fill_pieces(h, numel, T, cols, 3, chunks)) return rc;
    if (chunks == 0) return EDT_OK;
    if (int rc = check_scatter_ranges(src_t, theta_t, gdt, live, wdt, nmix, numel, T)) return rc;
    PieceList L;
    hipStream_t st = (hipStream_t)stream;
    if (int rc = upload_table(L, h, workspace, T, chunks, st)) return rc;
    const ListLaunch ll = list_launch(T, chunks);
    const float c0 = (float)(1.0 - mix), c1 = (float)mix;      // as edt_lerp forms them
    return with_pair(gdt, wdt, [&](auto G, auto W) {
        return with_bool(mix == 1.0, [&](auto COPY) {
            return with_bool(ll.lds, [&](auto LDS) {
                theta_scatter_mix_list_kernel<decltype(G)::value, decltype(W)::value, decltype(COPY)::value,
                                              decltype(LDS)::value><<<ll.grid, kBlock, ll.shm, st>>>(L, nmix, c0, c1);
                return check_launch("theta_scatter_mix_list_kernel");
            });
        });
    });
}

}  // extern "C"
