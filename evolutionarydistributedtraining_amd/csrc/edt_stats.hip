// edt_stats.hip — the pseudo-gradient statistics of the DiLoCo outer step (edt_delta_stats): one
// read-only pass over theta and the K worker arenas that forms, per chunk of the arena, the fp64
// sums of the very deltas and mean the fused step (edt_outer.hip) would apply to these operands,
// and counts what is not finite — so a caller can screen workers and clip before theta is touched.
// edt_delta_stats_list is the same pass over T separate tensors (a device table of their pointers,
// chunk starts relative to their tensor): one kernel body, two operand accessors.
// The per-element arithmetic is edt_step.h's (delta_of, mean_add: add_delta's two halves), the
// sums' order edt_chunksum.h's (the canonical chunk-sum order).
#include "edt_chunksum.h"
#include "edt_mx.h"
#include "edt_step.h"

namespace {

// Workers per group: a lane holds the group's deltas of its 8 elements (64 floats) while their
// sums are formed; with K <= kStatsGroup (one group) they are still there when the mean is known,
// which is what the d_k . m sums need.
constexpr int kStatsGroup = 8;
constexpr int kStatsUpc = kTileSlots / kWavesPerBlock;        // units (workgroups) per chunk: 32
constexpr int kStatsMaxWidth = 3 * EDT_MAX_WORKERS + 2;

// Row of 3 K + 2 doubles: S_mm | S_kk[K] | S_km[K] | nonfinite_mean | nonfinite[K] (the counts are
// small integers, exact in fp64 through every sum of the tree).
__host__ __device__ constexpr int stats_width(int K) { return 3 * K + 2; }

struct StatsWorkers {
    const void* p[EDT_MAX_WORKERS];
};

struct StatsArgs {
    const void* theta;
    const uint64_t* chunks;
    double* rows;
    uint64_t units;      // nchunks * kStatsUpc
    uint64_t u0;         // first unit of this launch
    int K;
    float kdiv;
    float kinv;
    StatsWorkers w;
    static constexpr bool kList = false;
    __device__ __forceinline__ const StatsArgs& operands(uint64_t) const { return *this; }
    __device__ __forceinline__ const void* th() const { return theta; }
    __device__ __forceinline__ const void* wp(int k) const { return w.p[k]; }
};

// The tensor-list form's arguments (edt_delta_stats_list): the operands are T separate tensors
// named by a device table, and a chunk's start is relative to its tensor chunks[3 c + 2].
struct StatsListArgs;
// The operand accessor: where chunk c's operands lie (th, wp(k)). The arena form's are the launch's
// own pointers (StatsArgs is its own accessor), the list form's those of the chunk's tensor t, read
// from the device table (uniform across the workgroup).
struct TensorOperands {
    const StatsListArgs& a;
    uint64_t t;
    __device__ __forceinline__ const void* th() const;
    __device__ __forceinline__ const void* wp(int k) const;
};

struct StatsListArgs {
    const void* const* theta;   // T
    const void* const* w;       // K * T, worker-major
    const uint64_t* vec;        // T: nonzero when the tensor's K + 1 pointers are all 16-byte aligned
    const uint64_t* chunks;
    double* rows;
    uint64_t units;
    uint64_t u0;
    uint64_t T;
    int K;
    float kdiv;
    float kinv;
    static constexpr bool kList = true;
    __device__ __forceinline__ TensorOperands operands(uint64_t c) const { return {*this, chunks[3 * c + 2]}; }
};
__device__ __forceinline__ const void* TensorOperands::th() const { return a.theta[t]; }
__device__ __forceinline__ const void* TensorOperands::wp(int k) const { return a.w[(uint64_t)k * a.T + t]; }


template <int DT, bool VEC, bool NT>
__device__ __forceinline__ void ld8(const void* p, uint64_t i, float (&x)[kVec]) {
    if constexpr (VEC) {
        ld<DT, kVec, NT>(p, i, x);
    } else {                                          // an operand off a 16-byte boundary
#pragma unroll
        for (int j = 0; j < kVec; ++j) {
            float y[1];
            ld<DT, 1>(p, i + j, y);
            x[j] = y[0];
        }
    }
}

// Masks x in place: what is not finite becomes 0 (it adds nothing to a sum) and is counted.
template <int N>
__device__ __forceinline__ void mask_count(float (&x)[N], double& count) {
#pragma unroll
    for (int j = 0; j < N; ++j) {
        const bool bad = (__float_as_uint(x[j]) & 0x7fffffffu) >= 0x7f800000u;
        if (bad) {
            x[j] = 0.f;
            count += 1.0;
        }
    }
}

template <int N>
__device__ __forceinline__ void dot_chain(const float (&x)[N], const float (&y)[N], double& s) {
#pragma unroll
    for (int j = 0; j < N; ++j) s = __builtin_fma((double)x[j], (double)y[j], s);
}

// One workgroup per unit of four tiles of a chunk, one tile per wave (for_tile's lane mapping; tile
// 0's lanes also take the head / tail elements, after their vector). A lane without a vector or an
// edge element computes on zeros: every delta is then +0, finite, and adds nothing. The four tile
// sums are combined through LDS as the tree does, (t0 + t1) + (t2 + t3): a level-2 row per unit.
// KM: K <= kStatsGroup, the S_km columns are formed; else they are written as 0.
// Args = StatsArgs: the arena form, indices are the arena's, VEC the launch's alignment.
// Args = StatsListArgs: the chunk row names its tensor and indices are inside it (its aligned body
// starts at its element 0, so it has a tail only); a launch takes the tensors whose alignment is
// its VEC and leaves the others' units to the other launch (the whole workgroup: uniform).
template <int GDT, int WDT, int DIV, int KC, bool KM, bool VEC, class Args>
__global__ __launch_bounds__(kBlock) void delta_stats_kernel(Args a) {
    __shared__ double part[kWavesPerBlock][kStatsMaxWidth];
    const uint64_t u = a.u0 + blockIdx.x;
    if (u >= a.units) return;                         // the whole workgroup
    const auto& o = a.operands(u / kStatsUpc);       // a itself (no copy), or the chunk's tensor
    if constexpr (Args::kList)
        if ((a.vec[o.t] != 0) != VEC) return;
    constexpr bool NT = nt_worker_loads<WDT, 4>();
    constexpr int G = kStatsGroup;
    const int K = KC > 0 ? KC : a.K;
    const int wave = threadIdx.x >> 6;
    const uint64_t c = u / kStatsUpc;
    const int tile = (int)(u % kStatsUpc) * kWavesPerBlock + wave;
    const uint64_t start = a.chunks[3 * c], len = a.chunks[3 * c + 1];
    const uint64_t A = (start + kVec - 1) / kVec * kVec, B = (start + len) / kVec * kVec;
    const uint64_t i = A + (uint64_t)tile * kTileElems + (uint64_t)(threadIdx.x & 63) * kVec;
    const bool has_vec = A < B && i < B;
    bool has_edge = false;
    uint64_t e = 0;
    if (tile == 0)
        tile0_edge(start, len, [&](uint64_t x) {
            has_edge = true;
            e = x;
        });

    float g[kVec] = {}, ge[1] = {}, acc[kVec] = {}, acce[1] = {};
    if (has_vec) ld8<GDT, VEC, false>(o.th(), i, g);
    if (has_edge) ld<GDT, 1>(o.th(), e, ge);
    double smm = 0.0, cm = 0.0, skm[G] = {};
    double* row = &part[wave][0];

    for (int k0 = 0; k0 < K; k0 += G) {               // KM: one group
        float d[G][kVec], de[G][1];
        double skk[G] = {}, ck[G] = {};
#pragma unroll
        for (int q = 0; q < G; ++q) {                 // the group's loads, issued together
#pragma unroll
            for (int j = 0; j < kVec; ++j) d[q][j] = 0.f;
            de[q][0] = 0.f;
            if (KC > 0 ? q < KC : k0 + q < K) {
                if (has_vec) ld8<WDT, VEC, NT>(o.wp(k0 + q), i, d[q]);
                if (has_edge) ld<WDT, 1>(o.wp(k0 + q), e, de[q]);
            }
        }
#pragma unroll
        for (int q = 0; q < G; ++q) {
            if (KC > 0 ? q < KC : k0 + q < K) {
                delta_of<GDT>(d[q], g);
                mean_add<GDT, DIV, true>(a, d[q], acc);
                delta_of<GDT>(de[q], ge);
                mean_add<GDT, DIV, true>(a, de[q], acce);
                mask_count(d[q], ck[q]);
                mask_count(de[q], ck[q]);
                dot_chain(d[q], d[q], skk[q]);        // the lane's vector, then its edge element
                dot_chain(de[q], de[q], skk[q]);
            }
        }
        if constexpr (KM) {
            mask_count(acc, cm);
            mask_count(acce, cm);
            dot_chain(acc, acc, smm);
            dot_chain(acce, acce, smm);
#pragma unroll
            for (int q = 0; q < G; ++q) {
                dot_chain(d[q], acc, skm[q]);
                dot_chain(de[q], acce, skm[q]);
            }
            double v[3 * G + 2], r[Red<3 * G + 2>::N2];
            v[0] = smm;
            v[2 * G + 1] = cm;
#pragma unroll
            for (int q = 0; q < G; ++q) {
                v[1 + q] = skk[q];
                v[1 + G + q] = skm[q];
                v[2 * G + 2 + q] = ck[q];
            }
            tile_reduce<3 * G + 2>(v, r);
            red_store<3 * G + 2>(r, [&](int idx, double x) {
                if (idx == 0) row[0] = x;
                else if (idx <= G) { if (idx - 1 < K) row[idx] = x; }
                else if (idx <= 2 * G) { if (idx - 1 - G < K) row[K + idx - G] = x; }
                else if (idx == 2 * G + 1) row[2 * K + 1] = x;
                else if (idx - 2 * G - 2 < K) row[2 * K + idx - 2 * G] = x;
            });
        } else {
            double v[2 * G], r[Red<2 * G>::N2];
#pragma unroll
            for (int q = 0; q < G; ++q) {
                v[q] = skk[q];
                v[G + q] = ck[q];
            }
            tile_reduce<2 * G>(v, r);
            red_store<2 * G>(r, [&](int idx, double x) {
                const int k = k0 + (idx < G ? idx : idx - G);
                if (k < K) row[(idx < G ? 1 : 2 * K + 2) + k] = x;
            });
        }
    }
    if constexpr (!KM) {
        mask_count(acc, cm);
        mask_count(acce, cm);
        dot_chain(acc, acc, smm);
        dot_chain(acce, acce, smm);
        const double v[2] = {smm, cm};
        double r[Red<2>::N2];
        tile_reduce<2>(v, r);
        red_store<2>(r, [&](int idx, double x) { row[idx == 0 ? 0 : 2 * K + 1] = x; });
    }
    __syncthreads();
    const int W = stats_width(K);
    double* out = a.rows + unit_slot(u, a.units) * (uint64_t)W;
    for (int q = threadIdx.x; q < W; q += kBlock) {
        double x = 0.0;
        if (KM || q <= K || q > 2 * K) x = (part[0][q] + part[1][q]) + (part[2][q] + part[3][q]);
        out[q] = x;
    }
}

template <int GDT, int WDT, int DIV, int KC, bool KM, bool VEC, class A>
int launch_stats(A a, hipStream_t s) {
    const uint64_t units = a.units;
    for (uint64_t u0 = 0; u0 < units; u0 += kUnitGridCap) {
        a.u0 = u0;
        delta_stats_kernel<GDT, WDT, DIV, KC, KM, VEC, A><<<unit_grid(units - u0), kBlock, 0, s>>>(a);
        if (int rc = check_launch("delta_stats_kernel")) return rc;
    }
    return EDT_OK;
}

// The K = 8 and DIV / KM dispatch of both forms, then the tree over the rows. LIST: the alignment
// is per tensor — the vector launch, then (vec false: some tensor is unaligned) the scalar one.
template <class A, bool LIST>
int dispatch_stats(const A& a, Bool<LIST>, int gdt, int wdt, bool vec, int64_t nchunks, double* out, hipStream_t s) {
    const int K = a.K;
    const bool km = K <= kStatsGroup;
    int rc = with_pair(gdt, wdt, [&](auto G, auto Wd) {
        constexpr int GD = decltype(G)::value, WD = decltype(Wd)::value;
        auto go = [&](auto V) {
            constexpr bool VEC = decltype(V)::value;
            if (K == 8) return launch_stats<GD, WD, 0, 8, true, VEC>(a, s);
            return with_bool(!is_pow2(K), [&](auto D) {
                constexpr int DIV = decltype(D)::value ? 1 : 0;
                return with_bool(km, [&](auto M) { return launch_stats<GD, WD, DIV, 0, decltype(M)::value, VEC>(a, s); });
            });
        };
        if constexpr (LIST) {                         // vec: some tensor is off a 16-byte boundary
            if (int r = go(Bool<true>{})) return r;
            return vec ? EDT_OK : go(Bool<false>{});
        } else {
            return with_bool(vec, go);
        }
    });
    if (rc) return rc;
    return launch_tree_reduce(a.rows, stats_width(K), kStatsUpc, kStatsUpc, 1, nchunks, out, s);
}

// ---- the mean pseudo-gradient of a sharded step, from the per-rank partials its owner holds ------
// edt_partial_sum_stats: m = round_g(rank_sum of the shard's partials), exactly the value
// sgd_from_sum negates into the gradient (edt_step.h: the same rank_sum, the same rnd), so a shard
// owner can measure the step before theta is touched. delta_stats_kernel's unit, tile and lane
// mapping and its (t0 + t1) + (t2 + t3) level-2 row, with a row of two: S_mm | nonfinite_mean.
constexpr int kPartialStatsWidth = 2;

struct StatsPartials {
    const float* p[EDT_MAX_WORKERS];
};

struct PartialStatsArgs {
    const uint64_t* chunks;
    double* rows;
    uint64_t units;
    uint64_t u0;
    int np;
    StatsPartials P;
};

// NPC > 0: the partial count at compile time (rank_sum's loop unrolls and its loads issue
// together); 0: the generic loop over a.np.
template <int GDT, int NPC, bool VEC>
__global__ __launch_bounds__(kBlock) void partial_sum_stats_kernel(PartialStatsArgs a) {
    __shared__ double part[kWavesPerBlock][kPartialStatsWidth];
    const uint64_t u = a.u0 + blockIdx.x;
    if (u >= a.units) return;                         // the whole workgroup
    const int np = NPC > 0 ? NPC : a.np;
    const int wave = threadIdx.x >> 6;
    const uint64_t c = u / kStatsUpc;
    const int tile = (int)(u % kStatsUpc) * kWavesPerBlock + wave;
    const uint64_t start = a.chunks[3 * c], len = a.chunks[3 * c + 1];
    const uint64_t A = (start + kVec - 1) / kVec * kVec, B = (start + len) / kVec * kVec;
    const uint64_t i = A + (uint64_t)tile * kTileElems + (uint64_t)(threadIdx.x & 63) * kVec;
    const bool has_vec = A < B && i < B;
    bool has_edge = false;
    uint64_t e = 0;
    if (tile == 0)
        tile0_edge(start, len, [&](uint64_t x) {
            has_edge = true;
            e = x;
        });

    // a lane without a vector or an edge element sums zeros: m = +0, finite, adds nothing
    float m[kVec], me[1];
    rank_sum(np, m, [&](int r, float (&x)[kVec]) {
#pragma unroll
        for (int j = 0; j < kVec; ++j) x[j] = 0.f;
        if (has_vec) ld8<EDT_F32, VEC, false>(a.P.p[r], i, x);
    });
    rank_sum(np, me, [&](int r, float (&x)[1]) {
        x[0] = 0.f;
        if (has_edge) ld<EDT_F32, 1>(a.P.p[r], e, x);
    });
    rnd<GDT>(m);
    rnd<GDT>(me);
    double smm = 0.0, cm = 0.0;
    mask_count(m, cm);
    mask_count(me, cm);
    dot_chain(m, m, smm);                             // the lane's vector, then its edge element
    dot_chain(me, me, smm);
    const double v[2] = {smm, cm};
    double r[Red<2>::N2];
    tile_reduce<2>(v, r);
    red_store<2>(r, [&](int idx, double x) { part[wave][idx] = x; });
    __syncthreads();
    double* out = a.rows + unit_slot(u, a.units) * (uint64_t)kPartialStatsWidth;
    if (threadIdx.x < kPartialStatsWidth) {
        const int q = threadIdx.x;
        out[q] = (part[0][q] + part[1][q]) + (part[2][q] + part[3][q]);
    }
}

template <int GDT, int NPC, bool VEC>
int launch_partial_stats(PartialStatsArgs a, hipStream_t s) {
    const uint64_t units = a.units;
    for (uint64_t u0 = 0; u0 < units; u0 += kUnitGridCap) {
        a.u0 = u0;
        partial_sum_stats_kernel<GDT, NPC, VEC><<<unit_grid(units - u0), kBlock, 0, s>>>(a);
        if (int rc = check_launch("partial_sum_stats_kernel")) return rc;
    }
    return EDT_OK;
}

// ---- the same figures of the quantized schedule (reduce_q): the partials are packed regions ------
// edt_partial_sum_stats_q: m = round_g(rank_sum of D(q_r)), ld_q per rank (edt_mx.h) where
// partial_sum_stats_kernel loads fp32 — exactly the value edt_sgd_apply_sum_q / edt_sgd_delta_sum_q
// negate into the gradient, quantization error and residuals included. Read only. The same unit,
// tile, lane and tree mapping; a lane's 8 elements are the quantized kernels' (four lanes share a
// scale byte). n % 512 == 0 and the chunk bounds are multiples of 8, so a chunk is its aligned
// body: no head, no tail, no scalar path. A scale-255 block is 32 NaN elements: left out, counted.
struct PartialStatsQArgs {
    const uint64_t* chunks;
    double* rows;
    uint64_t units;
    uint64_t u0;
    uint64_t n;          // elements of one region
    int np;
    QRegions P;
};

template <int GDT, int FMT, int NPC>
__global__ __launch_bounds__(kBlock) void partial_sum_stats_q_kernel(PartialStatsQArgs a) {
    __shared__ double part[kWavesPerBlock][kPartialStatsWidth];
    const uint64_t u = a.u0 + blockIdx.x;
    if (u >= a.units) return;                         // the whole workgroup
    const int np = NPC > 0 ? NPC : a.np;
    const int wave = threadIdx.x >> 6;
    const uint64_t c = u / kStatsUpc;
    const int tile = (int)(u % kStatsUpc) * kWavesPerBlock + wave;
    const uint64_t start = a.chunks[3 * c], len = a.chunks[3 * c + 1];
    const uint64_t A = (start + kVec - 1) / kVec * kVec, B = (start + len) / kVec * kVec;
    const uint64_t i = A + (uint64_t)tile * kTileElems + (uint64_t)(threadIdx.x & 63) * kVec;
    // inside the chunk, and never past the region whatever the table says
    const bool has_vec = i < B && i + kVec <= a.n;

    // a lane without a vector sums zeros: m = +0, finite, adds nothing
    float m[kVec];
    rank_sum(np, m, [&](int r, float (&x)[kVec]) {
#pragma unroll
        for (int j = 0; j < kVec; ++j) x[j] = 0.f;
        if (has_vec) ld_q<FMT>(a.P.p[r], a.n, i, x);
    });
    rnd<GDT>(m);
    double smm = 0.0, cm = 0.0;
    mask_count(m, cm);
    dot_chain(m, m, smm);
    const double v[2] = {smm, cm};
    double r[Red<2>::N2];
    tile_reduce<2>(v, r);
    red_store<2>(r, [&](int idx, double x) { part[wave][idx] = x; });
    __syncthreads();
    double* out = a.rows + unit_slot(u, a.units) * (uint64_t)kPartialStatsWidth;
    if (threadIdx.x < kPartialStatsWidth) {
        const int q = threadIdx.x;
        out[q] = (part[0][q] + part[1][q]) + (part[2][q] + part[3][q]);
    }
}

template <int GDT, int FMT, int NPC>
int launch_partial_stats_q(PartialStatsQArgs a, hipStream_t s) {
    const uint64_t units = a.units;
    for (uint64_t u0 = 0; u0 < units; u0 += kUnitGridCap) {
        a.u0 = u0;
        partial_sum_stats_q_kernel<GDT, FMT, NPC><<<unit_grid(units - u0), kBlock, 0, s>>>(a);
        if (int rc = check_launch("partial_sum_stats_q_kernel")) return rc;
    }
    return EDT_OK;
}

}  // namespace

extern "C" {

uint64_t edt_partial_sum_stats_doubles(int64_t nchunks) {
    if (nchunks < 0) return 0;
    // the chunk rows, then one level-2 row per unit of four tiles
    return (uint64_t)nchunks * (uint64_t)kPartialStatsWidth * (1ull + kStatsUpc);
}

int edt_partial_sum_stats(const float* const* acc_f32, int nacc, int gdt, uint64_t n, const uint64_t* chunk_desc,
                          int64_t nchunks, double* out, void* stream) {
    g_err[0] = 0;
    int rc = check_master_dtype(gdt);
    if (!rc) rc = check_partial_count(nacc);
    if (rc) return rc;
    if (nchunks < 0) return fail(EDT_ERR_ARG, "negative chunk count");
    if (!acc_f32) return fail(EDT_ERR_ARG, "acc_f32 is null");
    if (n == 0 || nchunks == 0) return EDT_OK;
    if (!chunk_desc || !out) return fail(EDT_ERR_ARG, "null chunk table or output");
    if (reinterpret_cast<uintptr_t>(out) & 7u) return fail(EDT_ERR_ARG, "out must be 8-byte aligned");
    PartialStatsArgs a;
    memset(&a, 0, sizeof(a));
    bool vec = true;
    if ((rc = fill_table(a.P.p, acc_f32, nacc, "acc_f32", vec))) return rc;
    a.chunks = chunk_desc;
    a.rows = out + (uint64_t)nchunks * kPartialStatsWidth;
    a.units = (uint64_t)nchunks * kStatsUpc;
    a.np = nacc;
    hipStream_t s = (hipStream_t)stream;
    rc = with_dtype(gdt, [&](auto G) {
        constexpr int GD = decltype(G)::value;
        return with_bool(vec, [&](auto V) {
            constexpr bool VEC = decltype(V)::value;
            switch (nacc) {
                case 1: return launch_partial_stats<GD, 1, VEC>(a, s);
                case 2: return launch_partial_stats<GD, 2, VEC>(a, s);
                case 4: return launch_partial_stats<GD, 4, VEC>(a, s);
                case 8: return launch_partial_stats<GD, 8, VEC>(a, s);
                default: return launch_partial_stats<GD, 0, VEC>(a, s);
            }
        });
    });
    if (rc) return rc;
    return launch_tree_reduce(a.rows, kPartialStatsWidth, kStatsUpc, kStatsUpc, 1, nchunks, out, s);
}

// rows and workspace: edt_partial_sum_stats_doubles(nchunks), the same two columns and row levels
int edt_partial_sum_stats_q(const void* const* regions, int nacc, int fmt, int gdt, uint64_t n,
                            const uint64_t* chunk_desc, int64_t nchunks, double* out, void* stream) {
    g_err[0] = 0;
    int rc = check_master_dtype(gdt);
    if (!rc && fmt != EDT_MXFP8 && fmt != EDT_MXFP4)
        rc = fail(EDT_ERR_ARG, "unknown wire format %d (EDT_MXFP8 or EDT_MXFP4)", fmt);
    if (!rc) rc = check_partial_count(nacc);
    if (rc) return rc;
    if (n % 512) return fail(EDT_ERR_ARG, "n = %llu is not a multiple of 512 (one region)", (unsigned long long)n);
    if (nchunks < 0) return fail(EDT_ERR_ARG, "negative chunk count");
    if (!regions) return fail(EDT_ERR_ARG, "regions is null");
    if (n == 0 || nchunks == 0) return EDT_OK;
    if (!chunk_desc || !out) return fail(EDT_ERR_ARG, "null chunk table or output");
    if (reinterpret_cast<uintptr_t>(out) & 7u) return fail(EDT_ERR_ARG, "out must be 8-byte aligned");
    PartialStatsQArgs a;
    memset(&a, 0, sizeof(a));
    bool al = true;
    if ((rc = fill_table(a.P.p, regions, nacc, "regions", al))) return rc;
    if (!al) return fail(EDT_ERR_ARG, "the packed regions must be 16-byte aligned");
    a.chunks = chunk_desc;
    a.rows = out + (uint64_t)nchunks * kPartialStatsWidth;
    a.units = (uint64_t)nchunks * kStatsUpc;
    a.n = n;
    a.np = nacc;
    hipStream_t s = (hipStream_t)stream;
    rc = with_dtype(gdt, [&](auto G) {
        constexpr int GD = decltype(G)::value;
        return with_fmt(fmt, [&](auto F) {
            constexpr int FM = decltype(F)::value;
            switch (nacc) {
                case 1: return launch_partial_stats_q<GD, FM, 1>(a, s);
                case 2: return launch_partial_stats_q<GD, FM, 2>(a, s);
                case 4: return launch_partial_stats_q<GD, FM, 4>(a, s);
                case 8: return launch_partial_stats_q<GD, FM, 8>(a, s);
                default: return launch_partial_stats_q<GD, FM, 0>(a, s);
            }
        });
    });
    if (rc) return rc;
    return launch_tree_reduce(a.rows, kPartialStatsWidth, kStatsUpc, kStatsUpc, 1, nchunks, out, s);
}

uint64_t edt_delta_stats_doubles(int K, int64_t nchunks) {
    if (K < 1 || K > EDT_MAX_WORKERS || nchunks < 0) return 0;
    // the chunk rows, then one level-2 row per unit of four tiles
    return (uint64_t)nchunks * (uint64_t)stats_width(K) * (1ull + kStatsUpc);
}

int edt_delta_stats(const void* theta_g, int gdt, const void* const* theta_k, int wdt, int K, uint64_t n,
                    const uint64_t* chunk_desc, int64_t nchunks, double* out, void* stream) {
    g_err[0] = 0;
    if (!valid_pair(gdt, wdt)) return fail(EDT_ERR_ARG, "unsupported dtype pair (gdt/wdt)");
    if (K < 1 || K > EDT_MAX_WORKERS)
        return fail(EDT_ERR_ARG, "worker count %d out of range [1, %d]", K, EDT_MAX_WORKERS);
    if (nchunks < 0) return fail(EDT_ERR_ARG, "negative chunk count");
    if (!theta_k) return fail(EDT_ERR_ARG, "theta_k is null");
    if (n == 0 || nchunks == 0) return EDT_OK;
    if (!theta_g) return fail(EDT_ERR_ARG, "theta_g is null");
    if (!chunk_desc || !out) return fail(EDT_ERR_ARG, "null chunk table or output");
    if (reinterpret_cast<uintptr_t>(out) & 7u) return fail(EDT_ERR_ARG, "out must be 8-byte aligned");
    StatsArgs a;
    memset(&a, 0, sizeof(a));
    bool vec = aligned16(theta_g);
    for (int k = 0; k < K; ++k) {
        if (!theta_k[k]) return fail(EDT_ERR_ARG, "theta_k[%d] is null", k);
        a.w.p[k] = theta_k[k];
        vec = vec && aligned16(theta_k[k]);
    }
    a.theta = theta_g;
    a.chunks = chunk_desc;
    a.rows = out + (uint64_t)nchunks * stats_width(K);
    a.units = (uint64_t)nchunks * kStatsUpc;
    a.K = K;
    a.kdiv = (float)K;
    a.kinv = 1.0f / (float)K;
    return dispatch_stats(a, Bool<false>{}, gdt, wdt, vec, nchunks, out, (hipStream_t)stream);
}

uint64_t edt_delta_stats_list_workspace_bytes(int T, int K) {
    if (T < 0 || K < 1 || K > EDT_MAX_WORKERS) return 0;
    // table: theta[T] | w[K*T] | vec[T]   (all 8-byte words)
    return ((uint64_t)K + 2) * (uint64_t)T * sizeof(uint64_t);
}

int edt_delta_stats_list(const void* const* theta_t, int gdt, const void* const* theta_k, int wdt, int K,
                         const uint64_t* numel, int T, const uint64_t* chunk_desc, int64_t nchunks, double* out,
                         void* workspace, uint64_t workspace_bytes, void* stream) {
    g_err[0] = 0;
    if (!valid_pair(gdt, wdt)) return fail(EDT_ERR_ARG, "unsupported dtype pair (gdt/wdt)");
    if (K < 1 || K > EDT_MAX_WORKERS)
        return fail(EDT_ERR_ARG, "worker count %d out of range [1, %d]", K, EDT_MAX_WORKERS);
    if (T < 0) return fail(EDT_ERR_ARG, "tensor count %d < 0", T);
    if (nchunks < 0) return fail(EDT_ERR_ARG, "negative chunk count");
    if (T == 0 || nchunks == 0) return EDT_OK;
    if (!theta_t || !theta_k || !numel) return fail(EDT_ERR_ARG, "null tensor table");
    if (!chunk_desc || !out) return fail(EDT_ERR_ARG, "null chunk table or output");
    if (reinterpret_cast<uintptr_t>(out) & 7u) return fail(EDT_ERR_ARG, "out must be 8-byte aligned");
    const uint64_t need = edt_delta_stats_list_workspace_bytes(T, K);
    if (!workspace || workspace_bytes < need)
        return fail(EDT_ERR_ARG, "workspace of %llu bytes needed", (unsigned long long)need);
    if (reinterpret_cast<uintptr_t>(workspace) & 7u) return fail(EDT_ERR_ARG, "workspace must be 8-byte aligned");
    thread_local std::vector<uint64_t> h;
    h.assign(need / sizeof(uint64_t), 0);
    uint64_t* pth = h.data();
    uint64_t* pw = pth + T;
    uint64_t* pvec = pw + (uint64_t)K * T;
    bool all_vec = true;
    for (int t = 0; t < T; ++t) {
        bool vec = true;
        if (numel[t]) {                               // an empty tensor has no chunks: never read
            if (!theta_t[t]) return fail(EDT_ERR_ARG, "theta_t[%d] is null", t);
            vec = aligned16(theta_t[t]);
            for (int k = 0; k < K; ++k) {
                const void* p = theta_k[(uint64_t)k * T + t];
                if (!p) return fail(EDT_ERR_ARG, "theta_k[%d][%d] is null", k, t);
                vec = vec && aligned16(p);
            }
        }
        pth[t] = reinterpret_cast<uintptr_t>(theta_t[t]);
        for (int k = 0; k < K; ++k) pw[(uint64_t)k * T + t] = reinterpret_cast<uintptr_t>(theta_k[(uint64_t)k * T + t]);
        pvec[t] = vec ? 1 : 0;
        all_vec = all_vec && vec;
    }
    hipStream_t s = (hipStream_t)stream;
    // pageable source, overwritten by this thread's next call: stream-ordered, as edt_outer_step_list's
    hipError_t e = hipMemcpyAsync(workspace, h.data(), need, hipMemcpyHostToDevice, s);
    if (e != hipSuccess) return fail(EDT_ERR_LAUNCH, "tensor table upload failed: %s", hipGetErrorString(e));
    const uint64_t* d = static_cast<const uint64_t*>(workspace);
    StatsListArgs a;
    memset(&a, 0, sizeof(a));
    a.theta = reinterpret_cast<const void* const*>(d);
    a.w = reinterpret_cast<const void* const*>(d + T);
    a.vec = d + (uint64_t)T + (uint64_t)K * T;
    a.T = (uint64_t)T;
    a.chunks = chunk_desc;
    a.rows = out + (uint64_t)nchunks * stats_width(K);
    a.units = (uint64_t)nchunks * kStatsUpc;
    a.K = K;
    a.kdiv = (float)K;
    a.kinv = 1.0f / (float)K;
    return dispatch_stats(a, Bool<true>{}, gdt, wdt, all_vec, nchunks, out, s);
}

}  // extern "C"
