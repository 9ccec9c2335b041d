// edt_taskmerge.hip — task-vector merges of K models relative to a common base in ONE pass over
// tensor lists (edt_task_merge_list, include/edt_sync.h): task_arithmetic, dare_linear, dare_ties.
//
// Per element the kernel forms the K task vectors delta_k = M_k - B one at a time, drops each with
// probability 1 - density (DARE: 16 Philox bits per (model, element)), rescales the kept ones, and
// carries FIVE running values — the weighted sum A, the sums P / N of its positive / negative terms and
// the weights WP / WN behind them — from which the sign consensus elects the sum that agrees with A's
// sign. The K deltas are never held: one pass serves any K <= EDT_MAX_WORKERS and register use does not
// grow with K. All arithmetic is fp32, each operation rounded on its own (the unit is built with
// -ffp-contract=off and without packed fp32 forms, build.py).
//
// Work split: edt_table.h's chunk-prefix table (4,096-element chunks that never cross a tensor, the
// prefix sums staged in dynamic LDS, a grid-stride loop over chunks as outer_list_kernel's). Per chunk
// one uniform binary search finds the tensor t; threads 0..K-1 then stage that tensor's K model
// pointers and coefficient words (c, w, drop16) in static LDS once, so the element loop reads them as
// LDS broadcasts. A lane owns 8 consecutive elements (one 16-byte load per bf16 operand, two per fp32
// one); the models' loads are issued in batches of kBatch<WDT> before any is used (32 VGPRs of loads in
// flight: 8 bf16 or 4 fp32 models), then consumed in k order. One Philox call per (lane, model) gives
// the 8 x 16 bits of the lane's elements. Tensors whose operands are not all 16-byte aligned, and each
// tensor's last < 8 elements, take the same body at N = 1 with the same bits (the bits are indexed by
// the element's position in the padded packing of the list's sizes, not by its address).
#include "edt_mx.h"
#include "edt_table.h"

namespace {

using namespace edt_table;

struct TaskArgs {
    const uint64_t* prefix;      // T + 1 chunk prefix sums
    const uint64_t* numel;       // T, kVecFlag | numel
    void* const* base;           // T
    const void* const* models;   // K * T, model-major
    void* const* out;            // T (the base column again when the call writes in place)
    const uint64_t* coef;        // K * T: c's bits | w's bits << 32
    const uint64_t* drop;        // K * T: drop16
    const uint64_t* group;       // T: base_t / 8, the tensor's first Philox group
    uint64_t T;
    uint64_t chunks;             // prefix[T]
    int K;
    int normalize;
    int nt_store;                // no tensor is written in place: the child is stored non-temporally
    float lambda;
    uint32_t key0, key1, step;
};

// what threads 0..K-1 stage per chunk: the chunk's tensor's model pointers and coefficients
struct TaskStage {
    const void* m[EDT_MAX_WORKERS];
    float c[EDT_MAX_WORKERS];
    float w[EDT_MAX_WORKERS];
    uint32_t drop[EDT_MAX_WORKERS];
};

// models whose loads are in flight together: 32 VGPRs of raw loads per lane either way
template <int WDT> constexpr int kBatch = WDT == EDT_BF16 ? 8 : 4;

// A lane's N elements of one operand as loaded, widened to fp32 only when consumed.
template <int DT, int N> struct Raw;
template <> struct Raw<EDT_BF16, 8> { u32x4 v; };
template <> struct Raw<EDT_F32, 8> { f32x4 a, b; };
template <> struct Raw<EDT_BF16, 1> { uint16_t v; };
template <> struct Raw<EDT_F32, 1> { float v; };

template <int DT, int N, bool NT>
__device__ __forceinline__ Raw<DT, N> ld_raw(const void* p, uint64_t i) {
    Raw<DT, N> r;
    if constexpr (DT == EDT_BF16 && N == 8) {
        r.v = vload<u32x4, NT>(reinterpret_cast<const u32x4*>(static_cast<const uint16_t*>(p) + i));
    } else if constexpr (DT == EDT_F32 && N == 8) {
        const float* q = static_cast<const float*>(p) + i;
        r.a = vload<f32x4, NT>(reinterpret_cast<const f32x4*>(q));
        r.b = vload<f32x4, NT>(reinterpret_cast<const f32x4*>(q + 4));
    } else if constexpr (DT == EDT_BF16) {
        r.v = static_cast<const uint16_t*>(p)[i];
    } else {
        r.v = static_cast<const float*>(p)[i];
    }
    return r;
}

template <int DT, int N>
__device__ __forceinline__ void widen(const Raw<DT, N>& r, float (&x)[N]) {
    if constexpr (DT == EDT_BF16 && N == 8) {
        x[0] = bf_lo(r.v.x); x[1] = bf_hi(r.v.x); x[2] = bf_lo(r.v.y); x[3] = bf_hi(r.v.y);
        x[4] = bf_lo(r.v.z); x[5] = bf_hi(r.v.z); x[6] = bf_lo(r.v.w); x[7] = bf_hi(r.v.w);
    } else if constexpr (DT == EDT_F32 && N == 8) {
        x[0] = r.a.x; x[1] = r.a.y; x[2] = r.a.z; x[3] = r.a.w;
        x[4] = r.b.x; x[5] = r.b.y; x[6] = r.b.z; x[7] = r.b.w;
    } else if constexpr (DT == EDT_BF16) {
        x[0] = __uint_as_float((uint32_t)r.v << 16);
    } else {
        x[0] = r.v;
    }
}

// The N elements at i (relative to the tensor; a multiple of 8 when N == 8) of one tensor. S holds the
// tensor's model pointers and coefficients, group0 its first Philox group, wa the sum of its weights.
template <int GDT, int WDT, int ODT, bool DARE, bool CONS, int N>
__device__ __forceinline__ void task_elems(const TaskArgs& L, const TaskStage& S, const void* base, void* out,
                                           uint64_t group0, float wa, uint64_t i) {
    constexpr int KB = kBatch<WDT>;
    constexpr bool NTL = nt_worker_loads<WDT, 4>();              // the once-read bf16 model streams
    float b[N], A[N];
    [[maybe_unused]] float P[N], M[N], WP[N], WN[N];
    ld<GDT, N>(base, i, b);
#pragma unroll
    for (int j = 0; j < N; ++j) A[j] = 0.f;
    if constexpr (CONS) {
#pragma unroll
        for (int j = 0; j < N; ++j) P[j] = M[j] = WP[j] = WN[j] = 0.f;
    }
    const uint64_t g = group0 + (i >> 3);
    const int K = L.K;
    for (int k0 = 0; k0 < K; k0 += KB) {
        Raw<WDT, N> raw[KB];
#pragma unroll
        for (int u = 0; u < KB; ++u)
            if (k0 + u < K) raw[u] = ld_raw<WDT, N, NTL>(S.m[k0 + u], i);
#pragma unroll
        for (int u = 0; u < KB; ++u) {
            if (k0 + u >= K) continue;
            const int k = k0 + u;
            float m[N];
            widen<WDT, N>(raw[u], m);
            const float c = S.c[k];
            [[maybe_unused]] const float w = S.w[k];
            [[maybe_unused]] uint32_t r[4];
            [[maybe_unused]] uint32_t drop = 0;
            if constexpr (DARE) {
                r[0] = (uint32_t)g; r[1] = (uint32_t)(g >> 32); r[2] = L.step; r[3] = (uint32_t)k;
                philox4x32(r, L.key0, L.key1);
                drop = S.drop[k];
            }
#pragma unroll
            for (int j = 0; j < N; ++j) {
                float tau = c * (m[j] - b[j]);
                if constexpr (DARE) {
                    uint32_t word;
                    if constexpr (N == 8) {
                        word = r[j >> 1];
                    } else {
                        const uint32_t e = (uint32_t)i & 7u;        // selects, not a dynamic register index
                        word = e < 2 ? r[0] : e < 4 ? r[1] : e < 6 ? r[2] : r[3];
                    }
                    const uint32_t odd = N == 8 ? (uint32_t)(j & 1) : (uint32_t)i & 1u;
                    const uint32_t r16 = odd ? word >> 16 : word & 0xffffu;
                    tau = r16 >= drop ? tau : 0.f;
                }
                A[j] = A[j] + tau;
                if constexpr (CONS) {
                    const bool pos = tau > 0.f, neg = tau < 0.f;     // adding +0 leaves a sum's bits alone
                    P[j] = P[j] + (pos ? tau : 0.f);
                    M[j] = M[j] + (neg ? tau : 0.f);
                    WP[j] = WP[j] + (pos ? w : 0.f);
                    WN[j] = WN[j] + (neg ? w : 0.f);
                }
            }
        }
    }
    float o[N];
#pragma unroll
    for (int j = 0; j < N; ++j) {
        float num = A[j], den = wa;
        if constexpr (CONS) {
            num = A[j] > 0.f ? P[j] : A[j] < 0.f ? M[j] : A[j];      // A NaN: num = A
            den = A[j] > 0.f ? WP[j] : A[j] < 0.f ? WN[j] : 1.f;
        }
        float q = num;
        if (L.normalize) {
            den = __builtin_fabsf(den) < 1e-8f ? 1.f : den;
            q = __fdiv_rn(num, den);
        }
        o[j] = b[j] + L.lambda * q;
    }
    if (L.nt_store) st<ODT, N, true>(out, i, o);
    else st<ODT, N, false>(out, i, o);
}

template <int GDT, int WDT, int ODT, bool DARE, bool CONS>
__device__ __forceinline__ void task_chunk(const TaskArgs& L, const uint64_t* prefix, TaskStage& S, uint64_t b) {
    uint64_t lo = 0, hi = L.T;                       // last t with prefix[t] <= b
    while (hi - lo > 1) {
        const uint64_t mid = (lo + hi) >> 1;
        if (prefix[mid] <= b) lo = mid;
        else hi = mid;
    }
    const uint64_t t = lo;
    __syncthreads();                                 // the chunk before has read the stage
    if ((int)threadIdx.x < L.K) {
        const uint64_t at = (uint64_t)threadIdx.x * L.T + t;
        const uint64_t cw = L.coef[at];
        S.m[threadIdx.x] = L.models[at];
        S.c[threadIdx.x] = __uint_as_float((uint32_t)cw);
        S.w[threadIdx.x] = __uint_as_float((uint32_t)(cw >> 32));
        if constexpr (DARE) S.drop[threadIdx.x] = (uint32_t)L.drop[at];
    }
    __syncthreads();
    float wa = 0.f;                                  // WA, in k order (the no-consensus divisor)
    if constexpr (!CONS)
        for (int k = 0; k < L.K; ++k) wa = wa + S.w[k];
    const uint64_t nf = L.numel[t];
    const uint64_t n = nf & ~kVecFlag;
    const uint64_t c0 = (b - prefix[t]) * kListChunk;
    const uint64_t c1 = c0 + kListChunk < n ? c0 + kListChunk : n;
    const void* base = L.base[t];
    void* out = L.out[t];
    const uint64_t g0 = L.group[t];
    if (nf & kVecFlag) {
        const uint64_t vend = c0 + (c1 - c0) / kVec * kVec;
        for (uint64_t i = c0 + (uint64_t)threadIdx.x * kVec; i < vend; i += (uint64_t)kBlock * kVec)
            task_elems<GDT, WDT, ODT, DARE, CONS, kVec>(L, S, base, out, g0, wa, i);
        const uint64_t i = vend + threadIdx.x;       // the tensor's last < 8 elements
        if (i < c1) task_elems<GDT, WDT, ODT, DARE, CONS, 1>(L, S, base, out, g0, wa, i);
    } else {
        for (uint64_t i = c0 + threadIdx.x; i < c1; i += kBlock)
            task_elems<GDT, WDT, ODT, DARE, CONS, 1>(L, S, base, out, g0, wa, i);
    }
}

// LDS = true: the chunk prefix sums staged in dynamic LDS ((T + 1) x 8 bytes) once per workgroup;
// LDS = false (more than kListLdsMaxPieces tensors): the search reads the global table.
template <int GDT, int WDT, int ODT, bool DARE, bool CONS, bool LDS>
__global__ __launch_bounds__(kBlock) void task_merge_kernel(TaskArgs L) {
    extern __shared__ uint64_t s_prefix[];
    __shared__ TaskStage S;
    const uint64_t* prefix = L.prefix;
    if constexpr (LDS) {
        for (uint64_t i = threadIdx.x; i <= L.T; i += kBlock) s_prefix[i] = L.prefix[i];
        __syncthreads();
        prefix = s_prefix;
    }
    for (uint64_t b = blockIdx.x; b < L.chunks; b += gridDim.x) task_chunk<GDT, WDT, ODT, DARE, CONS>(L, prefix, S, b);
}

// rows of the table: base | models[K] | out | coef[K] | drop[K] | group
constexpr uint64_t task_rows(int K) { return 3 + 3 * (uint64_t)K; }

inline bool finite_f(float x) { return x - x == 0.f; }

}  // namespace

extern "C" {

uint64_t edt_task_merge_list_workspace_bytes(int T, int K) {
    if (T < 0 || K < 1) return 0;
    return prefix_table_words(T, task_rows(K)) * sizeof(uint64_t);
}

int edt_task_merge_list(void* const* base_t, int gdt, const void* const* model_k, int wdt, int K, void* const* out_t,
                        int odt, const uint64_t* numel, int T, const float* w, const float* c, const uint32_t* drop16,
                        double lambda, int consensus, int normalize, uint64_t seed, uint64_t step, void* workspace,
                        uint64_t workspace_bytes, void* stream) {
    g_err[0] = 0;
    if (!valid_pair(gdt, wdt)) return fail(EDT_ERR_ARG, "unsupported dtype pair (gdt/wdt)");
    if (odt != EDT_F32 && odt != EDT_BF16) return fail(EDT_ERR_ARG, "unsupported output dtype");
    if (K < 1 || K > EDT_MAX_WORKERS)
        return fail(EDT_ERR_ARG, "model count %d out of range [1, %d]", K, EDT_MAX_WORKERS);
    if (T < 0) return fail(EDT_ERR_ARG, "tensor count %d < 0", T);
    if (!finite_f((float)lambda)) return fail(EDT_ERR_ARG, "lambda %g is not finite in fp32", lambda);
    if (!out_t && odt != gdt) return fail(EDT_ERR_ARG, "the in-place form writes the base's dtype");
    if (T == 0) return EDT_OK;
    if (!base_t || !model_k || !numel) return fail(EDT_ERR_ARG, "null tensor table");
    if (!w || !c || !drop16) return fail(EDT_ERR_ARG, "null coefficient table");
    bool dare = false;
    const uint64_t KT = (uint64_t)K * T;
    for (uint64_t x = 0; x < KT; ++x) {
        const int k = (int)(x / T), t = (int)(x % T);
        if (!finite_f(w[x]) || !finite_f(c[x])) return fail(EDT_ERR_ARG, "w[%d][%d] or c[%d][%d] is not finite", k, t, k, t);
        if (drop16[x] > 65535u) return fail(EDT_ERR_ARG, "drop16[%d][%d] = %u > 65535", k, t, drop16[x]);
        dare = dare || drop16[x] != 0;
    }
    if (int rc = check_workspace(workspace, workspace_bytes, edt_task_merge_list_workspace_bytes(T, K))) return rc;
    // the raw columns: c | w << 32 and drop16 per (k, t); the first Philox group per tensor, from the sizes
    // packed with every start rounded up to a multiple of 8
    thread_local std::vector<uint64_t> raw;
    raw.assign((2 * (uint64_t)K + 1) * T, 0);
    for (uint64_t x = 0; x < KT; ++x) {
        uint32_t cb, wb;
        memcpy(&cb, &c[x], 4);
        memcpy(&wb, &w[x], 4);
        raw[x] = (uint64_t)cb | (uint64_t)wb << 32;
        raw[KT + x] = drop16[x];
    }
    uint64_t* group = raw.data() + 2 * KT;
    uint64_t g = 0;
    for (int t = 0; t < T; ++t) {
        group[t] = g;
        g += (numel[t] + 7) / 8;
    }
    thread_local std::vector<Column> cols;
    cols.clear();
    cols.push_back({reinterpret_cast<const void* const*>(base_t), 1, "base_t"});
    cols.push_back({model_k, K, "model_k", 0, true});
    cols.push_back({reinterpret_cast<const void* const*>(out_t), 1, "out_t"});      // in place: zeros, unused
    for (int r = 0; r < 2 * K + 1; ++r) cols.push_back({nullptr, 1, "coef", 0, false, raw.data() + (uint64_t)r * T});
    thread_local std::vector<uint64_t> h;
    uint64_t chunks;
    if (!fill_prefix_table(h, numel, T, cols.data(), (int)cols.size(), "tensor", chunks, last_error())) return EDT_ERR_ARG;
    if (chunks == 0) return EDT_OK;
    // aliasing: out[t] may be base[t] exactly, in the base's dtype (the same elements in the same thread);
    // any other overlap of a written range is refused
    const uint64_t bg = gdt == EDT_BF16 ? 2 : 4, bw = wdt == EDT_BF16 ? 2 : 4, bo = odt == EDT_BF16 ? 2 : 4;
    thread_local Sweep sw;
    sw.clear();
    bool alias = !out_t;
    for (int t = 0; t < T; ++t) {
        const uint64_t n = numel[t];
        if (!n) continue;
        const bool same = !out_t || (out_t[t] == base_t[t] && odt == gdt);
        alias = alias || same;
        sw.push(base_t[t], n * bg, same);
        if (!same) sw.push(out_t[t], n * bo, true);
        for (int k = 0; k < K; ++k) sw.push(model_k[(uint64_t)k * T + t], n * bw, false);
    }
    if (!sw.writes_disjoint())
        return fail(EDT_ERR_ARG, "an output overlaps another operand (only out_t[t] == base_t[t] may alias)");
    hipStream_t st = (hipStream_t)stream;
    if (int rc = upload_table(h, workspace, st, "tensor")) return rc;
    const uint64_t* d = static_cast<const uint64_t*>(workspace);
    const uint64_t* col = d + 2 * (uint64_t)T + 1;
    TaskArgs L;
    L.prefix = d;
    L.numel = d + T + 1;
    L.base = reinterpret_cast<void* const*>(col);
    L.models = reinterpret_cast<const void* const*>(col + T);
    L.out = out_t ? reinterpret_cast<void* const*>(col + (1 + (uint64_t)K) * T) : L.base;
    L.coef = col + (2 + (uint64_t)K) * T;
    L.drop = L.coef + KT;
    L.group = L.drop + KT;
    L.T = (uint64_t)T;
    L.chunks = chunks;
    L.K = K;
    L.normalize = normalize != 0;
    L.nt_store = !alias && EDT_NT_LERP_STORES != 0;          // lerp's measured store kind for a child
    L.lambda = (float)lambda;
    L.key0 = (uint32_t)seed;
    L.key1 = (uint32_t)(seed >> 32);
    L.step = (uint32_t)step;
    const ListLaunch ll = list_launch((uint64_t)T, chunks, (uint64_t)T + 1);
    return with_pair(gdt, wdt, [&](auto G, auto W) {
        return with_dtype(odt, [&](auto O) {
            return with_bool(dare, [&](auto D) {
                return with_bool(consensus != 0, [&](auto C) {
                    return with_bool(ll.lds, [&](auto LDS) {
                        task_merge_kernel<decltype(G)::value, decltype(W)::value, decltype(O)::value, decltype(D)::value,
                                          decltype(C)::value, decltype(LDS)::value><<<ll.grid, kBlock, ll.shm, st>>>(L);
                        return check_launch("task_merge_kernel");
                    });
                });
            });
        });
    });
}

}  // extern "C"
