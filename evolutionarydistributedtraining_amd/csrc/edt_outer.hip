// edt_outer.hip — the DiLoCo outer step (EDT_LM/diloco.py:238-289): the fused kernel over flat
// arenas or tensor lists, its sharded halves (partial sums, SGD on a shard) and the stream-ceiling
// probe, with their C ABI entries (include/edt_sync.h).
#include "edt_step.h"

#include <algorithm>
#include <atomic>

namespace {

// ---------------------------------------------------------------------------------------
// DiLoCo outer step

struct Workers {
    const void* p[EDT_MAX_WORKERS];
};

struct OuterArgs {
    void* theta;
    void* mom;
    float* acc_out;      // partial mode
    uint64_t n;
    int K;               // workers in this launch
    float kdiv;          // divisor (K_total)
    float kinv;          // 1/K_total when K_total is a power of two
    int div_exact;       // 1: true division, 0: multiply by kinv (identical for powers of two)
    int accumulate;      // partial mode: add into acc_out
    void* acc_ws;        // chain mode: running sum in theta's dtype between launches
    int acc_in;          // chain mode: start from acc_ws
    int acc_store;       // chain mode: store the running sum to acc_ws (no SGD)
    SgdScalars sgd;
    Workers w;
    Workers bc;          // broadcast mode: round_w(theta_new) stored to these (worker dtype)
    int nbc;
    float grad_scale;    // scaled mode (SC): the pseudo-gradient's clip coefficient, last so that no
                         // other kernel argument moves
    __device__ __forceinline__ const void* wp(int k) const { return w.p[k]; }
};

// One tensor of a tensor-list launch (outer_list_kernel), seen through outer_elems: the same
// fields, worker pointers read from the device-resident table (theta_k[k * T + t]).
struct TensorArgs {
    void* theta;
    void* mom;
    float* acc_out;
    int K;
    float kdiv;
    float kinv;
    int accumulate;
    void* acc_ws;
    int acc_in;
    int acc_store;
    SgdScalars sgd;
    const void* const* w;
    uint64_t T;
    uint64_t t;
    __device__ __forceinline__ const void* wp(int k) const { return w[(uint64_t)k * T + t]; }
};
// the scaled list step's tensor (SC): the clip coefficient beside the same fields
struct TensorArgsScaled : TensorArgs {
    float grad_scale;
};
// the mixing list step's run (MX): the merge destinations live[j * T + t], j < nmix, in the worker
// dtype, and lerp's two coefficients beside the same fields
struct TensorArgsMix : TensorArgs {
    void* const* live;
    int nmix;
    float c0, c1;
    __device__ __forceinline__ void* lp(int j) const { return live[(uint64_t)j * T + t]; }
};

// MX: what the step does with theta_new beyond storing it (edt_outer_step_list_mix).
//   MX_BLEND  every destination is loaded and blended (it may be a worker this thread has read)
//   MX_HELD   destination j IS worker j and nmix == K (KC > 0): the values the delta loaded are
//             blended from registers, no second load
//   MX_COPY   mix == 1: the destination is not read, round_w(theta_new) is stored (BC's stores)
enum MixKind : int { MX_NONE = 0, MX_BLEND = 1, MX_HELD = 2, MX_COPY = 3 };

// MODE_CHAIN = MODE_FUSED for populations above EDT_MAX_WORKERS: launches of <= 64 workers
// carry the running sum in theta's dtype (lossless: it is rounded to that dtype after every add).
enum { MODE_FUSED = 0, MODE_PARTIAL = 1, MODE_CHAIN = 2 };

// Per-element accumulation acc = sum_k round(round(w_k - g) / K) in the precision of GDT
// (worker-major order, EDT_LM/diloco.py:243-246). MODE_PARTIAL sums the rounded quotients
// in fp32 instead (the cross-rank sum is then an fp32 RCCL reduction).
template <int GDT, int WDT, int KC, int DIV, int MODE, int N, class A, int H2 = 4, bool BC = false, bool SC = false,
          int MX = MX_NONE>
__device__ __forceinline__ void outer_elems(const A& a, uint64_t i) {
    static_assert(MX != MX_HELD || KC > 0, "the held form needs a compile-time worker count");
    float g[N], acc[N], b_in[N];
    [[maybe_unused]] float held[MX == MX_HELD ? KC : 1][N];      // MX_HELD: every worker's values as loaded
    ld<GDT, N, (EDT_NT_RMW != 0), H2>(a.theta, i, g);
    if constexpr (MODE != MODE_PARTIAL) ld_momentum<GDT, N, H2>(a.mom, i, a.sgd, b_in);
    if (MODE == MODE_PARTIAL && a.accumulate) {
        ld<EDT_F32, N, false, H2>(a.acc_out, i, acc);      // continue the running sum in worker order
    } else if (MODE == MODE_CHAIN && a.acc_in) {
        ld<GDT, N, false, H2>(a.acc_ws, i, acc);
    } else {
#pragma unroll
        for (int j = 0; j < N; ++j) acc[j] = 0.f;
    }
    const int K = KC > 0 ? KC : a.K;
    [[maybe_unused]] auto body = [&](int k) { add_delta<GDT, WDT, DIV, N, H2, MODE != MODE_PARTIAL>(a, k, g, acc, i); };
    if constexpr (MX == MX_HELD) {
#pragma unroll
        for (int k = 0; k < KC; ++k) add_delta<GDT, WDT, DIV, N, H2, MODE != MODE_PARTIAL>(a, k, g, acc, i, held[k]);
    } else if constexpr (KC > 0) {
#pragma unroll
        for (int k = 0; k < KC; ++k) body(k);
    } else {
#pragma unroll 4
        for (int k = 0; k < K; ++k) body(k);
    }
    if constexpr (MODE == MODE_PARTIAL) {
        st<EDT_F32, N, (EDT_NT_STORES != 0), H2>(a.acc_out, i, acc);
    } else if (MODE == MODE_CHAIN && a.acc_store) {
        st<GDT, N, (EDT_NT_STORES != 0), H2>(a.acc_ws, i, acc);
    } else {
        float grad[N];
#pragma unroll
        for (int j = 0; j < N; ++j) grad[j] = -acc[j];               // p.grad = -avg_delta
        if constexpr (SC) {                                          // clipped: one fp32 multiply, rounded
#pragma unroll
            for (int j = 0; j < N; ++j) grad[j] = grad[j] * a.grad_scale;
            rnd<GDT>(grad);
        }
        sgd_update<GDT, N, H2>(g, grad, a.mom, i, a.sgd, b_in);
        st<GDT, N, (EDT_NT_STORES != 0), H2>(a.theta, i, g);
        if constexpr (BC) {
            // the broadcast of EDT_LM/diloco.py:302-308 fused in: every destination starts the
            // next inner loop from theta_new rounded to the worker dtype (torch copy_: RNE). A
            // destination may be a worker this thread just read (same elements, same thread).
#pragma unroll 4
            for (int k = 0; k < a.nbc; ++k) st<WDT, N, (EDT_NT_STORES != 0), H2>(const_cast<void*>(a.bc.p[k]), i, g);
        }
        if constexpr (MX != MX_NONE) {
            // Streaming DiLoCo's merge fused in: every destination, which has usually trained on
            // since the delta's snapshot was taken, moves towards v = round_w(theta_new) (what BC
            // stores) by lerp_elems' rule in the worker dtype. A destination may be a worker this
            // thread has just read (same elements, same thread), as BC's may.
            rnd<WDT>(g);
            if constexpr (MX == MX_COPY) {                           // mix == 1: the destination is not read
#pragma unroll 4
                for (int j = 0; j < a.nmix; ++j) st<WDT, N, (EDT_NT_STORES != 0), H2>(a.lp(j), i, g);
            } else {
                float y[N];                                          // round_w(c1 * v): one for every destination
#pragma unroll
                for (int j = 0; j < N; ++j) y[j] = a.c1 * g[j];
                rnd<WDT>(y);
                if constexpr (MX == MX_HELD) {
#pragma unroll
                    for (int k = 0; k < KC; ++k) {
                        lerp_held<WDT, N>(held[k], y, a.c0);
                        st<WDT, N, (EDT_NT_STORES != 0), H2>(a.lp(k), i, held[k]);
                    }
                } else {
#pragma unroll 4
                    for (int j = 0; j < a.nmix; ++j) {
                        float x[N];
                        ld<WDT, N, false, H2>(a.lp(j), i, x);
                        lerp_held<WDT, N>(x, y, a.c0);
                        st<WDT, N, (EDT_NT_STORES != 0), H2>(a.lp(j), i, x);
                    }
                }
            }
        }
    }
}

// DIV = 1: true division by K (torch CPU `delta / num_models`); DIV = 0: multiply by 1/K,
// bit-identical when K is a power of two.
// BC: also store round_w(theta_new) into a.bc (edt_outer_step_bcast).
// SC: grad = round_g(-acc * a.grad_scale) (edt_outer_step_scaled).
template <int GDT, int WDT, int KC, int DIV, int MODE, int N, bool BC = false, bool SC = false>
__global__ __launch_bounds__(kBlock, EDT_MIN_WAVES) void outer_kernel(OuterArgs a) {
    const uint64_t stride = (uint64_t)gridDim.x * kBlock;
    const uint64_t tid = xcd_block(blockIdx.x, gridDim.x) * kBlock + threadIdx.x;
    if constexpr (N == kVec && split_halves<GDT, WDT>()) {
        // tiles of kBlock x 8 elements; thread t owns [4t, 4t+4) and [4(kBlock+t), +4) of a tile
        constexpr int H2 = 4 * kBlock;
        const uint64_t nv = a.n / (kVec * kBlock) * kBlock;
        for (uint64_t v = tid; v < nv; v += stride)
            outer_elems<GDT, WDT, KC, DIV, MODE, kVec, OuterArgs, H2, BC, SC>(a, v * kVec - 4 * threadIdx.x);
        for (uint64_t e = nv * kVec + tid; e < a.n; e += stride)     // scalar tail (< 8 x kBlock)
            outer_elems<GDT, WDT, KC, DIV, MODE, 1, OuterArgs, 4, BC, SC>(a, e);
    } else if constexpr (N == kVec) {
        const uint64_t nv = a.n / kVec;
        for (uint64_t v = tid; v < nv; v += stride)
            outer_elems<GDT, WDT, KC, DIV, MODE, kVec, OuterArgs, 4, BC, SC>(a, v * kVec);
        const uint64_t t = nv * kVec + tid;      // scalar tail (< 8 elements)
        if (t < a.n) outer_elems<GDT, WDT, KC, DIV, MODE, 1, OuterArgs, 4, BC, SC>(a, t);
    } else {
        for (uint64_t e = tid; e < a.n; e += stride) outer_elems<GDT, WDT, KC, DIV, MODE, 1, OuterArgs, 4, BC, SC>(a, e);
    }
}

// Tensor-list form: the parameters are T separate allocations (HF models loaded straight to
// the GPU), described by a table in device memory. The flat index space is cut into chunks of
// kListChunk elements that never cross a tensor; a grid-stride loop (as outer_kernel's) hands
// chunk b to a workgroup, which finds its tensor t by a binary search over the chunk prefix
// sums (uniform across the workgroup) and runs the same per-thread 8-element body as
// outer_kernel on it. Tensors whose operands are not all 16-byte aligned take the scalar body.
#ifndef EDT_LIST_ITERS          // 8-element iterations per thread per chunk
#define EDT_LIST_ITERS 2        // measured: 2-4 with the grid-stride loop beat 1 and 8-64
#endif
constexpr uint64_t kListChunk = (uint64_t)kBlock * kVec * EDT_LIST_ITERS;   // 4096 elements
constexpr uint64_t kVecFlag = 1ull << 63;                          // numel[t] bit: vector body ok

struct ListArgs {
    const uint64_t* prefix;     // T + 1 chunk prefix sums
    const uint64_t* numel;      // T, kVecFlag | numel
    void* const* theta;         // T
    void* const* mom;           // T (unused without momentum)
    const void* const* w;       // K * T, worker-major
    uint64_t T;
    uint64_t chunks;            // prefix[T]
    int K;
    float kdiv;
    float kinv;
    SgdScalars sgd;
    const uint8_t* tail;        // nullable: bf16 scalar-tail bits, tensor t's from byte tail_off[t]
    const uint64_t* tail_off;   // T
};
// edt_outer_step_list_scaled's block (SC): grad_scale trails, so the unscaled kernels keep theirs
struct ListArgsScaled : ListArgs {
    float grad_scale;
};
// edt_outer_step_list_mix's block (MX): the merge's arguments trail, as grad_scale does
struct ListArgsMix : ListArgs {
    void* const* live;          // nmix * T, destination-major, worker dtype
    int nmix;
    float c0, c1;               // lerp's coefficients: (float)(1 - mix), (float)mix
};
// The kernel's argument block by (SC, MX). A trait with plain specialisations, not a conditional over
// an expression: the kernel's mangled name carries its parameter type as written, and the host and
// device passes must agree on it symbol for symbol.
template <bool SC, int MX> struct ListArgsSel { using type = ListArgsMix; };
template <> struct ListArgsSel<false, 0> { using type = ListArgs; };
template <> struct ListArgsSel<true, 0> { using type = ListArgsScaled; };
template <bool SC, int MX>
using ListArgsOf = typename ListArgsSel<SC, MX>::type;

// SC: grad = round_g(-acc * L.grad_scale) (edt_outer_step_list_scaled), outer_elems' SC branch.
// MX: the merge into L.live (edt_outer_step_list_mix), outer_elems' MX branch.
template <int GDT, int WDT, int KC, int DIV, bool SC, int MX, class LA>
__device__ __forceinline__ void outer_list_chunk(const LA& L, const uint64_t* prefix, uint64_t b) {
    uint64_t lo = 0, hi = L.T;                       // last t with prefix[t] <= b
    while (hi - lo > 1) {
        const uint64_t mid = (lo + hi) >> 1;
        if (prefix[mid] <= b) lo = mid;
        else hi = mid;
    }
    const uint64_t t = lo;
    const uint64_t nf = L.numel[t];
    const uint64_t n = nf & ~kVecFlag;
    const uint64_t c0 = (b - prefix[t]) * kListChunk;
    const uint64_t c1 = c0 + kListChunk < n ? c0 + kListChunk : n;
    static_assert(!(SC && MX != MX_NONE), "a clipped step merges in a pass of its own");
    using TA = std::conditional_t<MX != MX_NONE, TensorArgsMix, std::conditional_t<SC, TensorArgsScaled, TensorArgs>>;
    TA a;
    if constexpr (SC) a.grad_scale = L.grad_scale;
    if constexpr (MX != MX_NONE) {
        a.live = L.live;
        a.nmix = L.nmix;
        a.c0 = L.c0;
        a.c1 = L.c1;
    }
    a.theta = L.theta[t];
    a.mom = L.sgd.use_momentum ? L.mom[t] : nullptr;
    a.acc_out = nullptr;
    a.K = L.K;
    a.kdiv = L.kdiv;
    a.kinv = L.kinv;
    a.accumulate = 0;
    a.acc_ws = nullptr;
    a.acc_in = 0;
    a.acc_store = 0;
    a.sgd = L.sgd;
    if (L.tail) a.sgd.tail = L.tail + L.tail_off[t];     // the tensor's own bits, indexed locally
    a.w = L.w;
    a.T = L.T;
    a.t = t;
    if ((nf & kVecFlag) && split_halves<GDT, WDT>()) {
        // tiles of kBlock x 8 elements in split-halves order (as outer_kernel), then a scalar tail
        constexpr uint64_t tile = (uint64_t)kBlock * kVec;
        const uint64_t vend = c0 + (c1 - c0) / tile * tile;
        for (uint64_t i = c0 + 4ull * threadIdx.x; i < vend; i += tile)
            outer_elems<GDT, WDT, KC, DIV, MODE_FUSED, kVec, TA, 4 * kBlock, false, SC, MX>(a, i);
        for (uint64_t i = vend + threadIdx.x; i < c1; i += kBlock)
            outer_elems<GDT, WDT, KC, DIV, MODE_FUSED, 1, TA, 4, false, SC, MX>(a, i);
    } else if (nf & kVecFlag) {
        const uint64_t vend = c0 + (c1 - c0) / kVec * kVec;
        for (uint64_t i = c0 + (uint64_t)threadIdx.x * kVec; i < vend; i += (uint64_t)kBlock * kVec)
            outer_elems<GDT, WDT, KC, DIV, MODE_FUSED, kVec, TA, 4, false, SC, MX>(a, i);
        const uint64_t i = vend + threadIdx.x;
        if (i < c1) outer_elems<GDT, WDT, KC, DIV, MODE_FUSED, 1, TA, 4, false, SC, MX>(a, i);
    } else {
        for (uint64_t i = c0 + threadIdx.x; i < c1; i += kBlock)
            outer_elems<GDT, WDT, KC, DIV, MODE_FUSED, 1, TA, 4, false, SC, MX>(a, i);
    }
}

// LDS = true: the chunk prefix sums are staged in LDS once per workgroup (dynamic shared
// memory, (T + 1) x 8 bytes), so the per-chunk tensor search costs LDS reads, not a chain of
// dependent global loads; LDS = false (very long tensor lists) searches the global table.
template <int GDT, int WDT, int KC, int DIV, bool LDS, bool SC = false, int MX = MX_NONE>
__global__ __launch_bounds__(kBlock, EDT_MIN_WAVES) void outer_list_kernel(ListArgsOf<SC, MX> L) {
    extern __shared__ uint64_t s_prefix[];
    const uint64_t* prefix = L.prefix;
    if constexpr (LDS) {
        for (uint64_t i = threadIdx.x; i <= L.T; i += kBlock) s_prefix[i] = L.prefix[i];
        __syncthreads();
        prefix = s_prefix;
    }
    for (uint64_t b = blockIdx.x; b < L.chunks; b += gridDim.x) outer_list_chunk<GDT, WDT, KC, DIV, SC, MX>(L, prefix, b);
}

// SGD from N per-rank fp32 partial sums of the same shard, summed in rank order (the sharded
// step's "reduce_ordered" schedule: an all-to-all delivers every rank's partial of the owned
// shard, so the cross-rank sum has one fixed order whatever the collective library does).
struct Partials {
    const float* p[EDT_MAX_WORKERS];
};

// SC: grad = round_g((-sum) * grad_scale) (edt_sgd_apply_sum_scaled, edt_sgd_apply_scaled). The clip
// coefficient is a trailing argument only the SC instantiations have (`scale` is one float with SC,
// nothing without), so the unscaled kernels keep their argument block, hidden arguments included.
template <int GDT, int N, bool SC = false, class... S>
__global__ __launch_bounds__(kBlock) void sgd_apply_sum_kernel(void* theta, Partials P, int np, void* mom,
                                                               uint64_t n, SgdScalars s, S... scale) {
    static_assert(sizeof...(S) == (SC ? 1 : 0), "one grad_scale with SC, none without");
    for_vec_tail<N>(n, [&](auto tagN, uint64_t i) {
        constexpr int M = decltype(tagN)::value;
        float g0[M], g[M];
        sgd_from_sum<GDT, M, SC>(theta, mom, i, s, np, [&](int r, float (&x)[M]) { ld<EDT_F32, M>(P.p[r], i, x); }, g0, g,
                                 scale...);
        st<GDT, M>(theta, i, g);
    });
}

// SGD from a reduced fp32 sum (the "reduce" schedule): the same step from one partial.
template <int GDT, int N, bool SC = false, class... S>
__global__ __launch_bounds__(kBlock) void sgd_apply_kernel(void* theta, const float* acc, void* mom,
                                                           uint64_t n, SgdScalars s, S... scale) {
    static_assert(sizeof...(S) == (SC ? 1 : 0), "one grad_scale with SC, none without");
    for_vec_tail<N>(n, [&](auto tagN, uint64_t i) {
        constexpr int M = decltype(tagN)::value;
        float g0[M], g[M];
        sgd_from_sum<GDT, M, SC>(theta, mom, i, s, 1, [&](int, float (&x)[M]) { ld<EDT_F32, M>(acc, i, x); }, g0, g,
                                 scale...);
        st<GDT, M>(theta, i, g);
    });
}


// ---------------------------------------------------------------------------------------
// Diagnostic: the fused step's access pattern (same operands, loads, stores, cache policy, grid)
// with a trivial body. Its time is the memory-system ceiling of the step on the device at hand:
// the fused kernel's time over it says how much of the step is anything but HBM traffic.

template <int GDT, int WDT, int KC, int N, int H2 = 4>
__device__ __forceinline__ void probe_elems(const OuterArgs& a, uint64_t i) {
    float g[N], b[N], acc[N];
    ld<GDT, N, false, H2>(a.theta, i, g);
    ld<GDT, N, false, H2>(a.mom, i, b);
#pragma unroll
    for (int j = 0; j < N; ++j) acc[j] = 0.f;
    const int K = KC > 0 ? KC : a.K;
#pragma unroll 8
    for (int k = 0; k < K; ++k) {
        float w[N];
        ld<WDT, N, nt_worker_loads<WDT, H2>(), H2>(a.wp(k), i, w);
#pragma unroll
        for (int j = 0; j < N; ++j) acc[j] += w[j];
    }
#pragma unroll
    for (int j = 0; j < N; ++j) { g[j] += acc[j] * 1e-30f; b[j] += acc[j] * 1e-30f; }
    st<GDT, N, (EDT_NT_STORES != 0), H2>(a.theta, i, g);
    st<GDT, N, (EDT_NT_STORES != 0), H2>(a.mom, i, b);
}

template <int GDT, int WDT, int KC>
__global__ __launch_bounds__(kBlock, EDT_MIN_WAVES) void probe_kernel(OuterArgs a) {
    const uint64_t stride = (uint64_t)gridDim.x * kBlock;
    const uint64_t tid = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
    if constexpr (split_halves<GDT, WDT>()) {
        constexpr int H2 = 4 * kBlock;
        const uint64_t nv = a.n / (kVec * kBlock) * kBlock;
        for (uint64_t v = tid; v < nv; v += stride) probe_elems<GDT, WDT, KC, kVec, H2>(a, v * kVec - 4 * threadIdx.x);
        for (uint64_t e = nv * kVec + tid; e < a.n; e += stride) probe_elems<GDT, WDT, KC, 1>(a, e);
    } else {
        const uint64_t nv = a.n / kVec;
        for (uint64_t v = tid; v < nv; v += stride) probe_elems<GDT, WDT, KC, kVec>(a, v * kVec);
        const uint64_t t = nv * kVec + tid;
        if (t < a.n) probe_elems<GDT, WDT, KC, 1>(a, t);
    }
}


// The broadcast of EDT_LM/diloco.py:302-308 on its own (edt_broadcast_theta): theta is read once and
// round_w(theta) stored to every destination — outer_elems' BC stores for the sharded schedules whose
// new theta arrives through the all-gather, so no local kernel holds it in registers. A pure
// stream: one 16-byte load per lane (two for fp32), then d.n stores of the same registers.
template <int GDT, int WDT, int N>
__global__ __launch_bounds__(kBlock) void broadcast_theta_kernel(const void* theta, uint64_t n, BcastDst d) {
    for_vec_tail<N>(n, [&](auto V, uint64_t i) {
        constexpr int M = decltype(V)::value;
        float g[M];
        ld<GDT, M>(theta, i, g);
        st_bcast<WDT, M>(d, i, g);
    });
}

// ---------------------------------------------------------------------------------------
// launch helpers

// The in-flight window of the fp32 fused step (EDT_OUTER_WG_PER_CU, edt_common.h): the launch's
// dynamic-LDS bytes for kernel KERN, which never touches them. Only the mix that was measured is
// capped: fp32 master and workers, K = 8 (the compile-time body), the 8-element split-halves form,
// plain fused mode (no broadcast, no clip), and — at run time — a carried momentum buffer, i.e. 8
// buffers read and 2 read and rewritten. Every other instantiation launches as it did.
template <int GDT, int WDT, int KC, int MODE, int N, bool BC, bool SC>
constexpr bool window_capped() {
    return GDT == EDT_F32 && WDT == EDT_F32 && KC == 8 && MODE == MODE_FUSED && N == kVec && !BC && !SC &&
           split_halves<GDT, WDT>();
}
// A request above 64 KB is raised for the kernel once per device (the attribute belongs to the
// current one); where the runtime refuses, the launch is uncapped.
template <auto KERN>
size_t window_lds() {
    if constexpr (kOuterWindowLds > 64 * 1024) {
        constexpr int kMaxDev = 64;
        static std::atomic<signed char> state[kMaxDev];      // 0 not asked, 1 raised, -1 refused
        int dev = 0;
        if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= kMaxDev) {
            (void)hipGetLastError();
            return 0;
        }
        signed char st = state[dev].load(std::memory_order_relaxed);
        if (st == 0) {
            st = hipFuncSetAttribute(reinterpret_cast<const void*>(KERN), hipFuncAttributeMaxDynamicSharedMemorySize,
                                     (int)kOuterWindowLds) == hipSuccess ? 1 : -1;
            if (st < 0) (void)hipGetLastError();
            state[dev].store(st, std::memory_order_relaxed);
        }
        if (st < 0) return 0;
    }
    return kOuterWindowLds;
}

template <int MODE, bool BC = false, bool SC = false>
int launch_outer(int gdt, int wdt, const OuterArgs& a, bool vec, hipStream_t s) {
    const unsigned g = grid_for(a.n, vec);
    const int kc = MODE == MODE_CHAIN ? 0 : a.K;        // chained launches always take the generic loop
    return with_pair(gdt, wdt, [&](auto G, auto W) {
        return with_kc_div<KC_FUSED>(kc, a.div_exact, [&](auto KC, auto DIV) {
            return with_bool(vec, [&](auto V) {
                constexpr int N = decltype(V)::value ? kVec : 1;
                constexpr int GD = decltype(G)::value, WD = decltype(W)::value;
                constexpr auto kern = outer_kernel<GD, WD, decltype(KC)::value, decltype(DIV)::value, MODE, N, BC, SC>;
                size_t lds = 0;
                if constexpr (window_capped<GD, WD, decltype(KC)::value, MODE, N, BC, SC>())
                    if (a.sgd.use_momentum && a.sgd.has_buf) lds = window_lds<kern>();
                kern<<<g, kBlock, lds, s>>>(a);
                return check_launch("outer_kernel");
            });
        });
    });
}

constexpr uint64_t kListLdsMaxTensors = 8191;          // (T + 1) x 8 B <= 64 KiB of LDS

template <bool SC, class LA>
int launch_list(int gdt, int wdt, const LA& L, bool div_exact, unsigned grid, hipStream_t s) {
    const bool lds = L.T <= kListLdsMaxTensors;
    const size_t shm = lds ? (size_t)(L.T + 1) * sizeof(uint64_t) : 0;
    return with_pair(gdt, wdt, [&](auto G, auto W) {
        return with_kc_div<KC_FUSED>(L.K, div_exact, [&](auto KC, auto DIV) {
            return with_bool(lds, [&](auto LDS) {
                outer_list_kernel<decltype(G)::value, decltype(W)::value, decltype(KC)::value, decltype(DIV)::value,
                                  decltype(LDS)::value, SC><<<grid, kBlock, shm, s>>>(L);
                return check_launch("outer_list_kernel");
            });
        });
    });
}

// The mixing list step: mx is MX_BLEND, MX_HELD (the host has checked KC > 0 for it) or MX_COPY.
int launch_list_mix(int gdt, int wdt, const ListArgsMix& L, bool div_exact, int mx, unsigned grid, hipStream_t s) {
    const bool lds = L.T <= kListLdsMaxTensors;
    const size_t shm = lds ? (size_t)(L.T + 1) * sizeof(uint64_t) : 0;
    return with_pair(gdt, wdt, [&](auto G, auto W) {
        return with_kc_div<KC_FUSED>(L.K, div_exact, [&](auto KC, auto DIV) {
            return with_bool(lds, [&](auto LDS) {
                constexpr int GD = decltype(G)::value, WD = decltype(W)::value, KCV = decltype(KC)::value,
                              DV = decltype(DIV)::value;
                constexpr bool LD = decltype(LDS)::value;
                if (mx == MX_COPY) outer_list_kernel<GD, WD, KCV, DV, LD, false, MX_COPY><<<grid, kBlock, shm, s>>>(L);
                else if (mx == MX_BLEND) outer_list_kernel<GD, WD, KCV, DV, LD, false, MX_BLEND><<<grid, kBlock, shm, s>>>(L);
                else if constexpr (KCV > 0) outer_list_kernel<GD, WD, KCV, DV, LD, false, MX_HELD><<<grid, kBlock, shm, s>>>(L);
                else return fail(EDT_ERR_ARG, "the held merge needs a compile-time worker count");
                return check_launch("outer_list_kernel (mix)");
            });
        });
    });
}

int fill_outer(OuterArgs& a, const void* theta, const void* const* theta_k, int K, int K_total, uint64_t n) {
    memset(&a, 0, sizeof(a));
    if (!theta && n) return fail(EDT_ERR_ARG, "theta_g is null");
    if (K < 1 || K > EDT_MAX_WORKERS)
        return fail(EDT_ERR_ARG, "worker count %d out of range [1, %d]", K, EDT_MAX_WORKERS);
    if (K_total < 1) return fail(EDT_ERR_ARG, "total worker count %d < 1", K_total);
    if (!theta_k) return fail(EDT_ERR_ARG, "theta_k is null");
    for (int k = 0; k < K; ++k) {
        if (!theta_k[k] && n) return fail(EDT_ERR_ARG, "theta_k[%d] is null", k);
        a.w.p[k] = theta_k[k];
    }
    a.theta = const_cast<void*>(theta);
    a.n = n;
    a.K = K;
    a.kdiv = (float)K_total;
    a.kinv = 1.0f / (float)K_total;
    a.div_exact = is_pow2(K_total) ? 0 : 1;
    return EDT_OK;
}

// theta, the momentum (when the step uses one) and the K workers are 16-byte aligned: with every
// further operand of the entry aligned too, the launch takes the 8-element kernels
bool outer_vec(const void* theta, const void* momentum, const SgdScalars& sg, const void* const* theta_k, int K) {
    bool vec = aligned16(theta) && (!sg.use_momentum || aligned16(momentum));
    for (int k = 0; k < K; ++k) vec = vec && aligned16(theta_k[k]);
    return vec;
}

// What the fused-step entries share after their dtype check: the argument block, the SGD scalars,
// the momentum's null check and `vec` (outer_vec).
int outer_prologue(OuterArgs& a, bool& vec, void* theta_g, int gdt, const void* const* theta_k, int K, void* momentum,
                   int has_momentum, uint64_t n, double lr, double momentum_coef, int nesterov) {
    int rc = fill_outer(a, theta_g, theta_k, K, K, n);
    if (rc) return rc;
    a.sgd = make_sgd(gdt, lr, momentum_coef, has_momentum, nesterov);
    if (a.sgd.use_momentum && !momentum && n) return fail(EDT_ERR_ARG, "momentum buffer is null");
    a.mom = momentum;
    vec = outer_vec(theta_g, momentum, a.sgd, theta_k, K);
    return EDT_OK;
}

}  // namespace

extern "C" {

int edt_probe_stream(void* theta_g, int gdt, const void* const* theta_k, int wdt, int K, void* momentum,
                     uint64_t n, void* stream) {
    g_err[0] = 0;
    if (!valid_pair(gdt, wdt)) return fail(EDT_ERR_ARG, "unsupported dtype pair (gdt/wdt)");
    OuterArgs a;
    int rc = fill_outer(a, theta_g, theta_k, K, K, n);
    if (rc) return rc;
    if (!momentum) return fail(EDT_ERR_ARG, "momentum is null");
    a.mom = momentum;
    bool vec = aligned16(theta_g) && aligned16(momentum);
    for (int k = 0; k < K; ++k) vec = vec && aligned16(theta_k[k]);
    if (!vec) return fail(EDT_ERR_ARG, "the probe needs 16-byte aligned operands");
    if (n == 0) return EDT_OK;
    const unsigned g = grid_for(n, true);
    hipStream_t s = (hipStream_t)stream;
    return with_pair(gdt, wdt, [&](auto G, auto W) {
        return with_bool(K == 8, [&](auto K8) {
            constexpr int GD = decltype(G)::value, WD = decltype(W)::value;
            constexpr auto kern = probe_kernel<GD, WD, decltype(K8)::value ? 8 : 0>;
            size_t lds = 0;                                  // the step's window, so the ceiling tracks the kernel
            if constexpr (window_capped<GD, WD, decltype(K8)::value ? 8 : 0, MODE_FUSED, kVec, false, false>())
                lds = window_lds<kern>();
            kern<<<g, kBlock, lds, s>>>(a);
            return check_launch("probe_kernel");
        });
    });
}

int edt_outer_step_bytes_per_elem(int gdt, int wdt, int K, int with_momentum) {
    const int bg = gdt == EDT_BF16 ? 2 : 4, bw = wdt == EDT_BF16 ? 2 : 4;
    return K * bw + 2 * bg + (with_momentum ? 2 * bg : 0);
}

int edt_outer_step(void* theta_g, int gdt, const void* const* theta_k, int wdt, int K,
                   void* momentum, int has_momentum, uint64_t n, double lr, double momentum_coef,
                   int nesterov, void* stream) {
    g_err[0] = 0;
    if (!valid_pair(gdt, wdt)) return fail(EDT_ERR_ARG, "unsupported dtype pair (gdt/wdt)");
    OuterArgs a;
    bool vec;
    int rc = outer_prologue(a, vec, theta_g, gdt, theta_k, K, momentum, has_momentum, n, lr, momentum_coef, nesterov);
    if (rc) return rc;
    if (n == 0) return EDT_OK;
    return launch_outer<MODE_FUSED>(gdt, wdt, a, vec, (hipStream_t)stream);
}

int edt_outer_step_tail(void* theta_g, int gdt, const void* const* theta_k, int wdt, int K,
                        void* momentum, int has_momentum, uint64_t n, double lr, double momentum_coef,
                        int nesterov, const uint8_t* tail_bits, void* stream) {
    g_err[0] = 0;
    if (!valid_pair(gdt, wdt)) return fail(EDT_ERR_ARG, "unsupported dtype pair (gdt/wdt)");
    OuterArgs a;
    bool vec;
    int rc = outer_prologue(a, vec, theta_g, gdt, theta_k, K, momentum, has_momentum, n, lr, momentum_coef, nesterov);
    if (rc) return rc;
    if (gdt == EDT_BF16) a.sgd.tail = tail_bits;    // fp32: torch's tails are FMAs too, nothing to emulate
    if (n == 0) return EDT_OK;
    return launch_outer<MODE_FUSED>(gdt, wdt, a, vec, (hipStream_t)stream);
}

int edt_outer_step_scaled(void* theta_g, int gdt, const void* const* theta_k, int wdt, int K,
                          void* momentum, int has_momentum, uint64_t n, double lr, double momentum_coef,
                          int nesterov, const uint8_t* tail_bits, float grad_scale, void* stream) {
    g_err[0] = 0;
    if (!valid_pair(gdt, wdt)) return fail(EDT_ERR_ARG, "unsupported dtype pair (gdt/wdt)");
    if (!(grad_scale >= 0.f && grad_scale <= 1.f))          // NaN fails both comparisons
        return fail(EDT_ERR_ARG, "grad_scale %g outside [0, 1]", (double)grad_scale);
    OuterArgs a;
    bool vec;
    int rc = outer_prologue(a, vec, theta_g, gdt, theta_k, K, momentum, has_momentum, n, lr, momentum_coef, nesterov);
    if (rc) return rc;
    if (gdt == EDT_BF16) a.sgd.tail = tail_bits;
    a.grad_scale = grad_scale;
    if (n == 0) return EDT_OK;
    return launch_outer<MODE_FUSED, false, true>(gdt, wdt, a, vec, (hipStream_t)stream);
}

int edt_outer_step_bcast(void* theta_g, int gdt, const void* const* theta_k, int wdt, int K,
                         void* momentum, int has_momentum, uint64_t n, double lr, double momentum_coef,
                         int nesterov, void* const* bcast, int nbcast, void* stream) {
    g_err[0] = 0;
    if (!valid_pair(gdt, wdt)) return fail(EDT_ERR_ARG, "unsupported dtype pair (gdt/wdt)");
    if (nbcast < 0 || nbcast > EDT_MAX_WORKERS)
        return fail(EDT_ERR_ARG, "broadcast count %d out of range [0, %d]", nbcast, EDT_MAX_WORKERS);
    if (nbcast == 0)
        return edt_outer_step(theta_g, gdt, theta_k, wdt, K, momentum, has_momentum, n, lr, momentum_coef, nesterov,
                              stream);
    OuterArgs a;
    bool vec;
    int rc = outer_prologue(a, vec, theta_g, gdt, theta_k, K, momentum, has_momentum, n, lr, momentum_coef, nesterov);
    if (rc) return rc;
    if (!bcast) return fail(EDT_ERR_ARG, "bcast is null");
    const uintptr_t t0 = reinterpret_cast<uintptr_t>(theta_g), t1 = t0 + n * (gdt == EDT_BF16 ? 2 : 4);
    for (int k = 0; k < nbcast; ++k) {
        if (!bcast[k] && n) return fail(EDT_ERR_ARG, "bcast[%d] is null", k);
        const uintptr_t b0 = reinterpret_cast<uintptr_t>(bcast[k]), b1 = b0 + n * (wdt == EDT_BF16 ? 2 : 4);
        if (n && b0 < t1 && t0 < b1) return fail(EDT_ERR_ARG, "bcast[%d] overlaps theta_g", k);
        a.bc.p[k] = bcast[k];
    }
    a.nbc = nbcast;
    if (n == 0) return EDT_OK;
    for (int k = 0; k < nbcast; ++k) vec = vec && aligned16(bcast[k]);
    return launch_outer<MODE_FUSED, true>(gdt, wdt, a, vec, (hipStream_t)stream);
}

int edt_broadcast_theta(const void* theta_g, int gdt, uint64_t n, void* const* bcast, int wdt, int nbcast,
                        void* stream) {
    g_err[0] = 0;
    if (!valid_pair(gdt, wdt)) return fail(EDT_ERR_ARG, "unsupported dtype pair (gdt/wdt)");
    if (int rc = check_bcast_count(nbcast)) return rc;
    if (n == 0 || nbcast == 0) return EDT_OK;
    if (!theta_g) return fail(EDT_ERR_ARG, "theta_g is null");
    bool vec = aligned16(theta_g);
    BcastDst d;
    if (int rc = fill_bcast(d, bcast, nbcast, n, wdt, theta_g, n * (gdt == EDT_BF16 ? 2 : 4), nullptr, 0, vec)) return rc;
    const unsigned g = grid_for(n, vec);
    hipStream_t s = (hipStream_t)stream;
    return with_pair(gdt, wdt, [&](auto G, auto W) {
        return with_bool(vec, [&](auto V) {
            broadcast_theta_kernel<decltype(G)::value, decltype(W)::value, decltype(V)::value ? kVec : 1>
                <<<g, kBlock, 0, s>>>(theta_g, n, d);
            return check_launch("broadcast_theta_kernel");
        });
    });
}

int edt_outer_step_ws(void* theta_g, int gdt, const void* const* theta_k, int wdt, int K, void* momentum,
                      int has_momentum, uint64_t n, double lr, double momentum_coef, int nesterov, void* workspace,
                      void* stream) {
    if (K <= EDT_MAX_WORKERS)
        return edt_outer_step(theta_g, gdt, theta_k, wdt, K, momentum, has_momentum, n, lr, momentum_coef, nesterov,
                              stream);
    g_err[0] = 0;
    if (!valid_pair(gdt, wdt)) return fail(EDT_ERR_ARG, "unsupported dtype pair (gdt/wdt)");
    if (!workspace && n) return fail(EDT_ERR_ARG, "K = %d > %d needs a workspace of n elements of theta's dtype",
                                     K, EDT_MAX_WORKERS);
    if (!theta_k) return fail(EDT_ERR_ARG, "theta_k is null");
    const SgdScalars sg = make_sgd(gdt, lr, momentum_coef, has_momentum, nesterov);
    if (sg.use_momentum && !momentum && n) return fail(EDT_ERR_ARG, "momentum buffer is null");
    if (n == 0) return EDT_OK;
    bool vec = outer_vec(theta_g, momentum, sg, theta_k, K) && aligned16(workspace);
    for (int k = 0; k < K; ++k) vec = vec && theta_k[k];    // a null worker (refused by its chunk's fill_outer)
    for (int k0 = 0; k0 < K; k0 += EDT_MAX_WORKERS) {       // worker order preserved across launches
        const int kc = K - k0 < EDT_MAX_WORKERS ? K - k0 : EDT_MAX_WORKERS;
        OuterArgs a;
        int rc = fill_outer(a, theta_g, theta_k + k0, kc, K, n);
        if (rc) return rc;
        a.sgd = sg;
        a.mom = momentum;
        a.acc_ws = workspace;
        a.acc_in = k0 > 0;
        a.acc_store = k0 + kc < K;
        rc = launch_outer<MODE_CHAIN>(gdt, wdt, a, vec, (hipStream_t)stream);
        if (rc) return rc;
    }
    return EDT_OK;
}

uint64_t edt_outer_list_workspace_bytes(int T, int K) {
    if (T < 0 || K < 1) return 0;
    return (uint64_t)(5 * (uint64_t)T + 1 + (uint64_t)K * T) * sizeof(uint64_t);
}

uint64_t edt_outer_list_mix_workspace_bytes(int T, int K, int nmix) {
    if (T < 0 || K < 1 || nmix < 1) return 0;
    return edt_outer_list_workspace_bytes(T, K) + (uint64_t)nmix * T * sizeof(uint64_t);
}

}   // extern "C"

// edt_outer_step_list_mix's merge: the destinations and the weight of theta_new in them
struct MixSpec {
    void* const* live;
    int nmix;
    double mix;
};

// The aliasing rule of the mixing step over its non-empty runs: live[j][r] may be exactly
// theta_k[j][r] (same pointer, hence the same elements in the same thread); any other overlap of a
// destination with theta, the momentum, a worker or another destination is refused. `held` is set
// when every destination is its worker and nmix == K. One sort of the byte ranges, then a sweep.
static int check_mix_ranges(void* const* theta_t, int gdt, const void* const* theta_k, int wdt, int K,
                            void* const* momentum_t, bool use_momentum, const uint64_t* numel, int T,
                            const MixSpec& mx, bool& held) {
    struct Range {
        uintptr_t lo, hi;
        int live;            // a destination (written in the worker dtype)
    };
    const uint64_t bg = gdt == EDT_BF16 ? 2 : 4, bw = wdt == EDT_BF16 ? 2 : 4;
    thread_local std::vector<Range> rs;
    rs.clear();
    held = mx.nmix == K;
    auto push = [&](const void* p, uint64_t bytes, int live) {
        const uintptr_t lo = reinterpret_cast<uintptr_t>(p);
        rs.push_back({lo, lo + bytes, live});
    };
    for (int t = 0; t < T; ++t) {
        const uint64_t n = numel[t];
        if (!n) continue;
        push(theta_t[t], n * bg, 0);
        if (use_momentum) push(momentum_t[t], n * bg, 0);
        for (int j = 0; j < mx.nmix; ++j) push(mx.live[(uint64_t)j * T + t], n * bw, 1);
        for (int k = 0; k < K; ++k) {
            const void* w = theta_k[(uint64_t)k * T + t];
            if (k < mx.nmix && w == mx.live[(uint64_t)k * T + t]) continue;      // the allowed alias: one range
            held = false;
            push(w, n * bw, 0);
        }
    }
    std::sort(rs.begin(), rs.end(), [](const Range& a, const Range& b) { return a.lo < b.lo; });
    uintptr_t end_any = 0, end_live = 0;      // furthest end so far: of any range, of a destination
    for (const Range& r : rs) {
        if (r.lo < (r.live ? end_any : end_live))
            return fail(EDT_ERR_ARG, "a merge destination overlaps another operand (only live[j] == theta_k[j] may alias)");
        if (r.hi > end_any) end_any = r.hi;
        if (r.live && r.hi > end_live) end_live = r.hi;
    }
    return EDT_OK;
}

// SC: the scaled entry (grad_scale checked first, so a refused call writes nothing). mx: the mixing
// entry's merge (null: none); its table trails the list step's in the workspace.
template <bool SC>
static int outer_step_list_impl(void* const* theta_t, int gdt, const void* const* theta_k, int wdt, int K,
                                void* const* momentum_t, int has_momentum, const uint64_t* numel, int T,
                                double lr, double momentum_coef, int nesterov, const uint8_t* tail,
                                const uint64_t* tail_off, float grad_scale, void* workspace, uint64_t workspace_bytes,
                                void* stream, const MixSpec* mx = nullptr) {
    g_err[0] = 0;
    if (!valid_pair(gdt, wdt)) return fail(EDT_ERR_ARG, "unsupported dtype pair (gdt/wdt)");
    if constexpr (SC)
        if (int rc = check_grad_scale(grad_scale)) return rc;
    if (mx) {
        if (!(mx->mix > 0.0 && mx->mix <= 1.0))                 // NaN fails both comparisons
            return fail(EDT_ERR_ARG, "mix %g outside (0, 1]", mx->mix);
        if (mx->nmix < 1 || mx->nmix > EDT_MAX_WORKERS)
            return fail(EDT_ERR_ARG, "merge destination count %d out of range [1, %d]", mx->nmix, EDT_MAX_WORKERS);
    }
    if (K < 1 || K > EDT_MAX_WORKERS)
        return fail(EDT_ERR_ARG, "worker count %d out of range [1, %d]", K, EDT_MAX_WORKERS);
    if (T < 0) return fail(EDT_ERR_ARG, "tensor count %d < 0", T);
    if (T == 0) return EDT_OK;
    if (!theta_t || !theta_k || !numel) return fail(EDT_ERR_ARG, "null tensor table");
    const SgdScalars sg = make_sgd(gdt, lr, momentum_coef, has_momentum, nesterov);
    if (sg.use_momentum && !momentum_t) return fail(EDT_ERR_ARG, "momentum table is null");
    if (mx && !mx->live) return fail(EDT_ERR_ARG, "live is null");
    const uint64_t need = mx ? edt_outer_list_mix_workspace_bytes(T, K, mx->nmix) : edt_outer_list_workspace_bytes(T, K);
    if (!workspace || workspace_bytes < need)
        return fail(EDT_ERR_ARG, "workspace of %llu bytes needed", (unsigned long long)need);
    if (reinterpret_cast<uintptr_t>(workspace) & 7u) return fail(EDT_ERR_ARG, "workspace must be 8-byte aligned");
    if (tail && (gdt != EDT_BF16 || !tail_off)) return fail(EDT_ERR_ARG, "tail bits need a bf16 master and byte offsets");
    // table: prefix[T+1] | numel[T] | theta[T] | mom[T] | w[K*T] | tail_off[T] | live[nmix*T] (mx)   (all 8-byte words)
    thread_local std::vector<uint64_t> h;
    h.assign(need / sizeof(uint64_t), 0);
    uint64_t* prefix = h.data();
    uint64_t* nflag = prefix + T + 1;
    uint64_t* pth = nflag + T;
    uint64_t* pmo = pth + T;
    uint64_t* pw = pmo + T;
    uint64_t* ptail = pw + (uint64_t)K * T;
    uint64_t* plive = ptail + T;
    if (tail)
        for (int t = 0; t < T; ++t) ptail[t] = tail_off[t];
    for (int t = 0; t < T; ++t) {
        const uint64_t n = numel[t];
        if (n >= kVecFlag) return fail(EDT_ERR_ARG, "tensor %d too large", t);
        bool vec = true;
        if (n) {
            if (!theta_t[t]) return fail(EDT_ERR_ARG, "theta_t[%d] is null", t);
            vec = aligned16(theta_t[t]);
            if (sg.use_momentum) {
                if (!momentum_t[t]) return fail(EDT_ERR_ARG, "momentum_t[%d] is null", t);
                vec = vec && aligned16(momentum_t[t]);
            }
            for (int k = 0; k < K; ++k) {
                const void* p = theta_k[(uint64_t)k * T + t];
                if (!p) return fail(EDT_ERR_ARG, "theta_k[%d][%d] is null", k, t);
                vec = vec && aligned16(p);
            }
            if (mx)
                for (int j = 0; j < mx->nmix; ++j) {
                    const void* p = mx->live[(uint64_t)j * T + t];
                    if (!p) return fail(EDT_ERR_ARG, "live[%d][%d] is null", j, t);
                    vec = vec && aligned16(p);
                }
        }
        prefix[t + 1] = prefix[t] + (n + kListChunk - 1) / kListChunk;
        nflag[t] = n | (vec ? kVecFlag : 0);
        pth[t] = reinterpret_cast<uintptr_t>(theta_t[t]);
        pmo[t] = sg.use_momentum ? reinterpret_cast<uintptr_t>(momentum_t[t]) : 0;
        for (int k = 0; k < K; ++k) pw[(uint64_t)k * T + t] = reinterpret_cast<uintptr_t>(theta_k[(uint64_t)k * T + t]);
        if (mx)
            for (int j = 0; j < mx->nmix; ++j)
                plive[(uint64_t)j * T + t] = reinterpret_cast<uintptr_t>(mx->live[(uint64_t)j * T + t]);
    }
    const uint64_t chunks = prefix[T];
    if (chunks == 0) return EDT_OK;
    if (chunks > 0x7fffffffull) return fail(EDT_ERR_ARG, "too many elements for one launch");
    bool held = false;
    if (mx)
        if (int rc = check_mix_ranges(theta_t, gdt, theta_k, wdt, K, momentum_t, sg.use_momentum != 0, numel, T, *mx, held))
            return rc;
    hipStream_t st = (hipStream_t)stream;
    // pageable source, overwritten by this thread's next call: the runtime has read it when
    // hipMemcpyAsync returns and the copy is stream-ordered on the device — pinned by
    // tests/test_gpu_list_step.py::test_back_to_back_steps (two tables of up to 4.5 MB, no host wait)
    hipError_t e = hipMemcpyAsync(workspace, h.data(), need, hipMemcpyHostToDevice, st);
    if (e != hipSuccess) return fail(EDT_ERR_LAUNCH, "tensor table upload failed: %s", hipGetErrorString(e));
    const uint64_t* d = static_cast<const uint64_t*>(workspace);
    std::conditional_t<SC, ListArgsScaled, ListArgsMix> L;      // the plain entries launch its ListArgs base
    if constexpr (SC) L.grad_scale = grad_scale;
    L.prefix = d;
    L.numel = d + T + 1;
    L.theta = reinterpret_cast<void* const*>(d + 2 * (uint64_t)T + 1);
    L.mom = reinterpret_cast<void* const*>(d + 3 * (uint64_t)T + 1);
    L.w = reinterpret_cast<const void* const*>(d + 4 * (uint64_t)T + 1);
    L.T = (uint64_t)T;
    L.chunks = chunks;
    L.K = K;
    L.kdiv = (float)K;
    L.kinv = 1.0f / (float)K;
    L.sgd = sg;
    L.tail = tail;
    L.tail_off = d + 4 * (uint64_t)T + 1 + (uint64_t)K * T;
    const unsigned grid = chunks > kMaxBlocks ? (unsigned)kMaxBlocks : (unsigned)chunks;   // grid-stride
    if constexpr (!SC) {
        if (mx) {
            L.live = reinterpret_cast<void* const*>(L.tail_off + T);
            L.nmix = mx->nmix;
            L.c0 = (float)(1.0 - mx->mix);                      // as edt_lerp forms them
            L.c1 = (float)mx->mix;
            const bool kc = K == 1 || K == 2 || K == 3 || K == 4 || K == 8;       // with_kc_div<KC_FUSED>'s bodies
            const int mode = mx->mix == 1.0 ? MX_COPY : held && kc ? MX_HELD : MX_BLEND;
            return launch_list_mix(gdt, wdt, L, !is_pow2(K), mode, grid, st);
        }
        return launch_list<SC>(gdt, wdt, static_cast<const ListArgs&>(L), !is_pow2(K), grid, st);
    } else {
        return launch_list<SC>(gdt, wdt, L, !is_pow2(K), grid, st);
    }
}

// The two sharded SGD entries and their scaled forms (SC: the clip coefficient is checked first,
// so a refused call writes nothing).
template <bool SC>
static int sgd_apply_sum_impl(void* theta_g, int gdt, const float* const* acc_f32, int nacc, void* momentum,
                              int has_momentum, uint64_t n, double lr, double momentum_coef, int nesterov,
                              float grad_scale, void* stream) {
    g_err[0] = 0;
    int rc = check_master_dtype(gdt);
    if (!rc) rc = check_partial_count(nacc);
    if (!rc && SC) rc = check_grad_scale(grad_scale);
    if (rc) return rc;
    if (n == 0) return EDT_OK;
    if (!theta_g || !acc_f32) return fail(EDT_ERR_ARG, "null buffer");
    SgdScalars s;
    if ((rc = shard_sgd(s, gdt, lr, momentum_coef, has_momentum, nesterov, momentum))) return rc;
    Partials P;
    memset(&P, 0, sizeof(P));
    bool vec = aligned16(theta_g) && (!s.use_momentum || aligned16(momentum));
    if ((rc = fill_table(P.p, acc_f32, nacc, "acc_f32", vec))) return rc;
    const unsigned g = grid_for(n, vec);
    hipStream_t st = (hipStream_t)stream;
    return with_dtype(gdt, [&](auto G) {
        return with_bool(vec, [&](auto V) {
            constexpr int GD = decltype(G)::value, N = decltype(V)::value ? kVec : 1;
            if constexpr (SC)
                sgd_apply_sum_kernel<GD, N, true><<<g, kBlock, 0, st>>>(theta_g, P, nacc, momentum, n, s, grad_scale);
            else
                sgd_apply_sum_kernel<GD, N><<<g, kBlock, 0, st>>>(theta_g, P, nacc, momentum, n, s);
            return check_launch("sgd_apply_sum_kernel");
        });
    });
}

template <bool SC>
static int sgd_apply_impl(void* theta_g, int gdt, const float* acc_f32, void* momentum, int has_momentum, uint64_t n,
                          double lr, double momentum_coef, int nesterov, float grad_scale, void* stream) {
    g_err[0] = 0;
    int rc = check_master_dtype(gdt);
    if (!rc && SC) rc = check_grad_scale(grad_scale);
    if (rc) return rc;
    if (n == 0) return EDT_OK;
    if (!theta_g || !acc_f32) return fail(EDT_ERR_ARG, "null buffer");
    SgdScalars s;
    if ((rc = shard_sgd(s, gdt, lr, momentum_coef, has_momentum, nesterov, momentum))) return rc;
    const bool vec = aligned16(theta_g) && aligned16(acc_f32) && (!s.use_momentum || aligned16(momentum));
    const unsigned g = grid_for(n, vec);
    hipStream_t st = (hipStream_t)stream;
    return with_dtype(gdt, [&](auto G) {
        return with_bool(vec, [&](auto V) {
            constexpr int GD = decltype(G)::value, N = decltype(V)::value ? kVec : 1;
            if constexpr (SC)
                sgd_apply_kernel<GD, N, true><<<g, kBlock, 0, st>>>(theta_g, acc_f32, momentum, n, s, grad_scale);
            else
                sgd_apply_kernel<GD, N><<<g, kBlock, 0, st>>>(theta_g, acc_f32, momentum, n, s);
            return check_launch("sgd_apply_kernel");
        });
    });
}

extern "C" {

int edt_outer_step_list(void* const* theta_t, int gdt, const void* const* theta_k, int wdt, int K,
                        void* const* momentum_t, int has_momentum, const uint64_t* numel, int T,
                        double lr, double momentum_coef, int nesterov, void* workspace,
                        uint64_t workspace_bytes, void* stream) {
    return outer_step_list_impl<false>(theta_t, gdt, theta_k, wdt, K, momentum_t, has_momentum, numel, T, lr,
                                       momentum_coef, nesterov, nullptr, nullptr, 1.f, workspace, workspace_bytes, stream);
}

int edt_outer_step_list_tail(void* const* theta_t, int gdt, const void* const* theta_k, int wdt, int K,
                             void* const* momentum_t, int has_momentum, const uint64_t* numel, int T,
                             double lr, double momentum_coef, int nesterov, const uint8_t* tail_bits,
                             const uint64_t* tail_byte_offset, void* workspace, uint64_t workspace_bytes,
                             void* stream) {
    return outer_step_list_impl<false>(theta_t, gdt, theta_k, wdt, K, momentum_t, has_momentum, numel, T, lr,
                                       momentum_coef, nesterov, tail_bits, tail_byte_offset, 1.f, workspace,
                                       workspace_bytes, stream);
}

int edt_outer_step_list_scaled(void* const* theta_t, int gdt, const void* const* theta_k, int wdt, int K,
                               void* const* momentum_t, int has_momentum, const uint64_t* numel, int T,
                               double lr, double momentum_coef, int nesterov, const uint8_t* tail_bits,
                               const uint64_t* tail_byte_offset, float grad_scale, void* workspace,
                               uint64_t workspace_bytes, void* stream) {
    return outer_step_list_impl<true>(theta_t, gdt, theta_k, wdt, K, momentum_t, has_momentum, numel, T, lr,
                                      momentum_coef, nesterov, tail_bits, tail_byte_offset, grad_scale, workspace,
                                      workspace_bytes, stream);
}

int edt_outer_step_list_mix(void* const* theta_t, int gdt, const void* const* theta_k, int wdt, int K,
                            void* const* momentum_t, int has_momentum, const uint64_t* numel, int T,
                            double lr, double momentum_coef, int nesterov, void* const* live, int nmix,
                            double mix, void* workspace, uint64_t workspace_bytes, void* stream) {
    const MixSpec mx = {live, nmix, mix};
    return outer_step_list_impl<false>(theta_t, gdt, theta_k, wdt, K, momentum_t, has_momentum, numel, T, lr,
                                       momentum_coef, nesterov, nullptr, nullptr, 1.f, workspace, workspace_bytes, stream,
                                       &mx);
}

int edt_delta_partial(const void* theta_g, int gdt, const void* const* theta_k, int wdt, int K_local,
                      int K_total, uint64_t n, float* acc_f32, int accumulate, void* stream) {
    g_err[0] = 0;
    if (!valid_pair(gdt, wdt)) return fail(EDT_ERR_ARG, "unsupported dtype pair (gdt/wdt)");
    OuterArgs a;
    int rc = fill_outer(a, theta_g, theta_k, K_local, K_total, n);
    if (rc) return rc;
    if (!acc_f32 && n) return fail(EDT_ERR_ARG, "acc_f32 is null");
    a.acc_out = acc_f32;
    a.accumulate = accumulate;
    if (n == 0) return EDT_OK;
    bool vec = aligned16(theta_g) && aligned16(acc_f32);
    for (int k = 0; k < K_local; ++k) vec = vec && aligned16(theta_k[k]);
    return launch_outer<MODE_PARTIAL>(gdt, wdt, a, vec, (hipStream_t)stream);
}

int edt_sgd_apply_sum(void* theta_g, int gdt, const float* const* acc_f32, int nacc, void* momentum,
                      int has_momentum, uint64_t n, double lr, double momentum_coef, int nesterov, void* stream) {
    return sgd_apply_sum_impl<false>(theta_g, gdt, acc_f32, nacc, momentum, has_momentum, n, lr, momentum_coef, nesterov,
                                     1.f, stream);
}

int edt_sgd_apply_sum_scaled(void* theta_g, int gdt, const float* const* acc_f32, int nacc, void* momentum,
                             int has_momentum, uint64_t n, double lr, double momentum_coef, int nesterov,
                             float grad_scale, void* stream) {
    return sgd_apply_sum_impl<true>(theta_g, gdt, acc_f32, nacc, momentum, has_momentum, n, lr, momentum_coef, nesterov,
                                    grad_scale, stream);
}

int edt_sgd_apply(void* theta_g, int gdt, const float* acc_f32, void* momentum, int has_momentum,
                  uint64_t n, double lr, double momentum_coef, int nesterov, void* stream) {
    return sgd_apply_impl<false>(theta_g, gdt, acc_f32, momentum, has_momentum, n, lr, momentum_coef, nesterov, 1.f,
                                 stream);
}

int edt_sgd_apply_scaled(void* theta_g, int gdt, const float* acc_f32, void* momentum, int has_momentum,
                         uint64_t n, double lr, double momentum_coef, int nesterov, float grad_scale, void* stream) {
    return sgd_apply_impl<true>(theta_g, gdt, acc_f32, momentum, has_momentum, n, lr, momentum_coef, nesterov,
                                grad_scale, stream);
}

}  // extern "C"
