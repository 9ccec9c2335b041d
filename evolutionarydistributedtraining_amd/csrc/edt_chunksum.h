// edt_chunksum.h — the one text of the fp64 chunk sums' canonical order: the tile
// butterfly on the VALU, the tile / lane mapping of a chunk, the row table's placement and
// tree_reduce_kernel, which finishes every chunk's binary tree from the rows a pass wrote. Shared
// by the SLERP passes (edt_slerp.hip) and the pseudo-gradient statistics (edt_stats.hip), so both
// form bit-identical per-chunk sums from the same per-lane values.
#pragma once

#include "edt_common.h"

namespace {

__device__ __forceinline__ double wave_sum(double x) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) x += __shfl_xor(x, o, 64);
    return x;
}

// ---- the tile butterfly without LDS ------------------------------------------------------------
// wave_sum's descending xor butterfly (x_l += x_{l ^ o}, o = 32 .. 1) bit for bit, on the VALU:
// __shfl_xor is a ds_bpermute through the LDS crossbar (two per double and level), which on the
// Gram pass (36 sums per tile) cost more than streaming its members. Levels 32 / 16 use gfx950's
// v_permlane32_swap / v_permlane16_swap, levels 8 .. 1 DPP moves (row_ror:8; half-mirror after a
// quad reverse = xor 4; quad_perm xor 2 / xor 1). fp64 addition is commutative, so a lane forming
// partner + self instead of self + partner gets the same bits.
//
// Several values at once are TRANSPOSED at levels 32 and 16 (the swap exchanges half the values):
// for values A = v[k], B = v[h + k] a lane whose level bit is clear keeps A's pair sum, the other
// lane B's — the same pair sums the per-value butterfly forms, one swap + one add per pair instead
// of per value. After both levels, row r = lane / 16 holds N2 of the N values (index: red_index),
// and the remaining levels run on those alone.
__device__ __forceinline__ double join_d(uint32_t lo, uint32_t hi) {
    return __longlong_as_double((long long)(((uint64_t)hi << 32) | lo));
}

template <int LVL>
__device__ __forceinline__ double swap_sum(double x, double y) {
    const uint64_t bx = (uint64_t)__double_as_longlong(x), by = (uint64_t)__double_as_longlong(y);
    if constexpr (LVL == 32) {
        const auto lo = __builtin_amdgcn_permlane32_swap((uint32_t)bx, (uint32_t)by, false, false);
        const auto hi = __builtin_amdgcn_permlane32_swap((uint32_t)(bx >> 32), (uint32_t)(by >> 32), false, false);
        return join_d(lo[0], hi[0]) + join_d(lo[1], hi[1]);
    } else {
        static_assert(LVL == 16, "swap levels are 32 and 16");
        const auto lo = __builtin_amdgcn_permlane16_swap((uint32_t)bx, (uint32_t)by, false, false);
        const auto hi = __builtin_amdgcn_permlane16_swap((uint32_t)(bx >> 32), (uint32_t)(by >> 32), false, false);
        return join_d(lo[0], hi[0]) + join_d(lo[1], hi[1]);
    }
}

template <int CTRL>
__device__ __forceinline__ double dpp_d(double x) {
    const uint64_t b = (uint64_t)__double_as_longlong(x);
    return join_d((uint32_t)__builtin_amdgcn_mov_dpp((int)(uint32_t)b, CTRL, 0xf, 0xf, false),
                  (uint32_t)__builtin_amdgcn_mov_dpp((int)(uint32_t)(b >> 32), CTRL, 0xf, 0xf, false));
}

// levels 8, 4, 2, 1 of the butterfly (within each row of 16 lanes)
__device__ __forceinline__ double row_butterfly(double x) {
    x += dpp_d<0x128>(x);                 // row_ror:8       = lane ^ 8
    x += dpp_d<0x141>(dpp_d<0x1B>(x));    // half-mirror (lane ^ 7) of quad_perm [3,2,1,0] (lane ^ 3)
    x += dpp_d<0x4E>(x);                  // quad_perm [2,3,0,1] = lane ^ 2
    x += dpp_d<0xB1>(x);                  // quad_perm [1,0,3,2] = lane ^ 1
    return x;
}

template <int N>
struct Red {
    static constexpr int H1 = N / 2, N1 = H1 + (N & 1);       // after level 32
    static constexpr int H2 = N1 / 2, N2 = H2 + (N1 & 1);     // after level 16: values per row
};

// N tile sums at once: r[s] on lane l = the butterfly total of value red_index<N>(s, l)
template <int N>
__device__ __forceinline__ void tile_reduce(const double (&v)[N], double (&r)[Red<N>::N2]) {
    constexpr int H1 = Red<N>::H1, N1 = Red<N>::N1, H2 = Red<N>::H2, N2 = Red<N>::N2;
    double r1[N1];
#pragma unroll
    for (int k = 0; k < H1; ++k) r1[k] = swap_sum<32>(v[k], v[H1 + k]);
    if constexpr (N & 1) r1[H1] = swap_sum<32>(v[N - 1], v[N - 1]);
#pragma unroll
    for (int k = 0; k < H2; ++k) r[k] = swap_sum<16>(r1[k], r1[H2 + k]);
    if constexpr (N1 & 1) r[H2] = swap_sum<16>(r1[N1 - 1], r1[N1 - 1]);
#pragma unroll
    for (int s = 0; s < N2; ++s) r[s] = row_butterfly(r[s]);
}

// tile_reduce's swap levels (32 and 16) alone: r[s] on lane l = the level-16 partial of value
// red_index<N>(s, l), i.e. of the 16-lane row l / 16, position l % 16 in it.
template <int N>
__device__ __forceinline__ void tile_swap_levels(const double (&v)[N], double (&r)[Red<N>::N2]) {
    constexpr int H1 = Red<N>::H1, N1 = Red<N>::N1, H2 = Red<N>::H2;
    double r1[N1];
#pragma unroll
    for (int k = 0; k < H1; ++k) r1[k] = swap_sum<32>(v[k], v[H1 + k]);
    if constexpr (N & 1) r1[H1] = swap_sum<32>(v[N - 1], v[N - 1]);
#pragma unroll
    for (int k = 0; k < H2; ++k) r[k] = swap_sum<16>(r1[k], r1[H2 + k]);
    if constexpr (N1 & 1) r[H2] = swap_sum<16>(r1[N1 - 1], r1[N1 - 1]);
}

// row_butterfly's total (levels 8, 4, 2, 1 of the xor butterfly) of one row's 16 level-16
// partials p[i] (i = position in the row), formed serially by one lane in the butterfly's own
// pairing — lane 0's sums: (p0 + p8), then + (p4 + p12), ... — so bit-identical to it (fp64
// addition is commutative: a lane forming partner + self gets the same bits).
__device__ __forceinline__ double row_tree16(const double (&p)[16]) {
    double q8[8], q4[4];
#pragma unroll
    for (int i = 0; i < 8; ++i) q8[i] = p[i] + p[i + 8];
#pragma unroll
    for (int i = 0; i < 4; ++i) q4[i] = q8[i] + q8[i + 4];
    return (q4[0] + q4[2]) + (q4[1] + q4[3]);
}

// Which value slot s of lane `lane` holds after tile_reduce<N>, and whether this lane is the one
// writer of it (a leftover value at an odd level is held by both halves).
template <int N>
__device__ __forceinline__ int red_index(int s, int lane, bool& owner) {
    constexpr int H1 = Red<N>::H1, N1 = Red<N>::N1, H2 = Red<N>::H2;
    const bool b5 = (lane >> 5) & 1, b4 = (lane >> 4) & 1;
    owner = true;
    int s1;
    if (s < H2) {
        s1 = b4 ? H2 + s : s;
    } else {
        s1 = N1 - 1;
        owner = !b4;
    }
    if (s1 < H1) return b5 ? H1 + s1 : s1;
    owner = owner && !b5;
    return N - 1;
}

// Lane l writes, when it owns one, the value slot (l % 16) holds: store(index, value). One
// predicated store per slot (a register chosen by lane would be an indexed private array: scratch).
template <int N, typename Store>
__device__ __forceinline__ void red_store(const double (&r)[Red<N>::N2], Store&& store) {
    const int lane = threadIdx.x & 63, s = lane & 15;
#pragma unroll
    for (int q = 0; q < Red<N>::N2; ++q) {
        if (s == q) {
            bool owner;
            const int idx = red_index<N>(q, lane, owner);
            if (owner) store(idx, r[q]);
        }
    }
}

// ---- the chunk sums' canonical order (every form: pair, speculative, Gram, sharded) --------------
// A chunk [start, start + len) (len <= 64 Ki) is cut into kTileSlots = 128 tiles of its 16-B-aligned
// body [a, b): tile j holds, on lane l, the 8 elements at a + 512 j + 8 l (when below b); tile 0's
// lanes also take the < 16 head / tail elements (lane l the l-th of them) after their vector. Per
// lane the products are accumulated in element order by fp64 FMAs; the wave's xor butterfly
// (wave_sum's order, formed on the VALU by tile_reduce) gives the TILE SUM; the chunk's sum is the perfect binary tree over its 128 tile sums
// in order, adjacent pairs first ((t0 + t1) + (t2 + t3)) + ..., empty tiles 0.0. Every kernel forms
// complete subtrees — one tile per wave (the speculative passes: the workgroup's four combined
// through LDS into a level-2 row, kSpecWgRows; else a level-0 row), kStatsTPW tiles per wave combined in
// registers (the read-only stats pass), sixteen per workgroup combined in LDS (level 4) — and
// writes them as rows;
// tree_reduce_kernel finishes each chunk's tree from its rows. So every form's per-chunk sums are
// bit-identical whatever the work split (the read-only pass needs no workgroup barrier; the
// speculative passes take one: a quarter of the row bytes measured faster, EDT_SLERP_SPEC_WG_ROWS).
//
// Why this shape (profiles/r03_spec_probe_{a,b,c}.json, scripts/spec_probe.hip on the 7B body): the
// speculative pass is lerp's stream (2 reads + 1 write per element) plus the sums; one tile per wave
// in address order — lerp's own grid — costs little for the fp64 math and butterflies (6.91-7.02 ms
// vs lerp 6.80-6.92 with the row store removed); what does cost is the rows' second write stream:
// 24-B rows scattered over the table +11 %, rows padded to whole lines +3-7 %, rows placed XCD-major
// (each XCD's workgroups write one contiguous stretch, so its L2 writes back whole lines) +1.3 %.
// The previous form (one workgroup per 64 Ki chunk, grid-stride, an LDS block reduction per chunk)
// ran 7.1-8.3 ms depending on the allocation.
constexpr int kTileElems = 64 * kVec;                         // 512
constexpr int kTileSlots = 128;                               // tiles per chunk: chunks <= 64 Ki
constexpr uint32_t kMaxChunkElems = (uint32_t)kTileSlots * kTileElems;
constexpr int kWavesPerBlock = kBlock / 64;
// the row levels the kernels write: pair passes one tile per wave (level 0; the read-only stats
// pass kStatsTPW per wave, level log2 kStatsTPW), the Gram passes sixteen per workgroup (level 4)
constexpr int kPairRows = kTileSlots;                         // rows per chunk, level 0
constexpr int kGramRows = kTileSlots / 16;                    // rows per chunk, level 4
constexpr int kStatsTPW = EDT_SLERP_STATS_TPW;                // tiles per wave of the read-only pass
constexpr bool kSpecWgRows = EDT_SLERP_SPEC_WG_ROWS != 0;     // speculative pass: one row per workgroup

// One-pass grids of `units` workgroups in address order (a unit = a fixed set of a chunk's tiles);
// past the dispatch cap (a multiple of 8, so blockIdx % 8 stays the unit's XCD) they stride.
constexpr uint64_t kUnitGridCap = kGridBlockCap / 8 * 8;
inline unsigned unit_grid(uint64_t units) {
    return (unsigned)(units < kUnitGridCap ? (units ? units : 1) : kUnitGridCap);
}

// Where unit u's rows go: XCD-major — the units one XCD runs (u % 8 equal) are contiguous, so each
// XCD's L2 fills whole lines of the row table before writing them back.
__host__ __device__ __forceinline__ uint64_t unit_slot(uint64_t u, uint64_t units) {
    const uint64_t per = (units + 7) / 8;
    return (u % 8) * per + u / 8;
}

// The lane's share of tile j of chunk [start, start + len): vec(i) for its 8-element vector (when
// inside the aligned body), then (tile 0) elem(i) for its head / tail element.
template <typename Vec, typename Elem>
__device__ __forceinline__ void for_tile(uint64_t start, uint64_t len, int j, Vec&& vec, Elem&& elem) {
    const uint64_t lane = threadIdx.x & 63;
    const uint64_t end = start + len;
    const uint64_t a = (start + kVec - 1) / kVec * kVec;      // aligned body [a, b)
    const uint64_t b = end / kVec * kVec;
    const uint64_t i = a + (uint64_t)j * kTileElems + lane * kVec;
    if (a < b && i < b) vec(i);
    if (j == 0) {
        const uint64_t h_end = a < end ? a : end;
        const uint64_t t_beg = b > a ? b : h_end;
        const uint64_t nh = h_end - start, nt = end - t_beg;
        if (lane < nh + nt) elem(lane < nh ? start + lane : t_beg + (lane - nh));
    }
}

// Per chunk, one wave: the chunk's W sums from its `nrows` rows (level log2(128 / nrows)), as the
// perfect tree's upper levels — each lane combines its consecutive rows, then the ascending xor
// butterfly (1, 2, 4, ...) pairs adjacent subtrees level by level. Rows of chunk c: unit
// u = c * upc + r / rpu at row table slot unit_slot(u, nchunks * upc) * rpu + r % rpu.
__global__ __launch_bounds__(kBlock) void tree_reduce_kernel(const double* __restrict__ rows, int W, int nrows,
                                                             int upc, int rpu, int64_t nchunks,
                                                             double* __restrict__ out) {
    const uint64_t c = (uint64_t)blockIdx.x * kWavesPerBlock + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (c >= (uint64_t)nchunks) return;
    const uint64_t units = (uint64_t)nchunks * (uint64_t)upc;
    const int per_lane = nrows > 64 ? nrows / 64 : 1;
    const int lanes = nrows > 64 ? 64 : nrows;
    for (int q = 0; q < W; ++q) {
        double x = 0.0;
        if (lane < lanes) {
            for (int k = 0; k < per_lane; ++k) {              // per_lane is 1 or 2: a pair's sum
                const int r = lane * per_lane + k;
                const uint64_t u = c * (uint64_t)upc + (uint64_t)(r / rpu);
                const double v = rows[(unit_slot(u, units) * (uint64_t)rpu + (uint64_t)(r % rpu)) * (uint64_t)W + q];
                x = k == 0 ? v : x + v;
            }
        }
        for (int o = 1; o < lanes; o <<= 1) x += __shfl_xor(x, o, 64);
        if (lane == 0) out[c * (uint64_t)W + q] = x;
    }
}

inline int launch_tree_reduce(const double* rows, int W, int nrows, int upc, int rpu, int64_t nchunks, double* out,
                              hipStream_t s) {
    if (nchunks <= 0) return EDT_OK;
    const uint64_t g = ((uint64_t)nchunks + kWavesPerBlock - 1) / kWavesPerBlock;
    if (g > kGridBlockCap) return fail(EDT_ERR_ARG, "too many chunks for one launch");
    tree_reduce_kernel<<<(unsigned)g, kBlock, 0, s>>>(rows, W, nrows, upc, rpu, nchunks, out);
    return check_launch("tree_reduce_kernel");
}

// Tile 0's head / tail element of this lane, if any: elem(i).
template <typename Elem>
__device__ __forceinline__ void tile0_edge(uint64_t start, uint64_t len, Elem&& elem) {
    const uint64_t lane = threadIdx.x & 63;
    const uint64_t end = start + len;
    const uint64_t a = (start + kVec - 1) / kVec * kVec;
    const uint64_t b = end / kVec * kVec;
    const uint64_t h_end = a < end ? a : end;
    const uint64_t t_beg = b > a ? b : h_end;
    const uint64_t nh = h_end - start, nt = end - t_beg;
    if (lane < nh + nt) elem(lane < nh ? start + lane : t_beg + (lane - nh));
}

}  // namespace
