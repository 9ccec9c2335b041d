// edt_table.h — the host side of every launch that hands the GPU a table of per-tensor or per-piece
// pointers (edt_outer.hip's list steps, edt_fragment.hip, edt_fragment_q.hip, edt_stats.hip's list
// pass): which addresses a kernel may dereference, which written ranges may overlap, the upload and
// the launch geometry. Two layers:
//   pure  plain C++17, no ROCm headers, errors through a caller's buffer: the constants the device
//         code shares, the column walk, the three table layouts, the range sweep. Compiled and
//         tested on its own by tests/c_abi/table_host_test.cpp.
//   HIP   (under hipcc) the workspace check, the stream-ordered upload, the launch geometry.
// The kernels, their argument blocks and the device layouts stay in their units.
#pragma once

#include <stdarg.h>
#include <stddef.h>
#include <stdint.h>
#include <stdio.h>

#include <algorithm>
#include <vector>

#ifndef EDT_LIST_ITERS          // 8-element iterations per thread per chunk
#define EDT_LIST_ITERS 2        // measured: 2-4 with the grid-stride loop beat 1 and 8-64
#endif

namespace edt_table {

// ---------------------------------------------------------------------------------------
// pure layer

// A chunk never crosses a piece: 256 threads x 8 elements x EDT_LIST_ITERS (4096 elements).
constexpr uint64_t kListChunk = 256ull * 8 * EDT_LIST_ITERS;
constexpr uint64_t kVecFlag = 1ull << 63;           // numel[t] / start[t] bit: the piece takes the vector body
constexpr uint64_t kListLdsMaxPieces = 8191;        // (T + 1) x 8 B <= 64 KiB of LDS

// Where a refusal's message goes (the library: its thread-local edt_last_error buffer).
struct Err {
    char* buf;
    size_t cap;
};
#if defined(__GNUC__)
__attribute__((format(printf, 2, 3)))
#endif
inline bool refuse(const Err& e, const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    if (e.buf && e.cap) vsnprintf(e.buf, e.cap, fmt, ap);
    va_end(ap);
    return false;
}

// One column of a table: rows x T words at cols + (first row of the column + r) * T + t.
//   p     rows x T host pointers, row-major, to elements of elem_bytes; null (and no raw): an
//         operand the call does not use — zeros are written and nothing is checked
//   raw   instead of p: one row of T 8-byte words copied as they are (the list step's tail offsets)
//   matrix  messages say name[r][t] even when the column has one row
struct Column {
    const void* const* p;
    int rows;
    const char* name;
    uint64_t elem_bytes = 0;        // only the range form's rebase reads it
    bool matrix = false;
    const uint64_t* raw = nullptr;
};

inline uint64_t total_rows(const Column* cols, int ncols) {
    uint64_t rows = 0;
    for (int c = 0; c < ncols; ++c) rows += (uint64_t)cols[c].rows;
    return rows;
}

// The words of the NON-EMPTY piece t (an empty piece is never read by a kernel: its words stay 0
// and its pointers are not looked at). Every used pointer must be non-null; the word written is the
// pointer moved back by `off` elements (the range form's rebase; 0 otherwise), and vec says whether
// all of those are 16-byte aligned.
inline bool walk_piece(uint64_t* out, const Column* cols, int ncols, int T, int t, uint64_t off, bool& vec, const Err& e) {
    vec = true;
    uint64_t row = 0;
    for (int c = 0; c < ncols; ++c) {
        const Column& col = cols[c];
        if (col.raw) out[row * T + t] = col.raw[t];
        if (col.raw || !col.p) {
            row += (uint64_t)col.rows;
            continue;
        }
        for (int r = 0; r < col.rows; ++r, ++row) {
            const void* p = col.p[(uint64_t)r * T + t];
            if (!p)
                return col.rows > 1 || col.matrix ? refuse(e, "%s[%d][%d] is null", col.name, r, t)
                                                  : refuse(e, "%s[%d] is null", col.name, t);
            const uint64_t base = reinterpret_cast<uintptr_t>(p) - off * col.elem_bytes;
            vec = vec && (base & 15u) == 0;
            out[row * T + t] = base;
        }
    }
    return true;
}

// chunk-prefix layout: prefix[T + 1] | numel|flag [T] | cols. chunks = prefix[T].
inline uint64_t prefix_table_words(int T, uint64_t rows) { return (2 + rows) * (uint64_t)T + 1; }

inline bool fill_prefix_table(std::vector<uint64_t>& h, const uint64_t* numel, int T, const Column* cols, int ncols,
                              const char* noun, uint64_t& chunks, const Err& e) {
    h.assign(prefix_table_words(T, total_rows(cols, ncols)), 0);
    uint64_t* prefix = h.data();
    uint64_t* nflag = prefix + T + 1;
    uint64_t* out = nflag + T;
    for (int t = 0; t < T; ++t) {
        const uint64_t n = numel[t];
        if (n >= kVecFlag) return refuse(e, "%s %d too large", noun, t);
        bool vec = true;
        if (n && !walk_piece(out, cols, ncols, T, t, 0, vec, e)) return false;
        prefix[t + 1] = prefix[t] + (n + kListChunk - 1) / kListChunk;
        nflag[t] = n | (vec ? kVecFlag : 0);
    }
    chunks = prefix[T];
    if (chunks > 0x7fffffffull) return refuse(e, "too many elements for one launch");
    return true;
}

// range layout: end[T] | start|flag [T] | cols, for the pieces of the range [lo, lo + n): sorted,
// disjoint and inside it (empty pieces anywhere in it). end and start are relative to lo, and the
// pointers are rebased by the piece's start, so base[i] is element i of the range.
inline uint64_t range_table_words(int T, uint64_t rows) { return (2 + rows) * (uint64_t)T; }

inline bool fill_range_table(std::vector<uint64_t>& h, const uint64_t* start, const uint64_t* numel, int T, uint64_t lo,
                             uint64_t n, const Column* cols, int ncols, const Err& e) {
    h.assign(range_table_words(T, total_rows(cols, ncols)), 0);
    uint64_t* end = h.data();
    uint64_t* sflag = end + T;
    uint64_t* out = sflag + T;
    uint64_t prev = lo;                                  // where the piece before ends
    for (int t = 0; t < T; ++t) {
        const uint64_t s = start[t], m = numel[t];
        if (s < prev)
            return refuse(e, "piece %d starts before the range or before the end of piece %d: sorted, disjoint pieces", t,
                          t - 1);
        if (s - lo > n || m > n - (s - lo)) return refuse(e, "piece %d leaves the range", t);
        bool vec = false;
        if (m && !walk_piece(out, cols, ncols, T, t, s - lo, vec, e)) return false;
        prev = s + m;
        end[t] = prev - lo;
        sflag[t] = (s - lo) | (vec ? kVecFlag : 0);
    }
    return true;
}

// flag-column layout: cols | vec[T] (nonzero: the tensor's pointers are all 16-byte aligned).
// all_vec: every non-empty tensor's are.
inline uint64_t flag_table_words(int T, uint64_t rows) { return (rows + 1) * (uint64_t)T; }

inline bool fill_flag_table(std::vector<uint64_t>& h, const uint64_t* numel, int T, const Column* cols, int ncols,
                            bool& all_vec, const Err& e) {
    const uint64_t rows = total_rows(cols, ncols);
    h.assign(flag_table_words(T, rows), 0);
    uint64_t* pvec = h.data() + rows * (uint64_t)T;
    all_vec = true;
    for (int t = 0; t < T; ++t) {
        bool vec = true;
        if (numel[t] && !walk_piece(h.data(), cols, ncols, T, t, 0, vec, e)) return false;
        pvec[t] = vec ? 1 : 0;
        all_vec = all_vec && vec;
    }
    return true;
}

// The aliasing rule over byte ranges: a written range may overlap nothing, read ranges may overlap
// one another. Touching ranges (one ends where the next starts) do not overlap, and an empty range
// overlaps nothing. One sort, then one pass with the furthest end so far of any range and of a
// written one.
class Sweep {
public:
    void clear() { rs_.clear(); }
    void push(const void* p, uint64_t bytes, bool written) {
        const uintptr_t lo = reinterpret_cast<uintptr_t>(p);
        if (bytes) rs_.push_back({lo, lo + bytes, written});
    }
    bool writes_disjoint() {
        std::sort(rs_.begin(), rs_.end(), [](const Range& a, const Range& b) { return a.lo < b.lo; });
        uintptr_t end_any = 0, end_written = 0;
        for (const Range& r : rs_) {
            if (r.lo < (r.written ? end_any : end_written)) return false;
            if (r.hi > end_any) end_any = r.hi;
            if (r.written && r.hi > end_written) end_written = r.hi;
        }
        return true;
    }

private:
    struct Range {
        uintptr_t lo, hi;
        bool written;
    };
    std::vector<Range> rs_;
};

}  // namespace edt_table

// ---------------------------------------------------------------------------------------
// HIP layer
#if defined(__HIPCC__)
#include "edt_common.h"

namespace edt_table {
namespace {      // as edt_common.h's helpers, which these call: one copy per translation unit

static_assert(kListChunk == (uint64_t)kBlock * kVec * EDT_LIST_ITERS, "a chunk is EDT_LIST_ITERS iterations of a workgroup");

inline Err last_error() { return {g_err, sizeof(g_err)}; }

// need == 0: a launch without a table (no pieces), no workspace asked for
inline int check_workspace(const void* workspace, uint64_t workspace_bytes, uint64_t need) {
    if (!need) return EDT_OK;
    if (!workspace || workspace_bytes < need)
        return fail(EDT_ERR_ARG, "workspace of %llu bytes needed", (unsigned long long)need);
    if (reinterpret_cast<uintptr_t>(workspace) & 7u) return fail(EDT_ERR_ARG, "workspace must be 8-byte aligned");
    return EDT_OK;
}

// The table goes up by a stream-ordered copy from the caller's thread-local vector. A pageable
// source that this thread's next call overwrites is safe: the runtime has read it when the call
// returns, and the copy is ordered before the launch on the device — pinned by
// tests/test_gpu_list_step.py::test_back_to_back_steps (two tables of up to 4.5 MB, no host wait).
inline int upload_table(const std::vector<uint64_t>& h, void* workspace, hipStream_t st, const char* noun) {
    if (h.empty()) return EDT_OK;
    hipError_t e = hipMemcpyAsync(workspace, h.data(), h.size() * sizeof(uint64_t), hipMemcpyHostToDevice, st);
    if (e != hipSuccess) return fail(EDT_ERR_LAUNCH, "%s table upload failed: %s", noun, hipGetErrorString(e));
    return EDT_OK;
}

// The geometry of a launch over a table of T pieces: `blocks` workgroups of work, grid-stride past
// kMaxBlocks; lds_words 8-byte words of the table staged in LDS when T allows it.
struct ListLaunch {
    unsigned grid;
    size_t shm;
    bool lds;
};
inline ListLaunch list_launch(uint64_t T, uint64_t blocks, uint64_t lds_words) {
    const bool lds = T <= kListLdsMaxPieces;
    return {blocks > kMaxBlocks ? (unsigned)kMaxBlocks : (unsigned)blocks, lds ? (size_t)lds_words * sizeof(uint64_t) : 0, lds};
}

}  // namespace
}  // namespace edt_table
#endif
