// table_host_test.cpp — the pure layer of csrc/edt_table.h on its own: host C++ only, no ROCm, no
// GPU. Built with the host compiler under -fsanitize=address,undefined and run as a child process
// by tests/test_table_host_cpu.py. Addresses are made up and never dereferenced. Fixed seed.
#include "edt_table.h"

#include <stdlib.h>
#include <string.h>

#include <string>

using namespace edt_table;

#define CHECK(cond)                                                              \
    do {                                                                         \
        if (!(cond)) {                                                           \
            fprintf(stderr, "%s:%d: CHECK failed: %s\n", __FILE__, __LINE__, #cond); \
            exit(1);                                                             \
        }                                                                        \
    } while (0)

static uint64_t g_rng = 0x9e3779b97f4a7c15ull;
static uint64_t rnd() {                       // xorshift64
    g_rng ^= g_rng << 13;
    g_rng ^= g_rng >> 7;
    g_rng ^= g_rng << 17;
    return g_rng;
}
static uint64_t below(uint64_t n) { return rnd() % n; }

static char g_msg[512];
static const Err kErr = {g_msg, sizeof(g_msg)};
static bool said(const char* what) { return strstr(g_msg, what) != nullptr; }

static const void* addr(uint64_t a) { return reinterpret_cast<const void*>(static_cast<uintptr_t>(a)); }

static const uint64_t kSizes[] = {0, 1, 7, 8, 4096, 4097};

// ---------------------------------------------------------------------------------------
// the sweep against the pairwise rule: two non-empty ranges overlap when each starts before the
// other ends; refused when one of an overlapping pair is written

struct R {
    uint64_t lo, len;
    bool written;
};

static bool pairwise_ok(const std::vector<R>& rs) {
    for (size_t i = 0; i < rs.size(); ++i)
        for (size_t j = i + 1; j < rs.size(); ++j) {
            const R &a = rs[i], &b = rs[j];
            const bool overlap = a.len && b.len && a.lo < b.lo + b.len && b.lo < a.lo + a.len;
            if (overlap && (a.written || b.written)) return false;
        }
    return true;
}

static bool sweep_ok(const std::vector<R>& rs) {
    static Sweep sw;
    sw.clear();
    for (const R& r : rs) sw.push(addr(0x1000 + r.lo), r.len, r.written);
    return sw.writes_disjoint();
}

static void test_sweep() {
    // by hand: touching is allowed, identical reads are allowed, an identical write is not, an empty
    // range inside a written one overlaps nothing
    CHECK(sweep_ok({{0, 8, true}, {8, 8, true}}));
    CHECK(sweep_ok({{8, 8, true}, {0, 8, false}}));
    CHECK(sweep_ok({{0, 8, false}, {0, 8, false}, {4, 8, false}}));
    CHECK(!sweep_ok({{0, 8, false}, {0, 8, true}}));
    CHECK(!sweep_ok({{0, 8, true}, {0, 8, true}}));
    CHECK(!sweep_ok({{0, 16, false}, {20, 4, false}, {15, 1, true}}));
    CHECK(!sweep_ok({{0, 16, true}, {4, 2, false}}));            // a read inside a written range
    CHECK(!sweep_ok({{0, 4, false}, {2, 20, true}, {30, 1, false}, {21, 1, false}}));   // behind a later start
    CHECK(sweep_ok({{0, 16, true}, {4, 0, true}, {0, 0, false}}));
    CHECK(sweep_ok({}));
    int refused = 0, allowed = 0;
    for (int it = 0; it < 20000; ++it) {
        std::vector<R> rs(below(9));
        for (R& r : rs) {
            r.lo = below(40);
            r.len = below(4) == 0 ? 0 : below(9);
            r.written = below(3) == 0;
            if (!rs.empty() && below(6) == 0) r = rs[below(rs.size())];     // identical to another (or to itself)
            if (below(6) == 0) r.lo = rs[0].lo + rs[0].len;                 // touching the first
        }
        const bool want = pairwise_ok(rs);
        CHECK(sweep_ok(rs) == want);
        (want ? allowed : refused)++;
    }
    CHECK(refused > 1000 && allowed > 1000);       // the draw reaches both verdicts
}

// ---------------------------------------------------------------------------------------
// random columns: up to 3 columns of 1-3 rows over T <= 6 pieces

struct Cols {
    int T, ncols;
    std::vector<const void*> ptr[3];
    std::vector<uint64_t> raw;
    Column c[3];
    std::vector<uint64_t> numel;
};

static const char* kNames[3] = {"alpha", "beta", "gamma"};

// null_pct: percent of pointers that are null; skew_pct: percent that are off a 16-byte boundary
static void draw(Cols& x, unsigned null_pct, unsigned skew_pct) {
    x.T = 1 + (int)below(6);
    x.ncols = 1 + (int)below(3);
    x.numel.resize(x.T);
    for (uint64_t& n : x.numel) n = kSizes[below(6)];
    x.raw.clear();
    for (int c = 0; c < x.ncols; ++c) {
        const int rows = 1 + (int)below(3);
        const uint64_t eb = below(2) ? 2 : 4;
        x.ptr[c].resize((size_t)rows * x.T);
        for (const void*& p : x.ptr[c]) {
            const uint64_t a = 0x100000 + 16 * below(4096) + (below(100) < skew_pct ? eb * (1 + below(3)) : 0);
            p = below(100) < null_pct ? nullptr : addr(a);
        }
        x.c[c] = Column{x.ptr[c].data(), rows, kNames[c], eb, below(2) == 0};
        const unsigned kind = (unsigned)below(8);
        if (kind == 0) x.c[c].p = nullptr;                             // an operand the call does not use
        if (kind == 1) {                                               // one row of raw words
            x.raw.resize(x.T);
            for (uint64_t& w : x.raw) w = rnd();
            x.c[c] = Column{nullptr, 1, kNames[c], 0, false, x.raw.data()};
        }
    }
}

// What the walk must do for piece t with its pointers moved back by off elements: the first null in
// column / row order as a message ("" when none), the words, and the flag.
static std::string expect_piece(const Cols& x, int t, uint64_t off, std::vector<uint64_t>& words, bool& vec) {
    vec = true;
    words.clear();
    char buf[128];
    for (int c = 0; c < x.ncols; ++c) {
        const Column& col = x.c[c];
        for (int r = 0; r < col.rows; ++r) {
            if (col.raw) {
                words.push_back(col.raw[t]);
            } else if (!col.p) {
                words.push_back(0);
            } else {
                const void* p = col.p[(size_t)r * x.T + t];
                if (!p) {
                    if (col.rows > 1 || col.matrix) snprintf(buf, sizeof(buf), "%s[%d][%d] is null", col.name, r, t);
                    else snprintf(buf, sizeof(buf), "%s[%d] is null", col.name, t);
                    return buf;
                }
                const uint64_t base = reinterpret_cast<uintptr_t>(p) - off * col.elem_bytes;
                if (base % 16) vec = false;
                words.push_back(base);
            }
        }
    }
    return "";
}

static void test_walk_and_prefix_filler() {
    std::vector<uint64_t> h, words;
    int refused = 0, scalar = 0, vector = 0;
    for (int it = 0; it < 20000; ++it) {
        Cols x;
        draw(x, it % 3 == 0 ? 6 : 0, it % 2 ? 10 : 0);
        const uint64_t rows = total_rows(x.c, x.ncols);
        uint64_t chunks = ~0ull;
        g_msg[0] = 0;
        const bool ok = fill_prefix_table(h, x.numel.data(), x.T, x.c, x.ncols, "piece", chunks, kErr);
        // the first refusal in piece order; an empty piece's pointers are not looked at
        std::string want;
        bool vec;
        for (int t = 0; t < x.T && want.empty(); ++t)
            if (x.numel[t]) want = expect_piece(x, t, 0, words, vec);
        CHECK(ok == want.empty());
        if (!ok) {
            CHECK(want == g_msg);
            ++refused;
            continue;
        }
        CHECK(h.size() == prefix_table_words(x.T, rows) && h.size() == (2 + rows) * x.T + 1);
        const uint64_t *prefix = h.data(), *nflag = prefix + x.T + 1, *out = nflag + x.T;
        uint64_t sum = 0;
        CHECK(prefix[0] == 0);
        for (int t = 0; t < x.T; ++t) {
            const uint64_t n = x.numel[t];
            sum += n / kListChunk + (n % kListChunk ? 1 : 0);
            CHECK(prefix[t + 1] == sum);
            CHECK((nflag[t] & ~kVecFlag) == n);
            if (!n) continue;
            CHECK(expect_piece(x, t, 0, words, vec).empty());
            CHECK(((nflag[t] & kVecFlag) != 0) == vec);
            (vec ? vector : scalar)++;
            for (uint64_t row = 0; row < rows; ++row) CHECK(out[row * x.T + t] == words[row]);
        }
        CHECK(chunks == sum);
        // the flag-column layout over the same columns: the same words, the flag as a word of its own
        bool all_vec = false, want_all = true;
        CHECK(fill_flag_table(h, x.numel.data(), x.T, x.c, x.ncols, all_vec, kErr));
        CHECK(h.size() == flag_table_words(x.T, rows) && h.size() == (rows + 1) * x.T);
        for (int t = 0; t < x.T; ++t) {
            if (!x.numel[t]) continue;
            expect_piece(x, t, 0, words, vec);
            CHECK(h[rows * x.T + t] == (vec ? 1u : 0u));
            want_all = want_all && vec;
            for (uint64_t row = 0; row < rows; ++row) CHECK(h[row * x.T + t] == words[row]);
        }
        CHECK(all_vec == want_all);
    }
    CHECK(refused > 500 && scalar > 500 && vector > 500);
}

// prefix sums by hand at sizes that straddle a chunk, and the two size refusals
static void test_prefix_by_hand() {
    const uint64_t C = kListChunk;
    const uint64_t numel[] = {C - 1, C, C + 1, 0, 1, 2 * C, 2 * C + 1};
    const uint64_t want[] = {0, 1, 2, 4, 4, 5, 7, 10};
    const Column none[] = {{nullptr, 1, "unused"}};
    std::vector<uint64_t> h;
    uint64_t chunks = 0;
    CHECK(fill_prefix_table(h, numel, 7, none, 1, "piece", chunks, kErr));
    for (int t = 0; t <= 7; ++t) CHECK(h[t] == want[t]);
    CHECK(chunks == 10);
    if (C == 4096) {                              // the shipped chunk, in plain numbers
        const uint64_t n2[] = {0, 1, 7, 8, 4096, 4097};
        const uint64_t w2[] = {0, 0, 1, 2, 3, 4, 6};
        CHECK(fill_prefix_table(h, n2, 6, none, 1, "piece", chunks, kErr));
        for (int t = 0; t <= 6; ++t) CHECK(h[t] == w2[t]);
        CHECK(chunks == 6);
    }
    const uint64_t zero[] = {0, 0};
    CHECK(fill_prefix_table(h, zero, 2, none, 1, "piece", chunks, kErr) && chunks == 0);
    const uint64_t huge[] = {8, 1ull << 63};
    g_msg[0] = 0;
    CHECK(!fill_prefix_table(h, huge, 2, none, 1, "tensor", chunks, kErr) && said("tensor 1 too large"));
    CHECK(!fill_prefix_table(h, huge, 2, none, 1, "piece", chunks, kErr) && said("piece 1 too large"));
    const uint64_t many[] = {0x7fffffffull * C, 1};           // 2^31 chunks
    CHECK(!fill_prefix_table(h, many, 2, none, 1, "piece", chunks, kErr) && said("too many elements for one launch"));
    const uint64_t most[] = {0x7fffffffull * C};
    CHECK(fill_prefix_table(h, most, 1, none, 1, "piece", chunks, kErr) && chunks == 0x7fffffffull);
}

// ---------------------------------------------------------------------------------------
// the range layout

static void test_range_filler() {
    std::vector<uint64_t> h, words;
    // the refusals of test_sharded_fragment_q_cpu.py: the range [512, 1536), two pieces
    const void* th[] = {addr(0x4000), addr(0x8000)};
    const Column one[] = {{th, 1, "theta_t", 4}};
    auto fill2 = [&](uint64_t s0, uint64_t s1, uint64_t m0, uint64_t m1) {
        const uint64_t s[] = {s0, s1}, m[] = {m0, m1};
        g_msg[0] = 0;
        return fill_range_table(h, s, m, 2, 512, 1024, one, 1, kErr);
    };
    CHECK(fill2(512, 520, 8, 8) && g_msg[0] == 0);
    CHECK(!fill2(520, 512, 8, 8) && said("sorted, disjoint"));               // unsorted
    CHECK(!fill2(512, 516, 8, 8) && said("sorted, disjoint"));               // overlapping
    CHECK(!fill2(504, 520, 8, 8) && said("sorted, disjoint"));               // before the range
    CHECK(!fill2(512, 1530, 8, 8) && said("piece 1 leaves the range"));
    CHECK(!fill2(512, 520, 8, 2000) && said("piece 1 leaves the range"));
    CHECK(!fill2(512, 520, 8, 1100) && said("leaves the range"));
    CHECK(fill2(512, 1536, 8, 0));                                           // an empty piece at the range's end
    CHECK(!fill2(512, 1537, 8, 0) && said("leaves the range"));
    const void* nul[] = {addr(0x4000), nullptr};
    const Column cn[] = {{nul, 1, "theta_t", 4}};
    const uint64_t s[] = {512, 520}, m8[] = {8, 8}, m0[] = {8, 0};
    CHECK(!fill_range_table(h, s, m8, 2, 512, 1024, cn, 1, kErr) && said("theta_t[1] is null"));
    CHECK(fill_range_table(h, s, m0, 2, 512, 1024, cn, 1, kErr));            // ... which an empty piece may be
    CHECK(fill_range_table(h, nullptr, nullptr, 0, 512, 1024, cn, 1, kErr) && h.empty());   // all padding

    // by hand, an empty piece in the middle: the range [512, 1536); bf16 theta (2 B), two fp32 workers
    {
        const uint64_t st[] = {512, 600, 600, 1000}, nm[] = {8, 0, 7, 536};
        // piece 2 starts 88 elements into the range: theta 0x5000 + 176 -> base 0x5000 (aligned);
        // worker rows 0x9000 + 352 -> 0x9000, 0xa000 + 352 -> 0xa000. piece 3 (488 in): theta is
        // aligned as given, 0x6000, so its base 0x6000 - 976 is too; its worker 0 at 0xb008 rebases to
        // 0xb008 - 1952 = 0xa868: off a 16-byte boundary, so the piece takes the gather
        const void* t2[] = {addr(0x4000), nullptr, addr(0x5000 + 176), addr(0x6000)};
        const void* w2[] = {addr(0x8000), nullptr, addr(0x9000 + 352), addr(0xb008),
                            addr(0x8800), nullptr, addr(0xa000 + 352), addr(0xc000 + 1952)};
        const Column cols[] = {{t2, 1, "theta_t", 2}, {w2, 2, "theta_k", 4}};
        CHECK(fill_range_table(h, st, nm, 4, 512, 1024, cols, 2, kErr));
        CHECK(h.size() == range_table_words(4, 3) && h.size() == 20);
        const uint64_t end[] = {8, 88, 95, 1024};
        const uint64_t sflag[] = {0 | kVecFlag, 88, 88 | kVecFlag, 488};
        const uint64_t ptr[] = {0x4000, 0, 0x5000, 0x6000 - 976,            // theta
                                0x8000, 0, 0x9000, 0xa868,                   // worker 0
                                0x8800, 0, 0xa000, 0xc000};                  // worker 1
        for (int t = 0; t < 4; ++t) CHECK(h[t] == end[t] && h[4 + t] == sflag[t]);
        for (int i = 0; i < 12; ++i) CHECK(h[8 + i] == ptr[i]);
    }

    // random: consecutive pieces with gaps, the flag from the rebased pointers
    int scalar = 0, vector = 0;
    for (int it = 0; it < 20000; ++it) {
        Cols x;
        draw(x, 0, it % 2 ? 10 : 0);
        for (int c = 0; c < x.ncols; ++c) {                  // the range form has pointer columns only, all used
            if (x.c[c].raw) x.c[c] = Column{x.ptr[c].data(), 1, kNames[c], 4};
            x.c[c].p = x.ptr[c].data();
        }
        const uint64_t lo = 512 * below(4);
        std::vector<uint64_t> start(x.T);
        uint64_t at = lo;
        for (int t = 0; t < x.T; ++t) {
            at += below(3) ? 0 : below(20);
            start[t] = at;
            at += x.numel[t];
        }
        const uint64_t n = at - lo + below(3);
        CHECK(fill_range_table(h, start.data(), x.numel.data(), x.T, lo, n, x.c, x.ncols, kErr));
        const uint64_t rows = total_rows(x.c, x.ncols);
        CHECK(h.size() == (2 + rows) * x.T);
        for (int t = 0; t < x.T; ++t) {
            const uint64_t rel = start[t] - lo;
            CHECK(h[t] == rel + x.numel[t]);
            CHECK((h[x.T + t] & ~kVecFlag) == rel);
            if (!x.numel[t]) {
                CHECK(!(h[x.T + t] & kVecFlag));             // an empty piece never takes the vector loads
                continue;
            }
            bool vec;
            CHECK(expect_piece(x, t, rel, words, vec).empty());
            CHECK(((h[x.T + t] & kVecFlag) != 0) == vec);
            (vec ? vector : scalar)++;
            for (uint64_t row = 0; row < rows; ++row) CHECK(h[(2 + row) * x.T + t] == words[row]);
        }
        if (n) CHECK(!fill_range_table(h, start.data(), x.numel.data(), x.T, lo, at - lo - 1, x.c, x.ncols, kErr) ||
                     x.numel[x.T - 1] == 0);
    }
    CHECK(scalar > 500 && vector > 500);
}

int main() {
    static_assert(kVecFlag == 1ull << 63 && kListLdsMaxPieces == 8191 && kListChunk == 2048ull * EDT_LIST_ITERS,
                  "the constants the device code shares");
    test_sweep();
    test_walk_and_prefix_filler();
    test_prefix_by_hand();
    test_range_filler();
    printf("table host checks ok\n");
    return 0;
}
