// window_probe: does the size of the in-flight address window change the rate of the fused outer
// step's access pattern? Stand-alone (no library code, buffers from hipMalloc).
//
// The mix is the 1.3B x 8 fp32 step's: 8 worker streams read once with non-temporal loads in the
// split-halves mapping, theta and momentum read and rewritten in place, one 2,048-element tile per
// 256-thread workgroup, the grid in address order (one pass). The window is (workgroups resident
// on the chip) x 8 KB of each of the 10 buffers; resident workgroups per CU are capped by a
// dynamic-LDS request that the kernel never touches (160 KB / cap), so every cap runs the same
// instructions. Cap 0 is "uncapped": no LDS, residency as the register count allows (printed, from
// hipOccupancyMaxActiveBlocksPerMultiprocessor, as every cap's is).
//
// Per allocation draw (all 10 buffers allocated anew while the previous draw's are still held, so
// no page is reused) it runs ROUNDS rounds; a round is LAUNCHES passes over the caps, round-robin,
// each launch timed by HIP events. One JSON line per (draw, cap): the median of each round, and the
// median over all of the draw's launches of that cap. The spread of cap 0's round medians on one
// draw is the noise yardstick (scripts/window_probe_decide.py).
//
//   hipcc --offload-arch=gfx950 -O3 -std=c++17 -ffp-contract=off -o window_probe window_probe.hip
//   ./window_probe [--n N] [--draws 4] [--rounds 4] [--launches 20] [--caps 0,1,2,3,4,5,6,8] [--out F]
// -DWP_MIN_WAVES=8 bounds the body to 64 VGPRs, so that residencies above the default build's are
// reachable (another instruction schedule: its times compare with each other, not with the default).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#ifndef WP_MIN_WAVES
#define WP_MIN_WAVES 1
#endif

#define CK(x)                                                                                  \
    do {                                                                                       \
        hipError_t e_ = (x);                                                                   \
        if (e_ != hipSuccess) {                                                                \
            std::fprintf(stderr, "%s:%d %s: %s\n", __FILE__, __LINE__, #x, hipGetErrorString(e_)); \
            std::exit(2);                                                                      \
        }                                                                                      \
    } while (0)

typedef float f4 __attribute__((ext_vector_type(4)));

constexpr int kWorkers = 8;
constexpr int kThreads = 256;
constexpr uint64_t kTile = 2048;             // elements per workgroup
constexpr size_t kLdsPerCu = 160 * 1024;     // gfx950
constexpr size_t kLdsGranule = 5120;         // a multiple of every allocation granule in question

struct Args {
    const float* w[kWorkers];
    float* theta;
    float* mom;
    float kinv, mu, nlr;
};

// torch's SGD with Nesterov momentum on the averaged pseudo-gradient, one fp32 op per torch op
// (compiled with -ffp-contract=off; the two FMAs are add(..., alpha=)).
// Tile blockIdx.x is elements [2048 b, 2048 (b + 1)); thread t owns [4t, 4t + 4) of each half, so
// every access of a wave is contiguous across its lanes. The host launches exactly n / 2048
// workgroups over n % 2048 == 0 elements: no access leaves [0, n).
__global__ __launch_bounds__(kThreads, WP_MIN_WAVES) void window_step_kernel(Args a) {
    const uint64_t base = (uint64_t)blockIdx.x * kTile + 4ull * threadIdx.x;
    // both halves' loads are issued before the first store, as the step's are
    f4 w0[kWorkers], w1[kWorkers];
#pragma unroll
    for (int k = 0; k < kWorkers; ++k) {
        w0[k] = __builtin_nontemporal_load(reinterpret_cast<const f4*>(a.w[k] + base));
        w1[k] = __builtin_nontemporal_load(reinterpret_cast<const f4*>(a.w[k] + base + kTile / 2));
    }
    f4 g[2] = {*reinterpret_cast<const f4*>(a.theta + base), *reinterpret_cast<const f4*>(a.theta + base + kTile / 2)};
    f4 b[2] = {*reinterpret_cast<const f4*>(a.mom + base), *reinterpret_cast<const f4*>(a.mom + base + kTile / 2)};
    f4 acc[2] = {f4{0.f, 0.f, 0.f, 0.f}, f4{0.f, 0.f, 0.f, 0.f}};
#pragma unroll
    for (int k = 0; k < kWorkers; ++k) {
        acc[0] = acc[0] + (w0[k] - g[0]) * a.kinv;
        acc[1] = acc[1] + (w1[k] - g[1]) * a.kinv;
    }
#pragma unroll
    for (int h = 0; h < 2; ++h) {
        const f4 grad = -acc[h];
        b[h] = b[h] * a.mu + grad;
        f4 t;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const float u = __builtin_fmaf(a.mu, b[h][j], grad[j]);
            t[j] = __builtin_fmaf(a.nlr, u, g[h][j]);
        }
        g[h] = t;
    }
    *reinterpret_cast<f4*>(a.mom + base) = b[0];
    *reinterpret_cast<f4*>(a.mom + base + kTile / 2) = b[1];
    *reinterpret_cast<f4*>(a.theta + base) = g[0];
    *reinterpret_cast<f4*>(a.theta + base + kTile / 2) = g[1];
}

__global__ void fill_kernel(float* p, uint64_t n, float scale) {
    for (uint64_t i = blockIdx.x * 256ull + threadIdx.x; i < n; i += (uint64_t)gridDim.x * 256)
        p[i] = scale * (float)((i * 2654435761ull) % 1000) * 1e-3f;
}

static size_t lds_for_cap(int cap) {          // cap x lds <= 160 KB < (cap + 1) x lds, for caps 1-6 and 8
    return cap <= 0 ? 0 : kLdsPerCu / (size_t)cap / kLdsGranule * kLdsGranule;
}

static double median(std::vector<float> v) {
    std::sort(v.begin(), v.end());
    const size_t m = v.size() / 2;
    return v.size() % 2 ? v[m] : 0.5 * (v[m - 1] + v[m]);
}

int main(int argc, char** argv) {
    uint64_t n = 1315723264ull;
    int draws = 4, rounds = 4, launches = 20;
    std::vector<int> caps = {0, 1, 2, 3, 4, 5, 6, 8};
    const char* out_path = nullptr;
    for (int i = 1; i + 1 < argc; i += 2) {
        const std::string k = argv[i];
        const char* v = argv[i + 1];
        if (k == "--n") n = std::strtoull(v, nullptr, 10);
        else if (k == "--draws") draws = std::atoi(v);
        else if (k == "--rounds") rounds = std::atoi(v);
        else if (k == "--launches") launches = std::atoi(v);
        else if (k == "--out") out_path = v;
        else if (k == "--caps") {
            caps.clear();
            for (const char* q = v; *q;) {
                caps.push_back((int)std::strtol(q, const_cast<char**>(&q), 10));
                if (*q == ',') ++q;
            }
        } else {
            std::fprintf(stderr, "unknown option %s\n", argv[i]);
            return 1;
        }
    }
    n = n / kTile * kTile;
    if (n == 0 || n / kTile > 0x7fffffffull || draws < 1 || rounds < 1 || launches < 1 || caps.empty()) {
        std::fprintf(stderr, "bad arguments\n");
        return 1;
    }
    for (int c : caps)
        if (c < 0 || c > 8 || c == 7) {
            std::fprintf(stderr, "caps are 0 (uncapped), 1-6 and 8\n");
            return 1;
        }
    const unsigned grid = (unsigned)(n / kTile);
    const size_t bytes = n * sizeof(float);
    FILE* out = out_path ? std::fopen(out_path, "a") : stdout;
    if (!out) {
        std::perror(out_path);
        return 1;
    }

    // a request above 64 KB needs the attribute on some runtimes; where it is refused the launch says so
    hipError_t ea = hipFuncSetAttribute(reinterpret_cast<const void*>(window_step_kernel),
                                        hipFuncAttributeMaxDynamicSharedMemorySize, (int)kLdsPerCu);
    if (ea != hipSuccess) {
        std::fprintf(stderr, "hipFuncSetAttribute(MaxDynamicSharedMemorySize): %s\n", hipGetErrorString(ea));
        (void)hipGetLastError();
    }
    hipFuncAttributes fa;
    CK(hipFuncGetAttributes(&fa, reinterpret_cast<const void*>(window_step_kernel)));
    hipDeviceProp_t prop;
    CK(hipGetDeviceProperties(&prop, 0));
    std::vector<int> resident(caps.size(), 0);
    for (size_t c = 0; c < caps.size(); ++c)
        CK(hipOccupancyMaxActiveBlocksPerMultiprocessor(&resident[c], window_step_kernel, kThreads, lds_for_cap(caps[c])));
    std::printf("{\"probe\": \"window_probe\", \"device\": \"%s\", \"cus\": %d, \"n\": %llu, \"grid\": %u, "
                "\"min_waves\": %d, \"vgprs\": %d, \"bytes_per_launch\": %.0f}\n",
                prop.gcnArchName, prop.multiProcessorCount, (unsigned long long)n, grid, WP_MIN_WAVES, fa.numRegs,
                12.0 * (double)bytes);
    for (size_t c = 0; c < caps.size(); ++c)
        std::printf("{\"cap\": %d, \"lds_bytes\": %zu, \"resident_wg_per_cu\": %d%s}\n", caps[c], lds_for_cap(caps[c]),
                    resident[c], caps[c] == 0 ? ", \"note\": \"uncapped: the occupancy the API reports\"" : "");
    std::fflush(stdout);

    hipEvent_t e0, e1;
    CK(hipEventCreate(&e0));
    CK(hipEventCreate(&e1));
    std::vector<float*> held, spacers;
    for (int d = 0; d < draws; ++d) {
        // a new draw: an odd spacer, then 10 fresh buffers, taken while the last draw's are held
        float* sp = nullptr;
        CK(hipMalloc(&sp, (size_t)(2 * d + 1) * 3 << 20));
        spacers.push_back(sp);
        std::vector<float*> buf(kWorkers + 2, nullptr);
        for (auto& p : buf) CK(hipMalloc(&p, bytes));
        for (float* p : held) CK(hipFree(p));
        held = buf;
        for (int k = 0; k < kWorkers; ++k) fill_kernel<<<4096, 256>>>(buf[k], n, 0.02f + 0.001f * k);
        fill_kernel<<<4096, 256>>>(buf[kWorkers], n, 0.02f);
        CK(hipMemset(buf[kWorkers + 1], 0, bytes));
        CK(hipDeviceSynchronize());
        Args a;
        for (int k = 0; k < kWorkers; ++k) a.w[k] = buf[k];
        a.theta = buf[kWorkers];
        a.mom = buf[kWorkers + 1];
        a.kinv = 1.0f / kWorkers;
        a.mu = 0.9f;
        a.nlr = -0.7f;

        std::vector<int> ok(caps.size(), 1);
        for (size_t c = 0; c < caps.size(); ++c) {       // warm-up, and which caps launch at all
            window_step_kernel<<<grid, kThreads, lds_for_cap(caps[c])>>>(a);
            hipError_t e = hipGetLastError();
            if (e != hipSuccess) {
                ok[c] = 0;
                std::fprintf(stderr, "cap %d (%zu B of LDS): launch refused: %s\n", caps[c], lds_for_cap(caps[c]),
                             hipGetErrorString(e));
            }
        }
        CK(hipDeviceSynchronize());

        std::vector<std::vector<float>> all(caps.size());
        std::vector<std::vector<double>> round_med(caps.size());
        for (int r = 0; r < rounds; ++r) {
            std::vector<std::vector<float>> ms(caps.size());
            for (int l = 0; l < launches; ++l)
                for (size_t c = 0; c < caps.size(); ++c) {
                    if (!ok[c]) continue;
                    CK(hipEventRecord(e0, 0));
                    window_step_kernel<<<grid, kThreads, lds_for_cap(caps[c])>>>(a);
                    CK(hipEventRecord(e1, 0));
                    CK(hipEventSynchronize(e1));
                    float t;
                    CK(hipEventElapsedTime(&t, e0, e1));
                    ms[c].push_back(t);
                    all[c].push_back(t);
                }
            for (size_t c = 0; c < caps.size(); ++c)
                if (ok[c]) round_med[c].push_back(median(ms[c]));
        }
        CK(hipGetLastError());
        for (size_t c = 0; c < caps.size(); ++c) {
            std::string line = "{\"draw\": " + std::to_string(d) + ", \"cap\": " + std::to_string(caps[c]) +
                               ", \"lds_bytes\": " + std::to_string(lds_for_cap(caps[c])) +
                               ", \"resident_wg_per_cu\": " + std::to_string(resident[c]) +
                               ", \"min_waves\": " + std::to_string(WP_MIN_WAVES);
            if (!ok[c]) {
                line += ", \"launch\": \"refused\"}";
            } else {
                char t[160];
                const double med = median(all[c]);
                std::snprintf(t, sizeof(t), ", \"launches\": %zu, \"median_ms\": %.4f, \"TBps\": %.3f, \"round_median_ms\": [",
                              all[c].size(), med, 12.0 * (double)bytes / (med * 1e-3) / 1e12);
                line += t;
                for (size_t r = 0; r < round_med[c].size(); ++r) {
                    std::snprintf(t, sizeof(t), "%s%.4f", r ? ", " : "", round_med[c][r]);
                    line += t;
                }
                line += "]}";
            }
            std::fprintf(out, "%s\n", line.c_str());
            if (out != stdout) std::printf("%s\n", line.c_str());
        }
        std::fflush(out);
        std::fflush(stdout);
    }
    for (float* p : held) CK(hipFree(p));
    for (float* p : spacers) CK(hipFree(p));
    if (out != stdout) std::fclose(out);
    return 0;
}
