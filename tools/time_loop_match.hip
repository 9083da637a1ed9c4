// time_loop_match.hip -- device time of k_lc_brute (SearchBruteForce of one keyframe against K stored ones,
// DESIGN §9h) by HIP events: K = 1, 64, 512 keyframes of 2,000 corners each, random descriptors.  The kernel is
// the library's own text (ldso_amd/csrc/k_lc_brute.h); the store's layout is rebuilt here from random bytes.
// Per K: --warmup launches dropped, then the median [min, max] of --reps launches, each between two events;
// descriptor pairs per second = K * 2000 * 2000 / median.  Row 0 of the K = 1 result is checked against the
// sequential loop.  One JSON document on stdout.
//
//   hipcc -O3 -std=c++17 --offload-arch=gfx950 -o tools/time_loop_match tools/time_loop_match.hip
//   tools/time_loop_match [reps] [warmup]
//
// The same loop on one host thread: tools/loop_brute_host.cpp.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <random>
#include <vector>

#include "../ldso_amd/csrc/k_lc_brute.h"

#define CHECK(expr)                                                                      \
    do {                                                                                 \
        hipError_t e_ = (expr);                                                          \
        if (e_ != hipSuccess) {                                                          \
            std::fprintf(stderr, "%s: %s\n", #expr, hipGetErrorString(e_));              \
            return 1;                                                                    \
        }                                                                                \
    } while (0)

int main(int argc, char **argv) {
    const int reps = argc > 1 ? std::atoi(argv[1]) : 30, warmup = argc > 2 ? std::atoi(argv[2]) : 5;
    constexpr int F = 2000, kMaxK = 512, S = kMaxK + 1, th_low = 50;
    std::mt19937 rng(7);
    std::vector<uint32_t> desc((size_t)S * F * 8);
    for (uint32_t &w : desc) w = rng();
    std::vector<int> cidx((size_t)S * F);
    for (size_t i = 0; i < cidx.size(); i++) cidx[i] = (int)(i % F);
    std::vector<int2> pairs(kMaxK);
    for (int k = 0; k < kMaxK; k++) pairs[k] = make_int2(k + 1, F);  // slot 0 is kf1
    uint4 *d_desc;
    int *d_cidx, *d_idx, *d_dist;
    int2 *d_pairs;
    CHECK(hipMalloc(&d_desc, desc.size() * 4));
    CHECK(hipMalloc(&d_cidx, cidx.size() * 4));
    CHECK(hipMalloc(&d_pairs, pairs.size() * sizeof(int2)));
    CHECK(hipMalloc(&d_idx, (size_t)kMaxK * F * 4));
    CHECK(hipMalloc(&d_dist, (size_t)kMaxK * F * 4));
    CHECK(hipMemcpy(d_desc, desc.data(), desc.size() * 4, hipMemcpyHostToDevice));
    CHECK(hipMemcpy(d_cidx, cidx.data(), cidx.size() * 4, hipMemcpyHostToDevice));
    CHECK(hipMemcpy(d_pairs, pairs.data(), pairs.size() * sizeof(int2), hipMemcpyHostToDevice));
    hipStream_t stream;
    CHECK(hipStreamCreate(&stream));
    hipEvent_t a, b;
    CHECK(hipEventCreate(&a));
    CHECK(hipEventCreate(&b));
    LcBfParams P{d_desc, d_cidx, d_pairs, d_idx, d_dist, 0, F, F, th_low};
    std::printf("{\"corners\": %d, \"reps\": %d, \"warmup\": %d, \"clock\": \"HIP events around one launch\", \"rows\": [", F,
                reps, warmup);
    bool first = true;
    for (int K : {1, 64, 512}) {
        std::vector<float> ms;
        for (int r = 0; r < warmup + reps; r++) {
            CHECK(hipEventRecord(a, stream));
            k_lc_brute<<<dim3((F + kLcBfThreads - 1) / kLcBfThreads, K), kLcBfThreads, 0, stream>>>(P);
            CHECK(hipEventRecord(b, stream));
            CHECK(hipEventSynchronize(b));
            CHECK(hipGetLastError());
            float t;
            CHECK(hipEventElapsedTime(&t, a, b));
            if (r >= warmup) ms.push_back(t);
        }
        std::sort(ms.begin(), ms.end());
        const double med = ms[ms.size() / 2], pairs_n = (double)K * F * F;
        std::printf("%s\n {\"keyframes\": %d, \"median_ms\": %.4f, \"min_ms\": %.4f, \"max_ms\": %.4f, \"pairs\": %.0f, "
                    "\"pairs_per_s\": %.4g}",
                    first ? "" : ",", K, med, ms.front(), ms.back(), pairs_n, pairs_n / (med * 1e-3));
        first = false;
        if (K == 1) {  // the first keyframe's row against the sequential loop
            std::vector<int> idx(F), dist(F);
            CHECK(hipMemcpy(idx.data(), d_idx, F * 4, hipMemcpyDeviceToHost));
            CHECK(hipMemcpy(dist.data(), d_dist, F * 4, hipMemcpyDeviceToHost));
            for (int i = 0; i < F; i++) {
                int best = 9999, bj = -1;
                for (int j = 0; j < F; j++) {
                    int d = 0;
                    for (int w = 0; w < 8; w++) d += __builtin_popcount(desc[(size_t)i * 8 + w] ^ desc[((size_t)F + j) * 8 + w]);
                    if (d < best) {
                        best = d;
                        bj = j;
                    }
                }
                if (dist[i] != best || idx[i] != (best < th_low ? bj : -1)) {
                    std::fprintf(stderr, "corner %d: device (%d, %d), host (%d, %d)\n", i, idx[i], dist[i], bj, best);
                    return 2;
                }
            }
        }
    }
    std::printf("\n]}\n");
    return 0;
}
