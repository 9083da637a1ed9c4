// loop_brute_host.cpp -- FeatureMatcher::SearchBruteForce's double loop (FeatureMatcher.cc:35-64) as the
// reference runs it: one host thread, DescriptorDistance with the popcnt instruction per 32-bit word, 2,000
// corners against K keyframes of 2,000 corners.  The figure beside tools/time_loop_match.hip's.
// Wall clock (steady_clock) around the whole loop; one JSON line on stdout.
//
//   g++ -O3 -march=native -std=c++17 -o tools/loop_brute_host tools/loop_brute_host.cpp
//   tools/loop_brute_host [keyframes]
#include <nmmintrin.h>

#include <chrono>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <random>
#include <vector>

static inline int descriptor_distance(const unsigned char *desc1, const unsigned char *desc2) {
    int dist = 0;
    const int *pa = (const int *)desc1;
    const int *pb = (const int *)desc2;
    for (int i = 0; i < 8; i++, pa++, pb++) {
        unsigned int v = *pa ^ *pb;
        dist += (int)_mm_popcnt_u64(v);
    }
    return dist;
}

int main(int argc, char **argv) {
    const int K = argc > 1 ? std::atoi(argv[1]) : 8;
    constexpr int F = 2000, th_low = 50;
    std::mt19937 rng(7);
    std::vector<uint32_t> desc((size_t)(K + 1) * F * 8);
    for (uint32_t &w : desc) w = rng();
    const unsigned char *base = (const unsigned char *)desc.data();
    long long matches = 0, checksum = 0;
    const auto t0 = std::chrono::steady_clock::now();
    for (int k = 1; k <= K; k++)
        for (int i = 0; i < F; i++) {
            int min_dist = 9999, min_dist_index = -1;
            for (int j = 0; j < F; j++) {
                const int dist = descriptor_distance(base + (size_t)i * 32, base + ((size_t)k * F + j) * 32);
                if (dist < min_dist) {
                    min_dist = dist;
                    min_dist_index = j;
                }
            }
            if (min_dist < th_low) matches++;
            checksum += min_dist + min_dist_index;
        }
    const double s = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    const double pairs = (double)K * F * F;
    std::printf("{\"keyframes\": %d, \"corners\": %d, \"seconds\": %.4f, \"pairs\": %.0f, \"pairs_per_s\": %.4g, "
                "\"matches\": %lld, \"checksum\": %lld}\n",
                K, F, s, pairs, pairs / s, matches, checksum);
    return 0;
}
