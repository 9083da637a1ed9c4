// k_lc_brute.h -- FeatureMatcher::SearchBruteForce (FeatureMatcher.cc:35-64) of one keyframe against many:
//
//   k_lc_brute       grid (block of kf1's corners, keyframe).  One lane per corner of kf1 holds its eight
//                    descriptor words in registers; the other keyframe's compacted corner descriptors pass
//                    through LDS in tiles of kLcBfTile, and every lane reads the same one at a time (a
//                    broadcast read: no bank conflict).  A pair costs eight xor + popcount.  The running
//                    (dist, j) is replaced by strict <, j ascending, so the lowest j among equal minima
//                    stays: the reference's rule falls out of the loop order.
//                    One wave per block: a keyframe of 2,000 corners gives 32 blocks, and a block's barrier
//                    is its own wave's.  A tile is 4 KB: 40 blocks fit the 160 KB of a CU, more than the 32
//                    waves it holds, so LDS does not limit the occupancy (an 8 KB tile would: 5 waves per
//                    SIMD instead of 8).
//   k_lc_brute_emit  block per keyframe: the matches (dist < th_low) in ascending corner order by ballot
//                    prefix, and their count.
#pragma once
#include "k_lc_common.h"

namespace {

constexpr int kLcBfThreads = 64;  // one wave
constexpr int kLcBfTile = 128;    // descriptors per LDS tile: 4 KB
constexpr int kLcBfNone = 9999;   // min_dist's initial value (FeatureMatcher.cc:44)

struct LcBfParams {
    const uint4 *__restrict__ cdesc;  // the store's
    const int *__restrict__ cidx;
    const int2 *__restrict__ pairs;   // [n_kf] the other keyframes: slot, corner count
    int *__restrict__ idx;            // [n_kf][n1] partner feature index or -1
    int *__restrict__ dist;           // [n_kf][n1] minimum distance
    int slot1, n1, F, th_low;
};

__global__ __launch_bounds__(kLcBfThreads) void k_lc_brute(LcBfParams P) {
    __shared__ uint4 tile[2 * kLcBfTile];
    const int kf = blockIdx.y, i = blockIdx.x * kLcBfThreads + threadIdx.x;
    const int slot2 = P.pairs[kf].x, n2 = P.pairs[kf].y;
    uint4 a0 = make_uint4(0, 0, 0, 0), a1 = a0;
    if (i < P.n1) {
        const uint4 *a = P.cdesc + ((size_t)P.slot1 * P.F + i) * 2;
        a0 = a[0];
        a1 = a[1];
    }
    const uint4 *other = P.cdesc + (size_t)slot2 * P.F * 2;
    int best = kLcBfNone, best_j = -1;
    for (int t0 = 0; t0 < n2; t0 += kLcBfTile) {
        const int m = min(kLcBfTile, n2 - t0);
        __syncthreads();  // the previous tile has been read
        for (int k = threadIdx.x; k < 2 * m; k += kLcBfThreads) tile[k] = other[(size_t)2 * t0 + k];
        __syncthreads();
        // four pairs' reads in flight (54 VGPRs, still 8 waves per SIMD): a lone pair of keyframes, 32 waves on
        // the whole chip, took 16 % less time than with the compiler's two; at 512 keyframes it made no difference
#pragma unroll 4
        for (int k = 0; k < m; k++) {
            const int d = lc_distance(a0, a1, tile[2 * k], tile[2 * k + 1]);
            if (d < best) {
                best = d;
                best_j = t0 + k;
            }
        }
    }
    if (i < P.n1) {
        const size_t o = (size_t)kf * P.n1 + i;
        P.idx[o] = best_j >= 0 && best < P.th_low ? P.cidx[(size_t)slot2 * P.F + best_j] : -1;
        P.dist[o] = best;
    }
}

// matches [n_kf][n1] (a row's first counts[kf] entries), counts [n_kf]
__global__ __launch_bounds__(kLcThreads) void k_lc_brute_emit(const int *__restrict__ idx, const int *__restrict__ dist,
                                                              const int *__restrict__ cidx1, int n1,
                                                              ldso_lc_match *__restrict__ matches,
                                                              int *__restrict__ counts) {
    const int kf = blockIdx.x;
    const size_t row = (size_t)kf * n1;
    int n = 0;
    for (int i0 = 0; i0 < n1; i0 += kLcThreads) {
        const int i = i0 + threadIdx.x;
        const int j = i < n1 ? idx[row + i] : -1;
        int total;
        const int pre = lc_block_prefix(j >= 0, &total);
        if (j >= 0) {
            ldso_lc_match m;
            m.index1 = cidx1[i];
            m.index2 = j;
            m.dist = dist[row + i];
            matches[row + n + pre] = m;
        }
        n += total;
    }
    if (threadIdx.x == 0) counts[kf] = n;
}

}  // namespace
