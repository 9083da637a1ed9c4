// k_lc_common.h -- what the loop closer's kernels (k_lc_*.h) share: the device view of the keyframe
// feature store, DescriptorDistance, the float -> int rule and the block prefix of the ordered compactions.
#pragma once
#include <hip/hip_runtime.h>

#include <climits>
#include <cstdint>

#include "../../include/ldso_lc.h"

namespace {

constexpr int kLcWave = 64;
constexpr int kLcThreads = 256;
constexpr int kLcGrid = LDSO_LC_GRID_SIZE;

// The store: S slots of up to F features.  A slot's corners are held a second time, compacted in ascending
// feature index (cdesc, cidx), and once more sorted by grid cell (cell_begin, cell_feat): SetFeatureGrid.
struct LcStore {
    ldso_lc_feature *feat;  // [S][F]
    uint4 *cdesc;           // [S][F][2] the c-th corner's descriptor
    int *cidx;              // [S][F] the c-th corner's feature index
    int *cell_begin;        // [S][cells + 1] into cell_feat; cell = iy * gw + ix
    int *cell_feat;         // [S][F] corner feature indices by cell, ascending within a cell
    int *bow_node;          // [S][F] featVec: node ids, ascending
    int *bow_begin;         // [S][F + 1] into bow_feat
    int *bow_feat;          // [S][F] feature indices in the vector's order
    int F, cells, gw, gh, w, h;
};

// float -> int as x86's truncating conversion does it (undefined in C++ outside int's range): a value that
// is not finite or does not fit becomes INT_MIN
__device__ __forceinline__ int lc_to_int(float f) {
    return (f >= -2147483648.0f && f < 2147483648.0f) ? (int)f : INT_MIN;
}

// FeatureMatcher::DescriptorDistance (FeatureMatcher.cc:16-33): eight 32-bit words, xor and population count
__device__ __forceinline__ int lc_distance(const uint4 &a0, const uint4 &a1, const uint4 &b0, const uint4 &b1) {
    return __popc(a0.x ^ b0.x) + __popc(a0.y ^ b0.y) + __popc(a0.z ^ b0.z) + __popc(a0.w ^ b0.w) +
           __popc(a1.x ^ b1.x) + __popc(a1.y ^ b1.y) + __popc(a1.z ^ b1.z) + __popc(a1.w ^ b1.w);
}
// the same on two feature records (the descriptor sits at byte 24 of the 56 byte record: 8-byte aligned)
__device__ __forceinline__ int lc_distance(const ldso_lc_feature &a, const ldso_lc_feature &b) {
    const uint32_t *pa = reinterpret_cast<const uint32_t *>(a.descriptor);
    const uint32_t *pb = reinterpret_cast<const uint32_t *>(b.descriptor);
    int d = 0;
#pragma unroll
    for (int i = 0; i < 8; i++) d += __popc(pa[i] ^ pb[i]);
    return d;
}

// count of set predicates in the block -> *total, and each thread's exclusive prefix in thread order (wave64
// ballots, no atomics: the compactions that use it keep their input's order).  Every thread of the block
// calls it; a second call needs no barrier of the caller's in between.
__device__ __forceinline__ int lc_block_prefix(bool pred, int *total) {
    __shared__ int wave_cnt[kLcThreads / kLcWave];
    const int lane = threadIdx.x & (kLcWave - 1), wv = threadIdx.x / kLcWave;
    const unsigned long long mask = __ballot(pred);
    const int before = __popcll(mask & ((1ull << lane) - 1ull));
    __syncthreads();  // the previous call's reads of wave_cnt are done
    if (lane == 0) wave_cnt[wv] = __popcll(mask);
    __syncthreads();
    int base = 0, all = 0;
    const int nw = (blockDim.x + kLcWave - 1) / kLcWave;
    for (int k = 0; k < nw; k++) {
        if (k < wv) base += wave_cnt[k];
        all += wave_cnt[k];
    }
    *total = all;
    return base + before;
}

}  // namespace
