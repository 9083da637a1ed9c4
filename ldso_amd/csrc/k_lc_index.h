// k_lc_index.h -- a keyframe's features into the store:
//
//   k_lc_from_tracker  thread per feature of the tracker's last DetectCorners: the pixel from its feature
//                      list, angle, corner flag and descriptor from its output records; inv_d = -1,
//                      usable = 0 (Feature's defaults until the map fills them in).
//   k_lc_index         one block per put: the corners compacted in ascending feature index (descriptor and
//                      index: what SearchBruteForce walks), then Frame::SetFeatureGrid (Frame.cc:63-74) as a
//                      sort by (cell, feature index) -- a corner's place is the number of corners before it
//                      in that order, so a cell holds its corners in ascending index as push_back leaves
//                      them -- and the cells' starts by lower_bound over the sorted keys.  No atomics.
//                      A corner outside the grid is reported, not stored (the reference would index outside
//                      its vector).
#pragma once
#include "../../include/ldso_ct.h"
#include "k_lc_common.h"

#pragma clang fp contract(off)

namespace {

__global__ __launch_bounds__(kLcThreads) void k_lc_from_tracker(const int *__restrict__ pixel, int pixel_stride,
                                                                const ldso_ct_feature *__restrict__ src, int n,
                                                                ldso_lc_feature *__restrict__ dst) {
    const int i = blockIdx.x * kLcThreads + threadIdx.x;
    if (i >= n) return;
    const ldso_ct_feature s = src[i];
    ldso_lc_feature f;
    f.u = (float)pixel[(size_t)i * pixel_stride];
    f.v = (float)pixel[(size_t)i * pixel_stride + 1];
    f.angle = s.angle;
    f.inv_d = -1.0f;
    f.is_corner = s.is_corner;
    f.usable = 0;
#pragma unroll
    for (int k = 0; k < 32; k++) f.descriptor[k] = s.descriptor[k];
    dst[i] = f;
}

// SetFeatureGrid's cell of a corner (gridY * gw + gridX, int(uv / gridSize) in float), or -1 outside the grid
__device__ __forceinline__ int lc_cell_of(float u, float v, int gw, int gh) {
    if (!(u >= 0.0f && v >= 0.0f)) return -1;
    const int gx = lc_to_int(u / (float)kLcGrid), gy = lc_to_int(v / (float)kLcGrid);
    if (gx < 0 || gy < 0 || gx >= gw || gy >= gh) return -1;
    return gy * gw + gx;
}

constexpr int kLcIdxCorners = 0, kLcIdxBad = 1;  // status[]

// ckey, skey: [F] scratch; status (mapped host memory): the corner count, 1 if a corner lies outside the
// grid; corner_flag (mapped host memory): [n] the corner flags, which set_bow checks against
__global__ __launch_bounds__(kLcThreads) void k_lc_index(LcStore S, int slot, int n, int *__restrict__ ckey,
                                                         int *__restrict__ skey, int *__restrict__ status,
                                                         uint8_t *__restrict__ corner_flag) {
    __shared__ int s_bad;
    const ldso_lc_feature *feat = S.feat + (size_t)slot * S.F;
    uint4 *cdesc = S.cdesc + (size_t)slot * S.F * 2;
    int *cidx = S.cidx + (size_t)slot * S.F;
    int *cell_begin = S.cell_begin + (size_t)slot * (S.cells + 1);
    int *cell_feat = S.cell_feat + (size_t)slot * S.F;
    if (threadIdx.x == 0) s_bad = 0;
    __syncthreads();
    int nc = 0;
    for (int i0 = 0; i0 < n; i0 += kLcThreads) {
        const int i = i0 + threadIdx.x;
        const bool is = i < n && feat[i].is_corner != 0;
        if (i < n) corner_flag[i] = is ? 1 : 0;
        int total;
        const int c = nc + lc_block_prefix(is, &total);
        if (is) {
            // the record's descriptor is 8-byte aligned only: copied by words
            const uint32_t *w = reinterpret_cast<const uint32_t *>(feat[i].descriptor);
            cdesc[2 * c] = make_uint4(w[0], w[1], w[2], w[3]);
            cdesc[2 * c + 1] = make_uint4(w[4], w[5], w[6], w[7]);
            cidx[c] = i;
            const int cell = lc_cell_of(feat[i].u, feat[i].v, S.gw, S.gh);
            if (cell < 0) s_bad = 1;  // every writer stores the same value
            ckey[c] = cell;
        }
        nc += total;
    }
    __syncthreads();  // ckey, cidx and s_bad are complete
    const bool bad = s_bad != 0;
    if (threadIdx.x == 0) {
        status[kLcIdxCorners] = nc;
        status[kLcIdxBad] = bad ? 1 : 0;
    }
    if (bad) return;
    for (int c = threadIdx.x; c < nc; c += kLcThreads) {
        const int key = ckey[c];
        int rank = 0;
        for (int j = 0; j < nc; j++) {
            const int kj = ckey[j];
            rank += (kj < key || (kj == key && j < c)) ? 1 : 0;
        }
        cell_feat[rank] = cidx[c];
        skey[rank] = key;
    }
    __syncthreads();
    for (int cell = threadIdx.x; cell <= S.cells; cell += kLcThreads) {
        int lo = 0, hi = nc;  // lower_bound(skey, cell)
        while (lo < hi) {
            const int mid = (lo + hi) >> 1;
            if (skey[mid] < cell) lo = mid + 1;
            else hi = mid;
        }
        cell_begin[cell] = lo;
    }
}

}  // namespace
