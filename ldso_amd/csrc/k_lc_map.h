// k_lc_map.h -- the inverse-depth map of LoopClosing::ComputeOptimizedPose (LoopClosing.cc:266-295):
//
//   k_lc_map_gather  (from a BA context only) thread per residual of the window: the residual to the target
//                    frame with state IN writes its centerProjectedTo at its point's device index, which is
//                    the reference's traversal order (frames in window order, then point_rank); other
//                    points keep a NaN hole.  CoarseTracker.cc:364-374 tests the same condition, so this is
//                    the selection the tracker's reference cloud makes.
//   k_lc_map_write   thread per contribution: the reference stores idepthMap[u + w * v] = c[2] one
//                    contribution after the other, so a pixel keeps its last writer.  Here the contribution
//                    with no later one on the same pixel writes, with a plain store; keys travel through
//                    LDS in tiles.  No atomics.  The map has been cleared before.
//
// The pixel is int(c + 0.5f), truncating; a centre outside the image (the reference would write outside its
// array), a NaN or a hole writes nothing.  The reference's dilation loop (:297-310) runs over activePixels,
// which nothing fills: it does nothing, and nothing is dilated here.
#pragma once
#include "../../include/ldso_ba.h"
#include "k_lc_common.h"

#pragma clang fp contract(off)

namespace {

// pixel of a contribution, or -1: c + 0.5f in (-1, 0) truncates to pixel 0
__device__ __forceinline__ int lc_map_key(float cx, float cy, int w, int h) {
    const float tu = cx + 0.5f, tv = cy + 0.5f;
    if (!(tu > -1.0f && tu < (float)w && tv > -1.0f && tv < (float)h)) return -1;
    return (int)tu + w * (int)tv;
}

struct LcGatherParams {
    const float *__restrict__ center;  // planes x, y, z: center[k * plane_stride + r]
    long long plane_stride;
    const int8_t *__restrict__ state;
    const uint8_t *__restrict__ tgt;
    const int *__restrict__ slot;
    float4 *contrib;  // [P], preset to NaN holes
    int R, P, rec_base, target;
};

__global__ __launch_bounds__(kLcThreads) void k_lc_map_gather(LcGatherParams G) {
    const int r = blockIdx.x * kLcThreads + threadIdx.x;
    if (r >= G.R) return;
    if (G.tgt[r] != G.target || G.state[r] != LDSO_BA_RES_IN) return;
    const int s = G.slot[r] - G.rec_base;
    if (s < 0) return;
    const int q = s % G.P;  // a point has at most one residual per target: one writer
    G.contrib[q] = make_float4(G.center[r], G.center[G.plane_stride + r], G.center[2 * G.plane_stride + r], 0.f);
}

__global__ __launch_bounds__(kLcThreads) void k_lc_map_write(const float4 *__restrict__ contrib, int n,
                                                             float *__restrict__ map, int w, int h) {
    __shared__ int keys[kLcThreads];
    const int i = blockIdx.x * kLcThreads + threadIdx.x;
    float4 mine = make_float4(0.f, 0.f, 0.f, 0.f);
    int my = -1;
    if (i < n) {
        mine = contrib[i];
        my = lc_map_key(mine.x, mine.y, w, h);
    }
    bool last = my >= 0;
    // only the tiles from this block's own onwards hold a later contribution
    for (int t0 = blockIdx.x * kLcThreads; t0 < n; t0 += kLcThreads) {
        const int j = t0 + threadIdx.x;
        int kj = -1;
        if (j < n) {
            const float4 c = contrib[j];
            kj = lc_map_key(c.x, c.y, w, h);
        }
        __syncthreads();  // the previous tile has been read
        keys[threadIdx.x] = kj;
        __syncthreads();
        if (last) {
            const int m = min(kLcThreads, n - t0);
            for (int k = 0; k < m; k++)
                if (keys[k] == my && t0 + k > i) {
                    last = false;
                    break;
                }
        }
    }
    if (last) map[my] = mine.z;
}

}  // namespace
