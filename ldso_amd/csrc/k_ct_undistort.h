// k_ct_undistort.h -- frame ingestion from the raw image: PhotometricUndistorter::processFrame
// (Undistort.cc:190-230) fused with the remap loop of Undistort::undistort (Undistort.cc:398-443), or with
// its passthrough copy (:451-453).  Per new raw frame, one launch:
//   k_ct_undistort<T, kPass>   thread per output pixel, T = uint8_t / uint16_t the raw pixel type.
//       kPass false: the remap entry (xx, yy) of the pixel; xx < 0 writes 0; else the four source taps at
//       (xxi, yyi) .. (xxi + 1, yyi + 1) each get their photometric value and are blended with the
//       reference's expression, in its order.  The photometric value of a source pixel depends on that
//       pixel alone (factor * raw, G[raw] or G[raw] * vignetteInv[src]), so computing it per tap gives the
//       bits of the reference's two passes without the intermediate image.
//       kPass true: the photometric value of the pixel itself, a copy and not a blend with weights
//       1, 0, 0, 0 (0 * inf of a neighbour would be NaN).
//   The 256 entries an 8-bit frame can index go to LDS; the 65536-entry table of a 16-bit frame (256 KiB,
//   more than a CU's 160 KiB of LDS) is read from global memory.
// ldso_ct_undistort_init has stored every entry whose footprint is not inside the source as -1 (the
// footprint rule, include/ldso_ct.h), so no thread reads outside raw / vinv.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "k_ct_pyramid.h"

#pragma clang fp contract(off)

namespace {

enum : int { kUndFactor = 0, kUndLut = 1, kUndLutVignette = 2 };  // the photometric value of a source pixel

struct UndParams {
    const float2 *remap;  // [n] {xx, yy}; unused in passthrough
    const float *G;       // the LUT (kUndLut, kUndLutVignette)
    const float *vinv;    // [h_org*w_org] (kUndLutVignette)
    int w_org, n;         // source row length; output pixels
    int mode;
    float factor;         // kUndFactor
};

template <typename T>
__device__ __forceinline__ float und_photometric(const UndParams &P, const float *lut, const T *raw, int src) {
    const T r = raw[src];
    if (P.mode == kUndFactor) return P.factor * (float)r;
    const float g = lut[r];
    return P.mode == kUndLutVignette ? g * P.vinv[src] : g;
}

template <typename T, bool kPass>
__global__ __launch_bounds__(kCtThreads) void k_ct_undistort(const T *__restrict__ raw, float *__restrict__ out, UndParams P) {
    __shared__ float lut_lds[256];
    const float *lut = P.G;
    if (sizeof(T) == 1 && P.mode != kUndFactor) {  // uniform across the block
        for (int i = threadIdx.x; i < 256; i += kCtThreads) lut_lds[i] = P.G[i];
        __syncthreads();
        lut = lut_lds;
    }
    const int idx = blockIdx.x * kCtThreads + threadIdx.x;
    if (idx >= P.n) return;
    if (kPass) {
        out[idx] = und_photometric(P, lut, raw, idx);
        return;
    }
    const float2 m = P.remap[idx];
    float xx = m.x, yy = m.y;
    if (xx < 0) {
        out[idx] = 0;
        return;
    }
    const int xxi = (int)xx, yyi = (int)yy;
    xx -= xxi;
    yy -= yyi;
    const float xxyy = xx * yy;
    const int src = xxi + yyi * P.w_org;
    const float s00 = und_photometric(P, lut, raw, src), s01 = und_photometric(P, lut, raw, src + 1);
    const float s10 = und_photometric(P, lut, raw, src + P.w_org), s11 = und_photometric(P, lut, raw, src + 1 + P.w_org);
    out[idx] = xxyy * s11 + (yy - xxyy) * s10 + (xx - xxyy) * s01 + (1 - xx - yy + xxyy) * s00;
}

}  // namespace
