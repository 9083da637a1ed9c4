// k_ct_pyramid.h -- the new frame's pyramid (FrameHessian::makeImages, FrameHessian.cc:59-115), and the
// constants every tracker kernel header shares.  Per new frame, two launches:
//   k_ct_pyr_down   block per T x T level-0 tile (T = 2^(levels-1)): the tile's intensities go to
//                   LDS once and every coarser level of that tile is averaged there
//                   (0.25f * (((a + b) + c) + d), the reference's order), so one pass over the
//                   level-0 image builds the whole intensity pyramid.
//   k_ct_pyr_grad   thread per pixel of every level: central differences on the flattened index
//                   (rows 0 and h-1 zero, x = 0 / w-1 read across the row boundary exactly as the
//                   reference's idx +- 1 does), NaN / |d| > 255 -> 0, absSquaredGrad with the optional
//                   response-gradient weight; written as one float4 texel [I, dx, dy, |g|^2].
//
// This header, the other k_ct_*.h and ct_context.h are pieces of the one translation unit ldso_ct.hip
// (anonymous namespace), not headers for general inclusion.
#pragma once
#include <hip/hip_runtime.h>

#include "../../include/ldso_ct.h"
#include "ldso_ba_internal.h"

#pragma clang fp contract(off)

namespace {

constexpr int kWave = 64;
constexpr int kCtThreads = 256;
constexpr float kHuberTH = ldso_ba::kHuberTH;  // setting_huberTH, Setting.cc:76

struct PyrParams {
    int w, h, levels, tile;                  // tile = 2^(levels-1) level-0 pixels
    int wl[LDSO_CT_MAX_LEVELS], hl[LDSO_CT_MAX_LEVELS];
    int off[LDSO_CT_MAX_LEVELS + 1];         // pixel offset of each level in the flat buffers
};

// ---------------------------------------------------------------------------------------------
// k_ct_pyr_down: levels 0..L-1 intensities of one T x T level-0 tile (FrameHessian.cc:73-92)
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kCtThreads) void k_ct_pyr_down(const float *__restrict__ color, float *__restrict__ inten,
                                                            PyrParams P) {
    extern __shared__ float tile_lds[];  // [T*T] + [(T/2)*(T/2)]
    const int T = P.tile, tx0 = blockIdx.x * T, ty0 = blockIdx.y * T;
    float *A = tile_lds, *B = tile_lds + T * T;
    for (int i = threadIdx.x; i < T * T; i += kCtThreads) {
        const int x = tx0 + (i % T), y = ty0 + (i / T);
        const float v = color[(size_t)y * P.w + x];
        A[i] = v;
        inten[(size_t)y * P.w + x] = v;
    }
    __syncthreads();
    float *src = A, *dst = B;
    for (int l = 1; l < P.levels; l++) {
        const int Ts = T >> (l - 1), Td = T >> l;  // source / destination tile sides
        for (int i = threadIdx.x; i < Td * Td; i += kCtThreads) {
            const int x = i % Td, y = i / Td;
            const float *s = src + 2 * y * Ts + 2 * x;
            const float v = 0.25f * (s[0] + s[1] + s[Ts] + s[Ts + 1]);
            dst[i] = v;
            inten[P.off[l] + (size_t)(blockIdx.y * Td + y) * P.wl[l] + blockIdx.x * Td + x] = v;
        }
        __syncthreads();
        float *t = src;
        src = dst;
        dst = t;
    }
}

// ---------------------------------------------------------------------------------------------
// k_ct_pyr_grad: gradients and absSquaredGrad of every level (FrameHessian.cc:94-114)
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kCtThreads) void k_ct_pyr_grad(const float *__restrict__ inten, float4 *__restrict__ dIp,
                                                            const float *__restrict__ Bresp, PyrParams P) {
    const int g = blockIdx.x * kCtThreads + threadIdx.x;
    if (g >= P.off[P.levels]) return;
    int l = 0;
    while (g >= P.off[l + 1]) l++;
    const int wl = P.wl[l], hl = P.hl[l], idx = g - P.off[l];
    const float *I = inten + P.off[l];
    const float c = I[idx];
    float dx = 0, dy = 0, a = 0;
    if (idx >= wl && idx < wl * (hl - 1)) {
        dx = 0.5f * (I[idx + 1] - I[idx - 1]);
        dy = 0.5f * (I[idx + wl] - I[idx - wl]);
        if (isnan(dx) || fabsf(dx) > 255.0f) dx = 0;
        if (isnan(dy) || fabsf(dy) > 255.0f) dy = 0;
        a = dx * dx + dy * dy;
        if (Bresp) {  // CalibHessian::getBGradOnly (CalibHessian.h:102-111)
            int ci = c + 0.5f;
            if (ci < 5) ci = 5;
            if (ci > 250) ci = 250;
            const float gw = Bresp[ci + 1] - Bresp[ci];
            a *= gw * gw;
        }
    }
    dIp[g] = make_float4(c, dx, dy, a);
}

}  // namespace
