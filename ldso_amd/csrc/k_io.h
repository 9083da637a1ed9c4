// k_io.h -- results out and images in: k_pack_out, k_reset_oob, k_gather_idepth, the image staging and
// frame store kernels.
#pragma once
#include "ba_device.h"

namespace {

// up to kPackSegs device arrays (4-byte words) and optionally the idepth column of the point
// records into the mapped results buffer, one launch
constexpr int kPackSegs = 8;
struct PackOut {
    const unsigned *src[kPackSegs];
    unsigned *dst[kPackSegs];
    int words[kPackSegs];
    int n_seg;
    const float *pt_data;  // non-null: idepth of every point record into idepth_dst
    float *idepth_dst;
    int n_points;
};
__global__ __launch_bounds__(256) void k_pack_out(PackOut P) {
    const int tid = blockIdx.x * blockDim.x + threadIdx.x, nth = gridDim.x * blockDim.x;
    for (int s = 0; s < P.n_seg; s++)
        for (int e = tid; e < P.words[s]; e += nth) P.dst[s][e] = P.src[s][e];
    if (P.pt_data)
        for (int q = tid; q < P.n_points; q += nth) P.idepth_dst[q] = P.pt_data[(size_t)q * LDSO_BA_POINT_STRIDE + 2];
}
// resetOOB() over a residual range; optionally also the scratch copies of
// ldso_ba_linearize_residuals: centre "not projected" (all-ones NaN) and the flags copied
__global__ __launch_bounds__(256) void k_reset_oob(int8_t *state, int8_t *newstate, float *energy, float *newenergy,
                                                    int n, float *center = nullptr, long long cstride = 0,
                                                    uint8_t *flags = nullptr, const uint8_t *flags_src = nullptr) {
    for (int r = blockIdx.x * blockDim.x + threadIdx.x; r < n; r += gridDim.x * blockDim.x) {
        state[r] = LDSO_BA_RES_IN;
        newstate[r] = LDSO_BA_RES_OUTLIER;
        energy[r] = 0.f;
        newenergy[r] = 0.f;
        if (center) {
            const float q = __uint_as_float(0xFFFFFFFFu);
            for (int k = 0; k < 4; k++) center[k * cstride + r] = q;
            flags[r] = flags_src[r];
        }
    }
}
// idepth of every resident point (point-data column 2), compacted for one small download
__global__ __launch_bounds__(256) void k_gather_idepth(const float *__restrict__ pt_data, float *out, int n) {
    const int q = blockIdx.x * 256 + threadIdx.x;
    if (q < n) out[q] = pt_data[(size_t)q * LDSO_BA_POINT_STRIDE + 2];
}

// image layout 3 (default): the intensity channel only, band-interleaved (band_offset: an 8x4
// pixel tile per 128-byte line, 1/4 of the float4 texel bytes); k_linearize recomputes the
// gradients with makeImages' rule.  That is exact only if the caller's gradients ARE makeImages'
// (FrameHessian.cc:96-101): every pixel the taps can reach (x in [1, w-2], y in [1, h-2]) is
// checked and *mismatch is set if not (the context then falls back to layout 1).
__global__ void k_intensity_image(const float *__restrict__ src, float *dst, int w, int h, int tpr8, int hp,
                                  int *mismatch) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    const int wp = tpr8 * 8;
    if (i >= wp * hp) return;
    const int x = i % wp, y = i / wp;
    float v = 0.f;
    if (x < w && y < h) {
        const float *p = src + 3 * ((size_t)y * w + x);
        v = p[0];
        if (x >= 1 && x <= w - 2 && y >= 1 && y <= h - 2) {
            const float dx = make_grad(p[3], p[-3]), dy = make_grad(p[3 * w], p[-3 * w]);
            if (__float_as_uint(dx) != __float_as_uint(p[1]) || __float_as_uint(dy) != __float_as_uint(p[2]))
                atomicOr(mismatch, 1);
        }
    }
    dst[band_offset(x, y, (unsigned)wp * 16u) >> 2] = v;
}

// image layout 1: FrameHessian::dI (AoS [I, dx, dy]) -> [I, dx, dy, 0] texels in 2x4 tiles
__global__ void k_tile_image(const float *__restrict__ src, float4 *dst, int w, int h, int tpr2, int hp) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    const int wp = tpr2 * 2;
    if (i >= wp * hp) return;
    const int x = i % wp, y = i / wp;
    float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
    if (x < w && y < h) {
        const float *p = src + 3 * ((size_t)y * w + x);
        v = make_float4(p[0], p[1], p[2], 0.f);
    }
    dst[(((y >> 2) * tpr2 + (x >> 1)) << 3) + ((y & 3) << 1) + (x & 1)] = v;
}

// Frame store ingest from device memory (ldso_ba_frame_put_device / _tracker).  Both kernels write
// the whole slot, the padding (x >= w, y >= h) as zero, exactly as the two kernels above leave it.
// Layout 3: thread per (x, 4-row band): four row-coalesced 4-byte loads from the intensity plane and
// the band's 16 bytes of column x in one store (float4 index band * wp + x: a wavefront writes 1 KiB
// per instruction).  No gradient check: the caller's contract is that the frame's gradients are
// makeImages'.
__global__ __launch_bounds__(256) void k_ingest_intensity(const float *__restrict__ src, float4 *dst, int w, int h, int wp,
                                                           int hp) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= wp * (hp >> 2)) return;
    const int x = i % wp, y0 = (i / wp) << 2;
    float v[4] = {0.f, 0.f, 0.f, 0.f};
    if (x < w)
        for (int r = 0; r < 4; r++)
            if (y0 + r < h) v[r] = src[(size_t)(y0 + r) * w + x];
    dst[i] = make_float4(v[0], v[1], v[2], v[3]);
}
// Layout 1: thread per destination texel of the 2x4 tiles (consecutive threads, consecutive
// texels): [I, dx, dy, absSquaredGrad] -> [I, dx, dy, 0]
__global__ __launch_bounds__(256) void k_ingest_texels(const float4 *__restrict__ src, float4 *dst, int w, int h,
                                                        int tpr2, int hp) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= tpr2 * 2 * hp) return;
    const int tile = i >> 3, x = ((tile % tpr2) << 1) + (i & 1), y = ((tile / tpr2) << 2) + ((i >> 1) & 3);
    float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
    if (x < w && y < h) {
        v = src[(size_t)y * w + x];
        v.w = 0.f;
    }
    dst[i] = v;
}
// ldso_ba_frame_get: a slot back to row-major planes, intensity [h*w] and (layout 1) grad [h*w][2]
__global__ __launch_bounds__(256) void k_slot_unpack(const float4 *__restrict__ slot, int mode, float *inten, float *grad,
                                                      int w, int h, int tpr) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= w * h) return;
    const int x = i % w, y = i / w;
    if (mode == 3) {
        inten[i] = reinterpret_cast<const float *>(slot)[band_offset(x, y, (unsigned)tpr * 8u * 16u) >> 2];
    } else {
        const float4 v = slot[(((y >> 2) * tpr + (x >> 1)) << 3) + ((y & 3) << 1) + (x & 1)];
        inten[i] = v.x;
        grad[2 * (size_t)i] = v.y;
        grad[2 * (size_t)i + 1] = v.z;
    }
}

}  // namespace
