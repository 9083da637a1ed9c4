// ba_device.h -- what more than one kernel stage (k_*.h) of the ldso_ba.hip unit uses: the window
// descriptor, the image taps, the centre geometry of a residual record, the wave helpers, the
// packed-triangle and Top-slot indices, the sumNID chain and the setNewFrameEnergyTH selection.
#pragma once
#include <hip/hip_runtime.h>

#include "../../include/ldso_ba.h"
#include "layout.h"
#include "ldso_ba_internal.h"

// This header, the k_*.h stage headers, ba_context.h and ba_launch.h are pieces of the one translation
// unit ldso_ba.hip (anonymous namespace, the using-directive below), not headers for general inclusion.
using namespace ldso_ba;

namespace {

constexpr int kWave = 64;
constexpr int kTopVals = 96;    // 55 + 30 + 6 AccumulatorApprox entries, padded to 96

// Per-window device descriptor: the fields of layout.h's WinDesc under the name (and in the
// namespace) the kernels' symbols have always carried.
struct WinDev : WinDesc {};
static_assert(sizeof(WinDev) == sizeof(WinDesc), "WinDev adds nothing to WinDesc");
static_assert(sizeof(Item4) == sizeof(int4) && alignof(Item4) == alignof(int4) && sizeof(Item2) == sizeof(int2),
              "layout.h's work items are the kernels' int4 / int2");

__device__ __forceinline__ void wave_lds_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

struct Geo {
    float Ku, Kv, new_idepth;
    float d_xi_x[6], d_xi_y[6], d_C_x[4], d_C_y[4], d_d_x, d_d_y;
};

// projectPoint (full form), ResidualProjections.h:57-84 + Residuals.cc:69-106
__device__ inline bool centre_projection(const float *__restrict__ pre, float u, float v, float idz,
                                         float fxl, float fyl, float cxl, float cyl, float wM3, float hM3,
                                         Geo &g) {
#pragma clang fp contract(off)
    const float fxli = 1.0f / fxl, fyli = 1.0f / fyl;
    const float *R0 = pre + 12, *t0 = pre + 21;
    const float K0 = (u + 0 - cxl) * fxli, K1 = (v + 0 - cyl) * fyli;
    float ptp[3];
#pragma unroll
    for (int i = 0; i < 3; i++) ptp[i] = (R0[3 * i] * K0 + R0[3 * i + 1] * K1 + R0[3 * i + 2] * 1.0f) + t0[i] * idz;
    const float drescale = 1.0f / ptp[2];
    g.new_idepth = idz * drescale;
    if (!(drescale > 0)) return false;
    const float uu = ptp[0] * drescale, vv = ptp[1] * drescale;
    g.Ku = uu * fxl + cxl;
    g.Kv = vv * fyl + cyl;
    if (!(g.Ku > 1.1f && g.Kv > 1.1f && g.Ku < wM3 && g.Kv < hM3)) return false;
    g.d_d_x = drescale * (t0[0] - t0[2] * uu) * kScaleIdepth * fxl;
    g.d_d_y = drescale * (t0[1] - t0[2] * vv) * kScaleIdepth * fyl;
    g.d_C_x[2] = drescale * (R0[6] * uu - R0[0]);
    g.d_C_x[3] = fxl * drescale * (R0[7] * uu - R0[1]) * fyli;
    g.d_C_x[0] = K0 * g.d_C_x[2];
    g.d_C_x[1] = K1 * g.d_C_x[3];
    g.d_C_y[2] = fyl * drescale * (R0[6] * vv - R0[3]) * fxli;
    g.d_C_y[3] = drescale * (R0[7] * vv - R0[4]);
    g.d_C_y[0] = K0 * g.d_C_y[2];
    g.d_C_y[1] = K1 * g.d_C_y[3];
    g.d_C_x[0] = (g.d_C_x[0] + uu) * kScaleF;
    g.d_C_x[1] *= kScaleF;
    g.d_C_x[2] = (g.d_C_x[2] + 1) * kScaleC;
    g.d_C_x[3] *= kScaleC;
    g.d_C_y[0] *= kScaleF;
    g.d_C_y[1] = (g.d_C_y[1] + vv) * kScaleF;
    g.d_C_y[2] *= kScaleC;
    g.d_C_y[3] = (g.d_C_y[3] + 1) * kScaleC;
    const float ni = g.new_idepth;
    g.d_xi_x[0] = ni * fxl;
    g.d_xi_x[1] = 0;
    g.d_xi_x[2] = -ni * uu * fxl;
    g.d_xi_x[3] = -uu * vv * fxl;
    g.d_xi_x[4] = (1 + uu * uu) * fxl;
    g.d_xi_x[5] = -vv * fxl;
    g.d_xi_y[0] = 0;
    g.d_xi_y[1] = ni * fyl;
    g.d_xi_y[2] = -ni * vv * fyl;
    g.d_xi_y[3] = -(1 + vv * vv) * fyl;
    g.d_xi_y[4] = uu * vv * fyl;
    g.d_xi_y[5] = uu * fyl;
    return true;
}

constexpr int kGeoSnap = 16;  // floats per pair: R0 [0..8], t0 [9..11], calib fxl, fyl, cxl, cyl [12..15]
// JpJdF[0..5] of a record from its centre geometry: point_terms' statements
__device__ __forceinline__ void record_jp6(const Geo &g, float j0, float j1, float jp[6]) {
#pragma clang fp contract(off)
#pragma unroll
    for (int i = 0; i < 6; i++) jp[i] = g.d_xi_x[i] * j0 + g.d_xi_y[i] * j1;
}

// Image layout 1 texel fetch: FrameHessian::dI texels [I, dx, dy, 0] (16 B) tiled 2 (x) by 4 (y)
// per 128-byte line.  Used when the caller's gradients are not makeImages' (layout 3 would then
// not reproduce them) and by k_activate on such frames.
__device__ inline float3 tex(const float4 *__restrict__ img, int tpr2, int x, int y) {
    const float4 v = img[(((y >> 2) * tpr2 + (x >> 1)) << 3) + ((y & 3) << 1) + (x & 1)];
    return make_float3(v.x, v.y, v.z);
}

// Image layout 3 (default): the intensity channel only, in bands of 4 rows stored column by
// column, i.e. byte offset (y >> 2) * band + 16 x + 4 (y & 3) with band = 16 * padded width.
// A 128-byte line is an 8 x 4 pixel tile, and the four taps of one row of a pixel's
// neighbourhood are 16 B apart, so one row offset serves all of them (immediate offsets).
__device__ __forceinline__ unsigned band_offset(int x, int y, unsigned band) {
    return ((unsigned)y >> 2) * band + ((unsigned)x << 4) + (((unsigned)y & 3u) << 2);
}
__device__ __forceinline__ float ldb(__amdgpu_buffer_rsrc_t r, unsigned off) {
    return __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(r, (int)off, 0, 0));
}
__device__ __forceinline__ __amdgpu_buffer_rsrc_t frame_rsrc(const float *base, long long bytes) {
    return __builtin_amdgcn_make_buffer_rsrc(const_cast<float *>(base), (short)0, (int)bytes, 0x00020000);
}

// makeImages' gradient rule (FrameHessian.cc:96-101): 0.5 (a - b), zeroed when NaN or |d| > 255
// (one compare: NaN fails it too)
__device__ __forceinline__ float make_grad(float a, float b) {
#pragma clang fp contract(off)
    const float d = 0.5f * (a - b);
    return fabsf(d) <= 255.0f ? d : 0.0f;
}

// The 12 intensities a bilinear [I, dx, dy] sample at (ix + dx, iy + dy) needs, layout 3:
// rows iy-1 (ix, ix+1), iy and iy+1 (ix-1 .. ix+2), iy+2 (ix, ix+1).
__device__ __forceinline__ void load12(__amdgpu_buffer_rsrc_t r, unsigned band, int ix, int iy, float *iv) {
    const unsigned o0 = band_offset(ix - 1, iy - 1, band), o1 = band_offset(ix - 1, iy, band),
                   o2 = band_offset(ix - 1, iy + 1, band), o3 = band_offset(ix - 1, iy + 2, band);
    iv[0] = ldb(r, o0 + 16);
    iv[1] = ldb(r, o0 + 32);
    iv[2] = ldb(r, o1);
    iv[3] = ldb(r, o1 + 16);
    iv[4] = ldb(r, o1 + 32);
    iv[5] = ldb(r, o1 + 48);
    iv[6] = ldb(r, o2);
    iv[7] = ldb(r, o2 + 16);
    iv[8] = ldb(r, o2 + 32);
    iv[9] = ldb(r, o2 + 48);
    iv[10] = ldb(r, o3 + 16);
    iv[11] = ldb(r, o3 + 32);
}
// getInterpolatedElement33 (GlobalFuncs.h:89-103) from those 12 values with the gradients
// recomputed; bit-identical to sampling the caller's dI when dI's gradients are makeImages'.
__device__ __forceinline__ float3 bilin12(const float *v, float dx, float dy) {
#pragma clang fp contract(off)
    const float dxdy = dx * dy;
    const float w11 = dxdy, w01 = dy - dxdy, w10 = dx - dxdy, w00 = 1 - dx - dy + dxdy;
    const float3 t00 = make_float3(v[3], make_grad(v[4], v[2]), make_grad(v[7], v[0]));
    const float3 t10 = make_float3(v[4], make_grad(v[5], v[3]), make_grad(v[8], v[1]));
    const float3 t01 = make_float3(v[7], make_grad(v[8], v[6]), make_grad(v[10], v[3]));
    const float3 t11 = make_float3(v[8], make_grad(v[9], v[7]), make_grad(v[11], v[4]));
    return make_float3(w11 * t11.x + w01 * t01.x + w10 * t10.x + w00 * t00.x,
                       w11 * t11.y + w01 * t01.y + w10 * t10.y + w00 * t00.y,
                       w11 * t11.z + w01 * t01.z + w10 * t10.z + w00 * t00.z);
}

// slot (r, c) of the 13x13 finish() matrix -> index into the 96-slot partial layout
__device__ __forceinline__ int top_slot(int r, int c) {
    if (r > c) {
        const int t = r;
        r = c;
        c = t;
    }
    if (c < 10) return r * 10 - r * (r - 1) / 2 + (c - r);  // Data[] (upper row-major)
    if (r < 10) return 55 + 3 * r + (c - 10);                // TopRight
    const int a = r - 10, b = c - 10;                        // BotRight
    return 85 + (a == 0 ? b : a == 1 ? 2 + b : 5);
}

__device__ __forceinline__ long long pk_index(int row, int col, int D) {  // row <= col
    return (long long)row * D - (long long)row * (row - 1) / 2 + (col - row);
}

__device__ __forceinline__ double readlane_f64(double v, int l) {
    const unsigned long long u = __double_as_longlong(v);
    const unsigned lo = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)u, l);
    const unsigned hi = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)(u >> 32), l);
    return __longlong_as_double((long long)(((unsigned long long)hi << 32) | lo));
}
// |v| as an order-preserving key; NaN never wins (the host's '>' never selects one)
__device__ __forceinline__ unsigned long long abs_key(double v) {
    const double a = fabs(v);
    return a == a ? (unsigned long long)__double_as_longlong(a) : 0ull;
}

// doStepFromBackup's sumNID and numID (FullSystem.cc:1899-1909) for the step that follows this
// pass: the float sum of fabsf(idepth_backup) over the window's points in frames -> features order
// (host frames in window order, each host's points in the caller's order: the device point order),
// i.e. over the idepths this pass linearised at.  The chain of float adds is sequential by
// definition, so one lane walks it from LDS (the block stages chunks of the idepths), in a block of
// its own beside other work: extra blocks of k_solve_fast (the default), of k_point_sc (exact solve
// modes), or, with points sharded over ranks, over the exchange's gathered runs (NidSrc).
// The idepths of one window's chain: its own points (pt_data), or, with points sharded over ranks,
// every rank's run of |idepth| from the exchange's all-gather, concatenated in rank order -- the
// runs are contiguous pieces of the host-frame order, so the concatenation is the unsharded order
// and the chain is bit for bit the single-GPU one (runs zero-padded to prun: + 0 leaves s as is).
struct NidSrc {
    const float *pt_data;   // [points][LDSO_BA_POINT_STRIDE], idepth at + 2
    const float *gathered;  // non-null: [rank][window][slot] exchange slots, the run at + off
    long long slot, off;
    int n_ranks, n_win, prun;
};
__device__ void nid_chain(const WinDev &W, const NidSrc &src, double *win_nid, int w, float *lds, int chunk) {
    const int n = src.gathered ? src.n_ranks * src.prun : W.P, tid = threadIdx.x;
    const float *pd = src.pt_data + (size_t)W.point_base * LDSO_BA_POINT_STRIDE + 2;
    auto value = [&](int i) {
        if (!src.gathered) return fabsf(pd[(size_t)i * LDSO_BA_POINT_STRIDE]);
        const int r = i / src.prun, q = i - r * src.prun;
        return src.gathered[((size_t)r * src.n_win + w) * src.slot + src.off + q];
    };
    float s = 0.0f;
    for (int q0 = 0; q0 < n; q0 += chunk) {
        const int m = min(chunk, n - q0);
        for (int i = tid; i < m; i += blockDim.x) lds[i] = value(q0 + i);
        for (int i = m + tid; i < ((m + 3) & ~3); i += blockDim.x) lds[i] = 0.0f;  // +0 leaves s unchanged
        __syncthreads();
        if (tid == 0) {
            const float4 *l4 = reinterpret_cast<const float4 *>(lds);
#pragma unroll 8
            for (int i = 0; i < (m + 3) / 4; i++) {
                const float4 v = l4[i];
                s += v.x;
                s += v.y;
                s += v.z;
                s += v.w;
            }
        }
        __syncthreads();
    }
    if (tid == 0) {
        win_nid[2 * w] = (double)s;  // exact; read back as float
        win_nid[2 * w + 1] = (double)(float)W.p_all;  // numID++ per point (float): exact below 2^24
    }
}

constexpr int kStThreads = 256;
// setNewFrameEnergyTH (FullSystem.cc:2078-2109) as an exact 4-pass radix select with
// nth_element semantics over the candidates get(i), i in [0, n_cand), that are >= 0.
// Candidates are staged in LDS when they fit; larger sets are re-read from global memory.
// Every thread of the block must call it; thread 0 writes *th_out.
// LDS behind the candidate keys: a 256-bin histogram per wave, 16 words of shared scalars, and
// two doubles per wave for the energy sum
__host__ __device__ constexpr size_t th_fixed_bytes(int threads) {
    return ((size_t)(threads / 64) * 256 + 16) * sizeof(unsigned) + (size_t)(threads / 64) * 2 * sizeof(double);
}
template <int kT, class Get>
__device__ void select_frame_th(Get get, int n_cand, unsigned *keys, int cap, float *th_out) {
    // LDS: keys[cap] | hist[kW waves][256] | sh[16]
    constexpr int kW = kT / 64;
    unsigned *hist = keys + cap;
    unsigned *sh = hist + kW * 256;  // [0..kW) per-wave valid counts, [kW] prefix, [kW+1] rank
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    const bool in_lds = n_cand <= cap;
    // stage every candidate at its own index (no compaction, so no dependent slot atomics):
    // an invalid one (NewEnergyWithOutlier < 0) becomes 0xFFFFFFFF, above every valid key, and
    // is never selected because the rank is taken among the valid ones only
    constexpr int kU = 8;
    unsigned cnt = 0;
    for (int i0 = 0; i0 < n_cand; i0 += kT * kU) {
        float x[kU];
#pragma unroll
        for (int u = 0; u < kU; u++) x[u] = get(min(i0 + u * kT + tid, n_cand - 1));  // loads in flight
#pragma unroll
        for (int u = 0; u < kU; u++) {
            const int idx = i0 + u * kT + tid;
            const bool ok = idx < n_cand && x[u] >= 0;
            cnt += ok ? 1u : 0u;
            if (in_lds && idx < n_cand) keys[idx] = ok ? (__float_as_uint(x[u]) & 0x7FFFFFFFu) : 0xFFFFFFFFu;
        }
    }
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) cnt += __shfl_xor(cnt, m, kWave);
    if (lane == 0) sh[wid] = cnt;
    __syncthreads();
    unsigned n = 0;
#pragma unroll
    for (int q = 0; q < kW; q++) n += sh[q];
    if (n == 0) {
        if (tid == 0) *th_out = 12 * 12 * LDSO_BA_PATTERN_NUM;
        __syncthreads();
        return;
    }
    unsigned prefix = 0, rank = (unsigned)(int)(kFrameEnergyTHN * (float)n);  // int nthIdx = 0.7f * size()
    unsigned *wh = hist + 256 * wid;  // per-wave sub-histogram: 4x less same-address contention
    for (int pass = 0; pass < 4; pass++) {
        const int shift = 24 - 8 * pass;
        const unsigned pmask = pass == 0 ? 0u : (0xFFFFFFFFu << (32 - 8 * pass));
        for (int b = lane; b < 256; b += 64) wh[b] = 0;
        __syncthreads();
        if (in_lds) {
            for (int i = tid; i < n_cand; i += kT) {
                const unsigned key = keys[i];
                if ((key & pmask) == (prefix & pmask)) atomicAdd(&wh[(key >> shift) & 255u], 1u);
            }
        } else {
            for (int i = tid; i < n_cand; i += kT) {
                const float x = get(i);
                const unsigned key = x >= 0 ? (__float_as_uint(x) & 0x7FFFFFFFu) : 0xFFFFFFFFu;
                if ((key & pmask) == (prefix & pmask)) atomicAdd(&wh[(key >> shift) & 255u], 1u);
            }
        }
        __syncthreads();
        if (tid < 64) {  // one wave: lane l owns bins 4l..4l+3
            unsigned hb[4];
#pragma unroll
            for (int q = 0; q < 4; q++) {
                hb[q] = 0;
#pragma unroll
                for (int v = 0; v < kW; v++) hb[q] += hist[256 * v + 4 * tid + q];
            }
            unsigned incl = hb[0] + hb[1] + hb[2] + hb[3];
#pragma unroll
            for (int m = 1; m < 64; m <<= 1) {
                const unsigned y = __shfl_up(incl, m, kWave);
                if (tid >= m) incl += y;
            }
            const unsigned long long hit = __ballot(incl > rank);
            const int first = __ffsll((long long)hit) - 1;
            if (tid == first) {
                unsigned acc = incl - (hb[0] + hb[1] + hb[2] + hb[3]);
                int d = 4 * tid;
                for (int q = 0; q < 4; q++, d++) {
                    if (acc + hb[q] > rank) break;
                    acc += hb[q];
                }
                sh[kW + 1] = rank - acc;
                sh[kW] = prefix | ((unsigned)d << shift);
            }
        }
        __syncthreads();
        prefix = sh[kW];
        rank = sh[kW + 1];
    }
    if (tid == 0) {
#pragma clang fp contract(off)
        const float nth = sqrtf(__uint_as_float(prefix));
        float v = nth * kFrameEnergyTHFacMedian;
        v = 26.0f * kFrameEnergyTHConstWeight + v * (1 - kFrameEnergyTHConstWeight);
        v = v * v;
        v *= kOverallEnergyTHWeight * kOverallEnergyTHWeight;
        *th_out = v;
    }
    __syncthreads();
}

}  // namespace
