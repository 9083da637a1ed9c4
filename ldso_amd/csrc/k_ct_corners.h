// k_ct_corners.h -- FeatureDetector::DetectCorners (FeatureDetector.cc:34-130) with ShiTomasiScore and IC_Angle
// (FeatureDetector.h:49-114), ComputeDescriptor (FeatureDetector.cc:132-189) and makeNewTraces' loop for
// setting_pointSelection == 1 (FullSystem.cc:1428-1438), on level 0 of the resident pyramid.  What the
// reference does sequentially is order-free but for the output order and the float chains:
//   k_ct_cor_cell      workgroup per grid cell (gx outer, gy inner): maxGrad as an LDS integer max over the
//                      bits of the positive gradients (only `>` decides, a NaN never wins); a lane per
//                      candidate runs ShiTomasiScore's three sequential 64-tap chains; maxScore the same way
//                      (an LDS max, then one global integer max per cell); the picks are the k largest keys
//                      (score descending, candidate order ascending, a non-finite score after every number):
//                      a k-fold LDS max over (ordered score bits, reversed candidate index), k_ct_sel_block's
//                      first-maximum keys again.  A stable sort's first k elements are exactly these.
//   k_ct_sel_scan      (k_ct_select.h) exclusive prefix of the cells' pick counts: the feature order is cell
//                      order, then rank
//   k_ct_cor_emit      thread per (cell, rank): the feature's (x, y, score), its corner candidacy
//                      (score > 0.01 maxScore) and its immature record (ip_make_record, type 1)
//   k_ct_cor_suppress  thread per feature.  The reference's double loop never reads the flag it clears, so
//                      candidate i survives iff for every other candidate j with dx^2 + dy^2 < 25:
//                      s_i > s_j when i < j, and not s_j > s_i when j < i.  The neighbours come from the grid
//                      cells within 4 pixels, through the cells' offsets.
//   k_ct_cor_orb       wavefront per feature: a corner's 31 x 31 intensity patch goes to LDS once; lane 0 runs
//                      m_10's sequential chain, lanes 1-15 the v_sum chain of their row pair, m_01 is summed in
//                      row order; the angle is atan2 in double rounded once; the 256 comparisons of the
//                      descriptor are 4 per lane, read from the patch, and a ballot is 8 descriptor bytes.
// No float atomics anywhere; f32 denormals are kept (the gfx950 default); no contraction.
#pragma once
#include <float.h>
#include <math.h>

#include "k_ct_pyramid.h"
#include "k_ct_immature.h"
#include "ct_lm.h"

#pragma clang fp contract(off)

namespace {

constexpr int kCorHalfPatch = 15;                  // HALF_PATCH_SIZE, FeatureDetector.h:20
constexpr int kCorPatchSide = 2 * kCorHalfPatch + 1;
constexpr int kCorPatternRange = 13;               // |entry| of the ORB sampling table
constexpr int kCorMaxGrid = 2 * kCorHalfPatch;     // gridsize above it: the last cells touch the border
constexpr int kCorWavesPerBlock = kCtThreads / kWave;
// the counters of a call on the device
enum : int { kCorCntFeatures, kCorCntCandidates, kCorCntCorners, kCorCntMaxScore, kCorCnts = 8 };

struct CorGrid {
    int w, h;
    int g, skip;   // gridsize, cells left out at each border
    int ncx, ncy;  // cells visited per row / column; cell c = (gx - skip) * ncy + (gy - skip)
    int k, kk;     // picks per cell: floor(nfeatInGrid) + 1; min(k, g * g), the slots a cell owns
};
struct CorUmax {
    int u[kCorHalfPatch + 1];  // FeatureDetector::FeatureDetector (FeatureDetector.cc:10-28)
};
struct CorSlot {  // a pick of a cell; then a feature in output order (flag: corner candidate)
    int x, y;
    float score;
    int flag;
};

// float -> int as x86's truncating conversion does it (undefined in C++ outside int's range): a value that
// is not finite or does not fit becomes INT_MIN
__device__ __forceinline__ int cor_to_int(float f) {
    return (f >= -2147483648.f && f < 2147483648.f) ? (int)f : INT_MIN;
}

// ShiTomasiScore (FeatureDetector.h:49-82), halfbox 4, level 0
__device__ __forceinline__ float cor_score(const float4 *__restrict__ dI0, int w, int h, int u, int v) {
    float dXX = 0, dYY = 0, dXY = 0;
    const int x_min = u - 4, x_max = u + 4, y_min = v - 4, y_max = v + 4;
    if (x_min < 1 || x_max >= w - 1 || y_min < 1 || y_max >= h - 1) return 0;
    for (int y = y_min; y < y_max; ++y)
        for (int x = x_min; x < x_max; ++x) {
            const float4 t = dI0[(size_t)y * w + x];
            const float dx = t.y, dy = t.z;
            dXX += dx * dx;
            dYY += dy * dy;
            dXY += dx * dy;
        }
    dXX = (float)((double)dXX / (2.0 * 64));
    dYY = (float)((double)dYY / (2.0 * 64));
    dXY = (float)((double)dXY / (2.0 * 64));
    // sqrt's float overload: NumTypes.h:12 has a global `using namespace std`
    const float r = dXX + dYY - sqrtf((dXX + dYY) * (dXX + dYY) - 4 * (dXX * dYY - dXY * dXY));
    return (float)(0.5 * (double)r);
}

// larger score first, then the earlier candidate; a score that is not finite after every number.
// Never 0: e < g * g <= 900.
__device__ __forceinline__ unsigned long long cor_key(float s, unsigned e) {
    unsigned b = 0;
    if (isfinite(s)) {
        b = s == 0 ? 0u : __float_as_uint(s);           // -0 ties with +0
        b = (b & 0x80000000u) ? ~b : (b | 0x80000000u);  // ordered as unsigned; above 0 for every number
    }
    return ((unsigned long long)b << 32) | (unsigned)~e;
}

__global__ __launch_bounds__(kCtThreads) void k_ct_cor_cell(const float4 *__restrict__ dI0, CorGrid G,
                                                            int *__restrict__ cell_cnt, int *__restrict__ cell_off,
                                                            CorSlot *__restrict__ slot, int *__restrict__ cnt) {
    extern __shared__ unsigned long long cor_keys[];  // [g*g] keys, then [g*g] scores
    __shared__ int s_max_grad, s_max_score, s_ncand;
    __shared__ unsigned long long s_best;
    const int g = G.g, gg = g * g, tid = threadIdx.x, c = blockIdx.x;
    float *scores = reinterpret_cast<float *>(cor_keys + gg);
    const int x0 = (G.skip + c / G.ncy) * g, y0 = (G.skip + c % G.ncy) * g;
    if (tid == 0) {
        s_max_grad = 0;
        s_max_score = 0;
        s_ncand = 0;
    }
    __syncthreads();
    // candidate order e: x outer, y inner (FeatureDetector.cc:62-63)
    for (int e = tid; e < gg; e += blockDim.x) {
        const float a = dI0[(size_t)(y0 + e % g) * G.w + x0 + e / g].w;
        if (a > 0) atomicMax(&s_max_grad, __float_as_int(a));
    }
    __syncthreads();
    const float maxGrad = __int_as_float(s_max_grad);
    const float gradTH = (float)((0.5 * maxGrad) > 5 ? 0.5 * maxGrad : 5);
    for (int e = tid; e < gg; e += blockDim.x) {
        const int x = x0 + e / g, y = y0 + e % g;
        unsigned long long key = 0;
        float s = 0;
        if (dI0[(size_t)y * G.w + x].w > gradTH) {
            s = cor_score(dI0, G.w, G.h, x, y);
            key = cor_key(s, (unsigned)e);
            atomicAdd(&s_ncand, 1);
            if (s > 0) atomicMax(&s_max_score, __float_as_int(s));
        }
        cor_keys[e] = key;
        scores[e] = s;
    }
    __syncthreads();
    const int picks = min(s_ncand, G.k);
    unsigned long long prev = ~0ull;
    for (int r = 0; r < picks; r++) {
        if (tid == 0) s_best = 0;
        __syncthreads();
        unsigned long long best = 0;
        for (int e = tid; e < gg; e += blockDim.x) {
            const unsigned long long key = cor_keys[e];
            if (key < prev && key > best) best = key;
        }
        if (best) atomicMax(&s_best, best);
        __syncthreads();
        prev = s_best;
        if (tid == 0) {
            const int e = (int)~(unsigned)prev;
            slot[(size_t)c * G.kk + r] = CorSlot{x0 + e / g, y0 + e % g, scores[e], 0};
        }
        __syncthreads();
    }
    if (tid == 0) {
        cell_cnt[c] = picks;
        cell_off[c] = picks;
        if (s_ncand) atomicAdd(&cnt[kCorCntCandidates], s_ncand);
        if (s_max_score > 0) atomicMax(&cnt[kCorCntMaxScore], s_max_score);
    }
}

__global__ __launch_bounds__(kCtThreads) void k_ct_cor_emit(const float4 *__restrict__ dI0, CorGrid G, int n_slots,
                                                            const int *__restrict__ cell_cnt,
                                                            const int *__restrict__ cell_off,
                                                            const CorSlot *__restrict__ slot,
                                                            const int *__restrict__ cnt, int host,
                                                            CorSlot *__restrict__ feat, IpRec *__restrict__ rec,
                                                            int capacity) {
    const int k = blockIdx.x * kCtThreads + threadIdx.x;
    if (k >= n_slots) return;
    const int c = k / G.kk, r = k - c * G.kk;
    if (r >= cell_cnt[c]) return;
    const int i = cell_off[c] + r;
    CorSlot f = slot[k];
    const float scoreTH = (float)(0.01 * (double)__int_as_float(cnt[kCorCntMaxScore]));
    f.flag = f.score > scoreTH ? 1 : 0;
    feat[i] = f;
    if (i < capacity) rec[i] = ip_make_record(dI0, G.w, G.h, (float)f.x, (float)f.y, 1.0f, host);
}

__global__ __launch_bounds__(kCtThreads) void k_ct_cor_suppress(CorGrid G, const int *__restrict__ cell_cnt,
                                                                const int *__restrict__ cell_off,
                                                                const CorSlot *__restrict__ feat,
                                                                int *__restrict__ is_corner, int *__restrict__ cnt) {
    const int i = blockIdx.x * kCtThreads + threadIdx.x;
    bool alive = false;
    if (i < cnt[kCorCntFeatures]) {
        const CorSlot f = feat[i];
        alive = f.flag != 0;
        if (alive) {
            const int cx = f.x / G.g - G.skip, cy = f.y / G.g - G.skip, reach = (4 + G.g - 1) / G.g;
            for (int ox = max(cx - reach, 0); ox <= min(cx + reach, G.ncx - 1); ox++)
                for (int oy = max(cy - reach, 0); oy <= min(cy + reach, G.ncy - 1); oy++) {
                    const int c2 = ox * G.ncy + oy, j0 = cell_off[c2], j1 = j0 + cell_cnt[c2];
                    for (int j = j0; j < j1; j++) {
                        const CorSlot q = feat[j];
                        const int dx = q.x - f.x, dy = q.y - f.y;
                        if (j == i || !q.flag || dx * dx + dy * dy >= 25) continue;
                        if (i < j ? !(f.score > q.score) : q.score > f.score) alive = false;
                    }
                }
        }
        is_corner[i] = alive ? 1 : 0;
    }
    const unsigned long long m = __ballot(alive);
    if ((threadIdx.x & (kWave - 1)) == 0 && m) atomicAdd(&cnt[kCorCntCorners], __popcll(m));
}

// IC_Angle and ComputeDescriptor of one feature per wave; the counters go to the host with the first wave
__global__ __launch_bounds__(kCtThreads) void k_ct_cor_orb(const float4 *__restrict__ dI0, int w, int h,
                                                           const CorSlot *__restrict__ feat,
                                                           const int *__restrict__ is_corner,
                                                           const int4 *__restrict__ pattern, CorUmax U,
                                                           const int *__restrict__ cnt, int capacity,
                                                           ldso_ct_feature *__restrict__ out,
                                                           int *__restrict__ counts_host) {
    __shared__ float patch_s[kCorWavesPerBlock][kCorPatchSide * kCorPatchSide];
    const int lane = threadIdx.x & (kWave - 1), wv = threadIdx.x / kWave;
    const int i = blockIdx.x * kCorWavesPerBlock + wv;
    if (blockIdx.x == 0 && threadIdx.x < 4) counts_host[threadIdx.x] = cnt[threadIdx.x];
    if (i >= cnt[kCorCntFeatures] || i >= capacity) return;  // uniform over the wave
    const CorSlot f = feat[i];
    ldso_ct_feature *o = out + i;
    unsigned long long *desc = reinterpret_cast<unsigned long long *>(o->descriptor);
    if (!is_corner[i]) {
        if (lane == 0) {
            o->score = f.score;
            o->angle = 0;
            o->is_corner = 0;
            o->level = 0;
        }
        if (lane < 4) desc[lane] = 0;
        return;
    }
    float *patch = patch_s[wv];
    constexpr int S = kCorPatchSide, H = kCorHalfPatch;
    // the cells keep 16 pixels to every border (ldso_ct.h), so the clamps never act
    for (int k = lane; k < S * S; k += kWave) {
        const int px = min(max(f.x + k % S - H, 0), w - 1), py = min(max(f.y + k / S - H, 0), h - 1);
        patch[k] = dI0[(size_t)py * w + px].x;
    }
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    const float *center = patch + H * S + H;
    float m_10 = 0, v_sum = 0;
    if (lane == 0) {
        for (int u = -H; u <= H; ++u) m_10 += u * center[u];
        for (int v = 1; v <= H; ++v) {
            const int d = U.u[v];
            for (int u = -d; u <= d; ++u) {
                const float val_plus = center[u + v * S], val_minus = center[u - v * S];
                m_10 += u * (val_plus + val_minus);
            }
        }
    } else if (lane <= H) {
        const int v = lane, d = U.u[v];
        for (int u = -d; u <= d; ++u) {
            const float val_plus = center[u + v * S], val_minus = center[u - v * S];
            v_sum += (val_plus - val_minus);
        }
    }
    m_10 = __shfl(m_10, 0, kWave);
    float m_01 = 0;
    for (int v = 1; v <= H; ++v) m_01 += v * __shfl(v_sum, v, kWave);
    const float angle = (float)atan2((double)m_01, (double)m_10);
    // ComputeDescriptor: the angle in radians goes through the degrees-to-radians factor, as the reference has it
    const float factorPI = (float)(3.1415926535897932384626433832795 / 180.f);
    const float theta = angle * factorPI;
    double sn, cs;
    ldso_ct::SharedSinCos()((double)theta, sn, cs);
    const float a = (float)cs, b = (float)sn;
    auto tap = [&](int p0, int p1) {
        const int row = cor_to_int(p0 * b + p1 * a), col = cor_to_int(p0 * a - p1 * b);
        // outside the patch only when the angle is not finite (the reference reads outside the image there)
        if (row < -H || row > H || col < -H || col > H) return INT_MIN;
        return cor_to_int(center[row * S + col]);
    };
#pragma unroll
    for (int m = 0; m < 4; m++) {
        const int4 p = pattern[m * kWave + lane];  // comparison 8 i + j: byte i, bit j (pattern + 32 i, index 4 j)
        const int t0 = tap(p.x, p.y), t1 = tap(p.z, p.w);
        const unsigned long long bits = __ballot(t0 < t1);
        if (lane == 0) desc[m] = bits;
    }
    if (lane == 0) {
        o->score = f.score;
        o->angle = angle;
        o->is_corner = 1;
        o->level = 0;
    }
}

}  // namespace
