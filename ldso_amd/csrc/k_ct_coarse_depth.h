// k_ct_coarse_depth.h -- CoarseTracker::makeCoarseDepthL0 (CoarseTracker.cc:357-538) on the device:
// the reference frame's point clouds pc_u / pc_v / pc_idepth / pc_color of every pyramid level from
// the contributions (centerProjectedTo, HdiF) of the window's points.
//
//   k_ct_cd_gather   (from a BA context only) thread per residual of the window: the residual to
//                    the reference frame with state IN writes its point's contribution
//                    {c[0], c[1], c[2], HdiF} at the point's device index, which is the
//                    reference's traversal order; other points keep a NaN hole.
//   k_ct_cd_scatter  thread per contribution: the lowest-index contribution of a pixel (the
//                    "leader") sums its pixel's contributions in ascending index order, the
//                    reference's sequential float chain from 0, and writes the two sums with plain
//                    stores; every other contribution writes nothing.  Keys travel through LDS in
//                    tiles of 256: n^2 key comparisons over ceil(n / 256) blocks, no atomics.
//   k_ct_cd_pyr      block per T x T level-0 tile (T = 2^(levels-1)): both maps of the tile go to
//                    LDS once and every coarser level is the 2x2 sum ((a + b) + c) + d there.
//   k_ct_cd_flag     thread per pixel of every level: dilation, normalisation and the emit test
//                    fused.  A pixel with weight <= 0 is filled from its neighbours with weight
//                    > 0, which the dilation never modifies, so the final value of a pixel is a
//                    function of the undilated maps and no dilated map is ever written.
//                    Candidates {x, y, idepth, colour} (x = -1: not emitted) and a count per block.
//   k_ct_cd_scan     one block: exclusive prefix of the block counts per level, the level counts
//                    to mapped host memory and the level offsets of the cloud.
//   k_ct_cd_write    stable compaction in row-major order: wave64 ballots and prefix counts.
//
// Arithmetic in the reference's statement order, contraction off, default (correctly rounded)
// division and sqrtf.
#pragma once
#include <cstdint>

#include "../../include/ldso_ba.h"
#include "k_ct_pyramid.h"

#pragma clang fp contract(off)

namespace {

// pixel of a contribution, or -1: int(c + 0.5f) truncates, so c + 0.5f in (-1, 0) is pixel 0; a
// centre outside the image (the reference would write outside its arrays), a NaN or a hole is skipped
__device__ __forceinline__ int cd_key(float cx, float cy, int w, int h) {
    const float tu = cx + 0.5f, tv = cy + 0.5f;
    if (!(tu > -1.0f && tu < (float)w && tv > -1.0f && tv < (float)h)) return -1;
    return (int)tu + w * (int)tv;
}

// sqrtf(1e-3 / (ph->HdiF + 1e-12)): the sum and the quotient in double (CoarseTracker.cc:375)
__device__ __forceinline__ float cd_weight(float hdi) { return sqrtf((float)(1e-3 / ((double)hdi + 1e-12))); }

struct CdGatherParams {
    const float *__restrict__ center;  // planes, see BaRefView
    long long plane_stride;
    const int8_t *__restrict__ state;
    const uint8_t *__restrict__ tgt;
    const int *__restrict__ slot;
    const float *__restrict__ pt_out;
    float4 *contrib;  // [P], preset to NaN holes
    int R, P, rec_base, ref_frame;
};

__global__ __launch_bounds__(kCtThreads) void k_ct_cd_gather(CdGatherParams G) {
    const int r = blockIdx.x * kCtThreads + threadIdx.x;
    if (r >= G.R) return;
    if (G.tgt[r] != G.ref_frame || G.state[r] != LDSO_BA_RES_IN) return;
    const int s = G.slot[r] - G.rec_base;
    if (s < 0) return;
    const int q = s % G.P;
    G.contrib[q] = make_float4(G.center[r], G.center[G.plane_stride + r], G.center[2 * G.plane_stride + r],
                               G.pt_out[(size_t)q * 12]);
}

__global__ __launch_bounds__(kCtThreads) void k_ct_cd_scatter(const float4 *__restrict__ contrib, int n,
                                                              float *__restrict__ idepth0, float *__restrict__ wsum0,
                                                              int w, int h) {
    __shared__ int keys[kCtThreads];
    const int i = blockIdx.x * kCtThreads + threadIdx.x;
    int my = -1;
    if (i < n) {
        const float4 c = contrib[i];
        my = cd_key(c.x, c.y, w, h);
    }
    bool leader = my >= 0;
    float sid = 0, sw = 0;
    for (int t0 = 0; t0 < n; t0 += kCtThreads) {
        const int j = t0 + threadIdx.x;
        int kj = -1;
        if (j < n) {
            const float4 c = contrib[j];
            kj = cd_key(c.x, c.y, w, h);
        }
        keys[threadIdx.x] = kj;
        __syncthreads();
        if (leader) {
            const int m = min(kCtThreads, n - t0);
            for (int k = 0; k < m; k++) {
                if (keys[k] != my) continue;
                const int jj = t0 + k;
                if (jj < i) {  // an earlier contribution owns this pixel
                    leader = false;
                    break;
                }
                const float4 cj = contrib[jj];
                const float weight = cd_weight(cj.w);
                sid += cj.z * weight;
                sw += weight;
            }
        }
        __syncthreads();
    }
    if (leader) {
        idepth0[my] = sid;
        wsum0[my] = sw;
    }
}

// levels 1..L-1 of both maps from level 0 (CoarseTracker.cc:384-409)
__global__ __launch_bounds__(kCtThreads) void k_ct_cd_pyr(float *__restrict__ idepth, float *__restrict__ wsum,
                                                          PyrParams P) {
    extern __shared__ float cd_lds[];  // idepth [T*T] + [(T/2)^2], then the same for the weights
    const int T = P.tile, tx0 = blockIdx.x * T, ty0 = blockIdx.y * T;
    const int half = (T / 2) * (T / 2);
    float *Ai = cd_lds, *Bi = Ai + T * T, *Aw = Bi + half, *Bw = Aw + T * T;
    for (int i = threadIdx.x; i < T * T; i += kCtThreads) {
        const size_t g = (size_t)(ty0 + i / T) * P.w + tx0 + (i % T);
        Ai[i] = idepth[g];
        Aw[i] = wsum[g];
    }
    __syncthreads();
    float *si = Ai, *di = Bi, *sw = Aw, *dw = Bw;
    for (int l = 1; l < P.levels; l++) {
        const int Ts = T >> (l - 1), Td = T >> l;
        for (int i = threadIdx.x; i < Td * Td; i += kCtThreads) {
            const int x = i % Td, y = i / Td;
            const int b = 2 * y * Ts + 2 * x;
            const float vi = si[b] + si[b + 1] + si[b + Ts] + si[b + Ts + 1];
            const float vw = sw[b] + sw[b + 1] + sw[b + Ts] + sw[b + Ts + 1];
            di[i] = vi;
            dw[i] = vw;
            const size_t g = P.off[l] + (size_t)(blockIdx.y * Td + y) * P.wl[l] + blockIdx.x * Td + x;
            idepth[g] = vi;
            wsum[g] = vw;
        }
        __syncthreads();
        float *t = si;
        si = di;
        di = t;
        t = sw;
        sw = dw;
        dw = t;
    }
}

struct CdLevels {
    int blk_off[LDSO_CT_MAX_LEVELS + 1];  // first block of each level in the flag / write grids
};

// count of set predicates in the block -> *total (thread 0), and each thread's exclusive prefix
__device__ __forceinline__ int cd_block_prefix(bool pred, int *total) {
    __shared__ int wave_cnt[kCtThreads / kWave];
    const int lane = threadIdx.x & (kWave - 1), wv = threadIdx.x / kWave;
    const unsigned long long mask = __ballot(pred);
    const int before = __popcll(mask & ((1ull << lane) - 1ull));
    if (lane == 0) wave_cnt[wv] = __popcll(mask);
    __syncthreads();
    int base = 0, all = 0;
#pragma unroll
    for (int k = 0; k < kCtThreads / kWave; k++) {
        if (k < wv) base += wave_cnt[k];
        all += wave_cnt[k];
    }
    *total = all;
    return base + before;
}

// dilation (CoarseTracker.cc:411-495), normalisation and the emit test (:497-537) of one pixel
__global__ __launch_bounds__(kCtThreads) void k_ct_cd_flag(const float *__restrict__ idepth,
                                                           const float *__restrict__ wsum,
                                                           const float4 *__restrict__ dIp, float4 *__restrict__ cand,
                                                           int *__restrict__ blk_cnt, PyrParams P, CdLevels B) {
    int l = 0;
    while ((int)blockIdx.x >= B.blk_off[l + 1]) l++;
    const int wl = P.wl[l], hl = P.hl[l];
    const int idx = ((int)blockIdx.x - B.blk_off[l]) * kCtThreads + threadIdx.x;
    bool emit = false;
    if (idx < wl * hl) {
        const int x = idx % wl, y = idx / wl;
        float4 out = make_float4(-1.f, -1.f, -1.f, 0.f);
        if (x >= 2 && x < wl - 2 && y >= 2 && y < hl - 2) {
            const float *I = idepth + P.off[l], *W = wsum + P.off[l];
            float id = I[idx], wt = W[idx];
            if (wt <= 0) {  // a NaN weight is neither filled nor emitted, as in the reference
                // neighbour offsets in the reference's order: diagonal on levels 0 and 1, axis above
                const int o0 = l < 2 ? 1 + wl : 1, o1 = l < 2 ? -1 - wl : -1;
                const int o2 = l < 2 ? wl - 1 : wl, o3 = l < 2 ? -wl + 1 : -wl;
                const int o[4] = {o0, o1, o2, o3};
                float sum = 0, num = 0, numn = 0;
#pragma unroll
                for (int k = 0; k < 4; k++) {
                    const float wn = W[idx + o[k]];
                    if (wn > 0) {
                        sum += I[idx + o[k]];
                        num += wn;
                        numn++;
                    }
                }
                if (numn > 0) {
                    id = sum / numn;
                    wt = num / numn;
                }
            }
            if (wt > 0) {
                id = id / wt;
                const float color = dIp[P.off[l] + idx].x;
                if (isfinite(color) && id > 0) {
                    emit = true;
                    out = make_float4((float)x, (float)y, id, color);
                }
            }
        }
        cand[P.off[l] + idx] = out;
    }
    int total;
    (void)cd_block_prefix(emit, &total);
    if (threadIdx.x == 0) blk_cnt[blockIdx.x] = total;
}

// per level: exclusive prefix of the block counts (in place), the level's count to the mapped
// host array and the cumulative level offsets of the cloud
__global__ __launch_bounds__(kCtThreads) void k_ct_cd_scan(int *__restrict__ blk_cnt, int *__restrict__ lvl_off,
                                                           int *__restrict__ host_counts, int levels, CdLevels B) {
    __shared__ int wave_sum[kCtThreads / kWave];
    __shared__ int carry_s;
    const int lane = threadIdx.x & (kWave - 1), wv = threadIdx.x / kWave;
    int cum = 0;
    if (threadIdx.x == 0) lvl_off[0] = 0;
    for (int l = 0; l < levels; l++) {
        if (threadIdx.x == 0) carry_s = 0;
        __syncthreads();
        for (int b0 = B.blk_off[l]; b0 < B.blk_off[l + 1]; b0 += kCtThreads) {
            const int b = b0 + threadIdx.x;
            const int v = b < B.blk_off[l + 1] ? blk_cnt[b] : 0;
            int s = v;  // inclusive scan over the wave
#pragma unroll
            for (int m = 1; m < kWave; m <<= 1) {
                const int t = __shfl_up(s, m, kWave);
                if (lane >= m) s += t;
            }
            if (lane == kWave - 1) wave_sum[wv] = s;
            __syncthreads();
            int base = carry_s, all = 0;
#pragma unroll
            for (int k = 0; k < kCtThreads / kWave; k++) {
                if (k < wv) base += wave_sum[k];
                all += wave_sum[k];
            }
            if (b < B.blk_off[l + 1]) blk_cnt[b] = base + s - v;
            __syncthreads();
            if (threadIdx.x == 0) carry_s += all;
            __syncthreads();
        }
        const int n_l = carry_s;
        cum += n_l;
        if (threadIdx.x == 0) {
            host_counts[l] = n_l;
            lvl_off[l + 1] = cum;
        }
        __syncthreads();
    }
}

__global__ __launch_bounds__(kCtThreads) void k_ct_cd_write(const float4 *__restrict__ cand,
                                                            const int *__restrict__ blk_off_in_lvl,
                                                            const int *__restrict__ lvl_off, float4 *__restrict__ pc,
                                                            PyrParams P, CdLevels B) {
    int l = 0;
    while ((int)blockIdx.x >= B.blk_off[l + 1]) l++;
    const int idx = ((int)blockIdx.x - B.blk_off[l]) * kCtThreads + threadIdx.x;
    float4 v = make_float4(-1.f, -1.f, -1.f, 0.f);
    if (idx < P.wl[l] * P.hl[l]) v = cand[P.off[l] + idx];
    const bool emit = v.x >= 0;
    int total;
    const int pre = cd_block_prefix(emit, &total);
    if (emit) pc[(size_t)lvl_off[l] + blk_off_in_lvl[blockIdx.x] + pre] = v;
}

}  // namespace
