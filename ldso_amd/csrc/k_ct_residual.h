// k_ct_residual.h -- calcRes and calcGSSSE (CoarseTracker.cc:540-741), one launch per call each:
//   k_ct_calc_res   thread per reference point, grid.y = pose hypothesis: warp, bounds, bilinear
//                   [I, dx, dy] of the new frame, Huber energy, saturation; per point a state byte
//                   and the two float4 of the warped record (the reference's buf_warped_* before
//                   compaction); per block the {E, nE, nSat, shiftT, shiftRT, shiftNum, nWarped}
//                   partials, summed on the host in block order.
//   k_ct_calc_gs    thread per point with state "warped": the 8 Jacobian entries + residual of
//                   calcGSSSE and the 45 weighted outer-product terms of Accumulator9, reduced over
//                   the wavefront and the block into 45 partials per block.
// calcRes' statements for one point stand once, in ct_res_point: k_ct_calc_res<false>, <true> and
// k_ct_track.h's sweep call the same function; what surrounds a launch (the hypothesis' constants, the
// Vec6 and the scaled H, b from the sums) is ct_eval.h, the same functions on host and device.
// The per-point arithmetic is compiled with contraction off in the reference's statement order
// (states, warped records bit-identical to the CPU restatement); E and the H/b sums are
// reassociated (the reference sums them sequentially in float) and tolerance-checked.
#pragma once
#include <cstdint>

#include "ct_eval.h"
#include "k_ct_pyramid.h"

#pragma clang fp contract(off)

namespace {

using ldso_ct::CtEvalTerms, ldso_ct::CtLevel, ldso_ct::CtPose, ldso_ct::kGsParts, ldso_ct::kResParts;  // ct_eval.h

// ---------------------------------------------------------------------------------------------
// k_ct_calc_res
// ---------------------------------------------------------------------------------------------
struct CtResParams {
    CtLevel lv;
    const CtPose *__restrict__ poses;  // per hypothesis, from the host's ct_eval_setup
    uint8_t *state;                    // 0 skipped, 1 saturated, 2 warped (write_warp only)
    float4 *warp;                      // [n][2]: {idepth, u, v, dx}, {dy, residual, weight, refColor}
    double *parts;                     // [hyp][blocks][kResParts]
    int lvl, write_warp, n_blocks;
    CtEvalTerms ev;                    // the cutoff is one for all hypotheses
    // k_ct_calc_res<true> (ldso_ct_calc_res_gs): one pose passed by value, and calcGSSSE's 45
    // Accumulator9 terms of every warped point summed in the same pass
    CtPose pose0;
    double *gs_parts;  // [blocks][kGsParts]
};

template <int K>
__device__ __forceinline__ void block_sum_write(double (&v)[K], double *dst) {
    __shared__ double red[kCtThreads / kWave][K];
    const int lane = threadIdx.x & (kWave - 1), wv = threadIdx.x / kWave;
#pragma unroll
    for (int k = 0; k < K; k++) {
#pragma unroll
        for (int m = 32; m >= 1; m >>= 1) v[k] += __shfl_xor(v[k], m, kWave);
    }
    if (lane == 0) {
#pragma unroll
        for (int k = 0; k < K; k++) red[wv][k] = v[k];
    }
    __syncthreads();
    for (int k = threadIdx.x; k < K; k += kCtThreads) dst[k] = (red[0][k] + red[1][k]) + (red[2][k] + red[3][k]);
}

// calcGSSSE's Jacobian row of one warped point (CoarseTracker.cc:696-722) from the values the
// warped buffers hold: id, u, v, dx = dI.y fxl, dy = dI.z fyl, refColor, residual
__device__ __forceinline__ void ct_gs_terms(float id, float u, float v, float dx, float dy, float a, float b0,
                                            float refColor, float residual, float w, double *acc) {
    float J[9];
    J[0] = id * dx;
    J[1] = id * dy;
    J[2] = 0 - id * (u * dx + v * dy);
    J[3] = 0 - ((u * v) * dx + dy * (1 + v * v));
    J[4] = (u * v) * dy + dx * (1 + u * u);
    J[5] = u * dy - v * dx;
    J[6] = a * (b0 - refColor);
    J[7] = -1;
    J[8] = residual;
    int k = 0;
#pragma unroll
    for (int r = 0; r < 9; r++) {
        const float Jw = J[r] * w;
#pragma unroll
        for (int c = r; c < 9; c++) acc[k++] = (double)(Jw * J[c]);
    }
}

// calcRes for point i of level L at the hypothesis (T, E) (CoarseTracker.cc:571-660): the kResParts terms
// into acc and, with kGS, calcGSSSE's kGsParts terms into gs (both zeroed by the caller); returns the state
// byte (0 skipped, 1 saturated, 2 warped).  kWarp: a warped point's two records leave through w0, w1.
// k_ct_calc_res<false>, <true> and k_ct_track's sweep are instantiations of this one text.
template <bool kGS, bool kWarp>
__device__ __forceinline__ uint8_t ct_res_point(const CtLevel &P, const CtPose &T, const CtEvalTerms &E, int lvl, int i,
                                                double *acc, double *gs, float4 &w0, float4 &w1) {
    const float4 q = P.pc[i];
    const float x = q.x, y = q.y, id = q.z;
    const float *RKi = T.RKi, *t = T.t;
    float pt[3];
#pragma unroll
    for (int k = 0; k < 3; k++) pt[k] = (RKi[3 * k] * x + RKi[3 * k + 1] * y + RKi[3 * k + 2] * 1) + t[k] * id;
    const float u = pt[0] / pt[2], v = pt[1] / pt[2];
    const float Ku = P.fxl * u + P.cxl, Kv = P.fyl * v + P.cyl;
    const float new_idepth = id / pt[2];
    if (lvl == 0 && i % 32 == 0) {  // CoarseTracker.cc:583-619
        float ptT[3], ptT2[3], pt3[3];
#pragma unroll
        for (int k = 0; k < 3; k++) {
            const float kx = P.Ki[3 * k] * x + P.Ki[3 * k + 1] * y + P.Ki[3 * k + 2] * 1;
            ptT[k] = kx + t[k] * id;
            ptT2[k] = kx - t[k] * id;
            pt3[k] = (RKi[3 * k] * x + RKi[3 * k + 1] * y + RKi[3 * k + 2] * 1) - t[k] * id;
        }
        const float uT = ptT[0] / ptT[2], vT = ptT[1] / ptT[2];
        const float KuT = P.fxl * uT + P.cxl, KvT = P.fyl * vT + P.cyl;
        const float uT2 = ptT2[0] / ptT2[2], vT2 = ptT2[1] / ptT2[2];
        const float KuT2 = P.fxl * uT2 + P.cxl, KvT2 = P.fyl * vT2 + P.cyl;
        const float u3 = pt3[0] / pt3[2], v3 = pt3[1] / pt3[2];
        const float Ku3 = P.fxl * u3 + P.cxl, Kv3 = P.fyl * v3 + P.cyl;
        const float sT = (KuT - x) * (KuT - x) + (KvT - y) * (KvT - y);
        const float sT2 = (KuT2 - x) * (KuT2 - x) + (KvT2 - y) * (KvT2 - y);
        const float sRT = (Ku - x) * (Ku - x) + (Kv - y) * (Kv - y);
        const float sRT2 = (Ku3 - x) * (Ku3 - x) + (Kv3 - y) * (Kv3 - y);
        acc[3] = (double)sT + (double)sT2;
        acc[4] = (double)sRT + (double)sRT2;
        acc[5] = 2;
    }
    uint8_t st = 0;
    if (Ku > 2 && Kv > 2 && Ku < P.wl - 3 && Kv < P.hl - 3 && new_idepth > 0) {
        const float refColor = q.w;
        // getInterpolatedElement33 (GlobalFuncs.h:89-103)
        const int ix = (int)Ku, iy = (int)Kv;
        const float dx = Ku - ix, dy = Kv - iy, dxdy = dx * dy;
        const float4 *bp = P.img + ix + (size_t)iy * P.wl;
        const float4 t11 = bp[1 + P.wl], t01 = bp[P.wl], t10 = bp[1], t00 = bp[0];
        const float w11 = dxdy, w01 = dy - dxdy, w10 = dx - dxdy, w00 = 1 - dx - dy + dxdy;
        const float h0 = w11 * t11.x + w01 * t01.x + w10 * t10.x + w00 * t00.x;
        const float h1 = w11 * t11.y + w01 * t01.y + w10 * t10.y + w00 * t00.y;
        const float h2 = w11 * t11.z + w01 * t01.z + w10 * t10.z + w00 * t00.z;
        if (isfinite(h0)) {
            const float residual = h0 - (float)(T.aLL * refColor + T.bLL);
            const float hw = fabsf(residual) < kHuberTH ? 1 : kHuberTH / fabsf(residual);
            acc[1] = 1;
            if (fabsf(residual) > E.cutoffTH) {
                acc[0] = E.maxEnergy;
                acc[2] = 1;
                st = 1;
            } else {
                acc[0] = hw * residual * residual * (2 - hw);
                acc[6] = 1;
                st = 2;
                if constexpr (kWarp) {
                    w0 = make_float4(new_idepth, u, v, h1);
                    w1 = make_float4(h2, residual, hw, refColor);
                }
                if constexpr (kGS)
                    ct_gs_terms(new_idepth, u, v, h1 * P.fxl, h2 * P.fyl, E.gs_a, E.gs_b0, refColor, residual, hw, gs);
            }
        }
    }
    return st;
}

template <bool kGS>
__global__ __launch_bounds__(kCtThreads) void k_ct_calc_res(CtResParams P) {
    const CtPose &T = kGS ? P.pose0 : P.poses[blockIdx.y];
    double gs[kGS ? kGsParts : 1];
#pragma unroll
    for (int k = 0; k < (kGS ? kGsParts : 1); k++) gs[k] = 0;
    const int i = blockIdx.x * kCtThreads + threadIdx.x;
    double acc[kResParts] = {0, 0, 0, 0, 0, 0, 0, 0};
    if (i < P.lv.n) {
        float4 w0, w1;
        const uint8_t st = ct_res_point<kGS, true>(P.lv, T, P.ev, P.lvl, i, acc, gs, w0, w1);
        if (P.write_warp) {
            if (st == 2) {
                P.warp[2 * (size_t)i] = w0;
                P.warp[2 * (size_t)i + 1] = w1;
            }
            P.state[i] = st;
        }
    }
    block_sum_write<kResParts>(acc, P.parts + ((size_t)blockIdx.y * P.n_blocks + blockIdx.x) * kResParts);
    if constexpr (kGS) {
        __syncthreads();  // block_sum_write's LDS is reused
        block_sum_write<kGsParts>(gs, P.gs_parts + (size_t)blockIdx.x * kGsParts);
    }
}

// ---------------------------------------------------------------------------------------------
// k_ct_calc_gs: calcGSSSE's Jacobian (CoarseTracker.cc:696-722) and Accumulator9's weighted
// outer products (MatrixAccumulators.h:1250-1368), upper 9x9 = 45 terms
// ---------------------------------------------------------------------------------------------
struct CtGsParams {
    const uint8_t *__restrict__ state;
    const float4 *__restrict__ warp;
    double *parts;  // [blocks][kGsParts]
    int n;
    float fxl, fyl, a, b0;
};

__global__ __launch_bounds__(kCtThreads) void k_ct_calc_gs(CtGsParams P) {
    const int i = blockIdx.x * kCtThreads + threadIdx.x;
    double acc[kGsParts];
#pragma unroll
    for (int k = 0; k < kGsParts; k++) acc[k] = 0;
    if (i < P.n && P.state[i] == 2) {
        const float4 q0 = P.warp[2 * (size_t)i], q1 = P.warp[2 * (size_t)i + 1];
        ct_gs_terms(q0.x, q0.y, q0.z, q0.w * P.fxl, q1.x * P.fyl, P.a, P.b0, q1.w, q1.y, q1.z, acc);
    }
    block_sum_write<kGsParts>(acc, P.parts + (size_t)blockIdx.x * kGsParts);
}

}  // namespace
