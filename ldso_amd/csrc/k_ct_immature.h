// k_ct_immature.h -- immature points (ImmaturePoint.cc:14-39, 47-317; FullSystem::traceNewCoarse):
//   k_ct_make_immature  thread per new point: 8 bilinear pattern samples of the new frame.
//   k_ct_trace          wavefront per immature point: the scalar preamble (epipolar segment,
//                       bounds, error bound) runs uniformly on all lanes; lane i evaluates
//                       discrete search step i (and i + 64), its position reproduced by the
//                       reference's sequential ptx += dx; argmin (first index of the minimum)
//                       and the second best outside +-2 steps are wave reductions; each GN
//                       iteration samples the 8 pattern taps on lanes 0-7 and every lane sums
//                       them in pattern order.  Statuses and intervals are bit-identical to the
//                       CPU restatement.
//   k_ct_ip_count       one block: the traceNewCoarse status counters.
#pragma once
#include "k_ct_pyramid.h"

#pragma clang fp contract(off)

namespace {

// ---------------------------------------------------------------------------------------------
// immature points: ImmaturePoint::ImmaturePoint and ::traceOn (ImmaturePoint.cc:14-39, 47-317)
// ---------------------------------------------------------------------------------------------
constexpr int kPatX[8] = {0, -1, 1, -2, 0, 2, -1, 0}, kPatY[8] = {-2, -1, -1, 0, 0, 0, 1, 2};  // Setting.cc:275
constexpr float kOutlierTHSumComponent = ldso_ba::kOutlierTHSumComponent;  // Setting.cc:41
constexpr float kOutlierTH = 12 * 12;                    // Setting.cc:39
constexpr float kOverallEnergyTHWeight = ldso_ba::kOverallEnergyTHWeight;
constexpr float kMaxPixSearch = 0.027f;                  // Setting.cc:28
constexpr int kMinTraceTestRadius = 2;                   // Setting.cc:52
constexpr float kTraceStepsize = 1.0f;                   // Setting.cc:89
constexpr int kTraceGNIterations = 3;                    // Setting.cc:90
constexpr float kTraceGNThreshold = 0.1f;                // Setting.cc:91
constexpr float kTraceExtraSlackOnTH = 1.2f;             // Setting.cc:92
constexpr float kTraceSlackInterval = 1.5f;              // Setting.cc:93
constexpr float kTraceMinImprovementFactor = 2;          // Setting.cc:94
constexpr int kHostStride = 16;                          // KRKi[9], Kt[3], aff[2], pad[2]

// top-left texel of a bilinear tap, clamped into [0, w-2] x [0, h-2] (the reference would read
// past the image there; the oracle clamps the same way)
__device__ __forceinline__ int ip_base(float x, float y, int w, int h, float &fx, float &fy) {
    const int ix = (int)x, iy = (int)y;
    fx = x - ix;
    fy = y - iy;
    return min(max(ix, 0), w - 2) + min(max(iy, 0), h - 2) * w;
}

struct IpRec {  // ldso_ct_immature viewed as 32 words
    float u, v, idepth_min, idepth_max, quality, energy_th, color[8], weights[8], grad_h[4];
    int host, last_status;
    float last_uv[2], last_interval, type;
};
static_assert(sizeof(IpRec) == sizeof(ldso_ct_immature), "record layout");

// new ImmaturePoint(newFrame, feat, type, HCalib): getInterpolatedElement33BiLin (GlobalFuncs.h:186-207)
__device__ __forceinline__ IpRec ip_make_record(const float4 *__restrict__ dI, int w, int h, float u, float v,
                                                float type, int host) {
    IpRec p;
    p.u = u;
    p.v = v;
    p.idepth_min = 0;
    p.idepth_max = __builtin_nanf("");
    p.quality = 10000;
    p.type = type;
    p.host = host;
    p.last_status = LDSO_CT_IPS_UNINITIALIZED;
    p.last_uv[0] = p.last_uv[1] = 0;
    p.last_interval = 0;
    float G0 = 0, G1 = 0, G2 = 0, G3 = 0;
    bool ok = true;
#pragma unroll
    for (int idx = 0; idx < 8; idx++) p.color[idx] = p.weights[idx] = 0;
#pragma unroll
    for (int idx = 0; idx < 8; idx++) {
        if (!ok) break;
        float dx, dy;
        const int b = ip_base(p.u + kPatX[idx], p.v + kPatY[idx], w, h, dx, dy);
        const float tl = dI[b].x, tr = dI[b + 1].x, bl = dI[b + w].x, br = dI[b + w + 1].x;
        const float topInt = dx * tr + (1 - dx) * tl;
        const float botInt = dx * br + (1 - dx) * bl;
        const float leftInt = dy * bl + (1 - dy) * tl;
        const float rightInt = dy * br + (1 - dy) * tr;
        const float c0 = dx * rightInt + (1 - dx) * leftInt, g0 = rightInt - leftInt, g1 = botInt - topInt;
        p.color[idx] = c0;
        if (!isfinite(c0)) {
            ok = false;
            break;
        }
        G0 += g0 * g0;
        G1 += g0 * g1;
        G2 += g1 * g0;
        G3 += g1 * g1;
        p.weights[idx] = sqrtf(kOutlierTHSumComponent / (kOutlierTHSumComponent + (g0 * g0 + g1 * g1)));
    }
    p.grad_h[0] = G0;
    p.grad_h[1] = G1;
    p.grad_h[2] = G2;
    p.grad_h[3] = G3;
    float e = 8 * kOutlierTH;
    e *= kOverallEnergyTHWeight * kOverallEnergyTHWeight;
    p.energy_th = ok ? e : __builtin_nanf("");
    return p;
}

// thread per new point (ldso_ct_make_immature); k_ct_select.h's emit walk makes its records the same way
__global__ __launch_bounds__(kCtThreads) void k_ct_make_immature(const float4 *__restrict__ dI, int w, int h, int n,
                                                                 const float2 *__restrict__ uv, float type, int host,
                                                                 IpRec *__restrict__ out) {
    const int k = blockIdx.x * kCtThreads + threadIdx.x;
    if (k >= n) return;
    out[k] = ip_make_record(dI, w, h, uv[k].x, uv[k].y, type, host);
}

struct TraceParams {
    const float4 *__restrict__ dI;  // level 0 [I, dx, dy, |g|^2] (GN taps)
    const float *__restrict__ inten;  // level 0 intensities, = dI[].x (discrete-search taps: 4 B, not 16)
    const float *__restrict__ hosts;  // [n_hosts][kHostStride]
    IpRec *pts;
    int n, w, h;
};

__device__ __forceinline__ void ip_finish(IpRec *q, int status, float u, float v, float interval) {
    if (threadIdx.x % kWave == 0) {
        q->last_status = status;
        q->last_uv[0] = u;
        q->last_uv[1] = v;
        q->last_interval = interval;
    }
}

// getInterpolatedElement31 (GlobalFuncs.h:146-159)
__device__ __forceinline__ float interp31(const float *__restrict__ I, float x, float y, int w, int h) {
    float dx, dy;
    const int b = ip_base(x, y, w, h, dx, dy);
    const float dxdy = dx * dy;
    return dxdy * I[b + 1 + w] + (dy - dxdy) * I[b + w] + (dx - dxdy) * I[b + 1] + (1 - dx - dy + dxdy) * I[b];
}

// one wavefront per immature point; every branch before the search is wave-uniform
__global__ __launch_bounds__(kCtThreads) void k_ct_trace(TraceParams P) {
    const int lane = threadIdx.x % kWave;
    const int k = __builtin_amdgcn_readfirstlane(blockIdx.x * (kCtThreads / kWave) + threadIdx.x / kWave);
    if (k >= P.n) return;
    IpRec *q = P.pts + k;
    const int last = q->last_status;
    if (last == LDSO_CT_IPS_OOB) return;
    const int w = P.w, h = P.h;
    const float *H = P.hosts + (size_t)q->host * kHostStride;
    const float KR[9] = {H[0], H[1], H[2], H[3], H[4], H[5], H[6], H[7], H[8]};
    const float Kt[3] = {H[9], H[10], H[11]}, aff0 = H[12], aff1 = H[13];
    const float u = q->u, v = q->v, idepth_min = q->idepth_min, idepth_max = q->idepth_max;
    const float maxPixSearch = (w + h) * kMaxPixSearch;
    float pr[3], ptpMin[3];
#pragma unroll
    for (int i = 0; i < 3; i++) pr[i] = KR[3 * i] * u + KR[3 * i + 1] * v + KR[3 * i + 2] * 1.0f;
#pragma unroll
    for (int i = 0; i < 3; i++) ptpMin[i] = pr[i] + Kt[i] * idepth_min;
    const float uMin = ptpMin[0] / ptpMin[2], vMin = ptpMin[1] / ptpMin[2];
    if (!(uMin > 4 && vMin > 4 && uMin < w - 5 && vMin < h - 5)) return ip_finish(q, LDSO_CT_IPS_OOB, -1, -1, 0);
    const bool finite_max = isfinite(idepth_max);
    float dist, uMax, vMax;
    if (finite_max) {
        float ptpMax[3];
#pragma unroll
        for (int i = 0; i < 3; i++) ptpMax[i] = pr[i] + Kt[i] * idepth_max;
        uMax = ptpMax[0] / ptpMax[2];
        vMax = ptpMax[1] / ptpMax[2];
        if (!(uMax > 4 && vMax > 4 && uMax < w - 5 && vMax < h - 5)) return ip_finish(q, LDSO_CT_IPS_OOB, -1, -1, 0);
        dist = (uMin - uMax) * (uMin - uMax) + (vMin - vMax) * (vMin - vMax);
        dist = sqrtf(dist);
        if (dist < kTraceSlackInterval)
            return ip_finish(q, LDSO_CT_IPS_SKIPPED, (uMax + uMin) * 0.5f, (vMax + vMin) * 0.5f, dist);
    } else {
        dist = maxPixSearch;
        float ptpMax[3];
#pragma unroll
        for (int i = 0; i < 3; i++) ptpMax[i] = pr[i] + Kt[i] * 0.01f;
        uMax = ptpMax[0] / ptpMax[2];
        vMax = ptpMax[1] / ptpMax[2];
        const float dx = uMax - uMin, dy = vMax - vMin;
        const float d = 1.0f / sqrtf(dx * dx + dy * dy);
        uMax = uMin + dist * dx * d;
        vMax = vMin + dist * dy * d;
        if (!(uMax > 4 && vMax > 4 && uMax < w - 5 && vMax < h - 5)) return ip_finish(q, LDSO_CT_IPS_OOB, -1, -1, 0);
    }
    if (!(idepth_min < 0 || (ptpMin[2] > 0.75f && ptpMin[2] < 1.5f))) return ip_finish(q, LDSO_CT_IPS_OOB, -1, -1, 0);

    float dx = kTraceStepsize * (uMax - uMin);
    float dy = kTraceStepsize * (vMax - vMin);
    const float G0 = q->grad_h[0], G1 = q->grad_h[1], G2 = q->grad_h[2], G3 = q->grad_h[3];
    const float a = (dx * G0 + dy * G2) * dx + (dx * G1 + dy * G3) * dy;
    const float b = (dy * G0 + -dx * G2) * dy + (dy * G1 + -dx * G3) * -dx;
    float errorInPixel = 0.2f + 0.2f * (a + b) / a;
    if (errorInPixel * kTraceMinImprovementFactor > dist && finite_max)
        return ip_finish(q, LDSO_CT_IPS_BADCONDITION, (uMax + uMin) * 0.5f, (vMax + vMin) * 0.5f, dist);
    if (errorInPixel > 10) errorInPixel = 10;
    dx /= dist;
    dy /= dist;
    if (dist > maxPixSearch) dist = maxPixSearch;  // (uMax, vMax are not used past this point)
    int numSteps = 1.9999f + dist / kTraceStepsize;
    const float randShift = uMin * 1000 - floorf(uMin * 1000);
    const float ptx0 = uMin - randShift * dx, pty0 = vMin - randShift * dy;
    float rpx[8], rpy[8];
#pragma unroll
    for (int i = 0; i < 8; i++) {
        rpx[i] = KR[0] * (float)kPatX[i] + KR[1] * (float)kPatY[i];
        rpy[i] = KR[3] * (float)kPatX[i] + KR[4] * (float)kPatY[i];
    }
    if (!isfinite(dx) || !isfinite(dy)) return ip_finish(q, LDSO_CT_IPS_OOB, -1, -1, 0);
    if (numSteps >= 100) numSteps = 99;
    float col[8], wts[8];
#pragma unroll
    for (int i = 0; i < 8; i++) {
        col[i] = q->color[i];
        wts[i] = q->weights[i];
    }

    // ---- discrete search: lane i takes step i and step i + 64 ----
    float x0 = 0, y0 = 0, x1 = 0, y1 = 0;  // ptx, pty of the lane's steps (sequential sums)
    {
        float px = ptx0, py = pty0;
        for (int i = 0; i < numSteps; i++) {
            if (i == lane) {
                x0 = px;
                y0 = py;
            }
            if (i == lane + kWave) {
                x1 = px;
                y1 = py;
            }
            px += dx;
            py += dy;
        }
    }
    auto step_energy = [&](float ptx, float pty) {
        float energy = 0;
#pragma unroll
        for (int idx = 0; idx < 8; idx++) {
            const float hitColor = interp31(P.inten, (float)(ptx + rpx[idx]), (float)(pty + rpy[idx]), w, h);
            if (!isfinite(hitColor)) {
                energy += 1e5f;
                continue;
            }
            const float residual = hitColor - (float)(aff0 * col[idx] + aff1);
            const float hw = fabsf(residual) < kHuberTH ? 1 : kHuberTH / fabsf(residual);
            energy += hw * residual * residual * (2 - hw);
        }
        return energy;
    };
    const bool has0 = lane < numSteps, has1 = lane + kWave < numSteps;
    const float e0 = has0 ? step_energy(x0, y0) : 0.f;
    const float e1 = has1 ? step_energy(x1, y1) : 0.f;
    // first index of the minimum among energies < 1e10 (energies are >= 0 or NaN)
    auto key = [](bool has, float e, int i) -> unsigned long long {
        return (has && e < 1e10f) ? ((unsigned long long)__float_as_uint(e) << 32) | (unsigned)i : ~0ull;
    };
    unsigned long long kmin = min(key(has0, e0, lane), key(has1, e1, lane + kWave));
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) kmin = min(kmin, (unsigned long long)__shfl_xor(kmin, m, kWave));
    int bestIdx = -1;
    float bestEnergy = 1e10f, bestU = 0, bestV = 0;
    if (kmin != ~0ull) {
        bestIdx = (int)(unsigned)kmin;
        bestEnergy = __uint_as_float((unsigned)(kmin >> 32));
        const int src = bestIdx & (kWave - 1);
        const float bx0 = __shfl(x0, src, kWave), by0 = __shfl(y0, src, kWave);
        const float bx1 = __shfl(x1, src, kWave), by1 = __shfl(y1, src, kWave);
        bestU = bestIdx < kWave ? bx0 : bx1;
        bestV = bestIdx < kWave ? by0 : by1;
    }
    auto outside = [&](int i) { return i < bestIdx - kMinTraceTestRadius || i > bestIdx + kMinTraceTestRadius; };
    float sb = 1e10f;
    if (has0 && outside(lane) && e0 < sb) sb = e0;
    if (has1 && outside(lane + kWave) && e1 < sb) sb = e1;
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) sb = fminf(sb, __shfl_xor(sb, m, kWave));
    const float newQuality = sb / bestEnergy;
    float quality = q->quality;
    if (newQuality < quality || numSteps > 10) quality = newQuality;

    // ---- GN refinement: taps on lanes 0-7, sums in pattern order on every lane ----
    float uBak = bestU, vBak = bestV, gnstepsize = 1, stepBack = 0;
    if (kTraceGNIterations > 0) bestEnergy = 1e5f;
    for (int it = 0; it < kTraceGNIterations; it++) {
        const int idx = lane & 7;
        float rpxi = rpx[0], rpyi = rpy[0], ci = col[0], wi = wts[0];
#pragma unroll
        for (int i = 1; i < 8; i++)
            if (idx == i) {
                rpxi = rpx[i];
                rpyi = rpy[i];
                ci = col[i];
                wi = wts[i];
            }
        float fx, fy;
        const int bb = ip_base((float)(bestU + rpxi), (float)(bestV + rpyi), w, h, fx, fy);
        const float4 t00 = P.dI[bb], t10 = P.dI[bb + 1], t01 = P.dI[bb + w], t11 = P.dI[bb + w + 1];
        const float dxdy = fx * fy;
        const float w11 = dxdy, w01 = fy - dxdy, w10 = fx - dxdy, w00 = 1 - fx - fy + dxdy;
        const float hc0 = w11 * t11.x + w01 * t01.x + w10 * t10.x + w00 * t00.x;
        const float hc1 = w11 * t11.y + w01 * t01.y + w10 * t10.y + w00 * t00.y;
        const float hc2 = w11 * t11.z + w01 * t01.z + w10 * t10.z + w00 * t00.z;
        const bool fin = isfinite(hc0);
        const float residual = hc0 - (aff0 * ci + aff1);
        const float dResdDist = dx * hc1 + dy * hc2;
        const float hw = fabsf(residual) < kHuberTH ? 1 : kHuberTH / fabsf(residual);
        const float tH = hw * dResdDist * dResdDist;
        const float tb = hw * residual * dResdDist;
        const float tE = wi * wi * hw * residual * residual * (2 - hw);
        float Hs = 1, bs = 0, energy = 0;
#pragma unroll
        for (int i = 0; i < 8; i++) {
            const bool f = __shfl(fin ? 1 : 0, i, kWave) != 0;
            const float h_ = __shfl(tH, i, kWave), b_ = __shfl(tb, i, kWave), e_ = __shfl(tE, i, kWave);
            if (!f) {
                energy += 1e5f;
                continue;
            }
            Hs += h_;
            bs += b_;
            energy += e_;
        }
        if (energy > bestEnergy) {
            stepBack *= 0.5f;
            bestU = uBak + stepBack * dx;
            bestV = vBak + stepBack * dy;
        } else {
            float step = -gnstepsize * bs / Hs;
            if (step < -0.5f) step = -0.5f;
            else if (step > 0.5f) step = 0.5f;
            if (!isfinite(step)) step = 0;
            uBak = bestU;
            vBak = bestV;
            stepBack = step;
            bestU += step * dx;
            bestV += step * dy;
            bestEnergy = energy;
        }
        if (fabsf(stepBack) < kTraceGNThreshold) break;
    }
    if (lane == 0) q->quality = quality;

    if (!(bestEnergy < q->energy_th * kTraceExtraSlackOnTH))
        return ip_finish(q, last == LDSO_CT_IPS_OUTLIER ? LDSO_CT_IPS_OOB : LDSO_CT_IPS_OUTLIER, -1, -1, 0);
    float imin, imax;
    if (dx * dx > dy * dy) {
        imin = (pr[2] * (bestU - errorInPixel * dx) - pr[0]) / (Kt[0] - Kt[2] * (bestU - errorInPixel * dx));
        imax = (pr[2] * (bestU + errorInPixel * dx) - pr[0]) / (Kt[0] - Kt[2] * (bestU + errorInPixel * dx));
    } else {
        imin = (pr[2] * (bestV - errorInPixel * dy) - pr[1]) / (Kt[1] - Kt[2] * (bestV - errorInPixel * dy));
        imax = (pr[2] * (bestV + errorInPixel * dy) - pr[1]) / (Kt[1] - Kt[2] * (bestV + errorInPixel * dy));
    }
    if (imin > imax) {
        const float t = imin;
        imin = imax;
        imax = t;
    }
    if (lane == 0) {
        q->idepth_min = imin;
        q->idepth_max = imax;
    }
    if (!isfinite(imin) || !isfinite(imax) || (imax < 0)) return ip_finish(q, LDSO_CT_IPS_OUTLIER, -1, -1, 0);
    ip_finish(q, LDSO_CT_IPS_GOOD, bestU, bestV, 2 * errorInPixel);
}

// traceNewCoarse's counters (FullSystem.cc:1184-1190): one block
__global__ __launch_bounds__(1024) void k_ct_ip_count(const IpRec *__restrict__ pts, int n, int *__restrict__ counts) {
    __shared__ int c[8];
    if (threadIdx.x < 8) c[threadIdx.x] = 0;
    __syncthreads();
    int loc[6] = {0, 0, 0, 0, 0, 0};
    for (int k = threadIdx.x; k < n; k += blockDim.x) {
        const int s = pts[k].last_status;
#pragma unroll
        for (int j = 0; j < 6; j++) loc[j] += s == j;
    }
#pragma unroll
    for (int j = 0; j < 6; j++) {
        int x = loc[j];
#pragma unroll
        for (int m = 32; m >= 1; m >>= 1) x += __shfl_xor(x, m, kWave);
        if (threadIdx.x % kWave == 0 && x) atomicAdd(&c[j], x);
    }
    __syncthreads();
    if (threadIdx.x < 6) counts[threadIdx.x] = c[threadIdx.x];
}

}  // namespace
