// k_activate.h -- point activation (FullSystem::optimizeImmaturePoint).
#pragma once
#include "../../include/ldso_ct.h"
#include "ba_device.h"

namespace {

// ============================================================================================
// k_activate: FullSystem::optimizeImmaturePoint (FullSystem.cc:1035-1156) with
// ImmaturePoint::linearizeResidual (ImmaturePoint.cc:319-389), SURVEY §8f row 4.
// One wavefront per immature point; the temporary residual to the r-th other frame (window order)
// is evaluated by eight lanes, one per pattern pixel (see k_activate); the point's Hdd, bd and
// energy are summed on every lane in the reference's order (residual by residual, pixel by pixel,
// with the pixels before an OOB pixel still counted), so the LM steps are wave-uniform and
// bit-identical to the CPU restatement.
// ============================================================================================
struct ActParams {
    const WinDev *__restrict__ wins;
    const float4 *__restrict__ img;
    const float *__restrict__ precalc;
    const ldso_ct_immature *__restrict__ pts;
    ldso_ba_activation *out;
    long long frame_stride;
    int tpr, img_mode, win, n, min_obs;
};

// getInterpolatedElement33 (GlobalFuncs.h:89-103) of a resident frame (layout 3 or 1)
__device__ inline float3 sample33(const float4 *__restrict__ img, int mode, int tpr, long long frame_stride, float x,
                                  float y) {
#pragma clang fp contract(off)
    const int ix = (int)x, iy = (int)y;
    const float dx = x - ix, dy = y - iy;
    if (mode == 3) {
        float v[12];
        load12(frame_rsrc(reinterpret_cast<const float *>(img), frame_stride * 16), (unsigned)tpr * 128u, ix, iy, v);
        return bilin12(v, dx, dy);
    }
    const float dxdy = dx * dy;
    const float w11 = dxdy, w01 = dy - dxdy, w10 = dx - dxdy, w00 = 1 - dx - dy + dxdy;
    const float3 t00 = tex(img, tpr, ix, iy), t10 = tex(img, tpr, ix + 1, iy), t01 = tex(img, tpr, ix, iy + 1),
                 t11 = tex(img, tpr, ix + 1, iy + 1);
    return make_float3(w11 * t11.x + w01 * t01.x + w10 * t10.x + w00 * t00.x,
                       w11 * t11.y + w01 * t01.y + w10 * t10.y + w00 * t00.y,
                       w11 * t11.z + w01 * t01.z + w10 * t10.z + w00 * t00.z);
}

// Lanes per (residual, pattern pixel): lane 8 r' + idx evaluates pattern pixel idx of the
// temporary residual r = 8 round + r' (up to 8 residuals per round, two rounds for windows above
// 9 keyframes), so a residual's eight taps are sampled in parallel instead of one after another.
// The per-pixel terms go through the wave's LDS slot and every lane then folds them in the
// reference's order -- per residual the pixels up to its first OOB pixel, the residuals in window
// order -- so the point's energy, Hdd and bd, and every residual state, are wave-uniform and
// bit-identical to the CPU restatement.
constexpr int kActRes = 16;  // residual slots per point (N <= 16 -> at most 15)
struct ActLds {              // one wavefront's slot
    float e[kActRes][8], h[kActRes][8], b[kActRes][8];
    int first_oob[kActRes];  // pattern index of the first OOB pixel (8: none)
    float st_energy[kActRes], st_newenergy[kActRes];
    int st_state[kActRes], st_new[kActRes];
};
__global__ __launch_bounds__(256) void k_activate(ActParams P) {
#pragma clang fp contract(off)
    constexpr int pat[8][2] = {{0, -2}, {-1, -1}, {1, -1}, {-2, 0}, {0, 0}, {2, 0}, {-1, 1}, {0, 2}};
    constexpr float kMinIdepthHAct = 100;  // setting_minIdepthH_act, Setting.cc:25
    constexpr int kGNItsOnPointActivation = 3;  // Setting.cc:47
    __shared__ ActLds lds_act[4];
    const int lane = threadIdx.x & 63;
    const int k = __builtin_amdgcn_readfirstlane(blockIdx.x * 4 + (threadIdx.x >> 6));
    if (k >= P.n) return;
    ActLds &A = lds_act[threadIdx.x >> 6];
    const WinDev &W = P.wins[P.win];
    const ldso_ct_immature &ip = P.pts[k];
    const int N = W.N, host = ip.host, nres = N - 1, rounds = (nres + 7) >> 3;
    const float fxl = W.calib[0], fyl = W.calib[1], cxl = W.calib[2], cyl = W.calib[3];
    const float fxli = 1.0f / fxl, fyli = 1.0f / fyl;
    const float eth = ip.energy_th;
    const int idx = lane & 7;
    // this lane's pattern pixel in the host frame (ImmaturePoint.cc:336-343)
    const float K0 = (ip.u + pat[idx][0] - cxl) * fxli, K1 = (ip.v + pat[idx][1] - cyl) * fyli;
    const float col = ip.color[idx], wsq = ip.weights[idx] * ip.weights[idx];
    if (lane < kActRes) {  // ImmaturePointTemporaryResidual (ImmaturePoint.h:18-26) of slot lane
        A.st_state[lane] = LDSO_BA_RES_IN;
        A.st_new[lane] = LDSO_BA_RES_OUTLIER;
        A.st_energy[lane] = 0;
        A.st_newenergy[lane] = 0;
    }
    wave_lds_sync();

    // linearizeResidual(HCalib, slack, tmpRes, Hdd, bd, idepth) of every residual, then the
    // point's sums in the reference's order -> (energy, Hdd, bd), identical on every lane
    auto evaluate = [&](float slack, float idepth, float &E, float &Hdd, float &bd) {
        for (int rd = 0; rd < rounds; rd++) {
            const int r = 8 * rd + (lane >> 3);
            if (r < nres && A.st_state[r] != LDSO_BA_RES_OOB) {
                const int tgt = r + (r >= host);
                const float *pre = P.precalc + (size_t)(W.pair_base + host + N * tgt) * LDSO_BA_PRECALC_STRIDE;
                const float *R = pre + 27, *t = pre + 36;  // PRE_RTll, PRE_tTll (current poses)
                bool oob = false;
                float e = 0, h = 0, b = 0;
                float ptp[3];
#pragma unroll
                for (int i = 0; i < 3; i++) ptp[i] = (R[3 * i] * K0 + R[3 * i + 1] * K1 + R[3 * i + 2] * 1.0f) + t[i] * idepth;
                const float drescale = 1.0f / ptp[2];
                const float uu = ptp[0] * drescale, vv = ptp[1] * drescale;
                const float Ku = uu * fxl + cxl, Kv = vv * fyl + cyl;
                if (!(drescale > 0) || !(Ku > 1.1f && Kv > 1.1f && Ku < W.wM3 && Kv < W.hM3)) {
                    oob = true;
                } else {
                    const float4 *img = P.img + (size_t)(W.frame_base + tgt) * P.frame_stride;
                    const float3 hc = sample33(img, P.img_mode, P.tpr, P.frame_stride, Ku, Kv);
                    if (!isfinite(hc.x)) {
                        oob = true;
                    } else {
                        const float residual = hc.x - (pre[24] * col + pre[25]);
                        float hw = fabsf(residual) < kHuberTH ? 1 : kHuberTH / fabsf(residual);
                        e = wsq * hw * residual * residual * (2 - hw);
                        const float dxInterp = hc.y * fxl, dyInterp = hc.z * fyl;
                        const float d_idepth =
                            (dxInterp * drescale * (t[0] - t[2] * uu) + dyInterp * drescale * (t[1] - t[2] * vv)) *
                            kScaleIdepth;
                        hw *= wsq;
                        h = (hw * d_idepth) * d_idepth;
                        b = (hw * residual) * d_idepth;
                    }
                }
                A.e[r][idx] = e;
                A.h[r][idx] = h;
                A.b[r][idx] = b;
                const unsigned long long m = __ballot(oob);  // this round's OOB pixels
                if (idx == 0) {
                    const unsigned g = (unsigned)(m >> (8 * (lane >> 3))) & 0xFFu;
                    A.first_oob[r] = g ? __builtin_ctz(g) : 8;
                }
            } else {
                (void)__ballot(false);  // every lane takes part in the ballot
            }
        }
        wave_lds_sync();
        // the reference's order on every lane: residual by residual, pixel by pixel
        for (int r = 0; r < nres; r++) {
            float ret = A.st_energy[r];
            if (A.st_state[r] == LDSO_BA_RES_OOB) {
                if (lane == 0) A.st_new[r] = LDSO_BA_RES_OOB;
            } else {
                const int fo = A.first_oob[r];
                float energyLeft = 0;
                for (int i = 0; i < fo; i++) {
                    energyLeft += A.e[r][i];
                    Hdd += A.h[r][i];
                    bd += A.b[r][i];
                }
                int ns;
                if (fo < 8) {
                    ns = LDSO_BA_RES_OOB;
                } else {
                    if (energyLeft > eth * slack) {
                        energyLeft = eth * slack;
                        ns = LDSO_BA_RES_OUTLIER;
                    } else {
                        ns = LDSO_BA_RES_IN;
                    }
                    ret = energyLeft;
                    if (lane == 0) A.st_newenergy[r] = energyLeft;
                }
                if (lane == 0) A.st_new[r] = ns;
            }
            E = (float)((double)E + (double)ret);
        }
        wave_lds_sync();
    };
    auto commit = [&]() {
        if (lane < nres) {
            A.st_state[lane] = A.st_new[lane];
            A.st_energy[lane] = A.st_newenergy[lane];
        }
        wave_lds_sync();
    };

    float lastEnergy = 0, lastHdd = 0, lastbd = 0;
    float currentIdepth = (ip.idepth_max + ip.idepth_min) * 0.5f;
    evaluate(1000.f, currentIdepth, lastEnergy, lastHdd, lastbd);
    commit();
    int status = 0;
    if (!isfinite(lastEnergy) || lastHdd < kMinIdepthHAct) {
        status = 2;
    } else {
        float lambda = 0.1f;
        for (int iteration = 0; iteration < kGNItsOnPointActivation; iteration++) {
            float H = lastHdd;
            H *= 1 + lambda;
            const float step = (float)((1.0 / (double)H) * (double)lastbd);
            const float newIdepth = currentIdepth - step;
            float newHdd = 0, newbd = 0, newEnergy = 0;
            evaluate(1.f, newIdepth, newEnergy, newHdd, newbd);
            if (!isfinite(lastEnergy) || newHdd < kMinIdepthHAct) {
                status = 2;
                break;
            }
            if (newEnergy < lastEnergy) {
                currentIdepth = newIdepth;
                lastHdd = newHdd;
                lastbd = newbd;
                lastEnergy = newEnergy;
                commit();
                lambda *= 0.5f;
            } else {
                lambda = (float)((double)lambda * 5.0);
            }
            if ((double)fabsf(step) < 0.0001 * (double)currentIdepth) break;
        }
        if (status == 0 && !isfinite(currentIdepth)) status = 1;
    }
    unsigned mask = 0;
    if (status == 0) {
        const unsigned long long in = __ballot(lane < nres && A.st_state[lane] == LDSO_BA_RES_IN);
        if (__popcll(in) < P.min_obs) {
            status = 1;
        } else {
            for (int r = 0; r < nres; r++)
                if ((in >> r) & 1ull) mask |= 1u << (r + (r >= host));
        }
    }
    if (lane == 0) {
        ldso_ba_activation o;
        o.idepth = currentIdepth;
        o.status = status;
        o.in_mask = mask;
        o.energy = lastEnergy;
        P.out[k] = o;
    }
}

}  // namespace
