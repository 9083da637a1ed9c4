// k_lc_project.h -- the correspondence search of LoopClosing::ComputeOptimizedPose (LoopClosing.cc:323-398)
// with Frame::GetFeatureInGrid (Frame.cc:76-108) and Sophus' Sim(3) point action (rxso3.hpp:259-267,
// sim3.hpp:228-231), statement for statement:
//
//   pRef = (1.0 / invD) * Vec3(fxli * (u - cxl), fyli * (v - cyl), 1)   float products, the quotient and the
//                                                                       scaling in double
//   pc   = Scr * pRef                                                   double: scale * p + (w * t + vec x t),
//                                                                       t = 2 (vec x p), then + translation
//   x, y, u, v                                                          float
//   GetFeatureInGrid(u, v, windowSize)   its four early returns, int(x - radius) / 20 truncating toward zero,
//                                        the cells ix outer, iy inner, a cell in ascending feature index,
//                                        the float distance test against radius^2
//   fabsf(angle - angle) < 0.2           a float difference compared in double
//   idepthMap[int(v + 0.5f) * w + int(u + 0.5f)] == 0: skipped
//   best by strict <                     a thread walks its candidate's partners in the reference's order, so
//                                        the winner is the minimum of (dist, ix, iy, index in cell)
//   pcurr = (1.0f / idepth) * (Ki * Vec3(u, v, 1))   the float quotient widened, Ki in double from the float
//                                                    inverses, a row's dot product as (a0 b0 + a1 b1) + a2 b2
//
// scale = squaredNorm of the quaternion's (x, y, z, w) as Eigen's packet reduction of four doubles adds it:
// (x^2 + z^2) + (y^2 + w^2).
//
// This library's rules where the reference is undefined: a float -> int conversion of a value that is not
// finite or does not fit gives INT_MIN (lc_to_int), which makes GetFeatureInGrid return nothing; a NaN
// angle fails the gate; a map lookup outside the image (a corner within half a pixel of the right or lower
// border of the grid) reads 0.  The accepted candidates are compacted in candidate order by ballot prefix:
// one block, no atomics.
#pragma once
#include "k_lc_common.h"

#pragma clang fp contract(off)

namespace {

struct LcProjParams {
    LcStore S;
    const float *__restrict__ map;  // [w * h]
    int slot_cur, slot_cand, n_cand, th_high;
    float calib[8];                 // fxl, fyl, cxl, cyl, fxli, fyli, cxli, cyli
    double scr[7];                  // quaternion x, y, z, w; translation
    float window_size;
    ldso_lc_projection *__restrict__ out;  // [n_cand]
    int *__restrict__ count;               // mapped host memory
};

__device__ __forceinline__ float lc_map_at(const float *map, float fu, float fv, int w, int h) {
    const int ui = lc_to_int(fu + 0.5f), vi = lc_to_int(fv + 0.5f);
    if (ui < 0 || vi < 0 || ui >= w || vi >= h) return 0.0f;
    return map[(size_t)vi * w + ui];
}

__global__ __launch_bounds__(kLcThreads) void k_lc_project(LcProjParams P) {
    const LcStore &S = P.S;
    const ldso_lc_feature *cur = S.feat + (size_t)P.slot_cur * S.F, *cand = S.feat + (size_t)P.slot_cand * S.F;
    const int *cell_begin = S.cell_begin + (size_t)P.slot_cur * (S.cells + 1);
    const int *cell_feat = S.cell_feat + (size_t)P.slot_cur * S.F;
    const float fxl = P.calib[0], fyl = P.calib[1], cxl = P.calib[2], cyl = P.calib[3];
    const float fxli = P.calib[4], fyli = P.calib[5], cxli = P.calib[6], cyli = P.calib[7];
    const double qx = P.scr[0], qy = P.scr[1], qz = P.scr[2], qw = P.scr[3];
    const int gw = S.gw, gh = S.gh;
    int n = 0;
    for (int i0 = 0; i0 < P.n_cand; i0 += kLcThreads) {
        const int i = i0 + threadIdx.x;
        bool ok = false;
        ldso_lc_projection o;
        if (i < P.n_cand && cand[i].usable != 0) {
            const ldso_lc_feature &p = cand[i];
            // :337-347
            const double s = 1.0 / (double)p.inv_d;
            const float ax = fxli * (p.u - cxl), ay = fyli * (p.v - cyl);
            const double r0 = s * (double)ax, r1 = s * (double)ay, r2 = s * 1.0;
            const double scale = (qx * qx + qz * qz) + (qy * qy + qw * qw);
            double t0 = qy * r2 - qz * r1, t1 = qz * r0 - qx * r2, t2 = qx * r1 - qy * r0;
            t0 += t0;
            t1 += t1;
            t2 += t2;
            const double c0 = qy * t2 - qz * t1, c1 = qz * t0 - qx * t2, c2 = qx * t1 - qy * t0;
            const double pc0 = (scale * r0 + (qw * t0 + c0)) + P.scr[4];
            const double pc1 = (scale * r1 + (qw * t1 + c1)) + P.scr[5];
            const double pc2 = (scale * r2 + (qw * t2 + c2)) + P.scr[6];
            const float x = (float)(pc0 / pc2), y = (float)(pc1 / pc2);
            const float u = fxl * x + cxl, v = fyl * y + cyl;
            int best = 256, best2 = 256, best_idx = -1;
            // GetFeatureInGrid(u, v, windowSize)
            const float radius = P.window_size;
            bool any = true;
            const int gx_min = max(0, lc_to_int(u - radius) / kLcGrid);
            if (gx_min >= gw) any = false;
            const int gx_max = min(gw - 1, lc_to_int(u + radius) / kLcGrid);
            if (gx_max < 0) any = false;
            const int gy_min = max(0, lc_to_int(v - radius) / kLcGrid);
            if (gy_min >= gh) any = false;
            const int gy_max = min(gh - 1, lc_to_int(v + radius) / kLcGrid);
            if (gy_max < 0) any = false;
            const float rr = radius * radius;
            if (any)
                for (int ix = gx_min; ix <= gx_max; ix++)
                    for (int iy = gy_min; iy <= gy_max; iy++) {
                        const int cell = iy * gw + ix;
                        for (int q = cell_begin[cell]; q < cell_begin[cell + 1]; q++) {
                            const int k = cell_feat[q];
                            const ldso_lc_feature &f = cur[k];
                            if (!(((f.u - u) * (f.u - u) + (f.v - v) * (f.v - v)) < rr)) continue;
                            if (!((double)fabsf(f.angle - p.angle) < 0.2)) continue;
                            const int d = lc_distance(f, p);
                            if (lc_map_at(P.map, f.u, f.v, S.w, S.h) == 0.0f) continue;
                            if (d < best) {
                                best2 = best;
                                best = d;
                                best_idx = k;
                            } else if (d < best2) {
                                best2 = d;
                            }
                        }
                    }
            if (best <= P.th_high && best_idx >= 0) {
                const ldso_lc_feature &f = cur[best_idx];
                const float idepth = lc_map_at(P.map, f.u, f.v, S.w, S.h);
                const double inv = (double)(1.0f / idepth);
                const double bu = (double)f.u, bv = (double)f.v;
                const double k0 = ((double)fxli * bu + 0.0 * bv) + (double)cxli * 1.0;
                const double k1 = (0.0 * bu + (double)fyli * bv) + (double)cyli * 1.0;
                const double k2 = (0.0 * bu + 0.0 * bv) + 1.0 * 1.0;
                ok = true;
                o.index_cand = i;
                o.index_cur = best_idx;
                o.dist = best;
                o.reserved_ = 0;
                o.p_ref[0] = r0;
                o.p_ref[1] = r1;
                o.p_ref[2] = r2;
                o.p_curr[0] = inv * k0;
                o.p_curr[1] = inv * k1;
                o.p_curr[2] = inv * k2;
                o.pixel[0] = bu;
                o.pixel[1] = bv;
            }
        }
        int total;
        const int pre = lc_block_prefix(ok, &total);
        if (ok) P.out[n + pre] = o;
        n += total;
    }
    if (threadIdx.x == 0) *P.count = n;
}

}  // namespace
