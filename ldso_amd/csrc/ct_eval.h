// ct_eval.h -- what one calcRes + calcGSSSE evaluation (CoarseTracker.cc:540-741) takes and leaves, one
// text for host and device (as se3.h, FP contraction off):
//   CtLevel       a pyramid level as the kernels read it: the reference cloud, the new frame, the intrinsics
//   ct_eval_setup the per-evaluation constants from a 3x4 pose and an affine pair: CtPose (R K^-1, t, aLL,
//                 bLL) and CtEvalTerms (calcGSSSE's a and b0, the cutoff and the energy of a saturated residual)
//   ct_finish_res, ct_finish_gs_entry   the Vec6 from the kResParts sums; one entry of the scaled H / b from
//                 the kGsParts sums and the warped count
// ldso_ct.hip's entry points run them on the host around k_ct_calc_res / k_ct_calc_gs, k_ct_track on the
// device between two sweeps: the same functions, so the one-launch loop and a host loop over the ABI see
// the same constants and scale the same sums in the same order.
#pragma once
#include <hip/hip_vector_types.h>

#include "se3.h"

namespace ldso_ct {

constexpr int kResParts = 8;   // E, nE, nSat, shiftT, shiftRT, shiftNum, nWarped, pad
constexpr int kGsParts = 45;   // upper 9x9 of Accumulator9

// SCALE_XI_TRANS x3, SCALE_XI_ROT x3, SCALE_A, SCALE_B (Settings.h:29-35): the float factors of calcGSSSE's
// H, b and of the LM step's increment (ct_lm.h)
constexpr float kCtScale[8] = {(float)ldso_ba::kScaleXiTrans, (float)ldso_ba::kScaleXiTrans, (float)ldso_ba::kScaleXiTrans,
                               (float)ldso_ba::kScaleXiRot,   (float)ldso_ba::kScaleXiRot,   (float)ldso_ba::kScaleXiRot,
                               (float)ldso_ba::kScaleA,       (float)ldso_ba::kScaleB};

struct CtLevel {
    const float4 *__restrict__ pc;   // (u, v, idepth, color) of this level's points
    const float4 *__restrict__ img;  // this level of the new frame
    int n, wl, hl;
    float fxl, fyl, cxl, cyl, Ki[9];
};
struct CtPose {  // per hypothesis, in the reference's float arithmetic
    float RKi[9], t[3], aLL, bLL, pad[2];
};
struct CtEvalTerms {
    float gs_a, gs_b0, cutoffTH, maxEnergy;
};

// calcRes' per-hypothesis constants (CoarseTracker.cc:555-558, 565-566) and calcGSSSE's affine pair
// (:683-687: a = the float of fromToVecExposure's aLL, b0 = the reference's b).  T: ref_to_new, 3x4 row-major.
LDSO_HD inline void ct_eval_setup(const double *T, const float *Ki, float ref_exposure, float new_exposure, float ref_a,
                                  float ref_b, float aff_a, float aff_b, float cutoffTH, CtPose &p, CtEvalTerms &e) {
#pragma clang fp contract(off)
    float R[9], t[3];
    for (int i = 0; i < 3; i++) {
        for (int j = 0; j < 3; j++) R[3 * i + j] = (float)T[4 * i + j];
        t[i] = (float)T[4 * i + 3];
    }
    for (int i = 0; i < 3; i++)
        for (int j = 0; j < 3; j++)
            p.RKi[3 * i + j] = R[3 * i] * Ki[j] + R[3 * i + 1] * Ki[3 + j] + R[3 * i + 2] * Ki[6 + j];
    for (int i = 0; i < 3; i++) p.t[i] = t[i];
    ldso_ba::affine_from_to(ref_exposure, new_exposure, ref_a, ref_b, aff_a, aff_b, p.aLL, p.bLL);
    p.pad[0] = p.pad[1] = 0;
    e.gs_a = (float)(double)p.aLL;
    e.gs_b0 = ref_b;
    e.cutoffTH = cutoffTH;
    e.maxEnergy = 2 * ldso_ba::kHuberTH * cutoffTH - ldso_ba::kHuberTH * ldso_ba::kHuberTH;
}

// Vec6 of CoarseTracker.cc:662-670 from the kResParts sums; E and the shift sums are floats in the reference
LDSO_HD inline void ct_finish_res(const double *s, double rs[6]) {
#pragma clang fp contract(off)
    const float E = (float)s[0], sT = (float)s[3], sRT = (float)s[4], sNum = (float)s[5];
    const int nE = (int)s[1], nSat = (int)s[2];
    rs[0] = E;
    rs[1] = nE;
    rs[2] = sT / (sNum + 0.1);
    rs[3] = 0;
    rs[4] = sRT / (sNum + 0.1);
    rs[5] = nSat / (float)nE;
}

// Accumulator9::finish + CoarseTracker.cc:725-740: entry (r, cc) of the scaled 8x8 H, or b[r] for cc = 8, from
// the kGsParts sums g (upper triangle, row-major) and the count of warped points
LDSO_HD inline double ct_finish_gs_entry(const double *g, int n_warped, int r, int cc) {
#pragma clang fp contract(off)
    const int lo = r < cc ? r : cc, hi = r < cc ? cc : r;
    const float Hrc = (float)g[lo * 9 - lo * (lo - 1) / 2 + (hi - lo)];
    const int nw = (n_warped + 3) / 4 * 4;  // buf_warped_n (padded to a multiple of 4)
    const double inv_n = (double)(1.0f / nw);
    return cc < 8 ? (double)Hrc * inv_n * kCtScale[cc] * kCtScale[r] : (double)Hrc * inv_n * kCtScale[r];
}

}  // namespace ldso_ct
