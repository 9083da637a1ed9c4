// ct_init.h -- CoarseInitializer::trackFrame (CoarseInitializer.cc:45-183) for host and device, as
// ct_lm.h is for trackNewestCoarse (FP contraction off): the float LDLT, one LM step (:95-116), the
// constants of an evaluation that the pose fixes (:195-203, :260, :336), and the decisions the loop takes
// from the sums (:125-156).  k_ct_init.h runs them in one lane of a workgroup; ldso_ct_init_lm_step is
// the step's host instantiation.
//
// Accumulator9::finish (MatrixAccumulators.h:1121-1135) writes H(r, c) = H(c, r) = d: both triangles of
// acc9's and acc9SC's H are filled, Mat88f Hl = H is symmetric, and Hl.ldlt() -- LDLT<., Lower>, which
// reads the lower triangle -- factorises the full system.  (The coarse tracker's Hl is another case:
// DESIGN §9c.)
//
// Types follow the reference: H, b, lambda, the increment and AffLight's a, b are float, poses double.
#pragma once
#include <math.h>

#include "../../include/ldso_ct.h"
#include "ct_lm.h"

namespace ldso_ct {

constexpr int kInitMaxIterations = 1000;  // per level: what ldso_ct_init_track_frame accepts
constexpr int kInitMaxLevels = 5;         // maxIterations[] has five entries (:48)

// wM's diagonal (:29-32): SCALE_XI_ROT x3, SCALE_XI_TRANS x3, SCALE_A, SCALE_B
LDSO_HD inline float init_wm(int i) { return i < 3 ? 1.0f : (i < 6 ? 0.5f : (i == 6 ? 10.0f : 1000.0f)); }

// Eigen's fixed-size float reductions over 8 entries, in the order of its SSE packets: two packets
// multiplied and added lane by lane, then predux's (p0 + p2) + (p1 + p3)
LDSO_HD inline float init_dot8(const float *a, const float *b) {
#pragma clang fp contract(off)
    float p[4];
    for (int k = 0; k < 4; k++) p[k] = a[k] * b[k] + a[k + 4] * b[k + 4];
    return (p[0] + p[2]) + (p[1] + p[3]);
}
LDSO_HD inline float init_norm8(const float *a) { return sqrtf(init_dot8(a, a)); }

struct LdltWorkF {
    float A[64], col[8], y[8], rhs[8];
    int perm[8];
};
// ct_lm.h's ldlt_solve_small (Eigen::LDLT's pivoting, the lower triangle only) in float
LDSO_HD inline void ldlt_solve_small_f(int n, LdltWorkF &W, float *b) {
#pragma clang fp contract(off)
    float *a = W.A;
    for (int i = 0; i < n; i++) W.perm[i] = i;
    for (int k = 0; k < n; k++) {
        int piv = k;
        for (int i = k + 1; i < n; i++)
            if (fabsf(a[i * n + i]) > fabsf(a[piv * n + piv])) piv = i;
        if (piv != k) {
            float t;
            const int pt = W.perm[k];
            W.perm[k] = W.perm[piv];
            W.perm[piv] = pt;
#define LDSO_CT_SWAP(x, y) (t = (x), (x) = (y), (y) = t)
            for (int j = 0; j < k; j++) LDSO_CT_SWAP(a[k * n + j], a[piv * n + j]);
            for (int i = k + 1; i < piv; i++) LDSO_CT_SWAP(a[i * n + k], a[piv * n + i]);
            for (int i = piv + 1; i < n; i++) LDSO_CT_SWAP(a[i * n + k], a[i * n + piv]);
            LDSO_CT_SWAP(a[k * n + k], a[piv * n + piv]);
#undef LDSO_CT_SWAP
        }
        const float d = a[k * n + k];
        const float rd = d != 0 ? 1.0f / d : 0.0f;
        for (int i = k + 1; i < n; i++) W.col[i] = a[i * n + k];
        for (int i = k + 1; i < n; i++) {
            const float ci = W.col[i];
            float *row = a + i * n;
            for (int j = k + 1; j <= i; j++) row[j] = fmaf(-(ci * W.col[j]), rd, row[j]);
            row[k] = d != 0 ? ci / d : 0.0f;
        }
    }
    float *y = W.y;
    for (int i = 0; i < n; i++) y[i] = b[W.perm[i]];
    for (int i = 0; i < n; i++)
        for (int j = 0; j < i; j++) y[i] = fmaf(-a[i * n + j], y[j], y[i]);
    for (int i = 0; i < n; i++) y[i] = a[i * n + i] != 0 ? y[i] / a[i * n + i] : 0.0f;
    for (int j = n - 1; j >= 0; j--)
        for (int i = 0; i < j; i++) y[i] = fmaf(-a[j * n + i], y[j], y[i]);
    for (int i = 0; i < n; i++) b[W.perm[i]] = y[i];
}

// :95-116.  Hl = H with (1 + lambda) on the diagonal, minus Hsc / (1 + lambda); bl likewise; both scaled
// by wM and 0.01f / (w * h), coefficient by coefficient as Eigen evaluates the diagonal products; the
// 6x6 corner with fixAffine; inc = -(wM x); exp(inc.head<6>().cast<double>()) * cur; a, b += inc[6], [7].
LDSO_HD inline void init_lm_step(const float *H, const float *b, const float *Hsc, const float *bsc, float lambda,
                                 int w, int h, const Pose &cur, const float aff[2], const ldso_ct_init_params &p,
                                 LdltWorkF &W, float inc[8], Pose &cand, float aff_new[2]) {
#pragma clang fp contract(off)
    const float dl = 1 + lambda, sl = 1 / (1 + lambda), s = 0.01f / (float)(w * h);
    const int n = p.fix_affine ? 6 : 8;
    float *bl = W.rhs;
    for (int i = 0; i < n; i++) {
        for (int j = 0; j <= i; j++) {
            float v = H[8 * i + j];
            if (i == j) v = v * dl;
            v = v - Hsc[8 * i + j] * sl;
            W.A[i * n + j] = ((init_wm(i) * v) * init_wm(j)) * s;
        }
        bl[i] = (init_wm(i) * (b[i] - bsc[i] * sl)) * s;
    }
    ldlt_solve_small_f(n, W, bl);
    for (int i = 0; i < 8; i++) inc[i] = i < n ? -(init_wm(i) * bl[i]) : 0.0f;
    double a6[6];
    for (int i = 0; i < 6; i++) a6[i] = (double)inc[i];
    cand = Pose::exp(a6, SharedSinCos()) * cur;
    aff_new[0] = aff[0] + inc[6];
    aff_new[1] = aff[1] + inc[7];
}

// Pose::from_matrix (se3.h: Eigen's Quaternion(Matrix3)) with the branch on the largest diagonal entry
// written out per case, so that no array is indexed at run time (on the device that would be private
// memory): the same statements, the same bits
template <int I>
LDSO_HD inline void init_quat_case(const double *R, double *q) {
#pragma clang fp contract(off)
    constexpr int J = (I + 1) % 3, K = (J + 1) % 3;
    double tt = sqrt(((R[I * 4] - R[J * 4]) - R[K * 4]) + 1.0);
    q[I] = 0.5 * tt;
    tt = 0.5 / tt;
    q[3] = (R[K * 3 + J] - R[J * 3 + K]) * tt;
    q[J] = (R[J * 3 + I] + R[I * 3 + J]) * tt;
    q[K] = (R[K * 3 + I] + R[I * 3 + K]) * tt;
}
LDSO_HD inline Pose init_pose_from_matrix(const double T[12]) {
#pragma clang fp contract(off)
    const double R[9] = {T[0], T[1], T[2], T[4], T[5], T[6], T[8], T[9], T[10]};
    Pose p;
    double tt = (R[0] + R[4]) + R[8];
    if (tt > 0) {
        tt = sqrt(tt + 1.0);
        p.q[3] = 0.5 * tt;
        tt = 0.5 / tt;
        p.q[0] = (R[7] - R[5]) * tt;
        p.q[1] = (R[2] - R[6]) * tt;
        p.q[2] = (R[3] - R[1]) * tt;
    } else if (R[8] > (R[4] > R[0] ? R[4] : R[0])) {
        init_quat_case<2>(R, p.q);
    } else if (R[4] > R[0]) {
        init_quat_case<1>(R, p.q);
    } else {
        init_quat_case<0>(R, p.q);
    }
    p.t[0] = T[3];
    p.t[1] = T[7];
    p.t[2] = T[11];
    return p;
}

// makeK's Ki (:811-837): K in double from the float calibration of the level, Eigen's cofactor inverse
LDSO_HD inline void init_make_ki(double fx, double fy, double cx, double cy, double Ki[9]) {
#pragma clang fp contract(off)
    const double invdet = 1.0 / (fy * fx);
    Ki[0] = fy * invdet;
    Ki[1] = 0 * invdet;
    Ki[2] = (0 * cy - cx * fy) * invdet;
    Ki[3] = 0 * invdet;
    Ki[4] = fx * invdet;
    Ki[5] = (cx * 0 - fx * cy) * invdet;
    Ki[6] = 0 * invdet;
    Ki[7] = 0 * invdet;
    Ki[8] = (fx * fy - 0 * 0) * invdet;
}

// what calcResAndGS derives from the pose before it looks at a point (:195-197, :260, :336)
struct InitEval {
    float RKi[9], t[3], r2a, r2b, tlog[3];
    double tsq;  // refToNew.translation().squaredNorm()
};
LDSO_HD inline void init_eval_setup(const double T[12], const float aff[2], const double Ki[9], InitEval &E) {
#pragma clang fp contract(off)
    for (int i = 0; i < 3; i++) {
        for (int j = 0; j < 3; j++)
            E.RKi[3 * i + j] = (float)((T[4 * i] * Ki[j] + T[4 * i + 1] * Ki[3 + j]) + T[4 * i + 2] * Ki[6 + j]);
        E.t[i] = (float)T[4 * i + 3];
    }
    E.tsq = (T[3] * T[3] + T[7] * T[7]) + T[11] * T[11];
    E.r2a = ldso_ba::exp_float(aff[0]);
    E.r2b = aff[1];
    double xi[6];
    init_pose_from_matrix(T).log(xi);
    for (int i = 0; i < 3; i++) E.tlog[i] = (float)xi[i];
}

// :260-281 from accEAlpha's sum: the alpha energy, capped or not; returns alphaOpt
LDSO_HD inline float init_alpha(double tsq, float accEAlpha, int npts, const ldso_ct_init_params &p, float &alphaEnergy) {
#pragma clang fp contract(off)
    alphaEnergy = (float)(tsq * npts);
    alphaEnergy = alphaEnergy + accEAlpha;
    alphaEnergy = alphaEnergy * p.alpha_w;
    if (alphaEnergy > p.alpha_k * npts) {
        alphaEnergy = p.alpha_k * npts;
        return 0;
    }
    return p.alpha_w;
}

// :125-129
LDSO_HD inline bool init_accept(const float resOld[3], const float resNew[3], const float regEnergy[3]) {
#pragma clang fp contract(off)
    const float eTotalNew = (resNew[0] + resNew[1] + regEnergy[1]);
    const float eTotalOld = (resOld[0] + resOld[1] + regEnergy[0]);
    return eTotalOld > eTotalNew;
}

}  // namespace ldso_ct
