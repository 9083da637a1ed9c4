// ct_lm.h -- trackNewestCoarse's LM loop (CoarseTracker.cc:61-310) on the visual-only path, for host
// and device (as se3.h, FP contraction off): the 8x8 solve, one LM step, and the loop itself as a
// state machine that is fed one calcRes / calcGSSSE evaluation at a time.  k_ct_track.h runs it in
// one lane of a workgroup; ldso_ct_lm_step is the step's host instantiation.
//
// With setting_vi_enable false InertialCoarseTrackerHessian::compute leaves energy = 0 and H_I,
// H_I_sc, b_I_sc zero (InertialCoarseTrackerHessian.cc:78-83); b_I is zero from its initialiser and
// only written inside the same `if`; Hbb (15x15), Hab (8x15) and bb (15) keep their zero
// initialisers, and update / restore return at once.  So bl = -b, resIOld = resINew = 0, and the 15
// extra rows of Hl (setting_vi_use_schur_complement false) are zero rows with a zero right-hand
// side, whose increments Eigen's LDLT sets to zero: the 8x8 system is all that is left.
//
// Types follow the reference: lambda, extrapFac, levelCutoffRepeat and AffLight's a, b are float
// (the ABI widens them), poses and the increment double.  sqrt(limit / lambda) has a float
// argument under a using-directive for std (InertialCoarseTrackerHessian.h:5), hence sqrtf.
#pragma once
#include <float.h>
#include <math.h>

#include "../../include/ldso_ct.h"
#include "ct_eval.h"
#include "se3.h"

namespace ldso_ct {

using ldso_ba::Pose;

constexpr float kLambdaExtrapolationLimit = 0.001f;  // CoarseTracker.cc:74
constexpr int kTrackMaxIterations = 1000;            // per level: what ldso_ct_track accepts

// The sine and cosine of SE3::exp in the LM step, one text for host and device.  glibc's and the device
// library's sin / cos differ in the last bit now and then, and R(q)'s entries that cancel (tyz - twx) turn one
// ulp of the quaternion into tens of their own: with libm the device loop and ldso_ct_lm_step part ways on large
// steps (32 ulp in one rotation entry, measured).  Here both run the same IEEE statements: Cody-Waite
// reduction by pi/2 in four exact pieces (fdlibm's split, good to 2^-160) and the Taylor series with the
// leading terms in double-double, so the result is the correctly rounded one up to an error near 1e-4 ulp,
// which is also what glibc returns in all but rare cases.  |x| >= 1e5 or not finite: libm.
struct DD {
    double hi, lo;
};
LDSO_HD inline DD dd_fast(double a, double b) {  // |a| >= |b|
#pragma clang fp contract(off)
    const double s = a + b;
    return {s, b - (s - a)};
}
LDSO_HD inline DD dd_sum(double a, double b) {
#pragma clang fp contract(off)
    const double s = a + b, bb = s - a;
    return {s, (a - (s - bb)) + (b - bb)};
}
LDSO_HD inline DD dd_add(DD a, DD b) {
#pragma clang fp contract(off)
    const DD s = dd_sum(a.hi, b.hi);
    return dd_fast(s.hi, s.lo + (a.lo + b.lo));
}
LDSO_HD inline DD dd_mul(DD a, DD b) {
#pragma clang fp contract(off)
    const double p = a.hi * b.hi, e = fma(a.hi, b.hi, -p);
    return dd_fast(p, e + (a.hi * b.lo + a.lo * b.hi));
}
struct SharedSinCos {
    LDSO_HD void operator()(double x, double &s, double &c) const {
#pragma clang fp contract(off)
        if (!(fabs(x) < 1e5)) return sin_cos(x, s, c);
        const double fn = rint(x * 0x1.45f306dc9c883p-1);  // 2 / pi
        // fn times each of the first three pieces is exact (33 bits by 17)
        DD r = dd_sum(x, -(fn * 0x1.921FB54400000p+0));
        r = dd_add(r, DD{-(fn * 0x1.0B4611A600000p-34), 0});
        r = dd_add(r, DD{-(fn * 0x1.3198A2E000000p-69), 0});
        r = dd_add(r, DD{-(fn * 0x1.B839A252049C1p-104), 0});
        const DD z = dd_mul(r, r);
        const double y = z.hi;
        // the series' tails in double: their error is below 1e-20 of the result
        const double ts = -0.0001984126984126984 + y * (2.7557319223985893e-06 + y * (-2.505210838544172e-08 + y * (1.6059043836821613e-10 +
                          y * (-7.647163731819816e-13 + y * (2.8114572543455206e-15 + y * (-8.22063524662433e-18 +
                          y * (1.9572941063391263e-20 + y * -3.868170170630684e-23)))))));
        const double tc = 2.48015873015873e-05 + y * (-2.755731922398589e-07 + y * (2.08767569878681e-09 + y * (-1.1470745597729725e-11 +
                          y * (4.779477332387385e-14 + y * (-1.5619206968586225e-16 + y * (4.110317623312165e-19 +
                          y * (-8.896791392450574e-22 + y * 1.6117375710961184e-24)))))));
        // sin r = r + r z (S3 + z (S5 + z ts)), cos r = 1 + z (-1/2 + z (C4 + z (C6 + z tc)))
        DD q = dd_add(DD{0x1.1111111111111p-7, 0x1.1111111111111p-63}, dd_mul(z, DD{ts, 0}));
        q = dd_add(DD{-0x1.5555555555555p-3, -0x1.5555555555555p-57}, dd_mul(z, q));
        const DD sr = dd_add(r, dd_mul(dd_mul(r, z), q));
        DD w = dd_add(DD{-0x1.6c16c16c16c17p-10, 0x1.f49f49f49f49fp-65}, dd_mul(z, DD{tc, 0}));
        w = dd_add(DD{0x1.5555555555555p-5, 0x1.5555555555555p-59}, dd_mul(z, w));
        w = dd_add(DD{-0.5, 0}, dd_mul(z, w));
        const DD cr = dd_add(DD{1.0, 0}, dd_mul(z, w));
        const int n = (int)fn & 3;
        s = n == 0 ? sr.hi : n == 1 ? cr.hi : n == 2 ? -sr.hi : -cr.hi;
        c = n == 0 ? cr.hi : n == 1 ? -sr.hi : n == 2 ? -cr.hi : sr.hi;
    }
};

struct LdltWork {
    double A[64], col[8], y[8];
    int perm[8];
};

// host_math.cpp's ldlt_solve (Eigen::LDLT's pivoting, the lower triangle only) for n <= 8: W.A row-major
// [n][n], b in and out
LDSO_HD inline void ldlt_solve_small(int n, LdltWork &W, double *b) {
#pragma clang fp contract(off)
    double *a = W.A;
    for (int i = 0; i < n; i++) W.perm[i] = i;
    for (int k = 0; k < n; k++) {
        int piv = k;
        for (int i = k + 1; i < n; i++)
            if (fabs(a[i * n + i]) > fabs(a[piv * n + piv])) piv = i;
        if (piv != k) {
            double t;
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
        const double d = a[k * n + k];
        const double rd = d != 0 ? 1.0 / d : 0.0;
        for (int i = k + 1; i < n; i++) W.col[i] = a[i * n + k];
        for (int i = k + 1; i < n; i++) {
            const double ci = W.col[i];
            double *row = a + i * n;
            for (int j = k + 1; j <= i; j++) row[j] = fma(-(ci * W.col[j]), rd, row[j]);
            row[k] = d != 0 ? ci / d : 0.0;
        }
    }
    double *y = W.y;
    for (int i = 0; i < n; i++) y[i] = b[W.perm[i]];
    for (int i = 0; i < n; i++)
        for (int j = 0; j < i; j++) y[i] = fma(-a[i * n + j], y[j], y[i]);
    for (int i = 0; i < n; i++) y[i] = a[i * n + i] != 0 ? y[i] / a[i * n + i] : 0.0;
    for (int j = n - 1; j >= 0; j--)
        for (int i = 0; i < j; i++) y[i] = fma(-a[j * n + i], y[j], y[i]);
    for (int i = 0; i < n; i++) b[W.perm[i]] = y[i];
}

// CoarseTracker.cc:130-184 with bl = -b: Hl = H with (1 + lambda) on the diagonal, and the sub-system
// of the affine mode -- 8x8; 6x6 (a, b fixed); 7x7 (b fixed); the stitched 7x7 (a fixed: row and
// column 7 take the place of 6) -- solved once.  The reference solves the 8x8 system first and then
// overwrites its result; nothing else reads it.
//   FULL       the symmetric system, the lower triangle of H as upstream's Mat88 Hl = H; Hl.ldlt()
//   REFERENCE  this fork fills only the upper triangle of a zero Hl, and LDLT<., Lower> reads only
//              the lower one: D = diag(Hl), L = I, inc_i = bl_i / Hl_ii, and 0 where |Hl_ii| is not
//              above 1 / highest (LDLT::_solve_impl's tolerance)
LDSO_HD inline void lm_increment(const double *H, const double *b, float lambda, const ldso_ct_track_params &p,
                                 LdltWork &W, double inc[8]) {
#pragma clang fp contract(off)
    const bool fix_a = p.affine_opt_mode_a < 0, fix_b = p.affine_opt_mode_b < 0;
    const int n = fix_a && fix_b ? 6 : (fix_a || fix_b ? 7 : 8);
    int idx[8];
    for (int i = 0; i < 8; i++) idx[i] = i;
    if (fix_a && !fix_b) idx[6] = 7;
    const double dl = (double)(1 + lambda);  // Hl(i, i) *= (1 + lambda), a float sum
    double rhs[8];
    for (int i = 0; i < n; i++) {
        rhs[i] = -b[idx[i]];
        for (int j = 0; j <= i; j++) W.A[i * n + j] = H[idx[i] * 8 + idx[j]];
        W.A[i * n + i] = W.A[i * n + i] * dl;
    }
    if (p.solve == LDSO_CT_TRACK_SOLVE_REFERENCE) {
        for (int i = 0; i < n; i++) {
            const double d = W.A[i * n + i];
            rhs[i] = fabs(d) > 1.0 / DBL_MAX ? rhs[i] / d : 0.0;
        }
    } else {
        ldlt_solve_small(n, W, rhs);
    }
    for (int i = 0; i < 8; i++) inc[i] = 0;
    for (int i = 0; i < n; i++) inc[idx[i]] = rhs[i];
}

// CoarseTracker.cc:186-213: extrapolation, SCALE_*, the non-finite guard, exp(incScaled) * pose and the
// affine update.  inc: the unscaled increment after extrapolation (what line 263 takes the norm of).
LDSO_HD inline void lm_step(const double *H, const double *b, float lambda, const Pose &cur, const float aff[2],
                            const ldso_ct_track_params &p, LdltWork &W, double inc[8], Pose &cand, float aff_new[2]) {
#pragma clang fp contract(off)
    lm_increment(H, b, lambda, p, W, inc);
    float extrapFac = 1;
    if (lambda < kLambdaExtrapolationLimit) extrapFac = sqrtf(sqrtf(kLambdaExtrapolationLimit / lambda));
    double incScaled[8], sq = 0;
    for (int i = 0; i < 8; i++) {
        inc[i] = inc[i] * extrapFac;
        incScaled[i] = inc[i] * kCtScale[i];  // SCALE_XI_TRANS, _ROT, _A, _B
        sq = sq + incScaled[i] * incScaled[i];
    }
    if (!isfinite(sq))
        for (int i = 0; i < 8; i++) inc[i] = incScaled[i] = 0;
    cand = Pose::exp(incScaled, SharedSinCos()) * cur;
    aff_new[0] = (float)(aff[0] + incScaled[6]);  // AffLight's members are float
    aff_new[1] = (float)(aff[1] + incScaled[7]);
}

LDSO_HD inline void pose_matrix(const Pose &T, double out[12]) {
    const ldso_ba::Mat3 R = T.rotation_matrix();
    for (int i = 0; i < 3; i++) {
        for (int j = 0; j < 3; j++) out[4 * i + j] = R(i, j);
        out[4 * i + 3] = T.t[i];
    }
}
LDSO_HD inline Pose pose_from_matrix(const double T[12]) {
    const double R[9] = {T[0], T[1], T[2], T[4], T[5], T[6], T[8], T[9], T[10]}, t[3] = {T[3], T[7], T[11]};
    return Pose::from_matrix(R, t);
}

// The loop.  begin(), then while (more): evaluate calcRes + calcGSSSE at (lvl, cutoff(), eval_pose,
// eval_aff) and hand the Vec6, H and b to consume(), which returns whether another evaluation follows.
struct Track {
    ldso_ct_track_params p;
    double min_res[5], pose_in[12];
    float ref_exposure, new_exposure, ref_a, ref_b, aff_in[2];
    Pose cur, cand;        // cur: the quaternion of cur_pose, Eigen's Quaternion(Matrix3)
    double cur_pose[12];   // the accepted pose as the matrix that was evaluated
    float aff_cur[2], aff_new[2];
    int lvl, iteration, phase;  // phase 0: the level's initial / cutoff-doubling evaluations, 1: an LM step's
    float lambda, lambda_used, repeat;
    bool have_repeated;
    double res_old[6], H[64], b[8], inc[8];
    double eval_pose[12];
    float eval_aff[2];
    LdltWork W;
    ldso_ct_track_result R;

    LDSO_HD float cutoff() const {
#pragma clang fp contract(off)
        return p.coarse_cutoff_th * repeat;
    }
    LDSO_HD void set_eval() {
        if (phase)
            pose_matrix(cand, eval_pose);
        else
            for (int i = 0; i < 12; i++) eval_pose[i] = cur_pose[i];
        for (int i = 0; i < 2; i++) eval_aff[i] = phase ? aff_new[i] : aff_cur[i];
    }
    LDSO_HD void start_level() {
        repeat = 1;
        phase = 0;
        set_eval();
    }
    // start: ref_to_new_in [12], aff_in [2], min_res_for_abort [5]
    LDSO_HD void begin(const ldso_ct_track_params &params, int coarsest_lvl, const double *T, const double *aff,
                       const double *min_res_for_abort, float ref_exp, float new_exp, float ra, float rb) {
        p = params;
        ref_exposure = ref_exp;
        new_exposure = new_exp;
        ref_a = ra;
        ref_b = rb;
        for (int i = 0; i < 12; i++) pose_in[i] = T[i];
        for (int i = 0; i < 5; i++) {
            min_res[i] = min_res_for_abort[i];
            R.last_residuals[i] = NAN;
            R.iterations[i] = 0;
        }
        for (int i = 0; i < 3; i++) R.flow[i] = 1000;
        R.ok = 0;
        R.reason = 0;
        R.abort_level = -1;
        R.repeated_level = -1;
        for (int i = 0; i < 12; i++) cur_pose[i] = T[i];
        cur = pose_from_matrix(T);
        for (int i = 0; i < 2; i++) aff_cur[i] = aff_in[i] = (float)aff[i];
        have_repeated = false;
        lvl = coarsest_lvl;
        start_level();
    }
    LDSO_HD void log_eval(const double *rs, bool accept, ldso_ct_track_step *s) const {
        s->lvl = lvl;
        s->iteration = phase ? iteration : -1;
        s->accepted = accept ? 1 : 0;
        s->cutoff_th = cutoff();
        s->lambda = phase ? (double)lambda_used : 0.0;
        for (int i = 0; i < 12; i++) s->pose[i] = eval_pose[i];
        for (int i = 0; i < 2; i++) s->aff[i] = eval_aff[i];
        for (int i = 0; i < 6; i++) s->rs[i] = rs[i];
        for (int i = 0; i < 8; i++) s->inc[i] = phase ? inc[i] : 0.0;
    }
    LDSO_HD void fail_with(int reason, bool keep_input) {
        R.ok = 0;
        R.reason = reason;
        if (keep_input) {  // lastToNew_out and aff_g2l_out were never assigned
            for (int i = 0; i < 12; i++) R.ref_to_new[i] = pose_in[i];
            for (int i = 0; i < 2; i++) R.aff[i] = aff_in[i];
        }
    }
    // CoarseTracker.cc:285-309
    LDSO_HD void finish() {
#pragma clang fp contract(off)
        for (int i = 0; i < 12; i++) R.ref_to_new[i] = cur_pose[i];
        const float a = aff_cur[0], b = aff_cur[1], mA = p.affine_opt_mode_a, mB = p.affine_opt_mode_b;
        R.aff[0] = a;
        R.aff[1] = b;
        if ((mA != 0 && (double)fabsf(a) > 1.2) || (mB != 0 && (double)fabsf(b) > 200)) return fail_with(2, false);
        float ra, rb;
        ldso_ba::affine_from_to(ref_exposure, new_exposure, ref_a, ref_b, a, b, ra, rb);
        if ((mA == 0 && (double)fabsf(logf(ra)) > 1.5) || (mB == 0 && (double)fabsf(rb) > 200)) return fail_with(3, false);
        if (mA < 0) R.aff[0] = 0;
        if (mB < 0) R.aff[1] = 0;
        R.ok = 1;
    }
    // CoarseTracker.cc:268-283; returns whether another level follows
    LDSO_HD bool end_level() {
#pragma clang fp contract(off)
        const double last = (double)sqrtf((float)(res_old[0] / res_old[1] + 0.0));
        R.last_residuals[lvl] = last;
        for (int i = 0; i < 3; i++) R.flow[i] = res_old[2 + i];
        if (last > 1.5 * min_res[lvl]) {
            R.abort_level = lvl;
            fail_with(1, true);
            return false;
        }
        if (repeat > 1 && !have_repeated) {
            have_repeated = true;  // lvl++ under the for's lvl--
            R.repeated_level = lvl;
        } else {
            lvl--;
        }
        if (lvl < 0) {
            finish();
            return false;
        }
        start_level();
        return true;
    }
    LDSO_HD bool consume(const double *rs, const double *Hn, const double *bn, ldso_ct_track_step *log) {
#pragma clang fp contract(off)
        if (phase == 0) {
            if (log) log_eval(rs, false, log);
            for (int i = 0; i < 6; i++) res_old[i] = rs[i];
            if (rs[5] > 0.6 && repeat < 50) {
                repeat *= 2;
                return true;  // the same pose under the doubled cutoff
            }
            lambda = 0.01f;
            for (int i = 0; i < 64; i++) H[i] = Hn[i];
            for (int i = 0; i < 8; i++) b[i] = bn[i];
            iteration = 0;
        } else {
            const bool accept = (rs[0] / rs[1] + 0.0) < (res_old[0] / res_old[1] + 0.0);
            if (log) log_eval(rs, accept, log);
            if (accept) {
                for (int i = 0; i < 64; i++) H[i] = Hn[i];
                for (int i = 0; i < 8; i++) b[i] = bn[i];
                for (int i = 0; i < 6; i++) res_old[i] = rs[i];
                for (int i = 0; i < 2; i++) aff_cur[i] = aff_new[i];
                // the accepted pose is the matrix that was evaluated, and re-enters the next step through it
                // (Eigen's Quaternion(Matrix3)), as it does for a caller that runs this loop over the ABI:
                // q(R(q)) is not q in the last bits, and a large rotation carries that into R by several ulp,
                // so only this keeps the two loops bit for bit
                for (int i = 0; i < 12; i++) cur_pose[i] = eval_pose[i];
                cur = pose_from_matrix(cur_pose);
                lambda = (float)(lambda * p.lambda_decrease);
            } else {
                lambda = (float)(lambda * p.lambda_increase);
                if (lambda < kLambdaExtrapolationLimit) lambda = kLambdaExtrapolationLimit;
            }
            R.iterations[lvl]++;
            double sq = 0;
            for (int i = 0; i < 8; i++) sq = sq + inc[i] * inc[i];
            iteration++;
            if (!(sqrt(sq) > 1e-3) || iteration >= p.max_iterations[lvl]) return end_level();
        }
        lambda_used = lambda;
        lm_step(H, b, lambda, cur, aff_cur, p, W, inc, cand, aff_new);
        phase = 1;
        set_eval();
        return true;
    }
};

}  // namespace ldso_ct
