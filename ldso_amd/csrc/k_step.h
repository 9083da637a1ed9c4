// k_step.h -- the device GN loop's step: frame_step_block, k_step_resub, k_energy_to_history and
// k_set_point_vals.
#pragma once
#include "k_resubstitute.h"
#include "se3.h"

namespace {

// ============================================================================================
// Device GN loop (ldso_ba_optimize): FullSystem::doStepFromBackup +
// setPrecalcValues without a host round trip.  k_frame_step: one block per window, se3.h's
// statements (the host helpers' own code): calibration and frame steps from x, then
// FrameFramePrecalc::Set for every pair and the solver's prior vector (takeData's prior /
// delta_prior, cPrior * cDeltaF), with k_xad's xAd for the resubstitution computed in the same
// launch.  The point step -- setIdepth / setIdepthZero(idepth_backup + step), deltaF = 0
// (setDeltaF) -- is applied by k_resubstitute as it computes the step.
// ============================================================================================
struct FrameStepParams {
    WinDev *wins;
    ldso_ba_frame_state *fstate;  // [frames]
    double *calib_val;            // [win][4] CalibHessian::value
    const double *calib_zero;     // [win][4] value_zero
    const double *cprior;         // [win][4] cPrior
    const int *add_priors;        // [win]
    const double *x;              // [vec]
    float *precalc;               // [pairs][LDSO_BA_PRECALC_STRIDE]
    double *prior;                // [vec][2]: HL diagonal, bL
    // ldso_ba_optimize's loop exits (FullSystem.cc:922, 968-969): windows with it >= stop[w] skip;
    // canbreak at it >= min_its sets stop[w] = it + 1 (the pass after this step still runs)
    int *stop, *status;
    const double *win_nid;  // [win][2]: sumNID, numID of the idepths the step starts from (point_nid)
    int it, min_its;
    float th;  // setting_thOptIterations
    float aff_a, aff_b;  // setting_affineOptModeA / B: the affine priors of takeData (getPrior)
};
// one window's step: a whole 256-thread block (blk = the window)
__device__ __forceinline__ void frame_step_block(const FrameStepParams &P, int blk) {
    __shared__ double poses[LDSO_BA_MAX_FRAMES][4][7];  // ev, ev^-1, cur, cur^-1: quaternion (4), t (3)
    __shared__ float calib[4];
    // the stop flag and the window's descriptor in one round trip, then the exit
    const int stop_it = P.stop ? P.stop[blk] : INT_MAX;
    WinDev &W = P.wins[blk];
    const int N = W.N, tid = threadIdx.x;
    const double *xw = P.x + W.vec_base;
    if (P.it >= stop_it) return;  // lost in this iteration's solve, or stopped earlier
    if (P.stop && tid == 128 && P.it >= P.min_its &&
        step_canbreak(N, xw, (float)P.win_nid[2 * blk], (float)P.win_nid[2 * blk + 1], P.th)) {
        P.stop[blk] = P.it + 1;
        P.status[blk] = LDSO_BA_OPT_CONVERGED;
    }
    ldso_ba_frame_state *fs = P.fstate + W.frame_base;
    if (tid < 64) {
        // frame_step_one's two exponentials in one SIMT pass of the same code: lane f forms
        // exp(step_f), lane 32 + f exp(state_f), handed to lane f by a shuffle (N <= 16 < 32)
        const int f = tid & 31, fc = f < N ? f : 0;
        const ldso_ba_frame_state in = fs[fc];
        double v[6];
        if (tid < 32)
            frame_step_tangent(xw + 4 + 8 * fc, v);
        else
            for (int i = 0; i < 6; i++) v[i] = in.state[i];
        const Pose ex = Pose::exp(v);
        Pose eb;
        for (int k = 0; k < 4; k++) eb.q[k] = __shfl(ex.q[k], fc + 32, 64);
        for (int k = 0; k < 3; k++) eb.t[k] = __shfl(ex.t[k], fc + 32, 64);
        if (tid < N) {
            ldso_ba_frame_state o;
            frame_step_finish(in, xw + 4 + 8 * tid, ex, eb, o);
            fs[tid] = o;
            const Pose e = eval_pose(o), c = current_pose(o);
            const Pose ps[4] = {e, e.inverse(), c, c.inverse()};
            for (int q = 0; q < 4; q++) {
                for (int k = 0; k < 4; k++) poses[tid][q][k] = ps[q].q[k];
                for (int k = 0; k < 3; k++) poses[tid][q][4 + k] = ps[q].t[k];
            }
        }
    } else if (tid == 64) {
        double *v = P.calib_val + 4 * blk;
        float cd[4];
        calib_step(v, xw, P.calib_zero + 4 * blk, calib, cd);
        for (int k = 0; k < 4; k++) {
            W.calib[k] = calib[k];
            W.cdelta[k] = cd[k];
        }
        const bool add = P.add_priors[blk] != 0;
        for (int k = 0; k < 4; k++) {  // calibration prior: cPrior, cPrior * cDeltaF (upload_priors)
            P.prior[2 * (W.vec_base + k)] = add ? P.cprior[4 * blk + k] : 0.0;
            P.prior[2 * (W.vec_base + k) + 1] = add ? P.cprior[4 * blk + k] * (double)cd[k] : 0.0;
        }
    }
    __syncthreads();
    auto pose = [&](int f, int q) {
        Pose p;
        for (int k = 0; k < 4; k++) p.q[k] = poses[f][q][k];
        for (int k = 0; k < 3; k++) p.t[k] = poses[f][q][4 + k];
        return p;
    };
    for (int e = tid; e < N * N; e += blockDim.x) {
        const int h = e % N, t = e / N;
        pair_precalc(pose(t, 0), pose(h, 1), pose(t, 2), pose(h, 3), calib, fs[h], fs[t],
                     P.precalc + (size_t)(W.pair_base + e) * LDSO_BA_PRECALC_STRIDE);
    }
    if (tid < N) {
        double pr[8], dp[8];
        frame_take_data_one(fs[tid], P.aff_a, P.aff_b, pr, nullptr, dp);
        const bool add = P.add_priors[blk] != 0;
        for (int i = 0; i < 8; i++) {
            const int q = W.vec_base + 4 + 8 * tid + i;
            P.prior[2 * q] = add ? pr[i] : 0.0;
            P.prior[2 * q + 1] = add ? pr[i] * dp[i] : 0.0;
        }
    }
}
// ldso_ba_optimize: the frame / calibration step (blocks [0, n_win)) and the resubstitution with
// the point step (the rest) in one launch; both read only x and xAd, which the solve wrote
__global__ __launch_bounds__(256) void k_step_resub(FrameStepParams F, ResubParams R, int n_win) {
    if ((int)blockIdx.x < n_win) frame_step_block(F, blockIdx.x);
    else resubstitute_one(R, ((int)blockIdx.x - n_win) * 256 + threadIdx.x);
}
// ldso_ba_optimize's energy history with a communicator (the window blocks of k_stitch write it
// otherwise): row s <- the all-reduced energies
__global__ __launch_bounds__(256) void k_energy_to_history(const double *src, double *hist, int s, int n2) {
    for (int i = threadIdx.x; i < n2; i += 256) hist[(size_t)s * n2 + i] = src[i];
}
// ldso_ba_update_points: [P][4] (idepth_scaled, idepth_zero_scaled, priorF, deltaF) of one window in
// its sorted point order into the point records (columns 2..5)
__global__ __launch_bounds__(256) void k_set_point_vals(const float4 *__restrict__ vals, float *pt_data, int n) {
    const int q = blockIdx.x * 256 + threadIdx.x;
    if (q >= n) return;
    const float4 v = vals[q];
    float *d = pt_data + (size_t)q * LDSO_BA_POINT_STRIDE;
    d[2] = v.x;
    d[3] = v.y;
    d[4] = v.z;
    d[5] = v.w;
}

}  // namespace
