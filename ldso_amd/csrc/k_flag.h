// k_flag.h -- ldso_ba_flag_points: removeOutliers' and flagPointsForRemoval's decision (FullSystem.cc:
// 1654, 1356-1424; PointHessian::isOOB / isInlierNew, PointHessian.h:53-78) for every point of one
// loaded window, from the residual states and flags, the point records and idepth_hessian where the
// device holds them.  Two launches: k_flag_count (a thread per residual: the point's live and
// visible-in-a-flagged-frame counts, integer atomics) and k_flag_decide (a thread per point: the
// tree).  Every count is an integer, so the result does not depend on the execution order.  Nothing
// of the context is written: the outputs go to the call's own staging (FlagParams::cnt ... ls_out).
#pragma once
#include "ba_device.h"

namespace {

struct FlagParams {
    // the window's residuals (device order, already offset to the window) ...
    const uint8_t *rs_flags, *rs_tgt;
    const int8_t *rs_state;
    const int *rs_slot;
    // ... and points
    const float *pt_data;  // [P][LDSO_BA_POINT_STRIDE], [2] = idepth_scaled
    const float *pt_out;   // [P][12], [2] = idepth_hessian
    const int *pt_host;
    // the call's staging, device point / residual order
    const int *num_good;          // [P]
    const int *last_res;          // [P][2] residual position in the window, or -1
    const int8_t *last_state;     // [P][2]
    const uint8_t *frame_flagged; // [LDSO_BA_MAX_FRAMES]
    int *cnt;                     // [P], zero at entry: n_live | vis << 8
    int *counts;                  // [4], zero at entry
    int8_t *status;               // [P]
    int *num_good_out;            // [P]
    int8_t *ls_out;               // [P][2]
    uint8_t *res_live;            // [R]
    int R, P, rec_base;
    int min_good_active, min_good;
    float min_idepth_h;
};

// the point of a residual: record slot rec_base + s * P + q (layout.cpp)
__global__ __launch_bounds__(256) void k_flag_count(FlagParams F) {
    const int r = blockIdx.x * 256 + threadIdx.x;
    if (r >= F.R) return;
    const int live = F.rs_flags[r] & LDSO_BA_FLAG_ACTIVE;
    F.res_live[r] = (uint8_t)live;
    if (!live) return;
    const int q = (F.rs_slot[r] - F.rec_base) % F.P;
    const int vis = F.rs_state[r] == LDSO_BA_RES_IN && F.frame_flagged[F.rs_tgt[r]] ? 1 : 0;
    atomicAdd(&F.cnt[q], 1 + (vis << 8));  // at most LDSO_BA_MAX_FRAMES - 1 residuals per point
}

__global__ __launch_bounds__(256) void k_flag_decide(FlagParams F) {
    __shared__ int block_counts[4];
    if (threadIdx.x < 4) block_counts[threadIdx.x] = 0;
    __syncthreads();
    const int q = blockIdx.x * 256 + threadIdx.x;
    if (q < F.P) {
        const int c = F.cnt[q], n_live = c & 255, vis = c >> 8;
        int ls[2];
        for (int i = 0; i < 2; i++) {
            const int k = F.last_res[2 * q + i];
            ls[i] = k >= 0 ? F.rs_state[k] : F.last_state[2 * q + i];
        }
        const int ng = F.num_good[q] + n_live;
        const int A = F.min_good_active, G = F.min_good;
        int st;
        if (F.pt_data[(size_t)q * LDSO_BA_POINT_STRIDE + 2] < 0.f || n_live == 0) {
            st = LDSO_BA_PT_OUTLIER;
        } else {
            const bool oob = (n_live >= A && ng > G + 10 && n_live - vis < A) || ls[0] == LDSO_BA_RES_OOB ||
                             (n_live >= 2 && ls[0] == LDSO_BA_RES_OUTLIER && ls[1] == LDSO_BA_RES_OUTLIER);
            if (oob || F.frame_flagged[F.pt_host[q]])
                st = n_live >= A && ng >= G && F.pt_out[(size_t)q * 12 + 2] > F.min_idepth_h ? LDSO_BA_PT_MARGINALIZED
                                                                                              : LDSO_BA_PT_OUT;
            else
                st = LDSO_BA_PT_ACTIVE;
        }
        F.status[q] = (int8_t)st;
        F.num_good_out[q] = ng;
        F.ls_out[2 * q] = (int8_t)ls[0];
        F.ls_out[2 * q + 1] = (int8_t)ls[1];
        atomicAdd(&block_counts[st], 1);
    }
    __syncthreads();
    if (threadIdx.x < 4 && block_counts[threadIdx.x]) atomicAdd(&F.counts[threadIdx.x], block_counts[threadIdx.x]);
}

}  // namespace
