// k_edit.h -- ldso_ba_edit_window's one launch: the carried residual state and point records gathered
// from the old device arrays into the new layout's, the new entries spliced in from their compact
// upload, and everything a fresh load fills (ldso_ba_load's memsets) filled.
#pragma once
#include "ba_device.h"

namespace {

constexpr int kEditFills = 8;
struct EditParams {
    // per destination (device order of the new layout): old device position, or ~rank into the new entries
    const int *rs_src, *pt_src;
    // the old arrays
    const int8_t *o_state;
    const uint8_t *o_flags;
    const float *o_energy, *o_newenergy;
    const float4 *o_pt;  // LDSO_BA_POINT_STRIDE / 4 = 6 per point
    // the new entries, by rank (state_NewEnergy is loaded equal to state_energy)
    const int8_t *n_state;
    const uint8_t *n_flags;
    const float *n_energy;
    const float4 *n_pt;
    // the new arrays
    int8_t *state, *newstate;
    uint8_t *flags;
    float *energy, *newenergy;
    float4 *pt;
    int R, P;
    // 4-byte fills: records, centres, point outputs, the packed system ...
    unsigned *fill_dst[kEditFills];
    long long fill_words[kEditFills];
    unsigned fill_val[kEditFills];
    int n_fill;
    // ldso_ba_load_marginalization_device (the sources are the parent's arrays): priorF, float 4 of
    // every gathered record, times setting_idepthFixPriorMargFac (layout.cpp's marg load); 0 = an edit
    int scale_prior;
    float prior_fac;
};
constexpr int kPtVec = LDSO_BA_POINT_STRIDE / 4;

// Consecutive threads take consecutive destinations (a wavefront stores 64 consecutive elements of
// every array); only the sources are scattered.  Bounds: the planner's indices are positions of the
// old layout or ranks of the compact upload by construction (edit_plan.cpp).
__global__ __launch_bounds__(256) void k_edit_gather(EditParams E) {
    const int tid = blockIdx.x * 256 + threadIdx.x, nth = gridDim.x * 256;
    const int *__restrict__ rs_src = E.rs_src;
    const int *__restrict__ pt_src = E.pt_src;
    for (int r = tid; r < E.R; r += nth) {
        const int s = rs_src[r];
        int8_t st;
        uint8_t fl;
        float en, ne;
        if (s >= 0) {
            st = E.o_state[s];
            fl = E.o_flags[s];
            en = E.o_energy[s];
            ne = E.o_newenergy[s];
        } else {
            st = E.n_state[~s];
            fl = E.n_flags[~s];
            en = ne = E.n_energy[~s];
        }
        E.state[r] = st;
        E.flags[r] = fl;
        E.energy[r] = en;
        E.newenergy[r] = ne;
        E.newstate[r] = LDSO_BA_RES_OUTLIER;
    }
    for (int i = tid; i < kPtVec * E.P; i += nth) {
        const int q = i / kPtVec, k = i - kPtVec * q, s = pt_src[q];
        float4 v = s >= 0 ? E.o_pt[(size_t)s * kPtVec + k] : E.n_pt[(size_t)(~s) * kPtVec + k];
        if (E.scale_prior && k == 1) v.x *= E.prior_fac;
        E.pt[i] = v;
    }
    for (int f = 0; f < E.n_fill; f++) {
        unsigned *dst = E.fill_dst[f];
        const unsigned v = E.fill_val[f];
        for (long long i = tid; i < E.fill_words[f]; i += nth) dst[i] = v;
    }
}

}  // namespace
