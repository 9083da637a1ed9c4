// k_xad.h -- ResubParams and k_xad.  They belong to the resubstitution (k_resubstitute.h), but k_xad has
// always been defined before k_activate, and the kernels keep their definition order.
#pragma once
#include "k_solve.h"

namespace {

struct ResubParams {
    const float *__restrict__ xad;   // [win][kXadStride]: xAd[h*N + t][8], then x_c[4]
    const WinDev *__restrict__ wins;
    const int *__restrict__ pt_win;
    const int *__restrict__ pt_nres;
    const unsigned long long *__restrict__ pt_tgt;
    const float4 *__restrict__ rec_a;     // the pass's records (write_record)
    const float2 *__restrict__ rec_b;
    const float *__restrict__ geo_snap;   // [pairs][kGeoSnap]: the pass's centre geometry inputs
    const float *__restrict__ pt_geo;     // the point records (u, v)
    const float *__restrict__ pt_out;
    const int *__restrict__ pt_host;
    float *pt_step;
    float *pt_data;  // non-null: apply doStepFromBackup's point step in place (ldso_ba_optimize)
    int begin, count;
    float lambda;
    const int *stop;  // ldso_ba_optimize: points of windows with it >= stop[w] skip
    int it;
};

// xAd from the device solution (windows solved by k_solve, or x set otherwise)
__global__ __launch_bounds__(256) void k_xad(const WinDev *__restrict__ wins, const double *__restrict__ x,
                                             const double *__restrict__ adH, const double *__restrict__ adT,
                                             float *xad) {
    const WinDev &W = wins[blockIdx.x];
    xad_fill(W, x + W.vec_base, adH, adT, xad + (size_t)blockIdx.x * kXadStride, threadIdx.x, blockDim.x);
}

}  // namespace
