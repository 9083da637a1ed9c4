// ldso_ct.hip -- the C ABI of LDSO's coarse tracker (include/ldso_ct.h) on the MI355X (gfx950) and its
// host side: one translation unit in pieces.  This file creates and destroys the context, makes K and
// reads the kernel timing; everything else stands in the piece of its subsystem.
// The state and what every part shares:
//   ct_context.h         the timing slots; struct ldso_ct_ctx, a core and one member struct per part below;
//                        ct_launch, ct_grow, ct_read, ct_blocks, level_grid, level_of
//   hip_owning.h         shared with ldso_ba.hip and ldso_lc.hip: fail / HIP_TRY, the owning buffers and
//                        events, StreamBorrow, KernelTimer
// The host code of each part, with its helpers and its entry points (c->PART is its state):
//   ct_host_frame.h      set_new_frame[_raw[_device]], undistort_init, get_undistorted, get_frame_level
//   ct_host_ref.h        set_reference, make_reference[_ba], get_reference
//   ct_host_res.h        calc_res[_batch], calc_gs, calc_res_gs, get_warped, track, lm_step
//   ct_host_ip.h         make_immature, immature_upload / _download / _append, trace
//   ct_host_sel.h        select_init / _potential / _pixels, make_new_traces
//   ct_host_cor.h        corners_init, detect_corners
//   ct_host_as.h         make_distance_map[_ba], select_activation, selection_download
//   ct_host_init.h       every ldso_ct_init_*
// The kernels, each described where it stands:
//   k_ct_pyramid.h       k_ct_pyr_down, k_ct_pyr_grad: the new frame's pyramid
//   k_ct_residual.h      k_ct_calc_res, k_ct_calc_gs: calcRes / calcGSSSE (ct_eval.h: an evaluation's constants and
//                        the Vec6 / H / b from its sums, the same functions here and in k_ct_track)
//   k_ct_immature.h      k_ct_make_immature, k_ct_trace, k_ct_ip_count: immature points
//   k_ct_coarse_depth.h  k_ct_cd_*: the reference cloud from the window's contributions
//   k_ct_select.h        k_ct_sel_*: pixel selection (makeMaps) and makeNewTraces' walk
//   k_ct_actsel.h        k_ct_as_*: the distance map and activatePointsMT's walk
//   k_ct_track.h         k_ct_track: trackNewestCoarse's LM loop, one launch (ct_lm.h: the loop's host/device half)
//   k_ct_init.h          k_ct_init_track, k_ct_init_eval, k_ct_init_opt_reg: CoarseInitializer::trackFrame, one launch
//                        (ct_init.h: the loop's host/device half)
//   k_ct_undistort.h     k_ct_undistort: the new frame's image from the raw 8- / 16-bit one (Undistort::undistort)
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/ldso_ba.h"
#include "../../include/ldso_ct.h"
#include "ldso_ba_internal.h"
#include "hip_owning.h"
// the kernel headers in the order of their first inclusion, which is the order of the kernels in the code object
#include "k_ct_pyramid.h"
#include "k_ct_residual.h"
#include "k_ct_immature.h"
#include "k_ct_coarse_depth.h"
#include "k_ct_track.h"
#include "k_ct_actsel.h"
#include "k_ct_undistort.h"
#include "ct_context.h"

#pragma clang fp contract(off)

// The kernel templates' instances, in the order the code object holds them (behind every other kernel): a
// template is emitted where it is first used, so without this list the order of the pieces below would be
// the order of these kernels, and `make device-id` would change with every piece that moves.  A new kernel
// template's instances are appended here; a changed signature is changed here too (the compiler refuses a
// line that matches no template, and one left out only moves its kernel to the end of the code object).
namespace {
template __global__ void k_ct_calc_res<true>(CtResParams);
template __global__ void k_ct_calc_res<false>(CtResParams);
template __global__ void k_ct_sel_block<false>(SelParams, unsigned *, const int *, uint8_t *, int *);
template __global__ void k_ct_sel_block<true>(SelParams, unsigned *, const int *, uint8_t *, int *);
template __global__ void k_ct_undistort<uint8_t, true>(const uint8_t *, float *, UndParams);
template __global__ void k_ct_undistort<uint8_t, false>(const uint8_t *, float *, UndParams);
template __global__ void k_ct_undistort<uint16_t, true>(const uint16_t *, float *, UndParams);
template __global__ void k_ct_undistort<uint16_t, false>(const uint16_t *, float *, UndParams);
template __global__ void k_ct_sel_emit<false>(const float4 *, int, int, const uint8_t *, int, int *, IpRec *, int);
template __global__ void k_ct_sel_emit<true>(const float4 *, int, int, const uint8_t *, int, int *, IpRec *, int);
template __global__ void k_ct_track<kTrackWaves>(CtTrackParams);
}  // namespace

#include "ct_host_frame.h"
#include "ct_host_ref.h"
#include "ct_host_res.h"
#include "ct_host_ip.h"
#include "ct_host_sel.h"
#include "ct_host_cor.h"
#include "ct_host_as.h"
#include "ct_host_init.h"

extern "C" {

int ldso_ct_create(int32_t device, int32_t width, int32_t height, ldso_ct_ctx **out, int32_t *n_levels_out) {
    if (!out) return fail(-1, "null output pointer");
    *out = nullptr;
    if (width < 8 || height < 8) return fail(-1, "image too small");
    ldso_ct_ctx *c = new ldso_ct_ctx();
    c->device = device;
    hipError_t e = hipSetDevice(device);
    if (e == hipSuccess) e = hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking);
    if (e != hipSuccess) {
        delete c;
        return fail(-2, std::string("hip init: ") + hipGetErrorString(e));
    }
    // setGlobalCalib's level rule (GlobalCalib.cc:20-30)
    int wl = width, hl = height, L = 1;
    while (wl % 2 == 0 && hl % 2 == 0 && wl * hl > 5000 && L < LDSO_CT_MAX_LEVELS) {
        wl /= 2;
        hl /= 2;
        L++;
    }
    c->levels = L;
    PyrParams &P = c->pyr;
    P.w = width;
    P.h = height;
    P.levels = L;
    P.tile = 1 << (L - 1);
    int off = 0;
    for (int l = 0; l < L; l++) {
        P.wl[l] = width >> l;
        P.hl[l] = height >> l;
        P.off[l] = off;
        off += P.wl[l] * P.hl[l];
    }
    P.off[L] = off;
    int rc;
    if ((rc = c->frame.d_color.alloc((size_t)width * height)) || (rc = c->frame.d_inten.alloc(off)) ||
        (rc = c->frame.d_dIp.alloc(off)) || (rc = c->frame.d_B.alloc(256)) ||
        (rc = c->res.d_poses.alloc(kMaxHyp)) || (rc = c->res.h_poses.ensure(kMaxHyp)) ||
        (rc = c->ip.d_counts.alloc(8)) || (rc = c->ip.h_counts.ensure(8))) {
        const std::string why = ldso_ba::last_error();
        ldso_ct_destroy(c);
        return fail(-3, why);
    }
    if (n_levels_out) *n_levels_out = L;
    *out = c;
    return 0;
}

void ldso_ct_destroy(ldso_ct_ctx *c) {
    if (!c) return;
    (void)hipSetDevice(c->device);
    if (c->stream) (void)hipStreamSynchronize(c->stream);
    c->timer.drain();  // the pending events go back to the pool, which destroys them
    if (c->stream) (void)hipStreamDestroy(c->stream);
    delete c;  // every member frees what it owns: the work that used it has completed
}

int ldso_ct_make_k(ldso_ct_ctx *c, const float calib[4], float *k_out) {
    if (!c || !calib) return fail(-1, "null argument");
    // CoarseTracker::makeK (CoarseTracker.cc:312-339): fx/cx of level l from level 0 in double
    c->fx[0] = calib[0];
    c->fy[0] = calib[1];
    c->cx[0] = calib[2];
    c->cy[0] = calib[3];
    for (int l = 1; l < c->levels; l++) {
        c->fx[l] = c->fx[l - 1] * 0.5;
        c->fy[l] = c->fy[l - 1] * 0.5;
        c->cx[l] = (c->cx[0] + 0.5) / ((int)1 << l) - 0.5;
        c->cy[l] = (c->cy[0] + 0.5) / ((int)1 << l) - 0.5;
    }
    for (int l = 0; l < c->levels; l++) {
        // Eigen's cofactor inverse of K (Eigen/src/LU/InverseImpl.h), as FrameFramePrecalc's
        const float fx = c->fx[l], fy = c->fy[l], cx = c->cx[l], cy = c->cy[l];
        const float invdet = 1.0f / (fy * fx);
        float *Ki = c->Ki[l];
        Ki[0] = fy * invdet;
        Ki[1] = 0 * invdet;
        Ki[2] = (0 * cy - cx * fy) * invdet;
        Ki[3] = 0 * invdet;
        Ki[4] = fx * invdet;
        Ki[5] = (cx * 0 - fx * cy) * invdet;
        Ki[6] = 0 * invdet;
        Ki[7] = 0 * invdet;
        Ki[8] = (fx * fy - 0 * 0) * invdet;
        if (k_out) {
            float *o = k_out + 13 * l;
            o[0] = fx;
            o[1] = fy;
            o[2] = cx;
            o[3] = cy;
            std::memcpy(o + 4, Ki, 9 * sizeof(float));
        }
    }
    c->have_k = true;
    return 0;
}

int ldso_ct_set_kernel_timing(ldso_ct_ctx *c, int32_t enable) {
    if (!c) return fail(-1, "null context");
    c->timer.on = enable != 0;
    if (c->timer.on) c->timer.reset();
    return 0;
}

int ldso_ct_get_kernel_times(ldso_ct_ctx *c, double *ms, int64_t *counts, int32_t n) {
    if (!c) return fail(-1, "null context");
    HIP_TRY(hipStreamSynchronize(c->stream));
    c->timer.drain();
    for (int i = 0; i < std::min<int>(n, kNumCtKernels); i++) {
        if (ms) ms[i] = c->timer.ms[i];
        if (counts) counts[i] = c->timer.count[i];
    }
    return 0;
}

const char *ldso_ct_kernel_name(int32_t i) { return (i >= 0 && i < kNumCtKernels) ? kCtKernelNames[i] : nullptr; }
int32_t ldso_ct_num_kernels(void) { return kNumCtKernels; }

}  // extern "C"
