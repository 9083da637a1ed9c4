// ldso_ba.hip -- MI355X (gfx950) kernels and C ABI of LDSO's photometric-BA hot path.
//
// One Gauss-Newton pass over every loaded window (ldso_ba_linearize) is four stream-ordered
// launches:
//
//   k_linearize        one wavefront per <= 64-residual chunk of one (host,target) bucket:
//                      linearize (Residuals.cc:15-217) with 8 lanes per residual (one per pattern
//                      pixel; the residual's tap footprint loaded as 16-B band columns into an LDS
//                      box, phase_a_pieces), applyRes (Residuals.h:70-88) with a lane per residual,
//                      and the chunk's AccumulatorApprox block (AccumulatedTopHessian.cc:66-99,
//                      MatrixAccumulators.h:893-1045) as 32 fp32 MFMAs into a 96-float partial.
//                      The pair precalc, frame thresholds and image base are wave-uniform.
//   k_point_sc         per point: Hdd/bd/Hcd sums (AccumulatedTopHessian.cc:94-116), HdiF
//                      (AccumulatedSCHessian.cc:24-33); then the Schur terms of a 64-point chunk of
//                      one host as one symmetric rank-64 update G += U^T diag(HdiF) U staged in LDS
//                      (the accD/accE/accEB/accHcc/accbc sums of AccumulatedSCHessian.cc:35-50).
//                      Inside ldso_ba_optimize its leading blocks also sum doStepFromBackup's sumNID.
//   k_stitch_host      block per host frame (windows of up to 12 keyframes): the host's dense
//                      partial {HA, bA, Hsc, bsc} from its Top blocks and chunk SYRK partials
//                      (AccumulatedTopHessian.cc:213-239, AccumulatedSCHessian.cc:80-114) in double;
//                      one block per window runs setNewFrameEnergyTH (FullSystem.cc:2078-2109) as a
//                      radix select and sums the linearizeAll energy.
//   k_stitch_host_sum  thread per packed output element: the window's host partials summed in host
//                      order (no atomics: the stitched system is bitwise repeatable).
// Windows of 13-16 keyframes use k_stitch + k_stitch_sum instead (one contribution record per
// (pair, block), summed in a fixed pair order).
//
// Outside the pass: the device solve (k_solve_fast; exact mode k_solve_reg / k_solve), k_step_resub
// (doStepFromBackup + setPrecalcValues + resubstituteFPt inside ldso_ba_optimize), k_resubstitute,
// k_activate (optimizeImmaturePoint), k_tile_image / k_intensity_image (image staging at load and
// at a host put into the frame store), k_ingest_intensity / k_ingest_texels (device buffer -> frame
// store slot), k_export_newest + k_frame_th (sharded threshold exchange), k_pack_out (results to mapped memory).
//
// The per-residual arithmetic of k_linearize is compiled with contraction off and follows the
// reference's statement order, so states, energies, JpJdF and the per-point sums are
// bit-identical to the CPU restatement; the H/b sums are reassociated (tolerance-checked).
//
// The files:
//   ba_device.h       shared by the kernel stages: WinDev, the image taps (getInterpolatedElement33 on
//                     makeImages' dI), projectPoint's centre geometry, the packed-triangle and Top-slot
//                     indices, the sumNID chain, the setNewFrameEnergyTH radix select
//   k_linearize.h     PointFrameResidual::linearize + applyRes (Residuals.cc:15-217) and addPoint's
//                     AccumulatorApprox block; a template, so its instantiations are emitted after every
//                     other kernel wherever it is defined
//   k_point_sc.h, k_stitch.h, k_stitch_host.h, k_solve.h, k_solve_reg.h, k_solve_fast.h, k_exchange.h,
//   k_xad.h, k_activate.h, k_resubstitute.h, k_step.h, k_io.h, k_edit.h (ldso_ba_edit_window's gather,
//   which ldso_ba_load_marginalization_device points at the parent's arrays), k_flag.h (ldso_ba_flag_points)
//                     the 28 non-template kernels by stage, included below in the order the kernels have
//                     always been defined in
//   hip_owning.h      shared with ldso_ct.hip and ldso_lc.hip: fail / HIP_TRY, the owning buffers and events, StreamBorrow, KernelTimer
//   ba_context.h      the timing slots, the environment switches (read_switches), the allocation
//                     generation, the frame store, struct ldso_ba_ctx
//   ba_launch.h       staged uploads, timed launches, image staging, the parameter fillers and the
//                     launches several entry points share
//   ba_window.h       a laid-out window onto the device: the one table of the buffers a Layout sizes
//                     (window_buffers), walked by load_impl (ldso_ba_load*) and by edit_impl
//                     (ldso_ba_edit_window)
//   ldso_ba.hip       the C ABI and the helpers between its extern "C" blocks (the pass, the
//                     exchange, the device solve, the captured graphs)
#include <hip/hip_runtime.h>
#include <hip/hip_ext.h>
#include <rccl/rccl.h>

#include <algorithm>
#include <atomic>
#include <climits>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <string>
#include <vector>

#include "../../include/ldso_ba.h"
#include "../../include/ldso_ct.h"
#include "layout.h"
#include "ldso_ba_internal.h"
#include "se3.h"
#include "ba_device.h"
#include "k_linearize.h"
#include "k_point_sc.h"
#include "k_stitch.h"
#include "k_stitch_host.h"
#include "k_solve.h"
#include "k_solve_reg.h"
#include "k_solve_fast.h"
#include "k_exchange.h"
#include "k_xad.h"
#include "k_activate.h"
#include "k_resubstitute.h"
#include "k_step.h"
#include "k_io.h"
#include "k_edit.h"
#include "k_flag.h"
#include "edit_plan.h"
#include "marg_plan.h"
#include "ba_context.h"
#include "ba_launch.h"
#include "ba_window.h"

// =========================================================================================
// C ABI
// =========================================================================================
// the coarse tracker's view of window `win` after a pass (ldso_ct_make_reference_ba)
int ldso_ba::ba_ref_view(const ldso_ba_ctx *c, int win, ldso_ba::BaRefView *out) {
    if (!c || !out) return set_error(-1, "null argument");
    if (win < 0 || win >= c->n_win) return set_error(-1, "window index out of range");
    const WinDev &D = c->wd[win];
    out->center = reinterpret_cast<const float *>(c->d_rs_center.p) + D.res_base;
    out->plane_stride = c->R_tot;
    out->state = c->d_rs_state.p + D.res_base;
    out->tgt = c->d_rs_tgt.p + D.res_base;
    out->slot = c->d_rs_slot.p + D.res_base;
    out->pt_out = c->d_pt_out.p + (size_t)D.point_base * 12;
    out->pt_data = c->d_pt_data.p + (size_t)D.point_base * LDSO_BA_POINT_STRIDE;
    out->pt_host = c->d_pt_host.p + D.point_base;
    out->R = D.R;
    out->P = D.P;
    out->N = D.N;
    out->rec_base = D.rec_base;
    out->width = D.width;
    out->height = D.height;
    out->device = c->device;
    out->stream = (void *)c->stream;
    out->marg = c->marg;
    out->sharded = c->comm_world > 1 || c->shard_count > 1;
    out->have_pass = c->pass_since_load;
    return 0;
}

extern "C" {

int ldso_ba_abi_version(void) { return LDSO_BA_ABI_VERSION; }
const char *ldso_ba_last_error(void) { return last_error(); }

int ldso_ba_frame_precalc(int32_t n, const ldso_ba_frame_state *f, const float calib[4], float *out) {
    if (n < 1 || n > LDSO_BA_MAX_FRAMES || !f || !calib || !out) return fail(-1, "bad arguments");
    return frame_precalc(n, f, calib, out);
}
int ldso_ba_set_adjoints(int32_t n, const ldso_ba_frame_state *f, double *adH, double *adT, double *cp) {
    if (n < 1 || n > LDSO_BA_MAX_FRAMES || !f || !adH || !adT) return fail(-1, "bad arguments");
    return set_adjoints(n, f, adH, adT, cp);
}
int ldso_ba_adjoints_diagonal(int32_t n, const double *ad) {
    if (n < 1 || n > LDSO_BA_MAX_FRAMES || !ad) return fail(-1, "bad arguments");
    return adjoints_diagonal(ad, (size_t)n * n) ? 1 : 0;
}
int ldso_ba_frame_take_data(int32_t n, const ldso_ba_frame_state *f, const ldso_ba_opt_settings *st, double *prior,
                            double *delta, double *dp) {
    if (n < 1 || n > LDSO_BA_MAX_FRAMES || !f) return fail(-1, "bad arguments");
    int rc;
    if ((rc = ldso_ba_check_settings(st))) return rc;
    const ldso_ba_opt_settings s = st ? *st : ldso_ba_opt_settings LDSO_BA_OPT_SETTINGS_INIT;
    return frame_take_data(n, f, s.affine_opt_mode_a, s.affine_opt_mode_b, prior, delta, dp);
}
int ldso_ba_nullspaces(int32_t n, const ldso_ba_frame_state *f, double *out) {
    if (n < 1 || n > LDSO_BA_MAX_FRAMES || !f || !out) return fail(-1, "bad arguments");
    return nullspaces(n, f, out);
}
int ldso_ba_solve_system(const ldso_ba_opt_settings *st, int32_t n, int32_t it, double lambda, const double *HA,
                         const double *bA, const double *HL, const double *bL, const double *HM, const double *bM,
                         const double *Hsc, const double *bsc, const double *ns, int32_t nn, double *x) {
    if (n < 1 || n > LDSO_BA_MAX_FRAMES || !HA || !bA || !HL || !bL || !Hsc || !bsc || !x)
        return fail(-1, "bad arguments");
    int rc;
    if ((rc = ldso_ba_check_settings(st))) return rc;  // the default solver mode only, no inertial terms
    // without SOLVER_ORTHOGONALIZE_X_LATER the solve never projects (EnergyFunctional.cc:428-432)
    if (st && !(st->solver_mode & LDSO_BA_SOLVER_ORTHOGONALIZE_X_LATER)) nn = 0;
    return solve_system(n, it, lambda, HA, bA, HL, bL, HM, bM, Hsc, bsc, ns, nn, x);
}

int ldso_ba_marginalize_frame(int32_t n, int32_t idx, const double *HM, const double *bM, const double *prior,
                              const double *delta_prior, double *HM_out, double *bM_out) {
    if (n < 2 || n > LDSO_BA_MAX_FRAMES || idx < 0 || idx >= n || !HM || !bM || !prior || !delta_prior || !HM_out ||
        !bM_out)
        return fail(-1, "bad arguments");
    return marginalize_frame(n, idx, HM, bM, prior, delta_prior, HM_out, bM_out);
}

int ldso_ba_ad_ht_delta(int32_t n, const double *delta, const double *adH, const double *adT, float *out) {
    if (n < 1 || n > LDSO_BA_MAX_FRAMES || !delta || !adH || !adT || !out) return fail(-1, "bad arguments");
    return ad_ht_delta(n, delta, adH, adT, out);
}
int ldso_ba_calc_m_energy(int32_t n, const double *HM, const double *bM, const float *c_delta, const double *delta,
                          double *out) {
    if (n < 1 || n > LDSO_BA_MAX_FRAMES || !HM || !bM || !c_delta || !delta || !out) return fail(-1, "bad arguments");
    *out = calc_m_energy(n, HM, bM, c_delta, delta);
    return 0;
}
int ldso_ba_calc_l_energy(int32_t n, const double *prior, const double *delta_prior, const double *c_prior,
                          const float *c_delta, int32_t n_points, const float *deltaF, const float *priorF,
                          double *out) {
    if (n < 1 || n > LDSO_BA_MAX_FRAMES || !prior || !delta_prior || !c_prior || !c_delta || n_points < 0 ||
        (n_points > 0 && (!deltaF || !priorF)) || !out)
        return fail(-1, "bad arguments");
    *out = calc_l_energy(n, prior, delta_prior, c_prior, c_delta, n_points, deltaF, priorF);
    return 0;
}

int ldso_ba_shard_points(const ldso_ba_window *w, int32_t rank, int32_t count, int32_t *points_out,
                         int32_t *n_out) {
    if (!w || !n_out || count < 1 || rank < 0 || rank >= count) return fail(-1, "bad arguments");
    if (int rc = check_window(*w, false)) return rc;
    std::vector<int> pts;
    shard_points(*w, rank, count, pts);
    if (points_out) std::memcpy(points_out, pts.data(), pts.size() * sizeof(int32_t));
    *n_out = (int32_t)pts.size();
    return 0;
}

int ldso_ba_pack_upper(int32_t dim, const double *HA, const double *bA, const double *Hsc, const double *bsc,
                        double *packed) {
    if (dim < 1 || !HA || !bA || !Hsc || !bsc || !packed) return fail(-1, "bad arguments");
    const long long pl = packed_len(dim);
    long long q = 0;
    for (int r = 0; r < dim; r++)
        for (int c = r; c < dim; c++, q++) {
            packed[q] = HA[(size_t)r * dim + c];
            packed[pl + dim + q] = Hsc[(size_t)r * dim + c];
        }
    for (int r = 0; r < dim; r++) {
        packed[pl + r] = bA[r];
        packed[2 * pl + dim + r] = bsc[r];
    }
    return 0;
}

int ldso_ba_unpack_upper(int32_t dim, const double *packed, double *HA, double *bA, double *Hsc, double *bsc) {
    if (dim < 1 || !packed) return fail(-1, "bad arguments");
    const long long pl = packed_len(dim);
    long long q = 0;
    for (int r = 0; r < dim; r++)
        for (int c = r; c < dim; c++, q++) {
            if (HA) HA[(size_t)r * dim + c] = HA[(size_t)c * dim + r] = packed[q];
            if (Hsc) Hsc[(size_t)r * dim + c] = Hsc[(size_t)c * dim + r] = packed[pl + dim + q];
        }
    for (int r = 0; r < dim; r++) {
        if (bA) bA[r] = packed[pl + r];
        if (bsc) bsc[r] = packed[2 * pl + dim + r];
    }
    return 0;
}

// setNewFrameEnergyTH (FullSystem.cc:2078-2109) over gathered NewEnergyWithOutlier values (< 0:
// padding, skipped): the host form of k_frame_th, for callers that gather the slots themselves
int ldso_ba_frame_threshold(const float *values, int64_t n, float *th_out) {
    if (!th_out || n < 0 || (n > 0 && !values)) return fail(-1, "bad arguments");
    std::vector<float> v;
    v.reserve((size_t)n);
    for (int64_t i = 0; i < n; i++)
        if (values[i] >= 0) v.push_back(values[i]);
    if (v.empty()) {
        *th_out = 12 * 12 * LDSO_BA_PATTERN_NUM;
        return 0;
    }
    const int nth = (int)(kFrameEnergyTHN * (float)v.size());
    std::nth_element(v.begin(), v.begin() + nth, v.end());
    const float x = sqrtf(v[nth]);
    float th = x * kFrameEnergyTHFacMedian;
    th = 26.0f * kFrameEnergyTHConstWeight + th * (1 - kFrameEnergyTHConstWeight);
    th = th * th;
    th *= kOverallEnergyTHWeight * kOverallEnergyTHWeight;
    *th_out = th;
    return 0;
}

int ldso_ba_validate_window(const ldso_ba_window *w) {
    if (!w) return fail(-1, "null window");
    return check_window(*w);
}

int ldso_ba_create(int32_t device, ldso_ba_ctx **out) {
    if (!out) return fail(-1, "null out");
    *out = nullptr;
    int ndev = 0;
    HIP_TRY(hipGetDeviceCount(&ndev));
    if (device < 0 || device >= ndev) return fail(-1, "no such HIP device");
    HIP_TRY(hipSetDevice(device));
    ldso_ba_ctx *c = new ldso_ba_ctx();
    c->device = device;
    if (hipDeviceGetAttribute(&c->n_cu, hipDeviceAttributeMultiprocessorCount, device) != hipSuccess || c->n_cu <= 0)
        c->n_cu = 256;
    hipError_t e = hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking);
    if (e != hipSuccess) {
        delete c;
        return fail(-2, std::string("hipStreamCreate: ") + hipGetErrorString(e));
    }
    *out = c;
    return 0;
}

void ldso_ba_destroy(ldso_ba_ctx *c) {
    if (!c) return;
    (void)hipSetDevice(c->device);
    if (c->stream) (void)hipStreamSynchronize(c->stream);
    c->timer.drain();  // the pending events go back to the pool, which destroys them
    if (c->comm) (void)ncclCommDestroy(c->comm);
    if (c->stream) (void)hipStreamDestroy(c->stream);
    // every member frees what it owns (device and pinned buffers, events, graph execs): the work
    // that used them has completed, the device is current, and no release needs the stream
    delete c;
}

void *ldso_ba_stream(ldso_ba_ctx *c) { return c ? (void *)c->stream : nullptr; }

}  // extern "C"

namespace {
// Device -> slot on the context stream, ordered by events and never by the host: the ingest waits for
// what the producer's stream holds now, and whatever that stream is given later -- the producer's
// next overwrite of its buffers -- waits for the ingest (StreamBorrow).  The slot itself is
// only ever read and written on the context stream, so stream order keeps the write behind any load
// still copying out of it.
int store_ingest_device(ldso_ba_ctx *c, int64_t id, const float *inten, const void *texels, hipStream_t prod) {
    FrameStore &S = c->store;
    const ImageLayout &l = S.lay;
    int slot = -1;
    int rc = S.slot_for(id, &slot);
    if (rc) return rc;
    if (l.mode == 1 && !texels)
        return fail(-1, "image layout 1 stores [I, dx, dy]: the device source must give the texels");
    if (l.mode == 3 && !inten)
        return fail(-1, "image layout 3 stores intensities: the device source must give the intensity plane");
    HIP_TRY(hipSetDevice(c->device));
    if ((rc = S.borrow.begin(c->stream, prod))) return rc;
    const int nb = (int)((l.frame_stride + 255) / 256);  // a thread per float4 of the slot, both layouts
    if (l.mode == 3)
        k_ingest_intensity<<<nb, 256, 0, c->stream>>>(inten, S.slot(slot), l.width, l.height, l.tiles_per_row * 8, l.padded_h);
    else
        k_ingest_texels<<<nb, 256, 0, c->stream>>>(static_cast<const float4 *>(texels), S.slot(slot), l.width, l.height,
                                                   l.tiles_per_row, l.padded_h);
    HIP_TRY(hipGetLastError());
    if ((rc = S.borrow.end(c->stream, prod))) return rc;
    c->xfer[1] += (int64_t)l.slot_bytes();
    S.commit(slot, id);
    c->xfer[3]++;
    return 0;
}
}  // namespace

extern "C" {

int ldso_ba_edit_window(ldso_ba_ctx *c, int32_t win, const ldso_ba_edit *e) { return edit_impl(c, win, e); }

int ldso_ba_edit_stats(ldso_ba_ctx *c, double out[6]) {
    if (!c || !out) return fail(-1, "null argument");
    HIP_TRY(hipSetDevice(c->device));
    edit_events_drain(c);
    for (int i = 0; i < 6; i++) out[i] = c->ed_stat[i];
    return 0;
}

int ldso_ba_load(ldso_ba_ctx *c, int32_t n_windows, const ldso_ba_window *ws, int32_t shard_rank,
                 int32_t shard_count) {
    return load_impl(c, n_windows, ws, shard_rank, shard_count, nullptr, 0);
}

int ldso_ba_load_marginalization(ldso_ba_ctx *marg, const ldso_ba_ctx *parent, int32_t parent_win,
                                 const ldso_ba_window *points) {
    if (!marg || !parent || !points || marg == parent) return fail(-1, "bad arguments");
    if (parent_win < 0 || parent_win >= parent->n_win) return fail(-1, "parent window out of range");
    if (marg->device != parent->device) return fail(-1, "contexts on different devices");
    const WinDev &pw = parent->wd[parent_win];
    if (points->n_frames != pw.N || points->width != pw.width || points->height != pw.height)
        return fail(-1, "marginalisation window does not match the parent window's frames");
    marg->settings = parent->settings;  // the parent's affine modes shape res_toZeroF and Jab_r
    return load_impl(marg, 1, points, 0, 1, parent, parent_win);
}

int ldso_ba_load_marginalization_device(ldso_ba_ctx *marg, const ldso_ba_ctx *parent, int32_t parent_win,
                                        const ldso_ba_window *frame_terms, int32_t n_points, const int32_t *points,
                                        const uint8_t *res_live) {
    if (!marg || !parent || !frame_terms || marg == parent) return fail(-1, "bad arguments");
    if (parent_win < 0 || parent_win >= parent->n_win) return fail(-1, "parent window out of range");
    if (marg->device != parent->device) return fail(-1, "contexts on different devices");
    if (parent->marg) return fail(-1, "the parent is a marginalisation context");
    if (parent->shard_count > 1 || parent->comm) return fail(-1, "marginalisation from the device: not from a sharded parent");
    const WinDev &pw = parent->wd[parent_win];
    if (frame_terms->n_frames != pw.N || frame_terms->width != pw.width || frame_terms->height != pw.height)
        return fail(-1, "marginalisation window does not match the parent window's frames");
    MargPlan plan;
    int rc = plan_marg(parent->wh[parent_win], pw, *frame_terms, n_points, points, res_live, marg->item_order,
                       marg->top_chunk, plan);
    if (rc) return rc;
    marg->settings = parent->settings;
    return load_impl(marg, 1, frame_terms, 0, 1, parent, parent_win, nullptr, &plan);
}

void ldso_ba_default_flag_params(ldso_ba_flag_params *p) {
    if (p) *p = ldso_ba_flag_params{3, 4, 50.0f, 0};  // Setting.cc: minGoodActiveResForMarg, minGoodResForMarg, minIdepthH_marg
}

int ldso_ba_flag_points(ldso_ba_ctx *c, int32_t win, const ldso_ba_flag_params *params, const uint8_t *frame_flagged,
                        const int32_t *num_good, const int32_t *last_res, const int8_t *last_state, int8_t *status,
                        uint8_t *res_live, int32_t *num_good_out, int8_t *last_state_out, int32_t *counts) {
    if (!c || win < 0 || win >= c->n_win || !frame_flagged) return fail(-1, "bad arguments");
    if (c->marg) return fail(-1, "flag_points: not on a marginalisation context");
    if (c->shard_count > 1 || c->comm) return fail(-1, "flag_points: not on a sharded context");
    const WinDev &D = c->wd[win];
    const WinHost &H = c->wh[win];
    const int P = D.P, R = D.R;
    if (P > 0 && (!num_good || !last_res)) return fail(-1, "flag_points: null num_good or last_res");
    ldso_ba_flag_params fp;
    ldso_ba_default_flag_params(&fp);
    if (params) fp = *params;
    if (c->flag_map_win != win) {
        read_old(H, D, c->flag_map);
        c->flag_map_win = win;
    }
    const OldWindow &o = c->flag_map;
    for (int i = 0; i < 2 * P; i++) {
        const int k = last_res[i];
        if (k == -1) {
            if (!last_state) return fail(-1, "flag_points: last_res holds -1 and last_state is null");
            continue;
        }
        if (k < 0 || k >= R || o.rs_point[k] != i / 2)
            return fail(-1, "flag_points: last_res[" + std::to_string(i / 2) + "][" + std::to_string(i & 1) + "] = " +
                                std::to_string(k) + " is neither -1 nor a residual of its point");
    }
    // one block of 32-bit words: [num_good P | last_res 2P | last_state 2P bytes | frame_flagged 16 bytes |
    // cnt P (0) | counts 4 (0)] goes up, [counts 4 | num_good_out P | status P bytes | ls 2P bytes |
    // res_live R bytes] comes back
    const size_t w4 = sizeof(int);
    const size_t o_ng = 0, o_lr = o_ng + P, o_ls = o_lr + 2 * (size_t)P, o_ff = o_ls + pad4(2 * (size_t)P) / w4,
                 o_cnt = o_ff + LDSO_BA_MAX_FRAMES / w4, o_counts = o_cnt + P, o_ngo = o_counts + 4, o_st = o_ngo + P,
                 o_lso = o_st + pad4(P) / w4, o_live = o_lso + pad4(2 * (size_t)P) / w4, n_words = o_live + pad4(R) / w4;
    HIP_TRY(hipSetDevice(c->device));
    int rc;
    if (c->d_flag.n < n_words || c->pin_flag.n < n_words) {  // nothing of an earlier call is in flight: each ends synchronised
        const size_t grow = std::max(n_words, c->d_flag.n + c->d_flag.n / 2);
        if ((rc = c->d_flag.alloc(grow)) || (rc = c->pin_flag.ensure(grow))) return rc;
    }
    int *hp = c->pin_flag.p;
    std::memset(hp, 0, (o_counts + 4) * w4);
    int8_t *h_ls = reinterpret_cast<int8_t *>(hp + o_ls);
    for (int q = 0; q < P; q++) {
        const int p = H.pt_orig[q];
        hp[o_ng + q] = num_good[p];
        for (int i = 0; i < 2; i++) {
            const int k = last_res[2 * p + i];
            hp[o_lr + 2 * q + i] = k >= 0 ? o.rs_pos[k] : -1;
            h_ls[2 * q + i] = k >= 0 ? 0 : last_state[2 * p + i];
        }
    }
    std::memcpy(hp + o_ff, frame_flagged, (size_t)D.N);
    int *dp = c->d_flag.p;
    HIP_TRY(hipMemcpyAsync(dp, hp, (o_counts + 4) * w4, hipMemcpyHostToDevice, c->stream));
    FlagParams F{};
    F.rs_flags = c->d_rs_flags.p + D.res_base;
    F.rs_tgt = c->d_rs_tgt.p + D.res_base;
    F.rs_state = c->d_rs_state.p + D.res_base;
    F.rs_slot = c->d_rs_slot.p + D.res_base;
    F.pt_data = c->d_pt_data.p + (size_t)D.point_base * LDSO_BA_POINT_STRIDE;
    F.pt_out = c->d_pt_out.p + (size_t)D.point_base * 12;
    F.pt_host = c->d_pt_host.p + D.point_base;
    F.num_good = dp + o_ng;
    F.last_res = dp + o_lr;
    F.last_state = reinterpret_cast<const int8_t *>(dp + o_ls);
    F.frame_flagged = reinterpret_cast<const uint8_t *>(dp + o_ff);
    F.cnt = dp + o_cnt;
    F.counts = dp + o_counts;
    F.num_good_out = dp + o_ngo;
    F.status = reinterpret_cast<int8_t *>(dp + o_st);
    F.ls_out = reinterpret_cast<int8_t *>(dp + o_lso);
    F.res_live = reinterpret_cast<uint8_t *>(dp + o_live);
    F.R = R;
    F.P = P;
    F.rec_base = D.rec_base;
    F.min_good_active = fp.min_good_active_res_for_marg;
    F.min_good = fp.min_good_res_for_marg;
    F.min_idepth_h = fp.min_idepth_h_marg;
    if (R) k_flag_count<<<(R + 255) / 256, 256, 0, c->stream>>>(F);
    if (P) k_flag_decide<<<(P + 255) / 256, 256, 0, c->stream>>>(F);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(hp + o_counts, dp + o_counts, (n_words - o_counts) * w4, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    if (counts) std::memcpy(counts, hp + o_counts, 4 * w4);
    const int8_t *h_st = reinterpret_cast<const int8_t *>(hp + o_st), *h_lso = reinterpret_cast<const int8_t *>(hp + o_lso);
    for (int q = 0; q < P; q++) {
        const int p = H.pt_orig[q];
        if (status) status[p] = h_st[q];
        if (num_good_out) num_good_out[p] = hp[o_ngo + q];
        if (last_state_out) {
            last_state_out[2 * p] = h_lso[2 * q];
            last_state_out[2 * p + 1] = h_lso[2 * q + 1];
        }
    }
    if (res_live) {
        const uint8_t *h_live = reinterpret_cast<const uint8_t *>(hp + o_live);
        for (int pos = 0; pos < R; pos++) res_live[H.rs_orig[pos]] = h_live[pos];
    }
    return 0;
}

// ---- frame store ----------------------------------------------------------------------------
int ldso_ba_frames_reserve(ldso_ba_ctx *c, int32_t capacity, int32_t width, int32_t height) {
    if (!c) return fail(-1, "null ctx");
    if (capacity < 1 || capacity > 4096) return fail(-1, "frame store capacity must be in [1, 4096]");
    if (width < 4 || height < 4 || (long long)width * height > (1ll << 26)) return fail(-1, "bad frame size");
    if (c->marg) return fail(-1, "a marginalisation context borrows its parent's images and has no frame store");
    HIP_TRY(hipSetDevice(c->device));
    HIP_TRY(hipStreamSynchronize(c->stream));  // a load may still be copying out of the old slots
    FrameStore &S = c->store;
    S.cap = 0;
    S.id.clear();
    S.seq.clear();
    c->img_tag.clear();
    S.lay = image_layout(c->img_mode_pref, width, height);
    int rc = S.d_store.alloc((size_t)capacity * S.lay.frame_stride);
    c->xfer[2]++;
    if (rc) return rc;
    if ((rc = image_staging(c, S.lay.npix()))) return rc;
    if ((rc = c->pin_img.ensure(S.lay.npix() * 3 * sizeof(float) + 64))) return rc;
    S.id.assign((size_t)capacity, 0);
    S.seq.assign((size_t)capacity, 0ull);
    S.cap = capacity;
    return 0;
}

int ldso_ba_frame_put(ldso_ba_ctx *c, int64_t frame_id, const float *dI) {
    if (!c || !dI) return fail(-1, "null argument");
    FrameStore &S = c->store;
    int slot = -1;
    int rc = S.slot_for(frame_id, &slot);
    if (rc) return rc;
    HIP_TRY(hipSetDevice(c->device));
    const size_t npix = S.lay.npix(), bytes = npix * 3 * sizeof(float);
    if ((rc = image_staging(c, npix))) return rc;
    if ((rc = c->pin_img.ensure(bytes + 64))) return rc;
    // every use of the pinned frame ends behind a synchronisation, so it is free here
    std::memcpy(c->pin_img.p, dI, bytes);
    int *mismatch = reinterpret_cast<int *>(c->pin_img.p + bytes);
    *mismatch = 0;
    HIP_TRY(hipMemsetAsync(c->d_img_flag.p, 0, sizeof(int), c->stream));
    HIP_TRY(hipMemcpyAsync(c->d_img_stage.p, c->pin_img.p, bytes, hipMemcpyHostToDevice, c->stream));
    c->xfer[0] += (int64_t)bytes;
    launch_repack(S.lay, c->d_img_stage.p, S.slot(slot), c->d_img_flag.p, c->stream);
    HIP_TRY(hipGetLastError());
    if (S.lay.mode == 3) HIP_TRY(hipMemcpyAsync(mismatch, c->d_img_flag.p, sizeof(int), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    if (S.lay.mode == 3 && *mismatch) {
        S.seq[slot] = 0;  // the slot holds intensities whose recomputed gradients are not the caller's
        return fail(LDSO_BA_ERR_GRADIENT_MISMATCH,
                    "frame id " + std::to_string((long long)frame_id) +
                        ": dI's gradients are not makeImages' (FrameHessian.cc:96-101), which image layout 3 recomputes; "
                        "reserve the frame store in layout 1 (LDSO_BA_TUNE_TILED_IMAGES = 1 before ldso_ba_frames_reserve)");
    }
    S.commit(slot, frame_id);
    c->xfer[3]++;
    return 0;
}

int ldso_ba_frame_put_device(ldso_ba_ctx *c, int64_t frame_id, const float *dev_intensity, const void *dev_texels,
                             void *producer_stream) {
    if (!c) return fail(-1, "null ctx");
    if (!dev_intensity && !dev_texels) return fail(-1, "no device source: give the intensity plane and / or the texels");
    return store_ingest_device(c, frame_id, dev_intensity, dev_texels, static_cast<hipStream_t>(producer_stream));
}

int ldso_ba_frame_put_tracker(ldso_ba_ctx *c, int64_t frame_id, const ldso_ct_ctx *tracker) {
    if (!c || !tracker) return fail(-1, "null argument");
    const ImageLayout &l = c->store.lay;
    if (c->store.cap == 0) return fail(LDSO_BA_ERR_FRAME_STORE, "no frame store: call ldso_ba_frames_reserve first");
    ldso_ba::CtFrameView v{};
    int rc = ldso_ba::ct_frame_view(tracker, &v);
    if (rc) return rc;
    if (v.device != c->device) return fail(-1, "tracker and context are on different devices");
    if (v.width != l.width || v.height != l.height)
        return fail(LDSO_BA_ERR_FRAME_STORE, "tracker frame is " + std::to_string(v.width) + "x" + std::to_string(v.height) +
                                                 ", the frame store holds " + std::to_string(l.width) + "x" +
                                                 std::to_string(l.height));
    if (!v.have_frame) return fail(-1, "the tracker has no new frame: ldso_ct_set_new_frame not called");
    return store_ingest_device(c, frame_id, v.intensity, v.texels, static_cast<hipStream_t>(v.stream));
}

int ldso_ba_frame_put_initializer(ldso_ba_ctx *c, int64_t frame_id, const ldso_ct_ctx *tracker) {
    if (!c || !tracker) return fail(-1, "null argument");
    const ImageLayout &l = c->store.lay;
    if (c->store.cap == 0) return fail(LDSO_BA_ERR_FRAME_STORE, "no frame store: call ldso_ba_frames_reserve first");
    ldso_ba::CtFrameView v{};
    int rc = ldso_ba::ct_init_frame_view(tracker, &v);
    if (rc) return rc;
    if (v.device != c->device) return fail(-1, "tracker and context are on different devices");
    if (v.width != l.width || v.height != l.height)
        return fail(LDSO_BA_ERR_FRAME_STORE, "the initializer's first frame is " + std::to_string(v.width) + "x" +
                                                 std::to_string(v.height) + ", the frame store holds " +
                                                 std::to_string(l.width) + "x" + std::to_string(l.height));
    if (!v.have_frame) return fail(-1, "the tracker has no first frame: ldso_ct_init_set_first not called");
    return store_ingest_device(c, frame_id, v.intensity, v.texels, static_cast<hipStream_t>(v.stream));
}

int ldso_ba_frame_drop(ldso_ba_ctx *c, int64_t frame_id) {
    if (!c) return fail(-1, "null ctx");
    const int s = c->store.find(frame_id);
    if (s < 0)
        return fail(LDSO_BA_ERR_FRAME_STORE, "frame id " + std::to_string((long long)frame_id) + " is not resident in the frame store");
    c->store.seq[s] = 0;  // the next put into the slot is ordered behind its readers on the context stream
    return 0;
}

int ldso_ba_frame_get(ldso_ba_ctx *c, int64_t frame_id, float *intensity, float *grad) {
    if (!c || !intensity) return fail(-1, "null argument");
    const FrameStore &S = c->store;
    const ImageLayout &l = S.lay;
    const int s = S.find(frame_id);
    if (s < 0)
        return fail(LDSO_BA_ERR_FRAME_STORE, "frame id " + std::to_string((long long)frame_id) + " is not resident in the frame store");
    if (grad && l.mode != 1) return fail(-1, "image layout 3 stores no gradients: grad must be NULL");
    HIP_TRY(hipSetDevice(c->device));
    const size_t npix = l.npix();
    int rc = image_staging(c, npix);
    if (rc) return rc;
    if ((rc = c->pin_img.ensure(npix * 3 * sizeof(float) + 64))) return rc;
    float *d_i = c->d_img_stage.p, *d_g = c->d_img_stage.p + npix;
    k_slot_unpack<<<(int)((npix + 255) / 256), 256, 0, c->stream>>>(S.slot(s), l.mode, d_i, d_g, l.width, l.height,
                                                                    l.tiles_per_row);
    HIP_TRY(hipGetLastError());
    const size_t n = npix * (grad ? 3 : 1);
    HIP_TRY(hipMemcpyAsync(c->pin_img.p, d_i, n * sizeof(float), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    std::memcpy(intensity, c->pin_img.p, npix * sizeof(float));
    if (grad) std::memcpy(grad, c->pin_img.p + npix * sizeof(float), 2 * npix * sizeof(float));
    return 0;
}

int ldso_ba_load_frames(ldso_ba_ctx *c, int32_t n_windows, const ldso_ba_window *ws, const int64_t *frame_ids,
                        int32_t shard_rank, int32_t shard_count) {
    if (!c || !ws || !frame_ids) return fail(-1, "bad arguments");
    return load_impl(c, n_windows, ws, shard_rank, shard_count, nullptr, 0, frame_ids);
}

int ldso_ba_transfer_stats(ldso_ba_ctx *c, int64_t out[4]) {
    if (!c || !out) return fail(-1, "null argument");
    for (int i = 0; i < 4; i++) out[i] = c->xfer[i];
    return 0;
}

int ldso_ba_update(ldso_ba_ctx *c, int32_t win, const ldso_ba_window *w) {
    if (!c || !w || win < 0 || win >= c->n_win) return fail(-1, "bad arguments");
    c->th_host_valid = false;
    WinHost &H = c->wh[win];
    WinDev &D = c->wd[win];
    if (w->n_frames != H.N || w->n_points != H.P_all || w->n_residuals != H.R_all)
        return fail(-1, "update() cannot change the window structure; call ldso_ba_load");
    const int N = H.N;
    HIP_TRY(hipSetDevice(c->device));
    for (int i = 0; i < 4; i++) D.calib[i] = w->calib[i];
    D.adt_diag = adjoints_diagonal(w->ad_target, (size_t)N * N) ? 1 : 0;  // travels with the adjoints below
    H.c_prior.assign(w->c_prior, w->c_prior + 4);
    H.c_delta.assign(w->c_delta, w->c_delta + 4);
    H.frame_prior.assign(w->frame_prior, w->frame_prior + 8 * N);
    H.frame_delta_prior.assign(w->frame_delta_prior, w->frame_delta_prior + 8 * N);
    for (size_t k = 0; k < H.adHF.size(); k++) {
        H.adHF[k] = (float)w->ad_host[k];
        H.adTF[k] = (float)w->ad_target[k];
    }
    std::vector<float> pd(w->point_data ? (size_t)H.P * LDSO_BA_POINT_STRIDE : 0);
    if (w->point_data)
        for (int q = 0; q < H.P; q++)
            std::memcpy(&pd[(size_t)q * LDSO_BA_POINT_STRIDE],
                        w->point_data + (size_t)H.pt_orig[q] * LDSO_BA_POINT_STRIDE, LDSO_BA_POINT_STRIDE * sizeof(float));
    std::vector<double> pr;
    priors_vector(c, win, pr);
    // every array of the update through the mapped staging buffer in one launch, stream-ordered
    // (the caller's arrays are copied before this returns; no synchronisation)
    InBatch B;
    B.add(c->d_wins.p + win, &D, sizeof(WinDev));
    B.add(c->d_precalc.p + (size_t)D.pair_base * LDSO_BA_PRECALC_STRIDE, w->precalc,
          (size_t)N * N * LDSO_BA_PRECALC_STRIDE * sizeof(float));
    B.add(c->d_adH.p + (size_t)D.pair_base * 64, w->ad_host, (size_t)N * N * 64 * sizeof(double));
    B.add(c->d_adT.p + (size_t)D.pair_base * 64, w->ad_target, (size_t)N * N * 64 * sizeof(double));
    B.add(c->d_frame_th.p + D.frame_base, w->frame_energy_th, N * sizeof(float));
    B.add(c->d_prior.p + (size_t)2 * D.vec_base, pr.data(), pr.size() * sizeof(double));
    if (H.P && w->point_data)
        B.add(c->d_pt_data.p + (size_t)D.point_base * LDSO_BA_POINT_STRIDE, pd.data(), pd.size() * sizeof(float));
    c->sys_host_valid = false;
    return B.flush(c);
}

int ldso_ba_update_points(ldso_ba_ctx *c, int32_t win, const float *vals) {
    if (!c || win < 0 || win >= c->n_win || (!vals && c->wh[win].P_all > 0)) return fail(-1, "bad arguments");
    const WinHost &H = c->wh[win];
    const WinDev &D = c->wd[win];
    if (H.P == 0) return 0;
    HIP_TRY(hipSetDevice(c->device));
    int rc = c->d_pt_vals.ensure((size_t)c->P_tot);
    if (rc) return rc;
    if ((rc = c->pin_out.ensure((size_t)H.P * sizeof(float4)))) return rc;
    HIP_TRY(hipStreamSynchronize(c->stream));  // pin_out may feed an earlier copy
    float4 *st = reinterpret_cast<float4 *>(c->pin_out.p);
    for (int q = 0; q < H.P; q++) {
        const float *v = vals + 4 * (size_t)H.pt_orig[q];
        st[q] = make_float4(v[0], v[1], v[2], v[3]);
    }
    HIP_TRY(hipMemcpyAsync(c->d_pt_vals.p + D.point_base, st, (size_t)H.P * sizeof(float4), hipMemcpyHostToDevice,
                           c->stream));
    k_set_point_vals<<<(H.P + 255) / 256, 256, 0, c->stream>>>(c->d_pt_vals.p + D.point_base,
                                                              c->d_pt_data.p + (size_t)D.point_base * LDSO_BA_POINT_STRIDE, H.P);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(c->stream));
    return 0;
}

int ldso_ba_update_residuals(ldso_ba_ctx *c, int32_t win, const int8_t *state, const float *state_energy,
                             const float *new_energy, const uint8_t *flags) {
    if (!c || win < 0 || win >= c->n_win) return fail(-1, "bad arguments");
    const WinHost &H = c->wh[win];
    const WinDev &D = c->wd[win];
    if (D.R == 0) return 0;
    if (!state || !state_energy || !new_energy || !flags) return fail(-1, "bad arguments");
    HIP_TRY(hipSetDevice(c->device));
    const size_t R = (size_t)D.R;
    int rc = c->pin_out.ensure(R * (2 * sizeof(float) + 2));
    if (rc) return rc;
    HIP_TRY(hipStreamSynchronize(c->stream));
    float *se = reinterpret_cast<float *>(c->pin_out.p), *ne = se + R;
    int8_t *st = reinterpret_cast<int8_t *>(ne + R);
    uint8_t *fl = reinterpret_cast<uint8_t *>(st + R);
    for (size_t pos = 0; pos < R; pos++) {
        const int k = H.rs_orig[pos];
        se[pos] = state_energy[k];
        ne[pos] = new_energy[k];
        st[pos] = state[k];
        fl[pos] = flags[k];
    }
    HIP_TRY(hipMemcpyAsync(c->d_rs_energy.p + D.res_base, se, R * sizeof(float), hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipMemcpyAsync(c->d_rs_newenergy.p + D.res_base, ne, R * sizeof(float), hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipMemcpyAsync(c->d_rs_state.p + D.res_base, st, R, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipMemcpyAsync(c->d_rs_flags.p + D.res_base, fl, R, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return 0;
}

int ldso_ba_reset_oob(ldso_ba_ctx *c, int32_t win) {
    if (!c || win >= c->n_win) return fail(-1, "bad arguments");
    HIP_TRY(hipSetDevice(c->device));
    // resetOOB(): state_NewEnergy = state_energy = 0; state_NewState = OUTLIER; state_state = IN,
    // for the windows' residual range (contiguous: windows back to back) in one launch instead of
    // four fills per window
    const int w0 = win < 0 ? 0 : win, w1 = win < 0 ? c->n_win : win + 1;
    const long long r0 = c->wd[w0].res_base, r1 = c->wd[w1 - 1].res_base + c->wd[w1 - 1].R;
    if (r1 <= r0) return 0;
    const int n = (int)(r1 - r0);
    k_reset_oob<<<std::min(1024, (n + 255) / 256), 256, 0, c->stream>>>(
        c->d_rs_state.p + r0, c->d_rs_newstate.p + r0, c->d_rs_energy.p + r0, c->d_rs_newenergy.p + r0, n);
    HIP_TRY(hipGetLastError());
    return 0;
}

}  // extern "C"

namespace {
#define NCCL_TRY(expr)                                                                            \
    do {                                                                                          \
        ncclResult_t r_ = (expr);                                                                 \
        if (r_ != ncclSuccess) return fail(-2, std::string(#expr) + ": " + ncclGetErrorString(r_)); \
    } while (0)

// SURVEY.md §8e's exchange, stream-ordered after k_stitch on the context stream (no host
// synchronisation): one fp64 sum all-reduce of every window's packed {HA, bA, Hsc, bsc} (the priors
// are not in it: every rank adds its own copy in the solve) and of the linearizeAll energy / #IN
// pairs, then an all-gather of per-window slots -- the newest-frame NewEnergyWithOutlier values,
// after which k_frame_th re-selects the exact setNewFrameEnergyTH threshold on every rank, and,
// inside ldso_ba_optimize, the rank's run of |idepth|, from which every rank walks the window's
// whole sumNID chain (doStepFromBackup's float sum in the unsharded order: nid_source).
int comm_exchange(ldso_ba_ctx *c, bool accumulate, int pass, const Switches &sw) {
    hipStream_t st = c->stream;
    if (c->x_stride == 0) {  // first exchange since the load: agree on the slot stride and run length
        int64_t m[2] = {1, 0};
        for (const WinDev &D : c->wd) {
            m[0] = std::max<int64_t>(m[0], D.newest_end - D.newest_begin);
            m[1] = std::max<int64_t>(m[1], D.P);
        }
        m[1] = (m[1] + 3) & ~(int64_t)3;  // the chain reads float4s of one rank's run
        GraphBuf<int64_t> t;
        if (int rc = t.alloc(2)) return rc;
        HIP_TRY(hipMemcpyAsync(t.p, m, sizeof(m), hipMemcpyHostToDevice, st));
        NCCL_TRY(ncclAllReduce(t.p, t.p, 2, ncclInt64, ncclMax, c->comm, st));
        HIP_TRY(hipMemcpyAsync(m, t.p, sizeof(m), hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
        t.release();
        c->x_stride = m[0];
        c->x_prun = m[1];
        const size_t slot_max = (size_t)(m[0] + m[1]);
        if (int rc = c->d_x_local.alloc((size_t)c->n_win * slot_max)) return rc;
        if (int rc = c->d_x_gathered.alloc((size_t)c->comm_world * c->n_win * slot_max)) return rc;
    }
    const size_t nw2 = (size_t)2 * c->n_win;
    double *xb = accumulate ? c->d_sys.p : c->win_energy();
    const size_t xn = (accumulate ? c->sys_n : 0) + nw2;
    NCCL_TRY(ncclAllReduce(xb, xb, xn, ncclFloat64, ncclSum, c->comm, st));
    // inside optimize() an accumulating pass also ships the idepth runs of the next step's sumNID
    const bool nid = pass >= 0 && accumulate;
    const long long stride = c->x_stride, prun = nid ? c->x_prun : 0, slot = stride + prun;
    const dim3 grid((unsigned)std::min<long long>((slot + 255) / 256, 64), (unsigned)c->n_win);
    k_export_newest<<<grid, 256, 0, st>>>(c->d_wins.p, c->d_rs_energy_wo.p, c->d_x_local.p, stride, slot,
                                          c->d_pt_data.p, (int)prun);
    HIP_TRY(hipGetLastError());
    NCCL_TRY(ncclAllGather(c->d_x_local.p, c->d_x_gathered.p, (size_t)c->n_win * slot, ncclFloat32, c->comm, st));
    // the chains run here when the solve does not host them (exact solve modes)
    const bool chain_here = nid && !nid_in_solve(c, sw);
    NidSrc src = chain_here ? nid_source(c) : NidSrc{};
    const int* stop = pass >= 0 ? c->d_stop.p : nullptr;
    return timed_launch(c, kSlotFrameTh, st, [&] {
        k_frame_th<<<c->n_win * (chain_here ? 2 : 1), kStThreads, 0, st>>>(
            c->d_wins.p, c->d_x_gathered.p, c->comm_world, c->n_win, stride, slot, c->d_frame_th.p, src,
            chain_here ? c->win_nid() : nullptr, stop, pass);
    });
}

// k_activate's argument for n immature records at pts (the context's staging or the tracker's selection)
ActParams act_params(ldso_ba_ctx *c, int win, const ldso_ct_immature *pts, int n, int min_obs) {
    ActParams A;
    A.wins = c->d_wins.p;
    A.img = c->images();
    A.precalc = c->d_precalc.p;
    A.pts = pts;
    A.out = c->d_act_out.p;
    A.frame_stride = c->img.frame_stride;
    A.tpr = c->img.tiles_per_row;
    A.img_mode = c->img.mode;
    A.win = win;
    A.n = n;
    A.min_obs = min_obs;
    return A;
}
}  // namespace

extern "C" {

int ldso_ba_comm_unique_id(uint8_t *id_out) {
    if (!id_out) return fail(-1, "null id");
    static_assert(sizeof(ncclUniqueId) == LDSO_BA_COMM_ID_BYTES, "RCCL unique id size");
    ncclUniqueId id;
    NCCL_TRY(ncclGetUniqueId(&id));
    std::memcpy(id_out, &id, sizeof(id));
    return 0;
}

int ldso_ba_comm_init(ldso_ba_ctx *c, const uint8_t *id_in, int32_t rank, int32_t world) {
    if (!c || !id_in || world < 1 || rank < 0 || rank >= world) return fail(-1, "bad arguments");
    if (c->comm) return fail(-1, "communicator already initialised");
    HIP_TRY(hipSetDevice(c->device));
    ncclUniqueId id;
    std::memcpy(&id, id_in, sizeof(id));
    NCCL_TRY(ncclCommInitRank(&c->comm, world, id, rank));
    c->comm_rank = rank;
    c->comm_world = world;
    c->x_stride = 0;
    c->x_prun = 0;
    return 0;
}

// ldso_ba_linearize under the caller's reading of the switches.  pass: inside ldso_ba_optimize the
// index of the pass being issued (0 = the initial linearizeAll, k = the pass after step k-1), else
// -1.  A pass of the loop writes row `pass` of the energy history and the windows' sumNID / numID,
// and its launches honour the per-window loop exits (d_stop); so do the solve and the exchange.
static int linearize_pass(ldso_ba_ctx *c, int fix, int accumulate, int pass, const Switches &sw) {
    if (!c || c->n_win == 0) return fail(-1, "no windows loaded");
    int rc;
    if ((rc = ldso_ba_check_settings(&c->settings))) return rc;
    HIP_TRY(hipSetDevice(c->device));
    c->pass_issued();
    const bool in_opt = pass >= 0;
    LinParams L = lin_params(c);
    L.fix = fix;
    L.accumulate = accumulate;
    PointParams Pp = point_params(c);
    StitchParams Sp = stitch_params(c);
    Sp.ehist = in_opt && !c->comm ? c->d_ehist.p : nullptr;  // with RCCL: after the exchange
    Sp.accumulate = accumulate;
    L.stop = Pp.stop = Sp.stop = in_opt ? c->d_stop.p : nullptr;
    L.pass = Pp.pass = Sp.pass = pass;
    const size_t sc_smem = std::max<size_t>(c->sc_smem_max, 4096);  // point_nid stages >= 1024 idepths
    if (in_opt && accumulate && !nid_in_solve(c, sw) && !c->comm) {  // the next step's sumNID / numID (its backup idepths are this pass's)
        Pp.win_nid = c->win_nid();
        Pp.n_nid = c->n_win;
        Pp.nid_chunk = (int)std::min<size_t>(1024, (sc_smem / sizeof(float)) & ~(size_t)3);
    }
    // two 512-thread blocks fit a CU: split the host blocks when the doubled grid still runs at once
    Sp.hs_split = Sp.n_win + 2 * c->n_frames <= 2 * c->n_cu ? 1 : 0;
    if (sw.hs_split >= 0) Sp.hs_split = sw.hs_split;  // tests: force either
    Sp.dense_adt = sw.stitch_dense_adt ? 1 : 0;
    const bool hs = c->host_stitch;
    const int n_max = std::max(2, c->max_frames);
    const size_t st_smem = hs ? stitch_host_smem_bytes(n_max, &Sp.th_cap) : stitch_smem_bytes(c->kp_max, n_max, &Sp.th_cap);
    hipStream_t st = c->stream;
    if (L.n_items > 0) {
        rc = timed_launch_ext(c, kSlotLinearize, [&](hipEvent_t a, hipEvent_t b) {
            if (c->marg) launch_linearize<true>(c->img.mode, L.n_blocks, st, L, a, b);
            else launch_linearize<false>(c->img.mode, L.n_blocks, st, L, a, b);
        });
        if (rc) return rc;
    }
    if (accumulate && Pp.n_nid + Pp.n_items > 0) {
        rc = timed_launch(c, kSlotPointSc, st,
                          [&] { k_point_sc<<<Pp.n_nid + Pp.n_items, kScThreads, sc_smem, st>>>(Pp); });
        if (rc) return rc;
    }
    if (hs) {
        static std::once_flag once;
        std::call_once(once, [] {
            int th;
            (void)hipFuncSetAttribute((const void *)k_stitch_host, hipFuncAttributeMaxDynamicSharedMemorySize,
                                      (int)stitch_host_smem_bytes(kHostStitchMaxN, &th));
        });
    }
    // a block per window, then per host frame (host stitch; two when split) or per frame pair (records)
    const int st_grid = Sp.n_win + (hs ? (Sp.hs_split ? 2 : 1) * c->n_frames : c->n_pairs);
    rc = timed_launch(c, kSlotStitch, st, [&] {
        if (hs) k_stitch_host<<<st_grid, kHsThreads, st_smem, st>>>(Sp);
        else k_stitch<<<st_grid, kStThreads, st_smem, st>>>(Sp);
    });
    if (!rc && accumulate)
        rc = timed_launch(c, kSlotStitchSum, st, [&] {
            if (hs) k_stitch_host_sum<<<c->n_sum_blocks, 256, 0, st>>>(c->d_wins.p, c->d_sum_blocks.p, c->d_stage.p, c->d_sys.p);
            else k_stitch_sum<<<c->n_sum_blocks, 256, 0, st>>>(c->d_wins.p, c->d_sum_blocks.p, c->d_stage.p, c->d_sys.p);
        });
    if (rc || !c->comm) return rc;
    rc = comm_exchange(c, accumulate != 0, pass, sw);
    if (!rc && in_opt) {  // the reduced energies into the optimize() history
        k_energy_to_history<<<1, 256, 0, st>>>(c->win_energy(), c->d_ehist.p, pass, 2 * c->n_win);
        HIP_TRY(hipGetLastError());
    }
    return rc;
}

int ldso_ba_linearize(ldso_ba_ctx *c, int32_t fix, int32_t accumulate) {
    return linearize_pass(c, fix, accumulate, -1, read_switches());
}

// k_record_jpjdf into d_jp_out and down to the host: [R][8] in device order
int record_jpjdf(ldso_ba_ctx *c, int win, const float4 *rec_a, const float2 *rec_b, const float *geo_snap,
                 std::vector<float> &out) {
    const WinDev &D = c->wd[win];
    int rc = c->d_jp_out.ensure((size_t)D.R * 8);
    if (rc) return rc;
    k_record_jpjdf<<<(D.R + 255) / 256, 256, 0, c->stream>>>(c->d_wins.p, win, c->d_rs_slot.p, c->d_pt_host.p,
                                                            c->d_pt_data.p, rec_a, rec_b, geo_snap, c->d_jp_out.p);
    HIP_TRY(hipGetLastError());
    out.resize((size_t)D.R * 8);
    HIP_TRY(hipMemcpyAsync(out.data(), c->d_jp_out.p, out.size() * sizeof(float), hipMemcpyDeviceToHost, c->stream));
    return 0;
}

int ldso_ba_linearize_residuals(ldso_ba_ctx *c, int32_t win, int8_t *new_state, float *new_energy,
                                float *new_energy_wo, float *center, uint8_t *center_ok, float *jpjdf) {
    if (!c || win < 0 || win >= c->n_win) return fail(-1, "bad arguments");
    if (c->marg) return fail(-1, "not on a marginalisation context");
    const WinDev &D = c->wd[win];
    const WinHost &H = c->wh[win];
    // every caller slot is written: a sharded window holds only its run of the residuals
    if (H.R_all != D.R) return fail(-1, "ldso_ba_linearize_residuals: the window is sharded (single-shard only)");
    HIP_TRY(hipSetDevice(c->device));
    const size_t R = (size_t)D.R;
    if (R == 0 || D.n_top_items == 0) return 0;  // no residuals: nothing to write
    int rc;
    const size_t Rt = (size_t)c->R_tot, slots = c->d_rec_a.n;
    if ((rc = c->d_sx_state.ensure(Rt)) || (rc = c->d_sx_newstate.ensure(Rt)) || (rc = c->d_sx_flags.ensure(Rt)) ||
        (rc = c->d_sx_energy.ensure(Rt)) || (rc = c->d_sx_newenergy.ensure(Rt)) || (rc = c->d_sx_ewo.ensure(Rt)) ||
        (rc = c->d_sx_center.ensure(Rt)) || (rc = c->d_sx_rec_a.ensure(slots)) || (rc = c->d_sx_rec_b.ensure(slots)) ||
        (rc = c->d_sx_geo_snap.ensure(c->d_geo_snap.n)) ||
        (rc = c->d_sx_item.ensure((size_t)2 * c->n_top_items)))
        return rc;
    hipStream_t st = c->stream;
    const size_t b = (size_t)D.res_base;
    // resetOOB() of every residual of the window on the copies: state IN, NewState OUTLIER,
    // energies 0; the centre marked "not projected" (NaN) so a failed centre projection shows
    if (R) {  // one launch for the five fills and the flag copy
        k_reset_oob<<<std::min<int>(1024, (int)((R + 255) / 256)), 256, 0, st>>>(
            c->d_sx_state.p + b, c->d_sx_newstate.p + b, c->d_sx_energy.p + b, c->d_sx_newenergy.p + b, (int)R,
            reinterpret_cast<float *>(c->d_sx_center.p) + b, (long long)Rt, c->d_sx_flags.p + b, c->d_rs_flags.p + b);
        HIP_TRY(hipGetLastError());
    }
    LinParams L = lin_params(c);  // this window's items on the scratch state, nothing accumulated
    L.rs_state = c->d_sx_state.p;
    L.rs_newstate = c->d_sx_newstate.p;
    L.rs_flags = c->d_sx_flags.p;
    L.rs_energy = c->d_sx_energy.p;
    L.rs_newenergy = c->d_sx_newenergy.p;
    L.rs_energy_wo = c->d_sx_ewo.p;
    L.rs_center = reinterpret_cast<float *>(c->d_sx_center.p);
    L.rec_a = c->d_sx_rec_a.p;
    L.rec_b = c->d_sx_rec_b.p;
    L.geo_snap = c->d_sx_geo_snap.p;
    L.top_slab = nullptr;
    L.item_energy = c->d_sx_item.p;
    L.item_base = D.top_item_base;
    L.n_items = D.n_top_items;
    L.n_blocks = (L.n_items + 3) / 4;
    rc = timed_launch(c, kSlotLinearize, st, [&] {
        if (c->marg) launch_linearize<true>(c->img.mode, L.n_blocks, st, L);
        else launch_linearize<false>(c->img.mode, L.n_blocks, st, L);
    });
    if (rc) return rc;
    std::vector<int8_t> ns(R);
    std::vector<float> ne(R), ew(R);
    std::vector<float4> ce(R);
    HIP_TRY(hipMemcpyAsync(ns.data(), c->d_sx_newstate.p + b, R, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(ne.data(), c->d_sx_newenergy.p + b, R * sizeof(float), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(ew.data(), c->d_sx_ewo.p + b, R * sizeof(float), hipMemcpyDeviceToHost, st));
    for (int k = 0; k < 4; k++)  // the planes back into (x, y, z, relBS) per residual
        HIP_TRY(hipMemcpy2DAsync(reinterpret_cast<float *>(ce.data()) + k, sizeof(float4),
                                 reinterpret_cast<const float *>(c->d_sx_center.p) + (size_t)k * Rt + b, sizeof(float),
                                 sizeof(float), R, hipMemcpyDeviceToHost, st));
    std::vector<float> jp;
    if (jpjdf && (rc = record_jpjdf(c, win, c->d_sx_rec_a.p, c->d_sx_rec_b.p, c->d_sx_geo_snap.p, jp))) return rc;
    if ((rc = ldso_ba_sync(c))) return rc;
    for (size_t pos = 0; pos < R; pos++) {
        const int k = H.rs_orig[pos];
        const bool cok = !std::isnan(ce[pos].x);
        if (new_state) new_state[k] = ns[pos];
        if (new_energy) new_energy[k] = ne[pos];
        if (new_energy_wo) new_energy_wo[k] = ew[pos];
        if (center_ok) center_ok[k] = cok ? 1 : 0;
        if (center) {
            center[3 * k] = cok ? ce[pos].x : 0.f;
            center[3 * k + 1] = cok ? ce[pos].y : 0.f;
            center[3 * k + 2] = cok ? ce[pos].z : 0.f;
        }
        if (jpjdf) {
            float v[8] = {0, 0, 0, 0, 0, 0, 0, 0};
            if (ns[pos] == LDSO_BA_RES_IN) std::memcpy(v, &jp[8 * pos], sizeof(v));
            std::memcpy(jpjdf + 8 * (size_t)k, v, sizeof(v));
        }
    }
    return 0;
}

int ldso_ba_activate_points(ldso_ba_ctx *c, int32_t win, int32_t n, const ldso_ct_immature *pts, int32_t min_obs,
                            ldso_ba_activation *out) {
    if (!c || win < 0 || win >= c->n_win || n < 0 || (n > 0 && (!pts || !out))) return fail(-1, "bad arguments");
    const int N = c->wh[win].N;
    for (int k = 0; k < n; k++)
        if (pts[k].host < 0 || pts[k].host >= N) return fail(-1, "immature point host index outside the window");
    if (n == 0) return 0;
    HIP_TRY(hipSetDevice(c->device));
    if ((size_t)n > c->d_act_in.n || (size_t)n > c->d_act_out.n || !c->d_act_in.p || !c->d_act_out.p) {
        int rc = c->d_act_in.alloc(n);
        if (!rc) rc = c->d_act_out.alloc(n);
        if (rc) return rc;
    }
    HIP_TRY(hipMemcpyAsync(c->d_act_in.p, pts, (size_t)n * sizeof(ldso_ct_immature), hipMemcpyHostToDevice, c->stream));
    const ActParams A = act_params(c, win, c->d_act_in.p, n, min_obs);
    int rc = timed_launch(c, kSlotActivate, c->stream, [&] { k_activate<<<(n + 3) / 4, 256, 0, c->stream>>>(A); });
    if (rc) return rc;
    HIP_TRY(hipMemcpyAsync(out, c->d_act_out.p, (size_t)n * sizeof(ldso_ba_activation), hipMemcpyDeviceToHost,
                           c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return 0;
}

int ldso_ba_activate_points_tracker(ldso_ba_ctx *c, int32_t win, const ldso_ct_ctx *tracker, int32_t min_obs,
                                    ldso_ba_activation *out) {
    if (!c || win < 0 || win >= c->n_win || !tracker) return fail(-1, "bad arguments");
    CtSelectionView V;
    int rc = ct_selection_view(tracker, &V);
    if (rc) return rc;
    if (V.device != c->device) return fail(-1, "the tracker is on a different device");
    if (V.n < 0) return fail(-1, "the tracker holds no selection: call ldso_ct_select_activation first");
    if (V.n_hosts != c->wh[win].N) return fail(-1, "the selection's n_hosts differs from the window's frame count");
    const int n = V.n;
    if (n == 0) return 0;
    if (!out) return fail(-1, "bad arguments");
    HIP_TRY(hipSetDevice(c->device));
    if ((size_t)n > c->d_act_out.n || !c->d_act_out.p)
        if ((rc = c->d_act_out.alloc(n))) return rc;
    // read the records behind what the tracker's stream holds now; its later work waits for the read
    hipStream_t ts = static_cast<hipStream_t>(V.stream);
    if ((rc = c->act_borrow.begin(c->stream, ts))) return rc;
    const ActParams A = act_params(c, win, static_cast<const ldso_ct_immature *>(V.records), n, min_obs);
    rc = timed_launch(c, kSlotActivate, c->stream, [&] { k_activate<<<(n + 3) / 4, 256, 0, c->stream>>>(A); });
    if (rc) return rc;
    if ((rc = c->act_borrow.end(c->stream, ts))) return rc;
    HIP_TRY(hipMemcpyAsync(out, c->d_act_out.p, (size_t)n * sizeof(ldso_ba_activation), hipMemcpyDeviceToHost,
                           c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return 0;
}

int ldso_ba_marginalize_points(ldso_ba_ctx *c, const float *ad_ht_delta, double *H, double *b) {
    if (!c || !ad_ht_delta || !H || !b) return fail(-1, "bad arguments");
    if (!c->marg || c->n_win != 1) return fail(-1, "not a marginalisation context (ldso_ba_load_marginalization)");
    HIP_TRY(hipSetDevice(c->device));
    const WinDev &D = c->wd[0];
    HIP_TRY(hipMemcpyAsync(c->d_adhtd.p, ad_ht_delta, (size_t)D.N * D.N * 8 * sizeof(float), hipMemcpyHostToDevice,
                           c->stream));
    int rc = ldso_ba_reset_oob(c, 0);
    if (rc) return rc;
    rc = ldso_ba_linearize(c, 0, 1);
    if (rc) return rc;
    const int n = D.D;
    std::vector<double> Hsc((size_t)n * n), bsc(n);
    rc = ldso_ba_get_system(c, 0, H, b, nullptr, nullptr, Hsc.data(), bsc.data());
    if (rc) return rc;
    for (size_t i = 0; i < (size_t)n * n; i++) H[i] -= Hsc[i];  // EnergyFunctional.cc:242-243
    for (int i = 0; i < n; i++) b[i] -= bsc[i];
    return 0;
}

int ldso_ba_sync(ldso_ba_ctx *c) {
    if (!c) return fail(-1, "null ctx");
    HIP_TRY(hipSetDevice(c->device));
    HIP_TRY(hipStreamSynchronize(c->stream));
    c->timer.drain();
    return 0;
}

int ldso_ba_get_energy(ldso_ba_ctx *c, int32_t win, double *out) {
    if (!c || !out || win < 0 || win >= c->n_win) return fail(-1, "bad arguments");
    int rc = ldso_ba_sync(c);
    if (rc) return rc;
    double e[2];
    HIP_TRY(hipMemcpy(e, c->win_energy() + 2 * win, sizeof(e), hipMemcpyDeviceToHost));
    out[0] = e[0];
    out[1] = 0;
    out[2] = e[1];
    return 0;
}

// n point steps from point `base` on into pin_step (grown as needed), synchronised
static int fetch_point_steps(ldso_ba_ctx *c, int base, int n) {
    int rc = c->pin_step.ensure((size_t)n);
    if (rc) return rc;
    if (n) HIP_TRY(hipMemcpyAsync(c->pin_step.p, c->d_pt_step.p + base, n * sizeof(float), hipMemcpyDeviceToHost, c->stream));
    return ldso_ba_sync(c);
}

// download one window's packed system (through pinned staging) unless the host copy is fresh
static int fetch_sys(ldso_ba_ctx *c, int win) {
    if (!c->sys_host_valid) {
        c->sys_valid.assign(c->n_win, 0);
        c->sys_host.resize(c->sys_n);
        c->sys_host_valid = true;
    }
    if (c->sys_valid[win]) return 0;
    const WinDev &D = c->wd[win];
    const size_t n = (size_t)sys_len(D.D);
    int rc = c->pin_sys.ensure(n);
    if (rc) return rc;
    HIP_TRY(hipSetDevice(c->device));
    HIP_TRY(hipMemcpyAsync(c->pin_sys.p, c->d_sys.p + D.sys_base, n * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    if ((rc = ldso_ba_sync(c))) return rc;
    std::memcpy(c->sys_host.data() + D.sys_base, c->pin_sys.p, n * sizeof(double));
    c->sys_valid[win] = 1;
    return 0;
}

static void expand(const double *packed, int D, double *full) {
    long long q = 0;
    for (int r = 0; r < D; r++)
        for (int col = r; col < D; col++, q++) full[(size_t)r * D + col] = full[(size_t)col * D + r] = packed[q];
}

int ldso_ba_get_system(ldso_ba_ctx *c, int32_t win, double *HA, double *bA, double *HL, double *bL, double *Hsc,
                       double *bsc) {
    if (!c || win < 0 || win >= c->n_win) return fail(-1, "bad arguments");
    int rc = fetch_sys(c, win);
    if (rc) return rc;
    const WinDev &D = c->wd[win];
    const int n = D.D;
    const long long pl = packed_len(n);
    const double *s = c->sys_host.data() + D.sys_base;
    if (HA) expand(s, n, HA);
    if (bA) std::memcpy(bA, s + pl, n * sizeof(double));
    if (Hsc) expand(s + pl + n, n, Hsc);
    if (bsc) std::memcpy(bsc, s + 2 * pl + n, n * sizeof(double));
    // HL / bL: accumulateLF_MT in the hot path has no linearized residuals, so it is exactly the
    // priors of stitchDoubleInternal(usePrior=true) (AccumulatedTopHessian.cc:241-250).
    std::vector<double> pr;  // [q] = {HL(q, q), bL(q)}
    if (HL || bL) priors_vector(c, win, pr);
    if (HL) {
        std::memset(HL, 0, sizeof(double) * n * n);
        for (int q = 0; q < n; q++) HL[(size_t)q * n + q] = pr[2 * q];
    }
    if (bL)
        for (int q = 0; q < n; q++) bL[q] = pr[2 * q + 1];
    return 0;
}

int ldso_ba_solve(ldso_ba_ctx *c, int32_t win, int32_t iteration, double lambda, const double *ns, int32_t n_null,
                  double *x_out) {
    if (!c || !x_out || win < 0 || win >= c->n_win) return fail(-1, "bad arguments");
    const int n = c->wd[win].D;
    std::vector<double> HA((size_t)n * n), bA(n), HL((size_t)n * n), bL(n), Hsc((size_t)n * n), bsc(n);
    int rc = ldso_ba_get_system(c, win, HA.data(), bA.data(), HL.data(), bL.data(), Hsc.data(), bsc.data());
    if (rc) return rc;
    return ldso_ba_solve_system(&c->settings, c->wh[win].N, iteration, lambda, HA.data(), bA.data(), HL.data(),
                                bL.data(), nullptr, nullptr, Hsc.data(), bsc.data(), ns, n_null, x_out);
}

int ldso_ba_get_residuals(ldso_ba_ctx *c, int32_t win, int8_t *new_state, int8_t *state, float *state_energy,
                          float *new_energy_wo, float *center, uint8_t *flags, float *jpjdf, float *rel_bs) {
    if (!c || win < 0 || win >= c->n_win) return fail(-1, "bad arguments");
    int rc = ldso_ba_sync(c);
    if (rc) return rc;
    const WinDev &D = c->wd[win];
    const WinHost &H = c->wh[win];
    const int R = D.R;
    if (R == 0) return 0;
    // only the arrays the caller asked for cross PCIe (a NULL output costs nothing)
    std::vector<int8_t> ns(new_state ? R : 0), st(state ? R : 0);
    std::vector<uint8_t> fl(flags ? R : 0);
    std::vector<float> se(state_energy ? R : 0), ew(new_energy_wo ? R : 0);
    std::vector<float4> ce(center || rel_bs ? R : 0);
    if (new_state) HIP_TRY(hipMemcpy(ns.data(), c->d_rs_newstate.p + D.res_base, R, hipMemcpyDeviceToHost));
    if (state) HIP_TRY(hipMemcpy(st.data(), c->d_rs_state.p + D.res_base, R, hipMemcpyDeviceToHost));
    if (flags) HIP_TRY(hipMemcpy(fl.data(), c->d_rs_flags.p + D.res_base, R, hipMemcpyDeviceToHost));
    if (state_energy)
        HIP_TRY(hipMemcpy(se.data(), c->d_rs_energy.p + D.res_base, R * sizeof(float), hipMemcpyDeviceToHost));
    if (new_energy_wo)
        HIP_TRY(hipMemcpy(ew.data(), c->d_rs_energy_wo.p + D.res_base, R * sizeof(float), hipMemcpyDeviceToHost));
    for (int k = 0; k < 4 && (center || rel_bs); k++) {  // the planes back into (x, y, z, relBS) per residual
        if ((k < 3 && !center) || (k == 3 && !rel_bs)) continue;
        HIP_TRY(hipMemcpy2D(reinterpret_cast<float *>(ce.data()) + k, sizeof(float4),
                            reinterpret_cast<const float *>(c->d_rs_center.p) + (size_t)k * c->R_tot + D.res_base,
                            sizeof(float), sizeof(float), R, hipMemcpyDeviceToHost));
    }
    std::vector<float> jp;
    if (jpjdf) {
        if ((rc = record_jpjdf(c, win, c->d_rec_a.p, c->d_rec_b.p, c->d_geo_snap.p, jp))) return rc;
        HIP_TRY(hipStreamSynchronize(c->stream));
    }
    for (int pos = 0; pos < R; pos++) {
        const int k = H.rs_orig[pos];
        if (new_state) new_state[k] = ns[pos];
        if (state) state[k] = st[pos];
        if (state_energy) state_energy[k] = se[pos];
        if (new_energy_wo) new_energy_wo[k] = ew[pos];
        if (center) {
            center[3 * k] = ce[pos].x;
            center[3 * k + 1] = ce[pos].y;
            center[3 * k + 2] = ce[pos].z;
        }
        if (flags) flags[k] = fl[pos];
        if (rel_bs) rel_bs[k] = ce[pos].w;
        if (jpjdf) std::memcpy(jpjdf + 8 * (size_t)k, &jp[8 * (size_t)pos], 8 * sizeof(float));
    }
    return 0;
}

int ldso_ba_get_points(ldso_ba_ctx *c, int32_t win, float *HdiF, float *bdSumF, float *ih, float *Hdd, float *bd,
                       float *Hcd) {
    if (!c || win < 0 || win >= c->n_win) return fail(-1, "bad arguments");
    int rc = ldso_ba_sync(c);
    if (rc) return rc;
    const WinDev &D = c->wd[win];
    const WinHost &H = c->wh[win];
    if (D.P == 0) return 0;
    std::vector<float> o((size_t)D.P * 12);
    HIP_TRY(hipMemcpy(o.data(), c->d_pt_out.p + (size_t)D.point_base * 12, o.size() * sizeof(float), hipMemcpyDeviceToHost));
    for (int q = 0; q < D.P; q++) {
        const int p = H.pt_orig[q];
        const float *v = &o[(size_t)q * 12];
        if (HdiF) HdiF[p] = v[0];
        if (bdSumF) bdSumF[p] = v[1];
        if (ih) ih[p] = v[2];
        if (Hdd) Hdd[p] = v[3];
        if (bd) bd[p] = v[4];
        if (Hcd)
            for (int i = 0; i < 4; i++) Hcd[4 * (size_t)p + i] = v[5 + i];
    }
    return 0;
}

int ldso_ba_get_point_data(ldso_ba_ctx *c, int32_t win, float *point_data) {
    if (!c || !point_data || win < 0 || win >= c->n_win) return fail(-1, "bad arguments");
    int rc = ldso_ba_sync(c);
    if (rc) return rc;
    const WinDev &D = c->wd[win];
    const WinHost &H = c->wh[win];
    if (D.P == 0) return 0;
    std::vector<float> o((size_t)D.P * LDSO_BA_POINT_STRIDE);
    HIP_TRY(hipMemcpy(o.data(), c->d_pt_data.p + (size_t)D.point_base * LDSO_BA_POINT_STRIDE, o.size() * sizeof(float),
                      hipMemcpyDeviceToHost));
    for (int q = 0; q < D.P; q++)
        std::memcpy(point_data + (size_t)H.pt_orig[q] * LDSO_BA_POINT_STRIDE, &o[(size_t)q * LDSO_BA_POINT_STRIDE],
                    LDSO_BA_POINT_STRIDE * sizeof(float));
    return 0;
}

int ldso_ba_get_frame_energy_th(ldso_ba_ctx *c, int32_t win, float *th) {
    if (!c || !th || win < 0 || win >= c->n_win) return fail(-1, "bad arguments");
    if (c->th_host_valid) {  // ldso_ba_optimize brought it back with its other results
        std::memcpy(th, c->th_host.data() + c->wd[win].frame_base, c->wd[win].N * sizeof(float));
        return 0;
    }
    int rc = ldso_ba_sync(c);
    if (rc) return rc;
    HIP_TRY(hipMemcpy(th, c->d_frame_th.p + c->wd[win].frame_base, c->wd[win].N * sizeof(float), hipMemcpyDeviceToHost));
    return 0;
}

int ldso_ba_resubstitute(ldso_ba_ctx *c, int32_t win, const double *x, double lambda, float *point_step_out) {
    if (!c || !x || win < 0 || win >= c->n_win) return fail(-1, "bad arguments");
    HIP_TRY(hipSetDevice(c->device));
    const WinDev &D = c->wd[win];
    const WinHost &H = c->wh[win];
    const int N = H.N;
    // xAd[N*h + t] = x_h^T adHostF[h + N t] + x_t^T adTargetF[h + N t] (EnergyFunctional.cc:624-632)
    const size_t nx = (size_t)N * N * 8 + 4;
    // the largest window's size, once
    int rc = c->pin_xad.ensure((size_t)LDSO_BA_MAX_FRAMES * LDSO_BA_MAX_FRAMES * 8 + 4);
    if (rc) return rc;
    HIP_TRY(hipStreamSynchronize(c->stream));  // a previous upload from pin_xad has completed
    std::vector<float> xF(D.D);
    float *host = c->pin_xad.p;
    for (int i = 0; i < D.D; i++) xF[i] = (float)x[i];
    for (int h = 0; h < N; h++)
        for (int t = 0; t < N; t++) {
            const float *AH = &H.adHF[(size_t)(h + N * t) * 64], *AT = &H.adTF[(size_t)(h + N * t) * 64];
            for (int cc = 0; cc < 8; cc++) {
                float s1 = 0, s2 = 0;
                for (int k = 0; k < 8; k++) s1 += xF[4 + 8 * h + k] * AH[k * 8 + cc];
                for (int k = 0; k < 8; k++) s2 += xF[4 + 8 * t + k] * AT[k * 8 + cc];
                host[(size_t)(N * h + t) * 8 + cc] = s1 + s2;
            }
        }
    for (int i = 0; i < 4; i++) host[(size_t)N * N * 8 + i] = xF[i];
    HIP_TRY(hipMemcpyAsync(c->d_xad.p + (size_t)win * kXadStride, host, nx * sizeof(float), hipMemcpyHostToDevice,
                           c->stream));
    if (D.P > 0) {
        int rc = launch_resubstitute(c, D.point_base, D.P, lambda);
        if (rc) return rc;
    }
    if (point_step_out) {
        int rc = fetch_point_steps(c, D.point_base, D.P);
        if (rc) return rc;
        for (int q = 0; q < D.P; q++) point_step_out[H.pt_orig[q]] = c->pin_step.p[q];
    }
    return 0;
}

// ---- device-side solve / resubstitute ----------------------------------
}  // extern "C"
namespace {
// The caller's nullspaces (every window's [7][D] back to back) to d_ns and k_ortho_prep's
// normalised Nm, G and G^-1 for n_null of them; skipped when they equal the last prepared ones.
int upload_nullspaces(ldso_ba_ctx *c, const double *ns, int n_null) {
    const size_t cnt = (size_t)7 * c->vec_total;
    if (c->ns_cache_null == n_null && c->ns_cache.size() == cnt &&
        std::memcmp(c->ns_cache.data(), ns, cnt * sizeof(double)) == 0)
        return 0;
    HIP_TRY(hipMemcpyAsync(c->d_ns.p, ns, cnt * sizeof(double), hipMemcpyHostToDevice, c->stream));
    const int dmax = c->dmax();
    if (dmax > kSolveMaxDim) return fail(-1, "device solve supports windows of up to 11 keyframes");
    SolveParams S{};
    S.wins = c->d_wins.p;
    S.ns = c->d_ns.p;
    S.iteration = 2;
    S.n_null = n_null;
    const size_t smem = solve_smem_bytes(dmax) + 16 + (size_t)7 * dmax * sizeof(double);
    static std::once_flag once;
    std::call_once(once, [] {
        (void)hipFuncSetAttribute((const void *)k_ortho_prep, hipFuncAttributeMaxDynamicSharedMemorySize,
                                  (int)(solve_smem_bytes(kSolveMaxDim) + 16 + (size_t)7 * kSolveMaxDim * sizeof(double)));
    });
    k_ortho_prep<<<c->n_win, 64, smem, c->stream>>>(S, c->d_ns_nm.p, c->d_ns_g.p);
    HIP_TRY(hipGetLastError());
    c->ns_cache.assign(ns, ns + cnt);
    c->ns_cache_null = n_null;
    return 0;
}
// SOLVER_ORTHOGONALIZE_X_LATER in the context's solver mode: the solve projects x from iteration 2
// (EnergyFunctional.cc:428-432); without it the nullspaces are ignored
inline bool ortho_x_later(const ldso_ba_ctx *c) {
    return (c->settings.solver_mode & LDSO_BA_SOLVER_ORTHOGONALIZE_X_LATER) != 0;
}
// k_solve_fast (or the exact k_solve_reg / k_solve) for every loaded window; n_null > 0 projects
// with the nullspaces upload_nullspaces prepared (iteration >= 2), n_null == 0 does not project;
// pass as linearize_pass's: the index of the loop's last pass, or -1 outside ldso_ba_optimize
int solve_device_launch(ldso_ba_ctx *c, int iteration, int n_null, int pass, const Switches &sw) {
    const int dmax = c->dmax();
    if (dmax > kSolveMaxDim) return fail(-1, "device solve supports windows of up to 11 keyframes");
    SolveParams S{};
    S.wins = c->d_wins.p;
    S.sys = c->d_sys.p;
    S.prior = c->d_prior.p;
    S.ns = c->d_ns.p;
    S.x = c->d_x.p;
    S.adH = c->d_adH.p;
    S.adT = c->d_adT.p;
    S.xad = c->d_xad.p;  // the resubstitution's xAd comes with x (k_xad after the LDS kernel)
    S.prep_nm = c->d_ns_nm.p;
    S.prep_g = c->d_ns_g.p;
    S.iteration = iteration;
    S.n_null = iteration >= 2 ? n_null : 0;
    if (pass >= 0) {  // inside ldso_ba_optimize: the per-window loop exits
        S.stop = c->d_stop.p;
        S.status = c->d_status.p;
    }
    static std::once_flag once;
    std::call_once(once, [] {
        (void)hipFuncSetAttribute((const void *)k_solve, hipFuncAttributeMaxDynamicSharedMemorySize,
                                  (int)solve_smem_bytes(kSolveMaxDim));
        (void)hipFuncSetAttribute((const void *)k_solve_reg, hipFuncAttributeMaxDynamicSharedMemorySize,
                                  (int)solve_reg_smem_bytes(kSolveRegDim));
        (void)hipFuncSetAttribute((const void *)k_solve_fast, hipFuncAttributeMaxDynamicSharedMemorySize,
                                  (int)solve_fast_smem_bytes(kSolveMaxDim));
    });
    if (nid_in_solve(c, sw)) {  // the default: unpivoted, xAd fused; the sumNID chains run beside it
        const size_t smem = solve_fast_smem_bytes(dmax);
        int grid = c->n_win;
        if (pass >= 0) {  // the step's sumNID chains in blocks of their own
            S.win_nid = c->win_nid();
            S.nid_src = nid_source(c);
            S.n_win = c->n_win;
            S.nid_chunk = (int)std::min<size_t>(1024, (smem / sizeof(float)) & ~(size_t)3);
            grid *= 2;
        }
        return timed_launch(c, kSlotSolve, c->stream,
                            [&] { k_solve_fast<<<grid, kSolveFastThreads, smem, c->stream>>>(S); });
    }
    // exact mode: windows of up to 7 keyframes (n <= 64) the register factorisation, larger the LDS one
    const bool reg = dmax <= kSolveRegDim && !sw.solve_lds;
    const size_t smem = reg ? solve_reg_smem_bytes(dmax) : solve_smem_bytes(dmax);
    int rc = timed_launch(c, kSlotSolve, c->stream, [&] {
        if (reg)
            k_solve_reg<<<c->n_win, kSolveRegThreads, smem, c->stream>>>(S);
        else
            k_solve<<<c->n_win, kSolveThreads, smem, c->stream>>>(S);
    });
    if (rc) return rc;
    if (!reg) {
        k_xad<<<c->n_win, 256, 0, c->stream>>>(c->d_wins.p, c->d_x.p, c->d_adH.p, c->d_adT.p, c->d_xad.p);
        HIP_TRY(hipGetLastError());
    }
    return 0;
}
}  // namespace
extern "C" {

// The projection (iteration >= 2) uses the nullspaces passed in THIS call; without them the
// solve does not project, exactly as the host solver (ldso_ba_solve / ldso_ba_solve_system).
int ldso_ba_solve_device(ldso_ba_ctx *c, int32_t iteration, double lambda, const double *ns, int32_t n_null,
                         double *x_out) {
    (void)lambda;  // SOLVER_FIX_LAMBDA, as the host solver
    if (!c || c->n_win == 0) return fail(-1, "no windows loaded");
    if (n_null < 0 || n_null > 7) return fail(-1, "n_null must be in [0, 7]");
    int rc;
    if ((rc = ldso_ba_check_settings(&c->settings))) return rc;
    HIP_TRY(hipSetDevice(c->device));
    const bool project = iteration >= 2 && ns && n_null > 0 && ortho_x_later(c);
    if (project && (rc = upload_nullspaces(c, ns, n_null))) return rc;
    rc = solve_device_launch(c, iteration, project ? n_null : 0, -1, read_switches());
    if (rc) return rc;
    if (x_out) {
        HIP_TRY(hipMemcpyAsync(x_out, c->d_x.p, (size_t)c->vec_total * sizeof(double), hipMemcpyDeviceToHost,
                               c->stream));
        rc = ldso_ba_sync(c);
        if (rc) return rc;
    }
    return 0;
}

int ldso_ba_resubstitute_device(ldso_ba_ctx *c, double lambda, float *point_step_out) {
    if (!c || c->n_win == 0) return fail(-1, "no windows loaded");
    HIP_TRY(hipSetDevice(c->device));
    k_xad<<<c->n_win, 256, 0, c->stream>>>(c->d_wins.p, c->d_x.p, c->d_adH.p, c->d_adT.p, c->d_xad.p);
    HIP_TRY(hipGetLastError());
    if (c->P_tot > 0) {
        int rc = launch_resubstitute(c, 0, c->P_tot, lambda);
        if (rc) return rc;
    }
    if (point_step_out) {
        int rc = fetch_point_steps(c, 0, c->P_tot);
        if (rc) return rc;
        scatter_points(c, c->pin_step.p, point_step_out);
    }
    return 0;
}

}  // extern "C"
namespace {
// The launch parameters a captured pass / solve sequence depends on besides the call's own
// arguments: the solve kernel (exact or fast), the stitch split, and every setting the kernels read.
std::vector<unsigned long long> capture_key(const ldso_ba_ctx *c, const Switches &sw) {
    unsigned a, b, th;
    std::memcpy(&a, &c->settings.affine_opt_mode_a, 4);
    std::memcpy(&b, &c->settings.affine_opt_mode_b, 4);
    std::memcpy(&th, &c->settings.th_opt_iterations, 4);
    return {(unsigned long long)c->solve_exact, (unsigned long long)sw.solve_lds,
            (unsigned long long)(sw.hs_split < 0 ? 0 : sw.hs_split == 1 ? 1 : 2), (unsigned long long)sw.stitch_dense_adt,
            (unsigned long long)(unsigned)c->settings.solver_mode,
            (unsigned long long)(unsigned)c->settings.min_opt_iterations, a, b, th};
}
// Launch a captured sequence: replay g if it was captured under the current allocation
// generation and key, else capture `body`'s launches on the context stream, instantiate, cache.
template <typename F>
int launch_cached_graph(ldso_ba_ctx *c, ldso_ba_ctx::Graph &g, const std::vector<unsigned long long> &key, F &&body) {
    const unsigned long long gen = g_alloc_gen.load();
    if (g.exec && (g.gen != gen || g.key != key)) g.reset();
    if (!g.exec) {
        hipGraph_t gr = nullptr;
        HIP_TRY(hipStreamBeginCapture(c->stream, hipStreamCaptureModeThreadLocal));
        const int rcap = body();
        const hipError_t ecap = hipStreamEndCapture(c->stream, &gr);
        if (rcap || ecap != hipSuccess) {
            if (gr) (void)hipGraphDestroy(gr);
            return rcap ? rcap : fail(-2, std::string("graph capture: ") + hipGetErrorString(ecap));
        }
        const hipError_t ei = hipGraphInstantiate(&g.exec, gr, nullptr, nullptr, 0);
        (void)hipGraphDestroy(gr);
        if (ei != hipSuccess) {
            g.exec = nullptr;
            return fail(-2, std::string("graph instantiate: ") + hipGetErrorString(ei));
        }
        g.gen = gen;
        g.key = key;
    }
    const hipError_t el = hipGraphLaunch(g.exec, c->stream);
    if (el != hipSuccess) return fail(-2, std::string("graph launch: ") + hipGetErrorString(el));
    c->pass_issued();  // a replay skips the host side of the captured calls
    return 0;
}
}  // namespace
extern "C" {

int ldso_ba_iterate(ldso_ba_ctx *c, int32_t iteration, double lambda, const double *ns, int32_t n_null, double *x_out,
                    float *point_step_out, double *energy_out) {
    if (!c || c->n_win == 0) return fail(-1, "no windows loaded");
    if (n_null < 0 || n_null > 7) return fail(-1, "n_null must be in [0, 7]");
    int rc;
    if ((rc = ldso_ba_check_settings(&c->settings))) return rc;
    HIP_TRY(hipSetDevice(c->device));
    // the projection uses the nullspaces of THIS call (as ldso_ba_solve_device)
    const bool project = iteration >= 2 && n_null > 0 && ns && ortho_x_later(c);
    if (project && (rc = upload_nullspaces(c, ns, n_null)))  // before (outside) the captured sequence
        return rc;
    // pass + solve + resubstitution (LDSO_BA_ITERATE_GRAPH=1: one captured graph per (projection,
    // lambda, n_null) without a communicator or kernel timing); the downloads stay outside it
    const Switches sw = read_switches();  // one reading for the launches and the graph's key
    auto body = [&]() -> int {
        int r;
        if ((r = linearize_pass(c, 0, 1, -1, sw))) return r;
        if ((r = solve_device_launch(c, project ? 2 : 0, project ? n_null : 0, -1, sw))) return r;
        return c->P_tot > 0 ? launch_resubstitute(c, 0, c->P_tot, lambda) : 0;
    };
    // direct launches by default: for this six-launch sequence hipGraphLaunch costs more host
    // time than it saves (one S7 window: 89 vs 95 us per call, tools/iter_probe.py)
    if (!c->comm && !c->timer.on && sw.iterate_graph && !sw.no_graph) {
        unsigned long long lb;
        std::memcpy(&lb, &lambda, sizeof(lb));
        // keyed by everything fixed at capture: lambda, n_null, the solve kernel, the stitch split,
        // the settings the pass reads
        std::vector<unsigned long long> key = capture_key(c, sw);
        key.push_back(lb);
        key.push_back((unsigned long long)n_null);
        rc = launch_cached_graph(c, c->it_graph[project ? 1 : 0], key, body);
    } else {
        rc = body();
    }
    if (rc) return rc;
    // x, the energies and the point steps into the mapped results buffer (one launch), one
    // synchronisation
    const size_t xb = (size_t)c->vec_total * sizeof(double), eb = (size_t)2 * c->n_win * sizeof(double),
                 sb = (size_t)c->P_tot * sizeof(float);
    if ((rc = pin_map_ensure(c, xb + eb + sb))) return rc;
    const double *px = reinterpret_cast<const double *>(c->pin_map.p), *pe = px + c->vec_total;
    const float *ps = reinterpret_cast<const float *>(pe + 2 * c->n_win);
    {
        PackOut K{};
        char *pd = c->pin_map.dev;
        if (x_out) pack_seg(K, c->d_x.p, pd, xb);
        if (energy_out) pack_seg(K, c->win_energy(), pd + xb, eb);
        if (point_step_out && sb) pack_seg(K, c->d_pt_step.p, pd + xb + eb, sb);
        if (K.n_seg) {
            k_pack_out<<<std::min(64, (int)((xb + eb + sb) / 1024) + 1), 256, 0, c->stream>>>(K);
            HIP_TRY(hipGetLastError());
        }
    }
    if ((rc = ldso_ba_sync(c))) return rc;
    if (x_out) std::memcpy(x_out, px, xb);
    if (point_step_out) scatter_points(c, ps, point_step_out);
    if (energy_out)
        for (int w = 0; w < c->n_win; w++) {
            energy_out[3 * w] = pe[2 * w];
            energy_out[3 * w + 1] = 0;
            energy_out[3 * w + 2] = pe[2 * w + 1];
        }
    return 0;
}

int ldso_ba_check_settings(const ldso_ba_opt_settings *s) {
    if (!s) return 0;
    static const struct {
        int bit;
        const char *name, *where;
    } kUnsupported[] = {
        {LDSO_BA_SOLVER_SVD, "SOLVER_SVD", "EnergyFunctional.cc:383-411"},
        {LDSO_BA_SOLVER_ORTHOGONALIZE_SYSTEM, "SOLVER_ORTHOGONALIZE_SYSTEM", "EnergyFunctional.cc:325"},
        {LDSO_BA_SOLVER_ORTHOGONALIZE_POINTMARG, "SOLVER_ORTHOGONALIZE_POINTMARG", "EnergyFunctional.cc:245"},
        {LDSO_BA_SOLVER_ORTHOGONALIZE_FULL, "SOLVER_ORTHOGONALIZE_FULL", "EnergyFunctional.cc:257"},
        {LDSO_BA_SOLVER_SVD_CUT7, "SOLVER_SVD_CUT7", "EnergyFunctional.cc:404"},
        {LDSO_BA_SOLVER_REMOVE_POSEPRIOR, "SOLVER_REMOVE_POSEPRIOR", "FrameHessian.h:147"},
        {LDSO_BA_SOLVER_USE_GN, "SOLVER_USE_GN", "EnergyFunctional.cc:282"},
        {LDSO_BA_SOLVER_ORTHOGONALIZE_X, "SOLVER_ORTHOGONALIZE_X", "EnergyFunctional.cc:428"},
        {LDSO_BA_SOLVER_MOMENTUM, "SOLVER_MOMENTUM", "FullSystem.cc:1840-1867"},
        {LDSO_BA_SOLVER_STEPMOMENTUM, "SOLVER_STEPMOMENTUM", "FullSystem.cc:913-920"},
    };
    for (const auto &u : kUnsupported)
        if (s->solver_mode & u.bit)
            return fail(-1, std::string("setting_solverMode: ") + u.name + " (" + u.where + ") is not implemented");
    if (s->solver_mode & ~(LDSO_BA_SOLVER_DEFAULT | 0xFFF))
        return fail(-1, "setting_solverMode: unknown bits");
    if (!(s->solver_mode & LDSO_BA_SOLVER_FIX_LAMBDA))
        return fail(-1, "setting_solverMode without SOLVER_FIX_LAMBDA (the LM lambda, EnergyFunctional.cc:283) is not "
                        "implemented");
    if (!s->force_accept_step)
        return fail(-1, "setting_forceAceptStep = false (the accept / reject branch with loadStateBackup, "
                        "FullSystem.cc:935-966) is not implemented");
    if (s->min_opt_iterations < 0) return fail(-1, "setting_minOptIterations < 0");
    if (s->vi_enable)
        return fail(-1, "setting_vi_enable = true: the inertial terms (combineInertialHessians and H_I / b_I in "
                        "solveSystemF, EnergyFunctional.cc:307-376; linearizeInertial, FullSystem.cc:879-926; the "
                        "inertial step and canbreak terms of doStepFromBackup, FullSystem.cc:1871-1931) are not "
                        "implemented: run visual-only (setting_vi_enable = false)");
    if (!std::isfinite(s->affine_opt_mode_a) || !std::isfinite(s->affine_opt_mode_b))
        return fail(-1, "setting_affineOptModeA / B must be finite");
    if (s->reserved_ != 0) return fail(-1, "ldso_ba_opt_settings.reserved_ must be 0");
    return 0;
}

void ldso_ba_default_settings(ldso_ba_opt_settings *s) {
    if (s) *s = ldso_ba_opt_settings LDSO_BA_OPT_SETTINGS_INIT;
}

int ldso_ba_set_settings(ldso_ba_ctx *c, const ldso_ba_opt_settings *s) {
    if (!c) return fail(-1, "bad arguments");
    int rc;
    if ((rc = ldso_ba_check_settings(s))) return rc;
    c->settings = s ? *s : ldso_ba_opt_settings LDSO_BA_OPT_SETTINGS_INIT;
    return 0;
}

int ldso_ba_get_settings(ldso_ba_ctx *c, ldso_ba_opt_settings *out) {
    if (!c || !out) return fail(-1, "bad arguments");
    *out = c->settings;
    return 0;
}

// The loop's first pass and solve use the priors the caller loaded (ldso_ba_window::frame_prior); every
// later step recomputes them on the device from the settings (k_step_resub, getPrior).  In the
// reference both come from the same setting_affineOptModeA / B, so a window whose loaded affine priors
// do not follow the settings the loop runs with is refused rather than run half with each.
static int check_affine_priors(const ldso_ba_ctx *c, const ldso_ba_frame_state *frames,
                               const ldso_ba_opt_settings &st) {
    for (int w = 0; w < c->n_win; w++) {
        const WinHost &H = c->wh[w];
        for (int f = 0; f < H.N; f++) {
            double p[8];
            frame_take_data_one(frames[c->wd[w].frame_base + f], st.affine_opt_mode_a, st.affine_opt_mode_b, p,
                                nullptr, nullptr);
            if (H.frame_prior[8 * f + 6] != p[6] || H.frame_prior[8 * f + 7] != p[7])
                return fail(-1, "window " + std::to_string(w) + " frame " + std::to_string(f) +
                                    ": the loaded affine priors (frame_prior[6..7]) do not follow the settings' "
                                    "setting_affineOptModeA / B; load the window with priors from "
                                    "ldso_ba_frame_take_data under the same settings");
        }
    }
    return 0;
}

int ldso_ba_optimize(ldso_ba_ctx *c, int32_t n_its, const ldso_ba_opt_settings *settings,
                     const ldso_ba_frame_state *frames, const double *calib_value, const double *calib_value_zero,
                     const double *ns, double *energy_out, ldso_ba_frame_state *frames_out, double *calib_out,
                     float *idepth_out, int32_t *iterations_out, int32_t *status_out) {
    if (!c || c->n_win == 0) return fail(-1, "no windows loaded");
    if (n_its < 0 || !frames || !calib_value || !calib_value_zero) return fail(-1, "bad arguments");
    if (c->marg) return fail(-1, "not on a marginalisation context");
    int rc;
    if (settings && (rc = ldso_ba_check_settings(settings))) return rc;
    if ((rc = check_affine_priors(c, frames, settings ? *settings : c->settings))) return rc;
    if (settings && (rc = ldso_ba_set_settings(c, settings))) return rc;  // checked, then installed
    const ldso_ba_opt_settings st = c->settings;
    // without SOLVER_ORTHOGONALIZE_X_LATER the solve never projects (EnergyFunctional.cc:428-432)
    if (!ortho_x_later(c)) ns = nullptr;
    HIP_TRY(hipSetDevice(c->device));
    const int nw = c->n_win;
    // ensure(): the buffers keep their addresses across calls, so cached graphs stay valid
    if ((rc = c->d_fstate.ensure(c->n_frames)) || (rc = c->d_calib_val.ensure((size_t)4 * nw)) ||
        (rc = c->d_calib_zero.ensure((size_t)4 * nw)) || (rc = c->d_cprior.ensure((size_t)4 * nw)) ||
        (rc = c->d_add_priors.ensure(nw)) || (rc = c->d_ehist.ensure((size_t)2 * nw * (n_its + 1))) ||
        (rc = c->d_stop.ensure(nw)) || (rc = c->d_status.ensure(nw)))
        return rc;
    std::vector<double> cp((size_t)4 * nw);
    std::vector<int> ap(nw);
    for (int w = 0; w < nw; w++) {
        for (int k = 0; k < 4; k++) cp[4 * w + k] = c->wh[w].c_prior[k];
        ap[w] = c->wh[w].add_priors ? 1 : 0;
    }
    {  // the call's inputs in one staged launch
        InBatch B;
        B.add(c->d_fstate.p, frames, (size_t)c->n_frames * sizeof(ldso_ba_frame_state));
        B.add(c->d_calib_val.p, calib_value, (size_t)4 * nw * sizeof(double));
        B.add(c->d_calib_zero.p, calib_value_zero, (size_t)4 * nw * sizeof(double));
        B.add(c->d_cprior.p, cp.data(), cp.size() * sizeof(double));
        B.add(c->d_add_priors.p, ap.data(), ap.size() * sizeof(int));
        if ((rc = B.flush(c))) return rc;
    }
    if (ns && (rc = upload_nullspaces(c, ns, 7)))  // evalPT is fixed during optimize(): valid for every iteration
        return rc;
    FrameStepParams F{};
    F.wins = c->d_wins.p;
    F.fstate = c->d_fstate.p;
    F.calib_val = c->d_calib_val.p;
    F.calib_zero = c->d_calib_zero.p;
    F.cprior = c->d_cprior.p;
    F.add_priors = c->d_add_priors.p;
    F.x = c->d_x.p;
    F.precalc = c->d_precalc.p;
    F.prior = c->d_prior.p;
    F.stop = c->d_stop.p;
    F.status = c->d_status.p;
    F.win_nid = c->win_nid();
    F.min_its = st.min_opt_iterations;
    F.th = st.th_opt_iterations;
    F.aff_a = st.affine_opt_mode_a;
    F.aff_b = st.affine_opt_mode_b;
    // one GN iteration: solveSystemF (a NaN x: the window is lost), resubstituteF_MT,
    // doStepFromBackup + setPrecalcValues (canbreak), linearizeAll + applyRes (+ the accumulation
    // the next solve uses); windows that left the loop skip every launch
    const Switches sw = read_switches();  // one reading for the launches and the graph's key
    auto gn_iteration = [&](int it) -> int {
        int r;
        if ((r = solve_device_launch(c, it, ns ? 7 : 0, it, sw))) return r;  // pass `it` precedes step `it`
        // the frame / calibration step + FrameFramePrecalc and the resubstitution with the point
        // step applied in place, in one launch (the solve wrote x and xAd)
        FrameStepParams Fi = F;
        Fi.it = it;
        ResubParams R = resub_params(c, 0, c->P_tot, 1e-5, true);
        R.stop = c->d_stop.p;
        R.it = it;
        if ((r = timed_launch(c, kSlotResubstitute, c->stream, [&] {
                 k_step_resub<<<nw + (c->P_tot + 255) / 256, 256, 0, c->stream>>>(Fi, R, nw);
             })))
            return r;
        return linearize_pass(c, 0, it + 1 < n_its ? 1 : 0, it + 1, sw);
    };
    // FullSystem::optimize (FullSystem.cc:853-976) with setting_forceAceptStep: resetOOB, then
    // linearizeAll + applyRes, then the GN iterations.  Every launch argument of the whole
    // sequence is fixed by (n_its, nullspaces or not), so without a communicator or kernel timing
    // the calls after the first replay ONE captured HIP graph of it (graph launches are
    // separated by ~9 us on the GPU; one per call instead of one per iteration), cached in the
    // context and re-captured after a device (re)allocation or when anything fixed at capture
    // changes: n_its, the settings, the solve kernel (exact or not), the stitch split.
    auto body = [&]() -> int {
        int r;
        // every window in the loop: stop = INT_MAX-ish (0x7f7f7f7f), status LDSO_BA_OPT_RAN_ALL
        HIP_TRY(hipMemsetAsync(c->d_stop.p, 0x7f, (size_t)nw * sizeof(int), c->stream));
        HIP_TRY(hipMemsetAsync(c->d_status.p, 0, (size_t)nw * sizeof(int), c->stream));
        // every pass of this call writes its energies into the history too: pass 0, then it + 1 after step it
        if ((r = ldso_ba_reset_oob(c, -1)) || (r = linearize_pass(c, 0, n_its > 0 ? 1 : 0, 0, sw))) return r;
        for (int it = 0; it < n_its; it++)
            if ((r = gn_iteration(it))) return r;
        return 0;
    };
    const bool use_graph = !c->comm && !c->timer.on && !sw.no_graph;
    if (use_graph && c->opt_warm) {
        std::vector<unsigned long long> key = capture_key(c, sw);  // the settings were installed above
        key.push_back((unsigned long long)(unsigned)n_its);
        rc = launch_cached_graph(c, c->opt_graph[ns ? 1 : 0], key, body);
    } else {
        rc = body();  // the first call runs directly (one-time setup stays out of any capture)
        c->opt_warm = rc == 0;
    }
    if (rc) return rc;
    // every result into one pinned buffer (energy history, frame states, calibration, the window
    // descriptors, the idepth column), one synchronisation
    const size_t hb = (size_t)2 * nw * (n_its + 1) * sizeof(double),
                 fb = (size_t)c->n_frames * sizeof(ldso_ba_frame_state), cb = (size_t)4 * nw * sizeof(double),
                 wb = (size_t)nw * sizeof(WinDev), ib = (size_t)c->P_tot * sizeof(float),
                 tb = (size_t)c->n_frames * sizeof(float), sb = (size_t)nw * sizeof(int);
    auto up16 = [](size_t v) { return (v + 15) & ~(size_t)15; };
    const size_t o_f = up16(hb), o_c = o_f + up16(fb), o_w = o_c + up16(cb), o_t = o_w + up16(wb), o_s = o_t + up16(tb),
                 o_u = o_s + up16(sb), o_i = o_u + up16(sb);
    if ((rc = pin_map_ensure(c, o_i + ib))) return rc;
    char *po = c->pin_map.p, *pd = c->pin_map.dev;
    {  // one launch writes every result into the mapped buffer (the idepth column only)
        PackOut K{};
        if (energy_out) pack_seg(K, c->d_ehist.p, pd, hb);
        if (frames_out) pack_seg(K, c->d_fstate.p, pd + o_f, fb);
        if (calib_out) pack_seg(K, c->d_calib_val.p, pd + o_c, cb);
        pack_seg(K, c->d_wins.p, pd + o_w, wb);  // the host mirror of WinDev (calibration, cDeltaF) follows the device
        pack_seg(K, c->d_frame_th.p, pd + o_t, tb);  // setNewFrameEnergyTH of the last pass (ldso_ba_get_frame_energy_th)
        pack_seg(K, c->d_stop.p, pd + o_s, sb);      // the loop exits
        pack_seg(K, c->d_status.p, pd + o_u, sb);
        if (idepth_out && c->P_tot) {
            K.pt_data = c->d_pt_data.p;
            K.idepth_dst = reinterpret_cast<float *>(pd + o_i);
            K.n_points = c->P_tot;
        }
        k_pack_out<<<std::min(64, (int)((o_i + ib) / 1024) + 1), 256, 0, c->stream>>>(K);
        HIP_TRY(hipGetLastError());
    }
    if ((rc = ldso_ba_sync(c))) return rc;
    {
        const int *stop = reinterpret_cast<const int *>(po + o_s), *status = reinterpret_cast<const int *>(po + o_u);
        for (int w = 0; w < nw; w++) {
            // lost at iteration k: stop = k and k + 1 solves ran; converged at k: stop = k + 1
            const int its = status[w] == LDSO_BA_OPT_LOST ? stop[w] + 1 : std::min(stop[w], n_its);
            if (iterations_out) iterations_out[w] = its;
            if (status_out) status_out[w] = status[w];
        }
    }
    if (energy_out) {
        const double *e = reinterpret_cast<const double *>(po);
        for (int s = 0; s <= n_its; s++)
            for (int w = 0; w < nw; w++) {
                double *o = energy_out + ((size_t)s * nw + w) * 3;
                o[0] = e[(size_t)2 * (s * nw + w)];
                o[1] = 0;
                o[2] = e[(size_t)2 * (s * nw + w) + 1];
            }
    }
    if (frames_out) std::memcpy(frames_out, po + o_f, fb);
    if (calib_out) std::memcpy(calib_out, po + o_c, cb);
    std::memcpy(c->wd.data(), po + o_w, wb);
    c->th_host.assign(reinterpret_cast<const float *>(po + o_t), reinterpret_cast<const float *>(po + o_t) + c->n_frames);
    c->th_host_valid = true;
    if (idepth_out) scatter_points(c, reinterpret_cast<const float *>(po + o_i), idepth_out);
    c->sys_host_valid = false;
    c->energy_valid = false;
    return 0;
}

int ldso_ba_get_loop_state(ldso_ba_ctx *c, int32_t win, double *x, float *precalc, double *prior) {
    if (!c) return fail(-1, "null ctx");
    if (c->n_win == 0) return fail(-1, "no windows loaded");
    if (win < 0 || win >= c->n_win) return fail(-1, "bad window index");
    if (!c->d_x.p || !c->d_precalc.p || !c->d_prior.p) return fail(-1, "this context holds no loop state");
    HIP_TRY(hipSetDevice(c->device));
    int rc = ldso_ba_sync(c);
    if (rc) return rc;
    const WinDev &D = c->wd[win];
    const size_t dim = (size_t)8 * D.N + 4, pairs = (size_t)D.N * D.N;
    if (x) HIP_TRY(hipMemcpy(x, c->d_x.p + D.vec_base, dim * sizeof(double), hipMemcpyDeviceToHost));
    if (precalc)
        HIP_TRY(hipMemcpy(precalc, c->d_precalc.p + (size_t)D.pair_base * LDSO_BA_PRECALC_STRIDE,
                          pairs * LDSO_BA_PRECALC_STRIDE * sizeof(float), hipMemcpyDeviceToHost));
    if (prior) HIP_TRY(hipMemcpy(prior, c->d_prior.p + (size_t)2 * D.vec_base, 2 * dim * sizeof(double), hipMemcpyDeviceToHost));
    return 0;
}

int ldso_ba_frame_step(int32_t n, const ldso_ba_frame_state *in, const double *x, ldso_ba_frame_state *out,
                       double *calib_value, const double *calib_value_zero, float *calib_scaled_out,
                       float *c_delta_out) {
    if (n < 1 || n > LDSO_BA_MAX_FRAMES || !in || !x || !out) return fail(-1, "bad arguments");
    for (int f = 0; f < n; f++) frame_step_one(in[f], x + 4 + 8 * f, out[f]);
    if (calib_value) {
        float sf[4], cd[4];
        const double zero[4] = {0, 0, 0, 0};
        calib_step(calib_value, x, calib_value_zero ? calib_value_zero : zero, sf, cd);
        for (int k = 0; k < 4; k++) {
            if (calib_scaled_out) calib_scaled_out[k] = sf[k];
            if (c_delta_out) c_delta_out[k] = cd[k];
        }
    }
    return 0;
}

int ldso_ba_step_canbreak(int32_t n, const double *x, float sum_nid, float num_id, float th, int32_t *out) {
    if (n < 1 || n > LDSO_BA_MAX_FRAMES || !x || !out) return fail(-1, "bad arguments");
    *out = step_canbreak(n, x, sum_nid, num_id, th) ? 1 : 0;
    return 0;
}

int ldso_ba_packed_system(ldso_ba_ctx *c, void **dev_ptr, int64_t *n_doubles, int64_t *stride) {
    if (!c || !dev_ptr) return fail(-1, "bad arguments");
    *dev_ptr = c->d_sys.p;
    if (n_doubles) *n_doubles = (int64_t)c->sys_n;
    if (stride) *stride = c->n_win ? (int64_t)sys_len(c->wd[0].D) : 0;
    return 0;
}

int ldso_ba_unpack_system(ldso_ba_ctx *c) {
    if (!c) return fail(-1, "null ctx");
    c->sys_host_valid = false;  // get_system re-reads the (externally reduced) device buffer
    return 0;
}

int ldso_ba_copy_packed(ldso_ba_ctx *c, void *buf, int64_t n, int32_t direction) {
    if (!c || !buf || n != (int64_t)c->sys_n) return fail(-1, "bad arguments (size must equal the packed system)");
    HIP_TRY(hipSetDevice(c->device));
    if (direction == 0)
        HIP_TRY(hipMemcpyAsync(buf, c->d_sys.p, c->sys_n * sizeof(double), hipMemcpyDeviceToDevice, c->stream));
    else
        HIP_TRY(hipMemcpyAsync(c->d_sys.p, buf, c->sys_n * sizeof(double), hipMemcpyDeviceToDevice, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    c->sys_host_valid = false;
    return 0;
}

int ldso_ba_newest_stride(ldso_ba_ctx *c, int64_t *stride) {
    if (!c || !stride) return fail(-1, "bad arguments");
    int64_t m = 1;  // as comm_exchange: a slot of one pad where no residual targets a newest frame
    for (const WinDev &D : c->wd) m = std::max<int64_t>(m, D.newest_end - D.newest_begin);
    *stride = m;
    return 0;
}

int ldso_ba_export_newest(ldso_ba_ctx *c, float *dev_buf, int64_t stride) {
    if (!c || !dev_buf || c->n_win == 0 || stride < 1) return fail(-1, "bad arguments");
    for (const WinDev &D : c->wd)
        if (D.newest_end - D.newest_begin > stride) return fail(-1, "stride smaller than a newest-frame segment");
    HIP_TRY(hipSetDevice(c->device));
    const dim3 grid((unsigned)std::min<int64_t>((stride + 255) / 256, 64), (unsigned)c->n_win);
    k_export_newest<<<grid, 256, 0, c->stream>>>(c->d_wins.p, c->d_rs_energy_wo.p, dev_buf, (long long)stride,
                                                 (long long)stride, nullptr, 0);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(c->stream));
    return 0;
}

int ldso_ba_frame_threshold_gathered(ldso_ba_ctx *c, const float *dev_buf, int32_t n_ranks, int64_t stride) {
    if (!c || !dev_buf || c->n_win == 0 || n_ranks < 1 || stride < 1) return fail(-1, "bad arguments");
    if ((int64_t)n_ranks * stride > INT32_MAX) return fail(-1, "too many candidates");
    HIP_TRY(hipSetDevice(c->device));
    c->th_host_valid = false;
    int rc = timed_launch(c, kSlotFrameTh, c->stream, [&] {
        k_frame_th<<<c->n_win, kStThreads, 0, c->stream>>>(c->d_wins.p, dev_buf, n_ranks, c->n_win, (long long)stride,
                                                           (long long)stride, c->d_frame_th.p, NidSrc{}, nullptr,
                                                           nullptr, 0);
    });
    if (rc) return rc;
    HIP_TRY(hipStreamSynchronize(c->stream));
    return 0;
}

int ldso_ba_set_tuning(ldso_ba_ctx *c, int32_t key, int32_t value) {
    if (!c) return fail(-1, "null ctx");
    if (key == LDSO_BA_TUNE_TILED_IMAGES) {
        if (c->n_win) return fail(-1, "image layout must be chosen before ldso_ba_load");
        if (value != 1 && value != 3) return fail(-1, "image layout must be 1 or 3");
        c->img_mode_pref = value;
        return 0;
    }
    if (key == LDSO_BA_TUNE_ITEM_ORDER) {
        if (c->n_win) return fail(-1, "item order must be chosen before ldso_ba_load");
        if (value < 0 || value > 2) return fail(-1, "item order must be 0, 1 or 2");
        c->item_order = value;
        return 0;
    }
    if (key == LDSO_BA_TUNE_SOLVE_EXACT) {
        if (value != 0 && value != 1) return fail(-1, "solve mode must be 0 (fast) or 1 (exact)");
        c->solve_exact = value;
        return 0;
    }
    if (key == LDSO_BA_TUNE_TIMING_MASK) {
        c->timing_mask = (unsigned)value;
        return 0;
    }
    if (key == LDSO_BA_TUNE_TOP_CHUNK) {
        if (value < 0 || value > 64 || value % 8) return fail(-1, "chunk must be 0 or a multiple of 8 up to 64");
        if (c->n_win) return fail(-1, "chunk size must be chosen before ldso_ba_load");
        c->top_chunk = value;
        return 0;
    }
    return fail(-1, "unknown tuning key");
}

int ldso_ba_set_kernel_timing(ldso_ba_ctx *c, int32_t enable) {
    if (!c) return fail(-1, "null ctx");
    int rc = ldso_ba_sync(c);
    if (rc) return rc;
    c->timer.on = enable != 0;
    c->timer.reset();
    if (c->timer.on) c->timer.reserve(256);  // the events the timed launches will take, created now
    return 0;
}

int ldso_ba_get_kernel_times(ldso_ba_ctx *c, double *ms, int64_t *counts, int32_t n) {
    if (!c) return fail(-1, "null ctx");
    int rc = ldso_ba_sync(c);
    if (rc) return rc;
    for (int i = 0; i < n && i < kNumKernels; i++) {
        if (ms) ms[i] = c->timer.ms[i];
        if (counts) counts[i] = c->timer.count[i];
    }
    return 0;
}

const char *ldso_ba_kernel_name(int32_t i) { return (i >= 0 && i < kNumKernels) ? kKernelNames[i] : ""; }
int32_t ldso_ba_num_kernels(void) { return kNumKernels; }

int ldso_ba_stats(ldso_ba_ctx *c, int64_t *device_bytes, int64_t *n_points, int64_t *n_residuals) {
    if (!c) return fail(-1, "null ctx");
    if (device_bytes)
        *device_bytes = (int64_t)(c->d_img.bytes() + c->store.d_store.bytes() + c->d_precalc.bytes() + c->d_pt_data.bytes() + c->d_rec_a.bytes() + c->d_rec_b.bytes() +
                                  c->d_top_slab.bytes() + c->d_sc_slab.bytes() + c->d_sys.bytes());
    if (n_points) *n_points = c->P_tot;
    if (n_residuals) *n_residuals = c->R_tot;
    return 0;
}

}  // extern "C"
