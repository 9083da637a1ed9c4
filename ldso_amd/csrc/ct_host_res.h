// ct_host_res.h -- calcRes / calcGSSSE and trackNewestCoarse's LM loop (k_ct_residual.h, k_ct_track.h, ct_eval.h, ct_lm.h).
// Owns c->res.  Reads the reference (ref.d_pc, its exposure and affine pair) and frame.d_dIp.
// A piece of the one translation unit ldso_ct.hip (k_ct_pyramid.h).
#pragma once
#include <algorithm>
#include <cmath>
#include <cstring>
#include <vector>

#include "ct_context.h"

#pragma clang fp contract(off)

namespace {

// ct_eval_setup for the context's reference and new frame: the pose of one hypothesis, and the terms every
// hypothesis under this cutoff shares
CtEvalTerms make_pose(const ldso_ct_ctx *c, int lvl, const double *T, double aff_a, double aff_b, float cutoffTH, CtPose &p) {
    CtEvalTerms e;
    ldso_ct::ct_eval_setup(T, c->Ki[lvl], c->ref.exposure, c->frame.exposure, c->ref.a, c->ref.b, (float)aff_a, (float)aff_b,
                           cutoffTH, p, e);
    return e;
}

// calcGSSSE's affine pair alone: it reads neither the pose nor the cutoff
CtEvalTerms gs_affine(const ldso_ct_ctx *c, int lvl, double aff_a, double aff_b) {
    const double T0[12] = {0};
    CtPose unused;
    return make_pose(c, lvl, T0, aff_a, aff_b, 0, unused);
}

int check_level(const ldso_ct_ctx *c, int lvl) {
    if (!c) return fail(-1, "null context");
    if (lvl < 0 || lvl >= c->levels) return fail(-1, "pyramid level out of range");
    if (!c->have_k) return fail(-1, "ldso_ct_make_k not called");
    if (!c->frame.have) return fail(-1, "ldso_ct_set_new_frame not called");
    if (!c->ref.have) return fail(-1, "ldso_ct_set_reference not called");
    return 0;
}

// launch calcRes for n_hyp poses already staged in h_poses by make_pose, which returned ev (partials to
// parts[0, n_hyp*nb*8))
// gs (n_hyp == 1): the pose by value and calcGSSSE in the same kernel (k_ct_calc_res<true>), its
// partials at parts + n_hyp * nb * kResParts
int launch_calc_res(ldso_ct_ctx *c, int lvl, int n_hyp, const CtEvalTerms &ev, bool write_warp, size_t extra_parts,
                    bool gs = false) {
    const int nb = level_grid(c, lvl).nb;
    int rc = ct_grow(c, c->res.parts, (size_t)n_hyp * nb * kResParts + extra_parts);
    if (rc) return rc;
    if (!gs)
        HIP_TRY(hipMemcpyAsync(c->res.d_poses.p, c->res.h_poses.p, (size_t)n_hyp * sizeof(CtPose), hipMemcpyHostToDevice,
                               c->stream));
    CtResParams P;
    P.lv = level_of(c, lvl);
    P.poses = c->res.d_poses.p;
    P.state = c->res.d_state.p;
    P.warp = c->res.d_warp.p;
    P.parts = c->res.parts.dev;
    P.lvl = lvl;
    P.write_warp = write_warp ? 1 : 0;
    P.n_blocks = nb;
    P.ev = ev;
    P.pose0 = c->res.h_poses.p[0];
    P.gs_parts = c->res.parts.dev + (size_t)n_hyp * nb * kResParts;
    const dim3 grid(nb, gs ? 1 : n_hyp);
    if (gs) return ct_launch(c, kCtSlotCalcRes, [&] { k_ct_calc_res<true><<<grid, kCtThreads, 0, c->stream>>>(P); });
    return ct_launch(c, kCtSlotCalcRes, [&] { k_ct_calc_res<false><<<grid, kCtThreads, 0, c->stream>>>(P); });
}

// the Vec6 of every hypothesis from the block partials already on the host
void finish_calc_res(ldso_ct_ctx *c, int lvl, int n_hyp, bool write_warp, double *rs_out) {
    const int nb = level_grid(c, lvl).nb;
    for (int hI = 0; hI < n_hyp; hI++) {
        double s[kResParts] = {0};
        const double *p = c->res.parts.p + (size_t)hI * nb * kResParts;
        for (int b = 0; b < nb; b++)
            for (int k = 0; k < kResParts; k++) s[k] += p[(size_t)b * kResParts + k];
        ldso_ct::ct_finish_res(s, rs_out + 6 * (size_t)hI);
        if (write_warp && hI == 0) c->res.last_warped = (int)s[6];
    }
}

int run_calc_res(ldso_ct_ctx *c, int lvl, int n_hyp, const CtEvalTerms &ev, bool write_warp, double *rs_out) {
    int rc = launch_calc_res(c, lvl, n_hyp, ev, write_warp, 0);
    if (rc) return rc;
    HIP_TRY(hipStreamSynchronize(c->stream));  // the partials are in parts.p already
    finish_calc_res(c, lvl, n_hyp, write_warp, rs_out);
    return 0;
}

// calcGSSSE launch over the warped buffers, partials at parts + off
int launch_calc_gs(ldso_ct_ctx *c, int lvl, double aff_a, double aff_b, size_t off) {
    const LevelGrid g = level_grid(c, lvl);
    const CtEvalTerms e = gs_affine(c, lvl, aff_a, aff_b);
    CtGsParams P;
    P.state = c->res.d_state.p;
    P.warp = c->res.d_warp.p;
    P.parts = c->res.parts.dev + off;
    P.n = g.n;
    P.fxl = c->fx[lvl];
    P.fyl = c->fy[lvl];
    P.a = e.gs_a;
    P.b0 = e.gs_b0;
    return ct_launch(c, kCtSlotCalcGs, [&] { k_ct_calc_gs<<<g.nb, kCtThreads, 0, c->stream>>>(P); });
}

// the scaled H, b from the GS block partials on the host and the last calcRes' warped count
void finish_calc_gs(ldso_ct_ctx *c, int lvl, const double *parts, double *H_out, double *b_out) {
    const int nb = level_grid(c, lvl).nb;
    double s[kGsParts] = {0};
    for (int b = 0; b < nb; b++)
        for (int k = 0; k < kGsParts; k++) s[k] += parts[(size_t)b * kGsParts + k];
    for (int r = 0; r < 8; r++) {
        for (int cc = 0; cc < 8; cc++) H_out[8 * r + cc] = ldso_ct::ct_finish_gs_entry(s, c->res.last_warped, r, cc);
        b_out[r] = ldso_ct::ct_finish_gs_entry(s, c->res.last_warped, r, 8);
    }
}

// ---- the LM loop (k_ct_track.h, ct_lm.h) ---------------------------------------------------------
// Setting.cc:82, 136-137, 65-66 (affineOptModeA / B), CoarseTracker.cc:73; the symmetric solve
constexpr ldso_ct_track_params kTrackDefaults = {20.f, 4.0, 0.5, 1e12f, 1e8f, {10, 20, 50, 50, 50}, LDSO_CT_TRACK_SOLVE_FULL};

int track_check_params(const ldso_ct_track_params &p) {
    if (!std::isfinite(p.coarse_cutoff_th) || !(p.coarse_cutoff_th > 0)) return fail(-1, "coarse_cutoff_th must be finite and > 0");
    if (!std::isfinite(p.lambda_increase) || !(p.lambda_increase > 0) || !std::isfinite(p.lambda_decrease) ||
        !(p.lambda_decrease > 0))
        return fail(-1, "lambda_increase and lambda_decrease must be finite and > 0");
    if (!std::isfinite(p.affine_opt_mode_a) || !std::isfinite(p.affine_opt_mode_b))
        return fail(-1, "affine_opt_mode_a / _b must be finite");
    for (int l = 0; l < 5; l++)
        if (p.max_iterations[l] < 1 || p.max_iterations[l] > ldso_ct::kTrackMaxIterations)
            return fail(-1, "max_iterations out of range [1, 1000]");
    if (p.solve != LDSO_CT_TRACK_SOLVE_FULL && p.solve != LDSO_CT_TRACK_SOLVE_REFERENCE) return fail(-1, "unknown solve mode");
    return 0;
}

}  // namespace

extern "C" {

int ldso_ct_calc_res(ldso_ct_ctx *c, int32_t lvl, const double ref_to_new[12], double aff_a, double aff_b,
                     float cutoff_th, double rs_out[6]) {
    int rc = check_level(c, lvl);
    if (rc) return rc;
    if (!ref_to_new || !rs_out) return fail(-1, "null argument");
    HIP_TRY(hipSetDevice(c->device));
    rc = run_calc_res(c, lvl, 1, make_pose(c, lvl, ref_to_new, aff_a, aff_b, cutoff_th, c->res.h_poses.p[0]), true, rs_out);
    if (rc) return rc;
    c->res.last_lvl = lvl;
    return 0;
}

int ldso_ct_calc_res_batch(ldso_ct_ctx *c, int32_t lvl, int32_t n_hyp, const double *ref_to_new, const double *aff_ab,
                           float cutoff_th, double *rs_out) {
    int rc = check_level(c, lvl);
    if (rc) return rc;
    if (!ref_to_new || !aff_ab || !rs_out) return fail(-1, "null argument");
    if (n_hyp < 1 || n_hyp > kMaxHyp) return fail(-1, "n_hyp out of range [1, 256]");
    HIP_TRY(hipSetDevice(c->device));
    CtEvalTerms ev;
    for (int k = 0; k < n_hyp; k++)
        ev = make_pose(c, lvl, ref_to_new + 12 * k, aff_ab[2 * k], aff_ab[2 * k + 1], cutoff_th, c->res.h_poses.p[k]);
    return run_calc_res(c, lvl, n_hyp, ev, false, rs_out);
}

int ldso_ct_calc_gs(ldso_ct_ctx *c, int32_t lvl, const double ref_to_new[12], double aff_a, double aff_b,
                    double *H_out, double *b_out) {
    int rc = check_level(c, lvl);
    if (rc) return rc;
    if (!H_out || !b_out) return fail(-1, "null argument");
    if (c->res.last_lvl != lvl) return fail(-1, "calcGSSSE needs a calcRes at this level first");
    (void)ref_to_new;  // calcGSSSE reads only the warped buffers and the affine parameters
    HIP_TRY(hipSetDevice(c->device));
    rc = ct_grow(c, c->res.parts, (size_t)level_grid(c, lvl).nb * kGsParts);
    if (rc) return rc;
    rc = launch_calc_gs(c, lvl, aff_a, aff_b, 0);
    if (rc) return rc;
    HIP_TRY(hipStreamSynchronize(c->stream));  // the partials are in parts.p already
    finish_calc_gs(c, lvl, c->res.parts.p, H_out, b_out);
    return 0;
}

int ldso_ct_calc_res_gs(ldso_ct_ctx *c, int32_t lvl, const double ref_to_new[12], double aff_a, double aff_b,
                        float cutoff_th, double rs_out[6], double *H_out, double *b_out) {
    int rc = check_level(c, lvl);
    if (rc) return rc;
    if (!ref_to_new || !rs_out || !H_out || !b_out) return fail(-1, "null argument");
    HIP_TRY(hipSetDevice(c->device));
    const int nb = level_grid(c, lvl).nb;
    const size_t res_parts = (size_t)nb * kResParts;
    const CtEvalTerms ev = make_pose(c, lvl, ref_to_new, aff_a, aff_b, cutoff_th, c->res.h_poses.p[0]);
    // calcRes and calcGSSSE in one launch (the GS terms of each warped point from the same values
    // the warped buffers receive; the block partials are those of k_ct_calc_gs)
    rc = launch_calc_res(c, lvl, 1, ev, true, (size_t)nb * kGsParts, true);
    if (rc) return rc;
    HIP_TRY(hipStreamSynchronize(c->stream));  // the partials are in parts.p already
    finish_calc_res(c, lvl, 1, true, rs_out);
    c->res.last_lvl = lvl;
    finish_calc_gs(c, lvl, c->res.parts.p + res_parts, H_out, b_out);
    return 0;
}

void ldso_ct_track_default_params(ldso_ct_track_params *p) {
    if (p) *p = kTrackDefaults;
}

int ldso_ct_track(ldso_ct_ctx *c, int32_t n, const double *ref_to_new_in, const double *aff_in, int32_t coarsest_lvl,
                  const double *min_res_for_abort, const ldso_ct_track_params *params, ldso_ct_track_result *out,
                  ldso_ct_track_step *trace, int32_t trace_capacity, int32_t *trace_n) {
    if (!c) return fail(-1, "null context");
    if (coarsest_lvl < 0 || coarsest_lvl >= std::min(c->levels, 5))
        return fail(-1, "coarsest_lvl out of range [0, min(levels, 5))");
    int rc = check_level(c, coarsest_lvl);
    if (rc) return rc;
    if (n < 1) return fail(-1, "n must be >= 1");
    if (!ref_to_new_in || !aff_in || !min_res_for_abort || !out) return fail(-1, "null argument");
    const ldso_ct_track_params p = params ? *params : kTrackDefaults;
    if ((rc = track_check_params(p))) return rc;
    if (trace && trace_capacity < 1) return fail(-1, "trace_capacity must be >= 1 with a trace");
    HIP_TRY(hipSetDevice(c->device));
    if ((rc = ct_grow(c, c->res.track_in, n)) || (rc = ct_grow(c, c->res.track_out, n)) || (rc = ct_grow(c, c->res.track_n, 1)) ||
        (trace && (rc = ct_grow(c, c->res.track_trace, trace_capacity))))
        return rc;
    for (int k = 0; k < n; k++) {
        CtTrackStart &S = c->res.track_in.p[k];
        std::memcpy(S.ref_to_new, ref_to_new_in + 12 * (size_t)k, sizeof S.ref_to_new);
        std::memcpy(S.aff, aff_in + 2 * (size_t)k, sizeof S.aff);
        std::memcpy(S.min_res, min_res_for_abort + 5 * (size_t)k, sizeof S.min_res);
    }
    CtTrackParams P{};
    for (int l = 0; l <= coarsest_lvl; l++) P.lv[l] = level_of(c, l);
    P.p = p;
    P.starts = c->res.track_in.dev;
    P.out = c->res.track_out.dev;
    P.trace = trace ? c->res.track_trace.dev : nullptr;
    P.trace_n = c->res.track_n.dev;
    P.trace_capacity = trace ? trace_capacity : 0;
    P.coarsest = coarsest_lvl;
    P.ref_exposure = c->ref.exposure;
    P.new_exposure = c->frame.exposure;
    P.ref_a = c->ref.a;
    P.ref_b = c->ref.b;
    c->res.last_lvl = -1;  // the warped buffers describe no evaluation of this call
    k_ct_track<kTrackWaves><<<n, kTrackWaves * kWave, 0, c->stream>>>(P);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(c->stream));  // results and trace are in host memory already
    std::memcpy(out, c->res.track_out.p, (size_t)n * sizeof *out);
    const int n_eval = c->res.track_n.p[0];
    if (trace) std::memcpy(trace, c->res.track_trace.p, (size_t)std::min(n_eval, trace_capacity) * sizeof *trace);
    if (trace_n) *trace_n = n_eval;
    return 0;
}

int ldso_ct_lm_step(const double H[64], const double b[8], double lambda, const double pose[12], const double aff[2],
                    const ldso_ct_track_params *params, double inc_out[8], double pose_out[12], double aff_out[2]) {
    if (!H || !b || !pose || !aff || !inc_out || !pose_out || !aff_out) return fail(-1, "null argument");
    const ldso_ct_track_params p = params ? *params : kTrackDefaults;
    if (int rc = track_check_params(p)) return rc;
    ldso_ct::LdltWork W;
    ldso_ct::Pose cand;
    const float a[2] = {(float)aff[0], (float)aff[1]};
    float an[2];
    ldso_ct::lm_step(H, b, (float)lambda, ldso_ct::pose_from_matrix(pose), a, p, W, inc_out, cand, an);
    ldso_ct::pose_matrix(cand, pose_out);
    aff_out[0] = an[0];
    aff_out[1] = an[1];
    return 0;
}

int ldso_ct_get_warped(ldso_ct_ctx *c, int32_t *n_out, float *out, int32_t capacity) {
    if (!c || !n_out) return fail(-1, "null argument");
    if (c->res.last_lvl < 0) return fail(-1, "no calcRes yet");
    const int nw = (c->res.last_warped + 3) / 4 * 4;
    *n_out = nw;
    if (!out) return 0;
    if (capacity < nw) return fail(-1, "capacity below buf_warped_n");
    const int n = level_grid(c, c->res.last_lvl).n;
    std::vector<uint8_t> st(std::max(1, n));
    std::vector<float4> wp(2 * (size_t)std::max(1, n));
    HIP_TRY(hipSetDevice(c->device));
    if (n) {
        HIP_TRY(hipMemcpyAsync(st.data(), c->res.d_state.p, (size_t)n, hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(hipMemcpyAsync(wp.data(), c->res.d_warp.p, (size_t)n * 2 * sizeof(float4), hipMemcpyDeviceToHost, c->stream));
    }
    HIP_TRY(hipStreamSynchronize(c->stream));
    int k = 0;
    for (int i = 0; i < n; i++) {
        if (st[i] != 2) continue;
        const float4 a = wp[2 * (size_t)i], b = wp[2 * (size_t)i + 1];
        const float v[8] = {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w};
        std::memcpy(out + 8 * (size_t)k, v, sizeof v);
        k++;
    }
    for (; k < nw; k++) std::memset(out + 8 * (size_t)k, 0, 8 * sizeof(float));
    return 0;
}

}  // extern "C"
