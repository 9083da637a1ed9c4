// ldso_ct.hip -- the C ABI of LDSO's coarse tracker (include/ldso_ct.h) on the MI355X (gfx950) and its
// host side.  The kernels, each described where it stands:
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
//   ct_context.h        the timing slots and struct ldso_ct_ctx
//   hip_owning.h         shared with ldso_ba.hip: fail / HIP_TRY, the owning buffers and events, KernelTimer
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
#include "k_ct_pyramid.h"
#include "k_ct_residual.h"
#include "k_ct_immature.h"
#include "k_ct_coarse_depth.h"
#include "k_ct_track.h"
#include "k_ct_actsel.h"
#include "k_ct_undistort.h"
#include "ct_context.h"

#pragma clang fp contract(off)

// ---------------------------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------------------------
// the BA frame store's view of the new frame (ldso_ba_frame_put_tracker)
int ldso_ba::ct_frame_view(const ldso_ct_ctx *c, ldso_ba::CtFrameView *out) {
    if (!c || !out) return fail(-1, "null argument");
    out->intensity = c->d_inten.p;
    out->texels = c->d_dIp.p;
    out->width = c->pyr.w;
    out->height = c->pyr.h;
    out->device = c->device;
    out->stream = (void *)c->stream;
    out->have_frame = c->have_frame;
    return 0;
}

// the BA context's view of the last activation selection (ldso_ba_activate_points_tracker)
int ldso_ba::ct_selection_view(const ldso_ct_ctx *c, ldso_ba::CtSelectionView *out) {
    if (!c || !out) return fail(-1, "null argument");
    out->records = c->d_as_selected.p;
    out->n = c->as_sel_n;
    out->n_hosts = c->as_sel_hosts;
    out->device = c->device;
    out->stream = (void *)c->stream;
    return 0;
}

// the loop closer's view of the last corner detection (ldso_lc_keyframe_put_tracker)
int ldso_ba::ct_corners_view(const ldso_ct_ctx *c, ldso_ba::CtCornersView *out) {
    if (!c || !out) return fail(-1, "null argument");
    static_assert(sizeof(CorSlot) == 4 * sizeof(int) && offsetof(CorSlot, x) == 0 && offsetof(CorSlot, y) == sizeof(int),
                  "CtCornersView reads x, y at the start of a CorSlot");
    out->pixel = reinterpret_cast<const int *>(c->d_cor_feat.p);
    out->pixel_stride = sizeof(CorSlot) / sizeof(int);
    out->records = c->d_cor_out.p;
    out->n = c->cor_n;
    out->width = c->pyr.w;
    out->height = c->pyr.h;
    out->device = c->device;
    out->stream = (void *)c->stream;
    return 0;
}

namespace {

// one launch on the context's stream into kernel-timing slot `slot`
template <typename F>
int ct_launch(ldso_ct_ctx *c, int slot, F &&launch) {
    return c->timer.launch(slot, c->timer.on, c->stream, [&](hipEvent_t, hipEvent_t) { launch(); });
}

// Grow-only: a buffer that fits keeps its address; one in use is replaced behind a synchronisation of
// the context's stream, which may still read or write it.
template <typename Buf>
int ct_grow(ldso_ct_ctx *c, Buf &buf, size_t n) {
    if (buf.p && buf.n >= n) return 0;
    if (buf.p) HIP_TRY(hipStreamSynchronize(c->stream));
    return buf.ensure(n);
}

// a level's point count and its blocks of kCtThreads (never none: every launch writes its partials)
struct LevelGrid {
    int n, nb;
};
LevelGrid level_grid(const ldso_ct_ctx *c, int lvl) {
    const int n = c->pc_off[lvl + 1] - c->pc_off[lvl];
    return {n, std::max(1, (n + kCtThreads - 1) / kCtThreads)};
}

// a level as the kernels read it
CtLevel level_of(const ldso_ct_ctx *c, int lvl) {
    CtLevel L;
    L.pc = c->d_pc.p + c->pc_off[lvl];
    L.img = c->d_dIp.p + c->pyr.off[lvl];
    L.n = level_grid(c, lvl).n;
    L.wl = c->pyr.wl[lvl];
    L.hl = c->pyr.hl[lvl];
    L.fxl = c->fx[lvl];
    L.fyl = c->fy[lvl];
    L.cxl = c->cx[lvl];
    L.cyl = c->cy[lvl];
    for (int k = 0; k < 9; k++) L.Ki[k] = c->Ki[lvl][k];
    return L;
}

// ct_eval_setup for the context's reference and new frame: the pose of one hypothesis, and the terms every
// hypothesis under this cutoff shares
CtEvalTerms make_pose(const ldso_ct_ctx *c, int lvl, const double *T, double aff_a, double aff_b, float cutoffTH, CtPose &p) {
    CtEvalTerms e;
    ldso_ct::ct_eval_setup(T, c->Ki[lvl], c->ref_exposure, c->new_exposure, c->ref_a, c->ref_b, (float)aff_a, (float)aff_b,
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
    if (!c->have_frame) return fail(-1, "ldso_ct_set_new_frame not called");
    if (!c->have_ref) return fail(-1, "ldso_ct_set_reference not called");
    return 0;
}

// launch calcRes for n_hyp poses already staged in h_poses by make_pose, which returned ev (partials to
// parts[0, n_hyp*nb*8))
// gs (n_hyp == 1): the pose by value and calcGSSSE in the same kernel (k_ct_calc_res<true>), its
// partials at parts + n_hyp * nb * kResParts
int launch_calc_res(ldso_ct_ctx *c, int lvl, int n_hyp, const CtEvalTerms &ev, bool write_warp, size_t extra_parts,
                    bool gs = false) {
    const int nb = level_grid(c, lvl).nb;
    int rc = ct_grow(c, c->parts, (size_t)n_hyp * nb * kResParts + extra_parts);
    if (rc) return rc;
    if (!gs)
        HIP_TRY(hipMemcpyAsync(c->d_poses.p, c->h_poses.p, (size_t)n_hyp * sizeof(CtPose), hipMemcpyHostToDevice,
                               c->stream));
    CtResParams P;
    P.lv = level_of(c, lvl);
    P.poses = c->d_poses.p;
    P.state = c->d_state.p;
    P.warp = c->d_warp.p;
    P.parts = c->parts.dev;
    P.lvl = lvl;
    P.write_warp = write_warp ? 1 : 0;
    P.n_blocks = nb;
    P.ev = ev;
    P.pose0 = c->h_poses.p[0];
    P.gs_parts = c->parts.dev + (size_t)n_hyp * nb * kResParts;
    const dim3 grid(nb, gs ? 1 : n_hyp);
    if (gs) return ct_launch(c, kCtSlotCalcRes, [&] { k_ct_calc_res<true><<<grid, kCtThreads, 0, c->stream>>>(P); });
    return ct_launch(c, kCtSlotCalcRes, [&] { k_ct_calc_res<false><<<grid, kCtThreads, 0, c->stream>>>(P); });
}

// the Vec6 of every hypothesis from the block partials already on the host
void finish_calc_res(ldso_ct_ctx *c, int lvl, int n_hyp, bool write_warp, double *rs_out) {
    const int nb = level_grid(c, lvl).nb;
    for (int hI = 0; hI < n_hyp; hI++) {
        double s[kResParts] = {0};
        const double *p = c->parts.p + (size_t)hI * nb * kResParts;
        for (int b = 0; b < nb; b++)
            for (int k = 0; k < kResParts; k++) s[k] += p[(size_t)b * kResParts + k];
        ldso_ct::ct_finish_res(s, rs_out + 6 * (size_t)hI);
        if (write_warp && hI == 0) c->last_warped = (int)s[6];
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
    P.state = c->d_state.p;
    P.warp = c->d_warp.p;
    P.parts = c->parts.dev + off;
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
        for (int cc = 0; cc < 8; cc++) H_out[8 * r + cc] = ldso_ct::ct_finish_gs_entry(s, c->last_warped, r, cc);
        b_out[r] = ldso_ct::ct_finish_gs_entry(s, c->last_warped, r, 8);
    }
}

// ---- the reference cloud built on the device (k_ct_coarse_depth.h) ----------------------------
// the work buffers, whose sizes follow the context's image size: allocated by the first call only.
// The cloud holds at most the interior pixels of every level, the warped buffers those of level 0.
int cd_ensure(ldso_ct_ctx *c) {
    const PyrParams &P = c->pyr;
    const int npx = P.off[P.levels];
    if (!c->cd_interior0 && !c->cd_lv.blk_off[P.levels]) {
        int nb = 0;
        for (int l = 0; l <= LDSO_CT_MAX_LEVELS; l++) {
            c->cd_lv.blk_off[l] = nb;
            if (l >= P.levels) continue;
            nb += (P.wl[l] * P.hl[l] + kCtThreads - 1) / kCtThreads;
            const int in = std::max(0, P.wl[l] - 4) * std::max(0, P.hl[l] - 4);
            c->cd_interior += in;
            if (l == 0) c->cd_interior0 = in;
        }
    }
    const int nb = c->cd_lv.blk_off[P.levels];
    int rc;
    if ((rc = c->d_cd_maps.ensure(2 * (size_t)npx)) || (rc = c->d_cd_cand.ensure(npx)) ||
        (rc = c->d_cd_blk.ensure((size_t)nb + LDSO_CT_MAX_LEVELS + 1)) || (rc = c->cd_counts.ensure(LDSO_CT_MAX_LEVELS)) ||
        (rc = c->cd_ev_a.ensure(hipEventDisableTiming)) || (rc = c->cd_ev_b.ensure(hipEventDisableTiming)) ||
        (rc = ct_grow(c, c->d_pc, std::max(1, c->cd_interior))))
        return rc;
    const size_t n0 = c->cd_interior0;
    if (c->d_state.n < n0 || c->d_warp.n < 2 * n0) {
        HIP_TRY(hipStreamSynchronize(c->stream));
        if ((rc = c->d_state.ensure(n0)) || (rc = c->d_warp.ensure(2 * n0))) return rc;
    }
    return 0;
}

// the checks both make calls share, before any HIP call; *src = the context whose frame is read
int cd_check(ldso_ct_ctx *c, const ldso_ct_ctx *frame_src, const ldso_ct_ctx **src) {
    if (!c) return fail(-1, "null context");
    const ldso_ct_ctx *s = frame_src ? frame_src : c;
    if (s->device != c->device) return fail(-1, "frame_src is on a different device");
    if (s->pyr.w != c->pyr.w || s->pyr.h != c->pyr.h) return fail(-1, "frame_src has a different image size");
    if (!s->have_frame) return fail(-1, "ldso_ct_set_new_frame has not been called on the frame source");
    *src = s;
    return 0;
}

// from n contributions in d_cd_contrib to the resident cloud: maps, pyramid, dilation, compaction,
// one synchronisation for the per-level counts
int cd_build(ldso_ct_ctx *c, const ldso_ct_ctx *src, int n, double ref_ab_exposure, double ref_aff_a, double ref_aff_b,
             int32_t *pc_n_out) {
    const PyrParams &P = c->pyr;
    const int npx = P.off[P.levels], nb = c->cd_lv.blk_off[P.levels];
    const size_t px0 = (size_t)P.w * P.h;
    float *idm = c->d_cd_maps.p, *wm = idm + npx;
    int *blk = c->d_cd_blk.p, *lvl_off = blk + nb;
    // level 0 of both maps is summed into; the coarser levels are written whole
    HIP_TRY(hipMemsetAsync(idm, 0, px0 * sizeof(float), c->stream));
    HIP_TRY(hipMemsetAsync(wm, 0, px0 * sizeof(float), c->stream));
    if (n > 0)
        k_ct_cd_scatter<<<(n + kCtThreads - 1) / kCtThreads, kCtThreads, 0, c->stream>>>(c->d_cd_contrib.p, n, idm, wm,
                                                                                        P.w, P.h);
    if (P.levels > 1) {
        const size_t lds = 2 * ((size_t)P.tile * P.tile + (size_t)(P.tile / 2) * (P.tile / 2)) * sizeof(float);
        k_ct_cd_pyr<<<dim3(P.w / P.tile, P.h / P.tile), kCtThreads, lds, c->stream>>>(idm, wm, P);
    }
    // the colours come from the frame source's pyramid: wait for what its stream holds now, and
    // let whatever it is given later (its next frame) wait for the read
    if (src != c) {
        HIP_TRY(hipEventRecord(c->cd_ev_a.e, src->stream));
        HIP_TRY(hipStreamWaitEvent(c->stream, c->cd_ev_a.e, 0));
    }
    k_ct_cd_flag<<<nb, kCtThreads, 0, c->stream>>>(idm, wm, src->d_dIp.p, c->d_cd_cand.p, blk, P, c->cd_lv);
    if (src != c) {
        HIP_TRY(hipEventRecord(c->cd_ev_b.e, c->stream));
        HIP_TRY(hipStreamWaitEvent(src->stream, c->cd_ev_b.e, 0));
    }
    k_ct_cd_scan<<<1, kCtThreads, 0, c->stream>>>(blk, lvl_off, c->cd_counts.dev, P.levels, c->cd_lv);
    k_ct_cd_write<<<nb, kCtThreads, 0, c->stream>>>(c->d_cd_cand.p, blk, lvl_off, c->d_pc.p, P, c->cd_lv);
    HIP_TRY(hipGetLastError());
    c->have_ref = false;  // until the counts are in
    HIP_TRY(hipStreamSynchronize(c->stream));
    int off = 0;
    for (int l = 0; l < c->levels; l++) {
        c->pc_off[l] = off;
        off += c->cd_counts.p[l];
        if (pc_n_out) pc_n_out[l] = c->cd_counts.p[l];
    }
    c->pc_off[c->levels] = off;
    c->ref_exposure = (float)ref_ab_exposure;
    c->ref_a = (float)ref_aff_a;
    c->ref_b = (float)ref_aff_b;
    c->have_ref = true;
    c->last_lvl = -1;
    return 0;
}

// ---- pixel selection (k_ct_select.h) ------------------------------------------------------------
constexpr ldso_ct_select_params kSelDefaults = {1500.f, 1, 1.f, 0.5f, 7.f, 0.75f, 1};  // Setting.cc:29, 83-87

int sel_blocks(int n) { return std::max(1, (n + kCtThreads - 1) / kCtThreads); }

int sel_check(const ldso_ct_ctx *c, const ldso_ct_select_params &p) {
    if (!c) return fail(-1, "null context");
    if (c->levels < 3) return fail(-1, "pixel selection reads pyramid levels 0-2: the context has fewer than 3 levels");
    if (!c->sel_potential) return fail(-1, "ldso_ct_select_init not called");
    if (!c->have_frame) return fail(-1, "ldso_ct_set_new_frame not called");
    if (!std::isfinite(p.density) || !(p.density > 0)) return fail(-1, "density must be finite and > 0");
    if (p.recursions < 0) return fail(-1, "recursions must be >= 0");
    return 0;
}

// the work buffers: their sizes follow the image size, so only the first selection allocates
int sel_ensure(ldso_ct_ctx *c) {
    const int w = c->pyr.w, h = c->pyr.h, w32 = w / 32, h32 = h / 32, n = w * h;
    // every index (x >> 5) + (y >> 5) * w32 of a pixel, and the grid makeHists fills
    const size_t n_ths = std::max((size_t)((w - 1) >> 5) + (size_t)((h - 1) >> 5) * w32 + 1, (size_t)w32 * h32);
    if (c->d_sel_ths.p && c->d_sel_map.p) return 0;
    int rc;
    if ((rc = c->d_sel_map.ensure(n)) || (rc = c->h_sel_map.ensure(n)) ||
        (rc = c->d_sel_ths_raw.ensure(std::max(1, w32 * h32))) || (rc = c->d_sel_mask.ensure(n)) ||
        (rc = c->d_sel_n2.ensure(n)) || (rc = c->d_sel_nu.ensure(n)) ||
        (rc = c->d_sel_blk.ensure(2 * (size_t)sel_blocks(n))) || (rc = c->d_sel_cnt.ensure(kSelCnts)) ||
        (rc = c->h_sel_cnt.ensure(kSelCnts)) || (rc = c->d_sel_ths.ensure(n_ths)))
        return rc;
    HIP_TRY(hipMemsetAsync(c->d_sel_ths.p, 0, n_ths * sizeof(float), c->stream));  // the entries makeHists never writes
    return 0;
}

// one select(fh, map_out, pot, thFactor): the map on the device, n = (n2, n3, n4) behind one wait
int sel_pass(ldso_ct_ctx *c, const ldso_ct_select_params &p, int pot, int n[3]) {
    const PyrParams &P = c->pyr;
    SelParams S;
    S.dI0 = c->d_dIp.p;
    S.dI1 = c->d_dIp.p + P.off[1];
    S.dI2 = c->d_dIp.p + P.off[2];
    S.ths = c->d_sel_ths.p;
    S.pattern = c->d_sel_pattern.p;
    S.w = P.w;
    S.h = P.h;
    S.w1 = P.wl[1];
    S.w2 = P.wl[2];
    S.w32 = P.w / 32;
    S.pot = std::min(pot, std::max(P.w, P.h));  // a cell as large as the image is the image
    S.ncx = (P.w + S.pot - 1) / S.pot;
    S.ncy = (P.h + S.pot - 1) / S.pot;
    S.dw1 = p.grad_downweight_per_level;
    S.dw2 = S.dw1 * S.dw1;
    S.th_factor = p.th_factor;
    S.dir_dist = p.select_direction_distribution != 0;
    const int nc = S.ncx * S.ncy, nb = sel_blocks(nc);
    const dim3 grid4((S.ncx + 3) / 4, (S.ncy + 3) / 4);
    const int threads = 16 * S.pot * S.pot <= kCtThreads ? kWave : kCtThreads;
    int *cnt = c->d_sel_cnt.p, *blk = c->d_sel_blk.p;
    HIP_TRY(hipMemsetAsync(c->d_sel_map.p, 0, (size_t)P.w * P.h, c->stream));
    HIP_TRY(hipMemsetAsync(cnt, 0, kSelCnts * sizeof(int), c->stream));
    k_ct_sel_block<false><<<grid4, threads, 0, c->stream>>>(S, c->d_sel_mask.p, nullptr, nullptr, nullptr);
    for (int round = 0; round < 2; round++) {
        k_ct_sel_cell_count<<<nb, kCtThreads, 0, c->stream>>>(c->d_sel_mask.p, nc, nb, blk);
        k_ct_sel_scan<<<1, kCtThreads, 0, c->stream>>>(blk, nb, 2, cnt + kSelCntN2);  // [N2], [NonUniform]
        k_ct_sel_cell_apply<<<nb, kCtThreads, 0, c->stream>>>(c->d_sel_mask.p, nc, nb, blk, c->d_sel_n2.p, c->d_sel_nu.p);
        if (round == 0)
            k_ct_sel_fixup<<<1, kWave, 0, c->stream>>>(c->d_sel_nu.p, cnt, c->d_sel_n2.p, c->d_sel_mask.p,
                                                       c->d_sel_pattern.p, P.w * P.h);
    }
    k_ct_sel_block<true><<<grid4, threads, 0, c->stream>>>(S, nullptr, c->d_sel_n2.p, c->d_sel_map.p, cnt);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(c->h_sel_cnt.p, cnt, kSelCnts * sizeof(int), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    n[0] = c->h_sel_cnt.p[kSelCntN2];
    n[1] = c->h_sel_cnt.p[kSelCntN3];
    n[2] = c->h_sel_cnt.p[kSelCntN4];
    return 0;
}

// PixelSelector::makeMaps (PixelSelector2.cc:111-169), the recursion as a loop.  Leaves the map on the
// device, the sub-selection (if any) enqueued: *sub tells the caller to take stats[0] from
// h_sel_cnt[kSelCntKept] after its synchronisation.  The context's potential is set.
int sel_make_maps(ldso_ct_ctx *c, const ldso_ct_select_params &p, int32_t stats[LDSO_CT_SELECT_STATS], bool *sub) {
    const PyrParams &P = c->pyr;
    int rc = sel_ensure(c);
    if (rc) return rc;
    const int w32 = P.w / 32, h32 = P.h / 32;
    if (w32 > 0 && h32 > 0) {  // makeHists
        k_ct_sel_hist<<<dim3(w32, h32), kCtThreads, 0, c->stream>>>(c->d_dIp.p, P.w, P.h, w32, p.min_grad_hist_cut,
                                                                   p.min_grad_hist_add, c->d_sel_ths_raw.p);
        k_ct_sel_smooth<<<sel_blocks(w32 * h32), kCtThreads, 0, c->stream>>>(c->d_sel_ths_raw.p, w32, h32, c->d_sel_ths.p);
    }
    int recursionsLeft = p.recursions, currentPotential = c->sel_potential, idealPotential, n[3], passes = 0;
    const float numWant = p.density;
    float numHave, quotia;
    for (;;) {
        if ((rc = sel_pass(c, p, currentPotential, n))) return rc;
        passes++;
        numHave = n[0] + n[1] + n[2];
        quotia = numWant / numHave;
        const float K = numHave * (currentPotential + 1) * (currentPotential + 1);
        const float ideal = sqrtf(K / numWant) - 1;  // round down
        idealPotential = ideal < (float)kSelMaxPotential ? (int)ideal : kSelMaxPotential;
        if (idealPotential < 1) idealPotential = 1;
        if (recursionsLeft > 0 && quotia > 1.25 && currentPotential > 1) {
            if (idealPotential >= currentPotential) idealPotential = currentPotential - 1;
        } else if (recursionsLeft > 0 && quotia < 0.25) {
            if (idealPotential <= currentPotential) idealPotential = currentPotential + 1;
            idealPotential = std::min(idealPotential, kSelMaxPotential);
        } else {
            break;
        }
        currentPotential = idealPotential;
        recursionsLeft--;
    }
    *sub = quotia < 0.95;
    if (*sub) {
        const int npx = P.w * P.h, nb = sel_blocks(npx);
        const unsigned char charTH = 255 * quotia;
        k_ct_sel_px_count<<<nb, kCtThreads, 0, c->stream>>>(c->d_sel_map.p, npx, c->d_sel_blk.p);
        k_ct_sel_scan<<<1, kCtThreads, 0, c->stream>>>(c->d_sel_blk.p, nb, 1, c->d_sel_cnt.p + kSelCntScratch);
        k_ct_sel_sub<<<nb, kCtThreads, 0, c->stream>>>(c->d_sel_map.p, npx, c->d_sel_blk.p, c->d_sel_pattern.p, charTH,
                                                       c->d_sel_cnt.p);
        HIP_TRY(hipGetLastError());
    }
    stats[0] = (int)numHave;
    stats[1] = n[0];
    stats[2] = n[1];
    stats[3] = n[2];
    stats[4] = currentPotential;
    stats[5] = idealPotential;
    stats[6] = passes;
    c->sel_potential = idealPotential;
    return 0;
}

// ---- corner detection (k_ct_corners.h) -----------------------------------------------------------
// DetectCorners' grid (FeatureDetector.cc:37-42), in the reference's types: the quotient w * h / n is an
// integer division, nfeatInGrid a float product.  The loop `picked++; if (picked > nfeatInGrid) break`
// makes floor(nfeatInGrid) + 1 picks where a cell has that many candidates.
int cor_grid(const ldso_ct_ctx *c, int n_features, CorGrid &G) {
    const int w = c->pyr.w, h = c->pyr.h;
    const int gridsize = int(sqrtf(w * h / n_features) + 0.5);
    if (gridsize < 1 || gridsize > kCorMaxGrid)
        return fail(-1, "gridsize " + std::to_string(gridsize) + " outside [1, 30]: n_features does not suit the image size");
    const int gridX = w / gridsize + 1, gridY = h / gridsize + 1;
    const float nfeatInGrid = float(n_features) / (w * h) * (gridsize * gridsize);
    G.w = w;
    G.h = h;
    G.g = gridsize;
    G.skip = (kCorHalfPatch * 2 / gridsize) + 1;
    G.ncx = std::max(0, gridX - 2 * G.skip);
    G.ncy = std::max(0, gridY - 2 * G.skip);
    G.k = (int)std::floor(nfeatInGrid) + 1;
    G.kk = std::min(G.k, gridsize * gridsize);
    return 0;
}

// ---- activation candidates (k_ct_actsel.h) --------------------------------------------------------
constexpr ldso_ct_actsel_params kActselDefaults = LDSO_CT_ACTSEL_PARAMS_INIT;

AsGrid as_grid(const ldso_ct_ctx *c) {
    AsGrid G;
    G.w1 = c->pyr.w >> 1;  // wG[1], hG[1], whatever the context's pyramid holds
    G.h1 = c->pyr.h >> 1;
    G.bw = (G.w1 + (1 << kAsBinShift) - 1) >> kAsBinShift;
    G.bh = (G.h1 + (1 << kAsBinShift) - 1) >> kAsBinShift;
    return G;
}

// the checks both distance-map calls share, and the level-1 host tables onto the device
int as_begin_map(ldso_ct_ctx *c, int n_hosts, const float *krki1, const float *kt1) {
    if (n_hosts < 1 || n_hosts > kAsMaxHosts) return fail(-1, "n_hosts out of range [1, 16]");
    if (!krki1 || !kt1) return fail(-1, "null host tables");
    const AsGrid G = as_grid(c);
    if (G.w1 >= kAsMaxSide || G.h1 >= kAsMaxSide)
        return fail(-1, "level 1 of the frame is " + std::to_string(G.w1) + " x " + std::to_string(G.h1) +
                            ": the activation selection packs a pixel into 2 x 15 bits (sides below 32768)");
    HIP_TRY(hipSetDevice(c->device));
    const size_t npx = (size_t)G.w1 * G.h1, n_tab = (size_t)kAsMaxHosts * 12;
    int rc;
    if ((rc = c->d_as_map.ensure(npx)) || (rc = c->h_as_map.ensure(npx)) || (rc = c->d_as_hosts.ensure(n_tab)) ||
        (rc = c->h_as_hosts.ensure(n_tab)))
        return rc;
    HIP_TRY(hipStreamSynchronize(c->stream));  // the staging buffer may still feed a previous copy
    c->as_have_map = false;
    for (int i = 0; i < n_hosts; i++) {
        std::memcpy(c->h_as_hosts.p + 12 * (size_t)i, krki1 + 9 * (size_t)i, 9 * sizeof(float));
        std::memcpy(c->h_as_hosts.p + 12 * (size_t)i + 9, kt1 + 3 * (size_t)i, 3 * sizeof(float));
    }
    HIP_TRY(hipMemcpyAsync(c->d_as_hosts.p, c->h_as_hosts.p, (size_t)n_hosts * 12 * sizeof(float), hipMemcpyHostToDevice,
                           c->stream));
    HIP_TRY(hipMemsetD32Async((hipDeviceptr_t)c->d_as_map.p, kAsFar, npx, c->stream));
    return 0;
}

// growDistBFS over the seeded map, the map to the caller if asked
int as_finish_map(ldso_ct_ctx *c, int n_hosts, float *map_out) {
    const AsGrid G = as_grid(c);
    const size_t npx = (size_t)G.w1 * G.h1;
    k_ct_as_grow<<<dim3((G.w1 + kAsTile - 1) / kAsTile, (G.h1 + kAsTile - 1) / kAsTile), kAsGrowThreads, 0, c->stream>>>(
        c->d_as_map.p, G);
    HIP_TRY(hipGetLastError());
    if (map_out) {
        HIP_TRY(hipMemcpyAsync(c->h_as_map.p, c->d_as_map.p, npx * sizeof(int), hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(hipStreamSynchronize(c->stream));
        for (size_t i = 0; i < npx; i++) map_out[i] = (float)c->h_as_map.p[i];
    }
    c->as_n_hosts = n_hosts;
    c->as_have_map = true;
    return 0;
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

// ---- the new frame (k_ct_pyramid.h, k_ct_undistort.h) --------------------------------------------
// makeImages behind a level-0 image in d_color: the response table's upload and the two pyramid launches
// on the context's stream, no synchronisation.  Both ways of setting the new frame end here.
int frame_pyramid(ldso_ct_ctx *c, const float *b_response) {
    const PyrParams &P = c->pyr;
    if (b_response)
        HIP_TRY(hipMemcpyAsync(c->d_B.p, b_response, 256 * sizeof(float), hipMemcpyHostToDevice, c->stream));
    const float *B = b_response ? c->d_B.p : nullptr;
    const dim3 grid(P.w / P.tile, P.h / P.tile);
    const size_t lds = ((size_t)P.tile * P.tile + (size_t)(P.tile / 2) * (P.tile / 2) + 1) * sizeof(float);
    int rc = ct_launch(c, kCtSlotPyrDown,
                       [&] { k_ct_pyr_down<<<grid, kCtThreads, lds, c->stream>>>(c->d_color.p, c->d_inten.p, P); });
    if (rc) return rc;
    const int npx = P.off[P.levels];
    return ct_launch(c, kCtSlotPyrGrad, [&] {
        k_ct_pyr_grad<<<(npx + kCtThreads - 1) / kCtThreads, kCtThreads, 0, c->stream>>>(c->d_inten.p, c->d_dIp.p, B, P);
    });
}

// What processFrame does with this frame (Undistort.cc:198-228): the photometric value of a source pixel and
// ImageAndExposure::exposure_time.  Refuses what the frame cannot be read with.
int und_frame_mode(const ldso_ct_ctx *c, int bits, float exposure_time, int &mode, float &exposure) {
    if (!c->und_init) return fail(-1, "ldso_ct_undistort_init not called");
    if (bits != 8 && bits != 16) return fail(-1, "bits must be 8 or 16");
    const bool valid = c->und_g_depth > 0;
    if (!valid || exposure_time <= 0 || c->und_mode == 0)
        mode = kUndFactor;
    else
        mode = c->und_mode == 2 ? kUndLutVignette : kUndLut;
    if (mode != kUndFactor && bits == 16 && c->und_g_depth != 65536)
        return fail(-1, "a 16-bit frame indexes 65536 entries of G: g_depth is " + std::to_string(c->und_g_depth));
    exposure = c->und_use_exposure ? exposure_time : 1.0f;
    return 0;
}

// k_ct_undistort from the raw frame at dev_raw into d_color, on the context's stream
int launch_undistort(ldso_ct_ctx *c, const void *dev_raw, int bits, int mode, float factor) {
    const int n = c->pyr.w * c->pyr.h, nb = (n + kCtThreads - 1) / kCtThreads;
    const UndParams U{c->d_und_remap.p, c->d_und_g.p, c->d_und_vinv.p, c->und_w_org, n, mode, factor};
    float *out = c->d_color.p;
    if (bits == 8) {
        const uint8_t *raw = static_cast<const uint8_t *>(dev_raw);
        if (c->und_pass)
            k_ct_undistort<uint8_t, true><<<nb, kCtThreads, 0, c->stream>>>(raw, out, U);
        else
            k_ct_undistort<uint8_t, false><<<nb, kCtThreads, 0, c->stream>>>(raw, out, U);
    } else {
        const uint16_t *raw = static_cast<const uint16_t *>(dev_raw);
        if (c->und_pass)
            k_ct_undistort<uint16_t, true><<<nb, kCtThreads, 0, c->stream>>>(raw, out, U);
        else
            k_ct_undistort<uint16_t, false><<<nb, kCtThreads, 0, c->stream>>>(raw, out, U);
    }
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return fail(-2, std::string("launch k_ct_undistort: ") + hipGetErrorString(e));
    return 0;
}

}  // namespace

extern "C" {

void ldso_ct_select_default_params(ldso_ct_select_params *p) {
    if (p) *p = kSelDefaults;
}

int ldso_ct_select_init(ldso_ct_ctx *c, const uint8_t *random_pattern, int32_t potential) {
    if (!c || !random_pattern) return fail(-1, "null argument");
    if (c->levels < 3) return fail(-1, "pixel selection reads pyramid levels 0-2: the context has fewer than 3 levels");
    if (potential < 1 || potential > kSelMaxPotential) return fail(-1, "potential out of range [1, 32767]");
    if (std::max(c->pyr.w, c->pyr.h) >= kSelMaxSide) return fail(-1, "image side too large for the selector");
    HIP_TRY(hipSetDevice(c->device));
    const size_t n = (size_t)c->pyr.w * c->pyr.h;
    if (int rc = ct_grow(c, c->d_sel_pattern, n)) return rc;
    HIP_TRY(hipMemcpyAsync(c->d_sel_pattern.p, random_pattern, n, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));  // the caller's pattern may be reused on return
    c->sel_potential = potential;
    return 0;
}

int ldso_ct_select_potential(ldso_ct_ctx *c, int32_t *out) {
    if (!c || !out) return fail(-1, "null argument");
    if (!c->sel_potential) return fail(-1, "ldso_ct_select_init not called");
    *out = c->sel_potential;
    return 0;
}

int ldso_ct_select_pixels(ldso_ct_ctx *c, const ldso_ct_select_params *params, float *map_out, int32_t *stats_out) {
    const ldso_ct_select_params p = params ? *params : kSelDefaults;
    int rc = sel_check(c, p);
    if (rc) return rc;
    HIP_TRY(hipSetDevice(c->device));
    int32_t stats[LDSO_CT_SELECT_STATS];
    bool sub = false;
    if ((rc = sel_make_maps(c, p, stats, &sub))) return rc;
    const size_t n = (size_t)c->pyr.w * c->pyr.h;
    if (map_out) HIP_TRY(hipMemcpyAsync(c->h_sel_map.p, c->d_sel_map.p, n, hipMemcpyDeviceToHost, c->stream));
    if (sub)
        HIP_TRY(hipMemcpyAsync(c->h_sel_cnt.p, c->d_sel_cnt.p, kSelCnts * sizeof(int), hipMemcpyDeviceToHost, c->stream));
    if (map_out || sub) HIP_TRY(hipStreamSynchronize(c->stream));
    if (sub) stats[0] = c->h_sel_cnt.p[kSelCntKept];
    if (map_out)
        for (size_t i = 0; i < n; i++) map_out[i] = c->h_sel_map.p[i];
    if (stats_out) std::memcpy(stats_out, stats, sizeof stats);
    return 0;
}

int ldso_ct_make_new_traces(ldso_ct_ctx *c, const ldso_ct_select_params *params, int32_t host, int32_t capacity,
                            ldso_ct_immature *out, int32_t *n_out, int32_t *stats_out) {
    const ldso_ct_select_params p = params ? *params : kSelDefaults;
    int rc = sel_check(c, p);
    if (rc) return rc;
    if (!n_out || capacity < 0 || (capacity > 0 && !out)) return fail(-1, "bad output arguments");
    if (host < 0) return fail(-1, "negative host index");
    HIP_TRY(hipSetDevice(c->device));
    int32_t stats[LDSO_CT_SELECT_STATS];
    bool sub = false;
    const int potential_before = c->sel_potential;
    if ((rc = sel_make_maps(c, p, stats, &sub))) return rc;
    // the walk: survivors counted per block, the counts scanned, the records written in order
    const int w = c->pyr.w, h = c->pyr.h, npx = w * h, nb = sel_blocks(npx);
    const int cap = std::min(capacity, stats[1] + stats[2] + stats[3]);  // no more than select picked
    if ((rc = ct_grow(c, c->d_mk, std::max(1, cap)))) return rc;
    int *cnt = c->d_sel_cnt.p;
    k_ct_sel_emit<false><<<nb, kCtThreads, 0, c->stream>>>(c->d_dIp.p, w, h, c->d_sel_map.p, host, c->d_sel_blk.p, nullptr, 0);
    k_ct_sel_scan<<<1, kCtThreads, 0, c->stream>>>(c->d_sel_blk.p, nb, 1, cnt + kSelCntEmit);
    k_ct_sel_emit<true><<<nb, kCtThreads, 0, c->stream>>>(c->d_dIp.p, w, h, c->d_sel_map.p, host, c->d_sel_blk.p,
                                                         c->d_mk.p, cap);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(c->h_sel_cnt.p, cnt, kSelCnts * sizeof(int), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    if (sub) stats[0] = c->h_sel_cnt.p[kSelCntKept];
    const int n = c->h_sel_cnt.p[kSelCntEmit];
    *n_out = n;
    if (stats_out) std::memcpy(stats_out, stats, sizeof stats);
    if (n > capacity) {
        c->sel_potential = potential_before;
        return fail(-1, "capacity below the number of new immature points (see *n_out)");
    }
    if (n > 0) {
        HIP_TRY(hipMemcpyAsync(out, c->d_mk.p, (size_t)n * sizeof(IpRec), hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(hipStreamSynchronize(c->stream));
    }
    return 0;
}

int ldso_ct_corners_init(ldso_ct_ctx *c, const int32_t *bit_pattern) {
    if (!c || !bit_pattern) return fail(-1, "null argument");
    for (int i = 0; i < 1024; i++)
        if (bit_pattern[i] < -kCorPatternRange || bit_pattern[i] > kCorPatternRange)
            return fail(-1, "bit_pattern entry " + std::to_string(i) + " outside [-13, 13]");
    HIP_TRY(hipSetDevice(c->device));
    if (int rc = ct_grow(c, c->d_cor_pattern, 256)) return rc;
    HIP_TRY(hipMemcpyAsync(c->d_cor_pattern.p, bit_pattern, 1024 * sizeof(int32_t), hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));  // the caller's table may be reused on return
    // FeatureDetector::FeatureDetector (FeatureDetector.cc:10-28); cvFloor / cvCeil / cvRound as floor / ceil / rint
    constexpr int H = kCorHalfPatch;
    int *umax = c->cor_umax.u;
    int v, v0;
    const int vmax = (int)std::floor(H * std::sqrt(2.f) / 2 + 1), vmin = (int)std::ceil(H * std::sqrt(2.f) / 2);
    const double hp2 = H * H;
    for (v = 0; v <= vmax; ++v) umax[v] = (int)std::rint(std::sqrt(hp2 - v * v));
    for (v = H, v0 = 0; v >= vmin; --v) {
        while (umax[v0] == umax[v0 + 1]) ++v0;
        umax[v] = v0;
        ++v0;
    }
    c->cor_init = true;
    return 0;
}

int ldso_ct_detect_corners(ldso_ct_ctx *c, int32_t n_features, int32_t host, int32_t capacity,
                           ldso_ct_immature *recs_out, ldso_ct_feature *feat_out, int32_t *n_out,
                           int32_t *stats_out) {
    if (!c) return fail(-1, "null context");
    if (!c->cor_init) return fail(-1, "ldso_ct_corners_init not called");
    if (!c->have_frame) return fail(-1, "ldso_ct_set_new_frame not called");
    if (n_features <= 0) return fail(-1, "n_features must be > 0");
    if (!n_out || capacity < 0 || (capacity > 0 && (!recs_out || !feat_out))) return fail(-1, "bad output arguments");
    if (host < 0) return fail(-1, "negative host index");
    CorGrid G;
    int rc = cor_grid(c, n_features, G);
    if (rc) return rc;
    HIP_TRY(hipSetDevice(c->device));
    const int ncells = G.ncx * G.ncy;
    int32_t stats[LDSO_CT_CORNER_STATS] = {G.g, G.k, 0, 0, 0, 0};
    *n_out = 0;
    c->cor_n = -1;
    if (ncells > 0) {
        // every feature slot the grid has (each cell full of candidates), whatever the image holds
        const int n_slots = ncells * G.kk, cap = std::min(capacity, n_slots);
        if ((rc = ct_grow(c, c->d_cor_cell, 2 * (size_t)ncells)) || (rc = ct_grow(c, c->d_cor_slot, n_slots)) ||
            (rc = ct_grow(c, c->d_cor_feat, n_slots)) || (rc = ct_grow(c, c->d_cor_corner, n_slots)) ||
            (rc = ct_grow(c, c->d_cor_out, std::max(1, cap))) || (rc = ct_grow(c, c->d_mk, std::max(1, cap))) ||
            (rc = c->d_cor_cnt.ensure(kCorCnts)) || (rc = c->cor_counts.ensure(kCorCnts)))
            return rc;
        int *cnt = c->d_cor_cnt.p, *cell_cnt = c->d_cor_cell.p, *cell_off = cell_cnt + ncells;
        const int gg = G.g * G.g, nb_slots = sel_blocks(n_slots);
        HIP_TRY(hipMemsetAsync(cnt, 0, kCorCnts * sizeof(int), c->stream));
        k_ct_cor_cell<<<ncells, gg <= kWave ? kWave : kCtThreads, (size_t)gg * (sizeof(unsigned long long) + sizeof(float)),
                        c->stream>>>(c->d_dIp.p, G, cell_cnt, cell_off, c->d_cor_slot.p, cnt);
        k_ct_sel_scan<<<1, kCtThreads, 0, c->stream>>>(cell_off, ncells, 1, cnt + kCorCntFeatures);
        k_ct_cor_emit<<<nb_slots, kCtThreads, 0, c->stream>>>(c->d_dIp.p, G, n_slots, cell_cnt, cell_off, c->d_cor_slot.p,
                                                              cnt, host, c->d_cor_feat.p, c->d_mk.p, cap);
        k_ct_cor_suppress<<<nb_slots, kCtThreads, 0, c->stream>>>(G, cell_cnt, cell_off, c->d_cor_feat.p,
                                                                  c->d_cor_corner.p, cnt);
        k_ct_cor_orb<<<(n_slots + kCorWavesPerBlock - 1) / kCorWavesPerBlock, kCtThreads, 0, c->stream>>>(
            c->d_dIp.p, G.w, G.h, c->d_cor_feat.p, c->d_cor_corner.p, c->d_cor_pattern.p, c->cor_umax, cnt, cap,
            c->d_cor_out.p, c->cor_counts.dev);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipStreamSynchronize(c->stream));  // the counters are in mapped host memory
        const int *hc = c->cor_counts.p;
        stats[2] = hc[kCorCntCandidates];
        stats[3] = hc[kCorCntFeatures];
        stats[4] = hc[kCorCntCorners];
        stats[5] = hc[kCorCntMaxScore];
        *n_out = hc[kCorCntFeatures];
    }
    const int n = *n_out;
    c->cor_n = n <= capacity ? n : -1;  // the device holds a record per feature only when they all fitted
    if (stats_out) std::memcpy(stats_out, stats, sizeof stats);
    if (n > capacity) return fail(-1, "capacity below the number of features (see *n_out)");
    if (n > 0) {
        HIP_TRY(hipMemcpyAsync(recs_out, c->d_mk.p, (size_t)n * sizeof(IpRec), hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(hipMemcpyAsync(feat_out, c->d_cor_out.p, (size_t)n * sizeof(ldso_ct_feature), hipMemcpyDeviceToHost,
                               c->stream));
        HIP_TRY(hipStreamSynchronize(c->stream));
    }
    return 0;
}

int ldso_ct_make_reference(ldso_ct_ctx *c, const ldso_ct_ctx *frame_src, int32_t n, const float *center,
                           const float *hdi, double ref_ab_exposure, double ref_aff_a, double ref_aff_b,
                           int32_t *pc_n_out) {
    const ldso_ct_ctx *src = nullptr;
    int rc = cd_check(c, frame_src, &src);
    if (rc) return rc;
    if (n < 0 || (n > 0 && (!center || !hdi))) return fail(-1, "bad contribution arguments");
    HIP_TRY(hipSetDevice(c->device));
    if ((rc = cd_ensure(c))) return rc;
    if (n > 0) {
        if ((rc = ct_grow(c, c->d_cd_contrib, n)) || (rc = ct_grow(c, c->h_cd_contrib, n))) return rc;
        // (the staging buffer is free: every call that copies out of it ends with a synchronisation)
        for (int i = 0; i < n; i++)
            c->h_cd_contrib.p[i] = make_float4(center[3 * (size_t)i], center[3 * (size_t)i + 1], center[3 * (size_t)i + 2], hdi[i]);
        HIP_TRY(hipMemcpyAsync(c->d_cd_contrib.p, c->h_cd_contrib.p, (size_t)n * sizeof(float4), hipMemcpyHostToDevice,
                               c->stream));
    }
    return cd_build(c, src, n, ref_ab_exposure, ref_aff_a, ref_aff_b, pc_n_out);
}

int ldso_ct_make_reference_ba(ldso_ct_ctx *c, const ldso_ct_ctx *frame_src, const ldso_ba_ctx *ba, int32_t win,
                              int32_t ref_frame, double ref_ab_exposure, double ref_aff_a, double ref_aff_b,
                              int32_t *pc_n_out) {
    const ldso_ct_ctx *src = nullptr;
    int rc = cd_check(c, frame_src, &src);
    if (rc) return rc;
    if (!ba) return fail(-1, "null bundle-adjustment context");
    ldso_ba::BaRefView V;
    if ((rc = ldso_ba::ba_ref_view(ba, win, &V))) return rc;
    if (V.device != c->device) return fail(-1, "the bundle-adjustment context is on a different device");
    if (V.marg) return fail(-1, "a marginalisation context holds no tracking reference");
    if (V.sharded) return fail(-1, "the context holds a shard of its points: the reference needs the whole window");
    if (!V.have_pass) return fail(-1, "no linearisation pass has run since the context's last load");
    if (ref_frame < -1 || ref_frame >= V.N) return fail(-1, "ref_frame out of range");
    if (V.width != c->pyr.w || V.height != c->pyr.h)
        return fail(-1, "the tracker's frame size differs from the window's images");
    if (ref_frame < 0) ref_frame = V.N - 1;
    HIP_TRY(hipSetDevice(c->device));
    if ((rc = cd_ensure(c))) return rc;
    const int n = V.R > 0 ? V.P : 0;
    if (n > 0) {
        if ((rc = ct_grow(c, c->d_cd_contrib, n))) return rc;
        // read the pass's arrays behind what the BA stream holds now; its later work waits for the read
        hipStream_t bs = static_cast<hipStream_t>(V.stream);
        HIP_TRY(hipEventRecord(c->cd_ev_a.e, bs));
        HIP_TRY(hipStreamWaitEvent(c->stream, c->cd_ev_a.e, 0));
        HIP_TRY(hipMemsetAsync(c->d_cd_contrib.p, 0xFF, (size_t)n * sizeof(float4), c->stream));  // NaN: no contribution
        CdGatherParams G{V.center, V.plane_stride, V.state, V.tgt, V.slot, V.pt_out, c->d_cd_contrib.p,
                         V.R,      V.P,            V.rec_base, ref_frame};
        k_ct_cd_gather<<<(V.R + kCtThreads - 1) / kCtThreads, kCtThreads, 0, c->stream>>>(G);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipEventRecord(c->cd_ev_b.e, c->stream));
        HIP_TRY(hipStreamWaitEvent(bs, c->cd_ev_b.e, 0));
    }
    return cd_build(c, src, n, ref_ab_exposure, ref_aff_a, ref_aff_b, pc_n_out);
}

int ldso_ct_get_reference(ldso_ct_ctx *c, int32_t lvl, int32_t *n_out, float *out, int32_t capacity) {
    if (!c || !n_out) return fail(-1, "null argument");
    if (lvl < 0 || lvl >= c->levels) return fail(-1, "pyramid level out of range");
    if (!c->have_ref) return fail(-1, "no reference: call ldso_ct_set_reference or ldso_ct_make_reference first");
    const int n = level_grid(c, lvl).n;
    *n_out = n;
    if (!out || n == 0) return 0;
    if (capacity < n) return fail(-1, "capacity below the level's point count");
    HIP_TRY(hipSetDevice(c->device));
    HIP_TRY(hipMemcpyAsync(out, c->d_pc.p + c->pc_off[lvl], (size_t)n * sizeof(float4), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return 0;
}

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
    if ((rc = c->d_color.alloc((size_t)width * height)) || (rc = c->d_inten.alloc(off)) || (rc = c->d_dIp.alloc(off)) ||
        (rc = c->d_B.alloc(256)) || (rc = c->d_poses.alloc(kMaxHyp)) || (rc = c->h_poses.ensure(kMaxHyp)) ||
        (rc = c->d_counts.alloc(8)) || (rc = c->h_counts.ensure(8))) {
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

int ldso_ct_set_new_frame(ldso_ct_ctx *c, const float *color, double ab_exposure, const float *b_response) {
    if (!c || !color) return fail(-1, "null argument");
    HIP_TRY(hipSetDevice(c->device));
    const PyrParams &P = c->pyr;
    HIP_TRY(hipMemcpyAsync(c->d_color.p, color, (size_t)P.w * P.h * sizeof(float), hipMemcpyHostToDevice, c->stream));
    const int rc = frame_pyramid(c, b_response);
    if (rc) return rc;
    HIP_TRY(hipStreamSynchronize(c->stream));  // the caller's buffers may be reused on return
    c->new_exposure = (float)ab_exposure;
    c->have_frame = true;
    return 0;
}

int ldso_ct_undistort_init(ldso_ct_ctx *c, const ldso_ct_undistort_desc *d, int32_t *n_outside_out) {
    if (!c || !d) return fail(-1, "null argument");
    if (d->w_org < 2 || d->h_org < 2) return fail(-1, "the raw image must be at least 2 x 2");
    if ((d->remap_x == nullptr) != (d->remap_y == nullptr)) return fail(-1, "remap_x and remap_y come together: one of them is NULL");
    if (d->photometric_mode < 0 || d->photometric_mode > 2) return fail(-1, "photometric_mode out of range [0, 2]");
    if (d->g && d->g_depth < 256) return fail(-1, "g_depth must be at least 256");
    if (d->g && !d->vignette_inv) return fail(-1, "g needs vignette_inv: the photometric calibration is valid with both only");
    const PyrParams &P = c->pyr;
    const bool pass = !d->remap_x;
    if (pass && (d->w_org != P.w || d->h_org != P.h))
        return fail(-1, "passthrough needs a raw image of the context's size " + std::to_string(P.w) + "x" + std::to_string(P.h));
    if ((int64_t)d->w_org * d->h_org > INT32_MAX / 2) return fail(-1, "the raw image is too large");
    HIP_TRY(hipSetDevice(c->device));
    HIP_TRY(hipStreamSynchronize(c->stream));  // no launch still reads the tables this call replaces
    c->und_init = false;
    const size_t n = (size_t)P.w * P.h, n_org = (size_t)d->w_org * d->h_org;
    int rc, outside = 0;
    if (!pass) {
        // the footprint rule (include/ldso_ct.h): what the kernel would read outside the source becomes -1
        std::vector<float2> m(n);
        for (size_t i = 0; i < n; i++) {
            const float xx = d->remap_x[i], yy = d->remap_y[i];
            m[i] = make_float2(xx, yy);
            if (xx < 0) continue;  // the reference's own mark: its pixel is 0
            bool inside = std::isfinite(xx) && std::isfinite(yy) && xx < (float)d->w_org && yy > -1.0f && yy < (float)d->h_org;
            if (inside) {
                const int xxi = (int)xx, yyi = (int)yy;
                inside = xxi + 1 <= d->w_org - 1 && yyi >= 0 && yyi + 1 <= d->h_org - 1;
            }
            if (!inside) {
                m[i] = make_float2(-1.0f, -1.0f);
                outside++;
            }
        }
        if ((rc = c->d_und_remap.ensure(n))) return rc;
        HIP_TRY(hipMemcpy(c->d_und_remap.p, m.data(), n * sizeof(float2), hipMemcpyHostToDevice));
    }
    if (d->g) {
        if ((rc = c->d_und_g.ensure((size_t)d->g_depth)) || (rc = c->d_und_vinv.ensure(n_org))) return rc;
        HIP_TRY(hipMemcpy(c->d_und_g.p, d->g, (size_t)d->g_depth * sizeof(float), hipMemcpyHostToDevice));
        HIP_TRY(hipMemcpy(c->d_und_vinv.p, d->vignette_inv, n_org * sizeof(float), hipMemcpyHostToDevice));
    }
    if ((rc = c->h_und_raw.ensure(n_org * 2)) || (rc = c->d_und_raw.ensure(n_org * 2))) return rc;
    if ((rc = c->und_ev_prod.ensure(hipEventDisableTiming)) || (rc = c->und_ev_cons.ensure(hipEventDisableTiming))) return rc;
    c->und_pass = pass;
    c->und_w_org = d->w_org;
    c->und_h_org = d->h_org;
    c->und_g_depth = d->g ? d->g_depth : 0;
    c->und_mode = d->photometric_mode;
    c->und_use_exposure = d->use_exposure != 0;
    c->und_init = true;
    if (n_outside_out) *n_outside_out = outside;
    return 0;
}

int ldso_ct_set_new_frame_raw(ldso_ct_ctx *c, const void *raw, int32_t bits, float exposure_time, float factor,
                              const float *b_response, float *exposure_out) {
    if (!c || !raw) return fail(-1, "null argument");
    int mode;
    float exposure;
    int rc = und_frame_mode(c, bits, exposure_time, mode, exposure);
    if (rc) return rc;
    HIP_TRY(hipSetDevice(c->device));
    // every use of the pinned frame ends behind a synchronisation, so it is free here
    const size_t bytes = (size_t)c->und_w_org * c->und_h_org * (bits / 8);
    std::memcpy(c->h_und_raw.p, raw, bytes);
    HIP_TRY(hipMemcpyAsync(c->d_und_raw.p, c->h_und_raw.p, bytes, hipMemcpyHostToDevice, c->stream));
    if ((rc = launch_undistort(c, c->d_und_raw.p, bits, mode, factor)) || (rc = frame_pyramid(c, b_response))) return rc;
    HIP_TRY(hipStreamSynchronize(c->stream));
    c->new_exposure = exposure;
    c->have_frame = true;
    if (exposure_out) *exposure_out = exposure;
    return 0;
}

int ldso_ct_set_new_frame_raw_device(ldso_ct_ctx *c, const void *dev_raw, int32_t bits, float exposure_time, float factor,
                                     const float *b_response, void *producer_stream, float *exposure_out) {
    if (!c || !dev_raw) return fail(-1, "null argument");
    int mode;
    float exposure;
    int rc = und_frame_mode(c, bits, exposure_time, mode, exposure);
    if (rc) return rc;
    if (bits == 16 && (reinterpret_cast<uintptr_t>(dev_raw) & 1)) return fail(-1, "a 16-bit device source must be 2-byte aligned");
    HIP_TRY(hipSetDevice(c->device));
    hipStream_t prod = static_cast<hipStream_t>(producer_stream);
    HIP_TRY(hipEventRecord(c->und_ev_prod.e, prod));
    HIP_TRY(hipStreamWaitEvent(c->stream, c->und_ev_prod.e, 0));
    if ((rc = launch_undistort(c, dev_raw, bits, mode, factor))) return rc;
    // the producer may overwrite its buffer once the one reader of it has run
    HIP_TRY(hipEventRecord(c->und_ev_cons.e, c->stream));
    HIP_TRY(hipStreamWaitEvent(prod, c->und_ev_cons.e, 0));
    if ((rc = frame_pyramid(c, b_response))) return rc;
    c->new_exposure = exposure;
    c->have_frame = true;
    if (exposure_out) *exposure_out = exposure;
    return 0;
}

int ldso_ct_get_undistorted(ldso_ct_ctx *c, float *image) {
    if (!c || !image) return fail(-1, "null argument");
    if (!c->have_frame) return fail(-1, "ldso_ct_set_new_frame not called");
    HIP_TRY(hipSetDevice(c->device));
    HIP_TRY(hipMemcpyAsync(image, c->d_color.p, (size_t)c->pyr.w * c->pyr.h * sizeof(float), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return 0;
}

int ldso_ct_get_frame_level(ldso_ct_ctx *c, int32_t lvl, float *dI, float *abs_sq_grad) {
    if (!c) return fail(-1, "null context");
    if (lvl < 0 || lvl >= c->levels) return fail(-1, "pyramid level out of range");
    if (!c->have_frame) return fail(-1, "ldso_ct_set_new_frame not called");
    const int n = c->pyr.wl[lvl] * c->pyr.hl[lvl];
    std::vector<float4> tmp(n);
    HIP_TRY(hipMemcpyAsync(tmp.data(), c->d_dIp.p + c->pyr.off[lvl], (size_t)n * sizeof(float4), hipMemcpyDeviceToHost,
                          c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    for (int i = 0; i < n; i++) {
        if (dI) {
            dI[3 * i] = tmp[i].x;
            dI[3 * i + 1] = tmp[i].y;
            dI[3 * i + 2] = tmp[i].z;
        }
        if (abs_sq_grad) abs_sq_grad[i] = tmp[i].w;
    }
    return 0;
}

int ldso_ct_set_reference(ldso_ct_ctx *c, const int32_t *pc_n, const float *const *pc_u, const float *const *pc_v,
                          const float *const *pc_idepth, const float *const *pc_color, double ref_ab_exposure,
                          double ref_aff_a, double ref_aff_b) {
    if (!c || !pc_n || !pc_u || !pc_v || !pc_idepth || !pc_color) return fail(-1, "null argument");
    HIP_TRY(hipSetDevice(c->device));
    int off = 0, nmax = 0;
    for (int l = 0; l < c->levels; l++) {
        if (pc_n[l] < 0) return fail(-1, "negative point count");
        if (pc_n[l] > 0 && (!pc_u[l] || !pc_v[l] || !pc_idepth[l] || !pc_color[l]))
            return fail(-1, "null point-cloud level");
        c->pc_off[l] = off;
        off += pc_n[l];
        nmax = std::max(nmax, pc_n[l]);
    }
    c->pc_off[c->levels] = off;
    std::vector<float4> h(std::max(1, off));
    for (int l = 0; l < c->levels; l++)
        for (int i = 0; i < pc_n[l]; i++)
            h[c->pc_off[l] + i] = make_float4(pc_u[l][i], pc_v[l][i], pc_idepth[l][i], pc_color[l][i]);
    HIP_TRY(hipStreamSynchronize(c->stream));  // nothing reads the buffers a larger cloud replaces
    int rc;
    if ((rc = c->d_pc.ensure(off)) || (rc = c->d_state.ensure(nmax)) || (rc = c->d_warp.ensure(2 * (size_t)nmax))) return rc;
    if (off)
        HIP_TRY(hipMemcpyAsync(c->d_pc.p, h.data(), (size_t)off * sizeof(float4), hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    c->ref_exposure = (float)ref_ab_exposure;
    c->ref_a = (float)ref_aff_a;
    c->ref_b = (float)ref_aff_b;
    c->have_ref = true;
    c->last_lvl = -1;
    return 0;
}

int ldso_ct_calc_res(ldso_ct_ctx *c, int32_t lvl, const double ref_to_new[12], double aff_a, double aff_b,
                     float cutoff_th, double rs_out[6]) {
    int rc = check_level(c, lvl);
    if (rc) return rc;
    if (!ref_to_new || !rs_out) return fail(-1, "null argument");
    HIP_TRY(hipSetDevice(c->device));
    rc = run_calc_res(c, lvl, 1, make_pose(c, lvl, ref_to_new, aff_a, aff_b, cutoff_th, c->h_poses.p[0]), true, rs_out);
    if (rc) return rc;
    c->last_lvl = lvl;
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
        ev = make_pose(c, lvl, ref_to_new + 12 * k, aff_ab[2 * k], aff_ab[2 * k + 1], cutoff_th, c->h_poses.p[k]);
    return run_calc_res(c, lvl, n_hyp, ev, false, rs_out);
}

int ldso_ct_calc_gs(ldso_ct_ctx *c, int32_t lvl, const double ref_to_new[12], double aff_a, double aff_b,
                    double *H_out, double *b_out) {
    int rc = check_level(c, lvl);
    if (rc) return rc;
    if (!H_out || !b_out) return fail(-1, "null argument");
    if (c->last_lvl != lvl) return fail(-1, "calcGSSSE needs a calcRes at this level first");
    (void)ref_to_new;  // calcGSSSE reads only the warped buffers and the affine parameters
    HIP_TRY(hipSetDevice(c->device));
    rc = ct_grow(c, c->parts, (size_t)level_grid(c, lvl).nb * kGsParts);
    if (rc) return rc;
    rc = launch_calc_gs(c, lvl, aff_a, aff_b, 0);
    if (rc) return rc;
    HIP_TRY(hipStreamSynchronize(c->stream));  // the partials are in parts.p already
    finish_calc_gs(c, lvl, c->parts.p, H_out, b_out);
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
    const CtEvalTerms ev = make_pose(c, lvl, ref_to_new, aff_a, aff_b, cutoff_th, c->h_poses.p[0]);
    // calcRes and calcGSSSE in one launch (the GS terms of each warped point from the same values
    // the warped buffers receive; the block partials are those of k_ct_calc_gs)
    rc = launch_calc_res(c, lvl, 1, ev, true, (size_t)nb * kGsParts, true);
    if (rc) return rc;
    HIP_TRY(hipStreamSynchronize(c->stream));  // the partials are in parts.p already
    finish_calc_res(c, lvl, 1, true, rs_out);
    c->last_lvl = lvl;
    finish_calc_gs(c, lvl, c->parts.p + res_parts, H_out, b_out);
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
    if ((rc = ct_grow(c, c->track_in, n)) || (rc = ct_grow(c, c->track_out, n)) || (rc = ct_grow(c, c->track_n, 1)) ||
        (trace && (rc = ct_grow(c, c->track_trace, trace_capacity))))
        return rc;
    for (int k = 0; k < n; k++) {
        CtTrackStart &S = c->track_in.p[k];
        std::memcpy(S.ref_to_new, ref_to_new_in + 12 * (size_t)k, sizeof S.ref_to_new);
        std::memcpy(S.aff, aff_in + 2 * (size_t)k, sizeof S.aff);
        std::memcpy(S.min_res, min_res_for_abort + 5 * (size_t)k, sizeof S.min_res);
    }
    CtTrackParams P{};
    for (int l = 0; l <= coarsest_lvl; l++) P.lv[l] = level_of(c, l);
    P.p = p;
    P.starts = c->track_in.dev;
    P.out = c->track_out.dev;
    P.trace = trace ? c->track_trace.dev : nullptr;
    P.trace_n = c->track_n.dev;
    P.trace_capacity = trace ? trace_capacity : 0;
    P.coarsest = coarsest_lvl;
    P.ref_exposure = c->ref_exposure;
    P.new_exposure = c->new_exposure;
    P.ref_a = c->ref_a;
    P.ref_b = c->ref_b;
    c->last_lvl = -1;  // the warped buffers describe no evaluation of this call
    k_ct_track<kTrackWaves><<<n, kTrackWaves * kWave, 0, c->stream>>>(P);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(c->stream));  // results and trace are in host memory already
    std::memcpy(out, c->track_out.p, (size_t)n * sizeof *out);
    const int n_eval = c->track_n.p[0];
    if (trace) std::memcpy(trace, c->track_trace.p, (size_t)std::min(n_eval, trace_capacity) * sizeof *trace);
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
    if (c->last_lvl < 0) return fail(-1, "no calcRes yet");
    const int nw = (c->last_warped + 3) / 4 * 4;
    *n_out = nw;
    if (!out) return 0;
    if (capacity < nw) return fail(-1, "capacity below buf_warped_n");
    const int n = level_grid(c, c->last_lvl).n;
    std::vector<uint8_t> st(std::max(1, n));
    std::vector<float4> wp(2 * (size_t)std::max(1, n));
    HIP_TRY(hipSetDevice(c->device));
    if (n) {
        HIP_TRY(hipMemcpyAsync(st.data(), c->d_state.p, (size_t)n, hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(hipMemcpyAsync(wp.data(), c->d_warp.p, (size_t)n * 2 * sizeof(float4), hipMemcpyDeviceToHost, c->stream));
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

int ldso_ct_make_immature(ldso_ct_ctx *c, int32_t n, const float *uv, float type, int32_t host,
                          ldso_ct_immature *out) {
    if (!c) return fail(-1, "null context");
    if (n < 0 || (n > 0 && (!uv || !out))) return fail(-1, "bad point arguments");
    if (!c->have_frame) return fail(-1, "ldso_ct_set_new_frame has not been called");
    if (n == 0) return 0;
    HIP_TRY(hipSetDevice(c->device));
    // (the stream is idle: every call that uses these buffers ends with a synchronisation)
    int rc;
    if ((rc = c->d_uv.ensure(n)) || (rc = c->d_mk.ensure(n))) return rc;
    HIP_TRY(hipMemcpyAsync(c->d_uv.p, uv, (size_t)n * sizeof(float2), hipMemcpyHostToDevice, c->stream));
    const int w = c->pyr.w, h = c->pyr.h;
    rc = ct_launch(c, kCtSlotMakeImmature, [&] {
        k_ct_make_immature<<<(n + kCtThreads - 1) / kCtThreads, kCtThreads, 0, c->stream>>>(
            c->d_dIp.p, w, h, n, c->d_uv.p, type, host, c->d_mk.p);
    });
    if (rc) return rc;
    HIP_TRY(hipMemcpyAsync(out, c->d_mk.p, (size_t)n * sizeof(IpRec), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return 0;
}

int ldso_ct_immature_upload(ldso_ct_ctx *c, int32_t n, const ldso_ct_immature *pts) {
    if (!c) return fail(-1, "null context");
    if (n < 0 || (n > 0 && !pts)) return fail(-1, "bad point arguments");
    int max_host = -1;
    for (int k = 0; k < n; k++) {
        if (pts[k].host < 0) return fail(-1, "immature point with a negative host index");
        if (pts[k].last_status < 0 || pts[k].last_status > LDSO_CT_IPS_UNINITIALIZED)
            return fail(-1, "immature point with an invalid status");
        max_host = std::max(max_host, (int)pts[k].host);
    }
    HIP_TRY(hipSetDevice(c->device));
    if (int rc = c->d_ip.ensure(n)) return rc;  // (the stream is idle, as in ldso_ct_make_immature)
    if (n) HIP_TRY(hipMemcpyAsync(c->d_ip.p, pts, (size_t)n * sizeof(IpRec), hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    c->ip_n = n;
    c->ip_max_host = max_host;
    return 0;
}

int ldso_ct_immature_download(ldso_ct_ctx *c, int32_t n, ldso_ct_immature *pts) {
    if (!c) return fail(-1, "null context");
    if (n != c->ip_n) return fail(-1, "count differs from the resident immature points");
    if (n == 0) return 0;
    if (!pts) return fail(-1, "null output");
    HIP_TRY(hipSetDevice(c->device));
    HIP_TRY(hipMemcpyAsync(pts, c->d_ip.p, (size_t)n * sizeof(IpRec), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return 0;
}

int ldso_ct_trace(ldso_ct_ctx *c, int32_t n_hosts, const float *krki, const float *kt, const float *aff,
                  int32_t *counts_out) {
    if (!c) return fail(-1, "null context");
    if (!c->have_frame) return fail(-1, "ldso_ct_set_new_frame has not been called");
    if (n_hosts <= c->ip_max_host) return fail(-1, "an immature point's host index is >= n_hosts");
    if (n_hosts > 0 && (!krki || !kt || !aff)) return fail(-1, "null host tables");
    HIP_TRY(hipSetDevice(c->device));
    const size_t n_tab = (size_t)n_hosts * kHostStride;
    int rc;
    if (n_hosts > 0 && ((rc = c->d_hosts.ensure(n_tab)) || (rc = c->h_hosts.ensure(n_tab)))) return rc;
    HIP_TRY(hipStreamSynchronize(c->stream));  // the staging buffer may still feed a previous copy
    for (int i = 0; i < n_hosts; i++) {
        float *o = c->h_hosts.p + (size_t)i * kHostStride;
        std::memcpy(o, krki + 9 * (size_t)i, 9 * sizeof(float));
        std::memcpy(o + 9, kt + 3 * (size_t)i, 3 * sizeof(float));
        o[12] = aff[2 * (size_t)i];
        o[13] = aff[2 * (size_t)i + 1];
        o[14] = o[15] = 0;
    }
    if (n_hosts)
        HIP_TRY(hipMemcpyAsync(c->d_hosts.p, c->h_hosts.p, (size_t)n_hosts * kHostStride * sizeof(float),
                              hipMemcpyHostToDevice, c->stream));
    const int n = c->ip_n;
    if (n > 0) {
        TraceParams P{c->d_dIp.p, c->d_inten.p, c->d_hosts.p, c->d_ip.p, n, c->pyr.w, c->pyr.h};
        const int per = kCtThreads / kWave;
        rc = ct_launch(c, kCtSlotTrace, [&] { k_ct_trace<<<(n + per - 1) / per, kCtThreads, 0, c->stream>>>(P); });
        if (rc) return rc;
    }
    if (counts_out) {
        rc = ct_launch(c, kCtSlotIpCount, [&] { k_ct_ip_count<<<1, 1024, 0, c->stream>>>(c->d_ip.p, n, c->d_counts.p); });
        if (rc) return rc;
        HIP_TRY(hipMemcpyAsync(c->h_counts.p, c->d_counts.p, 6 * sizeof(int), hipMemcpyDeviceToHost, c->stream));
    }
    HIP_TRY(hipStreamSynchronize(c->stream));
    if (counts_out) std::memcpy(counts_out, c->h_counts.p, 6 * sizeof(int));
    return 0;
}

int ldso_ct_make_distance_map(ldso_ct_ctx *c, int32_t n_hosts, const float *krki1, const float *kt1, int32_t n,
                              const float *uvd, const int32_t *host, float *map_out) {
    if (!c) return fail(-1, "null context");
    if (n < 0 || (n > 0 && (!uvd || !host))) return fail(-1, "bad seed arguments");
    for (int k = 0; k < n; k++)
        if (host[k] < 0 || host[k] >= n_hosts) return fail(-1, "a seed's host index is outside [0, n_hosts)");
    int rc = as_begin_map(c, n_hosts, krki1, kt1);
    if (rc) return rc;
    if (n > 0) {
        // (the stream is idle but for the copies above: as_begin_map synchronised)
        if ((rc = c->d_as_uvd.ensure(3 * (size_t)n)) || (rc = c->d_as_seed_host.ensure(n))) return rc;
        HIP_TRY(hipMemcpyAsync(c->d_as_uvd.p, uvd, 3 * (size_t)n * sizeof(float), hipMemcpyHostToDevice, c->stream));
        HIP_TRY(hipMemcpyAsync(c->d_as_seed_host.p, host, (size_t)n * sizeof(int), hipMemcpyHostToDevice, c->stream));
        k_ct_as_seed<<<(n + kCtThreads - 1) / kCtThreads, kCtThreads, 0, c->stream>>>(
            c->d_as_uvd.p, 3, c->d_as_seed_host.p, n, n_hosts, -1, c->d_as_hosts.p, as_grid(c), c->d_as_map.p);
        HIP_TRY(hipGetLastError());
    }
    if ((rc = as_finish_map(c, n_hosts, map_out))) return rc;
    HIP_TRY(hipStreamSynchronize(c->stream));  // the caller's arrays may be reused on return
    return 0;
}

int ldso_ct_make_distance_map_ba(ldso_ct_ctx *c, const ldso_ba_ctx *ba, int32_t win, int32_t newest, const float *krki1,
                                 const float *kt1, float *map_out) {
    if (!c) return fail(-1, "null context");
    if (!ba) return fail(-1, "null bundle-adjustment context");
    ldso_ba::BaRefView V;
    int rc = ldso_ba::ba_ref_view(ba, win, &V);
    if (rc) return rc;
    if (V.device != c->device) return fail(-1, "the bundle-adjustment context is on a different device");
    if (V.marg) return fail(-1, "a marginalisation context holds no active window");
    if (V.sharded) return fail(-1, "the context holds a shard of its points: the distance map needs the whole window");
    if (V.width != c->pyr.w || V.height != c->pyr.h)
        return fail(-1, "the tracker's frame size differs from the window's images");
    if (newest < -1 || newest >= V.N) return fail(-1, "newest out of range");
    if (newest < 0) newest = V.N - 1;
    if ((rc = as_begin_map(c, V.N, krki1, kt1))) return rc;
    if ((rc = c->as_ev_a.ensure(hipEventDisableTiming)) || (rc = c->as_ev_b.ensure(hipEventDisableTiming))) return rc;
    if (V.P > 0) {
        // read the points behind what the BA stream holds now; its later work waits for the read
        hipStream_t bs = static_cast<hipStream_t>(V.stream);
        HIP_TRY(hipEventRecord(c->as_ev_a.e, bs));
        HIP_TRY(hipStreamWaitEvent(c->stream, c->as_ev_a.e, 0));
        k_ct_as_seed<<<(V.P + kCtThreads - 1) / kCtThreads, kCtThreads, 0, c->stream>>>(
            V.pt_data, LDSO_BA_POINT_STRIDE, V.pt_host, V.P, V.N, newest, c->d_as_hosts.p, as_grid(c), c->d_as_map.p);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipEventRecord(c->as_ev_b.e, c->stream));
        HIP_TRY(hipStreamWaitEvent(bs, c->as_ev_b.e, 0));
    }
    return as_finish_map(c, V.N, map_out);
}

int ldso_ct_select_activation(ldso_ct_ctx *c, const ldso_ct_actsel_params *params, const uint8_t *flagged,
                              int32_t compact, int32_t *disposition_out, int32_t *selected_idx_out,
                              int32_t *n_selected_out, int32_t *counts_out) {
    if (!c) return fail(-1, "null context");
    if (!c->as_have_map) return fail(-1, "no distance map: call ldso_ct_make_distance_map first");
    const int n_hosts = c->as_n_hosts, n = c->ip_n;
    ldso_ct_actsel_params p = params ? *params : kActselDefaults;
    if (!params || p.newest_host == -2) p.newest_host = n_hosts - 1;
    if (!(p.current_min_act_dist >= 0 && p.current_min_act_dist <= 4))
        return fail(-1, "current_min_act_dist outside [0, 4]");
    if (std::isnan(p.min_trace_quality)) return fail(-1, "min_trace_quality is NaN");
    if (p.newest_host < -1 || p.newest_host >= n_hosts) return fail(-1, "newest_host out of range");
    if (n_hosts <= c->ip_max_host) return fail(-1, "an immature point's host index is >= the distance map's n_hosts");
    HIP_TRY(hipSetDevice(c->device));
    const AsGrid G = as_grid(c);
    const int n_bins = G.bw * G.bh, nb = sel_blocks(n);
    const size_t cap = std::max<size_t>(c->d_ip.n, 1);
    int rc;
    if ((rc = c->d_as_cand.ensure(cap)) || (rc = c->d_as_entry.ensure(cap)) || (rc = c->d_as_disp.ensure(cap)) ||
        (rc = c->d_as_out.ensure(2 * cap)) || (rc = c->h_as_out.ensure(2 * cap)) ||
        (rc = c->d_as_blk.ensure((size_t)(kAsMaxHosts + 1) * sel_blocks((int)cap))) ||
        (rc = c->d_as_tot.ensure(kAsMaxHosts + 1)) || (rc = c->d_as_cnt.ensure(kAsCnts + 2 * (size_t)n_bins + 1)) ||
        (rc = c->h_as_cnt.ensure(kAsCnts)) || (rc = c->as_counts.ensure(kAsCnts)) ||
        (rc = c->d_as_selected.ensure(cap)) || (rc = c->d_as_flag.ensure(kAsMaxHosts)) ||
        (rc = c->h_as_flag.ensure(kAsMaxHosts)) || (compact && (rc = c->d_ip_alt.ensure(cap))))
        return rc;
    HIP_TRY(hipStreamSynchronize(c->stream));  // the staging buffers and the selection may still be read
    c->as_sel_n = -1;
    int32_t counts[4] = {0, 0, 0, 0};
    int max_host = -1;
    if (n > 0) {
        for (int i = 0; i < kAsMaxHosts; i++) c->h_as_flag.p[i] = (flagged && i < n_hosts && flagged[i]) ? 1 : 0;
        HIP_TRY(hipMemcpyAsync(c->d_as_flag.p, c->h_as_flag.p, kAsMaxHosts, hipMemcpyHostToDevice, c->stream));
        // the counters, the bins' counts (then offsets) and the scatter's cursors: one buffer, one memset
        int *cnt = c->d_as_cnt.p, *bin = cnt + kAsCnts, *cursor = bin + n_bins + 1;
        HIP_TRY(hipMemsetAsync(cnt, 0, (kAsCnts + 2 * (size_t)n_bins + 1) * sizeof(int), c->stream));
        AsClassify K{c->d_ip.p, c->d_as_hosts.p, c->d_as_flag.p, c->d_as_map.p, n, n_hosts, p.newest_host,
                     p.current_min_act_dist, p.min_trace_quality, G};
        k_ct_as_classify<<<nb, kCtThreads, 0, c->stream>>>(K, c->d_as_cand.p, c->d_as_disp.p, bin);
        k_ct_sel_scan<<<1, kCtThreads, 0, c->stream>>>(bin, n_bins + 1, 1, cnt + kAsCntLive);
        k_ct_as_scatter<<<nb, kCtThreads, 0, c->stream>>>(c->d_as_cand.p, c->d_as_disp.p, n, G, bin, cursor,
                                                          c->d_as_entry.p);
        // the rounds, a few launches between two looks at the count of the undecided: four at first (a
        // candidate tries kAsAttempts times per launch), then eight at a time.  The corner pixel's candidates
        // get one launch per batch: enough for the earliest undecided candidate to decide in every batch.
        AsRound R{c->d_as_cand.p, c->d_as_entry.p, bin, c->d_as_map.p, c->d_as_disp.p, cnt, G, n_bins, 0};
        for (int batches = 0, batch = 4;; batches++, batch = 8) {
            if (batches > n + 1) return fail(-2, "the activation walk did not end (internal error)");  // each decides one
            if (batches) HIP_TRY(hipMemsetAsync(cnt + kAsCntUndecided, 0, sizeof(int), c->stream));
            for (int k = 0; k < batch; k++) {
                R.count_undecided = k == batch - 1;
                k_ct_as_round<<<nb, kCtThreads, 0, c->stream>>>(R);
                if (k == batch - 1) k_ct_as_round_corner<<<1, kCtThreads, 0, c->stream>>>(R);
            }
            HIP_TRY(hipGetLastError());
            HIP_TRY(hipMemcpyAsync(c->h_as_cnt.p, cnt, kAsCnts * sizeof(int), hipMemcpyDeviceToHost, c->stream));
            HIP_TRY(hipStreamSynchronize(c->stream));
            if (c->h_as_cnt.p[kAsCntUndecided] == 0) break;
        }
        AsOut O{c->d_ip.p, c->d_as_disp.p, c->d_as_blk.p, cnt, n, nb, n_hosts};
        k_ct_as_count<<<nb, kCtThreads, 0, c->stream>>>(O);
        k_ct_sel_scan<<<1, kCtThreads, 0, c->stream>>>(c->d_as_blk.p, nb, n_hosts + 1, c->d_as_tot.p);
        k_ct_as_write<<<nb, kCtThreads, 0, c->stream>>>(O, c->d_as_tot.p, c->d_as_selected.p, c->d_as_out.p + n,
                                                        compact ? c->d_ip_alt.p : nullptr, c->d_as_out.p,
                                                        c->as_counts.dev);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipMemcpyAsync(c->h_as_out.p, c->d_as_out.p, 2 * (size_t)n * sizeof(int), hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(hipStreamSynchronize(c->stream));  // the counters are in mapped host memory
        for (int k = 0; k < 4; k++) counts[k] = c->as_counts.p[k];
        max_host = c->as_counts.p[kAsCntMaxHost] - 1;
        if (disposition_out) std::memcpy(disposition_out, c->h_as_out.p, (size_t)n * sizeof(int));
        if (selected_idx_out) std::memcpy(selected_idx_out, c->h_as_out.p + n, (size_t)counts[2] * sizeof(int));
        if (compact) {
            std::swap(c->d_ip.p, c->d_ip_alt.p);
            std::swap(c->d_ip.n, c->d_ip_alt.n);
            c->ip_n = counts[0];
            c->ip_max_host = max_host;
        }
    }
    c->as_sel_n = counts[2];
    c->as_sel_hosts = n_hosts;
    if (n_selected_out) *n_selected_out = counts[2];
    if (counts_out) std::memcpy(counts_out, counts, sizeof counts);
    return 0;
}

int ldso_ct_selection_download(ldso_ct_ctx *c, int32_t n, ldso_ct_immature *pts) {
    if (!c) return fail(-1, "null context");
    if (c->as_sel_n < 0) return fail(-1, "no selection: call ldso_ct_select_activation first");
    if (n != c->as_sel_n) return fail(-1, "count differs from the selection");
    if (n == 0) return 0;
    if (!pts) return fail(-1, "null output");
    HIP_TRY(hipSetDevice(c->device));
    HIP_TRY(hipMemcpyAsync(pts, c->d_as_selected.p, (size_t)n * sizeof(IpRec), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return 0;
}

int ldso_ct_immature_append(ldso_ct_ctx *c, int32_t n, const ldso_ct_immature *pts) {
    if (!c) return fail(-1, "null context");
    if (n < 0 || (n > 0 && !pts)) return fail(-1, "bad point arguments");
    int max_host = c->ip_max_host;
    for (int k = 0; k < n; k++) {
        if (pts[k].host < 0) return fail(-1, "immature point with a negative host index");
        if (pts[k].last_status < 0 || pts[k].last_status > LDSO_CT_IPS_UNINITIALIZED)
            return fail(-1, "immature point with an invalid status");
        max_host = std::max(max_host, (int)pts[k].host);
    }
    if (n == 0) return 0;
    HIP_TRY(hipSetDevice(c->device));
    const size_t need = (size_t)c->ip_n + n;
    if (c->d_ip.n < need || !c->d_ip.p) {
        // a larger buffer with room to spare, the resident records moved over on the device
        HIP_TRY(hipStreamSynchronize(c->stream));
        if (int rc = c->d_ip_alt.alloc(std::max(need, 2 * c->d_ip.n))) return rc;
        if (c->ip_n)
            HIP_TRY(hipMemcpyAsync(c->d_ip_alt.p, c->d_ip.p, (size_t)c->ip_n * sizeof(IpRec), hipMemcpyDeviceToDevice,
                                   c->stream));
        std::swap(c->d_ip.p, c->d_ip_alt.p);
        std::swap(c->d_ip.n, c->d_ip_alt.n);
    }
    HIP_TRY(hipMemcpyAsync(c->d_ip.p + c->ip_n, pts, (size_t)n * sizeof(IpRec), hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    c->ip_n += n;
    c->ip_max_host = max_host;
    return 0;
}

}  // extern "C"

// ---- the coarse initializer (k_ct_init.h, ct_init.h) -------------------------------------------
// the BA frame store's view of firstFrame's level 0 (ldso_ba_frame_put_initializer)
int ldso_ba::ct_init_frame_view(const ldso_ct_ctx *c, ldso_ba::CtFrameView *out) {
    if (!c || !out) return fail(-1, "null argument");
    out->intensity = c->d_init_inten.p;
    out->texels = c->d_init_first.p;
    out->width = c->pyr.w;
    out->height = c->pyr.h;
    out->device = c->device;
    out->stream = (void *)c->stream;
    out->have_frame = c->init_have_first;
    return 0;
}

namespace {

constexpr ldso_ct_init_params kInitDefaults = {2.5f * 2.5f, 150.f * 150.f, 0.8f, 1.0f, {5, 5, 10, 30, 50}, 1, 9.0f};

int init_check_params(const ldso_ct_init_params &p) {
    const float v[5] = {p.alpha_k, p.alpha_w, p.reg_weight, p.coupling_weight, p.huber_th};
    for (float x : v)
        if (!std::isfinite(x) || !(x > 0))
            return fail(-1, "alpha_k, alpha_w, reg_weight, coupling_weight and huber_th must be finite and > 0");
    for (int l = 0; l < 5; l++)
        if (p.max_iterations[l] < 0 || p.max_iterations[l] > ldso_ct::kInitMaxIterations)
            return fail(-1, "max_iterations out of range [0, 1000]");
    if (p.fix_affine != 0 && p.fix_affine != 1) return fail(-1, "fix_affine must be 0 or 1");
    return 0;
}

int init_check_ready(const ldso_ct_ctx *c) {
    if (!c) return fail(-1, "null context");
    if (!c->init_have_first) return fail(-1, "ldso_ct_init_set_first not called");
    if (!c->have_frame) return fail(-1, "ldso_ct_set_new_frame not called");
    return 0;
}

// the kernels' argument: the levels, the buffers and the carried state
void init_fill(const ldso_ct_ctx *c, const ldso_ct_init_params &p, CtInitParams &P) {
    P = CtInitParams{};
    const int *tab = c->d_init_tab.p;
    const double fx0 = c->fx[0], fy0 = c->fy[0], cx0 = c->cx[0], cy0 = c->cy[0];
    double fx = fx0, fy = fy0;
    for (int l = 0; l < c->levels; l++) {
        CtInitLevel &L = P.lv[l];
        L.pts = c->d_init_pts.p + c->init_off[l];
        L.ref = c->d_init_first.p + c->pyr.off[l];
        L.img = c->d_dIp.p + c->pyr.off[l];
        L.order = tab + c->init_order_off[l];
        L.rank_off = tab + c->init_rank_off[l];
        L.child_off = tab + c->init_child_off[l];
        L.child = tab + c->init_child[l];
        L.n = c->init_off[l + 1] - c->init_off[l];
        L.n_ranks = c->init_n_ranks[l];
        L.wl = c->pyr.wl[l];
        L.hl = c->pyr.hl[l];
        // makeK (:811-837): fx, cx per level in double, fxl = the float of it
        if (l > 0) {
            fx = fx * 0.5;
            fy = fy * 0.5;
        }
        const double cx = l == 0 ? cx0 : (cx0 + 0.5) / ((int)1 << l) - 0.5;
        const double cy = l == 0 ? cy0 : (cy0 + 0.5) / ((int)1 << l) - 0.5;
        L.fxl = (float)fx;
        L.fyl = (float)fy;
        L.cxl = (float)cx;
        L.cyl = (float)cy;
        ldso_ct::init_make_ki(fx, fy, cx, cy, L.Ki);
    }
    P.p = p;
    P.jb[0] = c->d_init_jb.p;
    P.jb[1] = c->d_init_jb.p + (size_t)c->init_max_n * 10;
    P.jb_cur = c->init_jb_cur;
    P.levels = c->levels;
    std::memcpy(P.this_to_next, c->init_this_to_next, sizeof P.this_to_next);
    P.aff[0] = c->init_aff[0];
    P.aff[1] = c->init_aff[1];
    P.snapped = c->init_snapped;
    P.frame_id = c->init_frame_id;
    P.snapped_at = c->init_snapped_at;
    P.out = c->init_out.dev;
}

}  // namespace

extern "C" {

void ldso_ct_init_default_params(ldso_ct_init_params *p) {
    if (p) *p = kInitDefaults;
}

int ldso_ct_init_check_points(int32_t levels, int32_t width, int32_t height, const int32_t *n_per_level,
                              const ldso_ct_init_point *const *pts_per_level) {
    if (!n_per_level || !pts_per_level) return fail(-1, "null argument");
    if (levels < 1 || levels > ldso_ct::kInitMaxLevels) return fail(-1, "the initializer covers 1 to 5 pyramid levels");
    for (int l = 0; l < levels; l++) {
        if (n_per_level[l] < 1) return fail(-1, "every level needs at least one point (level " + std::to_string(l) + ")");
        if (!pts_per_level[l]) return fail(-1, "null point list (level " + std::to_string(l) + ")");
    }
    for (int l = 0; l < levels; l++) {
        const int n = n_per_level[l], wl = width >> l, hl = height >> l;
        const std::string at = " (level " + std::to_string(l) + ")";
        for (int i = 0; i < n; i++) {
            const ldso_ct_init_point &pt = pts_per_level[l][i];
            // the pattern reaches 2 pixels, and the first frame is interpolated there without a check
            if (!(pt.u >= 2 && pt.v >= 2 && pt.u + 2 < wl - 1 && pt.v + 2 < hl - 1))
                return fail(-1, "point " + std::to_string(i) + at + ": u, v must be finite and at least 2 pixels inside the interpolable area");
            for (int j = 0; j < 10; j++)
                if (pt.neighbours[j] < -1 || pt.neighbours[j] >= n)
                    return fail(-1, "point " + std::to_string(i) + at + ": neighbour " + std::to_string(j) + " is neither -1 nor in range");
            if (l == levels - 1) {
                if (pt.parent != -1) return fail(-1, "point " + std::to_string(i) + at + ": parent must be -1 on the top level");
            } else if (pt.parent < 0 || pt.parent >= n_per_level[l + 1]) {
                return fail(-1, "point " + std::to_string(i) + at + ": parent out of range of the next level");
            }
        }
    }
    return 0;
}

int ldso_ct_init_set_first(ldso_ct_ctx *c, const int32_t *n_per_level, const ldso_ct_init_point *const *pts_per_level) {
    if (!c) return fail(-1, "null context");
    if (!c->have_k) return fail(-1, "ldso_ct_make_k not called");
    if (!c->have_frame) return fail(-1, "ldso_ct_set_new_frame not called");
    int rc = ldso_ct_init_check_points(c->levels, c->pyr.w, c->pyr.h, n_per_level, pts_per_level);
    if (rc) return rc;
    HIP_TRY(hipSetDevice(c->device));
    const int Lv = c->levels;
    int off = 0, max_n = 0;
    for (int l = 0; l < Lv; l++) {
        c->init_off[l] = off;
        off += n_per_level[l];
        max_n = std::max(max_n, (int)n_per_level[l]);
    }
    c->init_off[Lv] = off;
    // the int table: per level the sweep order [n], the rank offsets [n_ranks + 1], and, for the level
    // above, the child offsets [n + 1] and the children [n of the level below]
    std::vector<int> tab;
    std::vector<ldso_ct_init_point> all((size_t)off);
    for (int l = 0; l < Lv; l++) {
        const int n = n_per_level[l];
        const ldso_ct_init_point *pts = pts_per_level[l];
        std::copy(pts, pts + n, all.begin() + c->init_off[l]);
        // rank = 1 + the largest rank among the adjacent points of smaller index; adjacent: one lists the other
        std::vector<int> rank(n, 0);
        for (int i = 0; i < n; i++) {
            for (int j = 0; j < 10; j++) {
                const int nb = pts[i].neighbours[j];
                if (nb >= 0 && nb < i) rank[i] = std::max(rank[i], rank[nb] + 1);
            }
            for (int j = 0; j < 10; j++) {
                const int nb = pts[i].neighbours[j];
                if (nb > i) rank[nb] = std::max(rank[nb], rank[i] + 1);
            }
        }
        const int n_ranks = *std::max_element(rank.begin(), rank.end()) + 1;
        std::vector<int> roff(n_ranks + 1, 0), order(n);
        for (int i = 0; i < n; i++) roff[rank[i] + 1]++;
        for (int r = 0; r < n_ranks; r++) roff[r + 1] += roff[r];
        std::vector<int> cur(roff.begin(), roff.end() - 1);
        for (int i = 0; i < n; i++) order[cur[rank[i]]++] = i;
        c->init_n_ranks[l] = n_ranks;
        c->init_order_off[l] = (int)tab.size();
        tab.insert(tab.end(), order.begin(), order.end());
        c->init_rank_off[l] = (int)tab.size();
        tab.insert(tab.end(), roff.begin(), roff.end());
        // the children of this level's points (the level below's, by parent, ascending)
        std::vector<int> coff(n + 1, 0), child;
        if (l > 0) {
            const int nc = n_per_level[l - 1];
            const ldso_ct_init_point *cp = pts_per_level[l - 1];
            child.resize(nc);
            for (int i = 0; i < nc; i++) coff[cp[i].parent + 1]++;
            for (int i = 0; i < n; i++) coff[i + 1] += coff[i];
            std::vector<int> cc(coff.begin(), coff.end() - 1);
            for (int i = 0; i < nc; i++) child[cc[cp[i].parent]++] = i;
        }
        c->init_child_off[l] = (int)tab.size();
        tab.insert(tab.end(), coff.begin(), coff.end());
        c->init_child[l] = (int)tab.size();
        tab.insert(tab.end(), child.begin(), child.end());
    }
    tab.push_back(0);  // never empty
    HIP_TRY(hipStreamSynchronize(c->stream));  // nothing reads the buffers a larger set replaces
    const size_t npx = c->pyr.off[Lv], px0 = (size_t)c->pyr.w * c->pyr.h;
    if ((rc = c->d_init_first.ensure(npx)) || (rc = c->d_init_inten.ensure(px0)) || (rc = c->d_init_pts.ensure(off)) ||
        (rc = c->d_init_tab.ensure(tab.size())) || (rc = c->d_init_jb.ensure((size_t)max_n * 20)) ||
        (rc = c->init_out.ensure(1)))
        return rc;
    c->init_have_first = false;
    HIP_TRY(hipMemcpyAsync(c->d_init_first.p, c->d_dIp.p, npx * sizeof(float4), hipMemcpyDeviceToDevice, c->stream));
    HIP_TRY(hipMemcpyAsync(c->d_init_inten.p, c->d_inten.p, px0 * sizeof(float), hipMemcpyDeviceToDevice, c->stream));
    HIP_TRY(hipMemcpyAsync(c->d_init_pts.p, all.data(), all.size() * sizeof all[0], hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipMemcpyAsync(c->d_init_tab.p, tab.data(), tab.size() * sizeof(int), hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipMemsetAsync(c->d_init_jb.p, 0, (size_t)max_n * 20 * sizeof(float), c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));  // the caller's lists may be reused on return
    c->init_max_n = max_n;
    c->init_jb_cur = 0;
    c->init_first_exposure = c->new_exposure;
    const double eye[12] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0};
    std::memcpy(c->init_this_to_next, eye, sizeof eye);
    c->init_aff[0] = c->init_aff[1] = 0;
    c->init_snapped = c->init_frame_id = c->init_snapped_at = 0;  // setFirst, :730-732
    c->init_have_first = true;
    return 0;
}

int ldso_ct_init_rank_counts(ldso_ct_ctx *c, int32_t *out) {
    if (!c || !out) return fail(-1, "null argument");
    if (!c->init_have_first) return fail(-1, "ldso_ct_init_set_first not called");
    for (int l = 0; l < c->levels; l++) out[l] = c->init_n_ranks[l];
    return 0;
}

int ldso_ct_init_get_points(ldso_ct_ctx *c, int32_t lvl, ldso_ct_init_point *out, int32_t capacity, int32_t *n_out) {
    if (!c) return fail(-1, "null context");
    if (!c->init_have_first) return fail(-1, "ldso_ct_init_set_first not called");
    if (lvl < 0 || lvl >= c->levels) return fail(-1, "pyramid level out of range");
    const int n = c->init_off[lvl + 1] - c->init_off[lvl];
    if (n_out) *n_out = n;
    if (!out) return 0;
    if (capacity < n) return fail(-1, "capacity below the level's point count");
    HIP_TRY(hipSetDevice(c->device));
    HIP_TRY(hipMemcpyAsync(out, c->d_init_pts.p + c->init_off[lvl], (size_t)n * sizeof *out, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return 0;
}

int ldso_ct_init_set_points(ldso_ct_ctx *c, int32_t lvl, int32_t n, const ldso_ct_init_point *pts) {
    if (!c || !pts) return fail(-1, "null argument");
    if (!c->init_have_first) return fail(-1, "ldso_ct_init_set_first not called");
    if (lvl < 0 || lvl >= c->levels) return fail(-1, "pyramid level out of range");
    if (n != c->init_off[lvl + 1] - c->init_off[lvl]) return fail(-1, "n is not the level's point count");
    std::vector<ldso_ct_init_point> cur((size_t)n);
    int rc = ldso_ct_init_get_points(c, lvl, cur.data(), n, nullptr);
    if (rc) return rc;
    for (int i = 0; i < n; i++)
        if (pts[i].parent != cur[i].parent || std::memcmp(pts[i].neighbours, cur[i].neighbours, sizeof cur[i].neighbours) ||
            pts[i].u != cur[i].u || pts[i].v != cur[i].v)
            return fail(-1, "point " + std::to_string(i) + ": u, v and the tables must be the resident ones");
    HIP_TRY(hipMemcpyAsync(c->d_init_pts.p + c->init_off[lvl], pts, (size_t)n * sizeof *pts, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return 0;
}

int ldso_ct_init_eval(ldso_ct_ctx *c, int32_t lvl, const double ref_to_new[12], const double aff[2],
                      const ldso_ct_init_params *params, float H[64], float b[8], float Hsc[64], float bsc[8],
                      float res[3], int32_t *alpha_capped_out) {
    const ldso_ct_init_params p = params ? *params : kInitDefaults;
    int rc = init_check_params(p);
    if (rc) return rc;
    if ((rc = init_check_ready(c))) return rc;
    if (lvl < 0 || lvl >= c->levels) return fail(-1, "pyramid level out of range");
    if (!ref_to_new || !aff || !H || !b || !Hsc || !bsc || !res) return fail(-1, "null argument");
    HIP_TRY(hipSetDevice(c->device));
    CtInitParams P;
    init_fill(c, p, P);
    P.arg_lvl = lvl;
    std::memcpy(P.arg_pose, ref_to_new, sizeof P.arg_pose);
    P.arg_aff[0] = (float)aff[0];
    P.arg_aff[1] = (float)aff[1];
    k_ct_init_eval<<<1, kInitThreads, 0, c->stream>>>(P);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(c->stream));  // the results are in host memory already
    const CtInitOut &O = *c->init_out.p;
    std::memcpy(H, O.H, sizeof O.H);
    std::memcpy(b, O.b, sizeof O.b);
    std::memcpy(Hsc, O.Hsc, sizeof O.Hsc);
    std::memcpy(bsc, O.bsc, sizeof O.bsc);
    std::memcpy(res, O.res, sizeof O.res);
    if (alpha_capped_out) *alpha_capped_out = O.alpha_capped;
    return 0;
}

int ldso_ct_init_lm_step(const float H[64], const float b[8], const float Hsc[64], const float bsc[8], float lambda,
                         int32_t w, int32_t h, const double pose[12], const double aff[2],
                         const ldso_ct_init_params *params, float inc_out[8], double pose_out[12], double aff_out[2]) {
    if (!H || !b || !Hsc || !bsc || !pose || !aff || !inc_out || !pose_out || !aff_out) return fail(-1, "null argument");
    const ldso_ct_init_params p = params ? *params : kInitDefaults;
    if (int rc = init_check_params(p)) return rc;
    if (w < 1 || h < 1 || (long long)w * h > (1ll << 30)) return fail(-1, "bad level size");
    ldso_ct::LdltWorkF W;
    ldso_ct::Pose cand;
    const float a[2] = {(float)aff[0], (float)aff[1]};
    float an[2];
    ldso_ct::init_lm_step(H, b, Hsc, bsc, lambda, w, h, ldso_ct::init_pose_from_matrix(pose), a, p, W, inc_out, cand, an);
    ldso_ct::pose_matrix(cand, pose_out);
    aff_out[0] = an[0];
    aff_out[1] = an[1];
    return 0;
}

int ldso_ct_init_opt_reg(ldso_ct_ctx *c, int32_t lvl, float reg_weight, int32_t snapped) {
    if (!c) return fail(-1, "null context");
    if (!c->init_have_first) return fail(-1, "ldso_ct_init_set_first not called");
    if (lvl < 0 || lvl >= c->levels) return fail(-1, "pyramid level out of range");
    if (!std::isfinite(reg_weight)) return fail(-1, "reg_weight must be finite");
    HIP_TRY(hipSetDevice(c->device));
    CtInitParams P;
    init_fill(c, kInitDefaults, P);
    P.arg_lvl = lvl;
    P.arg_reg_weight = reg_weight;
    P.snapped = snapped != 0;
    k_ct_init_opt_reg<<<1, kInitThreads, 0, c->stream>>>(P);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(c->stream));
    return 0;
}

int ldso_ct_init_track_frame(ldso_ct_ctx *c, const ldso_ct_init_params *params, ldso_ct_init_result *result,
                             ldso_ct_init_step *trace, int32_t trace_capacity, int32_t *trace_n) {
    const ldso_ct_init_params p = params ? *params : kInitDefaults;
    int rc = init_check_params(p);
    if (rc) return rc;
    if ((rc = init_check_ready(c))) return rc;
    if (!result) return fail(-1, "null argument");
    if (trace && trace_capacity < 1) return fail(-1, "trace_capacity must be >= 1 with a trace");
    HIP_TRY(hipSetDevice(c->device));
    if (trace && (rc = ct_grow(c, c->init_trace, trace_capacity))) return rc;
    CtInitParams P;
    init_fill(c, p, P);
    // :71-73, the exposure-ratio guess; logf on the host, so that one libm serves every caller
    if (c->init_first_exposure > 0 && c->new_exposure > 0) {
        P.have_guess = 1;
        P.aff_guess = logf(c->new_exposure / c->init_first_exposure);
    }
    P.trace = trace ? c->init_trace.dev : nullptr;
    P.trace_capacity = trace ? trace_capacity : 0;
    k_ct_init_track<<<1, kInitThreads, 0, c->stream>>>(P);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(c->stream));  // result and trace are in host memory already
    const CtInitOut &O = *c->init_out.p;
    *result = O.R;
    int clock_khz = 0;  // of wall_clock64
    if (hipDeviceGetAttribute(&clock_khz, hipDeviceAttributeWallClockRate, c->device) != hipSuccess || clock_khz <= 0)
        clock_khz = 100000;
    for (int i = 0; i < 4; i++) result->phase_us[i] = (float)((double)O.ticks[i] * 1e3 / clock_khz);
    std::memcpy(c->init_this_to_next, O.R.this_to_next, sizeof O.R.this_to_next);
    c->init_aff[0] = (float)O.R.this_to_next_aff[0];
    c->init_aff[1] = (float)O.R.this_to_next_aff[1];
    c->init_snapped = O.R.snapped;
    c->init_frame_id = O.R.frame_id;
    c->init_snapped_at = O.R.snapped_at;
    c->init_jb_cur = O.jb_cur;
    if (trace) std::memcpy(trace, c->init_trace.p, (size_t)std::min(O.n_eval, trace_capacity) * sizeof *trace);
    if (trace_n) *trace_n = O.n_eval;
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
