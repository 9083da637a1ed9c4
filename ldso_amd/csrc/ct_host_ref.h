// ct_host_ref.h -- the reference cloud: set from the host or built on the device from the window's contributions
// (k_ct_coarse_depth.h).  Owns c->ref.  Reads frame.d_dIp of this or another context; grows res.d_state /
// res.d_warp to the reference's largest level and resets res.last_lvl.
// A piece of the one translation unit ldso_ct.hip (k_ct_pyramid.h).
#pragma once
#include <algorithm>
#include <vector>

#include "../../include/ldso_ba.h"
#include "ldso_ba_internal.h"
#include "ct_context.h"

#pragma clang fp contract(off)

namespace {

// ---- the reference cloud built on the device (k_ct_coarse_depth.h) ----------------------------
// the work buffers, whose sizes follow the context's image size: allocated by the first call only.
// The cloud holds at most the interior pixels of every level, the warped buffers those of level 0.
int cd_ensure(ldso_ct_ctx *c) {
    const PyrParams &P = c->pyr;
    const int npx = P.off[P.levels];
    if (!c->ref.interior0 && !c->ref.lv.blk_off[P.levels]) {
        int nb = 0;
        for (int l = 0; l <= LDSO_CT_MAX_LEVELS; l++) {
            c->ref.lv.blk_off[l] = nb;
            if (l >= P.levels) continue;
            nb += (P.wl[l] * P.hl[l] + kCtThreads - 1) / kCtThreads;
            const int in = std::max(0, P.wl[l] - 4) * std::max(0, P.hl[l] - 4);
            c->ref.interior += in;
            if (l == 0) c->ref.interior0 = in;
        }
    }
    const int nb = c->ref.lv.blk_off[P.levels];
    int rc;
    if ((rc = c->ref.d_maps.ensure(2 * (size_t)npx)) || (rc = c->ref.d_cand.ensure(npx)) ||
        (rc = c->ref.d_blk.ensure((size_t)nb + LDSO_CT_MAX_LEVELS + 1)) || (rc = c->ref.counts.ensure(LDSO_CT_MAX_LEVELS)) ||
        (rc = ct_grow(c, c->ref.d_pc, std::max(1, c->ref.interior))))
        return rc;
    const size_t n0 = c->ref.interior0;
    if (c->res.d_state.n < n0 || c->res.d_warp.n < 2 * n0) {
        HIP_TRY(hipStreamSynchronize(c->stream));
        if ((rc = c->res.d_state.ensure(n0)) || (rc = c->res.d_warp.ensure(2 * n0))) return rc;
    }
    return 0;
}

// the checks both make calls share, before any HIP call; *src = the context whose frame is read
int cd_check(ldso_ct_ctx *c, const ldso_ct_ctx *frame_src, const ldso_ct_ctx **src) {
    if (!c) return fail(-1, "null context");
    const ldso_ct_ctx *s = frame_src ? frame_src : c;
    if (s->device != c->device) return fail(-1, "frame_src is on a different device");
    if (s->pyr.w != c->pyr.w || s->pyr.h != c->pyr.h) return fail(-1, "frame_src has a different image size");
    if (!s->frame.have) return fail(-1, "ldso_ct_set_new_frame has not been called on the frame source");
    *src = s;
    return 0;
}

// from n contributions in ref.d_contrib to the resident cloud: maps, pyramid, dilation, compaction,
// one synchronisation for the per-level counts
int cd_build(ldso_ct_ctx *c, const ldso_ct_ctx *src, int n, double ref_ab_exposure, double ref_aff_a, double ref_aff_b,
             int32_t *pc_n_out) {
    const PyrParams &P = c->pyr;
    const int npx = P.off[P.levels], nb = c->ref.lv.blk_off[P.levels];
    const size_t px0 = (size_t)P.w * P.h;
    float *idm = c->ref.d_maps.p, *wm = idm + npx;
    int *blk = c->ref.d_blk.p, *lvl_off = blk + nb;
    // level 0 of both maps is summed into; the coarser levels are written whole
    HIP_TRY(hipMemsetAsync(idm, 0, px0 * sizeof(float), c->stream));
    HIP_TRY(hipMemsetAsync(wm, 0, px0 * sizeof(float), c->stream));
    if (n > 0)
        k_ct_cd_scatter<<<(n + kCtThreads - 1) / kCtThreads, kCtThreads, 0, c->stream>>>(c->ref.d_contrib.p, n, idm, wm,
                                                                                        P.w, P.h);
    if (P.levels > 1) {
        const size_t lds = 2 * ((size_t)P.tile * P.tile + (size_t)(P.tile / 2) * (P.tile / 2)) * sizeof(float);
        k_ct_cd_pyr<<<dim3(P.w / P.tile, P.h / P.tile), kCtThreads, lds, c->stream>>>(idm, wm, P);
    }
    // the colours come from the frame source's pyramid: wait for what its stream holds now, and
    // let whatever it is given later (its next frame) wait for the read
    int rc;
    if (src != c && (rc = c->ref.borrow.begin(c->stream, src->stream))) return rc;
    k_ct_cd_flag<<<nb, kCtThreads, 0, c->stream>>>(idm, wm, src->frame.d_dIp.p, c->ref.d_cand.p, blk, P, c->ref.lv);
    if (src != c && (rc = c->ref.borrow.end(c->stream, src->stream))) return rc;
    k_ct_cd_scan<<<1, kCtThreads, 0, c->stream>>>(blk, lvl_off, c->ref.counts.dev, P.levels, c->ref.lv);
    k_ct_cd_write<<<nb, kCtThreads, 0, c->stream>>>(c->ref.d_cand.p, blk, lvl_off, c->ref.d_pc.p, P, c->ref.lv);
    HIP_TRY(hipGetLastError());
    c->ref.have = false;  // until the counts are in
    HIP_TRY(hipStreamSynchronize(c->stream));
    int off = 0;
    for (int l = 0; l < c->levels; l++) {
        c->ref.pc_off[l] = off;
        off += c->ref.counts.p[l];
        if (pc_n_out) pc_n_out[l] = c->ref.counts.p[l];
    }
    c->ref.pc_off[c->levels] = off;
    c->ref.exposure = (float)ref_ab_exposure;
    c->ref.a = (float)ref_aff_a;
    c->ref.b = (float)ref_aff_b;
    c->ref.have = true;
    c->res.last_lvl = -1;
    return 0;
}

}  // namespace

extern "C" {

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
        if ((rc = ct_grow(c, c->ref.d_contrib, n)) || (rc = ct_grow(c, c->ref.h_contrib, n))) return rc;
        // (the staging buffer is free: every call that copies out of it ends with a synchronisation)
        for (int i = 0; i < n; i++)
            c->ref.h_contrib.p[i] = make_float4(center[3 * (size_t)i], center[3 * (size_t)i + 1], center[3 * (size_t)i + 2], hdi[i]);
        HIP_TRY(hipMemcpyAsync(c->ref.d_contrib.p, c->ref.h_contrib.p, (size_t)n * sizeof(float4), hipMemcpyHostToDevice,
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
        if ((rc = ct_grow(c, c->ref.d_contrib, n))) return rc;
        // read the pass's arrays behind what the BA stream holds now; its later work waits for the read
        hipStream_t bs = static_cast<hipStream_t>(V.stream);
        if ((rc = c->ref.borrow.begin(c->stream, bs))) return rc;
        HIP_TRY(hipMemsetAsync(c->ref.d_contrib.p, 0xFF, (size_t)n * sizeof(float4), c->stream));  // NaN: no contribution
        CdGatherParams G{V.center, V.plane_stride, V.state, V.tgt, V.slot, V.pt_out, c->ref.d_contrib.p,
                         V.R,      V.P,            V.rec_base, ref_frame};
        k_ct_cd_gather<<<(V.R + kCtThreads - 1) / kCtThreads, kCtThreads, 0, c->stream>>>(G);
        HIP_TRY(hipGetLastError());
        if ((rc = c->ref.borrow.end(c->stream, bs))) return rc;
    }
    return cd_build(c, src, n, ref_ab_exposure, ref_aff_a, ref_aff_b, pc_n_out);
}

int ldso_ct_get_reference(ldso_ct_ctx *c, int32_t lvl, int32_t *n_out, float *out, int32_t capacity) {
    if (!c || !n_out) return fail(-1, "null argument");
    if (lvl < 0 || lvl >= c->levels) return fail(-1, "pyramid level out of range");
    if (!c->ref.have) return fail(-1, "no reference: call ldso_ct_set_reference or ldso_ct_make_reference first");
    const int n = level_grid(c, lvl).n;
    *n_out = n;
    if (!out || n == 0) return 0;
    if (capacity < n) return fail(-1, "capacity below the level's point count");
    HIP_TRY(hipSetDevice(c->device));
    return ct_read(c, out, c->ref.d_pc.p + c->ref.pc_off[lvl], n);
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
        c->ref.pc_off[l] = off;
        off += pc_n[l];
        nmax = std::max(nmax, pc_n[l]);
    }
    c->ref.pc_off[c->levels] = off;
    std::vector<float4> h(std::max(1, off));
    for (int l = 0; l < c->levels; l++)
        for (int i = 0; i < pc_n[l]; i++)
            h[c->ref.pc_off[l] + i] = make_float4(pc_u[l][i], pc_v[l][i], pc_idepth[l][i], pc_color[l][i]);
    HIP_TRY(hipStreamSynchronize(c->stream));  // nothing reads the buffers a larger cloud replaces
    int rc;
    if ((rc = c->ref.d_pc.ensure(off)) || (rc = c->res.d_state.ensure(nmax)) || (rc = c->res.d_warp.ensure(2 * (size_t)nmax))) return rc;
    if (off)
        HIP_TRY(hipMemcpyAsync(c->ref.d_pc.p, h.data(), (size_t)off * sizeof(float4), hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    c->ref.exposure = (float)ref_ab_exposure;
    c->ref.a = (float)ref_aff_a;
    c->ref.b = (float)ref_aff_b;
    c->ref.have = true;
    c->res.last_lvl = -1;
    return 0;
}

}  // extern "C"
