// ct_host_cor.h -- corner detection: DetectCorners with ORB (k_ct_corners.h).  Owns c->cor.  Reads frame.d_dIp;
// ldso_ct_detect_corners fills the core's d_mk.
// A piece of the one translation unit ldso_ct.hip (k_ct_pyramid.h).
#pragma once
#include <algorithm>
#include <cmath>
#include <cstddef>
#include <cstring>
#include <string>

#include "ldso_ba_internal.h"
#include "ct_context.h"

#pragma clang fp contract(off)

// the loop closer's view of the last corner detection (ldso_lc_keyframe_put_tracker)
int ldso_ba::ct_corners_view(const ldso_ct_ctx *c, ldso_ba::CtCornersView *out) {
    if (!c || !out) return fail(-1, "null argument");
    static_assert(sizeof(CorSlot) == 4 * sizeof(int) && offsetof(CorSlot, x) == 0 && offsetof(CorSlot, y) == sizeof(int),
                  "CtCornersView reads x, y at the start of a CorSlot");
    out->pixel = reinterpret_cast<const int *>(c->cor.d_feat.p);
    out->pixel_stride = sizeof(CorSlot) / sizeof(int);
    out->records = c->cor.d_out.p;
    out->n = c->cor.n;
    out->width = c->pyr.w;
    out->height = c->pyr.h;
    out->device = c->device;
    out->stream = (void *)c->stream;
    return 0;
}

namespace {

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

}  // namespace

extern "C" {

int ldso_ct_corners_init(ldso_ct_ctx *c, const int32_t *bit_pattern) {
    if (!c || !bit_pattern) return fail(-1, "null argument");
    for (int i = 0; i < 1024; i++)
        if (bit_pattern[i] < -kCorPatternRange || bit_pattern[i] > kCorPatternRange)
            return fail(-1, "bit_pattern entry " + std::to_string(i) + " outside [-13, 13]");
    HIP_TRY(hipSetDevice(c->device));
    if (int rc = ct_grow(c, c->cor.d_pattern, 256)) return rc;
    HIP_TRY(hipMemcpyAsync(c->cor.d_pattern.p, bit_pattern, 1024 * sizeof(int32_t), hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));  // the caller's table may be reused on return
    // FeatureDetector::FeatureDetector (FeatureDetector.cc:10-28); cvFloor / cvCeil / cvRound as floor / ceil / rint
    constexpr int H = kCorHalfPatch;
    int *umax = c->cor.umax.u;
    int v, v0;
    const int vmax = (int)std::floor(H * std::sqrt(2.f) / 2 + 1), vmin = (int)std::ceil(H * std::sqrt(2.f) / 2);
    const double hp2 = H * H;
    for (v = 0; v <= vmax; ++v) umax[v] = (int)std::rint(std::sqrt(hp2 - v * v));
    for (v = H, v0 = 0; v >= vmin; --v) {
        while (umax[v0] == umax[v0 + 1]) ++v0;
        umax[v] = v0;
        ++v0;
    }
    c->cor.init = true;
    return 0;
}

int ldso_ct_detect_corners(ldso_ct_ctx *c, int32_t n_features, int32_t host, int32_t capacity,
                           ldso_ct_immature *recs_out, ldso_ct_feature *feat_out, int32_t *n_out,
                           int32_t *stats_out) {
    if (!c) return fail(-1, "null context");
    if (!c->cor.init) return fail(-1, "ldso_ct_corners_init not called");
    if (!c->frame.have) return fail(-1, "ldso_ct_set_new_frame not called");
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
    c->cor.n = -1;
    if (ncells > 0) {
        // every feature slot the grid has (each cell full of candidates), whatever the image holds
        const int n_slots = ncells * G.kk, cap = std::min(capacity, n_slots);
        if ((rc = ct_grow(c, c->cor.d_cell, 2 * (size_t)ncells)) || (rc = ct_grow(c, c->cor.d_slot, n_slots)) ||
            (rc = ct_grow(c, c->cor.d_feat, n_slots)) || (rc = ct_grow(c, c->cor.d_corner, n_slots)) ||
            (rc = ct_grow(c, c->cor.d_out, std::max(1, cap))) || (rc = ct_grow(c, c->d_mk, std::max(1, cap))) ||
            (rc = c->cor.d_cnt.ensure(kCorCnts)) || (rc = c->cor.counts.ensure(kCorCnts)))
            return rc;
        int *cnt = c->cor.d_cnt.p, *cell_cnt = c->cor.d_cell.p, *cell_off = cell_cnt + ncells;
        const int gg = G.g * G.g, nb_slots = ct_blocks(n_slots);
        HIP_TRY(hipMemsetAsync(cnt, 0, kCorCnts * sizeof(int), c->stream));
        k_ct_cor_cell<<<ncells, gg <= kWave ? kWave : kCtThreads, (size_t)gg * (sizeof(unsigned long long) + sizeof(float)),
                        c->stream>>>(c->frame.d_dIp.p, G, cell_cnt, cell_off, c->cor.d_slot.p, cnt);
        k_ct_sel_scan<<<1, kCtThreads, 0, c->stream>>>(cell_off, ncells, 1, cnt + kCorCntFeatures);
        k_ct_cor_emit<<<nb_slots, kCtThreads, 0, c->stream>>>(c->frame.d_dIp.p, G, n_slots, cell_cnt, cell_off, c->cor.d_slot.p,
                                                              cnt, host, c->cor.d_feat.p, c->d_mk.p, cap);
        k_ct_cor_suppress<<<nb_slots, kCtThreads, 0, c->stream>>>(G, cell_cnt, cell_off, c->cor.d_feat.p,
                                                                  c->cor.d_corner.p, cnt);
        k_ct_cor_orb<<<(n_slots + kCorWavesPerBlock - 1) / kCorWavesPerBlock, kCtThreads, 0, c->stream>>>(
            c->frame.d_dIp.p, G.w, G.h, c->cor.d_feat.p, c->cor.d_corner.p, c->cor.d_pattern.p, c->cor.umax, cnt, cap,
            c->cor.d_out.p, c->cor.counts.dev);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipStreamSynchronize(c->stream));  // the counters are in mapped host memory
        const int *hc = c->cor.counts.p;
        stats[2] = hc[kCorCntCandidates];
        stats[3] = hc[kCorCntFeatures];
        stats[4] = hc[kCorCntCorners];
        stats[5] = hc[kCorCntMaxScore];
        *n_out = hc[kCorCntFeatures];
    }
    const int n = *n_out;
    c->cor.n = n <= capacity ? n : -1;  // the device holds a record per feature only when they all fitted
    if (stats_out) std::memcpy(stats_out, stats, sizeof stats);
    if (n > capacity) return fail(-1, "capacity below the number of features (see *n_out)");
    if (n > 0) {
        HIP_TRY(hipMemcpyAsync(recs_out, c->d_mk.p, (size_t)n * sizeof(IpRec), hipMemcpyDeviceToHost, c->stream));
        if ((rc = ct_read(c, feat_out, c->cor.d_out.p, n))) return rc;
    }
    return 0;
}

}  // extern "C"
