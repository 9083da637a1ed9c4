// ct_host_sel.h -- pixel selection: makeMaps and makeNewTraces' walk (k_ct_select.h).  Owns c->sel.  Reads frame.d_dIp;
// ldso_ct_make_new_traces fills the core's d_mk.
// A piece of the one translation unit ldso_ct.hip (k_ct_pyramid.h).
#pragma once
#include <algorithm>
#include <cmath>
#include <cstring>

#include "ct_context.h"

#pragma clang fp contract(off)

namespace {

// ---- pixel selection (k_ct_select.h) ------------------------------------------------------------
constexpr ldso_ct_select_params kSelDefaults = {1500.f, 1, 1.f, 0.5f, 7.f, 0.75f, 1};  // Setting.cc:29, 83-87

int sel_check(const ldso_ct_ctx *c, const ldso_ct_select_params &p) {
    if (!c) return fail(-1, "null context");
    if (c->levels < 3) return fail(-1, "pixel selection reads pyramid levels 0-2: the context has fewer than 3 levels");
    if (!c->sel.potential) return fail(-1, "ldso_ct_select_init not called");
    if (!c->frame.have) return fail(-1, "ldso_ct_set_new_frame not called");
    if (!std::isfinite(p.density) || !(p.density > 0)) return fail(-1, "density must be finite and > 0");
    if (p.recursions < 0) return fail(-1, "recursions must be >= 0");
    return 0;
}

// the work buffers: their sizes follow the image size, so only the first selection allocates
int sel_ensure(ldso_ct_ctx *c) {
    const int w = c->pyr.w, h = c->pyr.h, w32 = w / 32, h32 = h / 32, n = w * h;
    // every index (x >> 5) + (y >> 5) * w32 of a pixel, and the grid makeHists fills
    const size_t n_ths = std::max((size_t)((w - 1) >> 5) + (size_t)((h - 1) >> 5) * w32 + 1, (size_t)w32 * h32);
    if (c->sel.d_ths.p && c->sel.d_map.p) return 0;
    int rc;
    if ((rc = c->sel.d_map.ensure(n)) || (rc = c->sel.h_map.ensure(n)) ||
        (rc = c->sel.d_ths_raw.ensure(std::max(1, w32 * h32))) || (rc = c->sel.d_mask.ensure(n)) ||
        (rc = c->sel.d_n2.ensure(n)) || (rc = c->sel.d_nu.ensure(n)) ||
        (rc = c->sel.d_blk.ensure(2 * (size_t)ct_blocks(n))) || (rc = c->sel.d_cnt.ensure(kSelCnts)) ||
        (rc = c->sel.h_cnt.ensure(kSelCnts)) || (rc = c->sel.d_ths.ensure(n_ths)))
        return rc;
    HIP_TRY(hipMemsetAsync(c->sel.d_ths.p, 0, n_ths * sizeof(float), c->stream));  // the entries makeHists never writes
    return 0;
}

// one select(fh, map_out, pot, thFactor): the map on the device, n = (n2, n3, n4) behind one wait
int sel_pass(ldso_ct_ctx *c, const ldso_ct_select_params &p, int pot, int n[3]) {
    const PyrParams &P = c->pyr;
    SelParams S;
    S.dI0 = c->frame.d_dIp.p;
    S.dI1 = c->frame.d_dIp.p + P.off[1];
    S.dI2 = c->frame.d_dIp.p + P.off[2];
    S.ths = c->sel.d_ths.p;
    S.pattern = c->sel.d_pattern.p;
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
    const int nc = S.ncx * S.ncy, nb = ct_blocks(nc);
    const dim3 grid4((S.ncx + 3) / 4, (S.ncy + 3) / 4);
    const int threads = 16 * S.pot * S.pot <= kCtThreads ? kWave : kCtThreads;
    int *cnt = c->sel.d_cnt.p, *blk = c->sel.d_blk.p;
    HIP_TRY(hipMemsetAsync(c->sel.d_map.p, 0, (size_t)P.w * P.h, c->stream));
    HIP_TRY(hipMemsetAsync(cnt, 0, kSelCnts * sizeof(int), c->stream));
    k_ct_sel_block<false><<<grid4, threads, 0, c->stream>>>(S, c->sel.d_mask.p, nullptr, nullptr, nullptr);
    for (int round = 0; round < 2; round++) {
        k_ct_sel_cell_count<<<nb, kCtThreads, 0, c->stream>>>(c->sel.d_mask.p, nc, nb, blk);
        k_ct_sel_scan<<<1, kCtThreads, 0, c->stream>>>(blk, nb, 2, cnt + kSelCntN2);  // [N2], [NonUniform]
        k_ct_sel_cell_apply<<<nb, kCtThreads, 0, c->stream>>>(c->sel.d_mask.p, nc, nb, blk, c->sel.d_n2.p, c->sel.d_nu.p);
        if (round == 0)
            k_ct_sel_fixup<<<1, kWave, 0, c->stream>>>(c->sel.d_nu.p, cnt, c->sel.d_n2.p, c->sel.d_mask.p,
                                                       c->sel.d_pattern.p, P.w * P.h);
    }
    k_ct_sel_block<true><<<grid4, threads, 0, c->stream>>>(S, nullptr, c->sel.d_n2.p, c->sel.d_map.p, cnt);
    HIP_TRY(hipGetLastError());
    if (int rc = ct_read(c, c->sel.h_cnt.p, cnt, kSelCnts)) return rc;
    n[0] = c->sel.h_cnt.p[kSelCntN2];
    n[1] = c->sel.h_cnt.p[kSelCntN3];
    n[2] = c->sel.h_cnt.p[kSelCntN4];
    return 0;
}

// PixelSelector::makeMaps (PixelSelector2.cc:111-169), the recursion as a loop.  Leaves the map on the
// device, the sub-selection (if any) enqueued: *sub tells the caller to take stats[0] from
// sel.h_cnt[kSelCntKept] after its synchronisation.  The context's potential is set.
int sel_make_maps(ldso_ct_ctx *c, const ldso_ct_select_params &p, int32_t stats[LDSO_CT_SELECT_STATS], bool *sub) {
    const PyrParams &P = c->pyr;
    int rc = sel_ensure(c);
    if (rc) return rc;
    const int w32 = P.w / 32, h32 = P.h / 32;
    if (w32 > 0 && h32 > 0) {  // makeHists
        k_ct_sel_hist<<<dim3(w32, h32), kCtThreads, 0, c->stream>>>(c->frame.d_dIp.p, P.w, P.h, w32, p.min_grad_hist_cut,
                                                                   p.min_grad_hist_add, c->sel.d_ths_raw.p);
        k_ct_sel_smooth<<<ct_blocks(w32 * h32), kCtThreads, 0, c->stream>>>(c->sel.d_ths_raw.p, w32, h32, c->sel.d_ths.p);
    }
    int recursionsLeft = p.recursions, currentPotential = c->sel.potential, idealPotential, n[3], passes = 0;
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
        const int npx = P.w * P.h, nb = ct_blocks(npx);
        const unsigned char charTH = 255 * quotia;
        k_ct_sel_px_count<<<nb, kCtThreads, 0, c->stream>>>(c->sel.d_map.p, npx, c->sel.d_blk.p);
        k_ct_sel_scan<<<1, kCtThreads, 0, c->stream>>>(c->sel.d_blk.p, nb, 1, c->sel.d_cnt.p + kSelCntScratch);
        k_ct_sel_sub<<<nb, kCtThreads, 0, c->stream>>>(c->sel.d_map.p, npx, c->sel.d_blk.p, c->sel.d_pattern.p, charTH,
                                                       c->sel.d_cnt.p);
        HIP_TRY(hipGetLastError());
    }
    stats[0] = (int)numHave;
    stats[1] = n[0];
    stats[2] = n[1];
    stats[3] = n[2];
    stats[4] = currentPotential;
    stats[5] = idealPotential;
    stats[6] = passes;
    c->sel.potential = idealPotential;
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
    if (int rc = ct_grow(c, c->sel.d_pattern, n)) return rc;
    HIP_TRY(hipMemcpyAsync(c->sel.d_pattern.p, random_pattern, n, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));  // the caller's pattern may be reused on return
    c->sel.potential = potential;
    return 0;
}

int ldso_ct_select_potential(ldso_ct_ctx *c, int32_t *out) {
    if (!c || !out) return fail(-1, "null argument");
    if (!c->sel.potential) return fail(-1, "ldso_ct_select_init not called");
    *out = c->sel.potential;
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
    if (map_out) HIP_TRY(hipMemcpyAsync(c->sel.h_map.p, c->sel.d_map.p, n, hipMemcpyDeviceToHost, c->stream));
    if (sub)
        HIP_TRY(hipMemcpyAsync(c->sel.h_cnt.p, c->sel.d_cnt.p, kSelCnts * sizeof(int), hipMemcpyDeviceToHost, c->stream));
    if (map_out || sub) HIP_TRY(hipStreamSynchronize(c->stream));
    if (sub) stats[0] = c->sel.h_cnt.p[kSelCntKept];
    if (map_out)
        for (size_t i = 0; i < n; i++) map_out[i] = c->sel.h_map.p[i];
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
    const int potential_before = c->sel.potential;
    if ((rc = sel_make_maps(c, p, stats, &sub))) return rc;
    // the walk: survivors counted per block, the counts scanned, the records written in order
    const int w = c->pyr.w, h = c->pyr.h, npx = w * h, nb = ct_blocks(npx);
    const int cap = std::min(capacity, stats[1] + stats[2] + stats[3]);  // no more than select picked
    if ((rc = ct_grow(c, c->d_mk, std::max(1, cap)))) return rc;
    int *cnt = c->sel.d_cnt.p;
    k_ct_sel_emit<false><<<nb, kCtThreads, 0, c->stream>>>(c->frame.d_dIp.p, w, h, c->sel.d_map.p, host, c->sel.d_blk.p, nullptr, 0);
    k_ct_sel_scan<<<1, kCtThreads, 0, c->stream>>>(c->sel.d_blk.p, nb, 1, cnt + kSelCntEmit);
    k_ct_sel_emit<true><<<nb, kCtThreads, 0, c->stream>>>(c->frame.d_dIp.p, w, h, c->sel.d_map.p, host, c->sel.d_blk.p,
                                                         c->d_mk.p, cap);
    HIP_TRY(hipGetLastError());
    if ((rc = ct_read(c, c->sel.h_cnt.p, cnt, kSelCnts))) return rc;
    if (sub) stats[0] = c->sel.h_cnt.p[kSelCntKept];
    const int n = c->sel.h_cnt.p[kSelCntEmit];
    *n_out = n;
    if (stats_out) std::memcpy(stats_out, stats, sizeof stats);
    if (n > capacity) {
        c->sel.potential = potential_before;
        return fail(-1, "capacity below the number of new immature points (see *n_out)");
    }
    return n > 0 ? ct_read(c, out, c->d_mk.p, n) : 0;
}

}  // extern "C"
