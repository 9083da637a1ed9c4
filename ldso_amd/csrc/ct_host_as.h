// ct_host_as.h -- activation candidates: the distance map and activatePointsMT's walk (k_ct_actsel.h).  Owns c->as.
// Reads ip.d_ip; a compacting selection writes ip.d_ip_alt and swaps it with ip.d_ip.
// A piece of the one translation unit ldso_ct.hip (k_ct_pyramid.h).
#pragma once
#include <algorithm>
#include <cmath>
#include <cstring>
#include <string>

#include "../../include/ldso_ba.h"
#include "ldso_ba_internal.h"
#include "ct_context.h"

#pragma clang fp contract(off)

// the BA context's view of the last activation selection (ldso_ba_activate_points_tracker)
int ldso_ba::ct_selection_view(const ldso_ct_ctx *c, ldso_ba::CtSelectionView *out) {
    if (!c || !out) return fail(-1, "null argument");
    out->records = c->as.d_selected.p;
    out->n = c->as.sel_n;
    out->n_hosts = c->as.sel_hosts;
    out->device = c->device;
    out->stream = (void *)c->stream;
    return 0;
}

namespace {

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
    if ((rc = c->as.d_map.ensure(npx)) || (rc = c->as.h_map.ensure(npx)) || (rc = c->as.d_hosts.ensure(n_tab)) ||
        (rc = c->as.h_hosts.ensure(n_tab)))
        return rc;
    HIP_TRY(hipStreamSynchronize(c->stream));  // the staging buffer may still feed a previous copy
    c->as.have_map = false;
    for (int i = 0; i < n_hosts; i++) {
        std::memcpy(c->as.h_hosts.p + 12 * (size_t)i, krki1 + 9 * (size_t)i, 9 * sizeof(float));
        std::memcpy(c->as.h_hosts.p + 12 * (size_t)i + 9, kt1 + 3 * (size_t)i, 3 * sizeof(float));
    }
    HIP_TRY(hipMemcpyAsync(c->as.d_hosts.p, c->as.h_hosts.p, (size_t)n_hosts * 12 * sizeof(float), hipMemcpyHostToDevice,
                           c->stream));
    HIP_TRY(hipMemsetD32Async((hipDeviceptr_t)c->as.d_map.p, kAsFar, npx, c->stream));
    return 0;
}

// growDistBFS over the seeded map, the map to the caller if asked
int as_finish_map(ldso_ct_ctx *c, int n_hosts, float *map_out) {
    const AsGrid G = as_grid(c);
    const size_t npx = (size_t)G.w1 * G.h1;
    k_ct_as_grow<<<dim3((G.w1 + kAsTile - 1) / kAsTile, (G.h1 + kAsTile - 1) / kAsTile), kAsGrowThreads, 0, c->stream>>>(
        c->as.d_map.p, G);
    HIP_TRY(hipGetLastError());
    if (map_out) {
        if (int rc = ct_read(c, c->as.h_map.p, c->as.d_map.p, npx)) return rc;
        for (size_t i = 0; i < npx; i++) map_out[i] = (float)c->as.h_map.p[i];
    }
    c->as.n_hosts = n_hosts;
    c->as.have_map = true;
    return 0;
}

}  // namespace

extern "C" {

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
        if ((rc = c->as.d_uvd.ensure(3 * (size_t)n)) || (rc = c->as.d_seed_host.ensure(n))) return rc;
        HIP_TRY(hipMemcpyAsync(c->as.d_uvd.p, uvd, 3 * (size_t)n * sizeof(float), hipMemcpyHostToDevice, c->stream));
        HIP_TRY(hipMemcpyAsync(c->as.d_seed_host.p, host, (size_t)n * sizeof(int), hipMemcpyHostToDevice, c->stream));
        k_ct_as_seed<<<(n + kCtThreads - 1) / kCtThreads, kCtThreads, 0, c->stream>>>(
            c->as.d_uvd.p, 3, c->as.d_seed_host.p, n, n_hosts, -1, c->as.d_hosts.p, as_grid(c), c->as.d_map.p);
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
    if (V.P > 0) {
        // read the points behind what the BA stream holds now; its later work waits for the read
        hipStream_t bs = static_cast<hipStream_t>(V.stream);
        if ((rc = c->as.borrow.begin(c->stream, bs))) return rc;
        k_ct_as_seed<<<(V.P + kCtThreads - 1) / kCtThreads, kCtThreads, 0, c->stream>>>(
            V.pt_data, LDSO_BA_POINT_STRIDE, V.pt_host, V.P, V.N, newest, c->as.d_hosts.p, as_grid(c), c->as.d_map.p);
        HIP_TRY(hipGetLastError());
        if ((rc = c->as.borrow.end(c->stream, bs))) return rc;
    }
    return as_finish_map(c, V.N, map_out);
}

int ldso_ct_select_activation(ldso_ct_ctx *c, const ldso_ct_actsel_params *params, const uint8_t *flagged,
                              int32_t compact, int32_t *disposition_out, int32_t *selected_idx_out,
                              int32_t *n_selected_out, int32_t *counts_out) {
    if (!c) return fail(-1, "null context");
    if (!c->as.have_map) return fail(-1, "no distance map: call ldso_ct_make_distance_map first");
    const int n_hosts = c->as.n_hosts, n = c->ip.n;
    ldso_ct_actsel_params p = params ? *params : kActselDefaults;
    if (!params || p.newest_host == -2) p.newest_host = n_hosts - 1;
    if (!(p.current_min_act_dist >= 0 && p.current_min_act_dist <= 4))
        return fail(-1, "current_min_act_dist outside [0, 4]");
    if (std::isnan(p.min_trace_quality)) return fail(-1, "min_trace_quality is NaN");
    if (p.newest_host < -1 || p.newest_host >= n_hosts) return fail(-1, "newest_host out of range");
    if (n_hosts <= c->ip.max_host) return fail(-1, "an immature point's host index is >= the distance map's n_hosts");
    HIP_TRY(hipSetDevice(c->device));
    const AsGrid G = as_grid(c);
    const int n_bins = G.bw * G.bh, nb = ct_blocks(n);
    const size_t cap = std::max<size_t>(c->ip.d_ip.n, 1);
    int rc;
    if ((rc = c->as.d_cand.ensure(cap)) || (rc = c->as.d_entry.ensure(cap)) || (rc = c->as.d_disp.ensure(cap)) ||
        (rc = c->as.d_out.ensure(2 * cap)) || (rc = c->as.h_out.ensure(2 * cap)) ||
        (rc = c->as.d_blk.ensure((size_t)(kAsMaxHosts + 1) * ct_blocks((int)cap))) ||
        (rc = c->as.d_tot.ensure(kAsMaxHosts + 1)) || (rc = c->as.d_cnt.ensure(kAsCnts + 2 * (size_t)n_bins + 1)) ||
        (rc = c->as.h_cnt.ensure(kAsCnts)) || (rc = c->as.counts.ensure(kAsCnts)) ||
        (rc = c->as.d_selected.ensure(cap)) || (rc = c->as.d_flag.ensure(kAsMaxHosts)) ||
        (rc = c->as.h_flag.ensure(kAsMaxHosts)) || (compact && (rc = c->ip.d_ip_alt.ensure(cap))))
        return rc;
    HIP_TRY(hipStreamSynchronize(c->stream));  // the staging buffers and the selection may still be read
    c->as.sel_n = -1;
    int32_t counts[4] = {0, 0, 0, 0};
    int max_host = -1;
    if (n > 0) {
        for (int i = 0; i < kAsMaxHosts; i++) c->as.h_flag.p[i] = (flagged && i < n_hosts && flagged[i]) ? 1 : 0;
        HIP_TRY(hipMemcpyAsync(c->as.d_flag.p, c->as.h_flag.p, kAsMaxHosts, hipMemcpyHostToDevice, c->stream));
        // the counters, the bins' counts (then offsets) and the scatter's cursors: one buffer, one memset
        int *cnt = c->as.d_cnt.p, *bin = cnt + kAsCnts, *cursor = bin + n_bins + 1;
        HIP_TRY(hipMemsetAsync(cnt, 0, (kAsCnts + 2 * (size_t)n_bins + 1) * sizeof(int), c->stream));
        AsClassify K{c->ip.d_ip.p, c->as.d_hosts.p, c->as.d_flag.p, c->as.d_map.p, n, n_hosts, p.newest_host,
                     p.current_min_act_dist, p.min_trace_quality, G};
        k_ct_as_classify<<<nb, kCtThreads, 0, c->stream>>>(K, c->as.d_cand.p, c->as.d_disp.p, bin);
        k_ct_sel_scan<<<1, kCtThreads, 0, c->stream>>>(bin, n_bins + 1, 1, cnt + kAsCntLive);
        k_ct_as_scatter<<<nb, kCtThreads, 0, c->stream>>>(c->as.d_cand.p, c->as.d_disp.p, n, G, bin, cursor,
                                                          c->as.d_entry.p);
        // the rounds, a few launches between two looks at the count of the undecided: four at first (a
        // candidate tries kAsAttempts times per launch), then eight at a time.  The corner pixel's candidates
        // get one launch per batch: enough for the earliest undecided candidate to decide in every batch.
        AsRound R{c->as.d_cand.p, c->as.d_entry.p, bin, c->as.d_map.p, c->as.d_disp.p, cnt, G, n_bins, 0};
        for (int batches = 0, batch = 4;; batches++, batch = 8) {
            if (batches > n + 1) return fail(-2, "the activation walk did not end (internal error)");  // each decides one
            if (batches) HIP_TRY(hipMemsetAsync(cnt + kAsCntUndecided, 0, sizeof(int), c->stream));
            for (int k = 0; k < batch; k++) {
                R.count_undecided = k == batch - 1;
                k_ct_as_round<<<nb, kCtThreads, 0, c->stream>>>(R);
                if (k == batch - 1) k_ct_as_round_corner<<<1, kCtThreads, 0, c->stream>>>(R);
            }
            HIP_TRY(hipGetLastError());
            if ((rc = ct_read(c, c->as.h_cnt.p, cnt, kAsCnts))) return rc;
            if (c->as.h_cnt.p[kAsCntUndecided] == 0) break;
        }
        AsOut O{c->ip.d_ip.p, c->as.d_disp.p, c->as.d_blk.p, cnt, n, nb, n_hosts};
        k_ct_as_count<<<nb, kCtThreads, 0, c->stream>>>(O);
        k_ct_sel_scan<<<1, kCtThreads, 0, c->stream>>>(c->as.d_blk.p, nb, n_hosts + 1, c->as.d_tot.p);
        k_ct_as_write<<<nb, kCtThreads, 0, c->stream>>>(O, c->as.d_tot.p, c->as.d_selected.p, c->as.d_out.p + n,
                                                        compact ? c->ip.d_ip_alt.p : nullptr, c->as.d_out.p,
                                                        c->as.counts.dev);
        HIP_TRY(hipGetLastError());
        // (the synchronisation brings the counters too: they are in mapped host memory)
        if ((rc = ct_read(c, c->as.h_out.p, c->as.d_out.p, 2 * (size_t)n))) return rc;
        for (int k = 0; k < 4; k++) counts[k] = c->as.counts.p[k];
        max_host = c->as.counts.p[kAsCntMaxHost] - 1;
        if (disposition_out) std::memcpy(disposition_out, c->as.h_out.p, (size_t)n * sizeof(int));
        if (selected_idx_out) std::memcpy(selected_idx_out, c->as.h_out.p + n, (size_t)counts[2] * sizeof(int));
        if (compact) {
            std::swap(c->ip.d_ip.p, c->ip.d_ip_alt.p);
            std::swap(c->ip.d_ip.n, c->ip.d_ip_alt.n);
            c->ip.n = counts[0];
            c->ip.max_host = max_host;
        }
    }
    c->as.sel_n = counts[2];
    c->as.sel_hosts = n_hosts;
    if (n_selected_out) *n_selected_out = counts[2];
    if (counts_out) std::memcpy(counts_out, counts, sizeof counts);
    return 0;
}

int ldso_ct_selection_download(ldso_ct_ctx *c, int32_t n, ldso_ct_immature *pts) {
    if (!c) return fail(-1, "null context");
    if (c->as.sel_n < 0) return fail(-1, "no selection: call ldso_ct_select_activation first");
    if (n != c->as.sel_n) return fail(-1, "count differs from the selection");
    if (n == 0) return 0;
    if (!pts) return fail(-1, "null output");
    HIP_TRY(hipSetDevice(c->device));
    return ct_read(c, pts, c->as.d_selected.p, n);
}

}  // extern "C"
