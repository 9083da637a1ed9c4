// ba_launch.h -- the host side's helpers over the context: staged uploads, timed launches, image
// staging, priors, the kernels' parameter fillers and the launches more than one entry point shares.
#pragma once
#include <hip/hip_ext.h>

#include <algorithm>
#include <cstring>

#include "ba_context.h"
#include "k_linearize.h"
#include "k_point_sc.h"
#include "k_stitch.h"
#include "k_stitch_host.h"
#include "k_solve.h"
#include "k_xad.h"
#include "k_resubstitute.h"
#include "k_io.h"
#include "se3.h"

namespace {

// LinParams::aff_fix of the context's settings: which of JabF[0] / JabF[1] linearize zeroes
inline int aff_fix_bits(const ldso_ba_ctx *c) {
    return (c->settings.affine_opt_mode_a < 0 ? 1 : 0) | (c->settings.affine_opt_mode_b < 0 ? 2 : 0);
}

// the results buffer the device writes directly, so a call's results come back in one launch
// instead of one blit per array; a launch of an earlier call may still be writing the old one
int pin_map_ensure(ldso_ba_ctx *c, size_t bytes) {
    if (c->pin_map.p && c->pin_map.n < bytes) HIP_TRY(hipStreamSynchronize(c->stream));
    return c->pin_map.ensure(bytes);
}

// one more array (whole 4-byte words) for k_pack_out to copy
inline void pack_seg(PackOut &K, const void *src, void *dst, size_t bytes) {
    K.src[K.n_seg] = static_cast<const unsigned *>(src);
    K.dst[K.n_seg] = static_cast<unsigned *>(dst);
    K.words[K.n_seg++] = (int)(bytes / 4);
}

// Small host -> device uploads of one call gathered into the mapped staging buffer and written
// by ONE k_pack_out launch (pageable hipMemcpyAsync costs ~10 us of host time per array)
struct InBatch {
    struct Item {
        void *dst;
        const void *src;
        size_t bytes;
    };
    std::vector<Item> items;
    void add(void *dst, const void *src, size_t bytes) {
        if (bytes) items.push_back({dst, src, bytes});
    }
    int flush(ldso_ba_ctx *c);
};
int InBatch::flush(ldso_ba_ctx *c) {
    if (items.empty()) return 0;
    size_t total = 0;
    for (const Item &it : items) total += (it.bytes + 15) & ~(size_t)15;
    if (c->pin_in_busy) {  // the previous launch must have read the staging buffer
        HIP_TRY(hipEventSynchronize(c->pin_in_ev.e));
        c->pin_in_busy = false;
    }
    int rc = c->pin_in.ensure(total, 4096);
    if (rc || (rc = c->pin_in_ev.ensure(hipEventDisableTiming))) return rc;
    size_t off = 0;
    PackOut K{};
    for (size_t k = 0; k < items.size(); k++) {
        const Item &it = items[k];
        std::memcpy(c->pin_in.p + off, it.src, it.bytes);
        pack_seg(K, c->pin_in.dev + off, it.dst, it.bytes);
        off += (it.bytes + 15) & ~(size_t)15;
        if (K.n_seg == kPackSegs || k + 1 == items.size()) {
            k_pack_out<<<std::min(64, (int)(total / 1024) + 1), 256, 0, c->stream>>>(K);
            HIP_TRY(hipGetLastError());
            K = PackOut{};
        }
    }
    HIP_TRY(hipEventRecord(c->pin_in_ev.e, c->stream));
    c->pin_in_busy = true;
    items.clear();
    return 0;
}

// One launch into kernel-timing slot `slot` (KernelTimer::launch), timed when timing is on and the
// slot is in timing_mask.
template <typename F>
int timed_launch_events(ldso_ba_ctx *c, int slot, hipStream_t record_on, F &&launch) {
    return c->timer.launch(slot, c->timer.on && ((c->timing_mask >> slot) & 1u), record_on, launch);
}
// timed_launch for a launch that takes the events itself (hipExtLaunchKernelGGL's start / stop
// events, stamped by the dispatch): the stream carries no event packets around the kernel, which
// on this path cost ~5 us of idle GPU on each side of it
template <typename F>
int timed_launch_ext(ldso_ba_ctx *c, int slot, F &&launch) {
    return timed_launch_events(c, slot, nullptr, launch);
}
template <typename F>
int timed_launch(ldso_ba_ctx *c, int slot, hipStream_t st, F &&launch) {
    return timed_launch_events(c, slot, st, [&](hipEvent_t, hipEvent_t) { launch(); });
}

// One staged float3 frame repacked into a slot of layout l (of the window's image array or of the
// frame store).  Layout 3 keeps the intensities and raises *flag if the frame's gradients are not
// the ones it will recompute.
void launch_repack(const ImageLayout &l, const float *stage, float4 *dst, int *flag, hipStream_t st) {
    const int nb = (int)((l.repack_elems() + 255) / 256);
    if (l.mode == 3)
        k_intensity_image<<<nb, 256, 0, st>>>(stage, reinterpret_cast<float *>(dst), l.width, l.height, l.tiles_per_row,
                                              l.padded_h, flag);
    else
        k_tile_image<<<nb, 256, 0, st>>>(stage, dst, l.width, l.height, l.tiles_per_row, l.padded_h);
}

// the context's device staging of one float3 frame and the gradient-mismatch flag (grow-only)
int image_staging(ldso_ba_ctx *c, size_t npix) {
    if (c->d_img_stage.n < npix * 3 || !c->d_img_stage.p) {
        int rc = c->d_img_stage.alloc(npix * 3);
        if (rc) return rc;
        c->xfer[2]++;
    }
    return c->d_img_flag.ensure(1);
}

int stage_images(ldso_ba_ctx *c, const ldso_ba_window *ws, int n_windows, int *mismatch) {
    const size_t npix = c->img.npix();
    int rc = image_staging(c, npix);
    if (rc) return rc;
    float *stage = c->d_img_stage.p;
    int *flag = c->d_img_flag.p;
    hipError_t e = hipMemsetAsync(flag, 0, sizeof(int), c->stream);
    int fb = 0;
    for (int w = 0; w < n_windows && e == hipSuccess; w++)
        for (int f = 0; f < ws[w].n_frames && e == hipSuccess; f++, fb++) {
            e = hipMemcpyAsync(stage, ws[w].dI + (size_t)f * npix * 3, npix * 3 * sizeof(float), hipMemcpyHostToDevice,
                               c->stream);
            if (e != hipSuccess) break;
            c->xfer[0] += (int64_t)(npix * 3 * sizeof(float));
            c->xfer[3]++;
            launch_repack(c->img, stage, c->d_img.p + (size_t)fb * c->img.frame_stride, flag, c->stream);
            e = hipGetLastError();
        }
    if (e == hipSuccess) e = hipMemcpyAsync(mismatch, flag, sizeof(int), hipMemcpyDeviceToHost, c->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    if (e != hipSuccess) return fail(-2, std::string("image staging: ") + hipGetErrorString(e));
    return 0;
}

// HL diagonal and bL of one window (the priors accumulateLF_MT stitches, AccumulatedTopHessian.cc:
// 241-250) as the device solver reads them; zero on ranks other than 0 of a sharded window
void priors_vector(const ldso_ba_ctx *c, int win, std::vector<double> &pr) {
    const WinHost &H = c->wh[win];
    const WinDev &D = c->wd[win];
    pr.assign((size_t)2 * D.D, 0.0);
    if (H.add_priors) {
        for (int i = 0; i < 4; i++) {
            pr[2 * i] = H.c_prior[i];
            pr[2 * i + 1] = H.c_prior[i] * (double)H.c_delta[i];
        }
        for (int f = 0; f < H.N; f++)
            for (int i = 0; i < 8; i++) {
                const int q = 4 + 8 * f + i;
                pr[2 * q] = H.frame_prior[8 * f + i];
                pr[2 * q + 1] = H.frame_prior[8 * f + i] * H.frame_delta_prior[8 * f + i];
            }
    }
}
int upload_priors(ldso_ba_ctx *c, int win) {
    std::vector<double> pr;
    priors_vector(c, win, pr);
    HIP_TRY(hipMemcpyAsync(c->d_prior.p + (size_t)2 * c->wd[win].vec_base, pr.data(), pr.size() * sizeof(double),
                           hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return 0;
}

// where ldso_ba_optimize computes the step's sumNID: in extra blocks of k_solve_fast, beside the
// factorisation; with an exact solve mode in leading blocks of the pass's k_point_sc, or, with a
// communicator, in extra blocks of the exchange's k_frame_th
inline bool nid_in_solve(const ldso_ba_ctx *c, const Switches &sw) { return !c->solve_exact && !sw.solve_lds; }
// the idepths the sumNID chain walks: the context's points, or with a communicator every rank's
// run of the window from the last exchange's all-gather (the runs concatenated in rank order are
// the unsharded host-frame order, so the chain is the single-GPU one bit for bit)
NidSrc nid_source(const ldso_ba_ctx *c) {
    NidSrc n{};
    n.pt_data = c->d_pt_data.p;
    if (c->comm) {
        n.gathered = c->d_x_gathered.p;
        n.slot = c->x_stride + c->x_prun;
        n.off = c->x_stride;
        n.n_ranks = c->comm_world;
        n.n_win = c->n_win;
        n.prun = (int)c->x_prun;
    }
    return n;
}
// k_linearize over every top item on the context's own residual state and records, outside any
// optimize() loop (pass 0, no loop exits), fix and accumulate off: the callers set what differs
LinParams lin_params(const ldso_ba_ctx *c) {
    LinParams L{};
    L.items = c->d_top_items.p;
    L.wins = c->d_wins.p;
    L.img = c->images();
    L.ad_ht_delta = c->marg ? c->d_adhtd.p : nullptr;
    L.precalc = c->d_precalc.p;
    L.frame_th = c->d_frame_th.p;
    L.rs_slot = c->d_rs_slot.p;
    L.pt_data = c->d_pt_data.p;
    L.rs_state = c->d_rs_state.p;
    L.rs_newstate = c->d_rs_newstate.p;
    L.rs_flags = c->d_rs_flags.p;
    L.rs_energy = c->d_rs_energy.p;
    L.rs_newenergy = c->d_rs_newenergy.p;
    L.rs_energy_wo = c->d_rs_energy_wo.p;
    L.rs_center = reinterpret_cast<float *>(c->d_rs_center.p);
    L.center_stride = c->R_tot;
    L.rec_a = c->d_rec_a.p;
    L.rec_b = c->d_rec_b.p;
    L.geo_snap = c->d_geo_snap.p;
    L.top_slab = c->d_top_slab.p;
    L.item_energy = c->d_item_energy.p;
    L.frame_stride = c->img.frame_stride;
    L.tiles_per_row = c->img.tiles_per_row;
    L.aff_fix = aff_fix_bits(c);
    L.item_base = 0;
    L.n_items = c->n_top_items;
    L.n_blocks = (L.n_items + 3) / 4;
    return L;
}
// k_point_sc over every sc item (no sumNID blocks, no loop exits)
PointParams point_params(const ldso_ba_ctx *c) {
    PointParams Pp{};
    Pp.items = c->d_sc_items.p;
    Pp.wins = c->d_wins.p;
    Pp.pt_data = c->d_pt_data.p;
    Pp.pt_nres = c->d_pt_nres.p;
    Pp.pt_tgt = c->d_pt_tgt.p;
    Pp.rec_a = c->d_rec_a.p;
    Pp.rec_b = c->d_rec_b.p;
    Pp.precalc = c->d_precalc.p;
    Pp.pt_out = c->d_pt_out.p;
    Pp.sc_slab = c->d_sc_slab.p;
    Pp.shift_prior = c->marg ? 0 : 1;
    Pp.item_base = 0;
    Pp.n_items = c->n_sc_items;
    return Pp;
}
// either stitch over every window; the caller sets accumulate, the loop fields, hs_split and th_cap
StitchParams stitch_params(const ldso_ba_ctx *c) {
    StitchParams Sp{};
    Sp.wins = c->d_wins.p;
    Sp.pair_win = c->d_pair_win.p;
    Sp.e_wo = c->d_rs_energy_wo.p;
    Sp.frame_th = c->d_frame_th.p;
    Sp.pair_items = c->d_pair_items.p;
    Sp.top_slab = c->d_top_slab.p;
    Sp.item_energy = c->d_item_energy.p;
    Sp.host_items = c->d_host_items.p;
    Sp.sc_slab = c->d_sc_slab.p;
    Sp.adH = c->d_adH.p;
    Sp.adT = c->d_adT.p;
    Sp.sys = c->d_sys.p;
    Sp.stage = c->d_stage.p;
    Sp.win_energy = c->win_energy();
    Sp.pair_base = 0;
    Sp.win_base = 0;
    Sp.n_win = c->n_win;
    Sp.frame_win = c->d_frame_win.p;
    Sp.frame_base = 0;
    return Sp;
}
// a per-point value of every window from device order into the caller's: windows back to back,
// each in its caller point order
void scatter_points(const ldso_ba_ctx *c, const float *dev_order, float *out) {
    long long out_base = 0;
    for (int w = 0; w < c->n_win; w++) {
        const WinDev &D = c->wd[w];
        const WinHost &H = c->wh[w];
        for (int q = 0; q < D.P; q++) out[out_base + H.pt_orig[q]] = dev_order[D.point_base + q];
        out_base += H.P_all;
    }
}
ResubParams resub_params(ldso_ba_ctx *c, int begin, int count, double lambda, bool apply_step) {
    ResubParams R{};
    R.pt_data = apply_step ? c->d_pt_data.p : nullptr;
    R.xad = c->d_xad.p;
    R.wins = c->d_wins.p;
    R.pt_win = c->d_pt_win.p;
    R.pt_nres = c->d_pt_nres.p;
    R.pt_tgt = c->d_pt_tgt.p;
    R.rec_a = c->d_rec_a.p;
    R.rec_b = c->d_rec_b.p;
    R.geo_snap = c->d_geo_snap.p;
    R.pt_geo = c->d_pt_data.p;
    R.pt_out = c->d_pt_out.p;
    R.pt_host = c->d_pt_host.p;
    R.pt_step = c->d_pt_step.p;
    R.begin = begin;
    R.count = count;
    R.lambda = (float)lambda;
    return R;
}
int launch_resubstitute(ldso_ba_ctx *c, int begin, int count, double lambda, bool apply_step = false) {
    const ResubParams R = resub_params(c, begin, count, lambda, apply_step);
    return timed_launch(c, kSlotResubstitute, c->stream,
                        [&] { k_resubstitute<<<(count + 255) / 256, 256, 0, c->stream>>>(R); });
}
// k_stitch dynamic LDS: max of the Top phase, the SC phase of the largest window, and the
// frame-threshold staging (at least 1024 candidates; more if the SC phase leaves room)
size_t stitch_smem_bytes(int KP, int N, int *th_cap) {
    const size_t top = (96 + 169 + 4 * 64) * sizeof(double);
    const size_t sc = (size_t)(kStTopLds + 8 * KP + 4 * (N - 1) * 64 + 20) * sizeof(double);
    const size_t th_fixed = th_fixed_bytes(kStThreads);
    size_t bytes = std::max(top, sc);
    bytes = std::max(bytes, th_fixed + 1024 * sizeof(unsigned));
    bytes = (bytes + 15) & ~(size_t)15;
    *th_cap = (int)((bytes - th_fixed) / sizeof(unsigned)) & ~3;
    return bytes;
}

// k_stitch_host dynamic LDS: the host block's staging for the largest window, at least the
// frame-threshold staging of 1024 candidates (more if the host phase leaves room).  Always the dense
// path's size, the larger: which path a block takes is read on the device (WinDev::adt_diag), after
// the launch -- and its LDS size -- may have been captured in a graph
size_t stitch_host_smem_bytes(int N, int *th_cap) {
    const size_t th_fixed = th_fixed_bytes(kHsThreads);
    const size_t host = std::max(hs_lds_doubles(N, false), hs_lds_doubles(N, true)) * sizeof(double);
    size_t bytes = std::max(host, th_fixed + 1024 * sizeof(unsigned));
    bytes = (bytes + 15) & ~(size_t)15;
    *th_cap = (int)((bytes - th_fixed) / sizeof(unsigned)) & ~3;
    return bytes;
}

}  // namespace
