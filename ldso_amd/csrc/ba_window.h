// ba_window.h -- a laid-out window onto the device.  window_buffers is the one table of the device
// buffers a Layout sizes; ldso_ba_load* (load_impl: every buffer allocated anew and uploaded) and
// ldso_ba_edit_window (edit_impl: grown where too small, the carried arrays gathered on the device)
// each walk it once, so that an edited context is a fresh load of the same window by construction.
// ldso_ba_load_marginalization_device is load_impl's walk with the carried arrays sized instead of
// uploaded and k_edit_gather pointed at the parent's arrays (marg_gather).
#pragma once
#include <algorithm>
#include <chrono>
#include <cstring>
#include <string>
#include <vector>

#include "ba_launch.h"
#include "edit_plan.h"
#include "k_edit.h"
#include "layout.h"
#include "marg_plan.h"

namespace {

inline size_t pad4(size_t n) { return (n + 3) & ~(size_t)3; }

// Every device buffer a laid-out window sizes, each named once: its element count -- from the Layout
// alone, for nw windows -- and where its content comes from.  A new buffer of the pass is added
// here and nowhere else.  The visitor (WindowWalk) is told
//   host(buf, v, count)       the Layout's array v, uploaded as is
//   carried(buf, other, v)    state a window keeps across an edit: a load uploads v; an edit sizes
//                             the other half of the double buffer, which k_edit_gather writes
//   fill(buf, count, word)    every 32-bit word of the count elements is `word`
//   res_newstate(buf, count)  every byte is LDSO_BA_RES_OUTLIER (state_NewState before a pass)
//   sized(buf, count)         no initial content: written before it is read
// Not in the table, because the two paths really differ there: d_img and d_adhtd, the edit's own
// staging (d_ed_*_src, d_ed_n*) and the content of d_prior.
template <typename V>
void window_buffers(ldso_ba_ctx *c, Layout &L, size_t nw, V &v) {
    const size_t P = L.pt_host.size(), R = L.rs_slot.size(), np = L.pair_win.size(), vt = (size_t)L.vec_total;
    const size_t n_top = L.top_items.size(), n_rec = (size_t)L.rec_base;
    auto host = [&v](auto &buf, auto &arr) { v.host(buf, arr, arr.size()); };
    host(c->d_wins, L.wd);
    host(c->d_precalc, L.precalc);
    host(c->d_frame_th, L.frame_th);
    v.carried(c->d_pt_data, c->d_ed_pt, L.pt_data);
    v.fill(c->d_pt_out, P * 12, 0u);
    v.fill(c->d_pt_step, P, 0u);
    host(c->d_pt_host, L.pt_host);
    host(c->d_adH, L.adH);
    host(c->d_adT, L.adT);
    host(c->d_pt_nres, L.pt_nres);
    host(c->d_rs_slot, L.rs_slot);
    host(c->d_pt_tgt, L.pt_tgt);
    host(c->d_pair_win, L.pair_win);
    host(c->d_frame_win, L.frame_win);
    v.host(c->d_rs_tgt, L.rs_tgt, pad4(R));  // whole words: k_pack_out copies words
    v.carried(c->d_rs_flags, c->d_ed_flags, L.rs_flags);
    v.carried(c->d_rs_state, c->d_ed_state, L.rs_state);
    v.res_newstate(c->d_rs_newstate, R);
    v.carried(c->d_rs_energy, c->d_ed_energy, L.rs_energy);
    v.carried(c->d_rs_newenergy, c->d_ed_newenergy, L.rs_energy);  // state_NewEnergy is loaded equal to state_energy
    v.fill(c->d_rs_energy_wo, R, 0xBF800000u);                    // -1.0f: nothing evaluated yet
    v.fill(c->d_rs_center, R, 0u);
    v.fill(c->d_rec_a, n_rec, 0u);
    v.fill(c->d_rec_b, n_rec, 0xFFFFFFFFu);  // NaN: not active
    v.fill(c->d_geo_snap, np * kGeoSnap, 0u);
    host(c->d_top_items, L.top_items);
    host(c->d_sc_items, L.sc_items);
    host(c->d_pair_items, L.pair_items);
    host(c->d_host_items, L.host_items);
    v.sized(c->d_top_slab, n_top * kTopVals);
    v.sized(c->d_sc_slab, (size_t)L.sc_slab_total);
    v.sized(c->d_item_energy, n_top * 2);
    v.fill(c->d_sys, (size_t)L.sys_total + 4 * nw, 0u);  // + win_energy() + win_nid()
    v.sized(c->d_stage, (size_t)L.stage_total);
    host(c->d_sum_blocks, L.sum_blocks);
    v.sized(c->d_xad, nw * kXadStride);
    v.sized(c->d_prior, 2 * vt);
    v.sized(c->d_x, vt);
    v.sized(c->d_ns, 7 * vt);
    v.sized(c->d_ns_nm, 7 * vt);
    v.sized(c->d_ns_g, (size_t)kPrepGStride * nw);
    host(c->d_pt_win, L.pt_win);
}

// ldso_ba_edit_window: a buffer that is too small grows to half again its size, so that a cycle
// whose counts wander (7 -> 6 -> 7 keyframes) stops allocating after its first round.
template <typename T>
int edit_grow(ldso_ba_ctx *c, GraphBuf<T> &b, size_t need) {
    need = std::max<size_t>(need, 1);
    if (b.p && b.n >= need) return 0;
    c->xfer[2]++;  // ldso_ba_transfer_stats counts the edit's growths with the image allocations
    return b.alloc(std::max(need, b.n + b.n / 2));
}
template <typename T>
void swap_halves(GraphBuf<T> &a, GraphBuf<T> &b) {
    std::swap(a.p, b.p);
    std::swap(a.n, b.n);
}

// One walk of the table.  A load (kEdit false) frees every buffer and allocates it at its count,
// never fewer than one element, so every pointer is valid (not counted by ldso_ba_transfer_stats);
// an edit grows a buffer only where it is too small.  Both paths record the same uploads and the
// same fills -- the fills in the form k_edit_gather takes them -- and apply them their own way once
// the walk is over.  The first failure ends the walk: later calls do nothing and rc keeps its code
// (an edit has changed nothing of the loaded window by then).
template <bool kEdit>
struct WindowWalk {
    ldso_ba_ctx *c;
    int rc = 0;
    InBatch ups;     // the host arrays: a load copies each on the stream, an edit flushes the batch
    EditParams E{};  // fill_*, and state_NewState as newstate [R]
    // a load whose carried arrays are gathered on the device (ldso_ba_load_marginalization_device):
    // they are sized and not uploaded
    bool gather_carried = false;
    template <typename T>
    void sized(GraphBuf<T> &buf, size_t count) {
        if (!rc) rc = kEdit ? edit_grow(c, buf, count) : buf.alloc(std::max<size_t>(1, count));
    }
    template <typename T, typename V>
    void host(GraphBuf<T> &buf, std::vector<V> &v, size_t count) {
        static_assert(sizeof(T) == sizeof(V), "uploaded as is");
        sized(buf, count);
        v.resize(count);  // d_rs_tgt: its staged copy is whole words too
        if (!rc) ups.add(buf.p, v.data(), count * sizeof(V));
    }
    template <typename T, typename V>
    void carried(GraphBuf<T> &buf, GraphBuf<T> &other, std::vector<V> &v) {
        if (kEdit) sized(other, v.size());
        else if (gather_carried) sized(buf, v.size());
        else host(buf, v, v.size());
    }
    // a fill covers the count and not the allocation: they differ by the one dummy element of an
    // empty buffer, which nothing reads
    template <typename T>
    void fill(GraphBuf<T> &buf, size_t count, unsigned word) {
        static_assert(sizeof(T) % 4 == 0, "filled by words");
        sized(buf, count);
        if (!rc && E.n_fill == kEditFills) rc = fail(-1, "the buffer table has more fills than kEditFills");
        if (rc) return;
        E.fill_dst[E.n_fill] = reinterpret_cast<unsigned *>(buf.p);
        E.fill_words[E.n_fill] = (long long)(count * (sizeof(T) / 4));
        E.fill_val[E.n_fill++] = word;
    }
    void res_newstate(GraphBuf<int8_t> &buf, size_t count) {  // an edit: k_edit_gather's residual loop
        sized(buf, count);
        E.newstate = buf.p;
        E.R = (int)count;
    }
};
// what a load's walk recorded, once every buffer is allocated: the uploads and the fills on the
// context stream, behind one synchronisation
int load_apply(ldso_ba_ctx *c, const WindowWalk<false> &A) {
    if (A.rc) return A.rc;
    const EditParams &F = A.E;
    for (const InBatch::Item &u : A.ups.items)
        HIP_TRY(hipMemcpyAsync(u.dst, u.src, u.bytes, hipMemcpyHostToDevice, c->stream));
    for (int f = 0; f < F.n_fill; f++)
        if (F.fill_words[f])
            HIP_TRY(hipMemsetD32Async((hipDeviceptr_t)F.fill_dst[f], (int)F.fill_val[f], (size_t)F.fill_words[f], c->stream));
    if (F.R) HIP_TRY(hipMemsetAsync(F.newstate, LDSO_BA_RES_OUTLIER, (size_t)F.R, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return 0;
}

// The host-side fields a layout fixes: the windows' descriptors and orders, the counts the launches
// are sized by, and the cached host copies and pass results it makes stale.
void adopt_layout(ldso_ba_ctx *c, Layout &L, int n_windows) {
    c->sys_host_valid = c->energy_valid = c->th_host_valid = c->pass_since_load = false;
    c->x_stride = c->x_prun = 0;
    c->wh = std::move(L.wh);
    c->wd.assign(n_windows, WinDev());
    // WinDev is WinDesc under the name the kernels' symbols carry (see WinDev): keep both, copy across
    c->kp_max = 0;
    for (int w = 0; w < n_windows; w++) {
        static_cast<WinDesc &>(c->wd[w]) = L.wd[w];
        c->kp_max = std::max(c->kp_max, L.wd[w].KP);
    }
    c->n_top_items = (int)L.top_items.size();
    c->n_sc_items = (int)L.sc_items.size();
    c->n_pairs = (int)L.pair_win.size();
    c->n_frames = (int)L.frame_win.size();
    c->max_frames = L.max_frames;
    c->host_stitch = c->max_frames <= kHostStitchMaxN && !read_switches().stitch_records;
    c->P_tot = (int)L.pt_host.size();
    c->vec_total = L.vec_total;
    c->R_tot = (int)L.rs_slot.size();
    c->sc_smem_max = L.smem_max;
    c->sys_n = (size_t)L.sys_total;
    c->n_sum_blocks = (int)L.sum_blocks.size();
    c->ns_cache.clear();
    c->ns_cache_null = -1;
    c->flag_map_win = -1;
}

// k_point_sc's dynamic LDS where the widest loaded window needs more than the default limit
int point_sc_lds_limit(ldso_ba_ctx *c) {
    if (c->sc_smem_max > 64 * 1024)
        HIP_TRY(hipFuncSetAttribute((const void *)k_point_sc, hipFuncAttributeMaxDynamicSharedMemorySize, (int)c->sc_smem_max));
    return 0;
}

// The store slot of every frame of the windows, named by frame_ids ([sum N], window after window):
// every frame must be resident before anything of the loaded state changes
int store_slots(const FrameStore &S, const ldso_ba_window *ws, int n_windows, const int64_t *frame_ids, std::vector<int> &fslot) {
    size_t k = 0;
    for (int w = 0; w < n_windows; w++) {
        if (ws[w].width != S.lay.width || ws[w].height != S.lay.height)
            return fail(LDSO_BA_ERR_FRAME_STORE, "window size differs from the frame store's");
        for (int f = 0; f < ws[w].n_frames; f++, k++) {
            const int s = S.find(frame_ids[k]);
            if (s < 0)
                return fail(LDSO_BA_ERR_FRAME_STORE,
                            "frame id " + std::to_string((long long)frame_ids[k]) + " is not resident in the frame store");
            fslot.push_back(s);
        }
    }
    return 0;
}

// Store slot -> window position, device to device on the context stream, where the position does
// not hold that slot's content already (fslot: the store slot of every frame position)
int place_store_frames(ldso_ba_ctx *c, const std::vector<int> &fslot) {
    const FrameStore &S = c->store;
    c->img_tag.resize((size_t)c->n_frames, 0ull);
    const size_t bytes = c->img.slot_bytes();
    for (int p = 0; p < c->n_frames; p++) {
        const unsigned long long seq = S.seq[fslot[p]];
        if (c->img_tag[p] == seq) continue;
        c->img_tag[p] = 0;
        HIP_TRY(hipMemcpyAsync(c->d_img.p + (size_t)p * c->img.frame_stride, S.slot(fslot[p]), bytes,
                               hipMemcpyDeviceToDevice, c->stream));
        c->img_tag[p] = seq;
        c->xfer[1] += (int64_t)bytes;
    }
    return 0;
}

// ldso_ba_load_marginalization_device's gather, once the marginalisation context's buffers stand and
// its gather indices (d_ed_rs_src, d_ed_pt_src: positions in the parent's window) are uploaded:
// k_edit_gather with its sources at the parent's arrays, priorF scaled.  The two streams are ordered
// by events and never by the host: the gather waits for what the parent's stream holds now, and
// whatever that stream is given later -- a pass, an edit that swaps the arrays -- waits for the gather.
// F: the load walk's parameters (newstate and R; its fills are load_apply's).
int marg_gather(ldso_ba_ctx *c, const ldso_ba_ctx *parent, int parent_win, const EditParams &F) {
    const WinDev &pw = parent->wd[parent_win];
    EditParams E = F;
    E.n_fill = 0;
    E.rs_src = c->d_ed_rs_src.p;
    E.pt_src = c->d_ed_pt_src.p;
    E.o_state = parent->d_rs_state.p + pw.res_base;
    E.o_flags = parent->d_rs_flags.p + pw.res_base;
    E.o_energy = parent->d_rs_energy.p + pw.res_base;
    E.o_newenergy = E.o_energy;  // as a load: state_NewEnergy is loaded equal to state_energy
    E.o_pt = reinterpret_cast<const float4 *>(parent->d_pt_data.p) + (size_t)pw.point_base * kPtVec;
    E.n_state = nullptr;  // every index is a position of the parent (marg_plan.cpp): no new entries
    E.n_flags = nullptr;
    E.n_energy = nullptr;
    E.n_pt = nullptr;
    E.state = c->d_rs_state.p;
    E.flags = c->d_rs_flags.p;
    E.energy = c->d_rs_energy.p;
    E.newenergy = c->d_rs_newenergy.p;
    E.pt = reinterpret_cast<float4 *>(c->d_pt_data.p);
    E.newstate = c->d_rs_newstate.p;
    E.R = c->R_tot;
    E.P = c->P_tot;
    E.scale_prior = 1;
    E.prior_fac = kIdepthFixPriorMargFac;
    // read the parent's window behind what its stream holds now; its later work waits for the read
    if (int rc = c->mg_borrow.begin(c->stream, parent->stream)) return rc;
    const size_t work = std::max<size_t>((size_t)E.R, (size_t)E.P * kPtVec);
    if (work) {
        const int nb = (int)std::min<size_t>(1024, (work + 255) / 256);
        k_edit_gather<<<nb, 256, 0, c->stream>>>(E);
        HIP_TRY(hipGetLastError());
    }
    return c->mg_borrow.end(c->stream, parent->stream);
}

// parent != nullptr: a marginalisation context over `ws[0]` whose frames are the parent's window
// parent_win (images borrowed, not uploaded; priorF scaled by setting_idepthFixPriorMargFac)
// frame_ids != nullptr (ldso_ba_load_frames): the windows' frames are resident in the frame store
// under these ids, [sum N]; the windows' dI is not read
// gather != nullptr (ldso_ba_load_marginalization_device, with parent): the layout is the plan's, and
// the carried arrays -- the point records and the residuals' state, energy and flags -- are gathered
// from the parent's device arrays by k_edit_gather instead of uploaded; ws is not read
int load_impl(ldso_ba_ctx *c, int32_t n_windows, const ldso_ba_window *ws, int32_t shard_rank, int32_t shard_count,
              const ldso_ba_ctx *parent, int parent_win, const int64_t *frame_ids = nullptr, MargPlan *gather = nullptr) {
    if (!c || n_windows < 1 || !ws) return fail(-1, "bad arguments");
    if (shard_count < 1 || shard_rank < 0 || shard_rank >= shard_count) return fail(-1, "bad shard");
    const FrameStore &S = c->store;
    if (frame_ids && S.cap == 0) return fail(LDSO_BA_ERR_FRAME_STORE, "no frame store: call ldso_ba_frames_reserve first");
    Layout L_own;
    int rc = gather ? 0
                    : build_layout(ws, n_windows, shard_rank, shard_count, c->item_order, c->top_chunk, parent != nullptr, L_own,
                                   frame_ids != nullptr);
    if (rc) return rc;
    Layout &L = gather ? gather->L : L_own;
    std::vector<int> fslot;
    if (frame_ids && (rc = store_slots(S, ws, n_windows, frame_ids, fslot))) return rc;
    HIP_TRY(hipSetDevice(c->device));
    HIP_TRY(hipStreamSynchronize(c->stream));
    c->n_win = n_windows;
    c->shard_count = shard_count;
    c->marg = parent != nullptr;
    c->by_id = frame_ids != nullptr;
    c->img_ext = nullptr;
    if (parent) {
        c->img = parent->img;
        c->img_mode_pref = parent->img.mode;
        c->img_ext = parent->d_img.p + (size_t)parent->wd[parent_win].frame_base * parent->img.frame_stride;
    } else {
        // a load from the store runs in the store's layout, ldso_ba_load in the preferred one
        c->img = image_layout(frame_ids ? S.lay.mode : c->img_mode_pref, ws[0].width, ws[0].height);
    }
    adopt_layout(c, L, n_windows);
    WindowWalk<false> A{c};
    const size_t img_n = (size_t)c->n_frames * c->img.frame_stride;
    if (c->marg) {
        c->d_img.release();
        c->img_tag.clear();
        A.sized(c->d_adhtd, (size_t)c->n_pairs * 8);
    } else if (!frame_ids || !c->d_img.p || c->d_img.n < img_n) {
        A.sized(c->d_img, img_n);  // a new array (and ldso_ba_load's own images) invalidates the tags
        c->xfer[2]++;
        c->img_tag.clear();
    }
    if (gather) {  // the gather indices travel with the load's uploads
        A.gather_carried = true;
        A.sized(c->d_ed_rs_src, gather->rs_gather.size());
        A.sized(c->d_ed_pt_src, gather->pt_gather.size());
        if (!A.rc) {
            A.ups.add(c->d_ed_rs_src.p, gather->rs_gather.data(), gather->rs_gather.size() * sizeof(int));
            A.ups.add(c->d_ed_pt_src.p, gather->pt_gather.data(), gather->pt_gather.size() * sizeof(int));
        }
    }
    window_buffers(c, L, (size_t)n_windows, A);
    if ((rc = load_apply(c, A))) return rc;
    if (gather && (rc = marg_gather(c, parent, parent_win, A.E))) return rc;
    // images: per frame through a float3 staging buffer, repacked on the device; the
    // intensity-only layout falls back to 2x4 float4 tiles if the caller's gradients are not
    // makeImages' (then recomputing them would not be exact)
    if (frame_ids) {
        if ((rc = place_store_frames(c, fslot))) return rc;
    } else if (!c->marg) {
        int mismatch = 0;
        if ((rc = stage_images(c, ws, n_windows, &mismatch))) return rc;
        if (c->img.mode == 3 && mismatch) {
            c->img_mode_pref = 1;  // for later loads and reserves too
            c->img = image_layout(1, c->img.width, c->img.height);
            rc = c->d_img.alloc((size_t)c->n_frames * c->img.frame_stride);
            c->xfer[2]++;
            if (rc || (rc = stage_images(c, ws, n_windows, &mismatch))) return rc;
        }
    }
    if ((rc = point_sc_lds_limit(c))) return rc;
    for (int w = 0; w < n_windows; w++)
        if ((rc = upload_priors(c, w))) return rc;
    return 0;
}

// the device times of the last timed edit into ed_stat (its events have been recorded on the stream)
void edit_events_drain(ldso_ba_ctx *c) {
    if (!c->ed_ev_pending) return;
    c->ed_ev_pending = false;
    float a = 0, b = 0;
    if (hipEventSynchronize(c->ed_ev[2].e) == hipSuccess && hipEventElapsedTime(&a, c->ed_ev[0].e, c->ed_ev[1].e) == hipSuccess &&
        hipEventElapsedTime(&b, c->ed_ev[1].e, c->ed_ev[2].e) == hipSuccess) {
        c->ed_stat[4] += a;
        c->ed_stat[5] += b;
    }
}

int edit_impl(ldso_ba_ctx *c, int win, const ldso_ba_edit *e) {
    if (!c || !e || !e->after || !e->frame_ids) return fail(-1, "bad arguments");
    using EdClock = std::chrono::steady_clock;
    const EdClock::time_point ed_t0 = EdClock::now();
    if (c->n_win != 1 || win != 0) return fail(-1, "edit: the context must hold exactly one window (window 0)");
    if (c->marg) return fail(-1, "edit: not on a marginalisation context");
    if (c->shard_count > 1 || c->comm) return fail(-1, "edit: not on a sharded context");
    if (!c->by_id) return fail(-1, "edit: the window was not loaded with ldso_ba_load_frames");
    EditPlan plan;
    int rc = plan_edit(c->wh[0], c->wd[0], *e, c->item_order, c->top_chunk, plan);
    if (rc) return rc;
    const EdClock::time_point ed_t1 = EdClock::now();
    const ldso_ba_window &a = *e->after;
    std::vector<int> fslot;
    if ((rc = store_slots(c->store, &a, 1, e->frame_ids, fslot))) return rc;
    // ---- nothing is refused from here on ----
    Layout &L = plan.L;
    const size_t n_new_r = plan.new_res.size(), n_new_p = plan.new_pts.size();
    HIP_TRY(hipSetDevice(c->device));
    const bool ed_timed = c->timer.on;
    if (ed_timed) {
        edit_events_drain(c);
        for (Event &ev : c->ed_ev)
            if ((rc = ev.ensure(hipEventDefault))) return rc;
    }
    const size_t img_n = L.frame_win.size() * c->img.frame_stride;
    if (!c->d_img.p || c->d_img.n < img_n) {  // as a load: a new image array invalidates the tags
        if ((rc = c->d_img.alloc(std::max(img_n, c->d_img.n + c->d_img.n / 2)))) return rc;
        c->xfer[2]++;
        c->img_tag.clear();
    }
    WindowWalk<true> T{c};
    window_buffers(c, L, 1, T);
    InBatch &B = T.ups;
    EditParams &E = T.E;
    // the gather indices and the new entries
    if ((rc = T.rc) || (rc = edit_grow(c, c->d_ed_rs_src, plan.rs_gather.size())) ||
        (rc = edit_grow(c, c->d_ed_pt_src, plan.pt_gather.size())) || (rc = edit_grow(c, c->d_ed_nstate, pad4(n_new_r))) ||
        (rc = edit_grow(c, c->d_ed_nflags, pad4(n_new_r))) || (rc = edit_grow(c, c->d_ed_nenergy, n_new_r)) ||
        (rc = edit_grow(c, c->d_ed_npt, n_new_p * LDSO_BA_POINT_STRIDE)))
        return rc;

    // the old arrays, before the layout is adopted
    E.o_state = c->d_rs_state.p;
    E.o_flags = c->d_rs_flags.p;
    E.o_energy = c->d_rs_energy.p;
    E.o_newenergy = c->d_rs_newenergy.p;
    E.o_pt = reinterpret_cast<const float4 *>(c->d_pt_data.p);
    adopt_layout(c, L, 1);

    // the compact upload: the new points' records and the new residuals' state, energy and flags
    std::vector<float> n_pt(n_new_p * LDSO_BA_POINT_STRIDE), n_en(n_new_r);
    std::vector<int8_t> n_st(pad4(n_new_r), 0);
    std::vector<uint8_t> n_fl(pad4(n_new_r), 0);
    for (size_t i = 0; i < n_new_p; i++)
        std::memcpy(&n_pt[i * LDSO_BA_POINT_STRIDE], a.point_data + (size_t)plan.new_pts[i] * LDSO_BA_POINT_STRIDE,
                    LDSO_BA_POINT_STRIDE * sizeof(float));
    for (size_t i = 0; i < n_new_r; i++) {
        n_st[i] = a.res_state[plan.new_res[i]];
        n_fl[i] = a.res_flags[plan.new_res[i]];
        n_en[i] = a.res_energy[plan.new_res[i]];
    }
    std::vector<double> pr;
    priors_vector(c, 0, pr);
    auto put = [&B](void *dst, const auto &v) { B.add(dst, v.data(), v.size() * sizeof(v[0])); };
    put(c->d_prior.p, pr);
    put(c->d_ed_rs_src.p, plan.rs_gather);
    put(c->d_ed_pt_src.p, plan.pt_gather);
    put(c->d_ed_nstate.p, n_st);
    put(c->d_ed_nflags.p, n_fl);
    put(c->d_ed_nenergy.p, n_en);
    put(c->d_ed_npt.p, n_pt);
    if (ed_timed) HIP_TRY(hipEventRecord(c->ed_ev[0].e, c->stream));
    if ((rc = B.flush(c))) return rc;
    if (ed_timed) HIP_TRY(hipEventRecord(c->ed_ev[1].e, c->stream));

    E.rs_src = c->d_ed_rs_src.p;
    E.pt_src = c->d_ed_pt_src.p;
    E.n_state = c->d_ed_nstate.p;
    E.n_flags = c->d_ed_nflags.p;
    E.n_energy = c->d_ed_nenergy.p;
    E.n_pt = reinterpret_cast<const float4 *>(c->d_ed_npt.p);
    E.state = c->d_ed_state.p;
    E.flags = c->d_ed_flags.p;
    E.energy = c->d_ed_energy.p;
    E.newenergy = c->d_ed_newenergy.p;
    E.pt = reinterpret_cast<float4 *>(c->d_ed_pt.p);
    E.P = c->P_tot;  // newstate and R: the walk's
    size_t work = std::max<size_t>(E.R, (size_t)E.P * kPtVec);
    for (int f = 0; f < E.n_fill; f++) work = std::max(work, (size_t)E.fill_words[f]);
    const int nb = (int)std::min<size_t>(1024, (work + 255) / 256 + 1);
    k_edit_gather<<<nb, 256, 0, c->stream>>>(E);
    HIP_TRY(hipGetLastError());
    if (ed_timed) {
        HIP_TRY(hipEventRecord(c->ed_ev[2].e, c->stream));
        c->ed_ev_pending = true;
    }
    // the gathered halves become the context's arrays; captured graphs hold the old addresses
    swap_halves(c->d_rs_state, c->d_ed_state);
    swap_halves(c->d_rs_flags, c->d_ed_flags);
    swap_halves(c->d_rs_energy, c->d_ed_energy);
    swap_halves(c->d_rs_newenergy, c->d_ed_newenergy);
    swap_halves(c->d_pt_data, c->d_ed_pt);
    BumpAllocGen::changed();
    if ((rc = place_store_frames(c, fslot))) return rc;
    if ((rc = point_sc_lds_limit(c))) return rc;
    const EdClock::time_point ed_t2 = EdClock::now();
    c->ed_stat[0] += 1;
    c->ed_stat[1] += std::chrono::duration<double, std::milli>(ed_t1 - ed_t0).count();
    c->ed_stat[2] += std::chrono::duration<double, std::milli>(ed_t2 - ed_t1).count();
    c->ed_stat[3] += std::chrono::duration<double, std::milli>(ed_t2 - ed_t0).count();
    return 0;
}

}  // namespace
