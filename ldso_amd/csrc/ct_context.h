// ct_context.h -- the tracker's host-side state and the helpers every part of its host code shares.
// struct ldso_ct_ctx is a core (device, stream, pyramid geometry, calibration, scratch, timer) and one
// member struct per subsystem; each ct_host_<part>.h holds the helpers and entry points of one part.
// The part structs stand here and not in those headers: the core holds them by value, so it needs their
// complete types, while a part's functions need the complete core -- and each header compiles alone.
// For the same reason ct_launch, ct_grow, ct_blocks, level_grid, level_of and ct_read stand below the
// core and not in ldso_ct.hip.  Every member (hip_owning.h) owns its buffer or events: deleting the
// context frees them.
// A part reads or grows another part's members only through the context; the three such dependencies
// are named at the part they reach into (CtFrame::d_dIp, CtRes::d_state / d_warp, CtIp::d_ip / d_ip_alt).
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>

#include "../../include/ldso_ct.h"
#include "hip_owning.h"
#include "k_ct_pyramid.h"
#include "k_ct_residual.h"
#include "k_ct_immature.h"
#include "k_ct_coarse_depth.h"
#include "k_ct_select.h"
#include "k_ct_corners.h"
#include "k_ct_track.h"
#include "k_ct_actsel.h"
#include "k_ct_init.h"
#include "k_ct_undistort.h"

namespace {

constexpr int kMaxHyp = 256;
// the timed launches' slots (ldso_ct_get_kernel_times / _kernel_name): each name below its slot
enum : int { kCtSlotPyrDown,      kCtSlotPyrGrad, kCtSlotCalcRes, kCtSlotCalcGs,
             kCtSlotMakeImmature, kCtSlotTrace,   kCtSlotIpCount, kNumCtKernels };
const char *kCtKernelNames[kNumCtKernels] = {"k_ct_pyr_down",      "k_ct_pyr_grad", "k_ct_calc_res", "k_ct_calc_gs",
                                             "k_ct_make_immature", "k_ct_trace",    "k_ct_ip_count"};

// the new frame (ct_host_frame.h): its level-0 image, intensity pyramid and texels, allocated at create.
// Every other part reads d_dIp (the initializer d_inten too).  Frame ingestion (k_ct_undistort.h): the
// tables of ldso_ct_undistort_init; the raw frame's pinned and device staging, sized for 16 bits
struct CtFrame {
    DevBuf<float> d_color, d_inten, d_B;
    DevBuf<float4> d_dIp;
    float exposure = 0;
    bool have = false;
    DevBuf<float2> d_und_remap;
    DevBuf<float> d_und_g, d_und_vinv;
    bool und_init = false, und_pass = false;
    int und_w_org = 0, und_h_org = 0, und_g_depth = 0;  // g_depth 0: no photometric calibration
    int und_mode = 0, und_use_exposure = 1;
    PinBuf<uint8_t> h_und_raw;
    DevBuf<uint8_t> d_und_raw;
    StreamBorrow borrow;  // a device source's stream (ldso_ct_set_new_frame_raw_device)
};

// the reference (ct_host_ref.h): the point clouds of all levels back to back.  makeCoarseDepthL0 on the
// device (k_ct_coarse_depth.h): work buffers allocated on first use; only the contributions grow.
// Setting or making a reference grows res.d_state / res.d_warp to its largest level.
struct CtRef {
    DevBuf<float4> d_pc;
    int pc_off[LDSO_CT_MAX_LEVELS + 1] = {0};
    float exposure = 0, a = 0, b = 0;
    bool have = false;
    DevBuf<float4> d_contrib;
    PinBuf<float4> h_contrib;  // pinned staging
    DevBuf<float> d_maps;      // idepth | weightSums, every level flat (2 x pyr.off[levels])
    DevBuf<float4> d_cand;     // a candidate per pixel of every level
    DevBuf<int> d_blk;         // [blocks] counts, then offsets; [blocks .. +levels] level offsets
    PinMappedOf<int> counts;   // pc_n per level
    CdLevels lv{};
    int interior = 0, interior0 = 0;  // interior pixels of all levels / of level 0
    StreamBorrow borrow;              // another context's frame, the BA pass's arrays
};

// calcRes / calcGSSSE and the LM loop (ct_host_res.h)
struct CtRes {
    // warped buffers of the last single-pose calcRes: n states and 2 n records, grown together (by ref:
    // ldso_ct_set_reference and cd_ensure size them for the reference's largest level)
    DevBuf<uint8_t> d_state;
    DevBuf<float4> d_warp;
    int last_lvl = -1, last_warped = 0;
    // per-call staging.  The block partials live in coherent mapped host memory: the kernels write
    // them straight to the host (a few KB), so a call needs no copy launch, only the synchronisation
    PinBuf<CtPose> h_poses;
    DevBuf<CtPose> d_poses;
    PinMappedOf<double> parts;
    // the LM loop (k_ct_track.h): starts in, results and start 0's trace out, all in mapped host memory
    PinMappedOf<CtTrackStart> track_in;
    PinMappedOf<ldso_ct_track_result> track_out;
    PinMappedOf<ldso_ct_track_step> track_trace;
    PinMappedOf<int> track_n;
};

// immature points (ct_host_ip.h): resident records, per-host tables, make staging, counters
struct CtIp {
    DevBuf<IpRec> d_ip;
    int n = 0, max_host = -1;
    DevBuf<float> d_hosts;
    PinBuf<float> h_hosts;
    DevBuf<float2> d_uv;
    DevBuf<int> d_counts;
    PinBuf<int> h_counts;
    // d_ip_alt: the target of the activation selection's compaction (as), then swapped with d_ip (so the
    // immature set is held twice once a call has compacted); after ldso_ct_immature_append has grown d_ip
    // it is the old, smaller buffer, which stays allocated until the next compaction replaces it with one
    // of d_ip's capacity
    DevBuf<IpRec> d_ip_alt;
};

// pixel selection (ct_host_sel.h, k_ct_select.h): the pattern and the potential from ldso_ct_select_init,
// the work buffers (sizes follow the image size) allocated by the first selection
struct CtSel {
    DevBuf<uint8_t> d_pattern, d_map;
    PinBuf<uint8_t> h_map;
    DevBuf<float> d_ths_raw, d_ths;  // ths [w32*h32]; thsSmoothed, every index select can form, the unwritten 0
    DevBuf<unsigned> d_mask;         // per cell, in traversal order
    DevBuf<int> d_n2, d_nu;          // n2 at each cell's start; the direction-dependent cells
    DevBuf<int> d_blk;               // block counts / offsets of the scans (two arrays)
    DevBuf<int> d_cnt;
    PinBuf<int> h_cnt;
    int potential = 0;  // currentPotential; 0: ldso_ct_select_init not called
};

// corner detection (ct_host_cor.h, k_ct_corners.h): the ORB table and umax from ldso_ct_corners_init; the
// work buffers, sized by the grid alone (every pixel of a cell a candidate), allocated by the first detection
struct CtCor {
    DevBuf<int4> d_pattern;
    CorUmax umax{};
    bool init = false;
    int n = -1;  // features of the last detection whose records d_feat / d_out hold; -1: none
    DevBuf<int> d_cell;               // [cells] pick counts, then [cells] their exclusive prefix
    DevBuf<CorSlot> d_slot, d_feat;   // the picks per cell; the features in output order
    DevBuf<int> d_corner, d_cnt;
    DevBuf<ldso_ct_feature> d_out;
    PinMappedOf<int> counts;          // the counters, written by the last launch
};

// activation candidates (ct_host_as.h, k_ct_actsel.h): the level-1 map and the host tables of the last
// distance-map call; the work buffers, sized by the frame (map, bins) and by the resident set's capacity,
// allocated by the first call that needs them; the OPTIMIZE records of the last selection.  A compacting
// selection writes the survivors to ip.d_ip_alt and swaps it with ip.d_ip.
struct CtAs {
    DevBuf<int> d_map;
    PinBuf<int> h_map;
    DevBuf<float> d_hosts, d_uvd;  // [n_hosts][KRKi 9, Kt 3] of level 1; the host seeds
    PinBuf<float> h_hosts;
    DevBuf<int> d_seed_host;
    DevBuf<uint8_t> d_flag;
    PinBuf<uint8_t> h_flag;
    int n_hosts = 0;
    bool have_map = false;
    DevBuf<AsCand> d_cand;
    DevBuf<AsEntry> d_entry;
    DevBuf<int> d_disp, d_out;  // the walk's states; dispositions [n], then selected indices [n]
    PinBuf<int> h_out;
    DevBuf<int> d_blk, d_tot, d_cnt;  // d_cnt: the counters, then the bins and the scatter's cursors
    PinBuf<int> h_cnt;
    PinMappedOf<int> counts;  // the counters, written by the last launch
    DevBuf<IpRec> d_selected;
    int sel_n = -1, sel_hosts = 0;  // -1: no selection yet
    StreamBorrow borrow;            // the BA window's points (ldso_ct_make_distance_map_ba)
};

// the coarse initializer (ct_host_init.h, k_ct_init.h): firstFrame's pyramid and level-0 intensities,
// snapshots of the new frame at ldso_ct_init_set_first; the points of every level back to back; the sweep
// orders, rank offsets and child lists, one int table; JbBuffer | JbBuffer_new; the state trackFrame
// carries from call to call; result, evaluation and trace in mapped host memory
struct CtInit {
    DevBuf<float4> d_first;
    DevBuf<float> d_inten;
    DevBuf<ldso_ct_init_point> d_pts;
    DevBuf<int> d_tab;
    DevBuf<float> d_jb;
    PinMappedOf<CtInitOut> out;
    PinMappedOf<ldso_ct_init_step> trace;
    bool have_first = false;
    int off[ldso_ct::kInitMaxLevels + 1] = {0};
    int order_off[ldso_ct::kInitMaxLevels] = {0}, rank_off[ldso_ct::kInitMaxLevels] = {0};
    int child_off[ldso_ct::kInitMaxLevels] = {0}, child[ldso_ct::kInitMaxLevels] = {0};
    int n_ranks[ldso_ct::kInitMaxLevels] = {0};
    int max_n = 0, jb_cur = 0;
    float first_exposure = 0;
    double this_to_next[12] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0};
    float aff[2] = {0, 0};
    int snapped = 0, frame_id = 0, snapped_at = 0;
};

}  // namespace

struct ldso_ct_ctx {
    // the core: what every part reads
    int device = 0;
    hipStream_t stream = nullptr;
    PyrParams pyr{};
    int levels = 1;
    float fx[LDSO_CT_MAX_LEVELS], fy[LDSO_CT_MAX_LEVELS], cx[LDSO_CT_MAX_LEVELS], cy[LDSO_CT_MAX_LEVELS];
    float Ki[LDSO_CT_MAX_LEVELS][9];
    bool have_k = false;
    // scratch records shared by ldso_ct_make_immature, ldso_ct_make_new_traces and ldso_ct_detect_corners:
    // each grows it, fills it and copies it out, and every such use ends behind a synchronisation of the
    // stream, so none meets another's records
    DevBuf<IpRec> d_mk;
    CtFrame frame;
    CtRef ref;
    CtRes res;
    CtIp ip;
    CtSel sel;
    CtCor cor;
    CtAs as;
    CtInit init;
    // kernel timing, on events with the default flags
    KernelTimer<kNumCtKernels> timer{hipEventDefault, kCtKernelNames};
};

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

// n records from the device to the caller's memory on the context's stream, and the synchronisation
// behind which the caller may read them
template <typename T>
int ct_read(ldso_ct_ctx *c, void *out, const T *dev, size_t n) {
    HIP_TRY(hipMemcpyAsync(out, dev, n * sizeof(T), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return 0;
}

// the blocks of kCtThreads over n items (never none: every launch writes its partials or counts)
int ct_blocks(int n) { return std::max(1, (n + kCtThreads - 1) / kCtThreads); }

// a level's point count and its blocks
struct LevelGrid {
    int n, nb;
};
LevelGrid level_grid(const ldso_ct_ctx *c, int lvl) {
    const int n = c->ref.pc_off[lvl + 1] - c->ref.pc_off[lvl];
    return {n, ct_blocks(n)};
}

// a level as the kernels read it
CtLevel level_of(const ldso_ct_ctx *c, int lvl) {
    CtLevel L;
    L.pc = c->ref.d_pc.p + c->ref.pc_off[lvl];
    L.img = c->frame.d_dIp.p + c->pyr.off[lvl];
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

}  // namespace
