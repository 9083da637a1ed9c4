// ct_context.h -- the tracker's host-side state: the timing slots and struct ldso_ct_ctx, whose members
// (hip_owning.h) own every buffer and event: deleting the context frees them.
#pragma once
#include <hip/hip_runtime.h>

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

}  // namespace

struct ldso_ct_ctx {
    int device = 0;
    hipStream_t stream = nullptr;
    PyrParams pyr{};
    int levels = 1;
    float fx[LDSO_CT_MAX_LEVELS], fy[LDSO_CT_MAX_LEVELS], cx[LDSO_CT_MAX_LEVELS], cy[LDSO_CT_MAX_LEVELS];
    float Ki[LDSO_CT_MAX_LEVELS][9];
    bool have_k = false, have_frame = false, have_ref = false;
    DevBuf<float> d_color, d_inten, d_B;
    DevBuf<float4> d_dIp;
    float new_exposure = 0, ref_exposure = 0, ref_a = 0, ref_b = 0;
    // reference point clouds, all levels back to back
    DevBuf<float4> d_pc;
    int pc_off[LDSO_CT_MAX_LEVELS + 1] = {0};
    // warped buffers of the last single-pose calcRes: n states and 2 n records, grown together
    DevBuf<uint8_t> d_state;
    DevBuf<float4> d_warp;
    int last_lvl = -1, last_warped = 0;
    // per-call staging.  The block partials live in coherent mapped host memory: the kernels write
    // them straight to the host (a few KB), so a call needs no copy launch, only the synchronisation
    PinBuf<CtPose> h_poses;
    DevBuf<CtPose> d_poses;
    PinMappedOf<double> parts;
    // immature points (resident records, per-host tables, make staging, counters)
    DevBuf<IpRec> d_ip;
    int ip_n = 0, ip_max_host = -1;
    DevBuf<float> d_hosts;
    PinBuf<float> h_hosts;
    DevBuf<float2> d_uv;
    DevBuf<IpRec> d_mk;
    DevBuf<int> d_counts;
    PinBuf<int> h_counts;
    // makeCoarseDepthL0 on the device (k_ct_coarse_depth.h): work buffers, allocated on first use;
    // only the contributions grow
    DevBuf<float4> d_cd_contrib;
    PinBuf<float4> h_cd_contrib;  // pinned staging
    DevBuf<float> d_cd_maps;      // idepth | weightSums, every level flat (2 x pyr.off[levels])
    DevBuf<float4> d_cd_cand;     // a candidate per pixel of every level
    DevBuf<int> d_cd_blk;         // [blocks] counts, then offsets; [blocks .. +levels] level offsets
    PinMappedOf<int> cd_counts;   // pc_n per level
    CdLevels cd_lv{};
    int cd_interior = 0, cd_interior0 = 0;  // interior pixels of all levels / of level 0
    Event cd_ev_a, cd_ev_b;
    // pixel selection (k_ct_select.h): the pattern and the potential from ldso_ct_select_init, the work
    // buffers (sizes follow the image size) allocated by the first selection
    DevBuf<uint8_t> d_sel_pattern, d_sel_map;
    PinBuf<uint8_t> h_sel_map;
    DevBuf<float> d_sel_ths_raw, d_sel_ths;  // ths [w32*h32]; thsSmoothed, every index select can form, the unwritten 0
    DevBuf<unsigned> d_sel_mask;             // per cell, in traversal order
    DevBuf<int> d_sel_n2, d_sel_nu;          // n2 at each cell's start; the direction-dependent cells
    DevBuf<int> d_sel_blk;                   // block counts / offsets of the scans (two arrays)
    DevBuf<int> d_sel_cnt;
    PinBuf<int> h_sel_cnt;
    int sel_potential = 0;  // currentPotential; 0: ldso_ct_select_init not called
    // corner detection (k_ct_corners.h): the ORB table and umax from ldso_ct_corners_init; the work buffers,
    // sized by the grid alone (every pixel of a cell a candidate), allocated by the first detection
    DevBuf<int4> d_cor_pattern;
    CorUmax cor_umax{};
    bool cor_init = false;
    int cor_n = -1;  // features of the last detection whose records d_cor_feat / d_cor_out hold; -1: none
    DevBuf<int> d_cor_cell;               // [cells] pick counts, then [cells] their exclusive prefix
    DevBuf<CorSlot> d_cor_slot, d_cor_feat;  // the picks per cell; the features in output order
    DevBuf<int> d_cor_corner, d_cor_cnt;
    DevBuf<ldso_ct_feature> d_cor_out;
    PinMappedOf<int> cor_counts;          // the counters, written by the last launch
    // the LM loop (k_ct_track.h): starts in, results and start 0's trace out, all in mapped host memory
    PinMappedOf<CtTrackStart> track_in;
    PinMappedOf<ldso_ct_track_result> track_out;
    PinMappedOf<ldso_ct_track_step> track_trace;
    PinMappedOf<int> track_n;
    // activation candidates (k_ct_actsel.h): the level-1 map and the host tables of the last distance-map
    // call; the work buffers, sized by the frame (map, bins) and by the resident set's capacity, allocated
    // by the first call that needs them; the OPTIMIZE records of the last selection
    DevBuf<int> d_as_map;
    PinBuf<int> h_as_map;
    DevBuf<float> d_as_hosts, d_as_uvd;  // [n_hosts][KRKi 9, Kt 3] of level 1; the host seeds
    PinBuf<float> h_as_hosts;
    DevBuf<int> d_as_seed_host;
    DevBuf<uint8_t> d_as_flag;
    PinBuf<uint8_t> h_as_flag;
    int as_n_hosts = 0;
    bool as_have_map = false;
    DevBuf<AsCand> d_as_cand;
    DevBuf<AsEntry> d_as_entry;
    DevBuf<int> d_as_disp, d_as_out;  // the walk's states; dispositions [n], then selected indices [n]
    PinBuf<int> h_as_out;
    DevBuf<int> d_as_blk, d_as_tot, d_as_cnt;  // d_as_cnt: the counters, then the bins and the scatter's cursors
    PinBuf<int> h_as_cnt;
    PinMappedOf<int> as_counts;       // the counters, written by the last launch
    // d_ip_alt: the compaction's target, then swapped with d_ip (so the immature set is held twice once a
    // call has compacted); after ldso_ct_immature_append has grown d_ip it is the old, smaller buffer, which
    // stays allocated until the next compaction replaces it with one of d_ip's capacity
    DevBuf<IpRec> d_as_selected, d_ip_alt;
    int as_sel_n = -1, as_sel_hosts = 0;    // -1: no selection yet
    Event as_ev_a, as_ev_b;
    // the coarse initializer (k_ct_init.h): firstFrame's pyramid and level-0 intensities, snapshots of the
    // new frame at ldso_ct_init_set_first; the points of every level back to back; the sweep orders, rank
    // offsets and child lists, one int table; JbBuffer | JbBuffer_new; the state trackFrame carries from
    // call to call; result, evaluation and trace in mapped host memory
    DevBuf<float4> d_init_first;
    DevBuf<float> d_init_inten;
    DevBuf<ldso_ct_init_point> d_init_pts;
    DevBuf<int> d_init_tab;
    DevBuf<float> d_init_jb;
    PinMappedOf<CtInitOut> init_out;
    PinMappedOf<ldso_ct_init_step> init_trace;
    bool init_have_first = false;
    int init_off[ldso_ct::kInitMaxLevels + 1] = {0};
    int init_order_off[ldso_ct::kInitMaxLevels] = {0}, init_rank_off[ldso_ct::kInitMaxLevels] = {0};
    int init_child_off[ldso_ct::kInitMaxLevels] = {0}, init_child[ldso_ct::kInitMaxLevels] = {0};
    int init_n_ranks[ldso_ct::kInitMaxLevels] = {0};
    int init_max_n = 0, init_jb_cur = 0;
    float init_first_exposure = 0;
    double init_this_to_next[12] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0};
    float init_aff[2] = {0, 0};
    int init_snapped = 0, init_frame_id = 0, init_snapped_at = 0;
    // frame ingestion (k_ct_undistort.h): the tables of ldso_ct_undistort_init; the raw frame's pinned and
    // device staging, sized for 16 bits; the events that order a device source's stream with the context's
    DevBuf<float2> d_und_remap;
    DevBuf<float> d_und_g, d_und_vinv;
    bool und_init = false, und_pass = false;
    int und_w_org = 0, und_h_org = 0, und_g_depth = 0;  // g_depth 0: no photometric calibration
    int und_mode = 0, und_use_exposure = 1;
    PinBuf<uint8_t> h_und_raw;
    DevBuf<uint8_t> d_und_raw;
    Event und_ev_prod, und_ev_cons;
    // kernel timing, on events with the default flags
    KernelTimer<kNumCtKernels> timer{hipEventDefault, kCtKernelNames};
};
