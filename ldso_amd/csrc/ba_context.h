// ba_context.h -- the host side's state: the timing slots, the environment switches, the allocation
// generation of the captured graphs, the frame store and struct ldso_ba_ctx (on hip_owning.h's members).
#pragma once
#include <hip/hip_runtime.h>
#include <rccl/rccl.h>

#include <atomic>
#include <chrono>
#include <cstdlib>
#include <string>
#include <vector>

#include "../../include/ldso_ba.h"
#include "../../include/ldso_ct.h"
#include "ba_device.h"
#include "edit_plan.h"
#include "hip_owning.h"

namespace {

// the timed launches' slots (ldso_ba_kernel_times / _kernel_name): each name below its slot
enum : int { kSlotLinearize, kSlotPointSc, kSlotStitch,   kSlotResubstitute,
             kSlotFrameTh,   kSlotSolve,   kSlotActivate, kSlotStitchSum,    kNumKernels };
const char *kKernelNames[kNumKernels] = {"k_linearize", "k_point_sc", "k_stitch",   "k_resubstitute",
                                         "k_frame_th",  "k_solve",    "k_activate", "k_stitch_sum"};

// The environment switches ("environment"): debugging / A-B aids, read here and
// nowhere else.  A flag is on when set and not "0".
struct Switches {
    bool stitch_records;  // LDSO_BA_STITCH_RECORDS: k_stitch for every window size (read at load)
    int hs_split;         // LDSO_BA_HS_SPLIT: -1 unset (by grid size), else 1 for "1...", 0 otherwise
    bool solve_lds;       // LDSO_BA_SOLVE_LDS: the LDS solve k_solve
    bool no_graph;        // LDSO_BA_NO_GRAPH: ldso_ba_optimize / _iterate launch directly
    bool iterate_graph;   // LDSO_BA_ITERATE_GRAPH: ldso_ba_iterate replays a captured graph
    bool stitch_dense_adt;  // LDSO_BA_STITCH_DENSE_ADT: k_stitch_host multiplies by whole ad_target blocks, diagonal or not
};
Switches read_switches() {
    auto flag = [](const char *name) {
        const char *v = std::getenv(name);
        return v && *v && !(v[0] == '0' && v[1] == 0);
    };
    const char *hs = std::getenv("LDSO_BA_HS_SPLIT");
    return {flag("LDSO_BA_STITCH_RECORDS"), hs ? (hs[0] == '1' ? 1 : 0) : -1, flag("LDSO_BA_SOLVE_LDS"),
            flag("LDSO_BA_NO_GRAPH"), flag("LDSO_BA_ITERATE_GRAPH"), flag("LDSO_BA_STITCH_DENSE_ADT")};
}

// ============================================================================================
// host side
// ============================================================================================
// Captured graphs hold device addresses, so launch_cached_graph replays a graph only while
// g_alloc_gen is what it was at the capture.  Every device buffer of the BA unit is a GraphBuf, whose
// alloc / release bump the counter (the contexts' buffers, the frame store, comm_exchange's scratch);
// the tracker's plain DevBufs never appear in a BA graph and do not bump it.
std::atomic<unsigned long long> g_alloc_gen{1};
struct BumpAllocGen {
    static void changed() { g_alloc_gen.fetch_add(1); }
};
template <typename T>
using GraphBuf = DevBuf<T, BumpAllocGen>;

// Frame store (ldso_ba_frames_reserve ...): cap slots of one ImageLayout.  A slot's content is named
// by the sequence number of the put that wrote it (seq, 0 = free).
struct FrameStore {
    GraphBuf<float4> d_store;
    ImageLayout lay;
    int cap = 0;
    std::vector<int64_t> id;
    std::vector<unsigned long long> seq;
    unsigned long long next_seq = 1;
    StreamBorrow borrow;  // producer -> ingest, ingest -> producer's next write
    float4 *slot(int s) const { return d_store.p + (size_t)s * lay.frame_stride; }
    // slot of a resident frame id, or -1
    int find(int64_t frame_id) const {
        for (int s = 0; s < cap; s++)
            if (seq[s] && id[s] == frame_id) return s;
        return -1;
    }
    // the slot a put of `frame_id` writes: the id's own if it is resident, else a free one
    int slot_for(int64_t frame_id, int *out) const {
        if (cap == 0) return fail(LDSO_BA_ERR_FRAME_STORE, "no frame store: call ldso_ba_frames_reserve first");
        int s = find(frame_id);
        for (int k = 0; s < 0 && k < cap; k++)
            if (!seq[k]) s = k;
        if (s < 0)
            return fail(LDSO_BA_ERR_FRAME_STORE, "frame store full (" + std::to_string(cap) +
                                                     " slots): drop a frame before putting id " +
                                                     std::to_string((long long)frame_id));
        *out = s;
        return 0;
    }
    void commit(int s, int64_t frame_id) {
        id[s] = frame_id;
        seq[s] = next_seq++;
    }
};

}  // namespace

struct ldso_ba_ctx {
    int device = 0;
    hipStream_t stream = nullptr;
    // captured launch sequences: ldso_ba_optimize's GN iterations [projection][last pass][ns given]
    // and ldso_ba_iterate's pass + solve + resubstitution [projection]
    // a cached graph and everything fixed at its capture, compared field by field (no packing into
    // one word: a collision would replay a graph whose launch parameters differ)
    struct Graph {
        hipGraphExec_t exec = nullptr;
        unsigned long long gen = 0;
        std::vector<unsigned long long> key;
        Graph() = default;
        Graph(const Graph &) = delete;
        Graph &operator=(const Graph &) = delete;
        ~Graph() { reset(); }
        void reset() {
            if (exec) (void)hipGraphExecDestroy(exec);
            exec = nullptr;
        }
    };
    Graph opt_graph[2], it_graph[2];  // ldso_ba_optimize's whole call (without / with nullspaces)
    bool opt_warm = false;            // an optimize call ran directly on this context
    int item_order = 0;  // k_linearize chunk order: 0 target-major, 1 host-major, 2 target-major banded
    // the reference's settings this context runs with (ldso_ba_set_settings; always checked)
    ldso_ba_opt_settings settings = LDSO_BA_OPT_SETTINGS_INIT;
    int n_win = 0;
    std::vector<WinHost> wh;
    std::vector<WinDev> wd;
    int n_top_items = 0, n_sc_items = 0, n_pairs = 0, n_frames = 0, P_tot = 0, R_tot = 0;
    int max_frames = 0, kp_max = 0;  // the largest window of the load: its N and its WinDev::KP
    int dmax() const { return 8 * max_frames + 4; }  // ... and its WinDev::D
    GraphBuf<WinDev> d_wins;
    // the frames the kernels read: n_frames x img.frame_stride float4.  img is the layout of what is
    // loaded; img_mode_pref the one ldso_ba_load and ldso_ba_frames_reserve take
    // (LDSO_BA_TUNE_TILED_IMAGES, or ldso_ba_load's fallback to 1), which a load from the store, in
    // the store's layout, leaves alone.  img_tag[position of d_img] is the sequence number of the
    // store slot content copied there (0 = not from the store), so ldso_ba_load_frames copies only
    // positions whose tag differs.
    GraphBuf<float4> d_img;
    ImageLayout img;
    int img_mode_pref = 3;
    std::vector<unsigned long long> img_tag;
    FrameStore store;
    GraphBuf<ldso_ct_immature> d_act_in;  // point activation staging (ldso_ba_activate_points)
    GraphBuf<ldso_ba_activation> d_act_out;
    StreamBorrow act_borrow;  // ldso_ba_activate_points_tracker: tracker -> k_activate, k_activate -> tracker
    GraphBuf<float> d_precalc, d_frame_th, d_pt_data, d_pt_out, d_pt_step;
    GraphBuf<double> d_adH, d_adT;
    GraphBuf<int> d_rs_slot, d_pt_nres, d_pair_win, d_frame_win, d_pt_host;
    GraphBuf<unsigned long long> d_pt_tgt;
    GraphBuf<uint8_t> d_rs_tgt, d_rs_flags;
    GraphBuf<int8_t> d_rs_state, d_rs_newstate;
    GraphBuf<float> d_rs_energy, d_rs_newenergy, d_rs_energy_wo;
    GraphBuf<float4> d_rs_center, d_rec_a;
    GraphBuf<float2> d_rec_b;
    GraphBuf<float> d_geo_snap;  // [pairs][kGeoSnap] (LinParams::geo_snap)
    GraphBuf<int4> d_top_items, d_sc_items;
    GraphBuf<int2> d_pair_items, d_host_items;
    GraphBuf<float> d_top_slab, d_sc_slab;
    // d_sys = the exchange buffer: every window's packed system [sys_n], then the linearizeAll
    // energy / #IN pairs [n_win][2] (win_energy()), then doStepFromBackup's sumNID / numID
    // [n_win][2] (win_nid(), double: the ranks' float partials summed) -- contiguous, so that the
    // multi-GPU exchange reduces all three in ONE collective
    GraphBuf<double> d_item_energy, d_sys, d_stage;
    size_t sys_n = 0;
    double *win_energy() const { return d_sys.p + sys_n; }
    double *win_nid() const { return d_sys.p + sys_n + 2 * (size_t)n_win; }
    GraphBuf<int2> d_sum_blocks;  // k_stitch_sum: {window, first packed element} per 256-thread block
    int n_sum_blocks = 0;
    // in-library multi-GPU exchange (ldso_ba_comm_init): RCCL communicator over this context's
    // device, the newest-frame energy slot stride (max over ranks, set at the first exchange
    // after a load) and its staging buffers
    ncclComm_t comm = nullptr;
    int comm_rank = 0, comm_world = 1;
    // the shard count of the last load, and whether a linearisation pass has run since it
    // (ldso_ct_make_reference_ba reads the pass's centres and HdiF of whole windows only)
    int shard_count = 1;
    bool pass_since_load = false;
    // a linearisation pass has been issued: every host copy of its results is stale
    void pass_issued() {
        sys_host_valid = energy_valid = th_host_valid = false;
        pass_since_load = true;
    }
    int64_t x_stride = 0;
    int64_t x_prun = 0;  // |idepth| run length per window slot (max local points over windows and ranks)
    GraphBuf<float> d_x_local, d_x_gathered;
    // device GN loop (ldso_ba_optimize): frame states, CalibHessian::value / value_zero and the
    // prior switches per window, the energy history
    GraphBuf<ldso_ba_frame_state> d_fstate;
    GraphBuf<double> d_calib_val, d_calib_zero, d_cprior, d_ehist;
    GraphBuf<int> d_stop, d_status;  // ldso_ba_optimize: per window, see FrameStepParams
    GraphBuf<int> d_add_priors;
    GraphBuf<float> d_xad;            // [win][kXadStride]
    GraphBuf<double> d_prior, d_x, d_ns;  // per-window (8N+4)-vectors: priors (HL diag, bL), x, nullspaces
    GraphBuf<double> d_ns_nm, d_ns_g;     // k_ortho_prep's Nm [7 vec] and per-window G | G^-1 | fast
    std::vector<double> ns_cache;       // the nullspaces k_ortho_prep last prepared (host copy) ...
    int ns_cache_null = -1;             // ... and their count; -1: nothing prepared
    GraphBuf<int> d_pt_win;
    // marginalisation context (ldso_ba_load_marginalization): images borrowed from the parent
    // context's window, addPoint<2> sums, no prior shift in the SC pass
    bool marg = false;
    bool host_stitch = false;
    int n_cu = 256;  // compute units (k_stitch_host splits its blocks when the grid fits at once)  // k_stitch_host + k_stitch_host_sum (every window <= kHostStitchMaxN keyframes)
    const float4 *img_ext = nullptr;
    const float4 *images() const { return img_ext ? img_ext : d_img.p; }  // the frames the kernels read
    GraphBuf<float> d_adhtd;  // [pairs][8] adHTdeltaF
    int vec_total = 0;
    size_t sc_smem_max = 0;
    unsigned timing_mask = ~0u;  // kernel slots bracketed by events when timing (timer.on) is on
    int top_chunk = 0;  // residuals per k_linearize wave (0 = automatic); LDSO_BA_TUNE_TOP_CHUNK
    int solve_exact = 0;  // LDSO_BA_TUNE_SOLVE_EXACT: 1 = the pivoted k_solve_reg / k_solve (bit-identical to the host)
    // image staging, allocated once and grown only: device float3 frame + mismatch flag, pinned host frame
    GraphBuf<float> d_img_stage;
    GraphBuf<int> d_img_flag;
    PinBuf<char> pin_img;
    // ldso_ba_edit_window.  by_id: the last load named its frames by store id.  d_ed_state ... d_ed_pt:
    // the other halves of the double buffers of d_rs_state, d_rs_flags, d_rs_energy, d_rs_newenergy
    // and d_pt_data (the carried arrays are gathered into them, then the halves change places);
    // d_ed_*_src the gather indices; d_ed_n* the compact upload of the new entries.  Grow-only.
    bool by_id = false;
    GraphBuf<int8_t> d_ed_state, d_ed_nstate;
    GraphBuf<uint8_t> d_ed_flags, d_ed_nflags;
    GraphBuf<float> d_ed_energy, d_ed_newenergy, d_ed_pt, d_ed_nenergy, d_ed_npt;
    GraphBuf<int> d_ed_rs_src, d_ed_pt_src;
    // ldso_ba_edit_stats: edits applied, host clock of the planner / of the rest of the call, and (with
    // kernel timing on) the device time of the staging launches and of k_edit_gather between three events
    double ed_stat[6] = {0, 0, 0, 0, 0, 0};
    Event ed_ev[3];
    bool ed_ev_pending = false;
    // ldso_ba_flag_points: one device block and one pinned block for the call's upload and download
    // (grow-only), and the loaded window's caller-order maps (flag_map_win: the window they were read
    // for, -1 after every load or edit).  d_flag is in no captured graph: a plain DevBuf, so that its
    // growth makes no context capture its graphs again
    DevBuf<int> d_flag;
    PinBuf<int> pin_flag;
    ldso_ba::OldWindow flag_map;
    int flag_map_win = -1;
    // ldso_ba_load_marginalization_device, on the marginalisation context: parent -> gather, gather -> parent
    StreamBorrow mg_borrow;
    int64_t xfer[4] = {0, 0, 0, 0};  // ldso_ba_transfer_stats
    // timing-only events: no system-scope fence (its L2 write-back and invalidate would be timed, and
    // would slow the kernel after the start event)
    KernelTimer<kNumKernels> timer{hipEventDisableSystemFence, kKernelNames};
    std::vector<double> sys_host;  // last downloaded packed systems (per window, see sys_valid)
    std::vector<char> sys_valid;
    bool sys_host_valid = false;   // false => every window's host copy is stale
    // pinned staging for the per-iteration host round trips (system download, xAd upload,
    // point-step download): async copies with one synchronisation each
    PinBuf<double> pin_sys;
    PinBuf<float> pin_xad, pin_step;
    // pinned staging for the results of ldso_ba_iterate / ldso_ba_optimize: every download of
    // one call lands here, behind a single synchronisation
    PinBuf<char> pin_out;
    PinMapped pin_map;  // fine-grained pinned results buffer, written by k_pack_out
    PinMapped pin_in;   // mapped staging of small uploads, read by k_pack_out
    Event pin_in_ev;    // the last launch reading pin_in
    bool pin_in_busy = false;
    std::vector<double> energy_host;
    bool energy_valid = false;
    std::vector<float> th_host;  // d_frame_th as of the end of the last ldso_ba_optimize ...
    bool th_host_valid = false;  // ... until the next pass, update or threshold exchange
    // ldso_ba_linearize_residuals: k_linearize runs on copies of the residual state so that the
    // context's own state (and its records, read by resubstitution) stay untouched
    GraphBuf<int8_t> d_sx_state, d_sx_newstate;
    GraphBuf<uint8_t> d_sx_flags;
    GraphBuf<float> d_sx_energy, d_sx_newenergy, d_sx_ewo;
    GraphBuf<float4> d_sx_center, d_sx_rec_a, d_pt_vals;
    GraphBuf<float2> d_sx_rec_b;
    GraphBuf<float> d_sx_geo_snap, d_jp_out;
    GraphBuf<double> d_sx_item;
};
