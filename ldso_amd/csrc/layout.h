// layout.h -- the window layout ldso_ba_load builds on the host: sharding, the residual bucket
// sort, the k_linearize / k_point_sc work items and every base offset of the device arrays.
// Host-only code (layout.cpp is compiled without an offload architecture), so it runs on a CPU,
// under a sanitizer, and in tests that need no GPU.  The device translation unit includes this
// header for the descriptor both sides share.
#pragma once
#include <cstddef>
#include <cstdint>
#include <vector>

#include "ldso_ba_internal.h"

namespace ldso_ba {

// Per-window device descriptor (uploaded as is; the kernels know it as WinDev, ba_device.h).
struct WinDesc {
    int N, P, R, D;
    int frame_base, pair_base, point_base, res_base;
    int top_item_base, n_top_items;
    int sc_item_base, n_sc_items;
    int K, KP, ntiles, p_all;  // p_all: the window's points over every shard (numID)
    long long sc_slab_base;  // floats
    long long sys_base;      // doubles: packed system
    long long stage_base;    // doubles: k_stitch contribution records, N^2 pairs x stage_rec(N)
    int newest_begin, newest_end;
    int rec_base;            // record slots: rec_base + s * P + q (s = target slot of host's point q)
    int vec_base;            // per-window (8N+4)-vectors (priors, x): vec_base + i
    int width, height;
    float wM3, hM3;
    float calib[4];
    float cdelta[4];         // EnergyFunctional::cDeltaF (marginalisation pass only)
    int adt_diag;            // every ad_target block of the window is diagonal (adjoints_diagonal): k_stitch_host scales
};

struct WinHost {
    int N, P, R;                    // this shard
    int P_all, R_all;               // caller's counts
    std::vector<int> pt_orig;       // sorted -> caller point index
    std::vector<int> rs_orig;       // sorted -> caller residual index
    std::vector<int> rs_slot;       // sorted residual -> record slot (global)
    std::vector<int> pt_host;       // sorted point host
    std::vector<double> c_prior, frame_prior, frame_delta_prior;
    std::vector<float> c_delta;
    std::vector<float> adHF, adTF;  // float adjoints (resubstitute)
    bool add_priors = true;
};

LDSO_HD inline long long packed_len(int D) { return (long long)D * (D + 1) / 2; }
LDSO_HD inline long long sys_len(int D) { return 2 * (packed_len(D) + D); }
// doubles of k_stitch's contribution record of one (h, t) pair (its fields: ba_device.h)
LDSO_HD inline int stage_rec(int N) { return 520 + 64 * (N - 1); }

// One frame as the kernels read it, in the window's image array or in a frame-store slot, padded
// to whole tiles.  mode 3: intensity only, 8-pixel x 4-row bands (band_offset); mode 1:
// [I, dx, dy, 0] texels in 2x4 tiles.
struct ImageLayout {
    int mode = 3, width = 0, height = 0;
    int tiles_per_row = 0;       // mode 3: 8-pixel tiles per row; mode 1: 2-texel tiles per row
    int padded_h = 0;            // height rounded up to whole 4-row tiles
    long long frame_stride = 0;  // float4 units per frame
    size_t npix() const { return (size_t)width * height; }
    size_t slot_bytes() const { return (size_t)frame_stride * 16; }
    // elements the repack of a staged float3 frame writes, one thread each: mode 3 the padded
    // intensities (k_intensity_image), mode 1 the padded texels (k_tile_image)
    long long repack_elems() const { return mode == 3 ? (long long)tiles_per_row * 8 * padded_h : frame_stride; }
};
ImageLayout image_layout(int mode, int width, int height);

constexpr int kScPoints = 64;  // points per k_point_sc block (large loads; small ones take 16)
constexpr int kPrePitch = 12;  // floats of staged precalc (R0, t0) per target in k_point_sc's LDS
// k_point_sc dynamic LDS of a window whose padded Schur block is KP wide
size_t sc_smem_bytes(int KP);

// work items as the kernels read them (the device side's int4 / int2)
struct alignas(16) Item4 {
    int x, y, z, w;
};
struct alignas(8) Item2 {
    int x, y;
};

// Everything ldso_ba_load uploads or sizes its buffers by.  Per-residual and per-point arrays are
// in device order (WinHost::rs_orig / pt_orig), the windows back to back.
struct Layout {
    std::vector<WinHost> wh;
    std::vector<WinDesc> wd;
    std::vector<Item4> top_items;   // k_linearize: {first residual, count | first-of-pair << 16, pair, window}
    std::vector<Item4> sc_items;    // k_point_sc: {first point, count, host, window}
    std::vector<Item2> pair_items;  // per pair h + N t: {first top item, count}
    std::vector<Item2> host_items;  // per frame: {first sc item, count}
    std::vector<Item2> sum_blocks;  // k_stitch_sum: {window, first packed element} per 256-thread block
    std::vector<int> pair_win, frame_win, pt_win;
    std::vector<int> rs_slot, pt_nres, pt_host;
    std::vector<unsigned long long> pt_tgt;  // a point's residual targets, 4 bits each
    std::vector<uint8_t> rs_tgt, rs_flags;
    std::vector<int8_t> rs_state;
    std::vector<float> rs_energy, pt_data, precalc, frame_th;
    std::vector<double> adH, adT;
    long long sc_slab_total = 0, sys_total = 0, stage_total = 0;
    int vec_total = 0, rec_base = 0, max_frames = 0;
    int chunk = 0, sc_chunk = 0;  // residuals per k_linearize wave, points per k_point_sc block
    size_t smem_max = 0;          // k_point_sc dynamic LDS of the widest window
};

// Whether each of the n_blocks 8x8 row-major blocks of `ad` has all 56 off-diagonal entries equal
// to zero (exactly: -0.0 is zero, a denormal is not).  setAdjointsF's adTarget is (ldso_ba_set_adjoints).
bool adjoints_diagonal(const double *ad, size_t n_blocks);

// The ldso_ba_window contract (ldso_ba_validate_window); -1 and the thread's error message if not.
int check_window(const ldso_ba_window &w, bool need_images = true);

// SURVEY.md §8e's partition: the caller's point indices rank `rank` of `count` owns, in device order.
void shard_points(const ldso_ba_window &in, int rank, int count, std::vector<int> &out);

// Checks every window (images are not needed for a marginalisation context) and lays out this
// shard of them.  item_order: ldso_ba_set_tuning's LDSO_BA_TUNE_ITEM_ORDER; top_chunk: its
// LDSO_BA_TUNE_TOP_CHUNK (0 = by load size); marg: a marginalisation context (priorF scaled by
// setting_idepthFixPriorMargFac); resident_frames: the frames are named by frame-store ids
// (ldso_ba_load_frames), so the windows' dI is not needed either.  Returns 0, or -1 with the
// thread's error message set.
int build_layout(const ldso_ba_window *ws, int n_windows, int shard_rank, int shard_count, int item_order,
                 int top_chunk, bool marg, Layout &out, bool resident_frames = false);

}  // namespace ldso_ba
