// k_linearize.h -- the linearize kernel of the pass (Residuals.cc:15-217, the chunk's
// AccumulatorApprox block) and the residual record it writes.
#pragma once
#include <hip/hip_ext.h>

#include "ba_device.h"

namespace {

// ============================================================================================
// k_linearize
// ============================================================================================
struct LinParams {
    const int4 *__restrict__ items;  // {res_begin, count, pair_global, win}
    const WinDev *__restrict__ wins;
    const float4 *__restrict__ img;  // frames: layout 3 (band_offset) or layout 1 (tex())
    const float *__restrict__ precalc;
    const float *__restrict__ frame_th;
    const int *__restrict__ rs_slot;   // record slot (WinDev::rec_base layout)
    const float *__restrict__ pt_data;
    int8_t *rs_state;
    int8_t *rs_newstate;
    uint8_t *rs_flags;
    float *rs_energy;      // state_energy
    float *rs_newenergy;   // state_NewEnergy (persists: applyRes copies it on a later OOB)
    float *rs_energy_wo;   // state_NewEnergyWithOutlier
    float *rs_center;      // four planes of center_stride floats: centerProjectedTo x, y, z and relBS
    long long center_stride;
    float4 *rec_a;         // [slots]: (j0, j1, JpJdF[6], JpJdF[7]) -- see write_record
    float2 *rec_b;         // [slots]: (bd_r, idepth linearised at; NaN: not active)
    float *geo_snap;       // [pairs][kGeoSnap]: the pass's R0, t0 and calibration (the first chunk of a pair)
    float *top_slab;       // [items][96]
    double *item_energy;   // [items][2]
    int n_items;             // chunks of this launch: [item_base, item_base + n_items)
    int item_base;
    int n_blocks;
    long long frame_stride;  // float4 units per frame
    int tiles_per_row;       // layout 3: 8-pixel tiles per row; layout 1: 2-texel tiles per row
    int fix;
    int accumulate;
    const float *ad_ht_delta;  // [pair_global][8] EnergyFunctional::adHTdeltaF (marginalisation pass)
    const int *stop;           // ldso_ba_optimize: [win] first pass index a window skips - 1 (see linearize_pass)
    int pass;                  // ldso_ba_optimize: this pass's index (0 = the initial linearizeAll)
    int aff_fix;               // bit 0: setting_affineOptModeA < 0, bit 1: ...B < 0 (JabF zeroed, Residuals.cc:186-187)
};

struct PhotoSums {
    float energy, wJI2;
    float JIdx2_00, JIdx2_10, JIdx2_11;
    float JabJIdx_00, JabJIdx_01, JabJIdx_10, JabJIdx_11;
    float Jab2_00, Jab2_01, Jab2_11;
    float JI_r0, JI_r1, Jab_r0, Jab_r1, rr;  // AccumulatedTopHessian.cc:69-77 (mode 0: resApprox = resF)
};

// Point-side terms of AccumulatedTopHessian.cc:94-97 and takeData (Residuals.h:120-129).
__device__ inline void point_terms(const Geo &g, const PhotoSums &s, float jpjdf[8], float hcd[4], float &hdd,
                                   float &bd) {
#pragma clang fp contract(off)
    const float j0 = s.JIdx2_00 * g.d_d_x + s.JIdx2_10 * g.d_d_y;  // JIdx2 * Jpdd
    const float j1 = s.JIdx2_10 * g.d_d_x + s.JIdx2_11 * g.d_d_y;
#pragma unroll
    for (int i = 0; i < 6; i++) jpjdf[i] = g.d_xi_x[i] * j0 + g.d_xi_y[i] * j1;
    jpjdf[6] = s.JabJIdx_00 * g.d_d_x + s.JabJIdx_01 * g.d_d_y;
    jpjdf[7] = s.JabJIdx_10 * g.d_d_x + s.JabJIdx_11 * g.d_d_y;
    bd = s.JI_r0 * g.d_d_x + s.JI_r1 * g.d_d_y;
    hdd = j0 * g.d_d_x + j1 * g.d_d_y;
#pragma unroll
    for (int i = 0; i < 4; i++) hcd[i] = g.d_C_x[i] * j0 + g.d_C_y[i] * j1;
}

// applyRes(true) + takeData record of one residual (Residuals.h:70-88, 120-129) at its slot
// (target-slot major, point minor: a bucket chunk writes consecutive records and a block of
// k_point_sc reads them back coalesced), 24 B in two arrays: A = (j0, j1, JpJdF[6], JpJdF[7]) with
// (j0, j1) = JIdx2 Jpdd, B = (bd_r, idepth) if active; only B = (0, NaN) otherwise (an active
// residual's idepth is never NaN: its centre projection would have failed).  Everything else of
// the residual's takeData is a function of (j0, j1) and its centre geometry -- JpJdF[0..5] =
// Jpdxi^T (j0, j1), Hdd_r = Jpdd^T (j0, j1), Hcd_r = Jpdc^T (j0, j1) (AccumulatedTopHessian.cc:
// 94-97) -- and the geometry is recomputed from the point, the pair precalc and the calibration of
// the pass (centre_projection: the same statements, so the same bits as if they had been stored):
// k_point_sc from the live precalc of the pass, the resubstitution and the JpJdF read-back from the
// geometry snapshot the pass's first chunk of each pair writes (the frame step rewrites the live
// precalc in the same launch as the resubstitution).  64 -> 48 -> 24 B written and read back.
// non-temporal stores for k_linearize's per-residual outputs: nothing reads them again while the
// pass's image lines want the L2 (the next pass, or k_point_sc after the XCD's L2 has turned over
// many times); k_linearize 93.6 -> 91.2 us, FETCH -1.7 MB (r5, profiles/r5/af)
typedef float ntf4 __attribute__((ext_vector_type(4)));
typedef float ntf2 __attribute__((ext_vector_type(2)));
__device__ __forceinline__ void st_nt(float4 *p, float4 v) { __builtin_nontemporal_store(ntf4{v.x, v.y, v.z, v.w}, reinterpret_cast<ntf4 *>(p)); }
__device__ __forceinline__ void st_nt(float2 *p, float2 v) { __builtin_nontemporal_store(ntf2{v.x, v.y}, reinterpret_cast<ntf2 *>(p)); }
template <typename T>
__device__ __forceinline__ void st_nt(T *p, T v) { __builtin_nontemporal_store(v, p); }
__device__ __forceinline__ void write_record(float4 *rec_a, float2 *rec_b, bool active, float idz, const Geo &g,
                                             const PhotoSums &s) {
    if (active) {
        float jp[8], hc[4], hdd, bd;
        point_terms(g, s, jp, hc, hdd, bd);  // jp[0..5], hc, hdd: dead here (recomputed from the geometry)
        const float j0 = s.JIdx2_00 * g.d_d_x + s.JIdx2_10 * g.d_d_y;  // point_terms' statements
        const float j1 = s.JIdx2_10 * g.d_d_x + s.JIdx2_11 * g.d_d_y;
        st_nt(rec_a, make_float4(j0, j1, jp[6], jp[7]));
        st_nt(rec_b, make_float2(bd, idz));
    } else {
        st_nt(rec_b, make_float2(0.f, __builtin_nanf("")));
    }
}
constexpr int kSums = 17;      // energy, wJI2, JIdx2 (3), JabJIdx (4), Jab2 (3), JI_r (2), Jab_r (2), rr
constexpr int kSumStride = kSums;  // floats per residual in the sums buffer (energy < 0: pattern not ok)

// a / b rounded to nearest, without v_div_scale / v_div_fmas / v_div_fixup: the compiler's IEEE
// sequence's rcp, Newton step and two fma corrections, so the same bits as a / b (8 instead of 11
// VALU) PROVIDED a and b are finite, |b| is normal and below 2^126 (so rcp(b) is normal) and the
// quotient and the intermediate products stay in the normal range.  Outside that precondition the
// result may differ from IEEE division (e.g. a denormal b makes rcp overflow to inf and the result
// NaN).  Used for the pattern-pixel projections, where a pixel is kept only when 1.1 < Ku < w - 3:
// a non-finite or out-of-range quotient fails that test whichever way it was rounded, so the one
// input that can decide differently is a subnormal (or > 2^126) homogeneous depth ptp[2] with a
// comparably tiny ptp[0] / ptp[1] -- a point on the target camera's plane at infinity, which LDSO's
// windows do not produce -- that IEEE division would place inside the image and this sequence
// marks OOB.  pixel_terms uses it only on image layout 3 (see there).
__device__ __forceinline__ float div_rn_normal(float a, float b) {
#pragma clang fp contract(off)
    float r = __builtin_amdgcn_rcpf(b);
    const float e = fmaf(-b, r, 1.0f);
    r = fmaf(e, r, r);
    float q = a * r;
    float rem = fmaf(-b, q, a);
    q = fmaf(rem, r, q);
    rem = fmaf(-b, q, a);
    return fmaf(rem, r, q);
}

// sqrt rounded to nearest for a normal, finite a >= 2^-96: the compiler's correctly rounded
// sequence (v_sqrt_f32, then the neighbours one ulp down / up tested by an fma residual) without its
// denormal scaling and its 0 / inf class fixup, which only act outside that range (outside it the
// result may differ from sqrtf; pixel_terms only takes roots of quotients in (1e-5, 1]).
__device__ __forceinline__ float sqrt_rn_normal(float a) {
    const float s = __builtin_amdgcn_sqrtf(a);
    const float sd = __int_as_float(__float_as_int(s) - 1), su = __int_as_float(__float_as_int(s) + 1);
    float r = fmaf(-sd, s, a) <= 0.0f ? sd : s;
    return fmaf(-su, s, a) > 0.0f ? su : r;
}

// one pattern pixel of Residuals.cc:128-190: the 17 addends, in the reference's expression order.
// kMarg: the JI_r / Jab_r / rr addends use res_toZeroF of fixLinearizationF (Residuals.cc:219-245,
// resF - JIdx Jp_delta - JabF delta_ab) as AccumulatedTopHessianSSE::addPoint<2> does
// (AccumulatedTopHessian.cc:44-45, 66-76); jx, jy = Jp_delta_x/y, da, db = adHTdeltaF[6], [7].
// fixA / fixB (setting_affineOptModeA / B < 0, wave-uniform): JabF[0] / JabF[1] are zeroed after the
// pattern sums (Residuals.cc:186-187), i.e. they leave JabJIdx and Jab2 alone and remove the affine
// parameter from Jab_r (AccumulatedTopHessian.cc:71-72) and from res_toZeroF (Residuals.cc:239-240).
// kIeee: plain IEEE division and sqrtf (image layout 1, whose gradients are the caller's and may be
// anything, e.g. inf, where 2500 / (2500 + inf) must give 0).  Otherwise (layout 3: the gradients are
// recomputed with makeImages' clamp, |g| <= 255, and the sample is finite wherever the sums are
// kept) the quotients lie in (0.01, 1], the square roots' arguments in (1e-5, 1] and the Huber
// quotient's |residual| below 2^126, i.e. inside div_rn_normal / sqrt_rn_normal's precondition: same bits.
template <bool kMarg, bool kIeee = false>
__device__ __forceinline__ void pixel_terms(float I, float gx, float gy, float color, float weight, float aff0,
                                            float aff1, float b0, float t[kSums], float jx, float jy, float da,
                                            float db, bool fixA, bool fixB) {
#pragma clang fp contract(off)
    const float residual = I - (float)(aff0 * color + aff1);
    const float drdA = (color - b0);
    auto div = [](float a, float b) { return kIeee ? a / b : div_rn_normal(a, b); };
    auto sqrt_ = [](float a) { return kIeee ? sqrtf(a) : sqrt_rn_normal(a); };
    float wg = sqrt_(div(kOutlierTHSumComponent, kOutlierTHSumComponent + (gx * gx + gy * gy)));
    wg = 0.5f * (wg + weight);
    float hw = fabsf(residual) < kHuberTH ? 1 : div(kHuberTH, fabsf(residual));
    t[0] = wg * wg * hw * residual * residual * (2 - hw);
    if (hw < 1) hw = sqrt_(hw);
    hw = hw * wg;
    gx *= hw;
    gy *= hw;
    const float resF = residual * hw;
    const float jab0 = fixA ? 0.0f : drdA * hw;  // JabF[0], JabF[1] as Jab_r and res_toZeroF see them
    const float jab1 = fixB ? 0.0f : hw;
    t[2] = gx * gx;
    t[4] = gy * gy;
    t[3] = gx * gy;
    t[5] = drdA * hw * gx;
    t[6] = drdA * hw * gy;
    t[7] = hw * gx;
    t[8] = hw * gy;
    t[9] = drdA * drdA * hw * hw;
    t[10] = drdA * hw * hw;
    t[11] = hw * hw;
    t[1] = hw * hw * (gx * gx + gy * gy);
    float ra = resF;
    if constexpr (kMarg) {
        ra = ra - gx * jx;
        ra = ra - gy * jy;
        ra = ra - jab0 * da;
        ra = ra - jab1 * db;
    }
    t[12] = ra * gx;
    t[13] = ra * gy;
    t[14] = ra * jab0;
    t[15] = ra * jab1;
    t[16] = ra * ra;
}

// ---------------------------------------------------------------------------------------------
// AccumulatorApprox of one chunk on the matrix cores.  The chunk's Top block (13x13, index layout
// [0:4 intrinsics, 4:10 xi, 10 a, 11 b, 12 r]) is
//   [0:10, 0:10]  sum_r Jp^T JIdx2 Jp                 (update, MatrixAccumulators.h:893-979)
//   [0:10, 10:13] sum_r Jp^T [JabJIdx | JI_r]          (updateTopRight, :982-1030)
//   [10:13,10:13] sum_r [Jab2, Jab_r; ., rr]           (updateBotRight, :1032-1045)
// with Jp = [x; y] = [Jpdc | Jpdxi] (2x10).  As one GEMM over K = 2 x 64 (residual, row of Jp):
//   D = A B,  A[i][(r,c)] = Jp_r[c][i],  B[(r,0)][j] = (a x + b y)_j,  B[(r,1)][j] = (b x + c y)_j
//   for j < 10, and B[(r,c)][10 + m] = column m of [JabJIdx | JI_r] row c.
// Rows 13 / 14 of A are the indicators of c = 0 / c = 1 and columns 13..15 of B carry the six
// BotRight terms, so D[13][13..15] and D[14][13..15] are their sums.  32 v_mfma_f32_16x16x4f32
// per wavefront, operands staged through the wave's LDS (36 floats per residual, all 64 rows at
// once).  fp32 products accumulated in fp32 like the blocked AccumulatorApprox sums
// (tolerance-checked).
// ---------------------------------------------------------------------------------------------
typedef float f32x4 __attribute__((ext_vector_type(4)));
constexpr int kTopRow = 36;
constexpr int kTermQ = 9;                      // quantities per transposition round (17 = 9 + 8)
// k_linearize footprint box of one residual (layout 3): 3 bands x 9 columns of
// 16-B band-column pieces (4 rows each) + one dummy slot, in floats
constexpr int kBoxCols = 9, kBoxBands = 3, kBoxFloats = 112;
static_assert(kBoxFloats >= (kBoxCols * kBoxBands + 1) * 4, "box");
// floats between the 8 residuals' term tables of a step (dense).  Bank-swizzled bases that make the
// pattern-order sums' 16-B reads conflict-free turn the terms' paired 4-B stores into 2-way
// conflicts instead (r4, PMC ablations: 8.66 vs 8.36 M conflict cycles per launch, time unchanged)
constexpr int kTermStride = 72;
constexpr int kRoundQ = kTermQ;
static_assert(kTermStride >= kRoundQ * 8, "term tables");
constexpr int kTermsOnly = 8 * kTermStride;      // per-pixel addends of one round [8 residuals][kRoundQ][8]
// the terms region also holds the 8 residuals' footprint boxes of a step (used before the terms)
constexpr int kTermsPerWave = 8 * kBoxFloats > kTermsOnly ? 8 * kBoxFloats : kTermsOnly;
constexpr int kSumsPerWave = 64 * kSumStride;   // per-residual sums [64][17]

__device__ __forceinline__ void top_mfma(float *tab, int lane, bool active, const Geo &g, const PhotoSums &s,
                                         float *slab_item) {
    // the residual's operand row; an inactive residual's row is zero (written by a separate
    // exec-masked path, so the active values need no zero-select merge in registers)
    auto stage = [&](float4 *row) {
        if (active) {
            row[0] = make_float4(g.d_C_x[0], g.d_C_y[0], g.d_C_x[1], g.d_C_y[1]);
            row[1] = make_float4(g.d_C_x[2], g.d_C_y[2], g.d_C_x[3], g.d_C_y[3]);
            row[2] = make_float4(g.d_xi_x[0], g.d_xi_y[0], g.d_xi_x[1], g.d_xi_y[1]);
            row[3] = make_float4(g.d_xi_x[2], g.d_xi_y[2], g.d_xi_x[3], g.d_xi_y[3]);
            row[4] = make_float4(g.d_xi_x[4], g.d_xi_y[4], g.d_xi_x[5], g.d_xi_y[5]);
            row[5] = make_float4(s.JabJIdx_00, s.JabJIdx_01, s.JabJIdx_10, s.JabJIdx_11);
            row[6] = make_float4(s.JI_r0, s.JI_r1, s.Jab2_00, s.Jab2_11);
            row[7] = make_float4(s.Jab2_01, s.Jab_r1, s.Jab_r0, s.rr);
            row[8] = make_float4(s.JIdx2_00, s.JIdx2_10, s.JIdx2_11, 0.f);
        } else {
            const float4 z = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
            for (int k = 0; k < 9; k++) row[k] = z;
        }
    };
    const int i = lane & 15, kk = lane >> 4;
    const bool geo = i < 10, ind = i >= 13;
    const float a0c = i == 13 ? 1.f : 0.f, a1c = i == 14 ? 1.f : 0.f;
    // all 64 rows staged at once (one table, one barrier), two independent accumulator chains
    stage(reinterpret_cast<float4 *>(tab + lane * kTopRow));
    wave_lds_sync();
    f32x4 acc0 = {0.f, 0.f, 0.f, 0.f}, acc1 = {0.f, 0.f, 0.f, 0.f};
    {
        // K rows (residual 4 (m + u) + kk, c): the four lane groups read consecutive rows, 36 floats
        // apart, not rows 16 x 36 = 0 mod 64 banks apart (LDS bank conflicts 8.78 -> 7.51 M cycles)
        const float *base = tab + kk * kTopRow;
#pragma unroll 4
        for (int m = 0; m < 16; m += 2) {
#pragma unroll
            for (int u = 0; u < 2; u++) {
                const float *rr = base + 4 * (m + u) * kTopRow;
                const float2 p = *reinterpret_cast<const float2 *>(rr + 2 * i);
                const float4 q = *reinterpret_cast<const float4 *>(rr + 32);
                const float A0 = ind ? a0c : p.x, A1 = ind ? a1c : p.y;
                const float B0 = geo ? q.x * p.x + q.y * p.y : p.x;
                const float B1 = geo ? q.y * p.x + q.z * p.y : p.y;
                f32x4 &acc = u ? acc1 : acc0;
                acc = __builtin_amdgcn_mfma_f32_16x16x4f32(A0, B0, acc, 0, 0, 0);
                acc = __builtin_amdgcn_mfma_f32_16x16x4f32(A1, B1, acc, 0, 0, 0);
            }
        }
    }
    wave_lds_sync();
    const f32x4 acc = acc0 + acc1;
    // lane holds D[4 kk + v][i]; scatter into the 96-slot partial layout read by k_stitch
#pragma unroll
    for (int v = 0; v < 4; v++) {
        const int r = 4 * kk + v, c = i;
        int slot = -1;
        if (r < 10 && c < 10 && c >= r) slot = r * 10 - r * (r - 1) / 2 + (c - r);
        else if (r < 10 && c >= 10 && c < 13) slot = 55 + 3 * r + (c - 10);
        else if (r == 13 && c >= 13) slot = 85 + (c - 13);
        else if (r == 14 && c >= 13) slot = 88 + (c - 13);
        if (slot >= 0) slab_item[slot] = acc[v];
        else if (r == 15 && c < 5) slab_item[91 + c] = 0.f;
    }
}

// ============================================================================================
// k_linearize: one wavefront per chunk of <= 64 residuals of one (host, target) bucket, 4 per
// workgroup, XCD-contiguous chunk ranges.
//   phase A  8 lanes per residual (lane = pattern pixel), 8 residuals per step, a one-step
//            software pipeline: the projection and the 12 intensity taps (layout 3) or 4 texels
//            (layout 1) of step k+1 are issued before step k's arithmetic.  The 17 per-pixel
//            addends of Residuals.cc:128-190 go through LDS and are summed in pattern order.
//   phase B  lane per residual: centre projection (FEJ Jacobians), state / energy
//            (Residuals.cc:192-217), applyRes + the takeData record, relBS on the fix pass.
//   Top      the chunk's AccumulatorApprox block on the matrix cores (top_mfma).
// kMarg: the marginalisation pass (addPoint<2> sums with fixLinearizationF's res_toZeroF).
// ============================================================================================
constexpr int kPtTable = 64 * 4;  // floats: [64 residuals][u, v, idepth, state]
// the Top operand table holds all 64 rows: one stage, one barrier, two independent MFMA chains
// (r5: 94.6 vs 96.5 us against two 32-row halves in one chain; fits the wave's 10 KB of LDS)
constexpr int kTopRows = 64;
constexpr int kTopTab = kTopRows * kTopRow;
constexpr int kWaveLdsA = kTermsPerWave + kSumsPerWave + kPtTable;
// floats of LDS per wavefront (the Top operand table reuses the wave's region after phase B)
constexpr int kWaveLds = kWaveLdsA > kTopTab ? kWaveLdsA : kTopTab;
// LDS requested per 4-wave workgroup: sets the resident workgroups per CU (= waves per SIMD).
// 160 KB / 32 KB = 5: measured fastest (64 x S7: 121.6 us; 4 blocks 125.7, 3 blocks 143.5; 6
// waves/SIMD need <= 80 VGPRs and spill, 145 us).
// 4 workgroups (16 waves) per CU: LDS (kLinLdsBytes) and the register budget of __launch_bounds__
// (<= 128 VGPRs; 101 used).  5 per CU measured slower (r3: 127.5 vs 117.4 us with 44 B spilled; r4:
// 123.7 vs 106.1 us, 32 B spilled, the pt table dropped for LDS)
constexpr int kLinBlocksPerCu = 4;
constexpr size_t kLinLdsBytes = (160 * 1024 / kLinBlocksPerCu) & ~(size_t)511;
static_assert(kLinLdsBytes >= 4 * kWaveLds * sizeof(float), "k_linearize LDS");

// 8-lane group reductions (lanes 8g .. 8g+7) on DPP: quad swaps, then the half-row mirror
// (lane i <-> 7 - i) joins the two quads.
// every lane active, full row / bank masks: no "old" value, so the DPP move can fold into the
// min / or (one DPP-modified VALU op per stage instead of a copy, a DPP move and the op)
#define LDSO_DPP(v, ctrl) __builtin_amdgcn_mov_dpp(v, ctrl, 0xF, 0xF, true)
__device__ __forceinline__ int grp8_min(int v) {
    v = min(v, LDSO_DPP(v, 0xB1));    // quad_perm [1,0,3,2]
    v = min(v, LDSO_DPP(v, 0x4E));    // quad_perm [2,3,0,1]
    return min(v, LDSO_DPP(v, 0x141));  // row_half_mirror
}
__device__ __forceinline__ int grp8_or(int v) {
    v |= LDSO_DPP(v, 0xB1);
    v |= LDSO_DPP(v, 0x4E);
    return v | LDSO_DPP(v, 0x141);
}
__device__ __forceinline__ float4 ldb4(__amdgpu_buffer_rsrc_t r, unsigned off) {
    typedef int i32x4 __attribute__((ext_vector_type(4)));
    const i32x4 v = __builtin_bit_cast(i32x4, __builtin_amdgcn_raw_buffer_load_b128(r, (int)off, 0, 0));
    return make_float4(__int_as_float(v.x), __int_as_float(v.y), __int_as_float(v.z), __int_as_float(v.w));
}

// Phase A of k_linearize on image layout 3 with footprint pieces.  The 8 pattern
// pixels of a residual read their 96 taps (12 each, load12's stencil) from the residual's tap
// footprint: the 16-B band columns (4 rows of one column) that hold at least one of the taps,
// i.e. exactly the 128-B lines the per-lane gathers touch.  The residual's 8 lanes load them with
// one buffer_load_dwordx4 per box band (lane = column) plus one for a 9th column, into a box of
// 3 bands x 9 columns in the wave's LDS (aliasing the terms table of the same step), and the
// pattern lanes read their taps from there: 4 wide loads per lane instead of 12 scalar ones
// (TCP accesses per launch 64.9 M -> 12.4 M on 64 x S7).  The pieces of step k+1 are in flight
// while step k reads its box and sums its terms.  A residual whose footprint does not fit the box
// (pattern spread > 5 pixels) is left out of the pipelined loop and gathered per lane in a second
// loop over the steps that hold one (a gather inside the pipelined loop would make the compiler
// wait for every load in flight, the next step's pieces included).  Taps bit-identical to load12's.
template <bool kMarg>
__device__ __forceinline__ void phase_a_pieces(int lane, float *lds_terms_w, float *S, const float *pre, int jlimit,
                                               int my_state, float4 my_pd0, float jp_dx, float jp_dy, float da,
                                               float db, __amdgpu_buffer_rsrc_t rsrc, unsigned band, float wM3,
                                               float hM3, int aff_fix) {
#pragma clang fp contract(off)
    const int g = lane >> 3, sl = lane & 7;
    const bool fixA = (aff_fix & 1) != 0, fixB = (aff_fix & 2) != 0;
    // staticPattern[8] (Setting.cc:275) offset of this lane's pixel
    const int px = sl == 1 || sl == 6 ? -1 : sl == 2 ? 1 : sl == 3 ? -2 : sl == 5 ? 2 : 0;
    const int py = sl == 0 ? -2 : sl <= 2 ? -1 : sl <= 5 ? 0 : sl == 6 ? 1 : 2;
    const float aff0 = pre[24], aff1 = pre[25], b0a = pre[26];
    float *T = lds_terms_w + g * kTermStride;
    float *box = lds_terms_w + g * kBoxFloats;
    const int nsteps = (jlimit + 7) >> 3;
    constexpr unsigned kOOB = 0x7FFFFFF0u;  // beyond the frame's buffer range: the load returns 0, no access

    struct Geo8 {
        float Ku, Kv, jx, jy;
        int cx0, b0, m;  // box origin (column, band); needed pieces, bit 9 band + column
        bool gok, wide;
    };
    // projection of the lane's pattern pixel of residual 8k + g (Residuals.cc:128-135) and the box
    auto geo = [&](int k, Geo8 &q) {
        const int j = 8 * k + g;
        const float4 pt = *reinterpret_cast<const float4 *>(S + kSumsPerWave + 4 * (j & 63));
        const float pu = pt.x, pv = pt.y, pz = pt.z;
        const int st = __float_as_int(pt.w);
        const bool go = j < jlimit && st != LDSO_BA_RES_OOB;
        if constexpr (kMarg) {
            q.jx = __shfl(jp_dx, j, kWave);
            q.jy = __shfl(jp_dy, j, kWave);
        }
        const float up = pu + px, vp = pv + py;
        float ptp[3];
#pragma unroll
        for (int i = 0; i < 3; i++) ptp[i] = (pre[3 * i] * up + pre[3 * i + 1] * vp + pre[3 * i + 2] * 1.0f) + pre[9 + i] * pz;
        q.Ku = div_rn_normal(ptp[0], ptp[2]);
        q.Kv = div_rn_normal(ptp[1], ptp[2]);
        const bool pok = go && q.Ku > 1.1f && q.Kv > 1.1f && q.Ku < wM3 && q.Kv < hM3;
        const unsigned long long m1 = __ballot(pok);
        q.gok = ((m1 >> (8 * g)) & 0xFFull) == 0xFFull;
        const int ix = pok ? (int)q.Ku : 1, iy = pok ? (int)q.Kv : 1;
        // the box: columns from min(ix) - 1, bands from that of min(iy) - 1
        const int cx0 = grp8_min(ix) - 1, b0 = (grp8_min(iy) - 1) >> 2;
        const int rx = ix - cx0;  // >= 1
        // rows iy-1 / iy+2 use columns ix, ix+1 (pattern 0110 from column ix-1), rows iy, iy+1
        // columns ix-1 .. ix+2 (1111).  The four rows lie in band bA = band(iy-1) and, from row
        // 4 - ph on (ph = (iy-1) & 3), in band bA + 1: the columns needed in band bA are 1111 unless
        // only row iy-1 is there (ph 3: 0110); in band bA + 1 none (ph 0), row iy+2 only (ph 1:
        // 0110) or 1111 (ph 2, 3)
        const int ph = (iy - 1) & 3, bA = ((iy - 1) >> 2) - b0, bD = bA + (ph != 0 ? 1 : 0);
        const int colA = ph == 3 ? 6 : 15, colB = ph == 0 ? 0 : ph == 1 ? 6 : 15;
        const bool wide_l = rx + 2 >= kBoxCols || bD >= kBoxBands;
        int m = wide_l ? 0 : (colA | (colB << kBoxCols)) << (bA * kBoxCols + rx - 1);
        m = grp8_or(m);
        const unsigned long long mw = __ballot(wide_l);
        q.wide = ((mw >> (8 * g)) & 0xFFull) != 0;
        q.m = (q.gok && !q.wide) ? m : 0;
        q.cx0 = cx0;
        q.b0 = b0;
    };
    float4 pc[4];
    bool any8 = true;  // some residual of the step in flight needs the 9th column
    auto issue = [&](int k, Geo8 &q) {
        geo(k, q);
        const int m = q.m;
        const unsigned col = (unsigned)(q.cx0 + sl) << 4, base = (unsigned)q.b0 * band;
#pragma unroll
        for (int b = 0; b < kBoxBands; b++)
            pc[b] = ldb4(rsrc, (m >> (b * kBoxCols + sl)) & 1 ? base + b * band + col : kOOB);
        const bool n8 = sl < kBoxBands && ((m >> (sl * kBoxCols + 8)) & 1);
        any8 = __ballot(n8) != 0;
        if (any8)
            pc[3] = ldb4(rsrc, n8 ? base + sl * band + ((unsigned)(q.cx0 + 8) << 4) : kOOB);
    };
    auto store = [&]() {
        float4 *bx = reinterpret_cast<float4 *>(box);
#pragma unroll
        for (int b = 0; b < kBoxBands; b++) bx[b * kBoxCols + sl] = pc[b];
        if (any8)
            bx[sl < kBoxBands ? sl * kBoxCols + 8 : kBoxBands * kBoxCols] = pc[3];
    };
    // the 12 taps of the lane's pixel from the residual's box
    auto box_taps = [&](const Geo8 &q, float *iv) {
        const int ix = (int)q.Ku, iy = (int)q.Kv;
        // row y of column ix - 1: box float (((y >> 2) - b0) * 9 + ix - 1 - cx0) * 4 + (y & 3)
        // = y + 32 (y >> 2) + 4 (ix - 1 - cx0) - 36 b0; the next columns are 4 floats apart
        static_assert(kBoxCols == 9, "row offsets below assume 9 columns of 4 floats per band");
        const int base = 4 * (ix - 1 - q.cx0) - 36 * q.b0;
        auto row = [&](int y) { return box + (y + ((y >> 2) << 5) + base); };
        const float *r0 = row(iy - 1), *r1 = row(iy), *r2 = row(iy + 1), *r3 = row(iy + 2);
        iv[0] = r0[4];
        iv[1] = r0[8];
        iv[2] = r1[0];
        iv[3] = r1[4];
        iv[4] = r1[8];
        iv[5] = r1[12];
        iv[6] = r2[0];
        iv[7] = r2[4];
        iv[8] = r2[8];
        iv[9] = r2[12];
        iv[10] = r3[4];
        iv[11] = r3[8];
    };
    // the 17 addends of the residuals this pass owns (kWide: the wide ones), summed in pattern order
    // into their sums rows; an owned residual with a pixel out of bounds or not finite gets the
    // "pattern not ok" mark.  Residuals the pass does not own are left untouched.
    auto terms = [&](int k, const Geo8 &q, bool owner, const float *iv) {
        const int j = 8 * k + g;
        const bool part = owner && q.gok;
        bool fin = false;
        float tt[kSums];
        if (part) {
            const float color = S[j * kSumStride + sl], weight = S[j * kSumStride + 8 + sl];
            const int ix = (int)q.Ku, iy = (int)q.Kv;
            const float3 s3 = bilin12(iv, q.Ku - ix, q.Kv - iy);
            fin = isfinite(s3.x);
            pixel_terms<kMarg>(s3.x, s3.y, s3.z, color, weight, aff0, aff1, b0a, tt, kMarg ? q.jx : 0.f,
                               kMarg ? q.jy : 0.f, da, db, fixA, fixB);
        }
        const unsigned long long m2 = __ballot(fin);
        const bool rok = part && ((m2 >> (8 * g)) & 0xFFull) == 0xFFull;
        auto sum8 = [&](int qq, int e) {
            const float4 a = *(const float4 *)&T[e * 8], b = *(const float4 *)&T[e * 8 + 4];
            float sum = 0.0f;
            sum += a.x;
            sum += a.y;
            sum += a.z;
            sum += a.w;
            sum += b.x;
            sum += b.y;
            sum += b.z;
            sum += b.w;
            S[j * kSumStride + qq] = sum;
        };
        wave_lds_sync();  // every box read is done before the terms overwrite the boxes
        if (part) {
#pragma unroll
            for (int e = 0; e < kTermQ; e++) T[e * 8 + sl] = tt[e];
        }
        wave_lds_sync();
        if (rok) {
            sum8(sl, sl);
            if (sl == 0) sum8(8, 8);
        } else if (owner && sl == 0 && j < jlimit) {
            S[j * kSumStride] = -1.0f;  // energy slot: pattern not ok
        }
        wave_lds_sync();
        if (part) {
#pragma unroll
            for (int e = 0; e < kSums - kTermQ; e++) T[e * 8 + sl] = tt[kTermQ + e];
        }
        wave_lds_sync();
        if (rok) sum8(kTermQ + sl, sl);
        wave_lds_sync();
    };
    Geo8 cur, nxt;
    pc[3] = make_float4(0.f, 0.f, 0.f, 0.f);
    unsigned wide_steps = 0;
    auto step = [&](int k, Geo8 &now, Geo8 &next) {
        store();             // waits for step k's pieces
        issue(k + 1, next);  // step k+1's pieces in flight during step k's arithmetic
        wave_lds_sync();
        const bool wide = now.gok && now.wide;
        if (__ballot(wide)) wide_steps |= 1u << k;
        float iv[12];
        if (now.gok && !wide) box_taps(now, iv);
        terms(k, now, !wide, iv);
    };
    issue(0, cur);
    for (int k = 0; k < nsteps; k += 2) {  // ping-pong: no copies of the in-flight step's geometry
        step(k, cur, nxt);
        if (k + 1 >= nsteps) break;
        step(k + 1, nxt, cur);
    }
    // residuals whose footprint exceeds the box: per-lane gathers, step by step
    while (wide_steps) {
        const int k = __builtin_ctz(wide_steps);
        wide_steps &= wide_steps - 1;
        geo(k, cur);
        const bool wide = cur.gok && cur.wide;
        float iv[12];
        if (wide) load12(rsrc, band, (int)cur.Ku, (int)cur.Kv, iv);
        terms(k, cur, wide, iv);
    }
}

template <int kImg, bool kMarg>
__global__ __launch_bounds__(256, kLinBlocksPerCu) void k_linearize(LinParams P) {
    static_assert(kImg == 1 || kImg == 3, "image layouts 1 and 3");
    extern __shared__ __attribute__((aligned(16))) float lds_dyn[];
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    float *lds_terms_w = lds_dyn + wave * kWaveLds;
    float *lds_sums_w = lds_terms_w + kTermsPerWave;
    // XCD-aware mapping: blocks b, b+8, b+16, ... share an XCD (round-robin dispatch), so each XCD
    // gets one contiguous range of chunks; chunks are ordered (window, target, host), so the
    // chunks reading one target frame run on one XCD and share its L2.
    const int nb = P.n_blocks, xcd = blockIdx.x & 7, q8 = nb >> 3, r8 = nb & 7;
    const int lblock = xcd * q8 + min(xcd, r8) + (blockIdx.x >> 3);
    if (lblock * 4 + wave >= P.n_items) return;
    const int itemL = P.item_base + lblock * 4 + wave;  // global chunk index
    const int4 it = P.items[itemL];                     // {res_begin, count, pair_global, win}
    if (P.stop && P.pass > P.stop[__builtin_amdgcn_readfirstlane(it.w)]) return;  // window left the GN loop
    const int cnt = it.y & 0xFFFF;  // bit 16: the pair's first chunk (writes the geometry snapshot)
    const bool valid = lane < cnt;
    const int pair = __builtin_amdgcn_readfirstlane(it.z), jlimit = __builtin_amdgcn_readfirstlane(cnt);
    const WinDev &W = P.wins[__builtin_amdgcn_readfirstlane(it.w)];
    const int N = W.N;
    const int h = (pair - W.pair_base) % N, t = (pair - W.pair_base) / N;
    const float *pre = P.precalc + (size_t)pair * LDSO_BA_PRECALC_STRIDE;
    const float th = fmaxf(P.frame_th[W.frame_base + h], P.frame_th[W.frame_base + t]);
    const float wM3 = W.wM3, hM3 = W.hM3;
    const float4 *img = P.img + (size_t)(W.frame_base + t) * P.frame_stride;
    const __amdgpu_buffer_rsrc_t rsrc = frame_rsrc(reinterpret_cast<const float *>(img), P.frame_stride * 16);
    const unsigned band = (unsigned)P.tiles_per_row * 8u * 16u;

    const int r = it.x + lane;
    // Everything phase B needs is loaded up front (unconditionally, from a clamped index: a load
    // inside a divergent branch is waited for at the branch's end) so it lands during phase A.
    const int rq = valid ? r : 0;
    int my_state = P.rs_state[rq];
    const int my_slot = P.rs_slot[rq];
    // the point from the record slot (rec_base + s P + q, s = the target's slot of host h): no
    // per-residual point index is read
    const int my_point = valid ? W.point_base + (my_slot - W.rec_base - (t < h ? t : t - 1) * W.P) : W.point_base;
    uint8_t flags = P.rs_flags[rq];
    float state_energy = P.rs_energy[rq];
    float new_energy = P.rs_newenergy[rq];
    const float4 my_pd0 = *(const float4 *)(P.pt_data + (size_t)my_point * LDSO_BA_POINT_STRIDE);
    // the point's color[8] and weights[8] (record floats 8..23: one 64-B piece per residual)
    // into this residual's row of the sums table: phase A's pattern lanes read them from LDS at
    // the step that later overwrites the row with the residual's sums (no per-step gathers)
    {
        const float4 *cw = reinterpret_cast<const float4 *>(P.pt_data + (size_t)my_point * LDSO_BA_POINT_STRIDE + 8);
        float4 v[4];
#pragma unroll
        for (int u = 0; u < 4; u++) v[u] = cw[u];
        float *row = lds_sums_w + lane * kSumStride;
#pragma unroll
        for (int u = 0; u < 4; u++) {
            row[4 * u] = v[u].x;
            row[4 * u + 1] = v[u].y;
            row[4 * u + 2] = v[u].z;
            row[4 * u + 3] = v[u].w;
        }
    }
    if (!valid) my_state = LDSO_BA_RES_OOB;
    // marginalisation pass: Jp * delta of fixLinearizationF (Residuals.cc:221-232) from the centre
    // geometry, per residual, before the pattern pixels need it (dot products left to right)
    float jp_dx = 0.f, jp_dy = 0.f, da = 0.f, db = 0.f;
    if constexpr (kMarg) {
#pragma clang fp contract(off)
        const float *dp = P.ad_ht_delta + (size_t)pair * 8;
        da = dp[6];  // delta_a, delta_b of the pair (adHTdeltaF[6], [7])
        db = dp[7];
        Geo gm;
        if (centre_projection(pre, my_pd0.x, my_pd0.y, my_pd0.w, W.calib[0], W.calib[1], W.calib[2], W.calib[3],
                              wM3, hM3, gm)) {
            const float dd = P.pt_data[(size_t)my_point * LDSO_BA_POINT_STRIDE + 5];
            float x6 = 0.f, y6 = 0.f, x4 = 0.f, y4 = 0.f;
#pragma unroll
            for (int i = 0; i < 6; i++) {
                x6 += gm.d_xi_x[i] * dp[i];
                y6 += gm.d_xi_y[i] * dp[i];
            }
#pragma unroll
            for (int i = 0; i < 4; i++) {
                x4 += gm.d_C_x[i] * W.cdelta[i];
                y4 += gm.d_C_y[i] * W.cdelta[i];
            }
            jp_dx = x6 + x4 + gm.d_d_x * dd;
            jp_dy = y6 + y4 + gm.d_d_y * dd;
        }
    }

    // ---------------- phase A: pattern pixels, 8 residuals per step -------------------------
    wave_lds_sync();  // every row's color / weights are in before any lane reads another's
    if constexpr (kImg == 3) {
        *reinterpret_cast<float4 *>(lds_sums_w + kSumsPerWave + 4 * lane) =
            make_float4(my_pd0.x, my_pd0.y, my_pd0.z, __int_as_float(my_state));
        wave_lds_sync();
        phase_a_pieces<kMarg>(lane, lds_terms_w, lds_sums_w, pre, jlimit, my_state, my_pd0, jp_dx, jp_dy, da, db,
                              rsrc, band, wM3, hM3, __builtin_amdgcn_readfirstlane(P.aff_fix));
    } else {
#pragma clang fp contract(off)
        const int g = lane >> 3, sl = lane & 7;
        // staticPattern[8] (Setting.cc:275) offset of this lane's pixel
        const int px = sl == 1 || sl == 6 ? -1 : sl == 2 ? 1 : sl == 3 ? -2 : sl == 5 ? 2 : 0;
        const int py = sl == 0 ? -2 : sl <= 2 ? -1 : sl <= 5 ? 0 : sl == 6 ? 1 : 2;
        const float aff0 = pre[24], aff1 = pre[25], b0 = pre[26];
        float *T = lds_terms_w + g * (kTermQ * 8);
        float *S = lds_sums_w;
        const int nsteps = (jlimit + 7) >> 3;
        const int tpr2 = P.tiles_per_row;

        struct Stage {
            float Ku, Kv, color, weight;
            float iv[12];               // layout 3: the 12 intensities (load12)
            float3 t00, t10, t01, t11;  // layout 1: the four texels
            float jx, jy;               // kMarg: Jp_delta of the residual
            bool gok;
        };
        auto issue = [&](int k, Stage &q) {
            const int j = 8 * k + g;
            const int st = __shfl(my_state, j, kWave);
            const int p = __shfl(my_point, j, kWave);
            const float pu = __shfl(my_pd0.x, j, kWave), pv = __shfl(my_pd0.y, j, kWave),
                        pz = __shfl(my_pd0.z, j, kWave);
            const bool go = j < jlimit && st != LDSO_BA_RES_OOB;
            if constexpr (kMarg) {
                q.jx = __shfl(jp_dx, j, kWave);
                q.jy = __shfl(jp_dy, j, kWave);
            }
            (void)p;
            q.color = S[j * kSumStride + sl];
            q.weight = S[j * kSumStride + 8 + sl];
            const float up = pu + px, vp = pv + py;
            float ptp[3];
#pragma unroll
            for (int i = 0; i < 3; i++)
                ptp[i] = (pre[3 * i] * up + pre[3 * i + 1] * vp + pre[3 * i + 2] * 1.0f) + pre[9 + i] * pz;
            q.Ku = ptp[0] / ptp[2];
            q.Kv = ptp[1] / ptp[2];
            const bool pok = go && q.Ku > 1.1f && q.Kv > 1.1f && q.Ku < wM3 && q.Kv < hM3;
            const unsigned long long m1 = __ballot(pok);
            q.gok = ((m1 >> (8 * g)) & 0xFFull) == 0xFFull;
            // taps of an in-bounds pixel are always addressable; others read around texel (1, 1)
            const int ix = pok ? (int)q.Ku : 1, iy = pok ? (int)q.Kv : 1;
            if constexpr (kImg == 3) {
                load12(rsrc, band, ix, iy, q.iv);
            } else {
                q.t00 = tex(img, tpr2, ix, iy);
                q.t10 = tex(img, tpr2, ix + 1, iy);
                q.t01 = tex(img, tpr2, ix, iy + 1);
                q.t11 = tex(img, tpr2, ix + 1, iy + 1);
            }
        };
        auto consume = [&](int k, const Stage &q) {
            const int j = 8 * k + g;
            bool fin = false;
            float tt[kSums];
            if (q.gok) {
                const int ix = (int)q.Ku, iy = (int)q.Kv;
                const float dx = q.Ku - ix, dy = q.Kv - iy;
                float I, gx, gy;
                if constexpr (kImg == 3) {
                    const float3 s3 = bilin12(q.iv, dx, dy);
                    I = s3.x;
                    gx = s3.y;
                    gy = s3.z;
                } else {
                    const float dxdy = dx * dy;
                    const float w11 = dxdy, w01 = dy - dxdy, w10 = dx - dxdy, w00 = 1 - dx - dy + dxdy;
                    I = w11 * q.t11.x + w01 * q.t01.x + w10 * q.t10.x + w00 * q.t00.x;
                    gx = w11 * q.t11.y + w01 * q.t01.y + w10 * q.t10.y + w00 * q.t00.y;
                    gy = w11 * q.t11.z + w01 * q.t01.z + w10 * q.t10.z + w00 * q.t00.z;
                }
                fin = isfinite(I);
                pixel_terms<kMarg, kImg == 1>(I, gx, gy, q.color, q.weight, aff0, aff1, b0, tt, kMarg ? q.jx : 0.f,
                                   kMarg ? q.jy : 0.f, da, db, (P.aff_fix & 1) != 0, (P.aff_fix & 2) != 0);
            }
            const unsigned long long m2 = __ballot(fin);
            const bool rok = q.gok && ((m2 >> (8 * g)) & 0xFFull) == 0xFFull;
            // two transposition rounds (quantities 0-8, then 9-16): lane sl adds quantity q0 + sl
            // (lane 0 also quantity 8) over the 8 pixels in pattern order
            auto sum8 = [&](int qq, int e) {
                const float4 a = *(const float4 *)&T[e * 8], b = *(const float4 *)&T[e * 8 + 4];
                float sum = 0.0f;
                sum += a.x;
                sum += a.y;
                sum += a.z;
                sum += a.w;
                sum += b.x;
                sum += b.y;
                sum += b.z;
                sum += b.w;
                S[j * kSumStride + qq] = sum;
            };
            if (q.gok) {
#pragma unroll
                for (int e = 0; e < kTermQ; e++) T[e * 8 + sl] = tt[e];
            }
            wave_lds_sync();
            if (rok) {
                sum8(sl, sl);
                if (sl == 0) sum8(8, 8);
            } else if (sl == 0 && j < jlimit) {
                S[j * kSumStride] = -1.0f;  // energy slot: pattern not ok
            }
            wave_lds_sync();
            if (q.gok) {
#pragma unroll
                for (int e = 0; e < kSums - kTermQ; e++) T[e * 8 + sl] = tt[kTermQ + e];
            }
            wave_lds_sync();
            if (rok) sum8(kTermQ + sl, sl);
            wave_lds_sync();
        };
        // ping-pong stages, loads issued unconditionally (a step past the chunk's end has no valid
        // group and reads around texel (1, 1)), so no load result crosses a branch join
        Stage A, B;
        issue(0, A);
        for (int k = 0; k < nsteps; k += 2) {
            issue(k + 1, B);
            consume(k, A);
            issue(k + 2, A);
            consume(k + 1, B);
        }
    }

    // ---------------- phase B: lane per residual ---------------------------------------------
    double energy = 0;
    bool isIN = false, active = false;
    Geo g;
    PhotoSums s;
    if (valid) {
        const int8_t old_state = (int8_t)my_state;
        int8_t new_state = LDSO_BA_RES_OOB;
        float e_wo = -1;
        if (old_state == LDSO_BA_RES_OOB) {
            energy = state_energy;  // linearize returns state_energy; applyRes returns early
            st_nt(P.rec_b + my_slot, make_float2(0.f, __builtin_nanf("")));  // not active
        } else {
            const float4 pd0 = my_pd0;
            const float *Sr = lds_sums_w + lane * kSumStride;
            s.energy = Sr[0];
            s.wJI2 = Sr[1];
            s.JIdx2_00 = Sr[2];
            s.JIdx2_10 = Sr[3];
            s.JIdx2_11 = Sr[4];
            s.JabJIdx_00 = Sr[5];
            s.JabJIdx_01 = Sr[6];
            s.JabJIdx_10 = Sr[7];
            s.JabJIdx_11 = Sr[8];
            s.Jab2_00 = Sr[9];
            s.Jab2_01 = Sr[10];
            s.Jab2_11 = Sr[11];
            s.JI_r0 = Sr[12];
            s.JI_r1 = Sr[13];
            s.Jab_r0 = Sr[14];
            s.Jab_r1 = Sr[15];
            s.rr = Sr[16];
            const bool pat_ok = !(s.energy < 0.0f);
            bool ok = centre_projection(pre, pd0.x, pd0.y, pd0.w, W.calib[0], W.calib[1], W.calib[2], W.calib[3],
                                        wM3, hM3, g);
            // centerProjectedTo: written where projected, kept (not re-read) where not
            float *centre = P.rs_center + r;  // planes: coalesced 4-B stores, whole lines
            const long long cs = P.center_stride;
            if (ok) {
                st_nt(centre, g.Ku);
                st_nt(centre + cs, g.Kv);
                st_nt(centre + 2 * cs, g.new_idepth);
            }
            ok = ok && pat_ok;
            if (!ok) {
                energy = state_energy;  // OOB: return state_energy, NewEnergy untouched
            } else {
                e_wo = s.energy;
                float el = s.energy;
                if (el > th || s.wJI2 < 2) {
                    el = th;
                    new_state = LDSO_BA_RES_OUTLIER;
                } else {
                    new_state = LDSO_BA_RES_IN;
                }
                new_energy = el;
                energy = el;
            }
            // applyRes(true), Residuals.h:70-88 (state_state != OOB here)
            active = (new_state == LDSO_BA_RES_IN);
            flags = active ? (flags | LDSO_BA_FLAG_ACTIVE) : (flags & ~LDSO_BA_FLAG_ACTIVE);
            state_energy = new_energy;
            write_record(P.rec_a + my_slot, P.rec_b + my_slot, active, pd0.w, g, s);
            if (P.fix && active && (flags & LDSO_BA_FLAG_NEW)) {
                // linearizeAll_Reductor relBS (FullSystem.cc:1800-1812)
#pragma clang fp contract(off)
                float pi[3], pr[3];
#pragma unroll
                for (int i = 0; i < 3; i++) {
                    pi[i] = pre[3 * i] * pd0.x + pre[3 * i + 1] * pd0.y + pre[3 * i + 2] * 1.0f;
                    pr[i] = pi[i] + pre[9 + i] * pd0.z;
                }
                const float dx = pi[0] / pi[2] - pr[0] / pr[2], dy = pi[1] / pi[2] - pr[1] / pr[2];
                centre[3 * cs] = 0.01f * sqrtf(dx * dx + dy * dy);
            }
            st_nt(P.rs_state + r, new_state);
            st_nt(P.rs_flags + r, flags);
            st_nt(P.rs_energy + r, state_energy);
            st_nt(P.rs_newenergy + r, new_energy);
        }
        isIN = (new_state == LDSO_BA_RES_IN);
        st_nt(P.rs_newstate + r, new_state);
        st_nt(P.rs_energy_wo + r, e_wo);
    }

    // linearizeAll stats: sum of returned energies (double) and #IN, per chunk
    double esum = energy;
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) esum += __shfl_xor(esum, m, kWave);
    const unsigned long long inmask = __ballot(isIN);
    if (lane == 0) {
        P.item_energy[2 * itemL] = esum;
        P.item_energy[2 * itemL + 1] = (double)__popcll(inmask);
    }
    // the pass's centre geometry inputs of this pair, for the readers of the records after the
    // live precalc has moved on (write_record); by the pair's first chunk, after its real work
    if ((it.y >> 16) && P.geo_snap && lane < kGeoSnap)
        P.geo_snap[(size_t)pair * kGeoSnap + lane] = lane < 12 ? pre[12 + lane] : W.calib[lane - 12];
    if (!P.accumulate) return;
    wave_lds_sync();  // every lane has read its sums: the wave's LDS becomes the operand table
    top_mfma(lds_terms_w, lane, active, g, s, P.top_slab + (size_t)itemL * kTopVals);
}

template <bool kMarg>
void launch_linearize(int img_mode, int nb, hipStream_t st, const LinParams &L, hipEvent_t ev_start = nullptr,
                      hipEvent_t ev_stop = nullptr) {
    if (ev_start) {  // timed: the dispatch itself stamps the events (no separate event packets in the stream)
        if (img_mode == 3)
            hipExtLaunchKernelGGL(k_linearize<3, kMarg>, dim3(nb), dim3(256), kLinLdsBytes, st, ev_start, ev_stop, 0, L);
        else
            hipExtLaunchKernelGGL(k_linearize<1, kMarg>, dim3(nb), dim3(256), kLinLdsBytes, st, ev_start, ev_stop, 0, L);
        return;
    }
    if (img_mode == 3) k_linearize<3, kMarg><<<nb, 256, kLinLdsBytes, st>>>(L);
    else k_linearize<1, kMarg><<<nb, 256, kLinLdsBytes, st>>>(L);
}

}  // namespace
