// k_ct_init.h -- CoarseInitializer::trackFrame (CoarseInitializer.cc:45-183) in one launch:
//   k_ct_init_track    one workgroup of four wavefronts walks the levels and the LM iterations.  Every
//                      phase is a loop over the level's points, i = lane, lane + 256, ...: calcResAndGS's
//                      three passes fused into two (init_eval), doStep, applyStep, calcEC, optReg,
//                      resetPoints, propagateDown / Up; lane 0 runs ct_init.h's decisions between them.
//                      The only synchronisation is __syncthreads() and the kernel boundary; every loop is
//                      bounded by a point count, a rank count, max_iterations or the level count.
//   k_ct_init_eval     one init_eval at a given pose (ldso_ct_init_eval): the same text, the same sums.
//   k_ct_init_opt_reg  optReg alone (ldso_ct_init_opt_reg).
// The points stay in global memory (L2-resident: about 10^4 records of 112 bytes a level at VGA); a
// workgroup's waves share their CU's vector cache, so a barrier orders one phase's stores before the
// next phase's loads.
// The sum tree (the same in the loop and in ldso_ct_init_eval): a lane adds its points in index order,
// each good point's 45 acc9 entries first summed over its eight pattern pixels in pattern order; a wave
// folds its 64 lanes with the xor tree v += shfl_xor(v, m), m = 32 ... 1; the four waves are added as
// ((w0 + w1) + w2) + w3.  All in float, contraction off: repeatable, and any order's error bound holds.
// The three traps:
//   optReg (:547-565) and the top level's resetPoints (:747-758) are sequential in-place sweeps.  They run
//     rank by rank over the order ldso_ct_init_set_first computed, a barrier between ranks: two points of a
//     rank are never neighbours of each other, a point's earlier neighbours have lower ranks, its later
//     ones higher ranks.  isGood only removes reads.  The median is the nnn/2-th order statistic, found by
//     counting (ties by position), so no private array is indexed at run time.
//   The pattern loop (:419-483) runs its eight pixels in order and updates maxstep before the next pixel's
//     bounds check can break: a point that leaves the image at pixel k keeps the minimum over 0 .. k-1.
//   propagateUp (:586-593) adds iR * lastHessian into a parent in child order: one lane per parent walks
//     the parent's children, grouped at set_first in ascending order.
#pragma once
#include <cstdint>

#include "ct_init.h"
#include "k_ct_pyramid.h"

#pragma clang fp contract(off)

namespace {

constexpr int kInitThreads = kCtThreads;  // four wavefronts, one per SIMD
constexpr int kInitWaves = kInitThreads / kWave;
constexpr int kInitSums = 47;  // acc9's 45 entries | accE | accEAlpha
static_assert(kInitWaves == 4, "the sum tree adds four waves");

struct CtInitLevel {
    ldso_ct_init_point *pts;
    const float4 *ref, *img;       // firstFrame->dIp[lvl], newFrame->dIp[lvl]
    const int *order, *rank_off;   // the sweep: points by (rank, index); [n_ranks + 1]
    const int *child_off, *child;  // [n + 1]; the points of the level below, grouped by parent, ascending
    int n, n_ranks, wl, hl;
    float fxl, fyl, cxl, cyl;
    double Ki[9];
};
struct CtInitOut {  // mapped host memory
    ldso_ct_init_result R;
    float H[64], b[8], Hsc[64], bsc[8], res[3];
    int alpha_capped, jb_cur, n_eval;
    long long ticks[4];  // wall_clock64 counts of lane 0: evaluations | rank sweeps | the other point phases | lane 0's decisions
};
struct CtInitParams {
    CtInitLevel lv[ldso_ct::kInitMaxLevels];
    ldso_ct_init_params p;
    float *jb[2];  // JbBuffer / JbBuffer_new: [max n][10] each; jb_cur is JbBuffer
    int jb_cur, levels;
    double this_to_next[12];
    float aff[2], aff_guess;
    int have_guess, snapped, frame_id, snapped_at;
    CtInitOut *out;
    ldso_ct_init_step *trace;
    int trace_capacity;
    // k_ct_init_eval / k_ct_init_opt_reg
    int arg_lvl;
    double arg_pose[12];
    float arg_aff[2], arg_reg_weight;
};
struct CtInitShared {
    ldso_ct::InitEval E;
    float sums[kInitSums], sums_sc[45], red[kInitWaves][kInitSums];
    float Hn[64], bn[8], Hscn[64], bscn[8], resn[3];  // the last evaluation
    float alphaOpt;
    int capped;
    float H[64], b[8], Hsc[64], bsc[8], res_old[3], latest_res[3];
    ldso_ct::Pose cur, cand;
    double cur_pose[12], eval_pose[12];
    float aff_cur[2], aff_new[2], eval_aff[2];
    float lambda, lambda_step, inc[8], reg[3];
    int iteration, fails, accept, quit, snapped, jb_cur, n_eval, iters[5];
    long long ticks[4], t_last;
    ldso_ct::LdltWorkF W;
};
enum : int { kInitTickEval, kInitTickSweep, kInitTickPoints, kInitTickLane0 };

// lane 0's clock: the time since the last call goes to `slot` (every phase ends with a barrier, so lane 0's
// time is the workgroup's)
__device__ __forceinline__ void init_tick(CtInitShared &S, int tid, int slot) {
    if (tid == 0) {
        const long long now = wall_clock64();
        S.ticks[slot] += now - S.t_last;
        S.t_last = now;
    }
}

__device__ __forceinline__ int init_tri(int r, int c) {  // acc9's entry (r <= c) in SSEData's order
    return r * 9 - r * (r - 1) / 2 + (c - r);
}

// v [N] per lane -> out [N], the tree of the header; every lane of the workgroup calls it
template <int N>
__device__ __forceinline__ void init_block_sum(float (&v)[N], float (*red)[kInitSums], float *out, int tid) {
    const int lane = tid & (kWave - 1), wv = tid / kWave;
#pragma unroll
    for (int k = 0; k < N; k++) {
        float x = v[k];
#pragma unroll
        for (int m = 32; m >= 1; m >>= 1) x = x + __shfl_xor(x, m, kWave);
        if (lane == 0) red[wv][k] = x;
    }
    __syncthreads();
    if (tid < N) out[tid] = ((red[0][tid] + red[1][tid]) + red[2][tid]) + red[3][tid];
    __syncthreads();
}

// calculateAllResiduals (:391-518) and calculateAlphaEnergy (:376-389) for point i: the point's _new
// fields, maxstep and JbBuffer_new [0, 10); acc9's terms into acc [0, 45), accE's into acc [45], accEAlpha's
// into acc [46]
__device__ __forceinline__ void init_point_residuals(const CtInitLevel &L, const ldso_ct::InitEval &E,
                                                     const ldso_ct_init_params &p, float *jbn, int i,
                                                     float (&acc)[kInitSums]) {
    ldso_ct_init_point &pt = L.pts[i];
    if (!pt.is_good) {
        pt.maxstep = 1e10f;
        const float e0 = pt.energy[0], e1 = pt.energy[1];
        acc[45] = acc[45] + e0;
        pt.energy_new[0] = e0;
        pt.energy_new[1] = e1;
        pt.is_good_new = 0;
        acc[46] = acc[46] + e1;
        return;
    }
    const float pu = pt.u, pv = pt.v, idn = pt.idepth_new;
    float hp[45], jb[10];
#pragma unroll
    for (int k = 0; k < 45; k++) hp[k] = 0;
#pragma unroll
    for (int k = 0; k < 10; k++) jb[k] = 0;
    float ms = 1e10f, energy = 0;
    bool good = true;
    const float *RKi = E.RKi, *t = E.t;
#pragma nounroll
    for (int idx = 0; idx < 8; idx++) {
        // staticPattern[8] (Setting.cc:275): dx = {0, -1, 1, -2, 0, 2, -1, 0}, dy = {-2, -1, -1, 0, 0, 0, 1, 2}
        const int dx = (int)((0x0F20E1F0u >> (4 * idx)) & 15u) - ((0x0F20E1F0u >> (4 * idx)) & 8u ? 16 : 0);
        const int dy = (int)((0x21000FFEu >> (4 * idx)) & 15u) - ((0x21000FFEu >> (4 * idx)) & 8u ? 16 : 0);
        const float x = pu + dx, y = pv + dy;
        float P[3];
#pragma unroll
        for (int k = 0; k < 3; k++) P[k] = (RKi[3 * k] * x + RKi[3 * k + 1] * y + RKi[3 * k + 2] * 1) + t[k] * idn;
        const float u = P[0] / P[2], v = P[1] / P[2];
        const float Ku = L.fxl * u + L.cxl, Kv = L.fyl * v + L.cyl;
        const float new_idepth = idn / P[2];
        if (!(Ku > 1 && Kv > 1 && Ku < L.wl - 2 && Kv < L.hl - 2 && new_idepth > 0)) {
            good = false;
            break;
        }
        float h0, h1, h2, rlR;
        {  // getInterpolatedElement33 (GlobalFuncs.h:89-103) of the new frame
            const int ix = (int)Ku, iy = (int)Kv;
            const float ddx = Ku - ix, ddy = Kv - iy, dxdy = ddx * ddy;
            const float4 *bp = L.img + ix + (size_t)iy * L.wl;
            const float4 t11 = bp[1 + L.wl], t01 = bp[L.wl], t10 = bp[1], t00 = bp[0];
            const float w11 = dxdy, w01 = ddy - dxdy, w10 = ddx - dxdy, w00 = 1 - ddx - ddy + dxdy;
            h0 = w11 * t11.x + w01 * t01.x + w10 * t10.x + w00 * t00.x;
            h1 = w11 * t11.y + w01 * t01.y + w10 * t10.y + w00 * t00.y;
            h2 = w11 * t11.z + w01 * t01.z + w10 * t10.z + w00 * t00.z;
        }
        {  // getInterpolatedElement31 (GlobalFuncs.h:145-159) of the first frame; set_first checked u, v
            const int ix = (int)x, iy = (int)y;
            const float ddx = x - ix, ddy = y - iy, dxdy = ddx * ddy;
            const float4 *bp = L.ref + ix + (size_t)iy * L.wl;
            rlR = dxdy * bp[1 + L.wl].x + (ddy - dxdy) * bp[L.wl].x + (ddx - dxdy) * bp[1].x +
                  (1 - ddx - ddy + dxdy) * bp[0].x;
        }
        if (!isfinite(rlR) || !isfinite(h0)) {
            good = false;
            break;
        }
        const float residual = h0 - E.r2a * rlR - E.r2b;
        float hw = fabsf(residual) < p.huber_th ? 1 : p.huber_th / fabsf(residual);
        energy = energy + hw * residual * residual * (2 - hw);
        const float dxdd = (t[0] - t[2] * u) / P[2];
        const float dydd = (t[1] - t[2] * v) / P[2];
        if (hw < 1) hw = sqrtf(hw);
        const float dxInterp = hw * h1 * L.fxl;
        const float dyInterp = hw * h2 * L.fyl;
        float J[9];
        J[0] = new_idepth * dxInterp;
        J[1] = new_idepth * dyInterp;
        J[2] = -new_idepth * (u * dxInterp + v * dyInterp);
        J[3] = -u * v * dxInterp - (1 + v * v) * dyInterp;
        J[4] = (1 + u * u) * dxInterp + u * v * dyInterp;
        J[5] = -v * dxInterp + u * dyInterp;
        J[6] = -hw * E.r2a * rlR;
        J[7] = -hw * 1;
        J[8] = hw * residual;
        const float dd = dxInterp * dxdd + dyInterp * dydd;
        const float sx = dxdd * L.fxl, sy = dydd * L.fyl;
        const float maxstep = 1.0f / sqrtf(sx * sx + sy * sy);
        if (maxstep < ms) ms = maxstep;
#pragma unroll
        for (int k = 0; k < 9; k++) jb[k] = jb[k] + J[k] * dd;
        jb[9] = jb[9] + dd * dd;
#pragma unroll
        for (int r = 0; r < 9; r++)
#pragma unroll
            for (int c = r; c < 9; c++) hp[init_tri(r, c)] = hp[init_tri(r, c)] + J[r] * J[c];
    }
    pt.maxstep = ms;
    float *o = jbn + 10 * (size_t)i;
#pragma unroll
    for (int k = 0; k < 10; k++) o[k] = jb[k];
    if (!good || energy > pt.outlier_th * 20) {
        const float e0 = pt.energy[0], e1 = pt.energy[1];
        acc[45] = acc[45] + e0;
        pt.is_good_new = 0;
        pt.energy_new[0] = e0;
        pt.energy_new[1] = e1;
        acc[46] = acc[46] + e1;
        return;
    }
    acc[45] = acc[45] + energy;
    pt.is_good_new = 1;
    pt.energy_new[0] = energy;
#pragma unroll
    for (int k = 0; k < 45; k++) acc[k] = acc[k] + hp[k];
    const float e1 = (idn - 1) * (idn - 1);
    pt.energy_new[1] = e1;
    acc[46] = acc[46] + e1;
}

// calculateSC (:349-374) for point i; Accumulator9::updateSingleWeighted's terms into acc [0, 45)
__device__ __forceinline__ void init_point_sc(const CtInitLevel &L, const ldso_ct_init_params &p, float alphaOpt,
                                              float *jbn, int i, float (&acc)[45]) {
    ldso_ct_init_point &pt = L.pts[i];
    if (!pt.is_good_new) return;
    float *jb = jbn + 10 * (size_t)i;
    float J[9];
#pragma unroll
    for (int k = 0; k < 8; k++) J[k] = jb[k];
    float j8 = jb[8], j9 = jb[9];
    pt.last_hessian_new = j9;
    const float idn = pt.idepth_new;
    j8 = j8 + alphaOpt * (idn - 1);
    j9 = j9 + alphaOpt;
    if (alphaOpt == 0) {
        j8 = j8 + p.coupling_weight * (idn - pt.ir);
        j9 = j9 + p.coupling_weight;
    }
    j9 = 1 / (1 + j9);
    jb[8] = j8;
    jb[9] = j9;
    J[8] = j8;
    const float w = j9;
#pragma unroll
    for (int r = 0; r < 9; r++) {
        acc[init_tri(r, r)] = acc[init_tri(r, r)] + J[r] * J[r] * w;
        J[r] = J[r] * w;
#pragma unroll
        for (int c = r + 1; c < 9; c++) acc[init_tri(r, c)] = acc[init_tri(r, c)] + J[c] * J[r];
    }
}

// calcResAndGS (:186-342) at the pose S.E describes: S.Hn, bn, Hscn, bscn, resn, alphaOpt, capped
__device__ __forceinline__ void init_eval(const CtInitLevel &L, const ldso_ct_init_params &p, CtInitShared &S, float *jbn,
                                          int tid) {
    {
        float acc[kInitSums];
#pragma unroll
        for (int k = 0; k < kInitSums; k++) acc[k] = 0;
        for (int i = tid; i < L.n; i += kInitThreads) init_point_residuals(L, S.E, p, jbn, i, acc);
        init_block_sum<kInitSums>(acc, S.red, S.sums, tid);
    }
    if (tid == 0) {
        S.alphaOpt = ldso_ct::init_alpha(S.E.tsq, S.sums[46], L.n, p, S.resn[1]);
        S.capped = S.alphaOpt == 0;
        S.resn[0] = S.sums[45];
        S.resn[2] = (float)L.n;  // accE[0].num: every point adds once
    }
    __syncthreads();
    const float alphaOpt = S.alphaOpt;
    {
        float acc[45];
#pragma unroll
        for (int k = 0; k < 45; k++) acc[k] = 0;
        for (int i = tid; i < L.n; i += kInitThreads) init_point_sc(L, p, alphaOpt, jbn, i, acc);
        init_block_sum<45>(acc, S.red, S.sums_sc, tid);
    }
    if (tid < 64) {  // Accumulator9::finish: both triangles
        const int r = tid / 8, c = tid % 8;
        const int k = init_tri(r < c ? r : c, r < c ? c : r);
        S.Hn[tid] = S.sums[k];
        S.Hscn[tid] = S.sums_sc[k];
    } else if (tid < 72) {
        S.bn[tid - 64] = S.sums[init_tri(tid - 64, 8)];
        S.bscn[tid - 64] = S.sums_sc[init_tri(tid - 64, 8)];
    }
    __syncthreads();
    if (tid == 0) {  // :332-339
        const float an = alphaOpt * L.n;
        for (int k = 0; k < 3; k++) {
            S.Hn[9 * k] = S.Hn[9 * k] + an;
            S.bn[k] = S.bn[k] + S.E.tlog[k] * alphaOpt * L.n;
        }
    }
    __syncthreads();
}

// the k-th smallest (k counted from 0) of the valid entries among ten, without indexing at run time
__device__ __forceinline__ float init_order_stat(const float (&val)[10], unsigned valid, int k) {
    float out = 0;
#pragma unroll
    for (int j = 0; j < 10; j++) {
        int below = 0;
#pragma unroll
        for (int m = 0; m < 10; m++)
            if (m != j && (valid >> m & 1u) && (val[m] < val[j] || (val[m] == val[j] && m < j))) below++;
        if ((valid >> j & 1u) && below == k) out = val[j];
    }
    return out;
}

// optReg (:538-567)
__device__ __forceinline__ void init_opt_reg(const CtInitLevel &L, float regWeight, int snapped, int tid) {
    ldso_ct_init_point *pts = L.pts;
    if (!snapped) {
        for (int i = tid; i < L.n; i += kInitThreads) pts[i].ir = 1;
        __syncthreads();
        return;
    }
    for (int r = 0; r < L.n_ranks; r++) {
        const int end = L.rank_off[r + 1];
        for (int k = L.rank_off[r] + tid; k < end; k += kInitThreads) {
            ldso_ct_init_point &pt = pts[L.order[k]];
            if (!pt.is_good) continue;
            float val[10];
            unsigned valid = 0;
            int nnn = 0;
#pragma unroll
            for (int j = 0; j < 10; j++) {
                const int nb = pt.neighbours[j];
                val[j] = 0;
                if (nb == -1) continue;
                if (!pts[nb].is_good) continue;
                val[j] = pts[nb].ir;
                valid |= 1u << j;
                nnn++;
            }
            if (nnn > 2) pt.ir = (1 - regWeight) * pt.idepth + regWeight * init_order_stat(val, valid, nnn / 2);
        }
        __syncthreads();
    }
}

// resetPoints (:739-761)
__device__ __forceinline__ void init_reset_points(const CtInitLevel &L, bool top, int tid) {
    ldso_ct_init_point *pts = L.pts;
    for (int i = tid; i < L.n; i += kInitThreads) {
        pts[i].energy[0] = 0;
        pts[i].energy[1] = 0;
        pts[i].idepth_new = pts[i].idepth;
    }
    __syncthreads();
    if (!top) return;
    for (int r = 0; r < L.n_ranks; r++) {
        const int end = L.rank_off[r + 1];
        for (int k = L.rank_off[r] + tid; k < end; k += kInitThreads) {
            ldso_ct_init_point &pt = pts[L.order[k]];
            if (pt.is_good) continue;
            float snd = 0, sn = 0;
#pragma unroll
            for (int j = 0; j < 10; j++) {
                const int nb = pt.neighbours[j];
                if (nb == -1 || !pts[nb].is_good) continue;
                snd = snd + pts[nb].ir;
                sn = sn + 1;
            }
            if (sn > 0) {
                pt.is_good = 1;
                pt.ir = pt.idepth = pt.idepth_new = snd / sn;
            }
        }
        __syncthreads();
    }
}

// propagateDown (:606-631): Lp the source level, L the level below it
__device__ __forceinline__ void init_propagate_down(const CtInitLevel &Lp, const CtInitLevel &L, float regWeight,
                                                    int snapped, int tid) {
    for (int i = tid; i < L.n; i += kInitThreads) {
        ldso_ct_init_point &pt = L.pts[i];
        const ldso_ct_init_point &parent = Lp.pts[pt.parent];
        if (!parent.is_good || parent.last_hessian < 0.1) continue;
        if (!pt.is_good) {
            pt.ir = pt.idepth = pt.idepth_new = parent.ir;
            pt.is_good = 1;
            pt.last_hessian = 0;
        } else {
            const float newiR = (pt.ir * pt.last_hessian * 2 + parent.ir * parent.last_hessian) /
                                (pt.last_hessian * 2 + parent.last_hessian);
            pt.ir = pt.idepth = pt.idepth_new = newiR;
        }
    }
    __syncthreads();
    init_opt_reg(L, regWeight, snapped, tid);
}

// propagateUp (:570-604): L the source level, Lp the level above it
__device__ __forceinline__ void init_propagate_up(const CtInitLevel &L, const CtInitLevel &Lp, float regWeight,
                                                  int snapped, int tid) {
    for (int i = tid; i < Lp.n; i += kInitThreads) {
        ldso_ct_init_point &parent = Lp.pts[i];
        float iR = 0, sum = 0;
        const int end = Lp.child_off[i + 1];
        for (int k = Lp.child_off[i]; k < end; k++) {
            const ldso_ct_init_point &pt = L.pts[Lp.child[k]];
            if (!pt.is_good) continue;
            iR = iR + pt.ir * pt.last_hessian;
            sum = sum + pt.last_hessian;
        }
        parent.ir = iR;
        parent.ir_sum_num = sum;
        if (sum > 0) {
            parent.idepth = parent.ir = (iR / sum);
            parent.is_good = 1;
        }
    }
    __syncthreads();
    init_opt_reg(Lp, regWeight, snapped, tid);
}

// doStep (:763-789)
__device__ __forceinline__ void init_do_step(const CtInitLevel &L, const float *jbuf, float lambda, const float *inc,
                                             int tid) {
    const float maxPixelStep = 0.25f, idMaxStep = 1e10f;
    float in[8];
#pragma unroll
    for (int k = 0; k < 8; k++) in[k] = inc[k];
    for (int i = tid; i < L.n; i += kInitThreads) {
        ldso_ct_init_point &pt = L.pts[i];
        if (!pt.is_good) continue;
        const float *jb = jbuf + 10 * (size_t)i;
        float j[8];
#pragma unroll
        for (int k = 0; k < 8; k++) j[k] = jb[k];
        const float b = jb[8] + ldso_ct::init_dot8(j, in);
        float step = -b * jb[9] / (1 + lambda);
        float maxstep = maxPixelStep * pt.maxstep;
        if (maxstep > idMaxStep) maxstep = idMaxStep;
        if (step > maxstep) step = maxstep;
        if (step < -maxstep) step = -maxstep;
        float newIdepth = pt.idepth + step;
        if (newIdepth < 1e-3f) newIdepth = 1e-3f;
        if (newIdepth > 50) newIdepth = 50;
        pt.idepth_new = newIdepth;
    }
    __syncthreads();
}

// applyStep (:791-809)
__device__ __forceinline__ void init_apply_step(const CtInitLevel &L, CtInitShared &S, int tid) {
    for (int i = tid; i < L.n; i += kInitThreads) {
        ldso_ct_init_point &pt = L.pts[i];
        if (!pt.is_good) {
            pt.idepth = pt.idepth_new = pt.ir;
            continue;
        }
        pt.energy[0] = pt.energy_new[0];
        pt.energy[1] = pt.energy_new[1];
        pt.is_good = pt.is_good_new;
        pt.idepth = pt.idepth_new;
        pt.last_hessian = pt.last_hessian_new;
    }
    __syncthreads();
    if (tid == 0) S.jb_cur ^= 1;  // std::swap(JbBuffer, JbBuffer_new)
    __syncthreads();
}

// calcEC (:520-536) -> S.reg
__device__ __forceinline__ void init_calc_ec(const CtInitLevel &L, const ldso_ct_init_params &p, CtInitShared &S, int tid) {
    if (!S.snapped) {
        if (tid == 0) {
            S.reg[0] = 0;
            S.reg[1] = 0;
            S.reg[2] = (float)L.n;
        }
        __syncthreads();
        return;
    }
    float acc[3] = {0, 0, 0};
    for (int i = tid; i < L.n; i += kInitThreads) {
        const ldso_ct_init_point &pt = L.pts[i];
        if (!pt.is_good_new) continue;
        const float rOld = (pt.idepth - pt.ir), rNew = (pt.idepth_new - pt.ir);
        acc[0] = acc[0] + rOld * rOld;
        acc[1] = acc[1] + rNew * rNew;
        acc[2] = acc[2] + 1;
    }
    init_block_sum<3>(acc, S.red, S.sums_sc, tid);
    if (tid == 0) {
        S.reg[0] = p.coupling_weight * S.sums_sc[0];
        S.reg[1] = p.coupling_weight * S.sums_sc[1];
        S.reg[2] = S.sums_sc[2];
    }
    __syncthreads();
}

// ---- lane 0 between the phases ------------------------------------------------------------------------
__device__ inline void init_set_eval(const CtInitLevel &L, CtInitShared &S, bool cand) {
    if (cand)
        ldso_ct::pose_matrix(S.cand, S.eval_pose);
    else
        for (int i = 0; i < 12; i++) S.eval_pose[i] = S.cur_pose[i];
    for (int i = 0; i < 2; i++) S.eval_aff[i] = cand ? S.aff_new[i] : S.aff_cur[i];
    ldso_ct::init_eval_setup(S.eval_pose, S.eval_aff, L.Ki, S.E);
}
__device__ inline void init_log(const CtInitParams &P, CtInitShared &S, int lvl, int iteration, bool accept) {
    if (P.trace && S.n_eval < P.trace_capacity) {
        ldso_ct_init_step &s = P.trace[S.n_eval];
        for (int i = 0; i < 12; i++) s.pose[i] = S.eval_pose[i];
        for (int i = 0; i < 2; i++) s.aff[i] = S.eval_aff[i];
        s.lvl = lvl;
        s.iteration = iteration;
        s.accepted = accept ? 1 : 0;
        s.alpha_capped = S.capped;
        s.snapped = S.snapped;
        s.lambda = iteration < 0 ? 0.0f : S.lambda_step;
        for (int i = 0; i < 8; i++) s.inc[i] = iteration < 0 ? 0.0f : S.inc[i];
        for (int i = 0; i < 3; i++) {
            s.res[i] = S.resn[i];
            s.reg_energy[i] = iteration < 0 ? 0.0f : S.reg[i];
        }
    }
    S.n_eval++;
}
__device__ inline void init_next_step(const CtInitParams &P, CtInitShared &S, int lvl) {
    const CtInitLevel &L = P.lv[lvl];
    S.lambda_step = S.lambda;
    ldso_ct::init_lm_step(S.H, S.b, S.Hsc, S.bsc, S.lambda, L.wl, L.hl, S.cur, S.aff_cur, P.p, S.W, S.inc, S.cand, S.aff_new);
    init_set_eval(L, S, true);
}
__device__ inline void init_begin(const CtInitParams &P, CtInitShared &S) {
    S.snapped = P.snapped;
    S.jb_cur = P.jb_cur;
    S.n_eval = 0;
    for (int i = 0; i < 12; i++) S.cur_pose[i] = P.this_to_next[i];
    if (!S.snapped) S.cur_pose[3] = S.cur_pose[7] = S.cur_pose[11] = 0;  // thisToNext.translation().setZero()
    S.cur = ldso_ct::init_pose_from_matrix(S.cur_pose);
    S.aff_cur[0] = P.aff[0];
    S.aff_cur[1] = P.aff[1];
    if (P.have_guess) {  // :71-73
        S.aff_cur[0] = P.aff_guess;
        S.aff_cur[1] = 0;
    }
    for (int i = 0; i < 3; i++) S.latest_res[i] = 0;
    for (int i = 0; i < 5; i++) S.iters[i] = 0;
    for (int i = 0; i < 4; i++) S.ticks[i] = 0;
    S.t_last = wall_clock64();
}
__device__ inline void init_level_start(const CtInitParams &P, CtInitShared &S, int lvl) {
    init_set_eval(P.lv[lvl], S, false);
}
// :85-93 after the level's first evaluation
__device__ inline void init_after_first(const CtInitParams &P, CtInitShared &S, int lvl) {
    init_log(P, S, lvl, -1, false);
    for (int i = 0; i < 64; i++) {
        S.H[i] = S.Hn[i];
        S.Hsc[i] = S.Hscn[i];
    }
    for (int i = 0; i < 8; i++) {
        S.b[i] = S.bn[i];
        S.bsc[i] = S.bscn[i];
    }
    for (int i = 0; i < 3; i++) S.res_old[i] = S.resn[i];
    S.lambda = 0.1f;
    S.fails = 0;
    S.iteration = 0;
    init_next_step(P, S, lvl);
}
// :125-165 after a step's evaluation and calcEC
__device__ inline void init_after_step(const CtInitParams &P, CtInitShared &S, int lvl) {
    const CtInitLevel &L = P.lv[lvl];
    const bool accept = ldso_ct::init_accept(S.res_old, S.resn, S.reg);
    if (accept) {
        if (S.resn[1] == P.p.alpha_k * L.n) S.snapped = 1;
        for (int i = 0; i < 64; i++) {
            S.H[i] = S.Hn[i];
            S.Hsc[i] = S.Hscn[i];
        }
        for (int i = 0; i < 8; i++) {
            S.b[i] = S.bn[i];
            S.bsc[i] = S.bscn[i];
        }
        for (int i = 0; i < 3; i++) S.res_old[i] = S.resn[i];
        for (int i = 0; i < 2; i++) S.aff_cur[i] = S.aff_new[i];
        // the accepted pose is the matrix that was evaluated (ct_lm.h's door)
        for (int i = 0; i < 12; i++) S.cur_pose[i] = S.eval_pose[i];
        S.cur = ldso_ct::init_pose_from_matrix(S.cur_pose);
        S.lambda = S.lambda * 0.5f;
        S.fails = 0;
        if (S.lambda < 0.0001f) S.lambda = 0.0001f;
    } else {
        S.fails++;
        S.lambda = S.lambda * 4;
        if (S.lambda > 10000) S.lambda = 10000;
    }
    init_log(P, S, lvl, S.iteration, accept);
    S.accept = accept ? 1 : 0;
    S.iters[lvl]++;
    const float eps = 1e-4f;
    S.quit = (!(ldso_ct::init_norm8(S.inc) > eps) || S.iteration >= P.p.max_iterations[lvl] || S.fails >= 2) ? 1 : 0;
    if (S.quit) {
        for (int i = 0; i < 3; i++) S.latest_res[i] = S.res_old[i];
        return;
    }
    S.iteration++;
    init_next_step(P, S, lvl);
}
// :170-182
__device__ inline void init_finish(const CtInitParams &P, CtInitShared &S) {
    CtInitOut &O = *P.out;
    for (int i = 0; i < 12; i++) O.R.this_to_next[i] = S.cur_pose[i];
    for (int i = 0; i < 2; i++) O.R.this_to_next_aff[i] = S.aff_cur[i];
    for (int i = 0; i < 3; i++) O.R.latest_res[i] = S.latest_res[i];
    int frame_id = P.frame_id + 1, snapped_at = P.snapped_at;
    if (!S.snapped) snapped_at = 0;
    if (S.snapped && snapped_at == 0) snapped_at = frame_id;
    O.R.snapped = S.snapped;
    O.R.frame_id = frame_id;
    O.R.snapped_at = snapped_at;
    O.R.ret = (S.snapped && frame_id > snapped_at + 5) ? 1 : 0;
    for (int i = 0; i < 5; i++) O.R.iterations[i] = S.iters[i];
    O.jb_cur = S.jb_cur;
    O.n_eval = S.n_eval;
    for (int i = 0; i < 4; i++) O.ticks[i] = S.ticks[i];
}

__global__ __launch_bounds__(kInitThreads) void k_ct_init_track(CtInitParams P) {
    __shared__ CtInitShared S;
    const int tid = threadIdx.x;
    if (tid == 0) init_begin(P, S);
    __syncthreads();
    if (!S.snapped) {  // :55-66
        for (int lvl = 0; lvl < P.levels; lvl++) {
            ldso_ct_init_point *pts = P.lv[lvl].pts;
            for (int i = tid; i < P.lv[lvl].n; i += kInitThreads) {
                pts[i].ir = 1;
                pts[i].idepth_new = 1;
                pts[i].last_hessian = 0;
            }
        }
        __syncthreads();
    }
    const float regWeight = P.p.reg_weight;
    init_tick(S, tid, kInitTickPoints);
    for (int lvl = P.levels - 1; lvl >= 0; lvl--) {
        const CtInitLevel &L = P.lv[lvl];
        if (lvl < P.levels - 1) init_propagate_down(P.lv[lvl + 1], L, regWeight, S.snapped, tid);
        init_reset_points(L, lvl == P.levels - 1, tid);
        init_tick(S, tid, kInitTickSweep);
        if (tid == 0) init_level_start(P, S, lvl);
        __syncthreads();
        init_tick(S, tid, kInitTickLane0);
        init_eval(L, P.p, S, P.jb[1 - S.jb_cur], tid);
        init_tick(S, tid, kInitTickEval);
        if (tid == 0) init_after_first(P, S, lvl);
        __syncthreads();
        init_tick(S, tid, kInitTickLane0);
        init_apply_step(L, S, tid);
        for (;;) {
            init_do_step(L, P.jb[S.jb_cur], S.lambda_step, S.inc, tid);
            init_tick(S, tid, kInitTickPoints);
            init_eval(L, P.p, S, P.jb[1 - S.jb_cur], tid);
            init_tick(S, tid, kInitTickEval);
            init_calc_ec(L, P.p, S, tid);
            init_tick(S, tid, kInitTickPoints);
            if (tid == 0) init_after_step(P, S, lvl);
            __syncthreads();
            init_tick(S, tid, kInitTickLane0);
            if (S.accept) {
                init_apply_step(L, S, tid);
                init_tick(S, tid, kInitTickPoints);
                init_opt_reg(L, regWeight, S.snapped, tid);
                init_tick(S, tid, kInitTickSweep);
            }
            if (S.quit) break;
        }
        __syncthreads();
    }
    for (int i = 0; i < P.levels - 1; i++) init_propagate_up(P.lv[i], P.lv[i + 1], regWeight, S.snapped, tid);
    init_tick(S, tid, kInitTickSweep);
    if (tid == 0) init_finish(P, S);
}

__global__ __launch_bounds__(kInitThreads) void k_ct_init_eval(CtInitParams P) {
    __shared__ CtInitShared S;
    const int tid = threadIdx.x;
    const CtInitLevel &L = P.lv[P.arg_lvl];
    if (tid == 0) {
        S.jb_cur = P.jb_cur;
        for (int i = 0; i < 12; i++) S.eval_pose[i] = P.arg_pose[i];
        for (int i = 0; i < 2; i++) S.eval_aff[i] = P.arg_aff[i];
        ldso_ct::init_eval_setup(S.eval_pose, S.eval_aff, L.Ki, S.E);
    }
    __syncthreads();
    init_eval(L, P.p, S, P.jb[1 - S.jb_cur], tid);
    CtInitOut &O = *P.out;
    if (tid < 64) {
        O.H[tid] = S.Hn[tid];
        O.Hsc[tid] = S.Hscn[tid];
    } else if (tid < 72) {
        O.b[tid - 64] = S.bn[tid - 64];
        O.bsc[tid - 64] = S.bscn[tid - 64];
    } else if (tid < 75) {
        O.res[tid - 72] = S.resn[tid - 72];
    } else if (tid == 75) {
        O.alpha_capped = S.capped;
    }
}

__global__ __launch_bounds__(kInitThreads) void k_ct_init_opt_reg(CtInitParams P) {
    init_opt_reg(P.lv[P.arg_lvl], P.arg_reg_weight, P.snapped, threadIdx.x);
}

}  // namespace
