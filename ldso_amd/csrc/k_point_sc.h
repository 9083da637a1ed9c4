// k_point_sc.h -- the per-point sums and the Schur chunk partials of the pass
// (AccumulatedTopHessian.cc:94-116, AccumulatedSCHessian.cc:24-50).
#pragma once
#include "ba_device.h"

namespace {

// ============================================================================================
// k_point_sc
// ============================================================================================
struct PointParams {
    const int4 *__restrict__ items;  // {pt_begin, count, host, win}
    const WinDev *__restrict__ wins;
    const float *__restrict__ pt_data;
    const int *__restrict__ pt_nres;
    const unsigned long long *__restrict__ pt_tgt;  // [P]: residual targets, 4 bits each, caller order
    const float4 *__restrict__ rec_a;                // [slots] (WinDev::rec_base layout, write_record)
    const float2 *__restrict__ rec_b;
    const float *__restrict__ precalc;               // the pass's pair precalc (centre geometry)
    float *pt_out;                     // [P][12]
    float *sc_slab;
    int n_items;
    int item_base;
    int shift_prior;  // AccumulatedSCHessianSSE::addPoint's shiftPriorToZero (false when marginalising)
    const int *stop;  // ldso_ba_optimize (LinParams::stop)
    int pass;
    // ldso_ba_optimize: blocks [0, n_nid) compute doStepFromBackup's sumNID / numID of window
    // blockIdx.x (point_nid); the point-chunk blocks follow
    double *win_nid;  // [win][2] (ldso_ba_ctx::win_nid)
    int n_nid, nid_chunk;
};

// G += U'^T U' over the upper 4x4 tiles of the (KP x KP) block of one point chunk, whose rows U' carry
// sqrt(HdiF) (k_point_sc): U'^T U' = U^T diag(HdiF) U
// (AccumulatedSCHessianSSE::addPoint's accD/accE/accEB/accHcc/accbc updates, summed by point):
// 16 products per point as 8 packed FMAs on diagonal pairs (after 2 packed weight multiplies),
// e.g. {acc00, acc11} += {ua.x, ua.y} * {ub.x, ub.y} and {acc01, acc10} += {ua.x, ua.y} *
// {ub.y, ub.x}: both operands are natural register pairs (or a swapped one), no broadcast moves.
__device__ __forceinline__ void syrk_tiles(const float *U, int pitch, int nt, int ntiles, int cnt,
                                           float *slab, int tid, int nthreads) {
    for (int tile = tid; tile < ntiles; tile += nthreads) {
        int a = 0, rem = tile;
        while (rem >= nt - a) {
            rem -= nt - a;
            a++;
        }
        const int bb = a + rem;
        typedef float f2 __attribute__((ext_vector_type(2)));
        f2 c[8];
#pragma unroll
        for (int i = 0; i < 8; i++) c[i] = f2{0.f, 0.f};
        const float *pa = U + 4 * a, *pb = U + 4 * bb;
#pragma unroll 4
        for (int p = 0; p < cnt; p++, pa += pitch, pb += pitch) {
            const float4 ua = *(const float4 *)pa;
            const float4 ub = *(const float4 *)pb;
            const f2 a01 = f2{ua.x, ua.y}, a23 = f2{ua.z, ua.w};
            const f2 b01 = {ub.x, ub.y}, b10 = {ub.y, ub.x}, b23 = {ub.z, ub.w}, b32 = {ub.w, ub.z};
            c[0] += a01 * b01;  // (0,0) (1,1)
            c[1] += a01 * b10;  // (0,1) (1,0)
            c[2] += a01 * b23;  // (0,2) (1,3)
            c[3] += a01 * b32;  // (0,3) (1,2)
            c[4] += a23 * b01;  // (2,0) (3,1)
            c[5] += a23 * b10;  // (2,1) (3,0)
            c[6] += a23 * b23;  // (2,2) (3,3)
            c[7] += a23 * b32;  // (2,3) (3,2)
        }
        float acc[16];
        acc[0] = c[0].x, acc[5] = c[0].y, acc[1] = c[1].x, acc[4] = c[1].y;
        acc[2] = c[2].x, acc[7] = c[2].y, acc[3] = c[3].x, acc[6] = c[3].y;
        acc[8] = c[4].x, acc[13] = c[4].y, acc[9] = c[5].x, acc[12] = c[5].y;
        acc[10] = c[6].x, acc[15] = c[6].y, acc[11] = c[7].x, acc[14] = c[7].y;
        float4 *o = (float4 *)(slab + (size_t)tile * 16);
        o[0] = make_float4(acc[0], acc[1], acc[2], acc[3]);
        o[1] = make_float4(acc[4], acc[5], acc[6], acc[7]);
        o[2] = make_float4(acc[8], acc[9], acc[10], acc[11]);
        o[3] = make_float4(acc[12], acc[13], acc[14], acc[15]);
    }
}

__device__ void point_nid(const PointParams &P, int w, float *lds) {
    if (P.stop && P.pass > P.stop[w]) return;
    NidSrc src{};
    src.pt_data = P.pt_data;
    nid_chain(P.wins[w], src, P.win_nid, w, lds, P.nid_chunk);
}

// points per k_point_sc block (one SYRK chunk partial).  128 (both waves gather, half the slab
// partials) measured 28.5 vs 26.5 us with the stitch 0.8 us faster: the SYRK chains double (r4)
constexpr int kScThreads = 128;  // 2 waves: a lane per point gathers, both run the SYRK tiles
static_assert(kScPoints <= kScThreads, "one gathering lane per point");
// residual records per round trip (r4: 3 -> two round trips at N = 7, 27.6 vs 28.3 us; r5: 6 -> one round
// trip, 30.0 vs 27.6 us with 48-B records, 30.6 vs 25.9 us with 24-B records)
constexpr int kScBatch = 3;
__global__ __launch_bounds__(kScThreads) void k_point_sc(PointParams P) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    if ((int)blockIdx.x < P.n_nid) {
        point_nid(P, blockIdx.x, smem);
        return;
    }
    const int item = P.item_base + blockIdx.x - P.n_nid;
    const int4 it = P.items[item];
    if (P.stop && P.pass > P.stop[it.w]) return;  // window left the GN loop
    const WinDev &W = P.wins[it.w];
    const int host = it.z, KP = W.KP, nt = KP / 4, ntiles = W.ntiles;
    const int Kj = 8 * (W.N - 1);
    // rows of KP + 4 floats: KP is a multiple of 8, so a pitch of 4 mod 8 dwords spreads the lanes'
    // 16-B row accesses (a lane per point) over distinct bank slots (ds_write_b128: 8-lane groups,
    // banks mod 32; ds_read_b128: 16-lane groups, banks mod 64); a pitch of KP put lanes q and q + 4
    // (writes) or q and q + 24 (reads) on the same banks
    const int KPP = KP + 4;
    float *U = smem;               // [kScPoints][KPP]
    const int tid = threadIdx.x;
    // this lane's point and its first records are requested before the block waits for the
    // precalc staging below, so those round trips overlap (unconditional loads from a clamped index)
    const bool mine = tid < it.y;
    const int p = it.x + (mine ? tid : 0);
    const int nres = P.pt_nres[p];
    const unsigned long long tgs = P.pt_tgt[p];
    const float4 pd0 = *reinterpret_cast<const float4 *>(P.pt_data + (size_t)p * LDSO_BA_POINT_STRIDE);
    const float2 pd1 = *reinterpret_cast<const float2 *>(P.pt_data + (size_t)p * LDSO_BA_POINT_STRIDE + 4);
    const size_t rp = (size_t)W.rec_base + (p - W.point_base), sstride = (size_t)W.P;
    float4 ra[kScBatch];
    float2 rb[kScBatch];
    auto load_batch = [&](int k0) {  // records k0 .. k0 + kScBatch - 1 (clamped to the point's last)
#pragma unroll
        for (int u = 0; u < kScBatch; u++) {
            const int k = max(0, min(k0 + u, nres - 1));
            const int tg = (int)((tgs >> (4 * k)) & 15ull);
            const size_t q = rp + (nres > 0 ? (tg < host ? tg : tg - 1) : 0) * sstride;
            ra[u] = P.rec_a[q];
            rb[u] = P.rec_b[q];
        }
    };
    load_batch(0);
    // the host's pair precalc R0 / t0 (record floats 12..23) for every target, staged once per block:
    // every residual's centre geometry reads them from LDS (kPrePitch floats per target)
    float *pre_lds = smem + kScPoints * KPP;
    for (int e = tid; e < W.N * 12; e += blockDim.x) {
        const int t = e / 12, k = e - 12 * t;
        pre_lds[t * kPrePitch + k] = P.precalc[(size_t)(W.pair_base + host + W.N * t) * LDSO_BA_PRECALC_STRIDE + 12 + k];
    }
    __syncthreads();
    if (mine) {
#pragma clang fp contract(off)
        // the sums in residual order exactly as AccumulatedTopHessian.cc:94-116 adds them
        float hdd = 0, bd = 0, hcd[4] = {0, 0, 0, 0};
        int ngood = 0;
        float *row = U + tid * KPP;
        unsigned filled = 0;  // target slots whose JpJdF is in the row
        for (int k0 = 0; k0 < nres; k0 += kScBatch) {
            if (k0) load_batch(k0);
#pragma unroll
            for (int u = 0; u < kScBatch; u++) {
                const int k = k0 + u;
                if (k >= nres || rb[u].y != rb[u].y) continue;  // NaN idepth: not active
                ngood++;
                const int tg = (int)((tgs >> (4 * k)) & 15ull);
                // the residual's centre geometry, as k_linearize's phase B formed it (same inputs,
                // same statements), then point_terms' Hdd_r / Hcd_r from its (j0, j1)
                Geo g;
                (void)centre_projection(pre_lds + tg * kPrePitch - 12,  // R0 = [12..20], t0 = [21..23]
                                        pd0.x, pd0.y, pd0.w, W.calib[0], W.calib[1], W.calib[2], W.calib[3], W.wM3,
                                        W.hM3, g);
                const float4 ja = ra[u];
                float jp[6];
                record_jp6(g, ja.x, ja.y, jp);
                bd += rb[u].x;
                hdd += ja.x * g.d_d_x + ja.y * g.d_d_y;
#pragma unroll
                for (int i = 0; i < 4; i++) hcd[i] += g.d_C_x[i] * ja.x + g.d_C_y[i] * ja.y;
                const int slot = tg < host ? tg : tg - 1;
                *(float4 *)(row + 8 * slot) = make_float4(jp[0], jp[1], jp[2], jp[3]);
                *(float4 *)(row + 8 * slot + 4) = make_float4(jp[4], jp[5], ja.z, ja.w);
                filled |= 1u << slot;
            }
        }
        {  // the rest of the row: zeros (the SYRK reads every column of the point's row)
            const float4 z = make_float4(0.f, 0.f, 0.f, 0.f);
            for (int sl = 0; sl < W.N - 1; sl++)
                if (!((filled >> sl) & 1u)) {
                    *(float4 *)(row + 8 * sl) = z;
                    *(float4 *)(row + 8 * sl + 4) = z;
                }
            for (int c = Kj; c < KP; c++) row[c] = 0.f;
        }
        const float priorF = pd1.x, deltaF = pd1.y;
        float HdiF = 0, bdSum = 0, ih = 0;
        if (ngood > 0) {
            // AccumulatedSCHessian.cc:24-33 (Hdd_accLF = bd_accLF = Hcd_accLF = 0 in the hot path)
            float H = hdd + 0.0f + priorF;
            if (H < 1e-10f) H = 1e-10f;
            ih = H;
            HdiF = (float)(1.0 / (double)H);
            bdSum = bd + 0.0f;
            if (P.shift_prior) bdSum += priorF * deltaF;
            row[Kj + 0] = hcd[0] + 0.0f;
            row[Kj + 1] = hcd[1] + 0.0f;
            row[Kj + 2] = hcd[2] + 0.0f;
            row[Kj + 3] = hcd[3] + 0.0f;
            row[Kj + 4] = bdSum;
        }
        {
            const float sw = sqrtf(HdiF);
            float4 *r4 = reinterpret_cast<float4 *>(row);
            for (int q = 0; q < (Kj + 5 + 3) / 4; q++) {
                float4 v = r4[q];
                v.x *= sw;
                v.y *= sw;
                v.z *= sw;
                v.w *= sw;
                r4[q] = v;
            }
        }
        float *o = P.pt_out + (size_t)p * 12;
        o[0] = HdiF;
        o[1] = bdSum;
        o[2] = ih;
        o[3] = hdd;
        o[4] = bd;
        o[5] = hcd[0];
        o[6] = hcd[1];
        o[7] = hcd[2];
        o[8] = hcd[3];
        o[9] = (float)ngood;
    }
    __syncthreads();
    // symmetric rank-k update of the upper 4x4 tiles: G += U^T diag(HdiF) U
    float *slab = P.sc_slab + W.sc_slab_base + (size_t)(item - W.sc_item_base) * ntiles * 16;
    syrk_tiles(U, KPP, nt, ntiles, it.y, slab, tid, blockDim.x);
}

}  // namespace
