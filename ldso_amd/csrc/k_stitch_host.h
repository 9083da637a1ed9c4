// k_stitch_host.h -- the host stitch (windows of up to kHostStitchMaxN keyframes): k_stitch_host and
// k_stitch_host_sum.
#pragma once
#include "k_stitch.h"

namespace {

// ============================================================================================
// k_stitch_host + k_stitch_host_sum (the default for windows of up to kHostStitchMaxN keyframes):
// one 256-thread block per host frame i of every window stitches everything host i owns --
// the Top pairs (i, t) (AccumulatedTopHessian.cc:213-239) and host i's Schur complement
// (AccumulatedSCHessian.cc:80-114, its targets j, k) -- into a dense packed partial system
// {HA, bA, Hsc, bsc} of the window, and k_stitch_host_sum adds the N partials of every element in
// host order (no atomics: the system is bitwise repeatable).  The terms are k_stitch's, grouped
// by host instead of by pair:
//   HA  (f,f): f == i: sum_t AH_it A_t AH_it^T; else AT_if A_f AT_if^T
//       (f1<f2): f1 == i: AH_i,f2 A AT_i,f2^T; f2 == i: (AH_i,f1 A AT_i,f1^T)^T; else 0
//       (c,f): f == i: sum_t AH_it A_t[8C]; else AT_if A_f[8C]    b(f) likewise, (c,c) / b(c): sum_t
//   Hsc (f,f): f == i: sum_j AH_ij S_j; else AT_if D_ff AT_if^T   with S_j = sum_k D_jk AH_ik^T
//       (f1<f2): i not in {f1,f2}: AT_i,f1 D_f1f2 AT_i,f2^T; f2 == i: AT_i,f1 S_f1; f1 == i: (AT_i,f2 S_f2)^T
//       (c,f) / b(f): f == i: sum_j AH_ij E_j / EB_j; else AT_if E_f / EB_f;  (c,c) / b(c): accHcc / accbc
// where A_t is pair (i,t)'s 13x13 AccumulatorApprox block and D, E, EB, accHcc, accbc the blocks of
// G_i = U^T diag(HdiF) U (k_point_sc's chunk partials summed in double).  Everything host i
// reads is staged in LDS once: G_i (both triangles), the adjoints of the N pairs (i, k), the
// N-1 Top accumulators; then S_j and TH_t = AH_it A_t; then every element of the partial.  Windows
// with more keyframes use k_stitch's records.
//
// The target adjoints.  setAdjointsF builds AT as a diagonal matrix, and the host marks a window
// whose ad_target blocks are all diagonal (WinDev::adt_diag, set wherever ad_target is uploaded).
// For such a window (the diagonal path) only the 8 diagonal entries at_k of every AT_ik are staged
// and every product with an AT factor is the scaled element, left factor first:
//   (AT_j M)[r][c] = at_j[r] M[r][c],   (M AT_k^T)[r][c] = M[r][c] at_k[c]
// each product as fma(a, m, +0), which is what the dense sum of eight terms (seven of them exact
// zeros) rounds to, the sign of a zero included.  The two paths differ only where M holds a
// non-finite entry (the dense sum spreads it over the row, 0 * inf).  Any other window, and every
// window under LDSO_BA_STITCH_DENSE_ADT (StitchParams::dense_adt), takes the dense path: the whole
// AT blocks staged, X_jk = AT_ij D_jk (j <= k) and TT_t = AT_it A_t formed as 8x8 products.  The
// choice is a block-uniform branch on data the block reads, so a captured graph follows an
// ldso_ba_update of the adjoints; the launch always reserves the dense path's LDS.
// ============================================================================================
constexpr int kHostStitchMaxN = 11;
constexpr int kHsThreads = 512;
// the 8x8 blocks in LDS: row r at hs_row(r) (rows 4..7 shifted by two doubles), blocks kHsB = 72
// doubles apart, so the rows {0, 2, 4, 6} a 2x2 task group reads, in a block and in its
// neighbour, fall on distinct bank quads of ds_read_b128's 16-lane groups (dense 8x8 blocks put
// rows r and r + 4, and neighbouring blocks, on the same banks).  Rows r0, r0 + 1 (r0 even) stay
// 8 doubles apart.
constexpr int kHsB = 72;
__device__ __forceinline__ int hs_row(int r) { return 8 * r + ((r & 4) >> 1); }
__host__ __device__ inline int hs_k5(int N) { return 8 * (N - 1) + 5; }
__host__ __device__ inline int hs_ldg(int N) { return (hs_k5(N) + 1) & ~1; }  // even: 16-byte aligned rows
__host__ __device__ inline int hs_npair(int N) { return (N - 1) * N / 2; }
// the block's LDS in doubles (the regions: k_stitch_host); the diagonal path has no X and no TT and
// keeps 8 entries of every AT.  75 KB dense and 56 KB diagonal at N = 7, 154 KB and 111 KB at N = 11.
__host__ __device__ inline size_t hs_lds_doubles(int N, bool diag) {
    const size_t n = (size_t)N;
    return (size_t)hs_k5(N) * hs_ldg(N) + kHsB * n + (diag ? 8 : kHsB) * n + 182 * n +
           (diag ? 0 : kHsB * (size_t)hs_npair(N)) + 2 * kHsB * n + (diag ? 0 : kHsB * n) + 208 * (n - 1);
}
// tile index t of the upper-tile order (a <= b) over nt tile rows -> (a, b)
__device__ __forceinline__ void tile_ab(int t, int nt, int &a, int &b) {
    int r = 0;
    while (t >= nt - r) {
        t -= nt - r;
        r++;
    }
    a = r;
    b = r + t;
}
// the (r, c) of top-partial slot s (the inverse of top_slot, r <= c)
__device__ __forceinline__ void top_slot_rc(int s, int &r, int &c) {
    if (s < 55) {  // Data[]: upper row-major 10x10
        int a = 0;
        while (s >= 10 - a) {
            s -= 10 - a;
            a++;
        }
        r = a;
        c = a + s;
    } else if (s < 85) {  // TopRight 10x3
        r = (s - 55) / 3;
        c = 10 + (s - 55) % 3;
    } else {  // BotRight: (0,0) (0,1) (0,2) (1,1) (1,2) (2,2)
        const int b = s - 85;
        r = 10 + (b < 3 ? 0 : b < 5 ? 1 : 2);
        c = 10 + (b < 3 ? b : b < 5 ? b - 2 : 2);
    }
}
// v[a][b] += sum_q L_a[q] R_b[q] (a, b in {0, 1}): two q-contiguous, 16-byte aligned 8-double
// rows of each operand; each element's 8 products summed in q order, then added to v
__device__ __forceinline__ void mm22(const double *L0, const double *L1, const double *R0, const double *R1,
                                     double (&v)[2][2]) {
    double l[2][8], r[2][8];
#pragma unroll
    for (int q = 0; q < 8; q += 2) {
        const double2 a0 = *reinterpret_cast<const double2 *>(L0 + q), a1 = *reinterpret_cast<const double2 *>(L1 + q);
        const double2 b0 = *reinterpret_cast<const double2 *>(R0 + q), b1 = *reinterpret_cast<const double2 *>(R1 + q);
        l[0][q] = a0.x;
        l[0][q + 1] = a0.y;
        l[1][q] = a1.x;
        l[1][q + 1] = a1.y;
        r[0][q] = b0.x;
        r[0][q + 1] = b0.y;
        r[1][q] = b1.x;
        r[1][q + 1] = b1.y;
    }
#pragma unroll
    for (int a = 0; a < 2; a++)
#pragma unroll
        for (int b = 0; b < 2; b++) {
            double t = 0;
#pragma unroll
            for (int q = 0; q < 8; q++) t += l[a][q] * r[b][q];
            v[a][b] += t;
        }
}
__global__ __launch_bounds__(kHsThreads) void k_stitch_host(StitchParams P) {
    extern __shared__ __attribute__((aligned(16))) double sm[];
    if ((int)blockIdx.x < P.n_win) {  // setNewFrameEnergyTH + the energy sum, as k_stitch
        const int w = P.win_base + blockIdx.x;
        frame_threshold_and_energy<kHsThreads>(P, P.wins[w], w, reinterpret_cast<unsigned *>(sm));
        return;
    }
    if (!P.accumulate) return;
    // one block per host, or (hs_split: grids that fit the GPU at once, e.g. one window) two: the
    // Top half (HA, bA) and the Schur complement (Hsc, bsc) of the host's partial
    const int hb = blockIdx.x - P.n_win;
    const int fr = P.frame_base + (P.hs_split ? hb >> 1 : hb);
    const bool do_top = !P.hs_split || (hb & 1) == 0, do_sc = !P.hs_split || (hb & 1) == 1;
    const int w = P.frame_win[fr];
    if (P.stop && P.pass > P.stop[w]) return;  // window left the GN loop: its partials stay as they are
    const WinDev &W = P.wins[w];
    const int N = W.N, D = W.D, i = fr - W.frame_base, tid = threadIdx.x;
    const int Kc = 8 * (N - 1), K5 = Kc + 5, ldg = hs_ldg(N), nt = W.KP / 4, per = W.ntiles * 16;
    const int Nm1 = N - 1, npair = hs_npair(N);
    const bool diag = W.adt_diag && !P.dense_adt;  // block-uniform: see the head of this file
    // LDS (every region an even number of doubles: 16-byte aligned rows for the b128 reads)
    double *Gd = sm;                     // [K5][ldg] G_i, both triangles
    double *AH = Gd + (size_t)K5 * ldg;  // [N][8][8] adH of pair (i, k)
    double *AT = AH + kHsB * N;          // [N][8][8] adT of pair (i, k); diagonal path: [N][8] its diagonal
    double *A14 = AT + (diag ? 8 : kHsB) * N;  // [N][13][14] pair (i, t)'s 13x13 Top block (t == i unused)
    double *X = A14 + 182 * N;           // [npair][8][8] X_jk = AT_ij D_jk, target slots sj <= sk (dense path)
    double *SSt = X + (diag ? 0 : kHsB * npair);  // [N][8][8] S_j^T, S_j = sum_k D_jk AH_ik^T
    double *TH = SSt + kHsB * N;         // [N][8][8] AH_it A_t(88)
    double *TT = TH + kHsB * N;          // [N][8][8] AT_it A_t(88) (dense path)
    double *HP = TT + (diag ? 0 : kHsB * N);  // [2 parts][16 2x2s][N-1][4] the (i,i) block's per-term 2x2s
    double *CP = HP + 128 * (N - 1);     // [2 parts][40 items][N-1] the (calib, i) / b(i) per-term dots
    auto frame_of = [&](int slot) { return slot < i ? slot : slot + 1; };
    auto A_t = [&](int t, int r, int c) { return A14[182 * t + 14 * r + c]; };
    // ---- every load of the block in one round trip -------------------------------------
    {
        // G_i: each float4 of the host's chunk partials is one row of a 4x4 tile; summed over the
        // chunks in order (four in flight), then written to both triangles
        const int2 hi = P.host_items[W.frame_base + i];
        const float4 *slab = reinterpret_cast<const float4 *>(P.sc_slab + W.sc_slab_base +
                                                              (size_t)(hi.x - W.sc_item_base) * per);
        const int per4 = per / 4;
        for (int q = tid; q < (do_sc ? per4 : 0); q += kHsThreads) {
            double s[4] = {0, 0, 0, 0};
            int k = 0;
            for (; k + 4 <= hi.y; k += 4) {
                float4 v[4];
#pragma unroll
                for (int u = 0; u < 4; u++) v[u] = slab[(size_t)(k + u) * per4 + q];
#pragma unroll
                for (int u = 0; u < 4; u++) {
                    s[0] += (double)v[u].x;
                    s[1] += (double)v[u].y;
                    s[2] += (double)v[u].z;
                    s[3] += (double)v[u].w;
                }
            }
            for (; k < hi.y; k++) {
                const float4 v = slab[(size_t)k * per4 + q];
                s[0] += (double)v.x;
                s[1] += (double)v.y;
                s[2] += (double)v.z;
                s[3] += (double)v.w;
            }
            int a, b;
            tile_ab(q >> 2, nt, a, b);
            const int row = 4 * a + (q & 3);
#pragma unroll
            for (int u = 0; u < 4; u++) {
                const int col = 4 * b + u;
                if (row < K5 && col < K5 && row <= col) {
                    Gd[row * ldg + col] = s[u];
                    Gd[col * ldg + row] = s[u];
                }
            }
        }
        // the adjoints of the pairs (i, k), k = 0..N-1
        for (int e = tid; e < 64 * N; e += kHsThreads) {
            const size_t pk = (size_t)(W.pair_base + i + N * (e >> 6)) * 64 + (e & 63);
            const int eb = kHsB * (e >> 6) + hs_row((e >> 3) & 7) + (e & 7);
            AH[eb] = P.adH[pk];
            if (!diag)
                AT[eb] = P.adT[pk];
            else if ((e & 63) % 9 == 0)
                AT[8 * (e >> 6) + ((e >> 3) & 7)] = P.adT[pk];
        }
        // Top accumulators of the pairs (i, t): 24 float4 per item, summed over the pair's items
        for (int e = tid; e < (do_top ? 24 * Nm1 : 0); e += kHsThreads) {
            const int t = frame_of(e / 24), q = e % 24;
            const int2 pi = P.pair_items[W.pair_base + i + N * t];
            const float4 *src = reinterpret_cast<const float4 *>(P.top_slab + (size_t)pi.x * kTopVals) + q;
            double s[4] = {0, 0, 0, 0};
            int k = 0;
            for (; k + 4 <= pi.y; k += 4) {
                float4 v[4];
#pragma unroll
                for (int u = 0; u < 4; u++) v[u] = src[(size_t)(k + u) * (kTopVals / 4)];
#pragma unroll
                for (int u = 0; u < 4; u++) {
                    s[0] += (double)v[u].x;
                    s[1] += (double)v[u].y;
                    s[2] += (double)v[u].z;
                    s[3] += (double)v[u].w;
                }
            }
            for (; k < pi.y; k++) {
                const float4 v = src[(size_t)k * (kTopVals / 4)];
                s[0] += (double)v.x;
                s[1] += (double)v.y;
                s[2] += (double)v.z;
                s[3] += (double)v.w;
            }
#pragma unroll
            for (int u = 0; u < 4; u++) {  // both triangles of the 13x13 block (slots 91..95: padding)
                if (4 * q + u >= 91) continue;
                int r, c;
                top_slot_rc(4 * q + u, r, c);
                A14[182 * t + 14 * r + c] = s[u];
                A14[182 * t + 14 * c + r] = s[u];
            }
        }
    }
    __syncthreads();
    // ---- intermediates, 2x2 per thread, 16 threads per 8x8 block: S_j^T (N-1 blocks of N-1
    // terms each, first), TH_t and, on the dense path, X_jk (sj <= sk) and TT_t ---------------
    {
        const int n_ss = do_sc ? Nm1 : 0, n_x = do_sc && !diag ? npair : 0, n_th = do_top ? Nm1 : 0;
        const int total = 16 * (n_ss + n_x + (diag ? 1 : 2) * n_th);
        for (int u = tid; u < total; u += kHsThreads) {
            int blk = u >> 4;
            const int r0 = 2 * ((u & 15) >> 2), c0 = 2 * (u & 3);
            double v[2][2] = {{0, 0}, {0, 0}};
            if (blk < n_ss) {  // S_j[r][c] = sum_k sum_q D_jk[r][q] AH_ik[c][q], k in slot order
                const int sj = blk, j = frame_of(sj);
                for (int sk = 0; sk < Nm1; sk++) {
                    const double *d = Gd + (size_t)(8 * sj + r0) * ldg + 8 * sk, *ah = AH + kHsB * frame_of(sk) + hs_row(c0);
                    mm22(d, d + ldg, ah, ah + 8, v);
                }
#pragma unroll
                for (int a = 0; a < 2; a++)
#pragma unroll
                    for (int b = 0; b < 2; b++) SSt[kHsB * j + hs_row(c0 + b) + r0 + a] = v[a][b];
                continue;
            }
            blk -= n_ss;
            if (blk < n_x) {  // X_jk[r][c] = sum_q AT_ij[r][q] D_jk[q][c], D_jk[q][c] = G[8sk+c][8sj+q]
                int sj = 0, rem = blk;
                while (rem >= Nm1 - sj) {
                    rem -= Nm1 - sj;
                    sj++;
                }
                const int sk = sj + rem;
                const double *at = AT + kHsB * frame_of(sj) + hs_row(r0), *d = Gd + (size_t)(8 * sk + c0) * ldg + 8 * sj;
                mm22(at, at + 8, d, d + ldg, v);
                double *o = X + kHsB * blk;
#pragma unroll
                for (int a = 0; a < 2; a++)
#pragma unroll
                    for (int b = 0; b < 2; b++) o[hs_row(r0 + a) + c0 + b] = v[a][b];
                continue;
            }
            blk -= n_x;  // TH_t / TT_t [r][c] = sum_k AH_it / AT_it [r][k] A_t(4+c, 4+k)
            const bool th = blk < n_th;
            const int t = frame_of(th ? blk : blk - n_th);
            const double *ad = (th ? AH : AT) + kHsB * t + hs_row(r0), *at = A14 + 182 * t + 14 * (4 + c0) + 4;
            mm22(ad, ad + 8, at, at + 14, v);
            double *o = (th ? TH : TT) + kHsB * t;
#pragma unroll
            for (int a = 0; a < 2; a++)
#pragma unroll
                for (int b = 0; b < 2; b++) o[hs_row(r0 + a) + c0 + b] = v[a][b];
        }
    }
    __syncthreads();
    // ---- host i's partial system: every packed element written (zeros included) ------------
    const long long pl = packed_len(D);
    double *HAp = P.stage + W.stage_base + (size_t)i * sys_len(D), *bAp = HAp + pl, *Hsp = bAp + D, *bsp = Hsp + pl;
    auto xblk = [&](int sj, int sk) { return X + kHsB * (sj * Nm1 - sj * (sj - 1) / 2 + (sk - sj)); };
    const int n_fb = 16 * (N * (N + 1) / 2), n_rest = 32 * N + 8 * N + 20, per_part = n_fb + n_rest;
    // The sums over t / j of the (i, i) block and of the (calib, i) / b(i) items are split into
    // one task per term (partials to HP / CP, summed after a barrier in the same order as one
    // task would: (0 + t_0) + t_1 + ...), so no thread carries N-1 terms of them alone.
    const int nH = 56 * Nm1, nparts = do_top + do_sc, pbase = do_top ? 0 : 1;
    for (int uh = tid; uh < nparts * nH; uh += kHsThreads) {
        const int part = pbase + uh / nH, hu = uh % nH;
        const bool top = part == 0;
        if (hu < 16 * Nm1) {  // (i, i) 2x2 sub-block `sub`, term st
            const int sub = hu / Nm1, st = hu % Nm1, r0 = 2 * (sub >> 2), c0 = 2 * (sub & 3);
            if (r0 > c0) continue;
            const int t = frame_of(st);
            const double *th = TH + kHsB * t + hs_row(r0), *ah = AH + kHsB * t, *ss = SSt + kHsB * t + hs_row(c0);
            double v[2][2] = {{0, 0}, {0, 0}};
            if (top)
                mm22(th, th + 8, ah + hs_row(c0), ah + hs_row(c0) + 8, v);
            else
                mm22(ah + hs_row(r0), ah + hs_row(r0) + 8, ss, ss + 8, v);
            double *o = HP + ((part * 16 + sub) * Nm1 + st) * 4;
            o[0] = v[0][0];
            o[1] = v[0][1];
            o[2] = v[1][0];
            o[3] = v[1][1];
        } else {  // (calib cc, frame i, rr) item < 32 / b(i)[rr] item >= 32, term st
            const int item = (hu - 16 * Nm1) / Nm1, st = (hu - 16 * Nm1) % Nm1;
            const int rr = item < 32 ? item >> 2 : item - 32, cI = item < 32 ? (item & 3) : 12, cS = item < 32 ? (item & 3) : 4;
            const int t = frame_of(st);
            double a = 0;
#pragma unroll
            for (int k = 0; k < 8; k++)
                a += AH[kHsB * t + hs_row(rr) + k] * (top ? A_t(t, 4 + k, cI) : Gd[(8 * st + k) * ldg + Kc + cS]);
            CP[(part * 40 + item) * Nm1 + st] = a;
        }
    }
    for (int uo = tid; uo < nparts * per_part; uo += kHsThreads) {
        const bool top = do_top && uo < per_part;  // the Top items first, then the SC ones
        const int u = uo - (do_top && !top ? per_part : 0);
        if (u < n_fb) {  // a 2x2 of frame block (f1 <= f2), upper-block order
            const int r0 = 2 * ((u & 15) >> 2), c0 = 2 * (u & 3);
            int f1 = 0, rem = u >> 4;
            while (rem >= N - f1) {
                rem -= N - f1;
                f1++;
            }
            const int f2 = f1 + rem;
            if (f1 == f2 && r0 > c0) continue;  // below the diagonal
            if (f1 == f2 && f1 == i) continue;  // the (i, i) block: per-term tasks above
            double v[2][2] = {{0, 0}, {0, 0}};
            if (diag) {  // the dense products below with diagonal AT: left scaling first, then right
                const int s1 = f1 < i ? f1 : f1 - 1, s2 = f2 < i ? f2 : f2 - 1;
                auto ld2 = [](const double *p) { return *reinterpret_cast<const double2 *>(p); };  // 16-byte aligned
                const double2 l2 = ld2(AT + 8 * f1 + r0), r2 = ld2(AT + 8 * f2 + c0);
                const double la[2] = {l2.x, l2.y}, ra[2] = {r2.x, r2.y};  // at_f1[r0 + a], at_f2[c0 + b]
                if (f1 == i) {  // M at_f2, M = TH_f2 / S_f2^T: rows r0, r0 + 1 of its columns c0, c0 + 1
                    const double *m = (top ? TH : SSt) + kHsB * f2 + hs_row(r0) + c0;
                    const double2 m0 = ld2(m), m1 = ld2(m + 8);
                    v[0][0] = fma(m0.x, ra[0], 0.0);
                    v[0][1] = fma(m0.y, ra[1], 0.0);
                    v[1][0] = fma(m1.x, ra[0], 0.0);
                    v[1][1] = fma(m1.y, ra[1], 0.0);
                } else if (f2 == i || !top || f1 == f2) {
                    // the other factor transposed, m[b][a] = M[r0 + a][c0 + b]: TH_f1^T / S_f1 (f2 == i, no
                    // right scaling), D_f1f2[r][c] = G[8 s2 + c][8 s1 + r], A_f1(4 + c, 4 + r)
                    const double *m = f2 == i ? (top ? TH : SSt) + kHsB * f1 + hs_row(c0) + r0
                                      : !top  ? Gd + (size_t)(8 * s2 + c0) * ldg + 8 * s1 + r0
                                              : A14 + 182 * f1 + 14 * (4 + c0) + 4 + r0;
                    const double2 m0 = ld2(m), m1 = ld2(m + (f2 == i ? 8 : !top ? ldg : 14));
                    const double mm[2][2] = {{m0.x, m0.y}, {m1.x, m1.y}};
#pragma unroll
                    for (int a = 0; a < 2; a++)
#pragma unroll
                        for (int b = 0; b < 2; b++) {
                            const double x = fma(la[a], mm[b][a], 0.0);
                            v[a][b] = f2 == i ? x : fma(x, ra[b], 0.0);
                        }
                }
            } else if (f1 == f2) {
                const int f = f1, sf = f < i ? f : f - 1;
                const double *tt = TT + kHsB * f + hs_row(r0), *at = AT + kHsB * f + hs_row(c0);
                const double *x = top ? tt : xblk(sf, sf) + hs_row(r0);
                mm22(top ? tt : x, (top ? tt : x) + 8, at, at + 8, v);
            } else if (f1 == i) {
                const double *th = TH + kHsB * f2 + hs_row(r0), *at = AT + kHsB * f2 + hs_row(c0), *ss = SSt + kHsB * f2 + hs_row(r0);
                const double *l = top ? th : ss;  // (AT_i,f2 S_f2)^T on the SC side
                mm22(l, l + 8, at, at + 8, v);
            } else if (f2 == i) {
                const double *at = AT + kHsB * f1 + hs_row(r0), *th = TH + kHsB * f1 + hs_row(c0), *ss = SSt + kHsB * f1 + hs_row(c0);
                const double *rr = top ? th : ss;  // (AH A AT^T)^T of pair (i, f1) / AT_i,f1 S_f1
                mm22(at, at + 8, rr, rr + 8, v);
            } else if (!top) {
                const int s1 = f1 < i ? f1 : f1 - 1, s2 = f2 < i ? f2 : f2 - 1;
                const double *x = xblk(s1, s2) + hs_row(r0), *at = AT + kHsB * f2 + hs_row(c0);
                mm22(x, x + 8, at, at + 8, v);
            }
            double *o = top ? HAp : Hsp;
#pragma unroll
            for (int a = 0; a < 2; a++)
#pragma unroll
                for (int b = 0; b < 2; b++) {
                    if (f1 == f2 && r0 + a > c0 + b) continue;
                    o[pk_index(4 + 8 * f1 + r0 + a, 4 + 8 * f2 + c0 + b, D)] = v[a][b];
                }
            continue;
        }
        const int l0 = u - n_fb;
        double ha = 0;  // this part's value: HA / bA (top) or Hsc / bsc
        long long q;
        bool bvec = false;
        if (l0 < 32 * N) {  // (calib cc, frame f, rr)
            const int f = l0 >> 5, rr = (l0 >> 2) & 7, cc = l0 & 3;
            if (f == i) continue;  // per-term tasks above
            const int sf = f < i ? f : f - 1;
            if (diag) {
                ha = fma(AT[8 * f + rr], top ? A_t(f, 4 + rr, cc) : Gd[(8 * sf + rr) * ldg + Kc + cc], 0.0);
            } else {
#pragma unroll
                for (int k = 0; k < 8; k++)
                    ha += AT[kHsB * f + hs_row(rr) + k] * (top ? A_t(f, 4 + k, cc) : Gd[(8 * sf + k) * ldg + Kc + cc]);
            }
            q = pk_index(cc, 4 + 8 * f + rr, D);
        } else if (l0 < 40 * N) {  // b(f)[rr]
            const int f = (l0 - 32 * N) >> 3, rr = l0 & 7;
            if (f == i) continue;  // per-term tasks above
            const int sf = f < i ? f : f - 1;
            if (diag) {
                ha = fma(AT[8 * f + rr], top ? A_t(f, 4 + rr, 12) : Gd[(8 * sf + rr) * ldg + Kc + 4], 0.0);
            } else {
#pragma unroll
                for (int k = 0; k < 8; k++)
                    ha += AT[kHsB * f + hs_row(rr) + k] * (top ? A_t(f, 4 + k, 12) : Gd[(8 * sf + k) * ldg + Kc + 4]);
            }
            q = 4 + 8 * f + rr;
            bvec = true;
        } else {  // the calibration block (16, upper used) and b(calib) (4)
            const int l = l0 - 40 * N;
            const int r = l < 16 ? l >> 2 : l - 16, cI = l < 16 ? (l & 3) : 12, cS = l < 16 ? (l & 3) : 4;
            if (l < 16 && r > cI) continue;
            if (top)
                for (int st = 0; st < Nm1; st++) ha += A_t(frame_of(st), r, cI);
            else
                ha = Gd[(Kc + r) * ldg + Kc + cS];
            bvec = l >= 16;
            q = bvec ? r : pk_index(r, cI, D);
        }
        (bvec ? (top ? bAp : bsp) : (top ? HAp : Hsp))[q] = ha;
    }
    __syncthreads();
    for (int uf = tid; uf < nparts * 56; uf += kHsThreads) {  // the split sums, terms in order
        const int part = pbase + uf / 56, fu = uf % 56;
        const bool top = part == 0;
        if (fu < 16) {
            const int r0 = 2 * (fu >> 2), c0 = 2 * (fu & 3);
            if (r0 > c0) continue;
            double v[4] = {0, 0, 0, 0};
            for (int st = 0; st < Nm1; st++) {
                const double *hp = HP + ((part * 16 + fu) * Nm1 + st) * 4;
#pragma unroll
                for (int e = 0; e < 4; e++) v[e] += hp[e];
            }
            double *o = top ? HAp : Hsp;
#pragma unroll
            for (int a = 0; a < 2; a++)
#pragma unroll
                for (int b = 0; b < 2; b++) {
                    if (r0 + a > c0 + b) continue;
                    o[pk_index(4 + 8 * i + r0 + a, 4 + 8 * i + c0 + b, D)] = v[2 * a + b];
                }
        } else {
            const int item = fu - 16, rr = item < 32 ? item >> 2 : item - 32, cc = item & 3;
            double ha = 0;
            for (int st = 0; st < Nm1; st++) ha += CP[(part * 40 + item) * Nm1 + st];
            if (item < 32)
                (top ? HAp : Hsp)[pk_index(cc, 4 + 8 * i + rr, D)] = ha;
            else
                (top ? bAp : bsp)[4 + 8 * i + rr] = ha;
        }
    }
}
// sys = sum over the window's hosts of their partials, in host order, one thread per element
__global__ __launch_bounds__(256) void k_stitch_host_sum(const WinDev *__restrict__ wins,
                                                          const int2 *__restrict__ blocks,
                                                          const double *__restrict__ stage, double *sys) {
    const int2 bw = blocks[blockIdx.x];  // {window, first element of this block}
    const WinDev &W = wins[bw.x];
    const long long n_el = sys_len(W.D), e = (long long)bw.y + threadIdx.x;
    if (e >= n_el) return;
    const double *p = stage + W.stage_base + e;
    double x[kHostStitchMaxN];
#pragma unroll
    for (int h = 0; h < kHostStitchMaxN; h++) x[h] = p[(size_t)min(h, W.N - 1) * n_el];
    double v = 0;
#pragma unroll
    for (int h = 0; h < kHostStitchMaxN; h++)
        if (h < W.N) v += x[h];
    sys[W.sys_base + e] = v;
}

}  // namespace
