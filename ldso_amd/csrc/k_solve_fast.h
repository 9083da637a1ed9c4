// k_solve_fast.h -- the unpivoted blocked LDL^T solve (the default).
#pragma once
#include "k_solve.h"

namespace {

// ============================================================================================
// k_solve_fast: the same solveSystemF without pivoting (LDSO_BA_SOLVE_FAST, the default; windows
// up to 11 keyframes).  After solve_assemble the scaled matrix is symmetric positive definite
// (Jacobi-scaled HA + priors + lambda damping - Hsc / (1 + lambda)), so an unpivoted LDL^T is
// stable; dropping the pivot search removes the serial pivot reduction and the cross-wave
// hand-off of every step.  Blocked right-looking LDL^T in LDS: wave 0 factorises an 8-column
// panel out of registers (lane = row, the in-panel columns broadcast with readlane) together with
// the forward substitution, while the other waves apply the previous panel's rank-8 update to
// the trailing matrix (look-ahead, two barriers per panel).  Trailing elements see
// fma(-(c_i c_j), 1/d, A(i,j)) for the steps in ascending order, as the host solver, just without
// the row exchanges; in-panel ones fma(-c_i, c_j / d, A(i,j)); L(i,k) = c_i * (1/d).  Wave 0
// then runs the backward substitution and the projection (prepared by k_ortho_prep).  x differs from the pivoted
// solve (k_solve_reg / k_solve / ldso_ba_solve) only by rounding (tests: within the system's
// float sensitivity envelope; optimize energies within 1e-4).
// ============================================================================================
#ifndef LDSO_SOLVE_FAST_THREADS
#define LDSO_SOLVE_FAST_THREADS 512
#endif
constexpr int kSolveFastThreads = LDSO_SOLVE_FAST_THREADS;  // 8 waves: the trailing updates hide LDS latency
constexpr int kSolveFastPanel = 8;
__host__ __device__ inline size_t solve_fast_smem_bytes(int n) {
    // SolveLds | W [2][8][128] panel columns (double-buffered) | rd [2][8]
    return solve_smem_bytes(n) + 16 + 2 * ((size_t)kSolveFastPanel * 128 + kSolveFastPanel) * sizeof(double);
}
// row k's value of a lane-per-row register pair (rows lane, lane + 64)
template <int kH>
__device__ __forceinline__ double fast_row(const double *v, int k) {
    if constexpr (kH == 1)
        return readlane_f64(v[0], k);
    else
        return k < 64 ? readlane_f64(v[0], k) : readlane_f64(v[1], k - 64);
}
// Wave 0: LDL^T of panel columns p .. p+w-1 (rows lane + 64 h).  Lane i updates its rows' panel
// entries unconditionally -- entries above the diagonal and rows past n turn into finite junk that
// is never stored nor read -- so a step is one readlane pair, one product cj / d and one fma per
// later column and row half, with the h = 1 half compiled out for n <= 64.  Only what the pivot
// chain needs runs here: the step's column c and 1/d go to LDS (Wc, rdv), and the other waves
// write L(i, k) = c_i / d and d into H (fast_store_l) and run the forward substitution
// (fast_forward) from them while this wave factorises the next panel: the same statements, so the
// same bits as when this wave did both (round 6: 40 -> 25 instructions per pivot on the chain).
template <int kH>
__device__ __forceinline__ void fast_panel(double *H, double *Wc, double *rdv, int n, int ld, int p, int w, int lane) {
#pragma clang fp contract(off)
    double r[kSolveFastPanel][kH];
#pragma unroll
    for (int h = 0; h < kH; h++)
#pragma unroll
        for (int jj = 0; jj < kSolveFastPanel; jj++) {
            const int i = lane + 64 * h;
            r[jj][h] = i < n && jj < w && i >= p + jj ? H[i * ld + p + jj] : 0.0;
        }
#pragma unroll
    for (int kk = 0; kk < kSolveFastPanel; kk++) {
        if (kk >= w) break;
        const int k = p + kk;
        const double d = fast_row<kH>(r[kk], k);
        // 1/d: v_rcp_f64 and two Newton steps (the IEEE divide's 10-deep chain sits on every step)
        double rd = __builtin_amdgcn_rcp(d);
        rd = fma(rd, fma(-d, rd, 1.0), rd);
        rd = fma(rd, fma(-d, rd, 1.0), rd);
        rd = d != 0 ? rd : 0.0;
#pragma unroll
        for (int jj = kk + 1; jj < kSolveFastPanel; jj++) {
            const double wj = fast_row<kH>(r[kk], p + jj) * rd;  // A(j, k) / d; columns past n are junk
#pragma unroll
            for (int h = 0; h < kH; h++) r[jj][h] = fma(-r[kk][h], wj, r[jj][h]);
        }
#pragma unroll
        for (int h = 0; h < kH; h++) Wc[kk * 128 + lane + 64 * h] = r[kk][h];  // 128 rows a column
        rdv[kk] = rd;  // every lane the same value: no exec-mask branch
    }
}
// L(i, k) = c_i * (1/d) below the diagonal and d on it, for the w columns of panel p (columns c and
// 1/d from Wc / rdv), threads t, t + nth, ...; rows above the diagonal are never read
__device__ __forceinline__ void fast_store_l(double *H, const double *Wp, const double *rp, int n, int ld, int p,
                                             int w, int t, int nth) {
#pragma clang fp contract(off)
    for (int e = t; e < (n - p) * w; e += nth) {
        const int i = p + e / w, kk = e % w, k = p + kk;
        if (i >= k) H[i * ld + k] = i > k ? Wp[kk * 128 + i] * rp[kk] : Wp[kk * 128 + i];
    }
}
// the forward substitution L y = b over panel p's w columns (y in the calling wave's registers,
// rows lane, lane + 64): y_i = fma(-L(i, k), y_k, y_i) for k in order
template <int kH>
__device__ __forceinline__ void fast_forward(const double *Wp, const double *rp, double *y, int p, int w, int lane) {
#pragma clang fp contract(off)
    for (int kk = 0; kk < w; kk++) {
        const int k = p + kk;
        const double yk = fast_row<kH>(y, k), rd = rp[kk];
#pragma unroll
        for (int h = 0; h < kH; h++) {
            const int i = lane + 64 * h;
            const double l = i > k ? Wp[kk * 128 + i] * rd : 0.0;  // L(i,k) (rd = 0 for d = 0)
            y[h] = fma(-l, yk, y[h]);
        }
    }
}
// After the last panel (the wave holding y): D, L^T x = y (y in lanes i, i + 64), x = s y into S.y
template <int kH>
__device__ __forceinline__ void fast_back_subst(const double *H, const SolveLds &S, double *y, int n, int ld,
                                                int lane) {
#pragma clang fp contract(off)
    int ri[kH];
#pragma unroll
    for (int h = 0; h < kH; h++) {
        const int i = lane + 64 * h;
        ri[h] = min(i, n - 1);
        if (i < n) y[h] = H[i * ld + i] != 0 ? y[h] / H[i * ld + i] : 0.0;
    }
    constexpr int kSubAhead = 4;
    // the L columns of a block of kSubAhead steps, loaded one block ahead (H is read-only here)
    double f[kSubAhead][kH], fn[kSubAhead][kH];
    auto ldf = [&](int j0, double (&F)[kSubAhead][kH]) {
#pragma unroll
        for (int u = 0; u < kSubAhead; u++)
#pragma unroll
            for (int h = 0; h < kH; h++) F[u][h] = H[max(j0 - u, 0) * ld + ri[h]];
    };
    ldf(n - 1, f);
    for (int j0 = n - 1; j0 >= 0; j0 -= kSubAhead) {
        ldf(max(j0 - kSubAhead, 0), fn);
#pragma unroll
        for (int u = 0; u < kSubAhead; u++) {
            const int j = j0 - u;
            if (j < 0) break;
            const double yj = fast_row<kH>(y, j);
#pragma unroll
            for (int h = 0; h < kH; h++) {
                const int i = lane + 64 * h;
                if (i < j) y[h] = fma(-f[u][h], yj, y[h]);
            }
        }
#pragma unroll
        for (int u = 0; u < kSubAhead; u++)
#pragma unroll
            for (int h = 0; h < kH; h++) f[u][h] = fn[u][h];
    }
#pragma unroll
    for (int h = 0; h < kH; h++) {
        const int i = lane + 64 * h;
        if (i < n) S.y[i] = S.sc[i] * y[h];  // x = s y
    }
}
// panel (Wp, rp: its c columns and 1/d, w steps) applied to A(i, j), steps in order
__device__ __forceinline__ double fast_update(const double *Wp, const double *rp, int w, int i, int j, double a) {
#pragma clang fp contract(off)
    double wi[kSolveFastPanel], wj[kSolveFastPanel], rk[kSolveFastPanel];
#pragma unroll
    for (int kk = 0; kk < kSolveFastPanel; kk++) {  // every operand in flight before the chain
        wi[kk] = Wp[kk * 128 + i];
        wj[kk] = Wp[kk * 128 + j];
        rk[kk] = rp[kk];
    }
#pragma unroll
    for (int kk = 0; kk < kSolveFastPanel; kk++)
        if (kk < w) a = fma(-(wi[kk] * wj[kk]), rk[kk], a);
    return a;
}
__global__ __launch_bounds__(kSolveFastThreads) void k_solve_fast(SolveParams P) {
#pragma clang fp contract(off)
    extern __shared__ double lds[];
    if (P.win_nid && (int)blockIdx.x >= P.n_win) {  // doStepFromBackup's sumNID (FullSystem.cc:1899-1909)
        const int w = blockIdx.x - P.n_win;
        if (P.stop && P.iteration >= P.stop[w]) return;
        nid_chain(P.wins[w], P.nid_src, P.win_nid, w, reinterpret_cast<float *>(lds), P.nid_chunk);
        return;
    }
    static_assert(7 * kSolveMaxDim <= 2 * kSolveFastThreads, "OrthoPre: two Nm elements per thread");
    // the stop flag and the window's descriptor in one round trip, then the exit
    const int stop_it = P.stop ? P.stop[blockIdx.x] : INT_MAX;
    const WinDev W = P.wins[blockIdx.x];  // a register copy (see k_solve)
    if (P.iteration >= stop_it) return;  // the window left the GN loop
    const int n = W.D, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int ld = solve_ld(n);
    const SolveLds S(lds, n);
    double *H = S.H;
    double *Wc = lds + (solve_smem_bytes(n) + 16) / sizeof(double);  // [2][8][128]: c of each panel step
    double *rdv = Wc + 2 * kSolveFastPanel * 128;                     // [2][8]: 1/d of each panel step
    XadPre xp;
    if (P.xad) xp.load(W, P.adH, P.adT, tid);
    OrthoPre op;
    op.load(P, W, tid, kSolveFastThreads);
    solve_assemble<kSolveFastThreads>(P, W, S, tid);
    op.store(P, W, S, tid, kSolveFastThreads);  // published by the factorisation's barriers
    double y[2] = {0.0, 0.0};  // wave 1: the forward substitution's y (rows lane, lane + 64)
    if (wave == 1) {
        y[0] = lane < n ? S.b[lane] : 0.0;
        y[1] = lane + 64 < n ? S.b[lane + 64] : 0.0;
    }
    auto panel = [&](int p, int w, int buf) {
        double *Wb = Wc + buf * kSolveFastPanel * 128, *rb = rdv + buf * kSolveFastPanel;
        if (n > 64)
            fast_panel<2>(H, Wb, rb, n, ld, p, w, lane);
        else
            fast_panel<1>(H, Wb, rb, n, ld, p, w, lane);
    };
    auto forward = [&](const double *Wp, const double *rp, int p, int w) {
        if (n > 64)
            fast_forward<2>(Wp, rp, y, p, w, lane);
        else
            fast_forward<1>(Wp, rp, y, p, w, lane);
    };
    // Blocked right-looking LDL^T with look-ahead: after panel p is factorised, all waves apply
    // it to the next panel's columns; then wave 0 factorises the next panel while the other
    // waves apply panel p to the rest of the trailing triangle (double-buffered panel columns).
    if (wave == 0) panel(0, min(kSolveFastPanel, n), 0);
    __syncthreads();
    int p = 0, buf = 0;
    for (; p + kSolveFastPanel < n; p += kSolveFastPanel, buf ^= 1) {
        const int w = kSolveFastPanel, m0 = p + w, w1 = min(kSolveFastPanel, n - m0), m1 = m0 + w1;
        const double *Wp = Wc + buf * kSolveFastPanel * 128, *rp = rdv + buf * kSolveFastPanel;
        for (int e = tid; e < (n - m0) * w1; e += kSolveFastThreads) {  // the next panel's columns
            const int i = m0 + e / w1, j = m0 + e % w1;
            if (i >= j) H[i * ld + j] = fast_update(Wp, rp, w, i, j, H[i * ld + j]);
        }
        __syncthreads();
        if (wave == 0) {
            panel(m0, w1, buf ^ 1);
        } else {  // panel p's forward substitution, the rest of the trailing triangle (m1 <= j <= i < n), L and d of panel p
            if (wave == 1) forward(Wp, rp, p, w);
            const int nt = n - m1, ne = nt * (nt + 1) / 2;
            for (int e = tid - 64; e < ne; e += kSolveFastThreads - 64) {
                int ii = (int)((sqrtf(8.0f * e + 1.0f) - 1.0f) * 0.5f);  // row ii of the nt x nt triangle
                if (ii * (ii + 1) / 2 > e) ii--;
                if ((ii + 1) * (ii + 2) / 2 <= e) ii++;
                const int i = m1 + ii, j = m1 + (e - ii * (ii + 1) / 2);
                H[i * ld + j] = fast_update(Wp, rp, w, i, j, H[i * ld + j]);
            }
            fast_store_l(H, Wp, rp, n, ld, p, w, tid - 64, kSolveFastThreads - 64);
        }
        __syncthreads();
    }
    {  // the last panel (p, buffer buf): its forward substitution and L, then the backward one
        const double *Wl = Wc + buf * kSolveFastPanel * 128, *rl = rdv + buf * kSolveFastPanel;
        const int wl = n - p;
        if (wave == 1) forward(Wl, rl, p, wl);
        fast_store_l(H, Wl, rl, n, ld, p, wl, tid, kSolveFastThreads);
    }
    __syncthreads();
    if (wave == 1) {
        if (n > 64)
            fast_back_subst<2>(H, S, y, n, ld, lane);
        else
            fast_back_subst<1>(H, S, y, n, ld, lane);
    }
    __syncthreads();
    if (wave == 0) solve_ortho_apply_store(P, W, S, lane);
    if (P.xad) {  // x is in S.y: the resubstitution's xAd by all waves
        __syncthreads();
        xp.fill(W, S.y, P.adH, P.adT, P.xad + (size_t)blockIdx.x * kXadStride, tid, kSolveFastThreads);
    }
}

}  // namespace
