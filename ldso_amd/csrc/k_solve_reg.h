// k_solve_reg.h -- the pivoted solve out of registers (windows of up to 7 keyframes).
#pragma once
#include "k_solve.h"

namespace {

// ============================================================================================
// k_solve_reg: the same solve for windows of up to 7 keyframes (n <= 64), factorised out of
// registers by four wavefronts without block barriers.  Lane p of wave w holds H(p, q) for the
// 16 columns q = 16w .. 16w+15 of the scaled symmetric H (both triangles) and, in every wave,
// the diagonal of row p.  Pivoting is logical: rows never move, pos tracks the host's index of
// each physical row (the swap k <-> piv is bookkeeping), and every wave selects the pivot
// itself from its copy of the diagonal (the copies are bitwise equal).  The wave owning the
// pivot's column publishes it in LDS (one slot per step, then a ready flag; LDS requests of a
// wave are served in order, so a flag seen set means the column is there).  Look-ahead: right
// after a step's column arrives each wave updates the diagonal and picks the next pivot, and
// its owner updates and publishes that one column before its own trailing update, so the
// serial chain per step is read column -> diagonal -> pivot -> one fma -> publish; 1/d is
// computed off that chain.  Every element sees the host's operations in the host's order (the
// update is symmetric in i, j), so x stays bit-identical to ldso_ba_solve.
// A fifth wave prepares the nullspace projection, then follows the published columns: L(i,k)
// = c_i / d into Ls and the forward substitution step by step (the host's per-element order),
// then the diagonal, the backward substitution and the projection -- all in physical row order
// (b[perm[i]] = y_i makes the host's permutation disappear).
// ============================================================================================
constexpr int kSolveRegDim = 64;
constexpr int kSolveLsLd = 65;            // odd: a column walk of Ls is bank-conflict free
constexpr int kSolveRegThreads = 5 * 64;  // 4 factorisation waves + the substitution wave
__host__ __device__ inline size_t solve_reg_base(int n) { return (solve_smem_bytes(n) + 15) / 16 * 2; }  // doubles
__host__ __device__ inline size_t solve_reg_smem_bytes(int n) {
    return solve_reg_base(n) * sizeof(double) +
           ((size_t)kSolveRegDim * kSolveLsLd + kSolveRegDim * kSolveRegDim + kSolveRegDim + 7 * kSolveRegDim + 1) *
               sizeof(double) +
           2 * kSolveRegDim * sizeof(int);
}
struct RegLds {
    double *cb, *Ls, *Dv, *raw;  // cb: [step][64] published columns (16-byte aligned); Dv: d of step
    int *pv, *flag;              // pivot row and ready flag of each step
    __device__ RegLds(double *lds, int n) {
        cb = lds + solve_reg_base(n);
        Ls = cb + kSolveRegDim * kSolveRegDim;
        Dv = Ls + kSolveRegDim * kSolveLsLd;
        raw = Dv + kSolveRegDim;
        pv = reinterpret_cast<int *>(raw + 7 * kSolveRegDim + 1);
        flag = pv + kSolveRegDim;
    }
};
#define LDSO_COMPILER_FENCE() asm volatile("" ::: "memory")
// wave-wide maximum of a 32-bit key (0 = identity), broadcast: row_shr 1/2/4/8 within each row
// of 16, then row_bcast15 / row_bcast31 carry rows 0-2 into lane 63
__device__ __forceinline__ unsigned wave_max_u32(unsigned x) {
#define LDSO_DPP_MAX32(CTRL, ROWS)                                                                          \
    {                                                                                                       \
        const unsigned o = (unsigned)__builtin_amdgcn_update_dpp(0, (int)x, CTRL, ROWS, 0xF, true);         \
        x = o > x ? o : x;                                                                                  \
    }
    LDSO_DPP_MAX32(0x111, 0xF)
    LDSO_DPP_MAX32(0x112, 0xF)
    LDSO_DPP_MAX32(0x114, 0xF)
    LDSO_DPP_MAX32(0x118, 0xF)
    LDSO_DPP_MAX32(0x142, 0xA)
    LDSO_DPP_MAX32(0x143, 0xC)
#undef LDSO_DPP_MAX32
    return (unsigned)__builtin_amdgcn_readlane((int)x, 63);
}
// pivot of step k: the largest |diag| among the live rows, ties to the smallest host index; a
// NaN never wins, except at the host's row k itself, which then keeps k (the host's strict '>'
// scan from k).  The maximum of the order-preserving 64-bit keys: the high words by DPP first,
// the low words among high-word ties (an LDS atomic-max variant measured slower).
__device__ __forceinline__ int reg_pivot(double dg, unsigned long long act, int pos, int k, int lane) {
    const bool live = (act >> lane) & 1;
    const unsigned long long key = !live ? 0ull : (dg != dg && pos == k) ? ~0ull : abs_key(dg);
    const unsigned hi = (unsigned)(key >> 32), lo = (unsigned)key;
    const unsigned mh = wave_max_u32(hi);
    unsigned long long cand = __ballot(live && hi == mh);
    if (cand & (cand - 1)) {
        const bool c = (cand >> lane) & 1;
        const unsigned ml = wave_max_u32(c ? lo : 0u);
        cand = __ballot(c && lo == ml);
    }
    int piv = __builtin_ctzll(cand);
    if (cand & (cand - 1)) {  // exact tie: the smallest host index
        int best = __builtin_amdgcn_readlane(pos, piv);
        for (unsigned long long m = cand & (cand - 1); m; m &= m - 1) {
            const int l = __builtin_ctzll(m), pl = __builtin_amdgcn_readlane(pos, l);
            if (pl < best) {
                best = pl;
                piv = l;
            }
        }
    }
    return __builtin_amdgcn_readfirstlane(piv);
}
// column of step k, then its ready flag = pivot row + 1 (no wait: the LDS serves a wave's
// requests in order).  The pivot row's own entry of the column is d.
__device__ __forceinline__ void reg_publish(const RegLds &R, int k, int lane, double c, int piv) {
    R.cb[k * kSolveRegDim + lane] = c;
    LDSO_COMPILER_FENCE();
    if (lane == 0) __hip_atomic_store(R.flag + k, piv + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    LDSO_COMPILER_FENCE();
}
// poll the flag and the column together: a set flag read before the column read means the
// column read returns the published value; returns the pivot row
// A bounded wait: after ~2^22 polls (well over 100 ms) it gives up with a NaN column and row 0,
// so the kernel always drains even if a publication were ever missing (x then reads NaN).
template <bool kSleep = false>
__device__ __forceinline__ int reg_wait(const RegLds &R, int k, int lane, double &v) {
    int f;
    unsigned polls = 0;
    do {
        f = __hip_atomic_load(R.flag + k, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        LDSO_COMPILER_FENCE();
        v = R.cb[k * kSolveRegDim + lane];
        LDSO_COMPILER_FENCE();
        f = __builtin_amdgcn_readfirstlane(f);
        if (kSleep && f == 0) __builtin_amdgcn_s_sleep(2);
        if (f == 0 && ++polls > (1u << 22)) {
            v = __longlong_as_double(0x7ff8000000000000ll);
            return 0;
        }
    } while (f == 0);
    return f - 1;
}
// the factorisation waves of k_solve_reg: 16 columns of H in registers per wave
__device__ __forceinline__ void solve_reg_factor(const RegLds &R, const SolveLds &S, int n, int ld, int wave,
                                                 int lane) {
#pragma clang fp contract(off)
    typedef double d16 __attribute__((ext_vector_type(16)));
    d16 rv;
    const int q0 = 16 * wave;
#pragma unroll
    for (int j = 0; j < 16; j++) {
        const int q = q0 + j, r = lane > q ? lane : q, c = lane > q ? q : lane;
        rv[j] = q < n && lane < n ? S.H[r * ld + c] : 0.0;
    }
    double dg = lane < n ? S.H[lane * ld + lane] : 0.0;
    int pos = lane;
    unsigned long long act = n >= 64 ? ~0ull : ((1ull << n) - 1);  // rows not yet pivoted
    int piv = reg_pivot(dg, act, pos, 0, lane);
    double d = readlane_f64(dg, piv);
    double cl = 0.0;
    if ((piv >> 4) == wave) {
        cl = rv[piv & 15];
        reg_publish(R, 0, lane, cl, piv);
    }
    double rd = d != 0 ? 1.0 / d : 0.0;
    for (int k = 0; k < n; k++) {
        if ((piv >> 4) != wave) (void)reg_wait(R, k, lane, cl);  // column k of the host: A(i, k) after the swap
        const int kphys = __builtin_ctzll(__ballot(((act >> lane) & 1) && pos == k));
        const int ppos = __builtin_amdgcn_readlane(pos, piv);
        pos = lane == piv ? k : (lane == kphys ? ppos : pos);
        act &= ~(1ull << piv);
        dg = fma(-(cl * cl), rd, dg);
        int nxt = 0;
        double cn = 0.0, rdn = 0.0;
        if (k + 1 < n) {
            nxt = reg_pivot(dg, act, pos, k + 1, lane);
            const double dn = readlane_f64(dg, nxt);
            if ((nxt >> 4) == wave) {  // look-ahead: the next pivot's column first
                cn = fma(-(cl * readlane_f64(cl, nxt)), rd, rv[nxt & 15]);
                reg_publish(R, k + 1, lane, cn, nxt);
            }
            rdn = dn != 0 ? 1.0 / dn : 0.0;
        }
        // trailing update of this wave's 16 columns, c_q broadcast from the published column
        // (dead columns too: never read again; the look-ahead column gets the same bits again)
        const double2 *cq2 = reinterpret_cast<const double2 *>(R.cb + k * kSolveRegDim + q0);
#pragma unroll
        for (int u = 0; u < 8; u++) {
            const double2 cq = cq2[u];
            rv[2 * u] = fma(-(cl * cq.x), rd, rv[2 * u]);
            rv[2 * u + 1] = fma(-(cl * cq.y), rd, rv[2 * u + 1]);
        }
        piv = nxt;
        cl = cn;
        rd = rdn;
    }
}
__global__ __launch_bounds__(kSolveRegThreads) void k_solve_reg(SolveParams P) {
#pragma clang fp contract(off)
    extern __shared__ double lds[];
    if (P.stop && P.iteration >= P.stop[blockIdx.x]) return;  // the window left the GN loop
    const WinDev W = P.wins[blockIdx.x];  // a register copy (see k_solve)
    const int n = W.D, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int ld = solve_ld(n);
    const SolveLds S(lds, n);
    const RegLds R(lds, n);
    for (int i = tid; i < kSolveRegDim; i += kSolveRegThreads) R.flag[i] = 0;
    solve_ortho_load(P, W, S, tid, kSolveRegThreads);
    solve_assemble<kSolveRegThreads>(P, W, S, tid);  // its barriers also publish the flags
    if (wave == 4) __builtin_amdgcn_s_setprio(0);  // the factorisation's chain first
    else __builtin_amdgcn_s_setprio(2);
    if (wave == 4) {
        // ---- the projection's x-independent half, then the substitutions (physical rows)
        double y = lane < n ? S.b[lane] : 0.0;
        unsigned long long act = n >= 64 ? ~0ull : ((1ull << n) - 1);
        for (int k = 0; k < n; k++) {  // forward: y_i = fma(-L(i,k), y_k, y_i), k ascending
            double cl;
            const int piv = reg_wait<true>(R, k, lane, cl);  // off the critical chain: poll gently
            const double d = readlane_f64(cl, piv);
            if (lane == 0) {
                R.Dv[k] = d;
                R.pv[k] = piv;
            }
            act &= ~(1ull << piv);
            const double yk = readlane_f64(y, piv);
            if ((act >> lane) & 1) {
                const double l = d != 0 ? cl / d : 0.0;
                R.Ls[k * kSolveLsLd + lane] = l;
                y = fma(-l, yk, y);
            }
        }
        // to the host's order: lane i takes y_i = y of physical row pv[i]; then the diagonal
        if (lane < n) S.col[lane] = y;
        wave_lds_sync();
        const int pvl = lane < n ? R.pv[lane] : 0;
        double yl = lane < n ? S.col[pvl] : 0.0;
        if (lane < n) {
            const double dd = R.Dv[lane];
            yl = dd != 0 ? yl / dd : 0.0;
        }
        // backward: y_i = fma(-L(j,i), y_j, y_i) for j descending, L(j,i) = Ls[i][pv[j]] (a
        // rolled loop: this code runs once, so its size is instruction fetches)
        const int me = min(lane, n - 1);
        constexpr int kSubAhead = 4;
#pragma unroll 1
        for (int j0 = n - 1; j0 >= 0; j0 -= kSubAhead) {
            double fa[kSubAhead];
#pragma unroll
            for (int u = 0; u < kSubAhead; u++)
                fa[u] = R.Ls[me * kSolveLsLd + __builtin_amdgcn_readlane(pvl, max(j0 - u, 0))];
#pragma unroll
            for (int u = 0; u < kSubAhead; u++) {
                const int j = j0 - u;
                if (j < 0) break;
                const double t = fma(-fa[u], readlane_f64(yl, j), yl);
                yl = lane < j ? t : yl;
            }
        }
        if (lane < n) S.b[pvl] = yl;  // b[perm[i]] = y_i
        wave_lds_sync();
        y = lane < n ? S.b[lane] : 0.0;
        if (lane < n) S.y[lane] = S.sc[lane] * y;  // x = s b, b[perm[i]] = y_i
        wave_lds_sync();
        solve_ortho_apply_store(P, W, S, lane);
    } else {
        solve_reg_factor(R, S, n, ld, wave, lane);
    }
    if (P.xad) {  // x is in S.y: the resubstitution's xAd by all five waves
        __syncthreads();
        xad_fill(W, S.y, P.adH, P.adT, P.xad + (size_t)blockIdx.x * kXadStride, tid, kSolveRegThreads);
    }
}

}  // namespace
