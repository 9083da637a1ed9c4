// k_solve.h -- solveSystemF on the device: what the three solve kernels share (xad_fill, SolveParams,
// SolveLds, the assembly and the orthogonalisation), k_ortho_prep and the LDS solve k_solve.
#pragma once
#include "ba_device.h"

namespace {

// ============================================================================================
// k_solve: EnergyFunctional::solveSystemF on the GPU, one workgroup of 4 wavefronts per window
// (SURVEY §8f row 1).  Statement for statement the host solver (host_math.cpp solve_system:
// assembly with the FIX_LAMBDA damping, Jacobi scaling, lower-triangle LDL^T with diagonal
// pivoting, column substitutions, orthogonalize); every element sees the host's operations in
// the host's order, so x is bit-identical to ldso_ba_solve's.  H lives in LDS (n <= kSolveMaxDim).
// ============================================================================================
constexpr int kSolveMaxDim = 8 * 11 + 4;  // windows up to 11 keyframes (68 KB of LDS for H)
#ifndef LDSO_SOLVE_THREADS
#define LDSO_SOLVE_THREADS 256
#endif
constexpr int kSolveThreads = LDSO_SOLVE_THREADS;  // wavefronts share the assembly and the LDL^T updates
// Round-robin (circle method) schedule of the 7 x 7 Jacobi sweep: 7 rounds of 3 disjoint pairs
// (p < q); player r sits out round r.  Shared with host_math.cpp's project_out.
__device__ constexpr int kJacobiRounds[7][3][2] = {
    {{1, 6}, {2, 5}, {3, 4}}, {{0, 2}, {3, 6}, {4, 5}}, {{1, 3}, {0, 4}, {5, 6}}, {{2, 4}, {1, 5}, {0, 6}},
    {{3, 5}, {2, 6}, {0, 1}}, {{4, 6}, {0, 3}, {1, 2}}, {{0, 5}, {1, 4}, {2, 3}}};
constexpr int kXadStride = LDSO_BA_MAX_FRAMES * LDSO_BA_MAX_FRAMES * 8 + 4;  // floats per window
// xAd[N*h + t] = x_h^T adHostF[h + N t] + x_t^T adTargetF[h + N t] in float (EnergyFunctional.cc:
// 624-632), then x_c: the statements of the host path of ldso_ba_resubstitute, over threads
// tid, tid + nthreads, ... of one window, from item tid + start_round * nthreads (XadPre::fill has
// done round 0 itself and passes 1)
__device__ __forceinline__ void xad_fill(const WinDev &W, const double *xw, const double *__restrict__ adH,
                                         const double *__restrict__ adT, float *o, int tid, int nthreads,
                                         int start_round = 0) {
#pragma clang fp contract(off)
    const int N = W.N;
    for (int e = tid + start_round * nthreads; e < N * N * 8; e += nthreads) {
        const int cc = e & 7, ht = e >> 3, h = ht / N, t = ht % N;
        const double *AH = adH + (size_t)(W.pair_base + h + N * t) * 64, *AT = adT + (size_t)(W.pair_base + h + N * t) * 64;
        float s1 = 0, s2 = 0;
        for (int k = 0; k < 8; k++) s1 += (float)xw[4 + 8 * h + k] * (float)AH[k * 8 + cc];
        for (int k = 0; k < 8; k++) s2 += (float)xw[4 + 8 * t + k] * (float)AT[k * 8 + cc];
        o[(size_t)(N * h + t) * 8 + cc] = s1 + s2;
    }
    if (tid < 4) o[(size_t)N * N * 8 + tid] = (float)xw[tid];
}
// xad_fill with the adjoint columns of item tid loaded at kernel start (their load latency hides
// behind the factorisation); items tid + nthreads, ... as xad_fill
struct XadPre {
    float ah[8], at[8];
    __device__ void load(const WinDev &W, const double *__restrict__ adH, const double *__restrict__ adT, int tid) {
        const int N = W.N, e = min(tid, N * N * 8 - 1), cc = e & 7, ht = e >> 3, h = ht / N, t = ht % N;
        const double *AH = adH + (size_t)(W.pair_base + h + N * t) * 64, *AT = adT + (size_t)(W.pair_base + h + N * t) * 64;
#pragma unroll
        for (int k = 0; k < 8; k++) {
            ah[k] = (float)AH[k * 8 + cc];
            at[k] = (float)AT[k * 8 + cc];
        }
    }
    __device__ void fill(const WinDev &W, const double *xw, const double *__restrict__ adH,
                         const double *__restrict__ adT, float *o, int tid, int nthreads) const {
#pragma clang fp contract(off)
        const int N = W.N;
        if (tid < N * N * 8) {
            const int cc = tid & 7, ht = tid >> 3, h = ht / N, t = ht % N;
            float s1 = 0, s2 = 0;
            for (int k = 0; k < 8; k++) s1 += (float)xw[4 + 8 * h + k] * ah[k];
            for (int k = 0; k < 8; k++) s2 += (float)xw[4 + 8 * t + k] * at[k];
            o[(size_t)(N * h + t) * 8 + cc] = s1 + s2;
        }
        xad_fill(W, xw, adH, adT, o, tid, nthreads, 1);
    }
};

struct SolveParams {
    const WinDev *__restrict__ wins;
    const double *__restrict__ sys;
    const double *__restrict__ prior;  // [vec][2]: HL diagonal, bL
    const double *__restrict__ ns;     // [win][7][n] nullspaces (iteration >= 2)
    double *x;                         // [vec]
    const double *adH, *adT;           // k_solve_reg with xad non-null: also the resubstitution's
    float *xad;                        // xAd from the solution (k_xad fused)
    const double *prep_nm, *prep_g;    // k_ortho_prep's results: Nm [vec][n_null], per window G | G^-1 | fast
    int iteration, n_null;
    int *stop, *status;  // ldso_ba_optimize: windows with iteration >= stop skip; a NaN x marks the window lost
    // ldso_ba_optimize without a communicator (k_solve_fast): blocks [n_win, 2 n_win) compute the
    // sumNID / numID of the step that follows (nid_chain) over the idepths this solve's system was
    // linearised at -- a chain of ~P dependent float adds that fits inside the solve's own time
    double *win_nid;
    NidSrc nid_src;
    int n_win, nid_chunk;
};
constexpr int kPrepGStride = 192;  // doubles per window in prep_g: G [49], G^-1 [49], fast flag, V [49], ev [7], keep [7]
// H's row stride in LDS: odd (in doubles), so a column walk touches 32 distinct bank pairs
__host__ __device__ inline int solve_ld(int n) { return n | 1; }
__host__ __device__ inline size_t solve_smem_bytes(int n) {
    return ((size_t)n * solve_ld(n) + 7 * (size_t)n + 9 * (size_t)n + 7 * 7 * 3 + 64) * sizeof(double) +
           ((size_t)n + 1) * sizeof(int) + kSolveThreads * sizeof(double);
}

// wave-wide maximum of a 64-bit key, broadcast to every lane: inclusive max-scan within each
// row of 16 (row_shr 1/2/4/8), then row_bcast15 / row_bcast31 carry rows 0-2 into lane 63.
// Keys >= 0 with 0 as identity; every lane of the wave must be active.
__device__ __forceinline__ unsigned long long wave_max_u64(unsigned long long x) {
#define LDSO_DPP_MAX(CTRL, ROWS)                                                                  \
    {                                                                                             \
        const unsigned lo = (unsigned)__builtin_amdgcn_update_dpp(0, (int)(unsigned)x, CTRL, ROWS, 0xF, true); \
        const unsigned hi = (unsigned)__builtin_amdgcn_update_dpp(0, (int)(unsigned)(x >> 32), CTRL, ROWS, 0xF, true); \
        const unsigned long long o = ((unsigned long long)hi << 32) | lo;                         \
        x = o > x ? o : x;                                                                        \
    }
    LDSO_DPP_MAX(0x111, 0xF)
    LDSO_DPP_MAX(0x112, 0xF)
    LDSO_DPP_MAX(0x114, 0xF)
    LDSO_DPP_MAX(0x118, 0xF)
    LDSO_DPP_MAX(0x142, 0xA)
    LDSO_DPP_MAX(0x143, 0xC)
#undef LDSO_DPP_MAX
    const unsigned lo = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)x, 63);
    const unsigned hi = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)(x >> 32), 63);
    return ((unsigned long long)hi << 32) | lo;
}

// LDS layout shared by both solve kernels (doubles unless noted)
struct SolveLds {
    double *H, *b, *sc, *y, *col, *Nm, *lr, *G, *V, *Gi, *misc;
    int *perm;
    __device__ SolveLds(double *lds, int n) {
        H = lds;                  // [n][ld] row-major (the host's [n][n]); lower triangle used
        b = H + (size_t)n * solve_ld(n);
        sc = b + n;
        y = sc + n;
        col = y + n;
        Nm = col + n;             // [n][7]
        lr = Nm + 7 * (size_t)n;  // [n]
        G = lr + n;
        V = G + 49;
        Gi = V + 49;              // (N^T N)^-1 of the fast projection path
        misc = Gi + 49;           // ntx[7], fast flag, coef[7], rd
        perm = reinterpret_cast<int *>(misc + 16);
    }
};

// ---- assembly (EnergyFunctional.cc:342-378), every thread of the block, each element in the
// host's order of operations: H = (HL + 0) + HA, diagonal *= (1 + lambda), H -= Hsc * scl,
// mirror, H(i,j) *= s_i s_j.  Every global load is issued up front (one memory round trip):
// the packed upper elements f = tid + kThreads u, and for row tid < n its diagonal, prior and
// b terms; the Jacobi scale of row tid from its diagonal, a barrier, then every element
// straight into its scaled lower position (c, r) (products of two scales commute exactly).
// Ends with a block barrier.
template <int kThreads>
__device__ __forceinline__ void solve_assemble(const SolveParams &P, const WinDev &W, const SolveLds &S, int tid) {
#pragma clang fp contract(off)
    const int n = W.D, ld = solve_ld(n);
    const long long pl = packed_len(n);
    const double *HA = P.sys + W.sys_base, *bA = HA + pl, *Hs = HA + pl + n, *bs = HA + 2 * pl + n;
    const double lambda = 1e-5;  // SOLVER_FIX_LAMBDA
    const double scl = 1.0f / (1 + lambda);
    auto element = [&](bool diag, double prior, double ha, double hs) {
        double h = ((diag ? prior : 0.0) + 0.0) + ha;
        if (diag) h *= (1 + lambda);
        return h - hs * scl;
    };
    constexpr int kPer = (int)((kSolveMaxDim * (kSolveMaxDim + 1) / 2 + kThreads - 1) / kThreads);
    static_assert(kSolveMaxDim <= kThreads, "one row per thread for the diagonal terms");
    // element u of this thread: f = tid + kThreads u in the "folded" order of the packed upper
    // triangle (row p paired with row n-1-p: n/2 rows of n+1 elements, n = 8N+4 is even), decoded
    // without loops; then unconditional loads at clamped positions (a guarded load becomes a
    // branch with its own wait)
    const int np1 = n + 1;
    const float inv = 1.0f / (float)np1;
    int rr[kPer], cc[kPer];
    double ha[kPer], hs[kPer];
#pragma unroll
    for (int u = 0; u < kPer; u++) {
        const int f = min(tid + kThreads * u, (int)pl - 1);
        int p = (int)((float)f * inv);
        p = p * np1 > f ? p - 1 : ((p + 1) * np1 <= f ? p + 1 : p);
        const int o = f - p * np1;
        const bool first = o < n - p;
        const int r = first ? p : n - 1 - p;
        rr[u] = r;
        cc[u] = first ? p + o : r + (o - (n - p));
        const int q = r * (2 * n - r + 1) / 2 + (cc[u] - r);  // pk_index(r, c, n)
        ha[u] = HA[q];
        hs[u] = Hs[q];
    }
    const int tr = min(tid, n - 1);
    const long long qd = pk_index(tr, tr, n);
    const double dha = HA[qd], dhs = Hs[qd], dpr = P.prior[2 * (W.vec_base + tr)],
                 bpr = P.prior[2 * (W.vec_base + tr) + 1], ba = bA[tr], bsv = bs[tr];
    double sci = 0, hdiag = 0;
    if (tid < n) {
        hdiag = element(true, dpr, dha, dhs);
        sci = 1.0 / sqrt(hdiag + 10);
        S.sc[tid] = sci;
        S.perm[tid] = tid;
    }
    __syncthreads();
    if (tid < n) {
        S.b[tid] = (((bpr + 0.0) + ba) - bsv / (1 + lambda)) * sci;
        S.H[tid * ld + tid] = hdiag * (sci * sci);
    }
#pragma unroll
    for (int u = 0; u < kPer; u++) {
        const int f = tid + kThreads * u, r = rr[u], c = cc[u];
        if (f < pl && r != c) S.H[c * ld + r] = element(false, 0.0, ha[u], hs[u]) * (S.sc[c] * S.sc[r]);
    }
    __syncthreads();
}

// ---- orthogonalize (EnergyFunctional.cc:809-841), iteration >= 2: x -= N (N^T N)^+ N^T x.
// solve_ortho_prepare (one wavefront) does the x-independent half -- normalised nullspaces Nm,
// G = Nm^T Nm and, for 7 nullspaces, the fast path's G^-1 (gram_pinv7; misc[7] = 1 when it
// applies) -- so it can run beside the factorisation; raw: >= 7 n doubles of free LDS.
__device__ __forceinline__ void solve_ortho_prepare(const SolveParams &P, const WinDev &W, const SolveLds &S,
                                                    double *raw, int lane) {
#pragma clang fp contract(off)
    const int n = W.D, kk = P.n_null;
    double *Nm = S.Nm, *lr = S.lr, *G = S.G, *V = S.V;
    const double *ns = P.ns + (size_t)7 * W.vec_base;
    for (int e = lane; e < kk * n; e += 64) raw[e] = ns[e];  // raw nullspaces [kk][n], coalesced
    wave_lds_sync();
    if (lane < kk) {
        double s2 = 0;
#pragma unroll 1
        for (int i0 = 0; i0 < n; i0 += 4) {
            double p[4];
#pragma unroll
            for (int u = 0; u < 4; u++) {
                const double v = raw[lane * n + min(i0 + u, n - 1)];
                p[u] = v * v;
            }
#pragma unroll
            for (int u = 0; u < 4; u++) s2 = i0 + u < n ? s2 + p[u] : s2;
        }
        lr[lane] = sqrt(s2);
    }
    wave_lds_sync();
    for (int e = lane; e < kk * n; e += 64) {
        const int i = e / kk, a = e - i * kk;
        Nm[e] = raw[a * n + i] / lr[a];
    }
    wave_lds_sync();
    if (lane < kk * kk) {
        const int a = lane / kk, c = lane % kk;
        double g = 0.0;
#pragma unroll 1
        for (int i0 = 0; i0 < n; i0 += 4) {
            double p[4];
#pragma unroll
            for (int u = 0; u < 4; u++) {
                const int ic = min(i0 + u, n - 1);
                p[u] = Nm[(size_t)ic * kk + a] * Nm[(size_t)ic * kk + c];
            }
#pragma unroll
            for (int u = 0; u < 4; u++) g = i0 + u < n ? g + p[u] : g;
        }
        G[lane] = g;
        V[lane] = a == c ? 1.0 : 0.0;
    }
    wave_lds_sync();
    bool fast = false;
    if (kk == 7) {  // every lane redundantly; lane 0 stores
        double g[7][7], gi[7][7];
#pragma unroll
        for (int r = 0; r < 7; r++)
#pragma unroll
            for (int q = 0; q < 7; q++) g[r][q] = G[r * 7 + q];
        fast = gram_pinv7(g, gi);
        if (lane == 0 && fast)
#pragma unroll
            for (int r = 0; r < 7; r++)
#pragma unroll
                for (int q = 0; q < 7; q++) S.Gi[r * 7 + q] = gi[r][q];
    }
    if (lane == 0) S.misc[7] = fast ? 1.0 : 0.0;
    if (!fast) {  // the round-robin Jacobi eigen-decomposition of host_math.cpp project_out (lane 0)
        if (lane == 0) {
            double g[7][7], v[7][7];
#pragma unroll
            for (int r = 0; r < 7; r++)
#pragma unroll
                for (int q = 0; q < 7; q++) {
                    g[r][q] = r < kk && q < kk ? G[r * kk + q] : 0.0;
                    v[r][q] = r == q ? 1.0 : 0.0;
                }
            for (int sweep = 0; sweep < 64; sweep++) {
                double off = 0;
                for (int p = 0; p < 7; p++)
                    for (int q = p + 1; q < 7; q++)
                        if (q < kk) off += g[p][q] * g[p][q];
                if (off < 1e-30) break;
                for (int rd = 0; rd < 7; rd++) {
                    double c[3], sn[3];
                    bool on[3];
                    for (int e = 0; e < 3; e++) {
                        const int p = kJacobiRounds[rd][e][0], q = kJacobiRounds[rd][e][1];
                        const double apq = g[p][q];
                        on[e] = q < kk && apq != 0;
                        const double th = (g[q][q] - g[p][p]) / (2 * apq);
                        const double t = (th >= 0 ? 1.0 : -1.0) / (fabs(th) + sqrt(th * th + 1));
                        c[e] = 1 / sqrt(t * t + 1);
                        sn[e] = t * c[e];
                    }
                    for (int e = 0; e < 3; e++) {  // column phase
                        const int p = kJacobiRounds[rd][e][0], q = kJacobiRounds[rd][e][1];
                        if (!on[e]) continue;
                        for (int r = 0; r < 7; r++) {
                            const double gp = g[r][p], gq = g[r][q];
                            g[r][p] = c[e] * gp - sn[e] * gq;
                            g[r][q] = sn[e] * gp + c[e] * gq;
                        }
                    }
                    for (int e = 0; e < 3; e++) {  // row phase, then V
                        const int p = kJacobiRounds[rd][e][0], q = kJacobiRounds[rd][e][1];
                        if (!on[e]) continue;
                        for (int r = 0; r < 7; r++) {
                            const double gp = g[p][r], gq = g[q][r];
                            g[p][r] = c[e] * gp - sn[e] * gq;
                            g[q][r] = sn[e] * gp + c[e] * gq;
                            const double vp = v[r][p], vq = v[r][q];
                            v[r][p] = c[e] * vp - sn[e] * vq;
                            v[r][q] = sn[e] * vp + c[e] * vq;
                        }
                    }
                }
            }
            double smax = 0;
            for (int e = 0; e < 7; e++)
                if (e < kk) smax = fmax(smax, sqrt(fmax(0.0, g[e][e])));
            for (int e = 0; e < 7; e++) {
                S.lr[e] = g[e][e];  // eigenvalue
                S.lr[7 + e] = e < kk && sqrt(fmax(0.0, g[e][e])) > kSolverModeDelta * smax ? 1.0 : 0.0;
                for (int a = 0; a < 7; a++) V[a * 7 + e] = v[a][e];
            }
        }
    }
    wave_lds_sync();
}

// k_ortho_prep runs solve_ortho_prepare once per nullspace upload (the nullspaces, hence Nm, G
// and G^-1, stay fixed over an optimize() call and usually over consecutive iterate calls); the
// solve kernels load the results with their assembly loads, every thread, before the assembly's
// barriers.
__device__ __forceinline__ void solve_ortho_load(const SolveParams &P, const WinDev &W, const SolveLds &S, int tid,
                                                 int nthreads) {
    if (P.iteration < 2 || P.n_null <= 0) return;
    const int n = W.D, kk = P.n_null;
    const double *nm = P.prep_nm + (size_t)7 * W.vec_base, *g = P.prep_g + (size_t)kPrepGStride * blockIdx.x;
    for (int e = tid; e < kk * n; e += nthreads) S.Nm[e] = nm[e];
    if (tid < 49) {
        S.G[tid] = g[tid];
        S.Gi[tid] = g[49 + tid];
        S.V[tid] = g[99 + tid];
    }
    if (tid < 14) S.lr[tid] = g[148 + tid];  // eigenvalues, kept modes (the Jacobi fallback)
    if (tid == 0) S.misc[7] = g[98];
}

// solve_ortho_load split in two for k_solve_fast: the loads into registers at kernel start (their
// round trip overlaps the assembly's), the LDS stores after the assembly (read only after the
// factorisation's barriers).  Thread tid holds Nm elements tid + k nthreads (k < 2: n <= 92, 7 n <=
// 2 x 512) and, below 49 / 14 / 1, its G / G^-1 / V, lr and fast-flag entries.
struct OrthoPre {
    double nm[2], g, gi, v, lr, fast;
    bool on;
    __device__ void load(const SolveParams &P, const WinDev &W, int tid, int nthreads) {
        on = P.iteration >= 2 && P.n_null > 0;
        if (!on) return;
        const int n = W.D, kk = P.n_null;
        const double *pnm = P.prep_nm + (size_t)7 * W.vec_base, *pg = P.prep_g + (size_t)kPrepGStride * blockIdx.x;
#pragma unroll
        for (int k = 0; k < 2; k++) nm[k] = pnm[min(tid + k * nthreads, kk * n - 1)];
        const int t49 = min(tid, 48), t14 = min(tid, 13);
        g = pg[t49];
        gi = pg[49 + t49];
        v = pg[99 + t49];
        lr = pg[148 + t14];
        fast = pg[98];
    }
    __device__ void store(const SolveParams &P, const WinDev &W, const SolveLds &S, int tid, int nthreads) const {
        if (!on) return;
        const int n = W.D, kk = P.n_null;
#pragma unroll
        for (int k = 0; k < 2; k++)
            if (tid + k * nthreads < kk * n) S.Nm[tid + k * nthreads] = nm[k];
        if (tid < 49) {
            S.G[tid] = g;
            S.Gi[tid] = gi;
            S.V[tid] = v;
        }
        if (tid < 14) S.lr[tid] = lr;
        if (tid == 0) S.misc[7] = fast;
    }
};

__global__ __launch_bounds__(64) void k_ortho_prep(SolveParams P, double *prep_nm, double *prep_g) {
    extern __shared__ double lds[];
    const WinDev W = P.wins[blockIdx.x];
    const int n = W.D, kk = P.n_null, lane = threadIdx.x;
    const SolveLds S(lds, n);
    double *raw = lds + (solve_smem_bytes(n) + 15) / 16 * 2;
    solve_ortho_prepare(P, W, S, raw, lane);  // ends with its results visible to the wave
    double *nm = prep_nm + (size_t)7 * W.vec_base, *g = prep_g + (size_t)kPrepGStride * blockIdx.x;
    for (int e = lane; e < kk * n; e += 64) nm[e] = S.Nm[e];
    if (lane < 49) {
        g[lane] = S.G[lane];
        g[49 + lane] = S.Gi[lane];
        g[99 + lane] = S.V[lane];
    }
    if (lane < 14) g[148 + lane] = S.lr[lane];
    if (lane == 0) g[98] = S.misc[7];
}

// the x-dependent half (one wavefront, after solve_ortho_load's results are visible): N^T y,
// coef = G^-1 N^T y (fast path) or the round-robin Jacobi pseudo-inverse of host_math.cpp
// project_out, y -= Nm coef; then x (= y) to global memory.
__device__ __forceinline__ void solve_ortho_apply_store(const SolveParams &P, const WinDev &W, const SolveLds &S,
                                                        int lane) {
#pragma clang fp contract(off)
    const int n = W.D;
    double *y = S.y, *Nm = S.Nm;
    const int kk = P.n_null;
    if (P.iteration >= 2 && kk > 0) {
        double *ntx = S.misc, *coef = S.misc + 8;
        if (lane < kk) {  // t += Nm(i, a) y(i) in row order; only the adds chain (no selects on it):
                          // blocks of 4 rows whose operands are loaded one block ahead, then the tail
            double t = 0.0;
            const int a = lane, nb = n >> 2;
            double cn[4], cy[4], nn[4], ny[4];
            auto ld4 = [&](int blk, double (&m)[4], double (&v)[4]) {
#pragma unroll
                for (int u = 0; u < 4; u++) {
                    m[u] = Nm[(size_t)(4 * blk + u) * kk + a];
                    v[u] = y[4 * blk + u];
                }
            };
            if (nb > 0) ld4(0, cn, cy);
#pragma unroll 1
            for (int bk = 0; bk < nb; bk++) {
                ld4(min(bk + 1, nb - 1), nn, ny);
#pragma unroll
                for (int u = 0; u < 4; u++) {
                    const double p = cn[u] * cy[u];
                    t += p;
                }
#pragma unroll
                for (int u = 0; u < 4; u++) {
                    cn[u] = nn[u];
                    cy[u] = ny[u];
                }
            }
            for (int i = 4 * nb; i < n; i++) {
                const double p = Nm[(size_t)i * kk + a] * y[i];
                t += p;
            }
            ntx[lane] = t;
            coef[lane] = 0.0;
        }
        wave_lds_sync();
        if (kk == 7 && S.misc[7] != 0.0) {  // fast path: coef = G^-1 N^T y, one row per lane
            if (lane < 7) {
                double gr[7], nt[7];
#pragma unroll
                for (int b = 0; b < 7; b++) {
                    gr[b] = S.Gi[7 * lane + b];
                    nt[b] = ntx[b];
                }
                coef[lane] = gram_apply7_row(gr, nt);
            }
        } else {  // (NtN)^+ NtX from k_ortho_prep's eigen-decomposition (V, eigenvalues, kept modes)
            if (lane < kk) {
                const double *V = S.V, *ev = S.lr, *keep = S.lr + 7;
                double cf = 0, nt[7];
#pragma unroll
                for (int a = 0; a < 7; a++) nt[a] = a < kk ? ntx[a] : 0.0;
#pragma unroll
                for (int e = 0; e < 7; e++) {  // host_math.cpp project_out's accumulation, row `lane`
                    if (e >= kk || keep[e] == 0.0) continue;
                    double proj = 0;
#pragma unroll
                    for (int a = 0; a < 7; a++)
                        if (a < kk) proj += V[a * 7 + e] * nt[a];
                    cf += V[lane * 7 + e] * proj / ev[e];
                }
                coef[lane] = cf;
            }
        }
        wave_lds_sync();
        for (int i = lane; i < n; i += 64) {
            double t = 0;
#pragma unroll
            for (int a = 0; a < 7; a++) {
                const int ac = min(a, kk - 1);
                const double p = Nm[(size_t)i * kk + ac] * coef[ac];
                t = a < kk ? t + p : t;
            }
            y[i] -= t;
        }
        wave_lds_sync();
    }
    bool nan = false;
    for (int i = lane; i < n; i += 64) {
        P.x[W.vec_base + i] = y[i];
        nan |= isnan(y[i]);
    }
    // FullSystem::optimize (FullSystem.cc:907-911): isnan(lastX.norm()) -- a NaN element (inf
    // elements give an inf norm, not NaN) -- is isLost: no step in this iteration, the loop ends
    if (P.stop && __any(nan) && lane == 0) {
        P.stop[blockIdx.x] = P.iteration;
        P.status[blockIdx.x] = LDSO_BA_OPT_LOST;
    }
}

// The trailing update of step k is A(i,j) = fma(-(c_i c_j), 1/d, A(i,j)) with c = column k and
// d the pivot (host_math.cpp ldlt_solve states the same): symmetric in i and j, so a kernel may
// hold both triangles and update either copy; L(i,k) = c_i / d is the exact quotient.
__global__ __launch_bounds__(kSolveThreads) void k_solve(SolveParams P) {
#pragma clang fp contract(off)
    extern __shared__ double lds[];
    if (P.stop && P.iteration >= P.stop[blockIdx.x]) return;  // the window left the GN loop
    const WinDev W = P.wins[blockIdx.x];  // a register copy: the helpers would re-read global memory after every LDS store
    const int n = W.D, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int ld = solve_ld(n);
    const SolveLds S(lds, n);
    double *H = S.H, *b = S.b, *sc = S.sc, *y = S.y, *col = S.col, *misc = S.misc;
    int *perm = S.perm;
    // one private dummy slot per thread: masked-off update elements land there (no branches)
    double *dummy = reinterpret_cast<double *>(perm + (n + 1) / 2 * 2) + tid;
    // Strictly-lower elements (i, j), j < i, ordered by column j descending: the elements LDL^T
    // step k updates (k < j < i) are exactly a prefix, so every step is element-parallel.  Wave w
    // lane l always owns the elements e = l + 64 (w + 4 t).  Column n-2-mm holds mm+1 elements
    // and starts at e = mm (mm + 1) / 2.  Entry: offset of (i, j) in H (16 bits) | i << 16 | j << 23.
    constexpr int kWaves = kSolveThreads / 64;
    constexpr int kOffRegs = ((kSolveMaxDim - 1) * kSolveMaxDim / 2 + 64 * kWaves - 1) / (64 * kWaves);
    int tri[kOffRegs];
    const int noff = n * (n - 1) / 2;
#pragma unroll
    for (int t = 0; t < kOffRegs; t++) {
        const int e = lane + 64 * (wave + kWaves * t);
        int mm = (int)((sqrtf(8.0f * e + 1.0f) - 1.0f) * 0.5f);
        if (mm * (mm + 1) / 2 > e) mm--;
        if ((mm + 1) * (mm + 2) / 2 <= e) mm++;
        const int j = n - 2 - mm, i = j + 1 + (e - mm * (mm + 1) / 2);
        tri[t] = e < noff ? ((i * ld + j) | (i << 16) | (j << 23)) : 0;  // padding: (0, 0), never stored
    }
    auto at = [&](int r, int c) -> double & { return H[r * ld + c]; };
    solve_ortho_load(P, W, S, tid, kSolveThreads);
    solve_assemble<kSolveThreads>(P, W, S, tid);
    // ---- LDL^T with symmetric diagonal pivoting (lower triangle).  Wave 0 runs the serial part
    // of each step (pivot, swap, column k) with the diagonal in its registers (lane i mod 64); all
    // waves then share the trailing update.
    double dg0 = lane < n ? at(lane, lane) : 0.0, dg1 = lane + 64 < n ? at(lane + 64, lane + 64) : 0.0;
    for (int k = 0; k < n; k++) {
        if (wave == 0) {
            // pivot = first index of the largest |diag| (the host's strict '>' scan from k: a NaN
            // never wins, except that a NaN at k itself keeps k)
            int piv;
            {
                const int i0 = lane, i1 = lane + 64;
                const bool c0 = i0 >= k && i0 < n, c1 = i1 >= k && i1 < n;
                const unsigned long long k0 = !c0 ? 0ull : (dg0 != dg0 && i0 == k) ? ~0ull : abs_key(dg0);
                const unsigned long long k1 = !c1 ? 0ull : (dg1 != dg1 && i1 == k) ? ~0ull : abs_key(dg1);
                const unsigned long long mx = wave_max_u64(k0 > k1 ? k0 : k1);
                const unsigned long long b0 = __ballot(c0 && k0 == mx);
                piv = b0 ? __builtin_ctzll(b0) : 64 + __builtin_ctzll(__ballot(c1 && k1 == mx));
            }
            // symmetric swap k <-> piv (lower triangle: (k,j)<->(piv,j) for j < k, (i,k)<->(piv,i)
            // for k < i < piv, (i,k)<->(i,piv) for i > piv, the two diagonals), fused with taking
            // column k: col = the new A(i,k), L(i,k) = col / d written back; the diagonal's share
            // of the trailing update happens here
            const double dk = readlane_f64(k < 64 ? dg0 : dg1, k & 63);
            const double d = readlane_f64(piv < 64 ? dg0 : dg1, piv & 63);
            const double rd = d != 0 ? 1.0 / d : 0.0;
            if (piv != k) {
                if (lane == (k & 63)) (k < 64 ? dg0 : dg1) = d;
                if (lane == (piv & 63)) (piv < 64 ? dg0 : dg1) = dk;
                for (int j = lane; j < k; j += 64) {
                    const double t = at(k, j), u = at(piv, j);
                    at(k, j) = u;
                    at(piv, j) = t;
                }
            }
#pragma unroll
            for (int sgm = 0; sgm < 2; sgm++) {
                const int i = lane + 64 * sgm;
                if (i <= k || i >= n) continue;
                double *own = &at(i, k);
                double *src = piv == k || i == piv ? own : (i < piv ? &at(piv, i) : &at(i, piv));
                const double old = *own, v = *src;
                *(src != own ? src : dummy) = old;
                col[i] = v;
                *own = d != 0 ? v / d : 0.0;
                double &dgi = sgm == 0 ? dg0 : dg1;
                dgi = fma(-(v * v), rd, dgi);
            }
            if (lane == 0) {
                misc[15] = rd;
                if (piv != k) {
                    const int pt = perm[k];
                    perm[k] = perm[piv];
                    perm[piv] = pt;
                }
            }
        }
        __syncthreads();
        const int m = (n - k - 2) * (n - k - 1) / 2;  // off-diagonal elements with k < j < i
        const double rd = misc[15];
        constexpr int kUpdBatch = 6;
#pragma unroll
        for (int t0 = 0; t0 < kOffRegs; t0 += kUpdBatch) {
            if (64 * (wave + kWaves * t0) >= m) continue;  // uniform per wave: chunks past the prefix
            double a[kUpdBatch], ci[kUpdBatch], cj[kUpdBatch], *dst[kUpdBatch];
#pragma unroll
            for (int u = 0; u < kUpdBatch; u++) {
                if (t0 + u >= kOffRegs) continue;
                const int x = tri[t0 + u], off = x & 0xFFFF, i = (x >> 16) & 0x7F, j = x >> 23;
                ci[u] = col[i];
                cj[u] = col[j];
                a[u] = H[off];
                dst[u] = lane + 64 * (wave + kWaves * (t0 + u)) < m ? H + off : dummy;
            }
#pragma unroll
            for (int u = 0; u < kUpdBatch; u++) {
                if (t0 + u >= kOffRegs) continue;
                *dst[u] = fma(-(ci[u] * cj[u]), rd, a[u]);
            }
        }
        __syncthreads();
    }
    if (wave != 0) return;  // the rest is one wavefront's work (wave-level synchronisation only)
    if (lane < n) at(lane, lane) = dg0;
    if (lane + 64 < n) at(lane + 64, lane + 64) = dg1;
    wave_lds_sync();
    // ---- substitutions (column by column, as the host); y[i] lives in lane i (mod 64); the
    // matrix entries of the next 4 columns are loaded ahead of the dependent chain
    const int ia = lane, ib = lane + 64, ra = min(ia, n - 1), rb = min(ib, n - 1);
    double ya = ia < n ? b[perm[ia]] : 0.0, yb = ib < n ? b[perm[ib]] : 0.0;
    constexpr int kSubAhead = 4;
    for (int j0 = 0; j0 < n; j0 += kSubAhead) {
        double fa[kSubAhead], fb[kSubAhead];
#pragma unroll
        for (int u = 0; u < kSubAhead; u++) {
            const int j = min(j0 + u, n - 1);
            fa[u] = at(ra, j);
            fb[u] = at(rb, j);
        }
#pragma unroll
        for (int u = 0; u < kSubAhead; u++) {
            const int j = j0 + u;
            if (j >= n) break;
            const double yj = j < 64 ? readlane_f64(ya, j) : readlane_f64(yb, j - 64);
            if (ia > j && ia < n) ya = fma(-fa[u], yj, ya);
            if (ib > j && ib < n) yb = fma(-fb[u], yj, yb);
        }
    }
    if (ia < n) ya = at(ia, ia) != 0 ? ya / at(ia, ia) : 0.0;
    if (ib < n) yb = at(ib, ib) != 0 ? yb / at(ib, ib) : 0.0;
    for (int j0 = n - 1; j0 >= 0; j0 -= kSubAhead) {
        double fa[kSubAhead], fb[kSubAhead];
#pragma unroll
        for (int u = 0; u < kSubAhead; u++) {
            const int j = max(j0 - u, 0);
            fa[u] = at(j, ra);
            fb[u] = at(j, rb);
        }
#pragma unroll
        for (int u = 0; u < kSubAhead; u++) {
            const int j = j0 - u;
            if (j < 0) break;
            const double yj = j < 64 ? readlane_f64(ya, j) : readlane_f64(yb, j - 64);
            if (ia < j) ya = fma(-fa[u], yj, ya);
            if (ib < j) yb = fma(-fb[u], yj, yb);
        }
    }
    if (ia < n) b[perm[ia]] = ya;
    if (ib < n) b[perm[ib]] = yb;
    wave_lds_sync();
    for (int i = lane; i < n; i += 64) y[i] = sc[i] * b[i];  // x
    wave_lds_sync();
    solve_ortho_apply_store(P, W, S, lane);
}

}  // namespace
