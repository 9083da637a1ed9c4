// k_stitch.h -- the records stitch (windows of 13-16 keyframes, LDSO_BA_STITCH_RECORDS): StitchParams,
// k_stitch and k_stitch_sum.
#pragma once
#include "ba_device.h"

namespace {

// ============================================================================================
// k_stitch: one 256-thread block per frame pair (h,t) of every window, straight from the
// partial slabs of k_linearize / k_point_sc, writing the pair's contributions to the packed
// upper triangles of {HA, bA, Hsc, bsc} as one record per (pair, block) that k_stitch_sum adds
// in a fixed pair order (no atomics: the system is bitwise repeatable):
//   Top  bucket (h,t): sum the chunk partials, AccumulatorApprox::finish layout, adjoint
//        sandwiches (AccumulatedTopHessian.cc:213-239), symmetrised as stitchDoubleMT does
//        (H(a,b) = H(a,b) + H(b,a)^T, H(c,h) = H(h,c)^T; AccumulatedTopHessian.h:91-104)
//   SC   host i = h, target j = t: rows of G_i for slot j (accD/accE/accEB of
//        AccumulatedSCHessian.cc:35-50) summed from the SYRK chunk partials, then
//        AccumulatedSCHessian.cc:80-114; only the upper triangle is produced (the solve reads
//        only it, EnergyFunctional.cc:378) using D_kj = D_jk^T.
// The diagonal (h == t) blocks have no residuals; block (0,0) of each window instead runs
// setNewFrameEnergyTH (FullSystem.cc:2078-2109) and the linearizeAll energy sum.
// ============================================================================================
constexpr int kStTopLds = 528;  // doubles of k_stitch LDS used by the Top half (521, padded)
constexpr int kThMaxLds = 8192;  // k_frame_th: candidate energies staged in LDS; larger sets re-read HBM

// k_stitch's contribution record of one (h, t) pair (doubles): every term the reference's
// stitchDouble adds for this pair, stored instead of accumulated, so that k_stitch_sum can add
// each output element's terms in one fixed order (bitwise repeatable, no atomics).
//   Top  (AccumulatedTopHessian.cc:213-239): T1 (h,h) 8x8, T2 (t,t) 8x8, T3 AH A AT^T 8x8,
//        T4a/T4b the (calib, h) / (calib, t) 8x4 column blocks [rr * 4 + cc], T5 the 4x4
//        calibration block, T6a/T6b b(h) / b(t), T7 b(calib)
//   SC   (AccumulatedSCHessian.cc:80-114, i = h, j = t): S1 the (j, k) blocks for the N-1 k != i,
//        S2 H(j, i), S3 H(i, i), S4a/S4b (calib, i) / (calib, j) [rr * 4 + cc], S5a/S5b b(i) / b(j),
//        S6 accHcc / accbc [r * 5 + c] (only in the record of host i's first target)
enum : int { kT1 = 0, kT2 = 64, kT3 = 128, kT4a = 192, kT4b = 224, kT5 = 256, kT6a = 272, kT6b = 280, kT7 = 288,
             kS1 = 292 };
__host__ __device__ inline int st_S2(int N) { return kS1 + 64 * (N - 1); }

struct StitchParams {
    const WinDev *__restrict__ wins;
    const int *__restrict__ pair_win;
    const float *__restrict__ e_wo;
    float *frame_th;
    const int2 *__restrict__ pair_items;  // per global pair: {first top item, n items}
    const float *__restrict__ top_slab;
    const double *__restrict__ item_energy;
    const int2 *__restrict__ host_items;  // per global frame: {first sc item, n items}
    const float *__restrict__ sc_slab;
    const double *__restrict__ adH;
    const double *__restrict__ adT;
    double *sys;
    double *stage;  // k_stitch -> k_stitch_sum contribution records (WinDev::stage_base)
    double *win_energy;
    double *ehist;         // non-null (ldso_ba_optimize): also win_energy into row `pass` of the history
    const int *stop;       // ldso_ba_optimize (LinParams::stop): host / pair blocks of stopped windows skip
    int pass;
    int accumulate;
    int th_cap;  // newest-frame energies staged in LDS by setNewFrameEnergyTH
    int pair_base;  // first global pair of this launch
    int hs_split;   // k_stitch_host: two blocks per host (Top / SC halves)
    int dense_adt;  // k_stitch_host: the dense products for every window (else by WinDev::adt_diag)
    const int *__restrict__ frame_win;  // k_stitch_host: window of each global frame
    int frame_base;                     // k_stitch_host: first global host frame of this launch
    int win_base;   // first window of this launch
    int n_win;      // windows of this launch: blocks [0, n_win) run their setNewFrameEnergyTH
};

template <int kT>
__device__ void frame_threshold_and_energy(const StitchParams &P, const WinDev &W, int w, unsigned *keys) {
    constexpr int kW = kT / 64;
    const int tid = threadIdx.x, N = W.N;
    const float *e_wo = P.e_wo + W.newest_begin;
    select_frame_th<kT>([&](int i) { return e_wo[i]; }, W.newest_end - W.newest_begin, keys, P.th_cap,
                        P.frame_th + W.frame_base + N - 1);
    double *red = reinterpret_cast<double *>(keys + P.th_cap + kW * 256 + 16);
    // linearizeAll: sum of returned energies and #IN in a fixed order (strided per thread, then
    // a fixed tree), so repeated passes give identical sums
    double se = 0, sn = 0;
    for (int k = tid; k < W.n_top_items; k += kT) {
        se += P.item_energy[2 * (W.top_item_base + k)];
        sn += P.item_energy[2 * (W.top_item_base + k) + 1];
    }
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) {
        se += __shfl_xor(se, m, kWave);
        sn += __shfl_xor(sn, m, kWave);
    }
    if ((tid & 63) == 0) {
        red[2 * (tid >> 6)] = se;
        red[2 * (tid >> 6) + 1] = sn;
    }
    __syncthreads();
    if (tid == 0) {
        double e = 0, nin = 0;  // the waves in a fixed tree: pairs, then pairs of pairs
        if constexpr (kW == 4) {
            e = (red[0] + red[2]) + (red[4] + red[6]);
            nin = (red[1] + red[3]) + (red[5] + red[7]);
        } else {
            static_assert(kW == 8, "4 or 8 waves");
            e = ((red[0] + red[2]) + (red[4] + red[6])) + ((red[8] + red[10]) + (red[12] + red[14]));
            nin = ((red[1] + red[3]) + (red[5] + red[7])) + ((red[9] + red[11]) + (red[13] + red[15]));
        }
        P.win_energy[2 * w] = e;
        P.win_energy[2 * w + 1] = nin;
        if (P.ehist) {  // the optimize() energy history, without a launch of its own
            double *hs = P.ehist + (size_t)P.pass * 2 * P.n_win;
            hs[2 * w] = e;
            hs[2 * w + 1] = nin;
        }
    }
}

// element (row, col) of G_h summed over the host's SYRK chunk partials (upper tiles only)
__device__ __forceinline__ double g_elem(const float *__restrict__ slab, int n_items, int per, int nt, int row,
                                         int col) {
    if (row > col) {
        const int t = row;
        row = col;
        col = t;
    }
    const int a = row >> 2, b = col >> 2;
    const int tile = a * nt - a * (a - 1) / 2 + (b - a);
    const float *src = slab + (size_t)tile * 16 + ((row & 3) << 2) + (col & 3);
    double s0 = 0, s1 = 0, s2 = 0, s3 = 0;  // 4 independent loads in flight
    int k = 0;
    for (; k + 4 <= n_items; k += 4) {
        s0 += (double)src[(size_t)k * per];
        s1 += (double)src[(size_t)(k + 1) * per];
        s2 += (double)src[(size_t)(k + 2) * per];
        s3 += (double)src[(size_t)(k + 3) * per];
    }
    for (; k < n_items; k++) s0 += (double)src[(size_t)k * per];
    return (s0 + s1) + (s2 + s3);
}

__global__ __launch_bounds__(kStThreads) void k_stitch(StitchParams P) {
    extern __shared__ double sm[];  // sized on the host for the largest window (stitch_smem_bytes)
    if ((int)blockIdx.x < P.n_win) {  // the longest single-block chain goes first in the grid
        const int w = P.win_base + blockIdx.x;
        frame_threshold_and_energy<kStThreads>(P, P.wins[w], w, reinterpret_cast<unsigned *>(sm));
        return;
    }
    const int pair = P.pair_base + blockIdx.x - P.n_win;
    const int w = P.pair_win[pair];
    if (P.stop && P.pass > P.stop[w]) return;  // window left the GN loop: its records stay as they are
    const WinDev &W = P.wins[w];
    const int N = W.N, D = W.D, aidx = pair - W.pair_base, h = aidx % N, t = aidx / N;
    const int tid = threadIdx.x;
    if (h == t) return;
    if (!P.accumulate) return;
    (void)D;
    double *rec = P.stage + W.stage_base + (size_t)aidx * stage_rec(N);

    // All global loads of both halves are issued first (one round trip for the block): the
    // Top bucket partial sums and pair adjoints, and the SC rows of G_i with the host's adjoints.
    const bool do_top = true, do_sc = true;
    double *acc = sm, *A = acc + 96, *AH = A + 169, *AT = AH + 64, *TH = AT + 64, *TT = TH + 64;  // 521
    const int i = h, j = t, KP = W.KP, nt = KP / 4, per = W.ntiles * 16, Kc = 8 * (N - 1);
    const int sj = j < i ? j : j - 1;
    double *Gj = sm + kStTopLds;           // [8][KP]: rows 8 sj.. of G_i
    double *AHk = Gj + 8 * KP;             // [N-1][64] AH_ik
    double *ATk = AHk + (N - 1) * 64;      // [N-1][64] AT_ik
    double *X = ATk + (N - 1) * 64;        // [N-1][64]
    double *Sk = X + (N - 1) * 64;         // [N-1][64]
    double *Cc = Sk + (N - 1) * 64;        // [4][5]: G_i[Kc+r][Kc+c], bc
    const double *Ah = AH, *At = AT;       // AH_ij, AT_ij are the Top pair's adjoints
    {
        const int2 pi = P.pair_items[pair];
        if (tid < kTopVals) {
            if (do_top) {
            const float *src = P.top_slab + (size_t)pi.x * kTopVals + tid;
            double s0 = 0, s1 = 0, s2 = 0, s3 = 0;
            int k = 0;
            for (; k + 4 <= pi.y; k += 4) {  // 4 independent loads in flight
                s0 += (double)src[(size_t)k * kTopVals];
                s1 += (double)src[(size_t)(k + 1) * kTopVals];
                s2 += (double)src[(size_t)(k + 2) * kTopVals];
                s3 += (double)src[(size_t)(k + 3) * kTopVals];
            }
            for (; k < pi.y; k++) s0 += (double)src[(size_t)k * kTopVals];
            acc[tid] = (s0 + s1) + (s2 + s3);
            }
        } else if (tid < kTopVals + 64) {
            AH[tid - kTopVals] = P.adH[(size_t)pair * 64 + tid - kTopVals];
        } else if (tid < kTopVals + 128) {
            AT[tid - kTopVals - 64] = P.adT[(size_t)pair * 64 + tid - kTopVals - 64];
        }
        const int2 hi = P.host_items[W.frame_base + i];
        const float *slab = P.sc_slab + W.sc_slab_base + (size_t)(hi.x - W.sc_item_base) * per;
        for (int e = do_sc ? tid : 8 * KP; e < 8 * KP; e += kStThreads) {
            const int r = e / KP, col = e % KP;
            Gj[e] = col < Kc + 5 ? g_elem(slab, hi.y, per, nt, 8 * sj + r, col) : 0.0;
        }
        if (do_sc && sj == 0 && tid < 20) {  // accHcc / accbc once per host (AccumulatedSCHessian.cc:105-113)
            const int r = tid / 5, c = tid % 5;
            Cc[tid] = g_elem(slab, hi.y, per, nt, Kc + r, Kc + c);
        }
        for (int e = do_sc ? tid : (N - 1) * 64; e < (N - 1) * 64; e += kStThreads) {
            const int s = e >> 6, k = s + (s >= i), pik = W.pair_base + i + N * k;
            AHk[e] = P.adH[(size_t)pik * 64 + (e & 63)];
            ATk[e] = P.adT[(size_t)pik * 64 + (e & 63)];
        }
    }
    __syncthreads();

    // ---------------- Top: bucket (h, t) ------------------------------------------------
    if (tid < 169) A[tid] = acc[top_slot(tid / 13, tid % 13)];
    __syncthreads();
    if (tid < 128) {
        const int l = tid & 63, r = l >> 3, c = l & 7;
        const double *Ad = tid < 64 ? AH : AT;
        double sacc = 0;
        for (int k = 0; k < 8; k++) sacc += Ad[r * 8 + k] * A[(4 + k) * 13 + 4 + c];
        (tid < 64 ? TH : TT)[l] = sacc;
    }
    __syncthreads();
    if (tid < 192) {
        const int which = tid >> 6, l = tid & 63, r = l >> 3, c = l & 7;
        double v = 0;
        if (which == 0) {  // H(h,h) += AH A AH^T
            for (int k = 0; k < 8; k++) v += TH[r * 8 + k] * AH[c * 8 + k];
            rec[kT1 + l] = v;
        } else if (which == 1) {  // H(t,t) += AT A AT^T
            for (int k = 0; k < 8; k++) v += TT[r * 8 + k] * AT[c * 8 + k];
            rec[kT2 + l] = v;
        } else {  // H(h,t) += AH A AT^T; the (t,h) term is its transpose (symmetrisation)
            for (int k = 0; k < 8; k++) v += TH[r * 8 + k] * AT[c * 8 + k];
            rec[kT3 + l] = v;
        }
    } else {  // 64 threads: H(h,c) = AH A_8C and H(t,c) = AT A_8C
        const int l = tid - 192, which = l >> 5, rr = (l & 31) >> 2, cc = l & 3;
        const double *Ad = which == 0 ? AH : AT;
        double v = 0;
        for (int k = 0; k < 8; k++) v += Ad[rr * 8 + k] * A[(4 + k) * 13 + cc];
        rec[(which == 0 ? kT4a : kT4b) + rr * 4 + cc] = v;
    }
    if (tid < 16) {
        rec[kT5 + tid] = A[(tid >> 2) * 13 + (tid & 3)];
    } else if (tid < 32) {
        const int l = tid - 16, which = l >> 3, r = l & 7;
        const double *Ad = which == 0 ? AH : AT;
        double v = 0;
        for (int k = 0; k < 8; k++) v += Ad[r * 8 + k] * A[(4 + k) * 13 + 12];
        rec[(which == 0 ? kT6a : kT6b) + r] = v;
    } else if (tid < 36) {
        rec[kT7 + tid - 32] = A[(tid - 32) * 13 + 12];
    }

    // ---------------- SC: host i = h, target j = t ---------------------------------------
    // per k != i: X_k = AT_ij D_jk, S_k = D_jk AH_ik^T
    for (int e = tid; e < (N - 1) * 64; e += kStThreads) {
        const int s = e >> 6, r = (e >> 3) & 7, c = e & 7;
        const double *Dm = Gj + 8 * s;  // D_jk[r][c] = Gj[r * KP + 8 s + c]
        double x = 0, sv = 0;
        for (int q = 0; q < 8; q++) {
            x += At[r * 8 + q] * Dm[q * KP + c];
            sv += Dm[r * KP + q] * AHk[s * 64 + c * 8 + q];
        }
        X[e] = x;
        Sk[e] = sv;
    }
    __syncthreads();
    // H(j,k) += AT_ij D_jk AT_ik^T (k_stitch_sum keeps the upper-triangle ones)
    for (int e = tid; e < (N - 1) * 64; e += kStThreads) {
        const int s = e >> 6, r = (e >> 3) & 7, c = e & 7;
        double v = 0;
        for (int q = 0; q < 8; q++) v += X[s * 64 + r * 8 + q] * ATk[s * 64 + c * 8 + q];
        rec[kS1 + e] = v;
    }
    const int s2 = st_S2(N);
    if (tid < 64) {
        const int r = tid >> 3, c = tid & 7;
        double hji = 0, hii = 0;
        for (int q = 0; q < 8; q++) {
            double sq = 0;  // S = sum_k S_k, fixed order
            for (int s = 0; s < N - 1; s++) sq += Sk[s * 64 + q * 8 + c];
            hji += At[r * 8 + q] * sq;
            hii += Ah[r * 8 + q] * sq;
        }
        rec[s2 + tid] = hji;       // H(j,i) += sum_k AT_ij D AH_ik^T
        rec[s2 + 64 + tid] = hii;  // H(i,i)
    } else if (tid < 128) {  // H(i,c) += AH_ij E, H(j,c) += AT_ij E
        const int l = tid - 64, which = l >> 5, rr = (l & 31) >> 2, cc = l & 3;
        const double *Ad = which == 0 ? Ah : At;
        double v = 0;
        for (int q = 0; q < 8; q++) v += Ad[rr * 8 + q] * Gj[q * KP + Kc + cc];
        rec[s2 + 128 + which * 32 + rr * 4 + cc] = v;
    } else if (tid < 144) {  // b(i) += AH_ij EB, b(j) += AT_ij EB
        const int l = tid - 128, which = l >> 3, rr = l & 7;
        const double *Ad = which == 0 ? Ah : At;
        double v = 0;
        for (int q = 0; q < 8; q++) v += Ad[rr * 8 + q] * Gj[q * KP + Kc + 4];
        rec[s2 + 192 + which * 8 + rr] = v;
    } else if (sj == 0 && tid < 164) {  // H_cc += accHcc, b_c += accbc (once per host)
        rec[s2 + 208 + tid - 144] = Cc[tid - 144];
    }
}

// Sum of every stitch term of one packed output element, in one fixed order over the window's
// pairs (t major, h minor): HA / bA from the Top records, Hsc / bsc from the SC records.  One
// thread per element of {HA upper, bA, Hsc upper, bsc} of every window; writes every element
// (no memset, no atomics: the stitched system is bitwise repeatable).  Each element's terms
// form one of five closed-form sequences (below), so the k-th term's record offset is a formula
// and the loads go out eight at a time instead of one per visited pair.
enum StitchSeq : int {
    kSeqAll = 0,    // every pair (h, t), h != t, one record index
    kSeqScCal = 1,  // the pairs (h, first target of h): (1..N-1, 0), then (0, 1)
    kSeqAB = 2,     // (f, t) for t < f [A], (h, f) for h != f [B], (f, t) for t > f [A]
    kSeqHaOff = 3,  // (f2, f1) then (f1, f2): H(h,t) of the two orientations
    kSeqScOff = 4   // (h, f1) for h != f1 (S2 term at h = f2, S1 otherwise), then (f1, f2)
};
struct StitchTerms {
    int seq, N, f, f2, idxA, idxB, s1rc, s2;  // s1rc >= 0: B index = kS1 + (F - (F > h)) * 64 + s1rc
    int r, c;
    __device__ int count() const {
        switch (seq) {
        case kSeqAll: return N * (N - 1);
        case kSeqScCal: return N;
        case kSeqAB: return 2 * (N - 1);
        case kSeqHaOff: return 2;
        default: return N;
        }
    }
    __device__ long long offset(int k, int R) const {
        int h, t, idx;
        switch (seq) {
        case kSeqAll: {
            t = k / (N - 1);
            const int hh = k - t * (N - 1);
            h = hh < t ? hh : hh + 1;
            idx = idxA;
            break;
        }
        case kSeqScCal:
            h = k < N - 1 ? k + 1 : 0;
            t = k < N - 1 ? 0 : 1;
            idx = idxA;
            break;
        case kSeqAB:
            if (k < f) {
                h = f;
                t = k;
                idx = idxA;
            } else if (k - f < N - 1) {
                const int kk = k - f;
                h = kk < f ? kk : kk + 1;
                t = f;
                idx = s1rc >= 0 ? kS1 + (f - (f > h ? 1 : 0)) * 64 + s1rc : idxB;
            } else {
                h = f;
                t = f + 1 + (k - f - (N - 1));
                idx = idxA;
            }
            break;
        case kSeqHaOff:
            h = k == 0 ? f2 : f;
            t = k == 0 ? f : f2;
            idx = k == 0 ? kT3 + c * 8 + r : kT3 + r * 8 + c;
            break;
        default:  // kSeqScOff, f = f1
            if (k < N - 1) {
                h = k < f ? k : k + 1;
                t = f;
                idx = h == f2 ? s2 + r * 8 + c : kS1 + (f2 - (f2 > h ? 1 : 0)) * 64 + r * 8 + c;
            } else {
                h = f;
                t = f2;
                idx = s2 + c * 8 + r;
            }
            break;
        }
        return (long long)(h + N * t) * R + idx;
    }
};
__global__ __launch_bounds__(256) void k_stitch_sum(const WinDev *__restrict__ wins, const int2 *__restrict__ blocks,
                                                     const double *__restrict__ stage, double *sys) {
    const int2 bw = blocks[blockIdx.x];  // {window, first element of this block}
    const WinDev &W = wins[bw.x];
    const int N = W.N, D = W.D;
    const long long pl = packed_len(D), n_el = 2 * (pl + D);
    const long long e = (long long)bw.y + threadIdx.x;
    if (e >= n_el) return;
    const int R = stage_rec(N), s2 = st_S2(N);
    const double *st = stage + W.stage_base;
    const bool sc = e >= pl + D;
    const long long q = sc ? e - (pl + D) : e;
    StitchTerms T;
    T.N = N;
    T.s2 = s2;
    T.s1rc = -1;
    T.f = T.f2 = T.r = T.c = 0;
    T.idxA = T.idxB = 0;
    if (q >= pl) {  // b element
        const int r = (int)(q - pl);
        if (r < 4) {
            T.seq = sc ? kSeqScCal : kSeqAll;
            T.idxA = sc ? s2 + 208 + r * 5 + 4 : kT7 + r;
        } else {
            const int rr = (r - 4) & 7;
            T.seq = kSeqAB;
            T.f = (r - 4) >> 3;
            T.idxA = (sc ? s2 + 192 : kT6a) + rr;
            T.idxB = (sc ? s2 + 200 : kT6b) + rr;
        }
    } else {  // upper element (row, col) of the packed triangle
        int row = (int)((2 * D + 1 - sqrt((double)(2 * D + 1) * (2 * D + 1) - 8.0 * (double)q)) * 0.5);
        row = row < 0 ? 0 : (row > D - 1 ? D - 1 : row);
        while (row < D - 1 && pk_index(row + 1, row + 1, D) <= q) row++;
        while (row > 0 && pk_index(row, row, D) > q) row--;
        const int col = row + (int)(q - pk_index(row, row, D));
        if (col < 4) {  // calibration block (row <= col < 4)
            T.seq = sc ? kSeqScCal : kSeqAll;
            T.idxA = sc ? s2 + 208 + row * 5 + col : kT5 + row * 4 + col;
        } else if (row < 4) {  // (calib cc = row, frame f, rr)
            const int rr = (col - 4) & 7, cc = row;
            T.seq = kSeqAB;
            T.f = (col - 4) >> 3;
            T.idxA = (sc ? s2 + 128 : kT4a) + rr * 4 + cc;
            T.idxB = (sc ? s2 + 160 : kT4b) + rr * 4 + cc;
        } else {
            const int f1 = (row - 4) >> 3, r = (row - 4) & 7, f2 = (col - 4) >> 3, c = (col - 4) & 7;
            T.r = r;
            T.c = c;
            if (f1 == f2) {
                T.seq = kSeqAB;
                T.f = f1;
                if (!sc) {
                    T.idxA = kT1 + r * 8 + c;  // h == f1
                    T.idxB = kT2 + r * 8 + c;  // t == f1
                } else {
                    T.idxA = s2 + 64 + r * 8 + c;  // i == f1: H(i,i)
                    T.s1rc = r * 8 + c;             // j == f1: H(j,j) from S1
                }
            } else {
                T.seq = sc ? kSeqScOff : kSeqHaOff;
                T.f = f1;
                T.f2 = f2;
            }
        }
    }
    const int cnt = T.count();
    double v = 0;
    constexpr int kBatch = 24;  // the 42-term calibration sums in two round trips
    for (int k0 = 0; k0 < cnt; k0 += kBatch) {
        double x[kBatch];
#pragma unroll
        for (int u = 0; u < kBatch; u++) x[u] = st[k0 + u < cnt ? T.offset(k0 + u, R) : 0];
#pragma unroll
        for (int u = 0; u < kBatch; u++)
            if (k0 + u < cnt) v += x[u];
    }
    sys[W.sys_base + e] = v;
}

}  // namespace
