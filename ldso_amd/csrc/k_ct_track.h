// k_ct_track.h -- trackNewestCoarse's whole LM loop (CoarseTracker.cc:61-310) in one launch:
//   k_ct_track   grid.x = starts, one workgroup per start.  The workgroup walks the levels and the LM
//                iterations itself: all lanes evaluate calcRes + calcGSSSE at the pose lane 0 set up
//                (ct_res_point, the function k_ct_calc_res<true> calls, with nothing written per
//                point), lane 0 runs ct_lm.h's state machine on the sums.  No workgroup reads what
//                another wrote: the only synchronisation is __syncthreads() and the kernel boundary.
// The sums are bitwise those of ldso_ct_calc_res_gs: a chunk of 256 consecutive points is that
// kernel's block -- each wave reduced in double with the xor tree, the four waves combined as
// (w0 + w1) + (w2 + w3) -- and the chunk partials are added in chunk order in double; a workgroup
// of kWaves wavefronts takes kWaves / 4 chunks per sweep.  The constants of an evaluation and the
// Vec6, H and b from its sums are ct_eval.h's, the same functions the host entry points call.
#pragma once
#include <cstdint>

#include "ct_lm.h"
#include "k_ct_residual.h"

#pragma clang fp contract(off)

namespace {

constexpr int kTrackWaves = 8;  // 512 lanes, two chunks per sweep: 147 VGPRs per lane, no spill
constexpr int kTrackSums = kResParts + kGsParts;

struct CtTrackStart {  // one start, in mapped host memory
    double ref_to_new[12], aff[2], min_res[5];
};
struct CtTrackParams {
    CtLevel lv[5];
    ldso_ct_track_params p;
    const CtTrackStart *starts;
    ldso_ct_track_result *out;
    ldso_ct_track_step *trace;  // start 0's evaluations (may be null)
    int *trace_n;
    int trace_capacity, coarsest;
    float ref_exposure, new_exposure, ref_a, ref_b;
};
struct CtTrackEval {  // what lane 0 hands to the sweep
    CtPose pose;
    CtEvalTerms ev;
    int lvl, more;
};

// the constants of the evaluation the state machine asks for
__device__ inline void ct_track_setup(const CtTrackParams &P, const ldso_ct::Track &T, CtTrackEval &E) {
    ldso_ct::ct_eval_setup(T.eval_pose, P.lv[T.lvl].Ki, P.ref_exposure, P.new_exposure, P.ref_a, P.ref_b, T.eval_aff[0],
                           T.eval_aff[1], T.cutoff(), E.pose, E.ev);
    E.lvl = T.lvl;
}

// the Vec6, H and b from the sums s [kTrackSums], one output per lane
__device__ inline void ct_track_finish(const double *s, int tid, double *rs, double *H, double *b) {
    if (tid < 72) {
        const int r = tid < 64 ? tid / 8 : tid - 64, cc = tid < 64 ? tid % 8 : 8;
        const double e = ldso_ct::ct_finish_gs_entry(s + kResParts, (int)s[6], r, cc);
        if (tid < 64)
            H[tid] = e;
        else
            b[r] = e;
    } else if (tid == 72) {
        ldso_ct::ct_finish_res(s, rs);
    }
}

// lane 0 between two evaluations: the state machine takes the sums' results and sets up what it asks
// for next.  Not inlined: the sweep's 53 double accumulators per lane keep their registers.
__device__ __noinline__ int ct_track_advance(const CtTrackParams &P, ldso_ct::Track &T, CtTrackEval &E, const double *rs,
                                             const double *Hn, const double *bn, ldso_ct_track_step *log) {
    if (!T.consume(rs, Hn, bn, log)) return 0;
    ct_track_setup(P, T, E);
    return 1;
}

// block_sum_write's wave reduction, v += __shfl_xor(v, m) for m = 32 ... 1, for all kTrackSums values at once
// and with the same bits.  In that tree every lane computes every total; here each step keeps one value of
// a pair in the lanes whose bit m is clear and the other in the lanes where it is set, so 64 values fold to
// 32, 16, ... and lane k ends with the total of value k: 63 additions per wave instead of 318, and no LDS
// permute (one workgroup has nothing to hide them under).  A lane's partial of a value equals the tree's
// partial in that lane, because after the steps above m the tree's value depends on the lower lane bits only.
//   m = 32, 16: v_permlane32_swap / v_permlane16_swap (gfx950) exchange the upper halves (odd rows) of a with
//               the lower halves (even rows) of b: a' + b' is a_i + a_(i ^ m) where bit m is clear, b's where set
//   m = 8, 2, 1: DPP row_ror:8 and two quad_perms bring the partner's value; m = 4 has no DPP control
//               (row_ror:4 reaches a lane that by now holds another value) and takes __shfl_xor for its 4 pairs
template <bool k32>
__device__ __forceinline__ double ct_track_fold_swap(double a, double b) {
    typedef unsigned uint2v __attribute__((ext_vector_type(2)));
    const unsigned alo = (unsigned)__double2loint(a), ahi = (unsigned)__double2hiint(a);
    const unsigned blo = (unsigned)__double2loint(b), bhi = (unsigned)__double2hiint(b);
    const uint2v l = k32 ? __builtin_amdgcn_permlane32_swap(alo, blo, false, false)
                         : __builtin_amdgcn_permlane16_swap(alo, blo, false, false);
    const uint2v h = k32 ? __builtin_amdgcn_permlane32_swap(ahi, bhi, false, false)
                         : __builtin_amdgcn_permlane16_swap(ahi, bhi, false, false);
    return __hiloint2double((int)h.x, (int)l.x) + __hiloint2double((int)h.y, (int)l.y);
}
template <int kCtrl>
__device__ __forceinline__ double ct_track_fold_dpp(double a, double b, bool set) {
    const double keep = set ? b : a, send = set ? a : b;
    const int lo = __builtin_amdgcn_mov_dpp(__double2loint(send), kCtrl, 0xf, 0xf, false);
    const int hi = __builtin_amdgcn_mov_dpp(__double2hiint(send), kCtrl, 0xf, 0xf, false);
    return keep + __hiloint2double(hi, lo);
}
// v [64]: the values (zero beyond kTrackSums); returns, in lane k, the wave's total of v[k]
__device__ __forceinline__ double ct_track_wave_sums(double (&v)[64], int lane) {
#pragma unroll
    for (int j = 0; j < 32; j++) v[j] = ct_track_fold_swap<true>(v[j], v[j + 32]);
#pragma unroll
    for (int j = 0; j < 16; j++) v[j] = ct_track_fold_swap<false>(v[j], v[j + 16]);
#pragma unroll
    for (int j = 0; j < 8; j++) v[j] = ct_track_fold_dpp<0x128>(v[j], v[j + 8], lane & 8);  // row_ror:8
#pragma unroll
    for (int j = 0; j < 4; j++) {  // no DPP control is lane ^ 4: the four pairs left go through the LDS permute
        const bool set = lane & 4;
        v[j] = (set ? v[j + 4] : v[j]) + __shfl_xor(set ? v[j] : v[j + 4], 4, kWave);
    }
#pragma unroll
    for (int j = 0; j < 2; j++) v[j] = ct_track_fold_dpp<0x4E>(v[j], v[j + 2], lane & 2);   // quad_perm [2, 3, 0, 1]
    return ct_track_fold_dpp<0xB1>(v[0], v[1], lane & 1);                                    // quad_perm [1, 0, 3, 2]
}

template <int kWaves>
__global__ __launch_bounds__(kWaves *kWave) void k_ct_track(CtTrackParams P) {
    static_assert(kWaves % 4 == 0, "a chunk is four wavefronts");
    constexpr int kChunks = kWaves / 4;
    __shared__ ldso_ct::Track T;
    __shared__ CtTrackEval E;
    __shared__ double red[kWaves][kTrackSums], sums[kTrackSums], rs[6], Hn[64], bn[8];
    const int tid = threadIdx.x, lane = tid & (kWave - 1), wv = tid / kWave;
    int n_eval = 0;
    if (tid == 0) {
        const CtTrackStart &S = P.starts[blockIdx.x];
        T.begin(P.p, P.coarsest, S.ref_to_new, S.aff, S.min_res, P.ref_exposure, P.new_exposure, P.ref_a, P.ref_b);
        ct_track_setup(P, T, E);
    }
    __syncthreads();
    for (;;) {
        const CtLevel &L = P.lv[E.lvl];
        const int nb = L.n > 0 ? (L.n + kCtThreads - 1) / kCtThreads : 1;
        double tot = 0;
        for (int base = 0; base < nb; base += kChunks) {
            const int i = (base + tid / kCtThreads) * kCtThreads + tid % kCtThreads;
            double v[64];  // acc [kResParts] | gs [kGsParts] | zeros
#pragma unroll
            for (int k = 0; k < 64; k++) v[k] = 0;
            float4 w0, w1;  // not formed: kWarp is false
            if (i < L.n) ct_res_point<true, false>(L, E.pose, E.ev, E.lvl, i, v, v + kResParts, w0, w1);
            const double total = ct_track_wave_sums(v, lane);
            if (lane < kTrackSums) red[wv][lane] = total;
            __syncthreads();
            if (tid < kTrackSums) {
                for (int c = 0; c < kChunks && base + c < nb; c++)
                    tot += (red[4 * c][tid] + red[4 * c + 1][tid]) + (red[4 * c + 2][tid] + red[4 * c + 3][tid]);
            }
            __syncthreads();
        }
        if (tid < kTrackSums) sums[tid] = tot;
        __syncthreads();
        ct_track_finish(sums, tid, rs, Hn, bn);
        __syncthreads();
        if (tid == 0) {
            ldso_ct_track_step *log =
                blockIdx.x == 0 && P.trace && n_eval < P.trace_capacity ? P.trace + n_eval : nullptr;
            n_eval++;
            E.more = ct_track_advance(P, T, E, rs, Hn, bn, log);
        }
        __syncthreads();
        if (!E.more) break;
    }
    if (tid == 0) {
        P.out[blockIdx.x] = T.R;
        if (blockIdx.x == 0 && P.trace_n) *P.trace_n = n_eval;
    }
}

}  // namespace
