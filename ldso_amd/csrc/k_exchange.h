// k_exchange.h -- the sharded threshold exchange: k_export_newest and k_frame_th.
#pragma once
#include "k_stitch.h"

namespace {

// ---- sharded setNewFrameEnergyTH ---------------------------------------
// With points sharded over ranks, the newest frame's NewEnergyWithOutlier values are spread
// over the ranks; nth_element needs all of them.  Each rank exports its newest-frame segment
// of every window into a fixed-stride slot (padding -1, which the selection skips), the host
// all-gathers the slots, and k_frame_th reruns the exact selection over all ranks' values.
// slot of window w (pitch `slot` floats): the newest-frame energies [0, stride) (padding -1), then,
// with prun > 0, the rank's |idepth| run of the window in device point order [stride, stride +
// prun) (padding 0) -- the sharded sumNID chain's input (NidSrc)
__global__ __launch_bounds__(256) void k_export_newest(const WinDev *__restrict__ wins, const float *__restrict__ e_wo,
                                                       float *out, long long stride, long long slot,
                                                       const float *__restrict__ pt_data, int prun) {
    const WinDev &W = wins[blockIdx.y];
    const int n = W.newest_end - W.newest_begin;
    float *dst = out + (size_t)blockIdx.y * slot;
    for (long long i = blockIdx.x * 256 + threadIdx.x; i < stride; i += (long long)gridDim.x * 256)
        dst[i] = i < n ? e_wo[W.newest_begin + i] : -1.0f;
    for (long long i = blockIdx.x * 256 + threadIdx.x; i < prun; i += (long long)gridDim.x * 256)
        dst[stride + i] = i < W.P ? fabsf(pt_data[(size_t)(W.point_base + i) * LDSO_BA_POINT_STRIDE + 2]) : 0.0f;
}

// blocks [0, n_win): the exact setNewFrameEnergyTH over every rank's slot; with nid.gathered, blocks
// [n_win, 2 n_win) the windows' sumNID chains over the gathered runs (ldso_ba_optimize, exact solve modes)
__global__ __launch_bounds__(kStThreads) void k_frame_th(const WinDev *__restrict__ wins, const float *__restrict__ buf,
                                                         int n_ranks, int n_win, long long stride, long long slot,
                                                         float *frame_th, NidSrc nid, double *win_nid,
                                                         const int *stop, int pass) {
    __shared__ unsigned keys[kThMaxLds + th_fixed_bytes(kStThreads) / sizeof(unsigned)];
    if ((int)blockIdx.x >= n_win) {
        const int w = blockIdx.x - n_win;
        if (stop && pass > stop[w]) return;
        nid_chain(wins[w], nid, win_nid, w, reinterpret_cast<float *>(keys), kThMaxLds);
        return;
    }
    const int w = blockIdx.x;
    const WinDev &W = wins[w];
    const long long n_cand = (long long)n_ranks * stride;
    select_frame_th<kStThreads>(
        [&](int i) {
            const int r = (int)(i / stride);
            return buf[((size_t)r * n_win + w) * slot + (i - (long long)r * stride)];
        },
        (int)n_cand, keys, kThMaxLds, frame_th + W.frame_base + W.N - 1);
}

}  // namespace
