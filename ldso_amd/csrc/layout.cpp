// layout.cpp -- see layout.h.  No HIP in here.
#include "layout.h"

#include <algorithm>
#include <cmath>
#include <utility>

namespace ldso_ba {

int check_window(const ldso_ba_window &w, bool need_images) {
    constexpr int kMaxRes = LDSO_BA_MAX_FRAMES - 1;
    if (w.n_frames < 2 || w.n_frames > LDSO_BA_MAX_FRAMES) return set_error(-1, "n_frames out of range [2,16]");
    if (w.n_points < 0 || w.n_residuals < 0) return set_error(-1, "negative counts");
    if ((need_images && !w.dI) || !w.frame_energy_th || !w.precalc || !w.ad_host || !w.ad_target || !w.c_prior || !w.c_delta ||
        !w.frame_prior || !w.frame_delta_prior)
        return set_error(-1, "null frame-level pointer");
    if (w.n_points > 0 && (!w.point_host || !w.point_data || !w.point_res_begin))
        return set_error(-1, "null point pointer");
    if (w.n_residuals > 0 && (!w.res_target || !w.res_state || !w.res_energy || !w.res_flags))
        return set_error(-1, "null residual pointer");
    if (w.width < 8 || w.height < 8) return set_error(-1, "image too small");
    if (w.point_res_begin && (w.point_res_begin[0] != 0 || w.point_res_begin[w.n_points] != w.n_residuals))
        return set_error(-1, "point_res_begin must span [0, n_residuals]");
    for (int p = 0; p < w.n_points; p++) {
        const int h = w.point_host[p];
        if (h < 0 || h >= w.n_frames) return set_error(-1, "point_host out of range");
        const int b = w.point_res_begin[p], e = w.point_res_begin[p + 1];
        if (e < b || e - b > kMaxRes) return set_error(-1, "a point has more than N-1 residuals");
        unsigned seen = 0;
        for (int k = b; k < e; k++) {
            const int t = w.res_target[k];
            if (t < 0 || t >= w.n_frames || t == h) return set_error(-1, "res_target out of range or equal to host");
            if (seen & (1u << t)) return set_error(-1, "duplicate (point, target) residual");
            seen |= 1u << t;
        }
    }
    return 0;
}

ImageLayout image_layout(int mode, int width, int height) {
    ImageLayout l;
    l.mode = mode;
    l.width = width;
    l.height = height;
    l.padded_h = (height + 3) / 4 * 4;
    if (mode == 3) {
        l.tiles_per_row = (width + 7) / 8;
        l.frame_stride = (long long)l.tiles_per_row * 8 * l.padded_h / 4;
    } else {
        l.tiles_per_row = (width + 1) / 2;
        l.frame_stride = (long long)l.tiles_per_row * 2 * l.padded_h;
    }
    return l;
}

size_t sc_smem_bytes(int KP) {
    return ((size_t)kScPoints * (KP + 4) + (size_t)LDSO_BA_MAX_FRAMES * kPrePitch) * sizeof(float);
}

// SURVEY.md §8e's partition: points in host-frame order, cut into shard_count contiguous runs of
// (as nearly as possible) equal residual counts, so a shard holds whole host frames except at
// its two ends (a host is split only where a cut falls inside it, e.g. when shards outnumber
// hosts).  Rank r owns the points whose first residual lies in [r T / G, (r + 1) T / G).  A window
// without residuals (T = 0) is cut by point count instead: the point at position i of the order
// goes to rank i G / P, so its runs are contiguous pieces of the host-frame order too.
void shard_points(const ldso_ba_window &in, int rank, int count, std::vector<int> &out) {
    out.clear();
    // the device point order: host frames in window order, each host's points in features order
    // (point_rank; the caller's order without it)
    std::vector<int> order;
    order.reserve(in.n_points);
    for (int f = 0; f < in.n_frames; f++) {
        const size_t b = order.size();
        for (int p = 0; p < in.n_points; p++)
            if (in.point_host[p] == f) order.push_back(p);
        if (in.point_rank)
            std::stable_sort(order.begin() + b, order.end(),
                             [&](int a, int c) { return in.point_rank[a] < in.point_rank[c]; });
    }
    const long long T = in.n_residuals;
    long long acc = 0, pos = 0;
    for (int p : order) {
        const long long owner = T > 0 ? std::min<long long>(count - 1, acc * count / T) : pos * count / in.n_points;
        if (owner == rank) out.push_back(p);
        acc += in.point_res_begin[p + 1] - in.point_res_begin[p];
        pos++;
    }
}

bool adjoints_diagonal(const double *ad, size_t n_blocks) {
    for (size_t b = 0; b < n_blocks; b++)
        for (int e = 0; e < 64; e++)
            if (e % 9 != 0 && ad[b * 64 + e] != 0.0) return false;  // a NaN is not zero either
    return true;
}

int build_layout(const ldso_ba_window *ws, int n_windows, int shard_rank, int shard_count, int item_order,
                 int top_chunk, bool marg, Layout &out, bool resident_frames) {
    for (int w = 0; w < n_windows; w++) {
        int rc = check_window(ws[w], !marg && !resident_frames);
        if (rc) return rc;
        if (ws[w].width != ws[0].width || ws[w].height != ws[0].height)
            return set_error(-1, "all windows of a context must share the image size");
    }
    out = Layout();
    Layout &L = out;
    L.wh.assign(n_windows, WinHost());
    L.wd.assign(n_windows, WinDesc());
    // residuals per k_linearize wave: 64 when the grid is large anyway; small workloads (one
    // window) use shorter chunks so more waves start at once (latency, not throughput, bound)
    long long r_est = 0;
    for (int w = 0; w < n_windows; w++) r_est += ws[w].n_residuals;
    r_est /= shard_count;
    const int chunk = top_chunk ? top_chunk : r_est >= 64LL * 4096 ? 64 : r_est >= 32LL * 2048 ? 32 : 16;
    // k_point_sc points per block: 64 for large loads; a small load (one window: 32 blocks of 64
    // points on 256 CUs) takes 16-point blocks, whose SYRK chains are a quarter as long (one S7
    // window's pass 30 -> 28 us; optimize unchanged: its sumNID block is the longest there)
    const int sc_chunk = r_est < 64LL * 4096 ? 16 : kScPoints;
    L.chunk = chunk;
    L.sc_chunk = sc_chunk;
    int frame_base = 0, pair_base = 0, point_base = 0, res_base = 0;

    for (int w = 0; w < n_windows; w++) {
        const ldso_ba_window &in = ws[w];
        WinHost &H = L.wh[w];
        WinDesc &D = L.wd[w];
        const int N = in.n_frames;
        L.max_frames = std::max(L.max_frames, N);
        H.N = N;
        H.P_all = in.n_points;
        H.R_all = in.n_residuals;
        // the priors (HL, bL) are not part of the reduced packed system: every rank adds them in
        // its own (redundant) solve, so every shard keeps them
        H.add_priors = true;
        H.c_prior.assign(in.c_prior, in.c_prior + 4);
        H.c_delta.assign(in.c_delta, in.c_delta + 4);
        H.frame_prior.assign(in.frame_prior, in.frame_prior + 8 * N);
        H.frame_delta_prior.assign(in.frame_delta_prior, in.frame_delta_prior + 8 * N);
        H.adHF.resize((size_t)N * N * 64);
        H.adTF.resize((size_t)N * N * 64);
        for (size_t k = 0; k < H.adHF.size(); k++) {
            H.adHF[k] = (float)in.ad_host[k];
            H.adTF[k] = (float)in.ad_target[k];
        }
        // points of this shard (host-frame partition, shard_points)
        shard_points(in, shard_rank, shard_count, H.pt_orig);
        const int P = (int)H.pt_orig.size();
        H.P = P;
        // residual bucket sort by pair index h + N t (stable in point order)
        std::vector<int> bucket_cnt(N * N, 0);
        int R = 0;
        for (int q = 0; q < P; q++) {
            const int p = H.pt_orig[q], h = in.point_host[p];
            for (int k = in.point_res_begin[p]; k < in.point_res_begin[p + 1]; k++) {
                bucket_cnt[h + N * in.res_target[k]]++;
                R++;
            }
        }
        H.R = R;
        std::vector<int> bucket_start(N * N + 1, 0);
        for (int b = 0; b < N * N; b++) bucket_start[b + 1] = bucket_start[b] + bucket_cnt[b];
        std::vector<int> fill(bucket_start.begin(), bucket_start.end() - 1);
        H.rs_orig.assign(R, -1);
        std::vector<int> res_pos_of(in.n_residuals, -1);
        for (int q = 0; q < P; q++) {
            const int p = H.pt_orig[q], h = in.point_host[p];
            for (int k = in.point_res_begin[p]; k < in.point_res_begin[p + 1]; k++) {
                const int pos = fill[h + N * in.res_target[k]]++;
                H.rs_orig[pos] = k;
                res_pos_of[k] = pos;
            }
        }
        // item order 2: inside each bucket the residuals are ranked by their projection into the
        // target (row, then column) and dealt round robin, in groups of 8 consecutive ranks (one
        // phase-A step of a wavefront), over the bucket's chunks: every chunk of a bucket sweeps the
        // target image top to bottom and the concurrent chunks of one target are at the same band
        // at the same step (the target's live lines: one band, not the frame).  Chunks stay
        // multiples of 8 but the last, so the phase-A steps are the same as in order 0.
        std::vector<int> bucket_nch(N * N, 0);
        std::vector<int> chunk_len;  // item order 2: residuals per chunk, bucket by bucket
        if (item_order == 2) {
            std::vector<std::pair<std::pair<float, float>, int>> key;
            for (int b = 0; b < N * N; b++) {
                const int n = bucket_cnt[b];
                if (n == 0) continue;
                const float *pre = in.precalc + (size_t)b * LDSO_BA_PRECALC_STRIDE;  // PRE_KRKiTll, PRE_KtTll
                key.clear();
                for (int pos = bucket_start[b]; pos < bucket_start[b + 1]; pos++) key.push_back({{0.f, 0.f}, H.rs_orig[pos]});
                for (auto &e : key) {
                    const int k = e.second;  // its point: point_res_begin is sorted
                    const int p = (int)(std::upper_bound(in.point_res_begin, in.point_res_begin + in.n_points + 1, k) -
                                        in.point_res_begin) - 1;
                    const float *d = in.point_data + (size_t)p * LDSO_BA_POINT_STRIDE;
                    float q[3];
                    for (int i = 0; i < 3; i++) q[i] = pre[3 * i] * d[0] + pre[3 * i + 1] * d[1] + pre[3 * i + 2] + pre[9 + i] * d[2];
                    const float y = q[1] / q[2], x = q[0] / q[2];
                    e.first = {std::isfinite(y) ? y : 0.f, std::isfinite(x) ? x : 0.f};
                }
                std::sort(key.begin(), key.end());
                const int G = (n + 7) / 8, nch = (n + chunk - 1) / chunk;
                bucket_nch[b] = nch;
                std::vector<int> start(nch + 1, 0);
                for (int cc = 0; cc < nch; cc++) {
                    const int groups = (G - cc + nch - 1) / nch;  // groups cc, cc + nch, ...
                    int len = 8 * groups;
                    if ((G - 1) % nch == cc) len -= 8 * G - n;  // the last (short) group ends this chunk
                    start[cc + 1] = start[cc] + len;
                    chunk_len.push_back(len);
                }
                for (int i = 0; i < n; i++) {
                    const int g = i / 8, cc = g % nch;
                    const int pos = bucket_start[b] + start[cc] + 8 * (g / nch) + (i & 7);
                    H.rs_orig[pos] = key[i].second;
                    res_pos_of[key[i].second] = pos;
                }
            }
        }
        // per-residual arrays (global, sorted)
        for (int pos = 0; pos < R; pos++) {
            const int k = H.rs_orig[pos];
            L.rs_tgt.push_back((uint8_t)in.res_target[k]);
            L.rs_flags.push_back(in.res_flags[k]);
            L.rs_state.push_back(in.res_state[k]);
            L.rs_energy.push_back(in.res_energy[k]);
            L.rs_slot.push_back(0);
        }
        H.rs_slot.assign(R, 0);
        // per-point arrays
        H.pt_host.resize(P);
        for (int q = 0; q < P; q++) {
            const int p = H.pt_orig[q];
            H.pt_host[q] = in.point_host[p];
            L.pt_host.push_back(in.point_host[p]);
            L.pt_data.insert(L.pt_data.end(), in.point_data + (size_t)p * LDSO_BA_POINT_STRIDE,
                             in.point_data + (size_t)(p + 1) * LDSO_BA_POINT_STRIDE);
            if (marg)  // marginalizePointsF: p->priorF *= setting_idepthFixPriorMargFac (EnergyFunctional.cc:216)
                L.pt_data[L.pt_data.size() - LDSO_BA_POINT_STRIDE + 4] *= kIdepthFixPriorMargFac;
            const int b = in.point_res_begin[p], e = in.point_res_begin[p + 1];
            L.pt_nres.push_back(e - b);
            unsigned long long tg = 0;
            for (int k = 0; k < e - b; k++) {
                const int pos = res_pos_of[b + k];
                const int tgk = in.res_target[b + k], hk = in.point_host[p];
                const int slot = L.rec_base + (tgk < hk ? tgk : tgk - 1) * P + q;
                L.rs_slot[res_base + pos] = slot;
                H.rs_slot[pos] = slot;
                tg |= (unsigned long long)in.res_target[b + k] << (4 * k);
            }
            L.pt_tgt.push_back(tg);
        }
        // descriptors
        D.N = N;
        D.P = P;
        D.R = R;
        D.D = 8 * N + 4;
        D.frame_base = frame_base;
        D.pair_base = pair_base;
        D.point_base = point_base;
        D.res_base = res_base;
        D.width = in.width;
        D.height = in.height;
        D.wM3 = (float)(in.width - 3);
        D.hM3 = (float)(in.height - 3);
        for (int i = 0; i < 4; i++) D.calib[i] = in.calib[i];
        for (int i = 0; i < 4; i++) D.cdelta[i] = in.c_delta[i];
        D.p_all = in.n_points;  // numID counts every shard's points
        D.adt_diag = adjoints_diagonal(in.ad_target, (size_t)N * N) ? 1 : 0;
        D.K = 8 * (N - 1) + 5;
        D.KP = (D.K + 3) / 4 * 4;
        const int nt = D.KP / 4;
        D.ntiles = nt * (nt + 1) / 2;
        L.smem_max = std::max(L.smem_max, sc_smem_bytes(D.KP));
        // top items: chunks of `chunk` residuals of one bucket (one wave each)
        D.top_item_base = (int)L.top_items.size();
        const size_t pi0 = L.pair_items.size();
        L.pair_items.resize(pi0 + (size_t)N * N);
        std::vector<int> chunk_off(N * N + 1, 0);  // item order 2: first chunk_len entry of each bucket
        for (int b = 0; b < N * N; b++) chunk_off[b + 1] = chunk_off[b] + bucket_nch[b];
        for (int bb = 0; bb < N * N; bb++) {
            // bucket b = h + N t; chunks in target-major order (the N-1 buckets reading one target
            // image run together) or host-major (the buckets of one host's points run together)
            const int b = item_order == 1 ? (bb / N) + N * (bb % N) : bb;
            const int first = (int)L.top_items.size();
            if (bucket_nch[b] > 0) {  // item order 2: the chunks dealt above
                int s0 = bucket_start[b];
                for (int cc = 0; cc < bucket_nch[b]; cc++) {
                    const int len = chunk_len[chunk_off[b] + cc];
                    L.top_items.push_back({res_base + s0, len | (cc == 0 ? 1 << 16 : 0), pair_base + b, w});
                    s0 += len;
                }
            } else {
                for (int s = bucket_start[b]; s < bucket_start[b + 1]; s += chunk)  // bit 16: the pair's first chunk
                    L.top_items.push_back({res_base + s, std::min(chunk, bucket_start[b + 1] - s) | (s == bucket_start[b] ? 1 << 16 : 0),
                                           pair_base + b, w});
            }
            L.pair_items[pi0 + b] = {first, (int)L.top_items.size() - first};
        }
        L.pair_win.insert(L.pair_win.end(), N * N, w);
        D.n_top_items = (int)L.top_items.size() - D.top_item_base;
        // sc items: chunks of sc_chunk points of one host
        D.sc_item_base = (int)L.sc_items.size();
        {
            int q = 0;
            for (int f = 0; f < N; f++) {
                const int first = (int)L.sc_items.size();
                int q0 = q;
                while (q < P && H.pt_host[q] == f) q++;
                for (int s = q0; s < q; s += sc_chunk)
                    L.sc_items.push_back({point_base + s, std::min(sc_chunk, q - s), f, w});
                L.host_items.push_back({first, (int)L.sc_items.size() - first});
                L.frame_win.push_back(w);
            }
        }
        D.n_sc_items = (int)L.sc_items.size() - D.sc_item_base;
        D.sc_slab_base = L.sc_slab_total;
        L.sc_slab_total += (long long)D.n_sc_items * D.ntiles * 16;
        D.sys_base = L.sys_total;
        L.sys_total += sys_len(D.D);
        D.stage_base = L.stage_total;
        // k_stitch's per-pair records, or k_stitch_host's per-host partial systems
        L.stage_total += std::max<long long>((long long)N * N * stage_rec(N), (long long)N * sys_len(D.D));
        D.newest_begin = res_base + bucket_start[N * (N - 1)];
        D.newest_end = res_base + bucket_start[N * N];
        D.rec_base = L.rec_base;
        D.vec_base = L.vec_total;
        L.vec_total += D.D;
        L.pt_win.insert(L.pt_win.end(), P, w);
        for (long long e0 = 0; e0 < sys_len(D.D); e0 += 256) L.sum_blocks.push_back({w, (int)e0});
        // frame-level inputs
        L.precalc.insert(L.precalc.end(), in.precalc, in.precalc + (size_t)N * N * LDSO_BA_PRECALC_STRIDE);
        L.adH.insert(L.adH.end(), in.ad_host, in.ad_host + (size_t)N * N * 64);
        L.adT.insert(L.adT.end(), in.ad_target, in.ad_target + (size_t)N * N * 64);
        L.frame_th.insert(L.frame_th.end(), in.frame_energy_th, in.frame_energy_th + N);
        frame_base += N;
        pair_base += N * N;
        point_base += P;
        L.rec_base += P * (N - 1);
        res_base += R;
    }
    return 0;
}

}  // namespace ldso_ba
