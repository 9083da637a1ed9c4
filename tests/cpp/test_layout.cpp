// test_layout.cpp -- the window layout of ldso_ba_load (ldso_amd/csrc/layout.cpp) on the CPU: the
// shard partition, the residual bucket sort, the k_linearize / k_point_sc work items and the base
// offsets, over synthetic windows and a few built by hand.  Links layout.o, error.o and
// libldso_synth.so; no HIP.
#include <algorithm>
#include <cstdio>
#include <cstring>
#include <set>
#include <string>
#include <vector>

#include "../../ldso_amd/csrc/layout.h"
#include "../../ldso_amd/csrc/synth.h"

using namespace ldso_ba;

namespace {

int g_fail = 0;
long long g_checks = 0;
std::string g_case;
#define CHECK(cond)                                                                         \
    do {                                                                                    \
        g_checks++;                                                                         \
        if (!(cond)) {                                                                      \
            if (g_fail++ < 40) std::printf("FAIL %s:%d [%s] %s\n", __FILE__, __LINE__, g_case.c_str(), #cond); \
        }                                                                                   \
    } while (0)

// a caller's window with its storage
struct Win {
    int N = 0, P = 0, w = 64, h = 48;
    std::vector<float> dI, calib, th, precalc, c_delta, point_data, res_energy;
    std::vector<double> adH, adT, c_prior, frame_prior, frame_delta_prior;
    std::vector<int32_t> point_host, res_begin, res_target, point_rank;  // point_rank: empty = none
    std::vector<int8_t> res_state;
    std::vector<uint8_t> res_flags;
    ldso_ba_window view() const {
        ldso_ba_window v;
        std::memset(&v, 0, sizeof(v));
        v.n_frames = N;
        v.n_points = P;
        v.n_residuals = (int)res_target.size();
        v.width = w;
        v.height = h;
        for (int i = 0; i < 4; i++) v.calib[i] = calib[i];
        v.dI = dI.data();
        v.frame_energy_th = th.data();
        v.precalc = precalc.data();
        v.ad_host = adH.data();
        v.ad_target = adT.data();
        v.c_prior = c_prior.data();
        v.c_delta = c_delta.data();
        v.frame_prior = frame_prior.data();
        v.frame_delta_prior = frame_delta_prior.data();
        v.point_host = point_host.data();
        v.point_data = point_data.data();
        v.point_res_begin = res_begin.data();
        v.res_target = res_target.data();
        v.res_state = res_state.data();
        v.res_energy = res_energy.data();
        v.res_flags = res_flags.data();
        v.point_rank = point_rank.empty() ? nullptr : point_rank.data();
        return v;
    }
};

// a synthetic window; every `drop`-th residual removed (0: none), so points differ in residual count
Win make_win(int N, int P, uint64_t seed, int drop) {
    Win W;
    W.N = N;
    W.P = P;
    ldso_synth_params prm;
    std::memset(&prm, 0, sizeof(prm));
    prm.n_frames = N;
    prm.n_points = P;
    prm.width = W.w;
    prm.height = W.h;
    prm.seed = seed;
    prm.outlier_frac = 0.1f;
    prm.idepth_noise = 0.02f;
    prm.baseline = 0.1f;
    const int R = P * (N - 1);
    std::vector<ldso_ba_frame_state> frames(N);
    W.dI.resize((size_t)N * W.w * W.h * 3);
    W.calib.resize(4);
    W.th.resize(N);
    W.point_host.resize(P);
    W.point_data.resize((size_t)P * LDSO_BA_POINT_STRIDE);
    W.res_begin.resize(P + 1);
    W.res_target.resize(R);
    W.res_state.resize(R);
    W.res_energy.resize(R);
    W.res_flags.resize(R);
    const int rc = ldso_synth_fill(&prm, frames.data(), W.dI.data(), W.calib.data(), W.th.data(), W.point_host.data(),
                                   W.point_data.data(), W.res_begin.data(), W.res_target.data(), W.res_state.data(),
                                   W.res_energy.data(), W.res_flags.data());
    if (rc) {
        std::printf("ldso_synth_fill failed\n");
        g_fail++;
    }
    // frame-level inputs: the layout copies them through; the precalc only orders item order 2, so
    // a small per-pair warp (near identity, shifted) is enough to make the ranks differ
    W.precalc.assign((size_t)N * N * LDSO_BA_PRECALC_STRIDE, 0.f);
    for (int b = 0; b < N * N; b++) {
        float *pre = &W.precalc[(size_t)b * LDSO_BA_PRECALC_STRIDE];
        pre[0] = pre[4] = pre[8] = 1.f;
        pre[1] = 0.01f * (b % 5);
        pre[3] = -0.02f * (b % 3);
        pre[9] = 3.f * (b % 7);
        pre[10] = -2.f * (b % 4);
        pre[11] = 0.05f;
    }
    W.adH.resize((size_t)N * N * 64);
    W.adT.resize((size_t)N * N * 64);
    for (size_t i = 0; i < W.adH.size(); i++) {
        W.adH[i] = 0.001 * (double)(i % 97);
        W.adT[i] = -0.002 * (double)(i % 89);
    }
    W.c_prior.assign(4, 5e9);
    W.c_delta.assign(4, 0.f);
    W.frame_prior.assign((size_t)8 * N, 1.0);
    W.frame_delta_prior.assign((size_t)8 * N, 0.0);
    if (drop > 0) {
        std::vector<int32_t> rb(1, 0), rt;
        for (int p = 0; p < P; p++) {
            for (int k = W.res_begin[p]; k < W.res_begin[p + 1]; k++)
                if ((k * 7 + p) % drop != 0) rt.push_back(W.res_target[k]);
            rb.push_back((int32_t)rt.size());
        }
        W.res_begin = rb;
        W.res_target = rt;
        W.res_state.resize(rt.size());
        W.res_energy.resize(rt.size());
        W.res_flags.resize(rt.size());
    }
    // distinct per-residual values, so a permuted array is recognisable
    for (size_t k = 0; k < W.res_target.size(); k++) {
        W.res_energy[k] = (float)k;
        W.res_flags[k] = (uint8_t)(k % 3);
        W.res_state[k] = (int8_t)(k % 2);
    }
    return W;
}
void keep_points(Win &W, const std::vector<char> &keep) {
    Win O = W;
    W.point_host.clear();
    W.point_data.clear();
    W.res_begin.assign(1, 0);
    W.res_target.clear();
    W.res_state.clear();
    W.res_energy.clear();
    W.res_flags.clear();
    for (int p = 0; p < O.P; p++) {
        if (!keep[p]) continue;
        W.point_host.push_back(O.point_host[p]);
        W.point_data.insert(W.point_data.end(), O.point_data.begin() + (size_t)p * LDSO_BA_POINT_STRIDE,
                            O.point_data.begin() + (size_t)(p + 1) * LDSO_BA_POINT_STRIDE);
        for (int k = O.res_begin[p]; k < O.res_begin[p + 1]; k++) {
            W.res_target.push_back(O.res_target[k]);
            W.res_state.push_back(O.res_state[k]);
            W.res_energy.push_back(O.res_energy[k]);
            W.res_flags.push_back(O.res_flags[k]);
        }
        W.res_begin.push_back((int32_t)W.res_target.size());
    }
    W.P = (int)W.point_host.size();
}
void drop_residuals(Win &W) {
    W.res_begin.assign(W.P + 1, 0);
    W.res_target.clear();
    W.res_state.clear();
    W.res_energy.clear();
    W.res_flags.clear();
}

// the caller's points in device order, restated: host frames in window order, each host's points
// by point_rank (ties and no ranks: the caller's order)
std::vector<int> host_order(const ldso_ba_window &in) {
    std::vector<int> o(in.n_points);
    for (int p = 0; p < in.n_points; p++) o[p] = p;
    std::stable_sort(o.begin(), o.end(), [&](int a, int b) {
        if (in.point_host[a] != in.point_host[b]) return in.point_host[a] < in.point_host[b];
        return in.point_rank && in.point_rank[a] < in.point_rank[b];
    });
    return o;
}
// SURVEY.md 8e's partition, restated: the owner of a point is the rank whose share [r T / G, (r + 1) T / G)
// of the T residuals holds the point's first residual in device order; without residuals, the rank
// whose share [r P / G, (r + 1) P / G) of the P positions of the device order holds the point's
std::vector<int> ref_shard(const ldso_ba_window &in, int rank, int count) {
    std::vector<int> mine;
    long long first = 0, pos = 0;
    for (int p : host_order(in)) {
        const long long T = in.n_residuals;
        long long owner = T > 0 ? first * count / T : pos * count / in.n_points;
        if (owner > count - 1) owner = count - 1;
        if (owner == rank) mine.push_back(p);
        first += in.point_res_begin[p + 1] - in.point_res_begin[p];
        pos++;
    }
    return mine;
}

// the sizes ldso_ba_load gives its per-window regions, restated
long long ref_sys_len(int D) { return 2 * ((long long)D * (D + 1) / 2 + D); }
long long ref_stage_len(int N) {
    return std::max<long long>((long long)N * N * (520 + 64 * (N - 1)), (long long)N * ref_sys_len(8 * N + 4));
}

using ItemSet = std::multiset<std::vector<int>>;
ItemSet item_set(const Layout &L) {
    ItemSet s;
    for (const Item4 &it : L.top_items) s.insert({it.x, it.y, it.z, it.w});
    return s;
}

// every property of one shard's layout that needs no other shard
void check_shard(const std::vector<ldso_ba_window> &ws, const Layout &L, int rank, int count, int order, int chunk) {
    const int n_win = (int)ws.size();
    CHECK((int)L.wd.size() == n_win && (int)L.wh.size() == n_win);
    CHECK(L.chunk == chunk);
    int frame_base = 0, pair_base = 0, point_base = 0, res_base = 0, rec_base = 0, vec_base = 0;
    long long sys_base = 0, stage_base = 0, slab_base = 0;
    size_t top_i = 0, sc_i = 0, sum_i = 0;
    int max_frames = 0;
    size_t smem = 0;
    for (int w = 0; w < n_win; w++) {
        const ldso_ba_window &in = ws[w];
        const WinDesc &D = L.wd[w];
        const WinHost &H = L.wh[w];
        const int N = in.n_frames, P = D.P, R = D.R;
        max_frames = std::max(max_frames, N);
        CHECK(D.N == N && H.N == N && H.P == P && H.R == R && H.P_all == in.n_points && H.R_all == in.n_residuals);
        CHECK(D.D == 8 * N + 4 && D.p_all == in.n_points && D.width == in.width && D.height == in.height);
        CHECK(D.K == 8 * (N - 1) + 5 && D.KP % 4 == 0 && D.KP >= D.K && D.KP < D.K + 4);
        CHECK(D.ntiles == (D.KP / 4) * (D.KP / 4 + 1) / 2);
        smem = std::max(smem, sc_smem_bytes(D.KP));
        // the running sums of the sizes ldso_ba_load uses
        CHECK(D.frame_base == frame_base && D.pair_base == pair_base && D.point_base == point_base && D.res_base == res_base);
        CHECK(D.rec_base == rec_base && D.vec_base == vec_base);
        CHECK(D.sys_base == sys_base && D.stage_base == stage_base && D.sc_slab_base == slab_base);
        CHECK(D.top_item_base == (int)top_i && D.sc_item_base == (int)sc_i);
        // pt_orig: this rank's points (the restated partition; shard_points gives the same);
        // rs_orig: a permutation of their residuals
        std::vector<int> mine;
        shard_points(in, rank, count, mine);
        CHECK(ref_shard(in, rank, count) == H.pt_orig && mine == H.pt_orig && (int)H.pt_orig.size() == P);
        std::vector<int> want_res;
        for (int p : H.pt_orig)
            for (int k = in.point_res_begin[p]; k < in.point_res_begin[p + 1]; k++) want_res.push_back(k);
        std::vector<int> got_res = H.rs_orig;
        std::sort(want_res.begin(), want_res.end());
        std::sort(got_res.begin(), got_res.end());
        CHECK(got_res == want_res && (int)H.rs_orig.size() == R);
        // points: host order, the per-point arrays
        for (int q = 0; q < P; q++) {
            const int p = H.pt_orig[q];
            CHECK(q == 0 || H.pt_host[q - 1] <= H.pt_host[q]);
            if (in.point_rank && q > 0 && H.pt_host[q - 1] == H.pt_host[q])  // a host's points by rank
                CHECK(in.point_rank[H.pt_orig[q - 1]] <= in.point_rank[p]);
            CHECK(H.pt_host[q] == in.point_host[p] && L.pt_host[point_base + q] == in.point_host[p]);
            CHECK(L.pt_win[point_base + q] == w);
            CHECK(L.pt_nres[point_base + q] == in.point_res_begin[p + 1] - in.point_res_begin[p]);
            CHECK(std::memcmp(&L.pt_data[(size_t)(point_base + q) * LDSO_BA_POINT_STRIDE],
                              in.point_data + (size_t)p * LDSO_BA_POINT_STRIDE, LDSO_BA_POINT_STRIDE * sizeof(float)) == 0);
            for (int k = 0; k < L.pt_nres[point_base + q]; k++)
                CHECK((int)((L.pt_tgt[point_base + q] >> (4 * k)) & 15) == in.res_target[in.point_res_begin[p] + k]);
        }
        // residuals: buckets h + N t in order, the per-residual arrays, the record slots
        std::vector<int> point_of(in.n_residuals, -1), q_of(in.n_points, -1);
        for (int p = 0; p < in.n_points; p++)
            for (int k = in.point_res_begin[p]; k < in.point_res_begin[p + 1]; k++) point_of[k] = p;
        for (int q = 0; q < P; q++) q_of[H.pt_orig[q]] = q;
        std::vector<int> bucket_start(N * N + 1, 0);
        std::set<int> slots;
        int newest = 0, prev_bucket = -1;
        for (int pos = 0; pos < R; pos++) {
            const int k = H.rs_orig[pos], p = point_of[k], h = in.point_host[p], t = in.res_target[k], b = h + N * t;
            CHECK(b >= prev_bucket);
            prev_bucket = b;
            bucket_start[b + 1]++;
            if (t == N - 1) newest++;
            CHECK(L.rs_tgt[res_base + pos] == t && L.rs_flags[res_base + pos] == in.res_flags[k]);
            CHECK(L.rs_state[res_base + pos] == in.res_state[k] && L.rs_energy[res_base + pos] == in.res_energy[k]);
            const int slot = L.rs_slot[res_base + pos];
            CHECK(slot == H.rs_slot[pos]);
            CHECK(slot >= D.rec_base && slot < D.rec_base + P * (N - 1));
            CHECK(slot == D.rec_base + (t < h ? t : t - 1) * P + q_of[p]);
            slots.insert(slot);
        }
        CHECK((int)slots.size() == R);
        for (int b = 0; b < N * N; b++) bucket_start[b + 1] += bucket_start[b];
        // newest_begin / newest_end bound exactly the residuals into frame N-1 (the last N buckets)
        CHECK(D.newest_begin == res_base + bucket_start[N * (N - 1)] && D.newest_end == res_base + R);
        CHECK(D.newest_end - D.newest_begin == newest);
        for (int pos = 0; pos < R; pos++)
            CHECK((L.rs_tgt[res_base + pos] == N - 1) == (res_base + pos >= D.newest_begin && res_base + pos < D.newest_end));
        // top items: pair_items[b] spans the bucket's items, which tile [bucket_start, bucket_end)
        int n_top = 0;
        for (int b = 0; b < N * N; b++) {
            const Item2 pi = L.pair_items[pair_base + b];
            CHECK(L.pair_win[pair_base + b] == w);
            const int cnt = bucket_start[b + 1] - bucket_start[b];
            CHECK((pi.y == 0) == (cnt == 0));
            CHECK(pi.y == (cnt + chunk - 1) / chunk);
            CHECK(pi.x >= D.top_item_base && pi.x + pi.y <= D.top_item_base + D.n_top_items);
            n_top += pi.y;
            int at = res_base + bucket_start[b], not_mult8 = 0;
            for (int i = 0; i < pi.y; i++) {
                const Item4 it = L.top_items[pi.x + i];
                const int len = it.y & 0xFFFF;
                CHECK(it.x == at);  // no gap, no overlap
                CHECK(len >= 1 && len <= chunk);
                CHECK(((it.y >> 16) & 1) == (i == 0 ? 1 : 0) && (it.y >> 17) == 0);
                CHECK(it.z == pair_base + b && it.w == w);
                if (len % 8) not_mult8++;
                at += len;
            }
            CHECK(at == res_base + bucket_start[b + 1]);  // the lengths sum to the bucket's count
            if (order == 2) CHECK(not_mult8 <= 1);
        }
        CHECK(n_top == D.n_top_items);
        // item order: target-major (0, 2) walks the buckets in index order, host-major (1) by host
        for (int i = 1; i < D.n_top_items; i++) {
            const int b0 = L.top_items[D.top_item_base + i - 1].z - pair_base, b1 = L.top_items[D.top_item_base + i].z - pair_base;
            if (order == 1) CHECK((b0 % N) * N + b0 / N <= (b1 % N) * N + b1 / N);
            else CHECK(b0 <= b1);
        }
        // sc items: host f's items tile its points in runs of at most sc_chunk
        int n_sc = 0, at_pt = point_base;
        for (int f = 0; f < N; f++) {
            const Item2 hi = L.host_items[frame_base + f];
            CHECK(L.frame_win[frame_base + f] == w);
            CHECK(hi.x == (int)sc_i + n_sc);
            int host_pts = 0;
            for (int q = 0; q < P; q++) host_pts += H.pt_host[q] == f;
            int covered = 0;
            for (int i = 0; i < hi.y; i++) {
                const Item4 it = L.sc_items[hi.x + i];
                CHECK(it.x == at_pt && it.y >= 1 && it.y <= L.sc_chunk && it.z == f && it.w == w);
                CHECK(i + 1 == hi.y || it.y == L.sc_chunk);
                for (int j = 0; j < it.y; j++) CHECK(H.pt_host[it.x - point_base + j] == f);
                at_pt += it.y;
                covered += it.y;
            }
            CHECK(covered == host_pts);
            n_sc += hi.y;
        }
        CHECK(n_sc == D.n_sc_items && at_pt == point_base + P);
        // k_stitch_sum blocks: the window's packed elements in steps of 256
        for (long long e0 = 0; e0 < ref_sys_len(D.D); e0 += 256, sum_i++)
            CHECK(sum_i < L.sum_blocks.size() && L.sum_blocks[sum_i].x == w && L.sum_blocks[sum_i].y == (int)e0);
        // frame-level inputs copied through
        CHECK(std::memcmp(&L.precalc[(size_t)pair_base * LDSO_BA_PRECALC_STRIDE], in.precalc,
                          (size_t)N * N * LDSO_BA_PRECALC_STRIDE * sizeof(float)) == 0);
        CHECK(std::memcmp(&L.adH[(size_t)pair_base * 64], in.ad_host, (size_t)N * N * 64 * sizeof(double)) == 0);
        CHECK(std::memcmp(&L.adT[(size_t)pair_base * 64], in.ad_target, (size_t)N * N * 64 * sizeof(double)) == 0);
        CHECK(std::memcmp(&L.frame_th[frame_base], in.frame_energy_th, N * sizeof(float)) == 0);
        frame_base += N;
        pair_base += N * N;
        point_base += P;
        res_base += R;
        rec_base += P * (N - 1);
        vec_base += 8 * N + 4;
        sys_base += ref_sys_len(8 * N + 4);
        stage_base += ref_stage_len(N);
        slab_base += (long long)D.n_sc_items * D.ntiles * 16;
        top_i += D.n_top_items;
        sc_i += D.n_sc_items;
    }
    CHECK(L.top_items.size() == top_i && L.sc_items.size() == sc_i && L.sum_blocks.size() == sum_i);
    CHECK((int)L.pair_items.size() == pair_base && (int)L.pair_win.size() == pair_base);
    CHECK((int)L.host_items.size() == frame_base && (int)L.frame_win.size() == frame_base);  // one entry per frame
    CHECK((int)L.pt_host.size() == point_base && (int)L.pt_win.size() == point_base && (int)L.pt_nres.size() == point_base);
    CHECK((int)L.rs_tgt.size() == res_base && (int)L.rs_slot.size() == res_base);
    CHECK(L.rec_base == rec_base && L.vec_total == vec_base && L.sys_total == sys_base && L.stage_total == stage_base);
    CHECK(L.sc_slab_total == slab_base && L.max_frames == max_frames && L.smem_max == smem);
}

void check_case(const std::string &name, const std::vector<Win> &wins) {
    std::vector<ldso_ba_window> ws;
    for (const Win &W : wins) ws.push_back(W.view());
    for (int count : {1, 2, 3, 5})
        for (int chunk : {16, 32, 64}) {
            std::vector<ItemSet> order0(count);
            for (int order : {0, 1, 2}) {
                std::vector<Layout> Ls(count);
                for (int rank = 0; rank < count; rank++) {
                    g_case = name + " shards " + std::to_string(rank) + "/" + std::to_string(count) + " order " +
                             std::to_string(order) + " chunk " + std::to_string(chunk);
                    const int rc = build_layout(ws.data(), (int)ws.size(), rank, count, order, chunk, false, Ls[rank]);
                    CHECK(rc == 0);
                    if (rc) continue;
                    check_shard(ws, Ls[rank], rank, count, order, chunk);
                    if (order == 0) order0[rank] = item_set(Ls[rank]);
                    if (order == 1) CHECK(item_set(Ls[rank]) == order0[rank]);  // the same items, another order
                }
                // over the ranks: pt_orig partition the caller's points; for T > 0 each rank's run is
                // contiguous in host-frame order and the runs in rank order are that order
                for (size_t w = 0; w < ws.size(); w++) {
                    std::vector<int> cat, all;
                    for (int rank = 0; rank < count; rank++)
                        cat.insert(cat.end(), Ls[rank].wh[w].pt_orig.begin(), Ls[rank].wh[w].pt_orig.end());
                    all = cat;
                    std::sort(all.begin(), all.end());
                    bool partition = (int)all.size() == ws[w].n_points;
                    for (size_t i = 0; i < all.size(); i++) partition = partition && all[i] == (int)i;
                    CHECK(partition);
                    if (ws[w].n_residuals > 0) CHECK(cat == host_order(ws[w]));
                }
            }
        }
}

void check_marg_and_auto_chunk() {
    g_case = "marginalisation flag, automatic chunk";
    Win W = make_win(5, 120, 11, 0);
    for (int p = 0; p < W.P; p++) W.point_data[(size_t)p * LDSO_BA_POINT_STRIDE + 4] = 1.f + p;
    W.dI.clear();  // a marginalisation context borrows its images
    ldso_ba_window v = W.view();
    v.dI = nullptr;
    Layout L;
    CHECK(build_layout(&v, 1, 0, 1, 0, 0, true, L) == 0);
    CHECK(L.chunk == 16 && L.sc_chunk == 16);  // a small load
    for (int q = 0; q < L.wd[0].P; q++)
        CHECK(L.pt_data[(size_t)q * LDSO_BA_POINT_STRIDE + 4] == (1.f + L.wh[0].pt_orig[q]) * kIdepthFixPriorMargFac);
    CHECK(build_layout(&v, 1, 0, 1, 0, 0, false, L) == -1);  // a load needs the images
    CHECK(std::string(last_error()) == "null frame-level pointer");
}

void expect_reject(const Win &W, const char *msg) {
    const ldso_ba_window v = W.view();
    CHECK(check_window(v) == -1);
    CHECK(std::string(last_error()) == msg);
    Layout L;
    CHECK(build_layout(&v, 1, 0, 1, 0, 0, false, L) == -1);
    CHECK(std::string(last_error()) == msg);
}
void check_rejections() {
    const Win base = make_win(4, 40, 5, 0);
    g_case = "accepted";
    {
        const ldso_ba_window v = base.view();
        CHECK(check_window(v) == 0);
    }
    g_case = "duplicate target";
    {
        Win W = base;
        const int k = W.res_begin[3];
        W.res_target[k + 1] = W.res_target[k];
        expect_reject(W, "duplicate (point, target) residual");
    }
    g_case = "target equals host";
    {
        Win W = base;
        W.res_target[W.res_begin[7]] = W.point_host[7];
        expect_reject(W, "res_target out of range or equal to host");
    }
    g_case = "point_res_begin not spanning";
    {
        Win W = base;
        W.res_begin[W.P] -= 1;
        expect_reject(W, "point_res_begin must span [0, n_residuals]");
        W = base;
        W.res_begin[0] = 1;
        expect_reject(W, "point_res_begin must span [0, n_residuals]");
    }
    g_case = "image sizes differ";
    {
        Win A = base, B = make_win(3, 40, 6, 0);
        B.w = 48;  // the view only: the layout never reads the pixels
        const ldso_ba_window v[2] = {A.view(), B.view()};
        Layout L;
        CHECK(build_layout(v, 2, 0, 1, 0, 0, false, L) == -1);
        CHECK(std::string(last_error()) == "all windows of a context must share the image size");
    }
}

// image_layout against values worked out by hand from its rules: padded_h = (h+3)/4*4; mode 3:
// tpr = (w+7)/8, stride = tpr*8*padded_h/4; mode 1: tpr = (w+1)/2, stride = tpr*2*padded_h
void check_image_layout() {
    g_case = "image_layout";
    static const struct {
        int w, h, mode, tpr, hp;
        long long stride, repack;
    } kCases[] = {
        {13, 7, 3, 2, 8, 32, 128},
        {13, 7, 1, 7, 8, 112, 112},
        {162, 118, 3, 21, 120, 5040, 20160},
        {162, 118, 1, 81, 120, 19440, 19440},
        {640, 480, 3, 80, 480, 76800, 307200},
        {640, 480, 1, 320, 480, 307200, 307200},
    };
    for (const auto &k : kCases) {
        const ImageLayout l = image_layout(k.mode, k.w, k.h);
        CHECK(l.mode == k.mode && l.width == k.w && l.height == k.h);
        CHECK(l.tiles_per_row == k.tpr);
        CHECK(l.padded_h == k.hp);
        CHECK(l.frame_stride == k.stride);
        CHECK(l.npix() == (size_t)k.w * k.h);
        CHECK(l.slot_bytes() == (size_t)k.stride * 16);
        CHECK(l.repack_elems() == k.repack);  // mode 3: one per padded intensity, 4 to a float4
    }
}

}  // namespace

int main() {
    const int frames[6] = {2, 3, 7, 12, 13, 16}, points[6] = {40, 77, 300, 150, 101, 64};
    for (int i = 0; i < 6; i++)
        check_case("synth N=" + std::to_string(frames[i]), {make_win(frames[i], points[i], 100 + i, i % 2 ? 5 : 0)});
    {
        Win W = make_win(5, 60, 21, 0);
        keep_points(W, std::vector<char>(W.P, 0));
        check_case("no points", {W});
    }
    {
        Win W = make_win(5, 60, 22, 0);
        drop_residuals(W);
        check_case("points but no residuals", {W});
    }
    {
        Win W = make_win(6, 90, 23, 4);
        std::vector<char> keep(W.P, 1);
        for (int p = 0; p < W.P; p++) keep[p] = W.point_host[p] != 2;
        keep_points(W, keep);
        check_case("a host frame without points", {W});
    }
    {
        Win W = make_win(7, 130, 24, 5);  // features order differs from the caller's, with ties
        W.point_rank.resize(W.P);
        for (int p = 0; p < W.P; p++) W.point_rank[p] = (p * 37 + 11) % 50;
        check_case("point_rank", {W});
    }
    check_case("three windows", {make_win(7, 120, 31, 3), make_win(3, 50, 32, 0), make_win(13, 45, 33, 6)});
    check_marg_and_auto_chunk();
    check_rejections();
    check_image_layout();
    std::printf("%lld checks, %d failure(s)\n", g_checks, g_fail);
    return g_fail ? 1 : 0;
}
