// test_marg_plan.cpp -- ldso_ba_load_marginalization_device's host planner (ldso_amd/csrc/marg_plan.cpp)
// as a stand-alone program: a hand-made parent window, selections of its points and residuals, the
// plan checked array for array against build_layout of the explicit marginalisation window
// (ldso_ba_marg_plan_check's n_mismatch, which also compares the values at the gather positions)
// and the gather indices against the two layouts' own orders, then the refusals.  Links layout.o,
// edit_plan.o, marg_plan.o and error.o only (no HIP, no images), so the same source builds under
// -fsanitize=address,undefined (make sanitize-marg-plan).
#include <cstdio>
#include <cstring>
#include <map>
#include <string>
#include <vector>

#include "../../ldso_amd/csrc/marg_plan.h"

using namespace ldso_ba;

namespace {

int g_fail = 0;
long long g_checks = 0;
std::string g_case;
#define CHECK(cond)                                                                                            \
    do {                                                                                                       \
        g_checks++;                                                                                            \
        if (!(cond) && g_fail++ < 40) std::printf("FAIL %s:%d [%s] %s\n", __FILE__, __LINE__, g_case.c_str(), #cond); \
    } while (0)

struct Lcg {
    uint64_t s;
    uint32_t next() {
        s = s * 6364136223846793005ull + 1442695040888963407ull;
        return (uint32_t)(s >> 33);
    }
};

struct Win {
    int N = 0;
    std::vector<int32_t> point_host, res_begin{0}, res_target, point_rank;
    std::vector<float> point_data, res_energy, th, precalc, c_delta;
    std::vector<double> adH, adT, c_prior, fp, fdp;
    std::vector<int8_t> res_state;
    std::vector<uint8_t> res_flags;
    ldso_ba_window view() const {
        ldso_ba_window v;
        std::memset(&v, 0, sizeof(v));
        v.n_frames = N;
        v.n_points = (int)point_host.size();
        v.n_residuals = (int)res_target.size();
        v.width = 64;
        v.height = 48;
        for (int i = 0; i < 4; i++) v.calib[i] = 10.f + i;
        v.frame_energy_th = th.data();
        v.precalc = precalc.data();
        v.ad_host = adH.data();
        v.ad_target = adT.data();
        v.c_prior = c_prior.data();
        v.c_delta = c_delta.data();
        v.frame_prior = fp.data();
        v.frame_delta_prior = fdp.data();
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
Win make_parent(int N, int P, uint64_t seed, bool ranked) {
    Win W;
    W.N = N;
    Lcg g{seed};
    int id = 0;
    for (int p = 0; p < P; p++) {
        const int h = (int)(g.next() % N);
        W.point_host.push_back(h);
        if (ranked) W.point_rank.push_back((int)((p * 7919u) % 1009u));
        for (int k = 0; k < LDSO_BA_POINT_STRIDE; k++) W.point_data.push_back((float)p + 0.01f * k);
        for (int k = 0; k < N; k++) {
            const int f = (k + p) % N;  // shuffled target order
            if (f != h && g.next() % 10 < 6) {
                W.res_target.push_back(f);
                W.res_state.push_back((int8_t)(id % 3));
                W.res_energy.push_back((float)id);
                W.res_flags.push_back((uint8_t)(id & 3));
                id++;
            }
        }
        W.res_begin.push_back((int32_t)W.res_target.size());
    }
    W.th.assign(N, 1.f);
    W.precalc.resize((size_t)N * N * LDSO_BA_PRECALC_STRIDE);
    for (size_t i = 0; i < W.precalc.size(); i++) W.precalc[i] = (float)i;
    W.c_delta = {0.1f, 0.2f, 0.3f, 0.4f};
    W.adH.assign((size_t)N * N * 64, 0.5);
    W.adT.assign((size_t)N * N * 64, 0.25);
    W.c_prior.assign(4, 2.0);
    W.fp.assign((size_t)N * 8, 3.0);
    W.fdp.assign((size_t)N * 8, 4.0);
    return W;
}

bool has_target(const Win &W, int p, int t) {
    for (int k = W.res_begin[p]; k < W.res_begin[p + 1]; k++)
        if (W.res_target[k] == t) return true;
    return false;
}

struct Counts {
    std::map<std::pair<int, int>, int> bucket;
    std::map<int, int> host;
    int R = 0;
};
Counts count(const Win &W, const std::vector<int32_t> &pts, const std::vector<uint8_t> *live) {
    Counts c;
    for (int p : pts) {
        c.host[W.point_host[p]]++;
        for (int k = W.res_begin[p]; k < W.res_begin[p + 1]; k++)
            if (!live || (*live)[k]) {
                c.bucket[{W.point_host[p], W.res_target[k]}]++;
                c.R++;
            }
    }
    return c;
}

void good(const char *name, const Win &W, const std::vector<int32_t> &pts, const std::vector<uint8_t> *live, int item_order = 0) {
    g_case = name;
    const ldso_ba_window wp = W.view();
    const Counts cn = count(W, pts, live);
    std::vector<int32_t> rg(cn.R + 1), pg(pts.size() + 1);
    int32_t n_res = -1, mism = -1;
    const int rc = ldso_ba_marg_plan_check(&wp, (int)pts.size(), pts.data(), live ? live->data() : nullptr, item_order, 0, rg.data(),
                                           pg.data(), &n_res, &mism);
    CHECK(rc == 0);
    if (rc) {
        std::printf("  %s\n", last_error());
        return;
    }
    CHECK(n_res == cn.R);
    CHECK(mism == 0);
    // the gather indices against the two layouts' orders
    Layout B;
    CHECK(build_layout(&wp, 1, 0, 1, item_order, 0, false, B, true) == 0);
    MargPlan plan;
    CHECK(plan_marg(B.wh[0], B.wd[0], wp, (int)pts.size(), pts.data(), live ? live->data() : nullptr, item_order, 0, plan) == 0);
    const WinHost &M = plan.L.wh[0], &Bh = B.wh[0];
    CHECK(M.P == (int)pts.size() && M.R == cn.R);
    std::vector<int32_t> caller_res;  // the marginalisation window's caller residual -> the parent's
    for (int p : pts)
        for (int k = W.res_begin[p]; k < W.res_begin[p + 1]; k++)
            if (!live || (*live)[k]) caller_res.push_back(k);
    std::vector<char> used_r(wp.n_residuals, 0), used_p(wp.n_points, 0);
    for (int pos = 0; pos < M.R; pos++) {
        const int g = rg[pos];
        CHECK(g == plan.rs_gather[pos]);
        CHECK(g >= 0 && g < Bh.R);
        if (g < 0 || g >= Bh.R) continue;
        CHECK(!used_r[g]);
        used_r[g] = 1;
        CHECK(Bh.rs_orig[g] == caller_res[M.rs_orig[pos]]);
    }
    for (int q = 0; q < M.P; q++) {
        const int g = pg[q];
        CHECK(g == plan.pt_gather[q]);
        CHECK(g >= 0 && g < Bh.P);
        if (g < 0 || g >= Bh.P) continue;
        CHECK(!used_p[g]);
        used_p[g] = 1;
        CHECK(Bh.pt_orig[g] == pts[M.pt_orig[q]]);
    }
}

void refused(const char *name, const Win &W, const std::vector<int32_t> &pts, const char *msg, int item_order = 0) {
    g_case = name;
    const ldso_ba_window wp = W.view();
    const int rc = ldso_ba_marg_plan_check(&wp, (int)pts.size(), pts.data(), nullptr, item_order, 0, nullptr, nullptr, nullptr, nullptr);
    CHECK(rc < 0);
    CHECK(std::strstr(last_error(), msg) != nullptr);
}

}  // namespace

int main() {
    for (int ranked = 0; ranked < 2; ranked++) {
        const Win W = make_parent(4, 300, 11, ranked);
        const int P = (int)W.point_host.size(), R = (int)W.res_target.size();
        std::vector<int32_t> all(P);
        for (int p = 0; p < P; p++) all[p] = p;
        good("empty selection", W, {}, nullptr);
        good("one point", W, {7}, nullptr);
        const std::vector<uint8_t> none(R, 0);
        good("one point without residuals", W, {7}, &none);
        good("all points without residuals", W, all, &none);
        good("all points", W, all, nullptr);
        good("all points, host-major", W, all, nullptr, 1);
        {  // all points in reverse: the marginalisation window's caller order is the list's
            std::vector<int32_t> rev(all.rbegin(), all.rend());
            good("all points reversed", W, rev, nullptr);
        }
        {  // buckets 0 -> 1 of exactly 16 and 1 -> 0 of exactly 17 residuals (k_linearize's chunk), hosts
           // of exactly 16 and 17 points (k_point_sc's block), the hosts interleaved in caller order
            std::vector<int32_t> pts;
            int n0 = 0, n1 = 0;
            for (int p = 0; p < P; p++) {
                if (W.point_host[p] == 0 && has_target(W, p, 1) && n0 < 16) pts.push_back(p), n0++;
                else if (W.point_host[p] == 1 && has_target(W, p, 0) && n1 < 17) pts.push_back(p), n1++;
                else if (W.point_host[p] == 2 && p % 3 == 0) pts.push_back(p);
            }
            const Counts cn = count(W, pts, nullptr);
            g_case = "edges: the selection";
            CHECK(cn.bucket.at({0, 1}) == 16 && cn.bucket.at({1, 0}) == 17 && cn.host.at(0) == 16 && cn.host.at(1) == 17);
            good("bucket and block edges", W, pts, nullptr);
            good("bucket and block edges, host-major", W, pts, nullptr, 1);
            // res_live takes residuals away: every third, and one point keeps a single one
            std::vector<uint8_t> live(R, 1);
            for (int k = 0; k < R; k++) live[k] = k % 3 != 0;
            const int p1 = pts[3];
            for (int k = W.res_begin[p1]; k < W.res_begin[p1 + 1]; k++) live[k] = k == W.res_begin[p1];
            good("res_live removes residuals", W, pts, &live);
            // 16 -> 17 and 17 -> 16 by one residual each way
            std::vector<uint8_t> live2(R, 1);
            bool cut = false;
            for (int p : pts)
                for (int k = W.res_begin[p]; k < W.res_begin[p + 1] && !cut; k++)
                    if (W.point_host[p] == 1 && W.res_target[k] == 0) live2[k] = 0, cut = true;
            const Counts c2 = count(W, pts, &live2);
            CHECK(c2.bucket.at({1, 0}) == 16);
            good("bucket 17 -> 16", W, pts, &live2);
        }
    }
    const Win W = make_parent(4, 300, 11, false);
    const int P = (int)W.point_host.size();
    refused("index out of range", W, {3, P}, "not a point of the parent");
    refused("negative index", W, {-1}, "not a point of the parent");
    refused("a point twice", W, {3, 5, 3}, "twice");
    refused("item order 2", W, {3, 5}, "ITEM_ORDER 2", 2);
    {
        g_case = "frame count differs";
        const ldso_ba_window wp = W.view();
        Layout B;
        CHECK(build_layout(&wp, 1, 0, 1, 0, 0, false, B, true) == 0);
        ldso_ba_window ft = wp;
        ft.n_frames = 3;
        MargPlan plan;
        const int32_t one = 1;
        CHECK(plan_marg(B.wh[0], B.wd[0], ft, 1, &one, nullptr, 0, 0, plan) < 0);
        CHECK(std::strstr(last_error(), "parent window's frames") != nullptr);
        // a sharded parent
        Layout S;
        CHECK(build_layout(&wp, 1, 0, 2, 0, 0, false, S, true) == 0);
        CHECK(plan_marg(S.wh[0], S.wd[0], wp, 1, &one, nullptr, 0, 0, plan) < 0);
        CHECK(std::strstr(last_error(), "sharded") != nullptr);
    }
    std::printf("%s: %lld checks, %d failed\n", g_fail ? "FAILED" : "ok", g_checks, g_fail);
    return g_fail ? 1 : 0;
}
