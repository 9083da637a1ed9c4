// test_edit_plan.cpp -- ldso_ba_edit_window's host planner (ldso_amd/csrc/edit_plan.cpp) as a
// stand-alone program: windows cut from one hand-made pool, the keyframe cycle's edits between them,
// the plan checked against build_layout(after) and the gather indices against the identities, then
// the refusals.  Links layout.o, edit_plan.o and error.o only (no HIP, no images: the planner reads
// structure), so the same source builds under -fsanitize=address,undefined (make sanitize-edit-plan).
#include <cstdio>
#include <cstring>
#include <map>
#include <string>
#include <vector>

#include "../../ldso_amd/csrc/edit_plan.h"

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

// the pool: points with a host and residuals to some other frames, each with an identity
struct Pool {
    int N = 0;
    std::vector<int> host;
    std::vector<std::vector<int>> targets;  // per point
    std::vector<std::vector<int>> res_id;   // per point: the residuals' identities
};
Pool make_pool(int N, int P, uint64_t seed) {
    Pool pl;
    pl.N = N;
    Lcg g{seed};
    int id = 0;
    for (int p = 0; p < P; p++) {
        const int h = (int)(g.next() % N);
        pl.host.push_back(h);
        std::vector<int> t, ids;
        for (int k = 0; k < N; k++) {
            const int f = (k + p) % N;  // shuffled target order
            if (f != h && g.next() % 10 < 6) {
                t.push_back(f);
                ids.push_back(id++);
            }
        }
        pl.targets.push_back(t);
        pl.res_id.push_back(ids);
    }
    return pl;
}

// a window cut from the pool, with its storage and the identities of its entries
struct Win {
    std::vector<int> frames, pt_id, rs_id;
    std::vector<int32_t> point_host, res_begin{0}, res_target, point_rank;
    std::vector<float> point_data, res_energy, th, precalc, c_delta;
    std::vector<double> adH, adT, c_prior, fp, fdp;
    std::vector<int8_t> res_state;
    std::vector<uint8_t> res_flags;
    ldso_ba_window view(bool values = true) const {
        ldso_ba_window v;
        std::memset(&v, 0, sizeof(v));
        v.n_frames = (int)frames.size();
        v.n_points = (int)point_host.size();
        v.n_residuals = (int)res_target.size();
        v.width = 64;
        v.height = 48;
        v.frame_energy_th = th.data();
        v.precalc = precalc.data();
        v.ad_host = adH.data();
        v.ad_target = adT.data();
        v.c_prior = c_prior.data();
        v.c_delta = c_delta.data();
        v.frame_prior = fp.data();
        v.frame_delta_prior = fdp.data();
        v.point_host = point_host.data();
        v.point_res_begin = res_begin.data();
        v.res_target = res_target.data();
        v.point_rank = point_rank.empty() ? nullptr : point_rank.data();
        if (values) {
            v.point_data = point_data.data();
            v.res_state = res_state.data();
            v.res_energy = res_energy.data();
            v.res_flags = res_flags.data();
        }
        return v;
    }
};
// keep_pt(p), keep_res(p, target): what of the pool the window holds; points in pool order
template <typename KP, typename KR>
Win cut(const Pool &pl, const std::vector<int> &frames, KP keep_pt, KR keep_res, bool ranked = false) {
    Win W;
    W.frames = frames;
    std::map<int, int> remap;
    for (size_t i = 0; i < frames.size(); i++) remap[frames[i]] = (int)i;
    for (size_t p = 0; p < pl.host.size(); p++) {
        if (!remap.count(pl.host[p]) || !keep_pt((int)p)) continue;
        W.pt_id.push_back((int)p);
        W.point_host.push_back(remap[pl.host[p]]);
        if (ranked) W.point_rank.push_back((int)((p * 7919u) % 1009u));
        for (int k = 0; k < LDSO_BA_POINT_STRIDE; k++) W.point_data.push_back((float)p + 0.01f * k);
        for (size_t k = 0; k < pl.targets[p].size(); k++) {
            const int t = pl.targets[p][k];
            if (!remap.count(t) || !keep_res((int)p, t)) continue;
            W.rs_id.push_back(pl.res_id[p][k]);
            W.res_target.push_back(remap[t]);
            W.res_state.push_back((int8_t)(pl.res_id[p][k] % 3));
            W.res_energy.push_back((float)pl.res_id[p][k]);
            W.res_flags.push_back((uint8_t)(pl.res_id[p][k] & 3));
        }
        W.res_begin.push_back((int32_t)W.res_target.size());
    }
    const size_t N = frames.size();
    W.th.assign(N, 1.f);
    W.precalc.assign(N * N * LDSO_BA_PRECALC_STRIDE, 0.f);
    W.c_delta.assign(4, 0.f);
    W.adH.assign(N * N * 64, 0.0);
    W.adT.assign(N * N * 64, 0.0);
    W.c_prior.assign(4, 0.0);
    W.fp.assign(N * 8, 0.0);
    W.fdp.assign(N * 8, 0.0);
    return W;
}

struct Src {
    std::vector<int32_t> frame, point, res;
    ldso_ba_edit edit(const ldso_ba_window *after) const { return {after, nullptr, frame.data(), point.data(), res.data()}; }
};
Src sources(const Win &before, const Win &after) {
    std::map<int, int> f, p, r;
    for (size_t i = 0; i < before.frames.size(); i++) f[before.frames[i]] = (int)i;
    for (size_t i = 0; i < before.pt_id.size(); i++) p[before.pt_id[i]] = (int)i;
    for (size_t i = 0; i < before.rs_id.size(); i++) r[before.rs_id[i]] = (int)i;
    Src s;
    for (int x : after.frames) s.frame.push_back(f.count(x) ? f[x] : -1);
    for (int x : after.pt_id) s.point.push_back(p.count(x) ? p[x] : -1);
    for (int x : after.rs_id) s.res.push_back(r.count(x) ? r[x] : -1);
    return s;
}

void check_gather(const std::vector<int32_t> &gather, const std::vector<int32_t> &order, const std::vector<int32_t> &old_order,
                  const std::vector<int32_t> &src) {
    std::vector<char> used(old_order.size(), 0);
    std::vector<int> fresh;
    for (size_t i = 0; i < src.size(); i++)
        if (src[i] < 0) fresh.push_back((int)i);
    for (size_t pos = 0; pos < gather.size(); pos++) {
        const int g = gather[pos], caller = order[pos];
        if (g >= 0) {
            CHECK((size_t)g < old_order.size());
            if ((size_t)g >= old_order.size()) continue;
            CHECK(!used[g]);
            used[g] = 1;
            CHECK(old_order[g] == src[caller]);
        } else {
            CHECK(src[caller] == -1);
            CHECK((size_t)~g < fresh.size() && fresh[~g] == caller);
        }
    }
}

void good(const char *name, const Win &before, const Win &after, int item_order = 0) {
    g_case = name;
    const Src s = sources(before, after);
    const ldso_ba_window wb = before.view(), wa = after.view();
    const ldso_ba_edit e = s.edit(&wa);
    std::vector<int32_t> rg(wa.n_residuals), pg(wa.n_points), bro(wb.n_residuals), bpo(wb.n_points), aro(wa.n_residuals),
        apo(wa.n_points);
    int32_t mism = -1;
    const int rc = ldso_ba_edit_plan_check(&wb, &e, item_order, 0, rg.data(), pg.data(), bro.data(), bpo.data(), aro.data(),
                                           apo.data(), &mism);
    CHECK(rc == 0);
    if (rc) {
        std::printf("  %s\n", last_error());
        return;
    }
    CHECK(mism == 0);
    check_gather(rg, aro, bro, s.res);
    check_gather(pg, apo, bpo, s.point);
}

template <typename F>
void refused(const char *name, const Win &before, const Win &after_in, const char *msg, F spoil, int item_order = 0) {
    g_case = name;
    Win after = after_in;
    Src s = sources(before, after);
    spoil(after, s);
    const ldso_ba_window wb = before.view(), wa = after.view();
    const ldso_ba_edit e = s.edit(&wa);
    const int rc = ldso_ba_edit_plan_check(&wb, &e, item_order, 0, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr);
    CHECK(rc < 0);
    CHECK(std::strstr(last_error(), msg) != nullptr);
    good(name, before, after_in);  // the refusal left nothing behind
}

}  // namespace

int main() {
    const Pool pl = make_pool(5, 300, 11);
    auto all_pt = [](int) { return true; };
    auto all_rs = [](int, int) { return true; };
    const std::vector<int> f4 = {0, 1, 2, 3}, f5 = {0, 1, 2, 3, 4};
    for (int ranked = 0; ranked < 2; ranked++) {
        const Win base = cut(pl, f4, all_pt, all_rs, ranked);
        good("identity", base, base);
        good("identity, host-major", base, base, 1);
        good("drop residuals", base, cut(pl, f4, all_pt, [](int p, int t) { return (p + t) % 3 != 0; }, ranked));
        good("empty a bucket", base, cut(pl, f4, all_pt, [&](int p, int t) { return !(pl.host[p] == 3 && t == 0); }, ranked));
        good("remove a host's points", base, cut(pl, f4, [&](int p) { return pl.host[p] != 2; }, all_rs, ranked));
        good("remove frame 0", base, cut(pl, {1, 2, 3}, all_pt, all_rs, ranked));
        good("remove frame 2", base, cut(pl, {0, 1, 3}, all_pt, all_rs, ranked));
        good("append a frame", cut(pl, f4, all_pt, all_rs, ranked),
             cut(pl, f5, [&](int p) { return pl.host[p] != 4; }, all_rs, ranked));
        good("keyframe cycle", base,
             cut(pl, {1, 2, 3, 4}, [&](int p) { return pl.host[p] != 4 && p % 11 != 0; }, [](int p, int t) { return (p + 2 * t) % 5 != 0; },
                 ranked));
        good("insert points", cut(pl, f4, [](int p) { return p % 5 != 0; }, all_rs, ranked), base);
        good("everything new", cut(pl, f4, [](int p) { return p % 2 == 0; }, all_rs, ranked),
             cut(pl, f4, [](int p) { return p % 2 == 1; }, all_rs, ranked));
        const Win none = cut(pl, f4, [](int) { return false; }, all_rs, ranked);
        good("no points left", base, none);
        good("from empty", none, base);
        good("empty to empty", none, none);
        good("points without residuals", base, cut(pl, f4, all_pt, [](int, int) { return false; }, ranked));
    }
    const Win base = cut(pl, f4, all_pt, all_rs);
    const Win dropped = cut(pl, f4, all_pt, [](int p, int t) { return (p + t) % 3 != 0; });
    refused("an old residual twice", base, dropped, "twice", [](Win &, Src &s) { s.res[1] = s.res[0]; });
    refused("an old point twice", base, dropped, "twice", [](Win &, Src &s) { s.point[1] = s.point[0]; });
    refused("an old frame twice", base, dropped, "twice", [](Win &, Src &s) { s.frame[1] = s.frame[0]; });
    refused("index out of range", base, dropped, "not an index", [&](Win &, Src &s) { s.res[0] = (int32_t)base.rs_id.size(); });
    refused("residual of another point", base, dropped, "image of its old point", [](Win &w, Src &s) {
        int a = -1, b = -1;
        for (size_t p = 0; p + 1 < w.res_begin.size() && b < 0; p++)
            if (w.res_begin[p + 1] > w.res_begin[p]) (a < 0 ? a : b) = w.res_begin[p];
        std::swap(s.res[a], s.res[b]);
    });
    refused("host is not the image", base, dropped, "image of its old host",
            [](Win &w, Src &) {
                for (size_t p = 0; p + 1 < w.res_begin.size(); p++)
                    if (w.res_begin[p + 1] == w.res_begin[p]) {
                        w.point_host[p] = (w.point_host[p] + 1) % 4;
                        return;
                    }
            });
    refused("carried from a removed frame", base, dropped, "removed frame", [](Win &, Src &s) { s.frame[0] = -1; });
    refused("invalid window", base, dropped, "out of range", [](Win &w, Src &) { w.res_target[0] = 9; });
    refused("item order 2", base, dropped, "ITEM_ORDER 2", [](Win &, Src &) {}, 2);
    {  // nothing new: after's per-entry arrays may be NULL; something new: they may not
        g_case = "null value arrays";
        const Src s = sources(base, dropped);
        const ldso_ba_window wb = base.view(), wa = dropped.view(false);
        const ldso_ba_edit e = s.edit(&wa);
        CHECK(ldso_ba_edit_plan_check(&wb, &e, 0, 0, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr) == 0);
        const Src s2 = sources(dropped, base);
        const ldso_ba_window wb2 = dropped.view(), wa2 = base.view(false);
        const ldso_ba_edit e2 = s2.edit(&wa2);
        CHECK(ldso_ba_edit_plan_check(&wb2, &e2, 0, 0, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr) < 0);
    }
    std::printf("%s: %lld checks, %d failed\n", g_fail ? "FAILED" : "ok", g_checks, g_fail);
    return g_fail ? 1 : 0;
}
