// test_tracking_ref.cpp -- EnergyFunctional::setCoarseTrackingRef (the tracker's reference cloud built
// on the device from the window's last pass, ldso_ct_make_reference_ba) against
// ldso_ct_make_reference fed from the face's own host-side view of that pass.
//
// Scene: one keyframe of a 5-frame window of 160x120 (300 points): optimize(3), setAdjointsF /
// setDeltaF / linearizeAll(true) as FullSystem::optimize ends, then
//   tracker A: ef->setCoarseTrackingRef(A, ...)                       device to device
//   tracker B: ldso_ct_make_reference(B, ...) with, in the face's traversal order (frames in window
//              order, each frame's points in allPoints order), every point whose residual to the
//              newest keyframe is IN (residualState): residualCenter and the point's HdiF
// The clouds of every level must be bit-identical.  A structural change that the face has not yet
// applied to the device (dropResidual) leaves the call valid and the cloud unchanged; once the
// mirror has been rebuilt the call fails with ok() false.
//
//   test_tracking_ref --cpu   argument checks without a device
//   test_tracking_ref         the GPU run
#include <cmath>
#include <cstdio>
#include <cstring>
#include <memory>
#include <vector>

#include "../../include/ldso_amd/energy_functional.h"
#include "../../include/ldso_ct.h"
#include "../../ldso_amd/csrc/synth.h"

using namespace ldso_amd;

static int g_fail = 0;
#define CHECK(cond, ...)                                     \
    do {                                                     \
        if (!(cond)) {                                       \
            std::printf("FAIL %s:%d: ", __FILE__, __LINE__); \
            std::printf(__VA_ARGS__);                        \
            std::printf("\n");                               \
            g_fail++;                                        \
        }                                                    \
    } while (0)

struct Synth {
    int N, P, R, w, h;
    std::vector<ldso_ba_frame_state> fs;
    std::vector<float> dI, th, pd, re;
    float calib[4];
    std::vector<int32_t> ph, rb, rt;
    std::vector<int8_t> rs;
    std::vector<uint8_t> rf;
    Synth(int N_, int P_, int w_, int h_, uint64_t seed) : N(N_), P(P_), R(P_ * (N_ - 1)), w(w_), h(h_) {
        fs.resize(N);
        dI.resize((size_t)N * w * h * 3);
        th.resize(N);
        pd.resize((size_t)P * LDSO_BA_POINT_STRIDE);
        ph.resize(P);
        rb.resize(P + 1);
        rt.resize(R);
        rs.resize(R);
        re.resize(R);
        rf.resize(R);
        ldso_synth_params prm = {N, P, w, h, seed, 0.05f, 0.01f, 1e-3f, 0.04f};
        ldso_synth_fill(&prm, fs.data(), dI.data(), calib, th.data(), ph.data(), pd.data(), rb.data(), rt.data(),
                        rs.data(), re.data(), rf.data());
    }
};

struct Scene {
    shared_ptr<CalibHessian> calib = std::make_shared<CalibHessian>();
    std::vector<shared_ptr<FrameHessian>> frames;
    std::vector<shared_ptr<PointHessian>> points;
    explicit Scene(const Synth &S) {
        calib->wG0 = S.w;
        calib->hG0 = S.h;
        std::memcpy(calib->value_scaledf, S.calib, sizeof(S.calib));
        for (int k = 0; k < 4; k++) calib->value[k] = calib->value_zero[k] = (double)S.calib[k] * (1.0 / 50.0);
        for (int f = 0; f < S.N; f++) {
            auto F = std::make_shared<FrameHessian>();
            F->frameID = f;
            std::memcpy(F->worldToCam_evalPT, S.fs[f].world_to_cam_evalpt, sizeof(F->worldToCam_evalPT));
            std::memcpy(F->state, S.fs[f].state, sizeof(F->state));
            std::memcpy(F->state_zero, S.fs[f].state_zero, sizeof(F->state_zero));
            F->ab_exposure = S.fs[f].ab_exposure;
            F->dI = &S.dI[(size_t)f * S.w * S.h * 3];
            F->frameEnergyTH = S.th[f];
            frames.push_back(F);
        }
        for (int p = 0; p < S.P; p++) {
            auto Pt = std::make_shared<PointHessian>();
            const float *d = &S.pd[(size_t)p * LDSO_BA_POINT_STRIDE];
            Pt->host = frames[S.ph[p]];
            Pt->u = d[0];
            Pt->v = d[1];
            Pt->setIdepth(d[2]);
            Pt->setIdepthZero(d[3]);
            Pt->priorF = d[4];
            Pt->deltaF = d[5];
            std::memcpy(Pt->color, d + 8, sizeof(Pt->color));
            std::memcpy(Pt->weights, d + 16, sizeof(Pt->weights));
            for (int k = S.rb[p]; k < S.rb[p + 1]; k++) {
                auto r = std::make_shared<PointFrameResidual>(Pt, frames[S.ph[p]], frames[S.rt[k]]);
                r->isNew = true;
                Pt->residuals.push_back(r);
            }
            points.push_back(Pt);
        }
    }
    void insertInto(EnergyFunctional &ef) {
        for (auto &F : frames) ef.insertFrame(F, calib);
        for (auto &P : points) {
            ef.insertPoint(P);
            for (auto &r : P->residuals) ef.insertResidual(r);
        }
        ef.makeIDX();
        ef.setAdjointsF(calib);
        ef.setDeltaF(calib);
    }
};

// every level of a tracker's resident cloud, [n][4] each
static std::vector<std::vector<float>> clouds(ldso_ct_ctx *ct, int levels) {
    std::vector<std::vector<float>> out;
    for (int l = 0; l < levels; l++) {
        int32_t n = -1;
        CHECK(ldso_ct_get_reference(ct, l, &n, nullptr, 0) == 0 && n >= 0, "get_reference(query): %s", ldso_ba_last_error());
        std::vector<float> v((size_t)4 * (n > 0 ? n : 0));
        if (n > 0)
            CHECK(ldso_ct_get_reference(ct, l, &n, v.data(), n) == 0, "get_reference: %s", ldso_ba_last_error());
        out.push_back(v);
    }
    return out;
}

static bool same_clouds(const std::vector<std::vector<float>> &a, const std::vector<std::vector<float>> &b) {
    if (a.size() != b.size()) return false;
    for (size_t l = 0; l < a.size(); l++)
        if (a[l].size() != b[l].size() || (!a[l].empty() && std::memcmp(a[l].data(), b[l].data(), a[l].size() * 4) != 0))
            return false;
    return true;
}

static int gpu_tests() {
    Synth S(5, 300, 160, 120, 11);
    Scene G(S);
    auto ef = std::make_shared<EnergyFunctional>(0);
    CHECK(ef->ok(), "%s", ef->lastError().c_str());
    if (!ef->ok()) return 0;
    G.insertInto(*ef);
    // the keyframe's image in two trackers: A is driven by the face, B by the host route
    const int kf = S.N - 1;
    std::vector<float> color((size_t)S.w * S.h);
    for (size_t i = 0; i < color.size(); i++) color[i] = S.dI[((size_t)kf * S.w * S.h + i) * 3];
    ldso_ct_ctx *A = nullptr, *B = nullptr;
    int32_t nl = 0;
    CHECK(ldso_ct_create(0, S.w, S.h, &A, &nl) == 0 && ldso_ct_create(0, S.w, S.h, &B, nullptr) == 0, "ldso_ct_create: %s",
          ldso_ba_last_error());
    if (!A || !B) return 0;
    CHECK(ldso_ct_set_new_frame(A, color.data(), S.fs[kf].ab_exposure, nullptr) == 0 &&
              ldso_ct_set_new_frame(B, color.data(), S.fs[kf].ab_exposure, nullptr) == 0,
          "set_new_frame: %s", ldso_ba_last_error());
    const double expo = S.fs[kf].ab_exposure, aff_a = 0.01, aff_b = 0.5;

    // before any pass the library has nothing to read
    CHECK(!ef->setCoarseTrackingRef(A, nullptr, expo, aff_a, aff_b) && !ef->ok(), "no pass yet: refused");
    ef = std::make_shared<EnergyFunctional>(0);
    G = Scene(S);
    G.insertInto(*ef);

    ef->optimize(3, G.calib);
    ef->setAdjointsF(G.calib);
    ef->setDeltaF(G.calib);
    ef->linearizeAll(true);
    CHECK(ef->ok(), "optimize + linearizeAll(true): %s", ef->lastError().c_str());

    CHECK(ef->setCoarseTrackingRef(A, nullptr, expo, aff_a, aff_b) && ef->ok(), "setCoarseTrackingRef: %s",
          ef->lastError().c_str());
    const auto dev = clouds(A, nl);

    // the host route from the face's own view of the pass, in the face's traversal order
    std::vector<float> center, hdi;
    const FrameHessian *newest = ef->frames.back().get();
    for (auto &F : ef->frames)
        for (auto &p : ef->allPoints) {
            if (p->host.lock() != F) continue;
            for (auto &r : p->residuals) {
                if (r->target.lock().get() != newest || r->mirrorIdx < 0) continue;
                if (ef->residualState(r->mirrorIdx) != IN) continue;
                const float *c = ef->residualCenter(r->mirrorIdx);
                center.insert(center.end(), c, c + 3);
                hdi.push_back(p->HdiF);
            }
        }
    CHECK(ef->ok(), "residualState / residualCenter: %s", ef->lastError().c_str());
    CHECK(hdi.size() >= 50, "contributions: %zu", hdi.size());
    std::vector<int32_t> pc_n(LDSO_CT_MAX_LEVELS, -1);
    CHECK(ldso_ct_make_reference(B, nullptr, (int32_t)hdi.size(), center.data(), hdi.data(), expo, aff_a, aff_b,
                                 pc_n.data()) == 0,
          "ldso_ct_make_reference: %s", ldso_ba_last_error());
    const auto host = clouds(B, nl);
    CHECK(nl >= 2 && (size_t)pc_n[0] > hdi.size(), "levels %d, pc_n[0] %d: the dilation ran", nl, pc_n[0]);
    for (int l = 0; l < nl; l++) {
        CHECK((size_t)pc_n[l] * 4 == host[l].size() && pc_n[l] > 0, "level %d: pc_n %d", l, pc_n[l]);
        CHECK(dev[l].size() == host[l].size() &&
                  (dev[l].empty() || std::memcmp(dev[l].data(), host[l].data(), dev[l].size() * 4) == 0),
              "level %d: face cloud (%zu) differs from the host route's (%zu)", l, dev[l].size() / 4, host[l].size() / 4);
    }
    // a frame source of its own: tracker B's frame feeds tracker A's cloud
    CHECK(ef->setCoarseTrackingRef(A, B, expo, aff_a, aff_b) && same_clouds(clouds(A, nl), dev), "frame_src = B: %s",
          ef->lastError().c_str());

    // a structural change the face has not applied to the device yet: the pass is still there
    shared_ptr<PointFrameResidual> victim;
    for (auto &p : ef->allPoints)
        for (auto &r : p->residuals)
            if (!victim && r->target.lock().get() == newest) victim = r;
    ef->syncResiduals();  // the objects hold the pass, as after the reference's linearizeAll(true)
    ef->dropResidual(victim);
    CHECK(ef->setCoarseTrackingRef(A, nullptr, expo, aff_a, aff_b) && same_clouds(clouds(A, nl), dev),
          "pending structural change: %s", ef->lastError().c_str());
    // marginalizePointsF rebuilds the mirror (and runs its pass on the marginalisation context)
    int marked = 0;
    for (auto &p : ef->allPoints)
        if (p->host.lock() == ef->frames[0] && marked < 5) {
            p->status = PointStatus::MARGINALIZED;
            marked++;
        }
    ef->marginalizePointsF();
    CHECK(ef->ok() && marked == 5, "marginalizePointsF: %s", ef->lastError().c_str());
    CHECK(!ef->setCoarseTrackingRef(A, nullptr, expo, aff_a, aff_b) && !ef->ok() &&
              ef->lastError().find("pass") != std::string::npos,
          "rebuilt mirror refused: %s", ef->lastError().c_str());
    CHECK(same_clouds(clouds(A, nl), dev), "a refused call leaves the tracker's reference alone");

    ef.reset();
    ldso_ct_destroy(A);
    ldso_ct_destroy(B);
    return 0;
}

static int cpu_tests() {
    Synth S(4, 60, 160, 120, 3);
    Scene G(S);
    auto ef = std::make_shared<EnergyFunctional>(1 << 20);  // no such device: reported, never thrown
    CHECK(!ef->ok(), "creating a context on a missing device must fail");
    G.insertInto(*ef);
    CHECK(!ef->setCoarseTrackingRef(nullptr, nullptr, 1.0, 0.0, 0.0) &&
              ef->lastError().find("null tracker") != std::string::npos,
          "null tracker refused: %s", ef->lastError().c_str());
    // without a device context nothing is dereferenced
    CHECK(!ef->setCoarseTrackingRef(reinterpret_cast<ldso_ct_ctx *>(&S), nullptr, 1.0, 0.0, 0.0) && !ef->ok(),
          "no device context: refused");
    // the C ABI refuses null arguments before any device call
    float c[3] = {0, 0, 0}, h[1] = {1};
    int32_t n = 0;
    CHECK(ldso_ct_make_reference(nullptr, nullptr, 1, c, h, 1.0, 0.0, 0.0, nullptr) < 0 &&
              std::strlen(ldso_ba_last_error()) > 0,
          "make_reference(null)");
    CHECK(ldso_ct_make_reference_ba(nullptr, nullptr, nullptr, 0, -1, 1.0, 0.0, 0.0, nullptr) < 0, "make_reference_ba(null)");
    CHECK(ldso_ct_get_reference(nullptr, 0, &n, nullptr, 0) < 0, "get_reference(null)");
    return 0;
}

int main(int argc, char **argv) {
    const bool cpu = argc > 1 && std::strcmp(argv[1], "--cpu") == 0;
    if (cpu) cpu_tests();
    else gpu_tests();
    std::printf("%s: %d failure(s)\n", cpu ? "cpu" : "gpu", g_fail);
    return g_fail ? 1 : 0;
}
