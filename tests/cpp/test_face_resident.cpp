// test_face_resident.cpp -- the C++ host face with resident frames (the default: images enter the
// context's frame store once, the window is reloaded by frame id) against the same face with
// setResidentFrames(false) (every structural change gathers and uploads all images through
// ldso_ba_load, the path tests/cpp/test_energy_functional.cpp checks against the oracle).
//
// Scene: 5 keyframes of 160x120 with the points they host (of 300 over 6 frames), then
//   optimize(3), setAdjointsF / setDeltaF / linearizeAll(true)
//   frame 0 leaves: its points MARGINALIZED + marginalizePointsF (the marginalisation context
//   borrows the parent's window images), marginalizeFrame, dropResidual of its observations
//   a sixth keyframe enters with a residual from every remaining point:
//     resident face: ldso_ct_set_new_frame on its intensities, insertFrame(fh, Hcalib, tracker)
//                    with fh->dI == nullptr
//     legacy face:   insertFrame(fh, Hcalib) with the host dI
//   optimize(2)
// Frame states, energies, point inverse depths, HM and bM must be bit-identical between the two,
// and the resident face must move no image bytes host -> device over the second keyframe.
//
//   test_face_resident --cpu   bookkeeping and argument checks without a device
//   test_face_resident         the GPU run
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

// what the two faces must agree on, bit for bit
struct Trace {
    std::vector<Vec3> energies;
    std::vector<double> states, HM, bM;
    std::vector<float> idepth;
    int64_t h2d_second = -1, d2d_second = -1, allocs_second = -1;
    bool ok = false;
};

static shared_ptr<FrameHessian> make_frame(const Synth &S, int f, bool host_image) {
    auto F = std::make_shared<FrameHessian>();
    F->frameID = f;
    std::memcpy(F->worldToCam_evalPT, S.fs[f].world_to_cam_evalpt, sizeof(F->worldToCam_evalPT));
    std::memcpy(F->state, S.fs[f].state, sizeof(F->state));
    std::memcpy(F->state_zero, S.fs[f].state_zero, sizeof(F->state_zero));
    F->ab_exposure = S.fs[f].ab_exposure;
    F->dI = host_image ? &S.dI[(size_t)f * S.w * S.h * 3] : nullptr;
    F->frameEnergyTH = S.th[f];
    return F;
}

// the window of frames [0, n0) of S: the points they host, the residuals among them
struct Scene {
    shared_ptr<CalibHessian> calib = std::make_shared<CalibHessian>();
    std::vector<shared_ptr<FrameHessian>> frames;
    std::vector<shared_ptr<PointHessian>> points;
    Scene(const Synth &S, int n0) {
        calib->wG0 = S.w;
        calib->hG0 = S.h;
        std::memcpy(calib->value_scaledf, S.calib, sizeof(S.calib));
        for (int k = 0; k < 4; k++) calib->value[k] = calib->value_zero[k] = (double)S.calib[k] * (1.0 / 50.0);
        for (int f = 0; f < n0; f++) frames.push_back(make_frame(S, f, true));
        for (int p = 0; p < S.P; p++) {
            if (S.ph[p] >= n0) continue;
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
                if (S.rt[k] >= n0) continue;
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

static void record(EnergyFunctional &ef, Trace &T) {
    for (auto &F : ef.frames) T.states.insert(T.states.end(), F->state, F->state + 10);
    for (auto &p : ef.allPoints) T.idepth.push_back(p->idepth);
    T.HM.insert(T.HM.end(), ef.HM.data(), ef.HM.data() + (size_t)ef.HM.rows() * ef.HM.cols());
    T.bM.insert(T.bM.end(), ef.bM.data(), ef.bM.data() + ef.bM.size());
}

static Trace drive(const Synth &S, bool resident) {
    Trace T;
    const char *tag = resident ? "resident" : "legacy";
    const int n0 = S.N - 1;
    Scene G(S, n0);
    auto ef = std::make_shared<EnergyFunctional>(0);
    CHECK(ef->ok(), "%s: %s", tag, ef->lastError().c_str());
    if (!ef->ok()) return T;
    CHECK(ef->residentFrames(), "resident frames are the default");
    ef->setResidentFrames(resident);
    G.insertInto(*ef);
    ldso_ba_opt_settings all_its = LDSO_BA_OPT_SETTINGS_INIT;
    all_its.th_opt_iterations = 0.0f;  // every iteration: both faces run the same number by construction
    std::vector<Vec3> e;
    ef->optimize(3, G.calib, &e, nullptr, nullptr, &all_its);
    CHECK(ef->ok() && e.size() == 4, "%s optimize(3): %s", tag, ef->lastError().c_str());
    T.energies = e;
    ef->setAdjointsF(G.calib);
    ef->setDeltaF(G.calib);
    T.energies.push_back(ef->linearizeAll(true));
    record(*ef, T);

    int64_t x0[4], x1[4];
    CHECK(ldso_ba_transfer_stats(ef->context(), x0) == 0, "transfer stats");
    // frame 0 leaves the window
    auto f0 = ef->frames[0];
    f0->flaggedForMarginalization = true;
    for (auto &p : ef->allPoints)
        if (p->host.lock() == f0) p->status = PointStatus::MARGINALIZED;
    ef->marginalizePointsF();
    CHECK(ef->ok() && ef->resInM > 0, "%s marginalizePointsF: %s", tag, ef->lastError().c_str());
    ef->marginalizeFrame(f0);
    CHECK(ef->ok() && ef->nFrames == n0 - 1, "%s marginalizeFrame: %s", tag, ef->lastError().c_str());
    for (auto &p : std::vector<shared_ptr<PointHessian>>(ef->allPoints)) {
        const auto rs = p->residuals;
        for (auto &r : rs)
            if (r->target.lock() == f0) ef->dropResidual(r);
    }
    // the sixth keyframe enters
    ldso_ct_ctx *ct = nullptr;
    auto F = make_frame(S, n0, !resident);
    if (resident) {
        int32_t nl = 0;
        std::vector<float> color((size_t)S.w * S.h);
        for (size_t i = 0; i < color.size(); i++) color[i] = S.dI[((size_t)n0 * S.w * S.h + i) * 3];
        CHECK(ldso_ct_create(0, S.w, S.h, &ct, &nl) == 0, "ldso_ct_create: %s", ldso_ba_last_error());
        CHECK(ct && ldso_ct_set_new_frame(ct, color.data(), S.fs[n0].ab_exposure, nullptr) == 0, "set_new_frame: %s",
              ldso_ba_last_error());
        CHECK(F->dI == nullptr, "the handed-over frame has no host image");
        ef->insertFrame(F, G.calib, ct);
    } else {
        ef->insertFrame(F, G.calib);
    }
    CHECK(ef->ok() && ef->nFrames == n0, "%s insertFrame: %s", tag, ef->lastError().c_str());
    for (auto &p : ef->allPoints) {
        auto r = std::make_shared<PointFrameResidual>(p, p->host.lock(), F);
        r->isNew = true;
        p->residuals.push_back(r);
        ef->insertResidual(r);
    }
    ef->makeIDX();
    ef->setAdjointsF(G.calib);
    ef->setDeltaF(G.calib);
    e.clear();
    ef->optimize(2, G.calib, &e, nullptr, nullptr, &all_its);
    CHECK(ef->ok() && e.size() == 3, "%s optimize(2): %s", tag, ef->lastError().c_str());
    CHECK(ldso_ba_transfer_stats(ef->context(), x1) == 0, "transfer stats");
    T.h2d_second = x1[0] - x0[0];
    T.d2d_second = x1[1] - x0[1];
    T.allocs_second = x1[2] - x0[2];
    T.energies.insert(T.energies.end(), e.begin(), e.end());
    record(*ef, T);
    T.ok = ef->ok();
    ef.reset();
    if (ct) ldso_ct_destroy(ct);
    return T;
}

template <typename V>
static bool same_bits(const std::vector<V> &a, const std::vector<V> &b) {
    return a.size() == b.size() && (a.empty() || std::memcmp(a.data(), b.data(), a.size() * sizeof(V)) == 0);
}

static int gpu_tests() {
    Synth S(6, 300, 160, 120, 11);
    const Trace A = drive(S, true), B = drive(S, false);
    CHECK(A.ok && B.ok, "both faces ran");
    if (!A.ok || !B.ok) return 0;
    CHECK(A.energies.size() == B.energies.size(), "energy count");
    for (size_t i = 0; i < A.energies.size() && i < B.energies.size(); i++)
        CHECK(std::memcmp(A.energies[i].data(), B.energies[i].data(), sizeof(Vec3)) == 0,
              "energy %zu: resident (%.17g, %g) legacy (%.17g, %g)", i, A.energies[i][0], A.energies[i][2], B.energies[i][0],
              B.energies[i][2]);
    CHECK(A.energies[0][2] > 100, "the passes see residuals (#IN %g)", A.energies[0][2]);
    CHECK(same_bits(A.states, B.states), "frame states bit-identical");
    CHECK(same_bits(A.idepth, B.idepth), "point inverse depths bit-identical");
    CHECK(same_bits(A.HM, B.HM), "HM bit-identical");
    CHECK(same_bits(A.bM, B.bM), "bM bit-identical");
    double hm = 0;
    for (double v : A.HM) hm += std::fabs(v);
    CHECK(hm > 0, "HM carries the marginalised points");
    const int64_t frame_bytes = (int64_t)S.w * S.h * 3 * sizeof(float);
    std::printf("second keyframe: resident h2d %lld d2d %lld allocs %lld | legacy h2d %lld d2d %lld allocs %lld\n",
                (long long)A.h2d_second, (long long)A.d2d_second, (long long)A.allocs_second, (long long)B.h2d_second,
                (long long)B.d2d_second, (long long)B.allocs_second);
    CHECK(A.h2d_second == 0, "resident face: %lld image bytes host -> device over the second keyframe", (long long)A.h2d_second);
    CHECK(A.allocs_second == 0, "resident face: %lld image allocations over the second keyframe", (long long)A.allocs_second);
    CHECK(A.d2d_second > 0, "resident face copies device to device");
    CHECK(B.h2d_second == (S.N - 1) * frame_bytes, "legacy face uploads the whole window: %lld", (long long)B.h2d_second);
    return 0;
}

static int cpu_tests() {
    Synth S(4, 60, 160, 120, 3);
    Scene G(S, 4);
    auto ef = std::make_shared<EnergyFunctional>(1 << 20);  // no such device: reported, never thrown
    CHECK(!ef->ok(), "creating a context on a missing device must fail");
    CHECK(ef->residentFrames(), "resident frames are the default");
    G.insertInto(*ef);  // no context: nothing is put, the bookkeeping runs
    CHECK(ef->nFrames == 4 && ef->nPoints == 60 && ef->nResiduals == 180, "counts %d %d %d", ef->nFrames, ef->nPoints,
          ef->nResiduals);
    auto F = make_frame(S, 0, false);
    F->frameID = 77;
    ef->insertFrame(F, G.calib, nullptr);
    CHECK(ef->nFrames == 4 && ef->lastError().find("null tracker") != std::string::npos, "null tracker refused: %s",
          ef->lastError().c_str());
    ef->setResidentFrames(false);
    CHECK(!ef->residentFrames(), "setResidentFrames(false)");
    ef->insertFrame(F, G.calib, reinterpret_cast<const ldso_ct_ctx *>(&S));  // never dereferenced on this path
    CHECK(ef->nFrames == 4 && ef->lastError().find("resident frames") != std::string::npos,
          "tracker hand-off needs resident frames: %s", ef->lastError().c_str());
    ef->marginalizeFrame(G.frames[3]);
    CHECK(ef->nFrames == 3, "marginalizeFrame without a store");
    // the C ABI refuses null arguments before any device call
    int64_t ids[2] = {0, 1}, st[4];
    float px[12] = {0};
    ldso_ba_window w;
    std::memset(&w, 0, sizeof(w));
    CHECK(ldso_ba_frames_reserve(nullptr, 4, 160, 120) < 0, "reserve(null)");
    CHECK(ldso_ba_frame_put(nullptr, 0, px) < 0, "put(null)");
    CHECK(ldso_ba_frame_put_device(nullptr, 0, px, nullptr, nullptr) < 0, "put_device(null)");
    CHECK(ldso_ba_frame_put_tracker(nullptr, 0, nullptr) < 0, "put_tracker(null)");
    CHECK(ldso_ba_frame_drop(nullptr, 0) < 0, "drop(null)");
    CHECK(ldso_ba_frame_get(nullptr, 0, px, nullptr) < 0, "get(null)");
    CHECK(ldso_ba_load_frames(nullptr, 1, &w, ids, 0, 1) < 0, "load_frames(null)");
    CHECK(ldso_ba_transfer_stats(nullptr, st) < 0 && std::strlen(ldso_ba_last_error()) > 0, "transfer_stats(null)");
    return 0;
}

int main(int argc, char **argv) {
    const bool cpu = argc > 1 && std::strcmp(argv[1], "--cpu") == 0;
    if (cpu) cpu_tests();
    else gpu_tests();
    std::printf("%s: %d failure(s)\n", cpu ? "cpu" : "gpu", g_fail);
    return g_fail ? 1 : 0;
}
