// test_face_close.cpp -- closing a keyframe through the C++ host face with the device path
// (flagPoints + setDeviceMarginalization(true): ldso_ba_flag_points classifies the points where the
// residual states live, marginalizePointsF gathers its second context from the loaded window's device
// arrays, one ldso_ba_edit_window applies the whole close) against the same face on the host path
// (the residuals are read back, the decision of FullSystem::flagPointsForRemoval is taken on the
// objects, marginalizePointsF packs its window from them).
//
// The scene and its keyframes are test_face_resident.cpp's, both faces resident with incremental
// edits: optimize(3), linearizeAll(true), then the full close of FullSystem::makeKeyFrame
// (FullSystem.cc:606-634) with frame 0 flagged for marginalisation: removeOutliers and
// flagPointsForRemoval's decision, dropResidual of the inactive residuals, dropPointsF,
// marginalizePointsF, marginalizeFrame; a sixth keyframe enters from the tracker with a residual from
// every remaining point, optimize(2).  min_idepth_h_marg is the median idepth_hessian of frame 0's
// points, so that both MARGINALIZED and OUT occur.  Point statuses, the bookkeeping (numGood,
// lastState, the dropped residuals), frame states, energies, inverse depths, HM, bM and resInM must be
// bit-identical; on the device path no residual array is read back over the cycle
// (residualReadBacks() == 0), marginalizePointsF is served from the device and no edit falls back.
// A second comparison lets the sixth keyframe's residuals enter with a state_NewEnergy that is not
// their state_energy: the edit then cannot carry the deferred read-back, which happens once, before it.
//
//   test_face_close --cpu   the switches, counters and refusals without a device
//   test_face_close         the GPU run
#define main face_resident_main
#include "test_face_resident.cpp"  // Synth, Scene, Trace, make_frame, record, same_bits, CHECK
#undef main

#include <algorithm>

struct CloseTrace : Trace {
    std::vector<int8_t> status, lastState;
    std::vector<int> numGood, removed;  // removed: (point, position in its residuals) of every dropped residual
    int counts[4] = {0, 0, 0, 0};
    int resInM = -1;
    long readBacks = -1, deviceMargs = -1, applied = -1, fallen = -1;
};

// the decision tree of ldso_ba_flag_points (include/ldso_ba.h) on the objects, after a read-back:
// FullSystem.cc:1356-1424 and :1654 with PointHessian::isOOB / isInlierNew (PointHessian.h:53-78)
static int host_status(const PointHessian &p, const ldso_ba_flag_params &fp, int numGood, const int8_t ls[2], int *ng_out) {
    int n_live = 0, vis = 0;
    for (auto &r : p.residuals) {
        if (!r->isActive()) continue;
        n_live++;
        if (r->state_state == IN && r->target.lock()->flaggedForMarginalization) vis++;
    }
    const int A = fp.min_good_active_res_for_marg, G = fp.min_good_res_for_marg, ng = numGood + n_live;
    *ng_out = ng;
    if (p.idepth_scaled < 0 || n_live == 0) return LDSO_BA_PT_OUTLIER;
    const bool oob = (n_live >= A && ng > G + 10 && n_live - vis < A) || ls[0] == OOB ||
                     (n_live >= 2 && ls[0] == OUTLIER && ls[1] == OUTLIER);
    if (oob || p.host.lock()->flaggedForMarginalization)
        return n_live >= A && ng >= G && p.idepth_hessian > fp.min_idepth_h_marg ? LDSO_BA_PT_MARGINALIZED : LDSO_BA_PT_OUT;
    return LDSO_BA_PT_ACTIVE;
}

// newEnergyDiffers: the sixth keyframe's residuals enter with state_NewEnergy = 1.5, not their
// state_energy, so they need an upload of their own after the edit and the deferred read-back cannot
// stay deferred through it
static CloseTrace drive_close(const Synth &S, bool device, bool newEnergyDiffers) {
    CloseTrace T;
    const char *tag = device ? "device" : "host";
    const int n0 = S.N - 1;
    Scene G(S, n0);
    auto ef = std::make_shared<EnergyFunctional>(0);
    CHECK(ef->ok(), "%s: %s", tag, ef->lastError().c_str());
    if (!ef->ok()) return T;
    CHECK(!ef->deviceMarginalization(), "device marginalisation is off by default");
    ef->setIncrementalEdits(true);
    ef->setDeviceMarginalization(device);
    G.insertInto(*ef);
    ldso_ba_opt_settings all_its = LDSO_BA_OPT_SETTINGS_INIT;
    all_its.th_opt_iterations = 0.0f;
    std::vector<Vec3> e;
    ef->optimize(3, G.calib, &e, nullptr, nullptr, &all_its);
    CHECK(ef->ok() && e.size() == 4, "%s optimize(3): %s", tag, ef->lastError().c_str());
    T.energies = e;
    ef->setAdjointsF(G.calib);
    ef->setDeltaF(G.calib);
    T.energies.push_back(ef->linearizeAll(true));
    record(*ef, T);
    const long rb0 = ef->residualReadBacks();

    // ---- the close: frame 0 is flagged -------------------------------------------------------
    auto f0 = ef->frames[0];
    f0->flaggedForMarginalization = true;
    const std::vector<shared_ptr<PointHessian>> pts = ef->allPoints;
    const int P = (int)pts.size(), N = ef->nFrames;
    // the frontend's bookkeeping: numGoodResiduals, lastResiduals (the residuals to the newest and
    // second-newest keyframe; where the point is hosted there, a retained state)
    std::vector<int32_t> numGood(P), lastRes(2 * P, -1);
    std::vector<int8_t> lastState(2 * P);
    std::vector<PointFrameResidual *> lastPtr(2 * P, nullptr);
    std::vector<float> ih0;
    for (int q = 0; q < P; q++) {
        numGood[q] = q % 3 == 0 ? 12 : 2;
        lastState[2 * q] = (int8_t)(q % 5 == 0 ? OUTLIER : q % 11 == 0 ? OOB : IN);
        lastState[2 * q + 1] = (int8_t)(q % 5 == 0 ? OUTLIER : IN);
        for (auto &r : pts[q]->residuals) {
            const int t = r->target.lock()->idx;
            if (t >= N - 2) lastPtr[2 * q + (N - 1 - t)] = r.get();
        }
        for (int i = 0; i < 2; i++)
            if (lastPtr[2 * q + i]) lastRes[2 * q + i] = lastPtr[2 * q + i]->mirrorIdx;
        if (pts[q]->host.lock() == f0) ih0.push_back(pts[q]->idepth_hessian);  // linearizeAll wrote it back
    }
    CHECK(!ih0.empty(), "frame 0 hosts points");
    if (ih0.empty()) return T;
    std::sort(ih0.begin(), ih0.end());
    ldso_ba_flag_params fp;
    ldso_ba_default_flag_params(&fp);
    fp.min_idepth_h_marg = ih0[ih0.size() / 2];

    std::vector<PointFrameResidual *> toRemove;
    T.status.resize(P);
    T.numGood.resize(P);
    T.lastState.resize(2 * P);
    if (device) {
        const EnergyFunctional::FlagResult fr = ef->flagPoints(&fp, {}, numGood, lastRes, lastState);
        CHECK(fr.ok && ef->ok(), "flagPoints: %s", ef->lastError().c_str());
        if (!fr.ok) return T;
        toRemove = fr.toRemove;
        T.numGood = fr.numGood;
        T.lastState = fr.lastState;
        std::memcpy(T.counts, fr.counts, sizeof(T.counts));
        for (int q = 0; q < P; q++) T.status[q] = (int8_t)pts[q]->status;
    } else {
        ef->syncResiduals();  // the read-back flagPointsForRemoval's loop over the residuals costs
        for (int q = 0; q < P; q++) {
            int8_t ls[2];
            for (int i = 0; i < 2; i++) ls[i] = lastPtr[2 * q + i] ? (int8_t)lastPtr[2 * q + i]->state_state : lastState[2 * q + i];
            const int st = host_status(*pts[q], fp, numGood[q], ls, &T.numGood[q]);
            pts[q]->status = (PointStatus)st;
            T.status[q] = (int8_t)st;
            T.counts[st]++;
            T.lastState[2 * q] = ls[0];
            T.lastState[2 * q + 1] = ls[1];
            for (auto &r : pts[q]->residuals)
                if (!r->isActive()) toRemove.push_back(r.get());
        }
    }
    std::printf("%s: ACTIVE %d OUTLIER %d OUT %d MARGINALIZED %d, %zu residuals dropped\n", tag, T.counts[0], T.counts[1],
                T.counts[2], T.counts[3], toRemove.size());
    for (PointFrameResidual *r : toRemove) {
        auto p = r->point.lock();
        const auto it = std::find_if(p->residuals.begin(), p->residuals.end(),
                                     [r](const shared_ptr<PointFrameResidual> &x) { return x.get() == r; });
        T.removed.push_back((int)(std::find(pts.begin(), pts.end(), p) - pts.begin()));
        T.removed.push_back((int)(it - p->residuals.begin()));
        ef->dropResidual(*it);
    }
    ef->dropPointsF();
    ef->marginalizePointsF();
    CHECK(ef->ok(), "%s marginalizePointsF: %s", tag, ef->lastError().c_str());
    T.resInM = ef->resInM;
    ef->marginalizeFrame(f0);
    CHECK(ef->ok() && ef->nFrames == n0 - 1, "%s marginalizeFrame: %s", tag, ef->lastError().c_str());
    for (auto &p : std::vector<shared_ptr<PointHessian>>(ef->allPoints)) {
        const auto rs = p->residuals;
        for (auto &r : rs)
            if (r->target.lock() == f0) ef->dropResidual(r);
    }
    // the sixth keyframe enters from the tracker
    ldso_ct_ctx *ct = nullptr;
    auto F = make_frame(S, n0, false);
    int32_t nl = 0;
    std::vector<float> color((size_t)S.w * S.h);
    for (size_t i = 0; i < color.size(); i++) color[i] = S.dI[((size_t)n0 * S.w * S.h + i) * 3];
    CHECK(ldso_ct_create(0, S.w, S.h, &ct, &nl) == 0, "ldso_ct_create: %s", ldso_ba_last_error());
    CHECK(ct && ldso_ct_set_new_frame(ct, color.data(), S.fs[n0].ab_exposure, nullptr) == 0, "set_new_frame: %s",
          ldso_ba_last_error());
    ef->insertFrame(F, G.calib, ct);
    CHECK(ef->ok() && ef->nFrames == n0, "%s insertFrame: %s", tag, ef->lastError().c_str());
    for (auto &p : ef->allPoints) {
        auto r = std::make_shared<PointFrameResidual>(p, p->host.lock(), F);
        r->isNew = true;
        if (newEnergyDiffers) r->state_NewEnergy = 1.5;
        p->residuals.push_back(r);
        ef->insertResidual(r);
    }
    ef->makeIDX();
    ef->setAdjointsF(G.calib);
    ef->setDeltaF(G.calib);
    e.clear();
    ef->optimize(2, G.calib, &e, nullptr, nullptr, &all_its);
    CHECK(ef->ok() && e.size() == 3, "%s optimize(2): %s", tag, ef->lastError().c_str());
    T.energies.insert(T.energies.end(), e.begin(), e.end());
    record(*ef, T);
    T.readBacks = ef->residualReadBacks() - rb0;
    T.deviceMargs = ef->deviceMarginalizations();
    T.applied = ef->editsApplied();
    T.fallen = ef->editsFallenBack();
    T.ok = ef->ok();
    ef.reset();
    if (ct) ldso_ct_destroy(ct);
    return T;
}

// the device path against the host path over the same close: everything they compute is bit-identical
static bool same_results(const CloseTrace &A, const CloseTrace &B) {
    CHECK(A.ok && B.ok, "both faces ran");
    if (!A.ok || !B.ok) return false;
    CHECK(same_bits(A.status, B.status), "point statuses identical");
    CHECK(std::memcmp(A.counts, B.counts, sizeof(A.counts)) == 0, "status counts identical");
    CHECK(A.counts[LDSO_BA_PT_MARGINALIZED] > 0 && A.counts[LDSO_BA_PT_OUT] > 0 && A.counts[LDSO_BA_PT_ACTIVE] > 0,
          "MARGINALIZED, OUT and ACTIVE all occur (%d %d %d)", A.counts[3], A.counts[2], A.counts[0]);
    CHECK(same_bits(A.numGood, B.numGood), "numGoodResiduals identical");
    CHECK(same_bits(A.lastState, B.lastState), "lastResiduals' states identical");
    CHECK(same_bits(A.removed, B.removed), "the dropped residuals are the same, in the same order");
    CHECK(A.energies.size() == B.energies.size(), "energy count");
    for (size_t i = 0; i < A.energies.size() && i < B.energies.size(); i++)
        CHECK(std::memcmp(A.energies[i].data(), B.energies[i].data(), sizeof(Vec3)) == 0,
              "energy %zu: device (%.17g, %g) host (%.17g, %g)", i, A.energies[i][0], A.energies[i][2], B.energies[i][0],
              B.energies[i][2]);
    CHECK(same_bits(A.states, B.states), "frame states bit-identical");
    CHECK(same_bits(A.idepth, B.idepth), "point inverse depths bit-identical");
    CHECK(same_bits(A.HM, B.HM), "HM bit-identical");
    CHECK(same_bits(A.bM, B.bM), "bM bit-identical");
    CHECK(A.resInM == B.resInM && A.resInM > 0, "resInM %d / %d", A.resInM, B.resInM);
    double hm = 0;
    for (double v : A.HM) hm += std::fabs(v);
    CHECK(hm > 0, "HM carries the marginalised points");
    return true;
}

static void gpu_close_tests() {
    Synth S(6, 300, 160, 120, 11);
    const CloseTrace A = drive_close(S, true, false), B = drive_close(S, false, false);
    if (same_results(A, B)) {
        std::printf("device path: %ld read-backs, %ld device marginalisations, %ld edits applied, %ld fallen back; "
                    "host path: %ld, %ld, %ld, %ld\n",
                    A.readBacks, A.deviceMargs, A.applied, A.fallen, B.readBacks, B.deviceMargs, B.applied, B.fallen);
        CHECK(A.readBacks == 0, "device path: %ld residual read-backs over the cycle", A.readBacks);
        CHECK(A.deviceMargs == 1, "marginalizePointsF was served from the device (%ld): %s", A.deviceMargs, ldso_ba_last_error());
        CHECK(A.applied >= 1 && A.fallen == 0, "device path: %ld edits applied, %ld fallen back: %s", A.applied, A.fallen,
              ldso_ba_last_error());
        CHECK(B.readBacks >= 1 && B.deviceMargs == 0 && B.fallen == 0, "host path: %ld read-backs, %ld device, %ld fallen back",
              B.readBacks, B.deviceMargs, B.fallen);
    }
    // new residuals whose state_NewEnergy differs: the edit is still applied, after the one read-back it
    // forces (the loaded window into the loaded mirror's objects)
    const CloseTrace C = drive_close(S, true, true), D = drive_close(S, false, true);
    if (same_results(C, D)) {
        std::printf("new energies differ: device path: %ld read-backs, %ld device marginalisations, %ld edits applied, "
                    "%ld fallen back; host path: %ld, %ld, %ld, %ld\n",
                    C.readBacks, C.deviceMargs, C.applied, C.fallen, D.readBacks, D.deviceMargs, D.applied, D.fallen);
        CHECK(C.readBacks == 1 && C.applied == 1 && C.fallen == 0,
              "device path with differing new energies: %ld read-backs, %ld edits applied, %ld fallen back: %s", C.readBacks,
              C.applied, C.fallen, ldso_ba_last_error());
    }
}

static void cpu_close_tests() {
    auto ef = std::make_shared<EnergyFunctional>(1 << 20);  // no such device
    CHECK(!ef->deviceMarginalization(), "off by default");
    ef->setDeviceMarginalization(true);
    CHECK(ef->deviceMarginalization() && ef->deviceMarginalizations() == 0 && ef->residualReadBacks() == 0,
          "the switch and its counters");
    const EnergyFunctional::FlagResult fr = ef->flagPoints(nullptr, {}, {}, {}, {});
    CHECK(!fr.ok && !ef->lastError().empty(), "flagPoints without a context is refused: %s", ef->lastError().c_str());
    ef->marginalizePointsF();  // nothing flagged: nothing to do on either path
    CHECK(ef->residualReadBacks() == 0 && ef->resInM == 0, "an empty marginalizePointsF reads nothing");
    ldso_ba_flag_params fp;
    ldso_ba_default_flag_params(&fp);
    CHECK(fp.min_good_active_res_for_marg == 3 && fp.min_good_res_for_marg == 4 && fp.min_idepth_h_marg == 50.0f,
          "Setting.cc's flag parameters");
    CHECK(ldso_ba_flag_points(nullptr, 0, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr,
                              nullptr) < 0 && std::strlen(ldso_ba_last_error()) > 0, "flag_points(null)");
    CHECK(ldso_ba_load_marginalization_device(nullptr, nullptr, 0, nullptr, 0, nullptr, nullptr) < 0, "load_marginalization_device(null)");
}

int main(int argc, char **argv) {
    const bool cpu = argc > 1 && std::strcmp(argv[1], "--cpu") == 0;
    if (cpu) cpu_close_tests();
    else gpu_close_tests();
    std::printf("%s: %d failure(s)\n", cpu ? "cpu" : "gpu", g_fail);
    return g_fail ? 1 : 0;
}
