// test_face_edits.cpp -- the C++ host face with incremental edits (setIncrementalEdits(true): a
// structural change becomes one ldso_ba_edit_window, the surviving points and residuals keep their
// device state) against the same face with them off (the window is rebuilt by ldso_ba_load_frames).
//
// The scene and its two keyframes are test_face_resident.cpp's, both faces with resident frames:
// optimize(3), linearizeAll(true), frame 0 leaves with its points (marginalizePointsF,
// marginalizeFrame, dropResidual of its observations), a sixth keyframe enters from the tracker with
// a residual from every remaining point, optimize(2).  A third change follows: every seventh point is
// flagged OUTLIER and removed (dropPointsF), then optimize(1) -- an edit on top of an edit, after the
// device loop stepped the points.  Frame states, energies, inverse depths, HM and bM must be
// bit-identical between the two;
// the incremental face must have applied edits and fallen back on none.  The same comparison once
// more with LDSO_BA_TUNE_ITEM_ORDER 2 on both faces, under which the library refuses every edit: the
// incremental face falls back to the reload each time, the third time with the residuals' read-back
// still deferred, and must stay bit-identical.
//
//   test_face_edits --cpu   the switch and its counters without a device
//   test_face_edits         the GPU run
#define main face_resident_main
#include "test_face_resident.cpp"  // Synth, Scene, Trace, make_frame, record, same_bits, CHECK
#undef main

struct EditTrace : Trace {
    long applied = -1, fallen = -1;
};

// itemOrder: LDSO_BA_TUNE_ITEM_ORDER of the face's context, set before the first pass (2: the library
// refuses every edit when it plans it, before anything is launched)
static EditTrace drive_edits(const Synth &S, bool incremental, int itemOrder) {
    EditTrace T;
    const char *tag = incremental ? "incremental" : "reload";
    const int n0 = S.N - 1;
    Scene G(S, n0);
    auto ef = std::make_shared<EnergyFunctional>(0);
    CHECK(ef->ok(), "%s: %s", tag, ef->lastError().c_str());
    if (!ef->ok()) return T;
    CHECK(!ef->incrementalEdits(), "incremental edits are off by default");
    ef->setIncrementalEdits(incremental);
    CHECK(ldso_ba_set_tuning(ef->context(), LDSO_BA_TUNE_ITEM_ORDER, itemOrder) == 0, "%s item order %d: %s", tag, itemOrder,
          ldso_ba_last_error());
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
    CHECK(ef->editsApplied() == 0 && ef->editsFallenBack() == 0, "%s: the first load is no edit", tag);

    // second keyframe: frame 0 leaves, a sixth enters from the tracker
    auto f0 = ef->frames[0];
    f0->flaggedForMarginalization = true;
    for (auto &p : ef->allPoints)
        if (p->host.lock() == f0) p->status = PointStatus::MARGINALIZED;
    ef->marginalizePointsF();
    CHECK(ef->ok() && ef->resInM > 0, "%s marginalizePointsF: %s", tag, ef->lastError().c_str());
    ef->marginalizeFrame(f0);
    for (auto &p : std::vector<shared_ptr<PointHessian>>(ef->allPoints)) {
        const auto rs = p->residuals;
        for (auto &r : rs)
            if (r->target.lock() == f0) ef->dropResidual(r);
    }
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

    // third keyframe: every seventh point goes (dropPointsF), then one more iteration
    int k = 0;
    for (auto &p : ef->allPoints)
        if (k++ % 7 == 3) p->status = PointStatus::OUTLIER;
    ef->dropPointsF();
    ef->setAdjointsF(G.calib);
    ef->setDeltaF(G.calib);
    e.clear();
    ef->optimize(1, G.calib, &e, nullptr, nullptr, &all_its);
    CHECK(ef->ok() && e.size() == 2, "%s optimize(1): %s", tag, ef->lastError().c_str());
    T.energies.insert(T.energies.end(), e.begin(), e.end());
    record(*ef, T);
    T.applied = ef->editsApplied();
    T.fallen = ef->editsFallenBack();
    T.ok = ef->ok();
    ef.reset();
    if (ct) ldso_ct_destroy(ct);
    return T;
}

// both faces over the same keyframes: everything they compute is bit-identical
static bool same_results(const EditTrace &A, const EditTrace &B) {
    CHECK(A.ok && B.ok, "both faces ran");
    if (!A.ok || !B.ok) return false;
    CHECK(A.energies.size() == B.energies.size(), "energy count");
    for (size_t i = 0; i < A.energies.size() && i < B.energies.size(); i++)
        CHECK(std::memcmp(A.energies[i].data(), B.energies[i].data(), sizeof(Vec3)) == 0,
              "energy %zu: incremental (%.17g, %g) reload (%.17g, %g)", i, A.energies[i][0], A.energies[i][2], B.energies[i][0],
              B.energies[i][2]);
    CHECK(A.energies[0][2] > 100, "the passes see residuals (#IN %g)", A.energies[0][2]);
    CHECK(same_bits(A.states, B.states), "frame states bit-identical");
    CHECK(same_bits(A.idepth, B.idepth), "point inverse depths bit-identical");
    CHECK(same_bits(A.HM, B.HM), "HM bit-identical");
    CHECK(same_bits(A.bM, B.bM), "bM bit-identical");
    return true;
}

static void gpu_edit_tests() {
    Synth S(6, 300, 160, 120, 11);
    const EditTrace A = drive_edits(S, true, 0), B = drive_edits(S, false, 0);
    if (same_results(A, B)) {
        std::printf("incremental face: %ld edits applied, %ld fallen back; reload face: %ld, %ld\n", A.applied, A.fallen,
                    B.applied, B.fallen);
        CHECK(A.applied >= 2, "the incremental face edited the window (%ld)", A.applied);
        CHECK(A.fallen == 0, "no edit fell back (%ld): %s", A.fallen, ldso_ba_last_error());
        CHECK(B.applied == 0 && B.fallen == 0, "the reload face edits nothing");
    }
    // item order 2: every edit is refused and the window reloaded instead; the third change (dropPointsF
    // after optimize(2)) is refused with the read-back of the residuals still deferred
    const EditTrace C = drive_edits(S, true, 2), D = drive_edits(S, false, 2);
    if (same_results(C, D)) {
        std::printf("item order 2: incremental face: %ld edits applied, %ld fallen back; reload face: %ld, %ld\n", C.applied,
                    C.fallen, D.applied, D.fallen);
        CHECK(C.applied == 0 && C.fallen >= 2, "every edit was refused and fell back (%ld applied, %ld fallen back)", C.applied,
              C.fallen);
        CHECK(D.applied == 0 && D.fallen == 0, "the reload face edits nothing");
    }
}

static void cpu_edit_tests() {
    auto ef = std::make_shared<EnergyFunctional>(1 << 20);  // no such device
    CHECK(!ef->incrementalEdits(), "off by default");
    ef->setIncrementalEdits(true);
    CHECK(ef->incrementalEdits() && ef->editsApplied() == 0 && ef->editsFallenBack() == 0, "the switch and its counters");
    CHECK(ldso_ba_edit_window(nullptr, 0, nullptr) < 0 && std::strlen(ldso_ba_last_error()) > 0, "edit_window(null)");
}

int main(int argc, char **argv) {
    const bool cpu = argc > 1 && std::strcmp(argv[1], "--cpu") == 0;
    if (cpu) cpu_edit_tests();
    else gpu_edit_tests();
    std::printf("%s: %d failure(s)\n", cpu ? "cpu" : "gpu", g_fail);
    return g_fail ? 1 : 0;
}
