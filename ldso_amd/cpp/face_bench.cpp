// face_bench.cpp -- times the C++ host face (include/ldso_amd/energy_functional.h) the way LDSO's
// FullSystem drives it, on one synthetic S7 window (7 keyframes, 2000 points, 640x480), beside
// the C ABI's ldso_ba_optimize on the same window in the same process.  Run by bench.py
// (cpp_face); prints one JSON object.
//
//   optimize        EnergyFunctional::optimize(6) with the early exit off (th_opt_iterations = 0:
//                   all 6 iterations, so per-iteration times compare across calls and with the C
//                   ABI): FullSystem::optimize's GN loop on the device plus the face's write-back
//                   (frame states, calibration, point idepths, setDeltaF), host clock per call;
//                   iterations_default: what the reference's exits (canbreak) leave of the 6
//   shim            INTEGRATION.md §3's reference-side forwarding around one FullSystem::optimize
//                   (copy-in, optimize, copy-back, linearizeAll(true), residual / point copy-out)
//                   on stand-ins for the reference's heap objects: the copy loops alone, through
//                   std::unordered_map (as §3 wrote it in round 3) and by walking the face's own
//                   containers with the objects' `user` back-pointers (§3 now)
//   optimize_full   the same + setAdjointsF + setDeltaF + linearizeAll(true) with the complete
//                   residual / point write-back: everything FullSystem::optimize asks of the
//                   backend after the frontend's setEvalPT
//   c_abi_optimize  ldso_ba_optimize(6) on a context loaded with the same window (no face)
//   flag_loop       FullSystem::flagPointsForRemoval's per-residual resetOOB / linearize /
//                   applyRes over every residual of 10 % of the points (one device pass)
//   keyframe_cycle  one keyframe's structural round on a window of its own: insertFrame + its
//                   residuals, optimize(6), dropResidual of those residuals, marginalizeFrame; host
//                   clock per cycle (median, min, max over the repetitions), once with resident
//                   frames (the image enters the frame store once, the reload names frames by id) and
//                   once with setResidentFrames(false) (every reload gathers and uploads all images),
//                   each with its ldso_ba_transfer_stats deltas per cycle; ingest_us: one
//                   ldso_ba_frame_put_tracker of a 640x480 frame, host clock over a back-to-back run
//   keyframe_cycle_incremental  only with `ldso_face_bench REPS --incremental`: the resident cycle
//                   with setIncrementalEdits off and on (the structural round becomes one
//                   ldso_ba_edit_window), alternated A B A B in this process, each run with its own
//                   warm-up, the timed cycles of each kind pooled (median, min, max); split: where a
//                   cycle's structural uploads spend their host time (EnergyFunctional::uploadSplit and
//                   ldso_ba_edit_stats, ms per cycle); device: a further incremental run with kernel
//                   timing on, whose HIP events bracket the edit's staging launches and k_edit_gather
//   keyframe_cycle_close  only with `ldso_face_bench REPS --close`: the resident incremental cycle
//                   extended by the keyframe's close (FullSystem.cc:606-634): after optimize(6) and
//                   linearizeAll(true), removeOutliers' and flagPointsForRemoval's decision (a tenth of
//                   the points, another tenth each cycle, is put out of bounds through its
//                   lastResiduals; the threshold on idepth_hessian is their median, so half of them is
//                   MARGINALIZED and half OUT), dropResidual of the inactive residuals, dropPointsF,
//                   marginalizePointsF, marginalizeFrame, and as many new points activated as left.
//                   With the device path off the decision is taken on the objects after the residual
//                   read-back and marginalizePointsF packs its window from them; with it on
//                   (flagPoints, setDeviceMarginalization) both stay on the device.  Alternated A B A B
//                   in this process, each run with its own warm-up, the timed cycles pooled (median,
//                   min, max); split: host clock per cycle of the decision, of marginalizePointsF, of
//                   the read-backs (uploadSplit) and of the edit calls
#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstring>
#include <memory>
#include <random>
#include <string>
#include <type_traits>
#include <unordered_map>
#include <vector>

#include "../../include/ldso_amd/energy_functional.h"
#include "../../include/ldso_ct.h"
#include "../csrc/synth.h"

using namespace ldso_amd;
using Clock = std::chrono::steady_clock;

static double ms_since(Clock::time_point t0) {
    return std::chrono::duration<double, std::milli>(Clock::now() - t0).count();
}

int main(int argc, char **argv) {
    const int N = 7, P = 2000, W = 640, H = 480, n_its = 6;
    const int reps = argc > 1 ? std::atoi(argv[1]) : 10;
    const bool with_incremental = argc > 2 && std::strcmp(argv[2], "--incremental") == 0;
    const bool with_close = argc > 2 && std::strcmp(argv[2], "--close") == 0;
    const int R = P * (N - 1);
    std::vector<ldso_ba_frame_state> fs(N);
    std::vector<float> dI((size_t)N * W * H * 3), th(N), pd((size_t)P * LDSO_BA_POINT_STRIDE), re(R);
    std::vector<int32_t> ph(P), rb(P + 1), rt(R);
    std::vector<int8_t> rs(R);
    std::vector<uint8_t> rf(R);
    float calib[4];
    ldso_synth_params prm = {N, P, W, H, 1, 0.05f, 0.01f, 1e-3f, 0.04f};
    if (ldso_synth_fill(&prm, fs.data(), dI.data(), calib, th.data(), ph.data(), pd.data(), rb.data(), rt.data(),
                        rs.data(), re.data(), rf.data())) {
        std::printf("{\"error\": \"synth\"}\n");
        return 1;
    }
    // the LDSO object graph (shared_ptr ownership, as the reference)
    auto HCalib = std::make_shared<CalibHessian>();
    HCalib->wG0 = W;
    HCalib->hG0 = H;
    std::memcpy(HCalib->value_scaledf, calib, sizeof(calib));
    for (int k = 0; k < 4; k++) HCalib->value[k] = HCalib->value_zero[k] = (double)calib[k] * (1.0 / 50.0);
    std::vector<shared_ptr<FrameHessian>> frames;
    std::vector<shared_ptr<PointHessian>> points;
    for (int f = 0; f < N; f++) {
        auto F = std::make_shared<FrameHessian>();
        F->frameID = f;
        std::memcpy(F->worldToCam_evalPT, fs[f].world_to_cam_evalpt, sizeof(F->worldToCam_evalPT));
        std::memcpy(F->state, fs[f].state, sizeof(F->state));
        std::memcpy(F->state_zero, fs[f].state_zero, sizeof(F->state_zero));
        F->ab_exposure = fs[f].ab_exposure;
        F->dI = &dI[(size_t)f * W * H * 3];
        F->frameEnergyTH = th[f];
        frames.push_back(F);
    }
    auto ef = std::make_shared<EnergyFunctional>(0);
    if (!ef->ok()) {
        std::printf("{\"error\": \"%s\"}\n", ef->lastError().c_str());
        return 1;
    }
    for (auto &F : frames) ef->insertFrame(F, HCalib);
    for (int p = 0; p < P; p++) {
        auto Pt = std::make_shared<PointHessian>();
        const float *d = &pd[(size_t)p * LDSO_BA_POINT_STRIDE];
        Pt->host = frames[ph[p]];
        Pt->u = d[0];
        Pt->v = d[1];
        Pt->setIdepth(d[2]);
        Pt->setIdepthZero(d[3]);
        std::memcpy(Pt->color, d + 8, sizeof(Pt->color));
        std::memcpy(Pt->weights, d + 16, sizeof(Pt->weights));
        for (int k = rb[p]; k < rb[p + 1]; k++) {
            auto r = std::make_shared<PointFrameResidual>(Pt, frames[ph[p]], frames[rt[k]]);
            r->isNew = true;
            Pt->residuals.push_back(r);
        }
        points.push_back(Pt);
        ef->insertPoint(Pt);
        for (auto &r : Pt->residuals) ef->insertResidual(r);
    }
    ef->makeIDX();
    ef->setAdjointsF(HCalib);
    ef->setDeltaF(HCalib);

    // the reference's exits on the first call (the window as synthesised)
    int its_default = 0;
    {
        bool lost = false;
        ef->optimize(n_its, HCalib, nullptr, &lost, &its_default);
    }
    // EnergyFunctional::optimize(6), all iterations
    ldso_ba_opt_settings all_its = LDSO_BA_OPT_SETTINGS_INIT;
    all_its.th_opt_iterations = 0.0f;
    for (int i = 0; i < 2; i++) ef->optimize(n_its, HCalib, nullptr, nullptr, nullptr, &all_its);
    auto t0 = Clock::now();
    for (int i = 0; i < reps; i++) ef->optimize(n_its, HCalib, nullptr, nullptr, nullptr, &all_its);
    const double ms_opt = ms_since(t0) / reps;
    // + FullSystem::optimize's tail on the backend: setAdjointsF, setDeltaF, linearizeAll(true)
    auto full = [&] {
        ef->optimize(n_its, HCalib, nullptr, nullptr, nullptr, &all_its);
        ef->setAdjointsF(HCalib);
        ef->setDeltaF(HCalib);
        ef->linearizeAll(true);
    };
    for (int i = 0; i < 2; i++) full();
    t0 = Clock::now();
    for (int i = 0; i < reps; i++) full();
    const double ms_full = ms_since(t0) / reps;
    // flagPointsForRemoval's per-residual loop over 10 % of the points
    const long passes0 = ef->devicePasses();
    t0 = Clock::now();
    int nres = 0;
    for (size_t q = 0; q < ef->allPoints.size(); q += 10)
        for (auto &r : ef->allPoints[q]->residuals) {
            r->resetOOB();
            r->linearize(HCalib);
            r->applyRes(true);
            nres++;
        }
    const double ms_flag = ms_since(t0);
    const long flag_passes = ef->devicePasses() - passes0;

    // INTEGRATION.md §3's forwarding shim, timed: stand-ins for the reference's objects, each its
    // own heap allocation in the reference's creation order (frames, then per point the point and
    // its residuals), mapped to the face's objects either by std::unordered_map keyed by the
    // reference pointer (mf / mp / mr, as §3 writes it) or by index vectors filled in the same
    // order (the replacement)
    struct RefFrame {
        double state[10], state_zero[10], ab_exposure;
        float frameEnergyTH;
        char other[512];  // the rest of a FrameHessian
    };
    struct RefResidual;
    struct RefPoint {
        float idepth, idepth_zero, HdiF, bdSumF, idepth_hessian, step;
        float maxRelBaseline;
        int numGoodResiduals;
        std::pair<RefResidual *, int> lastResiduals[2];
        char other[128];
    };
    struct RefResidual {
        int state_state, state_NewState;
        double state_energy, state_NewEnergy, state_NewEnergyWithOutlier;
        float centerProjectedTo[3], JpJdF[8];
        bool isActiveAndIsGoodNEW;
        int mirrorIdx;  // the face's index, copied at makeIDX as hostIDX / targetIDX are
        char other[92];
    };
    std::vector<std::unique_ptr<RefFrame>> rframes;
    std::vector<std::unique_ptr<RefPoint>> rpoints;
    std::vector<std::unique_ptr<RefResidual>> rres;
    std::unordered_map<RefFrame *, FrameHessian *> mf;
    std::unordered_map<RefPoint *, PointHessian *> mp;
    std::unordered_map<RefResidual *, PointFrameResidual *> mr;
    for (auto &F : ef->frames) {
        rframes.emplace_back(new RefFrame());
        mf[rframes.back().get()] = F.get();
        F->user = rframes.back().get();
    }
    for (auto &Pt : ef->allPoints) {
        rpoints.emplace_back(new RefPoint());
        mp[rpoints.back().get()] = Pt.get();
        Pt->user = rpoints.back().get();
        for (auto &r : Pt->residuals) {
            rres.emplace_back(new RefResidual());
            mr[rres.back().get()] = r.get();
            r->user = rres.back().get();
            rres.back()->mirrorIdx = r->mirrorIdx;
        }
        // lastResiduals: the point's residuals to the two newest keyframes (FullSystem.cc:566-567)
        RefPoint &rp = *rpoints.back();
        rp.lastResiduals[0] = rp.lastResiduals[1] = {nullptr, 0};
        for (auto &r : Pt->residuals) {
            const int t = r->target.lock()->idx;
            if (t == N - 1) rp.lastResiduals[0].first = (RefResidual *)r->user;
            if (t == N - 2) rp.lastResiduals[1].first = (RefResidual *)r->user;
        }
    }
    // the replacement: walk the face's own containers (frames, allPoints, each point's residuals:
    // contiguous, in the device's order) and reach the reference object through `user`
    struct FaceFrames {
        EnergyFunctional &e;
        struct It {
            std::vector<shared_ptr<FrameHessian>>::iterator i;
            std::pair<RefFrame *, FrameHessian *> operator*() const { return {(RefFrame *)(*i)->user, i->get()}; }
            It &operator++() { ++i; return *this; }
            bool operator!=(const It &o) const { return i != o.i; }
        };
        It begin() { return {e.frames.begin()}; }
        It end() { return {e.frames.end()}; }
    } vf{*ef};
    struct FacePoints {
        EnergyFunctional &e;
        struct It {
            std::vector<shared_ptr<PointHessian>>::iterator i;
            std::pair<RefPoint *, PointHessian *> operator*() const { return {(RefPoint *)(*i)->user, i->get()}; }
            It &operator++() { ++i; return *this; }
            bool operator!=(const It &o) const { return i != o.i; }
        };
        It begin() { return {e.allPoints.begin()}; }
        It end() { return {e.allPoints.end()}; }
    } vp{*ef};
    std::vector<std::pair<RefResidual *, PointFrameResidual *>> vr;  // rebuilt at makeIDX in a real shim
    for (auto &Pt : ef->allPoints)
        for (auto &r : Pt->residuals) vr.emplace_back((RefResidual *)r->user, r.get());
    // the copy loops of one FullSystem::optimize through the shim (§3: "replaces
    // FullSystem.cc:853-970" and FullSystem::linearizeAll), without the face calls themselves
    auto shim_loops = [&](auto &F, auto &Pm, auto &Rm) {
        for (auto kv : F) std::memcpy(kv.second->state, kv.first->state, sizeof(kv.first->state));  // copyIn
        for (auto kv : Pm) {
            kv.second->setIdepth(kv.first->idepth);
            kv.second->setIdepthZero(kv.first->idepth_zero);
        }
        // ... gpu->optimize(...) ...
        for (auto kv : F) std::memcpy(kv.first->state, kv.second->state, sizeof(kv.first->state));
        for (auto kv : Pm) {
            kv.first->idepth = kv.second->idepth;
            kv.first->idepth_zero = kv.second->idepth_zero;
        }
        // FullSystem::linearizeAll(true): copy-in, gpu->linearizeAll, copy-out
        for (auto kv : F) std::memcpy(kv.second->state, kv.first->state, sizeof(kv.first->state));
        for (auto kv : Pm) kv.second->setIdepth(kv.first->idepth);
        auto copy_out = [](RefResidual &r, const PointFrameResidual &g) {
            r.state_state = (int)g.state_state;
            r.state_NewState = (int)g.state_NewState;
            r.state_energy = g.state_energy;
            r.state_NewEnergy = g.state_NewEnergy;
            r.state_NewEnergyWithOutlier = g.state_NewEnergyWithOutlier;
            std::memcpy(r.centerProjectedTo, g.centerProjectedTo, sizeof(r.centerProjectedTo));
            r.isActiveAndIsGoodNEW = g.isActiveAndIsGoodNEW;
            std::memcpy(r.JpJdF, g.JpJdF, sizeof(r.JpJdF));
        };
        if constexpr (std::is_same_v<std::decay_t<decltype(Rm)>, std::vector<std::pair<RefResidual *, PointFrameResidual *>>>) {
            // the objects are scattered on the heap: prefetch a few residuals ahead
            const size_t n = Rm.size();
            for (size_t k = 0; k < n; k++) {
                if (k + 8 < n) {
                    __builtin_prefetch(Rm[k + 8].first, 1);
                    __builtin_prefetch(Rm[k + 8].second, 0);
                }
                copy_out(*Rm[k].first, *Rm[k].second);
            }
        } else {
            for (auto kv : Rm) copy_out(*kv.first, *kv.second);
        }
        for (auto kv : Pm) {
            kv.first->HdiF = kv.second->HdiF;
            kv.first->bdSumF = kv.second->bdSumF;
            kv.first->idepth_hessian = kv.second->idepth_hessian;
        }
    };
    // the round-5 protocol: copy back only what the reference's consumers read.
    // After optimize: the frames' states and the points' idepths.  After linearizeAll(true): the
    // points' HdiF / idepth_hessian (CoarseTracker, flagPointsForRemoval), maxRelBaseline /
    // numGoodResiduals and lastResiduals' states from the face's per-point FixPassResult (allPoints
    // order: no residual object is touched), and the toRemove list for dropResidual.  centerProjectedTo stays with the face: its one
    // consumer per keyframe (CoarseTracker::makeCoarseDepthL0) reads gpu->residualCenter(mirrorIdx).
    std::vector<RefResidual *> toRemove;
    auto shim_digest = [&]() {
        for (auto &F : ef->frames)
            std::memcpy(((RefFrame *)F->user)->state, F->state, sizeof(F->state));
        // the face's own containers in order; FixPassResult is indexed like allPoints
        const auto &fx = ef->fixPassResult();
        const size_t P = ef->allPoints.size();
        for (size_t q = 0; q < P; q++) {
            if (q + 8 < P) __builtin_prefetch(ef->allPoints[q + 8]->user, 1);
            const PointHessian &g = *ef->allPoints[q];
            RefPoint &p = *(RefPoint *)g.user;
            p.idepth = g.idepth;
            p.idepth_zero = g.idepth_zero;
            p.HdiF = g.HdiF;
            p.idepth_hessian = g.idepth_hessian;
            if (fx.numGood.size() == P) {
                p.maxRelBaseline = std::max(p.maxRelBaseline, fx.maxRelBS[q]);
                p.numGoodResiduals += fx.numGood[q];
            }
            if (fx.lastState.size() == 2 * P)
                for (int i = 0; i < 2; i++)
                    if (p.lastResiduals[i].first) p.lastResiduals[i].second = fx.lastState[2 * q + i];
        }
        toRemove.clear();
        for (PointFrameResidual *g : fx.toRemove) toRemove.push_back((RefResidual *)g->user);
    };
    auto time_shim = [&](auto &&loops) {
        // between calls the frontend touches other memory (tracking, images): evict the caches
        std::vector<char> evict((size_t)64 << 20, 1);
        double tot = 0;
        for (int i = 0; i < reps; i++) {
            for (size_t k = 0; k < evict.size(); k += 64) evict[k]++;
            auto t1 = Clock::now();
            loops();
            tot += ms_since(t1);
        }
        return tot / reps;
    };
    // the face state after FullSystem::optimize: optimize, then linearizeAll(true) (its FixPassResult)
    ef->optimize(n_its, HCalib, nullptr, nullptr, nullptr, &all_its);
    ef->linearizeAll(true);
    (void)ef->residualState(0);  // states of the pass downloaded once (as the first consumer would)
    const double ms_shim_digest = time_shim(shim_digest);
    ef->syncResiduals();  // the round-4 per-field loops read every residual object
    const double ms_shim_map = time_shim([&] { shim_loops(mf, mp, mr); });
    const double ms_shim_vec = time_shim([&] { shim_loops(vf, vp, vr); });
    const bool ok = ef->ok();

    // the C ABI alone on a context of the same window
    std::vector<float> precalc((size_t)N * N * LDSO_BA_PRECALC_STRIDE);
    std::vector<double> adH((size_t)N * N * 64), adT((size_t)N * N * 64), cp(4), fp(8 * N), fd(8 * N), fdp(8 * N);
    ldso_ba_frame_precalc(N, fs.data(), calib, precalc.data());
    ldso_ba_set_adjoints(N, fs.data(), adH.data(), adT.data(), cp.data());
    ldso_ba_frame_take_data(N, fs.data(), nullptr, fp.data(), fd.data(), fdp.data());
    const float cdelta[4] = {0, 0, 0, 0};
    ldso_ba_window w;
    std::memset(&w, 0, sizeof(w));
    w.n_frames = N;
    w.n_points = P;
    w.n_residuals = R;
    w.width = W;
    w.height = H;
    std::memcpy(w.calib, calib, sizeof(calib));
    w.dI = dI.data();
    w.frame_energy_th = th.data();
    w.precalc = precalc.data();
    w.ad_host = adH.data();
    w.ad_target = adT.data();
    w.c_prior = cp.data();
    w.c_delta = cdelta;
    w.frame_prior = fp.data();
    w.frame_delta_prior = fdp.data();
    w.point_host = ph.data();
    w.point_data = pd.data();
    w.point_res_begin = rb.data();
    w.res_target = rt.data();
    w.res_state = rs.data();
    w.res_energy = re.data();
    w.res_flags = rf.data();
    ldso_ba_ctx *raw = nullptr;
    double ms_raw = -1;
    if (ldso_ba_create(0, &raw) == 0 && ldso_ba_load(raw, 1, &w, 0, 1) == 0) {
        const int n = 8 * N + 4;
        std::vector<double> ns((size_t)7 * n), e((size_t)3 * (n_its + 1)), cv(4), co(4);
        std::vector<ldso_ba_frame_state> fo(N);
        std::vector<float> id(P);
        for (int k = 0; k < 4; k++) cv[k] = HCalib->value_zero[k];
        ldso_ba_nullspaces(N, fs.data(), ns.data());
        for (int i = 0; i < 2; i++)
            ldso_ba_optimize(raw, n_its, &all_its, fs.data(), cv.data(), cv.data(), ns.data(), e.data(), fo.data(),
                             co.data(), id.data(), nullptr, nullptr);
        t0 = Clock::now();
        for (int i = 0; i < reps; i++)
            ldso_ba_optimize(raw, n_its, &all_its, fs.data(), cv.data(), cv.data(), ns.data(), e.data(), fo.data(),
                             co.data(), id.data(), nullptr, nullptr);
        ms_raw = ms_since(t0) / reps;
        ldso_ba_destroy(raw);
    }
    // keyframe_cycle: frames 0..5 and their points stay; frame 6 enters and leaves once per cycle
    struct CycleResult {
        double med = -1, lo = -1, hi = -1;
        double xfer[4] = {0, 0, 0, 0};
        bool ok = false;
        std::vector<double> ms;  // every timed cycle
        long edits = 0, fallen = 0;
        int cycles = 0;
        double split[6] = {0, 0, 0, 0, 0, 0};  // EnergyFunctional::uploadSplit over the timed cycles
        double lib[6] = {0, 0, 0, 0, 0, 0};    // ldso_ba_edit_stats over the timed cycles
    };
    // events: kernel timing on with an empty slot mask, so that only the edit's three events are
    // recorded (timing also makes ldso_ba_optimize launch directly: such a run's cycle time is not reported)
    auto keyframe_cycle = [&](bool resident, bool incremental = false, bool events = false) {
        CycleResult out;
        auto e2 = std::make_shared<EnergyFunctional>(0);
        if (!e2->ok()) return out;
        e2->setResidentFrames(resident);
        e2->setIncrementalEdits(incremental);
        if (events) {
            ldso_ba_set_tuning(e2->context(), LDSO_BA_TUNE_TIMING_MASK, 0);
            ldso_ba_set_kernel_timing(e2->context(), 1);
        }
        double split0[6] = {0, 0, 0, 0, 0, 0}, lib0[6] = {0, 0, 0, 0, 0, 0};
        auto make_frame = [&](int f, int id) {
            auto F = std::make_shared<FrameHessian>();
            F->frameID = id;
            std::memcpy(F->worldToCam_evalPT, fs[f].world_to_cam_evalpt, sizeof(F->worldToCam_evalPT));
            std::memcpy(F->state, fs[f].state, sizeof(F->state));
            std::memcpy(F->state_zero, fs[f].state_zero, sizeof(F->state_zero));
            F->ab_exposure = fs[f].ab_exposure;
            F->dI = &dI[(size_t)f * W * H * 3];
            F->frameEnergyTH = th[f];
            return F;
        };
        std::vector<shared_ptr<FrameHessian>> fr;
        for (int f = 0; f < N - 1; f++) {
            fr.push_back(make_frame(f, f));
            e2->insertFrame(fr.back(), HCalib);
        }
        std::vector<shared_ptr<PointHessian>> pts;
        for (int p = 0; p < P; p++) {
            if (ph[p] == N - 1) continue;
            auto Pt = std::make_shared<PointHessian>();
            const float *d = &pd[(size_t)p * LDSO_BA_POINT_STRIDE];
            Pt->host = fr[ph[p]];
            Pt->u = d[0];
            Pt->v = d[1];
            Pt->setIdepth(d[2]);
            Pt->setIdepthZero(d[3]);
            std::memcpy(Pt->color, d + 8, sizeof(Pt->color));
            std::memcpy(Pt->weights, d + 16, sizeof(Pt->weights));
            for (int k = rb[p]; k < rb[p + 1]; k++) {
                if (rt[k] == N - 1) continue;
                auto r = std::make_shared<PointFrameResidual>(Pt, fr[ph[p]], fr[rt[k]]);
                r->isNew = true;
                Pt->residuals.push_back(r);
            }
            pts.push_back(Pt);
            e2->insertPoint(Pt);
            for (auto &r : Pt->residuals) e2->insertResidual(r);
        }
        const int warm = 2;
        std::vector<double> ms;
        int64_t x0[4] = {0, 0, 0, 0}, x1[4] = {0, 0, 0, 0};
        for (int c = 0; c < warm + reps && e2->ok(); c++) {
            if (c == warm) {
                ldso_ba_transfer_stats(e2->context(), x0);
                std::memcpy(split0, e2->uploadSplit(), sizeof(split0));
                ldso_ba_edit_stats(e2->context(), lib0);
            }
            auto F = make_frame(N - 1, 100 + c);
            std::vector<shared_ptr<PointFrameResidual>> added;
            auto t1 = Clock::now();
            e2->insertFrame(F, HCalib);
            for (auto &Pt : pts) {
                auto r = std::make_shared<PointFrameResidual>(Pt, Pt->host.lock(), F);
                r->isNew = true;
                Pt->residuals.push_back(r);
                e2->insertResidual(r);
                added.push_back(r);
            }
            e2->makeIDX();
            e2->setAdjointsF(HCalib);
            e2->setDeltaF(HCalib);
            e2->optimize(n_its, HCalib, nullptr, nullptr, nullptr, &all_its);
            for (auto &r : added) e2->dropResidual(r);
            e2->marginalizeFrame(F);
            if (c >= warm) ms.push_back(ms_since(t1));
        }
        ldso_ba_transfer_stats(e2->context(), x1);
        if (!e2->ok() || ms.empty()) {
            std::fprintf(stderr, "keyframe_cycle: %s\n", e2->lastError().c_str());
            return out;
        }
        out.ms = ms;
        out.cycles = (int)ms.size();
        ldso_ba_edit_stats(e2->context(), out.lib);
        for (int i = 0; i < 6; i++) {
            out.split[i] = e2->uploadSplit()[i] - split0[i];
            out.lib[i] -= lib0[i];
        }
        out.edits = e2->editsApplied();
        out.fallen = e2->editsFallenBack();
        std::sort(ms.begin(), ms.end());
        out.med = ms[ms.size() / 2];
        out.lo = ms.front();
        out.hi = ms.back();
        for (int i = 0; i < 4; i++) out.xfer[i] = (double)(x1[i] - x0[i]) / (double)ms.size();
        out.ok = true;
        return out;
    };
    const CycleResult kc_res = keyframe_cycle(true), kc_leg = keyframe_cycle(false);
    // --incremental: the resident cycle with and without incremental edits (setIncrementalEdits), the
    // two alternated in this process (A B A B, each with its own warm-up), their cycles pooled
    std::string kc_inc_json;
    if (with_incremental) {
        auto pool = [](CycleResult a, const CycleResult &b) {
            a.ok = a.ok && b.ok;
            a.ms.insert(a.ms.end(), b.ms.begin(), b.ms.end());
            if (a.ok) {
                std::sort(a.ms.begin(), a.ms.end());
                a.med = a.ms[a.ms.size() / 2];
                a.lo = a.ms.front();
                a.hi = a.ms.back();
            }
            for (int i = 0; i < 4; i++) a.xfer[i] = 0.5 * (a.xfer[i] + b.xfer[i]);
            a.edits += b.edits;
            a.fallen += b.fallen;
            a.cycles += b.cycles;
            for (int i = 0; i < 6; i++) {
                a.split[i] += b.split[i];
                a.lib[i] += b.lib[i];
            }
            return a;
        };
        const CycleResult r1 = keyframe_cycle(true), i1 = keyframe_cycle(true, true), r2 = keyframe_cycle(true),
                          i2 = keyframe_cycle(true, true);
        const CycleResult r = pool(r1, r2), in = pool(i1, i2);
        const CycleResult ev = keyframe_cycle(true, true, true);
        // per cycle, ms: the face's structural uploads (host clock) and, inside ldso_ba_edit_window, the
        // planner and the rest of the call (host clock); per edit, ms: the device time of the staging
        // launches and of k_edit_gather (HIP events, from the run with events)
        auto split_json = [](const CycleResult &c) {
            char b[640];
            const double n = c.cycles > 0 ? c.cycles : 1;
            std::snprintf(b, sizeof(b),
                          "{\"structural_uploads\": %.2f, \"read_back_ms\": %.4f, \"graph_walk_and_mirror_ms\": %.4f, "
                          "\"frame_terms_ms\": %.4f, \"edit_or_reload_call_ms\": %.4f, \"follow_up_updates_ms\": %.4f, "
                          "\"edit_planner_ms\": %.4f, \"edit_rest_of_call_ms\": %.4f}",
                          c.split[0] / n, c.split[1] / n, c.split[2] / n, c.split[3] / n, c.split[4] / n, c.split[5] / n,
                          c.lib[1] / n, c.lib[2] / n);
            return std::string(b);
        };
        const double ne = ev.lib[0] > 0 ? ev.lib[0] : 1;
        char buf[4096];
        std::snprintf(buf, sizeof(buf),
                      ", \"keyframe_cycle_incremental\": {\"what\": \"the resident keyframe_cycle with setIncrementalEdits off / on, "
                      "alternated in one process, 2 x %d cycles each; split: host clock per cycle; device: HIP events per edit, "
                      "from a further incremental run with kernel timing on\", \"resident\": {\"ok\": %s, \"ms_median\": %.6f, "
                      "\"ms_min\": %.6f, \"ms_max\": %.6f, \"split\": %s}, \"incremental\": {\"ok\": %s, \"ms_median\": %.6f, "
                      "\"ms_min\": %.6f, \"ms_max\": %.6f, \"edits_applied\": %ld, \"edits_fallen_back\": %ld, "
                      "\"h2d_image_bytes_per_cycle\": %.1f, \"allocs_per_cycle\": %.3f, \"split\": %s}, "
                      "\"device\": {\"ok\": %s, \"edits\": %.0f, \"staging_launches_ms_per_edit\": %.5f, "
                      "\"k_edit_gather_ms_per_edit\": %.5f}}",
                      reps, r.ok ? "true" : "false", r.med, r.lo, r.hi, split_json(r).c_str(), in.ok ? "true" : "false", in.med,
                      in.lo, in.hi, in.edits, in.fallen, in.xfer[0], in.xfer[2], split_json(in).c_str(), ev.ok ? "true" : "false",
                      ev.lib[0], ev.lib[4] / ne, ev.lib[5] / ne);
        kc_inc_json = buf;
    }
    // --close: the resident incremental cycle with the keyframe's close, device path off and on
    std::string kc_close_json;
    if (with_close) {
        struct CloseResult {
            bool ok = false;
            std::vector<double> ms;
            double flag_ms = 0, marg_ms = 0, split[6] = {0, 0, 0, 0, 0, 0};
            long read_backs = 0, device_margs = 0, edits = 0, fallen = 0;
            long left[4] = {0, 0, 0, 0};  // points per status over the timed cycles
            int cycles = 0;
        };
        // every run starts from the same calibration (optimize steps it), so that the two paths see the
        // same windows and their point counts can be compared
        const CalibHessian calib0 = *HCalib;
        auto close_cycle = [&](bool device) {
            CloseResult out;
            auto HC = std::make_shared<CalibHessian>(calib0);
            auto e2 = std::make_shared<EnergyFunctional>(0);
            if (!e2->ok()) return out;
            e2->setIncrementalEdits(true);
            e2->setDeviceMarginalization(device);
            auto new_frame = [&](int f, int id) {
                auto F = std::make_shared<FrameHessian>();
                F->frameID = id;
                std::memcpy(F->worldToCam_evalPT, fs[f].world_to_cam_evalpt, sizeof(F->worldToCam_evalPT));
                std::memcpy(F->state, fs[f].state, sizeof(F->state));
                std::memcpy(F->state_zero, fs[f].state_zero, sizeof(F->state_zero));
                F->ab_exposure = fs[f].ab_exposure;
                F->dI = &dI[(size_t)f * W * H * 3];
                F->frameEnergyTH = th[f];
                return F;
            };
            std::vector<shared_ptr<FrameHessian>> fr;
            for (int f = 0; f < N - 1; f++) {
                fr.push_back(new_frame(f, f));
                e2->insertFrame(fr.back(), HC);
            }
            // a point of the synthetic window enters (at the start, and again after it left): `user`
            // keeps its index there
            std::vector<intptr_t> src_of;
            auto activate = [&](int p) {
                auto Pt = std::make_shared<PointHessian>();
                const float *d = &pd[(size_t)p * LDSO_BA_POINT_STRIDE];
                Pt->host = fr[ph[p]];
                Pt->u = d[0];
                Pt->v = d[1];
                Pt->setIdepth(d[2]);
                Pt->setIdepthZero(d[3]);
                std::memcpy(Pt->color, d + 8, sizeof(Pt->color));
                std::memcpy(Pt->weights, d + 16, sizeof(Pt->weights));
                Pt->user = reinterpret_cast<void *>((intptr_t)p);
                for (int k = rb[p]; k < rb[p + 1]; k++) {
                    if (rt[k] == N - 1) continue;
                    auto r = std::make_shared<PointFrameResidual>(Pt, fr[ph[p]], fr[rt[k]]);
                    r->isNew = true;
                    Pt->residuals.push_back(r);
                }
                e2->insertPoint(Pt);
                for (auto &r : Pt->residuals) e2->insertResidual(r);
            };
            for (int p = 0; p < P; p++)
                if (ph[p] != N - 1) activate(p);
            e2->makeIDX();
            ldso_ba_flag_params fpar;
            ldso_ba_default_flag_params(&fpar);
            const int warm = 2;
            double split0[6] = {0, 0, 0, 0, 0, 0};
            long rb0 = 0;
            for (int c = 0; c < warm + reps && e2->ok(); c++) {
                if (c == warm) {
                    std::memcpy(split0, e2->uploadSplit(), sizeof(split0));
                    rb0 = e2->residualReadBacks();
                }
                auto F = new_frame(N - 1, 100 + c);
                auto t1 = Clock::now();
                e2->insertFrame(F, HC);
                for (auto &Pt : std::vector<shared_ptr<PointHessian>>(e2->allPoints)) {
                    auto r = std::make_shared<PointFrameResidual>(Pt, Pt->host.lock(), F);
                    r->isNew = true;
                    Pt->residuals.push_back(r);
                    e2->insertResidual(r);
                }
                e2->makeIDX();
                e2->setAdjointsF(HC);
                e2->setDeltaF(HC);
                e2->optimize(n_its, HC, nullptr, nullptr, nullptr, &all_its);
                e2->setAdjointsF(HC);
                e2->setDeltaF(HC);
                e2->linearizeAll(true);
                // the frontend's bookkeeping, allPoints order (untimed share: the same on both paths)
                const std::vector<shared_ptr<PointHessian>> pts = e2->allPoints;
                const int Pn = (int)pts.size(), Nn = e2->nFrames;
                std::vector<int32_t> numGood(Pn, 10), lastRes(2 * (size_t)Pn, -1);
                std::vector<int8_t> lastState(2 * (size_t)Pn, (int8_t)IN);
                std::vector<PointFrameResidual *> lastPtr(2 * (size_t)Pn, nullptr);
                std::vector<float> ih;
                for (int q = 0; q < Pn; q++) {
                    if ((q + c) % 10 == 0) {  // its lastResiduals[0] left the window OOB
                        lastState[2 * (size_t)q] = (int8_t)OOB;
                        ih.push_back(pts[q]->idepth_hessian);
                        continue;
                    }
                    for (auto &r : pts[q]->residuals) {
                        const int t = r->target.lock()->idx;
                        if (t >= Nn - 2) {
                            lastPtr[2 * (size_t)q + (Nn - 1 - t)] = r.get();
                            lastRes[2 * (size_t)q + (Nn - 1 - t)] = r->mirrorIdx;
                        }
                    }
                }
                std::sort(ih.begin(), ih.end());
                fpar.min_idepth_h_marg = ih.empty() ? 50.0f : ih[ih.size() / 2];
                auto t2 = Clock::now();
                std::vector<PointFrameResidual *> toRemove;
                long left[4] = {0, 0, 0, 0};
                if (device) {
                    const EnergyFunctional::FlagResult fx = e2->flagPoints(&fpar, {}, numGood, lastRes, lastState);
                    if (!fx.ok) break;
                    toRemove = fx.toRemove;
                    for (int i = 0; i < 4; i++) left[i] = fx.counts[i];
                } else {
                    e2->syncResiduals();
                    const int A = fpar.min_good_active_res_for_marg, G = fpar.min_good_res_for_marg;
                    for (int q = 0; q < Pn; q++) {
                        PointHessian &pt = *pts[q];
                        int n_live = 0, vis = 0;
                        for (auto &r : pt.residuals) {
                            if (!r->isActive()) {
                                toRemove.push_back(r.get());
                                continue;
                            }
                            n_live++;
                            if (r->state_state == IN && r->target.lock()->flaggedForMarginalization) vis++;
                        }
                        int8_t ls[2];
                        for (int i = 0; i < 2; i++)
                            ls[i] = lastPtr[2 * (size_t)q + i] ? (int8_t)lastPtr[2 * (size_t)q + i]->state_state : lastState[2 * (size_t)q + i];
                        const int ng = numGood[q] + n_live;
                        int st = LDSO_BA_PT_ACTIVE;
                        if (pt.idepth_scaled < 0 || n_live == 0) {
                            st = LDSO_BA_PT_OUTLIER;
                        } else {
                            const bool oob = (n_live >= A && ng > G + 10 && n_live - vis < A) || ls[0] == OOB ||
                                             (n_live >= 2 && ls[0] == OUTLIER && ls[1] == OUTLIER);
                            if (oob || pt.host.lock()->flaggedForMarginalization)
                                st = n_live >= A && ng >= G && pt.idepth_hessian > fpar.min_idepth_h_marg ? LDSO_BA_PT_MARGINALIZED
                                                                                                         : LDSO_BA_PT_OUT;
                        }
                        pt.status = (PointStatus)st;
                        left[st]++;
                    }
                }
                const double flag_ms = ms_since(t2);
                for (PointFrameResidual *r : toRemove) {
                    auto pt = r->point.lock();
                    for (auto &x : pt->residuals)
                        if (x.get() == r) {
                            e2->dropResidual(x);
                            break;
                        }
                }
                std::vector<int> back;
                for (auto &pt : pts)
                    if (pt->status != PointStatus::ACTIVE) back.push_back((int)reinterpret_cast<intptr_t>(pt->user));
                e2->dropPointsF();
                auto t3 = Clock::now();
                e2->marginalizePointsF();
                const double marg_ms = ms_since(t3);
                for (auto &pt : std::vector<shared_ptr<PointHessian>>(e2->allPoints)) {
                    const auto rs = pt->residuals;
                    for (auto &r : rs)
                        if (r->target.lock() == F) e2->dropResidual(r);
                }
                e2->marginalizeFrame(F);
                for (int p : back) activate(p);
                e2->makeIDX();
                if (c >= warm) {
                    out.ms.push_back(ms_since(t1));
                    out.flag_ms += flag_ms;
                    out.marg_ms += marg_ms;
                    for (int i = 0; i < 4; i++) out.left[i] += left[i];
                }
            }
            if (!e2->ok() || out.ms.empty()) {
                std::fprintf(stderr, "keyframe_cycle_close: %s\n", e2->lastError().c_str());
                return out;
            }
            out.cycles = (int)out.ms.size();
            for (int i = 0; i < 6; i++) out.split[i] = e2->uploadSplit()[i] - split0[i];
            out.read_backs = e2->residualReadBacks() - rb0;
            out.device_margs = e2->deviceMarginalizations();
            out.edits = e2->editsApplied();
            out.fallen = e2->editsFallenBack();
            out.ok = true;
            return out;
        };
        auto pool = [](CloseResult a, const CloseResult &b) {
            a.ok = a.ok && b.ok;
            a.ms.insert(a.ms.end(), b.ms.begin(), b.ms.end());
            a.flag_ms += b.flag_ms;
            a.marg_ms += b.marg_ms;
            a.read_backs += b.read_backs;
            a.device_margs += b.device_margs;
            a.edits += b.edits;
            a.fallen += b.fallen;
            a.cycles += b.cycles;
            for (int i = 0; i < 6; i++) a.split[i] += b.split[i];
            for (int i = 0; i < 4; i++) a.left[i] += b.left[i];
            return a;
        };
        const CloseResult h1 = close_cycle(false), d1 = close_cycle(true), h2 = close_cycle(false), d2 = close_cycle(true);
        auto close_json = [](CloseResult c) {
            char b[1024];
            const double n = c.cycles > 0 ? c.cycles : 1;
            double med = -1, lo = -1, hi = -1;
            if (c.ok && !c.ms.empty()) {
                std::sort(c.ms.begin(), c.ms.end());
                med = c.ms[c.ms.size() / 2];
                lo = c.ms.front();
                hi = c.ms.back();
            }
            std::snprintf(b, sizeof(b),
                          "{\"ok\": %s, \"ms_median\": %.6f, \"ms_min\": %.6f, \"ms_max\": %.6f, \"cycles\": %d, "
                          "\"residual_read_backs_per_cycle\": %.3f, \"device_marginalizations\": %ld, \"edits_applied\": %ld, "
                          "\"edits_fallen_back\": %ld, \"points_per_cycle\": {\"active\": %.1f, \"outlier\": %.1f, \"out\": %.1f, "
                          "\"marginalized\": %.1f}, \"split\": {\"decision_ms\": %.4f, \"marginalize_points_ms\": %.4f, "
                          "\"read_back_ms\": %.4f, \"structural_uploads\": %.2f, \"edit_or_reload_call_ms\": %.4f}}",
                          c.ok ? "true" : "false", med, lo, hi, c.cycles, c.read_backs / n, c.device_margs, c.edits, c.fallen,
                          c.left[0] / n, c.left[1] / n, c.left[2] / n, c.left[3] / n, c.flag_ms / n, c.marg_ms / n, c.split[1] / n,
                          c.split[0] / n, c.split[4] / n);
            return std::string(b);
        };
        kc_close_json = ", \"keyframe_cycle_close\": {\"what\": \"the resident incremental keyframe_cycle with linearizeAll(true) and "
                        "the keyframe's close (decision, dropResidual, dropPointsF, marginalizePointsF, marginalizeFrame, "
                        "re-activation), device path off / on, alternated in one process, 2 x " + std::to_string(reps) +
                        " cycles each; host clock; the decision's time includes the host path's residual read-back\", "
                        "\"host\": " + close_json(pool(h1, h2)) + ", \"device\": " + close_json(pool(d1, d2)) + "}";
    }
    // one device-to-device ingest of the tracker's new frame (event record / wait, the layout-3
    // kernel): back to back on the host clock, one synchronisation at the end
    double ingest_us = -1;
    {
        ldso_ct_ctx *ct = nullptr;
        ldso_ba_ctx *bc = nullptr;
        int32_t nl = 0;
        std::vector<float> color((size_t)W * H);
        for (size_t i = 0; i < color.size(); i++) color[i] = dI[3 * i];
        if (ldso_ct_create(0, W, H, &ct, &nl) == 0 && ldso_ba_create(0, &bc) == 0 &&
            ldso_ba_frames_reserve(bc, 2, W, H) == 0 && ldso_ct_set_new_frame(ct, color.data(), 1.0, nullptr) == 0) {
            const int n_put = 200;
            bool good = true;
            for (int i = 0; i < 10; i++) good = good && ldso_ba_frame_put_tracker(bc, 1, ct) == 0;
            ldso_ba_sync(bc);
            auto t1 = Clock::now();
            for (int i = 0; i < n_put; i++) good = good && ldso_ba_frame_put_tracker(bc, 1, ct) == 0;
            ldso_ba_sync(bc);
            if (good) ingest_us = 1000.0 * ms_since(t1) / n_put;
        }
        if (bc) ldso_ba_destroy(bc);
        if (ct) ldso_ct_destroy(ct);
    }
    auto cycle_json = [](const CycleResult &r) {
        char buf[512];
        std::snprintf(buf, sizeof(buf),
                      "{\"ok\": %s, \"ms_median\": %.6f, \"ms_min\": %.6f, \"ms_max\": %.6f, "
                      "\"h2d_image_bytes_per_cycle\": %.1f, \"d2d_image_bytes_per_cycle\": %.1f, "
                      "\"image_allocs_per_cycle\": %.3f, \"frames_ingested_per_cycle\": %.3f}",
                      r.ok ? "true" : "false", r.med, r.lo, r.hi, r.xfer[0], r.xfer[1], r.xfer[2], r.xfer[3]);
        return std::string(buf);
    };
    const std::string kc_json = "{\"what\": \"S7: insertFrame + residuals, optimize(6), dropResidual, marginalizeFrame; host clock\", "
                                "\"resident\": " + cycle_json(kc_res) + ", \"legacy\": " + cycle_json(kc_leg) +
                                ", \"ingest_us\": " + std::to_string(ingest_us) + "}";
    std::printf(
        "{\"window\": \"S7 (7 KF, 2000 pts, 640x480, seed 1)\", \"n_its\": %d, \"reps\": %d, \"ok\": %s, "
        "\"optimize\": {\"ms_per_optimize\": %.6f, \"ms_per_gn_iteration\": %.6f, \"iterations\": %d, "
        "\"iterations_default\": %d}, "
        "\"shim\": {\"what\": \"INTEGRATION.md 3 reference-side copy loops of one FullSystem::optimize, %d residuals, "
        "%d points, caches evicted between calls: the consumers' fields only (FixPassResult incl. lastResiduals' "
        "states by point; digest_ms, the protocol of 3) vs every residual field through back-pointers / "
        "unordered_map (round 4)\", \"digest_ms\": %.6f, \"per_field_back_pointer_ms\": %.6f, "
        "\"unordered_map_ms\": %.6f, \"shim_ms_per_gn_iteration\": %.6f, "
        "\"frac_of_face_gn_iteration\": %.4f, \"per_field_frac_of_face_gn_iteration\": %.4f, "
        "\"to_remove\": %zu}, "
        "\"optimize_full\": {\"ms\": %.6f, \"what\": \"optimize(6) + setAdjointsF + setDeltaF + linearizeAll(true) "
        "with the residual / point write-back\"}, "
        "\"c_abi_optimize\": {\"ms_per_optimize\": %.6f, \"ms_per_gn_iteration\": %.6f}, "
        "\"flag_loop\": {\"residuals\": %d, \"ms\": %.6f, \"device_passes\": %ld}, "
        "\"keyframe_cycle\": %s%s%s}\n",
        n_its, reps, ok ? "true" : "false", ms_opt, ms_opt / n_its, n_its, its_default, (int)vr.size(), (int)ef->allPoints.size(),
        ms_shim_digest, ms_shim_vec, ms_shim_map, ms_shim_digest / n_its, ms_shim_digest / ms_opt, ms_shim_vec / ms_opt,
        toRemove.size(),
        ms_full, ms_raw, ms_raw / n_its, nres, ms_flag, flag_passes, kc_json.c_str(), kc_inc_json.c_str(), kc_close_json.c_str());
    return ok ? 0 : 1;
}
