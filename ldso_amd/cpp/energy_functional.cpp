// energy_functional.cpp -- the C++ host face (include/ldso_amd/energy_functional.h) on the C ABI
// of include/ldso_ba.h.  Packing and bookkeeping only: every number is computed by the HIP path
// or by the library's host helpers (precalc, adjoints, priors, deltas, energies, nullspaces,
// solve, frame marginalisation).
#include "../../include/ldso_amd/energy_functional.h"
#include "../../include/ldso_ct.h"

#include <algorithm>
#include <chrono>
#include <cstring>
#include <utility>

namespace ldso_amd {

namespace {

constexpr float kIdepthFixPriorMargFac = 600.0f * 600.0f;  // setting_idepthFixPriorMargFac (Setting.cc:17)
constexpr double kMargWeightFac = 0.5 * 0.5;                // setting_margWeightFac (Setting.cc:45)

uint64_t conn_key(const PointFrameResidual &r) {
    return ((uint64_t)r.host.lock()->frameID << 32) + (uint64_t)r.target.lock()->frameID;
}

void frame_state(const FrameHessian &F, ldso_ba_frame_state &S) {
    std::memset(&S, 0, sizeof(S));
    std::memcpy(S.world_to_cam_evalpt, F.worldToCam_evalPT, sizeof(S.world_to_cam_evalpt));
    std::memcpy(S.state, F.state, sizeof(S.state));
    std::memcpy(S.state_zero, F.state_zero, sizeof(S.state_zero));
    S.ab_exposure = F.ab_exposure;
    S.is_first_frame = F.frameID == 0 ? 1 : 0;
}

uint8_t res_flags(const PointFrameResidual &r) {
    return (uint8_t)((r.isActiveAndIsGoodNEW ? LDSO_BA_FLAG_ACTIVE : 0u) | (r.isNew ? LDSO_BA_FLAG_NEW : 0u));
}

// the four values of a point that change from step to step (ldso_ba_update_points)
void point_vals(const PointHessian &p, float v[4]) {
    v[0] = p.idepth_scaled;
    v[1] = p.idepth_zero_scaled;
    v[2] = p.priorF;
    v[3] = p.deltaF;
}

// write a device pass's per-residual results back into the residual objects
bool read_residuals(ldso_ba_ctx *ctx, const std::vector<PointFrameResidual *> &res) {
    const size_t R = res.size();
    if (!R) return true;
    std::vector<int8_t> ns(R), st(R);
    std::vector<float> se(R), ewo(R), ctr(3 * R), jp(8 * R), rb(R);
    std::vector<uint8_t> fl(R);
    if (ldso_ba_get_residuals(ctx, 0, ns.data(), st.data(), se.data(), ewo.data(), ctr.data(), fl.data(), jp.data(),
                              rb.data()))
        return false;
    for (size_t k = 0; k < R; k++) {
        if (!res[k]) continue;  // dropped since the load (a deferred read-back, see structuralTouch)
        PointFrameResidual &r = *res[k];
        r.state_NewState = (ResState)ns[k];
        r.state_state = (ResState)st[k];
        r.state_energy = se[k];
        r.state_NewEnergy = se[k];
        r.state_NewEnergyWithOutlier = ewo[k];
        std::memcpy(r.centerProjectedTo, &ctr[3 * k], 3 * sizeof(float));
        r.isActiveAndIsGoodNEW = (fl[k] & LDSO_BA_FLAG_ACTIVE) != 0;
        if (r.isActiveAndIsGoodNEW) {
            std::memcpy(r.JpJdF, &jp[8 * k], 8 * sizeof(float));
            std::memcpy(r.J_JpJdF, &jp[8 * k], 8 * sizeof(float));
        }
        r.relBS = rb[k];
    }
    return true;
}

}  // namespace

void EnergyFunctional::Mirror::build(std::vector<PointHessian *> points) {
    pts = std::move(points);
    host.assign(pts.size(), 0);
    rank.assign(pts.size(), 0);
    ranked = true;
    data.assign(pts.size() * LDSO_BA_POINT_STRIDE, 0.f);
    vals.resize(4 * pts.size());
    begin.assign(pts.size() + 1, 0);
    target.clear();
    energy.clear();
    state.clear();
    flags.clear();
    res.clear();
    resPoint.clear();
    for (size_t q = 0; q < pts.size(); q++) {
        const PointHessian &p = *pts[q];
        host[q] = p.host.lock()->idx;
        rank[q] = p.featureRank;
        ranked = ranked && p.featureRank >= 0;
        float *d = &data[q * LDSO_BA_POINT_STRIDE];
        d[0] = p.u;
        d[1] = p.v;
        point_vals(p, d + 2);
        point_vals(p, &vals[4 * q]);
        std::memcpy(d + 8, p.color, sizeof(p.color));
        std::memcpy(d + 16, p.weights, sizeof(p.weights));
        for (const shared_ptr<PointFrameResidual> &r : p.residuals) {
            target.push_back(r->target.lock()->idx);
            state.push_back((int8_t)r->state_state);
            energy.push_back((float)r->state_energy);
            flags.push_back(res_flags(*r));
            res.push_back(r.get());
            resPoint.push_back(pts[q]);
        }
        begin[q + 1] = (int32_t)target.size();
    }
}

void EnergyFunctional::Mirror::into(ldso_ba_window &w) const {
    w.n_points = (int32_t)host.size();
    w.n_residuals = (int32_t)target.size();
    w.point_host = host.data();
    w.point_data = data.data();
    w.point_res_begin = begin.data();
    w.res_target = target.data();
    w.res_state = state.data();
    w.res_energy = energy.data();
    w.res_flags = flags.data();
    w.point_rank = ranked ? rank.data() : nullptr;
}

// the device's state_NewEnergy is loaded equal to state_energy; the host's may differ
bool EnergyFunctional::Mirror::newEnergyDiffers() const {
    for (size_t k = 0; k < res.size(); k++)
        if ((float)res[k]->state_NewEnergy != energy[k]) return true;
    return false;
}

void FrameHessian::takeData(const ldso_ba_opt_settings *settings) {
    ldso_ba_frame_state S;
    frame_state(*this, S);
    ldso_ba_frame_take_data(1, &S, settings, prior, delta, delta_prior);
}

// Residuals.cc:15-217 (see the header): the OOB early return here, the rest from the window's
// relinearisation pass
double PointFrameResidual::linearize(shared_ptr<CalibHessian> &HCalib) {
    (void)HCalib;  // the window's calibration is its EnergyFunctional's (insertFrame / setAdjointsF)
    if (!ef) return state_energy;
    ef->residualTouched();
    state_NewEnergyWithOutlier = -1;
    if (state_state == OOB) {
        state_NewState = OOB;
        return state_energy;
    }
    return ef->linearizeResidual(*this);
}

// Residuals.h:63-68
void PointFrameResidual::resetOOB() {
    if (ef) ef->residualTouched();
    const bool same = state_NewEnergy == 0 && state_energy == 0 && state_NewState == OUTLIER && state_state == IN;
    state_NewEnergy = state_energy = 0;
    state_NewState = OUTLIER;
    state_state = IN;
    if (ef && !same) ef->residualEdited();
}

// Residuals.h:70-88; takeData (Residuals.h:120-129) is the JpJdF of the last linearisation
void PointFrameResidual::applyRes(bool copyJacobians) {
    if (ef) ef->residualTouched();
    const ResState s0 = state_state;
    const double e0 = state_energy;
    const bool a0 = isActiveAndIsGoodNEW;
    if (copyJacobians) {
        if (state_state == OOB) return;
        if (state_NewState == IN) {
            isActiveAndIsGoodNEW = true;
            std::memcpy(JpJdF, J_JpJdF, sizeof(JpJdF));
        } else {
            isActiveAndIsGoodNEW = false;
        }
    }
    state_state = state_NewState;
    state_energy = state_NewEnergy;
    if (ef && (s0 != state_state || e0 != state_energy || a0 != isActiveAndIsGoodNEW)) ef->residualEdited();
}

void PointFrameResidual::setState(ResState s) {
    if (ef) ef->residualTouched();
    if (ef && s != state_state) ef->residualEdited();
    state_state = s;
}

void PointFrameResidual::fixLinearizationF(shared_ptr<EnergyFunctional> e) {
    (void)e;
    isLinearized = true;
}

EnergyFunctional::EnergyFunctional(int device) : device_(device) {
    if (ldso_ba_create(device, &ctx_) != 0) {
        ctx_ = nullptr;
        fail("ldso_ba_create");
    }
}

EnergyFunctional::~EnergyFunctional() {
    for (const shared_ptr<PointHessian> &p : registry_)
        for (const shared_ptr<PointFrameResidual> &r : p->residuals)
            if (r->ef == this) r->ef = nullptr;
    if (margCtx_) ldso_ba_destroy(margCtx_);
    if (ctx_) ldso_ba_destroy(ctx_);
}

void EnergyFunctional::fail(const char *what) { err_ = std::string(what) + ": " + ldso_ba_last_error(); }

bool EnergyFunctional::setSettings(const ldso_ba_opt_settings &s) {
    if (!ctx_) return false;
    if (ldso_ba_set_settings(ctx_, &s) || (margCtx_ && ldso_ba_set_settings(margCtx_, &s))) {
        fail("ldso_ba_set_settings");
        return false;
    }
    const bool priors_change = s.affine_opt_mode_a != settings_.affine_opt_mode_a ||
                               s.affine_opt_mode_b != settings_.affine_opt_mode_b;
    settings_ = s;
    if (priors_change) {  // takeData's priors follow the affine modes: recompute and re-upload them
        for (const shared_ptr<FrameHessian> &f : frames) f->takeData(&settings_);
        fsUp_.clear();
        epoch_++;
    }
    return true;
}

void EnergyFunctional::packFrames(std::vector<ldso_ba_frame_state> &fs) const {
    fs.resize(frames.size());
    for (size_t f = 0; f < frames.size(); f++) frame_state(*frames[f], fs[f]);
}

// EnergyFunctional.cc:45-49 (the caller has pushed r into its point's residuals)
void EnergyFunctional::insertResidual(shared_ptr<PointFrameResidual> r) {
    structuralTouch();  // before any structural change: the mirror's residuals may not outlive it
    r->ef = this;
    r->mirrorIdx = -1;
    connectivityMap[conn_key(*r)][0]++;
    nResiduals++;
    dirty_ = true;
    epoch_++;
}

// EnergyFunctional.cc:51-98 (the non-VI part): HM, bM grow by the frame's 8 zero rows/columns
void EnergyFunctional::insertFrame(shared_ptr<FrameHessian> fh, shared_ptr<CalibHessian> Hcalib) {
    insertFrameImpl(fh, Hcalib, nullptr);
}
void EnergyFunctional::insertFrame(shared_ptr<FrameHessian> fh, shared_ptr<CalibHessian> Hcalib, const ldso_ct_ctx *tracker) {
    if (!tracker) {
        err_ = "insertFrame: null tracker";
        return;
    }
    if (!resident_) {
        err_ = "insertFrame from the tracker needs resident frames (setResidentFrames(true))";
        return;
    }
    insertFrameImpl(fh, Hcalib, tracker);
}

bool EnergyFunctional::storeHas(int frameID) const {
    return std::find(storeIds_.begin(), storeIds_.end(), frameID) != storeIds_.end();
}

// LDSO_BA_MAX_FRAMES + 1 slots of the current image size: the window plus the frame that enters
// before the marginalised one has left.  Re-reserving (another size) drops every resident frame.
bool EnergyFunctional::storeReserve() {
    if (storeW_ == width_ && storeH_ == height_) return true;
    storeIds_.clear();
    storeW_ = storeH_ = 0;
    if (ldso_ba_frames_reserve(ctx_, LDSO_BA_MAX_FRAMES + 1, width_, height_)) {
        fail("ldso_ba_frames_reserve");
        return false;
    }
    storeW_ = width_;
    storeH_ = height_;
    return true;
}

// fh.dI into the store.  Gradients that are not makeImages' (image layout 3 recomputes them) keep
// ldso_ba_load's silent fallback: the store is reserved again in layout 1 and the window's frames
// put again from their host dI; where that is not possible (the layout is fixed once a window is
// loaded, or a frame has no host image) the window goes back to ldso_ba_load, which falls back itself.
bool EnergyFunctional::storePutHost(const FrameHessian &fh) {
    if (!fh.dI) {
        err_ = "frame " + std::to_string(fh.frameID) + " has no host dI and was not handed over from the tracker";
        return false;
    }
    const int rc = ldso_ba_frame_put(ctx_, fh.frameID, fh.dI);
    if (rc == 0) {
        if (!storeHas(fh.frameID)) storeIds_.push_back(fh.frameID);
        return true;
    }
    if (rc != LDSO_BA_ERR_GRADIENT_MISMATCH) {
        fail("ldso_ba_frame_put");
        return false;
    }
    bool all_host = true;
    for (const shared_ptr<FrameHessian> &f : frames) all_host = all_host && f->dI;
    if (all_host && ldso_ba_set_tuning(ctx_, LDSO_BA_TUNE_TILED_IMAGES, 1) == 0) {
        storeW_ = storeH_ = 0;
        if (!storeReserve()) return false;
        for (const shared_ptr<FrameHessian> &f : frames) {
            if (ldso_ba_frame_put(ctx_, f->frameID, f->dI)) {
                fail("ldso_ba_frame_put (layout 1)");
                return false;
            }
            storeIds_.push_back(f->frameID);
        }
        if (!storeHas(fh.frameID)) {  // fh is not in the window yet
            if (ldso_ba_frame_put(ctx_, fh.frameID, fh.dI)) {
                fail("ldso_ba_frame_put (layout 1)");
                return false;
            }
            storeIds_.push_back(fh.frameID);
        }
        return true;
    }
    if (!all_host) {
        err_ = "frame " + std::to_string(fh.frameID) + ": gradients are not makeImages' and a frame of the window has no host dI";
        return false;
    }
    resident_ = false;
    dirty_ = true;
    return true;
}

void EnergyFunctional::setResidentFrames(bool on) {
    if (on == resident_) return;
    residualTouched();
    resident_ = on;
    dirty_ = true;  // the next pass reloads the window through the chosen path
    epoch_++;
}

void EnergyFunctional::insertFrameImpl(shared_ptr<FrameHessian> fh, shared_ptr<CalibHessian> Hcalib,
                                       const ldso_ct_ctx *tracker) {
    structuralTouch();
    fh->takeData(&settings_);
    frames.push_back(fh);
    fh->idx = (int)frames.size();
    nFrames++;
    const int n = 8 * nFrames + CPARS;
    MatXX H2(n, n);
    VecX b2(n);
    for (int i = 0; i < HM.rows(); i++) {
        b2[i] = bM[i];
        for (int j = 0; j < HM.cols(); j++) H2(i, j) = HM(i, j);
    }
    HM = H2;
    bM = b2;
    calib_ = *Hcalib;
    width_ = Hcalib->wG0;
    height_ = Hcalib->hG0;
    if (resident_ && ctx_ && storeReserve()) {
        if (tracker) {
            if (ldso_ba_frame_put_tracker(ctx_, fh->frameID, tracker)) fail("ldso_ba_frame_put_tracker");
            else if (!storeHas(fh->frameID)) storeIds_.push_back(fh->frameID);
        } else {
            storePutHost(*fh);
        }
    }
    setAdjointsF(Hcalib);
    makeIDX();
    for (const shared_ptr<FrameHessian> &fh2 : frames) {
        connectivityMap[((uint64_t)fh->frameID << 32) + (uint64_t)fh2->frameID] = {0, 0};
        if (fh2 != fh) connectivityMap[((uint64_t)fh2->frameID << 32) + (uint64_t)fh->frameID] = {0, 0};
    }
    dirty_ = true;
    epoch_++;
}

void EnergyFunctional::insertPoint(shared_ptr<PointHessian> ph) {
    structuralTouch();
    ph->status = PointStatus::ACTIVE;
    ph->alreadyRemoved = false;
    loaded_.pointIndex.erase(ph.get());  // a new point, even at the address of one the mirror held
    registry_.push_back(ph);
    allPoints.push_back(ph);
    nPoints++;
    dirty_ = true;
    epoch_++;
}

// EnergyFunctional.cc:100-107
void EnergyFunctional::dropResidual(shared_ptr<PointFrameResidual> r) {
    structuralTouch();
    shared_ptr<PointHessian> p = r->point.lock();
    if (p) {
        auto &v = p->residuals;
        auto it = std::find(v.begin(), v.end(), r);
        if (it != v.end()) v.erase(it);
    }
    connectivityMap[conn_key(*r)][0]--;
    nResiduals--;
    if (r->ef == this) r->ef = nullptr;
    forgetResidual(r.get());
    r->mirrorIdx = -1;
    dirty_ = true;
    epoch_++;
}

// EnergyFunctional.cc:109-191: the dense reorder / prior / Schur step on the host
// (ldso_ba_marginalize_frame), then the frame leaves the window
void EnergyFunctional::marginalizeFrame(shared_ptr<FrameHessian> fh) {
    structuralTouch();
    const int no = 8 * nFrames + CPARS, nn = no - 8;
    MatXX Ho(nn, nn);
    VecX bo(nn);
    if (ldso_ba_marginalize_frame(nFrames, fh->idx, HM.data(), bM.data(), fh->prior, fh->delta_prior, Ho.data(),
                                  bo.data())) {
        fail("ldso_ba_marginalize_frame");
        return;
    }
    HM = Ho;
    bM = bo;
    if (storeHas(fh->frameID)) {
        storeIds_.erase(std::find(storeIds_.begin(), storeIds_.end(), fh->frameID));
        if (ldso_ba_frame_drop(ctx_, fh->frameID)) fail("ldso_ba_frame_drop");
    }
    for (size_t i = (size_t)fh->idx; i + 1 < frames.size(); i++) {
        frames[i] = frames[i + 1];
        frames[i]->idx = (int)i;
    }
    frames.pop_back();
    nFrames--;
    makeIDX();
    dirty_ = true;
    epoch_++;
}

// EnergyFunctional.cc:193-203
void EnergyFunctional::removePoint(shared_ptr<PointHessian> ph) {
    structuralTouch();
    for (const shared_ptr<PointFrameResidual> &r : ph->residuals) {
        connectivityMap[conn_key(*r)][0]--;
        nResiduals--;
        if (r->ef == this) r->ef = nullptr;
        forgetResidual(r.get());
        r->mirrorIdx = -1;
    }
    if (incremental_) {
        const auto it = loaded_.pointIndex.find(ph.get());
        if (it != loaded_.pointIndex.end()) {
            if ((size_t)it->second < loaded_.pts.size() && loaded_.pts[it->second] == ph.get()) loaded_.pts[it->second] = nullptr;
            loaded_.pointIndex.erase(it);
        }
    }
    ph->residuals.clear();
    if (!ph->alreadyRemoved) nPoints--;
    ph->alreadyRemoved = true;
    dirty_ = true;
    epoch_++;
}

// ldso_ba_flag_points on the loaded window (see the header)
EnergyFunctional::FlagResult EnergyFunctional::flagPoints(const ldso_ba_flag_params *params,
                                                          const std::vector<uint8_t> &frameFlagged,
                                                          const std::vector<int32_t> &numGood,
                                                          const std::vector<int32_t> &lastRes,
                                                          const std::vector<int8_t> &lastState) {
    FlagResult out;
    if (!ctx_) {
        if (err_.empty()) err_ = "flagPoints: no device context";
        return out;
    }
    if (dirty_ || resSync_ == ResSync::HostNewer) {
        err_ = "flagPoints: the window changed since the last pass (call it after linearizeAll(true), before the "
               "structural changes and residual edits that follow)";
        return out;
    }
    const size_t P = loaded_.pts.size(), R = loaded_.res.size(), N = frames.size();
    if (numGood.size() != P || lastRes.size() != 2 * P || (!lastState.empty() && lastState.size() != 2 * P) ||
        (!frameFlagged.empty() && frameFlagged.size() != N)) {
        err_ = "flagPoints: array sizes do not match the window (allPoints order: numGood [P], lastRes / lastState [2 P])";
        return out;
    }
    std::vector<uint8_t> ff(frameFlagged);
    if (ff.empty())
        for (const shared_ptr<FrameHessian> &f : frames) ff.push_back(f->flaggedForMarginalization ? 1 : 0);
    std::vector<int8_t> status(P);
    std::vector<uint8_t> live(R);
    std::vector<int32_t> ng(P), counts(4, 0);
    out.lastState.assign(2 * P, -1);
    if (ldso_ba_flag_points(ctx_, 0, params, ff.data(), numGood.data(), lastRes.data(),
                            lastState.empty() ? nullptr : lastState.data(), status.data(), live.data(), ng.data(),
                            out.lastState.data(), counts.data())) {
        fail("ldso_ba_flag_points");
        return out;
    }
    for (size_t q = 0; q < P; q++) loaded_.pts[q]->status = (PointStatus)status[q];  // LDSO_BA_PT_* are PointStatus' values
    for (size_t k = 0; k < R; k++)
        if (!live[k]) out.toRemove.push_back(loaded_.res[k]);
    out.numGood.assign(ng.begin(), ng.end());
    for (int i = 0; i < 4; i++) out.counts[i] = counts[i];
    out.ok = true;
    return out;
}

// the frame-level fields of an ldso_ba_window, from the terms uploadFrameTerms computed last;
// hostImages: with the images stageImages gathered for ldso_ba_load
void EnergyFunctional::frameTermsWindow(ldso_ba_window &w, bool hostImages) {
    std::memset(&w, 0, sizeof(w));
    w.n_frames = nFrames;
    if (hostImages) w.dI = dI_.data();
    w.width = width_;
    w.height = height_;
    std::memcpy(w.calib, calib_.value_scaledf, sizeof(w.calib));
    w.frame_energy_th = frameTH_.data();
    w.precalc = precalc_.data();
    w.ad_host = adH_.data();
    w.ad_target = adT_.data();
    w.c_prior = cPrior_.data();
    w.c_delta = cDeltaF;
    w.frame_prior = fPrior_.data();
    w.frame_delta_prior = fDeltaPrior_.data();
}

// marginalizePointsF's tail (EnergyFunctional.cc:244-262): res are the marginalisation context's
// residuals with its results read into them, (H, b) its system
void EnergyFunctional::applyMarginalization(const std::vector<PointFrameResidual *> &res, const std::vector<double> &H,
                                            const std::vector<double> &b) {
    const int n = 8 * nFrames + CPARS;
    passes_++;
    int nres = 0;
    for (PointFrameResidual *r : res) {
        if (r->isActive()) {
            r->isLinearized = true;  // fixLinearizationF
            connectivityMap[conn_key(*r)][1]++;
            nres++;
        }
    }
    for (const shared_ptr<PointHessian> &p : allPointsToMarg) p->priorF *= kIdepthFixPriorMargFac;
    resInM += nres;
    for (int i = 0; i < n; i++) {
        bM[i] += kMargWeightFac * b[i];
        for (int j = 0; j < n; j++) HM(i, j) += kMargWeightFac * H[(size_t)i * n + j];
    }
    for (const shared_ptr<PointHessian> &p : allPointsToMarg) removePoint(p);
    makeIDX();
}

bool EnergyFunctional::margContext() {
    if (!margCtx_ && ldso_ba_create(device_, &margCtx_)) {
        margCtx_ = nullptr;
        fail("ldso_ba_create (marginalisation)");
    }
    return margCtx_ != nullptr;
}

// marginalizePointsF from the loaded window's device arrays (setDeviceMarginalization).  Returns false
// where that cannot give what the host path gives; true once the call is served (or failed: ok()).
bool EnergyFunctional::marginalizeFromDevice() {
    const Mirror &m = loaded_;
    if (!ctx_ || !incremental_ || !resident_ || !m.tracked || resSync_ == ResSync::HostNewer) return false;
    if ((int)m.loadedIds.size() != nFrames) return false;
    for (int f = 0; f < nFrames; f++)
        if (m.loadedIds[f] != frames[f]->frameID) return false;  // the loaded window has other frames
    // current frame terms; without a structural change pending also the host's point values and residual edits
    if (dirty_ ? !uploadFrameTerms() : !upload()) return true;
    if (resSync_ == ResSync::HostNewer) return false;
    std::vector<int32_t> pts;
    std::vector<uint8_t> live(m.res.size(), 0);
    std::vector<PointFrameResidual *> res;
    for (const shared_ptr<PointHessian> &p : allPointsToMarg) {
        const auto it = m.pointIndex.find(p.get());
        if (it == m.pointIndex.end() || (size_t)it->second >= m.pts.size() || m.pts[it->second] != p.get()) return false;
        const int q = it->second;
        float pv[4];
        point_vals(*p, pv);
        if (std::memcmp(pv, &m.vals[4 * (size_t)q], sizeof(pv)) != 0) return false;  // the device holds older values
        int last = m.begin[q] - 1;
        for (const shared_ptr<PointFrameResidual> &r : p->residuals) {  // the loaded ones, in the loaded order
            const int k = r->mirrorIdx;
            if (k <= last || k >= m.begin[q + 1] || m.res[k] != r.get()) return false;
            live[k] = 1;
            res.push_back(r.get());
            last = k;
        }
        pts.push_back(q);
    }
    if (!margContext()) return true;
    ldso_ba_window w;
    frameTermsWindow(w);
    if (ldso_ba_load_marginalization_device(margCtx_, ctx_, 0, &w, (int32_t)pts.size(), pts.data(), live.data()))
        return false;  // refused (ldso_ba_last_error says why): the host path
    const int n = 8 * nFrames + CPARS;
    std::vector<double> H((size_t)n * n), b(n);
    if (ldso_ba_marginalize_points(margCtx_, adHTdeltaF.data(), H.data(), b.data())) {
        fail("ldso_ba_marginalize_points");
        return true;
    }
    if (!read_residuals(margCtx_, res)) {
        fail("ldso_ba_get_residuals (marginalisation)");
        return true;
    }
    deviceMargs_++;
    applyMarginalization(res, H, b);
    return true;
}

// EnergyFunctional.cc:205-262 with FullSystem.cc:1384-1404 (see the header)
void EnergyFunctional::marginalizePointsF() {
    epoch_++;
    allPointsToMarg.clear();
    for (const shared_ptr<PointHessian> &p : registry_)
        if (p->status == PointStatus::MARGINALIZED && !p->alreadyRemoved) allPointsToMarg.push_back(p);
    if (deviceMarg_ && (allPointsToMarg.empty() || marginalizeFromDevice())) return;
    residualTouched();
    if (allPointsToMarg.empty()) return;
    if (!upload()) return;  // current frame terms; the parent window lends its device images
    if (!margContext()) return;
    // the parent window as loaded holds every point still flagged ACTIVE before this call
    std::vector<PointHessian *> pts;
    for (const shared_ptr<PointHessian> &p : allPointsToMarg) pts.push_back(p.get());
    Mirror pk;
    pk.build(pts);
    ldso_ba_window w;
    frameTermsWindow(w);
    pk.into(w);
    const int n = 8 * nFrames + CPARS;
    std::vector<double> H((size_t)n * n), b(n);
    if (ldso_ba_load_marginalization(margCtx_, ctx_, 0, &w) ||
        ldso_ba_marginalize_points(margCtx_, adHTdeltaF.data(), H.data(), b.data())) {
        fail("ldso_ba_marginalize_points");
        return;
    }
    if (!read_residuals(margCtx_, pk.res)) {
        fail("ldso_ba_get_residuals (marginalisation)");
        return;
    }
    applyMarginalization(pk.res, H, b);
}

// EnergyFunctional.cc:264-278
void EnergyFunctional::dropPointsF() {
    structuralTouch();
    for (const shared_ptr<PointHessian> &p : registry_)
        if ((p->status == PointStatus::OUTLIER || p->status == PointStatus::OUT) && !p->alreadyRemoved) removePoint(p);
    makeIDX();
}

// EnergyFunctional.cc:500-521: frame indices; the active, not removed points in host-frame order
// (the reference walks its frames' features; registry_ is that list)
void EnergyFunctional::makeIDX() {
    structuralTouch();
    epoch_++;
    for (size_t i = 0; i < frames.size(); i++) frames[i]->idx = (int)i;
    std::vector<shared_ptr<PointHessian>> keep, live;
    for (const shared_ptr<PointHessian> &p : registry_) {
        if (p->alreadyRemoved) continue;
        live.push_back(p);
        if (p->status == PointStatus::ACTIVE) keep.push_back(p);
    }
    registry_.swap(live);
    std::stable_sort(keep.begin(), keep.end(), [](const shared_ptr<PointHessian> &a, const shared_ptr<PointHessian> &b) {
        return a->host.lock()->idx < b->host.lock()->idx;
    });
    allPoints.swap(keep);
    for (size_t i = 0; i < allPoints.size(); i++) {
        allPoints[i]->idxInPoints = (int)i;
        for (const shared_ptr<PointFrameResidual> &r : allPoints[i]->residuals) {
            r->hostIDX = r->host.lock()->idx;
            r->targetIDX = r->target.lock()->idx;
        }
    }
    dirty_ = true;
}

// EnergyFunctional.cc:551-609 (ldso_ba_set_adjoints)
void EnergyFunctional::setAdjointsF(shared_ptr<CalibHessian> Hcalib) {
    (void)Hcalib;
    epoch_++;
    std::vector<ldso_ba_frame_state> fs;
    packFrames(fs);
    adHost.assign((size_t)nFrames * nFrames * 64, 0.0);
    adTarget.assign((size_t)nFrames * nFrames * 64, 0.0);
    if (nFrames && ldso_ba_set_adjoints(nFrames, fs.data(), adHost.data(), adTarget.data(), cPrior))
        fail("ldso_ba_set_adjoints");
}

// EnergyFunctional.cc:523-549: frames' delta / delta_prior, adHTdeltaF, cDeltaF, points' deltaF
void EnergyFunctional::setDeltaF(shared_ptr<CalibHessian> HCalib) {
    epoch_++;
    for (int k = 0; k < 4; k++) cDeltaF[k] = (float)HCalib->value_minus_value_zero[k];
    std::vector<double> delta((size_t)8 * nFrames);
    for (int f = 0; f < nFrames; f++) {
        frames[f]->takeData(&settings_);
        std::memcpy(&delta[(size_t)8 * f], frames[f]->delta, 8 * sizeof(double));
    }
    adHTdeltaF.assign((size_t)nFrames * nFrames * 8, 0.f);
    if (nFrames && ldso_ba_ad_ht_delta(nFrames, delta.data(), adHost.data(), adTarget.data(), adHTdeltaF.data()))
        fail("ldso_ba_ad_ht_delta");
    for (const shared_ptr<PointHessian> &p : allPoints) p->deltaF = p->idepth - p->idepth_zero;
    calib_ = *HCalib;
}

// EnergyFunctional.cc:473-479
double EnergyFunctional::calcMEnergyF() {
    std::vector<double> delta((size_t)8 * nFrames);
    for (int f = 0; f < nFrames; f++) std::memcpy(&delta[(size_t)8 * f], frames[f]->delta, 8 * sizeof(double));
    double e = 0;
    if (ldso_ba_calc_m_energy(nFrames, HM.data(), bM.data(), cDeltaF, delta.data(), &e)) fail("ldso_ba_calc_m_energy");
    return e;
}

// EnergyFunctional.cc:481-498
double EnergyFunctional::calcLEnergyF_MT() {
    std::vector<double> prior((size_t)8 * nFrames), dprior((size_t)8 * nFrames);
    for (int f = 0; f < nFrames; f++) {
        std::memcpy(&prior[(size_t)8 * f], frames[f]->prior, 8 * sizeof(double));
        std::memcpy(&dprior[(size_t)8 * f], frames[f]->delta_prior, 8 * sizeof(double));
    }
    std::vector<float> dd(allPoints.size()), pf(allPoints.size());
    for (size_t q = 0; q < allPoints.size(); q++) {
        dd[q] = allPoints[q]->deltaF;
        pf[q] = allPoints[q]->priorF;
    }
    double e = 0;
    if (ldso_ba_calc_l_energy(nFrames, prior.data(), dprior.data(), cPrior, cDeltaF, (int32_t)dd.size(), dd.data(),
                              pf.data(), &e))
        fail("ldso_ba_calc_l_energy");
    return e;
}

// Frame-level terms (setPrecalcValues, setAdjointsF, takeData) from the current frame states,
// uploaded only when a frame state, the calibration or a threshold changed since the last upload
bool EnergyFunctional::uploadFrameTerms() {
    const int N = nFrames;
    packFrames(fs_);
    frameTH_.resize(N);
    for (int f = 0; f < N; f++) frameTH_[f] = frames[f]->frameEnergyTH;
    const bool same = fsUp_.size() == fs_.size() && thUp_ == frameTH_ &&
                      std::memcmp(fsUp_.data(), fs_.data(), fs_.size() * sizeof(ldso_ba_frame_state)) == 0 &&
                      std::memcmp(calibUp_, calib_.value_scaledf, sizeof(calibUp_)) == 0 &&
                      std::memcmp(cDeltaUp_, cDeltaF, sizeof(cDeltaUp_)) == 0;  // the bL calibration prior
    if (same && !dirty_) return true;
    precalc_.assign((size_t)N * N * LDSO_BA_PRECALC_STRIDE, 0.f);
    adH_.assign((size_t)N * N * 64, 0.0);
    adT_.assign((size_t)N * N * 64, 0.0);
    cPrior_.assign(4, 0.0);
    fPrior_.assign((size_t)N * 8, 0.0);
    fDelta_.assign((size_t)N * 8, 0.0);
    fDeltaPrior_.assign((size_t)N * 8, 0.0);
    if (ldso_ba_frame_precalc(N, fs_.data(), calib_.value_scaledf, precalc_.data()) ||
        ldso_ba_set_adjoints(N, fs_.data(), adH_.data(), adT_.data(), cPrior_.data()) ||
        ldso_ba_frame_take_data(N, fs_.data(), &settings_, fPrior_.data(), fDelta_.data(), fDeltaPrior_.data())) {
        fail("frame terms");
        return false;
    }
    if (!dirty_) {  // structure unchanged: the frame terms alone (ldso_ba_update without point data)
        ldso_ba_window w;
        frameTermsWindow(w);
        w.n_points = (int32_t)loaded_.pts.size();  // the loaded counts, no point arrays
        w.n_residuals = (int32_t)loaded_.res.size();
        if (ldso_ba_update(ctx_, 0, &w)) {
            fail("ldso_ba_update");
            return false;
        }
    }
    fsUp_ = fs_;
    thUp_ = frameTH_;
    std::memcpy(calibUp_, calib_.value_scaledf, sizeof(calibUp_));
    std::memcpy(cDeltaUp_, cDeltaF, sizeof(cDeltaUp_));
    return true;
}

// Without a structural change only what changed goes up: the frame terms, the points' four per-step
// values (ldso_ba_update_points, 16 B a point, read through the mirror's raw pointers) and residual
// states edited on the host.
bool EnergyFunctional::uploadValues() {
    if (!uploadFrameTerms()) return false;
    const size_t P = loaded_.pts.size(), R = loaded_.res.size();
    std::vector<float> pv(4 * P);
    for (size_t q = 0; q < P; q++) point_vals(*loaded_.pts[q], &pv[4 * q]);
    if (P && std::memcmp(pv.data(), loaded_.vals.data(), pv.size() * sizeof(float)) != 0) {
        if (ldso_ba_update_points(ctx_, 0, pv.data())) {
            fail("ldso_ba_update_points");
            return false;
        }
        loaded_.vals.swap(pv);
    }
    if (resSync_ != ResSync::HostNewer) return true;
    std::vector<int8_t> st(R);
    std::vector<float> se(R), ne(R);
    std::vector<uint8_t> fl(R);
    for (size_t k = 0; k < R; k++) {
        const PointFrameResidual &r = *loaded_.res[k];
        st[k] = (int8_t)r.state_state;
        se[k] = (float)r.state_energy;
        ne[k] = (float)r.state_NewEnergy;
        fl[k] = res_flags(r);
    }
    if (ldso_ba_update_residuals(ctx_, 0, st.data(), se.data(), ne.data(), fl.data())) {
        fail("ldso_ba_update_residuals");
        return false;
    }
    resSync_ = ResSync::Synced;
    return true;
}

// loaded_ becomes the mirror of the window as the objects have it now (the only place the weak_ptr
// graph is walked).  sources: also where every entry lies in `old`, the mirror loaded so far (-1: new);
// a residual keeps its mirrorIdx until it is inserted or dropped, a point is found by address.  old's
// entries are compared by address and never dereferenced (dropped ones are null).
void EnergyFunctional::buildMirror(const Mirror &old, bool sources, std::vector<int32_t> &pointSrc,
                                   std::vector<int32_t> &resSrc) {
    std::vector<PointHessian *> pts;
    for (const shared_ptr<PointHessian> &p : allPoints) pts.push_back(p.get());
    Mirror &m = loaded_;
    m = Mirror();
    m.build(pts);
    if (sources) {
        pointSrc.assign(m.pts.size(), -1);
        resSrc.assign(m.res.size(), -1);
        for (size_t q = 0; q < m.pts.size(); q++) {
            const auto it = old.pointIndex.find(m.pts[q]);
            if (it != old.pointIndex.end()) pointSrc[q] = it->second;
        }
        bool new_ne_differs = false;
        for (size_t k = 0; k < m.res.size(); k++) {
            const int o = m.res[k]->mirrorIdx;
            if (o >= 0 && (size_t)o < old.res.size() && old.res[o] == m.res[k]) resSrc[k] = o;
            else new_ne_differs = new_ne_differs || (float)m.res[k]->state_NewEnergy != m.energy[k];
        }
        // a deferred read-back stays deferred through the edit only if the new residuals need no
        // upload of their own afterwards (state_NewEnergy is loaded equal to state_energy)
        if (deferred_ && new_ne_differs) {
            syncInto(old);  // reads the loaded window into the loaded mirror's objects
            m.build(pts);
        }
    }
    nResiduals = (int)m.res.size();
    for (size_t k = 0; k < m.res.size(); k++) m.res[k]->mirrorIdx = (int)k;
}

// The window's images: by frame id out of the store (frames missing there -- the path was switched on
// with the window in place, or the store was reserved again -- go in now from their host dI), or
// gathered on the host into dI_ for ldso_ba_load
bool EnergyFunctional::stageImages(std::vector<int64_t> &ids) {
    const int N = nFrames;
    if (resident_) {
        if (!storeReserve()) return false;
        for (int f = 0; f < N && resident_; f++)
            if (!storeHas(frames[f]->frameID) && !storePutHost(*frames[f])) return false;
    }
    if (resident_) {
        for (int f = 0; f < N; f++) ids.push_back(frames[f]->frameID);
        std::vector<float>().swap(dI_);
        return true;
    }
    const size_t px = (size_t)width_ * height_ * 3;
    dI_.resize(N * px);
    for (int f = 0; f < N; f++) {
        if (!frames[f]->dI) {
            err_ = "frame " + std::to_string(frames[f]->frameID) + " has no host dI (handed over from the tracker): ldso_ba_load needs it";
            return false;
        }
        std::memcpy(&dI_[f * px], frames[f]->dI, px * sizeof(float));
    }
    return true;
}

// ldso_ba_edit_window from `old`, the mirror of the window on the device, to loaded_.  False: refused
// (ldso_ba_last_error says why), the device's window is untouched and w current for the reload.
bool EnergyFunctional::editWindow(const Mirror &old, ldso_ba_window &w, const std::vector<int64_t> &ids,
                                  const std::vector<int32_t> &pointSrc, const std::vector<int32_t> &resSrc) {
    std::vector<int32_t> frameSrc(nFrames, -1);
    for (int f = 0; f < nFrames; f++) {
        const auto it = std::find(old.loadedIds.begin(), old.loadedIds.end(), frames[f]->frameID);
        if (it != old.loadedIds.end()) frameSrc[f] = (int32_t)(it - old.loadedIds.begin());
    }
    const ldso_ba_edit ed = {&w, ids.data(), frameSrc.data(), pointSrc.data(), resSrc.data()};
    if (ldso_ba_edit_window(ctx_, 0, &ed) == 0) return true;
    editsFallenBack_++;
    if (deferred_) {  // read the loaded window into the loaded mirror's objects first
        syncInto(old);
        loaded_.build(loaded_.pts);
        loaded_.into(w);
    }
    return false;
}

// the edit went through: loaded_ is the device's window
void EnergyFunctional::editApplied(const Mirror &old, const std::vector<int64_t> &ids, const std::vector<int32_t> &pointSrc) {
    Mirror &m = loaded_;
    editsApplied_++;
    m.loadedIds.assign(ids.begin(), ids.end());
    // the device holds, on a surviving point, the values it held before: uploadValues sends the
    // points' values if the host's differ
    for (size_t q = 0; q < m.pts.size(); q++)
        if (pointSrc[q] >= 0 && (size_t)4 * pointSrc[q] + 3 < old.vals.size())
            std::memcpy(&m.vals[4 * q], &old.vals[4 * (size_t)pointSrc[q]], 4 * sizeof(float));
    if (deferred_) {
        // the surviving residuals' state never came to the host and went into the new window
        // on the device; the last pass's results are gone, as after a load
        deferred_ = false;
        lostResultsAt_ = passes_;
        outStatePass_ = outCenterPass_ = -1;  // cached in the loaded mirror's order
        outState_.assign(m.res.size(), 0);
    } else if (m.newEnergyDiffers()) {
        // ... and on a surviving residual the state the host read back (or edited since: HostNewer,
        // sent by uploadValues)
        resSync_ = ResSync::HostNewer;
    }
    dirty_ = false;
}

bool EnergyFunctional::reload(const ldso_ba_window &w, const std::vector<int64_t> &ids) {
    deferred_ = false;
    lostResultsAt_ = -1;
    if (resident_ ? ldso_ba_load_frames(ctx_, 1, &w, ids.data(), 0, 1) : ldso_ba_load(ctx_, 1, &w, 0, 1)) {
        fail(resident_ ? "ldso_ba_load_frames" : "ldso_ba_load");
        return false;
    }
    if (resident_) loaded_.loadedIds.assign(ids.begin(), ids.end());
    resSync_ = loaded_.newEnergyDiffers() ? ResSync::HostNewer : ResSync::Synced;
    dirty_ = false;
    return true;
}

// The persistent SoA mirror of the window (ldso_ba_window), loaded_.  A structural change (insert /
// drop / remove / makeIDX / marginalisation) rebuilds it and edits or reloads the device's window;
// otherwise only what changed goes up (uploadValues).
bool EnergyFunctional::upload() {
    if (!ctx_) return false;
    if (nFrames < 2) {
        err_ = "need at least two frames";
        return false;
    }
    if (!dirty_) return uploadValues();
    using SplitClock = std::chrono::steady_clock;
    auto ms_since = [](SplitClock::time_point t) { return std::chrono::duration<double, std::milli>(SplitClock::now() - t).count(); };
    SplitClock::time_point t_part = SplitClock::now();
    // incremental edits: an edit can be tried if the loaded window's entries were tracked
    const bool tryEdit = incremental_ && resident_ && loaded_.tracked && !loaded_.loadedIds.empty();
    if (deferred_ && !tryEdit) syncResiduals();  // the reload below sends the host's values: make them current
    if (!uploadFrameTerms()) return false;
    split_[3] += ms_since(t_part);
    t_part = SplitClock::now();
    const Mirror old = std::move(loaded_);
    std::vector<int32_t> pointSrc, resSrc;
    buildMirror(old, tryEdit, pointSrc, resSrc);
    std::vector<int64_t> ids;
    if (!stageImages(ids)) return false;
    ldso_ba_window w;
    frameTermsWindow(w, !resident_);
    loaded_.into(w);
    loaded_.tracked = incremental_ && resident_;
    if (loaded_.tracked) {
        loaded_.pointIndex.reserve(loaded_.pts.size());
        for (size_t q = 0; q < loaded_.pts.size(); q++) loaded_.pointIndex[loaded_.pts[q]] = (int)q;
    }
    split_[0] += 1;
    split_[2] += ms_since(t_part);
    t_part = SplitClock::now();
    const bool edited = tryEdit && resident_ && editWindow(old, w, ids, pointSrc, resSrc);
    if (!edited && !reload(w, ids)) return false;
    split_[4] += ms_since(t_part);
    t_part = SplitClock::now();
    if (edited) editApplied(old, ids, pointSrc);
    if (!edited && resSync_ != ResSync::HostNewer) return true;
    const bool done = uploadValues();  // what the host changed on a surviving entry follows
    split_[5] += ms_since(t_part);
    return done;
}

void EnergyFunctional::resetOOB() {
    residualTouched();
    for (const shared_ptr<PointHessian> &p : allPoints)
        for (const shared_ptr<PointFrameResidual> &r : p->residuals)
            if (!r->isLinearized) {  // FullSystem.cc:866-869 (the mirror follows below)
                r->state_NewEnergy = r->state_energy = 0;
                r->state_NewState = OUTLIER;
                r->state_state = IN;
            }
    if (!dirty_ && ctx_) {
        if (ldso_ba_reset_oob(ctx_, 0)) fail("ldso_ba_reset_oob");
        else if (resSync_ == ResSync::DeviceNewer) resSync_ = ResSync::Synced;
    } else if (incremental_) {
        resSync_ = ResSync::HostNewer;  // an edit carries the device's residual state: the reset ones follow it
    }
}

// the points' HdiF / bdSumF / idepth_hessian of the device's last pass into m's points and, with
// `thresholds`, the frames' energy thresholds into the frames
bool EnergyFunctional::readPointsAndThresholds(const Mirror &m, bool thresholds) {
    const size_t P = m.pts.size();
    std::vector<float> hdi(P), bds(P), ih(P);
    if (P && ldso_ba_get_points(ctx_, 0, hdi.data(), bds.data(), ih.data(), nullptr, nullptr, nullptr)) {
        fail("ldso_ba_get_points");
        return false;
    }
    for (size_t q = 0; q < P; q++) {
        if (!m.pts[q]) continue;  // removed since the load (a deferred read-back)
        m.pts[q]->HdiF = hdi[q];
        m.pts[q]->bdSumF = bds[q];
        m.pts[q]->idepth_hessian = ih[q];
    }
    std::vector<float> th(nFrames);
    if (thresholds && ldso_ba_get_frame_energy_th(ctx_, 0, th.data()) == 0) {
        for (int f = 0; f < nFrames; f++) frames[f]->frameEnergyTH = th[f];
        thUp_ = th;  // the device holds these already
        frameTH_ = th;
    }
    return true;
}

// every per-residual / per-point result of the device's last pass into the objects of m, the mirror
// of the window the device holds
bool EnergyFunctional::readBack(const Mirror &m) {
    if (lostResultsAt_ == passes_) {
        // an edit carried the residuals' state past the host and reset the last pass's results, as a
        // load does: state, energy and flags are what the device still knows
        const size_t R = m.res.size();
        std::vector<int8_t> st(R);
        std::vector<float> se(R);
        std::vector<uint8_t> fl(R);
        if (R && ldso_ba_get_residuals(ctx_, 0, nullptr, st.data(), se.data(), nullptr, nullptr, fl.data(), nullptr, nullptr)) {
            fail("ldso_ba_get_residuals");
            return false;
        }
        for (size_t k = 0; k < R; k++) {
            if (!m.res[k]) continue;
            PointFrameResidual &r = *m.res[k];
            r.state_state = (ResState)st[k];
            r.state_energy = r.state_NewEnergy = se[k];
            r.isActiveAndIsGoodNEW = (fl[k] & LDSO_BA_FLAG_ACTIVE) != 0;
        }
        resSync_ = ResSync::Synced;
        return true;
    }
    if (!read_residuals(ctx_, m.res)) {
        fail("ldso_ba_get_residuals");
        return false;
    }
    resSync_ = ResSync::Synced;
    // the frames may have changed since the load (dirty_): their thresholds were read with the pass
    return readPointsAndThresholds(m, !dirty_);
}

// linearizeAll's read-back of what its callers need at once: the frame thresholds, the points'
// HdiF / bdSumF / idepth_hessian, the residual states and, on the fix pass, FixPassResult from the
// flags and relBS; every other residual field stays on the device until a consumer asks
// (syncResiduals, a residual method, residualCenter)
bool EnergyFunctional::readPassSummary(bool fix) {
    const Mirror &m = loaded_;
    const size_t R = m.res.size(), P = m.pts.size();
    const int N = nFrames;
    std::vector<uint8_t> fl(R);
    std::vector<float> rb(fix ? R : 0);
    outState_.resize(R);
    if (R && ldso_ba_get_residuals(ctx_, 0, nullptr, outState_.data(), nullptr, nullptr, nullptr, fl.data(), nullptr,
                                   fix ? rb.data() : nullptr)) {
        fail("ldso_ba_get_residuals");
        return false;
    }
    outStatePass_ = passes_;
    if (!readPointsAndThresholds(m, true)) return false;
    if (fix) {
        fix_.toRemove.clear();
        fix_.maxRelBS.assign(P, 0.f);
        fix_.numGood.assign(P, 0);
        fix_.lastState.assign(2 * P, -1);
        for (size_t q = 0; q < P; q++)
            for (int k = m.begin[q]; k < m.begin[q + 1]; k++) {
                const int t = m.target[k];
                if (t >= N - 2) fix_.lastState[2 * q + (N - 1 - t)] = outState_[k];
                if (!(fl[k] & LDSO_BA_FLAG_ACTIVE)) {
                    fix_.toRemove.push_back(m.res[k]);
                } else if (fl[k] & LDSO_BA_FLAG_NEW) {  // FullSystem.cc:1799-1813
                    fix_.maxRelBS[q] = std::max(fix_.maxRelBS[q], rb[k]);
                    fix_.numGood[q]++;
                }
            }
    }
    return true;
}

ResState EnergyFunctional::residualState(int k) {
    if (outStatePass_ != passes_ || resSync_ != ResSync::DeviceNewer) {  // not from the last pass
        if (resSync_ == ResSync::DeviceNewer && ldso_ba_get_residuals(ctx_, 0, nullptr, outState_.data(), nullptr,
                                                                      nullptr, nullptr, nullptr, nullptr, nullptr) == 0)
            outStatePass_ = passes_;
        else
            return loaded_.res[k]->state_state;  // the host copy is current
    }
    return (ResState)outState_[k];
}

const float *EnergyFunctional::residualCenter(int k) {
    if (resSync_ != ResSync::DeviceNewer) return loaded_.res[k]->centerProjectedTo;  // the host copy is current
    if (outCenterPass_ != passes_) {
        outCenter_.resize(3 * loaded_.res.size());
        if (ldso_ba_get_residuals(ctx_, 0, nullptr, nullptr, nullptr, nullptr, outCenter_.data(), nullptr, nullptr,
                                  nullptr)) {
            fail("ldso_ba_get_residuals");
            return loaded_.res[k]->centerProjectedTo;
        }
        outCenterPass_ = passes_;
    }
    return &outCenter_[3 * (size_t)k];
}

bool EnergyFunctional::setCoarseTrackingRef(ldso_ct_ctx *tracker, const ldso_ct_ctx *frame_src, double ab_exposure,
                                            double a, double b) {
    if (!tracker) {
        err_ = "setCoarseTrackingRef: null tracker";
        return false;
    }
    if (!ctx_) {
        if (err_.empty()) err_ = "setCoarseTrackingRef: no device context";
        return false;
    }
    // the library refuses a context that was loaded after its last pass (a rebuilt mirror)
    if (ldso_ct_make_reference_ba(tracker, frame_src, ctx_, 0, -1, ab_exposure, a, b, nullptr)) {
        fail("ldso_ct_make_reference_ba");
        return false;
    }
    return ok();
}

void EnergyFunctional::syncResiduals() { syncInto(loaded_); }

// m: the mirror of the window the device holds
void EnergyFunctional::syncInto(const Mirror &m) {
    // after a structural change the device's window is no longer the mirror's, unless the read-back
    // was deferred for an edit (structuralTouch): then the loaded window is still there to read
    if (resSync_ != ResSync::DeviceNewer || !ctx_ || (dirty_ && !deferred_)) return;
    resSync_ = ResSync::Synced;  // before the reads: the residual setters called below see it synced
    deferred_ = false;
    const auto t0 = std::chrono::steady_clock::now();
    readBacks_++;
    readBack(m);
    split_[1] += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
}

Vec3 EnergyFunctional::linearizeAll(bool fixLinearization) {
    Vec3 out = {0, 0, 0};
    epoch_++;
    if (!upload()) return out;
    if (ldso_ba_linearize(ctx_, fixLinearization ? 1 : 0, fixLinearization ? 0 : 1)) {
        fail("ldso_ba_linearize");
        return out;
    }
    passes_++;
    double e[3];
    if (ldso_ba_get_energy(ctx_, 0, e)) {
        fail("ldso_ba_get_energy");
        return out;
    }
    if (!readPassSummary(fixLinearization)) return out;
    resSync_ = ResSync::DeviceNewer;  // the residual objects' fields follow on demand (syncResiduals)
    if (!fixLinearization) resInA = (int)e[2];
    out = {e[0], e[1], e[2]};
    return out;
}

// One device pass (ldso_ba_linearize_residuals) relinearising every residual of the window from
// resetOOB; the entries serve PointFrameResidual::linearize until the next change of the window
bool EnergyFunctional::runRelinearization() {
    if (!upload()) return false;
    const size_t R = loaded_.res.size();
    cNewState_.assign(R, 0);
    cCenterOk_.assign(R, 0);
    cNewEnergy_.assign(R, 0.f);
    cEwo_.assign(R, 0.f);
    cCenter_.assign(3 * R, 0.f);
    cJp_.assign(8 * R, 0.f);
    if (R && ldso_ba_linearize_residuals(ctx_, 0, cNewState_.data(), cNewEnergy_.data(), cEwo_.data(), cCenter_.data(),
                                         cCenterOk_.data(), cJp_.data())) {
        fail("ldso_ba_linearize_residuals");
        return false;
    }
    passes_++;
    cSnap_.resize(4 * R);
    for (size_t k = 0; k < R; k++) {
        const PointHessian &p = *loaded_.resPoint[k];
        cSnap_[4 * k] = p.u;
        cSnap_[4 * k + 1] = p.v;
        cSnap_[4 * k + 2] = p.idepth_scaled;
        cSnap_[4 * k + 3] = p.idepth_zero_scaled;
    }
    cacheEpoch_ = epoch_;
    return true;
}

double EnergyFunctional::linearizeResidual(PointFrameResidual &r) {
    auto fresh = [&]() {
        if (dirty_ || cacheEpoch_ != epoch_ || r.mirrorIdx < 0 || (size_t)r.mirrorIdx >= cNewState_.size() ||
            loaded_.res[r.mirrorIdx] != &r)
            return false;
        const PointHessian &p = *loaded_.resPoint[r.mirrorIdx];
        const float *sn = &cSnap_[4 * (size_t)r.mirrorIdx];
        if (!(sn[0] == p.u && sn[1] == p.v && sn[2] == p.idepth_scaled && sn[3] == p.idepth_zero_scaled)) return false;
        // the frame terms the pass used: the residual's host and target as uploaded (state,
        // evaluation point, exposure, threshold) and the calibration -- a direct edit of either
        // without setDeltaF / setAdjointsF / linearizeAll in between is seen here
        if (std::memcmp(calibUp_, calib_.value_scaledf, sizeof(calibUp_)) != 0) return false;
        for (const auto &wf : {r.host, r.target}) {
            const auto f = wf.lock();
            if (!f) return false;
            const size_t i = (size_t)f->idx;
            if (i >= fsUp_.size() || i >= frames.size() || frames[i].get() != f.get()) return false;
            ldso_ba_frame_state fsn;
            frame_state(*f, fsn);
            if (std::memcmp(&fsn, &fsUp_[i], sizeof(fsn)) != 0 || f->frameEnergyTH != thUp_[i]) return false;
        }
        return true;
    };
    if (!fresh() && (!runRelinearization() || !fresh())) return r.state_energy;
    const size_t k = (size_t)r.mirrorIdx;
    const ResState ns = (ResState)cNewState_[k];
    r.state_NewState = ns;
    if (cCenterOk_[k]) std::memcpy(r.centerProjectedTo, &cCenter_[3 * k], 3 * sizeof(float));
    if (ns == OOB) return r.state_energy;  // Residuals.cc:59-63, 131-146: state_energy, NewEnergy kept
    r.state_NewEnergyWithOutlier = cEwo_[k];
    if (r.state_NewEnergy != (double)cNewEnergy_[k]) residualEdited();  // the device's NewEnergy follows
    r.state_NewEnergy = cNewEnergy_[k];
    if (ns == IN) std::memcpy(r.J_JpJdF, &cJp_[8 * k], sizeof(r.J_JpJdF));
    return r.state_NewEnergy;
}

// FullSystem::optimize's loop (FullSystem.cc:844-970) on the device; see the header
Vec3 EnergyFunctional::optimize(int n_its, shared_ptr<CalibHessian> HCalib, std::vector<Vec3> *energies,
                                bool *isLost, int *iterations, const ldso_ba_opt_settings *settings) {
    Vec3 out = {0, 0, 0};
    if (isLost) *isLost = false;
    if (iterations) *iterations = 0;
    if (nFrames < 2) return out;   // FullSystem.cc:846-851
    if (nFrames < 3) n_its = 20;
    if (nFrames < 4) n_its = 15;
    if (settings && !setSettings(*settings)) return out;
    epoch_++;
    calib_ = *HCalib;
    if (!upload()) return out;
    const std::vector<PointHessian *> &pts = loaded_.pts;
    const int N = nFrames, n = 8 * N + CPARS, P = (int)pts.size();
    std::vector<double> ns((size_t)7 * n), e((size_t)3 * (n_its + 1));
    if (ldso_ba_nullspaces(N, fs_.data(), ns.data())) {
        fail("ldso_ba_nullspaces");
        return out;
    }
    std::vector<ldso_ba_frame_state> fo(N);
    std::vector<float> idepth(P);
    double calib_out[4];
    int32_t its = 0, status = 0;
    if (ldso_ba_optimize(ctx_, n_its, &settings_, fs_.data(), HCalib->value, HCalib->value_zero, ns.data(), e.data(),
                         fo.data(), calib_out, idepth.data(), &its, &status)) {
        fail("ldso_ba_optimize");
        return out;
    }
    // the loop's exits: lost (FullSystem.cc:907-911) after its iterations (the state is that of
    // the step before), canbreak (:968-969); the passes the device ran: the first + one per step
    passes_ += 1 + (status == LDSO_BA_OPT_LOST ? its - 1 : its);
    if (isLost) *isLost = status == LDSO_BA_OPT_LOST;
    if (iterations) *iterations = its;
    // doStepFromBackup's results (FullSystem.cc:1843-1922) into the objects: frame states, the
    // calibration, every point's setIdepth / setIdepthZero
    for (int f = 0; f < N; f++) std::memcpy(frames[f]->state, fo[f].state, sizeof(fo[f].state));
    HCalib->setValue(calib_out);
    calib_ = *HCalib;
    for (int q = 0; q < P; q++) {
        pts[q]->setIdepth(idepth[q]);
        pts[q]->setIdepthZero(idepth[q]);
    }
    // setNewFrameEnergyTH of the loop's passes (the device holds it; the next frame-term upload
    // must not overwrite it with the old value)
    std::vector<float> th(N);
    if (ldso_ba_get_frame_energy_th(ctx_, 0, th.data())) {
        fail("ldso_ba_get_frame_energy_th");
        return out;
    }
    for (int f = 0; f < N; f++) frames[f]->frameEnergyTH = th[f];
    setDeltaF(HCalib);  // setPrecalcValues' setDeltaF after the last step: points' deltaF = 0
    // The frame terms are NOT marked uploaded: the next pass uses the host's FrameFramePrecalc /
    // takeData of the stepped states (the reference's setPrecalcValues), which differ from the
    // device's in libm's last ulp; upload() re-sends them in one staged launch.
    for (int q = 0; q < P; q++) {
        loaded_.vals[4 * q] = pts[q]->idepth_scaled;
        loaded_.vals[4 * q + 1] = pts[q]->idepth_zero_scaled;
        loaded_.vals[4 * q + 3] = pts[q]->deltaF;
    }
    resSync_ = ResSync::DeviceNewer;
    resInA = (int)e[3 * n_its + 2];
    if (energies)
        for (int s = 0; s <= n_its; s++) energies->push_back({e[3 * s], e[3 * s + 1], e[3 * s + 2]});
    out = {e[3 * n_its], e[3 * n_its + 1], e[3 * n_its + 2]};
    return out;
}

// EnergyFunctional.cc:280-471, non-VI branch: the stitched blocks of the last linearizeAll,
// HM / bM, the pose and scale nullspaces (FullSystem::getNullspaces) and the host LDL^T
void EnergyFunctional::solveSystemF(int iteration, double lambda, shared_ptr<CalibHessian> HCalib) {
    (void)HCalib;
    if (ldso_ba_check_settings(&settings_)) {  // the solver mode / vi_enable this branch implements
        fail("solveSystemF");
        return;
    }
    currentLambda_ = lambda;
    const int n = 8 * nFrames + CPARS;
    HA_top = MatXX(n, n);
    HL_top = MatXX(n, n);
    H_sc = MatXX(n, n);
    bA_top = VecX(n);
    bL_top = VecX(n);
    b_sc = VecX(n);
    if (ldso_ba_get_system(ctx_, 0, HA_top.data(), bA_top.data(), HL_top.data(), bL_top.data(), H_sc.data(),
                           b_sc.data())) {
        fail("ldso_ba_get_system");
        return;
    }
    std::vector<ldso_ba_frame_state> fs;
    packFrames(fs);
    std::vector<double> ns((size_t)7 * n);
    if (ldso_ba_nullspaces(nFrames, fs.data(), ns.data())) {
        fail("ldso_ba_nullspaces");
        return;
    }
    lastNullspaces_pose.assign(6, VecX(n));
    lastNullspaces_scale.assign(1, VecX(n));
    for (int k = 0; k < 7; k++)
        std::memcpy((k < 6 ? lastNullspaces_pose[k] : lastNullspaces_scale[0]).data(), &ns[(size_t)k * n],
                    n * sizeof(double));
    lastNullspaces_forLogging = lastNullspaces_pose;
    lastNullspaces_forLogging.push_back(lastNullspaces_scale[0]);
    lastX = VecX(n);
    if (ldso_ba_solve_system(&settings_, nFrames, iteration, lambda, HA_top.data(), bA_top.data(), HL_top.data(),
                             bL_top.data(), HM.data(), bM.data(), H_sc.data(), b_sc.data(), ns.data(), 7, lastX.data()))
        fail("ldso_ba_solve_system");
}

// EnergyFunctional.cc:611-667: calibration and frame steps are -x, point steps from the device
void EnergyFunctional::resubstituteF_MT(const VecX &x, shared_ptr<CalibHessian> HCalib, bool MT) {
    (void)MT;
    for (int k = 0; k < CPARS; k++) HCalib->step[k] = -x[k];
    for (const shared_ptr<FrameHessian> &h : frames) {
        for (int k = 0; k < 8; k++) h->step[k] = -x[CPARS + 8 * h->idx + k];
        h->step[8] = h->step[9] = 0;
    }
    std::vector<float> step(loaded_.pts.size());
    if (ldso_ba_resubstitute(ctx_, 0, x.data(), currentLambda_, step.data())) {
        fail("ldso_ba_resubstitute");
        return;
    }
    for (size_t q = 0; q < step.size(); q++) loaded_.pts[q]->step = step[q];
}

}  // namespace ldso_amd
