// marg_plan.cpp -- see marg_plan.h.  No HIP in here.
#include "marg_plan.h"

#include <cstring>
#include <string>

namespace ldso_ba {

int plan_marg(const WinHost &ph, const WinDesc &pd, const ldso_ba_window &frame_terms, int n_points,
              const int32_t *points, const uint8_t *res_live, int item_order, int top_chunk, MargPlan &out) {
    if (item_order == 2)
        return set_error(-1, "marginalisation from the device: LDSO_BA_TUNE_ITEM_ORDER 2 orders residuals by a float sort "
                             "of the point records; use ldso_ba_load_marginalization");
    if (ph.P != ph.P_all || ph.R != ph.R_all) return set_error(-1, "marginalisation from the device: the parent window is sharded");
    if (n_points < 0 || (n_points > 0 && !points)) return set_error(-1, "marginalisation from the device: bad point list");
    if (frame_terms.n_frames != ph.N) return set_error(-1, "marginalisation window does not match the parent window's frames");
    OldWindow o;
    read_old(ph, pd, o);
    // the parent's residual ranges: its caller order is point-major
    std::vector<int> begin(o.P + 1, 0);
    for (int k = 0; k < o.R; k++) begin[o.rs_point[k] + 1]++;
    for (int p = 0; p < o.P; p++) begin[p + 1] += begin[p];

    std::vector<char> used(o.P, 0);
    out.res_begin.assign(1, 0);
    out.res_parent.clear();
    out.res_target.clear();
    out.point_host.clear();
    for (int i = 0; i < n_points; i++) {
        const int p = points[i];
        if (p < 0 || p >= o.P)
            return set_error(-1, "points[" + std::to_string(i) + "] = " + std::to_string(p) + " is not a point of the parent window");
        if (used[p]) return set_error(-1, "points names point " + std::to_string(p) + " of the parent window twice");
        used[p] = 1;
        out.point_host.push_back(o.pt_host[p]);
        for (int k = begin[p]; k < begin[p + 1]; k++)
            if (!res_live || res_live[k]) {
                out.res_parent.push_back(k);
                out.res_target.push_back(o.rs_target[k]);
            }
        out.res_begin.push_back((int)out.res_parent.size());
    }
    const int R = (int)out.res_parent.size();

    // the selection as a load takes it; the values are placeholders (the device keeps them, and
    // nothing of the layout depends on them in item order 0 and 1)
    std::vector<float> pdata((size_t)n_points * LDSO_BA_POINT_STRIDE, 0.f), en(R, 0.f);
    std::vector<int8_t> st(R, LDSO_BA_RES_IN);
    std::vector<uint8_t> fl(R, 0);
    ldso_ba_window w = frame_terms;
    w.dI = nullptr;
    w.n_points = n_points;
    w.n_residuals = R;
    w.point_host = out.point_host.data();
    w.point_data = pdata.data();
    w.point_res_begin = out.res_begin.data();
    w.res_target = out.res_target.data();
    w.res_state = st.data();
    w.res_energy = en.data();
    w.res_flags = fl.data();
    w.point_rank = nullptr;
    int rc = build_layout(&w, 1, 0, 1, item_order, top_chunk, true, out.L, false);
    if (rc) return rc;
    const WinHost &H = out.L.wh[0];
    out.rs_gather.resize(H.R);
    for (int pos = 0; pos < H.R; pos++) out.rs_gather[pos] = o.rs_pos[out.res_parent[H.rs_orig[pos]]];
    out.pt_gather.resize(H.P);
    for (int q = 0; q < H.P; q++) out.pt_gather[q] = o.pt_pos[points[H.pt_orig[q]]];
    return 0;
}

}  // namespace ldso_ba

namespace {
using namespace ldso_ba;
template <typename T>
bool same_bytes(const std::vector<T> &a, const std::vector<T> &b) {
    return a.size() == b.size() && (a.empty() || std::memcmp(a.data(), b.data(), a.size() * sizeof(T)) == 0);
}
}  // namespace

extern "C" int ldso_ba_marg_plan_check(const ldso_ba_window *parent, int32_t n_points, const int32_t *points,
                                       const uint8_t *res_live, int32_t item_order, int32_t top_chunk,
                                       int32_t *res_gather, int32_t *point_gather, int32_t *n_res_out,
                                       int32_t *n_mismatch) {
    if (!parent) return set_error(-1, "bad arguments");
    Layout B;
    int rc = build_layout(parent, 1, 0, 1, item_order, top_chunk, false, B, true);
    if (rc) return rc;
    MargPlan plan;
    if ((rc = plan_marg(B.wh[0], B.wd[0], *parent, n_points, points, res_live, item_order, top_chunk, plan))) return rc;
    const int R = (int)plan.rs_gather.size();
    if (n_res_out) *n_res_out = R;
    if (res_gather && R) std::memcpy(res_gather, plan.rs_gather.data(), (size_t)R * sizeof(int32_t));
    if (point_gather && n_points) std::memcpy(point_gather, plan.pt_gather.data(), (size_t)n_points * sizeof(int32_t));
    if (n_mismatch) {
        // the explicit window: the selection written out from the caller's parent window alone (hosts,
        // ranges, targets and values; nothing of the plan), as a frontend packing it by hand would
        std::vector<float> pdata((size_t)n_points * LDSO_BA_POINT_STRIDE), en;
        std::vector<int8_t> st;
        std::vector<uint8_t> fl;
        std::vector<int32_t> host(n_points), begin(1, 0), target;
        for (int i = 0; i < n_points; i++) {
            const int p = points[i];
            host[i] = parent->point_host[p];
            std::memcpy(&pdata[(size_t)i * LDSO_BA_POINT_STRIDE], parent->point_data + (size_t)p * LDSO_BA_POINT_STRIDE,
                        LDSO_BA_POINT_STRIDE * sizeof(float));
            for (int k = parent->point_res_begin[p]; k < parent->point_res_begin[p + 1]; k++) {
                if (res_live && !res_live[k]) continue;
                target.push_back(parent->res_target[k]);
                st.push_back(parent->res_state[k]);
                en.push_back(parent->res_energy[k]);
                fl.push_back(parent->res_flags[k]);
            }
            begin.push_back((int32_t)target.size());
        }
        if ((int)target.size() != R) {  // the plan selected another number of residuals: every array differs
            *n_mismatch = 1 << 20;
            return 0;
        }
        ldso_ba_window w = *parent;
        w.dI = nullptr;
        w.n_points = n_points;
        w.n_residuals = R;
        w.point_host = host.data();
        w.point_data = pdata.data();
        w.point_res_begin = begin.data();
        w.res_target = target.data();
        w.res_state = st.data();
        w.res_energy = en.data();
        w.res_flags = fl.data();
        w.point_rank = nullptr;
        Layout A;
        if ((rc = build_layout(&w, 1, 0, 1, item_order, top_chunk, true, A, false))) return rc;
        const Layout &L = plan.L;
        // the gathered values are the explicit window's: state, energy, flags and records (priorF aside,
        // which the device scales) at the gather positions of the parent's layout
        bool values = true;
        for (int pos = 0; pos < R && values; pos++) {
            const int s = plan.rs_gather[pos];
            values = s >= 0 && s < (int)B.rs_state.size() && B.rs_state[s] == A.rs_state[pos] && B.rs_flags[s] == A.rs_flags[pos] &&
                     std::memcmp(&B.rs_energy[s], &A.rs_energy[pos], sizeof(float)) == 0;
        }
        for (int q = 0; q < n_points && values; q++) {
            const int s = plan.pt_gather[q];
            values = s >= 0 && s < (int)B.pt_host.size();
            for (int i = 0; i < LDSO_BA_POINT_STRIDE && values; i++) {
                float v = B.pt_data[(size_t)s * LDSO_BA_POINT_STRIDE + i];
                if (i == 4) v *= kIdepthFixPriorMargFac;
                values = std::memcmp(&v, &A.pt_data[(size_t)q * LDSO_BA_POINT_STRIDE + i], sizeof(float)) == 0;
            }
        }
        // ... the frame terms, which here come from frame_terms and not from an `after` window ...
        const bool same[] = {same_bytes(L.precalc, A.precalc), same_bytes(L.frame_th, A.frame_th), same_bytes(L.adH, A.adH),
                             same_bytes(L.adT, A.adT), std::memcmp(L.wd[0].calib, A.wd[0].calib, sizeof(A.wd[0].calib)) == 0,
                             std::memcmp(L.wd[0].cdelta, A.wd[0].cdelta, sizeof(A.wd[0].cdelta)) == 0, values};
        int bad = layout_index_mismatches(L, A);  // ... and every index array
        for (bool s : same) bad += s ? 0 : 1;
        *n_mismatch = bad;
    }
    return 0;
}
