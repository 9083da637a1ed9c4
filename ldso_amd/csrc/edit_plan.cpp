// edit_plan.cpp -- see edit_plan.h.  No HIP in here.
#include "edit_plan.h"

#include <cstring>
#include <string>

namespace ldso_ba {

void read_old(const WinHost &H, const WinDesc &D, OldWindow &o) {
    o.N = H.N;
    o.P = H.P;
    o.R = H.R;
    o.pt_pos.assign(o.P, -1);
    o.pt_host.assign(o.P, -1);
    for (int q = 0; q < o.P; q++) {
        o.pt_pos[H.pt_orig[q]] = q;
        o.pt_host[H.pt_orig[q]] = H.pt_host[q];
    }
    o.rs_pos.assign(o.R, -1);
    o.rs_point.assign(o.R, -1);
    o.rs_target.assign(o.R, -1);
    for (int pos = 0; pos < o.R; pos++) {
        // record slot rec_base + s * P + q: q the point's device position, s the target's slot
        // among the frames other than the host
        const int rel = H.rs_slot[pos] - D.rec_base, q = rel % o.P, s = rel / o.P, h = H.pt_host[q];
        const int k = H.rs_orig[pos];
        o.rs_pos[k] = pos;
        o.rs_point[k] = H.pt_orig[q];
        o.rs_target[k] = s < h ? s : s + 1;
    }
}

namespace {
// every src in [-1, n_old), no old index twice; counts the new entries
int check_src(const int32_t *src, int n, int n_old, const char *what, std::vector<int> &fresh) {
    std::vector<char> used(n_old, 0);
    fresh.clear();
    for (int i = 0; i < n; i++) {
        const int s = src[i];
        if (s == -1) {
            fresh.push_back(i);
            continue;
        }
        if (s < 0 || s >= n_old)
            return set_error(-1, std::string(what) + "_src[" + std::to_string(i) + "] = " + std::to_string(s) +
                                     " is not an index of the loaded window");
        if (used[s])
            return set_error(-1, std::string(what) + "_src names index " + std::to_string(s) + " of the loaded window twice");
        used[s] = 1;
    }
    return 0;
}
}  // namespace

int plan_edit(const WinHost &old_h, const WinDesc &old_d, const ldso_ba_edit &e, int item_order, int top_chunk,
              EditPlan &out) {
    if (!e.after || !e.frame_src) return set_error(-1, "edit: null after or frame_src");
    if (item_order == 2)
        return set_error(-1, "edit: LDSO_BA_TUNE_ITEM_ORDER 2 orders residuals by a float sort of the point records; "
                             "reload the window");
    if (old_h.P != old_h.P_all || old_h.R != old_h.R_all) return set_error(-1, "edit: the loaded window is sharded");
    const ldso_ba_window &a = *e.after;
    if (a.n_frames < 2 || a.n_frames > LDSO_BA_MAX_FRAMES) return set_error(-1, "n_frames out of range [2,16]");
    if (a.n_points < 0 || a.n_residuals < 0) return set_error(-1, "negative counts");
    if ((a.n_points > 0 && !e.point_src) || (a.n_residuals > 0 && !e.res_src))
        return set_error(-1, "edit: null point_src or res_src");
    OldWindow o;
    read_old(old_h, old_d, o);
    std::vector<int> new_frames;
    int rc;
    if ((rc = check_src(e.frame_src, a.n_frames, o.N, "frame", new_frames))) return rc;
    if ((rc = check_src(e.point_src, a.n_points, o.P, "point", out.new_pts))) return rc;
    if ((rc = check_src(e.res_src, a.n_residuals, o.R, "res", out.new_res))) return rc;
    if (!out.new_pts.empty() && !a.point_data) return set_error(-1, "edit: new points need point_data");
    if (!out.new_res.empty() && (!a.res_state || !a.res_energy || !a.res_flags))
        return set_error(-1, "edit: new residuals need res_state, res_energy and res_flags");

    // `after` as a load takes it: the caller's values at the new entries, placeholders at the carried
    // ones (the device keeps those; nothing of the layout depends on them in item order 0 and 1)
    std::vector<float> pd((size_t)a.n_points * LDSO_BA_POINT_STRIDE, 0.f), en(a.n_residuals, 0.f);
    std::vector<int8_t> st(a.n_residuals, LDSO_BA_RES_IN);
    std::vector<uint8_t> fl(a.n_residuals, 0);
    for (int p : out.new_pts)
        std::memcpy(&pd[(size_t)p * LDSO_BA_POINT_STRIDE], a.point_data + (size_t)p * LDSO_BA_POINT_STRIDE,
                    LDSO_BA_POINT_STRIDE * sizeof(float));
    for (int k : out.new_res) {
        st[k] = a.res_state[k];
        en[k] = a.res_energy[k];
        fl[k] = a.res_flags[k];
    }
    ldso_ba_window w = a;
    w.dI = nullptr;
    w.point_data = pd.data();
    w.res_state = st.data();
    w.res_energy = en.data();
    w.res_flags = fl.data();
    if ((rc = check_window(w, false))) return rc;

    // carried entries are the images of the old ones under frame_src and point_src
    std::vector<int> fmap(o.N, -1);  // old frame -> new index, -1 = removed
    for (int f = 0; f < a.n_frames; f++)
        if (e.frame_src[f] >= 0) fmap[e.frame_src[f]] = f;
    for (int p = 0; p < a.n_points; p++) {
        const int s = e.point_src[p];
        if (s < 0) continue;
        const int img = fmap[o.pt_host[s]];
        if (img < 0) return set_error(-1, "edit: point " + std::to_string(p) + " is carried from a removed frame");
        if (img != a.point_host[p])
            return set_error(-1, "edit: the host of carried point " + std::to_string(p) + " is not the image of its old host");
    }
    for (int p = 0; p < a.n_points; p++)
        for (int k = a.point_res_begin[p]; k < a.point_res_begin[p + 1]; k++) {
            const int s = e.res_src[k];
            if (s < 0) continue;
            if (e.point_src[p] != o.rs_point[s])
                return set_error(-1, "edit: carried residual " + std::to_string(k) + " is not on the image of its old point");
            const int img = fmap[o.rs_target[s]];
            if (img < 0) return set_error(-1, "edit: residual " + std::to_string(k) + " is carried into a removed frame");
            if (img != a.res_target[k])
                return set_error(-1, "edit: the target of carried residual " + std::to_string(k) +
                                         " is not the image of its old target");
        }

    if ((rc = build_layout(&w, 1, 0, 1, item_order, top_chunk, false, out.L, true))) return rc;
    const WinHost &H = out.L.wh[0];
    std::vector<int> rank_res(a.n_residuals, -1), rank_pt(a.n_points, -1);
    for (size_t i = 0; i < out.new_res.size(); i++) rank_res[out.new_res[i]] = (int)i;
    for (size_t i = 0; i < out.new_pts.size(); i++) rank_pt[out.new_pts[i]] = (int)i;
    out.rs_gather.resize(H.R);
    for (int pos = 0; pos < H.R; pos++) {
        const int k = H.rs_orig[pos], s = e.res_src[k];
        out.rs_gather[pos] = s >= 0 ? o.rs_pos[s] : ~rank_res[k];
    }
    out.pt_gather.resize(H.P);
    for (int q = 0; q < H.P; q++) {
        const int p = H.pt_orig[q], s = e.point_src[p];
        out.pt_gather[q] = s >= 0 ? o.pt_pos[s] : ~rank_pt[p];
    }
    return 0;
}

}  // namespace ldso_ba

namespace {
using namespace ldso_ba;
template <typename T>
bool same_bytes(const std::vector<T> &a, const std::vector<T> &b) {
    return a.size() == b.size() && (a.empty() || std::memcmp(a.data(), b.data(), a.size() * sizeof(T)) == 0);
}
template <typename T>
void copy_out(int32_t *dst, const std::vector<T> &v) {
    if (dst)
        for (size_t i = 0; i < v.size(); i++) dst[i] = (int32_t)v[i];
}
// the descriptor's integer fields and bases (the float fields follow from the window's frame terms alone)
bool same_desc(const WinDesc &a, const WinDesc &b) {
    return a.N == b.N && a.P == b.P && a.R == b.R && a.D == b.D && a.frame_base == b.frame_base && a.pair_base == b.pair_base &&
           a.point_base == b.point_base && a.res_base == b.res_base && a.top_item_base == b.top_item_base &&
           a.n_top_items == b.n_top_items && a.sc_item_base == b.sc_item_base && a.n_sc_items == b.n_sc_items && a.K == b.K &&
           a.KP == b.KP && a.ntiles == b.ntiles && a.p_all == b.p_all && a.sc_slab_base == b.sc_slab_base &&
           a.sys_base == b.sys_base && a.stage_base == b.stage_base && a.newest_begin == b.newest_begin &&
           a.newest_end == b.newest_end && a.rec_base == b.rec_base && a.vec_base == b.vec_base && a.width == b.width &&
           a.height == b.height && a.adt_diag == b.adt_diag;
}
}  // namespace

int ldso_ba::layout_index_mismatches(const Layout &L, const Layout &A) {
    const bool same[] = {same_bytes(L.top_items, A.top_items), same_bytes(L.sc_items, A.sc_items),
                         same_bytes(L.pair_items, A.pair_items), same_bytes(L.host_items, A.host_items),
                         same_bytes(L.sum_blocks, A.sum_blocks), same_bytes(L.pair_win, A.pair_win),
                         same_bytes(L.frame_win, A.frame_win), same_bytes(L.pt_win, A.pt_win),
                         same_bytes(L.rs_slot, A.rs_slot), same_bytes(L.pt_nres, A.pt_nres),
                         same_bytes(L.pt_host, A.pt_host), same_bytes(L.pt_tgt, A.pt_tgt),
                         same_bytes(L.rs_tgt, A.rs_tgt), same_bytes(L.wh[0].rs_orig, A.wh[0].rs_orig),
                         same_bytes(L.wh[0].pt_orig, A.wh[0].pt_orig), same_bytes(L.wh[0].rs_slot, A.wh[0].rs_slot),
                         same_desc(L.wd[0], A.wd[0]),
                         L.sc_slab_total == A.sc_slab_total && L.sys_total == A.sys_total &&
                             L.stage_total == A.stage_total && L.vec_total == A.vec_total && L.rec_base == A.rec_base &&
                             L.chunk == A.chunk && L.sc_chunk == A.sc_chunk && L.smem_max == A.smem_max};
    int bad = 0;
    for (bool s : same) bad += s ? 0 : 1;
    return bad;
}

extern "C" int ldso_ba_edit_plan_check(const ldso_ba_window *before, const ldso_ba_edit *e, int32_t item_order,
                                       int32_t top_chunk, int32_t *res_gather, int32_t *point_gather,
                                       int32_t *before_res_order, int32_t *before_point_order, int32_t *after_res_order,
                                       int32_t *after_point_order, int32_t *n_mismatch) {
    if (!before || !e) return set_error(-1, "bad arguments");
    Layout B;
    int rc = build_layout(before, 1, 0, 1, item_order, top_chunk, false, B, true);
    if (rc) return rc;
    EditPlan plan;
    if ((rc = plan_edit(B.wh[0], B.wd[0], *e, item_order, top_chunk, plan))) return rc;
    copy_out(res_gather, plan.rs_gather);
    copy_out(point_gather, plan.pt_gather);
    copy_out(before_res_order, B.wh[0].rs_orig);
    copy_out(before_point_order, B.wh[0].pt_orig);
    copy_out(after_res_order, plan.L.wh[0].rs_orig);
    copy_out(after_point_order, plan.L.wh[0].pt_orig);
    if (n_mismatch) {
        Layout A;
        if ((rc = build_layout(e->after, 1, 0, 1, item_order, top_chunk, false, A, true))) return rc;
        *n_mismatch = layout_index_mismatches(plan.L, A);
    }
    return 0;
}
