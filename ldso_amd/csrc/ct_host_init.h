// ct_host_init.h -- the coarse initializer: CoarseInitializer::setFirst and trackFrame (k_ct_init.h, ct_init.h).  Owns c->init.
// Reads frame.d_dIp / d_inten and the frame's exposure; snapshots them at ldso_ct_init_set_first.
// A piece of the one translation unit ldso_ct.hip (k_ct_pyramid.h).
#pragma once
#include <algorithm>
#include <cmath>
#include <cstring>
#include <string>
#include <vector>

#include "ldso_ba_internal.h"
#include "ct_context.h"

#pragma clang fp contract(off)

// the BA frame store's view of firstFrame's level 0 (ldso_ba_frame_put_initializer)
int ldso_ba::ct_init_frame_view(const ldso_ct_ctx *c, ldso_ba::CtFrameView *out) {
    if (!c || !out) return fail(-1, "null argument");
    out->intensity = c->init.d_inten.p;
    out->texels = c->init.d_first.p;
    out->width = c->pyr.w;
    out->height = c->pyr.h;
    out->device = c->device;
    out->stream = (void *)c->stream;
    out->have_frame = c->init.have_first;
    return 0;
}

namespace {

constexpr ldso_ct_init_params kInitDefaults = {2.5f * 2.5f, 150.f * 150.f, 0.8f, 1.0f, {5, 5, 10, 30, 50}, 1, 9.0f};

int init_check_params(const ldso_ct_init_params &p) {
    const float v[5] = {p.alpha_k, p.alpha_w, p.reg_weight, p.coupling_weight, p.huber_th};
    for (float x : v)
        if (!std::isfinite(x) || !(x > 0))
            return fail(-1, "alpha_k, alpha_w, reg_weight, coupling_weight and huber_th must be finite and > 0");
    for (int l = 0; l < 5; l++)
        if (p.max_iterations[l] < 0 || p.max_iterations[l] > ldso_ct::kInitMaxIterations)
            return fail(-1, "max_iterations out of range [0, 1000]");
    if (p.fix_affine != 0 && p.fix_affine != 1) return fail(-1, "fix_affine must be 0 or 1");
    return 0;
}

int init_check_ready(const ldso_ct_ctx *c) {
    if (!c) return fail(-1, "null context");
    if (!c->init.have_first) return fail(-1, "ldso_ct_init_set_first not called");
    if (!c->frame.have) return fail(-1, "ldso_ct_set_new_frame not called");
    return 0;
}

// the kernels' argument: the levels, the buffers and the carried state
void init_fill(const ldso_ct_ctx *c, const ldso_ct_init_params &p, CtInitParams &P) {
    P = CtInitParams{};
    const int *tab = c->init.d_tab.p;
    const double fx0 = c->fx[0], fy0 = c->fy[0], cx0 = c->cx[0], cy0 = c->cy[0];
    double fx = fx0, fy = fy0;
    for (int l = 0; l < c->levels; l++) {
        CtInitLevel &L = P.lv[l];
        L.pts = c->init.d_pts.p + c->init.off[l];
        L.ref = c->init.d_first.p + c->pyr.off[l];
        L.img = c->frame.d_dIp.p + c->pyr.off[l];
        L.order = tab + c->init.order_off[l];
        L.rank_off = tab + c->init.rank_off[l];
        L.child_off = tab + c->init.child_off[l];
        L.child = tab + c->init.child[l];
        L.n = c->init.off[l + 1] - c->init.off[l];
        L.n_ranks = c->init.n_ranks[l];
        L.wl = c->pyr.wl[l];
        L.hl = c->pyr.hl[l];
        // makeK (:811-837): fx, cx per level in double, fxl = the float of it
        if (l > 0) {
            fx = fx * 0.5;
            fy = fy * 0.5;
        }
        const double cx = l == 0 ? cx0 : (cx0 + 0.5) / ((int)1 << l) - 0.5;
        const double cy = l == 0 ? cy0 : (cy0 + 0.5) / ((int)1 << l) - 0.5;
        L.fxl = (float)fx;
        L.fyl = (float)fy;
        L.cxl = (float)cx;
        L.cyl = (float)cy;
        ldso_ct::init_make_ki(fx, fy, cx, cy, L.Ki);
    }
    P.p = p;
    P.jb[0] = c->init.d_jb.p;
    P.jb[1] = c->init.d_jb.p + (size_t)c->init.max_n * 10;
    P.jb_cur = c->init.jb_cur;
    P.levels = c->levels;
    std::memcpy(P.this_to_next, c->init.this_to_next, sizeof P.this_to_next);
    P.aff[0] = c->init.aff[0];
    P.aff[1] = c->init.aff[1];
    P.snapped = c->init.snapped;
    P.frame_id = c->init.frame_id;
    P.snapped_at = c->init.snapped_at;
    P.out = c->init.out.dev;
}

}  // namespace

extern "C" {

void ldso_ct_init_default_params(ldso_ct_init_params *p) {
    if (p) *p = kInitDefaults;
}

int ldso_ct_init_check_points(int32_t levels, int32_t width, int32_t height, const int32_t *n_per_level,
                              const ldso_ct_init_point *const *pts_per_level) {
    if (!n_per_level || !pts_per_level) return fail(-1, "null argument");
    if (levels < 1 || levels > ldso_ct::kInitMaxLevels) return fail(-1, "the initializer covers 1 to 5 pyramid levels");
    for (int l = 0; l < levels; l++) {
        if (n_per_level[l] < 1) return fail(-1, "every level needs at least one point (level " + std::to_string(l) + ")");
        if (!pts_per_level[l]) return fail(-1, "null point list (level " + std::to_string(l) + ")");
    }
    for (int l = 0; l < levels; l++) {
        const int n = n_per_level[l], wl = width >> l, hl = height >> l;
        const std::string at = " (level " + std::to_string(l) + ")";
        for (int i = 0; i < n; i++) {
            const ldso_ct_init_point &pt = pts_per_level[l][i];
            // the pattern reaches 2 pixels, and the first frame is interpolated there without a check
            if (!(pt.u >= 2 && pt.v >= 2 && pt.u + 2 < wl - 1 && pt.v + 2 < hl - 1))
                return fail(-1, "point " + std::to_string(i) + at + ": u, v must be finite and at least 2 pixels inside the interpolable area");
            for (int j = 0; j < 10; j++)
                if (pt.neighbours[j] < -1 || pt.neighbours[j] >= n)
                    return fail(-1, "point " + std::to_string(i) + at + ": neighbour " + std::to_string(j) + " is neither -1 nor in range");
            if (l == levels - 1) {
                if (pt.parent != -1) return fail(-1, "point " + std::to_string(i) + at + ": parent must be -1 on the top level");
            } else if (pt.parent < 0 || pt.parent >= n_per_level[l + 1]) {
                return fail(-1, "point " + std::to_string(i) + at + ": parent out of range of the next level");
            }
        }
    }
    return 0;
}

int ldso_ct_init_set_first(ldso_ct_ctx *c, const int32_t *n_per_level, const ldso_ct_init_point *const *pts_per_level) {
    if (!c) return fail(-1, "null context");
    if (!c->have_k) return fail(-1, "ldso_ct_make_k not called");
    if (!c->frame.have) return fail(-1, "ldso_ct_set_new_frame not called");
    int rc = ldso_ct_init_check_points(c->levels, c->pyr.w, c->pyr.h, n_per_level, pts_per_level);
    if (rc) return rc;
    HIP_TRY(hipSetDevice(c->device));
    const int Lv = c->levels;
    int off = 0, max_n = 0;
    for (int l = 0; l < Lv; l++) {
        c->init.off[l] = off;
        off += n_per_level[l];
        max_n = std::max(max_n, (int)n_per_level[l]);
    }
    c->init.off[Lv] = off;
    // the int table: per level the sweep order [n], the rank offsets [n_ranks + 1], and, for the level
    // above, the child offsets [n + 1] and the children [n of the level below]
    std::vector<int> tab;
    std::vector<ldso_ct_init_point> all((size_t)off);
    for (int l = 0; l < Lv; l++) {
        const int n = n_per_level[l];
        const ldso_ct_init_point *pts = pts_per_level[l];
        std::copy(pts, pts + n, all.begin() + c->init.off[l]);
        // rank = 1 + the largest rank among the adjacent points of smaller index; adjacent: one lists the other
        std::vector<int> rank(n, 0);
        for (int i = 0; i < n; i++) {
            for (int j = 0; j < 10; j++) {
                const int nb = pts[i].neighbours[j];
                if (nb >= 0 && nb < i) rank[i] = std::max(rank[i], rank[nb] + 1);
            }
            for (int j = 0; j < 10; j++) {
                const int nb = pts[i].neighbours[j];
                if (nb > i) rank[nb] = std::max(rank[nb], rank[i] + 1);
            }
        }
        const int n_ranks = *std::max_element(rank.begin(), rank.end()) + 1;
        std::vector<int> roff(n_ranks + 1, 0), order(n);
        for (int i = 0; i < n; i++) roff[rank[i] + 1]++;
        for (int r = 0; r < n_ranks; r++) roff[r + 1] += roff[r];
        std::vector<int> cur(roff.begin(), roff.end() - 1);
        for (int i = 0; i < n; i++) order[cur[rank[i]]++] = i;
        c->init.n_ranks[l] = n_ranks;
        c->init.order_off[l] = (int)tab.size();
        tab.insert(tab.end(), order.begin(), order.end());
        c->init.rank_off[l] = (int)tab.size();
        tab.insert(tab.end(), roff.begin(), roff.end());
        // the children of this level's points (the level below's, by parent, ascending)
        std::vector<int> coff(n + 1, 0), child;
        if (l > 0) {
            const int nc = n_per_level[l - 1];
            const ldso_ct_init_point *cp = pts_per_level[l - 1];
            child.resize(nc);
            for (int i = 0; i < nc; i++) coff[cp[i].parent + 1]++;
            for (int i = 0; i < n; i++) coff[i + 1] += coff[i];
            std::vector<int> cc(coff.begin(), coff.end() - 1);
            for (int i = 0; i < nc; i++) child[cc[cp[i].parent]++] = i;
        }
        c->init.child_off[l] = (int)tab.size();
        tab.insert(tab.end(), coff.begin(), coff.end());
        c->init.child[l] = (int)tab.size();
        tab.insert(tab.end(), child.begin(), child.end());
    }
    tab.push_back(0);  // never empty
    HIP_TRY(hipStreamSynchronize(c->stream));  // nothing reads the buffers a larger set replaces
    const size_t npx = c->pyr.off[Lv], px0 = (size_t)c->pyr.w * c->pyr.h;
    if ((rc = c->init.d_first.ensure(npx)) || (rc = c->init.d_inten.ensure(px0)) || (rc = c->init.d_pts.ensure(off)) ||
        (rc = c->init.d_tab.ensure(tab.size())) || (rc = c->init.d_jb.ensure((size_t)max_n * 20)) ||
        (rc = c->init.out.ensure(1)))
        return rc;
    c->init.have_first = false;
    HIP_TRY(hipMemcpyAsync(c->init.d_first.p, c->frame.d_dIp.p, npx * sizeof(float4), hipMemcpyDeviceToDevice, c->stream));
    HIP_TRY(hipMemcpyAsync(c->init.d_inten.p, c->frame.d_inten.p, px0 * sizeof(float), hipMemcpyDeviceToDevice, c->stream));
    HIP_TRY(hipMemcpyAsync(c->init.d_pts.p, all.data(), all.size() * sizeof all[0], hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipMemcpyAsync(c->init.d_tab.p, tab.data(), tab.size() * sizeof(int), hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipMemsetAsync(c->init.d_jb.p, 0, (size_t)max_n * 20 * sizeof(float), c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));  // the caller's lists may be reused on return
    c->init.max_n = max_n;
    c->init.jb_cur = 0;
    c->init.first_exposure = c->frame.exposure;
    const double eye[12] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0};
    std::memcpy(c->init.this_to_next, eye, sizeof eye);
    c->init.aff[0] = c->init.aff[1] = 0;
    c->init.snapped = c->init.frame_id = c->init.snapped_at = 0;  // setFirst, :730-732
    c->init.have_first = true;
    return 0;
}

int ldso_ct_init_rank_counts(ldso_ct_ctx *c, int32_t *out) {
    if (!c || !out) return fail(-1, "null argument");
    if (!c->init.have_first) return fail(-1, "ldso_ct_init_set_first not called");
    for (int l = 0; l < c->levels; l++) out[l] = c->init.n_ranks[l];
    return 0;
}

int ldso_ct_init_get_points(ldso_ct_ctx *c, int32_t lvl, ldso_ct_init_point *out, int32_t capacity, int32_t *n_out) {
    if (!c) return fail(-1, "null context");
    if (!c->init.have_first) return fail(-1, "ldso_ct_init_set_first not called");
    if (lvl < 0 || lvl >= c->levels) return fail(-1, "pyramid level out of range");
    const int n = c->init.off[lvl + 1] - c->init.off[lvl];
    if (n_out) *n_out = n;
    if (!out) return 0;
    if (capacity < n) return fail(-1, "capacity below the level's point count");
    HIP_TRY(hipSetDevice(c->device));
    return ct_read(c, out, c->init.d_pts.p + c->init.off[lvl], n);
}

int ldso_ct_init_set_points(ldso_ct_ctx *c, int32_t lvl, int32_t n, const ldso_ct_init_point *pts) {
    if (!c || !pts) return fail(-1, "null argument");
    if (!c->init.have_first) return fail(-1, "ldso_ct_init_set_first not called");
    if (lvl < 0 || lvl >= c->levels) return fail(-1, "pyramid level out of range");
    if (n != c->init.off[lvl + 1] - c->init.off[lvl]) return fail(-1, "n is not the level's point count");
    std::vector<ldso_ct_init_point> cur((size_t)n);
    int rc = ldso_ct_init_get_points(c, lvl, cur.data(), n, nullptr);
    if (rc) return rc;
    for (int i = 0; i < n; i++)
        if (pts[i].parent != cur[i].parent || std::memcmp(pts[i].neighbours, cur[i].neighbours, sizeof cur[i].neighbours) ||
            pts[i].u != cur[i].u || pts[i].v != cur[i].v)
            return fail(-1, "point " + std::to_string(i) + ": u, v and the tables must be the resident ones");
    HIP_TRY(hipMemcpyAsync(c->init.d_pts.p + c->init.off[lvl], pts, (size_t)n * sizeof *pts, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return 0;
}

int ldso_ct_init_eval(ldso_ct_ctx *c, int32_t lvl, const double ref_to_new[12], const double aff[2],
                      const ldso_ct_init_params *params, float H[64], float b[8], float Hsc[64], float bsc[8],
                      float res[3], int32_t *alpha_capped_out) {
    const ldso_ct_init_params p = params ? *params : kInitDefaults;
    int rc = init_check_params(p);
    if (rc) return rc;
    if ((rc = init_check_ready(c))) return rc;
    if (lvl < 0 || lvl >= c->levels) return fail(-1, "pyramid level out of range");
    if (!ref_to_new || !aff || !H || !b || !Hsc || !bsc || !res) return fail(-1, "null argument");
    HIP_TRY(hipSetDevice(c->device));
    CtInitParams P;
    init_fill(c, p, P);
    P.arg_lvl = lvl;
    std::memcpy(P.arg_pose, ref_to_new, sizeof P.arg_pose);
    P.arg_aff[0] = (float)aff[0];
    P.arg_aff[1] = (float)aff[1];
    k_ct_init_eval<<<1, kInitThreads, 0, c->stream>>>(P);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(c->stream));  // the results are in host memory already
    const CtInitOut &O = *c->init.out.p;
    std::memcpy(H, O.H, sizeof O.H);
    std::memcpy(b, O.b, sizeof O.b);
    std::memcpy(Hsc, O.Hsc, sizeof O.Hsc);
    std::memcpy(bsc, O.bsc, sizeof O.bsc);
    std::memcpy(res, O.res, sizeof O.res);
    if (alpha_capped_out) *alpha_capped_out = O.alpha_capped;
    return 0;
}

int ldso_ct_init_lm_step(const float H[64], const float b[8], const float Hsc[64], const float bsc[8], float lambda,
                         int32_t w, int32_t h, const double pose[12], const double aff[2],
                         const ldso_ct_init_params *params, float inc_out[8], double pose_out[12], double aff_out[2]) {
    if (!H || !b || !Hsc || !bsc || !pose || !aff || !inc_out || !pose_out || !aff_out) return fail(-1, "null argument");
    const ldso_ct_init_params p = params ? *params : kInitDefaults;
    if (int rc = init_check_params(p)) return rc;
    if (w < 1 || h < 1 || (long long)w * h > (1ll << 30)) return fail(-1, "bad level size");
    ldso_ct::LdltWorkF W;
    ldso_ct::Pose cand;
    const float a[2] = {(float)aff[0], (float)aff[1]};
    float an[2];
    ldso_ct::init_lm_step(H, b, Hsc, bsc, lambda, w, h, ldso_ct::init_pose_from_matrix(pose), a, p, W, inc_out, cand, an);
    ldso_ct::pose_matrix(cand, pose_out);
    aff_out[0] = an[0];
    aff_out[1] = an[1];
    return 0;
}

int ldso_ct_init_opt_reg(ldso_ct_ctx *c, int32_t lvl, float reg_weight, int32_t snapped) {
    if (!c) return fail(-1, "null context");
    if (!c->init.have_first) return fail(-1, "ldso_ct_init_set_first not called");
    if (lvl < 0 || lvl >= c->levels) return fail(-1, "pyramid level out of range");
    if (!std::isfinite(reg_weight)) return fail(-1, "reg_weight must be finite");
    HIP_TRY(hipSetDevice(c->device));
    CtInitParams P;
    init_fill(c, kInitDefaults, P);
    P.arg_lvl = lvl;
    P.arg_reg_weight = reg_weight;
    P.snapped = snapped != 0;
    k_ct_init_opt_reg<<<1, kInitThreads, 0, c->stream>>>(P);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(c->stream));
    return 0;
}

int ldso_ct_init_track_frame(ldso_ct_ctx *c, const ldso_ct_init_params *params, ldso_ct_init_result *result,
                             ldso_ct_init_step *trace, int32_t trace_capacity, int32_t *trace_n) {
    const ldso_ct_init_params p = params ? *params : kInitDefaults;
    int rc = init_check_params(p);
    if (rc) return rc;
    if ((rc = init_check_ready(c))) return rc;
    if (!result) return fail(-1, "null argument");
    if (trace && trace_capacity < 1) return fail(-1, "trace_capacity must be >= 1 with a trace");
    HIP_TRY(hipSetDevice(c->device));
    if (trace && (rc = ct_grow(c, c->init.trace, trace_capacity))) return rc;
    CtInitParams P;
    init_fill(c, p, P);
    // :71-73, the exposure-ratio guess; logf on the host, so that one libm serves every caller
    if (c->init.first_exposure > 0 && c->frame.exposure > 0) {
        P.have_guess = 1;
        P.aff_guess = logf(c->frame.exposure / c->init.first_exposure);
    }
    P.trace = trace ? c->init.trace.dev : nullptr;
    P.trace_capacity = trace ? trace_capacity : 0;
    k_ct_init_track<<<1, kInitThreads, 0, c->stream>>>(P);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(c->stream));  // result and trace are in host memory already
    const CtInitOut &O = *c->init.out.p;
    *result = O.R;
    int clock_khz = 0;  // of wall_clock64
    if (hipDeviceGetAttribute(&clock_khz, hipDeviceAttributeWallClockRate, c->device) != hipSuccess || clock_khz <= 0)
        clock_khz = 100000;
    for (int i = 0; i < 4; i++) result->phase_us[i] = (float)((double)O.ticks[i] * 1e3 / clock_khz);
    std::memcpy(c->init.this_to_next, O.R.this_to_next, sizeof O.R.this_to_next);
    c->init.aff[0] = (float)O.R.this_to_next_aff[0];
    c->init.aff[1] = (float)O.R.this_to_next_aff[1];
    c->init.snapped = O.R.snapped;
    c->init.frame_id = O.R.frame_id;
    c->init.snapped_at = O.R.snapped_at;
    c->init.jb_cur = O.jb_cur;
    if (trace) std::memcpy(trace, c->init.trace.p, (size_t)std::min(O.n_eval, trace_capacity) * sizeof *trace);
    if (trace_n) *trace_n = O.n_eval;
    return 0;
}

}  // extern "C"
