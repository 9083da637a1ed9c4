// ldso_lc.hip -- the C ABI of include/ldso_lc.h: the loop closer's keyframe feature store and its three
// searches on the device.  Kernels: k_lc_*.h; the context: lc_context.h.  Every entry point ends with a
// synchronisation of the context's stream, so the staging buffers are free when it returns.
#include <cstring>
#include <string>

#include "../../include/ldso_ct.h"
#include "lc_context.h"

namespace {

constexpr int kLcMaxKeyframes = 65535;  // k_lc_brute's grid runs over the keyframes in y

int lc_blocks(int n) { return (n + kLcThreads - 1) / kLcThreads; }

// the slot of a stored keyframe, or -1 with the error set
int lc_find(ldso_lc_ctx *c, int64_t kf) {
    const auto it = c->by_id.find(kf);
    if (it == c->by_id.end()) {
        (void)fail(-1, "keyframe " + std::to_string((long long)kf) + " is not in the store");
        return -1;
    }
    return it->second;
}

// the slot a put builds in: a free one (there always is one: max_kf + 1 slots), or -1 when the store is full
// and kf is new
int lc_put_slot(ldso_lc_ctx *c, int64_t kf, int n) {
    if (kf < 0) return fail(-1, "negative keyframe id"), -1;
    if (n < 0 || n > c->F) return fail(-1, "feature count outside [0, max_features]"), -1;
    if (!c->by_id.count(kf) && c->n_stored >= c->max_kf) return fail(-1, "the keyframe store is full"), -1;
    for (size_t s = 0; s < c->slots.size(); s++)
        if (c->slots[s].kf < 0) return (int)s;
    return fail(-1, "no free slot"), -1;
}

// the features of `slot` are on the device (stream order): index them, and on success make the slot kf's
int lc_commit(ldso_lc_ctx *c, int64_t kf, int slot, int n) {
    int rc;
    if ((rc = c->idx_corner.ensure(std::max(n, 1)))) return rc;
    k_lc_index<<<1, kLcThreads, 0, c->stream>>>(c->S, slot, n, c->d_ckey.p, c->d_skey.p, c->idx_status.dev,
                                                 c->idx_corner.dev);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(c->stream));
    if (c->idx_status.p[kLcIdxBad]) return fail(-1, "a corner lies outside the feature grid");
    const auto old = c->by_id.find(kf);
    if (old != c->by_id.end()) {
        c->slots[old->second] = LcSlot();
        c->n_stored--;
    }
    LcSlot &s = c->slots[slot];
    s.kf = kf;
    s.n = n;
    s.corners = c->idx_status.p[kLcIdxCorners];
    s.bow_nodes = -1;
    s.bow_entries = 0;
    s.corner.assign(c->idx_corner.p, c->idx_corner.p + n);
    c->by_id[kf] = slot;
    c->n_stored++;
    return 0;
}

// a device array of n records to the caller: the count first, then the capacity rule
template <typename T>
int lc_download(ldso_lc_ctx *c, const T *dev, int n, int capacity, T *out, int32_t *n_out) {
    *n_out = n;
    if (n > capacity) return fail(-1, "capacity below the count (see *n_out)");
    if (n > 0) {
        HIP_TRY(hipMemcpyAsync(out, dev, (size_t)n * sizeof(T), hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(hipStreamSynchronize(c->stream));
    }
    return 0;
}

// k_lc_brute and k_lc_brute_emit of slot1 against the keyframes in h_pairs [n_kf]; the results stay on the device
int lc_brute(ldso_lc_ctx *c, int slot1, int n_kf, int th_low) {
    const int n1 = c->slots[slot1].corners;
    int rc;
    const size_t cells = (size_t)n_kf * std::max(n1, 1);
    if ((rc = c->d_pairs.ensure(n_kf)) || (rc = c->d_bf_idx.ensure(cells)) || (rc = c->d_bf_dist.ensure(cells)) ||
        (rc = c->d_matches.ensure(std::max(cells, (size_t)c->F))) || (rc = c->d_bf_counts.ensure(n_kf)))
        return rc;
    HIP_TRY(hipMemcpyAsync(c->d_pairs.p, c->h_pairs.p, (size_t)n_kf * sizeof(int2), hipMemcpyHostToDevice, c->stream));
    if (n1 > 0) {
        LcBfParams P{c->d_cdesc.p, c->d_cidx.p, c->d_pairs.p, c->d_bf_idx.p, c->d_bf_dist.p, slot1, n1, c->F, th_low};
        k_lc_brute<<<dim3((n1 + kLcBfThreads - 1) / kLcBfThreads, n_kf), kLcBfThreads, 0, c->stream>>>(P);
        HIP_TRY(hipGetLastError());
    }
    k_lc_brute_emit<<<n_kf, kLcThreads, 0, c->stream>>>(c->d_bf_idx.p, c->d_bf_dist.p,
                                                        c->d_cidx.p + (size_t)slot1 * c->F, n1, c->d_matches.p,
                                                        c->d_bf_counts.p);
    HIP_TRY(hipGetLastError());
    return 0;
}

// clear the map and write the n contributions of d_contrib into it
int lc_write_map(ldso_lc_ctx *c, int n) {
    HIP_TRY(hipMemsetAsync(c->d_map.p, 0, c->d_map.bytes(), c->stream));
    if (n > 0) {
        k_lc_map_write<<<lc_blocks(n), kLcThreads, 0, c->stream>>>(c->d_contrib.p, n, c->d_map.p, c->w, c->h);
        HIP_TRY(hipGetLastError());
    }
    return 0;
}

}  // namespace

extern "C" {

int ldso_lc_abi_version(void) { return LDSO_LC_ABI_VERSION; }

int ldso_lc_create(int32_t device, int32_t width, int32_t height, int32_t max_keyframes, int32_t max_features,
                   ldso_lc_ctx **out) {
    if (!out) return fail(-1, "null output pointer");
    *out = nullptr;
    if (width < kLcGrid || height < kLcGrid) return fail(-1, "image too small for one grid cell");
    if ((long long)width * height > (1ll << 30)) return fail(-1, "image too large");
    if (max_keyframes < 1 || max_keyframes > kLcMaxKeyframes) return fail(-1, "max_keyframes outside [1, 65535]");
    if (max_features < 1 || max_features > (1 << 20)) return fail(-1, "max_features outside [1, 2^20]");
    ldso_lc_ctx *c = new ldso_lc_ctx();
    c->device = device;
    hipError_t e = hipSetDevice(device);
    if (e == hipSuccess) e = hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking);
    if (e != hipSuccess) {
        delete c;
        return fail(-2, std::string("hip init: ") + hipGetErrorString(e));
    }
    c->w = width;
    c->h = height;
    c->max_kf = max_keyframes;
    c->F = max_features;
    const size_t S = (size_t)max_keyframes + 1, F = max_features;
    const int gw = width / kLcGrid, gh = height / kLcGrid, cells = gw * gh;
    c->slots.resize(S);
    int rc;
    if ((rc = c->d_feat.alloc(S * F)) || (rc = c->d_cdesc.alloc(S * F * 2)) || (rc = c->d_cidx.alloc(S * F)) ||
        (rc = c->d_cell_begin.alloc(S * (cells + 1))) || (rc = c->d_cell_feat.alloc(S * F)) ||
        (rc = c->d_bow_node.alloc(S * F)) || (rc = c->d_bow_begin.alloc(S * (F + 1))) ||
        (rc = c->d_bow_feat.alloc(S * F)) || (rc = c->h_feat.ensure(F)) || (rc = c->h_ints.ensure(3 * F + 2)) ||
        (rc = c->h_floats.ensure(F)) || (rc = c->d_ints.alloc(F)) || (rc = c->d_floats.alloc(F)) ||
        (rc = c->d_ckey.alloc(F)) || (rc = c->d_skey.alloc(F)) || (rc = c->idx_status.ensure(2)) ||
        (rc = c->idx_corner.ensure(F)) || (rc = c->h_pairs.ensure(max_keyframes)) || (rc = c->d_matches.alloc(F)) ||
        (rc = c->d_proj.alloc(F)) || (rc = c->count.ensure(1)) || (rc = c->d_map.alloc((size_t)width * height))) {
        const std::string why = ldso_ba::last_error();
        ldso_lc_destroy(c);
        return fail(rc, why);
    }
    c->S = LcStore{c->d_feat.p,     c->d_cdesc.p,     c->d_cidx.p,     c->d_cell_begin.p, c->d_cell_feat.p,
                   c->d_bow_node.p, c->d_bow_begin.p, c->d_bow_feat.p, (int)F,            cells,
                   gw,              gh,               width,           height};
    *out = c;
    return 0;
}

void ldso_lc_destroy(ldso_lc_ctx *c) {
    if (!c) return;
    (void)hipSetDevice(c->device);
    if (c->stream) (void)hipStreamSynchronize(c->stream);
    if (c->stream) (void)hipStreamDestroy(c->stream);
    delete c;  // every member frees what it owns: the work that used it has completed
}

int ldso_lc_keyframe_put(ldso_lc_ctx *c, int64_t kf, int32_t n, const ldso_lc_feature *feats) {
    if (!c || (n > 0 && !feats)) return fail(-1, "null argument");
    const int slot = lc_put_slot(c, kf, n);
    if (slot < 0) return -1;
    // SetFeatureGrid's index, checked before anything is stored (k_lc_index applies the same rule)
    const int gw = c->S.gw, gh = c->S.gh;
    for (int i = 0; i < n; i++) {
        if (!feats[i].is_corner) continue;
        const float u = feats[i].u, v = feats[i].v;
        const float gx = u / (float)kLcGrid, gy = v / (float)kLcGrid;
        if (!(u >= 0.0f && v >= 0.0f && gx < (float)gw && gy < (float)gh && (int)gx < gw && (int)gy < gh))
            return fail(-1, "corner " + std::to_string(i) + " lies outside the feature grid");
    }
    HIP_TRY(hipSetDevice(c->device));
    if (n > 0) {
        std::memcpy(c->h_feat.p, feats, (size_t)n * sizeof(ldso_lc_feature));
        HIP_TRY(hipMemcpyAsync(c->d_feat.p + (size_t)slot * c->F, c->h_feat.p, (size_t)n * sizeof(ldso_lc_feature),
                               hipMemcpyHostToDevice, c->stream));
    }
    return lc_commit(c, kf, slot, n);
}

int ldso_lc_keyframe_put_tracker(ldso_lc_ctx *c, int64_t kf, const ldso_ct_ctx *tracker) {
    if (!c || !tracker) return fail(-1, "null argument");
    ldso_ba::CtCornersView V{};
    int rc = ldso_ba::ct_corners_view(tracker, &V);
    if (rc) return rc;
    if (V.device != c->device) return fail(-1, "the tracker is on a different device");
    if (V.width != c->w || V.height != c->h) return fail(-1, "the tracker's frame size differs from the store's");
    if (V.n < 0) return fail(-1, "the tracker holds no complete detection: call ldso_ct_detect_corners first");
    const int n = V.n, slot = lc_put_slot(c, kf, n);
    if (slot < 0) return -1;
    HIP_TRY(hipSetDevice(c->device));
    if (n > 0) {
        // read the detection behind what the tracker's stream holds now; its later work waits for the read
        hipStream_t ts = static_cast<hipStream_t>(V.stream);
        if ((rc = c->borrow.begin(c->stream, ts))) return rc;
        k_lc_from_tracker<<<lc_blocks(n), kLcThreads, 0, c->stream>>>(
            V.pixel, V.pixel_stride, static_cast<const ldso_ct_feature *>(V.records), n, c->d_feat.p + (size_t)slot * c->F);
        HIP_TRY(hipGetLastError());
        if ((rc = c->borrow.end(c->stream, ts))) return rc;
    }
    return lc_commit(c, kf, slot, n);
}

}  // extern "C"

namespace {

__global__ __launch_bounds__(kLcThreads) void k_lc_update(ldso_lc_feature *__restrict__ feat, int n,
                                                          const float *__restrict__ inv_d,
                                                          const int *__restrict__ usable) {
    const int i = blockIdx.x * kLcThreads + threadIdx.x;
    if (i >= n) return;
    feat[i].inv_d = inv_d[i];
    feat[i].usable = usable[i] != 0 ? 1 : 0;
}

}  // namespace

extern "C" {

int ldso_lc_keyframe_update(ldso_lc_ctx *c, int64_t kf, int32_t n, const float *inv_d, const int32_t *usable) {
    if (!c || (n > 0 && (!inv_d || !usable))) return fail(-1, "null argument");
    const int slot = lc_find(c, kf);
    if (slot < 0) return -1;
    if (n != c->slots[slot].n) return fail(-1, "n differs from the keyframe's feature count");
    if (n == 0) return 0;
    HIP_TRY(hipSetDevice(c->device));
    std::memcpy(c->h_floats.p, inv_d, (size_t)n * sizeof(float));
    std::memcpy(c->h_ints.p, usable, (size_t)n * sizeof(int32_t));
    HIP_TRY(hipMemcpyAsync(c->d_floats.p, c->h_floats.p, (size_t)n * sizeof(float), hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipMemcpyAsync(c->d_ints.p, c->h_ints.p, (size_t)n * sizeof(int), hipMemcpyHostToDevice, c->stream));
    k_lc_update<<<lc_blocks(n), kLcThreads, 0, c->stream>>>(c->d_feat.p + (size_t)slot * c->F, n, c->d_floats.p,
                                                            c->d_ints.p);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(c->stream));
    return 0;
}

int ldso_lc_keyframe_set_bow(ldso_lc_ctx *c, int64_t kf, int32_t n_nodes, const int32_t *node_id,
                             const int32_t *node_begin, const int32_t *feat_idx) {
    if (!c || n_nodes < 0 || !node_begin || (n_nodes > 0 && !node_id)) return fail(-1, "bad arguments");
    const int slot = lc_find(c, kf);
    if (slot < 0) return -1;
    const LcSlot &s = c->slots[slot];
    if (n_nodes > c->F) return fail(-1, "more nodes than max_features");
    if (node_begin[0] != 0) return fail(-1, "node_begin[0] must be 0");
    for (int k = 0; k < n_nodes; k++) {
        if (k > 0 && node_id[k] <= node_id[k - 1]) return fail(-1, "node ids are not strictly ascending");
        if (node_begin[k + 1] < node_begin[k]) return fail(-1, "node_begin decreases");
    }
    const int entries = node_begin[n_nodes];
    if (entries > c->F) return fail(-1, "more entries than max_features");
    if (entries > 0 && !feat_idx) return fail(-1, "bad arguments");
    for (int e = 0; e < entries; e++) {
        if (feat_idx[e] < 0 || feat_idx[e] >= s.n) return fail(-1, "feature index " + std::to_string(e) + " out of range");
        if (!s.corner[feat_idx[e]]) return fail(-1, "feature index " + std::to_string(e) + " is not a corner");
    }
    HIP_TRY(hipSetDevice(c->device));
    const size_t F = c->F;
    int *h = c->h_ints.p;  // ids [n_nodes] | begins [n_nodes + 1] | indices [entries]
    if (n_nodes > 0) std::memcpy(h, node_id, (size_t)n_nodes * sizeof(int));
    std::memcpy(h + F, node_begin, ((size_t)n_nodes + 1) * sizeof(int));
    if (entries > 0) std::memcpy(h + 2 * F + 1, feat_idx, (size_t)entries * sizeof(int));
    if (n_nodes > 0)
        HIP_TRY(hipMemcpyAsync(c->d_bow_node.p + slot * F, h, (size_t)n_nodes * sizeof(int), hipMemcpyHostToDevice,
                               c->stream));
    HIP_TRY(hipMemcpyAsync(c->d_bow_begin.p + slot * (F + 1), h + F, ((size_t)n_nodes + 1) * sizeof(int),
                           hipMemcpyHostToDevice, c->stream));
    if (entries > 0)
        HIP_TRY(hipMemcpyAsync(c->d_bow_feat.p + slot * F, h + 2 * F + 1, (size_t)entries * sizeof(int),
                               hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    c->slots[slot].bow_nodes = n_nodes;
    c->slots[slot].bow_entries = entries;
    return 0;
}

int ldso_lc_keyframe_get(ldso_lc_ctx *c, int64_t kf, int32_t capacity, ldso_lc_feature *feats_out, int32_t *n_out) {
    if (!c || !n_out || capacity < 0 || (capacity > 0 && !feats_out)) return fail(-1, "bad arguments");
    const int slot = lc_find(c, kf);
    if (slot < 0) return -1;
    HIP_TRY(hipSetDevice(c->device));
    return lc_download(c, c->d_feat.p + (size_t)slot * c->F, c->slots[slot].n, capacity, feats_out, n_out);
}

int ldso_lc_keyframe_drop(ldso_lc_ctx *c, int64_t kf) {
    if (!c) return fail(-1, "null context");
    const int slot = lc_find(c, kf);
    if (slot < 0) return -1;
    c->slots[slot] = LcSlot();
    c->by_id.erase(kf);
    c->n_stored--;
    return 0;
}

int ldso_lc_search_brute_force(ldso_lc_ctx *c, int64_t kf1, int64_t kf2, int32_t th_low, int32_t capacity,
                               ldso_lc_match *matches_out, int32_t *n_out) {
    if (!c || !n_out || capacity < 0 || (capacity > 0 && !matches_out)) return fail(-1, "bad arguments");
    const int s1 = lc_find(c, kf1), s2 = s1 < 0 ? -1 : lc_find(c, kf2);
    if (s1 < 0 || s2 < 0) return -1;
    HIP_TRY(hipSetDevice(c->device));
    c->h_pairs.p[0] = make_int2(s2, c->slots[s2].corners);
    int rc = lc_brute(c, s1, 1, th_low);
    if (rc) return rc;
    int n = 0;
    HIP_TRY(hipMemcpyAsync(&n, c->d_bf_counts.p, sizeof(int), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return lc_download(c, c->d_matches.p, n, capacity, matches_out, n_out);
}

int ldso_lc_search_brute_force_many(ldso_lc_ctx *c, int64_t kf1, int32_t n_kf, const int64_t *kf_ids, int32_t th_low,
                                    int32_t *counts_out, int32_t *idx_out, int32_t *dist_out) {
    if (!c || n_kf < 0 || (n_kf > 0 && (!kf_ids || !counts_out))) return fail(-1, "bad arguments");
    if (n_kf > c->max_kf) return fail(-1, "more keyframes than the store holds");
    const int s1 = lc_find(c, kf1);
    if (s1 < 0) return -1;
    for (int k = 0; k < n_kf; k++) {
        const int s2 = lc_find(c, kf_ids[k]);
        if (s2 < 0) return -1;
        c->h_pairs.p[k] = make_int2(s2, c->slots[s2].corners);
    }
    if (n_kf == 0) return 0;
    HIP_TRY(hipSetDevice(c->device));
    int rc = lc_brute(c, s1, n_kf, th_low);
    if (rc) return rc;
    const size_t cells = (size_t)n_kf * c->slots[s1].corners;
    HIP_TRY(hipMemcpyAsync(counts_out, c->d_bf_counts.p, (size_t)n_kf * sizeof(int), hipMemcpyDeviceToHost, c->stream));
    if (idx_out && cells)
        HIP_TRY(hipMemcpyAsync(idx_out, c->d_bf_idx.p, cells * sizeof(int), hipMemcpyDeviceToHost, c->stream));
    if (dist_out && cells)
        HIP_TRY(hipMemcpyAsync(dist_out, c->d_bf_dist.p, cells * sizeof(int), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return 0;
}

int ldso_lc_search_by_bow(ldso_lc_ctx *c, int64_t kf1, int64_t kf2, int32_t th_low, float nn_ratio, int32_t capacity,
                          ldso_lc_match *matches_out, int32_t *n_out) {
    if (!c || !n_out || capacity < 0 || (capacity > 0 && !matches_out)) return fail(-1, "bad arguments");
    const int s1 = lc_find(c, kf1), s2 = s1 < 0 ? -1 : lc_find(c, kf2);
    if (s1 < 0 || s2 < 0) return -1;
    const LcSlot &a = c->slots[s1], &b = c->slots[s2];
    if (a.bow_nodes < 0 || b.bow_nodes < 0) return fail(-1, "a keyframe has no featVec: call ldso_lc_keyframe_set_bow");
    HIP_TRY(hipSetDevice(c->device));
    LcBowParams P{c->S, s1, s2, a.bow_nodes, b.bow_nodes, a.bow_entries, th_low, nn_ratio, c->d_matches.p, c->count.dev};
    k_lc_bow<<<1, kLcThreads, 0, c->stream>>>(P);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(c->stream));  // the count is in mapped host memory
    return lc_download(c, c->d_matches.p, c->count.p[0], capacity, matches_out, n_out);
}

int ldso_lc_make_idepth_map_ba(ldso_lc_ctx *c, const ldso_ba_ctx *ba, int32_t win, int32_t target_frame,
                               float *map_out) {
    if (!c) return fail(-1, "null context");
    if (!ba) return fail(-1, "null bundle-adjustment context");
    ldso_ba::BaRefView V;
    int rc = ldso_ba::ba_ref_view(ba, win, &V);
    if (rc) return rc;
    if (V.device != c->device) return fail(-1, "the bundle-adjustment context is on a different device");
    if (V.marg) return fail(-1, "a marginalisation context holds no active window");
    if (V.sharded) return fail(-1, "the context holds a shard of its points: the map needs the whole window");
    if (!V.have_pass) return fail(-1, "no linearisation pass has run since the context's last load");
    if (target_frame < -1 || target_frame >= V.N) return fail(-1, "target_frame out of range");
    if (V.width != c->w || V.height != c->h) return fail(-1, "the store's frame size differs from the window's images");
    if (target_frame < 0) target_frame = V.N - 1;
    HIP_TRY(hipSetDevice(c->device));
    const int n = V.R > 0 ? V.P : 0;
    if (n > 0) {
        if ((size_t)n > c->d_contrib.n) {
            HIP_TRY(hipStreamSynchronize(c->stream));  // nothing reads the old buffer any more
            if ((rc = c->d_contrib.alloc(n))) return rc;
        }
        // read the pass's arrays behind what the BA stream holds now; its later work waits for the read
        hipStream_t bs = static_cast<hipStream_t>(V.stream);
        if ((rc = c->borrow.begin(c->stream, bs))) return rc;
        HIP_TRY(hipMemsetAsync(c->d_contrib.p, 0xFF, (size_t)n * sizeof(float4), c->stream));  // NaN: no contribution
        LcGatherParams G{V.center, V.plane_stride, V.state, V.tgt, V.slot, c->d_contrib.p, V.R, V.P, V.rec_base, target_frame};
        k_lc_map_gather<<<lc_blocks(V.R), kLcThreads, 0, c->stream>>>(G);
        HIP_TRY(hipGetLastError());
        if ((rc = c->borrow.end(c->stream, bs))) return rc;
    }
    if ((rc = lc_write_map(c, n))) return rc;
    if (map_out) HIP_TRY(hipMemcpyAsync(map_out, c->d_map.p, c->d_map.bytes(), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    c->have_map = true;
    return 0;
}

int ldso_lc_make_idepth_map(ldso_lc_ctx *c, int32_t n, const float *centers) {
    if (!c || n < 0 || (n > 0 && !centers)) return fail(-1, "bad arguments");
    HIP_TRY(hipSetDevice(c->device));
    int rc;
    if (n > 0) {
        if ((size_t)n > c->d_contrib.n && (rc = c->d_contrib.alloc(n))) return rc;  // the stream is idle between calls
        if ((rc = c->h_contrib.ensure(n))) return rc;
        for (int i = 0; i < n; i++)
            c->h_contrib.p[i] = make_float4(centers[3 * (size_t)i], centers[3 * (size_t)i + 1], centers[3 * (size_t)i + 2], 0.f);
        HIP_TRY(hipMemcpyAsync(c->d_contrib.p, c->h_contrib.p, (size_t)n * sizeof(float4), hipMemcpyHostToDevice, c->stream));
    }
    if ((rc = lc_write_map(c, n))) return rc;
    HIP_TRY(hipStreamSynchronize(c->stream));
    c->have_map = true;
    return 0;
}

int ldso_lc_get_idepth_map(ldso_lc_ctx *c, float *map_out) {
    if (!c || !map_out) return fail(-1, "null argument");
    if (!c->have_map) return fail(-1, "no inverse-depth map: call ldso_lc_make_idepth_map first");
    HIP_TRY(hipSetDevice(c->device));
    HIP_TRY(hipMemcpyAsync(map_out, c->d_map.p, c->d_map.bytes(), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return 0;
}

int ldso_lc_search_by_projection(ldso_lc_ctx *c, int64_t kf_cur, int64_t kf_cand, const float *calib, const double *scr,
                                 float window_size, int32_t th_high, int32_t capacity, ldso_lc_projection *out,
                                 int32_t *n_out) {
    if (!c || !calib || !scr || !n_out || capacity < 0 || (capacity > 0 && !out)) return fail(-1, "bad arguments");
    if (!c->have_map) return fail(-1, "no inverse-depth map: call ldso_lc_make_idepth_map first");
    const int s_cur = lc_find(c, kf_cur), s_cand = s_cur < 0 ? -1 : lc_find(c, kf_cand);
    if (s_cur < 0 || s_cand < 0) return -1;
    HIP_TRY(hipSetDevice(c->device));
    LcProjParams P{};
    P.S = c->S;
    P.map = c->d_map.p;
    P.slot_cur = s_cur;
    P.slot_cand = s_cand;
    P.n_cand = c->slots[s_cand].n;
    P.th_high = th_high;
    std::memcpy(P.calib, calib, sizeof P.calib);
    std::memcpy(P.scr, scr, sizeof P.scr);
    P.window_size = window_size;
    P.out = c->d_proj.p;
    P.count = c->count.dev;
    k_lc_project<<<1, kLcThreads, 0, c->stream>>>(P);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(c->stream));  // the count is in mapped host memory
    return lc_download(c, c->d_proj.p, c->count.p[0], capacity, out, n_out);
}

}  // extern "C"
