/* ldso_lc.h -- C ABI of the loop closer's matching on the device (gfx950): the keyframes' features kept
 * under the caller's ids, and the three searches the reference's loop closer runs over them (reference
 * paths relative to n-lalanne/LDSO):
 *
 *   FeatureMatcher::DescriptorDistance   src/frontend/FeatureMatcher.cc:16-33
 *   FeatureMatcher::SearchBruteForce     src/frontend/FeatureMatcher.cc:35-64    -> ldso_lc_search_brute_force
 *                                                                                  (+ _many: one keyframe against many)
 *   FeatureMatcher::SearchByBoW          src/frontend/FeatureMatcher.cc:66-124   -> ldso_lc_search_by_bow
 *   LoopClosing::ComputeOptimizedPose    src/frontend/LoopClosing.cc:264-295     -> ldso_lc_make_idepth_map (+ _ba)
 *     its correspondence search          src/frontend/LoopClosing.cc:313-398     -> ldso_lc_search_by_projection
 *   Frame::SetFeatureGrid / GetFeatureInGrid   src/Frame.cc:63-108 (gridSize 20, include/Frame.h:185)
 *   RxSO3 / Sim3 point action            thirdparty/Sophus/sophus/rxso3.hpp:259-267, sim3.hpp:228-231
 *
 * Everything here is integer work or arithmetic restated statement for statement (contraction off), so
 * every output is defined bit for bit and repeatable: no atomics, ordered compactions.
 *
 * What stays with the caller: DBoW3 (Frame::ComputeBoW, LoopClosing::DetectLoop; its featVec comes in
 * through ldso_lc_keyframe_set_bow), OpenCV's solvePnPRansac and the g2o Sim(3) refinement.
 *
 * This library's own rules, where the reference is undefined:
 *  - A corner outside SetFeatureGrid's grid (int(u / 20) >= w / 20, int(v / 20) >= h / 20 or a negative
 *    coordinate) is refused at put: the reference would index outside its grid, and DetectCorners never
 *    emits one.
 *  - A float -> int conversion of a value that is not finite or does not fit gives INT_MIN, as x86's
 *    truncating conversion does.  GetFeatureInGrid then returns nothing.  A NaN angle fails the angle gate.
 *  - A centre outside the image, a NaN or a hole writes nothing into the inverse-depth map (the reference
 *    would write outside its array).
 *  - The reference's "dilate idepth by 1" loop (LoopClosing.cc:297-310) runs over a vector that is never
 *    filled: it does nothing, and nothing is dilated here.
 *
 * Return convention: 0 on success, < 0 on failure; ldso_ba_last_error() (ldso_ba.h) gives the message.  A
 * context is bound to one HIP device and owns one stream; entry points are not re-entrant.  No call
 * touches the host state of a tracker or bundle-adjustment context: their device buffers are read behind
 * an event on their stream, and their later work waits for the read.
 */
#ifndef LDSO_LC_H_
#define LDSO_LC_H_

#include <stdint.h>
#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

#define LDSO_LC_ABI_VERSION 1
#define LDSO_LC_GRID_SIZE 20 /* Frame::gridSize, include/Frame.h:185 */

typedef struct ldso_lc_ctx ldso_lc_ctx;
struct ldso_ct_ctx;
struct ldso_ba_ctx;

int ldso_lc_abi_version(void);

/* what the loop closer reads of a Feature (Feature.h:81-90); 56 bytes */
typedef struct ldso_lc_feature {
    float   u, v;                      /* uv */
    float   angle;
    float   inv_d;                     /* invD, -1 until the map fills it in */
    int32_t is_corner;
    int32_t usable;                    /* status == VALID && point->status != OUTLIER */
    uint8_t descriptor[32];
} ldso_lc_feature;

/* Match (FeatureMatcher.h): feature indices into the two keyframes; 12 bytes */
typedef struct ldso_lc_match {
    int32_t index1, index2, dist;
} ldso_lc_match;

/* one accepted candidate of ldso_lc_search_by_projection; 80 bytes */
typedef struct ldso_lc_projection {
    int32_t index_cand, index_cur;     /* the candidate keyframe's feature, its partner in the current one */
    int32_t dist, reserved_;
    double  p_ref[3];                  /* matchedPoints */
    double  p_curr[3];                 /* matchedFeatures */
    double  pixel[2];                  /* matchedPixels */
} ldso_lc_projection;

/* width, height: wG[0], hG[0], at least LDSO_LC_GRID_SIZE each.  The store holds up to max_keyframes
 * keyframes of up to max_features features each. */
int ldso_lc_create(int32_t device, int32_t width, int32_t height, int32_t max_keyframes, int32_t max_features,
                   ldso_lc_ctx **out);
void ldso_lc_destroy(ldso_lc_ctx *ctx);

/* ---- the keyframe feature store ---------------------------------------------------------------------
 * kf is the caller's id (Frame::kfId), >= 0.  A put under an id the store holds replaces that keyframe.
 * Every put also builds SetFeatureGrid's cells (gw = w / 20, gh = h / 20; a cell holds its corners in
 * ascending feature index) and drops the keyframe's featVec.  A full store, an unknown id, n >
 * max_features and a corner outside the grid return < 0 and change nothing. */
int ldso_lc_keyframe_put(ldso_lc_ctx *ctx, int64_t kf, int32_t n, const ldso_lc_feature *feats);
/* device to device from the tracker's last ldso_ct_detect_corners: the pixel from its feature list, score
 * flag, angle and descriptor from its output records; inv_d = -1, usable = 0.  Refused: no detection (or
 * one whose capacity was too small), another device, another frame size. */
int ldso_lc_keyframe_put_tracker(ldso_lc_ctx *ctx, int64_t kf, const struct ldso_ct_ctx *tracker);
/* overwrite Feature::invD and the usable flag of every feature; n must be the keyframe's count */
int ldso_lc_keyframe_update(ldso_lc_ctx *ctx, int64_t kf, int32_t n, const float *inv_d, const int32_t *usable);
/* the keyframe's featVec as the caller's DBoW3 produced it: node_id [n_nodes] strictly ascending,
 * node_begin [n_nodes + 1] (0 first, non-decreasing), feat_idx [node_begin[n_nodes]] feature indices
 * (already through bowIdx) in the vector's order; at most max_features entries.  Refused: unsorted ids, an
 * index out of range or one that is not a corner. */
int ldso_lc_keyframe_set_bow(ldso_lc_ctx *ctx, int64_t kf, int32_t n_nodes, const int32_t *node_id,
                             const int32_t *node_begin, const int32_t *feat_idx);
/* *n_out = the keyframe's feature count; feats_out (may be NULL with capacity 0) receives them.  capacity
 * too small: < 0 with *n_out set, nothing written. */
int ldso_lc_keyframe_get(ldso_lc_ctx *ctx, int64_t kf, int32_t capacity, ldso_lc_feature *feats_out, int32_t *n_out);
int ldso_lc_keyframe_drop(ldso_lc_ctx *ctx, int64_t kf);

/* ---- SearchBruteForce ----------------------------------------------------------------------------------
 * Per corner i of kf1: the minimum DescriptorDistance over the corners j of kf2, the lowest j among equal
 * minima (the reference's strict < in ascending j), a match (i, j, dist) if dist < th_low.  Matches in
 * ascending i.  *n_out = the match count; capacity too small: < 0 with *n_out set, nothing written. */
int ldso_lc_search_brute_force(ldso_lc_ctx *ctx, int64_t kf1, int64_t kf2, int32_t th_low, int32_t capacity,
                               ldso_lc_match *matches_out, int32_t *n_out);
/* the same against n_kf stored keyframes in one launch.  counts_out [n_kf]: the match counts.  idx_out /
 * dist_out (each may be NULL): [n_kf][n1], n1 = the corners of kf1; entry c belongs to the c-th corner of
 * kf1 in ascending feature index and holds its partner's feature index in that keyframe, or -1 without a
 * match, and the minimum distance (9999, the reference's initial value, if that keyframe has no corner).
 * Every row equals the single-pair call bit for bit. */
int ldso_lc_search_brute_force_many(ldso_lc_ctx *ctx, int64_t kf1, int32_t n_kf, const int64_t *kf_ids, int32_t th_low,
                                    int32_t *counts_out, int32_t *idx_out, int32_t *dist_out);

/* ---- SearchByBoW ---------------------------------------------------------------------------------------
 * Per node present in both keyframes' featVec and per feature of kf1 in that node: best and second-best
 * distance over kf2's features of the node (both start at 256, the second-best counted with multiplicity),
 * the partner the first one at the minimum; accepted when best <= th_low and (float)best < nn_ratio *
 * (float)second.  Order: node id ascending, then kf1's order within the node.  Both keyframes need a
 * featVec (ldso_lc_keyframe_set_bow). */
int ldso_lc_search_by_bow(ldso_lc_ctx *ctx, int64_t kf1, int64_t kf2, int32_t th_low, float nn_ratio, int32_t capacity,
                          ldso_lc_match *matches_out, int32_t *n_out);

/* ---- ComputeOptimizedPose's correspondence search ------------------------------------------------------
 * The inverse-depth map of the current keyframe, kept in the context: 0 everywhere, then per contribution
 * (centerProjectedTo) in traversal order map[int(c[0] + 0.5f) + w * int(c[1] + 0.5f)] = c[2]; the last
 * writer of a pixel wins.
 * _ba: the contributions are the residuals of window win with target target_frame (-1: the last frame)
 * and state IN after the context's last pass, in device point order (frames in window order, then
 * point_rank: the reference's traversal).  Refused as ldso_ct_make_reference_ba refuses: another device, a
 * marginalisation context, a sharded one, no pass since the last load, a frame out of range, another
 * frame size.  map_out (may be NULL): [w * h]. */
int ldso_lc_make_idepth_map_ba(ldso_lc_ctx *ctx, const struct ldso_ba_ctx *ba, int32_t win, int32_t target_frame,
                               float *map_out);
/* the same from host centres [n][3] in traversal order */
int ldso_lc_make_idepth_map(ldso_lc_ctx *ctx, int32_t n, const float *centers);
/* the map of the last make call, [w * h] */
int ldso_lc_get_idepth_map(ldso_lc_ctx *ctx, float *map_out);

/* LoopClosing.cc:323-398 on kf_cand's usable features (in feature order) against kf_cur's grid and the
 * context's map.  calib [8]: fxl, fyl, cxl, cyl, fxli, fyli, cxli, cyli (value_scaledf / value_scaledi);
 * scr [7]: Sim(3) as Sophus holds it, the non-unit quaternion x, y, z, w (squared norm = scale), then the
 * translation.  The best partner is the minimum of (dist, ix, iy, index in cell), which is the reference's
 * strict < in its traversal order; accepted when best <= th_high (the reference's local TH_HIGH is 50, its
 * default window_size 5).  out [capacity] in candidate order; capacity too small: < 0 with *n_out set,
 * nothing written.  Refused: no map made yet. */
int ldso_lc_search_by_projection(ldso_lc_ctx *ctx, int64_t kf_cur, int64_t kf_cand, const float *calib /* [8] */,
                                 const double *scr /* [7] */, float window_size, int32_t th_high, int32_t capacity,
                                 ldso_lc_projection *out, int32_t *n_out);

#ifdef __cplusplus
}
#endif
#endif
