/*
 * ldso_ct.h -- C ABI of the MI355X-native coarse tracker.
 *
 * It replaces, for the GPU, the per-frame direct image alignment LDSO runs on every incoming
 * frame (reference paths relative to n-lalanne/LDSO):
 *
 *   FrameHessian::makeImages            src/internal/FrameHessian.cc:59-115  -> ldso_ct_set_new_frame
 *   CoarseTracker::makeK                src/frontend/CoarseTracker.cc:312-339 -> ldso_ct_make_k
 *   CoarseTracker::calcRes              src/frontend/CoarseTracker.cc:540-673 -> ldso_ct_calc_res
 *                                                                              (+ _batch: many poses)
 *   CoarseTracker::calcGSSSE            src/frontend/CoarseTracker.cc:675-741 -> ldso_ct_calc_gs
 *     with Accumulator9                 include/internal/OptimizationBackend/MatrixAccumulators.h:1104-1643
 *
 *   CoarseTracker::makeCoarseDepthL0    src/frontend/CoarseTracker.cc:357-538 -> ldso_ct_make_reference
 *                                                                              (+ _ba: from a BA pass)
 *   PixelSelector::makeMaps             src/frontend/PixelSelector2.cc:27-316 -> ldso_ct_select_pixels
 *   FullSystem::makeNewTraces           src/frontend/FullSystem.cc:1426-1482  -> ldso_ct_make_new_traces
 *                                                                              (setting_pointSelection 0)
 *   FeatureDetector::DetectCorners      src/frontend/FeatureDetector.cc:34-189 -> ldso_ct_detect_corners
 *     and makeNewTraces' loop over it   src/frontend/FullSystem.cc:1428-1438   (setting_pointSelection 1)
 *
 *   CoarseTracker::trackNewestCoarse    src/frontend/CoarseTracker.cc:61-310  -> ldso_ct_track
 *     one LM step of it on the host                                            (+ ldso_ct_lm_step)
 *   Undistort::undistort                src/frontend/Undistort.cc:190-230, 398-453 -> ldso_ct_set_new_frame_raw
 *     from the raw 8- / 16-bit image, makeImages behind it                     (+ _device; the tables' host
 *                                                                              helpers ldso_ct_undistort_make_*)
 *
 * The reference frame's point cloud (pc_u/pc_v/pc_idepth/pc_color per pyramid level) is built on
 * the device by ldso_ct_make_reference / ldso_ct_make_reference_ba, or handed over ready-made by
 * ldso_ct_set_reference.  trackNewestCoarse's LM loop (CoarseTracker.cc:61-310) runs on the device
 * in one call, ldso_ct_track; a caller that keeps the loop calls ldso_ct_calc_res_gs and
 * ldso_ct_lm_step exactly where the reference calls calcRes / calcGSSSE and solves its step.
 *
 * Conventions: poses are SE3 refToNew as a row-major 3x4 double matrix [R | t]
 * (Sophus::SE3::matrix3x4()); affine brightness parameters are AffLight (a, b) pairs;
 * exposures are FrameHessian::ab_exposure.  Outputs are the reference's types: calcRes returns
 * the Vec6 {E, numTermsInE, shiftT, 0, shiftRT, saturated fraction}; calcGSSSE the 8x8 H and
 * 8-vector b (row-major doubles) with the SCALE_* factors applied.
 *
 * Error convention as ldso_ba.h: 0 on success, < 0 on failure with ldso_ba_last_error() set.
 * A context is bound to one HIP device and stream; entry points are not re-entrant.
 */
#ifndef LDSO_CT_H_
#define LDSO_CT_H_

#include <stdint.h>
#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

#define LDSO_CT_MAX_LEVELS 6 /* PYR_LEVELS, NumTypes.h */

typedef struct ldso_ct_ctx ldso_ct_ctx;

/* CoarseTracker::CoarseTracker(w, h): level-0 size; the level count follows GlobalCalib's rule
 * (halve while both sides stay even and w*h > 5000, at most LDSO_CT_MAX_LEVELS;
 * src/internal/GlobalCalib.cc:20-30).  n_levels_out may be NULL. */
int ldso_ct_create(int32_t device, int32_t width, int32_t height, ldso_ct_ctx **out, int32_t *n_levels_out);
void ldso_ct_destroy(ldso_ct_ctx *ctx);

/* CoarseTracker::makeK (CoarseTracker.cc:312-339) from the level-0 fxl, fyl, cxl, cyl.
 * k_out (may be NULL): per level {fx, fy, cx, cy, Ki[9] row-major} = 13 floats. */
int ldso_ct_make_k(ldso_ct_ctx *ctx, const float calib[4], float *k_out);

/* FrameHessian::makeImages of the new frame on the device: level-0 intensities `color`
 * [height*width] -> dIp[lvl] = [I, dx, dy] and absSquaredGrad[lvl] for every level.
 * b_response: CalibHessian::B[256] for setting_gammaWeightsPixelSelect (NULL = identity,
 * i.e. no photometric calibration loaded).  ab_exposure: FrameHessian::ab_exposure. */
int ldso_ct_set_new_frame(ldso_ct_ctx *ctx, const float *color, double ab_exposure, const float *b_response);
/* read back level lvl of the new frame: dI [wl*hl][3], abs_sq_grad [wl*hl] (either may be NULL) */
int ldso_ct_get_frame_level(ldso_ct_ctx *ctx, int32_t lvl, float *dI, float *abs_sq_grad);

/* setCoarseTrackingRef's outputs: for each level, pc_n[lvl] points with pc_u, pc_v, pc_idepth,
 * pc_color (arrays of pointers, one per level), the reference frame's ab_exposure and
 * lastRef_aff_g2l (a, b). */
int ldso_ct_set_reference(ldso_ct_ctx *ctx, const int32_t *pc_n, const float *const *pc_u,
                          const float *const *pc_v, const float *const *pc_idepth,
                          const float *const *pc_color, double ref_ab_exposure, double ref_aff_a,
                          double ref_aff_b);

/* CoarseTracker::makeCoarseDepthL0 (CoarseTracker.cc:357-538) on the device: the cloud of every
 * level from n contributions, one per active point whose lastResiduals[0] targets the reference
 * frame with state IN, already filtered and in the reference's traversal order (frames in window
 * order, each frame's features in order): center [n][3] = r->centerProjectedTo, hdi [n] =
 * ph->HdiF.  The per-pixel sums of the scatter run in that order, so the cloud is the reference's
 * bit for bit.  A centre whose pixel (int(c[0] + 0.5f), int(c[1] + 0.5f)) falls outside
 * [0, w) x [0, h) -- the reference would write outside its arrays there, undefined behaviour --
 * contributes nothing, and nothing is ever read outside the maps.
 * frame_src: the tracker context whose current new frame (ldso_ct_set_new_frame) is the reference
 * keyframe, the source of pc_color = dIp[lvl][i][0]; NULL = ctx itself; another context (the
 * reference's coarseTracker_forNewKF / coarseTracker pair) must be on the same device and of the
 * same size, and is read on the device, ordered by events.
 * Leaves ctx as ldso_ct_set_reference does (the cloud, the exposure and affine pair, the warped
 * buffers invalidated).  pc_n_out (may be NULL): [levels] points per level.  The cloud and the
 * maps never leave the device: only the counts come back, behind one synchronisation. */
int ldso_ct_make_reference(ldso_ct_ctx *ctx, const ldso_ct_ctx *frame_src, int32_t n, const float *center,
                           const float *hdi, double ref_ab_exposure, double ref_aff_a, double ref_aff_b,
                           int32_t *pc_n_out);
/* The same from the last pass of a bundle-adjustment context, device to device (what
 * FullSystem::makeKeyFrame does after optimize, FullSystem.cc:613-621): the contributions are, for
 * the points of window `win` in the context's device point order (host frame, then point_rank),
 * each point's residual whose target is ref_frame (-1 = the window's last frame), if it exists and
 * its state is IN: its centre and the point's HdiF (the values ldso_ba_get_residuals /
 * ldso_ba_get_points return).  Refused (< 0): null arguments, another device, win or ref_frame out
 * of range, a marginalisation context, a context holding a shard of its points (a communicator of
 * more than one rank, or loaded with shard_count > 1), no pass since the context's last load, a
 * tracker frame size that differs from the window's images. */
struct ldso_ba_ctx;
int ldso_ct_make_reference_ba(ldso_ct_ctx *ctx, const ldso_ct_ctx *frame_src, const struct ldso_ba_ctx *ba,
                              int32_t win, int32_t ref_frame, double ref_ab_exposure, double ref_aff_a,
                              double ref_aff_b, int32_t *pc_n_out);
/* read back level lvl of the resident cloud, whichever call made it: out [n][4] = {u, v, idepth,
 * color}; *n_out = pc_n[lvl]; out may be NULL to query n. */
int ldso_ct_get_reference(ldso_ct_ctx *ctx, int32_t lvl, int32_t *n_out, float *out, int32_t capacity);

/* CoarseTracker::calcRes(lvl, refToNew, aff_g2l, cutoffTH) -> rs_out[6]; also keeps the warped
 * buffers on the device for the next ldso_ct_calc_gs (as the reference keeps buf_warped_*). */
int ldso_ct_calc_res(ldso_ct_ctx *ctx, int32_t lvl, const double ref_to_new[12], double aff_a, double aff_b,
                     float cutoff_th, double rs_out[6]);
/* calcRes for n_hyp poses at once (the motion hypotheses of FullSystem::trackNewCoarse,
 * FullSystem.cc:282-386): rs_out [n_hyp][6]; does not touch the warped buffers. */
int ldso_ct_calc_res_batch(ldso_ct_ctx *ctx, int32_t lvl, int32_t n_hyp, const double *ref_to_new,
                           const double *aff_ab, float cutoff_th, double *rs_out);
/* CoarseTracker::calcGSSSE(lvl, H, b, refToNew, aff_g2l) over the warped buffers of the last
 * ldso_ct_calc_res at this level.  H_out [8][8], b_out [8]. */
int ldso_ct_calc_gs(ldso_ct_ctx *ctx, int32_t lvl, const double ref_to_new[12], double aff_a, double aff_b,
                    double *H_out, double *b_out);
/* calcRes followed by calcGSSSE at the same pose (what trackNewestCoarse does at the start of
 * each level and for every LM step, CoarseTracker.cc:90-105, 218-245; a rejected step simply
 * ignores H and b): both launches
 * back to back on the context stream and one round trip; results equal the two separate calls. */
int ldso_ct_calc_res_gs(ldso_ct_ctx *ctx, int32_t lvl, const double ref_to_new[12], double aff_a, double aff_b,
                        float cutoff_th, double rs_out[6], double *H_out, double *b_out);
/* the warped buffers of the last calcRes, compacted in point order and zero-padded to a multiple
 * of 4 exactly as buf_warped_* / buf_warped_n: out [n][8] = {idepth, u, v, dx, dy, residual,
 * weight, refColor}; *n_out = buf_warped_n.  out may be NULL to query n. */
int ldso_ct_get_warped(ldso_ct_ctx *ctx, int32_t *n_out, float *out, int32_t capacity);

/* ---- trackNewestCoarse (CoarseTracker.cc:61-310): the coarse-to-fine LM loop, visual-only -------
 *
 * With setting_vi_enable false InertialCoarseTrackerHessian::compute zeroes its energy, H_I, H_I_sc
 * and b_I_sc and does nothing else (InertialCoarseTrackerHessian.cc:78-83); b_I, Hbb, Hab and bb keep
 * the zeros of their initialisers (InertialCoarseTrackerHessian.h:58-68), and update / restore return
 * at once.  What is left is the 8x8 system with bl = -b and resIOld = resINew = 0; the 15 zero rows
 * that Hbb appends to Hl get a zero increment from Eigen's LDLT.  The inertial terms are not covered.
 *
 * The solve.  The reference adds H into the *upper* triangle of a zero Hl and calls Hl.ldlt(), which
 * is LDLT<MatrixXd, Lower> and reads only the lower triangle: it factorises diag(Hl), so its step is
 * inc_i = -b_i / (H_ii (1 + lambda)) (the 6x6 / 7x7 / stitched sub-systems of the affine modes
 * likewise).  LDSO_CT_TRACK_SOLVE_REFERENCE is that step; LDSO_CT_TRACK_SOLVE_FULL, the default, is
 * the symmetric system upstream DSO / LDSO solve (Mat88 Hl = H), with the pivoted LDLT of
 * ldso_ba's solveSystemF.  lambda, the extrapolation factor, the cutoff repeat and AffLight's a, b
 * are float as in the reference; the ABI carries them widened. */
#define LDSO_CT_TRACK_SOLVE_FULL      0  /* the symmetric 8x8 system H(1+lambda on the diagonal), Eigen's pivoted LDLT */
#define LDSO_CT_TRACK_SOLVE_REFERENCE 1  /* what the reference's expression evaluates to: the diagonal step */

typedef struct ldso_ct_track_params {
    float   coarse_cutoff_th;          /* setting_coarseCutoffTH, 20 */
    double  lambda_increase;           /* setting_coarse_tracker_lambda_increase, 4.0 */
    double  lambda_decrease;           /* setting_coarse_tracker_lambda_decrease, 0.5 */
    float   affine_opt_mode_a, affine_opt_mode_b;   /* as ldso_ba_opt_settings */
    int32_t max_iterations[5];         /* 10, 20, 50, 50, 50; each in [1, 1000] */
    int32_t solve;                     /* LDSO_CT_TRACK_SOLVE_* */
} ldso_ct_track_params;
void ldso_ct_track_default_params(ldso_ct_track_params *p);

typedef struct ldso_ct_track_result {
    double  ref_to_new[12];            /* lastToNew_out (matrix3x4): the input pose after an abort (reason 1),
                                          which returns before the reference assigns it */
    double  aff[2];                    /* aff_g2l_out, with the final "< 0 -> 0" rule applied when ok; after an
                                          abort the input rounded to float, as AffLight holds it */
    double  last_residuals[5];         /* lastResiduals, NaN where a level was not reached */
    double  flow[3];                   /* lastFlowIndicators (1000 if no level finished) */
    int32_t ok;                        /* trackNewestCoarse's return value */
    int32_t reason;                    /* 0 ok, 1 residual above 1.5 * min_res_for_abort at abort_level,
                                          2 |a| / |b| too big, 3 relative affine too big */
    int32_t abort_level;               /* -1 = no abort */
    int32_t iterations[5];             /* LM iterations run per level, both visits of a repeated level summed */
    int32_t repeated_level;            /* -1 = none */
} ldso_ct_track_result;

typedef struct ldso_ct_track_step {    /* one calcRes evaluation of the loop, in program order */
    int32_t lvl, iteration;            /* iteration -1: the level's initial / cutoff-doubling evaluations */
    int32_t accepted;                  /* iteration >= 0 only */
    float   cutoff_th;                 /* the cutoff this evaluation used */
    double  lambda;                    /* the lambda the step was solved with (0 for iteration -1) */
    double  pose[12], aff[2];          /* what was evaluated */
    double  rs[6];                     /* its Vec6 */
    double  inc[8];                    /* the unscaled increment after extrapolation, iteration >= 0 only */
} ldso_ct_track_step;

/* n independent trackNewestCoarse runs on the context's new frame and reference cloud, one per start
 * (ref_to_new_in [n][12], aff_in [n][2], min_res_for_abort [n][5]), concurrently: one launch, one
 * workgroup per start, one synchronisation.  params NULL: the defaults.  trace (may be NULL): the
 * evaluations of start 0, at most trace_capacity, *trace_n = how many there were (trace_n may be NULL).
 * The sums of every evaluation are bitwise those ldso_ct_calc_res_gs returns at the same pose.
 * Two deviations from the reference's statements, both so that this loop and a host loop over
 * ldso_ct_calc_res_gs + ldso_ct_lm_step are one computation, bit for bit: an accepted pose is kept as
 * the matrix that was evaluated and becomes a quaternion again (Eigen's Quaternion(Matrix3)) for the
 * next step, where the reference keeps refToNew_new's quaternion; and SE3::exp's sine and cosine are
 * the library's own (ct_lm.h, correctly rounded but for an error near 1e-4 ulp) on host and device,
 * where the reference calls libm, whose last bit differs between glibc and the device library.
 * Refused (< 0): what ldso_ct_calc_res refuses, coarsest_lvl outside [0, min(levels, 5)), n < 1,
 * non-finite or non-positive params, an unknown solve, trace with trace_capacity < 1.
 * Leaves the warped buffers invalid, as ldso_ct_set_reference does. */
int ldso_ct_track(ldso_ct_ctx *ctx, int32_t n, const double *ref_to_new_in, const double *aff_in,
                  int32_t coarsest_lvl, const double *min_res_for_abort, const ldso_ct_track_params *params,
                  ldso_ct_track_result *out, ldso_ct_track_step *trace, int32_t trace_capacity, int32_t *trace_n);

/* one LM step on the host with the statements the kernel runs (context-free): solve, extrapolation,
 * scaling, the NaN guard, exp(inc) * pose, a/b update.  The pose enters through the matrix ABI
 * (Eigen's Quaternion(Matrix3)); the kernel takes each accepted pose through the same door, so a
 * host loop over ldso_ct_calc_res_gs and this call is ldso_ct_track's loop, evaluation for evaluation. */
int ldso_ct_lm_step(const double H[64], const double b[8], double lambda, const double pose[12],
                    const double aff[2], const ldso_ct_track_params *params,
                    double inc_out[8], double pose_out[12], double aff_out[2]);

/* ---- immature points: point creation and epipolar tracing ----------
 *
 *   ImmaturePoint::ImmaturePoint        src/internal/ImmaturePoint.cc:14-39   -> ldso_ct_make_immature
 *   ImmaturePoint::traceOn over all     src/internal/ImmaturePoint.cc:47-317  -> ldso_ct_trace
 *     immature points of all frames,    (FullSystem::traceNewCoarse,
 *     with the new frame                 src/frontend/FullSystem.cc:1157-1194)
 *
 * One record per ImmaturePoint (ImmaturePoint.h:101-121), 128 bytes.  `host` indexes the per-host
 * tables of ldso_ct_trace (traceNewCoarse's per-frame KRKi, Kt, aff).  The traced frame is the
 * context's new frame (ldso_ct_set_new_frame, level 0); ldso_ct_make_immature samples the same
 * frame, as makeNewTraces creates the points of the keyframe that was just made
 * (FullSystem.cc:1425-1475).  Where the reference would read outside the image (a rotated
 * pattern tap past the border: undefined behaviour there), both this path and the oracle clamp
 * the tap to the last interpolable texel. */
typedef struct ldso_ct_immature {
    float u, v;                  /* feature->uv */
    float idepth_min, idepth_max;
    float quality;
    float energy_th;             /* energyTH (NaN: a pattern colour was not finite) */
    float color[8];              /* pattern order: staticPattern[8], Setting.cc:275 */
    float weights[8];
    float grad_h[4];             /* gradH, row-major 2x2 */
    int32_t host;                /* index into ldso_ct_trace's host tables */
    int32_t last_status;         /* ImmaturePointStatus: GOOD 0, OOB 1, OUTLIER 2, SKIPPED 3,
                                    BADCONDITION 4, UNINITIALIZED 5 */
    float last_uv[2];            /* lastTraceUV */
    float last_interval;         /* lastTracePixelInterval */
    float type;                  /* my_type */
} ldso_ct_immature;

#define LDSO_CT_IPS_GOOD 0
#define LDSO_CT_IPS_OOB 1
#define LDSO_CT_IPS_OUTLIER 2
#define LDSO_CT_IPS_SKIPPED 3
#define LDSO_CT_IPS_BADCONDITION 4
#define LDSO_CT_IPS_UNINITIALIZED 5

/* new ImmaturePoint(newFrame, feat, type, HCalib) for n features at uv [n][2] on the context's
 * new frame: colour, weights, gradH and energyTH; idepth_min 0, idepth_max NaN, quality 10000,
 * status UNINITIALIZED, host = `host` for all n.  out: host memory [n]. */
int ldso_ct_make_immature(ldso_ct_ctx *ctx, int32_t n, const float *uv, float type, int32_t host,
                          ldso_ct_immature *out);
/* make the n records resident on the device (replaces the previous set) / read them back */
int ldso_ct_immature_upload(ldso_ct_ctx *ctx, int32_t n, const ldso_ct_immature *pts);
int ldso_ct_immature_download(ldso_ct_ctx *ctx, int32_t n, ldso_ct_immature *pts);
/* traceNewCoarse: traceOn of every resident record with the context's new frame.
 * krki [n_hosts][9] row-major, kt [n_hosts][3], aff [n_hosts][2] (AffLight::fromToVecExposure
 * host -> new frame), as traceNewCoarse builds them per host frame.
 * counts_out (may be NULL): [6] records per lastTraceStatus after the call (trace_good,
 * trace_oob, trace_out, trace_skip, trace_badcondition, trace_uninitialized). */
int ldso_ct_trace(ldso_ct_ctx *ctx, int32_t n_hosts, const float *krki, const float *kt, const float *aff,
                  int32_t *counts_out);

/* ---- pixel selection: where the new keyframe's immature points go ---------------------------
 *
 *   PixelSelector::makeHists / select / makeMaps   src/frontend/PixelSelector2.cc:27-316 -> ldso_ct_select_pixels
 *   FullSystem::makeNewTraces, pointSelection == 0  src/frontend/FullSystem.cc:1439-1461  -> ldso_ct_make_new_traces
 *
 * DSO's gradient-histogram selector on the context's new frame (levels 0-2 of the resident
 * pyramid), bit for bit: selection, sub-selection, the records and their ordered compaction run
 * on the device.  setting_pointSelection == 1, the reference's default, is ldso_ct_detect_corners
 * below; == 2 (OpenCV's RNG) is not covered.  The coarse initializer's calls
 * of makeMaps (th_factor 2, a density per level) are expressed by the parameters; nothing else of
 * the initializer is here.
 *
 * select() looks its threshold up at thsSmoothed[(x >> 5) + (y >> 5) * (w / 32)], which leaves the
 * grid makeHists fills when w or h is no multiple of 32: the strip right of the last whole block
 * reads the first block of the next block row (reproduced); the strip below the last block row,
 * and the right strip of that row, read entries the reference never writes (uninitialised memory
 * there).  Those entries are 0 here, and the array holds every index select can form.
 * Potentials above 32767 (the reference: undefined once the float leaves int's range) are 32767. */
typedef struct ldso_ct_select_params {
    float density;                          /* setting_desiredImmatureDensity / makeMaps' density */
    int32_t recursions;                     /* makeMaps' recursionsLeft */
    float th_factor;                        /* makeMaps' thFactor */
    float min_grad_hist_cut;                /* setting_minGradHistCut */
    float min_grad_hist_add;                /* setting_minGradHistAdd */
    float grad_downweight_per_level;        /* setting_gradDownweightPerLevel */
    int32_t select_direction_distribution;  /* setting_selectDirectionDistribution */
} ldso_ct_select_params;
/* Setting.cc:29, 83-87 and makeMaps' default arguments: 1500, 1, 1, 0.5, 7, 0.75, 1 */
void ldso_ct_select_default_params(ldso_ct_select_params *p);

/* PixelSelector::PixelSelector: random_pattern [width*height] is the selector's randomPattern (the
 * caller's, because the reference fills it from libc rand()), potential its currentPotential (the
 * constructor's 3; 1..32767).  The potential then persists from call to call as the member does;
 * ldso_ct_select_potential reads it.  Refused on a context with fewer than 3 pyramid levels or
 * with an image side of 16384 pixels or more. */
int ldso_ct_select_init(ldso_ct_ctx *ctx, const uint8_t *random_pattern, int32_t potential);
int ldso_ct_select_potential(ldso_ct_ctx *ctx, int32_t *out);

#define LDSO_CT_SELECT_STATS 7
/* makeMaps(newFrame, map_out, density, recursions, false, th_factor) on the context's new frame.
 * map_out (may be NULL): [width*height] 0 / 1 / 2 / 4 as the reference's float map.
 * stats_out (may be NULL): [LDSO_CT_SELECT_STATS] = makeMaps' return value, the last select's n2,
 * n3, n4, the potential that pass used, the potential left for the next frame, select passes run.
 * params NULL: the defaults.  Refused (< 0): no frame set, ldso_ct_select_init not called, density
 * not finite or <= 0, recursions < 0. */
int ldso_ct_select_pixels(ldso_ct_ctx *ctx, const ldso_ct_select_params *params, float *map_out, int32_t *stats_out);
/* makeMaps, then makeNewTraces' walk over x in [3, w-4), y in [3, h-4): one ImmaturePoint per
 * selected pixel at (x, y) with type = the map value and host = `host`, records whose energy_th is
 * not finite dropped, the survivors in the walk's row-major order in out [capacity] (host memory;
 * a copy, as with ldso_ct_make_immature: ldso_ct_immature_upload makes a set resident).
 * *n_out = the records made.  capacity too small: < 0 with *n_out = the count needed, nothing
 * written to out, and the potential put back to its value before the call, so that the retry
 * repeats the selection.  stats_out as above. */
int ldso_ct_make_new_traces(ldso_ct_ctx *ctx, const ldso_ct_select_params *params, int32_t host, int32_t capacity,
                            ldso_ct_immature *out, int32_t *n_out, int32_t *stats_out);

/* ---- corner detection: the reference's default point selection (setting_pointSelection == 1) ----
 *
 *   FeatureDetector::DetectCorners       src/frontend/FeatureDetector.cc:34-130
 *     ShiTomasiScore, IC_Angle           include/frontend/FeatureDetector.h:49-114
 *   FeatureDetector::ComputeDescriptor   src/frontend/FeatureDetector.cc:132-189
 *   FullSystem::makeNewTraces' loop      src/frontend/FullSystem.cc:1428-1438
 *
 * On level 0 of the context's new frame, in one call: the features in the reference's order (grid
 * cells gx outer, gy inner, each cell's picks by descending score), one ImmaturePoint (type 1) per
 * feature, and what loop closing later reads from the Feature: score, corner flag, angle, descriptor.
 *
 * Rules that are this library's, where the reference leaves the result open:
 *  - Ties.  DetectCorners orders a cell's candidates with std::sort, which leaves equal scores in an
 *    unspecified order.  Here the sort is stable: equal scores (-0 equals +0) keep candidate order
 *    (x outer, y inner), which is one of the reference's possible outcomes (libstdc++'s insertion
 *    sort for up to 16 elements is stable).  A score that is not finite (the square root of a
 *    discriminant that rounding made negative) makes the reference's comparator undefined; here it
 *    sorts after every number, in candidate order.
 *  - float -> int (the descriptor's tap offsets and `int t = intensity`): a value that is not finite
 *    or does not fit becomes INT_MIN, as x86's truncating conversion gives (undefined in C++).
 *  - A corner whose orientation patch holds a non-finite intensity has a NaN angle; its taps then fall
 *    outside the image in the reference (undefined); here a tap outside the 31 x 31 patch reads
 *    INT_MIN, so that corner's descriptor is 32 zero bytes.
 *  - The angle is (float)atan2((double)m_01, (double)m_10), where the reference calls atan2f, and the
 *    descriptor's rotation is (float)cos / sin of the double angle by the library's own sine and cosine
 *    (as ldso_ct_track's SE3::exp), where the reference calls cosf / sinf: libm's last bit differs
 *    between glibc and the device library, a double result rounded once does not, but for rare cases.
 *  - gridsize = int(sqrtf(w * h / n_features) + 0.5) outside [1, 30] is refused.  skip = 30 / gridsize
 *    + 1 cells are left out at each border, so the cells start at (30 / gridsize + 1) * gridsize >= 31
 *    and the last one ends at (w / gridsize - 30 / gridsize) * gridsize - 1 <= w - (30 / gridsize) *
 *    gridsize - 1.  For gridsize <= 30 that product is at least 16 (gridsize 16), which leaves the 15
 *    pixel orientation patch and the 13 pixel descriptor taps (|angle| <= pi, so the rotation is by
 *    at most 0.055 rad: |offset| < 13.8) inside the image; for gridsize > 30 it is 0, the last cells
 *    touch the border, and the reference's patch reads outside the image.
 */
typedef struct ldso_ct_feature {      /* Feature.h:86-90 */
    float   score;                     /* Shi-Tomasi score */
    float   angle;                     /* IC_Angle, 0 unless is_corner */
    int32_t is_corner;
    int32_t level;                     /* always 0 */
    uint8_t descriptor[32];            /* zeros unless is_corner */
} ldso_ct_feature;

/* bit_pattern: the ORB sampling table bit_pattern_31_ [256 * 4] (the caller's, as randomPattern is for
 * ldso_ct_select_init).  Refused: an entry outside [-13, 13], the table's range (see above). */
int ldso_ct_corners_init(ldso_ct_ctx *ctx, const int32_t *bit_pattern /* [1024] */);

#define LDSO_CT_CORNER_STATS 6
/* DetectCorners(n_features, frame) and makeNewTraces' loop on the context's new frame: recs_out
 * [capacity] the immature records (type 1, host = `host`; unlike ldso_ct_make_new_traces a record
 * whose energy_th is not finite is kept: mode 1 has no such filter), feat_out [capacity] the features'
 * score, corner flag, angle and descriptor, both in feature order (host memory).  *n_out = the features.
 * stats_out (may be NULL): [LDSO_CT_CORNER_STATS] = gridsize, picks per cell k = floor(nfeatInGrid)
 * + 1, candidates scored, features, corners, maxScore's bits.
 * capacity too small: < 0 with *n_out = the count needed, nothing written to recs_out / feat_out.
 * Refused (< 0): no frame set, ldso_ct_corners_init not called, n_features <= 0, gridsize < 1 or > 30.
 * Does not touch the pixel selector's state. */
int ldso_ct_detect_corners(ldso_ct_ctx *ctx, int32_t n_features, int32_t host, int32_t capacity,
                           ldso_ct_immature *recs_out, ldso_ct_feature *feat_out, int32_t *n_out,
                           int32_t *stats_out);

/* ---- activation candidates: which immature points become points ------------------------------
 *
 *   CoarseDistanceMap::makeDistanceMap / growDistBFS / addIntoDistFinal   src/frontend/CoarseTracker.cc:795-932
 *   FullSystem::activatePointsMT, the walk                                src/frontend/FullSystem.cc:1220-1298
 *
 * On level 1 (w1 = width >> 1, h1 = height >> 1, whatever the context's pyramid holds): the map of
 * growth steps to the nearest projected active point, then the walk over the resident immature
 * records that deletes, keeps or selects each for optimizeImmaturePoint, every accepted candidate
 * stamped into the map before the next one is looked at.  The result equals the sequential walk for
 * every input; the records never leave the device: ldso_ct_trace leaves them
 * resident, ldso_ba_activate_points_tracker (include/ldso_ba.h) reads the selection.
 * The policy part (FullSystem.cc:1199-1218: currentMinActDist from ef->nPoints) stays with the caller.
 *
 * Rules that are this library's:
 *  - float -> int (`int u = ptp[0] / ptp[2] + 0.5f`): a value that is not finite or does not fit
 *    becomes INT_MIN, as x86's truncating conversion gives (undefined in C++); it fails `u > 0`.
 *  - Frames whose level 1 has a side of 32768 pixels or more are refused. */

/* makeDistanceMap from n active points in host arrays: uvd [n][3] = PointHessian u, v, idepth_scaled,
 * host [n] the index of each point's host frame into krki1 [n_hosts][9] (K[1] R Ki[0], row-major) and
 * kt1 [n_hosts][3] (K[1] t), host -> newest frame in float as activatePointsMT builds them; the caller
 * leaves the newest frame's points out.  n_hosts in [1, 16].  The map and the tables stay in the context
 * for ldso_ct_select_activation.  map_out (may be NULL): [w1*h1] the map after makeDistanceMap, 1000
 * where no growth arrived. */
int ldso_ct_make_distance_map(ldso_ct_ctx *ctx, int32_t n_hosts, const float *krki1, const float *kt1, int32_t n,
                              const float *uvd, const int32_t *host, float *map_out);
/* The same with the seeds read on the device from window `win` of a bundle-adjustment context: every
 * point's u, v and current idepth (SCALE_IDEPTH is 1) of every host frame but `newest` (-1: the
 * window's last frame); n_hosts is the window's frame count.  Ordered with the BA context's stream by
 * events, not by the host.  Refused (< 0): another device, a marginalisation context, a context that
 * holds a shard of its points, a window whose image size differs from the tracker's. */
int ldso_ct_make_distance_map_ba(ldso_ct_ctx *ctx, const struct ldso_ba_ctx *ba, int32_t win, int32_t newest,
                                 const float *krki1, const float *kt1, float *map_out);

typedef struct ldso_ct_actsel_params {
    float current_min_act_dist;  /* currentMinActDist after the caller's update, in [0, 4] */
    float min_trace_quality;     /* setting_minTraceQuality */
    int32_t newest_host;         /* the host the walk skips; -1: none; -2: n_hosts - 1 */
} ldso_ct_actsel_params;
/* FullSystem.h's initial currentMinActDist, Setting.cc's setting_minTraceQuality, the last host */
#define LDSO_CT_ACTSEL_PARAMS_INIT {2.0f, 3.0f, -2}

#define LDSO_CT_ACT_KEEP 0
#define LDSO_CT_ACT_DELETE 1
#define LDSO_CT_ACT_OPTIMIZE 2
/* The walk of activatePointsMT over the n resident records, with the map and the tables of the last
 * distance-map call (refused without one).  Walk order: host ascending, and within a host the resident
 * order: the caller keeps each host's records in the host frame's feature order, as the reference
 * walks them.  flagged (may be NULL: none): [n_hosts] flaggedForMarginalization.  params NULL: the
 * defaults above.
 * disposition_out (may be NULL): [n] LDSO_CT_ACT_* per resident record; a record of newest_host is
 * KEEP and untouched.  selected_idx_out (may be NULL): room for n indices; the first *n_selected_out
 * are the OPTIMIZE records' resident indices in walk order.  Those records are copied, in that order,
 * to the context's selection, which ldso_ba_activate_points_tracker reads.  counts_out (may be NULL):
 * [4] = records kept, deleted, selected, and the kept ones that could activate but were too close.
 * compact != 0: the resident set becomes the KEEP records in their previous order (every OPTIMIZE
 * point leaves the immature set whatever its optimisation returns, FullSystem.cc:1313-1336), so
 * ldso_ct_immature_download then takes kept records; compact == 0 leaves the resident set untouched.
 * Refused (< 0): no distance map, current_min_act_dist outside [0, 4], newest_host out of range, a
 * resident record whose host is >= the map's n_hosts. */
int ldso_ct_select_activation(ldso_ct_ctx *ctx, const ldso_ct_actsel_params *params, const uint8_t *flagged,
                              int32_t compact, int32_t *disposition_out, int32_t *selected_idx_out,
                              int32_t *n_selected_out, int32_t *counts_out);
/* the last selection's n = *n_selected_out records, in walk order (a copy: tests and callers that
 * optimise on the host) */
int ldso_ct_selection_download(ldso_ct_ctx *ctx, int32_t n, ldso_ct_immature *pts);
/* n more records behind the resident set (the new keyframe's, after makeNewTraces): only they cross
 * the bus; the resident ones move on the device if the buffer has to grow. */
int ldso_ct_immature_append(ldso_ct_ctx *ctx, int32_t n, const ldso_ct_immature *pts);

/* kernel timing of the tracker's launches (same slots mechanism as ldso_ba); the selection's and the
 * corner detection's launches take no slot */
int ldso_ct_set_kernel_timing(ldso_ct_ctx *ctx, int32_t enable);
int ldso_ct_get_kernel_times(ldso_ct_ctx *ctx, double *ms, int64_t *counts, int32_t n);
const char *ldso_ct_kernel_name(int32_t i);
int32_t ldso_ct_num_kernels(void);

/* ---- the coarse initializer: CoarseInitializer::trackFrame on the device ----------------------
 *
 *   CoarseInitializer::trackFrame      src/frontend/CoarseInitializer.cc:45-183  -> ldso_ct_init_track_frame
 *     calcResAndGS, calculateAllResiduals, calculateAlphaEnergy, calculateSC  :186-518 -> ldso_ct_init_eval
 *     one LM step of it on the host    :95-116                                -> ldso_ct_init_lm_step
 *     calcEC, optReg, propagateUp / Down, resetPoints, doStep, applyStep      :520-631, 739-809
 *   CoarseInitializer::setFirst        :656-737, the state it leaves          -> ldso_ct_init_set_first
 *
 * The points and their neighbour / parent tables go up once, at ldso_ct_init_set_first; every frame is
 * then one call and one launch (one workgroup walks the levels and the LM iterations), and no image or
 * point record comes back unless the caller asks (ldso_ct_init_get_points).  The first frame's pyramid
 * is a device copy of the context's new frame, taken at set_first; ldso_ba_frame_put_initializer
 * (include/ldso_ba.h) hands its level 0 to the BA frame store.
 *
 * Parity target: the reference's multiThreading == false branch.  The true branch adds per-thread
 * accumulators in an order the scheduler picks and has no single answer: no parity claim.
 * Types follow the reference: points, H, b, lambda and the increment are float, poses double, and
 * SE3::exp(inc.head<6>().cast<double>()) is evaluated as written.  FP contraction is off.
 * Every per-point statement is the reference's, bit for bit.  The float sums (accE, accEAlpha, the 45
 * entries of acc9 and of acc9SC, calcEC's pair) have an order of this library's, the same in the loop
 * and in ldso_ct_init_eval and repeatable run to run (ct_init.h: a lane adds its points i = lane, lane +
 * 256, ... in order, each point's eight pattern terms first; a wave folds with the xor tree 32 ... 1;
 * the four waves add in order); they are not the reference's blocked SSE order and are only bounded
 * against it.  Two fixed-size Eigen reductions are written in their SSE packet order: doStep's
 * JbBuffer.head<8>().dot(inc) and inc.norm(), p_k = a_k b_k + a_(k+4) b_(k+4), (p_0 + p_2) + (p_1 + p_3).
 * Accumulator9::finish writes H(r, c) = H(c, r): both triangles of H and Hsc are filled, so Hl.ldlt()
 * (LDLT<., Lower>) factorises the full symmetric system here (unlike the coarse tracker's Hl, whose
 * lower triangle is empty).
 * The two doors of ldso_ct_track: an accepted pose is kept as the matrix that was evaluated and becomes
 * a quaternion again (Eigen's Quaternion(Matrix3)) for the next step, thisToNext is carried from call to
 * call as that matrix, and SE3::exp's sine and cosine are the library's own on host and device.
 * As in the reference, the LM loop tests `iteration >= max_iterations[lvl]` after a step: an entry of 0
 * still runs one step per level.
 * optReg and the top level's resetPoints are sequential in-place sweeps in the reference; here they run
 * rank by rank (rank = 1 + the largest rank among the points of smaller index that are the point's
 * neighbours or have it as a neighbour: kd-tree tables are not symmetric, and a point must also be swept
 * before a later one that it reads), with a barrier between ranks: the result equals the sequential
 * sweep for every input.  propagateUp adds each parent's children in child order.
 *
 * Not covered: setFirst's selection and makeNN (PixelSelector, makePixelStatus with its sparsityFactor,
 * nanoflann's kd-tree) stay on the host -- ldso_ct_select_pixels gives level 0's map,
 * ldso_ct_get_frame_level feeds makePixelStatus for the other levels, once per attempt; the inertial
 * path; multiThreading == true; FullSystem::initializeFromInitializer.  Contexts of more than 5 pyramid
 * levels are refused (maxIterations has five entries). */
typedef struct ldso_ct_init_point {    /* Pnt (CoarseInitializer.h:23-57), the fields trackFrame touches */
    float   u, v, idepth, ir, idepth_new;
    float   energy[2], energy_new[2];
    float   last_hessian, last_hessian_new, maxstep, outlier_th, my_type, ir_sum_num;
    int32_t is_good, is_good_new;
    int32_t parent;                    /* index in the next level; -1 on the top level */
    int32_t neighbours[10];            /* -1: none */
} ldso_ct_init_point;

typedef struct ldso_ct_init_params {
    float   alpha_k, alpha_w, reg_weight, coupling_weight;   /* 2.5^2, 150^2, 0.8, 1 */
    int32_t max_iterations[5];         /* 5, 5, 10, 30, 50; each in [0, 1000] */
    int32_t fix_affine;                /* fixAffine, 1 */
    float   huber_th;                  /* setting_huberTH, 9 */
} ldso_ct_init_params;
void ldso_ct_init_default_params(ldso_ct_init_params *p);

typedef struct ldso_ct_init_result {
    double  this_to_next[12];          /* thisToNext (matrix3x4) */
    double  this_to_next_aff[2];       /* thisToNext_aff */
    float   latest_res[3];
    int32_t snapped, frame_id, snapped_at;
    int32_t ret;                       /* trackFrame's return value */
    int32_t iterations[5];             /* LM steps per level */
    float   phase_us[4];               /* where the launch's time went, by the workgroup's own clock: the
                                          evaluations; the rank sweeps (optReg with propagateDown / Up, the top
                                          level's resetPoints); the other per-point phases; lane 0's decisions */
} ldso_ct_init_result;

typedef struct ldso_ct_init_step {     /* one calcResAndGS of the loop, in program order */
    double  pose[12], aff[2];          /* what was evaluated */
    int32_t lvl, iteration;            /* iteration -1: the level's first evaluation */
    int32_t accepted;                  /* iteration >= 0 only */
    int32_t alpha_capped;              /* alphaOpt == 0 */
    int32_t snapped;                   /* after this evaluation's decision */
    float   lambda;                    /* the lambda the step was solved with (0 for iteration -1) */
    float   inc[8];                    /* iteration >= 0 only */
    float   res[3];                    /* calcResAndGS's return value */
    float   reg_energy[3];             /* calcEC, iteration >= 0 only */
} ldso_ct_init_step;

/* setFirst's state from ready-made point lists (the caller's, as the ORB table is for
 * ldso_ct_corners_init): snapshots every level of the context's new frame and its exposure as firstFrame,
 * uploads pts_per_level[lvl][n_per_level[lvl]], resets thisToNext to the identity, thisToNext_aff to 0,
 * snapped, frameID and snappedAt to 0.  Refused (< 0) with a message: no frame or ldso_ct_make_k, more
 * than 5 levels, a level with n < 1, a neighbour that is neither -1 nor in range, a parent out of range
 * of the next level (or not -1 on the top level), u or v not finite or closer than 2 pixels to the
 * interpolable area's border (the pattern is read there without a check). */
int ldso_ct_init_set_first(ldso_ct_ctx *ctx, const int32_t *n_per_level, const ldso_ct_init_point *const *pts_per_level);
/* the list checks of ldso_ct_init_set_first alone (context-free), for a frame of width x height with
 * `levels` pyramid levels */
int ldso_ct_init_check_points(int32_t levels, int32_t width, int32_t height, const int32_t *n_per_level,
                              const ldso_ct_init_point *const *pts_per_level);
/* the records of level lvl as they stand; out may be NULL to query n */
int ldso_ct_init_get_points(ldso_ct_ctx *ctx, int32_t lvl, ldso_ct_init_point *out, int32_t capacity, int32_t *n_out);
/* overwrite the records of level lvl (n must be the level's count and the tables the resident ones):
 * for a caller that replays or edits a state */
int ldso_ct_init_set_points(ldso_ct_ctx *ctx, int32_t lvl, int32_t n, const ldso_ct_init_point *pts);
/* One calcResAndGS on the resident points against the context's new frame: writes the _new fields, maxstep
 * and JbBuffer_new as the reference does.  H, Hsc [8][8] row-major, b, bsc [8], res [3] = {E, alphaEnergy,
 * num}; alpha_capped_out may be NULL.  Bitwise what the loop of ldso_ct_init_track_frame computes at the
 * same pose and point state.  params NULL: the defaults. */
int ldso_ct_init_eval(ldso_ct_ctx *ctx, int32_t lvl, const double ref_to_new[12], const double aff[2],
                      const ldso_ct_init_params *params, float H[64], float b[8], float Hsc[64], float bsc[8],
                      float res[3], int32_t *alpha_capped_out);
/* lines :95-116 on the host with the statements the kernel runs (context-free): the damped, Schur-reduced,
 * wM-scaled float system, Hl.ldlt() in float (the 6x6 corner with fix_affine), exp(inc) * pose.  w, h: the
 * level's image size. */
int ldso_ct_init_lm_step(const float H[64], const float b[8], const float Hsc[64], const float bsc[8], float lambda,
                         int32_t w, int32_t h, const double pose[12], const double aff[2],
                         const ldso_ct_init_params *params, float inc_out[8], double pose_out[12], double aff_out[2]);
/* optReg(lvl) alone on the resident points, as if snapped were `snapped` */
int ldso_ct_init_opt_reg(ldso_ct_ctx *ctx, int32_t lvl, float reg_weight, int32_t snapped);
/* trackFrame on the context's new frame: one launch.  trace (may be NULL): every evaluation, at most
 * trace_capacity; *trace_n = how many there were (may be NULL).  params NULL: the defaults.
 * Refused: no ldso_ct_init_set_first, non-finite or non-positive params, iteration counts outside
 * [0, 1000], trace with trace_capacity < 1. */
int ldso_ct_init_track_frame(ldso_ct_ctx *ctx, const ldso_ct_init_params *params, ldso_ct_init_result *result,
                             ldso_ct_init_step *trace, int32_t trace_capacity, int32_t *trace_n);
/* ranks of the sweep per level (ldso_ct_init_set_first computed them): out [levels] */
int ldso_ct_init_rank_counts(ldso_ct_ctx *ctx, int32_t *out);

/* ---- frame ingestion: Undistort::undistort from the raw image (src/frontend/Undistort.cc) ----
 *
 *   PhotometricUndistorter::processFrame   Undistort.cc:190-230  \  one launch, k_ct_undistort, into the
 *   Undistort::undistort's remap loop      Undistort.cc:398-453  /  image ldso_ct_set_new_frame uploads
 *   Undistort::readFromFile's numeric part Undistort.cc:738-751, 802-868  -> ldso_ct_undistort_make_remap
 *   Undistort::makeOptimalK_crop           Undistort.cc:558-668              (host, no context)
 *   distortCoordinates of the five models  Undistort.cc:891-1125
 *   PhotometricUndistorter's tables        Undistort.cc:86-103, 120-154   -> ldso_ct_undistort_make_photometric
 *
 * A raw 8- or 16-bit frame goes to the device as the camera delivered it; the ImageAndExposure float
 * image, the pyramid and the BA frame store never exist on the host.  The image is the reference's bit
 * for bit (contraction off, every float statement in the reference's order); a NaN's sign and payload
 * are not part of that claim.
 *
 * The footprint rule.  The reference keeps a remap entry when iy < wOrg - 1 (Undistort.cc:860 tests the
 * width), so with hOrg < wOrg its blend reads past the source image.  As everywhere in this library the
 * reference's reads outside an array are not reproduced: ldso_ct_undistort_init stores an entry as
 * (-1, -1), whose output pixel is 0, when it is not finite or when its 2 x 2 footprint
 * [xxi, xxi + 1] x [yyi, yyi + 1] (xxi = (int)xx, yyi = (int)yy) is not inside the w_org x h_org source,
 * and counts it.  An entry with xx < 0 is the reference's own "write 0" mark: it is kept and not counted.
 * Nothing is ever read outside the source.
 *
 * Not built: the parsing of the calibration text, the photometric text and the vignette image (the
 * caller hands over numbers); benchmark_varNoise / benchmark_varBlurNoise (Undistort.cc:384-421,
 * 469-556), which draw from rand(); benchmarkSetting_* overrides; PhotometricUndistorter::unMapFloatImage;
 * makeOptimalK_full, where the reference asserts false. */
typedef struct ldso_ct_undistort_desc {
    int32_t w_org, h_org;       /* the raw image's size (>= 2 x 2) */
    const float *remap_x;       /* [height*width] at the context's size, source coordinates; both NULL: */
    const float *remap_y;       /*   passthrough (Undistort.cc:451-453), which needs w_org x h_org == the context's size */
    const float *g;             /* [g_depth] the response LUT G; NULL: no photometric calibration (valid == false) */
    int32_t g_depth;            /* >= 256 with g */
    const float *vignette_inv;  /* [h_org*w_org] vignetteMapInv; required with g (valid needs both) */
    int32_t photometric_mode;   /* setting_photometricCalibration: 0 factor * raw, 1 G[raw], 2 G[raw] * vignette_inv */
    int32_t use_exposure;       /* setting_useExposure */
} ldso_ct_undistort_desc;

/* The tables go to the device once.  n_outside_out (may be NULL): the entries the footprint rule stored
 * as -1.  Refused: null arguments, sizes below 2 x 2, g_depth < 256, g without vignette_inv, one remap
 * pointer without the other, passthrough with differing sizes, a mode outside 0..2. */
int ldso_ct_undistort_init(ldso_ct_ctx *ctx, const ldso_ct_undistort_desc *d, int32_t *n_outside_out);
/* Undistort::undistort(raw, exposure_time, ., factor) and makeImages of its image: raw [h_org*w_org] of
 * bits = 8 (uint8_t) or 16 (uint16_t) through pinned staging, k_ct_undistort, then the pyramid launches
 * of ldso_ct_set_new_frame.  *exposure_out (may be NULL): ImageAndExposure::exposure_time, that is
 * exposure_time, or 1 without use_exposure; it also becomes the new frame's ab_exposure.  factor applies
 * where the reference takes its first branch (no g, exposure_time <= 0 or mode 0).  Refused: before
 * ldso_ct_undistort_init; bits other than 8 / 16; 16 bits on the LUT branch unless g_depth == 65536. */
int ldso_ct_set_new_frame_raw(ldso_ct_ctx *ctx, const void *raw, int32_t bits, float exposure_time, float factor,
                              const float *b_response, float *exposure_out);
/* The same from device memory (a torch tensor, a capture card's DMA target) produced on producer_stream
 * (hipStream_t; NULL: the null stream): ordered by events in both directions, no host synchronisation,
 * as ldso_ba_frame_put_device.  dev_raw must stay alive until the stream work has run. */
int ldso_ct_set_new_frame_raw_device(ldso_ct_ctx *ctx, const void *dev_raw, int32_t bits, float exposure_time,
                                     float factor, const float *b_response, void *producer_stream,
                                     float *exposure_out);
/* the level-0 image of the new frame (either entry point's) as [height*width]: ImageAndExposure::image for
 * callers that still need it on the host (setting_pointSelection == 2, display) */
int ldso_ct_get_undistorted(ldso_ct_ctx *ctx, float *image);

enum { LDSO_CT_UNDISTORT_FOV = 0, LDSO_CT_UNDISTORT_RADTAN = 1, LDSO_CT_UNDISTORT_EQUIDISTANT = 2,
       LDSO_CT_UNDISTORT_KANNALA_BRANDT = 3, LDSO_CT_UNDISTORT_PINHOLE = 4 };
enum { LDSO_CT_UNDISTORT_OUT_CROP = 0, LDSO_CT_UNDISTORT_OUT_NONE = 1, LDSO_CT_UNDISTORT_OUT_CALIB = 2,
       LDSO_CT_UNDISTORT_OUT_FULL = 3 /* refused: the reference asserts false */ };
/* Host, no context: the remap tables and the rectified K the reference's Undistort constructor leaves.
 * pars: parsOrg as read from the first line {fx, fy, cx, cy, then omega (FOV) or four distortion
 * coefficients}; the relative format (cx < 1 and cy < 1) is rescaled as the reference does.  out_mode
 * CALIB: out_calib = the third line's {fx, fy, cx, cy}, relative to the output size (else may be NULL).
 * K_out: {fx, fy, cx, cy} of K, double as the reference's Mat33.  remap_x / remap_y [h*w]: the tables after
 * the "rounding resistant" pass, kept verbatim (iy == hOrg - 1 sets ix; the bound on iy is wOrg - 1), so
 * they are the reference's; ldso_ct_undistort_init applies the footprint rule.  *passthrough_out: 1 for
 * OUT_NONE (the tables are still written).  tanf / atanf / atan2f / sqrtf are the host libm's.
 * Refused: null arguments, an unknown model or mode, OUT_FULL, sizes below 2 x 2, OUT_NONE with differing
 * sizes, a crop search that does not end within 500 rounds (the reference exits). */
int ldso_ct_undistort_make_remap(int32_t model, const double pars[8], int32_t w_org, int32_t h_org, int32_t w, int32_t h,
                                 int32_t out_mode, const float out_calib[4], double K_out[4], float *remap_x,
                                 float *remap_y, int32_t *passthrough_out);
/* Host, no context: G [g_depth] and vignetteMapInv [n] from the numbers of the photometric text's first
 * line and the vignette image's pixels (vignette_bits 8: uint8_t, 16: uint16_t).  G: strictly increasing or
 * refused; 255.0 * (G[i] - min) / (max - min) in the reference's float / double mix; mode 0: the ramp
 * 255.0f * i / (g_depth - 1).  vignette_inv_out = 1.0f / (v / maxV): a zero pixel gives inf, which is kept. */
int ldso_ct_undistort_make_photometric(const float *g_raw, int32_t g_depth, const void *vignette, int32_t vignette_bits,
                                       int32_t n, int32_t photometric_mode, float *g_out, float *vignette_inv_out);

#ifdef __cplusplus
}
#endif

#endif
