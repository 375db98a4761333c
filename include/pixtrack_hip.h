/*
 * pixtrack_hip.h -- C ABI of the MI355X (gfx950) hot path of the pixtrack tracker.
 *
 * The reference (GiantAI/pixtrack) has no C ABI: its per-frame path is Python that
 * calls three third-party engines (pixloc's optimizer and UNet in PyTorch-CUDA, and
 * instant-ngp's Testbed through pyngp).  Each entry point below replaces ONE of the
 * Python-level interfaces that path goes through; the citation names the reference
 * line where pixtrack crosses that interface.  The Python host side
 * (the pixtrack_amd package) binds these with ctypes and keeps the reference's own
 * class/method names on top (INTEGRATION.md shows the stub a maintainer would add).
 *
 * Conventions
 *   - every pointer is a DEVICE pointer unless the name ends in _host (small records such as
 *     poses, cameras and configuration are read on the host and passed as kernel arguments);
 *   - the caller owns every buffer; the library keeps no reference after return
 *     (work is enqueued on `stream`; buffers must stay alive until it completes);
 *   - `stream` is a hipStream_t passed as void* (NULL = the default stream);
 *   - return value: 0 = enqueued OK; negative = PXT_E_* (argument / HIP error).
 *     Algorithmic failure of the optimiser (fewer than 10 valid points) is NOT an
 *     error: it is reported in the `failed` field of the output record, exactly like
 *     pixloc's `(T, failed)` return.
 *   - poses are 12 floats: row-major R (9) then t (3)   [pixloc Pose._data];
 *   - cameras are 10 floats: w,h,fx,fy,cx,cy,k1,k2,p1,p2 with the pixel-centre
 *     origin of pixloc Camera (cx,cy already shifted by -0.5), plus `ndist` in
 *     {0,2,4} saying how many distortion terms are live.
 *   - dense feature maps are HWC float32: map[(y*W + x)*cstride + c]; channels
 *     [0,C) are the descriptor, channel C is the confidence; cstride % 4 == 0 and
 *     cstride >= C+1.  Sparse reference features use the same record per point.
 */
#ifndef PIXTRACK_HIP_H
#define PIXTRACK_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PXT_OK 0
#define PXT_E_ARG -1     /* bad argument (null pointer, size, alignment) */
#define PXT_E_HIP -2     /* a HIP runtime call failed (pxt_last_error() has text) */
#define PXT_E_TIMEOUT -3 /* in-kernel spin bound exceeded (reported via status words) */
#define PXT_E_STATE -4   /* context misuse */
#define PXT_E_GUARD -5   /* pxt_lm_refine read a map tile its level's tile_flags call uncomputed (status word only) */

#define PXT_MAX_LEVELS 8
#define PXT_LM_LOG_STRIDE 20 /* floats per logged iteration, see pxt_lm_refine */

/* Library / device info ---------------------------------------------------- */
int pxt_version(void);               /* ABI version (13); bumps when an existing entry point's signature or a
                                        struct layout changes (added entry points and structs keep it) */
const char* pxt_last_error(void);    /* text of the last PXT_E_HIP on this thread */
int pxt_device_cus(int* n_cus_host); /* multiprocessor count of the current device */

/* -------------------------------------------------------------------------
 * Levenberg-Marquardt feature-metric pose refinement.
 *
 * Replaces, in one persistent launch and with no host round trip per iteration:
 *   for level in coarse..fine:  T, failed = opt[level].run(p3d, F_ref, F_q, T,
 *                                            camera.scale(s), W_ref_query=...)
 * i.e. pixloc BaseRefiner.refine_pose_using_features -> LearnedOptimizer._run,
 * reached from pixtrack/localization/pixloc_pose_refiners.py:260-262, with
 * pixtrack's early-stop-every-iteration rule
 * (pixtrack/optimizers/pixtrack_optimizer.py:5-18) and the per-iteration
 * masked-mean cost that DebugTracker logs (pixtrack/localization/tracker.py:32-46).
 * A single-level call (n_levels = 1) is exactly one `opt.run(...)`.
 * ---------------------------------------------------------------------- */
typedef struct {
  const float* fmap;   /* query map of this level, HWC, [h][w][cstride]; descriptor
                          channels already L2-normalised over C (A.4) */
  const float* fref;   /* reference observations [n_points][cstride]; descriptor
                          L2-normalised; channel C = reference confidence */
  int32_t h, w, C, cstride;
  float cam[10];       /* query camera ALREADY scaled to this level */
  int32_t ndist;
  float lambda[6];     /* damping 10^(lo + sigmoid(const)*(hi-lo)) of this level */
} pxt_lm_level;

typedef struct {
  int32_t num_iters;        /* per-level cap (pixloc_tracker_r9.py:47 -> 150) */
  int32_t pad;              /* interpolation border (pixloc_tracker_r9.py:48 -> 1) */
  int32_t loss;             /* 0 squared, 1 huber, 2 barron(alpha) */
  float loss_alpha;         /* barron alpha (0 = Cauchy-like) */
  float loss_scale;         /* pre/post scale `a` of pixloc scaled_loss */
  float grad_stop;          /* ||g|| < grad_stop            -> stop */
  float dt_stop, dR_stop;   /* dt < dt_stop AND dR(deg) < dR_stop -> stop */
  int32_t min_valid;        /* failed |= n_valid < min_valid (10) */
  int32_t n_workgroups;     /* persistent grid size; 0 = library default */
  int32_t spin_limit;       /* polls before an inter-workgroup wait gives up with PXT_E_TIMEOUT; 0 = library default
                               (2^22, seconds).  Tests force a time-out with 1. */
  int32_t path;             /* 0 = automatic: a level whose points fit the grid's lane groups keeps every point in
                               registers for the whole level (one round); 2 = always the general several-rounds path
                               (A/B, tests: both give the same poses to fp32 reduction order) */
} pxt_lm_conf;

/* Output record (device, floats):
 *   out[0..11]  T_refined (12)        out[12] failed (0/1)
 *   out[13]     status (0 ok, PXT_E_TIMEOUT as float if a spin bound tripped, PXT_E_GUARD if a level's tile guard did)
 *   out[14]     total iterations      out[15] 1.0, stored last with system-scope release
 *               (a host polling `out` in pinned memory may read the record once it sees it)
 *   out[16 + l] iterations run at level l (execution order), l < n_levels
 * Log (device, optional, may be NULL): log[(l*num_iters + i)*PXT_LM_LOG_STRIDE + k]
 *   k=0 masked-mean cost BEFORE the update of iteration i (tracker.py:40-41)
 *   k=1 number of valid points   k=2 dR (deg) of the step   k=3 dt of the step
 *   k=4 ||g||                    k=5 1 if the solve fell back from Cholesky to LU
 *   k=6 points that read an uncomputed tile (0 without tile_flags)
 *   k=8..19 pose after the update (12)
 */
int pxt_lm_refine(const float* p3d, const uint8_t* point_mask /* may be NULL */,
                  int32_t n_points, const pxt_lm_level* levels_host, int32_t n_levels,
                  const float* T_init_host /* 12 floats */, const pxt_lm_conf* conf_host,
                  float* out /* device, 16+PXT_MAX_LEVELS */, float* log /* device or NULL */,
                  void* workspace /* device, pxt_lm_workspace_bytes() */, void* stream);

/* pxt_lm_refine whose last act is the NEXT frame's camera: once the final pose stands, the kernel converts it
 * (get_camera_in_world_from_pixpose -> sfm_to_nerf_pose -> nerf_matrix_to_ngp, float64, pixtrack/utils/pose_utils.py:24,
 * pixtrack/utils/ingp_utils.py:47-63) and stores the 12 camera floats into up to two renderer camera slots
 * (pxt_ngp_camera_slot) and, optionally, a host-visible record cam_out13 (12 floats, then 1.0 stored last with
 * system-scope release; -1.0 instead, with the slots left untouched, when the refinement failed or timed out: the
 * camera record and the slots are valid only if out[12] == out[13] == 0).  A render enqueued behind this launch with pxt_ngp_render_frame(camera_from_slot = 1) then needs
 * no conversion launch of its own (pxt_ngp_render_both_from_pose's one-thread kernel).  cam_host == NULL: pxt_lm_refine. */
typedef struct {
  double conv27[27];   /* nerf2sfm centroid (3), 3 / avglen, R (4x4 row-major), totp (3), snapshot scale, offset (3) */
  float* cam_slot[2];  /* device float[12] each, or NULL */
  float* cam_out13;    /* pinned host or device float[13], or NULL */
} pxt_lm_camera;
int pxt_lm_refine_cam(const float* p3d, const uint8_t* point_mask, int32_t n_points, const pxt_lm_level* levels_host,
                      int32_t n_levels, const float* T_init_host, const pxt_lm_conf* conf_host, float* out, float* log,
                      void* workspace, const pxt_lm_camera* cam_host, void* stream);

/* pxt_lm_refine_cam with a tile guard on ONE level (guard_host == NULL: pxt_lm_refine_cam; cam_host may be NULL too).
 * That level's fmap was written in tiles of tile_rows x 16 texels, tiles_per_row of them per row of tiles, texel (0, 0)
 * of fmap being texel (tile_x0, tile_y0) of the tile grid, and only the tiles whose byte in tile_flags (device,
 * row-major) is 1 hold data - the query map of pxt_unet_forward_pair_tiles.  A valid point (an invalid one loads
 * nothing) whose 4 x 4 footprint box - columns ix0-1..ix0+2, rows iy0-1..iy0+2, clamped into the map as the loads are -
 * meets a tile with flag 0 is counted in the iteration's log word 6.  A non-zero count ends the launch at that
 * iteration, through the path a failed level takes: out[12] = 1, out[13] = PXT_E_GUARD, out[0..11] the pose that
 * iteration started from, the camera slots left alone and the camera record marked -1.  The count travels with the
 * iteration's other sums (accumulator slot 29): no atomics, barriers or exchanges of its own.  The batched launch and
 * every other reader of pxt_lm_level take no guard. */
typedef struct {
  int32_t level;              /* index into levels_host (execution order) */
  const uint8_t* tile_flags;  /* device */
  int32_t tile_rows, tiles_per_row, tile_x0, tile_y0;
} pxt_lm_tile_guard;
int pxt_lm_refine_guarded(const float* p3d, const uint8_t* point_mask, int32_t n_points, const pxt_lm_level* levels_host,
                          int32_t n_levels, const float* T_init_host, const pxt_lm_conf* conf_host, float* out, float* log,
                          void* workspace, const pxt_lm_camera* cam_host, const pxt_lm_tile_guard* guard_host, void* stream);

/* K independent refinements in ONE persistent launch - K objects tracked in lock-step on one GPU (BASELINE configs[3]:
 * the eight objects of /root/reference/config/<object>.sh, one tracker per object as
 * pixtrack/pose_trackers/pixloc_tracker_r9.py:287-318 builds it; on fewer than 8 GPUs a rank carries 8 / N of them).
 * Each problem is exactly one pxt_lm_refine_cam call - own points, levels, initial pose, output record, log, workspace
 * (pxt_lm_workspace_bytes() each, all different) and optional camera record - and is solved by its own share of the
 * grid: workgroup i works on problem i mod K, so the problems never wait for each other and an iteration's
 * inter-workgroup exchange and single-lane solve are paid once per iteration for all K.  conf_host is shared;
 * conf_host->n_workgroups is the grid PER PROBLEM; 0 = the library's default: 256 / K rounded down to a multiple of 8 (at
 * most 128), raised to what one round of 8-lane point groups needs for the largest problem (ceil(n_points / 64), a multiple
 * of 8, at most 128).  Either way the grid is then capped so that all K x n_workgroups workgroups are resident at once
 * (one 8-wave workgroup per CU).  A problem's result is bit-identical to pxt_lm_refine_cam with the same EFFECTIVE grid
 * (the fixed-order folds depend on the number of workgroups only): pass an explicit n_workgroups <= resident / K to pin it.  batch_workspace: device, pxt_lm_batch_workspace_bytes(K); it holds
 * the K parameter records, copied there from pinned staging memory ahead of the launch in `stream`. */
#define PXT_LM_MAX_BATCH 16
typedef struct {
  const float* p3d;
  const uint8_t* point_mask; /* may be NULL */
  int32_t n_points;
  const pxt_lm_level* levels_host;
  int32_t n_levels;
  const float* T_init_host;    /* 12 floats */
  float* out;                  /* device or pinned host, 16 + PXT_MAX_LEVELS */
  float* log;                  /* device or pinned host, or NULL */
  void* workspace;             /* device, pxt_lm_workspace_bytes(); one per problem */
  const pxt_lm_camera* cam_host; /* or NULL */
} pxt_lm_problem;
int64_t pxt_lm_batch_workspace_bytes(int32_t n_problems);
int pxt_lm_refine_batch(const pxt_lm_problem* problems_host, int32_t n_problems, const pxt_lm_conf* conf_host,
                        void* batch_workspace, void* stream);

/* Bytes of scratch pxt_lm_refine needs (control words + tagged partial sums), independent of N.  One workspace serves
 * one launch at a time; its content carries over between launches (the tags of a launch continue above those of the
 * previous one, so nothing is zeroed per launch).  Zero it once after allocation, and again after a launch that
 * reported PXT_E_TIMEOUT in out[13] (the kernel also skips a margin of tags on that path). */
int64_t pxt_lm_workspace_bytes(void);

/* -------------------------------------------------------------------------
 * Sparse reference observations.
 *
 * Replaces PoseTrackerRefiner.interp_sparse_observations
 * (pixtrack/localization/pixloc_pose_refiners.py:327-368) plus the per-point
 * stacking/normalisation that refine_pose_using_features does afterwards (A.4):
 * transform the reference image's 3-D points with `T`, project into the reference
 * camera of each level, bilinearly sample the RAW (un-normalised) HWC map, L2-
 * normalise the C descriptor channels of the sample, keep the sampled confidence in
 * channel C.  valid[n] = 1 iff the point is visible and inside the padded image on
 * EVERY level (line :356).
 * ---------------------------------------------------------------------- */
typedef struct {
  const float* fmap;  /* raw reference map, HWC [h][w][cstride] */
  float* out;         /* [n_points][cstride] */
  int32_t h, w, C, cstride;
  float cam[10];      /* reference camera scaled by reference_scale and level scale */
  int32_t ndist;      /* 0, 2 or 4 (anything else: PXT_E_ARG, nothing launched) */
  /* The map may be a WINDOW of the level's full map (round 5: the reference pass runs on a crop of the reference render
   * that holds every input pixel the sampled points depend on - the pyramid's dependency radius around the points'
   * bounding box - instead of on the whole render; pixloc_pose_refiners.py:282-290 computes the dense maps only to sample
   * them at the points, :236,316 `del`).  full_w > 0: the map holds columns [x0, x0 + w) and rows [y0, y0 + h) of a
   * full_w x full_h level; projection, visibility and the padded in-image test use the full level, texels are read at
   * (u - x0, v - y0) - bit for bit the samples of the full map wherever both hold the same texels.  full_w = 0: no window. */
  int32_t x0, y0, full_w, full_h;
} pxt_sample_level;

int pxt_sample_sparse(const float* p3d, int32_t n_points, const float* T_host /* 12 floats */,
                      const pxt_sample_level* levels_host, int32_t n_levels, int32_t pad,
                      int32_t normalize, uint8_t* valid /* [n_points] */, void* stream);

/* -------------------------------------------------------------------------
 * Pose hypothesis scoring (relocalisation: pixtrack_amd/relocalizer.py).
 *
 * The reference has no relocaliser (PixLocPoseTrackerR9.relocalize only counts).  One launch scores M pose
 * hypotheses against ONE query feature map (typically the stride-16 level, C = 128): hypothesis h has a pose
 * (poses[h], 12 floats, row-major R then t) and a contiguous range [begin, begin + count) = ranges[h] of one flat
 * point bank.  For each VALID point (the LM's rule: in front of the camera, inside the image with conf->pad, and
 * bank->valid[n] != 0 when a mask is given) the map is sampled bilinearly and, with r = F_q - F_ref over the C
 * descriptor channels and w = (query confidence) * (reference confidence):
 *   out[h][0] = sum rho(|r|^2)   out[h][1] = n_valid   out[h][2] = sum w * rho   out[h][3] = sum w
 * rho is the LM's loss (conf->loss, loss_alpha, loss_scale; the other conf fields are ignored).  out[h][0] / out[h][1]
 * is the masked-mean cost pxt_lm_refine logs at k = 0 of its first iteration for the same pose, points and level, and
 * out[h][1] that log's k = 1.  Deterministic: a hypothesis's four values depend on its own inputs only (fixed-order
 * reduction, one workgroup per hypothesis), not on M or on the other hypotheses.  A range outside the bank yields
 * {NaN, -1, NaN, NaN}.  poses, ranges and out are device arrays (M is bounded by memory); no workspace is needed.
 * ---------------------------------------------------------------------- */
typedef struct {
  const float* fmap;   /* query map, HWC [h][w][cstride], descriptor L2-normalised, confidence at channel C */
  int32_t h, w, C, cstride;
  float cam[10];       /* query camera scaled to this level (as pxt_lm_level holds it) */
  int32_t ndist;
} pxt_reloc_map;

typedef struct {
  const float* p3d;      /* [n_points][3] world points */
  const float* fref;     /* [n_points][cstride] reference records: descriptor L2-normalised, confidence at C */
  const uint8_t* valid;  /* [n_points] point mask, or NULL */
  int32_t n_points;
} pxt_reloc_bank;

int pxt_score_pose_hypotheses(const pxt_reloc_map* map_host, const pxt_reloc_bank* bank_host,
                              const float* poses /* device [M][12] */, const int32_t* ranges /* device [M][2] */,
                              int32_t n_hypotheses, const pxt_lm_conf* conf_host, float* out /* device [M][4] */,
                              void* stream);

/* pxt_score_pose_hypotheses_depth - the depth counterpart (opt-in: relocalizer.RelocDepth): the same
 * poses, ranges and bank points scored against the frame's sensor depth image.  Per point n of hypothesis h (n in
 * [begin, begin + count), skipped where bank->valid[n] == 0):
 *   p = transform_point(T_h, X_n); (u, v) = project_point(p) (the LM's projection, lens terms included).  A point
 *   project_point refuses or whose pixel (floor(u + 0.5), floor(v + 0.5)) - pxt_points_visible's addressing - is outside
 *   the image counts nowhere.  Otherwise it counts in n_in; raw = sensor[y][x], raw != 0 counts in n_measured;
 *   d = float(raw) * sensor_scale and r = d - p.z are ONE fp32 operation each (no contraction); |r| <= tolerance
 *   counts in n_agree (equality agrees), r > tolerance in n_behind (the sensor sees past the point).  A NaN counts in
 *   neither.
 *   out[h] = {n_in, n_measured, n_agree, n_behind}; a range outside the bank gives {-1, -1, -1, -1} and reads nothing.
 * One wave per hypothesis, integer counts by ballot: no atomics, no workspace; a hypothesis's four words depend on its
 * own inputs only.  bank->fref is ignored.  cam10_host / ndist: the UNSCALED query camera as pxt_points_visible takes it,
 * cam[0] == width and cam[1] == height.
 * Bounds: 1 <= M <= 2^22, width, height >= 1 and width * height <= 2^28, ndist 0 / 2 / 4, bank->n_points >= 1, poses and
 * out 16-byte, ranges 8-byte, sensor 2-byte aligned, no NULL except bank->valid; anything else is PXT_E_ARG and nothing
 * is launched or written. */
int pxt_score_pose_hypotheses_depth(const pxt_reloc_bank* bank_host, const float* poses /* device [M][12] */,
                                    const int32_t* ranges /* device [M][2] */, int32_t n_hypotheses,
                                    const uint16_t* sensor /* device [height][width], 0 = no measurement */, int32_t width,
                                    int32_t height, float sensor_scale /* SfM units per count */,
                                    float tolerance /* SfM units */, const float* cam10_host, int32_t ndist,
                                    int32_t* out /* device [M][4] */, void* stream);

/* -------------------------------------------------------------------------
 * Pose information (the LM's normal equations at a given pose, evaluated once).
 *
 * The reference has no counterpart: pixloc forms H = J^T W J on every iteration and drops it.  One launch evaluates, for
 * n_problems independent (points, level, pose) problems, the sums of ONE LM iteration at the given pose - validity,
 * bilinear taps, central-difference map gradients, w_unc = conf_query * conf_ref and the robust weight rho' are those
 * of pxt_lm_refine (restated in csrc/pxt_lm_info.hip), parameter order as the LM's delta (translation 3, rotation 3,
 * left update) - with NO damping, solve or update.  conf_host supplies pad, loss, loss_alpha, loss_scale and
 * min_valid; level.lambda is ignored.
 *
 * pose: device-readable, 16-byte aligned.  pose_is_lm_record = 0: 12 floats.  1: an output record of pxt_lm_refine*
 * (pose at [0..11], failed at [12], status at [13]), read ON THE DEVICE, so the launch can be queued behind the
 * refinement with no host round trip; when failed or status is non-zero the problem is skipped: no work is done and
 * ONLY word 47 of the record is written (-1.0).
 *
 * Output record (PXT_LM_INFO_RECORD = 48 floats, device or pinned host; word 47 is stored last with system-scope
 * release, so a host may poll it in pinned memory):
 *   [0]      sum over valid points of rho(|r|^2)        [1] n_valid
 *   [2]      sum w |r|^2   (w = rho' * w_unc * valid)    [3] sum w
 *   [4..9]   g = sum w J^T r
 *   [10..30] H = sum w J^T J, upper triangle row-major, UNDAMPED
 *   [31]     0
 *   [32..43] the pose that was evaluated
 *   [44..46] 0
 *   [47]     1.0 ok; -1.0 skipped (LM record failed or timed out: nothing else was written); -2.0 evaluated with
 *            n_valid < min_valid (the LM's own failure rule at this pose: the sums are written, but the LM would not
 *            have used them)
 * [0] / [1] is the masked-mean cost pxt_lm_refine logs at k = 0 of an iteration started at that pose, [1] its k = 1.
 *
 * Deterministic: a problem's points are dealt to a number of workgroups that depends on its n_points and C only;
 * sums are folded in a fixed order inside a workgroup (LDS) and across a problem's workgroups (partials in the
 * workspace, folded by a second small launch; no floating-point atomics).  A record therefore depends on its own
 * problem only - not on n_problems, the other problems, their order, or the run.
 * workspace: device, pxt_lm_information_workspace_bytes(n_problems); it holds the parameter records (more than two
 * problems: copied there from pinned staging memory ahead of the launch in `stream`) and the partial sums; one
 * workspace serves one launch at a time.
 * ---------------------------------------------------------------------- */
#define PXT_LM_INFO_RECORD 48
#define PXT_LM_INFO_MAX_PROBLEMS 64
typedef struct {
  const float* p3d;           /* [n_points][3] */
  const uint8_t* point_mask;  /* [n_points] or NULL */
  int32_t n_points;
  pxt_lm_level level;         /* query map, reference records, camera scaled to the level; lambda ignored */
  const float* pose;          /* device-readable, 16-byte aligned: 12 floats or an LM output record */
  int32_t pose_is_lm_record;
  float* out;                 /* PXT_LM_INFO_RECORD floats, device or pinned host */
} pxt_lm_info_problem;
int64_t pxt_lm_information_workspace_bytes(int32_t n_problems);
int pxt_lm_information(const pxt_lm_info_problem* problems_host, int32_t n_problems, const pxt_lm_conf* conf_host,
                       void* workspace, void* stream);

/* -------------------------------------------------------------------------
 * Per-point residual report (which points carried the pose; opt-in, off the default path).
 *
 * The reference keeps the point set of a refinement at debug >= 2 (pixtrack/localization/tracker.py:26-30, filled from
 * pixtrack/localization/pixloc_pose_refiners.py:200-271) and leaves the per-point terms to pixloc's plots.  One launch
 * evaluates, for n_problems independent (points, level, pose) problems, the POINT terms of ONE LM iteration at the
 * given pose and writes them out instead of summing them into normal equations: validity, the 2 x 2 bilinear taps, the
 * loss and w_unc = conf_query * conf_ref are those of pxt_lm_refine (csrc/pxt_lm_point.h); no gradients, no Jacobian.
 * conf_host supplies pad, loss, loss_alpha, loss_scale and min_valid; level.lambda is ignored.  pose and
 * pose_is_lm_record are those of pxt_lm_information: a failed / timed-out LM record skips the problem - ONLY word 15 of
 * the summary is written (-1.0), `points` stays untouched.
 *
 * Point record n (PXT_LM_POINT_RECORD = 8 floats; `points` is device memory, 16-byte aligned, or NULL: summary only):
 *   [0]    valid (1.0 / 0.0)
 *   [1,2]  (u, v) at the level's scale, in the LM's pixel convention; NaN when the point is not in front of the camera
 *   [3]    |r|^2 over the C descriptor channels           [4] rho(|r|^2)
 *   [5]    rho' (the robust weight)                       [6] w_unc              ([3..6] are 0 for an invalid point)
 *   [7]    reject code: 0 valid, 1 masked out, 2 projection failed (behind the camera or outside the distortion
 *          model's range), 3 outside the padded image
 * Summary (PXT_LM_REPORT_SUMMARY = 16 floats, device or pinned host; word 15 is stored last with system-scope release):
 *   [0] sum rho over valid points     [1] n_valid     [2] n_inliers: valid points with rho' >= inlier_weight
 *   [3] sum rho' * w_unc over valid points            [4] sum w_unc over valid points
 *   [5,6,7] the counts of reject codes 1, 2, 3        [8..14] 0
 *   [15] 1.0 ok; -1.0 skipped; -2.0 evaluated with n_valid < min_valid
 * [0] / [1] is the masked-mean cost pxt_lm_refine logs at k = 0 of an iteration started at that pose, [1] its k = 1.
 *
 * Deterministic in the way pxt_lm_information is: points are dealt to workgroups by n_points and C only, sums fold in
 * a fixed order in LDS and then across a problem's workgroups (partials in the workspace, a second small launch), no
 * floating-point atomics; a problem's output depends on that problem alone.
 * workspace: device, pxt_lm_point_report_workspace_bytes(n_problems); one workspace serves one launch at a time.
 * ---------------------------------------------------------------------- */
#define PXT_LM_POINT_RECORD 8
#define PXT_LM_REPORT_SUMMARY 16
#define PXT_LM_REPORT_MAX_PROBLEMS 64
typedef struct {
  const float* p3d;           /* [n_points][3] */
  const uint8_t* point_mask;  /* [n_points] or NULL */
  int32_t n_points;
  pxt_lm_level level;         /* as pxt_lm_info_problem: lambda ignored */
  const float* pose;          /* device-readable, 16-byte aligned: 12 floats or an LM output record */
  int32_t pose_is_lm_record;
  float inlier_weight;        /* a valid point is an inlier when its robust weight rho' >= this */
  float* points;              /* device [n_points][PXT_LM_POINT_RECORD], or NULL: summary only */
  float* summary;             /* PXT_LM_REPORT_SUMMARY floats, device or pinned host */
} pxt_lm_report_problem;
int64_t pxt_lm_point_report_workspace_bytes(int32_t n_problems);
int pxt_lm_point_report(const pxt_lm_report_problem* problems_host, int32_t n_problems, const pxt_lm_conf* conf_host,
                        void* workspace, void* stream);

/* -------------------------------------------------------------------------
 * UNet feature pyramid (pixloc `UNet`, experiment pixloc_megadepth).
 *
 * Replaces `pred = self.model({"image": image_tensor})`
 * (pixtrack/localization/feature_extractor.py:48) including prepare_input's
 * HWC->CHW, /255 (:31-32).  Weights live in an opaque context created from a flat
 * host blob (layout documented in pixtrack_amd/unet.py: pack_unet_weights).
 * ---------------------------------------------------------------------- */
typedef struct pxt_unet pxt_unet;

int pxt_unet_create(const void* weights_host, int64_t n_bytes, pxt_unet** out_ctx);
int pxt_unet_destroy(pxt_unet* ctx);
/* Scratch the forward pass needs for an H x W input. */
int64_t pxt_unet_workspace_bytes(const pxt_unet* ctx, int32_t H, int32_t W);

/* Diagnostic for a NEW checkpoint (not on the frame's path): pixloc runs this network in fp32, this library stores its
 * activations as fp16.  After a single-image pxt_unet_forward on `workspace`, writes for each of the 17 convolutions
 * stats[2 * l] = largest |activation| (float) and stats[2 * l + 1] = number of non-finite values (uint32 bits) of the
 * layer's output as it sits in the workspace; -1 for the two layers that are never materialised (the first one when it is
 * computed inside the second one's staging, the last one when the fine head is fused).  A non-zero count, or a maximum
 * near 65504, means the checkpoint needs rescaling (or bf16 storage) before its poses can be trusted. */
int pxt_unet_activation_stats(pxt_unet* ctx, int32_t H, int32_t W, const void* workspace, float* stats_device /* [34] */,
                              void* stream);

/* Read-only view of an fp16 pass, for tests that replay it layer by layer from a copy of the workspace (host arithmetic,
 * nothing is launched; PXT_E_ARG for an fp32 context).  For a pass over n_images images of H x W, out[0..16] describe the
 * 17 convolutions' outputs and out[17..20] the pooled inputs of encoder blocks 1..4: `offset` bytes into the pass's
 * workspace, fp16 [n_images][h][w][c]; in_memory == 0 for the two layers pxt_unet_activation_stats reports as -1.  The
 * fine head is fused only into fine maps of out_cstride[0] >= 36: layer 16's in_memory AND its plan (no split-K under
 * the fused head) are those of such a pass; a pass with a narrower fine map writes layer 16 and may split it, which
 * this view does not describe.  For the 3x3 layers 1..16 also the plan the pass takes: tile
 * configuration, split-K factor, whether the 2x2 max-pool of the output is written by the layer itself (else by a
 * separate kernel; out[17..20] repeat the flag of the layer they pool), and whether it is a decoder (upsample + concat)
 * layer.  peers == 1: a pass on its own (pxt_unet_forward, pxt_unet_forward_batch of n_images != 2); peers == 2
 * (n_images == 1): one image of pxt_unet_forward_pair - the second image's workspace starts at
 * pxt_unet_workspace_bytes(ctx, H[0], W[0]). */
typedef struct {
  int64_t offset;
  int32_t h, w, c;
  int32_t in_memory;
  int32_t cfg, splits, pool_fused, decoder;
  int32_t deep_ring, reserved; /* deep_ring: the configuration's deeper tap-fragment ring variant (few workgroups) */
} pxt_unet_layer_view;
int pxt_unet_layer_views(const pxt_unet* ctx, int32_t n_images, int32_t H, int32_t W, int32_t peers,
                         pxt_unet_layer_view* out /* [21] */);

/* The same for an fp32 context (pxt_unet_create_f32), whose pass has its own layout: where pxt_unet_forward_batch over
 * n_images images of H x W leaves its buffers, fp32 [n_images][h][w][c] at `offset` bytes into the workspace, all
 * in_memory.  out[0..16]: the 17 convolutions' outputs, with `cfg` the configuration pxt_conv3x3_f32_cfg names for the
 * layer (0 for layer 0, which has none), splits = 1, pool_fused = 0, deep_ring = 0, decoder = 1 for 13..16;
 * out[17..20]: the pooled inputs of encoder blocks 1..4; out[21]: the decoder-input buffer (upsampled previous layer,
 * then the cropped skip) as the last decoder layer leaves it, [n_images][h of 16][w of 16][input channels of 16] - the
 * four decoder layers share it.  A pair pass is two single passes (n_images = 1 each): the second image's workspace
 * starts at pxt_unet_workspace_bytes(ctx, H[0], W[0]).  PXT_E_ARG for a NULL argument, an fp16 context or a size the
 * pass refuses; nothing is launched. */
int pxt_unet_layer_views_f32(const pxt_unet* ctx, int32_t n_images, int32_t H, int32_t W,
                             pxt_unet_layer_view* out /* [22] */);

/* image: HWC, 3 channels, values 0..255 (float32 if image_is_u8 == 0, else uint8).
 * mask: optional H x W uint8 (0/1) multiplied into the image first
 *       (pixloc_tracker_r9.py:224-225), NULL for none.
 * out_maps[l]: HWC float32 [h_l][w_l][cstride_l], l = 0..2 (strides 1,4,16);
 *       channel C_l is sigmoid(-uncertainty) (A.5); if normalize != 0 the C_l
 *       descriptor channels are L2-normalised per pixel (A.4, query side). */
int pxt_unet_forward(pxt_unet* ctx, const void* image, int32_t image_is_u8, const uint8_t* mask,
                     int32_t H, int32_t W, float* const out_maps[3], const int32_t out_cstride[3],
                     int32_t normalize, void* workspace, void* stream);

/* The same pass over n_images (<= PXT_UNET_MAX_BATCH) equally sized images in one set of
 * launches: a frame's reference render and its masked query
 * (pixloc_pose_refiners.py:282-290 and :255, two model() calls per frame in the
 * reference) share every weight fetch, and the small deep layers get twice the tiles.
 * images[i] / image_is_u8[i] / masks[i] (masks may be NULL, entries may be NULL) /
 * normalize[i] as in pxt_unet_forward; out_maps[3*i + l] = image i, level l.  Each image's
 * result is independent of its batch neighbours; a layer's split-K factor depends on the
 * batch size, so a batched map equals the single-image one up to fp32 summation order. */
#define PXT_UNET_MAX_BATCH 16
int64_t pxt_unet_workspace_bytes_batch(const pxt_unet* ctx, int32_t n_images, int32_t H, int32_t W);
int pxt_unet_forward_batch(pxt_unet* ctx, int32_t n_images, const void* const* images,
                           const int32_t* image_is_u8, const uint8_t* const* masks, int32_t H, int32_t W,
                           float* const* out_maps, const int32_t out_cstride[3], const int32_t* normalize,
                           void* workspace, void* stream);

/* Constant-tile skipping in encoder blocks 1-3 (on by default; $PXT_UNET_SKIP=0 turns it off for the process).  The
 * tracker's images are mostly constant - the masked query is exactly 0 outside the dilated silhouette
 * (pixloc_tracker_r9.py:224-225), the NeRF reference render exactly 0 outside the object - and a convolution tile whose
 * whole dependency cone (through every layer up to it) lies in such a region and inside the image equals ONE vector per
 * layer.  Such tiles (found conservatively from `mask` / a uint8 image on an 8 x 8 block grid) are filled with that
 * vector - obtained once per layer plan by running the layer's own kernel configuration on a constant map, hence the
 * very bits the tile would have computed: the maps are unchanged, bit for bit.  An image with neither a mask nor a
 * uint8 type is computed in full. */
int pxt_unet_set_tile_skip(pxt_unet* ctx, int32_t on);

/* How a batch of MORE than two images plans its layers.  0 (default): tile configuration and split-K factor chosen for
 * the batch as launched (large batches need no split-K: the fastest).  1: every layer takes the plan a SINGLE image of
 * the tracker's two-stream pair pass takes, whatever the batch size, so each image's maps are bit for bit the maps the
 * one-object tracker computes for it (a layer's fp32 summation order is its tile's K walk and its split-K partition).
 * Used by the lock-step multi-object tracker's parity tests; workspace sizes cover both. */
int pxt_unet_set_batch_plan(pxt_unet* ctx, int32_t per_image_plan);

/* Two images of possibly DIFFERENT sizes (H[i] x W[i]) as two single-image passes side by side on two streams - a frame's
 * reference render (reference camera x reference_scale, pixloc_pose_refiners.py:145-152) and its masked query
 * (feature_extractor.py:48 twice per frame).  Arguments as pxt_unet_forward_batch with n_images = 2; out_maps[3 i + k];
 * workspace >= pxt_unet_workspace_bytes_pair. */
int64_t pxt_unet_workspace_bytes_pair(const pxt_unet* ctx, const int32_t H[2], const int32_t W[2]);
int pxt_unet_forward_pair(pxt_unet* ctx, const void* const* images, const int32_t* image_is_u8,
                          const uint8_t* const* masks, const int32_t H[2], const int32_t W[2],
                          float* const* out_maps, const int32_t out_cstride[3], const int32_t* normalize,
                          void* workspace, void* stream);
/* Reference tiles.  The reference image's dense maps exist only to be sampled at the projected 3-D points
 * (pixloc_pose_refiners.py:282-290, then `del`), and the last two decoder layers feed nothing but the fine head.  A pass
 * that is told the points its fine map WILL be sampled at - the arguments of the pxt_sample_sparse call that follows: the
 * points, the pose, the fine level's camera, pad and window - computes only the tiles of those two layers that a sample
 * depends on (the sampler's own arithmetic names the 2 x 2 texels of every point valid on the fine level; the layer
 * before takes the tiles under the needed tiles' up-sampling patches).  Every other tile of the fine map is NOT WRITTEN
 * (the buffer keeps what it held); the computed tiles, the other two maps and hence every sampled value are bit for bit
 * those of the full pass.  Never pass points for a map that anything else reads (the query, dumps, logs).
 * `p3d` is a device pointer [n_points][3]; everything else is read on the host.  full_w = 0: no window, else the pass's
 * fine map is the window [x0, x0 + w) x [y0, y0 + h) of a full_w x full_h level (pxt_sample_level).  The _sampled entry
 * points take the arguments of pxt_unet_forward / pxt_unet_forward_pair plus the points (NULL, or a NULL entry: as
 * the plain call).  They are ignored - every tile is computed - by an fp32 context, with $PXT_UNET_REF_TILES=0, after
 * pxt_unet_set_reference_tiles(ctx, 0), when $PXT_UNET_STREAMS=1 batches an equal-sized pair, and for a layer planned
 * with split-K. */
typedef struct {
  const float* p3d;
  int32_t n_points;
  float T[12];
  float cam[10];
  int32_t ndist, pad;
  int32_t x0, y0, full_w, full_h;
} pxt_unet_sample_points;
/* Query tiles: the record of a QUERY whose fine map will be read by nothing but the fine level of the pxt_lm_refine*
 * launch that starts from pose points.T (camera: the query's fine-level camera; pad: the LM's) and moves the points.
 * Every point in front of the camera, valid at that pose or not, takes the bounding box of the texels the LM's point
 * evaluation loads around floor(u, v) - columns ix0-1..ix0+2, rows iy0-1..iy0+2, clamped into the map as the kernel
 * clamps - grown by `margin` texels on every side and clipped to the map; every tile of the last layer the box meets
 * is computed, the layer before follows as for reference tiles, and the flags stay in the pass's workspace for the
 * LM's tile guard (pxt_unet_query_tiles, pxt_lm_refine_guarded), which sees a refinement that outruns the margin. */
typedef struct {
  pxt_unet_sample_points points;
  int32_t margin;
} pxt_unet_query_points;
int pxt_unet_forward_sampled(pxt_unet* ctx, const void* image, int32_t image_is_u8, const uint8_t* mask, int32_t H,
                             int32_t W, float* const out_maps[3], const int32_t out_cstride[3], int32_t normalize,
                             void* workspace, void* stream, const pxt_unet_sample_points* points_host);
int pxt_unet_forward_pair_sampled(pxt_unet* ctx, const void* const* images, const int32_t* image_is_u8,
                                  const uint8_t* const* masks, const int32_t H[2], const int32_t W[2],
                                  float* const* out_maps, const int32_t out_cstride[3], const int32_t* normalize,
                                  void* workspace, void* stream,
                                  const pxt_unet_sample_points* const* points_host /* [2], entries may be NULL */);
int pxt_unet_set_reference_tiles(pxt_unet* ctx, int32_t on);
/* pxt_unet_forward_pair_sampled whose SECOND image is a query with its own record (reference_points_host: the first
 * image's reference record or NULL; query_points_host NULL: the plain pair).  Gated like reference tiles: single-image
 * passes side by side, fused fine head, one K pass, the tile configuration the flags were made for.  Both passes launch
 * their flag kernel on their side stream at the head of the pass; decoder layer 2 waits for it. */
int pxt_unet_forward_pair_tiles(pxt_unet* ctx, const void* const* images, const int32_t* image_is_u8,
                                const uint8_t* const* masks, const int32_t H[2], const int32_t W[2],
                                float* const* out_maps, const int32_t out_cstride[3], const int32_t* normalize,
                                void* workspace, void* stream, const pxt_unet_sample_points* reference_points_host,
                                const pxt_unet_query_points* query_points_host);
/* Query tiles on / off for this context; $PXT_UNET_QUERY_TILES=0 turns them off for the process.  Off: the query's
 * record is ignored and every tile is computed. */
int pxt_unet_set_query_tiles(pxt_unet* ctx, int32_t on);
/* Where the pair pass over H[i] x W[i] images keeps the flags of image 1's last decoder layer, and that layer's tile
 * geometry: out[0] byte offset into the pair workspace, out[1] tile rows, out[2] tiles per row, out[3] rows of tiles,
 * out[4] 1 if the LAST forward call on this context was a pair call whose query pass used its record and wrote the
 * flags (0: that call computed every tile and wrote no flags - hand the LM no guard).  Ask after the pair call and
 * before any other forward call: the answer is the pass's own, whatever knob, stride, size or batching decided it.
 * Host only; nothing is launched. */
int pxt_unet_query_tiles(const pxt_unet* ctx, const int32_t H[2], const int32_t W[2], int64_t out[5]);
/* Image 1 of a pair call over H[i] x W[i] images again, alone and IN FULL (no record), on `stream`: into out_maps[3], in
 * image 1's part of the same pair `workspace`, and planned as one image of the pair - so the maps are bit for bit those
 * image 1 has in a pair call without a query record (a lone pxt_unet_forward plans its layers for an empty chip:
 * other tile configurations and split-K partitions, other bits).  What a caller runs after the LM's tile guard tripped.
 * fp16 contexts only. */
int pxt_unet_forward_pair_second(pxt_unet* ctx, const void* image, int32_t image_is_u8, const uint8_t* mask,
                                 const int32_t H[2], const int32_t W[2], float* const out_maps[3],
                                 const int32_t out_cstride[3], int32_t normalize, void* workspace, void* stream);
/* The flag rule alone, on the HOST (every pointer, `p3d` too, is host memory; no device is touched): for a fine_h x
 * fine_w fine map (even sizes) cut into fine_tile_rows x 16 tiles and the (fine_h / 2) x (fine_w / 2) layer before it cut
 * into low_tile_rows x 16 tiles, writes 1 for every tile a sampled pass computes and 0 for the others, row-major.  The
 * same functions the device kernel runs: what the tests hold against their own replica of the rule. */
int pxt_unet_reference_tiles_host(const pxt_unet_sample_points* points_host, int32_t fine_h, int32_t fine_w,
                                  int32_t fine_tile_rows, int32_t low_tile_rows, uint8_t* fine_flags_host,
                                  uint8_t* low_flags_host);
/* The same for a query's record (margin >= 0). */
int pxt_unet_query_tiles_host(const pxt_unet_query_points* query_points_host, int32_t fine_h, int32_t fine_w,
                              int32_t fine_tile_rows, int32_t low_tile_rows, uint8_t* fine_flags_host,
                              uint8_t* low_flags_host);

/* Deferred join of the pair entry (round 4): with pxt_unet_set_defer_join(ctx, 1), pxt_unet_forward_pair (and the
 * two-image pxt_unet_forward_batch that runs through it) returns with image 0's maps complete in the caller's stream
 * order and image 1's pass still running on the library's side stream; the caller may enqueue work that needs image 0
 * only - the tracker's sparse sampling of the REFERENCE maps (pixloc_pose_refiners.py:327-368) - and must call
 * pxt_unet_pair_join(ctx, stream) before anything reads image 1's maps (it makes `stream` wait for that pass; a no-op
 * when nothing is pending; the next forward call on the context joins by itself). */
int pxt_unet_set_defer_join(pxt_unet* ctx, int32_t on);
int pxt_unet_pair_join(pxt_unet* ctx, void* stream);

/* fp32 pass (ABI 13).  pxt_unet_create_f32 takes the fp32 pack of pixtrack_amd/unet.py (pack_unet_weights(w,
 * precision="fp32"): every 3x3 filter float32) and makes a context on which the whole network runs in fp32: fp32 NHWC
 * activations, 3x3 convolutions on the exact f32-input MFMA, the same output maps as the fp16 pass.  This is pixloc's own
 * precision and range: a checkpoint whose activations leave fp16's range runs unchanged.  Every pxt_unet_* entry point
 * above accepts such a context with the same signature:
 *   - the workspace_bytes* functions return the fp32 pass's sizes (about twice the fp16 ones);
 *   - forward / forward_batch / forward_pair run the fp32 pass.  Each image's maps are the same bits alone, in a batch
 *     of any size and in a pair (no split-K, no atomics: every value is one fixed-order chain);
 *   - set_tile_skip and set_batch_plan are accepted and have no effect (the pass computes every tile, and its bits do not
 *     depend on the batch);
 *   - a pair runs both images on the caller's stream, image 0 first, so set_defer_join's contract holds trivially and
 *     pair_join has nothing to wait for;
 *   - activation_stats reports all 17 layers (none is left unmaterialised) as fp32 values: a maximum above 65504 is
 *     a layer the fp16 pass cannot store.
 * pxt_unet_precision returns 16 or 32 (the context's storage precision), < 0 on a NULL context. */
int pxt_unet_create_f32(const void* weights_host, int64_t n_bytes, pxt_unet** out_ctx);
int pxt_unet_precision(const pxt_unet* ctx);


/* One 3x3 convolution (pad 1) of the pyramid as a stand-alone call, for layer-by-layer
 * parity tests against torch.nn.functional.conv2d (SURVEY KAT-6) and for profiling:
 * in  [H][W][Cin]  fp16 NHWC (Cin % 32 == 0), weights [Cout][3][3][Cin] fp16
 * (Cout % 32 == 0), bias [Cout] float32, out [H][W][Cout] fp16; fused bias (+ReLU). */
int pxt_conv3x3_nhwc_f16(const void* in, int32_t H, int32_t W, int32_t Cin, const void* weights,
                         const float* bias, int32_t Cout, int32_t relu, void* out, void* stream);

/* One 3x3 convolution (pad 1) of the fp32 pass, for layer-level tests: in [H][W][Cin] float32 NHWC (Cin % 16 == 0),
 * weights [Cout][3][3][Cin] float32 on the device (Cout % 32 == 0), bias [Cout], out [H][W][Cout] float32; fused bias
 * (+ReLU).  The taps are repacked into the kernel's fragment order on every call. */
int pxt_conv3x3_nhwc_f32(const void* in, int32_t H, int32_t W, int32_t Cin, const void* weights,
                         const float* bias, int32_t Cout, int32_t relu, void* out, void* stream);

/* The tile configuration the fp32 pass runs a 3x3 layer of H x W with Cout output channels in (host arithmetic only; the
 * pass's own choice function): 1..5 = conv3x3_f32_kernel<CB, PB, WC, WP> <2,2,2,2>, <2,1,2,2>, <2,2,1,4>, <2,1,1,4>,
 * <1,2,1,4>, whose workgroups span 128, 128, 64, 64 and 32 output channels; PXT_E_ARG for a shape the pass refuses
 * (H or W < 1, Cout < 32 or no multiple of 32).
 * pxt_conv3x3_nhwc_f32_cfg is pxt_conv3x3_nhwc_f32 with that choice as an argument, for tests: cfg 0 = the pass's
 * choice, 1..5 = that configuration whatever the map size; PXT_E_ARG for another value or when Cout is no multiple of
 * the configuration's span.  Every configuration forms each output value by the same chain, so all give the same bits. */
int pxt_conv3x3_f32_cfg(int32_t H, int32_t W, int32_t Cout);
int pxt_conv3x3_nhwc_f32_cfg(const void* in, int32_t H, int32_t W, int32_t Cin, const void* weights,
                             const float* bias, int32_t Cout, int32_t relu, void* out, int32_t cfg, void* stream);

/* The same layer with the taps already in the kernel's MFMA-fragment order (what pxt_unet_create
 * prepares once for every layer of the pyramid), for profiling the convolution alone and for
 * choosing tile configurations:
 *   pxt_conv3x3_packed_bytes   bytes of the packed taps (= Cout*9*Cin*2), < 0 on bad dims
 *   pxt_conv3x3_pack_weights   [Cout][3][3][Cin] fp16 (device) -> packed (device)
 *   pxt_conv3x3_packed         in / out as above; pool_out (optional) [H/2][W/2][Cout] receives the
 *                              2x2 max-pool of the output; cfg 0 = automatic, 1..6 = tile
 *                              configuration (csrc/pxt_unet.hip kTileCfgs); splits > 1 = split-K over
 *                              the input-channel chunks with splitk_ws >= splits*H*W*Cout*4 bytes. */
int64_t pxt_conv3x3_packed_bytes(int32_t Cin, int32_t Cout);
int pxt_conv3x3_pack_weights(const void* weights, int32_t Cin, int32_t Cout, void* packed, void* stream);
int pxt_conv3x3_packed(const void* in, int32_t H, int32_t W, int32_t Cin, const void* packed, const float* bias,
                       int32_t Cout, int32_t relu, void* out, void* pool_out, int32_t cfg, int32_t splits,
                       void* splitk_ws, int64_t splitk_ws_bytes, void* stream);

/* A decoder layer of the pyramid as a stand-alone call: the 3x3 convolution of
 * cat([bilinear x2 upsample (align_corners = false) of prev [Hp][Wp][Cp], skip [Hs][Ws][Cs] cropped to [2Hp][2Wp]])
 * -> out [2Hp][2Wp][Cout], the concatenation formed in the kernel's staging.  Cp, Cs, Cout multiples of 32, Hs >= 2Hp,
 * Ws >= 2Wp; packed: the taps of the Cp + Cs input channels (pxt_conv3x3_pack_weights); cfg 0 = automatic, else a tile
 * configuration that has a decoder variant for this Cout (kTileCfgs upcat_c: 64 for Cout % 64 == 0, else 32);
 * splits / splitk_ws as for pxt_conv3x3_packed. */
int pxt_conv3x3_upcat_packed(const void* prev, int32_t Hp, int32_t Wp, int32_t Cp, const void* skip, int32_t Hs, int32_t Ws,
                             int32_t Cs, const void* packed, const float* bias, int32_t Cout, int32_t relu, void* out,
                             int32_t cfg, int32_t splits, void* splitk_ws, int64_t splitk_ws_bytes, void* stream);

/* -------------------------------------------------------------------------
 * instant-ngp style NeRF inference renderer.
 *
 * Replaces `testbed.render(width, height, spp, True)` and the setters pixtrack
 * drives around it (pixtrack/visualization/run_vis_on_poses.py:38-56,
 * pixtrack/utils/ingp_utils.py:22-44).
 * ---------------------------------------------------------------------- */
typedef struct pxt_ngp pxt_ngp;

typedef struct {
  int32_t n_levels, n_features, log2_hashmap, base_res;
  float per_level_scale;
  int32_t grid_cascades;   /* occupancy cascades, 128^3 each */
  float aabb_scale;        /* scene box = [0.5 - s/2, 0.5 + s/2]^3 */
  float cone_angle;        /* dt growth (1/256 when aabb_scale > 1) */
  float depth_scale;       /* colour written in Depth mode = depth * depth_scale */
  int32_t linear_colors;   /* 0: Shade applies srgb_to_linear to every finished ray's colour before the spp mean
                              (instant-ngp's shade_kernel_nerf for snapshots trained on LDR images - pixtrack's);
                              1: the snapshot was trained in linear colours (HDR set): no conversion */
} pxt_ngp_model;

int pxt_ngp_create(const pxt_ngp_model* model_host, const void* grid_params_f16_host,
                   int64_t n_grid_params, const void* mlp_params_f16_host, int64_t n_mlp_params,
                   const uint8_t* occupancy_bits_host, int64_t n_occ_bytes, pxt_ngp** out_ctx);
int pxt_ngp_destroy(pxt_ngp* ctx);

typedef struct {
  float cam[12];        /* camera-to-world 3x4 row-major, ALREADY in ngp coordinates */
  float focal;          /* pixels; fov_axis = 0 (run_vis_on_poses.py:38) */
  float k1;             /* render_with_camera_distortion (ingp_utils.py:34) */
  float aabb_min[3], aabb_max[3]; /* render_aabb (ingp_utils.py:41-42) */
  float background[4];  /* ingp_utils.py:23-24 */
  float min_transmittance; /* ingp_utils.py:37 */
  int32_t width, height, spp;
  int32_t mode;         /* 0 Shade, 1 Depth (run_vis_on_poses.py:49-56) */
} pxt_ngp_view;

/* out_rgba: float32 [height][width][4], linear colour (render(..., linear=True)). */
int pxt_ngp_render(pxt_ngp* ctx, const pxt_ngp_view* view_host, float* out_rgba,
                   uint64_t* stats /* device, 4 counters (added to) or NULL: [0] samples composited, [1] rays that hit the
                                      render box, [2] wave steps that shaded samples (64 sample slots each), [3] hash-grid
                                      levels of those steps fetched as one 4 x 4 x 4 box per wave (of 16 per step) */,
                   void* stream);

/* Shade AND Depth of the SAME view in one march: bit-for-bit what two pxt_ngp_render calls
 * (mode 0, then mode 1) of this view produce, with the per-sample gathers and the density
 * network evaluated once.  pixtrack renders the mask (Depth, query camera) and the reference
 * image (Shade, SfM camera x reference_scale) at the same pose every frame
 * (pixloc_tracker_r9.py:224,227); when those two cameras coincide the tracker uses this. */
int pxt_ngp_render_both(pxt_ngp* ctx, const pxt_ngp_view* view_host, float* out_rgba, float* out_depth_rgba,
                        uint64_t* stats, void* stream);

/* pxt_ngp_render_both of a view whose CAMERA is not known on the host yet: `pose12` (device-readable, e.g. the pinned
 * record pxt_lm_refine writes: world->camera R row-major, then t, float32) is turned into the camera by a one-thread
 * kernel ahead of the render in `stream`, in the float64 arithmetic of the host chain it replaces
 * (pixtrack/utils/pose_utils.py:24-27 -> ingp_utils.py:47-63 -> Testbed.set_nerf_camera_matrix); view_host->cam is
 * ignored.  conv27 (host): nerf2sfm centroid[3], 3 / avglen, R[16] row-major, totp[3], then the snapshot's scale and
 * offset[3].  cam_out13 (optional, pinned host): the 12 camera floats + a completion word set last (system scope),
 * so that the caller can verify, once the pose reaches it, that the render used the bits it would have passed itself.
 * out_depth_rgba == NULL: ONE render in view_host->mode (0 Shade, 1 Depth) into out_rgba.
 * This lets a tracker enqueue frame t+1's render behind frame t's LM launch instead of after its result. */
int pxt_ngp_render_both_from_pose(pxt_ngp* ctx, const pxt_ngp_view* view_host, const float* pose12,
                                  const double* conv27_host, float* cam_out13, float* out_rgba,
                                  float* out_depth_rgba, uint64_t* stats, void* stream);

/* One render with the outputs the tracking loop consumes written by the renderer's last kernel itself, and - for a
 * render queued behind the LM launch - the camera taken from this context's camera slot instead of a conversion launch
 * (between-stage fusion).
 *   mode 0 Shade, 1 Depth, 2 Shade + Depth of the same view in one march (pxt_ngp_render_both).
 *   out->rgba / depth_rgba : the float32 images of pxt_ngp_render(_both); each may be NULL when its 8-bit stand-in is given
 *   out->rgb_u8  [H][W][3] : get_nerf_image's `(rgba[:, :, :3] * 255).astype(uint8)` of the Shade image
 *                            (pixtrack/visualization/run_vis_on_poses.py:52-54, alpha_thresh 0) - what pxt_rgba_to_u8 makes of rgba
 *   out->depth_nz [H][W]   : 1 where `uint8(depth * 255) != 0` - get_mask's plane before the morphology
 *                            (pixtrack/pose_trackers/pixloc_tracker_r9.py:210-212); feed it to pxt_depth_mask_plane
 *   camera_from_slot != 0  : view_host->cam is ignored; the 12 camera floats are read from pxt_ngp_camera_slot(ctx),
 *                            which an earlier kernel of the same stream wrote (pxt_lm_refine_cam's epilogue). */
typedef struct {
  float* rgba;
  float* depth_rgba;
  uint8_t* rgb_u8;
  uint8_t* depth_nz;
} pxt_ngp_outputs;
int pxt_ngp_render_frame(pxt_ngp* ctx, const pxt_ngp_view* view_host, int32_t mode, int32_t camera_from_slot,
                         const pxt_ngp_outputs* out, uint64_t* stats, void* stream);
float* pxt_ngp_camera_slot(pxt_ngp* ctx); /* device float[12], owned by the context */

/* pxt_ngp_render_frame for n_renders (<= PXT_NGP_MAX_BATCH) DIFFERENT contexts in ONE chain of launches on ONE stream:
 *   - a frame's two renders of different cameras - the mask's Depth render at the query camera and the reference image's
 *     Shade render at SfM camera 1 x reference_scale, at the same pose
 *     (pixtrack/pose_trackers/pixloc_tracker_r9.py:145-152, 207-214): modes {1, 0}, the second context made with
 *     pxt_ngp_create_shared;
 *   - K objects tracked in lock-step, one tracker (and one pyngp.Testbed) per object as
 *     pixtrack/pose_trackers/pixloc_tracker_r9.py:287-318 builds them: modes {2, 2, ...}.
 * The chain is four launches - ray generation, the first-hit pass, one persistent render kernel, resolve - and each of them
 * carries every render of the batch (blockIdx.y = render, one parameter record per render), so nothing depends on how streams are dealt
 * to hardware queues.
 * ctxs[k] / views_host[k] / modes[k] / outs_host[k] / stats[k] (stats or stats[k] may be NULL) are what K calls of
 * pxt_ngp_render_frame(ctxs[k], &views_host[k], modes[k], camera_from_slot, &outs_host[k], stats[k], stream) would take; the
 * images are bit for bit those calls' images.  Modes and sizes may differ per render.  batch_workspace: device memory of
 * pxt_ngp_batch_workspace_bytes(n_renders) bytes for the parameter records (may be NULL for n_renders <= 2, whose records
 * travel as kernel arguments); it must stay untouched until the chain has finished (a per-stream buffer is enough). */
#define PXT_NGP_MAX_BATCH 16
int64_t pxt_ngp_batch_workspace_bytes(int32_t n_renders);
int pxt_ngp_render_frame_batch(pxt_ngp* const* ctxs, const pxt_ngp_view* views_host, int32_t n_renders,
                               const int32_t* modes, int32_t camera_from_slot, const pxt_ngp_outputs* outs_host,
                               uint64_t* const* stats, void* batch_workspace, void* stream);

/* A second context over the SAME snapshot as `src`: own ray lists, counters and camera slot, shared (reference-counted)
 * hash table / MLP / occupancy tables - what a frame's second render needs (the testbed pixtrack drives is one object with
 * one snapshot, pixtrack/utils/ingp_utils.py:22-44, rendered twice per frame with different cameras).  Destroy each context
 * with pxt_ngp_destroy, in any order. */
int pxt_ngp_create_shared(pxt_ngp* src, pxt_ngp** out_ctx);

/* Live HIP-event timing of the renderer's dominant launch, for the roofline line of bench.py: the persistent render kernel
 * (march, hash-grid gathers, both MLPs and compositing of every ray) of a single-render chain (n_renders = 1; batched
 * chains are not timed).  every_nth > 0: that launch of every every_nth-th render is bracketed by an event pair recorded
 * on the render's own stream (an event record is a marker packet between kernels, so sampling keeps the measurement from
 * slowing what it measures); 0 disables.  pxt_ngp_timing_read synchronises those events, returns their summed duration
 * (ms) and the number of timed launches, and clears the list. */
int pxt_ngp_timing_enable(pxt_ngp* ctx, int32_t every_nth);
int pxt_ngp_timing_read(pxt_ngp* ctx, float* total_ms_host, int32_t* n_launches_host);

/* Network query at caller-given points, ngp coordinates + unit view directions (device
 * float32 [n][3] each): out[n][4] = (density logit, r, g, b).  Same device code as the
 * renderer's per-sample evaluation; used by the parity tests (SURVEY KAT-7). */
int pxt_ngp_query(pxt_ngp* ctx, const float* pos, const float* dir, int32_t n, float* out, void* stream);

/* -------------------------------------------------------------------------
 * Small image ops on the path (host cv2/numpy calls in the reference).
 * ---------------------------------------------------------------------- */
/* get_mask (pixloc_tracker_r9.py:207-214): depth RGBA -> uint8((d*255)) != 0 ->
 * erode 5x5 x n_erode -> dilate 5x5 x n_dilate.  tmp: 2*H*W bytes.
 * mask_out is a dense uint8 [H][W] (row stride W).  When W % 4 == 0 it must be 4-byte aligned: the single-pass
 * kernel (2 * (n_erode + n_dilate) <= 16) then stores four mask bytes as one dword.  No requirement otherwise. */
int pxt_depth_mask(const float* depth_rgba, int32_t H, int32_t W, int32_t n_erode,
                   int32_t n_dilate, uint8_t* mask_out, uint8_t* tmp, void* stream);
/* The same mask from the `uint8(depth * 255) != 0` byte plane a render wrote itself (pxt_ngp_render_frame's depth_nz):
 * bit for bit pxt_depth_mask of that render's float depth image.  tmp (2*H*W bytes) is only needed when
 * 2 * (n_erode + n_dilate) > 16 and may be NULL otherwise.  mask_out: dense uint8 [H][W], 4-byte aligned when
 * W % 4 == 0 (as for pxt_depth_mask). */
int pxt_depth_mask_plane(const uint8_t* depth_nz, int32_t H, int32_t W, int32_t n_erode, int32_t n_dilate,
                         uint8_t* mask_out, uint8_t* tmp, void* stream);
/* get_nerf_image tail (run_vis_on_poses.py:52-54): alpha threshold, *255, ->uint8. */
int pxt_rgba_to_u8(const float* rgba, int32_t H, int32_t W, float alpha_thresh, uint8_t* rgb_out,
                   void* stream);
/* pixloc resize(image, size, max, "linear") == cv2.INTER_LINEAR on float32 HWC
 * (feature_extractor.py:45). */
int pxt_resize_linear(const float* src, int32_t H, int32_t W, int32_t C, float* dst, int32_t Ho,
                      int32_t Wo, void* stream);

/* Which pixels of an image that pxt_resize_linear produces can be non-zero (uint8 [Ho][Wo], 1 = may be non-zero): 0 only
 * where every source pixel under the 2 x 2 bilinear taps, grown by one pixel, is inactive - `mask` 0 where the source was
 * multiplied by a mask (a masked query, feature_extractor.py:41-45 resizes after masking), else a uint8 source that is 0
 * in all three channels (a NeRF render's background).  Passed on as the `mask` of pxt_unet_forward (a multiplication by
 * exactly 0 or 1 there), it gives the constant-tile skipping its source for images above the extractor's size limit. */
int pxt_resize_activity(const uint8_t* mask, const uint8_t* image_u8, int32_t H, int32_t W, int32_t Ho, int32_t Wo,
                        uint8_t* active_out, void* stream);

/* -------------------------------------------------------------------------
 * Reference points from a Depth render (opt-in; csrc/pxt_points.hip).
 *
 * Stands in for the reference's use of the SfM points of the nearest mapping image as the points a frame is refined on
 * (pixtrack/localization/pixloc_pose_refiners.py:282-290): the points are a lattice of the render's own pixels,
 * back-projected with the renderer's pixel convention (pixel centre at +0.5, principal point at the image centre).
 *   depth [H][W][4] float32 (16-byte aligned): what a Depth-mode render writes - channel 0 the composited
 *       t * zdot * depth_scale after the spp mean, channel 3 alpha (background alpha 0).
 *   base test of a pixel: alpha >= min_alpha && depth0 > 0.  ACCEPTED: the base test holds on the whole
 *       (2 erode + 1)^2 square around it (erode 0..2; a square that leaves the image fails).
 *   stride s (chosen on the device): the smallest integer >= 1 with s * s * n_max >= A, A = accepted pixels.
 *   candidates: accepted pixels with x % s == s / 2 && y % s == s / 2; points: the first n_max candidates in row-major
 *       order (order-preserving compaction without atomics: the same bits every launch).
 *   point: z = depth0 / (alpha * depth_scale); p = b + z * M ((x + 0.5 - W/2) / focal, (y + 0.5 - H/2) / focal, 1)^T with
 *       xform_host = [M | b] (3x4 row-major, host): render camera-to-ngp chained with ngp -> SfM object coordinates.
 *       No lens undistortion: the caller refuses a Depth view with k1 != 0.
 *   p3d [n_max][3], slot_valid [n_max]: slots >= n_points get slot_valid 0 and p = b (the camera centre, which
 *       pxt_sample_sparse rejects at the reference pose: z > eps fails, so the LM gives them weight 0).
 *   record (4 int32, device or pinned host) = {A, s, n_points, n_candidates}, written by the last launch;
 *       n_candidates > n_max: the tail was cut.
 *   workspace: device memory of the size the _workspace_bytes call returns (< 0: unsupported size), 8-byte aligned,
 *       untouched until the launches have finished.  Three launches on `stream`, no host synchronisation. */
int64_t pxt_points_from_depth_workspace_bytes(int32_t width, int32_t height);
int pxt_points_from_depth(const float* depth, int32_t width, int32_t height, const float* xform_host, float focal,
                          float depth_scale, float min_alpha, int32_t erode, int32_t n_max, float* p3d,
                          uint8_t* slot_valid, int32_t* record, void* workspace, void* stream);

/* -------------------------------------------------------------------------
 * Reference points from the depth planes of a mesh template's frame call (opt-in; csrc/pxt_points.hip).
 *
 * pxt_points_from_depth for the planes the mesh rasteriser writes (pxt_mesh_render_frame's `depth` output: a covered
 * pixel holds z * depth_q in channel 0 and 1.0 in channel 3, background four zeros), up to PXT_POINTS_MAX_VIEWS views of
 * different sizes in ONE chain of three launches - the points of all the mesh objects a lock-step step tracks.
 *   depth: host array of n_views device pointers, view k's plane [H_k][W_k][4] float32 (16-byte aligned each);
 *   sizes [n_views][2] int32 (host): W_k, H_k, each 1..16384;
 *   views [n_views][PXT_MESH_VIEW] float32 (host): the 20 floats the frame call drew the plane with - [0..8] R row-major,
 *       [9..11] t (world -> camera), [12..15] fx fy cx cy, [16] near, [17] depth_q.  All finite, fx, fy, depth_q > 0.
 *   selection, per view, exactly pxt_points_from_depth's: base test of a pixel .w >= min_alpha && .x > 0; ACCEPTED: the
 *       base test holds on the whole (2 erode + 1)^2 square around it (erode 0..2; a square that leaves the image
 *       fails); stride s: the smallest integer >= 1 with s * s * n_max >= A, A = the view's accepted pixels; candidates:
 *       accepted pixels with x % s == s / 2 && y % s == s / 2; points: the first n_max candidates in row-major order.
 *   point of pixel (x, y), the mesh rasteriser's pixel rule (pixel centres at integer coordinates), every step a single
 *       fp32 operation (no contraction, IEEE division):
 *           z = d.x / depth_q;   xn = ((float) x - cx) / fx, yn = ((float) y - cy) / fy;
 *           c = (z * xn, z * yn, z);   q_k = c_k - t_k;   p_j = (R_0j q_0 + R_1j q_1) + R_2j q_2   (R^T q: object frame)
 *       mesh_render.points_reference restates selection and arithmetic in numpy; the two agree bit for bit.
 *   p3d [n_views][n_max][3], slot_valid [n_views][n_max]: view k's slots >= n_points get slot_valid 0 and the camera
 *       centre (the last line with q = -t), which pxt_sample_sparse rejects at the frame's pose.
 *   records [n_views][4] int32 (device or pinned host) = {A, s, n_points, n_candidates} per view.
 *   A view's p3d, slot_valid and record are a pure function of its plane, its 20 floats and (min_alpha, erode, n_max):
 *       they do not depend on n_views, on the view's index or on the other views; no atomics, slots in row-major order.
 *   workspace: device memory of pxt_points_from_depth_views_workspace_bytes(n_views, sizes) bytes (< 0: a count or size
 *       out of range), 16-byte aligned, untouched until the launches have finished; one workspace serves one call at a
 *       time.  The view table travels in the kernel arguments: three launches on `stream`, no upload, no host
 *       synchronisation, no allocation.
 * Bounds: 1 <= n_views <= PXT_POINTS_MAX_VIEWS, erode 0..2, 1 <= n_max <= 2^24, no NULL, p3d, slot_valid and records
 *   4-byte aligned; anything else is PXT_E_ARG and nothing is launched or written.
 * Measured on the MI355X: DESIGN.md 3.21.
 * ---------------------------------------------------------------------- */
#define PXT_POINTS_MAX_VIEWS 16
int64_t pxt_points_from_depth_views_workspace_bytes(int32_t n_views, const int32_t* sizes);
int pxt_points_from_depth_views(const float* const* depth, const int32_t* sizes, const float* views, int32_t n_views,
                                float min_alpha, int32_t erode, int32_t n_max, float* p3d, uint8_t* slot_valid,
                                int32_t* records, void* workspace, void* stream);

/* -------------------------------------------------------------------------
 * Pose-error evaluation (opt-in; csrc/pxt_eval.hip).
 *
 * Replaces, for a whole run in one call, the per-frame Python loop of the reference's notebooks/GetMetrics.ipynb
 * (`get_metrics`: mean one-to-one vertex distance, ADD) and pixtrack_amd/evaluation.py's adds_distance (ADD-S, one frame
 * at a time, O(V^2) numpy): F frames x V model points, F * V^2 distance evaluations for ADD-S.
 *   vertices  [V][3] float32, object frame, CENTRED by the caller (centroid subtracted).
 *   rel_poses [F][12]: R row-major then t of T_rel = T_gt^-1 T_est expressed for the centred vertices
 *       (evaluation.relative_poses forms it in float64 and rounds once).  In the ground-truth object frame
 *       |T_est v_j - T_gt v_i| = |T_rel v_j - v_i|, so the kernel works on object-sized numbers only.
 *   record of frame f (PXT_POSE_ERR_RECORD = 8 floats):
 *       [0] ADD   = mean_i |T_rel v_i - v_i|               [1] max_i of that distance
 *       [2] ADD-S = mean_i min_j |T_rel v_j - v_i|         [3] max_i of that minimum
 *           (adds_distance's direction: for every ground-truth point the nearest estimated point)
 *       [4] V as float      [5], [6] 0
 *       [7] status: 1.0 ok; -1.0 when the frame's pose holds a non-finite value - then ONLY [7] is written
 *       want_adds == 0: ADD only (O(V) per frame); [2] and [3] are written as 0, [0] and [1] keep their bits.
 *   Bounds: 1 <= V <= 2^20, 1 <= F <= 65535, every pointer 4-byte aligned; anything else is PXT_E_ARG.
 *   Deterministic: fixed-order reductions (wave butterfly, LDS, partials in the workspace folded in block order by a
 *   second launch), no atomics: a frame's record depends on its own pose and the vertex set only - not on F, on the
 *   frame's index or on the other frames.
 *   workspace: device memory of pxt_pose_errors_workspace_bytes(F, V) bytes (< 0: unsupported sizes); one workspace
 *   serves one call at a time.  Two launches on `stream`, no host synchronisation. */
#define PXT_POSE_ERR_RECORD 8
int64_t pxt_pose_errors_workspace_bytes(int32_t n_frames, int32_t n_vertices);
int pxt_pose_errors(const float* vertices, int32_t n_vertices, const float* rel_poses, int32_t n_frames,
                    int32_t want_adds, float* records, void* workspace, void* stream);

/* -------------------------------------------------------------------------
 * Mesh-free pose evaluation: two Depth renders compared pixel by pixel (opt-in; csrc/pxt_eval_render.hip).
 *
 * No reference counterpart.  For P (estimated, ground-truth) pairs of Depth renders it counts what the BOP benchmark's
 * Visible Surface Discrepancy, the silhouette IoU and the mean depth error on the overlap are made of
 * (pixtrack_amd/render_evaluation.py): no mesh and no symmetry flag are involved.
 *   depth_est, depth_gt [P][H][W][4] float32 (16-byte aligned; may be the same pointer): what a Depth-mode render
 *       writes - channel 0 the composited t * zdot * depth_scale after the spp mean, channel 3 alpha.
 *   per pixel, all fp32: vis(v) = v.w >= min_alpha && v.x > 0 (pxt_points_from_depth's base test); q(v) = v.x / v.w
 *       (correctly rounded); both = vis(e) && vis(g); dq = |q(e) - q(g)|; within_k = both && dq < tq[k] (strict; false
 *       for a NaN).  A `both` pixel whose dq is NaN or inf counts in n_both, is within no threshold and adds nothing to
 *       the sum or the max.
 *   tq_host [n_taus] (host; travels as kernel arguments): the thresholds in units of q - the caller divides a
 *       distance by the depth-to-distance factor in float64 and rounds once, so that the kernel multiplies no depth.
 *   record of pair p (PXT_DEPTH_AGREE_RECORD = 24 uint32 words, all written by the last launch):
 *       [0] n_est   [1] n_gt   [2] n_both   [3] n_union = n_est + n_gt - n_both
 *       [4] bits of float sum of dq over the `both` pixels with a finite dq   [5] bits of float max of the same (+0.0: none)
 *       [6] n_taus  [7] 1      [8 + k] n_within_k for k < n_taus, 0 for the rest
 *   Bounds: 1 <= P <= 65535, 1 <= n_taus <= 16, width, height >= 1 and width * height <= 2^28, the images and the
 *       workspace 16-byte aligned, records 4-byte aligned; anything else is PXT_E_ARG and nothing is launched or written.
 *   Deterministic: counts by ballot + population count, the float sum and max through fixed-order reductions (wave
 *   butterfly, LDS, one partial per workgroup in the workspace, folded in a fixed order by a second launch), no
 *   atomics: a pair's record depends on its own two images and the thresholds only - not on P or on the pair's index.
 *   workspace: device memory of pxt_depth_agreement_workspace_bytes(P, width, height) bytes (< 0: unsupported sizes);
 *   one workspace serves one call at a time.  Two launches on `stream`, no host synchronisation. */
#define PXT_DEPTH_AGREE_MAX_TAUS 16
#define PXT_DEPTH_AGREE_RECORD 24
int64_t pxt_depth_agreement_workspace_bytes(int32_t n_pairs, int32_t width, int32_t height);
int pxt_depth_agreement(const float* depth_est, const float* depth_gt, int32_t n_pairs, int32_t width, int32_t height,
                        float min_alpha, const float* tq_host, int32_t n_taus, uint32_t* records, void* workspace,
                        void* stream);

/* -------------------------------------------------------------------------
 * Symmetry-aware pose errors: BOP's MSSD and MSPD (opt-in; csrc/pxt_eval_sym.hip).
 *
 * No reference counterpart.  For F frames, V model points and a set of S symmetry transforms of the object
 * (pixtrack_amd/symmetry.py) it evaluates the F * S * V point pairs behind the BOP benchmark's Maximum Symmetry-aware
 * Surface Distance and Maximum Symmetry-aware Projection Distance:
 *       MSSD = min_s max_i |T_est v_i - T_gt S_s v_i|          MSPD = min_s max_i |pi(T_est v_i) - pi(T_gt S_s v_i)|
 *   vertices [V][3] float32, object frame, CENTRED by the caller (centroid c subtracted), as for pxt_pose_errors.
 *   syms     [S][12]: R row-major then t of every symmetry transform, expressed for the centred vertices
 *       (t' = R c + t - c).  The caller puts the identity first if it wants it in the set.
 *   frames   [F][PXT_SYM_ERR_FRAME = 40]: rel(12) = T_gt^-1 T_est for the centred vertices (exactly
 *       evaluation.relative_poses), est(12) and gt(12) the world-to-camera poses for the centred vertices
 *       (t' = R c + t), then fx, fy, cx, cy.  All formed on the host in float64 and rounded once.
 *   per (f, s, i), all fp32, u the centred vertex: w = S_s u; d3 = |T_rel u - w| (the relative form of pxt_pose_errors:
 *       object-sized numbers only); d2 = |pi(T_est u) - pi(T_gt w)| with pi(p) = (fx p.x / p.z + cx, fy p.y / p.z + cy),
 *       IEEE division, a pinhole without lens terms as in BOP; d2 = +inf when either p.z is <= 0 or not finite.
 *       e3[s] = max_i d3, e2[s] = max_i d2; squared distances are compared and one sqrtf is taken at the end.
 *   record of frame f (PXT_SYM_ERR_RECORD = 8 floats):
 *       [0] MSSD = min_s e3[s]        [1] its s as a float (a tie takes the lowest index)
 *       [2] MSPD = min_s e2[s], in pixels; may be +inf        [3] its s
 *       [4] V    [5] S    [6] 0
 *       [7] status: 1.0 ok; -1.0 when the frame's 40 floats hold a non-finite value - then ONLY [7] is written
 *   Bounds: 1 <= V <= 2^20, 1 <= S <= PXT_SYM_ERR_MAX_SYMS, 1 <= F <= 65535, every pointer 4-byte aligned; anything
 *       else is PXT_E_ARG and nothing is launched or written.
 *   Deterministic: per-block maxima in the workspace, folded by a second launch; max and min are order-independent and
 *   there are no atomics: a frame's record depends on its own 40 floats, the vertices and the set only - not on F, on
 *   the frame's index or on the other frames.
 *   workspace: device memory of pxt_symmetric_pose_errors_workspace_bytes(F, S, V) bytes (< 0: unsupported sizes; up
 *   to 2 MiB per frame); one workspace serves one call at a time.  Two launches on `stream`, no host synchronisation. */
#define PXT_SYM_ERR_RECORD 8
#define PXT_SYM_ERR_FRAME 40
#define PXT_SYM_ERR_MAX_SYMS 1024
int64_t pxt_symmetric_pose_errors_workspace_bytes(int32_t n_frames, int32_t n_syms, int32_t n_vertices);
int pxt_symmetric_pose_errors(const float* vertices, int32_t n_vertices, const float* syms, int32_t n_syms,
                              const float* frames, int32_t n_frames, float* records, void* workspace, void* stream);

/* -------------------------------------------------------------------------
 * BOP's sensor-depth Visible Surface Discrepancy: two Depth renders and the frame's sensor depth image compared pixel
 * by pixel (opt-in; csrc/pxt_eval_vsd.hip).
 *
 * No reference counterpart.  pxt_depth_agreement takes the two render silhouettes as the visibility masks; with a
 * sensor depth image the masks are BOP's (Hodan et al., ECCV 2018 / BOP 2019, visib_mode = bop19, step cost): a pixel
 * an occluder hides counts neither for nor against the estimate, and the object's visible fraction falls out of the
 * same counts (pixtrack_amd/sensor_evaluation.py).
 *   depth_est, depth_gt [P][H][W][4] float32 (16-byte aligned; may be the same pointer): as for pxt_depth_agreement.
 *   sensor [P][H][W] uint16 (2-byte aligned; never NULL): the raw counts of the depth sensor, 0 = no measurement.
 *   ray    [H][W] float32 (4-byte aligned) or NULL (= 1.0f everywhere): the factor that turns a camera-axis depth into
 *       the length of the pixel's ray; shared by every pair.
 *   shift_x, shift_y: the sensor pixel of render pixel (x, y) is (x + shift_x, y + shift_y); a position outside the
 *       image reads nothing and counts as raw = 0.  No address outside the pair's own H x W counts is ever formed.
 *   per pixel, all fp32, every product and difference rounded on its own (no FMA contraction):
 *       sil(v) = v.w >= min_alpha && v.x > 0;  q(v) = v.x / v.w (correctly rounded);  r = ray[y][x];
 *       d_e = q(e) * r;  d_g = q(g) * r;  d_s = (float(raw) * sensor_q) * r;
 *       vis(d, sil) = sil && (d - d_s <= delta_q || raw == 0)      (bop19 visibility);
 *       vis_g = vis(d_g, sil(g));  vis_e = vis(d_e, sil(e)) || (vis_g && sil(e));  inter = vis_g && vis_e;
 *       dd = |d_e - d_g|;  within_k = inter && dd < tq[k] (strict; false for a NaN).  An `inter` pixel whose dd is NaN
 *       or inf counts in n_inter, is within no threshold and adds nothing to the sum or the max.
 *   sensor_q, delta_q, tq_host [n_taus] (host; they travel as kernel arguments): the distance of one raw count, the
 *       visibility tolerance and the thresholds, all in units of q - the caller divides by the depth-to-distance factor
 *       in float64 and rounds once.
 *   record of pair p (PXT_SENSOR_VSD_RECORD = 32 uint32 words, all written by the last launch):
 *       [0] n_vis_est   [1] n_vis_gt   [2] n_inter   [3] n_union = n_vis_est + n_vis_gt - n_inter
 *       [4] bits of float sum of the finite dd over `inter`   [5] bits of float max of the same (+0.0: none)
 *       [6] n_taus  [7] 1   [8] n_sil_est   [9] n_sil_gt   [10] pixels whose shifted sensor count is != 0
 *       [11..15] 0          [16 + k] n_within_k for k < n_taus, 0 for the rest
 *   Bounds: 1 <= P <= 65535, 1 <= n_taus <= 16, width, height >= 1 and width * height <= 2^28, |shift_x|, |shift_y| <=
 *       32767, the float images and the workspace 16-byte aligned, records and ray 4-byte, sensor 2-byte aligned;
 *       anything else is PXT_E_ARG and nothing is launched or written.
 *   Deterministic: counts by ballot + population count, the float sum and max through fixed-order reductions (wave
 *   butterfly, LDS, one partial per workgroup in the workspace, folded in a fixed order by a second launch), no
 *   atomics: a pair's record depends on its own three images, ray, the shift and the scalars only - not on P or on the
 *   pair's index.
 *   workspace: device memory of pxt_sensor_vsd_workspace_bytes(P, width, height) bytes (< 0: unsupported sizes); one
 *   workspace serves one call at a time.  Two launches on `stream`, no host synchronisation. */
#define PXT_SENSOR_VSD_MAX_TAUS 16
#define PXT_SENSOR_VSD_RECORD 32
int64_t pxt_sensor_vsd_workspace_bytes(int32_t n_pairs, int32_t width, int32_t height);
int pxt_sensor_vsd(const float* depth_est, const float* depth_gt, const uint16_t* sensor, const float* ray,
                   int32_t n_pairs, int32_t width, int32_t height, int32_t shift_x, int32_t shift_y, float min_alpha,
                   float sensor_q, float delta_q, const float* tq_host, int32_t n_taus, uint32_t* records,
                   void* workspace, void* stream);

/* -------------------------------------------------------------------------
 * Sensor-depth pose refinement behind the LM (opt-in; csrc/pxt_depth_refine.hip).
 *
 * No reference counterpart: the reference tracker is monocular.  Starting at a given pose - 12 floats, or the output
 * record of a pxt_lm_refine* launch queued ahead in the same stream, read ON THE DEVICE - a damped Gauss-Newton
 * minimises, over the problem's 3-D points X, the robust sum of r = D(u, v) - p.z: the depth sensor's value under the
 * projected point against the point's own camera depth.  All iterations of all problems run in ONE launch.
 *
 * Per point at pose T, all fp32, operation order of csrc/pxt_lm_point.h / pxt_common.h:
 *   p = transform_point(T, X);  (u, v), Jw = project_point, narrowed by point_in_window with conf.pad.
 *   reject codes: 1 masked out (point_mask), 2 projection failed (behind the camera or outside the distortion model's
 *       range), 3 outside the padded image - as pxt_lm_point_report - then
 *   bilinear_weights(u, v) -> (ix0, iy0), w00..w11; the twelve raw counts of the LM's cross footprint around (ix0, iy0)
 *       (rows 0 and 3: columns 1, 2; rows 1 and 2: columns 0..3, (ix0, iy0) being row 1, column 1).  A tap outside the
 *       image reads nothing and counts as raw 0; no address outside the height x width counts is formed.
 *       4 any raw == 0 (no measurement);  5 float(max raw - min raw) * sensor_scale > max_edge (depth edge);
 *   a_k = float(raw_k) * sensor_scale;  F, gx, gy: five bilinear values and central differences, as PXT_LM_POINT_CH;
 *   r = F - p.z;  6 |r| > max_residual (an occluder in front, the far side behind);  else 0, valid.
 *   rho, w = robust_loss(loss, loss_alpha, loss_scale, r * r);  J0, J1 = point_jacobian(Jw, p);
 *   J = gx * J0 + gy * J1 - (0, 0, 1, p.y, -p.x, 0)     (translation 3, rotation 3, left update: the LM's delta).
 * Per evaluation: cost = sum rho, n_valid, g = sum w r J, H = sum w J J^T over the valid points, the counts of codes
 *   1..6; then the prior: g += P a, H += P, a being the sum of the deltas applied so far (the first-order log of the
 *   accumulated update).  "Mean cost" is cost / max(n_valid, 1).
 * Per iteration: the LM's damped solve (H_kk += max(H_kk * lambda_k, 1e-6); Cholesky, pivoted LU when a pivot is not
 *   positive), the LM's update T <- (so3exp(dw), dt) T, a += delta, the log line, the LM's stop rule (|g| < grad_stop,
 *   or dt < dt_stop and dR < dR_stop; g includes the prior's term).  After the last update one more evaluation without
 *   an update gives the final cost.  n_valid < min_valid at ANY evaluation ends the run: failed, the pose stays the one
 *   that evaluation was made at.
 * log (optional): line i, PXT_DEPTH_LOG_STRIDE floats, in PXT_LM_LOG_STRIDE's layout: k = 0 mean cost before the update
 *   of iteration i, 1 n_valid, 2 dR (deg), 3 dt, 4 |g|, 5 1 if the solve fell back to LU, 6, 7 0, 8..19 the pose after the
 *   update.  codes (optional): row i holds the reject codes of evaluation i (iterations run + 1 rows are written).
 *
 * Output record (PXT_DEPTH_RECORD = 32 floats, device or pinned host; word 31 is stored last with system-scope release):
 *   [0..11] final pose   [12] failed   [13] iterations run (updates applied)
 *   [14] / [15] mean cost and n_valid at the initial pose      [16] / [17] the same at the final pose
 *   [18..23] counts of codes 1..6 at the final pose            [24..29] a, the accumulated update   [30] 0
 *   [31] 1.0 ok; -1.0 skipped (pose_is_lm_record and the LM record failed or timed out: ONLY word 31 is written, log
 *        and codes stay untouched); -2.0 stopped on n_valid < min_valid.
 *
 * One workgroup of 1024 threads per problem; point n belongs to thread n % 1024; sums fold in a fixed order (16-lane
 * DPP rows, the wave, the waves' partials in LDS by index), no atomics: a problem's output depends on that problem
 * alone - not on n_problems, its index, or the run.
 * Bounds: 1 <= n_problems <= PXT_DEPTH_MAX_PROBLEMS, 1 <= n_points <= PXT_DEPTH_MAX_POINTS, 0 <= num_iters <=
 * PXT_DEPTH_MAX_ITERS, pad >= 0, loss 0..2, min_valid >= 0, width, height >= 4 and width * height <= 2^30, ndist 0 / 2 /
 * 4; p3d, pose, out and the workspace 16-byte aligned, log 4-byte, sensor 2-byte aligned; the problems' `out` all
 * different.  Anything else is PXT_E_ARG and nothing is launched or written.
 * workspace: device, pxt_depth_refine_workspace_bytes(n_problems): the parameter records of a launch of more than two
 * problems (copied there from pinned staging memory ahead of the launch in `stream`; up to two travel as kernel
 * arguments); one workspace serves one launch at a time.
 * Measured on the MI355X: 102 us per call at 600 points, 154 us at 2048 (10 iterations, 640 x 480
 * sensor image; 9 - 14 us per evaluation), the same for 8 problems per launch as for one.
 * ---------------------------------------------------------------------- */
#define PXT_DEPTH_MAX_POINTS 4096
#define PXT_DEPTH_MAX_ITERS 32
#define PXT_DEPTH_MAX_PROBLEMS 16
#define PXT_DEPTH_RECORD 32        /* floats */
#define PXT_DEPTH_LOG_STRIDE 20    /* floats per logged iteration, layout of PXT_LM_LOG_STRIDE */
typedef struct {
  int32_t num_iters;               /* 0..PXT_DEPTH_MAX_ITERS; 0 = evaluate only */
  int32_t pad;                     /* as pxt_lm_conf.pad */
  int32_t loss;                    /* robust_loss on x = r * r, as the LM: 0 squared, 1 huber, 2 barron(alpha) */
  float loss_alpha, loss_scale;
  float lambda[6];                 /* damping, the LM's rule: H_kk += max(H_kk * lambda_k, 1e-6) */
  float max_residual;              /* |r| above this: rejected (occluder in front, far side behind) */
  float max_edge;                  /* depth range over the footprint above this: rejected (depth edge) */
  float grad_stop, dt_stop, dR_stop;  /* the LM's stop rule */
  int32_t min_valid;
} pxt_depth_conf;

typedef struct {
  const float* p3d;                /* [n_points][3] */
  const uint8_t* point_mask;       /* [n_points] or NULL */
  int32_t n_points;                /* 1..PXT_DEPTH_MAX_POINTS */
  const uint16_t* sensor;          /* [height][width] raw counts, 0 = no measurement */
  int32_t width, height;
  float sensor_scale;              /* SfM units per count */
  float cam[10];                   /* the query camera at the sensor image's size, LM convention */
  int32_t ndist;
  const float* pose;               /* device-readable, 16-byte aligned: 12 floats or an LM output record */
  int32_t pose_is_lm_record;       /* as pxt_lm_info_problem */
  float prior[21];                 /* symmetric 6x6 prior, upper triangle row-major, (t, w) order; zeros = none */
  float* out;                      /* PXT_DEPTH_RECORD floats, device or pinned host */
  float* log;                      /* [num_iters][PXT_DEPTH_LOG_STRIDE] or NULL */
  uint8_t* codes;                  /* [num_iters + 1][n_points] reject codes or NULL */
} pxt_depth_problem;

int64_t pxt_depth_refine_workspace_bytes(int32_t n_problems);
int pxt_depth_refine(const pxt_depth_problem* problems_host, int32_t n_problems, const pxt_depth_conf* conf_host,
                     void* workspace, void* stream);

/* -------------------------------------------------------------------------
 * Occlusion handling from the frame's sensor depth image (opt-in; csrc/pxt_occlusion.hip).
 *
 * No reference counterpart: the reference tracker masks the query with the silhouette at the last pose and refines on
 * every point that projects into the image - a hand in front of the object sits inside that silhouette.  With a sensor
 * depth image the pixels that show something IN FRONT of the object can be told (the bop19 visibility rule of
 * pxt_sensor_vsd, turned round), taken out of the frame's mask, and the points that project onto them out of the LM's
 * point mask.
 *
 * pxt_occlusion_mask - one image pair:
 *   depth  [H][W][4] float32 (16-byte aligned): a Depth render; .x = composited depth * depth_scale, .w = alpha (what
 *       pxt_points_from_depth and pxt_sensor_vsd read).
 *   sensor [H][W] uint16 (2-byte aligned): the raw counts of the depth sensor, 0 = no measurement.
 *   shift_x, shift_y: the sensor pixel of render pixel (x, y) is (x + shift_x, y + shift_y); a position outside the
 *       image reads nothing and counts as raw = 0.  No address outside the H x W counts is ever formed.
 *   mask_in [H][W] uint8: the frame's plain mask (pxt_depth_mask_plane's output; != 0 counts as 1).
 *   per pixel, all fp32, every step a single IEEE operation (no FMA contraction):
 *       sil = v.w >= min_alpha && v.x > 0;  q = v.x / v.w (correctly rounded);  d_s = float(raw) * sensor_q;
 *       O = sil && raw != 0 && (q - d_s > delta_q)           (false for a NaN; q - d_s == delta_q is NOT occluded);
 *   E = erosion of O with the (2 r_open + 1)^2 box, pixels outside the image ignored (OpenCV's default border, as
 *       pxt_depth_mask);  G = dilation of E with the (2 r_grow + 1)^2 box, inside the image;
 *   mask_out [H][W] uint8 = mask_in && !G;  occluder [H][W] uint8 = G; both 0 / 1, dense (four bytes are stored as one
 *       dword when W % 4 == 0 and mask_in, mask_out and occluder are all 4-byte aligned).  mask_out != occluder.
 *   sensor_q, delta_q (host; kernel arguments): the distance of one raw count and the tolerance in units of q - the
 *       caller divides by the depth-to-distance factor in float64 and rounds once.
 *   record (PXT_OCCLUSION_RECORD = 16 int32 words, device or pinned host, all written by the last launch):
 *       [0] n_sil   [1] n_measured (sil && raw != 0)   [2] n_occluded (O)   [3] n_opened (E)   [4] n_occluder (G)
 *       [5] n_mask_in   [6] n_mask_out   [7] n_sil_occluder (sil && G)   [8..10] 0: pxt_points_visible's   [11..15] 0
 *   Bounds: width, height >= 1 and width * height <= 2^28, r_open, r_grow >= 0 and r_open + r_grow <=
 *       PXT_OCCLUSION_MAX_RADIUS, |shift_x|, |shift_y| <= 32767, depth and the workspace 16-byte, record 4-byte, sensor
 *       2-byte aligned, no NULL; anything else is PXT_E_ARG and nothing is launched or written.
 *   Deterministic: 64 x 16 tiles on bit planes (wave ballots; shift-AND / shift-OR along x, row AND / OR along y), the
 *   counts by population count, one partial per workgroup in the workspace, folded in a fixed order by a second
 *   launch; no atomics: the outputs depend on the call's own inputs only.
 *   workspace: device memory of pxt_occlusion_mask_workspace_bytes(width, height) bytes (< 0: unsupported sizes); one
 *   workspace serves one call at a time.  Two launches on `stream`, no host synchronisation, no allocation.
 *
 * pxt_points_visible - the point gate, one launch behind it:
 *   p3d [N][3] float32; valid_in [N] uint8 or NULL (= all 1); pose12_host: the pose the points are seen from (row-major
 *   R, then t; host, by value); cam10_host / ndist: the UNSCALED query camera as in pxt_depth_problem.cam, cam[0] ==
 *   width and cam[1] == height; occluder [H][W] uint8: pxt_occlusion_mask's plane.
 *   per point: p = transform_point(T, X); (u, v) = project_point (csrc/pxt_common.h: the LM's projection, distortion
 *   included).  Texel k's centre is at coordinate k - the addressing of pxt_depth_refine's centre tap, whose weight is 1
 *   exactly there - so the point's pixel is (floor(u + 0.5), floor(v + 0.5)).  A point project_point refuses (behind the
 *   camera, outside the distortion model's range or outside the image) or whose texel is outside the image keeps its
 *   input value: the LM judges it as before.  Otherwise valid_out = valid_in && !occluder[texel].
 *   valid_out [N] uint8 (0 / 1; may be valid_in); record: the SAME 16 words, of which [8] n_points, [9] n_points_in
 *   (valid_in set) and [10] n_points_out (valid_out set) are written; integer counts by ballot, no atomics.
 *   Bounds: 0 <= N <= 2^24 (N = 0 writes the three words only; p3d and valid_out may then be NULL), ndist 0 / 2 / 4,
 *   sizes as above; anything else is PXT_E_ARG and nothing is launched or written.
 *
 * pxt_mask_exclude - a mask minus an occluder plane that another call made (pxt_mesh_render_scene_batch's: the other
 *   tracked objects of the image): mask_out [H][W] uint8 = (mask_in != 0) && !(occluder != 0), dense 0 / 1; mask_out may
 *   be mask_in, not occluder.  record (device or pinned host, 4-byte aligned): [0] n_mask_in, [1] n_mask_out; nothing
 *   else is written.  The rule is elementwise, so the planes are walked as H * W bytes: 16 at a time where mask_in,
 *   occluder and mask_out are all 16-byte aligned, four where 4-byte, the remainder (and unaligned planes) bytewise.
 *   mask_exclude_reference (pixtrack_amd/occlusion.py) restates it; the two agree bit for bit.
 *   Bounds: width, height >= 1 and width * height <= 2^28, no NULL; anything else is PXT_E_ARG and nothing is launched
 *   or written.  One launch of one workgroup on `stream`, counts by population count, no atomics, no workspace.
 *   Measured on the MI355X: DESIGN.md 3.20.
 * Measured on the MI355X: DESIGN.md 3.13.
 *
 * pxt_occlusion_mask_views - 1..PXT_OCCLUSION_MAX_VIEWS image pairs of different sizes in ONE chain of two launches
 *   (the K mesh objects of one RGB-D frame in lock-step tracking):
 *   views_host [n_views]: per view the five planes of pxt_occlusion_mask, its size, shift and quanta (host; the table
 *       travels in the kernel arguments: no upload).  Several views may name ONE sensor image (and one depth plane or
 *       one mask_in).  min_alpha, r_open, r_grow hold for the whole call.
 *   records [n_views][PXT_OCCLUSION_RECORD] int32 (device or pinned host); workspace: device memory of
 *       pxt_occlusion_mask_views_workspace_bytes(n_views, sizes) bytes, sizes = n_views x (width, height) (< 0: a count
 *       or a size out of range); one workspace serves one call at a time.
 *   View k's mask_out, occluder and 16 record words are bit for bit what pxt_occlusion_mask writes for that pair alone,
 *   whatever k is and whatever the other views are: the tile grids of the views are concatenated, a workgroup runs the
 *   single call's tile on its view's own tile, and one wave per view folds the view's partials in the single call's
 *   order.  No atomics.
 *   Bounds: those of pxt_occlusion_mask per view; every mask_out / occluder plane overlaps no other output plane, no
 *       input plane of any view (a view's mask_out may BE its own mask_in), nor records or workspace; anything else is
 *       PXT_E_ARG and nothing is launched or written.  Two launches on `stream`, no host synchronisation, no allocation.
 * ---------------------------------------------------------------------- */
#define PXT_OCCLUSION_RECORD 16
#define PXT_OCCLUSION_MAX_RADIUS 16
#define PXT_OCCLUSION_MAX_VIEWS 16
typedef struct pxt_occlusion_view {
  const float* depth;     /* [height][width][4] float32, 16-byte aligned */
  const uint16_t* sensor; /* [height][width] */
  const uint8_t* mask_in; /* [height][width] */
  uint8_t* mask_out;      /* [height][width] */
  uint8_t* occluder;      /* [height][width] */
  int32_t width, height;
  int32_t shift_x, shift_y;
  float sensor_q, delta_q;
} pxt_occlusion_view;
int64_t pxt_occlusion_mask_views_workspace_bytes(int32_t n_views, const int32_t* sizes);
int pxt_occlusion_mask_views(const pxt_occlusion_view* views_host, int32_t n_views, float min_alpha, int32_t r_open,
                             int32_t r_grow, int32_t* records, void* workspace, void* stream);
int64_t pxt_occlusion_mask_workspace_bytes(int32_t width, int32_t height);
int pxt_occlusion_mask(const float* depth, const uint16_t* sensor, const uint8_t* mask_in, int32_t width,
                       int32_t height, int32_t shift_x, int32_t shift_y, float min_alpha, float sensor_q,
                       float delta_q, int32_t r_open, int32_t r_grow, uint8_t* mask_out, uint8_t* occluder,
                       int32_t* record, void* workspace, void* stream);
int pxt_points_visible(const float* p3d, const uint8_t* valid_in, int32_t n_points, const float* pose12_host,
                       const float* cam10_host, int32_t ndist, const uint8_t* occluder, int32_t width, int32_t height,
                       uint8_t* valid_out, int32_t* record, void* stream);
int pxt_mask_exclude(const uint8_t* mask_in, const uint8_t* occluder, int32_t width, int32_t height, uint8_t* mask_out,
                     int32_t* record, void* stream);

/* -------------------------------------------------------------------------
 * NeRF mesh extraction: the iso-surface of a scalar lattice as an indexed triangle mesh, and BOP's diameter of a point
 * set (opt-in; csrc/pxt_iso.hip, pixtrack_amd/mesh.py).
 *
 * Reference: testbed.compute_and_save_marching_cubes_mesh (pixtrack/pose_trackers/pixloc_tracker_ycb.py:94).  The
 * triangulation here is marching TETRAHEDRA on the Freudenthal (Kuhn) split, about twice the triangles of marching
 * cubes: every cell with base corner c is cut into the six tetrahedra {c, c + e_a, c + e_a + e_b, c + (1,1,1)}, one per
 * permutation (a, b, .) of the axes in the order (x,y,z) (x,z,y) (y,x,z) (y,z,x) (z,x,y) (z,y,x).  Neighbouring cells
 * agree on every face diagonal: the mesh is a closed oriented 2-manifold wherever the surface stays inside the lattice.
 *
 * The rule (pixtrack_amd/mesh.py iso_surface_reference restates it in numpy; the two agree bit for bit):
 *   values [nz][ny][nx] float32; point p = (z * ny + y) * nx + x; inside when v >= iso (a NaN is outside).
 *   A point owns up to seven edges: E0 +x, E1 +y, E2 +z, E3 +x+y, E4 +y+z, E5 +x+z, E6 +x+y+z.  An edge exists when its
 *   far end is in the lattice and carries a vertex when its ends differ in inside-ness; vertex id = rank of
 *   (p, edge type) among the vertex-carrying edges.
 *   position: t = (iso - v_a) / (v_b - v_a), a NaN -> 0.5, else clamped to [0, 1];
 *       pos = origin + ((x, y, z) + t * d) * spacing per component, every product and sum a single fp32 operation.
 *   triangles: by cell (= its base point p), then tetrahedron, then triangle within the case.  One or three inside
 *       corners: one triangle over the three crossing edges, in the order of the three corners on the other side; two
 *       inside corners {a, b} and two outside {c, d}, each sorted by tet-local index: the quad ac, ad, bd, bc as
 *       (ac, ad, bd) and (ac, bd, bc).  Each triangle is wound so that its normal points from inside to outside; where
 *       that needs a turn, its second and third vertex are exchanged.  The winding is part of the case table, decided
 *       on the unit cube when the table is built, never from the data.
 *   normals (optional): the central-difference gradient of the lattice at the edge's two ends (one-sided at the border,
 *       0 along an axis of extent 1; divided by the spacing), interpolated with t, negated, normalised; a zero or
 *       non-finite length gives (0, 0, 0).
 *
 * pxt_iso_case_table: host only, needs no GPU.  out_host [6][16][7] int32: per (tetrahedron, code; bit i of the code =
 *   tet corner i inside): the number of triangles, then their vertices as (owner corner << 3) | edge type, the owner
 *   corner being dx | dy << 1 | dz << 2 inside the cell; unused slots -1.  The table is computed by the compiler from
 *   the unit cube; this copies what the kernels use.
 * pxt_iso_surface_count: three launches on `stream` - one thread per lattice point (edge mask, counts, exclusive scan per
 *   workgroup), then two levels that scan the workgroup totals.  counts (device or pinned host) [2] int32: vertices,
 *   triangles.  The workspace keeps the per-point records for pxt_iso_surface_emit.
 * pxt_iso_surface_emit: one launch, after the caller has read the counts and allocated vertices [n_vertices][3] float32,
 *   normals the same or NULL, triangles [n_triangles][3] int32.  values, grid and workspace are those of the count call,
 *   unchanged.  n_vertices / n_triangles are the sizes of the caller's arrays: nothing is written past them.
 * Bounds: every extent >= 1 and nx * ny * nz <= 2^27; a lattice without cells (any extent 1) is valid and has no
 *   triangles; values and the arrays 4-byte, the workspace 16-byte aligned; anything else is PXT_E_ARG and nothing is
 *   launched or written.  No atomics: the output is a pure function of the input.
 * workspace: device memory of pxt_iso_surface_workspace_bytes(nx, ny, nz) bytes (< 0: unsupported sizes).
 *
 * pxt_max_pairwise_distance - BOP's diameter: the maximum over all pairs of sqrt(dx^2 + dy^2 + dz^2) in fp32.
 *   points [n][3] float32.  out (device or pinned host) [4] int32: the bits of float d, i, j (i <= j), 1.  The squared
 *   distances are compared and one square root taken (sqrtf is monotone); ties go to the lowest (i, j); n = 1 gives
 *   (0, 0, 0); a point with a NaN is in no pair; no comparable pair at all gives (NaN, -1, -1).
 *   Targets tiled through LDS as in pxt_pose_errors, a partial per workgroup in the workspace, folded in a fixed order
 *   by a second launch; no atomics.  Bounds: 1 <= n <= 2^22, 4-byte alignment.  workspace: device memory of
 *   pxt_max_pairwise_distance_workspace_bytes(n) bytes.
 * Measured on the MI355X: DESIGN.md 3.14.
 * ---------------------------------------------------------------------- */
#define PXT_ISO_CASE_TABLE_WORDS (6 * 16 * 7)
typedef struct {
  int32_t nx, ny, nz;
  float iso;
  float origin[3];                 /* position of lattice point (0, 0, 0) */
  float spacing[3];                /* distance between neighbouring lattice points along x, y, z */
} pxt_iso_grid;

int pxt_iso_case_table(int32_t* out_host);
int64_t pxt_iso_surface_workspace_bytes(int32_t nx, int32_t ny, int32_t nz);
int pxt_iso_surface_count(const float* values, const pxt_iso_grid* grid_host, void* workspace, int32_t* counts,
                          void* stream);
int pxt_iso_surface_emit(const float* values, const pxt_iso_grid* grid_host, const void* workspace, float* vertices,
                         int32_t n_vertices, float* normals, int32_t* triangles, int32_t n_triangles, void* stream);
int64_t pxt_max_pairwise_distance_workspace_bytes(int32_t n_points);
int pxt_max_pairwise_distance(const float* points, int32_t n_points, void* workspace, int32_t* out, void* stream);

/* -------------------------------------------------------------------------
 * Mesh rasteriser: depth images of a triangle mesh through a pinhole camera (opt-in; csrc/pxt_raster.hip,
 * pixtrack_amd/mesh_render.py, pixtrack_amd/mesh_evaluation.py).
 *
 * Reference: render_image (pixtrack/utils/pytorch3d_render_utils.py:55-93) and the YCB ground-truth renders built on
 * it.  BOP's VSD compares depth renders of the model's mesh at the estimated and the ground-truth pose; this draws
 * them.  An evaluation rasteriser for an object in front of the camera: no shading, no anti-aliasing, no near-plane
 * clipping, no lens terms (vertex colours: pxt_mesh_render below).
 *
 * The rule (mesh_render.rasterize_reference restates it in numpy; the two agree bit for bit on every output):
 *   vertices [V][3] float32 (object frame); triangles [T][3] int32; views [P][PXT_MESH_VIEW = 20] float32:
 *       [0..8] R row-major, [9..11] t (world -> camera), [12..15] fx fy cx cy, [16] near, [17] depth_q, [18..19] 0 -
 *       formed on the host in float64 and rounded once.  A pinhole as in pxt_symmetric_pose_errors, in the Camera
 *       convention: pixel centres at integer coordinates, pixel (i, j) is sampled at image point (i, j).
 *   per vertex, every operation a single fp32 operation (no contraction, IEEE division):
 *       p_k = ((R_k0 v0 + R_k1 v1) + R_k2 v2) + t_k;   x = fx * (p.x / p.z) + cx, y likewise;
 *       X = (int) rintf(x * 256), Y likewise (eight sub-pixel bits);   iz = 1 / p.z.
 *       The vertex is "guard" when p is not finite; else "near" when p.z <= near; else "guard" when
 *       |rintf(x * 256)| < 2^23 does not hold, or the same for y (a non-finite x or y fails it too).
 *   per triangle, culled whole and counted under the FIRST of these causes that holds:
 *       bad index (one outside [0, V); no address outside the vertex array is formed); guard (any vertex); near (any
 *       vertex); zero area; off-screen.  A = (X1 - X0) (Y2 - Y0) - (Y1 - Y0) (X2 - X0) in int64; A == 0 is zero area;
 *       A < 0 exchanges the second and third vertex (X, Y, iz) and negates A.  No back-face culling.  Off-screen: the
 *       sub-pixel bounding box misses [0, 256 (W - 1)] x [0, 256 (H - 1)].  Every other triangle counts as drawn,
 *       whether or not a pixel centre falls inside it.
 *   coverage of pixel (i, j), P = (256 i, 256 j), inside the box clipped to the image: the edge functions
 *       e_0 over (v1, v2), e_1 over (v2, v0), e_2 over (v0, v1), e(a, b) = (Xb - Xa) (P.y - Ya) - (Yb - Ya) (P.x - Xa),
 *       in int64 (exact: |X| < 2^23).  The pixel belongs to the triangle when every e_k > 0, or e_k == 0 on a top or
 *       left edge: Yb - Ya < 0, or Yb - Ya == 0 and Xb - Xa > 0.  Two triangles that share an edge never both claim a
 *       pixel or both miss it; a closed mesh covers every pixel an even number of times.
 *   depth, perspective-correct: l_k = (float) e_k / (float) A; inv = (l_0 iz_0 + l_1 iz_1) + l_2 iz_2; z = 1 / inv.  A
 *       z that is not a positive finite number is not written by that triangle.
 *   depth test: the smallest z wins; on equal bits the lowest triangle index.
 *
 * out_depth [P][H][W][4] float32: a covered pixel holds z * depth_q in channels 0..2 and 1.0 in channel 3, background
 *   is four zeros - what a Depth-mode render writes (.x / .w the depth, .w the alpha), so the images go into
 *   pxt_depth_agreement, pxt_sensor_vsd, pxt_points_from_depth and pxt_occlusion_mask unchanged.
 * out_tri [P][H][W] int32 or NULL: the winning triangle's index, -1 on the background.
 * records [P][PXT_MESH_RASTER_RECORD = 16] uint32 (device memory, all written by the call):
 *   [0] covered pixels  [1] triangles drawn  [2] near  [3] guard  [4] zero area  [5] bad index  [6] off-screen
 *   [7] the bits of the smallest z written (0xffffffff when no pixel is covered)  [8] of the largest (0 likewise)
 *   [9] status: 0, or 0xffffffff (-1) when one of the view's 20 floats is not finite - that view's image is all
 *   background and its counts are 0  [10..15] 0 ([10], [11]: pxt_mesh_render_scene_batch's counts).
 * Deterministic: every pixel owns a 64-bit key (z bits << 32 | triangle index) in the workspace, resolved with a vector
 *   atomicMin (z > 0: the bits order as the floats; the minimum of a total order does not depend on arrival); the counts
 *   are integer adds, min / max z bit-pattern atomics.  A view's outputs are a pure function of the mesh and its 20
 *   floats: they do not depend on P, on the view's index or on scheduling.
 * Bounds: 1 <= P <= 4096, 1 <= V, T <= 2^24, width, height >= 1 and width * height <= 2^26, out_depth and the workspace
 *   16-byte, everything else 4-byte aligned, no NULL but out_tri; anything else is PXT_E_ARG and nothing is launched
 *   or written.
 * workspace: device memory of pxt_mesh_raster_workspace_bytes(P, T, width, height) bytes (< 0: unsupported sizes); one
 *   workspace serves one call at a time.  Four launches on `stream`, no host synchronisation, no allocation.
 * Measured on the MI355X: DESIGN.md 3.15.
 * ---------------------------------------------------------------------- */
#define PXT_MESH_VIEW 20
#define PXT_MESH_RASTER_RECORD 16
int64_t pxt_mesh_raster_workspace_bytes(int32_t n_views, int32_t n_triangles, int32_t width, int32_t height);
int pxt_mesh_raster(const float* vertices, int32_t n_vertices, const int32_t* triangles, int32_t n_triangles,
                    const float* views, int32_t n_views, int32_t width, int32_t height, float* out_depth,
                    int32_t* out_tri, uint32_t* records, void* workspace, void* stream);

/* -------------------------------------------------------------------------
 * Colour renders of a mesh with vertex colours: pxt_mesh_raster's images plus the colour half of the reference's
 * render_image (pixtrack/utils/pytorch3d_render_utils.py:55-93; scripts/create_sfm_from_obj.py renders its mapping
 * images with it: ambient light only, black background), and the two 8-bit planes the tracker takes from the NeRF
 * renderer.  csrc/pxt_raster.hip; mesh_render.shade_reference restates the rule in numpy and the two agree bit for bit
 * on every output.
 *
 * vertices, triangles, views, width, height, records, workspace (pxt_mesh_raster_workspace_bytes) and the bounds are
 * pxt_mesh_raster's; colors [V][3] float32, 0..1.  Coverage, depth, the depth test, out_depth, out_tri and records
 * follow the rule above and equal what pxt_mesh_raster writes for the same inputs bit for bit.
 *
 * The colour of a covered pixel whose winning triangle is t: the triangle is set up again exactly as for the depth
 *   (the same snapped X, Y, the same iz, the same exchange of the second and third vertex when A < 0 - the vertex colours
 *   are exchanged with them), the three int64 edge functions are evaluated at the pixel, and then, every step a single
 *   fp32 operation with IEEE division,
 *       l_k = (float) e_k / (float) A;   w_k = l_k * iz_k;   inv = (w_0 + w_1) + w_2   (the bits of the depth rule's inv);
 *       c = ((w_0 c_0 + w_1 c_1) + w_2 c_2) / inv   per channel;   c = fminf(fmaxf(c, 0), 1)   (a NaN becomes 0):
 *   perspective-correct interpolation of the vertex colours, no lighting term.
 * out_rgba [P][H][W][4] float32 or NULL: (r, g, b, 1) on a covered pixel, four zeros on the background.
 * out_rgb_u8 [P][H][W][3] uint8 or NULL: pxt_rgba_to_u8's rule on out_rgba with threshold 0, (long long)(c * 255.0f) & 255.
 * out_depth [P][H][W][4] float32 or NULL, out_tri [P][H][W] int32 or NULL: as pxt_mesh_raster.
 * out_depth_nz [P][H][W] uint8 or NULL: pxt_ngp_render_frame's depth_nz rule on out_depth's first channel d,
 *   ((long long)(d * 255.0f) & 255) != 0 - a d whose product with 255 lands in [256, 257) gives 0, as in the reference.
 *   (d * 255 below 2^63; the conversion of a larger product is not part of the rule.)
 * At least one of the five outputs is not NULL.  Alignment: out_rgba, out_depth and the workspace 16-byte; colors,
 *   out_rgb_u8, out_depth_nz, out_tri and everything else 4-byte (the byte planes are stored as whole dwords, whatever
 *   width * height is).  Anything else is PXT_E_ARG and nothing is launched or written.
 * Four launches on `stream`: pxt_mesh_raster's first three unchanged, then one resolve that writes every requested
 *   output and folds the record.  No host synchronisation, no allocation.  Measured on the MI355X: DESIGN.md 3.16.
 * ---------------------------------------------------------------------- */
int pxt_mesh_render(const float* vertices, int32_t n_vertices, const int32_t* triangles, int32_t n_triangles,
                    const float* colors, const float* views, int32_t n_views, int32_t width, int32_t height,
                    float* out_rgba, uint8_t* out_rgb_u8, float* out_depth, uint8_t* out_depth_nz, int32_t* out_tri,
                    uint32_t* records, void* workspace, void* stream);

/* -------------------------------------------------------------------------
 * Colour renders of a textured mesh: pxt_mesh_render with the colour read from a texture map through per-corner UVs,
 * what the reference's render_image draws for the meshes load_objs_as_meshes gives it (YCB's textured.obj with
 * texture_map.png; BOP's PLYs with texture_u / texture_v).  csrc/pxt_raster.hip; mesh_render.shade_textured_reference
 * restates the rule in numpy and the two agree bit for bit on every output.
 *
 * Everything but the colour is pxt_mesh_render's: vertices, triangles, views, the five outputs and their rules, records,
 * workspace, bounds and alignment; coverage, depth, out_depth, out_depth_nz, out_tri and records equal what
 * pxt_mesh_raster and pxt_mesh_render write for the same mesh bit for bit.  In place of colors:
 *   uvs [n_uvs][2] float32;   triangle_uvs [T][3] int32: corner k of triangle t uses uvs[triangle_uvs[t][k]] - corner
 *   attributes, so a vertex on a seam may carry different UVs in different triangles;   texture [Ht][Wt][4] uint8: r, g,
 *   b and a fourth byte that is ignored, one texel one aligned dword.
 *
 * The colour of a covered pixel whose winning triangle is t: the set-up, l_k, w_k and inv are pxt_mesh_render's (the UV
 *   indices follow the exchange of the second and third corner when A < 0), and then, every step a single fp32 operation
 *   with IEEE division,
 *       u = ((w_0 u_0 + w_1 u_1) + w_2 u_2) / inv, v likewise;
 *       x = u * (float)(Wt - 1);   y = (1.0f - v) * (float)(Ht - 1)   (row 0 of the map is v = 1);
 *       x = fminf(fmaxf(x, 0), Wt - 1), y likewise   (a NaN becomes 0; the border texels continue outwards);
 *       x0 = floorf(x), ax = x - x0, i0 = (int) x0, i1 = min(i0 + 1, Wt - 1);   j0, j1, ay from y likewise;
 *       per channel, a texel's value being tau = (float) byte / 255.0f:
 *       top = tau00 + ax (tau01 - tau00);   bot = tau10 + ax (tau11 - tau10);   c = top + ay (bot - top)
 *       (tau_ji = texel (i_i, j_j));   c = fminf(fmaxf(c, 0), 1):
 *   pytorch3d's TexturesUV with its defaults as render_image uses it - the map flipped vertically, align_corners=True,
 *   bilinear, padding_mode="border".  No lighting term, no mip levels, no wrap mode: the reference has none.
 * out_rgb_u8 truncates, (long long)(c * 255.0f) & 255: where (byte / 255.0f) * 255.0f rounds below the integer, the
 *   byte written is one less than the texel's, even on a pixel that reads one texel alone.  The reference's
 *   (image * 255).astype(uint8) does the same.
 * A triangle with a vertex index outside [0, V) is never drawn; one with a UV index outside [0, n_uvs) shades black
 *   (alpha 1, its depth and id as ever).  No address outside uvs or the texture is formed.
 * Bounds in addition to pxt_mesh_render's: uvs, triangle_uvs and texture not NULL and 4-byte aligned, 1 <= n_uvs <= 2^24,
 *   1 <= tex_width, tex_height <= 16384.  Anything else is PXT_E_ARG and nothing is launched or written.
 * Four launches on `stream`: pxt_mesh_raster's first three unchanged, then pxt_mesh_render's resolve instantiated with
 *   this shading rule.  No host synchronisation, no allocation.  Measured on the MI355X: DESIGN.md 3.17.
 * ---------------------------------------------------------------------- */
int pxt_mesh_render_textured(const float* vertices, int32_t n_vertices, const int32_t* triangles, int32_t n_triangles,
                             const float* uvs, int32_t n_uvs, const int32_t* triangle_uvs, const uint8_t* texture,
                             int32_t tex_width, int32_t tex_height, const float* views, int32_t n_views, int32_t width,
                             int32_t height, float* out_rgba, uint8_t* out_rgb_u8, float* out_depth,
                             uint8_t* out_depth_nz, int32_t* out_tri, uint32_t* records, void* workspace, void* stream);

/* -------------------------------------------------------------------------
 * A tracker frame's renders of a mesh in one call: up to PXT_MESH_FRAME_MAX_VIEWS = 8 views of one mesh, each with its
 * own size, its own supersampling factor and its own choice of outputs (opt-in; csrc/pxt_raster.hip,
 * mesh_render.frame_reference restates the rule in numpy and the two agree bit for bit on every output and record;
 * pixtrack_amd/mesh_template.py draws the tracker's depth_nz plane at the query camera and its anti-aliased 8-bit
 * template at the reference camera with it).
 *
 * vertices, triangles, views [P][20], records [P][16] and their bounds are pxt_mesh_raster's.  The mesh is shaded by
 * vertex colours (colors [V][3] as pxt_mesh_render; uvs, triangle_uvs and texture NULL) or by a texture map (uvs, n_uvs,
 * triangle_uvs, texture, tex_width, tex_height as pxt_mesh_render_textured; colors NULL): exactly one of the two.
 * geometry [P][3] int32 (HOST memory): width W, height H and supersample S of each view, S in {1, 2, 4}.
 *
 * The fine view.  View p is rasterised on the fine lattice W' = S W, H' = S H through the fine view record, formed on
 *   the device from its 20 floats, each step a single fp32 operation:
 *       fx' = fx * (float)S;   fy' = fy * (float)S;   cx' = cx * (float)S + 0.5f * (float)(S - 1);   cy' likewise;
 *   everything else unchanged.  In the Camera convention (pixel centres at integer coordinates) fine pixel
 *   (S i + a, S j + b) is the sample of output pixel (i, j) at offset ((a + 0.5) / S - 0.5, (b + 0.5) / S - 0.5).
 *   Coverage, the depth test and the colour of a fine pixel are exactly pxt_mesh_raster's and
 *   pxt_mesh_render(_textured)'s rules on that W' x H' view.
 * out_rgba, per view [H][W][4] float32: per channel, the fine pixels of the S x S block in row-major order (b outer, a
 *   inner) - a covered one contributes (r, g, b, 1), an uncovered one four zeros; start from the first, add the next
 *   with one fp32 add each, multiply by 1.0f / (S * S) (exact).  Colour premultiplied over black, alpha the covered
 *   fraction: what a Shade render on the black background gives at a silhouette.
 * out_rgb_u8, per view [H][W][3] uint8: (long long)(c * 255.0f) & 255 on the first three channels of that.
 * out_depth, per view [H][W][4] float32, and out_depth_nz, per view [H][W] uint8: pxt_mesh_render's, for S = 1 alone.
 * Where the outputs go.  The four out_* pointers are the bases of four buffers of out_bytes[0..3] bytes (HOST array;
 *   a buffer no view uses may be NULL); out_offsets [P][4] int64 (HOST memory) holds, per view and in the order rgba,
 *   rgb_u8, depth, depth_nz, the byte offset of that view's plane in its buffer, or -1 for an output the view does not
 *   ask for.  Every view names at least one.  The planes of one call must not overlap.
 * records: pxt_mesh_raster's record of the fine view - the counts are fine pixels; the status is -1 and the image all
 *   background when one of the fine view's 20 floats is not finite.
 * With S = 1 every output and record equals pxt_mesh_render(_textured) on the same view bit for bit.  A view's outputs
 *   are a pure function of the mesh and that view's 20 floats, size and S: they do not depend on P, on the view's
 *   index, on the other views' sizes or on scheduling.
 * Bounds: 1 <= P <= 8; W, H >= 1 and W' * H' <= 2^26 per view; a depth output asked for with S > 1, an offset that is not
 *   a multiple of 16 (rgba, depth) or 4 (the byte planes: they are stored as whole dwords), a plane that does not fit
 *   its buffer, a view without output, both or neither shading inputs; plus the alignment and NULL rules of
 *   pxt_mesh_render(_textured).  Anything else is PXT_E_ARG and nothing is launched or written.
 * workspace: device memory of pxt_mesh_render_frame_workspace_bytes(P, T, geometry) bytes (< 0: unsupported), 16-byte
 *   aligned.  Four launches on `stream` for any P - clear, triangle and list as pxt_mesh_raster's, generalised to a
 *   per-view table (fine size, key-plane offset, S) that rides in the kernel arguments with the view as the grid's
 *   second dimension, and one resolve, one lane per output pixel.  No host synchronisation, no allocation.
 *   Measured on the MI355X: DESIGN.md 3.18.
 * ---------------------------------------------------------------------- */
#define PXT_MESH_FRAME_MAX_VIEWS 8
int64_t pxt_mesh_render_frame_workspace_bytes(int32_t n_views, int32_t n_triangles, const int32_t* geometry);
int pxt_mesh_render_frame(const float* vertices, int32_t n_vertices, const int32_t* triangles, int32_t n_triangles,
                          const float* colors, const float* uvs, int32_t n_uvs, const int32_t* triangle_uvs,
                          const uint8_t* texture, int32_t tex_width, int32_t tex_height, const float* views,
                          int32_t n_views, const int32_t* geometry, const int64_t* out_offsets, float* out_rgba,
                          uint8_t* out_rgb_u8, float* out_depth, uint8_t* out_depth_nz, const int64_t* out_bytes,
                          uint32_t* records, void* workspace, void* stream);

/* -------------------------------------------------------------------------
 * Lock-step tracking from mesh templates: n_views (<= PXT_MESH_BATCH_MAX_VIEWS) views of up to
 * PXT_MESH_BATCH_MAX_MESHES DIFFERENT meshes in ONE chain of launches on ONE stream (opt-in; csrc/pxt_raster.hip,
 * mesh_render.render_frame_batch, MeshTemplate.frames, MultiObjectTracker).  Each view names its mesh and has its own
 * size, supersample and choice of outputs.
 *
 * meshes [M] (HOST array): per mesh what pxt_mesh_render_frame takes - vertices, n_vertices, triangles, n_triangles and
 *   exactly one shading group: colors (uvs, triangle_uvs, texture NULL) or uvs, n_uvs, triangle_uvs, texture, tex_width,
 *   tex_height (colors NULL).  The pointers are device memory.  A mesh that no view names is allowed (it is still
 *   checked), and so are descriptors that name the same arrays.
 * view_mesh [P] int32 (HOST): the mesh of each view, 0 <= view_mesh[p] < M.
 * views [P][20] float32 (HOST memory, unlike pxt_mesh_render_frame's): the 20 floats of every view travel in the
 *   call's parameter record, so the per-frame view uploads of K trackers are one.
 * geometry [P][3], out_offsets [P][4], out_rgba / out_rgb_u8 / out_depth / out_depth_nz, out_bytes [4] and
 *   records [P][16] are exactly pxt_mesh_render_frame's.
 * The rule.  Every output plane and the record of view p equal, bit for bit, what pxt_mesh_render_frame writes for that
 *   view alone on mesh view_mesh[p]: a view's outputs are a pure function of its mesh, its 20 floats, its size and S -
 *   they do not depend on M, P, the view's index, the other meshes or scheduling.
 * Bounds: pxt_mesh_render_frame's per view and per mesh, 1 <= M <= 16, 1 <= P <= 32, 0 <= view_mesh[p] < M.  Anything
 *   else is PXT_E_ARG and nothing is launched or written.
 * workspace: device memory of pxt_mesh_render_frame_batch_workspace_bytes(M, n_triangles [M], P, view_mesh, geometry)
 *   bytes (< 0: unsupported), 16-byte aligned: the views' key planes, every view's own triangle list of
 *   min(T of its mesh, 16384) entries, and the call's parameter record (the mesh table, the view table, the views'
 *   floats), which is uploaded with one asynchronous copy on `stream` ahead of the launches.  The workspace must stay
 *   untouched until the chain has finished: one workspace per stream is enough, two streams must not share one.
 * Launches on `stream`: clear, triangle (the grid's first dimension is the largest mesh's, the second the view; a
 *   workgroup beyond its own mesh's triangles exits at once), list, and one resolve per shading kind that occurs -
 *   four when all meshes share a kind, five when they are mixed, for any M and P.  No host synchronisation other than
 *   the wait for the staging block's previous copy (a ring of pinned blocks per thread and device, allocated on first
 *   use), no other allocation.  Measured on the MI355X: DESIGN.md 3.19.
 * ---------------------------------------------------------------------- */
#define PXT_MESH_BATCH_MAX_MESHES 16
#define PXT_MESH_BATCH_MAX_VIEWS 32
typedef struct pxt_mesh_desc {
  const float* vertices;        /* [n_vertices][3] */
  const int32_t* triangles;     /* [n_triangles][3] */
  const float* colors;          /* [n_vertices][3], or NULL for a textured mesh */
  const float* uvs;             /* [n_uvs][2] */
  const int32_t* triangle_uvs;  /* [n_triangles][3] */
  const uint8_t* texture;       /* [tex_height][tex_width][4] */
  int32_t n_vertices, n_triangles, n_uvs, tex_width, tex_height, reserved;
} pxt_mesh_desc;
int64_t pxt_mesh_render_frame_batch_workspace_bytes(int32_t n_meshes, const int32_t* n_triangles, int32_t n_views,
                                                    const int32_t* view_mesh, const int32_t* geometry);
int pxt_mesh_render_frame_batch(const pxt_mesh_desc* meshes, int32_t n_meshes, const int32_t* view_mesh,
                                const float* views, int32_t n_views, const int32_t* geometry,
                                const int64_t* out_offsets, float* out_rgba, uint8_t* out_rgb_u8, float* out_depth,
                                uint8_t* out_depth_nz, const int64_t* out_bytes, uint32_t* records, void* workspace,
                                void* stream);

/* -------------------------------------------------------------------------
 * Lock-step tracking of objects that share an image: pxt_mesh_render_frame_batch plus, per view, the pixels where
 * ANOTHER view of the same scene lies in front (opt-in; csrc/pxt_raster.hip, mesh_render.render_frame_batch(scenes=),
 * MeshTemplate.frames, MultiObjectTracker(mutual_occlusion=)).  The occluders of a lock-step step are known exactly:
 * they are the other tracked meshes, and their per-pixel z already sits in the call's key planes.
 *
 * Everything pxt_mesh_render_frame_batch takes, and:
 *   view_scene [P] int32 (HOST): the scene of each view, -1 = the view is in no scene.  A scene id is any number in
 *       [0, P); the views that name the same number are that scene's members.
 *   r_grow: the occluder plane is grown by the (2 r_grow + 1)^2 box, 0 <= r_grow <= 8.
 *   out_occluder: the base of a uint8 device buffer of occluder_bytes bytes (may be NULL when no view wants a plane);
 *   occluder_offsets [P] int64 (HOST): the byte offset of the view's [H][W] uint8 plane in it, a multiple of 4, or -1
 *       for a view that does not want the plane.  The planes of one call must not overlap.
 * The rule (mesh_render.scene_reference restates it in numpy on its own key planes; the two agree bit for bit, no
 * tolerance, no excluded pixel):
 *   Every output plane and record words [0..9] of every view equal, bit for bit, what pxt_mesh_render_frame_batch writes
 *       for the same arguments: a scene changes nothing that exists.
 *   For view k with view_scene[k] = s >= 0, the other members are the views j != k with view_scene[j] = s;
 *       H_k(x) = key_k(x) != empty && exists j: key_j(x) != empty && zbits_j(x) < zbits_k(x), zbits the high 32 bits of
 *       the 64-bit key: the bits of the UNSCALED camera z (near and depth_q may differ between members).  Equal bits do
 *       NOT hide: two copies of one mesh at one pose hide nothing of each other.  The plane of a view is a pure function
 *       of its own inputs and the SET of the other members - not of the view order, M, P, views outside the scene or
 *       scheduling.  A scene of one member yields an all-zero plane.
 *   G_k = the dilation of H_k with the (2 r_grow + 1)^2 box, pixels outside the image ignored (pxt_occlusion_mask's G).
 *   out_occluder of view k = G_k, dense 0 / 1 bytes (four bytes as one dword when W % 4 == 0).
 *   records [P][16]: [10] n_hidden = the population of H_k, [11] n_occluder = of G_k, for scene views that want the
 *       plane, 0 otherwise; integer adds, deterministic.
 * Bounds, in addition to pxt_mesh_render_frame_batch's: a scene member with S != 1; members of one scene that differ in
 *   width or height or whose view floats [12..15] (fx fy cx cy) are not bit-equal; view_scene[p] outside [-1, P); an
 *   occluder offset on a view with view_scene = -1; r_grow outside 0..8; a plane that is not 4-byte aligned or does not
 *   fit the buffer; view_scene or occluder_offsets NULL.  Anything else is PXT_E_ARG and nothing is launched or written.
 * workspace: pxt_mesh_render_scene_batch_workspace_bytes(...) bytes (the batch call's plus the scene table, which
 *   travels in the same parameter record and the same one copy).
 * Launches: pxt_mesh_render_frame_batch's, and ONE more when at least one view wants a plane - 64 x 16 tiles with an
 *   r_grow halo, H from the members' keys (their high words alone) as wave ballots, shift-OR / row-OR dilation on bit
 *   planes, counts by population count.  It reads only finished keys and runs between the list launch and the resolves:
 *   the S = 1 key planes it reads were written last and are read again next.  No host synchronisation and no allocation
 *   beyond the batch call's.  Measured on the MI355X: DESIGN.md 3.20.
 * ---------------------------------------------------------------------- */
#define PXT_MESH_SCENE_MAX_GROW 8
int64_t pxt_mesh_render_scene_batch_workspace_bytes(int32_t n_meshes, const int32_t* n_triangles, int32_t n_views,
                                                    const int32_t* view_mesh, const int32_t* geometry);
int pxt_mesh_render_scene_batch(const pxt_mesh_desc* meshes, int32_t n_meshes, const int32_t* view_mesh,
                                const float* views, int32_t n_views, const int32_t* geometry,
                                const int64_t* out_offsets, float* out_rgba, uint8_t* out_rgb_u8, float* out_depth,
                                uint8_t* out_depth_nz, const int64_t* out_bytes, const int32_t* view_scene,
                                int32_t r_grow, uint8_t* out_occluder, int64_t occluder_bytes,
                                const int64_t* occluder_offsets, uint32_t* records, void* workspace, void* stream);

/* -------------------------------------------------------------------------
 * Render-ahead for mesh templates: pxt_mesh_render_frame_batch whose views take their pose ON THE DEVICE from the
 * output record of an LM launch queued ahead of the call on the same stream (opt-in; csrc/pxt_raster.hip,
 * mesh_render.render_frame_batch(poses=), MeshTemplate.frames_ahead, PixLocPoseTrackerR9 with a
 * MeshTemplate(render_ahead=True)).  The host forms the part of a view record that does not change between frames;
 * the pose and depth_q are filled in by one small launch once the refinement has written them, so the host need not
 * wait for the pose before it queues the frame's renders.
 *
 * Every argument of pxt_mesh_render_frame_batch, and:
 *   view_pose [P] (HOST array): per view the record its pose comes from.  pose_record: >= 16 float32 that the device
 *       can read (device memory or pinned host memory), laid out as pxt_lm_refine's `out` - [0..11] the pose (R
 *       row-major, then t), [12] failed, [13] status - or NULL for a view drawn from its 20 host floats.  radius: the
 *       farthest a vertex of the view's mesh lies from the mesh frame's origin (MeshTemplate.radius); ignored when
 *       pose_record is NULL.  Several views may name one record.
 *   views_out [P][PXT_MESH_VIEW_OUT] float32, pinned host or device memory, or NULL.
 * The rule (mesh_render.posed_view_reference restates it in float64; the two agree bit for bit):
 *   A view with pose_record == NULL is drawn from views[p][0..19], exactly as pxt_mesh_render_frame_batch draws it.
 *   A posed view p is drawn from the 20 floats v with
 *       v[12..16] = views[p][12..16] (fx fy cx cy near), v[18..19] = views[p][18..19],
 *       v[0..11]  = pose_record[0..11], a bit copy; with t = pose_record[9..11]
 *       v[17]     = (float)(1.0 / (sqrt(((double)t0*t0 + (double)t1*t1) + (double)t2*t2) + radius)):
 *                   every step one IEEE float64 operation in that order, nothing contracted, rounded to float32 once.
 *       views[p][0..11] and views[p][17] of a posed view are ignored.
 *   Every plane and record of a view equal, bit for bit, what pxt_mesh_render_frame_batch draws from the same 20
 *       floats: the rendering launches are that call's own kernels.
 *   views_out[p][0..19] = v for a posed view; [20] = 1.0 when pose_record[12] == 0 && pose_record[13] == 0, else
 *       -1.0; [21..23] = 0.  Word [20] is stored last, with a system-scope release (pxt_lm_refine_cam's cam_out13
 *       convention): a host that polls pinned memory may read the row once it sees the word.  Rows of un-posed views
 *       are not written.
 *   A posed view is drawn whatever the flag says: after a failed refinement out[0..11] holds a finite pose, and the
 *       caller discards the planes.  Non-finite floats in the record are not special-cased: they fall under the view
 *       rule of pxt_mesh_raster (record status -1, an all-background image).
 * Bounds: pxt_mesh_render_frame_batch's, and view_pose not NULL; a posed view's radius finite and >= 0; pose_record
 *   and views_out 4-byte aligned.  Anything else is PXT_E_ARG and nothing is launched or written.
 * workspace: pxt_mesh_render_frame_batch_workspace_bytes(...) bytes serve this call too - the posed views' floats are
 *   overwritten in place inside the uploaded parameter record, nothing is added to it.
 * Launches on `stream`: pxt_mesh_render_frame_batch's plus ONE - a single wave, one lane per view, after the
 *   parameter record's asynchronous upload and before the clear launch (no launch is added when no view is posed).
 *   No host synchronisation beyond the staging ring's, no allocation.  Measured on the MI355X: DESIGN.md 3.22.
 * ---------------------------------------------------------------------- */
typedef struct {
  const float* pose_record; /* device-readable (device or pinned host) LM output record, >= 16 floats, or NULL */
  double radius;            /* MeshTemplate.radius of the view's mesh; ignored when pose_record == NULL */
} pxt_mesh_view_pose;
#define PXT_MESH_VIEW_OUT 24   /* 20 view floats, [20] completion word, [21..23] 0 */
int pxt_mesh_render_frame_batch_posed(const pxt_mesh_desc* meshes, int32_t n_meshes, const int32_t* view_mesh,
                                      const float* views, int32_t n_views, const int32_t* geometry,
                                      const int64_t* out_offsets, float* out_rgba, uint8_t* out_rgb_u8,
                                      float* out_depth, uint8_t* out_depth_nz, const int64_t* out_bytes,
                                      uint32_t* records, void* workspace, const pxt_mesh_view_pose* view_pose,
                                      float* views_out, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* PIXTRACK_HIP_H */
