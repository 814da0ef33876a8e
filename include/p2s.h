/*
 * p2s.h -- C-ABI of the MI355X-native multi-view triangulation / person-association engine.
 *
 * Drop-in boundary for the hot path of Pose2Sim.triangulation() / Pose2Sim.personAssociation().
 * The reference is pure Python with no FFI of its own; each entry point below replaces the inner
 * loops of one reference function (citations relative to /root/reference/Pose2Sim/) and is what a
 * reference-side ctypes binding would call (INTEGRATION.md shows that binding).
 *
 * Conventions
 *   - plain pointers and sizes only; no exceptions cross the ABI; every call returns a status
 *     (0 = ok, <0 = error) and p2s_last_error() returns the message of the calling thread's
 *     last failure.
 *   - one context per GPU per process; a context is not re-entrant.
 *   - "_device" entry points take DEVICE pointers and enqueue on the context's stream without
 *     synchronising; "_host" entry points take HOST pointers, copy in/out and block.  One exception:
 *     p2s_triangulate_device on the work-list path (undistortion, L/R swap, or more than 16 cameras) with a camera
 *     count whose subset levels can exceed 4 096 subsets (15 cameras or more, min_cameras permitting) reads a 4-byte
 *     count after each chunk's search to drive the deep-level rounds, i.e. it synchronises the stream.
 *   - observation tensor layout: xyl[n_blocks][C][K][3] (x px, y px, likelihood), one block
 *     per (frame, person); NaN = missing.  dtype float32 or float64 (P2S_F32 / P2S_F64).  A detection whose
 *     coordinates are not finite is taken as missing whatever its likelihood (the reference reaches the same result one
 *     search level later); one whose likelihood is exactly 0 must carry finite coordinates (pose estimators write
 *     (0, 0, 0)) or be NaN throughout.
 *   - camera count C <= P2S_MAX_CAMS (the excluded-camera set is returned as a 32-bit mask).
 */
#ifndef P2S_H
#define P2S_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define P2S_MAX_CAMS 32
#define P2S_MAX_PERSONS_TOTAL 48   /* association: sum over cameras of detected persons per frame */

#define P2S_OK 0
#define P2S_ERR_INVALID_ARG (-1)
#define P2S_ERR_HIP (-2)
#define P2S_ERR_NO_DEVICE (-3)
#define P2S_ERR_NO_CALIB (-4)
#define P2S_ERR_OOM (-5)                /* device or host memory; what the call wrote to its outputs is unspecified */

#define P2S_F32 0
#define P2S_F64 1

typedef struct p2s_ctx p2s_ctx;

/* Parameters of triangulation_from_best_cameras (triangulation.py:389-393) plus the likelihood
 * mask applied by its caller (triangulation.py:686, 817-821). */
typedef struct p2s_tri_params {
    double reproj_error_threshold;  /* [triangulation] reproj_error_threshold_triangulation, px */
    double likelihood_threshold;    /* [triangulation] likelihood_threshold_triangulation       */
    int32_t min_cameras;            /* [triangulation] min_cameras_for_triangulation (>= 1)     */
    int32_t undistort_points;       /* [triangulation] undistort_points  (0/1)                  */
    int32_t handle_lr_swap;         /* [triangulation] handle_LR_swap    (0/1)                  */
    int32_t reserved;
} p2s_tri_params;

/* Parameters of the multi-person association (personAssociation.py:670-673, 799-801). */
typedef struct p2s_assoc_params {
    double reconstruction_error_threshold; /* [personAssociation.multi_person], metres */
    double min_affinity;                   /* [personAssociation.multi_person]         */
    int32_t min_cameras;                   /* [triangulation] min_cameras_for_triangulation */
    int32_t max_iter;                      /* matchSVT max_iter (reference: 20)  */
    double w_rank;                         /* matchSVT w_rank   (reference: 50)  */
    double tol;                            /* matchSVT tol      (reference: 1e-4)*/
    double w_sparse;                       /* matchSVT w_sparse (reference: 0.1) */
} p2s_assoc_params;

int p2s_version(void);
const char *p2s_last_error(void);

/* Number of visible HIP devices (0 without a GPU; never fails the process). */
int p2s_device_count(int *count);

/* Create / destroy the per-GPU context (device buffers, stream, calibration). */
int p2s_create(int device_id, p2s_ctx **out);
int p2s_destroy(p2s_ctx *ctx);

/* Enqueue on the caller's HIP stream (e.g. torch.cuda.current_stream().cuda_stream; NULL = HIP's
 * default stream).  A fresh context uses a private non-blocking stream. */
int p2s_set_stream(p2s_ctx *ctx, void *hip_stream);
int p2s_synchronize(p2s_ctx *ctx);

/* Calibration of C cameras, the outputs of computeP (common.py:291-324) and
 * retrieve_calib_params (common.py:254-288), all HOST pointers, float64, row-major:
 *   P[C][12]      projection matrices (built from optim_K when undistorting)
 *   Kmat[C][9]    original intrinsics               (may be NULL if never undistorting/associating)
 *   dist[C][5]    k1,k2,p1,p2,k3                    (may be NULL)
 *   Rmat[C][9]    rotation matrices                 (may be NULL)
 *   T[C][3]       translations                      (may be NULL)
 *   newK[C][9]    optim_K                           (may be NULL)
 */
int p2s_set_calibration(p2s_ctx *ctx, int32_t n_cams, const double *P, const double *Kmat,
                        const double *dist, const double *Rmat, const double *T, const double *newK);

/* Robust triangulation of every (block, keypoint) unit: replaces the frame / person / keypoint
 * loops of triangulate_all (triangulation.py:796-845) around triangulation_from_best_cameras
 * (triangulation.py:363-604), including undistortion (:808-813) and the likelihood mask
 * (:817-821).
 *   xyl       [n_blocks][C][K][3], dtype P2S_F32 or P2S_F64
 *   swap_idx  [K] keypoints_idx_swapped (triangulation.py:745); may be NULL when !handle_lr_swap
 * outputs, one per unit u = block*K + k:
 *   Q        [n][3] float64  3D point (NaN when rejected)
 *   err      [n]    float32  mean reprojection error px (NaN when rejected)
 *   n_excl   [n]    uint8    nb_cams_excluded
 *   excl_mask[n]    uint32   bit c set <=> camera c in id_excluded_cams
 */
int p2s_triangulate_device(p2s_ctx *ctx, int64_t n_blocks, int32_t n_kpts, int32_t dtype,
                           const void *d_xyl, const int32_t *d_swap_idx, const p2s_tri_params *params,
                           double *d_Q, float *d_err, uint8_t *d_n_excl, uint32_t *d_excl_mask);
int p2s_triangulate_host(p2s_ctx *ctx, int64_t n_blocks, int32_t n_kpts, int32_t dtype,
                         const void *xyl, const int32_t *swap_idx, const p2s_tri_params *params,
                         double *Q, float *err, uint8_t *n_excl, uint32_t *excl_mask);

/* Multi-person association of every frame: replaces the per-frame body of associate_all
 * (personAssociation.py:783-801): compute_rays (:277-316), compute_affinity (:347-408),
 * circular_constraint (:411-428), matchSVT (:450-509) and the min_affinity cut (:800).
 *   n_persons [F][C]  int32   persons detected per camera (read_json, :260-274)
 *   offsets   [F+1]   int64   start of each frame's rows in kpts (rows = sum_c n_persons[f][c])
 *   kpts      [rows][Kj][3]   dtype P2S_F32/P2S_F64: camera-major, then person, JSON keypoint order
 * output:
 *   affinity  [F][Nmax][Nmax] float64, the thresholded matchSVT result, top-left N_f x N_f valid
 *             (N_f = sum_c n_persons[f][c] <= Nmax <= P2S_MAX_PERSONS_TOTAL)
 * The order-sensitive proposal extraction (person_index_per_cam, :512-549) stays on the host.
 */
int p2s_associate_device(p2s_ctx *ctx, int64_t n_frames, int32_t n_kpts_json, int32_t n_max, int32_t dtype,
                         const int32_t *d_n_persons, const int64_t *d_offsets, const void *d_kpts,
                         const p2s_assoc_params *params, double *d_affinity);
int p2s_associate_host(p2s_ctx *ctx, int64_t n_frames, int32_t n_kpts_json, int32_t n_max, int32_t dtype,
                       const int32_t *n_persons, const int64_t *offsets, const void *kpts,
                       const p2s_assoc_params *params, double *affinity);

/* Parameters of the single-person association (personAssociation.py:177-180). */
typedef struct p2s_single_params {
    double reproj_error_threshold;  /* [personAssociation.single_person] reproj_error_threshold_association, px */
    double likelihood_threshold;    /* [personAssociation] likelihood_threshold_association               */
    int32_t min_cameras;            /* [triangulation] min_cameras_for_triangulation (>= 1)                */
    int32_t reserved;
} p2s_single_params;

/* Single-person association of every frame: replaces persons_combinations (personAssociation.py:67-99)
 * and best_persons_and_cameras_combination (:154-257, pinhole branch) with triangulate_comb (:102-151):
 * every combination of one person per camera x every subset of cameras switched off, in the
 * reference's visiting order and with its carry-over rules.
 *   n_persons [F][C]  int32   persons per camera (read_json order), each <= P2S_MAX_PERSONS_PER_CAM
 *   offsets   [F+1]   int64   start of each frame's rows in tracked
 *   tracked   [rows][3]       (x, y, likelihood) of the tracked keypoint of every person, camera-major,
 *                             dtype P2S_F32 / P2S_F64
 * outputs per frame:
 *   comb [F][C] int32  chosen person per camera, -1 = camera off / nothing detected (NaN in the reference)
 *   err  [F]    f64    best reprojection error (inf when no combination could be triangulated)
 *   Q    [F][3] f64    the tracked keypoint in 3D for that combination
 * The product of the per-camera person counts of a frame must not exceed P2S_MAX_COMBINATIONS. */
#define P2S_MAX_PERSONS_PER_CAM 16
#define P2S_MAX_COMBINATIONS (1 << 20)
#define P2S_MAX_SINGLE_SEARCH 2147483648.0  /* worst-case (combination, camera subset) evaluations per frame */
int p2s_associate_single_device(p2s_ctx *ctx, int64_t n_frames, int32_t dtype, const int32_t *d_n_persons,
                                const int64_t *d_offsets, const void *d_tracked, const p2s_single_params *params,
                                int32_t *d_comb, double *d_err, double *d_Q);
int p2s_associate_single_host(p2s_ctx *ctx, int64_t n_frames, int32_t dtype, const int32_t *n_persons,
                              const int64_t *offsets, const void *tracked, const p2s_single_params *params,
                              int32_t *comb, double *err, double *Q);

/* ---- downstream of the .trc: filtering and quality metrics -----------------------------------
 * Zero-phase Butterworth filter of every column of a row-major [n_frames][n_cols] float64 matrix: replaces
 * Q_coords.apply(butterworth_filter_1d) in filter_all (filtering.py:437-471, 804): per column, every run of valid
 * samples (not NaN, not 0) longer than padlen = 3 * n_coef goes through scipy.signal.filtfilt(b, a, run) (odd
 * padding, steady-state initial conditions); other samples are copied.  b, a [n_coef] from
 * scipy.signal.butter(order / 2, cutoff / (frame_rate / 2)) with a[0] = 1, zi [n_coef - 1] from
 * scipy.signal.lfilter_zi(b, a); 2 <= n_coef <= 9.  All pointers are HOST pointers; the call blocks. */
int p2s_butterworth_host(p2s_ctx *ctx, int64_t n_frames, int32_t n_cols, const double *data, int32_t n_coef,
                         const double *b, const double *a, const double *zi, double *out);

/* The other column filters of the reference's filtering stage, every column of a row-major [n_frames][n_cols] float64
 * matrix at once (replaces Q_coords.apply(hampel_filter) and Q_coords.apply(filter1d), filtering.py:794-798):
 *   P2S_FILTER_HAMPEL    hampel_filter filtering.py:63-85, 7-sample window; params = {n_sigma}
 *   P2S_FILTER_GAUSSIAN  gaussian_filter_1d :513-529 = scipy.ndimage.gaussian_filter1d(col, sigma), mode 'reflect';
 *                        params = the 2 radius + 1 kernel weights (scipy.ndimage._filters._gaussian_kernel1d)
 *   P2S_FILTER_MEDIAN    median_filter_1d :561-577 = scipy.signal.medfilt(col, kernel_size), zero padding;
 *                        params = {kernel_size} (odd); NaN samples are refused (scipy's result for them depends on its
 *                        selection algorithm)
 *   P2S_FILTER_ONE_EURO  one_euro_filter_1d :87-160, forward and backward pass over every run of >= 2 samples that are
 *                        not NaN; params = {1 / frame_rate, min_cutoff, beta, d_cutoff}
 *   P2S_FILTER_KALMAN    kalman_filter_1d :316-434: constant-acceleration Kalman filter (predict, Joseph-form update per
 *                        sample) and, with smooth != 0, the Rauch-Tung-Striebel smoother over every run of >= 4 samples
 *                        that are neither NaN nor 0; params = {1 / frame_rate, measurement_noise, process_noise, smooth}.
 *                        The initial state of a run is {z0, z1 - z0, z2 - 2 z1 + z0}: the reference's differences are not
 *                        divided by the frame period (:342-351).  The caller decides what smooth means (the reference:
 *                        only int(smooth) == 1).  The reference takes both passes from filterpy (not importable where
 *                        this was built); restated from filterpy's published algorithm and checked against goldens
 *                        recorded through the reference's set-up code and against an exact multiprecision solve
 * All pointers are HOST pointers; the call blocks. */
#define P2S_FILTER_HAMPEL 1
#define P2S_FILTER_GAUSSIAN 2
#define P2S_FILTER_MEDIAN 3
#define P2S_FILTER_ONE_EURO 4
#define P2S_FILTER_KALMAN 5
int p2s_filter_columns_host(p2s_ctx *ctx, int32_t kind, int64_t n_frames, int32_t n_cols, const double *data,
                            const double *params, int32_t n_params, double *out);
/* gcv_spline_filter_1d (filtering.py:163-313) on every column of a row-major [n_frames][n_cols] float64 matrix: every run
 * of >= 5 valid samples (not NaN, not 0) is replaced by the natural cubic smoothing spline through it, evaluated at its
 * samples (scipy.interpolate.make_smoothing_spline(arange(n), run, lam=...)); other samples are copied.
 *   auto_mode != 0  cut_off_frequency 'auto': the run is normalised, 1 + (run - median) / (1.4826 MAD) (MAD 0 -> 1),
 *                   lambda minimises the GCV criterion on (0, n) (minimize_scalar 'bounded', xatol 1e-5, 500
 *                   evaluations at most), the fit uses lambda * smoothing_factor and is denormalised; `lam` is ignored
 *   auto_mode == 0  the fit uses lam * smoothing_factor on the raw run (the caller passes
 *                   lam = (frame_rate / (2 pi cutoff))^4)
 * lam_out [n_frames][n_cols] (may be NULL): the lambda of the final fit at the first sample of every filtered run, NaN
 * elsewhere.  A run of 2 to 4 samples is refused as the reference refuses it (P2S_ERR_GCV_SHORT_RUN, checked before any
 * launch); the first run (column by column) whose search or solve fails decides the status, and p2s_last_error() then
 * holds the reference's message.  On any error `out` holds the input.  HOST pointers; blocks. */
#define P2S_ERR_GCV_SHORT_RUN (-6)     /* "``x`` and ``y`` length must be at least 5"                              */
#define P2S_ERR_GCV_ILL_POSED (-7)     /* the banded Cholesky factorisation failed: "Seems like the problem is ill-posed" */
#define P2S_ERR_GCV_NO_MINIMUM (-8)    /* the search hit 500 evaluations or a NaN: "Unable to find minimum of ..."  */
#define P2S_ERR_GCV_SINGULAR (-9)      /* a zero pivot in the banded LU solve: "singular matrix"                    */
int p2s_gcv_spline_host(p2s_ctx *ctx, int64_t n_frames, int32_t n_cols, const double *data, int32_t auto_mode,
                        double lam, double smoothing_factor, double *out, double *lam_out);
/* loess_filter_1d (filtering.py:532-558) on every column of a row-major [n_frames][n_cols] float64 matrix: every run of at
 * least min_run consecutive samples that are not NaN (zeros are data) is replaced by its local linear regression,
 * statsmodels' lowess(run, frame_indices, frac = k / len, it = 0, delta = 0): at sample i the weighted least-squares line
 * through the k run samples nearest to i -- the block [l, l + k) of the run with l = i - k / 2 clamped to the run --
 * evaluated at i, with the tricube weights (1 - (|j - i| / h)^3)^3, h = max(i - l, l + k - 1 - i).  A sample at distance h
 * weighs exactly 0, so the result does not depend on which of two equally distant neighbours is kept; a fit with one
 * non-zero weight (k = 2) returns the sample.  Other samples are copied.  The caller derives k and min_run from the
 * reference's nb_values_used: k = int(nb + 1e-10), min_run = floor(nb) + 1.  statsmodels is not importable where this
 * was built and has never run here: restated from its published algorithm, checked against goldens recorded through
 * the reference's own loess_filter_1d with a stand-in for lowess and against a multiprecision solve of the definition.
 * Refused with P2S_ERR_INVALID_ARG: k outside 2..8191, min_run <= k, and any infinity in the data (what statsmodels
 * answers for one has not been recorded); all of it is checked before anything is copied or launched, and on such a
 * refusal `out` is untouched.  An empty shape is P2S_OK.  HOST pointers; blocks. */
int p2s_loess_host(p2s_ctx *ctx, int64_t n_frames, int32_t n_cols, const double *data, int32_t k, int64_t min_run,
                   double *out);
/* trc_evaluate's per-frame quantities and sums (Utilities/trc_evaluate.py:114-238) for xyz [n_frames][n_markers][3]:
 *   bones      [n_bones][2] int32  (parent, child) marker indices
 *   bone_len   [n_bones][n_frames]      |child - parent|, 0 -> NaN             (compute_bone_lengths :135-139)
 *   bone_stats [n_bones][3]             nanmean, nanstd (population), n_valid   (:141-150)
 *   accel      [n_markers][n_frames-2]  |p[f+2] - 2 p[f+1] + p[f]|              (compute_smoothness :185-186)
 *   missing    [n_markers] int64        frames with a NaN coordinate            (compute_missing_data :226-227)
 * Medians / percentiles of accel stay with the caller (np.median, np.percentile).  HOST pointers; blocks. */
int p2s_trc_metrics_host(p2s_ctx *ctx, int64_t n_frames, int32_t n_markers, const double *xyz, int32_t n_bones,
                         const int32_t *bones, double *bone_len, double *bone_stats, double *accel, int64_t *missing);

/* ---- a .trc back onto the image planes (Utilities/reproj_from_trc_calib.py:446-475) ------------------------------------
 * One projection per (frame, marker, camera), float64 throughout: replaces the frame x keypoint x camera loop around
 * reprojection() (:183-201) / cv2.projectPoints (:455), the rounding to one decimal (:461-462) and the out-of-image mask
 * (:469-475).
 *   Q      [n_frames][n_markers][3]  the markers in the Z-up frame (X, Y, Z): a .trc row holds (Y, Z, X) per marker and
 *                                    the caller undoes that order; NaN = missing
 *   flags  0: pinhole.  P [n_cams][n_frames_p][12] with n_frames_p = 1 (static cameras) or n_frames (one matrix per
 *             frame: moving and / or zooming cameras); x = P0.q / P2.q, y = P1.q / P2.q, q = (X, Y, Z, 1).  Kmat, dist,
 *             Rmat and T are not read.
 *          P2S_REPROJ_DISTORTED: cv2.projectPoints with Kmat [n_cams][9], dist [n_cams][5] (k1, k2, p1, p2, k3), Rmat
 *             [n_cams][9], T [n_cams][3]: z == 0 -> 1, the skew term ignored; the same device code as the triangulation
 *             kernels' reprojection.  Static cameras only (n_frames_p = 1); P is not read.
 *   sizes  [n_cams][2] image width, height
 * outputs, [n_cams][n_frames][n_markers][2] (x, y) each:
 *   uv_raw the pixels as computed (may be NULL)
 *   uv     what the reference stores: np.round(v, decimals=1) = rint(10 v) / 10 with ties to even, then x and y both NaN
 *          unless 0 <= x < width and 0 <= y < height on the ROUNDED values; a NaN or infinite projection comes out NaN.
 * All of Q and of the outputs is device-resident during the call: n_frames x n_markers x n_cams x 32 bytes (16 without
 * uv_raw) must fit, or the call fails with P2S_ERR_OOM.  HOST pointers; blocks. */
#define P2S_REPROJ_DISTORTED 1
int p2s_reproject_host(p2s_ctx *ctx, int64_t n_frames, int32_t n_markers, const double *Q, int32_t n_cams, int64_t n_frames_p,
                       const double *P, const double *Kmat, const double *dist, const double *Rmat, const double *T,
                       const double *sizes, int32_t flags, double *uv_raw, double *uv);
/* Milliseconds the kernel of this context's last p2s_reproject_host took (HIP events around it; 0 for an empty call). */
int p2s_reproject_kernel_ms(p2s_ctx *ctx, float *elapsed_ms);
/* dataset_to_openpose (Utilities/reproj_from_trc_calib.py:245-286) for every camera and frame at once, on at most 16 host
 * threads (no GPU involved): file `<dir c>/<name_root>_cam<c+1, 2 digits>_openpose_<f, 4 digits>.json` holds json.dumps of
 * the reference's dictionary -- version 1.3, one person with "person_id": [-1], in "pose_keypoints_2d" per output position
 * k the triplet x, y, 1 of marker marker_index[k] (floats as Python's repr) or 0.0, 0.0, 0 when either is NaN, then the
 * seven empty lists.  uv [n_cams][n_frames][n_markers][2] as p2s_reproject_host returns it; marker_index [n_out];
 * directory names back to back as in p2s_json_parse, and they must exist.  n_written (may be NULL): files completed.  On
 * a failure the other files are still written and the first failing path (in camera, frame order) is reported. */
int p2s_write_openpose_files(const char *dir_paths, const int64_t *dir_offsets, const char *name_root, int32_t n_cams,
                             int64_t n_frames, int32_t n_markers, int32_t n_out, const int32_t *marker_index,
                             const double *uv, int32_t n_threads, int64_t *n_written);

/* ---- exact order statistics of columns ---------------------------------------------------------------------------------
 * For each of n_cols contiguous float64 columns of n_rows entries (data is column-major: column c starts at
 * data + c * n_rows), NaN entries skipped: counts[c] = the number m of non-NaN entries, out[c][j] = the entry at 0-based
 * position ranks[j] of the sorted non-NaN entries; a negative rank counts from the top (-1 = the largest); a rank outside
 * [0, m) gives NaN, so an all-NaN column gives NaN throughout.  Exact: a radix select on the bit patterns, no
 * arithmetic.  -0.0 orders before +0.0.  np.nanmedian is np.mean of out at (m - 1) / 2 and at m / 2 (of one entry when m is odd).  n_rows < 2^31;
 * counts may be NULL.  HOST pointers; blocks. */
int p2s_column_order_stats_host(p2s_ctx *ctx, int64_t n_rows, int32_t n_cols, const double *data, int32_t n_ranks,
                                const int64_t *ranks, double *out, int64_t *counts);

/* ---- 2D keypoint jitter (Utilities/keypoint_jitter_analyze.py:143-325) --------------------------------------------------
 * compute_displacements, compute_bb_areas, detect_jitter, np.argwhere and classify_pattern for every camera at once,
 * float64 throughout and bit for bit the reference's numbers.  series: the cameras' [n_frames[c]][26][3] (x, y,
 * confidence) tables back to back; n_frames[c] >= 1 and < 2^31.  With rows[c] = n_frames[c] - 1, every output holds the
 * cameras back to back and any of them may be NULL:
 *   displacements  per camera [26][rows[c]] -- COLUMN-major, one keypoint's series contiguous: sqrt(dx*dx + dy*dy)
 *                  between consecutive frames, NaN unless both confidences are > 0.1
 *   areas          per camera [n_frames[c]]: (xmax - xmin) * (ymax - ymin) over the keypoints with confidence > 0.1 when
 *                  there are at least 2 (a NaN coordinate among them gives NaN), otherwise NaN
 *   medians, thresholds [n_cams][26]: np.nanmedian of every displacement column; median * multiplier, 10 where the
 *                  median is 0;  median_area [n_cams]: np.nanmedian of the areas
 *   mask           per camera [rows[c]][26] bytes: displacement > threshold
 *   counts         [n_cams][26]: events per keypoint
 *   events         [event_capacity][4] int32 (camera, frame = row + 1, keypoint, pattern): the set cells of the mask in
 *                  camera, row, keypoint order (np.argwhere per camera).  pattern at frame row + 1, the first that holds:
 *                  0 'A' at least 2 valid keypoints and xmin < 10, ymin < 10, xmax > width - 10 or ymax > height - 10;
 *                  1 'C' area and median area not NaN and area < 0.5 * median area; 2 'D' confidence < 0.3; 3 'E'.
 *   n_events       the number of events, whatever the capacity: when it exceeds event_capacity only the first
 *                  event_capacity were written and the caller asks again with room for all.
 * HOST pointers; blocks. */
int p2s_jitter_host(p2s_ctx *ctx, int32_t n_cams, const int64_t *n_frames, const double *series, double multiplier,
                    double image_width, double image_height, double *displacements, double *areas, double *medians,
                    double *thresholds, double *median_area, uint8_t *mask, int32_t *counts, int64_t event_capacity,
                    int32_t *events, int64_t *n_events);
/* Milliseconds the kernels of this context's last p2s_jitter_host took (HIP events around them). */
int p2s_jitter_kernel_ms(p2s_ctx *ctx, float *elapsed_ms);

/* ---- np.mean and np.std of columns ------------------------------------------------------------------------------------
 * For each of n_cols contiguous float64 columns of n_rows entries (column-major, as p2s_column_order_stats_host takes
 * them), NaN entries skipped: counts[c] = the number m of non-NaN entries, mean[c] = np.mean and std[c] = np.std (ddof 0)
 * of those entries in row order, bit for bit: the sum is np.add.reduce's -- chunks of 8192 entries added left to right,
 * each summed pairwise over blocks of at most 128 with eight accumulators -- the deviations are squared after one
 * rounded subtraction, and the root is correctly rounded.  NaN for a column without entries.  n_rows < 2^31; any output
 * may be NULL.  HOST pointers; blocks. */
int p2s_column_mean_std_host(p2s_ctx *ctx, int64_t n_rows, int32_t n_cols, const double *data, double *mean, double *std,
                             int64_t *counts);

/* ---- 2D confidence statistics (Utilities/pose_confidence_analyze.py:118-219) ----------------------------------------------
 * compute_statistics, compute_band_distribution and simulate_threshold for every camera at once, float64 and bit for bit
 * the reference's numbers.  tables: the cameras' [n_frames[c]][n_kpts] confidences back to back, NaN = no person in the
 * frame; 1 <= n_frames[c] < 2^31, 1 <= n_kpts <= 64, n_thresholds <= 8.  Per (camera, keypoint), over the non-NaN entries
 * in frame order (any output may be NULL):
 *   stats   [n_cams][n_kpts][9]  np.mean, np.median, np.std, min, max, np.percentile at 5, 25, 75 and 95; NaN without entries
 *   counts  [n_cams][n_kpts]     the number of entries
 *   below   [n_thresholds][n_cams][n_kpts]  entries < thresholds[t]
 *   bands   [n_cams][n_kpts][5]  entries in [0, 0.4), [0.4, 0.6), [0.6, 0.8), [0.8, 1.0] (closed) and [1.0, inf): 1.0 counts
 *                                twice, a negative entry and +inf in none
 * The rates the reference reports are these counts divided by `counts`.  HOST pointers; blocks. */
int p2s_confidence_stats_host(p2s_ctx *ctx, int32_t n_cams, const int64_t *n_frames, int32_t n_kpts, const double *tables,
                              int32_t n_thresholds, const double *thresholds, double *stats, int64_t *counts, int64_t *below,
                              int64_t *bands);
/* Milliseconds the kernels of this context's last p2s_confidence_stats_host took (HIP events around them). */
int p2s_confidence_kernel_ms(p2s_ctx *ctx, float *elapsed_ms);

/* ---- linear_sum_assignment (scipy.optimize, 1.15.3) --------------------------------------------------------------------
 * n cost matrices [n_rows][n_cols] row-major back to back, 1 <= n_rows, n_cols <= 32.  Per matrix: status = 0 and the
 * min(n_rows, n_cols) assigned (row, column) pairs in ascending row order, exactly scipy's (row_ind, col_ind), ties
 * included (csrc/p2s_lsap.h lists the decisions that make it so); status = 1 for a matrix holding NaN or -inf (scipy:
 * 'matrix contains invalid numeric entries'), 2 for one without a finite assignment ('cost matrix is infeasible'), the
 * pairs then -1.  row_ind, col_ind [n][min(n_rows, n_cols)], status [n].  With a context the matrices are solved on the
 * GPU, one a wave; ctx == NULL solves them on the host with the same code (the restatement can be checked without a GPU).
 * HOST pointers; blocks. */
int p2s_lsap_host(p2s_ctx *ctx, int64_t n, int32_t n_rows, int32_t n_cols, const double *cost, int32_t *row_ind, int32_t *col_ind,
                  int32_t *status);

/* ---- frame-to-frame person matching (Utilities/id_switch_analyze.py:47-145, 148-291, 364-388) -----------------------------
 * For every camera at once, float64 and bit for bit the reference's numbers.  Camera c has n_frames[c] >= 0 frames (the
 * readable files, in order); the frames of all cameras stand back to back.  persons [N][26][3] (x, y, confidence): every
 * listed person of every frame in that order; person_off [frames + 1]: the first person of every frame, person_off[0] = 0.
 * A person is kept when some confidence is above 0 (parse_frame_people).  Per frame f, camera-local indices:
 *   tables [7][frames] int32
 *     0 count       kept persons
 *     1 prev        the last earlier frame of the camera with a kept person, -1 without one (prev_people)
 *     2 zero_run    the frames between the two, f - 1 - prev (zero_count on reaching f)
 *     3 n_matched   pairs of linear_sum_assignment over the mean-keypoint-distance matrix (compute_match_cost: keypoints
 *                   with both confidences above 0.1, fewer than 3 of them cost 1e9) whose cost is below 1e9; 0 for a
 *                   frame without kept persons or without a previous frame
 *     4 n_lost      kept persons of the previous frame left unmatched
 *     5 n_appeared  kept persons of this frame left unmatched
 *     6 flag        0; 1 / 2 = the cost matrix is refused as by p2s_lsap_host (a NaN coordinate on a shared keypoint);
 *                   4 = more than 32 kept persons in the frame or its previous one: not matched
 *   kept [N] int32         from person_off[f]: the frame's `count` kept persons in list order, as indices into the frame's
 *                          own list; the rest of the frame's run is unspecified
 *   distances     the matched costs, per camera in frame order and within a frame in previous-person order, the cameras
 *                 back to back; room for N values covers every case
 *   n_distances [n_cams]   how many of them each camera has
 *   stats [n_cams][6]      np.mean, np.median, np.percentile 95 and 99, min and max of the camera's distances; NaN without
 * Any output may be NULL.  HOST pointers; blocks. */
int p2s_id_switch_host(p2s_ctx *ctx, int32_t n_cams, const int64_t *n_frames, const int64_t *person_off, const double *persons,
                       int32_t *tables, int32_t *kept, double *distances, int64_t *n_distances, double *stats);
/* Milliseconds the kernels of this context's last p2s_id_switch_host took (HIP events around them). */
int p2s_id_switch_kernel_ms(p2s_ctx *ctx, float *elapsed_ms);

/* ---- primary-person selection (Utilities/pose_extract_person.py:37-87, the rule of p2s_json_select_tracked_person) ---------
 * For every camera at once, as a prefix scan instead of a loop over the frames.  The layout is p2s_id_switch_host's: camera c
 * has n_frames[c] >= 0 frames, the frames of all cameras stand back to back; persons [N][n_kpts][3] (x, y, confidence) holds
 * the persons whose list has exactly 3 * n_kpts numbers, in list order (no other can be a candidate; a longer list ends the
 * reference's run and is the caller's to deal with); person_off [frames + 1], person_off[0] = 0; 1 <= n_kpts <= 127.
 * A person is a candidate when some keypoint has confidence > conf_threshold and a non-NaN x.  A frame with candidates
 * selects one: the only one; else, after an earlier selection, the one with the strictly smallest mean distance to it over
 * the keypoints valid in both (sqrt(dx*dx + dy*dy) without contraction, summed in np.mean's order, the first on ties; NaN,
 * inf and no shared keypoint are not eligible); else the first candidate with the most confidences > conf_threshold.
 * Per frame, camera-local indices, each output may be NULL:
 *   chosen        the selected person as an index into the frame's run of `persons`, -1 for a frame without candidates
 *   n_candidates  candidates of the frame
 *   prev          the last earlier frame of the camera with a candidate, -1 without one
 * More than 32 candidates in one frame: P2S_ERR_INVALID_ARG naming the camera and the frame, nothing computed.
 * HOST pointers; blocks. */
int p2s_track_select_host(p2s_ctx *ctx, int32_t n_cams, const int64_t *n_frames, const int64_t *person_off, const double *persons,
                          int32_t n_kpts, double conf_threshold, int32_t *chosen, int32_t *n_candidates, int32_t *prev);
/* Milliseconds the kernels of this context's last p2s_track_select_host took (HIP events around them). */
int p2s_track_select_kernel_ms(p2s_ctx *ctx, float *elapsed_ms);

/* ---- person tracking across frames (triangulation.py:823-874, sort_people_sports2d of common.py:1037-1136) ----------------
 * Which detection every person slot of multi-person triangulation takes, frame after frame, for a batch of trials in one
 * launch (one workgroup a trial, the loop over its frames inside it).  float64 and bit for bit the reference's numbers.
 * The trials share n_persons (P, 1 .. 32) and n_kpts (K >= 1) and stand back to back: Q [N][P][K][3] (NaN = not
 * triangulated), frame_off [n_trials + 1] with frame_off[0] = 0, first_frame [n_trials] the absolute number of every
 * trial's first frame.  A trial keeps a state S [32][K][3], the last non-NaN value of every coordinate of every slot, n of
 * its rows live; it starts as P rows of NaN, or as the first n_state_in[t] rows (0 .. 32) of state_in [n_trials][32][K][3]
 * -- the state_out and n_state_out of an earlier call, which continues a trial in chunks.  Per frame: the n x P matrix of
 * mean keypoint distances (np.sqrt(np.nansum(diff**2)) per keypoint, np.nanmean over them in NumPy's summation order, NaN
 * and +inf as 1e10), p2s_lsap_host's assignment on it, with has_max_dist the pairs above max_dist dropped, the detections
 * left over as new slots n, n + 1, ... in ascending order, and S takes the placed detections' non-NaN values.  The
 * absolute frame 0 (and a state without rows) is not matched: detection p goes to slot p.  Outputs, each may be NULL
 * but status:
 *   ids [N][P] int32          the detection the first P slots took, -1 for none
 *   Q_rows [N][P][K][3]       the points in tracked order, NaN for a slot without a detection
 *   matched_dist [N][P]       the distance of the kept pair of every slot; NaN without one and in a frame not matched
 *   n_slots [N] int32         slots after the frame
 *   state_out [n_trials][32][K][3], n_state_out [n_trials] int32    the state after the trial's last frame
 *   status [n_trials][2] int32   0, 0; or the first frame (trial-local, plus 1) that would have passed 32 slots, and in
 *                             the second word what p2s_lsap_host's status says when that frame's matrix was refused
 *                             instead (-1: a slot count outside 0 .. 32 read on the device); nothing from that frame on
 *                             is defined for the trial
 * The workgroup's LDS -- S, one frame, the cost matrix and at least one pair's K distances, (96 + 3 P + 1) K + 1 024
 * doubles and 2 KB of the solver's and the placement's arrays -- must fit what the device gives a workgroup (queried), and K <= 240 there:
 * P2S_ERR_INVALID_ARG otherwise, as for P outside 1 .. 32, nothing written.
 * p2s_track_persons_host: HOST pointers; blocks.  ctx == NULL runs the same code on the host (no LDS limit): the
 * restatement can be checked without a GPU.
 * p2s_track_persons_device: Q, the states and every output are DEVICE pointers, frame_off and first_frame stay HOST
 * arrays (the shape, copied before the call returns); enqueues on the context's stream and reads nothing back -- the call
 * to chain after p2s_triangulate_device. */
int p2s_track_persons_host(p2s_ctx *ctx, int64_t n_trials, const int64_t *frame_off, const int64_t *first_frame, int32_t n_persons,
                           int32_t n_kpts, const double *Q, int32_t has_max_dist, double max_dist, const double *state_in,
                           const int32_t *n_state_in, int32_t *ids, double *Q_rows, double *matched_dist, int32_t *n_slots,
                           double *state_out, int32_t *n_state_out, int32_t *status);
int p2s_track_persons_device(p2s_ctx *ctx, int64_t n_trials, const int64_t *frame_off, const int64_t *first_frame, int32_t n_persons,
                             int32_t n_kpts, const double *d_Q, int32_t has_max_dist, double max_dist, const double *d_state_in,
                             const int32_t *d_n_state_in, int32_t *d_ids, double *d_Q_rows, double *d_matched_dist, int32_t *d_n_slots,
                             double *d_state_out, int32_t *d_n_state_out, int32_t *d_status);
/* Milliseconds the kernel of this context's last p2s_track_persons_host took (HIP events around it). */
int p2s_track_persons_kernel_ms(p2s_ctx *ctx, float *elapsed_ms);

/* ---- find_peaks (scipy.signal, 1.15.3) -----------------------------------------------------------------------------------
 * scipy.signal.find_peaks(x, prominence=p) for each of n_cols contiguous float64 columns of n_rows entries (column-major,
 * as p2s_column_order_stats_host takes them), bit for bit: _local_maxima_1d (a plateau's peak is (left_edge + right_edge)
 * / 2, the first and last samples are never peaks, a comparison with NaN is false) and _peak_prominences with wlen=None
 * (from the peak outwards while the samples are <= the peak -- a larger sample or a NaN ends the scan -- the smallest
 * sample met and the position nearest to the peak that holds it; prominence = x[peak] - max(left_min, right_min), one
 * subtraction).  prominence [n_cols]: a peak of column c is kept when prominence[c] <= its prominence, false for a NaN on
 * either side, so +inf keeps none but a peak of infinite prominence; NULL keeps every local maximum (its prominence is still computed).
 *   peaks, prominences, left_bases, right_bases [capacity]: the kept peaks of column 0 in ascending row order, then
 *                  column 1's, ...; rows as indices into the column
 *   col_counts [n_cols]  kept peaks per column
 *   n_peaks        their total, whatever the capacity: when it exceeds capacity only the first capacity were written and
 *                  the caller asks again with room for all.  capacity 0 only counts.
 * 1 <= n_rows < 2^31, n_cols >= 1, n_rows * n_cols <= 2^36.  HOST pointers; blocks. */
int p2s_find_peaks_host(p2s_ctx *ctx, int64_t n_rows, int32_t n_cols, const double *data, const double *prominence,
                        int64_t capacity, int64_t *peaks, double *prominences, int64_t *left_bases,
                        int64_t *right_bases, int32_t *col_counts, int64_t *n_peaks);

/* ---- gait contact signals (Utilities/trc_gaitevents.py:387-576) ------------------------------------------------------------
 * What gait_events_height_coords (method 0) and gait_events_fwd_vel (method 1) do to a toe column, for a batch of
 * columns of unequal length at once.  data [max_rows][n_cols] row-major: column c holds col_len[c] samples (1 <=
 * col_len[c] <= max_rows < 2^31), what follows them is never read.  With s = factor[c] * column:
 *   method 0  signal = scipy.signal.filtfilt(b, a, s[1:]) over the whole column (odd extension by padlen = 3 n_coef,
 *             lfilter_zi start): zeros are data, a NaN makes the column NaN.  b, a [n_coef] (a[0] = 1, 2 <= n_coef <= 9),
 *             zi [n_coef - 1].  A column with col_len[c] - 1 <= padlen is refused with scipy's message.
 *   method 1  v = diff(s) / dt[c]; v where it has the sign `sign` (1 or -1), else 0 (also for a NaN); abs; [1:];
 *             signal = scipy.ndimage.correlate1d(., weights, mode='reflect') with the n_weights = 2 radius + 1 weights of
 *             gaussian_filter1d.
 * signal [max_rows - 1][n_cols] row-major: col_len[c] - 1 samples per column, within 1e-9 relative of scipy's.  Then
 * low = signal < threshold[c] and start_end_true_seq (:116-133):
 *   on  [n_cols][event_capacity]  the samples i >= 1 with low[i] and not low[i - 1], ascending (index 0 is taken off,
 *                                 as the callers of start_end_true_seq do)
 *   off [n_cols][event_capacity]  i - 1 for the samples i >= 1 with low[i - 1] and not low[i] (the reference's -1 is dropped)
 *   n_on, n_off [n_cols]          how many there are, whatever the capacity: when one exceeds event_capacity only the
 *                                 first event_capacity of that column were written and the caller asks again with room
 *   first_low [n_cols]            low[0]: with n_off = 0 it tells an all-true signal, on which start_end_true_seq raises
 * signal, on and off may be NULL (on and off only with event_capacity 0).  HOST pointers; blocks. */
int p2s_gait_contacts_host(p2s_ctx *ctx, int32_t method, int32_t n_cols, int64_t max_rows, const int64_t *col_len,
                           const double *data, const double *dt, const double *threshold, const double *factor,
                           int32_t sign, int32_t n_coef, const double *b, const double *a, const double *zi,
                           int32_t n_weights, const double *weights, double *signal, int64_t event_capacity, int32_t *on,
                           int32_t *off, int32_t *n_on, int32_t *n_off, uint8_t *first_low);
/* Milliseconds the kernels of this context's last p2s_find_peaks_host or p2s_gait_contacts_host took (HIP events around
 * them). */
int p2s_gait_kernel_ms(p2s_ctx *ctx, float *elapsed_ms);

/* ---- body measurements from .trc tables (common.py:378-455, :715-1034; kinematics.py:278-304) ------------------------
 * The stable order of n_segments columns of float64 keys, data back to back, seg_len[s] entries each (1 .. 2^31 - 1):
 * order [sum seg_len] = np.argsort(column, kind='stable') per column -- -inf < ... < -0.0 = +0.0 < ... < inf < NaN, equal
 * keys in input order. */
int p2s_stable_argsort_host(p2s_ctx *ctx, int64_t n_segments, const int64_t *seg_len, const double *data, int32_t *order);
/* trimmed_mean (common.py:427-455) of every column, bit for bit: np.mean(np.sort(x)[int(n * half_trim) :
 * int(n * (1 - half_trim))]), np.mean(x) when that slice is empty; half_trim = trimmed_extrema_percent / 2 in [0, 0.5]. */
int p2s_trimmed_means_host(p2s_ctx *ctx, int64_t n_segments, const int64_t *seg_len, const double *data, double half_trim,
                           double *means);
/* best_coords_for_measurements, mean_angles, compute_height, compute_leg_length and the trimmed segment lengths of
 * dict_segment_ratio for n_files tables of unequal length in one call; no count comes back to the host between the steps.
 * data: the tables back to back, [n_rows[f]][3 n_markers[f]].  Per file:
 *   flags     P2S_MEASURE_SPEED     keep the frames whose summed speed is above speed_threshold[f], int(count *
 *                                   keep_fraction) of them by ascending speed (every frame in file order when none is above)
 *             P2S_MEASURE_ANGLES    mean_angles of the selected rows
 *             P2S_MEASURE_RESTRICT  keep the rows with angle < angle_limit; fewer than 50: the first 50 rows by angle, NaN last
 *             P2S_MEASURE_HEIGHT    row heights from pairs 0 .. 8; P2S_MEASURE_FEET_CONST: both feet are 0.10
 *             P2S_MEASURE_LEG       row leg lengths from pairs 2 .. 5
 *   roles     [10] marker indices of RShoulder LShoulder RHip LHip Hip Neck RKnee LKnee RAnkle LAnkle, -1 = not in the
 *             file (Hip: the mid-hip, Neck: the mid-shoulder stand in)
 *   pairs     [n_pairs][2] marker indices; n_markers[f] is the mid-shoulder, n_markers[f] + 1 the mid-hip, a pair with
 *             a -1 is skipped (its lengths are 0).  Pairs 0 .. 8 of compute_height: heel-ankle R, L; ankle-knee R, L;
 *             knee-hip R, L; hip-shoulder R, L; mid-shoulder to Head or Nose, times head_factor[f]
 *   n_speed_markers  (may be NULL: every marker) the summed speed runs over the file's first n_speed_markers[f] markers
 * When no row is left every frame of the file is kept.  At most 2^21 files (or segments, in the two calls above) and 2^33
 * rows a call.  angles of a file without P2S_MEASURE_ANGLES are NaN.  Outputs (those marked * may be NULL), rows of all files back to
 * back: sum_speeds* and angles* (the first n_selected[f] of a file), kept_pos and kept_frame (the first n_kept[f]: the
 * row's place among the selected rows, which is the reference's index label, and its frame), branch (P2S_MEASURE_ALL_SLOW,
 * _FEW_SMALL_ANGLES, _ALL_DATA), row_heights*, row_values* [n_pairs + 2][rows] (lengths per pair, heights, leg lengths),
 * means [n_files][n_pairs + 2]: their trimmed means with half_trim as above. */
#define P2S_MEASURE_SPEED 1
#define P2S_MEASURE_ANGLES 2
#define P2S_MEASURE_RESTRICT 4
#define P2S_MEASURE_FEET_CONST 8
#define P2S_MEASURE_HEIGHT 16
#define P2S_MEASURE_LEG 32
#define P2S_MEASURE_FLAGS 63
#define P2S_MEASURE_ALL_SLOW 1
#define P2S_MEASURE_FEW_SMALL_ANGLES 2
#define P2S_MEASURE_ALL_DATA 4
int p2s_body_measure_host(p2s_ctx *ctx, int32_t n_files, const int64_t *n_rows, const int32_t *n_markers, const double *data,
                          const int32_t *flags, const int32_t *roles, int32_t n_pairs, const int32_t *pairs,
                          const double *head_factor, const double *speed_threshold, const int32_t *n_speed_markers, double keep_fraction,
                          double angle_limit, double half_trim, double *sum_speeds, double *angles, int32_t *n_selected, int32_t *kept_pos,
                          int32_t *kept_frame, int32_t *n_kept, int32_t *branch, double *row_heights, double *row_values,
                          double *means);
/* Milliseconds the kernels of this context's last call of one of the three above took (HIP events around them). */
int p2s_measure_kernel_ms(p2s_ctx *ctx, float *elapsed_ms);

/* ---- synchronization (synchronize_cams_all, synchronization.py:1346-1612) ------------------------------------------
 * Speeds: replaces the per-camera pandas / scipy work of :1562-1584 (interpolate_zeros_nans :1565, bfill().ffill(),
 * signal.filtfilt :1568, vert_speed :1271-1288, abs().sum(axis=1) :1579, filtfilt of the sum :1585).  coords: the cameras'
 * [n_frames[c]][n_cols] row-major blocks back to back, the (x, y) columns of the keypoints to consider in model order with
 * the low-likelihood triplets already NaN (convert_json2pandas, drop_col, [kpt_id_in_df]).  Per column: linear
 * interpolation of NaN / 0 samples with extrapolation at the ends when more than 4 samples are good, bfill, ffill; then
 * per camera with more than 3 (n_coef - 1) frames filtfilt(b, a) over every column (odd extension, padlen 3 n_coef),
 * vertical speed = diff of the odd (y) columns, NaN -> 2x the second row's diff, sum of absolute values skipping NaN,
 * filtfilt of that sum under the same rule.  b, a [n_coef] (a[0] = 1), zi [n_coef - 1] = scipy.signal.lfilter_zi(b, a).
 * speeds: [sum n_frames] back to back.  Every camera needs >= 2 frames (the reference raises IndexError on 1); a camera
 * with 3 (n_coef - 1) < n_frames <= 3 n_coef frames is refused with P2S_ERR_SYNC_PADLEN and scipy's message.  HOST
 * pointers; blocks. */
#define P2S_ERR_SYNC_PADLEN (-10)
int p2s_sync_speeds_host(p2s_ctx *ctx, int32_t n_cams, const int64_t *n_frames, int32_t n_cols, const double *coords,
                         int32_t n_coef, const double *b, const double *a, const double *zi, double *speeds);
/* Lagged Pearson: replaces time_lagged_cross_corr (synchronization.py:1291-1343) for n_sig compared signals at once.
 * For signal s (sig_len[s] samples, back to back in sig) and lag l in [lag_lo, lag_hi):
 * r[s][l - lag_lo] = Series(ref).corr(Series(sig_s).shift(l)): the pairs (ref[i], sig_s[i - l]) with
 * i < min(n_ref, sig_len[s]), 0 <= i - l < sig_len[s], both values not NaN; np.corrcoef of them (two passes, clipped to
 * [-1, 1]); NaN with fewer than 2 pairs or a zero variance.  argmax[s] = np.argmax(r[s]) (the first maximum, or the
 * first NaN when there is one), max_corr[s] = np.nanmax(r[s]) (NaN when every r is NaN: the caller applies the
 * reference's offset 0 / correlation 0).  HOST pointers; blocks. */
int p2s_lagged_pearson_host(p2s_ctx *ctx, const double *ref, int64_t n_ref, int32_t n_sig, const double *sig,
                            const int64_t *sig_len, int64_t lag_lo, int64_t lag_hi, double *r, int64_t *argmax,
                            double *max_corr);

/* Counters of the triangulation calls of this context since creation (or the last reset), after synchronising its
 * streams; out holds 8 values: out[0] units that entered the camera-subset search (triangulation.py:408 beyond the
 * first pass), out[1] camera subsets evaluated, out[2] 64-lane evaluation passes, out[3] units whose search stopped at
 * the safety valve (a level with more than 2^26 subsets, i.e. C(32, 11) and beyond, is not entered: such a unit comes
 * back as not triangulated where the reference would have gone on for hours -- callers report the count), out[4]
 * per-camera reprojection errors computed for the candidates of the pruned passes (levels of hundreds of subsets and
 * more: hopeless candidates are dropped after a few cameras, so fewer than cameras x subsets), out[5] those candidates
 * (a part of out[1]), out[6] camera subsets looked at by the fp32 screen of the pooled kernel (only its survivors are
 * evaluated in fp64 and counted in out[1]), out[7] 64-lane screen passes. */
int p2s_get_tri_stats(p2s_ctx *ctx, uint64_t *out, int32_t reset);

/* Counters of the multi-person association calls of this context since creation (or the last reset), after
 * synchronising its stream: out[0] frames with at least one detection, out[1] ADMM passes of matchSVT
 * (personAssociation.py:477-505), out[2] Jacobi sweeps of their singular value decompositions, out[3] fp64 operations
 * by the kernels' own count (a multiplication or addition is 1, a fused multiply-add 2; rotations, products and
 * updates as the kernel that ran does them -- the figure bench.py divides by the fp64 vector peak). */
int p2s_get_assoc_stats(p2s_ctx *ctx, uint64_t *out, int32_t reset);

/* Experiments and tests only -- apart from P2S_TUNE_MAX_SUBSETS nothing here changes a result, and the library never
 * reads the environment.
 *   P2S_TUNE_TRI_PATH     P2S_TRI_PATH_AUTO (default): the pooled one-launch kernel (failures of five tiles pooled, fp32
 *                         screen + fp64 evaluation of the surviving camera subsets) where it applies (pinhole, no L/R swap,
 *                         float32 observations, up to 16 cameras), else round 2's one-launch kernel (float64 observations,
 *                         up to 8 cameras), else the streaming + work-list search pair;
 *                         P2S_TRI_PATH_POOLED: the same choice (named, for tests); P2S_TRI_PATH_TWO_TILES / _ONE_TILE: round
 *                         2's one-launch kernel with two tiles per wave where it pools / one tile everywhere;
 *                         P2S_TRI_PATH_WORKLIST: always the pair
 *   P2S_TUNE_SCREEN       0: the pooled kernel sends every camera subset to the fp64 evaluation (default 1: only those
 *                         its fp32 screen cannot rule out; same results bit for bit)
 *   P2S_TUNE_POOL_TILES   tiles of 64 units a wave of the pooled kernel streams before it searches their failures (2..6,
 *                         default 5; 9-16 cameras: always 2; up to 4 cameras: always 5)
 *   P2S_TUNE_POOL_SINGLES_PCT  share (%) of the tiles that the last workgroups of every XCD take one at a time instead
 *                         of several (default 8)
 *   P2S_TUNE_FORCE_TILED  1: the LDS-tiled streaming kernel even where observations fit in registers
 *   P2S_TUNE_NO_OVERLAP   1: search kernels on the main stream instead of beside the next chunk's streaming pass
 *   P2S_TUNE_SEARCH_JOB   work-list records a search wave takes at a time (8..64; 0 = automatic)
 *   P2S_TUNE_MAX_SUBSETS  the work-list search does not enter a level with more camera subsets than this (default
 *                         2^26; this one DOES change results -- tests of the valve only)
 *   P2S_TUNE_DEEP_MIN_SUBSETS  levels of the work-list search with more camera subsets than this (default 4 096) are
 *                         cut into chunks and spread over the whole GPU instead of being walked by one wave; 0 = never
 *   P2S_TUNE_DEEP_PRUNE   0: the long levels evaluate every camera of every candidate (default 1: exact pruning, same
 *                         results)
 *   P2S_TUNE_ASSOC_FORM   P2S_ASSOC_FORM_AUTO (default): up to 32 detections per frame take the symmetric one-wave kernel;
 *                         P2S_ASSOC_FORM_GENERAL: the general kernel (no symmetry assumed) at every size
 *   P2S_TUNE_GAPS_WORKSPACE_KB  cap (KiB, default P2S_GAPS_WORKSPACE_KB) of the spline kinds' workspace in
 *                         p2s_interpolate_gaps: the columns go through it in chunks that fit, one column at least
 *   P2S_TUNE_POISON_STAGING  -1 (default): off; 0..255: every buffer the context owns -- the staging slots of the *_host
 *                         calls and the work-list triangulation's list, counters and deep-level buffers -- is filled with
 *                         this byte over its whole capacity, on the context's stream, before the call that asked for it
 *                         uses it.  What a call finds in such a buffer is garbage by contract; this makes it the same
 *                         hostile garbage every time (0xFF: NaN, -1 and set flags) for tests/test_engine_reuse_gpu.py
 *   P2S_TUNE_DIAG_MODE    kernel diagnostics of a -DP2S_DIAG build (exp/README.md); refused by the shipped library */
#define P2S_TUNE_TRI_PATH 1
#define P2S_TUNE_FORCE_TILED 2
#define P2S_TUNE_NO_OVERLAP 3
#define P2S_TUNE_SEARCH_JOB 4
#define P2S_TUNE_DIAG_MODE 5
#define P2S_TUNE_MAX_SUBSETS 6
#define P2S_TUNE_DEEP_MIN_SUBSETS 7
#define P2S_TUNE_ASSOC_FORM 8
#define P2S_TUNE_POOL_SINGLES_PCT 9
#define P2S_TUNE_DEEP_PRUNE 10
#define P2S_TUNE_SCREEN 11
#define P2S_TUNE_POOL_TILES 12
#define P2S_TUNE_GAPS_WORKSPACE_KB 13
#define P2S_TUNE_POISON_STAGING 14
#define P2S_ASSOC_FORM_AUTO 0
#define P2S_ASSOC_FORM_GENERAL 1
#define P2S_TRI_PATH_AUTO 0
#define P2S_TRI_PATH_WORKLIST 1
#define P2S_TRI_PATH_ONE_TILE 2
#define P2S_TRI_PATH_POOLED 3
#define P2S_TRI_PATH_TWO_TILES 4
int p2s_set_tuning(p2s_ctx *ctx, int32_t key, int32_t value);

/* Kernel timing on the context's stream with HIP events: begin, enqueue work, end (blocks). */
int p2s_timing_begin(p2s_ctx *ctx);
int p2s_timing_end(p2s_ctx *ctx, float *elapsed_ms);

/* Tile geometry the triangulation kernel will use for (C, K, dtype): diagnostics for DESIGN.md /
 * bench.py (blocks per tile, threads per workgroup, LDS bytes). */
int p2s_tri_geometry(int32_t n_cams, int32_t n_kpts, int32_t dtype, int32_t *blocks_per_tile,
                     int32_t *threads, int32_t *lds_bytes);

/* ---- OpenPose-JSON ingest (host threads; no GPU involved) ------------------------------------------------
 * Replaces the reference's per-frame, per-person file parsing -- extract_files_frame_f
 * (triangulation.py:607-653: json.load of every camera file once PER PERSON), count_persons_in_json
 * (:77-90) and read_json (personAssociation.py:260-274) -- by one parse of every file into a batch and
 * gather calls that lay the numbers out for p2s_triangulate_* / p2s_associate_*.  A file counts as
 * unreadable exactly when Python's open(path, 'r') + json.load would raise (missing, not UTF-8, not JSON
 * in json.load's dialect: NaN / Infinity literals accepted, control characters in strings rejected,
 * trailing data rejected); repeated object keys take the last value. */
typedef struct p2s_json_batch p2s_json_batch;

#define P2S_JSON_UNREADABLE (-1)      /* people count of a file json.load would raise on (or an empty path) */
#define P2S_JSON_NO_PEOPLE_LIST (-2)  /* valid JSON without a top-level object holding a "people" array      */
#define P2S_JSON_PERSON_NO_LIST (-1)      /* person length: not an object / no "pose_keypoints_2d" array    */
#define P2S_JSON_PERSON_NOT_NUMERIC (-2)  /* person length: the array holds strings / arrays / objects      */

/* paths: the file names back to back (no separators needed), path_offsets [n_files+1] byte offsets into it;
 * an empty name = no file for that slot.  n_threads <= 0: one per hardware thread. */
int p2s_json_parse(const char *paths, const int64_t *path_offsets, int64_t n_files, int32_t n_threads,
                   p2s_json_batch **out);
int p2s_json_free(p2s_json_batch *batch);
/* counts [n_files]: len(js['people']) or a P2S_JSON_* code; person_base [n_files+1]: prefix sums of
 * max(count, 0) = row of each file's first person in p2s_json_person_lengths.  Either may be NULL. */
int p2s_json_people_counts(const p2s_json_batch *batch, int32_t *counts, int64_t *person_base);
/* lengths [person_base[n_files]]: len(person['pose_keypoints_2d']) or a P2S_JSON_PERSON_* code. */
int p2s_json_person_lengths(const p2s_json_batch *batch, int32_t *lengths);
/* The "person_id" value of every person (file-major, as p2s_json_person_lengths), as the raw JSON text of the value:
 * text_off [person_base[n_files] + 1] byte offsets into text, an empty text = the person has no such key (a repeated key
 * takes the last value).  text may be NULL: then only text_off is filled (text_off's last entry is the size to provide).
 * file_kind [n_files] (may be NULL): why a file has no person list, which the people counts do not tell apart --
 * what the reference's data.get('people', []) and the loop over it do with the document. */
#define P2S_JSON_DOC_UNREADABLE (-1)      /* P2S_JSON_UNREADABLE                                                    */
#define P2S_JSON_DOC_PEOPLE 0             /* an object whose "people" is a list                                     */
#define P2S_JSON_DOC_NO_PEOPLE_KEY 1      /* an object without "people": .get's default, no person                  */
#define P2S_JSON_DOC_PEOPLE_NULL 2        /* "people": null -- iterating None raises TypeError                      */
#define P2S_JSON_DOC_PEOPLE_OTHER 3       /* "people" is a number, a string, an object, true or false               */
#define P2S_JSON_DOC_LIST 4               /* the document is no object: .get raises AttributeError on a list, ...   */
#define P2S_JSON_DOC_STRING 5             /* ... a str,                                                             */
#define P2S_JSON_DOC_INT 6                /* ... an int,                                                            */
#define P2S_JSON_DOC_FLOAT 7              /* ... a float (NaN and the infinities included),                         */
#define P2S_JSON_DOC_BOOL 8               /* ... a bool,                                                            */
#define P2S_JSON_DOC_NULL 9               /* ... None                                                               */
int p2s_json_person_ids(const p2s_json_batch *batch, int64_t *text_off, char *text, int64_t text_capacity, int32_t *file_kind);
/* extract_files_frame_f for every file at once: for file i and person n < max_persons writes
 * out[file_offsets[i] + n*person_stride + 3*k + {0,1,2}] = values[3*keypoint_ids[k] + {0,1,2}], NaN when
 * the file, the person or the triplet does not exist (triangulation.py:629-644); file_offsets[i] < 0 skips
 * the file.  Offsets and strides are in elements of dtype.  n_inexact (may be NULL) counts the values a
 * P2S_F32 output could not hold exactly, so that the caller can ask again in P2S_F64. */
int p2s_json_gather_keypoints(const p2s_json_batch *batch, const int32_t *keypoint_ids, int32_t n_ids,
                              int32_t max_persons, const int64_t *file_offsets, int64_t person_stride,
                              int32_t dtype, void *out, int64_t *n_inexact);
/* read_json layout: row r = the first n_values numbers of person person_index[r] of file file_index[r]
 * (NaN-padded), out [n_rows][n_values]. */
int p2s_json_gather_people(const p2s_json_batch *batch, const int64_t *file_index, const int32_t *person_index,
                           int64_t n_rows, int32_t n_values, int32_t dtype, void *out, int64_t *n_inexact);

/* convert_json2pandas (synchronization.py:1185-1250, synchronization_gui false) for every file at once: in file i, the
 * person with the largest bounding-box area over the model's keypoints (keypoint_ids, (0, 0) points included; ties and
 * NaN as np.argmax: the first maximum, or the first NaN); then out[i][k] = (x, y, likelihood) of keypoint_ids[k] of that
 * person, (NaN, NaN, NaN) unless likelihood > threshold.  A file on which the reference's try block raises gets NaN
 * throughout: unreadable, no "people" list, no person, any person without a "pose_keypoints_2d" list of numbers (the
 * reference's comprehension indexes it before its `in` test, :1219-1224), any person's list too short for a model
 * keypoint's triplet.  JSON null reads as NaN.  out [n_files][n_ids][3] float64. */
int p2s_json_gather_largest_person(const p2s_json_batch *batch, const int32_t *keypoint_ids, int32_t n_ids,
                                   double likelihood_threshold, double *out);
/* shutil.copy for n_files (source, destination) pairs on host threads: the bytes, then the source's permission bits.
 * Paths as in p2s_json_parse.  ok [n_files] (may be NULL): 1 = copied, 0 = failed; the call then returns
 * P2S_ERR_INVALID_ARG with the first failure's path and errno text in p2s_last_error(). */
int p2s_copy_files(const char *src_paths, const int64_t *src_offsets, const char *dst_paths, const int64_t *dst_offsets,
                   int64_t n_files, int32_t n_threads, int8_t *ok);
/* load_keypoints_series / _select_person (Utilities/keypoint_jitter_analyze.py:50-140) over one camera's batch, the
 * files in the order given; sequential, since every choice depends on the one before.  out [n_files][n_kpts][3] float64:
 * the chosen person's first 3 * n_kpts numbers, NaN for a file without one.  A person is a candidate when its list has
 * at least 3 * n_kpts numbers and a keypoint with confidence > conf_threshold and a non-NaN x.  One candidate: taken.
 * Several, after an earlier choice: the one with the strictly smallest mean 2D distance to that choice over the
 * keypoints valid in both (the first on ties; no shared keypoint, or a NaN mean: not eligible) -- the mean is summed in
 * np.mean's order.  Otherwise the candidate with the most confidences > conf_threshold, the first on ties.
 * status [n_files], detail [n_files] (may be NULL):
 *   P2S_TRACK_SELECTED      detail = the person's index in "people"
 *   P2S_TRACK_NO_PEOPLE     an object without "people", or with an empty or null one
 *   P2S_TRACK_NO_CANDIDATE  persons, none of them a candidate
 *   P2S_TRACK_LONG_LIST     a person's list is longer than 3 * n_kpts (the reference's reshape raises); detail = its length
 *   P2S_TRACK_BAD_FILE      unreadable, or not JSON
 *   P2S_TRACK_BAD_CONTENT   the top level is not an object, "people" is neither a list nor null, a person is not an
 *                           object, or a list holds something that is not a number (null included)
 * The negative ones end the reference's run; the rows after them are still filled as if the file held no people. */
#define P2S_TRACK_SELECTED 1
#define P2S_TRACK_NO_PEOPLE 0
#define P2S_TRACK_NO_CANDIDATE 2
#define P2S_TRACK_LONG_LIST (-1)
#define P2S_TRACK_BAD_FILE (-2)
#define P2S_TRACK_BAD_CONTENT (-3)
int p2s_json_select_tracked_person(const p2s_json_batch *batch, int32_t n_kpts, double conf_threshold, double *out,
                                   int32_t *status, int32_t *detail);
/* flags [total persons] (file-major, as p2s_json_person_lengths): what np.array() of the person's "pose_keypoints_2d" list
 * would depend on beyond its numbers.  ALL_INTS: a non-empty list whose every element is a number token without fraction
 * and exponent (Python reads ints, NumPy makes an int64 array); HAS_NULL / HAS_BOOL: it holds null / true or false;
 * BIG_INT: an integer token beyond +-2^53, which float64 does not hold exactly; NOT_OBJECT: the person is not an object;
 * BAD_LIST: the value of the key is not an array. */
#define P2S_JSON_PERSON_ALL_INTS 1
#define P2S_JSON_PERSON_HAS_NULL 2
#define P2S_JSON_PERSON_HAS_BOOL 4
#define P2S_JSON_PERSON_BIG_INT 8
#define P2S_JSON_PERSON_NOT_OBJECT 16
#define P2S_JSON_PERSON_BAD_LIST 32
int p2s_json_person_flags(const p2s_json_batch *batch, int32_t *flags);

/* ---- .trc data rows (host threads) ---------------------------------------------------------------------------
 * Replaces DataFrame.to_csv in make_trc (triangulation.py:214): appends n_rows lines
 * `frames[r] \t repr(time[r]) \t repr(data[r][0]) \t ...\n` to the file (the 5 header lines are written by the
 * caller), floats exactly as Python's repr() prints them, NaN as an empty field. */
int p2s_trc_append_rows(const char *path, int64_t n_rows, int32_t n_cols, const int64_t *frames, const double *time,
                        const double *data, int32_t n_threads);
/* repr(float) of one value into out (>= 32 bytes, NUL-terminated); returns the length.  For tests. */
int p2s_format_float_repr(double value, char *out, int32_t capacity);

/* ---- associated-pose JSON files (host threads) -----------------------------------------------------------------
 * rewrite_json_files (personAssociation.py:552-580) for n_files (source, destination) pairs at once: destination =
 * json.dumps of the source document with 'people' replaced by the selected persons -- sel[sel_offsets[i] ..
 * sel_offsets[i+1]) holds, per proposal, the index of the person in the source's 'people' list or -1 for {} --
 * in Python's text (', ' / ': ' separators, ensure_ascii escapes, repr() floats, first-position / last-value for
 * repeated keys).  Whenever the reference would raise (unreadable or invalid source, no 'people' list, index out
 * of range) the destination is removed, as there.  Paths as in p2s_json_parse.  written [n_files] (may be NULL):
 * 1 = file written, 0 = removed. */
int p2s_json_rewrite_people(const char *src_paths, const int64_t *src_offsets, const char *dst_paths,
                            const int64_t *dst_offsets, int64_t n_files, const int64_t *sel_offsets, const int32_t *sel,
                            int32_t n_threads, int8_t *written);

/* ---- single-person JSON files (host threads) -----------------------------------------------------------------------
 * The documents Utilities/pose_extract_person.py:process writes, byte for byte json.dump's text, for n_files paths at once
 * (paths as in p2s_json_parse).  kind[i]: 0 = {"version": 1.3, "people": []}; 1 = one person, person_id [-1], its
 * pose_keypoints_2d the 3 * n_kpts numbers values[i][...] as repr() floats (NaN, Infinity, -Infinity) and the seven other
 * lists empty in the reference's key order; 2 = the same with the numbers as integers (values of kind 0 are not read).
 * A value of kind 2 that is not an integer within int64, another kind, or 3 * n_kpts outside [1, 381]: P2S_ERR_INVALID_ARG
 * before anything is written.  written [n_files] (may be NULL): 1 = file written, 0 = it could not be created or written. */
int p2s_write_person_files(const char *paths, const int64_t *path_offsets, int64_t n_files, const double *values,
                           const int8_t *kind, int32_t n_kpts, int32_t n_threads, int8_t *written);

/* ---- proposals from the association result, first half (host threads) -----------------------------------------
 * The per-detection rows of person_index_per_cam (personAssociation.py:512-527) for every frame: rows[f][r][c] =
 * np.argmax of detection r's affinities to camera c's detections, -1 when camera c has none or none is positive.
 * rows [F][n_max][C] (the first sum(n_persons[f]) rows of a frame are written).  The order-sensitive second half
 * (np.unique / np.argsort / first-come filter, :528-549) stays with the caller in NumPy: np.argsort's order among
 * equal counts is unspecified and build-dependent, and it decides the person order in the output files. */
int p2s_assoc_argmax_rows(int64_t n_frames, int32_t n_cams, int32_t n_max, const double *affinity, const int32_t *n_persons,
                          int32_t n_threads, int32_t *rows);

/* Proposals, second half (personAssociation.py:528-549), every frame at once, around the one call whose result is not
 * specified -- np.argsort of the multiplicities, which the caller makes itself on the array the reference would pass:
 *   p2s_assoc_unique_rows: np.unique(rows, axis=0, return_counts=True) per frame: uniq [F][n_max][C] (the distinct rows of
 *     rows[f][0 .. n_rows[f]) in lexicographic order), counts [F][n_max] int64, n_uniq [F];
 *   p2s_assoc_filter_rows: with rank[f][i] = index of the i-th ranked distinct row (np.argsort(counts)[::-1]): the
 *     first-come filter (a row that names, for some camera, a person named by ANY row ranked before it is dropped) and the
 *     minimum number of cameras; props [F][n_max][C] (-1 = the reference's NaN), n_props [F]. */
int p2s_assoc_unique_rows(int64_t n_frames, int32_t n_cams, int32_t n_max, const int32_t *rows, const int32_t *n_rows,
                          int32_t n_threads, int32_t *uniq, int64_t *counts, int32_t *n_uniq);
int p2s_assoc_filter_rows(int64_t n_frames, int32_t n_cams, int32_t n_max, const int32_t *uniq, const int32_t *n_uniq,
                          const int32_t *rank, int32_t min_cams, int32_t n_threads, int32_t *props, int32_t *n_props);

/* ---- trajectory gaps after triangulation (csrc/p2s_gaps.hip) --------------------------------------
 * The frame-sequential tail of triangulate_all (triangulation.py:888-953) for every column of a trial -- of all its
 * persons side by side -- in one call each.  Host arrays in and out; ctx == NULL runs the same functions on the host.
 * n_frames 1 .. 2^30, n_cols 1 .. 65535; a refused call (P2S_ERR_INVALID_ARG) has written nothing.
 *
 * p2s_interpolate_gaps: interpolate_zeros_nans (common.py:669-712) on coords [n_frames][n_cols] with the abscissae
 * labels [n_frames] (strictly increasing, within +-2^53).  A sample is bad when it is NaN or == 0 (-0.0 included; +-inf
 * is good).  A column with 4 or fewer good samples comes back untouched.  Bad samples form runs that break where two
 * consecutive bad labels differ by more than 1; a run of more than max_gap samples (a count, or +inf) becomes NaN, the
 * others take scipy's interp1d through the good samples:
 *   P2S_GAPS_KIND_NONE       kind='linear' without extrapolation (np.interp's arithmetic, bit for bit; NaN beyond the
 *                            first and last good label) -- the reference's call without a kind
 *   P2S_GAPS_KIND_LINEAR     'linear', fill_value='extrapolate' (interp1d._call_linear, bit for bit)
 *   P2S_GAPS_KIND_SLINEAR, _QUADRATIC, _CUBIC   make_interp_spline of degree 1, 2, 3 with scipy's knots, extrapolated;
 *                            the banded system is solved without pivoting: scipy's values to rounding
 * out [n_frames][n_cols]; status [n_cols]: 0, or P2S_GAPS_NONFINITE for a column of a spline kind with +-inf among its
 * good samples, which comes back untouched (the caller's host path decides). */
#define P2S_GAPS_KIND_NONE 0
#define P2S_GAPS_KIND_LINEAR 1
#define P2S_GAPS_KIND_SLINEAR 2
#define P2S_GAPS_KIND_QUADRATIC 3
#define P2S_GAPS_KIND_CUBIC 4
#define P2S_GAPS_NONFINITE 1
#define P2S_GAPS_WORKSPACE_KB (256 * 1024)
int p2s_interpolate_gaps(p2s_ctx *ctx, int64_t n_frames, int32_t n_cols, const double *coords, const int64_t *labels, double max_gap,
                         int32_t kind, double *out, int32_t *status);
/* fill_large_gaps_with (triangulation.py:922-926).  P2S_GAPS_FILL_LAST_VALUE: every NaN takes the last value before it
 * that is not NaN, leading ones the first after them; what is still NaN (a column never seen) and +inf become 0.
 * P2S_GAPS_FILL_ZEROS: NaN and +inf become 0.  Any other `how`: out = coords. */
#define P2S_GAPS_FILL_LAST_VALUE 1
#define P2S_GAPS_FILL_ZEROS 2
int p2s_fill_gaps(p2s_ctx *ctx, int64_t n_frames, int32_t n_cols, const double *coords, int32_t how, double *out);
/* The spans of the report (triangulation.py:917-919, 946-953): per column of x [n_frames][n_cols] the runs of
 * consecutive positions p, first < p < last, whose value is 0 or not finite.  table [capacity][4] gets the rows
 * (column, start, end, long) -- long: more than max_gap positions -- by column, then by position; *count the rows there
 * are.  With count > capacity the first `capacity` rows are written and *overflow is 1, else 0. */
int p2s_gap_runs(p2s_ctx *ctx, int64_t n_frames, int32_t n_cols, const double *x, int64_t first, int64_t last, double max_gap,
                 int64_t capacity, int32_t *table, int64_t *count, int32_t *overflow);
/* Kernel time of the last of the three calls above on this context, from HIP events around its kernels. */
int p2s_gaps_kernel_ms(p2s_ctx *ctx, float *elapsed_ms);

/* ---- confidence timeline (Utilities/confidence_timeline.py:89-130; csrc/p2s_timeline.hip) ------------
 * The rows of the reference's CSV and the series of its plot for every camera folder in one call.  Host arrays in and
 * out; ctx == NULL runs the same functions on the host.  Camera c has the files file_off[c] .. file_off[c + 1]
 * (file_off[0] = 0, a camera may have none); file f lists the persons person_base[f] .. person_base[f + 1] of valid [N]
 * (nonzero: the list held at least 78 numbers) and conf [N][n_kpts] (the confidences of the 1 .. 26 resolved keypoints).
 * Rows: a file contributes n_kpts rows for every valid person, by frame (the file's position in its camera), then
 * person (the position in the file's list, invalid entries counted), then slot (the index into the resolved names):
 *   row_off [n_cams + 1]; frame, person, slot (int32) and confidence [n_rows], n_rows = n_kpts x the valid persons.
 * Series: n_people [n_cams] is the longest list of every camera, P_c.  For every camera and every person index below
 * P_c, in that order, one series: the files in which that entry is valid, in file order:
 *   series_off [n_series + 1], n_series = the sum of P_c; series_frame [n_rows / n_kpts]; series_conf
 *   [n_kpts][n_rows / n_kpts], slot-major, a series at the same offsets in every slot.
 * n_rows and n_series are the caller's sizes of these arrays: other values than the input's are refused
 * (P2S_ERR_INVALID_ARG, nothing written, the message names the right ones).  Fewer than 2^31 files and persons. */
int p2s_timeline_rows_host(p2s_ctx *ctx, int32_t n_cams, const int64_t *file_off, const int64_t *person_base, const uint8_t *valid,
                           int32_t n_kpts, const double *conf, int64_t n_rows, int64_t n_series, int64_t *row_off, int32_t *frame,
                           int32_t *person, int32_t *slot, double *confidence, int64_t *n_people, int64_t *series_off,
                           int32_t *series_frame, double *series_conf);
/* Milliseconds the kernels of this context's last p2s_timeline_rows_host took (HIP events around them). */
int p2s_timeline_kernel_ms(p2s_ctx *ctx, float *elapsed_ms);
/* The reference's confidence_timeline.csv (csv.writer, newline=''): the header frame,person,keypoint,confidence and one
 * line a row, terminated by \r\n, the keypoint as names[name_off[slot] .. name_off[slot + 1]], the confidence as
 * repr(float): shortest digits that round-trip, nan, inf, -inf.  Row ranges are formatted on host threads (n_threads, 0
 * = the machine's, at most 32) and written in order.  The file is created or truncated.  A name holding a comma, a quote
 * or a line break, or a slot outside the names, is refused before the file is opened. */
int p2s_timeline_write_csv(const char *path, int64_t n_rows, const int32_t *frame, const int32_t *person, const int32_t *slot,
                           const double *confidence, int32_t n_names, const char *names, const int64_t *name_off, int32_t n_threads);

/* ---- extrinsics refinement from keypoints (csrc/p2s_refine.hip) -------------------------------------
 * Bundle adjustment of the cameras' rotations and translations on the 2D keypoints of a trial, the 3D points eliminated
 * by the Schur complement; intrinsics are held and the observations are pinhole (undistorted) pixels.  Host arrays in and
 * out, fp64 throughout; ctx == NULL runs the same functions on the host.
 *   xyl [n_points][n_cams][3] (x px, y px, likelihood; dtype P2S_F32 / P2S_F64), Kmats [n_cams][9], R_in [n_cams][9]
 *   (world -> camera, row-major), t_in [n_cams][3], X0 [n_points][3] the start points.
 * Weight of an observation: s = l when l >= lik_thr and x, y, l are finite, else 0.  A point with fewer than min_cams
 * (raised to 2) observations of s > 0, or with a non-finite X0 row, is dropped: its weights are 0 and its row of X_out is
 * NaN.  Residuals e = s (u_proj - u_obs), s (v_proj - v_obs) with u_proj = fx Xc.x / Xc.z + cx, Xc = R X + t; the cost is
 * the sum over the components of e^2 for |e| <= huber_px, else 2 huber_px |e| - huber_px^2 (scipy's loss='huber' with
 * f_scale = huber_px, without its factor 1/2).  Gauge: camera 0 is held, and of camera 1's translation the coordinate
 * j = argmax_j |(t1 - R1 R0^T t0)_j| (first index on ties): 6 n_cams - 7 free parameters.  Levenberg-Marquardt from
 * lambda = 1e-3 (/ 10 on an accepted trial, floor 1e-9; x 10 on a refused one), one trial an iteration, until the
 * relative decrease of an accepted trial is below ftol, a refused trial's cost is within ftol of the current one,
 * max_iter trials have run, or lambda > 1e12.
 * R_out, t_out [n_cams][..], X_out [n_points][3]; max_iter = 0 hands the input back with cost_after = cost_before.
 * Refused with P2S_ERR_INVALID_ARG, before any refinement kernel runs: n_cams outside 2 .. P2S_MAX_CAMS, non-finite Kmats,
 * R_in or t_in, no kept point, a camera without a kept observation, a kept observation whose point lies behind its
 * camera (Xc.z <= 0) at entry; the message names the camera (and the point).  Two calls on the same input return the same
 * bits: every sum is taken in a fixed order, P2S_REFINE_TILE points a workgroup pass, at most P2S_REFINE_MAX_PARTS
 * partial sums of a launch. */
#define P2S_REFINE_TILE 256
#define P2S_REFINE_MAX_PARTS 128
typedef struct p2s_refine_params {
    double lik_thr;      /* observations below it do not count */
    double huber_px;     /* delta of the Huber loss, px of weighted residual (> 0) */
    double ftol;         /* relative decrease of the cost that ends the iteration */
    int32_t min_cams;    /* cameras a point needs (values below 2 are taken as 2) */
    int32_t max_iter;    /* Levenberg-Marquardt trials at most (>= 0) */
} p2s_refine_params;
typedef struct p2s_refine_report {
    double cost_before, cost_after;   /* the Huber cost at the input and at the output */
    double lambda_final;
    int64_t kept_points;
    int32_t iterations, accepted;     /* trials run; trials that lowered the cost */
    int32_t held_coord;               /* j: the coordinate of camera 1's translation that is held */
    int32_t reserved;
    double rms_before[P2S_MAX_CAMS];  /* per camera sqrt(sum s^2 d^2 / sum s^2), d the reprojection distance in px */
    double rms_after[P2S_MAX_CAMS];
} p2s_refine_report;
int p2s_refine_extrinsics_host(p2s_ctx *ctx, int64_t n_points, int32_t n_cams, int32_t dtype, const void *xyl, const double *Kmats,
                               const double *R_in, const double *t_in, const double *X0, const p2s_refine_params *params,
                               double *R_out, double *t_out, double *X_out, p2s_refine_report *report);
/* Milliseconds between the HIP events around this context's last p2s_refine_extrinsics_host: its kernels and the
 * reduced solves on the host between them. */
int p2s_refine_kernel_ms(p2s_ctx *ctx, float *elapsed_ms);
/* The held coordinate j of the gauge above from R_in and t_in of cameras 0 and 1 (host arithmetic, no context). */
int p2s_refine_held_coord(const double *R_in, const double *t_in, int32_t *held);

/* ---- relative poses of camera pairs from correspondences (csrc/p2s_relpose.hip) -----------------------
 * The essential matrix of every camera pair out of contaminated correspondences: hypotheses from samples, MSAC scores,
 * refits on the inliers, the cheirality count.  Host arrays in and out, fp64 throughout; ctx == NULL runs the same
 * per-hypothesis and per-point functions on the host.
 *   xn [n_cams][n_points][2] normalised pinhole coordinates (undistorted, K^-1 applied), usable [n_cams][n_points],
 *   pairs [n_pairs][2] (a, b), samples [n_pairs][n_hyp][sample_size] point indices, thr2 [n_pairs] the squared Sampson
 *   threshold in normalised units.  A point counts in a camera when it is usable there and both coordinates are finite;
 *   the points of a pair are those that count in both of its cameras.
 * Hypothesis of a sample: each side's points translated to their centroid and scaled to an RMS distance of sqrt 2, the
 * sample_size x 9 system x_b'^T F' x_a' = 0, F' the eigenvector of the smallest eigenvalue of A^T A (first index on ties),
 * F = Tb^T F' Ta, E = U diag(1, 1, 0) V^T of F's singular value decomposition; the sign of E is free.  A sample with a
 * repeated index, an index outside [0, n_points) or a point that is not one of the pair's is refused, as is one whose F is
 * not finite or has no two singular values above 0: E is NaN, the cost +inf, 0 inliers; the call does not fail.
 * Score: d = (x_b^T E x_a)^2 / ((E x_a)_1^2 + (E x_a)_2^2 + (E^T x_b)_1^2 + (E^T x_b)_2^2) over the pair's points, or, with
 * score_points > 0 and more points than that in some pair, over the pair's points of rank floor(i k / score_points), i = 0 ..
 * score_points - 1, k the pair's count (every point of a pair with no more); a d that is not a number adds nothing.
 * cost = sum min(d, thr2), inliers = the count of d < thr2; the winner has the lowest cost, the lowest index on ties.
 * Then, over all of the pair's points: the winner's cost, and at most `rounds` refits: the 9 x 9 system of the inliers, with
 * the same normalisation from the inliers' moments (centroid sum x / n, mean squared distance sum |x|^2 / n - |centroid|^2),
 * is solved and projected as above; the refit is kept when its cost is lower, else the refits end; fewer than 8 inliers end
 * them too.  The four (R, t) of E, X_b = R X_a + t, |t| = 1, in this order: (Ra, t), (Ra, -t), (Rb, t), (Rb, -t), where t has
 * its largest coordinate (first on ties) positive and Ra is the rotation of the larger trace; front = the inliers with z_a >
 * 0 and z_b > 0, z_a = -((x_b x R x_a) . (x_b x t)) / |x_b x R x_a|^2, z_b = (z_a R x_a + t)_3; the highest count wins, the
 * first on ties.
 * Out, per pair: E [9], R [9], t [3], cost, inliers, front, winner (the hypothesis' index), refits (those kept), mask
 * [n_pairs][n_points] of the inliers.  A pair with fewer than sample_size points, or without a hypothesis of finite cost,
 * is no error: NaN, counts 0, winner -1.  hyp_E [n_pairs][n_hyp][9], hyp_cost and hyp_inliers [n_pairs][n_hyp] (each may be
 * NULL) receive every hypothesis.
 * Refused with P2S_ERR_INVALID_ARG before any kernel runs: n_cams outside 2 .. P2S_MAX_CAMS, sample_size outside
 * P2S_RELPOSE_MIN_SAMPLE .. P2S_RELPOSE_MAX_SAMPLE, n_hyp < 1, rounds < 0, a pair that names a camera twice or out of range,
 * a thr2 that is not positive and finite.  Two calls on the same input return the same bits: every floating-point sum is
 * taken in a fixed order (P2S_RELPOSE_TILE points a pass, at most P2S_RELPOSE_MAX_CHUNKS chunk sums a hypothesis and
 * P2S_RELPOSE_MAX_PARTS partial sums a pair), the counts are integers. */
#define P2S_RELPOSE_TILE 256
#define P2S_RELPOSE_MAX_CHUNKS 64
#define P2S_RELPOSE_MAX_PARTS 128
#define P2S_RELPOSE_MIN_SAMPLE 8
#define P2S_RELPOSE_MAX_SAMPLE 16
int p2s_relative_poses_host(p2s_ctx *ctx, int32_t n_cams, int64_t n_points, const double *xn, const uint8_t *usable, int32_t n_pairs,
                            const int32_t *pairs, int32_t n_hyp, int32_t sample_size, const int32_t *samples, const double *thr2,
                            int32_t rounds, int32_t score_points, double *E_out, double *R_out, double *t_out, double *cost_out,
                            int32_t *inliers_out, int32_t *front_out, int32_t *winner_out, int32_t *refits_out, uint8_t *mask_out,
                            double *hyp_E, double *hyp_cost, int32_t *hyp_inliers);
/* Milliseconds between the HIP events around this context's last p2s_relative_poses_host: its kernels and the eigen-solves
 * of the refits on the host between them. */
int p2s_relpose_kernel_ms(p2s_ctx *ctx, float *elapsed_ms);

#ifdef __cplusplus
}
#endif
#endif /* P2S_H */
