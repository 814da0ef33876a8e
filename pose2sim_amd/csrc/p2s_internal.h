// Internal structures shared by the C-ABI layer (p2s_api.hip) and the kernels.
#ifndef P2S_INTERNAL_H
#define P2S_INTERNAL_H

#include <hip/hip_runtime.h>
#include <stdint.h>
#include "p2s.h"

// One camera, device resident (computeP + retrieve_calib_params, common.py:254-324).
struct P2sCam {
    double P[12];          // projection matrix (optim_K based when undistorting)
    double fx, fy, cx, cy; // original intrinsics
    double ifx, ify;       // 1/fx, 1/fy (OpenCV multiplies by reciprocals)
    double k[5];           // k1 k2 p1 p2 k3
    double R[9];           // rotation matrix, world -> camera
    double T[3];
    double nk[9];          // optim_K
    double iK[9];          // inverse of the original K        (association rays)
    double center[3];      // -R^T T                            (association rays)
    float Pf[12];          // P rounded to float: the fp32 screen of the camera-subset search (p2s_tri_pool.hip)
    float pad_[4];
};

// Kernel diagnostics (phase stamps, memory-skeleton modes) exist only in a -DP2S_DIAG build (exp/README.md): in the
// shipped library the mode is the constant 0 and every branch on it is compiled out.
#ifdef P2S_DIAG
#define P2S_DEBUG_MODE(a) ((a).debug_mode)
#else
#define P2S_DEBUG_MODE(a) 0
#endif

// p2s_get_tri_stats: [0] units that entered the camera-subset search, [1] camera subsets evaluated (lane-evaluations of
// DLT + reprojection error beyond level 0), [2] evaluation passes (64-lane), [3] units whose search was cut short by
// P2S_MAX_SUBSETS_PER_LEVEL (they come back as not triangulated; the reference would have gone on), [4] per-camera errors
// computed for the candidates of the pruned passes, [5] those candidates (a part of [1]), [6] camera subsets looked at by
// the fp32 screen of p2s_tri_pool.hip (only its survivors are evaluated and counted in [1]), [7] screen passes (64-lane)
#define P2S_N_STATS 8
// the counters are kept in shards of their own 64-byte lines (a wave adds to shard blockIdx % P2S_STAT_SHARDS): one
// word takes ~88 atomics per microsecond, and 40 000 waves adding to ONE word cost 1.2 ms per launch
#define P2S_STAT_SHARDS 256
#define P2S_STAT_STRIDE 8        // unsigned long long per shard (64 bytes)

#define P2S_MAX_SUBSETS_PER_LEVEL (1u << 26)   // search kernel: deeper levels are not entered (see p2s_tri.hip)
// The work list is cut into shards (workgroup b appends to shard b % P2S_WL_SHARDS) so that the
// append counters do not serialise: one returning atomic per wave on ONE word caps near 90 per us.
#define P2S_WL_SHARDS 128
#define P2S_REC_HDR 16           // record header: u32 unit in chunk + padding to 16 bytes (records are 16-byte multiples)

struct P2sTriArgs {
    const void *xyl;             // whole tensor [n_blocks_total][C][K][3]
    const int32_t *swap_idx;
    double *Q;
    float *err;
    uint8_t *n_excl;
    uint32_t *mask;
    const P2sCam *cams;
    const uint32_t *binom;       // [33][33] binomial coefficients
    unsigned long long *stats;   // [P2S_N_STATS] counters of this context, added to with one atomic per wave (may be NULL)
    const uint16_t *sub_tab;     // fused kernel (C <= 16): every camera subset as a bit mask, by level, in itertools.combinations order
    const uint32_t *sub_off;     // [C + 2] start of level k in sub_tab
    uint32_t *wl_count;          // work list of this chunk: P2S_WL_SHARDS record counts, then P2S_WL_SHARDS job tickets (zeroed before kernel 1)
    unsigned char *wl_rec;       // records: {u32 unit id in chunk, pad to 16 B, T obs[C][3] (, T obs_swapped[C][3]), pad to 16 B}
    int64_t block0;              // first (frame, person) block of this chunk
    int64_t n_blocks;            // blocks in this chunk
    uint32_t wl_capacity;        // records per shard
    int32_t rec_bytes;
    int32_t K, C, FB;
    int32_t lds_binom_off, lds_rec_off;   // kernel 2 LDS layout: [P][binom][records]
    int32_t min_cams, undistort, lr_swap;
    unsigned char *deep_entries; // search kernel: units about to enter a level of more than deep_min_subsets subsets are
    uint32_t *deep_ctl;          //   exported here (NULL: every level is walked in the wave)
    uint32_t deep_capacity, deep_entry_bytes, deep_min_subsets;
    uint32_t max_subsets;        // search kernel: a level with more subsets is not entered (P2S_MAX_SUBSETS_PER_LEVEL unless tuned)
    uint32_t pool_pairs, pool_singles;   // p2s_tri_fused.hip: per XCD, workgroups that take two tiles, then workgroups that take one
    int32_t screen;              // p2s_tri_pool.hip: 1 = fp32 screen of the candidates, 0 = every candidate goes to the fp64 evaluation
    int32_t prune;               // exact pruning of the subset evaluations where a wave works on one unit (search kernel, deep rounds)
    int32_t job;                 // work-list records a search wave takes at a time (<= 64); sizes its LDS region
    int32_t debug_mode;          // 0 = normal; diagnostics only: 1 = stage + store (no compute), 2 = every tile reads tile 0
    double thr, lik_thr;
};

// ---- deep levels of the search, spread over the GPU (p2s_tri_deep.hip) ----------------------------------------------
#ifndef P2S_DEEP_CHUNK
#define P2S_DEEP_CHUNK 16384u            // consecutive subset ranks one wave evaluates per ticket (256 rounds of 64 lanes)
#endif
#define P2S_DEEP_MIN_SUBSETS 4096u       // a level with more subsets than this leaves the search kernel's wave (C(32, 3) = 4 960
                                         // and beyond: 7 % of the units of the 32-camera shard; the deep list holds 2^19 per
                                         // chunk of 4 M units, a unit that finds it full stays in its wave).  162 -> 142 ms on
                                         // the tenth-shard against 16 384 (1 024 the same, 256: 180)
#define P2S_DEEP_N_ENTRIES 0             // ctl words
#define P2S_DEEP_N_TICKETS 1
#define P2S_DEEP_TICKET 2
#define P2S_DEEP_PENDING 3
#define P2S_DEEP_WAITING 0u              // entry states
#define P2S_DEEP_SCHEDULED 1u
#define P2S_DEEP_DONE 2u
struct P2sDeepEntry {                    // followed by the unit's observations as in its work-list record
    uint32_t unit, level;                // unit id within the chunk; level to evaluate next
    int32_t Lmax;
    uint32_t nanmask, zeromask, mask, n_excl, state;
    uint32_t first_ticket, n_chunks, pad0, pad1;
    double err_min, Q[3];                // best of the last level (reporting only: a deeper level replaces it)
    double N[10];                        // level-0 normal matrix
};
struct P2sDeepPartial {                  // best plain and best swap candidate of one chunk
    double e, q[3], se, sq[3];
    uint32_t rank, S, srank, sS;
};
struct P2sDeepArgs {
    unsigned char *entries;
    uint32_t *ctl;
    uint32_t *sched_entry, *sched_chunk;
    P2sDeepPartial *partials;
    uint32_t capacity, max_tickets, entry_bytes, obs_bytes;
    uint32_t prune;                      // exact pruning of the evaluation (p2s_tri_deep.hip); 0: every camera of every candidate
};
hipError_t p2s_launch_deep_round(const struct P2sTriArgs &a, const P2sDeepArgs &d, int dtype, int grid_eval, int lds, hipStream_t s);

struct P2sTriLaunch {
    int grid0, threads0, lds0;   // level-0 (streaming) kernel
    int grid1, threads1, lds1;   // search kernel
    int force_tiled;             // diagnostics: use the LDS-tiled streaming kernel even when C <= 8
};

struct P2sAssocArgs {
    const int32_t *n_persons;   // [F][C]
    const int64_t *offsets;     // [F+1]
    const void *kpts;           // [rows][Kj][3]
    double *affinity;           // [F][Nmax][Nmax]
    const P2sCam *cams;
    int64_t n_frames;
    int32_t C, Kj, Nmax, max_iter;
    int32_t debug_mode;         // diagnostics only: 7 = per-frame phase timeline instead of the result (exp/assoc_trace.py)
    int32_t form;               // P2S_ASSOC_FORM_* (p2s_set_tuning: tests run both kernels on the same frames)
    unsigned long long *stats;  // sharded counters (frames, ADMM passes, Jacobi sweeps, fp64 operations) or NULL
    double recon_thr, min_affinity, w_rank, tol, w_sparse;
};

hipError_t p2s_launch_tri(const P2sTriArgs &a, int dtype, const P2sTriLaunch &g, hipStream_t s, hipStream_t side,
                          hipEvent_t k1_done);
// p2s_tri_fused.hip: streaming pass + in-wave subset search in one launch (pinhole, no L/R swap, C <= 16); up to 8
// cameras two tiles per wave, except for the last singles_pct % of every XCD's tiles
bool p2s_tri_fused_supports(int C, int dtype, int undistort, int lr_swap);
hipError_t p2s_launch_tri_fused(const P2sTriArgs &a, int dtype, int singles_pct, hipStream_t s);
// p2s_tri_pool.hip: persistent waves, failures pooled across tiles, fp32 screen + fp64 evaluation of the survivors
bool p2s_tri_pool_supports(int C, int dtype, int undistort, int lr_swap);
hipError_t p2s_launch_tri_pool(const P2sTriArgs &a, int dtype, int singles_pct, int tiles_per_wave, hipStream_t s);
struct P2sSingleArgs {
    const int32_t *n_persons;   // [F][C]
    const int64_t *offsets;     // [F+1]
    const void *tracked;        // [rows][3]
    int32_t *comb;              // [F][C]
    double *err;                // [F]
    double *Q;                  // [F][3]
    const P2sCam *cams;
    const uint32_t *binom;
    int64_t n_frames;
    int32_t C, min_cams;
    double thr, lik_thr;
};
hipError_t p2s_launch_single(const P2sSingleArgs &a, int dtype, hipStream_t s);

hipError_t p2s_launch_assoc(const P2sAssocArgs &a, int dtype, hipStream_t s);

// p2s_filter.hip
#define P2S_MAX_FILTER_ORDER 8
struct P2sFilterArgs {
    const double *in;            // [n_frames][n_cols]
    double *out;                 // [n_frames][n_cols]
    double *work;                // [n_frames + 2 padlen][n_cols] forward-pass output
    int64_t n_frames;
    int32_t n_cols, n_order, padlen;   // n_order = len(b) - 1
    double b[P2S_MAX_FILTER_ORDER + 1], a[P2S_MAX_FILTER_ORDER + 1], zi[P2S_MAX_FILTER_ORDER];
};
hipError_t p2s_launch_butter(const P2sFilterArgs &a, hipStream_t s);

// the window filters (Hampel, Gaussian, median) and the one-euro recurrence of filtering.py
struct P2sColFilterArgs {
    const double *in;            // [n_frames][n_cols]
    double *out;                 // [n_frames][n_cols]
    double *work;                // one-euro: forward pass [n_frames][n_cols]
    const double *w;             // Gaussian: 2 radius + 1 weights (device)
    int64_t n_frames;
    int32_t n_cols, kind, radius;
    double p[4];                 // Hampel: n_sigma; one-euro: dt, min_cutoff, beta, d_cutoff
};
hipError_t p2s_launch_col_filter(const P2sColFilterArgs &a, hipStream_t s);

// gcv_spline_filter_1d: one lane per run of >= 5 valid samples.  The host sorts the runs longest first; run r is lane
// r % 64 of wave r / 64, whose factor storage starts at work_off doubles into `work`: [sample][P2S_GCV_SLOTS][64 lanes]
// over the wave's longest run.
#define P2S_GCV_SLOTS 11
#define P2S_GCV_OK 0
#define P2S_GCV_ILL_POSED 1          // the banded Cholesky factorisation failed (scipy: 'Seems like the problem is ill-posed')
#define P2S_GCV_MAX_EVALS 2          // minimize_scalar stopped at maxiter = 500 evaluations
#define P2S_GCV_NAN 3                // minimize_scalar met a NaN
#define P2S_GCV_SINGULAR 4           // a zero pivot in the banded LU solve (LAPACK gbsv info > 0)
struct P2sGcvRun {
    int64_t work_off;            // doubles into P2sGcvArgs::work of this run's wave
    int32_t col, start, len;     // column, first frame, number of samples (>= 5)
    int32_t n_eval;              // out: GCV evaluations of the search ('auto')
    double med, scale;           // 'auto': the run's median and 1.4826 * MAD (MAD 0 -> 1)
    double lam;                  // out: the lambda of the final fit
    int32_t status, pad;         // out: P2S_GCV_*
};
struct P2sGcvArgs {
    double *data;                // [n_frames][n_cols]: read, and the filtered runs written in place
    P2sGcvRun *runs;             // [n_runs]
    double *work;
    int64_t n_frames;
    int32_t n_cols, n_runs;
    int32_t auto_mode;           // 1: GCV search of lambda on the normalised run; 0: lambda = fixed_lam on the raw run
    double fixed_lam, smoothing_factor;
};
hipError_t p2s_launch_gcv_spline(const P2sGcvArgs &a, hipStream_t s);

// p2s_sync.hip: synchronization speeds and their time-lagged Pearson correlation (synchronization.py:1271-1343, 1541-1575)
struct P2sSyncArgs {
    const double *coords;        // [total_rows][n_cols]: the cameras' masked (x, y) columns back to back
    double *filled;              // [total_rows][n_cols]: interpolated, filled and filtered columns
    double *work;                // [total_rows + 2 padlen n_cams][n_cols]: forward passes (camera c from row row0[c] + 2 padlen c)
    double *speed;               // [total_rows]: sum of |vertical speeds|, then filtered in place
    double *speed_work;          // [total_rows + 2 padlen n_cams]
    const int64_t *row0;         // [n_cams + 1] first row of each camera
    int64_t total_rows;
    int32_t n_cams, n_cols, n_order, padlen;   // n_order = len(b) - 1; padlen = 3 len(b) (scipy's filtfilt)
    int32_t filter_above;        // a camera is filtered when it has more frames than this (3 n_order, :1567)
    double b[P2S_MAX_FILTER_ORDER + 1], a[P2S_MAX_FILTER_ORDER + 1], zi[P2S_MAX_FILTER_ORDER];
};
hipError_t p2s_launch_sync_speeds(const P2sSyncArgs &a, hipStream_t s);

struct P2sPearsonArgs {
    const double *ref;           // [n_ref]
    const double *sig;           // the compared signals back to back
    const int64_t *sig0;         // [n_sig + 1] offsets into sig
    double *r;                   // [n_sig][n_lags]: r of lag lag_lo + t
    int64_t *argmax;             // [n_sig]
    double *max_corr;            // [n_sig]
    int64_t n_ref, lag_lo, n_lags;
    int32_t n_sig;
};
hipError_t p2s_launch_pearson(const P2sPearsonArgs &a, hipStream_t s);

struct P2sMetricsArgs {
    const double *xyz;           // [n_frames][n_markers][3]
    const int32_t *bones;        // [n_bones][2] (parent, child) marker indices
    double *bone_len;            // [n_bones][n_frames]
    double *bone_stats;          // [n_bones][3] mean, population sd, n_valid
    double *accel;               // [n_markers][n_frames - 2]
    int64_t *missing;            // [n_markers]
    int64_t n_frames;
    int32_t n_markers, n_bones;
};
hipError_t p2s_launch_trc_metrics(const P2sMetricsArgs &a, hipStream_t s);

// p2s_reproj.hip: 3D markers onto the image planes (Utilities/reproj_from_trc_calib.py:446-475)
struct P2sReprojArgs {
    const double *Q;             // [n_frames][K][3], Z-up (X, Y, Z); NaN = missing
    const double *P;             // plain mode: [C][Fp][12]
    const P2sCam *cams;          // distorted mode: [C] (R, T, fx, fy, cx, cy, k read); NULL = plain mode
    const double *sizes;         // [C][2] width, height
    double *uv_raw;              // [C][n_frames][K][2] unrounded pixels, or NULL
    double *uv;                  // [C][n_frames][K][2] rounded to one decimal, NaN outside the image
    int64_t n_units;             // n_frames * K
    int64_t Fp;                  // 1, or n_frames: one projection matrix per frame
    int32_t K, C;
};
hipError_t p2s_launch_reproject(const P2sReprojArgs &a, hipStream_t s);

// p2s_jitter.hip: exact order statistics of fp64 columns, NaN skipped (np.nanmedian and its kin)
struct P2sOrderArgs {
    const double *data;
    const int64_t *col_off;      // [n_cols] first element of every column, or NULL: col * n_rows
    const int64_t *col_len;      // [n_cols] length of every column, or NULL: n_rows
    const int64_t *ranks;        // [n_ranks] 0-based ranks among the non-NaN entries, negative = from the top; NULL: the
                                 // two middle positions (m - 1) / 2 and m / 2 of every column (n_ranks is taken as 2)
    double *out;                 // [n_cols][n_ranks]; NaN for a rank outside [0, m)
    int64_t *counts;             // [n_cols] non-NaN entries m, or NULL
    int64_t n_rows;
    int32_t n_cols, n_ranks;
};
hipError_t p2s_launch_order_stats(const P2sOrderArgs &a, hipStream_t s);

// p2s_jitter.hip: 2D keypoint jitter analysis (Utilities/keypoint_jitter_analyze.py:143-325).  Cameras back to back:
// camera c holds frames frame_off[c] .. frame_off[c + 1] and one displacement row fewer than frames, so its first row
// among all rows is frame_off[c] - c.
#define P2S_JITTER_KPTS 26
struct P2sJitterArgs {
    const double *series;        // [frames][26][3] (x, y, confidence)
    const int64_t *frame_off;    // [C + 1]
    const int64_t *tile_base;    // [C + 1] first 256-row tile of every camera
    double *disp;                // per camera [26][rows]: column-major, for the order statistics
    double *area;                // [frames] box area, NaN with fewer than 2 valid keypoints
    uint8_t *edge;               // [frames] 1: the box comes within 10 px of the image border
    const double *stats;         // [C][27][2] the two middle values of the 26 displacement columns and the area column
    const int64_t *stat_counts;  // [C][27] their non-NaN counts
    double *medians, *thresholds;   // [C][26]
    double *med_area;            // [C]
    uint8_t *mask;               // [rows][26]
    int32_t *counts;             // [C][26] events per keypoint (zeroed by the caller)
    uint32_t *tile_count;        // [n_tiles]
    long long *tile_off;         // [n_tiles] exclusive scan of tile_count
    long long *n_events;
    int32_t *events;             // [event_capacity][4] camera, frame, keypoint, pattern (0 A, 1 C, 2 D, 3 E)
    int64_t event_capacity;
    int64_t n_tiles, max_frames;
    double multiplier, x_edge, y_edge;   // width - 10, height - 10
    int32_t C;
};
hipError_t p2s_launch_jitter(const P2sJitterArgs &a, const P2sOrderArgs &o, hipStream_t s);

#endif
