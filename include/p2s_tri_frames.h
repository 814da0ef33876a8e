/* p2s_tri_frames.h -- the C ABI of triangulation with per-frame cameras (csrc/p2s_tri_frames.hip, libp2s_hip.so), beside
 * p2s.h, whose context, parameters, error codes and conventions it uses.  tests/test_tri_frames_host.py holds this header
 * against the library and the Python binding, tests/test_tri_frames_gpu.py runs the two calls among all other stages on one
 * shared, poisoned engine. */
#ifndef P2S_TRI_FRAMES_H
#define P2S_TRI_FRAMES_H

#include "p2s.h"

#ifdef __cplusplus
extern "C" {
#endif

/* The per-unit contract of p2s_triangulate_* (p2s.h) with PER-FRAME cameras (a moving and / or zooming rig; Utilities/reproj_from_trc_calib.py:86-141
 * reads such a calibration): unit (block b, keypoint k) is triangulated with the projection matrices of calibration frame
 * block_frame[b].  Pinhole branch without L/R swap, 2 <= n_cams <= 16; every camera-subset candidate is evaluated in
 * fp64 (no fp32 screen).  The calls are self-contained: they need no p2s_set_calibration and leave the context's static
 * calibration untouched.
 *   P            [n_cal_frames][n_cams][12] float64 projection matrices
 *   xyl          [n_blocks][n_cams][n_kpts][3], dtype P2S_F32 or P2S_F64
 *   block_frame  [n_blocks] int64, every entry in [0, n_cal_frames) and never decreasing: the blocks of one calibration
 *                frame (its persons) are consecutive; frames may be skipped or start anywhere
 * outputs as p2s_triangulate_*.  P2S_ERR_INVALID_ARG, with the cause in p2s_last_error() and nothing written, for
 * n_cams outside [2, 16], params->undistort_points or params->handle_lr_swap set, n_cal_frames < 1, a block_frame entry
 * out of range or below its predecessor, and null operands with n_blocks > 0; n_blocks == 0 succeeds and launches
 * nothing.  Counters 0 to 2 of p2s_get_tri_stats count these calls as well.
 * p2s_triangulate_frames_device reads block_frame back (8 bytes a block) to check it and to plan its waves, i.e. it
 * synchronises the stream once BEFORE its first launch; level 0 and the search run in one launch and nothing is read
 * after it. */
int p2s_triangulate_frames_device(p2s_ctx *ctx, int64_t n_cal_frames, int32_t n_cams, const double *d_P, int64_t n_blocks,
                                  int32_t n_kpts, int32_t dtype, const void *d_xyl, const int64_t *d_block_frame,
                                  const p2s_tri_params *params, double *d_Q, float *d_err, uint8_t *d_n_excl,
                                  uint32_t *d_excl_mask);
int p2s_triangulate_frames_host(p2s_ctx *ctx, int64_t n_cal_frames, int32_t n_cams, const double *P, int64_t n_blocks,
                                int32_t n_kpts, int32_t dtype, const void *xyl, const int64_t *block_frame,
                                const p2s_tri_params *params, double *Q, float *err, uint8_t *n_excl, uint32_t *excl_mask);

#ifdef __cplusplus
}
#endif
#endif /* P2S_TRI_FRAMES_H */
