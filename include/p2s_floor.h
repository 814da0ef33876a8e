/* p2s_floor.h -- the C ABI of the floor stage (csrc/p2s_floor.hip, libp2s_hip.so), beside p2s.h, whose context, error
 * codes and conventions it uses.  tests/test_floor_host.py holds this header against the library and the Python binding,
 * tests/test_floor_gpu.py runs the stage among all others on one shared, poisoned engine. */
#ifndef P2S_FLOOR_H
#define P2S_FLOOR_H

#include "p2s.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---- the dominant plane of point sets: the floor under a walk (csrc/p2s_floor.hip) ---------------------
 * n_problems independent problems (trials, persons), each the plane that most of its points lie on: hypotheses from sampled
 * triples, MSAC scores, refits on the inliers.  Host arrays in and out, fp64 throughout; ctx == NULL runs the same
 * per-hypothesis and per-point functions on the host.
 *   points [n_problems][n_points][3], usable [n_problems][n_points], ref [n_problems][3] a point known to lie above the
 *   plane (it orients the normal and is the origin of the refits' moments), samples [n_problems][n_hyp][3] point indices,
 *   thr [n_problems] in the points' unit.  A point counts when it is usable and its three coordinates are finite.
 * Hypothesis of a sample (i0, i1, i2): n = (p1 - p0) x (p2 - p0) / |.|, d = n . p0, (n, d) negated when n . ref - d < 0.
 * A sample with a repeated index, an index outside [0, n_points) or a point that does not count is refused, as is one
 * whose cross product's norm is not finite and above 0, or whose plane holds ref (n . ref - d = 0): the plane is NaN, the
 * cost +inf, 0 inliers; the call does not fail.
 * Score, over all of the problem's points: s = n . x - d, cost = sum min(s^2, thr^2), inliers = the count of s^2 < thr^2,
 * below = the count of s < -thr; an s that is not a number adds nothing.  The winner has the lowest cost, the lowest index
 * on ties.
 * Then the winner's sums over the points and at most `rounds` refits: with u = x - ref over the inliers, m = sum u / k and
 * S = sum u u^T / k - m m^T, the normal is the eigenvector of S's smallest eigenvalue (cyclic Jacobi; the lower index
 * first on ties), the plane passes through ref + m and is oriented by ref as above; the refit is kept when its cost is
 * lower, else the refits end; fewer than 3 inliers, or a refit plane that is not finite or holds ref, end them too.
 * Out, per problem: plane [4] (n, d), cost, inliers, below, winner (the hypothesis' index), refits (those kept), centroid
 * [3] = ref + m of the result's inliers, evals [3] the ascending eigenvalues of their S, mask [n_problems][n_points] of the
 * inliers.  A problem with fewer than 3 counting points, or without a hypothesis of finite cost, is no error: NaN, counts
 * 0, winner -1.  hyp_plane [n_problems][n_hyp][4], hyp_cost and hyp_inliers [n_problems][n_hyp] (each may be NULL) receive
 * every hypothesis.
 * Refused with P2S_ERR_INVALID_ARG before any kernel runs: n_problems outside 1 .. 65535, n_points outside 1 .. 2^30 - 1,
 * n_hyp < 1 (or 2^27 hypotheses and more in all), rounds < 0, a thr that is not positive and finite, a ref that is not
 * finite; the message names the problem.  Two calls on the same input return the same bits: every floating-point sum is
 * taken in a fixed order (P2S_FLOOR_TILE points a pass, at most P2S_FLOOR_MAX_CHUNKS chunk sums a hypothesis and
 * P2S_FLOOR_MAX_PARTS partial sums a problem), the counts are integers. */
#define P2S_FLOOR_TILE 256
#define P2S_FLOOR_MAX_CHUNKS 64
#define P2S_FLOOR_MAX_PARTS 128
int p2s_fit_planes_host(p2s_ctx *ctx, int32_t n_problems, int64_t n_points, const double *points, const uint8_t *usable, const double *ref,
                        int32_t n_hyp, const int32_t *samples, const double *thr, int32_t rounds, double *plane_out, double *cost_out,
                        int32_t *inliers_out, int32_t *below_out, int32_t *winner_out, int32_t *refits_out, double *centroid_out,
                        double *evals_out, uint8_t *mask_out, double *hyp_plane, double *hyp_cost, int32_t *hyp_inliers);
/* Milliseconds between the HIP events around this context's last p2s_fit_planes_host: its kernels and the eigen-solves of
 * the refits on the host between them. */
int p2s_floor_kernel_ms(p2s_ctx *ctx, float *elapsed_ms);

#ifdef __cplusplus
}
#endif
#endif /* P2S_FLOOR_H */
