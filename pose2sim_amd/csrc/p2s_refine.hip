// p2s_refine.hip -- refinement of the cameras' rotations and translations on the 2D keypoints of a trial: bundle
// adjustment with the 3D points eliminated by the Schur complement, Huber loss by reweighting inside Levenberg-Marquardt
// (include/p2s.h).  fp64 throughout; the points stay on the device for the whole iteration.
//
//   rf_prep_kernel     once: weights, kept points, the observations as [C][N] columns, what the refusals need
//   rf_point_kernel    build, per point: V = sum Jx^T W Jx, gp, and the inverse Cholesky factor of V + lambda diag V
//   rf_blocks_kernel   build, per (pass of points, camera pair a <= b): the 6 x 6 block sum_n Y_a Y_b^T of the Schur term,
//                      Y_c = W_c L^-T; per (pass, camera): U_c, g_c and W_c V^-1 gp.  The hot path: 3 N C (C + 1) / 2 x 36
//                      multiply-adds, blocked by camera pairs because the 6C x 6C triangle of 32 cameras (148 KB) leaves a
//                      workgroup no other LDS and a CU no second workgroup
//   RfStep             a pass of p2s_passes.h, per point: dX = -V^-1 (gp + sum_c W_c^T dc_c), the trial point, the trial's
//                      Huber cost
//   RfStats            a pass, per (part of the points, camera): cost, sum s^2 d^2, sum s^2 (the report's RMS)
//   rf_sum_kernel      (p2s_passes.h) the partial sums of a launch, added in a fixed order
//
// No floating-point atomic anywhere: a lane adds its points in order, a wave adds its lanes by the xor butterfly, a
// workgroup its waves in order (p2s_block_sum), rf_sum_kernel the workgroups' partial sums in order.  Two runs agree bit
// for bit.  The trial cameras R <- exp([dw]x) R, t <- t + dt are formed on the host next to the reduced solve (at most
// 185 unknowns) and go up with dc.  ctx == NULL runs the same per-point functions on the host, pass after pass
// (p2s_pass_host, the parts then added in order), in a Block of the host's memory.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include <string.h>

#include <algorithm>
#include <vector>

#include "p2s_ctx.h"
#include "p2s_passes.h"

#define RF_HD __host__ __device__ inline

struct P2sRfArgs {
    const double *ou, *ov, *os;  // [C][N] observations and weights (0: does not count)
    const uint8_t *kept;         // [N]
    const double *cams;          // [C][16] the cameras of the linearisation: fx fy cx cy R[9] t[3]
    const double *cams_t;        // [C][16] the trial's
    const double *X;             // [N][3]
    double *Xt;                  // [N][3] the trial's points
    double *pt;                  // [9][N] per point: L^-1 (l00 l10 l11 l20 l21 l22), gp
    const double *dc;            // [C][6] the cameras' step (dw, dt), 0 for held parameters
    double *partials;            // [width][parts]
    double *sums;                // [width]
    int64_t N;
    int32_t C, tiles, parts, move;
    double delta, lambda;
    double outer;                // curvature of a residual beyond delta, as a share of its reweighting weight
};

namespace {

constexpr int TILE = P2S_REFINE_TILE;              // points of a workgroup pass, lanes of a workgroup
constexpr int MAX_PARTS = P2S_REFINE_MAX_PARTS;    // workgroups along the points: what rf_sum_kernel adds per value
constexpr int NACC = 36;                           // values a lane accumulates in rf_blocks_kernel
constexpr int CAMW = 16;
// Weights of a residual component e: the gradient takes rho' = 1 for |e| <= delta, else w = delta / |e|.  The curvature
// takes 1 inside and outer x w outside, outer = clamp(1e3 lambda, 1e-3, 1): far from the minimum, where most residuals
// lie beyond delta and lambda is large, that is plain reweighting (outer = 1), whose step is the least-squares step;
// near it, where lambda has fallen, it is Huber's own second derivative (0 outside, with a floor that keeps V positive
// definite for a point with two cameras and an outlier), which converges quadratically.  Plain reweighting throughout
// majorises the linear branch and needed 120 .. 580 trials on the cases of DESIGN.md 4.21; the floor throughout
// overshoots from a start whose residuals all lie beyond delta (200 trials at 255 points); this needs 20 .. 45.
constexpr double OUTER_CURVATURE = 1e-3, OUTER_PER_LAMBDA = 1e3;

struct RfObs {
    double Jx[2][3], Jc[2][6], e[2], w[2], h[2];
};

RF_HD double rf_nan() { return __builtin_nan(""); }

// Xc = R X + t; rx = R X.
RF_HD void rf_transform(const double *cam, const double *X, double rx[3], double xc[3]) {
    const double *R = cam + 4, *t = cam + 13;
    for (int i = 0; i < 3; ++i) {
        rx[i] = R[3 * i] * X[0] + R[3 * i + 1] * X[1] + R[3 * i + 2] * X[2];
        xc[i] = rx[i] + t[i];
    }
}

// Residuals, reweighting and Jacobians of one observation of weight s > 0 (the local camera update: dXc/ddw = -[R X]x,
// dXc/ddt = I, dXc/dX = R).
RF_HD void rf_obs(const double *cam, const double *X, double u, double v, double s, double delta, double outer, RfObs &o) {
    const double *R = cam + 4;
    double rx[3], xc[3];
    rf_transform(cam, X, rx, xc);
    const double iz = 1.0 / xc[2];
    const double px = xc[0] * iz, py = xc[1] * iz;
    o.e[0] = s * (cam[0] * px + cam[2] - u);
    o.e[1] = s * (cam[1] * py + cam[3] - v);
    const double a0 = s * cam[0] * iz, a2 = -a0 * px;             // d e_u / d Xc = (a0, 0, a2)
    const double b1 = s * cam[1] * iz, b2 = -b1 * py;             // d e_v / d Xc = (0, b1, b2)
    for (int j = 0; j < 3; ++j) {
        o.Jx[0][j] = a0 * R[j] + a2 * R[6 + j];
        o.Jx[1][j] = b1 * R[3 + j] + b2 * R[6 + j];
    }
    o.Jc[0][0] = a2 * rx[1];
    o.Jc[0][1] = a0 * rx[2] - a2 * rx[0];
    o.Jc[0][2] = -a0 * rx[1];
    o.Jc[1][0] = b2 * rx[1] - b1 * rx[2];
    o.Jc[1][1] = -b2 * rx[0];
    o.Jc[1][2] = b1 * rx[0];
    o.Jc[0][3] = a0; o.Jc[0][4] = 0.0; o.Jc[0][5] = a2;
    o.Jc[1][3] = 0.0; o.Jc[1][4] = b1; o.Jc[1][5] = b2;
    for (int k = 0; k < 2; ++k) {
        const double ae = fabs(o.e[k]);
        o.w[k] = ae <= delta ? 1.0 : delta / ae;
        o.h[k] = ae <= delta ? 1.0 : outer * o.w[k];
    }
}

// delta^2 rho((e / delta)^2)
RF_HD double rf_huber(double e, double delta) {
    const double ae = fabs(e);
    return ae <= delta ? e * e : delta * (2.0 * ae - delta);
}

// W = Jc^T diag(w) Jx (6 x 3) and Y = W L^-T of an observation.
RF_HD void rf_wy(const RfObs &o, const double li[6], double W[6][3], double Y[6][3]) {
    for (int i = 0; i < 6; ++i) {
        const double c0 = o.h[0] * o.Jc[0][i], c1 = o.h[1] * o.Jc[1][i];
        for (int j = 0; j < 3; ++j) W[i][j] = c0 * o.Jx[0][j] + c1 * o.Jx[1][j];
        Y[i][0] = W[i][0] * li[0];
        Y[i][1] = W[i][0] * li[1] + W[i][1] * li[2];
        Y[i][2] = W[i][0] * li[3] + W[i][1] * li[4] + W[i][2] * li[5];
    }
}

RF_HD void rf_load_point(const P2sRfArgs &a, int64_t n, double X[3], double li[6], double gp[3]) {
    for (int i = 0; i < 3; ++i) X[i] = a.X[n * 3 + i];
    for (int i = 0; i < 6; ++i) li[i] = a.pt[i * a.N + n];
    if (gp)
        for (int i = 0; i < 3; ++i) gp[i] = a.pt[(6 + i) * a.N + n];
}

// ---- once: weights and kept points --------------------------------------------------------------------------------------
// -> the cameras that see the point (bit c), 0 for a dropped one; *behind the first camera with Xc.z <= 0 for one of the
// point's observations, -1 without one.  X0 is the caller's; Xw (the working copy) gets NaN for a dropped point.
template <typename T>
RF_HD uint32_t rf_prep_point(const T *xyl, const double *X0, const double *cams, double lik_thr, int min_cams, int64_t N, int C, int64_t n,
                             double *ou, double *ov, double *os, uint8_t *kept, double *Xw, int *behind) {
    uint32_t seen = 0;
    int count = 0;
    double X[3];
    for (int i = 0; i < 3; ++i) X[i] = X0[n * 3 + i];
    const bool start_ok = fabs(X[0]) + fabs(X[1]) + fabs(X[2]) < __builtin_huge_val();
    for (int c = 0; c < C; ++c) {
        const T *o = xyl + (n * C + c) * 3;
        const double x = (double)o[0], y = (double)o[1], l = (double)o[2];
        const bool ok = l >= lik_thr && l > 0.0 && fabs(x) + fabs(y) + fabs(l) < __builtin_huge_val();
        ou[(int64_t)c * N + n] = ok ? x : 0.0;
        ov[(int64_t)c * N + n] = ok ? y : 0.0;
        os[(int64_t)c * N + n] = ok ? l : 0.0;
        if (ok) {
            seen |= 1u << c;
            ++count;
        }
    }
    *behind = -1;
    if (count < min_cams || !start_ok) {
        for (int c = 0; c < C; ++c) os[(int64_t)c * N + n] = 0.0;
        for (int i = 0; i < 3; ++i) Xw[n * 3 + i] = rf_nan();
        kept[n] = 0;
        return 0;
    }
    for (int i = 0; i < 3; ++i) Xw[n * 3 + i] = X[i];
    kept[n] = 1;
    for (int c = C - 1; c >= 0; --c) {
        if (!(seen >> c & 1)) continue;
        double rx[3], xc[3];
        rf_transform(cams + c * CAMW, X, rx, xc);
        if (!(xc[2] > 0.0)) *behind = c;
    }
    return seen;
}

// ---- build, per point -----------------------------------------------------------------------------------------------------
RF_HD void rf_point_build(const P2sRfArgs &a, int64_t n) {
    double li[6] = {0, 0, 0, 0, 0, 0}, gp[3] = {0, 0, 0};
    if (a.kept[n]) {
        double X[3], V[6] = {0, 0, 0, 0, 0, 0};                  // v00 v10 v11 v20 v21 v22
        for (int i = 0; i < 3; ++i) X[i] = a.X[n * 3 + i];
        for (int c = 0; c < a.C; ++c) {
            const double s = a.os[(int64_t)c * a.N + n];
            if (s == 0.0) continue;
            RfObs o;
            rf_obs(a.cams + c * CAMW, X, a.ou[(int64_t)c * a.N + n], a.ov[(int64_t)c * a.N + n], s, a.delta, a.outer, o);
            for (int k = 0; k < 2; ++k) {
                const double h = o.h[k], *J = o.Jx[k];
                V[0] += h * J[0] * J[0];
                V[1] += h * J[1] * J[0];
                V[2] += h * J[1] * J[1];
                V[3] += h * J[2] * J[0];
                V[4] += h * J[2] * J[1];
                V[5] += h * J[2] * J[2];
                for (int i = 0; i < 3; ++i) gp[i] += o.w[k] * J[i] * o.e[k];
            }
        }
        const double d = 1.0 + a.lambda;
        const double l00s = V[0] * d;
        const double l00 = sqrt(l00s), i00 = 1.0 / l00;
        const double l10 = V[1] * i00, l20 = V[3] * i00;
        const double l11s = V[2] * d - l10 * l10;
        const double l11 = sqrt(l11s), i11 = 1.0 / l11;
        const double l21 = (V[4] - l20 * l10) * i11;
        const double l22s = V[5] * d - l20 * l20 - l21 * l21;
        const double l22 = sqrt(l22s), i22 = 1.0 / l22;
        // a point whose damped V is not positive definite stands still in this trial: L^-1 = 0
        if (l00s > 0.0 && l11s > 0.0 && l22s > 0.0 && i00 + i11 + i22 < __builtin_huge_val()) {
            li[0] = i00;
            li[1] = -l10 * i00 * i11;
            li[2] = i11;
            li[4] = -l21 * i11 * i22;
            li[3] = -(l20 * li[0] + l21 * li[1]) * i22;
            li[5] = i22;
        }
    }
    for (int i = 0; i < 6; ++i) a.pt[i * a.N + n] = li[i];
    for (int i = 0; i < 3; ++i) a.pt[(6 + i) * a.N + n] = gp[i];
}

// ---- build, per point and camera pair: acc [6][6] += Y_a Y_b^T -----------------------------------------------------------
RF_HD void rf_pair_point(const P2sRfArgs &a, int64_t n, int ca, int cb, double acc[NACC]) {
    const double sa = a.os[(int64_t)ca * a.N + n], sb = a.os[(int64_t)cb * a.N + n];
    if (sa == 0.0 || sb == 0.0) return;
    double X[3], li[6], W[6][3], Ya[6][3], Yb[6][3];
    rf_load_point(a, n, X, li, nullptr);
    RfObs o;
    rf_obs(a.cams + ca * CAMW, X, a.ou[(int64_t)ca * a.N + n], a.ov[(int64_t)ca * a.N + n], sa, a.delta, a.outer, o);
    rf_wy(o, li, W, Ya);
    if (cb != ca) {
        rf_obs(a.cams + cb * CAMW, X, a.ou[(int64_t)cb * a.N + n], a.ov[(int64_t)cb * a.N + n], sb, a.delta, a.outer, o);
        rf_wy(o, li, W, Yb);
    } else {
        for (int i = 0; i < 6; ++i)
            for (int j = 0; j < 3; ++j) Yb[i][j] = Ya[i][j];
    }
#pragma unroll
    for (int i = 0; i < 6; ++i)
#pragma unroll
        for (int j = 0; j < 6; ++j) acc[i * 6 + j] += Ya[i][0] * Yb[j][0] + Ya[i][1] * Yb[j][1] + Ya[i][2] * Yb[j][2];
}

// per point and camera: acc = U_c (upper triangle, 21), g_c (6), W_c V^-1 gp (6)
RF_HD void rf_cam_point(const P2sRfArgs &a, int64_t n, int c, double acc[NACC]) {
    const double s = a.os[(int64_t)c * a.N + n];
    if (s == 0.0) return;
    double X[3], li[6], gp[3], W[6][3], Y[6][3];
    rf_load_point(a, n, X, li, gp);
    RfObs o;
    rf_obs(a.cams + c * CAMW, X, a.ou[(int64_t)c * a.N + n], a.ov[(int64_t)c * a.N + n], s, a.delta, a.outer, o);
    rf_wy(o, li, W, Y);
    int k = 0;
#pragma unroll
    for (int i = 0; i < 6; ++i)
#pragma unroll
        for (int j = i; j < 6; ++j) acc[k++] += o.h[0] * o.Jc[0][i] * o.Jc[0][j] + o.h[1] * o.Jc[1][i] * o.Jc[1][j];
    const double q0 = li[0] * gp[0], q1 = li[1] * gp[0] + li[2] * gp[1], q2 = li[3] * gp[0] + li[4] * gp[1] + li[5] * gp[2];
    for (int i = 0; i < 6; ++i) {
        acc[21 + i] += o.w[0] * o.Jc[0][i] * o.e[0] + o.w[1] * o.Jc[1][i] * o.e[1];
        acc[27 + i] += Y[i][0] * q0 + Y[i][1] * q1 + Y[i][2] * q2;
    }
}

// Workgroup row y of rf_blocks_kernel: the camera pair a <= b of y < C (C + 1) / 2, else camera y - C (C + 1) / 2 (b = -1).
RF_HD void rf_row(int C, int y, int &ca, int &cb) {
    const int pairs = C * (C + 1) / 2;
    if (y >= pairs) {
        ca = y - pairs;
        cb = -1;
        return;
    }
    ca = 0;
    while (y >= C - ca) {
        y -= C - ca;
        ++ca;
    }
    cb = ca + y;
}

// ---- step, per point: the trial point and its cost ------------------------------------------------------------------------
RF_HD double rf_step_point(const P2sRfArgs &a, int64_t n) {
    if (!a.kept[n]) {
        for (int i = 0; i < 3; ++i) a.Xt[n * 3 + i] = rf_nan();
        return 0.0;
    }
    double X[3], li[6], gp[3];
    rf_load_point(a, n, X, li, a.move ? gp : nullptr);
    if (a.move) {
        for (int c = 0; c < a.C; ++c) {
            const double s = a.os[(int64_t)c * a.N + n];
            if (s == 0.0) continue;
            RfObs o;
            rf_obs(a.cams + c * CAMW, X, a.ou[(int64_t)c * a.N + n], a.ov[(int64_t)c * a.N + n], s, a.delta, a.outer, o);
            const double *dc = a.dc + c * 6;
            for (int k = 0; k < 2; ++k) {
                double jd = 0.0;                                  // Jc dc of this component
                for (int i = 0; i < 6; ++i) jd += o.Jc[k][i] * dc[i];
                for (int j = 0; j < 3; ++j) gp[j] += o.h[k] * o.Jx[k][j] * jd;
            }
        }
        const double q0 = li[0] * gp[0], q1 = li[1] * gp[0] + li[2] * gp[1], q2 = li[3] * gp[0] + li[4] * gp[1] + li[5] * gp[2];
        X[0] -= li[0] * q0 + li[1] * q1 + li[3] * q2;             // L^-T q
        X[1] -= li[2] * q1 + li[4] * q2;
        X[2] -= li[5] * q2;
    }
    for (int i = 0; i < 3; ++i) a.Xt[n * 3 + i] = X[i];
    double cost = 0.0;
    for (int c = 0; c < a.C; ++c) {
        const double s = a.os[(int64_t)c * a.N + n];
        if (s == 0.0) continue;
        const double *cam = a.cams_t + c * CAMW;
        double rx[3], xc[3];
        rf_transform(cam, X, rx, xc);
        if (!(xc[2] > 0.0)) return __builtin_huge_val();           // a trial that puts a point behind a camera is refused
        const double iz = 1.0 / xc[2];
        cost += rf_huber(s * (cam[0] * xc[0] * iz + cam[2] - a.ou[(int64_t)c * a.N + n]), a.delta);
        cost += rf_huber(s * (cam[1] * xc[1] * iz + cam[3] - a.ov[(int64_t)c * a.N + n]), a.delta);
    }
    return cost;
}

// per point and camera, at cams and X: acc = cost, sum s^2 d^2, sum s^2
RF_HD void rf_stats_point(const P2sRfArgs &a, int64_t n, int c, double acc[3]) {
    const double s = a.os[(int64_t)c * a.N + n];
    if (s == 0.0) return;
    const double *cam = a.cams + c * CAMW;
    double X[3], rx[3], xc[3];
    for (int i = 0; i < 3; ++i) X[i] = a.X[n * 3 + i];
    rf_transform(cam, X, rx, xc);
    const double iz = 1.0 / xc[2];
    const double du = cam[0] * xc[0] * iz + cam[2] - a.ou[(int64_t)c * a.N + n], dv = cam[1] * xc[1] * iz + cam[3] - a.ov[(int64_t)c * a.N + n];
    acc[0] += rf_huber(s * du, a.delta) + rf_huber(s * dv, a.delta);
    acc[1] += s * s * (du * du + dv * dv);
    acc[2] += s * s;
}

// ---- the passes and the kernels ----------------------------------------------------------------------------------------
struct RfBlocks : P2sPassAll {                                     // row y: rf_row; the host's form of rf_blocks_kernel
    RF_HD static void point(const P2sRfArgs &a, int y, int64_t n, double *acc) {
        int ca, cb;
        rf_row(a.C, y, ca, cb);
        if (cb >= 0) rf_pair_point(a, n, ca, cb, acc);
        else rf_cam_point(a, n, ca, acc);
    }
};
struct RfStep : P2sPassAll {                                       // one row
    RF_HD static void point(const P2sRfArgs &a, int, int64_t n, double *acc) { acc[0] += rf_step_point(a, n); }
};
struct RfStats : P2sPassAll {                                      // row c: a camera
    RF_HD static void point(const P2sRfArgs &a, int c, int64_t n, double *acc) { rf_stats_point(a, n, c, acc); }
};

struct RfPrepArgs {
    const void *xyl;
    const double *X0, *cams;
    double *ou, *ov, *os, *Xw;
    uint8_t *kept;
    unsigned int *cam_count;              // [C] kept observations of every camera
    unsigned long long *counters;         // kept points; the first (point * C + camera) behind its camera
    int64_t N;
    int32_t C, min_cams;
    double lik_thr;
};

template <typename T> __global__ void __launch_bounds__(TILE) rf_prep_kernel(const RfPrepArgs p) {
    __shared__ unsigned int cnt[P2S_MAX_CAMS + 1];
    const int tid = threadIdx.x;
    if (tid <= P2S_MAX_CAMS) cnt[tid] = 0;
    __syncthreads();
    const int64_t n = (int64_t)blockIdx.x * TILE + tid;
    if (n < p.N) {
        int behind;
        const uint32_t seen = rf_prep_point((const T *)p.xyl, p.X0, p.cams, p.lik_thr, p.min_cams, p.N, p.C, n, p.ou, p.ov, p.os, p.kept,
                                            p.Xw, &behind);
        for (int c = 0; c < p.C; ++c)
            if (seen >> c & 1) atomicAdd(&cnt[c], 1u);
        if (seen) atomicAdd(&cnt[P2S_MAX_CAMS], 1u);
        if (behind >= 0) atomicMin(&p.counters[1], (unsigned long long)(n * p.C + behind));
    }
    __syncthreads();
    if (tid < p.C && cnt[tid]) atomicAdd(&p.cam_count[tid], cnt[tid]);
    if (tid == P2S_MAX_CAMS && cnt[tid]) atomicAdd(&p.counters[0], (unsigned long long)cnt[tid]);
}

__global__ void __launch_bounds__(TILE) rf_point_kernel(const P2sRfArgs a) {
    const int64_t n = (int64_t)blockIdx.x * TILE + threadIdx.x;
    if (n < a.N) rf_point_build(a, n);
}

// RfBlocks with rf_row ahead of the points, written out: at the register limit (256 VGPRs, no scratch) any function between
// this body and the two per-point functions, p2s_pass_kernel<NACC, TILE, RfBlocks> included, is allocated otherwise.
__global__ void __launch_bounds__(TILE) rf_blocks_kernel(const P2sRfArgs a) {
    __shared__ double lds[(TILE / 64) * NACC];
    int ca, cb;
    rf_row(a.C, blockIdx.y, ca, cb);
    double acc[NACC];
    for (int i = 0; i < NACC; ++i) acc[i] = 0.0;
    for (int64_t t = blockIdx.x; t < a.tiles; t += a.parts) {      // uniform trip count
        const int64_t n = t * TILE + threadIdx.x;
        if (n >= a.N) continue;
        if (cb >= 0) rf_pair_point(a, n, ca, cb, acc);
        else rf_cam_point(a, n, ca, acc);
    }
    p2s_block_sum<NACC, TILE>(acc, lds, a.partials + (int64_t)blockIdx.y * NACC * a.parts + blockIdx.x, a.parts);
}

// ---- the driver ---------------------------------------------------------------------------------------------------------------
struct RfRun {
    p2s_ctx *ctx;                // NULL: on the host
    const Block *block;
    P2sRfArgs a;
    std::vector<double> sums;    // the host's copy of a.sums
    int rows() const { return a.C * (a.C + 1) / 2 + a.C; }

    // sums [width] of the pass that a.partials holds
    int fetch(size_t width) {
        if (!ctx) {
            p2s_sum_parts(a.partials, width, a.parts, sums.data());
            return P2S_OK;
        }
        hipLaunchKernelGGL(rf_sum_kernel, dim3((unsigned)width), dim3(64), 0, ctx->stream, a.partials, a.sums, a.parts);
        HIP_TRY(hipGetLastError());
        P2S_TRY(block->get(sums.data(), a.sums, width * 8));
        return block->wait();
    }
    // sums [rows][36]: the Schur blocks of the camera pairs, then U, g, W V^-1 gp of the cameras
    int build(double lambda) {
        a.lambda = lambda;
        a.outer = std::min(1.0, std::max(OUTER_CURVATURE, lambda * OUTER_PER_LAMBDA));
        if (ctx) {
            hipLaunchKernelGGL(rf_point_kernel, dim3((unsigned)a.tiles), dim3(TILE), 0, ctx->stream, a);
            hipLaunchKernelGGL(rf_blocks_kernel, dim3((unsigned)a.parts, (unsigned)rows()), dim3(TILE), 0, ctx->stream, a);
        } else {
            for (int64_t n = 0; n < a.N; ++n) rf_point_build(a, n);
            p2s_pass_host<NACC, TILE, RfBlocks>(a, rows());
        }
        return fetch((size_t)rows() * NACC);
    }
    // The trial (move: X + dX at cams_t; else X itself): Xt and its cost.
    int step(int move, double *cost) {
        a.move = move;
        P2S_TRY((p2s_pass<1, TILE, RfStep>(ctx, a, 1)));
        P2S_TRY(fetch(1));
        *cost = sums[0];
        return P2S_OK;
    }
    // sums [C][3] at a.cams and a.X
    int stats() {
        P2S_TRY((p2s_pass<3, TILE, RfStats>(ctx, a, a.C)));
        return fetch((size_t)a.C * 3);
    }
};

// In-place Cholesky solve of the n x n system A x = b (row-major, lower triangle used); false: not positive definite.
bool rf_cholesky_solve(std::vector<double> &A, std::vector<double> &b, int n) {
    for (int j = 0; j < n; ++j) {
        double d = A[(size_t)j * n + j];
        for (int k = 0; k < j; ++k) d -= A[(size_t)j * n + k] * A[(size_t)j * n + k];
        if (!(d > 0.0) || !std::isfinite(d)) return false;
        d = sqrt(d);
        A[(size_t)j * n + j] = d;
        for (int i = j + 1; i < n; ++i) {
            double s = A[(size_t)i * n + j];
            for (int k = 0; k < j; ++k) s -= A[(size_t)i * n + k] * A[(size_t)j * n + k];
            A[(size_t)i * n + j] = s / d;
        }
    }
    for (int i = 0; i < n; ++i) {
        double s = b[i];
        for (int k = 0; k < i; ++k) s -= A[(size_t)i * n + k] * b[k];
        b[i] = s / A[(size_t)i * n + i];
    }
    for (int i = n - 1; i >= 0; --i) {
        double s = b[i];
        for (int k = i + 1; k < n; ++k) s -= A[(size_t)k * n + i] * b[k];
        b[i] = s / A[(size_t)i * n + i];
    }
    for (int i = 0; i < n; ++i)
        if (!std::isfinite(b[i])) return false;
    return true;
}

// The reduced system of a build (sums) at `lambda`, restricted to the free parameters, solved: dc [C][6].
bool rf_solve_cameras(const std::vector<double> &sums, int C, double lambda, const std::vector<int> &free_idx, std::vector<double> &dc) {
    const int n6 = 6 * C, pairs = C * (C + 1) / 2, nf = (int)free_idx.size();
    std::vector<double> S((size_t)n6 * n6, 0.0), rhs(n6, 0.0);
    int y = 0;
    for (int ca = 0; ca < C; ++ca)
        for (int cb = ca; cb < C; ++cb, ++y) {
            const double *B = &sums[(size_t)y * NACC];
            for (int i = 0; i < 6; ++i)
                for (int j = 0; j < 6; ++j) {
                    S[(size_t)(6 * ca + i) * n6 + 6 * cb + j] -= B[i * 6 + j];
                    if (cb != ca) S[(size_t)(6 * cb + j) * n6 + 6 * ca + i] -= B[i * 6 + j];
                }
        }
    for (int c = 0; c < C; ++c) {
        const double *D = &sums[(size_t)(pairs + c) * NACC];
        int k = 0;
        for (int i = 0; i < 6; ++i)
            for (int j = i; j < 6; ++j, ++k) {
                const double u = i == j ? D[k] * (1.0 + lambda) : D[k];
                S[(size_t)(6 * c + i) * n6 + 6 * c + j] += u;
                if (j != i) S[(size_t)(6 * c + j) * n6 + 6 * c + i] += u;
            }
        for (int i = 0; i < 6; ++i) rhs[6 * c + i] = -(D[21 + i] - D[27 + i]);
    }
    std::vector<double> A((size_t)nf * nf), b(nf);
    for (int i = 0; i < nf; ++i) {
        b[i] = rhs[free_idx[i]];
        for (int j = 0; j < nf; ++j) A[(size_t)i * nf + j] = S[(size_t)free_idx[i] * n6 + free_idx[j]];
    }
    if (!rf_cholesky_solve(A, b, nf)) return false;
    std::fill(dc.begin(), dc.end(), 0.0);
    for (int i = 0; i < nf; ++i) dc[free_idx[i]] = b[i];
    return true;
}

// cam_t = the camera `cam` after the step d = (dw, dt): R <- exp([dw]x) R, t <- t + dt.
void rf_move_camera(const double *cam, const double *d, double *cam_t) {
    memcpy(cam_t, cam, CAMW * 8);
    const double th2 = d[0] * d[0] + d[1] * d[1] + d[2] * d[2], th = sqrt(th2);
    double A = 1.0, B = 0.5;                                       // sin(th) / th, (1 - cos(th)) / th^2
    if (th > 1e-8) {
        A = sin(th) / th;
        B = (1.0 - cos(th)) / th2;
    }
    const double K[9] = {0.0, -d[2], d[1], d[2], 0.0, -d[0], -d[1], d[0], 0.0};
    double E[9];
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) {
            double k2 = 0.0;
            for (int m = 0; m < 3; ++m) k2 += K[i * 3 + m] * K[m * 3 + j];
            E[i * 3 + j] = (i == j ? 1.0 : 0.0) + A * K[i * 3 + j] + B * k2;
        }
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) {
            double s = 0.0;
            for (int m = 0; m < 3; ++m) s += E[i * 3 + m] * cam[4 + m * 3 + j];
            cam_t[4 + i * 3 + j] = s;
        }
    for (int i = 0; i < 3; ++i) cam_t[13 + i] = cam[13 + i] + d[3 + i];
}

// The coordinate of camera 1's translation that is held: the largest of the baseline in camera 1's frame.
int rf_held_coord(const double *R, const double *t) {
    double c0[3], b[3];
    for (int i = 0; i < 3; ++i) c0[i] = R[i] * t[0] + R[3 + i] * t[1] + R[6 + i] * t[2];              // R0^T t0
    for (int i = 0; i < 3; ++i) b[i] = t[3 + i] - (R[9 + 3 * i] * c0[0] + R[9 + 3 * i + 1] * c0[1] + R[9 + 3 * i + 2] * c0[2]);
    int j = 0;
    for (int i = 1; i < 3; ++i)
        if (fabs(b[i]) > fabs(b[j])) j = i;
    return j;
}

void rf_rms(const std::vector<double> &sums, int C, double *rms) {
    for (int c = 0; c < C; ++c) rms[c] = sqrt(sums[(size_t)c * 3 + 1] / sums[(size_t)c * 3 + 2]);
}

}  // namespace

// ---- C-ABI entry points (include/p2s.h) ----------------------------------------------------------------------------
extern "C" {

int p2s_refine_held_coord(const double *R_in, const double *t_in, int32_t *held) {
    if (!R_in || !t_in || !held) return p2s_set_error(P2S_ERR_INVALID_ARG, "null argument");
    for (int i = 0; i < 18; ++i)
        if (!std::isfinite(R_in[i])) return p2s_set_error(P2S_ERR_INVALID_ARG, "R of cameras 0 and 1 must be finite");
    for (int i = 0; i < 6; ++i)
        if (!std::isfinite(t_in[i])) return p2s_set_error(P2S_ERR_INVALID_ARG, "t of cameras 0 and 1 must be finite");
    *held = rf_held_coord(R_in, t_in);
    return P2S_OK;
}

int p2s_refine_extrinsics_host(p2s_ctx *ctx, int64_t n_points, int32_t n_cams, int32_t dtype, const void *xyl, const double *Kmats,
                               const double *R_in, const double *t_in, const double *X0, const p2s_refine_params *params,
                               double *R_out, double *t_out, double *X_out, p2s_refine_report *report) {
    if (n_cams < 2 || n_cams > P2S_MAX_CAMS) return p2s_set_error(P2S_ERR_INVALID_ARG, "n_cams=%d outside [2, %d]", n_cams, P2S_MAX_CAMS);
    if (n_points < 1 || n_points >= ((int64_t)1 << 31) / P2S_MAX_CAMS)
        return p2s_set_error(P2S_ERR_INVALID_ARG, "n_points=%lld outside [1, %lld)", (long long)n_points, (long long)(((int64_t)1 << 31) / P2S_MAX_CAMS));
    if (dtype != P2S_F32 && dtype != P2S_F64) return p2s_set_error(P2S_ERR_INVALID_ARG, "dtype=%d is neither P2S_F32 nor P2S_F64", dtype);
    if (!xyl || !Kmats || !R_in || !t_in || !X0 || !params || !R_out || !t_out || !X_out || !report)
        return p2s_set_error(P2S_ERR_INVALID_ARG, "null argument");
    if (!(params->huber_px > 0.0) || !std::isfinite(params->huber_px) || !std::isfinite(params->lik_thr) || !(params->ftol >= 0.0) ||
        params->max_iter < 0)
        return p2s_set_error(P2S_ERR_INVALID_ARG, "huber_px must be positive, lik_thr finite, ftol and max_iter not negative");
    const int C = n_cams, min_cams = std::max(params->min_cams, 2);
    const size_t N = (size_t)n_points;
    std::vector<double> cams((size_t)C * CAMW), cams_t((size_t)C * CAMW), dc((size_t)C * 6, 0.0);
    for (int c = 0; c < C; ++c) {
        const double *K = Kmats + c * 9;
        for (int i = 0; i < 9; ++i)
            if (!std::isfinite(K[i]) || !std::isfinite(R_in[c * 9 + i]))
                return p2s_set_error(P2S_ERR_INVALID_ARG, "camera %d: K and R must be finite", c);
        for (int i = 0; i < 3; ++i)
            if (!std::isfinite(t_in[c * 3 + i])) return p2s_set_error(P2S_ERR_INVALID_ARG, "camera %d: t must be finite", c);
        double *cam = &cams[(size_t)c * CAMW];
        cam[0] = K[0]; cam[1] = K[4]; cam[2] = K[2]; cam[3] = K[5];
        memcpy(cam + 4, R_in + c * 9, 72);
        memcpy(cam + 13, t_in + c * 3, 24);
    }
    const int held = rf_held_coord(R_in, t_in);
    std::vector<int> free_idx;
    for (int c = 1; c < C; ++c)
        for (int k = 0; k < 6; ++k)
            if (!(c == 1 && k == 3 + held)) free_idx.push_back(6 * c + k);

    Block block{Stage{ctx}};
    RfRun run{ctx, &block, {}, {}};
    P2sRfArgs &a = run.a;
    a.N = n_points; a.C = C; a.delta = params->huber_px;
    a.tiles = (int32_t)((n_points + TILE - 1) / TILE);
    a.parts = std::min<int32_t>(a.tiles, MAX_PARTS);
    const size_t rows = (size_t)run.rows(), width = rows * NACC;
    run.sums.assign(width, 0.0);
    Layout lay;                                                   // one block: the small tables first
    const size_t o_cams = lay.add((size_t)C * CAMW * 8), o_camst = lay.add((size_t)C * CAMW * 8), o_dc = lay.add((size_t)C * 6 * 8),
                 o_count = lay.add(P2S_MAX_CAMS * 4), o_ctr = lay.add(16), o_sums = lay.add(width * 8),
                 o_parts = lay.add(width * (size_t)a.parts * 8), o_kept = lay.add(N), o_ou = lay.add(N * C * 8), o_ov = lay.add(N * C * 8),
                 o_os = lay.add(N * C * 8), o_x = lay.add(N * 24), o_xt = lay.add(N * 24), o_pt = lay.add(N * 72), o_x0 = lay.add(N * 24);
    const void *d_xyl = xyl;
    unsigned int cam_count[P2S_MAX_CAMS] = {};
    unsigned long long counters[2] = {0, ~0ull};
    if (ctx) {
        HIP_TRY(hipSetDevice(ctx->device));
        P2S_TRY(block.st.upload(d_xyl, xyl, N * C * 3 * (dtype == P2S_F32 ? 4 : 8)));
    }
    P2S_TRY(block.alloc(lay.bytes));
    char *blk = block.p;
    P2S_TRY(block.put(blk + o_x0, X0, N * 24));
    P2S_TRY(block.put(blk + o_cams, cams.data(), cams.size() * 8));
    P2S_TRY(block.put(blk + o_camst, cams.data(), cams.size() * 8));
    P2S_TRY(block.put(blk + o_dc, dc.data(), dc.size() * 8));
    P2S_TRY(block.put(blk + o_count, cam_count, sizeof cam_count));
    P2S_TRY(block.put(blk + o_ctr, counters, sizeof counters));
    double *d_cams[2] = {(double *)(blk + o_cams), (double *)(blk + o_camst)}, *d_X[2] = {(double *)(blk + o_x), (double *)(blk + o_xt)};
    double *d_dc = (double *)(blk + o_dc);
    a.ou = (double *)(blk + o_ou); a.ov = (double *)(blk + o_ov); a.os = (double *)(blk + o_os); a.kept = (uint8_t *)(blk + o_kept);
    a.pt = (double *)(blk + o_pt); a.dc = d_dc; a.partials = (double *)(blk + o_parts); a.sums = (double *)(blk + o_sums);
    RfPrepArgs p{d_xyl, (const double *)(blk + o_x0), d_cams[0], (double *)a.ou, (double *)a.ov, (double *)a.os, d_X[0], (uint8_t *)a.kept,
                 (unsigned int *)(blk + o_count), (unsigned long long *)(blk + o_ctr), n_points, C, min_cams, params->lik_thr};
    P2S_TRY(block.time_begin());
    if (ctx) {
        if (dtype == P2S_F32) hipLaunchKernelGGL(rf_prep_kernel<float>, dim3((unsigned)a.tiles), dim3(TILE), 0, ctx->stream, p);
        else hipLaunchKernelGGL(rf_prep_kernel<double>, dim3((unsigned)a.tiles), dim3(TILE), 0, ctx->stream, p);
        HIP_TRY(hipGetLastError());
        P2S_TRY(block.get(cam_count, p.cam_count, sizeof cam_count));
        P2S_TRY(block.get(counters, p.counters, sizeof counters));
        P2S_TRY(block.wait());
    } else {
        for (int64_t n = 0; n < n_points; ++n) {
            int behind;
            const uint32_t seen = dtype == P2S_F32
                ? rf_prep_point((const float *)xyl, p.X0, p.cams, p.lik_thr, min_cams, n_points, C, n, p.ou, p.ov, p.os, p.kept, p.Xw, &behind)
                : rf_prep_point((const double *)xyl, p.X0, p.cams, p.lik_thr, min_cams, n_points, C, n, p.ou, p.ov, p.os, p.kept, p.Xw, &behind);
            for (int c = 0; c < C; ++c) cam_count[c] += seen >> c & 1;
            counters[0] += seen != 0;
            if (behind >= 0) counters[1] = std::min(counters[1], (unsigned long long)(n * C + behind));
        }
    }
    if (counters[0] == 0) return p2s_set_error(P2S_ERR_INVALID_ARG, "no kept point: none of the %lld points has %d observations and a finite start", (long long)n_points, min_cams);
    for (int c = 0; c < C; ++c)
        if (cam_count[c] == 0) return p2s_set_error(P2S_ERR_INVALID_ARG, "camera %d has no kept observation", c);
    if (counters[1] != ~0ull)
        return p2s_set_error(P2S_ERR_INVALID_ARG, "point %lld lies behind camera %d at entry", (long long)(counters[1] / C), (int)(counters[1] % C));

    // the cost and the report's RMS at the input
    p2s_refine_report rep;
    memset(&rep, 0, sizeof rep);
    rep.kept_points = (int64_t)counters[0];
    rep.held_coord = held;
    int cur = 0, xcur = 0;                                        // which of d_cams / d_X holds the accepted state
    a.cams = a.cams_t = d_cams[0]; a.X = d_X[0]; a.Xt = d_X[1];
    double cost;
    P2S_TRY(run.step(0, &cost));
    P2S_TRY(run.stats());
    rf_rms(run.sums, C, rep.rms_before);
    rep.cost_before = cost;
    double lambda = 1e-3;
    while (rep.iterations < params->max_iter && cost > 0.0) {
        ++rep.iterations;
        a.cams = d_cams[cur]; a.cams_t = d_cams[cur ^ 1]; a.X = d_X[xcur]; a.Xt = d_X[xcur ^ 1];
        P2S_TRY(run.build(lambda));
        double trial = __builtin_huge_val();
        if (rf_solve_cameras(run.sums, C, lambda, free_idx, dc)) {
            for (int c = 0; c < C; ++c) rf_move_camera(&cams[(size_t)c * CAMW], &dc[(size_t)c * 6], &cams_t[(size_t)c * CAMW]);
            P2S_TRY(block.put_wait(d_dc, dc.data(), dc.size() * 8));
            P2S_TRY(block.put_wait(d_cams[cur ^ 1], cams_t.data(), cams_t.size() * 8));
            P2S_TRY(run.step(1, &trial));
        }
        if (trial < cost) {
            const double rel = (cost - trial) / cost;
            cost = trial;
            cams.swap(cams_t);
            cur ^= 1;
            xcur ^= 1;
            ++rep.accepted;
            lambda = std::max(lambda / 10.0, 1e-9);
            if (rel < params->ftol) break;
        } else {
            if (trial - cost <= params->ftol * cost) break;           // the minimum to rounding: no trial can tell a decrease
            lambda *= 10.0;
            if (lambda > 1e12) break;
        }
    }
    rep.cost_after = cost;
    rep.lambda_final = lambda;
    a.cams = a.cams_t = d_cams[cur]; a.X = d_X[xcur]; a.Xt = d_X[xcur ^ 1];
    P2S_TRY(run.stats());
    rf_rms(run.sums, C, rep.rms_after);
    P2S_TRY(block.time_end());
    P2S_TRY(block.get(X_out, d_X[xcur], N * 24));
    P2S_TRY(block.finish(P2S_TIMED_REFINE));
    for (int c = 0; c < C; ++c) {
        memcpy(R_out + c * 9, &cams[(size_t)c * CAMW + 4], 72);
        memcpy(t_out + c * 3, &cams[(size_t)c * CAMW + 13], 24);
    }
    *report = rep;
    return P2S_OK;
}

int p2s_refine_kernel_ms(p2s_ctx *ctx, float *elapsed_ms) { return p2s_kernel_ms_query(ctx, P2S_TIMED_REFINE, "p2s_refine_extrinsics_host", elapsed_ms); }

}  // extern "C"
