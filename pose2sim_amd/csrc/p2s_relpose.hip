// p2s_relpose.hip -- the relative pose of every camera pair out of contaminated correspondences: normalised m-point
// hypotheses of the essential matrix, MSAC scoring by the Sampson distance, refits on the winner's inliers that are kept
// while the cost falls, and the cheirality count of the four (R, t) of the result (include/p2s.h).  fp64
// throughout.
//
//   rp_hyp_kernel     one lane per (pair, hypothesis): the 9 x 9 normal matrix of its sample, the eigenvector of its
//                     smallest eigenvalue by cyclic Jacobi (the triangle and the eigenvectors in LDS, 126 doubles a lane,
//                     lane-interleaved: no bank conflict, no scratch), the 3 x 3 projection to an essential matrix by a
//                     one-sided Jacobi in registers
//   rp_score_kernel   the hot path, per (pair, 256 hypotheses, chunk of points): a lane keeps its hypothesis' nine doubles
//                     in registers, the workgroup streams the pair's points through LDS, 256 at a time, every lane reads
//                     the same point (a broadcast); P x H x N Sampson distances
//   rp_winner_kernel  per pair: the chunk sums of every hypothesis added in order, the lowest cost (lowest index on ties)
//   RpStat            a pass of p2s_passes.h, per (pair, part of the points), one lane a point, the pair's current E: cost,
//                     inliers and the inliers' moments;  RpNormal: the 45 sums of the inliers' normal matrix; both leave
//                     out the pairs that are not active
//   rp_front_kernel   the inlier mask and, per (R, t) candidate, the inliers in front of both cameras
//
// No floating-point atomic anywhere: a lane adds its points in order, a wave its lanes by the xor butterfly, a workgroup its
// waves in order (p2s_block_sum), the host the parts (and rp_winner_kernel the chunks) in order; counts are integers.  Two
// runs agree bit for bit.  The 9 x 9 eigen-solves of the refits and the decompositions run on the host between the
// launches, with the functions the kernels use.  ctx == NULL runs the same per-hypothesis and per-point functions on the
// host (the passes as p2s_pass_host), in a Block of the host's memory.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include <string.h>

#include <algorithm>
#include <vector>

#include "p2s_ctx.h"
#include "p2s_passes.h"

#define RP_HD __host__ __device__ inline

namespace {

constexpr int TILE = P2S_RELPOSE_TILE;             // points of a pass through LDS, lanes of a workgroup
constexpr int MAX_CHUNKS = P2S_RELPOSE_MAX_CHUNKS; // cuts of a pair's points in rp_score_kernel
constexpr int MAX_PARTS = P2S_RELPOSE_MAX_PARTS;   // workgroups along the points in the per-point kernels
constexpr int MIN_M = P2S_RELPOSE_MIN_SAMPLE, MAX_M = P2S_RELPOSE_MAX_SAMPLE;
constexpr int NSYM = 45, NWORK = NSYM + 81;        // the triangle of M, then its eigenvectors
constexpr int HYP_LANES = 64;                      // one wave a workgroup: 126 x 64 doubles are 63 KB of LDS
constexpr int NSTAT = 8;                           // cost, inliers, sum xa ya |a|^2, sum xb yb |b|^2
constexpr int FILL_BLOCKS = 1024;                  // workgroups that fill the GPU: 4 a CU

// Element i of a lane's work array: i * stride (stride = lanes of the workgroup in LDS, 1 on the host).
struct RpMem {
    double *p;
    int stride;
    RP_HD double &operator[](int i) const { return p[i * stride]; }
};

RP_HD double rp_nan() { return __builtin_nan(""); }
RP_HD bool rp_finite(double v) { return fabs(v) < __builtin_huge_val(); }
RP_HD int rp_sym(int i, int j) {                    // the triangle i <= j of a 9 x 9 matrix, row after row
    if (i > j) {
        const int k = i;
        i = j;
        j = k;
    }
    return i * 9 - i * (i - 1) / 2 + j - i;
}

// The eigenvector of the smallest eigenvalue (first index on ties) of the symmetric 9 x 9 matrix in w[0 .. 45) by cyclic
// Jacobi; w[45 .. 126) holds the eigenvectors.  -> second smallest over largest eigenvalue (the conditioning of f).
RP_HD double rp_eig_smallest(const RpMem w, double f[9]) {
    for (int i = 0; i < 9; ++i)
        for (int j = 0; j < 9; ++j) w[NSYM + i * 9 + j] = i == j ? 1.0 : 0.0;
    for (int sweep = 0; sweep < 16; ++sweep) {
        double off = 0.0, diag = 0.0;
        for (int i = 0; i < 9; ++i)
            for (int j = i; j < 9; ++j) {
                const double v = w[rp_sym(i, j)];
                if (i == j) diag += v * v;
                else off += v * v;
            }
        if (!(off > 1e-36 * diag)) break;
        for (int p = 0; p < 8; ++p)
            for (int q = p + 1; q < 9; ++q) {
                const double apq = w[rp_sym(p, q)];
                if (apq == 0.0) continue;
                const double app = w[rp_sym(p, p)], aqq = w[rp_sym(q, q)];
                const double theta = (aqq - app) / (2.0 * apq);
                const double t = (theta >= 0.0 ? 1.0 : -1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));
                const double c = 1.0 / sqrt(t * t + 1.0), s = t * c;
                for (int k = 0; k < 9; ++k) {
                    if (k != p && k != q) {
                        const int ikp = rp_sym(k, p), ikq = rp_sym(k, q);
                        const double akp = w[ikp], akq = w[ikq];
                        w[ikp] = c * akp - s * akq;
                        w[ikq] = s * akp + c * akq;
                    }
                    const double vkp = w[NSYM + k * 9 + p], vkq = w[NSYM + k * 9 + q];
                    w[NSYM + k * 9 + p] = c * vkp - s * vkq;
                    w[NSYM + k * 9 + q] = s * vkp + c * vkq;
                }
                w[rp_sym(p, p)] = app - t * apq;
                w[rp_sym(q, q)] = aqq + t * apq;
                w[rp_sym(p, q)] = 0.0;
            }
    }
    int k0 = 0;
    for (int i = 1; i < 9; ++i)
        if (w[rp_sym(i, i)] < w[rp_sym(k0, k0)]) k0 = i;
    double second = __builtin_huge_val(), largest = 0.0;
    for (int i = 0; i < 9; ++i) {
        const double v = w[rp_sym(i, i)];
        if (i != k0 && v < second) second = v;
        if (v > largest) largest = v;
    }
    for (int i = 0; i < 9; ++i) f[i] = w[NSYM + i * 9 + k0];
    return second / largest;
}

// The one-sided Jacobi SVD of the 3 x 3 matrix F (row-major) in registers: the columns of G = F V are rotated until they are
// orthogonal.  On return they are u_i sigma_i and the columns of V the v_i; -> the index of the smallest singular value.
RP_HD int rp_svd3(const double F[9], double G[9], double V[9], double sig[3]) {
    for (int i = 0; i < 9; ++i) {
        G[i] = F[i];
        V[i] = i % 4 == 0 ? 1.0 : 0.0;
    }
    for (int sweep = 0; sweep < 30; ++sweep) {
        bool moved = false;
#pragma unroll
        for (int pq = 0; pq < 3; ++pq) {
            const int p = pq == 2 ? 1 : 0, q = pq == 0 ? 1 : 2;
            const double alpha = G[p] * G[p] + G[3 + p] * G[3 + p] + G[6 + p] * G[6 + p];
            const double beta = G[q] * G[q] + G[3 + q] * G[3 + q] + G[6 + q] * G[6 + q];
            const double gamma = G[p] * G[q] + G[3 + p] * G[3 + q] + G[6 + p] * G[6 + q];
            if (!(gamma * gamma > 1e-34 * alpha * beta)) continue;
            moved = true;
            const double zeta = (beta - alpha) / (2.0 * gamma);
            const double t = (zeta >= 0.0 ? 1.0 : -1.0) / (fabs(zeta) + sqrt(zeta * zeta + 1.0));
            const double c = 1.0 / sqrt(t * t + 1.0), s = t * c;
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                const double gp = G[3 * k + p], gq = G[3 * k + q];
                G[3 * k + p] = c * gp - s * gq;
                G[3 * k + q] = s * gp + c * gq;
                const double vp = V[3 * k + p], vq = V[3 * k + q];
                V[3 * k + p] = c * vp - s * vq;
                V[3 * k + q] = s * vp + c * vq;
            }
        }
        if (!moved) break;
    }
    int k3 = 0;
#pragma unroll
    for (int i = 0; i < 3; ++i) sig[i] = sqrt(G[i] * G[i] + G[3 + i] * G[3 + i] + G[6 + i] * G[6 + i]);
    if (sig[1] < sig[k3]) k3 = 1;
    if (sig[2] < sig[k3]) k3 = 2;
    return k3;
}

// E = u1 v1^T + u2 v2^T of F's two largest singular values; NaN when F has no two, or is not finite.
RP_HD void rp_project(const double F[9], double E[9]) {
    double G[9], V[9], sig[3];
    const int k3 = rp_svd3(F, G, V, sig);
    const int i1 = k3 == 0 ? 1 : 0, i2 = k3 == 2 ? 1 : 2;
    const double r1 = 1.0 / sig[i1], r2 = 1.0 / sig[i2];
    const bool ok = rp_finite(r1) && rp_finite(r2) && rp_finite(sig[0] + sig[1] + sig[2]);
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) E[3 * i + j] = ok ? G[3 * i + i1] * r1 * V[3 * j + i1] + G[3 * i + i2] * r2 * V[3 * j + i2] : rp_nan();
}

// F = Tb^T F' Ta for the normalisations x' = s (x - c) of both sides (nrm = sa cax cay sb cbx cby), then the projection.
RP_HD void rp_denormalise_project(const double f[9], const double nrm[6], double E[9]) {
    const double sa = nrm[0], ax = nrm[1], ay = nrm[2], sb = nrm[3], bx = nrm[4], by = nrm[5];
    double H[9], F[9];                                             // H = F' Ta
    for (int i = 0; i < 3; ++i) {
        H[3 * i] = f[3 * i] * sa;
        H[3 * i + 1] = f[3 * i + 1] * sa;
        H[3 * i + 2] = f[3 * i + 2] - sa * (f[3 * i] * ax + f[3 * i + 1] * ay);
    }
    for (int j = 0; j < 3; ++j) {
        F[j] = sb * H[j];
        F[3 + j] = sb * H[3 + j];
        F[6 + j] = H[6 + j] - sb * (bx * H[j] + by * H[3 + j]);
    }
    rp_project(F, E);
}

// w[0 .. 45) += a a^T, a = (xb', yb', 1) x (xa', ya', 1) of one normalised correspondence.
RP_HD void rp_add_row(const RpMem w, double xa, double ya, double xb, double yb) {
    const double a[9] = {xb * xa, xb * ya, xb, yb * xa, yb * ya, yb, xa, ya, 1.0};
    int k = 0;
#pragma unroll
    for (int i = 0; i < 9; ++i)
#pragma unroll
        for (int j = i; j < 9; ++j, ++k) w[k] += a[i] * a[j];
}

struct RpArgs {
    const double *xn;            // [C][N][2]
    const uint8_t *ok;           // [C][N] usable and finite
    const int32_t *pairs;        // [P][2]
    const int32_t *samples;      // [P][H][m]
    const double *thr2;          // [P]
    double *hypE;                // [P][H][9]
    const int32_t *list;         // [P][S] the points the hypotheses are scored on, or NULL: every point
    const int32_t *n_list;       // [P]
    double *part_cost;           // [P][H][chunks]
    int32_t *part_inl;
    double *hyp_cost;            // [P][H]
    int32_t *hyp_inl;
    int32_t *winner;             // [P]
    double *winE;                // [P][9] the winners' E, NaN without one: where E points until the first refit
    const double *E;             // [P][9] of the per-point kernels
    const uint8_t *active;       // [P]
    const double *nrm;           // [P][6]
    const double *cand;          // [P][4][12] R, t
    double *partials;            // [P][W][parts]
    uint32_t *front;             // [P][4]
    uint8_t *mask;               // [P][N]
    int64_t N;
    int32_t P, H, m, S, chunks, tiles_per_chunk, tiles, parts;
};

// ---- one hypothesis ---------------------------------------------------------------------------------------------------------
RP_HD void rp_hypothesis(const RpArgs &a, int p, int h, const RpMem w) {
    double *E = a.hypE + ((int64_t)p * a.H + h) * 9;
    const int ca = a.pairs[2 * p], cb = a.pairs[2 * p + 1], m = a.m;
    const int32_t *smp = a.samples + ((int64_t)p * a.H + h) * m;
    const double *xa = a.xn + (int64_t)ca * a.N * 2, *xb = a.xn + (int64_t)cb * a.N * 2;
    const uint8_t *oka = a.ok + (int64_t)ca * a.N, *okb = a.ok + (int64_t)cb * a.N;
    bool good = true;
    for (int i = 0; i < m; ++i) {
        const int64_t n = smp[i];
        if (n < 0 || n >= a.N || !oka[n] || !okb[n]) {
            good = false;
            break;
        }
        for (int j = 0; j < i; ++j)
            if (smp[j] == smp[i]) good = false;
    }
    if (!good) {
        for (int i = 0; i < 9; ++i) E[i] = rp_nan();
        return;
    }
    double nrm[6] = {0, 0, 0, 0, 0, 0};
    for (int i = 0; i < m; ++i) {
        const int64_t n = smp[i];
        nrm[1] += xa[2 * n]; nrm[2] += xa[2 * n + 1]; nrm[4] += xb[2 * n]; nrm[5] += xb[2 * n + 1];
    }
    nrm[1] /= m; nrm[2] /= m; nrm[4] /= m; nrm[5] /= m;
    for (int i = 0; i < m; ++i) {
        const int64_t n = smp[i];
        const double ax = xa[2 * n] - nrm[1], ay = xa[2 * n + 1] - nrm[2], bx = xb[2 * n] - nrm[4], by = xb[2 * n + 1] - nrm[5];
        nrm[0] += ax * ax + ay * ay;
        nrm[3] += bx * bx + by * by;
    }
    nrm[0] = sqrt(2.0 / (nrm[0] / m));
    nrm[3] = sqrt(2.0 / (nrm[3] / m));
    for (int i = 0; i < NSYM; ++i) w[i] = 0.0;
    for (int i = 0; i < m; ++i) {
        const int64_t n = smp[i];
        rp_add_row(w, nrm[0] * (xa[2 * n] - nrm[1]), nrm[0] * (xa[2 * n + 1] - nrm[2]), nrm[3] * (xb[2 * n] - nrm[4]),
                   nrm[3] * (xb[2 * n + 1] - nrm[5]));
    }
    double f[9], Eh[9];
    rp_eig_smallest(w, f);
    rp_denormalise_project(f, nrm, Eh);
    for (int i = 0; i < 9; ++i) E[i] = Eh[i];
}

// ---- the Sampson distance -------------------------------------------------------------------------------------------------
RP_HD double rp_sampson(const double E[9], double xa, double ya, double xb, double yb) {
    const double e0 = E[0] * xa + E[1] * ya + E[2], e1 = E[3] * xa + E[4] * ya + E[5], e2 = E[6] * xa + E[7] * ya + E[8];
    const double num = xb * e0 + yb * e1 + e2;
    const double f0 = E[0] * xb + E[3] * yb + E[6], f1 = E[1] * xb + E[4] * yb + E[7];
    return num * num / (e0 * e0 + e1 * e1 + f0 * f0 + f1 * f1);
}

// min(d, thr2) of a distance that is a number, 0 of one that is not.
RP_HD double rp_msac(double d, double thr2) { return d < thr2 ? d : (d >= thr2 ? thr2 : 0.0); }

RP_HD bool rp_finite9(const double E[9]) {
    double s = 0.0;
    for (int i = 0; i < 9; ++i) s += fabs(E[i]);
    return rp_finite(s);
}

// Point k of the points pair p's hypotheses are scored on: its coordinates, NaN for one that does not count.
RP_HD void rp_score_point(const RpArgs &a, int p, int64_t k, double pt[4]) {
    const int ca = a.pairs[2 * p], cb = a.pairs[2 * p + 1];
    int64_t n = -1;
    if (a.list) {
        if (k < a.n_list[p]) n = a.list[(int64_t)p * a.S + k];
    } else if (k < a.N && a.ok[(int64_t)ca * a.N + k] && a.ok[(int64_t)cb * a.N + k]) {
        n = k;
    }
    if (n < 0) {
        pt[0] = pt[1] = pt[2] = pt[3] = rp_nan();
        return;
    }
    pt[0] = a.xn[((int64_t)ca * a.N + n) * 2];
    pt[1] = a.xn[((int64_t)ca * a.N + n) * 2 + 1];
    pt[2] = a.xn[((int64_t)cb * a.N + n) * 2];
    pt[3] = a.xn[((int64_t)cb * a.N + n) * 2 + 1];
}

// The mutually usable point n of pair p; false for another.
RP_HD bool rp_pair_point(const RpArgs &a, int p, int64_t n, double pt[4]) {
    const int ca = a.pairs[2 * p], cb = a.pairs[2 * p + 1];
    if (!a.ok[(int64_t)ca * a.N + n] || !a.ok[(int64_t)cb * a.N + n]) return false;
    pt[0] = a.xn[((int64_t)ca * a.N + n) * 2];
    pt[1] = a.xn[((int64_t)ca * a.N + n) * 2 + 1];
    pt[2] = a.xn[((int64_t)cb * a.N + n) * 2];
    pt[3] = a.xn[((int64_t)cb * a.N + n) * 2 + 1];
    return true;
}

RP_HD void rp_stat_point(const RpArgs &a, int p, int64_t n, double acc[NSTAT]) {
    double pt[4];
    if (!rp_pair_point(a, p, n, pt)) return;
    const double thr2 = a.thr2[p], d = rp_sampson(a.E + p * 9, pt[0], pt[1], pt[2], pt[3]);
    acc[0] += rp_msac(d, thr2);
    if (d < thr2) {
        acc[1] += 1.0;
        acc[2] += pt[0]; acc[3] += pt[1]; acc[4] += pt[0] * pt[0] + pt[1] * pt[1];
        acc[5] += pt[2]; acc[6] += pt[3]; acc[7] += pt[2] * pt[2] + pt[3] * pt[3];
    }
}

RP_HD void rp_normal_point(const RpArgs &a, int p, int64_t n, double acc[NSYM]) {
    double pt[4];
    if (!rp_pair_point(a, p, n, pt)) return;
    if (!(rp_sampson(a.E + p * 9, pt[0], pt[1], pt[2], pt[3]) < a.thr2[p])) return;
    const double *nrm = a.nrm + p * 6;
    rp_add_row(RpMem{acc, 1}, nrm[0] * (pt[0] - nrm[1]), nrm[0] * (pt[1] - nrm[2]), nrm[3] * (pt[2] - nrm[4]), nrm[3] * (pt[3] - nrm[5]));
}

// Depths of a correspondence in both views for X_b = R X_a + t: z_a from x_b x (z_a R x_a + t) = 0 by least squares,
// z_b the third coordinate of z_a R x_a + t.
RP_HD bool rp_in_front(const double *cand, const double pt[4]) {
    const double *R = cand, *t = cand + 9;
    const double r0 = R[0] * pt[0] + R[1] * pt[1] + R[2], r1 = R[3] * pt[0] + R[4] * pt[1] + R[5], r2 = R[6] * pt[0] + R[7] * pt[1] + R[8];
    const double c0 = pt[3] * r2 - r1, c1 = r0 - pt[2] * r2, c2 = pt[2] * r1 - pt[3] * r0;                   // x_b x R x_a
    const double d0 = pt[3] * t[2] - t[1], d1 = t[0] - pt[2] * t[2], d2 = pt[2] * t[1] - pt[3] * t[0];       // x_b x t
    const double za = -(c0 * d0 + c1 * d1 + c2 * d2) / (c0 * c0 + c1 * c1 + c2 * c2);
    const double zb = za * r2 + t[2];
    return za > 0.0 && zb > 0.0;
}

// -> bit 4: an inlier; bits 0 .. 3: in front of both cameras of candidate i.
RP_HD int rp_front_point(const RpArgs &a, int p, int64_t n) {
    double pt[4];
    if (!a.active[p] || !rp_pair_point(a, p, n, pt)) return 0;
    if (!(rp_sampson(a.E + p * 9, pt[0], pt[1], pt[2], pt[3]) < a.thr2[p])) return 0;
    int bits = 16;
    for (int i = 0; i < 4; ++i)
        if (rp_in_front(a.cand + (p * 4 + i) * 12, pt)) bits |= 1 << i;
    return bits;
}

// ---- kernels ----------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(HYP_LANES) rp_hyp_kernel(const RpArgs a) {
    __shared__ double lds[NWORK * HYP_LANES];
    const int64_t g = (int64_t)blockIdx.x * HYP_LANES + threadIdx.x;
    if (g >= (int64_t)a.P * a.H) return;
    rp_hypothesis(a, (int)(g / a.H), (int)(g % a.H), RpMem{lds + threadIdx.x, HYP_LANES});
}

__global__ void __launch_bounds__(TILE) rp_score_kernel(const RpArgs a) {
    __shared__ double pts[4][TILE];
    const int p = blockIdx.z, chunk = blockIdx.y, h = blockIdx.x * TILE + threadIdx.x;
    const bool mine = h < a.H;
    double E[9];
#pragma unroll
    for (int i = 0; i < 9; ++i) E[i] = mine ? a.hypE[((int64_t)p * a.H + h) * 9 + i] : 0.0;
    const double thr2 = a.thr2[p];
    double cost = 0.0;
    int inl = 0;
    const int t0 = chunk * a.tiles_per_chunk, t1 = min(a.tiles, t0 + a.tiles_per_chunk);
    for (int t = t0; t < t1; ++t) {                                  // uniform over the workgroup
        double pt[4];
        rp_score_point(a, p, (int64_t)t * TILE + threadIdx.x, pt);
        __syncthreads();
#pragma unroll
        for (int i = 0; i < 4; ++i) pts[i][threadIdx.x] = pt[i];
        __syncthreads();
#pragma unroll 4
        for (int j = 0; j < TILE; ++j) {
            const double d = rp_sampson(E, pts[0][j], pts[1][j], pts[2][j], pts[3][j]);
            cost += rp_msac(d, thr2);
            inl += d < thr2;
        }
    }
    if (!mine) return;
    if (!rp_finite9(E)) {
        cost = __builtin_huge_val();
        inl = 0;
    }
    a.part_cost[((int64_t)p * a.H + h) * a.chunks + chunk] = cost;
    a.part_inl[((int64_t)p * a.H + h) * a.chunks + chunk] = inl;
}

// The better of two (cost, index): the lower cost, the lower index on ties.
RP_HD bool rp_better(double c1, int i1, double c0, int i0) { return c1 < c0 || (c1 == c0 && i1 < i0); }

__global__ void __launch_bounds__(TILE) rp_winner_kernel(const RpArgs a) {
    __shared__ double wc[TILE / 64];
    __shared__ int wi[TILE / 64];
    const int p = blockIdx.x, tid = threadIdx.x;
    double best = __builtin_huge_val();
    int at = 0x7fffffff;
    for (int h = tid; h < a.H; h += TILE) {
        double cost = 0.0;
        int inl = 0;
        for (int c = 0; c < a.chunks; ++c) {
            cost += a.part_cost[((int64_t)p * a.H + h) * a.chunks + c];
            inl += a.part_inl[((int64_t)p * a.H + h) * a.chunks + c];
        }
        a.hyp_cost[(int64_t)p * a.H + h] = cost;
        a.hyp_inl[(int64_t)p * a.H + h] = inl;
        if (rp_better(cost, h, best, at)) {
            best = cost;
            at = h;
        }
    }
    for (int m = 32; m >= 1; m >>= 1) {
        const double c = __shfl_xor(best, m, 64);
        const int i = __shfl_xor(at, m, 64);
        if (rp_better(c, i, best, at)) {
            best = c;
            at = i;
        }
    }
    if ((tid & 63) == 0) {
        wc[tid >> 6] = best;
        wi[tid >> 6] = at;
    }
    __syncthreads();
    if (tid == 0) {
        for (int w = 1; w < TILE / 64; ++w)
            if (rp_better(wc[w], wi[w], best, at)) {
                best = wc[w];
                at = wi[w];
            }
        a.winner[p] = rp_finite(best) ? at : -1;
    }
    __syncthreads();
    if (tid < 9) a.winE[p * 9 + tid] = a.winner[p] >= 0 ? a.hypE[((int64_t)p * a.H + a.winner[p]) * 9 + tid] : rp_nan();
}

// The per-point passes: row p, a pair.
struct RpActive {
    RP_HD static bool skip(const RpArgs &a, int p) { return !a.active[p]; }
};
struct RpStat : RpActive {
    RP_HD static void point(const RpArgs &a, int p, int64_t n, double *acc) { rp_stat_point(a, p, n, acc); }
};
struct RpNormal : RpActive {
    RP_HD static void point(const RpArgs &a, int p, int64_t n, double *acc) { rp_normal_point(a, p, n, acc); }
};

__global__ void __launch_bounds__(TILE) rp_front_kernel(const RpArgs a) {
    __shared__ unsigned int cnt[4];
    const int p = blockIdx.y, tid = threadIdx.x;
    if (tid < 4) cnt[tid] = 0;
    __syncthreads();
    const int64_t n = (int64_t)blockIdx.x * TILE + tid;
    if (n < a.N) {
        const int bits = rp_front_point(a, p, n);
        a.mask[(int64_t)p * a.N + n] = (uint8_t)(bits >> 4);
        for (int i = 0; i < 4; ++i)
            if (bits >> i & 1) atomicAdd(&cnt[i], 1u);
    }
    __syncthreads();
    if (tid < 4 && cnt[tid]) atomicAdd(&a.front[p * 4 + tid], cnt[tid]);
}

// ---- the host's part ----------------------------------------------------------------------------------------------------------
// The four (R, t) of E in an order that does not depend on the decomposition's free signs: t with its largest coordinate
// (first on ties) positive, then negated; the rotation of the larger trace first.  cand [4][12]: (Ra, t), (Ra, -t), (Rb, t),
// (Rb, -t).
void rp_decompose(const double E[9], double cand[48]) {
    double G[9], V[9], sig[3];
    const int k3 = rp_svd3(E, G, V, sig);
    const int i1 = k3 == 0 ? 1 : 0, i2 = k3 == 2 ? 1 : 2;
    double U[9], Vm[9];                                               // columns u1 u2 u1 x u2, v1 v2 v1 x v2
    for (int k = 0; k < 3; ++k) {
        U[3 * k] = G[3 * k + i1] / sig[i1];
        U[3 * k + 1] = G[3 * k + i2] / sig[i2];
        Vm[3 * k] = V[3 * k + i1];
        Vm[3 * k + 1] = V[3 * k + i2];
    }
    for (double *Q : {U, Vm}) {
        Q[2] = Q[3] * Q[7] - Q[6] * Q[4];
        Q[5] = Q[6] * Q[1] - Q[0] * Q[7];
        Q[8] = Q[0] * Q[4] - Q[3] * Q[1];
    }
    double Ra[9], Rb[9], t[3] = {U[2], U[5], U[8]};
    // U W V^T and U W^T V^T, W = [0 -1 0; 1 0 0; 0 0 1]: U W = (u2, -u1, u3), U W^T = (-u2, u1, u3)
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) {
            const double x = U[3 * i + 1] * Vm[3 * j] - U[3 * i] * Vm[3 * j + 1], z = U[3 * i + 2] * Vm[3 * j + 2];
            Ra[3 * i + j] = x + z;
            Rb[3 * i + j] = -x + z;
        }
    int j = 0;
    for (int i = 1; i < 3; ++i)
        if (fabs(t[i]) > fabs(t[j])) j = i;
    if (t[j] < 0.0)
        for (int i = 0; i < 3; ++i) t[i] = -t[i];
    const double n = sqrt(t[0] * t[0] + t[1] * t[1] + t[2] * t[2]);
    for (int i = 0; i < 3; ++i) t[i] /= n;
    if (Rb[0] + Rb[4] + Rb[8] > Ra[0] + Ra[4] + Ra[8])
        for (int i = 0; i < 9; ++i) std::swap(Ra[i], Rb[i]);
    for (int c = 0; c < 4; ++c) {
        memcpy(cand + c * 12, c < 2 ? Ra : Rb, 72);
        for (int i = 0; i < 3; ++i) cand[c * 12 + 9 + i] = c % 2 ? -t[i] : t[i];
    }
}

struct RpRun {
    p2s_ctx *ctx;
    const Block *block;
    RpArgs a;
    std::vector<double> partials;          // the host's copy
    // sums [P][W] of the pass F over the points of the active pairs: parts in order
    template <int W, typename F> int sums(const std::vector<uint8_t> &active, std::vector<double> &out) {
        P2S_TRY((p2s_pass<W, TILE, F>(ctx, a, a.P)));
        P2S_TRY(block->get(partials.data(), a.partials, (size_t)a.P * W * a.parts * 8));
        P2S_TRY(block->wait());
        out.assign((size_t)a.P * W, 0.0);
        for (int p = 0; p < a.P; ++p)
            if (active[p]) p2s_sum_parts(&partials[(size_t)p * W * a.parts], W, a.parts, &out[(size_t)p * W]);
        return P2S_OK;
    }
};

}  // namespace

// ---- C-ABI entry points (include/p2s.h) ----------------------------------------------------------------------------
extern "C" {

int p2s_relative_poses_host(p2s_ctx *ctx, int32_t n_cams, int64_t n_points, const double *xn, const uint8_t *usable, int32_t n_pairs,
                            const int32_t *pairs, int32_t n_hyp, int32_t sample_size, const int32_t *samples, const double *thr2,
                            int32_t rounds, int32_t score_points, double *E_out, double *R_out, double *t_out, double *cost_out,
                            int32_t *inliers_out, int32_t *front_out, int32_t *winner_out, int32_t *refits_out, uint8_t *mask_out,
                            double *hyp_E, double *hyp_cost, int32_t *hyp_inliers) {
    if (n_cams < 2 || n_cams > P2S_MAX_CAMS) return p2s_set_error(P2S_ERR_INVALID_ARG, "n_cams=%d outside [2, %d]", n_cams, P2S_MAX_CAMS);
    if (sample_size < MIN_M || sample_size > MAX_M)
        return p2s_set_error(P2S_ERR_INVALID_ARG, "sample_size=%d outside [%d, %d]", sample_size, MIN_M, MAX_M);
    if (n_hyp < 1) return p2s_set_error(P2S_ERR_INVALID_ARG, "n_hyp=%d: at least one hypothesis a pair is needed", n_hyp);
    if (n_points < 1 || n_points >= ((int64_t)1 << 30)) return p2s_set_error(P2S_ERR_INVALID_ARG, "n_points=%lld outside [1, 2^30)", (long long)n_points);
    if (n_pairs < 1 || (int64_t)n_pairs * n_hyp >= ((int64_t)1 << 27) || n_pairs > 65535)
        return p2s_set_error(P2S_ERR_INVALID_ARG, "n_pairs=%d with n_hyp=%d: expected 1 .. 65535 pairs and fewer than 2^27 hypotheses", n_pairs, n_hyp);
    if (!xn || !usable || !pairs || !samples || !thr2 || !E_out || !R_out || !t_out || !cost_out || !inliers_out || !front_out || !winner_out ||
        !refits_out || !mask_out)
        return p2s_set_error(P2S_ERR_INVALID_ARG, "null argument");
    if (rounds < 0) return p2s_set_error(P2S_ERR_INVALID_ARG, "rounds=%d is negative", rounds);
    const int C = n_cams, P = n_pairs, H = n_hyp, m = sample_size;
    const int64_t N = n_points;
    for (int p = 0; p < P; ++p) {
        const int ca = pairs[2 * p], cb = pairs[2 * p + 1];
        if (ca < 0 || ca >= C || cb < 0 || cb >= C || ca == cb)
            return p2s_set_error(P2S_ERR_INVALID_ARG, "pair %d names the cameras %d and %d; expected two different cameras of 0 .. %d", p, ca, cb, C - 1);
        if (!(thr2[p] > 0.0) || !std::isfinite(thr2[p])) return p2s_set_error(P2S_ERR_INVALID_ARG, "thr2 of pair %d must be positive and finite", p);
    }
    // what counts: usable and finite; the pairs' mutual points and, with score_points, the list the hypotheses are scored on
    std::vector<uint8_t> ok((size_t)C * N);
    for (int c = 0; c < C; ++c)
        for (int64_t n = 0; n < N; ++n) {
            const double *x = xn + ((size_t)c * N + n) * 2;
            ok[(size_t)c * N + n] = usable[(size_t)c * N + n] && std::isfinite(x[0]) && std::isfinite(x[1]);
        }
    std::vector<int32_t> mutual(P), n_list, list;
    int64_t most = 0;
    for (int p = 0; p < P; ++p) {
        const uint8_t *oa = &ok[(size_t)pairs[2 * p] * N], *ob = &ok[(size_t)pairs[2 * p + 1] * N];
        int32_t k = 0;
        for (int64_t n = 0; n < N; ++n) k += oa[n] & ob[n];
        mutual[p] = k;
        most = std::max<int64_t>(most, k);
    }
    const int S = score_points > 0 && most > score_points ? score_points : 0;   // 0: no pair has more, every point is scored
    if (S) {
        n_list.assign(P, 0);
        list.assign((size_t)P * S, 0);
        std::vector<int32_t> all((size_t)most);
        for (int p = 0; p < P; ++p) {
            const uint8_t *oa = &ok[(size_t)pairs[2 * p] * N], *ob = &ok[(size_t)pairs[2 * p + 1] * N];
            int32_t k = 0;
            for (int64_t n = 0; n < N; ++n)
                if (oa[n] & ob[n]) all[k++] = (int32_t)n;
            n_list[p] = std::min<int32_t>(k, S);
            for (int32_t i = 0; i < n_list[p]; ++i) list[(size_t)p * S + i] = k <= S ? all[i] : all[(int64_t)i * k / S];
        }
    }

    Block block{Stage{ctx}};
    RpRun run{ctx, &block, {}, {}};
    RpArgs &a = run.a;
    a.N = N; a.P = P; a.H = H; a.m = m; a.S = S;
    a.tiles = (int32_t)((N + TILE - 1) / TILE);
    a.parts = std::max(1, std::min({a.tiles, MAX_PARTS, (FILL_BLOCKS + P - 1) / P}));
    const int score_tiles = S ? (S + TILE - 1) / TILE : a.tiles, h_blocks = (H + TILE - 1) / TILE;
    int chunks = std::max(1, std::min({score_tiles, MAX_CHUNKS, (int)((FILL_BLOCKS + (int64_t)P * h_blocks - 1) / ((int64_t)P * h_blocks))}));
    const int tiles_per_chunk = (score_tiles + chunks - 1) / chunks;
    chunks = (score_tiles + tiles_per_chunk - 1) / tiles_per_chunk;
    const size_t PH = (size_t)P * H, n_partials = (size_t)P * NSYM * a.parts;
    run.partials.assign(n_partials, 0.0);
    Layout lay;
    const size_t o_pairs = lay.add((size_t)P * 8), o_thr = lay.add((size_t)P * 8), o_E = lay.add((size_t)P * 72), o_act = lay.add(P),
                 o_nrm = lay.add((size_t)P * 48), o_cand = lay.add((size_t)P * 48 * 8), o_front = lay.add((size_t)P * 16), o_win = lay.add((size_t)P * 4),
                 o_nlist = lay.add((size_t)P * 4), o_parts = lay.add(n_partials * 8), o_xn = lay.add((size_t)C * N * 16), o_ok = lay.add((size_t)C * N),
                 o_smp = lay.add(PH * m * 4), o_hE = lay.add(PH * 72), o_pc = lay.add(PH * chunks * 8), o_pi = lay.add(PH * chunks * 4),
                 o_hc = lay.add(PH * 8), o_hi = lay.add(PH * 4), o_list = lay.add((size_t)P * S * 4), o_mask = lay.add((size_t)P * N);
    if (ctx) HIP_TRY(hipSetDevice(ctx->device));
    P2S_TRY(block.alloc(lay.bytes));
    char *blk = block.p;
    P2S_TRY(block.put(blk + o_pairs, pairs, (size_t)P * 8));
    P2S_TRY(block.put(blk + o_thr, thr2, (size_t)P * 8));
    P2S_TRY(block.put(blk + o_xn, xn, (size_t)C * N * 16));
    P2S_TRY(block.put(blk + o_ok, ok.data(), ok.size()));
    P2S_TRY(block.put(blk + o_smp, samples, PH * m * 4));
    if (S) {
        P2S_TRY(block.put(blk + o_nlist, n_list.data(), (size_t)P * 4));
        P2S_TRY(block.put(blk + o_list, list.data(), list.size() * 4));
    }
    a.xn = (const double *)(blk + o_xn); a.ok = (const uint8_t *)(blk + o_ok); a.pairs = (const int32_t *)(blk + o_pairs);
    a.samples = (const int32_t *)(blk + o_smp); a.thr2 = (const double *)(blk + o_thr); a.hypE = (double *)(blk + o_hE);
    a.list = S ? (const int32_t *)(blk + o_list) : nullptr; a.n_list = (const int32_t *)(blk + o_nlist);
    a.part_cost = (double *)(blk + o_pc); a.part_inl = (int32_t *)(blk + o_pi); a.hyp_cost = (double *)(blk + o_hc);
    a.hyp_inl = (int32_t *)(blk + o_hi); a.winner = (int32_t *)(blk + o_win); a.winE = (double *)(blk + o_E); a.E = (const double *)(blk + o_E);
    a.active = (const uint8_t *)(blk + o_act); a.nrm = (const double *)(blk + o_nrm); a.cand = (const double *)(blk + o_cand);
    a.partials = (double *)(blk + o_parts); a.front = (uint32_t *)(blk + o_front); a.mask = (uint8_t *)(blk + o_mask);
    a.chunks = chunks; a.tiles_per_chunk = tiles_per_chunk;
    a.tiles = score_tiles;                                           // of rp_score_kernel; the per-point kernels' below

    // hypotheses, their scores, the winners
    std::vector<int32_t> winner(P);
    std::vector<double> E((size_t)P * 9), Etry((size_t)P * 9);
    P2S_TRY(block.time_begin());
    if (ctx) {
        hipLaunchKernelGGL(rp_hyp_kernel, dim3((unsigned)((PH + HYP_LANES - 1) / HYP_LANES)), dim3(HYP_LANES), 0, ctx->stream, a);
        hipLaunchKernelGGL(rp_score_kernel, dim3((unsigned)h_blocks, (unsigned)chunks, (unsigned)P), dim3(TILE), 0, ctx->stream, a);
        hipLaunchKernelGGL(rp_winner_kernel, dim3((unsigned)P), dim3(TILE), 0, ctx->stream, a);
        HIP_TRY(hipGetLastError());
    } else {
        std::vector<double> work(NWORK);
        for (int p = 0; p < P; ++p) {
            double best = __builtin_huge_val();
            int at = 0x7fffffff;
            for (int h = 0; h < H; ++h) {
                rp_hypothesis(a, p, h, RpMem{work.data(), 1});
                const double *Eh = a.hypE + ((size_t)p * H + h) * 9;
                double cost = 0.0;
                int inl = 0;
                for (int c = 0; c < chunks; ++c) {
                    double part = 0.0;
                    for (int64_t k = (int64_t)c * tiles_per_chunk * TILE; k < std::min<int64_t>((int64_t)(c + 1) * tiles_per_chunk, score_tiles) * TILE; ++k) {
                        double pt[4];
                        rp_score_point(a, p, k, pt);
                        const double d = rp_sampson(Eh, pt[0], pt[1], pt[2], pt[3]);
                        part += rp_msac(d, thr2[p]);
                        inl += d < thr2[p];
                    }
                    cost += part;
                }
                if (!rp_finite9(Eh)) {
                    cost = __builtin_huge_val();
                    inl = 0;
                }
                a.hyp_cost[(size_t)p * H + h] = cost;
                a.hyp_inl[(size_t)p * H + h] = inl;
                if (rp_better(cost, h, best, at)) {
                    best = cost;
                    at = h;
                }
            }
            a.winner[p] = std::isfinite(best) ? at : -1;
            for (int i = 0; i < 9; ++i) a.winE[p * 9 + i] = a.winner[p] >= 0 ? a.hypE[((size_t)p * H + a.winner[p]) * 9 + i] : rp_nan();
        }
    }
    P2S_TRY(block.get(winner.data(), a.winner, (size_t)P * 4));
    P2S_TRY(block.get(E.data(), a.winE, (size_t)P * 72));
    P2S_TRY(block.get(hyp_E, a.hypE, PH * 72));
    P2S_TRY(block.get(hyp_cost, a.hyp_cost, PH * 8));
    P2S_TRY(block.get(hyp_inliers, a.hyp_inl, PH * 4));
    P2S_TRY(block.wait());
    a.tiles = (int32_t)((N + TILE - 1) / TILE);

    // the winners over every mutual point, then the refits
    std::vector<uint8_t> active(P), valid(P);
    std::vector<double> cost(P, rp_nan()), stat, stat_try, normal, nrm((size_t)P * 6, 0.0);
    std::vector<int32_t> refits(P, 0);
    for (int p = 0; p < P; ++p) {
        if (mutual[p] < m) winner[p] = -1;
        valid[p] = active[p] = winner[p] >= 0;
        if (!valid[p])
            for (int i = 0; i < 9; ++i) E[(size_t)p * 9 + i] = rp_nan();
    }
    double *dE = (double *)(blk + o_E);
    uint8_t *dact = (uint8_t *)(blk + o_act);
    P2S_TRY(block.put_wait(dE, E.data(), (size_t)P * 72));
    P2S_TRY(block.put_wait(dact, active.data(), P));
    P2S_TRY((run.sums<NSTAT, RpStat>(active, stat)));
    for (int p = 0; p < P; ++p)
        if (valid[p]) cost[p] = stat[(size_t)p * NSTAT];
    std::vector<double> work(NWORK);
    for (int r = 0; r < rounds; ++r) {
        bool any = false;
        for (int p = 0; p < P; ++p) {
            if (!active[p]) continue;
            const double *s = &stat[(size_t)p * NSTAT], n = s[1];
            double *q = &nrm[(size_t)p * 6];
            active[p] = 0;
            if (n < 8.0) continue;
            q[1] = s[2] / n; q[2] = s[3] / n; q[4] = s[5] / n; q[5] = s[6] / n;
            const double va = s[4] / n - (q[1] * q[1] + q[2] * q[2]), vb = s[7] / n - (q[4] * q[4] + q[5] * q[5]);
            q[0] = sqrt(2.0 / va);
            q[3] = sqrt(2.0 / vb);
            if (!(va > 0.0) || !(vb > 0.0) || !std::isfinite(q[0]) || !std::isfinite(q[3])) continue;
            active[p] = 1;
            any = true;
        }
        if (!any) break;
        P2S_TRY(block.put_wait(dact, active.data(), P));
        P2S_TRY(block.put_wait(blk + o_nrm, nrm.data(), (size_t)P * 48));
        P2S_TRY((run.sums<NSYM, RpNormal>(active, normal)));
        Etry = E;
        for (int p = 0; p < P; ++p) {
            if (!active[p]) continue;
            double f[9];
            memcpy(work.data(), &normal[(size_t)p * NSYM], NSYM * 8);
            rp_eig_smallest(RpMem{work.data(), 1}, f);
            rp_denormalise_project(f, &nrm[(size_t)p * 6], &Etry[(size_t)p * 9]);
            if (!rp_finite9(&Etry[(size_t)p * 9])) {
                active[p] = 0;
                memcpy(&Etry[(size_t)p * 9], &E[(size_t)p * 9], 72);
            }
        }
        P2S_TRY(block.put_wait(dact, active.data(), P));
        P2S_TRY(block.put_wait(dE, Etry.data(), (size_t)P * 72));
        P2S_TRY((run.sums<NSTAT, RpStat>(active, stat_try)));
        for (int p = 0; p < P; ++p) {
            if (!active[p]) continue;
            if (stat_try[(size_t)p * NSTAT] < cost[p]) {
                cost[p] = stat_try[(size_t)p * NSTAT];
                memcpy(&E[(size_t)p * 9], &Etry[(size_t)p * 9], 72);
                memcpy(&stat[(size_t)p * NSTAT], &stat_try[(size_t)p * NSTAT], NSTAT * 8);
                ++refits[p];
            } else {
                active[p] = 0;
            }
        }
    }

    // the four (R, t) of every result, the inliers in front of both cameras, the masks
    std::vector<double> cand((size_t)P * 48, 0.0);
    for (int p = 0; p < P; ++p)
        if (valid[p]) rp_decompose(&E[(size_t)p * 9], &cand[(size_t)p * 48]);
    std::vector<uint32_t> front((size_t)P * 4);
    P2S_TRY(block.put_wait(dact, valid.data(), P));
    P2S_TRY(block.put_wait(dE, E.data(), (size_t)P * 72));
    P2S_TRY(block.put_wait(blk + o_cand, cand.data(), cand.size() * 8));
    if (ctx) {
        HIP_TRY(hipMemsetAsync(a.front, 0, (size_t)P * 16, ctx->stream));
        hipLaunchKernelGGL(rp_front_kernel, dim3((unsigned)a.tiles, (unsigned)P), dim3(TILE), 0, ctx->stream, a);
        HIP_TRY(hipGetLastError());
    } else {
        memset(a.front, 0, (size_t)P * 16);
        for (int p = 0; p < P; ++p)
            for (int64_t n = 0; n < N; ++n) {
                const int bits = rp_front_point(a, p, n);
                a.mask[(size_t)p * N + n] = (uint8_t)(bits >> 4);
                for (int i = 0; i < 4; ++i) a.front[p * 4 + i] += bits >> i & 1;
            }
    }
    P2S_TRY(block.time_end());
    P2S_TRY(block.get(front.data(), a.front, (size_t)P * 16));
    P2S_TRY(block.get(mask_out, a.mask, (size_t)P * N));
    P2S_TRY(block.finish(P2S_TIMED_RELPOSE));
    for (int p = 0; p < P; ++p) {
        int best = 0;
        for (int i = 1; i < 4; ++i)
            if (front[(size_t)p * 4 + i] > front[(size_t)p * 4 + best]) best = i;
        for (int i = 0; i < 9; ++i) {
            E_out[(size_t)p * 9 + i] = E[(size_t)p * 9 + i];
            R_out[(size_t)p * 9 + i] = valid[p] ? cand[(size_t)p * 48 + best * 12 + i] : rp_nan();
        }
        for (int i = 0; i < 3; ++i) t_out[(size_t)p * 3 + i] = valid[p] ? cand[(size_t)p * 48 + best * 12 + 9 + i] : rp_nan();
        cost_out[p] = cost[p];
        inliers_out[p] = valid[p] ? (int32_t)stat[(size_t)p * NSTAT + 1] : 0;
        front_out[p] = valid[p] ? (int32_t)front[(size_t)p * 4 + best] : 0;
        winner_out[p] = winner[p];
        refits_out[p] = refits[p];
    }
    return P2S_OK;
}

int p2s_relpose_kernel_ms(p2s_ctx *ctx, float *elapsed_ms) { return p2s_kernel_ms_query(ctx, P2S_TIMED_RELPOSE, "p2s_relative_poses_host", elapsed_ms); }

}  // extern "C"
