// p2s_floor.hip -- the dominant plane of every problem's points (the floor under the feet of a walking person): planes
// through sampled triples, MSAC scoring by the signed distance, refits on the winner's inliers that are kept while the cost
// falls (include/p2s_floor.h).  fp64 throughout.
//
//   fl_score_kernel   the hot path, per (problem, 256 hypotheses, chunk of points): a lane forms its hypothesis from its three
//                     sample points in the prologue and keeps the plane's four doubles in registers, the workgroup streams the
//                     problem's points through LDS, 256 at a time, every lane reads the same point (a broadcast); B x H x N
//                     point-plane distances
//   fl_total_kernel   per (problem, 256 hypotheses): the chunk sums of every hypothesis added in order
//   fl_winner_kernel  per problem: the lowest cost (lowest index on ties)
//   FlStat            a pass of p2s_passes.h, per (problem, part of the points), one lane a point, the problem's current plane:
//                     cost, inliers, points below, and the inliers' first and second moments about ref; leaves out the
//                     problems that are not active
//   fl_mask_kernel    the inlier mask of the result
//
// No floating-point atomic anywhere: a lane adds its points in order, a wave its lanes by the xor butterfly, a workgroup its
// waves in order (p2s_block_sum), the host the parts (and fl_total_kernel the chunks) in order; counts are integers, or whole
// doubles below 2^53.  Two runs agree bit for bit.  The 3 x 3 eigen-solves of the refits run on the host between the launches.
// ctx == NULL runs the same per-hypothesis and per-point functions on the host (the pass as p2s_pass_host), in a Block of the
// host's memory.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include <string.h>

#include <algorithm>
#include <vector>

#include "p2s_ctx.h"
#include "p2s_floor.h"
#include "p2s_passes.h"

#define FL_HD __host__ __device__ inline

namespace {

constexpr int TILE = P2S_FLOOR_TILE;               // points of a pass through LDS, lanes of a workgroup
constexpr int MAX_CHUNKS = P2S_FLOOR_MAX_CHUNKS;   // cuts of a problem's points in fl_score_kernel
constexpr int MAX_PARTS = P2S_FLOOR_MAX_PARTS;     // workgroups along the points in the stat pass
constexpr int NSTAT = 12;                          // cost, inliers, below, sum u (3), sum u u^T (xx xy xz yy yz zz), u = x - ref
constexpr int FILL_BLOCKS = 1024;                  // workgroups that fill the GPU: 4 a CU

FL_HD double fl_nan() { return __builtin_nan(""); }
FL_HD bool fl_finite(double v) { return fabs(v) < __builtin_huge_val(); }

struct FlArgs {
    const double *pts;           // [B][N][3]
    const uint8_t *ok;           // [B][N] usable and finite
    const double *ref;           // [B][3]
    const int32_t *samples;      // [B][H][3]
    const double *thr;           // [B]
    double *hyp_plane;           // [B][H][4]
    double *part_cost;           // [B][chunks][H]: a wave's lanes side by side, for the kernel that writes and the one that reads
    int32_t *part_inl;
    double *hyp_cost;            // [B][H]
    int32_t *hyp_inl;
    int32_t *winner;             // [B]
    double *win_plane;           // [B][4] the winners' planes, NaN without one: where plane points until the first refit
    const double *plane;         // [B][4] of the per-point kernels
    const uint8_t *active;       // [B]
    double *partials;            // [B][NSTAT][parts]
    uint8_t *mask;               // [B][N]
    int64_t N;
    int32_t B, H, chunks, tiles_per_chunk, tiles, parts;
};

// Point k of problem b: its coordinates, NaN for one that does not count or lies past the last.
FL_HD void fl_point(const FlArgs &a, int b, int64_t k, double x[3]) {
    if (k < a.N && a.ok[(int64_t)b * a.N + k]) {
        const double *p = a.pts + ((int64_t)b * a.N + k) * 3;
        x[0] = p[0]; x[1] = p[1]; x[2] = p[2];
    } else {
        x[0] = x[1] = x[2] = fl_nan();
    }
}

// (n, d) with n . ref - d > 0; false for a plane that is not finite or holds ref.
FL_HD bool fl_orient(const double *ref, double pl[4]) {
    const double s = pl[0] * ref[0] + pl[1] * ref[1] + pl[2] * ref[2] - pl[3];
    if (s < 0.0) {
        pl[0] = -pl[0]; pl[1] = -pl[1]; pl[2] = -pl[2]; pl[3] = -pl[3];
    }
    return s != 0.0 && fl_finite(s);
}

// ---- one hypothesis ---------------------------------------------------------------------------------------------------------
// The plane through the three points of sample h of problem b, ref above it; NaN for a sample that is refused.
FL_HD void fl_hypothesis(const FlArgs &a, int b, int h, double pl[4]) {
    const int32_t *smp = a.samples + ((int64_t)b * a.H + h) * 3;
    const int64_t i0 = smp[0], i1 = smp[1], i2 = smp[2];
    bool good = i0 >= 0 && i0 < a.N && i1 >= 0 && i1 < a.N && i2 >= 0 && i2 < a.N && i0 != i1 && i0 != i2 && i1 != i2;
    const uint8_t *ok = a.ok + (int64_t)b * a.N;
    good = good && ok[i0] && ok[i1] && ok[i2];
    if (good) {
        const double *p0 = a.pts + ((int64_t)b * a.N + i0) * 3, *p1 = a.pts + ((int64_t)b * a.N + i1) * 3, *p2 = a.pts + ((int64_t)b * a.N + i2) * 3;
        const double u0 = p1[0] - p0[0], u1 = p1[1] - p0[1], u2 = p1[2] - p0[2];
        const double v0 = p2[0] - p0[0], v1 = p2[1] - p0[1], v2 = p2[2] - p0[2];
        const double c0 = u1 * v2 - u2 * v1, c1 = u2 * v0 - u0 * v2, c2 = u0 * v1 - u1 * v0;
        const double len = sqrt(c0 * c0 + c1 * c1 + c2 * c2);
        good = len > 0.0 && fl_finite(len);
        if (good) {
            pl[0] = c0 / len; pl[1] = c1 / len; pl[2] = c2 / len;
            pl[3] = pl[0] * p0[0] + pl[1] * p0[1] + pl[2] * p0[2];
            good = fl_orient(a.ref + b * 3, pl);
        }
    }
    if (!good) pl[0] = pl[1] = pl[2] = pl[3] = fl_nan();
}

// ---- the signed distance ----------------------------------------------------------------------------------------------------
FL_HD double fl_signed(const double pl[4], double x, double y, double z) { return pl[0] * x + pl[1] * y + pl[2] * z - pl[3]; }

// min(q, thr2) of a squared distance that is a number, 0 of one that is not.
FL_HD double fl_msac(double q, double thr2) { return q < thr2 ? q : (q >= thr2 ? thr2 : 0.0); }

FL_HD bool fl_finite4(const double pl[4]) { return fl_finite(fabs(pl[0]) + fabs(pl[1]) + fabs(pl[2]) + fabs(pl[3])); }

FL_HD void fl_stat_point(const FlArgs &a, int b, int64_t n, double acc[NSTAT]) {
    if (!a.ok[(int64_t)b * a.N + n]) return;
    const double *p = a.pts + ((int64_t)b * a.N + n) * 3, thr = a.thr[b], thr2 = thr * thr;
    const double s = fl_signed(a.plane + b * 4, p[0], p[1], p[2]), q = s * s;
    acc[0] += fl_msac(q, thr2);
    if (s < -thr) acc[2] += 1.0;
    if (q < thr2) {
        const double *ref = a.ref + b * 3, x = p[0] - ref[0], y = p[1] - ref[1], z = p[2] - ref[2];
        acc[1] += 1.0;
        acc[3] += x; acc[4] += y; acc[5] += z;
        acc[6] += x * x; acc[7] += x * y; acc[8] += x * z; acc[9] += y * y; acc[10] += y * z; acc[11] += z * z;
    }
}

FL_HD bool fl_inlier(const FlArgs &a, int b, int64_t n) {
    if (!a.active[b] || !a.ok[(int64_t)b * a.N + n]) return false;
    const double *p = a.pts + ((int64_t)b * a.N + n) * 3, thr = a.thr[b];
    const double s = fl_signed(a.plane + b * 4, p[0], p[1], p[2]);
    return s * s < thr * thr;
}

// ---- kernels ----------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(TILE) fl_score_kernel(const FlArgs a) {
    __shared__ double pts[3][TILE];
    const int b = blockIdx.z, chunk = blockIdx.y, h = blockIdx.x * TILE + threadIdx.x;
    const bool mine = h < a.H;
    double pl[4] = {0.0, 0.0, 0.0, 0.0};
    if (mine) {
        fl_hypothesis(a, b, h, pl);
        if (chunk == 0) {
#pragma unroll
            for (int i = 0; i < 4; ++i) a.hyp_plane[((int64_t)b * a.H + h) * 4 + i] = pl[i];
        }
    }
    const double thr = a.thr[b], thr2 = thr * thr;
    double cost = 0.0;
    int inl = 0;
    const int t0 = chunk * a.tiles_per_chunk, t1 = min(a.tiles, t0 + a.tiles_per_chunk);
    for (int t = t0; t < t1; ++t) {                                  // uniform over the workgroup
        double x[3];
        fl_point(a, b, (int64_t)t * TILE + threadIdx.x, x);
        __syncthreads();
#pragma unroll
        for (int i = 0; i < 3; ++i) pts[i][threadIdx.x] = x[i];
        __syncthreads();
#pragma unroll 8
        for (int j = 0; j < TILE; ++j) {
            const double s = fl_signed(pl, pts[0][j], pts[1][j], pts[2][j]), q = s * s;
            cost += fl_msac(q, thr2);
            inl += q < thr2;
        }
    }
    if (!mine) return;
    if (!fl_finite4(pl)) {
        cost = __builtin_huge_val();
        inl = 0;
    }
    a.part_cost[((int64_t)b * a.chunks + chunk) * a.H + h] = cost;
    a.part_inl[((int64_t)b * a.chunks + chunk) * a.H + h] = inl;
}

// The better of two (cost, index): the lower cost, the lower index on ties.
FL_HD bool fl_better(double c1, int i1, double c0, int i0) { return c1 < c0 || (c1 == c0 && i1 < i0); }

// A hypothesis' chunk sums added in order: one lane a hypothesis, a wave's lanes side by side in every chunk's row.
__global__ void __launch_bounds__(TILE) fl_total_kernel(const FlArgs a) {
    const int b = blockIdx.y, h = blockIdx.x * TILE + threadIdx.x;
    if (h >= a.H) return;
    double cost = 0.0;
    int inl = 0;
    for (int c = 0; c < a.chunks; ++c) {
        cost += a.part_cost[((int64_t)b * a.chunks + c) * a.H + h];
        inl += a.part_inl[((int64_t)b * a.chunks + c) * a.H + h];
    }
    a.hyp_cost[(int64_t)b * a.H + h] = cost;
    a.hyp_inl[(int64_t)b * a.H + h] = inl;
}

__global__ void __launch_bounds__(TILE) fl_winner_kernel(const FlArgs a) {
    __shared__ double wc[TILE / 64];
    __shared__ int wi[TILE / 64];
    __shared__ int won;
    const int b = blockIdx.x, tid = threadIdx.x;
    double best = __builtin_huge_val();
    int at = 0x7fffffff;
    for (int h = tid; h < a.H; h += TILE) {
        const double cost = a.hyp_cost[(int64_t)b * a.H + h];
        if (fl_better(cost, h, best, at)) {
            best = cost;
            at = h;
        }
    }
    for (int m = 32; m >= 1; m >>= 1) {
        const double c = __shfl_xor(best, m, 64);
        const int i = __shfl_xor(at, m, 64);
        if (fl_better(c, i, best, at)) {
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
            if (fl_better(wc[w], wi[w], best, at)) {
                best = wc[w];
                at = wi[w];
            }
        won = fl_finite(best) ? at : -1;
        a.winner[b] = won;
    }
    __syncthreads();
    if (tid < 4) a.win_plane[b * 4 + tid] = won >= 0 ? a.hyp_plane[((int64_t)b * a.H + won) * 4 + tid] : fl_nan();
}

// The per-point pass: row b, a problem.
struct FlStat {
    FL_HD static bool skip(const FlArgs &a, int b) { return !a.active[b]; }
    FL_HD static void point(const FlArgs &a, int b, int64_t n, double *acc) { fl_stat_point(a, b, n, acc); }
};

__global__ void __launch_bounds__(TILE) fl_mask_kernel(const FlArgs a) {
    const int b = blockIdx.y;
    const int64_t n = (int64_t)blockIdx.x * TILE + threadIdx.x;
    if (n < a.N) a.mask[(int64_t)b * a.N + n] = fl_inlier(a, b, n);
}

// ---- the host's part --------------------------------------------------------------------------------------------------------
// The eigenvalues (ascending) and eigenvectors (the columns of V, row-major) of the symmetric matrix xx xy xz yy yz zz by
// cyclic Jacobi; ties keep the lower index first.
void fl_eig3(const double s[6], double ev[3], double V[9]) {
    double A[3][3] = {{s[0], s[1], s[2]}, {s[1], s[3], s[4]}, {s[2], s[4], s[5]}};
    double Q[3][3] = {{1, 0, 0}, {0, 1, 0}, {0, 0, 1}};
    for (int sweep = 0; sweep < 32; ++sweep) {
        const double off = A[0][1] * A[0][1] + A[0][2] * A[0][2] + A[1][2] * A[1][2];
        const double diag = A[0][0] * A[0][0] + A[1][1] * A[1][1] + A[2][2] * A[2][2];
        if (!(off > 1e-36 * diag)) break;
        for (int p = 0; p < 2; ++p)
            for (int q = p + 1; q < 3; ++q) {
                const double apq = A[p][q];
                if (apq == 0.0) continue;
                const double theta = (A[q][q] - A[p][p]) / (2.0 * apq);
                const double t = (theta >= 0.0 ? 1.0 : -1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));
                const double c = 1.0 / sqrt(t * t + 1.0), sn = t * c;
                const int k = 3 - p - q;
                const double akp = A[k][p], akq = A[k][q];
                A[k][p] = A[p][k] = c * akp - sn * akq;
                A[k][q] = A[q][k] = sn * akp + c * akq;
                A[p][p] -= t * apq;
                A[q][q] += t * apq;
                A[p][q] = A[q][p] = 0.0;
                for (int i = 0; i < 3; ++i) {
                    const double vp = Q[i][p], vq = Q[i][q];
                    Q[i][p] = c * vp - sn * vq;
                    Q[i][q] = sn * vp + c * vq;
                }
            }
    }
    int order[3] = {0, 1, 2};
    for (int i = 0; i < 2; ++i)
        for (int j = 0; j < 2 - i; ++j)
            if (A[order[j + 1]][order[j + 1]] < A[order[j]][order[j]]) std::swap(order[j], order[j + 1]);
    for (int j = 0; j < 3; ++j) {
        ev[j] = A[order[j]][order[j]];
        for (int i = 0; i < 3; ++i) V[3 * i + j] = Q[i][order[j]];
    }
}

// From the sums of FlStat: the inliers' mean m about ref, the eigenvalues of their scatter over their count, and the plane
// through ref + m along the eigenvector of the smallest, ref above it.  false: no plane (not finite, or ref lies in it).
bool fl_refit(const double *stat, const double *ref, double m[3], double ev[3], double pl[4]) {
    const double n = stat[1];
    for (int i = 0; i < 3; ++i) m[i] = stat[3 + i] / n;
    const double S[6] = {stat[6] / n - m[0] * m[0], stat[7] / n - m[0] * m[1], stat[8] / n - m[0] * m[2],
                         stat[9] / n - m[1] * m[1], stat[10] / n - m[1] * m[2], stat[11] / n - m[2] * m[2]};
    double V[9];
    fl_eig3(S, ev, V);
    pl[0] = V[0]; pl[1] = V[3]; pl[2] = V[6];
    pl[3] = pl[0] * (ref[0] + m[0]) + pl[1] * (ref[1] + m[1]) + pl[2] * (ref[2] + m[2]);
    return fl_finite4(pl) && fl_orient(ref, pl);
}

}  // namespace

// ---- C-ABI entry points (include/p2s_floor.h) ----------------------------------------------------------------------------
extern "C" {

int p2s_fit_planes_host(p2s_ctx *ctx, int32_t n_problems, int64_t n_points, const double *points, const uint8_t *usable, const double *ref,
                        int32_t n_hyp, const int32_t *samples, const double *thr, int32_t rounds, double *plane_out, double *cost_out,
                        int32_t *inliers_out, int32_t *below_out, int32_t *winner_out, int32_t *refits_out, double *centroid_out,
                        double *evals_out, uint8_t *mask_out, double *hyp_plane, double *hyp_cost, int32_t *hyp_inliers) {
    if (n_problems < 1 || n_problems > 65535) return p2s_set_error(P2S_ERR_INVALID_ARG, "n_problems=%d outside [1, 65535]", n_problems);
    if (n_points < 1 || n_points >= ((int64_t)1 << 30)) return p2s_set_error(P2S_ERR_INVALID_ARG, "n_points=%lld outside [1, 2^30)", (long long)n_points);
    if (n_hyp < 1 || (int64_t)n_problems * n_hyp >= ((int64_t)1 << 27))
        return p2s_set_error(P2S_ERR_INVALID_ARG, "n_hyp=%d with n_problems=%d: expected 1 or more a problem and fewer than 2^27 hypotheses", n_hyp, n_problems);
    if (rounds < 0) return p2s_set_error(P2S_ERR_INVALID_ARG, "rounds=%d is negative", rounds);
    if (!points || !usable || !ref || !samples || !thr || !plane_out || !cost_out || !inliers_out || !below_out || !winner_out || !refits_out ||
        !centroid_out || !evals_out || !mask_out)
        return p2s_set_error(P2S_ERR_INVALID_ARG, "null argument");
    const int B = n_problems, H = n_hyp;
    const int64_t N = n_points;
    for (int b = 0; b < B; ++b) {
        if (!(thr[b] > 0.0) || !std::isfinite(thr[b])) return p2s_set_error(P2S_ERR_INVALID_ARG, "thr of problem %d must be positive and finite", b);
        if (!std::isfinite(ref[3 * b]) || !std::isfinite(ref[3 * b + 1]) || !std::isfinite(ref[3 * b + 2]))
            return p2s_set_error(P2S_ERR_INVALID_ARG, "ref of problem %d is not finite", b);
    }
    // what counts: usable and finite
    std::vector<uint8_t> ok((size_t)B * N);
    std::vector<int64_t> counting(B, 0);
    for (int b = 0; b < B; ++b)
        for (int64_t n = 0; n < N; ++n) {
            const double *x = points + ((size_t)b * N + n) * 3;
            ok[(size_t)b * N + n] = usable[(size_t)b * N + n] && std::isfinite(x[0]) && std::isfinite(x[1]) && std::isfinite(x[2]);
            counting[b] += ok[(size_t)b * N + n];
        }

    Block block{Stage{ctx}};
    FlArgs a = {};
    a.N = N; a.B = B; a.H = H;
    a.tiles = (int32_t)((N + TILE - 1) / TILE);
    a.parts = std::max(1, std::min({a.tiles, MAX_PARTS, (FILL_BLOCKS + B - 1) / B}));
    const int h_blocks = (H + TILE - 1) / TILE;
    int chunks = std::max(1, std::min({a.tiles, MAX_CHUNKS, (int)((FILL_BLOCKS + (int64_t)B * h_blocks - 1) / ((int64_t)B * h_blocks))}));
    a.tiles_per_chunk = (a.tiles + chunks - 1) / chunks;
    a.chunks = chunks = (a.tiles + a.tiles_per_chunk - 1) / a.tiles_per_chunk;
    const size_t BH = (size_t)B * H, n_partials = (size_t)B * NSTAT * a.parts;
    std::vector<double> partials(n_partials, 0.0);
    Layout lay;
    const size_t o_ref = lay.add((size_t)B * 24), o_thr = lay.add((size_t)B * 8), o_pl = lay.add((size_t)B * 32), o_act = lay.add(B),
                 o_win = lay.add((size_t)B * 4), o_parts = lay.add(n_partials * 8), o_pts = lay.add((size_t)B * N * 24), o_ok = lay.add((size_t)B * N),
                 o_smp = lay.add(BH * 12), o_hp = lay.add(BH * 32), o_pc = lay.add(BH * chunks * 8), o_pi = lay.add(BH * chunks * 4),
                 o_hc = lay.add(BH * 8), o_hi = lay.add(BH * 4), o_mask = lay.add((size_t)B * N);
    if (ctx) HIP_TRY(hipSetDevice(ctx->device));
    P2S_TRY(block.alloc(lay.bytes));
    char *blk = block.p;
    P2S_TRY(block.put(blk + o_ref, ref, (size_t)B * 24));
    P2S_TRY(block.put(blk + o_thr, thr, (size_t)B * 8));
    P2S_TRY(block.put(blk + o_pts, points, (size_t)B * N * 24));
    P2S_TRY(block.put(blk + o_ok, ok.data(), ok.size()));
    P2S_TRY(block.put(blk + o_smp, samples, BH * 12));
    a.pts = (const double *)(blk + o_pts); a.ok = (const uint8_t *)(blk + o_ok); a.ref = (const double *)(blk + o_ref);
    a.samples = (const int32_t *)(blk + o_smp); a.thr = (const double *)(blk + o_thr); a.hyp_plane = (double *)(blk + o_hp);
    a.part_cost = (double *)(blk + o_pc); a.part_inl = (int32_t *)(blk + o_pi); a.hyp_cost = (double *)(blk + o_hc);
    a.hyp_inl = (int32_t *)(blk + o_hi); a.winner = (int32_t *)(blk + o_win); a.win_plane = (double *)(blk + o_pl);
    a.plane = (const double *)(blk + o_pl); a.active = (const uint8_t *)(blk + o_act); a.partials = (double *)(blk + o_parts);
    a.mask = (uint8_t *)(blk + o_mask);

    // hypotheses, their scores, the winners
    std::vector<int32_t> winner(B);
    std::vector<double> plane((size_t)B * 4), plane_try((size_t)B * 4);
    P2S_TRY(block.time_begin());
    if (ctx) {
        hipLaunchKernelGGL(fl_score_kernel, dim3((unsigned)h_blocks, (unsigned)chunks, (unsigned)B), dim3(TILE), 0, ctx->stream, a);
        hipLaunchKernelGGL(fl_total_kernel, dim3((unsigned)h_blocks, (unsigned)B), dim3(TILE), 0, ctx->stream, a);
        hipLaunchKernelGGL(fl_winner_kernel, dim3((unsigned)B), dim3(TILE), 0, ctx->stream, a);
        HIP_TRY(hipGetLastError());
    } else {
        for (int b = 0; b < B; ++b) {
            const double thr2 = thr[b] * thr[b];
            double best = __builtin_huge_val();
            int at = 0x7fffffff;
            for (int h = 0; h < H; ++h) {
                double *pl = a.hyp_plane + ((size_t)b * H + h) * 4;
                fl_hypothesis(a, b, h, pl);
                double cost = 0.0;
                int inl = 0;
                for (int c = 0; c < chunks; ++c) {
                    double part = 0.0;
                    for (int64_t k = (int64_t)c * a.tiles_per_chunk * TILE; k < std::min<int64_t>((int64_t)(c + 1) * a.tiles_per_chunk, a.tiles) * TILE; ++k) {
                        double x[3];
                        fl_point(a, b, k, x);
                        const double s = fl_signed(pl, x[0], x[1], x[2]), q = s * s;
                        part += fl_msac(q, thr2);
                        inl += q < thr2;
                    }
                    cost += part;
                }
                if (!fl_finite4(pl)) {
                    cost = __builtin_huge_val();
                    inl = 0;
                }
                a.hyp_cost[(size_t)b * H + h] = cost;
                a.hyp_inl[(size_t)b * H + h] = inl;
                if (fl_better(cost, h, best, at)) {
                    best = cost;
                    at = h;
                }
            }
            a.winner[b] = std::isfinite(best) ? at : -1;
            for (int i = 0; i < 4; ++i) a.win_plane[b * 4 + i] = a.winner[b] >= 0 ? a.hyp_plane[((size_t)b * H + a.winner[b]) * 4 + i] : fl_nan();
        }
    }
    P2S_TRY(block.get(winner.data(), a.winner, (size_t)B * 4));
    P2S_TRY(block.get(plane.data(), a.win_plane, (size_t)B * 32));
    P2S_TRY(block.get(hyp_plane, a.hyp_plane, BH * 32));
    P2S_TRY(block.get(hyp_cost, a.hyp_cost, BH * 8));
    P2S_TRY(block.get(hyp_inliers, a.hyp_inl, BH * 4));
    P2S_TRY(block.wait());

    // the winners' sums, then the refits: a pass a round, the trial's plane from the sums of the plane before it
    std::vector<uint8_t> active(B), valid(B);
    std::vector<double> stat((size_t)B * NSTAT, 0.0), stat_try((size_t)B * NSTAT, 0.0);
    std::vector<int32_t> refits(B, 0);
    for (int b = 0; b < B; ++b) {
        if (counting[b] < 3) winner[b] = -1;
        valid[b] = active[b] = winner[b] >= 0;
        if (!valid[b])
            for (int i = 0; i < 4; ++i) plane[(size_t)b * 4 + i] = fl_nan();
    }
    double *dplane = (double *)(blk + o_pl);
    uint8_t *dact = (uint8_t *)(blk + o_act);
    auto sums = [&](std::vector<double> &out) -> int {
        P2S_TRY((p2s_pass<NSTAT, TILE, FlStat>(ctx, a, B)));
        P2S_TRY(block.get(partials.data(), a.partials, n_partials * 8));
        P2S_TRY(block.wait());
        for (int b = 0; b < B; ++b)
            if (active[b]) p2s_sum_parts(&partials[(size_t)b * NSTAT * a.parts], NSTAT, a.parts, &out[(size_t)b * NSTAT]);
        return P2S_OK;
    };
    P2S_TRY(block.put_wait(dplane, plane.data(), (size_t)B * 32));
    P2S_TRY(block.put_wait(dact, active.data(), B));
    P2S_TRY(sums(stat));
    for (int r = 0; r < rounds; ++r) {
        bool any = false;
        plane_try = plane;
        for (int b = 0; b < B; ++b) {
            if (!active[b]) continue;
            double m[3], ev[3];
            active[b] = stat[(size_t)b * NSTAT + 1] >= 3.0 && fl_refit(&stat[(size_t)b * NSTAT], ref + 3 * b, m, ev, &plane_try[(size_t)b * 4]);
            if (!active[b]) memcpy(&plane_try[(size_t)b * 4], &plane[(size_t)b * 4], 32);
            any = any || active[b];
        }
        if (!any) break;
        P2S_TRY(block.put_wait(dact, active.data(), B));
        P2S_TRY(block.put_wait(dplane, plane_try.data(), (size_t)B * 32));
        P2S_TRY(sums(stat_try));
        for (int b = 0; b < B; ++b) {
            if (!active[b]) continue;
            if (stat_try[(size_t)b * NSTAT] < stat[(size_t)b * NSTAT]) {
                memcpy(&plane[(size_t)b * 4], &plane_try[(size_t)b * 4], 32);
                memcpy(&stat[(size_t)b * NSTAT], &stat_try[(size_t)b * NSTAT], NSTAT * 8);
                ++refits[b];
            } else {
                active[b] = 0;
            }
        }
    }

    // the masks of the results
    P2S_TRY(block.put_wait(dact, valid.data(), B));
    P2S_TRY(block.put_wait(dplane, plane.data(), (size_t)B * 32));
    if (ctx) {
        hipLaunchKernelGGL(fl_mask_kernel, dim3((unsigned)a.tiles, (unsigned)B), dim3(TILE), 0, ctx->stream, a);
        HIP_TRY(hipGetLastError());
    } else {
        for (int b = 0; b < B; ++b)
            for (int64_t n = 0; n < N; ++n) a.mask[(size_t)b * N + n] = fl_inlier(a, b, n);
    }
    P2S_TRY(block.time_end());
    P2S_TRY(block.get(mask_out, a.mask, (size_t)B * N));
    P2S_TRY(block.finish(P2S_TIMED_FLOOR));
    for (int b = 0; b < B; ++b) {
        const double *s = &stat[(size_t)b * NSTAT];
        double m[3] = {fl_nan(), fl_nan(), fl_nan()}, ev[3] = {fl_nan(), fl_nan(), fl_nan()}, unused[4];
        if (valid[b] && s[1] >= 1.0) fl_refit(s, ref + 3 * b, m, ev, unused);
        for (int i = 0; i < 4; ++i) plane_out[(size_t)b * 4 + i] = plane[(size_t)b * 4 + i];
        for (int i = 0; i < 3; ++i) {
            centroid_out[(size_t)b * 3 + i] = ref[3 * b + i] + m[i];
            evals_out[(size_t)b * 3 + i] = ev[i];
        }
        cost_out[b] = valid[b] ? s[0] : fl_nan();
        inliers_out[b] = valid[b] ? (int32_t)s[1] : 0;
        below_out[b] = valid[b] ? (int32_t)s[2] : 0;
        winner_out[b] = winner[b];
        refits_out[b] = refits[b];
    }
    return P2S_OK;
}

int p2s_floor_kernel_ms(p2s_ctx *ctx, float *elapsed_ms) { return p2s_kernel_ms_query(ctx, P2S_TIMED_FLOOR, "p2s_fit_planes_host", elapsed_ms); }

}  // extern "C"
