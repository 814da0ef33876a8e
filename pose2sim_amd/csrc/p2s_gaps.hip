// p2s_gaps.hip -- the frame-sequential tail of triangulate_all after person tracking, every column of a trial at once:
// gap interpolation (common.py:669-712 through scipy's interp1d), the list of interpolated and not-interpolated spans
// (triangulation.py:917-919, 946-953) and gap filling (:922-926).  float64 end to end.
//
//   gap_tile_kernel<MODE>    per tile of 256 samples of a column: how many samples count, the last run start
//   cam_tile_scan_kernel     p2s_scan.h, the columns as its cameras: the tiles' sums and maxima scanned along the column
//   gap_index_kernel<MODE>   per sample: its rank among the counted ones and the start of its run; what follows from them
//   gap_linear_kernel        kinds None and 'linear': one thread a sample
//   spline_pack / spline_solve / spline_eval   kinds 'slinear', 'quadratic', 'cubic': one lane a column solves the banded
//                            collocation system, one thread a sample evaluates the spline in the gaps
//
// One index pass serves the three entry points.  A sample's rank is the number of counted samples before it in its
// column, its start the last position at or before it that opens a run.  MODE says what counts and what opens a run:
//   INTERP  good samples count (not NaN, not 0); a bad sample opens a run after a good one or a label step above 1.
//           The good samples are listed (pos [rank][C]) and every run's last sample leaves the run's length at the run's
//           start (runlen [start][C]): a bad sample of rank r then sits between the good samples r - 1 and r.
//   FILL    a sample that is not NaN opens a "run": start is the last valid sample at or before this one.
//   RUNS    the last sample of every run of bad positions counts: its rank is the run's row in the column's table.
//
// Bit equality.  Contraction is off for this file.  Kind None is np.interp's arithmetic ((y1 - y0) / (x1 - x0), then
// slope * (x - x0) + y0, the other end when that is NaN), kind 'linear' interp1d._call_linear's on the segment that
// searchsorted clipped to [1, n - 1] picks.  The spline kinds are scipy's make_interp_spline restated -- its knots, the
// collocation rows by de Boor's recurrence -- but solved by elimination without pivoting (the matrix is totally positive),
// so they agree with LAPACK's answer to rounding, not bit for bit.
// ctx == NULL runs the same functions on the host, column after column: the restatement is checked without a GPU.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include <string.h>

#include <algorithm>
#include <vector>

#include "p2s_ctx.h"
#include "p2s_scan.h"

#pragma clang fp contract(off)

#define GP_HD __host__ __device__ inline

enum { GP_INTERP, GP_FILL, GP_RUNS };

struct P2sGapArgs {
    const double *in;            // [F][C]
    double *out;                 // [F][C]
    const int64_t *labels;       // [F] INTERP
    int64_t F;
    int32_t C, tiles;
    double max_gap;
    int32_t kind;                // P2S_GAPS_KIND_* (INTERP), P2S_GAPS_FILL_* (FILL)
    int64_t first, last;         // RUNS: positions strictly between them
    int32_t *rank, *start;       // [F][C]
    int32_t *pos, *runlen;       // [F][C] INTERP
    int32_t *status;             // [C] INTERP
    int32_t *first_valid;        // [C] FILL: the first sample that is not NaN, F without one
    int64_t *tv_sum, *tb_sum, *tv_max, *tb_max;   // [C][tiles]
    int64_t *totals;             // [C] counted samples of every column
    int64_t *col_base;           // [C + 1] RUNS: the first row of every column, and the rows of all
    int32_t *table;              // [capacity][4] RUNS
    int64_t capacity;
    double *ws;                  // spline kinds: [rows][k + 4][cc] of the columns c0 .. c0 + cc
    int32_t c0, cc;
};

namespace {

constexpr int GT = CAM_TILE;             // samples of a tile, lanes of its workgroup

GP_HD double gp_nan() { return __builtin_nan(""); }
GP_HD bool gp_isnan(double v) { return v != v; }
GP_HD bool gp_finite(double v) { return v == v && v != __builtin_huge_val() && v != -__builtin_huge_val(); }
GP_HD bool gp_bad(double v) { return v != v || v == 0; }              // -0.0 == 0

template <int MODE> GP_HD bool gp_marked(const P2sGapArgs &a, int64_t f, int c) {
    const double v = a.in[f * a.C + c];
    if (MODE == GP_INTERP) return gp_bad(v);
    if (MODE == GP_FILL) return !gp_isnan(v);
    return (v == 0 || !gp_finite(v)) && f > a.first && f < a.last;
}

// What sample f of column c is to the scans: cnt, it counts; st, it opens a run; en, it closes one.
template <int MODE> GP_HD void gp_flags(const P2sGapArgs &a, int64_t f, int c, bool &cnt, bool &st, bool &en) {
    const bool m = gp_marked<MODE>(a, f, c);
    if (MODE == GP_FILL) { cnt = false; st = m; en = false; return; }
    if (!m) { cnt = MODE == GP_INTERP; st = en = false; return; }
    bool joins_prev = f > 0 && gp_marked<MODE>(a, f - 1, c), joins_next = f + 1 < a.F && gp_marked<MODE>(a, f + 1, c);
    if (MODE == GP_INTERP) {
        joins_prev = joins_prev && a.labels[f] - a.labels[f - 1] <= 1;
        joins_next = joins_next && a.labels[f + 1] - a.labels[f] <= 1;
    }
    st = !joins_prev; en = !joins_next;
    cnt = MODE == GP_RUNS && en;
}

// What the index pass leaves of sample f: rank, the counted samples before it; start, the last run start at or before it.
template <int MODE> GP_HD void gp_emit(const P2sGapArgs &a, int64_t f, int c, int64_t rank, int64_t start, bool cnt, bool en) {
    const int64_t at = f * a.C + c;
    if (MODE == GP_INTERP) {
        a.rank[at] = (int32_t)rank; a.start[at] = (int32_t)start;
        if (cnt) a.pos[rank * a.C + c] = (int32_t)f;                                  // rank < F
        if (en) a.runlen[start * a.C + c] = (int32_t)(f - start + 1);                 // a bad sample has a run start: start >= 0
    } else if (MODE == GP_FILL) {
        double v = a.in[at];
        if (a.kind == P2S_GAPS_FILL_LAST_VALUE && gp_isnan(v)) {
            const int64_t first = a.first_valid[c], src = start >= 0 ? start : first;
            if (first < a.F) v = a.in[src * a.C + c];
        }
        if (gp_isnan(v) || v == __builtin_huge_val()) v = 0;
        a.out[at] = v;
    } else if (en) {
        const int64_t row = a.col_base[c] + rank;
        if (row < a.capacity) {
            int32_t *t = a.table + row * 4;
            t[0] = c; t[1] = (int32_t)start; t[2] = (int32_t)f; t[3] = (double)(f - start + 1) > a.max_gap ? 1 : 0;
        }
    }
}

// ---- kinds None and 'linear' ----------------------------------------------------------------------------------------------
// The bad sample at f, rank r among the n > 4 good samples of its column (r good samples lie before it).
GP_HD double gp_linear_value(const P2sGapArgs &a, int64_t f, int c, int64_t r, int64_t n) {
    const int64_t xl = a.labels[f];
    if (a.kind == P2S_GAPS_KIND_NONE) {
        if (r == 0 || r == n) return gp_nan();                                        // outside the good samples: fill_value
        const int64_t p0 = a.pos[(r - 1) * a.C + c], p1 = a.pos[r * a.C + c];
        const double x = (double)xl, x0 = (double)a.labels[p0], x1 = (double)a.labels[p1], y0 = a.in[p0 * a.C + c], y1 = a.in[p1 * a.C + c];
        const double slope = (y1 - y0) / (x1 - x0);
        double res = slope * (x - x0) + y0;
        if (gp_isnan(res)) {
            res = slope * (x - x1) + y1;
            if (gp_isnan(res) && y0 == y1) res = y0;
        }
        return res;
    }
    const int64_t hi = r < 1 ? 1 : r > n - 1 ? n - 1 : r;
    const int64_t p0 = a.pos[(hi - 1) * a.C + c], p1 = a.pos[hi * a.C + c];
    const int64_t x0 = a.labels[p0], x1 = a.labels[p1];
    const double y0 = a.in[p0 * a.C + c], y1 = a.in[p1 * a.C + c];
    const double slope = (y1 - y0) / (double)(x1 - x0);
    return slope * (double)(xl - x0) + y0;
}

// Sample f of column c as interpolate_gaps leaves it when a value of the interpolant is not needed: true, *v is it.
GP_HD bool gp_settled(const P2sGapArgs &a, int64_t f, int c, double *v) {
    const int64_t at = f * a.C + c;
    *v = a.in[at];
    if (!gp_bad(*v) || a.totals[c] <= 4 || a.status[c]) return true;
    if ((double)a.runlen[(int64_t)a.start[at] * a.C + c] > a.max_gap) { *v = gp_nan(); return true; }
    return false;
}

GP_HD void gp_linear_sample(const P2sGapArgs &a, int64_t f, int c) {
    double v;
    if (!gp_settled(a, f, c, &v)) v = gp_linear_value(a, f, c, a.rank[f * a.C + c], a.totals[c]);
    a.out[f * a.C + c] = v;
}

// ---- the spline kinds ------------------------------------------------------------------------------------------------------
// A column's rows of the workspace, GP_SLOTS(k) doubles each: row i holds x_i, then y_i twice -- less the column's first
// good sample and less its last; the two sets of coefficients once solved -- then the eliminated row's diagonal and the k
// entries above it.
//
// Why two right-hand sides.  B-splines sum to 1, so the spline through y - m is the spline through y, less m.  Beyond
// the ends the end polynomial goes on and the B-splines grow like the cube of the distance: a coefficient that is wrong
// in its last bit moves the value by dozens of them.  A solve carries the rounding of its own magnitudes, and close to
// its reference sample y - m is small (and exact): the coefficients solved from y - y_first are as good as exact next to
// the first sample, those from y - y_last next to the last.  One elimination carries both; a sample takes the set of the
// nearer end.
#define GP_SLOTS(K) ((K) + 4)
struct GpCol {
    double *p;
    size_t srow, sslot;
    int64_t n;
    GP_HD double &at(int64_t i, int slot) const { return p[(size_t)i * srow + (size_t)slot * sslot]; }
    GP_HD double x(int64_t i) const { return at(i, 0); }
};

// Knot j of make_interp_spline's vector (n + k + 1 of them) over the abscissae x_0 .. x_{n-1}, n >= 5.
template <int K> GP_HD double gp_knot(const GpCol &w, int64_t j) {
    const int64_t n = w.n;
    if (K == 1) return w.x(j - 1 < 0 ? 0 : j - 1 > n - 1 ? n - 1 : j - 1);            // _augknt: x with its ends repeated
    if (j <= K) return w.x(0);
    if (j >= n) return w.x(n - 1);
    if (K == 2) return (w.x(j - 1) + w.x(j - 2)) / 2;                                 // _not_a_knot, even k: the midpoints but the first and last
    return w.x(j - 2);                                                                // odd k: the abscissae but the second and second to last
}

// The k + 1 B-splines that live on [t_ell, t_ell+1) at x: h[m] = B_{ell-k+m}(x), de Boor's recurrence as scipy runs it.
template <int K> GP_HD void gp_basis(const GpCol &w, int64_t ell, double x, double *h) {
    double t[2 * K], hh[K];
    for (int i = 0; i < 2 * K; ++i) t[i] = gp_knot<K>(w, ell - K + 1 + i);
    h[0] = 1.0;
    for (int j = 1; j <= K; ++j) {
        for (int i = 0; i < j; ++i) hh[i] = h[i];
        h[0] = 0.0;
        for (int m = 1; m <= j; ++m) {
            const double xb = t[K - 1 + m], xa = t[K - 1 + m - j];
            if (xb == xa) { h[m] = 0.0; continue; }
            const double q = hh[m - 1] / (xb - xa);
            h[m - 1] += q * (xb - x);
            h[m] = q * (x - xa);
        }
    }
}

// The interval of abscissa x_i: the last one whose left knot is at or below it, within [k, n - 1].
template <int K> GP_HD int64_t gp_row_interval(int64_t i, int64_t n) {
    const int64_t ell = i + (K == 3 ? 2 : 1);
    return ell < K ? K : ell > n - 1 ? n - 1 : ell;
}

// The coefficients of the interpolating spline of degree K through the column's n >= 5 samples, for both right-hand
// sides.  Row i of the collocation matrix, B_j(x_i), has its K + 1 entries within K of the diagonal; the matrix is totally
// positive, so elimination in the natural order meets no small pivot.  The last K eliminated rows stay in registers;
// every row goes to the workspace for the substitution that runs back from the last one.
template <int K> GP_HD void gp_spline_solve(const GpCol &w) {
    const int64_t n = w.n;
    double pd[K], pu[K][K], pa[K], pb[K];                         // rows i - K .. i - 1: diagonal, the K entries above it, right sides
    for (int p = 0; p < K; ++p) {
        pd[p] = 1.0; pa[p] = pb[p] = 0.0;
        for (int q = 0; q < K; ++q) pu[p][q] = 0.0;
    }
    for (int64_t i = 0; i < n; ++i) {
        const int64_t ell = gp_row_interval<K>(i, n);
        const int off = (int)(ell - i);                           // 0 .. K
        double h[K + 1], row[2 * K + 1];                          // row: columns i - K .. i + K
        gp_basis<K>(w, ell, w.x(i), h);
        for (int s = 0; s <= 2 * K; ++s) {
            row[s] = 0.0;
            for (int m = 0; m <= K; ++m)
                if (s == m + off) row[s] = h[m];
        }
        double ra = w.at(i, 1), rb = w.at(i, 2);
        for (int p = 0; p < K; ++p) {
            if (row[p] == 0.0) continue;                          // also every column before the first
            const double f = row[p] / pd[p];
            for (int q = 0; q < K; ++q) row[p + 1 + q] -= f * pu[p][q];
            ra -= f * pa[p]; rb -= f * pb[p];
        }
        w.at(i, 1) = ra; w.at(i, 2) = rb; w.at(i, 3) = row[K];
        for (int q = 0; q < K; ++q) w.at(i, 4 + q) = row[K + 1 + q];
        for (int p = 0; p + 1 < K; ++p) {
            pd[p] = pd[p + 1]; pa[p] = pa[p + 1]; pb[p] = pb[p + 1];
            for (int q = 0; q < K; ++q) pu[p][q] = pu[p + 1][q];
        }
        pd[K - 1] = row[K]; pa[K - 1] = ra; pb[K - 1] = rb;
        for (int q = 0; q < K; ++q) pu[K - 1][q] = row[K + 1 + q];
    }
    double na[K], nb[K];                                          // c_{i+1} .. c_{i+K}
    for (int q = 0; q < K; ++q) na[q] = nb[q] = 0.0;
    for (int64_t i = n - 1; i >= 0; --i) {
        double sa = w.at(i, 1), sb = w.at(i, 2);
        for (int q = 0; q < K; ++q) {
            const double u = w.at(i, 4 + q);
            sa -= u * na[q]; sb -= u * nb[q];
        }
        const double d = w.at(i, 3);
        sa /= d; sb /= d;
        w.at(i, 1) = sa; w.at(i, 2) = sb;
        for (int q = K - 1; q > 0; --q) { na[q] = na[q - 1]; nb[q] = nb[q - 1]; }
        na[0] = sa; nb[0] = sb;
    }
}

// The spline of the coefficients in `slot` at x, r of the n abscissae below it; beyond the ends the first and the last
// polynomial go on.
template <int K> GP_HD double gp_spline_value(const GpCol &w, int64_t r, double x, int slot) {
    const int64_t n = w.n;
    int64_t ell = r + 1 < K ? K : r + 1 > n - 1 ? n - 1 : r + 1;
    while (ell > K && gp_knot<K>(w, ell) > x) --ell;
    while (ell < n - 1 && gp_knot<K>(w, ell + 1) <= x) ++ell;
    double h[K + 1], v = 0.0;
    gp_basis<K>(w, ell, x, h);
    for (int m = 0; m <= K; ++m) v += w.at(ell - K + m, slot) * h[m];
    return v;
}

GP_HD GpCol gp_col(const P2sGapArgs &a, int c, int K) {
    return GpCol{a.ws + (c - a.c0), (size_t)GP_SLOTS(K) * a.cc, (size_t)a.cc, a.totals[c]};
}

GP_HD bool gp_spline_wanted(const P2sGapArgs &a, int c) { return a.totals[c] > 4 && !a.status[c]; }

// The reference sample of a right-hand side: the column's first good sample (which = 0) or its last (1); degree 1 has
// nothing to solve and takes the samples as they are.
GP_HD double gp_reference(const P2sGapArgs &a, int c, int K, int which) {
    if (K == 1) return 0.0;
    return a.in[(int64_t)a.pos[(which ? a.totals[c] - 1 : 0) * a.C + c] * a.C + c];
}

GP_HD void gp_pack_sample(const P2sGapArgs &a, int64_t f, int c, int K) {
    const double v = a.in[f * a.C + c];
    if (gp_bad(v) || !gp_spline_wanted(a, c)) return;
    const GpCol w = gp_col(a, c, K);
    const int64_t r = a.rank[f * a.C + c];
    w.at(r, 0) = (double)a.labels[f]; w.at(r, 1) = v - gp_reference(a, c, K, 0); w.at(r, 2) = v - gp_reference(a, c, K, 1);
}

GP_HD void gp_solve_column(const P2sGapArgs &a, int c, int K) {
    if (!gp_spline_wanted(a, c)) return;
    if (K == 2) gp_spline_solve<2>(gp_col(a, c, K));
    if (K == 3) gp_spline_solve<3>(gp_col(a, c, K));              // K == 1: the coefficients are the samples
}

GP_HD void gp_spline_sample(const P2sGapArgs &a, int64_t f, int c, int K) {
    double v;
    if (!gp_settled(a, f, c, &v)) {
        const GpCol w = gp_col(a, c, K);
        const int64_t r = a.rank[f * a.C + c];
        const double x = (double)a.labels[f];
        const int which = 2 * r >= w.n;                           // the nearer end, counted in samples
        v = K == 1 ? gp_spline_value<1>(w, r, x, 1) : K == 2 ? gp_spline_value<2>(w, r, x, 1 + which) : gp_spline_value<3>(w, r, x, 1 + which);
        if (K > 1) v += gp_reference(a, c, K, which);
    }
    a.out[f * a.C + c] = v;
}

// ---- kernels ------------------------------------------------------------------------------------------------------------------
template <int MODE> __global__ void __launch_bounds__(GT) gap_tile_kernel(const P2sGapArgs a) {
    __shared__ int64_t part[GT / 64];
    const int c = blockIdx.y, tid = threadIdx.x;
    const int64_t f = (int64_t)blockIdx.x * GT + tid;
    bool cnt = false, st = false, en = false;
    if (f < a.F) gp_flags<MODE>(a, f, c, cnt, st, en);
    int64_t n_cnt, last_st;
    block_scan_exclusive<OpSum>(cnt ? 1 : 0, part, &n_cnt);
    const int64_t before = block_scan_exclusive<OpMax>(st ? f : -1, part, &last_st);
    if (tid == 0) {
        a.tv_sum[(int64_t)c * a.tiles + blockIdx.x] = n_cnt;
        a.tv_max[(int64_t)c * a.tiles + blockIdx.x] = last_st;
    }
    if (MODE == GP_FILL && st && before < 0) atomicMin(&a.first_valid[c], (int)f);   // the tile's first valid sample
    if (MODE == GP_INTERP && a.kind >= P2S_GAPS_KIND_SLINEAR && cnt && !gp_finite(a.in[f * a.C + c])) a.status[c] = P2S_GAPS_NONFINITE;
}

template <int MODE> __global__ void __launch_bounds__(GT) gap_index_kernel(const P2sGapArgs a) {
    __shared__ int64_t part[GT / 64];
    const int c = blockIdx.y, tid = threadIdx.x;
    const int64_t f = (int64_t)blockIdx.x * GT + tid;
    bool cnt = false, st = false, en = false;
    if (f < a.F) gp_flags<MODE>(a, f, c, cnt, st, en);
    const int64_t tile = (int64_t)c * a.tiles + blockIdx.x;
    const int64_t rank = a.tb_sum[tile] + block_scan_exclusive<OpSum>(cnt ? 1 : 0, part, nullptr);
    int64_t start = OpMax::apply(a.tb_max[tile], block_scan_exclusive<OpMax>(st ? f : -1, part, nullptr));
    if (st) start = f;
    if (f < a.F) gp_emit<MODE>(a, f, c, rank, start, cnt, en);
    if (MODE == GP_INTERP && f == 0 && a.totals[c] <= 4) a.status[c] = 0;            // untouched whatever it holds
}

// col_base [C + 1] from the columns' run counts; one lane: C is a few dozen.
__global__ void gap_col_base_kernel(const P2sGapArgs a) {
    if (threadIdx.x || blockIdx.x) return;
    int64_t s = 0;
    for (int c = 0; c < a.C; ++c) { a.col_base[c] = s; s += a.totals[c]; }
    a.col_base[a.C] = s;
}

__global__ void __launch_bounds__(GT) gap_linear_kernel(const P2sGapArgs a) {
    const int64_t f = (int64_t)blockIdx.x * GT + threadIdx.x;
    if (f < a.F) gp_linear_sample(a, f, blockIdx.y);
}

template <int K> __global__ void __launch_bounds__(GT) spline_pack_kernel(const P2sGapArgs a) {
    const int64_t f = (int64_t)blockIdx.x * GT + threadIdx.x;
    if (f < a.F) gp_pack_sample(a, f, a.c0 + blockIdx.y, K);
}

template <int K> __global__ void __launch_bounds__(64) spline_solve_kernel(const P2sGapArgs a) {
    const int cl = blockIdx.x * 64 + threadIdx.x;
    if (cl < a.cc) gp_solve_column(a, a.c0 + cl, K);
}

template <int K> __global__ void __launch_bounds__(GT) spline_eval_kernel(const P2sGapArgs a) {
    const int64_t f = (int64_t)blockIdx.x * GT + threadIdx.x;
    if (f < a.F) gp_spline_sample(a, f, a.c0 + blockIdx.y, K);
}

template <int MODE> hipError_t launch_index(const P2sGapArgs &a, const int64_t *frame_off, hipStream_t s) {
    const dim3 grid((unsigned)a.tiles, (unsigned)a.C);
    hipLaunchKernelGGL(gap_tile_kernel<MODE>, grid, dim3(GT), 0, s, a);
    const CamScanArgs sum{frame_off, nullptr, a.tv_sum, a.tb_sum, nullptr, nullptr, a.totals, a.C, a.tiles};
    const CamScanArgs mx{frame_off, nullptr, a.tv_max, a.tb_max, nullptr, nullptr, nullptr, a.C, a.tiles};
    hipLaunchKernelGGL(cam_tile_scan_kernel<OpSum>, dim3((unsigned)a.C), dim3(1024), 0, s, sum);
    hipLaunchKernelGGL(cam_tile_scan_kernel<OpMax>, dim3((unsigned)a.C), dim3(1024), 0, s, mx);
    if (MODE == GP_RUNS) hipLaunchKernelGGL(gap_col_base_kernel, dim3(1), dim3(64), 0, s, a);
    hipLaunchKernelGGL(gap_index_kernel<MODE>, grid, dim3(GT), 0, s, a);
    return hipGetLastError();
}

template <int K> hipError_t launch_spline_chunk(const P2sGapArgs &a, hipStream_t s) {
    const dim3 grid((unsigned)a.tiles, (unsigned)a.cc);
    hipLaunchKernelGGL(spline_pack_kernel<K>, grid, dim3(GT), 0, s, a);
    if (K > 1) hipLaunchKernelGGL(spline_solve_kernel<K>, dim3((unsigned)((a.cc + 63) / 64)), dim3(64), 0, s, a);
    hipLaunchKernelGGL(spline_eval_kernel<K>, grid, dim3(GT), 0, s, a);
    return hipGetLastError();
}

// ---- the same passes on the host -------------------------------------------------------------------------------------------
template <int MODE> void host_index(const P2sGapArgs &a) {
    for (int c = 0; c < a.C; ++c) {
        if (MODE == GP_FILL) {
            a.first_valid[c] = (int32_t)a.F;
            for (int64_t f = a.F - 1; f >= 0; --f)
                if (gp_marked<MODE>(a, f, c)) a.first_valid[c] = (int32_t)f;
        }
        int64_t n = 0;
        for (int pass = MODE == GP_RUNS ? 0 : 1; pass < 2; ++pass) {      // RUNS: the column's count comes before its rows
            int64_t rank = 0, start = -1;
            for (int64_t f = 0; f < a.F; ++f) {
                bool cnt, st, en;
                gp_flags<MODE>(a, f, c, cnt, st, en);
                if (st) start = f;
                if (pass == 1) gp_emit<MODE>(a, f, c, rank, start, cnt, en);
                if (MODE == GP_INTERP && a.kind >= P2S_GAPS_KIND_SLINEAR && cnt && !gp_finite(a.in[f * a.C + c])) a.status[c] = P2S_GAPS_NONFINITE;
                rank += cnt;
            }
            n = rank;
            if (MODE == GP_RUNS && pass == 0) a.col_base[c + 1] = a.col_base[c] + n;
        }
        a.totals[c] = n;
        if (MODE == GP_INTERP && n <= 4) a.status[c] = 0;         // untouched whatever it holds
    }
}

// The columns that go through the spline kernels together: as many as the workspace cap holds, one at least.
int64_t spline_chunk_cols(int64_t F, int32_t C, int K, size_t cap_bytes) {
    const size_t per_col = (size_t)F * GP_SLOTS(K) * sizeof(double);
    return std::max<int64_t>(1, std::min<int64_t>(C, (int64_t)(cap_bytes / per_col)));
}

int gaps_check(int64_t F, int32_t C, const void *in, const void *out) {
    if (F < 1 || F > ((int64_t)1 << 30)) return p2s_set_error(P2S_ERR_INVALID_ARG, "n_frames=%lld outside [1, 2^30]", (long long)F);
    if (C < 1 || C > 65535) return p2s_set_error(P2S_ERR_INVALID_ARG, "n_cols=%d outside [1, 65535]", C);
    if (!in || !out) return p2s_set_error(P2S_ERR_INVALID_ARG, "null argument");
    return P2S_OK;
}

int kind_degree(int32_t kind) { return kind == P2S_GAPS_KIND_SLINEAR ? 1 : kind == P2S_GAPS_KIND_QUADRATIC ? 2 : kind == P2S_GAPS_KIND_CUBIC ? 3 : 0; }

// The scans' buffers of one call: the columns' offsets as the scan kernels read them (F frames a column), the tiles.
struct GapScan {
    std::vector<int64_t> frame_off;
    Layout words;
    size_t o_foff, o_tvs, o_tbs, o_tvm, o_tbm, o_tot;
    GapScan(int64_t F, int32_t C, int64_t tiles) : frame_off((size_t)C + 1) {
        for (size_t c = 0; c <= (size_t)C; ++c) frame_off[c] = (int64_t)c * F;
        const size_t nt = (size_t)C * tiles * 8;
        o_foff = words.add(((size_t)C + 1) * 8); o_tvs = words.add(nt); o_tbs = words.add(nt); o_tvm = words.add(nt); o_tbm = words.add(nt);
        o_tot = words.add((size_t)C * 8);
    }
    void point(P2sGapArgs &a, char *w) const {
        a.tv_sum = (int64_t *)(w + o_tvs); a.tb_sum = (int64_t *)(w + o_tbs); a.tv_max = (int64_t *)(w + o_tvm); a.tb_max = (int64_t *)(w + o_tbm);
        a.totals = (int64_t *)(w + o_tot);
    }
};

}  // namespace

// ---- C-ABI entry points (include/p2s.h) ----------------------------------------------------------------------------
extern "C" {

int p2s_interpolate_gaps(p2s_ctx *ctx, int64_t n_frames, int32_t n_cols, const double *coords, const int64_t *labels, double max_gap,
                         int32_t kind, double *out, int32_t *status) {
    P2S_TRY(gaps_check(n_frames, n_cols, coords, out));
    if (!labels || !status) return p2s_set_error(P2S_ERR_INVALID_ARG, "null argument");
    if (kind < P2S_GAPS_KIND_NONE || kind > P2S_GAPS_KIND_CUBIC) return p2s_set_error(P2S_ERR_INVALID_ARG, "unknown interpolation kind %d", kind);
    const int64_t F = n_frames, big = (int64_t)1 << 53;
    for (int64_t f = 0; f < F; ++f) {
        if (labels[f] < -big || labels[f] > big) return p2s_set_error(P2S_ERR_INVALID_ARG, "label %lld is beyond +-2^53", (long long)labels[f]);
        if (f && labels[f] <= labels[f - 1]) return p2s_set_error(P2S_ERR_INVALID_ARG, "labels must increase (frame %lld)", (long long)f);
    }
    const int K = kind_degree(kind);
    const size_t FC = (size_t)F * n_cols, C = (size_t)n_cols;
    const int64_t tiles = (F + GT - 1) / GT;
    P2sGapArgs a{};
    a.F = F; a.C = n_cols; a.tiles = (int32_t)tiles; a.max_gap = max_gap; a.kind = kind;
    if (!ctx) {                                                   // the same functions on the host
        std::vector<int32_t> ints(4 * FC);
        std::vector<int64_t> totals(C);
        a.in = coords; a.out = out; a.labels = labels; a.status = status; a.totals = totals.data();
        a.rank = ints.data(); a.start = a.rank + FC; a.pos = a.start + FC; a.runlen = a.pos + FC;
        std::fill(status, status + C, 0);
        host_index<GP_INTERP>(a);
        if (!K) {
            for (int64_t f = 0; f < F; ++f)
                for (int c = 0; c < n_cols; ++c) gp_linear_sample(a, f, c);
            return P2S_OK;
        }
        const int64_t cc = spline_chunk_cols(F, n_cols, K, (size_t)P2S_GAPS_WORKSPACE_KB << 10);
        std::vector<double> ws((size_t)F * GP_SLOTS(K) * cc);
        a.ws = ws.data();
        for (int64_t c0 = 0; c0 < n_cols; c0 += cc) {
            a.c0 = (int32_t)c0; a.cc = (int32_t)std::min<int64_t>(cc, n_cols - c0);
            for (int c = a.c0; c < a.c0 + a.cc; ++c) {
                for (int64_t f = 0; f < F; ++f) gp_pack_sample(a, f, c, K);
                gp_solve_column(a, c, K);
                for (int64_t f = 0; f < F; ++f) gp_spline_sample(a, f, c, K);
            }
        }
        return P2S_OK;
    }
    HIP_TRY(hipSetDevice(ctx->device));
    const GapScan sc(F, n_cols, tiles);
    const int64_t cc = K ? spline_chunk_cols(F, n_cols, K, (size_t)ctx->gaps_ws_kb << 10) : 0;
    Layout li;
    const size_t o_rank = li.add(FC * 4), o_start = li.add(FC * 4), o_pos = li.add(FC * 4), o_len = li.add(FC * 4), o_status = li.add(C * 4);
    Stage st{ctx};
    char *words, *ints;
    int64_t *d_labels;
    P2S_TRY(st.upload(a.in, coords, FC * 8));
    P2S_TRY(st.alloc(a.out, FC * 8));
    P2S_TRY(st.upload(d_labels, labels, (size_t)F * 8));
    P2S_TRY(st.alloc(words, sc.words.bytes));
    P2S_TRY(st.up(words + sc.o_foff, sc.frame_off.data(), (C + 1) * 8));
    P2S_TRY(st.alloc(ints, li.bytes));
    if (K) P2S_TRY(st.alloc(a.ws, (size_t)F * GP_SLOTS(K) * cc * sizeof(double)));
    a.labels = d_labels;
    sc.point(a, words);
    a.rank = (int32_t *)(ints + o_rank); a.start = (int32_t *)(ints + o_start); a.pos = (int32_t *)(ints + o_pos);
    a.runlen = (int32_t *)(ints + o_len); a.status = (int32_t *)(ints + o_status);
    HIP_TRY(hipMemsetAsync(a.status, 0, C * 4, ctx->stream));
    P2S_TRY(st.time_begin());
    HIP_TRY(launch_index<GP_INTERP>(a, (const int64_t *)(words + sc.o_foff), ctx->stream));
    if (!K) {
        hipLaunchKernelGGL(gap_linear_kernel, dim3((unsigned)tiles, (unsigned)n_cols), dim3(GT), 0, ctx->stream, a);
        HIP_TRY(hipGetLastError());
    }
    for (int64_t c0 = 0; K && c0 < n_cols; c0 += cc) {            // chunk after chunk through the one workspace
        a.c0 = (int32_t)c0; a.cc = (int32_t)std::min<int64_t>(cc, n_cols - c0);
        HIP_TRY(K == 1 ? launch_spline_chunk<1>(a, ctx->stream) : K == 2 ? launch_spline_chunk<2>(a, ctx->stream) : launch_spline_chunk<3>(a, ctx->stream));
    }
    P2S_TRY(st.time_end());
    P2S_TRY(st.down(out, a.out, FC * 8));
    P2S_TRY(st.down(status, a.status, C * 4));
    return st.finish(P2S_TIMED_GAPS);                             // labels and the offsets are host memory: alive until here
}

int p2s_fill_gaps(p2s_ctx *ctx, int64_t n_frames, int32_t n_cols, const double *coords, int32_t how, double *out) {
    P2S_TRY(gaps_check(n_frames, n_cols, coords, out));
    const int64_t F = n_frames, tiles = (F + GT - 1) / GT;
    const size_t FC = (size_t)F * n_cols, C = (size_t)n_cols;
    if (how != P2S_GAPS_FILL_LAST_VALUE && how != P2S_GAPS_FILL_ZEROS) {      // the gaps stay
        if (out != coords) memcpy(out, coords, FC * 8);
        return P2S_OK;
    }
    P2sGapArgs a{};
    a.F = F; a.C = n_cols; a.tiles = (int32_t)tiles; a.kind = how;
    if (!ctx) {
        std::vector<int32_t> first(C);
        std::vector<int64_t> totals(C);
        a.in = coords; a.out = out; a.first_valid = first.data(); a.totals = totals.data();
        host_index<GP_FILL>(a);
        return P2S_OK;
    }
    HIP_TRY(hipSetDevice(ctx->device));
    const GapScan sc(F, n_cols, tiles);
    Stage st{ctx};
    char *words;
    P2S_TRY(st.upload(a.in, coords, FC * 8));
    P2S_TRY(st.alloc(a.out, FC * 8));
    P2S_TRY(st.alloc(words, sc.words.bytes));
    P2S_TRY(st.up(words + sc.o_foff, sc.frame_off.data(), (C + 1) * 8));
    P2S_TRY(st.alloc(a.first_valid, C * 4));
    sc.point(a, words);
    HIP_TRY(hipMemsetAsync(a.first_valid, 0x7f, C * 4, ctx->stream));          // 0x7f7f7f7f > 2^30 >= F: no valid sample yet
    P2S_TRY(st.time_begin());
    HIP_TRY(launch_index<GP_FILL>(a, (const int64_t *)(words + sc.o_foff), ctx->stream));
    P2S_TRY(st.time_end());
    P2S_TRY(st.down(out, a.out, FC * 8));
    return st.finish(P2S_TIMED_GAPS);
}

int p2s_gap_runs(p2s_ctx *ctx, int64_t n_frames, int32_t n_cols, const double *x, int64_t first, int64_t last, double max_gap,
                 int64_t capacity, int32_t *table, int64_t *count, int32_t *overflow) {
    P2S_TRY(gaps_check(n_frames, n_cols, x, count));
    if (capacity < 0 || (capacity > 0 && !table) || !overflow) return p2s_set_error(P2S_ERR_INVALID_ARG, capacity < 0 ? "negative capacity" : "null argument");
    const int64_t F = n_frames, tiles = (F + GT - 1) / GT;
    const size_t FC = (size_t)F * n_cols, C = (size_t)n_cols;
    P2sGapArgs a{};
    a.F = F; a.C = n_cols; a.tiles = (int32_t)tiles; a.max_gap = max_gap; a.first = first; a.last = last; a.capacity = capacity;
    if (!ctx) {
        std::vector<int64_t> totals(C), base(C + 1, 0);
        a.in = x; a.totals = totals.data(); a.col_base = base.data(); a.table = table;
        host_index<GP_RUNS>(a);
        *count = base[C]; *overflow = base[C] > capacity;
        return P2S_OK;
    }
    HIP_TRY(hipSetDevice(ctx->device));
    const GapScan sc(F, n_cols, tiles);
    Stage st{ctx};
    char *words;
    P2S_TRY(st.upload(a.in, x, FC * 8));
    P2S_TRY(st.alloc(words, sc.words.bytes));
    P2S_TRY(st.up(words + sc.o_foff, sc.frame_off.data(), (C + 1) * 8));
    P2S_TRY(st.alloc(a.col_base, (C + 1) * 8));
    P2S_TRY(st.alloc(a.table, (size_t)capacity * 16));
    sc.point(a, words);
    P2S_TRY(st.time_begin());
    HIP_TRY(launch_index<GP_RUNS>(a, (const int64_t *)(words + sc.o_foff), ctx->stream));
    P2S_TRY(st.time_end());
    int64_t n = 0;
    P2S_TRY(st.down(&n, a.col_base + C, 8));
    HIP_TRY(hipStreamSynchronize(ctx->stream));                   // the count says how much of the table there is to fetch
    P2S_TRY(st.down(table, a.table, (size_t)std::min(n, capacity) * 16));
    P2S_TRY(st.finish(P2S_TIMED_GAPS));
    *count = n; *overflow = n > capacity;
    return P2S_OK;
}

int p2s_gaps_kernel_ms(p2s_ctx *ctx, float *elapsed_ms) {
    return p2s_kernel_ms_query(ctx, P2S_TIMED_GAPS, "none of p2s_interpolate_gaps, p2s_fill_gaps and p2s_gap_runs", elapsed_ms);
}

}  // extern "C"
