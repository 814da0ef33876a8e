// p2s_filter.hip -- zero-phase Butterworth filtering of .trc coordinate columns and the trc_evaluate quality metrics
// on gfx950 (the first consumer of the triangulation's output).
//
// p2s_butter_kernel: filtering.py:437-471 (butterworth_filter_1d) for every column at once.  A column is cut into its
// runs of valid samples (not NaN, not 0); a run longer than padlen goes through scipy.signal.filtfilt's algorithm
// (odd extension by padlen samples at either end, forward pass of the IIR filter in direct form II transposed with
// the steady-state initial condition scaled by the first sample, backward pass likewise, extension dropped), every
// other sample is copied.  The recurrence is sequential in time, so the parallel axis is the column: one lane per
// column, consecutive lanes = consecutive columns of the row-major [frame][column] matrix, i.e. coalesced loads
// while the columns' runs coincide (they do after triangulate_all's gap filling).  Latency-bound on the recurrence
// (2 passes x ~6 dependent fp64 operations per sample): a few ms for 100k frames, whatever the number of columns up
// to the chip's 16k resident lanes; HBM traffic is 5 x 8 B per sample and irrelevant.
//
// The other filter types of filtering.py have their kernels further down, each with its own comment: Hampel, Gaussian,
// median and LOESS (p2s_loess_kernel: local linear regression, filtering.py:532-558) one thread per element, one-euro
// and Kalman one lane per column, gcv_spline one lane per run.  With LOESS the stage has no filter type left out.
//
// p2s_trc_metrics_kernel: Utilities/trc_evaluate.py:114-228 -- per-frame bone lengths and second-difference
// magnitudes written out for the host's order statistics, sums for means and standard deviations, missing counts.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <math.h>

#include <algorithm>
#include <cmath>
#include <cstring>
#include <vector>

#include "p2s_ctx.h"
#include "p2s_iir.h"

struct P2sFilterArgs {
    const double *in;            // [n_frames][n_cols]
    double *out;                 // [n_frames][n_cols]
    double *work;                // [n_frames + 2 padlen][n_cols] forward-pass output
    int64_t n_frames;
    int32_t n_cols, n_order, padlen;   // n_order = len(b) - 1
    double b[P2S_MAX_FILTER_ORDER + 1], a[P2S_MAX_FILTER_ORDER + 1], zi[P2S_MAX_FILTER_ORDER];
};

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

// loess_filter_1d: local linear regression over the k nearest samples of a run
struct P2sLoessArgs {
    const double *in;            // [n_frames][n_cols]
    double *out;                 // [n_frames][n_cols]
    const double *wn;            // [k / 2] the interior window's normalised tricube weights by distance (device)
    int64_t n_frames, min_run;   // runs of at least min_run samples are filtered
    int32_t n_cols, k;
};

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

namespace {

__device__ __forceinline__ bool sample_valid(double v) { return (v == v) && (v != 0.0); }

template <int N>
__global__ void __launch_bounds__(64) p2s_butter_kernel(const P2sFilterArgs a) {
    const int col = blockIdx.x * 64 + threadIdx.x;
    if (col >= a.n_cols) return;
    const int64_t F = a.n_frames, S = a.n_cols;
    const double *in = a.in + col;
    double *out = a.out + col;
    double *work = a.work + col;
    const int64_t pad = a.padlen;
    int64_t f = 0;
    while (f < F) {
        const double v = in[f * S];
        if (!sample_valid(v)) { out[f * S] = v; ++f; continue; }
        int64_t r = f + 1;                                     // the run [f, r) of valid samples
        while (r < F && sample_valid(in[r * S])) ++r;
        const int64_t L = r - f;
        if (L <= pad) {                                        // filtering.py:466: only runs longer than padlen
            for (int64_t i = f; i < r; ++i) out[i * S] = in[i * S];
            f = r;
            continue;
        }
        // scipy.signal.filtfilt(b, a, x) with its defaults: padtype 'odd', padlen = 3 max(len(a), len(b))
        const double *x = in + f * S;
        const double x0 = x[0], xl = x[(L - 1) * S];
        const int64_t E = L + 2 * pad;
        auto ext = [&](int64_t i) -> double {
            if (i < pad) return 2.0 * x0 - x[(pad - i) * S];
            if (i < pad + L) return x[(i - pad) * S];
            return 2.0 * xl - x[(L - 2 - (i - pad - L)) * S];
        };
        double z[N];
        const double e0 = ext(0);
#pragma unroll
        for (int k = 0; k < N; ++k) z[k] = a.zi[k] * e0;
        for (int64_t i = 0; i < E; ++i) work[i * S] = iir_step<N>(a.b, a.a, z, ext(i));
        const double y0 = work[(E - 1) * S];
#pragma unroll
        for (int k = 0; k < N; ++k) z[k] = a.zi[k] * y0;
        for (int64_t i = E - 1; i >= 0; --i) {
            const double y = iir_step<N>(a.b, a.a, z, work[i * S]);
            if (i >= pad && i < pad + L) out[(f + i - pad) * S] = y;
        }
        f = r;
    }
}

// ---------------------------------------------------------------------------------------------------------------------
// The other column filters of filtering.py.  Hampel, Gaussian and median look at a fixed window of the INPUT around every
// sample: one thread per (frame, column) element, consecutive threads = consecutive columns of a row (coalesced).  The
// one-euro filter is a recurrence like the Butterworth one: one lane per column.

// hampel_filter (filtering.py:63-85): 7-sample window, median and median absolute deviation; the sample is replaced by
// the median when 0.6745 |x - median| / mad > n_sigma.  np.median of a window that holds a NaN is NaN, the comparison
// with it is false and the sample stays; the first and last window / 2 samples are never looked at.
__device__ __forceinline__ void sort2(double &a, double &b) { const double lo = fmin(a, b), hi = fmax(a, b); a = lo; b = hi; }

__device__ __forceinline__ double median7(double v0, double v1, double v2, double v3, double v4, double v5, double v6) {
    // the 4th smallest of 7 (no NaN among them) by a sorting network
    sort2(v0, v4); sort2(v1, v5); sort2(v2, v6); sort2(v0, v2); sort2(v1, v3); sort2(v4, v6); sort2(v2, v4); sort2(v3, v5);
    sort2(v0, v1); sort2(v2, v3); sort2(v4, v5); sort2(v1, v4); sort2(v3, v6); sort2(v1, v2); sort2(v3, v4); sort2(v5, v6);
    return v3;
}

__global__ void __launch_bounds__(256) p2s_hampel_kernel(const P2sColFilterArgs a) {
#pragma clang fp contract(off)
    const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int64_t total = a.n_frames * a.n_cols;
    if (idx >= total) return;
    const int64_t S = a.n_cols, f = idx / S;
    const double x = a.in[idx];
    double y = x;
    if (f >= 3 && f < a.n_frames - 3) {
        const double *p = a.in + idx;
        const double w0 = p[-3 * S], w1 = p[-2 * S], w2 = p[-S], w4 = p[S], w5 = p[2 * S], w6 = p[3 * S];
        const bool any_nan = !(w0 == w0) || !(w1 == w1) || !(w2 == w2) || !(x == x) || !(w4 == w4) || !(w5 == w5) || !(w6 == w6);
        if (!any_nan) {
            const double med = median7(w0, w1, w2, x, w4, w5, w6);
            const double mad = median7(fabs(w0 - med), fabs(w1 - med), fabs(w2 - med), fabs(x - med), fabs(w4 - med), fabs(w5 - med),
                                       fabs(w6 - med));
            if (mad != 0.0) {
                const double z = 0.6745 * (x - med) / mad;
                if (fabs(z) > a.p[0]) y = med;
            }
        }
    }
    a.out[idx] = y;
}

// gaussian_filter_1d (filtering.py:513-529) = scipy.ndimage.correlate1d(col, weights, mode='reflect') with the weights of
// scipy's own _gaussian_kernel1d (computed by the host with the same call): centre tap first, then the pairs from the
// far end inwards, as scipy's loop for a symmetric kernel adds them.  A NaN spreads over its whole neighbourhood.
__global__ void __launch_bounds__(256) p2s_gauss_kernel(const P2sColFilterArgs a) {
#pragma clang fp contract(off)
    const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int64_t total = a.n_frames * a.n_cols;
    if (idx >= total) return;
    const int64_t S = a.n_cols, F = a.n_frames, f = idx / S, c = idx - f * S;
    const int r = a.radius;
    auto at = [&](int64_t i) -> double {                       // 'reflect': d c b a | a b c d | d c b a
        while (i < 0 || i >= F) i = (i < 0) ? -i - 1 : 2 * F - 1 - i;
        return a.in[i * S + c];
    };
    double acc = a.in[idx] * a.w[r];
    for (int k = -r; k < 0; ++k) acc += (at(f + k) + at(f - k)) * a.w[k + r];
    a.out[idx] = acc;
}

// median_filter_1d (filtering.py:561-577) = scipy.signal.medfilt = ndimage.rank_filter(rank k / 2, mode='constant'): the
// window is padded with zeros beyond the ends.  The median is the window element with as many smaller ones as its rank
// allows (k is small: 3 to 15 in practice; windows are read through the cache).  Columns with NaN are refused by the host.
__global__ void __launch_bounds__(256) p2s_median_kernel(const P2sColFilterArgs a) {
    const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int64_t total = a.n_frames * a.n_cols;
    if (idx >= total) return;
    const int64_t S = a.n_cols, F = a.n_frames, f = idx / S, c = idx - f * S;
    const int r = a.radius, want = r;                           // rank k / 2 of k = 2 r + 1
    auto at = [&](int64_t i) -> double { return (i < 0 || i >= F) ? 0.0 : a.in[i * S + c]; };
    double med = 0.0;
    for (int i = -r; i <= r; ++i) {
        const double v = at(f + i);
        int less = 0, eq = 0;
        for (int j = -r; j <= r; ++j) {
            const double u = at(f + j);
            less += (u < v) ? 1 : 0;
            eq += (u == v) ? 1 : 0;
        }
        if (less <= want && want < less + eq) med = v;
    }
    a.out[idx] = med;
}

// loess_filter_1d (filtering.py:532-558) = statsmodels' lowess(run, frame_indices, frac=nb/L, it=0, delta=0) on every run
// of consecutive non-NaN samples (zeros are data) that is long enough: at sample i the weighted least-squares line
// through the k run samples nearest to i, evaluated at i.  The k nearest samples of equally spaced abscissae are a
// contiguous block [l, l + k) of the run, l = i - k / 2 clamped to the run; with h = max(i - l, l + k - 1 - i) the
// weights are the tricube (1 - (|j - i| / h)^3)^3.  Which of two equally distant neighbours statsmodels keeps only
// decides whether a sample at distance exactly h is in the window, and its weight is exactly 0: the fit does not depend
// on it.  A fit with a single non-zero weight (k = 2) returns the sample.  statsmodels is not importable where this was
// built and has never run here; this follows its published algorithm, and is checked against goldens recorded through
// the reference's own loess_filter_1d with a stand-in for lowess, and against a 60-digit solve of the definition
// (tests/golden/loess_units.npz).
//
// One thread per element, as for the other window filters.  The sums are taken in abscissae centred on the sample,
// u = j - i (statsmodels' sums over the frame indices themselves lose about frame index x eps).  Away from the ends of
// its run the window is symmetric, the slope term vanishes and the fit is a fixed FIR filter: its normalised weights
// come from the host (wn), pairs added from the far end inwards.
__host__ __device__ __forceinline__ double loess_tricube(double d, double h) {
#pragma clang fp contract(off)
    const double r = d / h;
    const double t = 1.0 - r * r * r;
    return t * t * t;
}

// the filtered value of element idx = frame * n_cols + column
__host__ __device__ __forceinline__ double loess_at(const P2sLoessArgs &a, int64_t idx) {
#pragma clang fp contract(off)
    const int64_t S = a.n_cols, F = a.n_frames, f = idx / S;
    const double *p = a.in + idx;                              // p[u * S]: the sample u frames on
    const double x = *p;
    if (!(x == x)) return x;
    // valid samples before and after this one, counted as far as the decisions below need them
    const int64_t cap = a.min_run - 1;
    int64_t before = 0, after = 0;
    while (before < cap && f - before > 0 && p[-(before + 1) * S] == p[-(before + 1) * S]) ++before;
    const int64_t k = a.k, m = k / 2;
    int64_t lo = before < m ? -before : -m;                    // the window [lo, lo + k) in u, clamped to the run's start
    const int64_t need = lo + k - 1 > cap - before ? lo + k - 1 : cap - before;
    while (after < need && f + after < F - 1 && p[(after + 1) * S] == p[(after + 1) * S]) ++after;
    if (before + after + 1 < a.min_run) return x;              // a run too short to be filtered
    if (lo + k - 1 > after) lo = after - (k - 1);              // clamped to the run's end
    const int64_t hi = lo + k - 1;
    if (lo == -m) {                                            // symmetric: non-zero weights on |u| <= m - 1
        double acc = 0.0;
        for (int64_t d = m - 1; d >= 1; --d) acc += (p[-d * S] + p[d * S]) * a.wn[d];
        return acc + x * a.wn[0];
    }
    const int64_t h = -lo > hi ? -lo : hi;
    const double hd = (double)h;
    double s0 = 0.0, s1 = 0.0, s2 = 0.0, t0 = 0.0, t1 = 0.0;
    int nonzero = 0;
    for (int64_t u = lo; u <= hi; ++u) {
        const int64_t d = u < 0 ? -u : u;
        if (d >= h) continue;                                  // weight exactly 0
        const double w = loess_tricube((double)d, hd), du = (double)u, v = p[u * S];
        const double wu = w * du;
        s0 += w; s1 += wu; s2 += wu * du;
        t0 += w * v; t1 += wu * v;
        ++nonzero;
    }
    if (nonzero < 2) return x;
    const double ubar = s1 / s0, ybar = t0 / s0;
    const double sxx = s2 - s1 * ubar, sxy = t1 - ubar * t0;
    return ybar - (sxy / sxx) * ubar;                          // the line at u = 0
}

__global__ void __launch_bounds__(256) p2s_loess_kernel(const P2sLoessArgs a) {
    const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (idx >= a.n_frames * a.n_cols) return;
    a.out[idx] = loess_at(a, idx);
}

// one_euro_filter_1d (filtering.py:87-160): every run of at least two samples that are not NaN goes through the adaptive
// first-order low-pass forwards, and the result through it again backwards; p = {dt, min_cutoff, beta, d_cutoff}.
__device__ __forceinline__ double one_euro_alpha(double dt, double cutoff) {
#pragma clang fp contract(off)
    const double r = 2 * 3.141592653589793 * cutoff * dt;
    return r / (r + 1);
}

__global__ void __launch_bounds__(64) p2s_one_euro_kernel(const P2sColFilterArgs a) {
#pragma clang fp contract(off)
    const int col = blockIdx.x * 64 + threadIdx.x;
    if (col >= a.n_cols) return;
    const int64_t F = a.n_frames, S = a.n_cols;
    const double *in = a.in + col;
    double *out = a.out + col;
    double *work = a.work + col;
    const double dt = a.p[0], min_cutoff = a.p[1], beta = a.p[2], d_cutoff = a.p[3];
    const double alpha_d = one_euro_alpha(dt, d_cutoff);
    int64_t f = 0;
    while (f < F) {
        const double v = in[f * S];
        if (!(v == v)) { out[f * S] = v; ++f; continue; }
        int64_t r = f + 1;
        while (r < F && (in[r * S] == in[r * S])) ++r;
        const int64_t L = r - f;
        if (L < 2) { out[f * S] = v; f = r; continue; }
        double x_prev = v, dx_prev = 0.0;
        work[f * S] = v;
        for (int64_t i = f + 1; i < r; ++i) {                  // forward pass
            const double x = in[i * S];
            const double dx = (x - x_prev) / dt;
            const double dx_hat = alpha_d * dx + (1 - alpha_d) * dx_prev;
            const double alpha = one_euro_alpha(dt, min_cutoff + beta * fabs(dx_hat));
            const double x_hat = alpha * x + (1 - alpha) * x_prev;
            work[i * S] = x_hat;
            x_prev = x_hat; dx_prev = dx_hat;
        }
        x_prev = work[(r - 1) * S]; dx_prev = 0.0;
        out[(r - 1) * S] = x_prev;
        for (int64_t i = r - 2; i >= f; --i) {                 // backward pass over the forward result
            const double x = work[i * S];
            const double dx = (x - x_prev) / dt;
            const double dx_hat = alpha_d * dx + (1 - alpha_d) * dx_prev;
            const double alpha = one_euro_alpha(dt, min_cutoff + beta * fabs(dx_hat));
            const double x_hat = alpha * x + (1 - alpha) * x_prev;
            out[i * S] = x_hat;
            x_prev = x_hat; dx_prev = dx_hat;
        }
        f = r;
    }
}

// ---------------------------------------------------------------------------------------------------------------------
// kalman_filter_1d (filtering.py:316-434): constant-acceleration Kalman filter of one coordinate (state position, velocity,
// acceleration; the measurement is the position) over every run of >= 4 samples that are neither NaN nor 0, then the
// Rauch-Tung-Striebel smoother.  The reference builds it from filterpy (KalmanFilter.batch_filter: predict, then update in
// Joseph form, per sample; rts_smoother) -- filterpy is not importable here, so this follows its published algorithm.  It
// is checked against goldens recorded through the reference's own set-up code with a stand-in for filterpy's recursion,
// and against an exact multiprecision solve of the model (tests/golden/kalman_units.npz).  The initial state is
// [z0, z1 - z0, z2 - 2 z1 + z0]: the reference differentiates with dt = 1 (:342-351), the differences are NOT divided by
// the frame period.  One lane per column; the forward pass leaves its means and covariances (12 doubles per sample) in
// `work` for the smoother.
struct M3 { double m[9]; };
__device__ __forceinline__ M3 mul3(const M3 &A, const M3 &B) {
    M3 C;
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) C.m[3 * i + j] = A.m[3 * i] * B.m[j] + A.m[3 * i + 1] * B.m[3 + j] + A.m[3 * i + 2] * B.m[6 + j];
    return C;
}
__device__ __forceinline__ M3 transpose3(const M3 &A) {
    M3 T;
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) T.m[3 * i + j] = A.m[3 * j + i];
    return T;
}
__device__ __forceinline__ M3 inverse3(const M3 &A) {
    const double *a = A.m;
    const double c00 = a[4] * a[8] - a[5] * a[7], c01 = a[5] * a[6] - a[3] * a[8], c02 = a[3] * a[7] - a[4] * a[6];
    const double id = 1.0 / (a[0] * c00 + a[1] * c01 + a[2] * c02);
    M3 R;
    R.m[0] = c00 * id; R.m[1] = (a[2] * a[7] - a[1] * a[8]) * id; R.m[2] = (a[1] * a[5] - a[2] * a[4]) * id;
    R.m[3] = c01 * id; R.m[4] = (a[0] * a[8] - a[2] * a[6]) * id; R.m[5] = (a[2] * a[3] - a[0] * a[5]) * id;
    R.m[6] = c02 * id; R.m[7] = (a[1] * a[6] - a[0] * a[7]) * id; R.m[8] = (a[0] * a[4] - a[1] * a[3]) * id;
    return R;
}

__global__ void __launch_bounds__(64) p2s_kalman_kernel(const P2sColFilterArgs a) {
    const int col = blockIdx.x * 64 + threadIdx.x;
    if (col >= a.n_cols) return;
    const int64_t F = a.n_frames, S = a.n_cols;
    const double *in = a.in + col;
    double *out = a.out + col;
    double *work = a.work + (size_t)col * 12;                          // [frame][col][12]
    const int64_t WS = S * 12;
    const double dt = a.p[0], meas = a.p[1], proc = a.p[2];
    const bool smooth = a.p[3] != 0.0;
    const M3 Fm{{1.0, dt, dt * dt / 2, 0.0, 1.0, dt, 0.0, 0.0, 1.0}};                              // :355-359
    const M3 Ft = transpose3(Fm);
    const double var = proc * proc, R = meas * meas;
    const M3 Q{{.25 * dt * dt * dt * dt * var, .5 * dt * dt * dt * var, .5 * dt * dt * var,        // Q_discrete_white_noise(3, dt, var)
                .5 * dt * dt * dt * var, dt * dt * var, dt * var,
                .5 * dt * dt * var, dt * var, var}};
    auto usable = [](double v) { return (v == v) && (v != 0.0); };     // :421
    int64_t f = 0;
    while (f < F) {
        const double v = in[f * S];
        if (!usable(v)) { out[f * S] = v; ++f; continue; }
        int64_t r = f + 1;
        while (r < F && usable(in[r * S])) ++r;
        if (r - f < 4) {                                               // :428: shorter runs stay as they are
            for (int64_t i = f; i < r; ++i) out[i * S] = in[i * S];
            f = r;
            continue;
        }
        // initial state: first and second difference of the first three samples, undivided (:342-351, derivate_array's
        // default dt = 1); covariance I * measurement_noise (:376)
        const double z0 = in[f * S], z1 = in[(f + 1) * S], z2 = in[(f + 2) * S];
        double x0 = z0, x1 = z1 - z0, x2 = (z2 - z1) - (z1 - z0);
        M3 P{{meas, 0.0, 0.0, 0.0, meas, 0.0, 0.0, 0.0, meas}};
        for (int64_t i = f; i < r; ++i) {
            // predict: x = F x, P = F P F^T + Q
            const double p0 = x0 + dt * x1 + (dt * dt / 2) * x2, p1 = x1 + dt * x2, p2 = x2;
            M3 Pp = mul3(mul3(Fm, P), Ft);
#pragma unroll
            for (int k = 0; k < 9; ++k) Pp.m[k] += Q.m[k];
            // update with z (H = [1 0 0]): K = P H^T / (H P H^T + R), x += K (z - x0), P = (I - K H) P (I - K H)^T + K R K^T
            const double y = in[i * S] - p0;
            const double Sinv = 1.0 / (Pp.m[0] + R);
            const double k0 = Pp.m[0] * Sinv, k1 = Pp.m[3] * Sinv, k2 = Pp.m[6] * Sinv;
            x0 = p0 + k0 * y; x1 = p1 + k1 * y; x2 = p2 + k2 * y;
            const M3 IKH{{1.0 - k0, 0.0, 0.0, -k1, 1.0, 0.0, -k2, 0.0, 1.0}};
            P = mul3(mul3(IKH, Pp), transpose3(IKH));
            const double kk[3] = {k0, k1, k2};
#pragma unroll
            for (int u = 0; u < 3; ++u)
#pragma unroll
                for (int w = 0; w < 3; ++w) P.m[3 * u + w] += kk[u] * R * kk[w];
            double *wk = work + i * WS;
            wk[0] = x0; wk[1] = x1; wk[2] = x2;
#pragma unroll
            for (int k = 0; k < 9; ++k) wk[3 + k] = P.m[k];
            if (!smooth) out[i * S] = x0;
        }
        if (smooth) {
            // rts_smoother: from the last sample backwards, x[k] += K (x[k+1] - F x[k]), P[k] += K (P[k+1] - Pp) K^T with
            // Pp = F P[k] F^T + Q and K = P[k] F^T Pp^-1
            double n0 = x0, n1 = x1, n2 = x2;                          // smoothed state and covariance of sample k + 1
            M3 Pn = P;
            out[(r - 1) * S] = n0;
            for (int64_t i = r - 2; i >= f; --i) {
                const double *wk = work + i * WS;
                const double c0 = wk[0], c1 = wk[1], c2 = wk[2];
                M3 Pk;
#pragma unroll
                for (int k = 0; k < 9; ++k) Pk.m[k] = wk[3 + k];
                M3 Pp = mul3(mul3(Fm, Pk), Ft);
#pragma unroll
                for (int k = 0; k < 9; ++k) Pp.m[k] += Q.m[k];
                const M3 K = mul3(mul3(Pk, Ft), inverse3(Pp));
                const double d0 = n0 - (c0 + dt * c1 + (dt * dt / 2) * c2), d1 = n1 - (c1 + dt * c2), d2 = n2 - c2;
                n0 = c0 + K.m[0] * d0 + K.m[1] * d1 + K.m[2] * d2;
                n1 = c1 + K.m[3] * d0 + K.m[4] * d1 + K.m[5] * d2;
                n2 = c2 + K.m[6] * d0 + K.m[7] * d1 + K.m[8] * d2;
                M3 D;
#pragma unroll
                for (int k = 0; k < 9; ++k) D.m[k] = Pn.m[k] - Pp.m[k];
                const M3 U = mul3(mul3(K, D), transpose3(K));
#pragma unroll
                for (int k = 0; k < 9; ++k) Pn.m[k] = Pk.m[k] + U.m[k];
                out[i * S] = n0;
            }
        }
        f = r;
    }
}

// ---------------------------------------------------------------------------------------------------------------------
// trc_evaluate: one workgroup per bone (blocks [0, n_bones)) or per marker (blocks [n_bones, n_bones + n_markers)).
__global__ void __launch_bounds__(256) p2s_trc_metrics_kernel(const P2sMetricsArgs a) {
    __shared__ double s_sum[256];
    __shared__ unsigned long long s_cnt[256];
    const int tid = threadIdx.x;
    const int64_t F = a.n_frames;
    const int K = a.n_markers;
    if ((int)blockIdx.x < a.n_bones) {
        // compute_bone_lengths (:114-156): |child - parent| per frame, 0 -> NaN; mean and population standard deviation
        // of the valid lengths (two passes over the frames: the deviations are taken from the final mean, as np.nanstd)
        const int bi = blockIdx.x;
        const int p = a.bones[2 * bi], c = a.bones[2 * bi + 1];
        double *len = a.bone_len + (int64_t)bi * F;
        double sum = 0.0;
        unsigned long long cnt = 0;
        for (int64_t f = tid; f < F; f += 256) {
            const double *P = a.xyz + (f * K + p) * 3, *C = a.xyz + (f * K + c) * 3;
            const double dx = C[0] - P[0], dy = C[1] - P[1], dz = C[2] - P[2];
            double l = sqrt(dx * dx + dy * dy + dz * dz);
            if (l == 0.0) l = __builtin_nan("");
            len[f] = l;
            if (l == l) { sum += l; ++cnt; }
        }
        s_sum[tid] = sum; s_cnt[tid] = cnt;
        __syncthreads();
        for (int o = 128; o > 0; o >>= 1) {
            if (tid < o) { s_sum[tid] += s_sum[tid + o]; s_cnt[tid] += s_cnt[tid + o]; }
            __syncthreads();
        }
        const unsigned long long n = s_cnt[0];
        const double mean = n ? s_sum[0] / (double)n : __builtin_nan("");
        __syncthreads();
        double dev = 0.0;
        for (int64_t f = tid; f < F; f += 256) {
            const double l = len[f];
            if (l == l) dev += (l - mean) * (l - mean);
        }
        s_sum[tid] = dev;
        __syncthreads();
        for (int o = 128; o > 0; o >>= 1) {
            if (tid < o) s_sum[tid] += s_sum[tid + o];
            __syncthreads();
        }
        if (tid == 0) {
            a.bone_stats[3 * bi + 0] = mean;
            a.bone_stats[3 * bi + 1] = n ? sqrt(s_sum[0] / (double)n) : __builtin_nan("");
            a.bone_stats[3 * bi + 2] = (double)n;
        }
        return;
    }
    // compute_smoothness (:159-207) and compute_missing_data (:210-238) of one marker
    const int m = blockIdx.x - a.n_bones;
    if (m >= K) return;
    double *acc = a.accel + (int64_t)m * (F > 2 ? F - 2 : 0);
    unsigned long long missing = 0;
    for (int64_t f = tid; f < F; f += 256) {
        const double *p0 = a.xyz + (f * K + m) * 3;
        if (!(p0[0] == p0[0]) || !(p0[1] == p0[1]) || !(p0[2] == p0[2])) ++missing;
        if (f + 2 < F) {
            const double *p1 = p0 + (int64_t)K * 3, *p2 = p1 + (int64_t)K * 3;
            const double ax = p2[0] - 2 * p1[0] + p0[0], ay = p2[1] - 2 * p1[1] + p0[1], az = p2[2] - 2 * p1[2] + p0[2];
            acc[f] = sqrt(ax * ax + ay * ay + az * az);
        }
    }
    s_cnt[tid] = missing;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if (tid < o) s_cnt[tid] += s_cnt[tid + o];
        __syncthreads();
    }
    if (tid == 0) a.missing[m] = (int64_t)s_cnt[0];
}

// ---------------------------------------------------------------------------------------------------------------------
// gcv_spline_filter_1d (filtering.py:163-313): natural cubic smoothing spline of every run of >= 5 valid samples, with
// lambda either fixed or chosen by generalised cross-validation (scipy.interpolate.make_smoothing_spline).
//
// The samples sit at x = 0, 1, ..., n - 1.  The spline is written in the cubic B-spline basis on the knots x with
// four-fold end knots; the natural end conditions s''(x_0) = s''(x_{n-1}) = 0 fix the two outermost B-spline
// coefficients at either end from their neighbours, which leaves n free coefficients c (Wahba 1990, ch. 2; the change
// of basis is make_smoothing_spline's documented one).  In that basis
//   X  [n][n]  the spline's values at the samples (s = X c): the uniform cubic B-spline's 1/6, 2/3, 1/6 on three
//              diagonals, and at either end the basis functions that absorbed the boundary coefficients
//   E  [n][n]  the penalty: Wahba's divided-difference form, 6 (x_{j+2} - x_{j-2}) [x_{j-2}..x_{j+2}] on column j,
//              i.e. the fourth difference 1 -4 6 -4 1, with the 3- and 4-point divided differences in the two
//              outermost columns at either end (unit weights, so W^-1 E = E)
// and the coefficients of lambda solve the 5-band, non-symmetric system (X + lambda E) c = y.  GCV(lambda) =
// (|lambda E c|^2 / n) / (1 - tr(A) / n)^2 (Wahba 1990, 4.3; Craven & Wahba 1979); the trace of the influence matrix A
// is sum_ij B_ij (X^T X)_ij with B = (X^T X + lambda X^T E)^-1 needed on its three central bands only, which Hutchinson
// & de Hoog (1985) get from the banded Cholesky factor U^T D^-1 U by a backward recurrence.  lambda minimises GCV on
// (0, n) by scipy.optimize.minimize_scalar(method='bounded') (Brent's method with golden-section start, xatol 1e-5,
// 500 evaluations at most).
//
// Operation order follows what scipy calls: the 5-band solve is LAPACK gbsv (unblocked band LU with partial pivoting on
// the first largest |pivot|, multipliers by the reciprocal pivot, then the column-oriented band back-substitution),
// the Cholesky factor is pbtrf('U') (reciprocal scaling, rank-1 trailing updates), the band products of X^T X and
// X^T E are summed row by row, and no operation is contracted into an FMA.  Sums over the samples (the trace, |E c|^2)
// run backwards here, so the GCV values agree with scipy's to rounding, not bit for bit.
//
// One lane per run: the search is sequential in lambda and an evaluation is sequential in the samples.  An evaluation
// is two sweeps over the run: forwards, the LU of X + lambda E with the elimination of y and, independent of it, the
// Cholesky factorisation of X^T X + lambda X^T E (both in registers over a sliding window, the bands computed on the
// fly); backwards, the back-substitution with |lambda E c|^2 and, again independent, the inverse-band recurrence with
// the trace.  The factors the backward sweep needs (U row of the LU, eliminated y, normalised Cholesky row and D) are
// the 10 slots per sample the forward sweep leaves in `work`; slot 10 holds the run's (normalised) samples.
namespace gcv {

constexpr double kSixth = 0x1.5555555555555p-3, kTwoThirds = 0x1.5555555555555p-1;   // 1/6, 2/3 rounded
constexpr double kEdge = kSixth + kTwoThirds;                                           // B_1 + B_2 at x_1
constexpr double kSqrtEps = 0x1.fda324be34921p-27;          // sqrt(2.2e-16), minimize_scalar's constant
constexpr double kGolden = 0x1.8722191a02d60p-2;            // 0.5 (3 - sqrt(5))
constexpr double kXatol = 1e-5;
constexpr int kMaxFun = 500;
enum { kU0 = 0, kYe = 5, kC1 = 6, kD = 9, kY = 10 };          // work slots

// X[r][c]: column c's basis function at sample r (nonzero for |r - c| <= 1)
__host__ __device__ __forceinline__ double xb(int64_t r, int64_t c, int64_t n) {
    const int64_t d = r - c;
    if (r < 0 || r >= n || c < 0 || c >= n || d < -1 || d > 1) return 0.0;
    if (c >= 2 && c <= n - 3) return d == 0 ? kTwoThirds : kSixth;
    if (c == 0) return d == 0 ? 3.0 : 0.5;
    if (c == n - 1) return d == 0 ? 3.0 : 0.5;
    if (c == 1) return d == -1 ? 1.0 : (d == 0 ? kEdge : kSixth);
    return d == 1 ? 1.0 : (d == 0 ? kEdge : kSixth);                 // c == n - 2
}

// E[r][c]: the penalty (nonzero for |r - c| <= 2)
__host__ __device__ __forceinline__ double eb(int64_t r, int64_t c, int64_t n) {
    const int64_t d = r - c;
    if (r < 0 || r >= n || c < 0 || c >= n || d < -2 || d > 2) return 0.0;
    if (c >= 2 && c <= n - 3) return d == 0 ? 6.0 : ((d == 1 || d == -1) ? -4.0 : 1.0);
    if (c == 0) return d == 0 ? 3.0 : (d == 1 ? -6.0 : (d == 2 ? 3.0 : 0.0));
    if (c == n - 1) return d == 0 ? 3.0 : (d == -1 ? -6.0 : (d == -2 ? 3.0 : 0.0));
    if (c == 1) return d == -1 ? -1.0 : (d == 0 ? 3.0 : (d == 1 ? -3.0 : (d == 2 ? 1.0 : 0.0)));
    return d == -2 ? 1.0 : (d == -1 ? -3.0 : (d == 0 ? 3.0 : (d == 1 ? -1.0 : 0.0)));   // c == n - 2
}

// (X^T X)[i][i + j] and (X^T E)[i][i + j], j = 0..3, summed over the rows in ascending order
__host__ __device__ __forceinline__ double xtx(int64_t i, int j, int64_t n) {
#pragma clang fp contract(off)
    if (i + j >= n) return 0.0;
    double s = 0.0;
    for (int k = j; k < 5; ++k) s = s + xb(i + k - 2, i, n) * xb(i + k - 2, i + j, n);
    return s;
}
__host__ __device__ __forceinline__ double xte(int64_t i, int j, int64_t n) {
#pragma clang fp contract(off)
    if (i + j >= n) return 0.0;
    double s = 0.0;
    for (int k = j; k < 5; ++k) s = s + xb(i + k - 2, i, n) * eb(i + k - 2, i + j, n);
    return s;
}

struct Lane {
    double *w;                   // slot k of sample i at w[i * ss + k * ks]
    int64_t ss, ks, n;
    double xx[4], xe[4];         // the interior values of the two band products
    __host__ __device__ double &at(int64_t i, int k) const { return w[i * ss + k * ks]; }
    __host__ __device__ double XX(int64_t i, int j) const { return (i >= 2 && i + j <= n - 3) ? xx[j] : xtx(i, j, n); }
    __host__ __device__ double XE(int64_t i, int j) const { return (i >= 2 && i + j <= n - 3) ? xe[j] : xte(i, j, n); }
};

__host__ __device__ inline void lane_init(Lane &L) {
    for (int j = 0; j < 4; ++j) { L.xx[j] = xtx(4, j, 12); L.xe[j] = xte(4, j, 12); }
}

// Forward sweep for one lambda: LU of X + lambda E with the elimination of y (slot kY) -> U rows and eliminated y; with
// kChol also the Cholesky factor of X^T X + lambda X^T E -> U_ij / U_ii (j = i+1..i+3) and D_i = 1 / U_ii^2.
template <bool kChol>
__host__ __device__ int forward(const Lane &L, double lam) {
#pragma clang fp contract(off)
    const int64_t n = L.n;
    auto M = [&](int64_t r, int64_t c) { return xb(r, c, n) + lam * eb(r, c, n); };
    auto A = [&](int64_t i, int j) { return L.XX(i, j) + lam * L.XE(i, j); };
    double R0[5], R1[5], R2[5];                       // rows j, j+1, j+2 over columns j..j+4
    for (int k = 0; k < 5; ++k) { R0[k] = M(0, k); R1[k] = M(1, k); R2[k] = M(2, k); }
    double y0 = L.at(0, kY), y1 = L.at(1, kY), y2 = L.at(2, kY);
    // Cholesky window: the partly updated upper triangle of rows/columns j..j+3
    double w00 = 0, w01 = 0, w02 = 0, w03 = 0, w11 = 0, w12 = 0, w13 = 0, w22 = 0, w23 = 0, w33 = 0;
    if (kChol) {
        w00 = A(0, 0); w01 = A(0, 1); w02 = A(0, 2); w03 = A(0, 3);
        w11 = A(1, 0); w12 = A(1, 1); w13 = A(1, 2); w22 = A(2, 0); w23 = A(2, 1); w33 = A(3, 0);
    }
    for (int64_t j = 0; j < n; ++j) {
        // LU, column j: pivot = first largest |.| among the rows j..j+km
        const int64_t km = (n - 1 - j) < 2 ? (n - 1 - j) : 2;
        int p = 0;
        double amax = fabs(R0[0]);
        if (km >= 1 && fabs(R1[0]) > amax) { p = 1; amax = fabs(R1[0]); }
        if (km >= 2 && fabs(R2[0]) > amax) p = 2;
        if (p == 1) {
            for (int k = 0; k < 5; ++k) { const double t = R0[k]; R0[k] = R1[k]; R1[k] = t; }
            const double t = y0; y0 = y1; y1 = t;
        } else if (p == 2) {
            for (int k = 0; k < 5; ++k) { const double t = R0[k]; R0[k] = R2[k]; R2[k] = t; }
            const double t = y0; y0 = y2; y2 = t;
        }
        if (R0[0] == 0.0) return P2S_GCV_SINGULAR;
        const double rinv = 1.0 / R0[0];
        const double l1 = R1[0] * rinv, l2 = R2[0] * rinv;
        for (int k = 1; k < 5; ++k) { R1[k] = R1[k] - l1 * R0[k]; R2[k] = R2[k] - l2 * R0[k]; }
        y1 = y1 - l1 * y0;
        y2 = y2 - l2 * y0;
        for (int k = 0; k < 5; ++k) L.at(j, kU0 + k) = R0[k];
        L.at(j, kYe) = y0;
        for (int k = 0; k < 4; ++k) { R0[k] = R1[k + 1]; R1[k] = R2[k + 1]; }
        R0[4] = 0.0; R1[4] = 0.0;
        for (int k = 0; k < 5; ++k) R2[k] = M(j + 3, j + 1 + k);
        y0 = y1; y1 = y2;
        y2 = (j + 3 < n) ? L.at(j + 3, kY) : 0.0;

        if (kChol) {
            // Cholesky, row j (pbtf2 'U'): U_jj = sqrt(a_jj), U_j,j+k = a_j,j+k * (1 / U_jj), trailing rank-1 update
            if (!(w00 > 0.0)) return P2S_GCV_ILL_POSED;
            const double ajj = sqrt(w00);
            const double ri = 1.0 / ajj;
            const double u1 = w01 * ri, u2 = w02 * ri, u3 = w03 * ri;
            w11 = w11 - u1 * u1; w12 = w12 - u1 * u2; w13 = w13 - u1 * u3;
            w22 = w22 - u2 * u2; w23 = w23 - u2 * u3;
            w33 = w33 - u3 * u3;
            L.at(j, kC1) = u1 / ajj; L.at(j, kC1 + 1) = u2 / ajj; L.at(j, kC1 + 2) = u3 / ajj;
            L.at(j, kD) = 1.0 / (ajj * ajj);
            w00 = w11; w01 = w12; w02 = w13; w03 = A(j + 1, 3);
            w11 = w22; w12 = w23; w13 = A(j + 2, 2);
            w22 = w33; w23 = A(j + 3, 1);
            w33 = A(j + 4, 0);
        }
    }
    return P2S_GCV_OK;
}

// Backward sweep after forward<true>: c by back-substitution, |lambda E c|^2, the inverse's central bands and the
// trace -> GCV(lambda).
__host__ __device__ double backward_gcv(const Lane &L, double lam) {
#pragma clang fp contract(off)
    const int64_t n = L.n;
    double c0 = 0, c1 = 0, c2 = 0, c3 = 0, c4 = 0;          // c_i .. c_{i+4}
    double sq = 0.0, tr = 0.0;
    double p0 = 0, p1 = 0, p2 = 0, q0 = 0, q1 = 0, r0 = 0;   // B bands 0..2 of row i+1, 0..1 of row i+2, 0 of row i+3
    auto resid = [&](int64_t m, double a0, double a1, double a2, double a3, double a4) {
        // (E c)_m, columns m+2 down to m-2 (c_{m-2+k} = a_k); (lambda (E c)_m)^2
        double s = 0.0;
        s = s + eb(m, m + 2, n) * a4; s = s + eb(m, m + 1, n) * a3; s = s + eb(m, m, n) * a2;
        s = s + eb(m, m - 1, n) * a1; s = s + eb(m, m - 2, n) * a0;
        const double v = lam * s;
        return v * v;
    };
    for (int64_t i = n - 1; i >= 0; --i) {
        const double *u = &L.at(i, kU0);
        const double ci = ((((L.at(i, kYe) - c3 * u[4 * L.ks]) - c2 * u[3 * L.ks]) - c1 * u[2 * L.ks]) - c0 * u[L.ks]) / u[0];
        c4 = c3; c3 = c2; c2 = c1; c1 = c0; c0 = ci;
        if (i + 2 <= n - 1) sq = sq + resid(i + 2, c0, c1, c2, c3, c4);

        const double U1 = L.at(i, kC1), U2 = L.at(i, kC1 + 1), U3 = L.at(i, kC1 + 2), D = L.at(i, kD);
        const double b3 = ((0.0 - U1 * p2) - U2 * q1) - U3 * r0;
        const double b2 = ((0.0 - U1 * p1) - U2 * q0) - U3 * q1;
        const double b1 = ((0.0 - U1 * p0) - U2 * p1) - U3 * p2;
        const double b0 = (((0.0 - U1 * b1) - U2 * b2) - U3 * b3) + D;
        if (i + 2 <= n - 1)                                   // column i+2 of tr = B * X^T X (off-diagonals twice)
            tr = tr + (((b2 * L.XX(i, 2)) * 2.0 + (p1 * L.XX(i + 1, 1)) * 2.0) + q0 * L.XX(i + 2, 0));
        r0 = q0; q0 = p0; q1 = p1;
        p0 = b0; p1 = b1; p2 = b2;
    }
    // columns 1 and 0 of the residual and the trace
    sq = sq + resid(1, 0.0, c0, c1, c2, c3);
    sq = sq + resid(0, 0.0, 0.0, c0, c1, c2);
    tr = tr + ((p1 * L.XX(0, 1)) * 2.0 + q0 * L.XX(1, 0));
    tr = tr + p0 * L.XX(0, 0);
    const double norm = sqrt(sq);
    const double numer = norm * norm / (double)n;
    const double t = 1.0 - tr / (double)n;
    return numer / (t * t);
}

// Backward sweep of the final fit: c, then s = X c at the samples, written to out[i * stride] (denormalised in 'auto').
__host__ __device__ void backward_fit(const Lane &L, double *out, int64_t stride, bool denorm, double scale, double med) {
#pragma clang fp contract(off)
    const int64_t n = L.n;
    double c0 = 0, c1 = 0, c2 = 0, c3 = 0;
    auto emit = [&](int64_t i, double s) { out[i * stride] = denorm ? (s - 1.0) * scale + med : s; };
    for (int64_t i = n - 1; i >= 0; --i) {
        const double *u = &L.at(i, kU0);
        const double ci = ((((L.at(i, kYe) - c3 * u[4 * L.ks]) - c2 * u[3 * L.ks]) - c1 * u[2 * L.ks]) - c0 * u[L.ks]) / u[0];
        c3 = c2; c2 = c1; c1 = c0; c0 = ci;
        if (i + 1 <= n - 1) emit(i + 1, (xb(i + 1, i, n) * c0 + xb(i + 1, i + 1, n) * c1) + xb(i + 1, i + 2, n) * c2);
    }
    emit(0, xb(0, 0, n) * c0 + xb(0, 1, n) * c1);
}

__host__ __device__ inline double nan_max(double a, double b) { return (a != a || b != b) ? a + b : (a > b ? a : b); }
__host__ __device__ inline double sign(double v) { return v > 0.0 ? 1.0 : (v < 0.0 ? -1.0 : (v == 0.0 ? 0.0 : v)); }

// One run: the (normalised) samples are in slot kY.  Returns P2S_GCV_*; lam_out = the lambda of the final fit.
__host__ __device__ int run(Lane &L, bool auto_mode, double fixed_lam, double sf, double *out, int64_t stride,
                            double scale, double med, double *lam_out, int32_t *n_eval) {
#pragma clang fp contract(off)
    lane_init(L);
    double lam = fixed_lam;
    *n_eval = 0;
    if (auto_mode) {
        int status = P2S_GCV_OK;
        auto f = [&](double x) -> double {
            if (status != P2S_GCV_OK) return 0.0;
            const int st = forward<true>(L, x);
            if (st != P2S_GCV_OK) { status = st; return 0.0; }
            return backward_gcv(L, x);
        };
        // scipy.optimize._optimize._minimize_scalar_bounded on (0, n)
        double a = 0.0, b = (double)L.n;
        double fulc = a + kGolden * (b - a);
        double nfc = fulc, xf = fulc;
        double rat = 0.0, e = 0.0;
        double x = xf;
        double fx = f(x);
        int num = 1;
        double fu = INFINITY;
        double ffulc = fx, fnfc = fx;
        double xm = 0.5 * (a + b);
        double tol1 = kSqrtEps * fabs(xf) + kXatol / 3.0;
        double tol2 = 2.0 * tol1;
        int flag = 0;
        while (status == P2S_GCV_OK && fabs(xf - xm) > (tol2 - 0.5 * (b - a))) {
            bool golden = true;
            if (fabs(e) > tol1) {
                golden = false;
                double r = (xf - nfc) * (fx - ffulc);
                double q = (xf - fulc) * (fx - fnfc);
                double p = (xf - fulc) * q - (xf - nfc) * r;
                q = 2.0 * (q - r);
                if (q > 0.0) p = -p;
                q = fabs(q);
                r = e;
                e = rat;
                if ((fabs(p) < fabs(0.5 * q * r)) && (p > q * (a - xf)) && (p < q * (b - xf))) {
                    rat = (p + 0.0) / q;
                    x = xf + rat;
                    if (((x - a) < tol2) || ((b - x) < tol2)) {
                        const double si = sign(xm - xf) + ((xm - xf) == 0.0 ? 1.0 : 0.0);
                        rat = tol1 * si;
                    }
                } else {
                    golden = true;
                }
            }
            if (golden) {
                e = (xf >= xm) ? a - xf : b - xf;
                rat = kGolden * e;
            }
            const double si = sign(rat) + (rat == 0.0 ? 1.0 : 0.0);
            x = xf + si * nan_max(fabs(rat), tol1);
            fu = f(x);
            num += 1;
            if (fu <= fx) {
                if (x >= xf) a = xf; else b = xf;
                fulc = nfc; ffulc = fnfc;
                nfc = xf; fnfc = fx;
                xf = x; fx = fu;
            } else {
                if (x < xf) a = x; else b = x;
                if ((fu <= fnfc) || (nfc == xf)) {
                    fulc = nfc; ffulc = fnfc;
                    nfc = x; fnfc = fu;
                } else if ((fu <= ffulc) || (fulc == xf) || (fulc == nfc)) {
                    fulc = x; ffulc = fu;
                }
            }
            xm = 0.5 * (a + b);
            tol1 = kSqrtEps * fabs(xf) + kXatol / 3.0;
            tol2 = 2.0 * tol1;
            if (num >= kMaxFun) { flag = 1; break; }
        }
        *n_eval = num;
        if (status != P2S_GCV_OK) return status;
        if (xf != xf || fx != fx || fu != fu) flag = 2;
        if (flag == 1) return P2S_GCV_MAX_EVALS;
        if (flag == 2) return P2S_GCV_NAN;
        lam = xf * sf;
    }
    *lam_out = lam;
    const int st = forward<false>(L, lam);
    if (st != P2S_GCV_OK) return st;
    backward_fit(L, out, stride, auto_mode, scale, med);
    return P2S_GCV_OK;
}

}  // namespace gcv

__global__ void __launch_bounds__(64) p2s_gcv_spline_kernel(const P2sGcvArgs a) {
#pragma clang fp contract(off)
    const int r = blockIdx.x * 64 + threadIdx.x;
    if (r >= a.n_runs) return;
    P2sGcvRun &run = a.runs[r];
    const int64_t S = a.n_cols, n = run.len;
    double *col = a.data + (int64_t)run.start * S + run.col;
    gcv::Lane L;
    L.w = a.work + run.work_off + threadIdx.x;
    L.ks = 64;
    L.ss = (int64_t)P2S_GCV_SLOTS * 64;
    L.n = n;
    for (int64_t i = 0; i < n; ++i) {                          // the run, normalised in 'auto' (filtering.py:281)
        const double v = col[i * S];
        L.at(i, gcv::kY) = a.auto_mode ? 1.0 + (v - run.med) / run.scale : v;
    }
    double lam = __builtin_nan("");
    int32_t n_eval = 0;
    const int st = gcv::run(L, a.auto_mode != 0, a.fixed_lam, a.smoothing_factor, col, S, run.scale, run.med, &lam, &n_eval);
    run.lam = lam;
    run.n_eval = n_eval;
    run.status = st;
}

}  // namespace

static hipError_t p2s_launch_butter(const P2sFilterArgs &a, hipStream_t s) {
    const unsigned grid = (unsigned)((a.n_cols + 63) / 64);
    switch (a.n_order) {
    case 1: hipLaunchKernelGGL((p2s_butter_kernel<1>), dim3(grid), dim3(64), 0, s, a); break;
    case 2: hipLaunchKernelGGL((p2s_butter_kernel<2>), dim3(grid), dim3(64), 0, s, a); break;
    case 3: hipLaunchKernelGGL((p2s_butter_kernel<3>), dim3(grid), dim3(64), 0, s, a); break;
    case 4: hipLaunchKernelGGL((p2s_butter_kernel<4>), dim3(grid), dim3(64), 0, s, a); break;
    case 5: hipLaunchKernelGGL((p2s_butter_kernel<5>), dim3(grid), dim3(64), 0, s, a); break;
    case 6: hipLaunchKernelGGL((p2s_butter_kernel<6>), dim3(grid), dim3(64), 0, s, a); break;
    case 7: hipLaunchKernelGGL((p2s_butter_kernel<7>), dim3(grid), dim3(64), 0, s, a); break;
    case 8: hipLaunchKernelGGL((p2s_butter_kernel<8>), dim3(grid), dim3(64), 0, s, a); break;
    default: return hipErrorInvalidValue;
    }
    return hipGetLastError();
}

static hipError_t p2s_launch_col_filter(const P2sColFilterArgs &a, hipStream_t s) {
    const int64_t total = a.n_frames * a.n_cols;
    if (total == 0) return hipSuccess;
    const unsigned grid_e = (unsigned)((total + 255) / 256), grid_c = (unsigned)((a.n_cols + 63) / 64);
    switch (a.kind) {
    case P2S_FILTER_HAMPEL: hipLaunchKernelGGL(p2s_hampel_kernel, dim3(grid_e), dim3(256), 0, s, a); break;
    case P2S_FILTER_GAUSSIAN: hipLaunchKernelGGL(p2s_gauss_kernel, dim3(grid_e), dim3(256), 0, s, a); break;
    case P2S_FILTER_MEDIAN: hipLaunchKernelGGL(p2s_median_kernel, dim3(grid_e), dim3(256), 0, s, a); break;
    case P2S_FILTER_ONE_EURO: hipLaunchKernelGGL(p2s_one_euro_kernel, dim3(grid_c), dim3(64), 0, s, a); break;
    case P2S_FILTER_KALMAN: hipLaunchKernelGGL(p2s_kalman_kernel, dim3(grid_c), dim3(64), 0, s, a); break;
    default: return hipErrorInvalidValue;
    }
    return hipGetLastError();
}

// ---- C-ABI entry points (include/p2s.h) ----------------------------------------------------------------------------
namespace {

// np.median of v (destroyed): the middle order statistic, or the mean of the two middle ones
double median_of(std::vector<double> &v) {
    const size_t n = v.size(), h = n / 2;
    std::nth_element(v.begin(), v.begin() + h, v.end());
    const double hi = v[h];
    if (n % 2) return hi;
    const double lo = *std::max_element(v.begin(), v.begin() + h);
    return (lo + hi) / 2.0;
}

}  // namespace

extern "C" {

int p2s_butterworth_host(p2s_ctx *ctx, int64_t n_frames, int32_t n_cols, const double *data, int32_t n_coef,
                         const double *b, const double *a, const double *zi, double *out) {
    if (!ctx) return p2s_set_error(P2S_ERR_INVALID_ARG, "null context");
    if (n_frames < 0 || n_cols < 0) return p2s_set_error(P2S_ERR_INVALID_ARG, "bad shape: n_frames=%lld n_cols=%d", (long long)n_frames, n_cols);
    if (n_coef < 2 || n_coef > P2S_MAX_FILTER_ORDER + 1)
        return p2s_set_error(P2S_ERR_INVALID_ARG, "filter with %d coefficients: supported 2..%d", n_coef, P2S_MAX_FILTER_ORDER + 1);
    if (n_frames == 0 || n_cols == 0) return P2S_OK;
    if (!data || !out || !b || !a || !zi) return p2s_set_error(P2S_ERR_INVALID_ARG, "null pointer");
    if (!(a[0] == 1.0)) return p2s_set_error(P2S_ERR_INVALID_ARG, "a[0] must be 1 (scipy.signal.butter normalises it)");
    P2sFilterArgs f{};
    f.n_frames = n_frames; f.n_cols = n_cols; f.n_order = n_coef - 1;
    f.padlen = 3 * n_coef;                                  // filtering.py:457
    for (int i = 0; i < n_coef; ++i) { f.b[i] = b[i]; f.a[i] = a[i]; }
    for (int i = 0; i < n_coef - 1; ++i) f.zi[i] = zi[i];
    const size_t bytes = (size_t)n_frames * n_cols * sizeof(double);
    HIP_TRY(hipSetDevice(ctx->device));
    Stage st{ctx};
    P2S_TRY(st.upload(f.in, data, bytes));
    P2S_TRY(st.alloc(f.out, bytes));
    P2S_TRY(st.alloc(f.work, (size_t)(n_frames + 2 * f.padlen) * n_cols * sizeof(double)));
    HIP_TRY(p2s_launch_butter(f, ctx->stream));
    P2S_TRY(st.down(out, f.out, bytes));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    return P2S_OK;
}

int p2s_filter_columns_host(p2s_ctx *ctx, int32_t kind, int64_t n_frames, int32_t n_cols, const double *data,
                            const double *params, int32_t n_params, double *out) {
    if (!ctx) return p2s_set_error(P2S_ERR_INVALID_ARG, "null context");
    if (n_frames < 0 || n_cols < 0) return p2s_set_error(P2S_ERR_INVALID_ARG, "bad shape: n_frames=%lld n_cols=%d", (long long)n_frames, n_cols);
    if (n_params < 0 || (n_params > 0 && !params)) return p2s_set_error(P2S_ERR_INVALID_ARG, "null parameters");
    P2sColFilterArgs f{};
    f.kind = kind; f.n_frames = n_frames; f.n_cols = n_cols;
    switch (kind) {
    case P2S_FILTER_HAMPEL:
        if (n_params != 1) return p2s_set_error(P2S_ERR_INVALID_ARG, "Hampel filter: params = {n_sigma}");
        f.p[0] = params[0];
        break;
    case P2S_FILTER_GAUSSIAN:
        if (n_params < 1 || n_params % 2 != 1 || n_params > 8191) return p2s_set_error(P2S_ERR_INVALID_ARG, "Gaussian filter: params = 2 radius + 1 weights");
        f.radius = n_params / 2;
        break;
    case P2S_FILTER_MEDIAN: {
        if (n_params != 1) return p2s_set_error(P2S_ERR_INVALID_ARG, "median filter: params = {kernel_size}");
        const int k = (int)params[0];
        if ((double)k != params[0] || k < 1 || k % 2 != 1 || k > 1023) return p2s_set_error(P2S_ERR_INVALID_ARG, "median filter: kernel_size must be odd, 1..1023");
        f.radius = k / 2;
        break;
    }
    case P2S_FILTER_ONE_EURO:
        if (n_params != 4) return p2s_set_error(P2S_ERR_INVALID_ARG, "one-euro filter: params = {dt, min_cutoff, beta, d_cutoff}");
        for (int i = 0; i < 4; ++i) f.p[i] = params[i];
        if (!(f.p[0] > 0.0)) return p2s_set_error(P2S_ERR_INVALID_ARG, "one-euro filter: dt must be positive");
        break;
    case P2S_FILTER_KALMAN:
        if (n_params != 4) return p2s_set_error(P2S_ERR_INVALID_ARG, "Kalman filter: params = {dt, measurement_noise, process_noise, smooth}");
        for (int i = 0; i < 4; ++i) f.p[i] = params[i];
        if (!(f.p[0] > 0.0)) return p2s_set_error(P2S_ERR_INVALID_ARG, "Kalman filter: dt must be positive");
        break;
    default: return p2s_set_error(P2S_ERR_INVALID_ARG, "unknown column filter %d", kind);
    }
    if (n_frames == 0 || n_cols == 0) return P2S_OK;
    if (!data || !out) return p2s_set_error(P2S_ERR_INVALID_ARG, "null pointer");
    const size_t bytes = (size_t)n_frames * n_cols * sizeof(double);
    if (kind == P2S_FILTER_MEDIAN)
        for (size_t i = 0, n = (size_t)n_frames * n_cols; i < n; ++i)
            if (!(data[i] == data[i])) return p2s_set_error(P2S_ERR_INVALID_ARG, "median filter: the data hold NaN (scipy.signal.medfilt's answer for them is not defined)");
    HIP_TRY(hipSetDevice(ctx->device));
    Stage st{ctx};
    P2S_TRY(st.upload(f.in, data, bytes));
    P2S_TRY(st.alloc(f.out, bytes));
    if (kind == P2S_FILTER_ONE_EURO || kind == P2S_FILTER_KALMAN) P2S_TRY(st.alloc(f.work, kind == P2S_FILTER_KALMAN ? 12 * bytes : bytes));
    if (kind == P2S_FILTER_GAUSSIAN) P2S_TRY(st.upload(f.w, params, (size_t)n_params * sizeof(double)));
    HIP_TRY(p2s_launch_col_filter(f, ctx->stream));
    P2S_TRY(st.down(out, f.out, bytes));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    return P2S_OK;
}

int p2s_gcv_spline_host(p2s_ctx *ctx, int64_t n_frames, int32_t n_cols, const double *data, int32_t auto_mode,
                        double lam, double smoothing_factor, double *out, double *lam_out) {
    if (!ctx) return p2s_set_error(P2S_ERR_INVALID_ARG, "null context");
    if (n_frames < 0 || n_frames > INT32_MAX || n_cols < 0)
        return p2s_set_error(P2S_ERR_INVALID_ARG, "bad shape: n_frames=%lld n_cols=%d", (long long)n_frames, n_cols);
    if (n_frames == 0 || n_cols == 0) return P2S_OK;
    if (!data || !out) return p2s_set_error(P2S_ERR_INVALID_ARG, "null pointer");
    const int64_t S = n_cols;
    const size_t total = (size_t)n_frames * n_cols;
    std::memcpy(out, data, total * sizeof(double));
    if (lam_out)
        for (size_t i = 0; i < total; ++i) lam_out[i] = NAN;

    // the runs of valid samples (neither NaN nor 0, filtering.py:265-270), column by column
    std::vector<P2sGcvRun> runs;
    std::vector<double> tmp;
    for (int32_t c = 0; c < n_cols; ++c) {
        int64_t f = 0;
        while (f < n_frames) {
            auto valid = [&](int64_t i) { const double v = data[i * S + c]; return v == v && v != 0.0; };
            if (!valid(f)) { ++f; continue; }
            int64_t r = f + 1;
            while (r < n_frames && valid(r)) ++r;
            const int64_t len = r - f;
            if (len >= 2 && len <= 4)                      // make_smoothing_spline / the GCV helper refuse n <= 4
                return p2s_set_error(P2S_ERR_GCV_SHORT_RUN, "``x`` and ``y`` length must be at least 5");
            if (len >= 5) {
                P2sGcvRun run{};
                run.col = c; run.start = (int32_t)f; run.len = (int32_t)len;
                run.med = 0.0; run.scale = 1.0;
                for (int64_t i = f; i < r; ++i)
                    if (std::isinf(data[i * S + c])) return p2s_set_error(P2S_ERR_INVALID_ARG, "array must not contain infs or NaNs");
                if (auto_mode) {                           // filtering.py:277-281
                    tmp.assign(len, 0.0);
                    for (int64_t i = 0; i < len; ++i) tmp[i] = data[(f + i) * S + c];
                    const double med = median_of(tmp);
                    for (int64_t i = 0; i < len; ++i) tmp[i] = std::fabs(data[(f + i) * S + c] - med);
                    double mad = median_of(tmp);
                    mad = mad > 0 ? mad : 1.0;
                    run.med = med;
                    run.scale = 1.4826 * mad;
                }
                runs.push_back(run);
            }
            f = r;
        }
    }
    if (runs.empty()) return P2S_OK;
    if (!((auto_mode ? smoothing_factor : lam * smoothing_factor) >= 0.0))
        return p2s_set_error(P2S_ERR_INVALID_ARG, "Regularization parameter should be non-negative");

    // longest first, so that the long runs start first and a wave's lanes have similar lengths; the factor storage of
    // a wave covers its longest run
    std::vector<int32_t> order(runs.size());
    for (size_t i = 0; i < order.size(); ++i) order[i] = (int32_t)i;
    std::stable_sort(order.begin(), order.end(), [&](int32_t x, int32_t y) { return runs[x].len > runs[y].len; });
    std::vector<P2sGcvRun> sorted(runs.size());
    size_t work_doubles = 0;
    for (size_t i = 0; i < order.size(); ++i) {
        sorted[i] = runs[order[i]];
        if (i % 64 == 0) {
            sorted[i].work_off = (int64_t)work_doubles;
            work_doubles += (size_t)sorted[i].len * P2S_GCV_SLOTS * 64;
        } else {
            sorted[i].work_off = sorted[i - i % 64].work_off;
        }
    }

    P2sGcvArgs g{};
    g.n_frames = n_frames; g.n_cols = n_cols; g.n_runs = (int32_t)sorted.size();
    g.auto_mode = auto_mode ? 1 : 0;
    g.fixed_lam = lam * smoothing_factor;                  // filtering.py:301-304
    g.smoothing_factor = smoothing_factor;
    const size_t bytes = total * sizeof(double), run_bytes = sorted.size() * sizeof(P2sGcvRun);
    HIP_TRY(hipSetDevice(ctx->device));
    Stage st{ctx};
    P2S_TRY(st.upload(g.data, data, bytes));
    P2S_TRY(st.upload(g.runs, sorted.data(), run_bytes));
    P2S_TRY(st.alloc(g.work, work_doubles * sizeof(double)));
    hipLaunchKernelGGL(p2s_gcv_spline_kernel, dim3((unsigned)((g.n_runs + 63) / 64)), dim3(64), 0, ctx->stream, g);
    HIP_TRY(hipGetLastError());
    P2S_TRY(st.down(out, g.data, bytes));
    P2S_TRY(st.down(sorted.data(), g.runs, run_bytes));
    HIP_TRY(hipStreamSynchronize(ctx->stream));

    // the reference stops at the first run (column by column) whose search or solve fails
    const P2sGcvRun *bad = nullptr;
    for (const P2sGcvRun &r : sorted)
        if (r.status != P2S_GCV_OK && (!bad || r.col < bad->col || (r.col == bad->col && r.start < bad->start))) bad = &r;
    if (bad) {
        std::memcpy(out, data, bytes);
        switch (bad->status) {
        case P2S_GCV_ILL_POSED: return p2s_set_error(P2S_ERR_GCV_ILL_POSED, "Seems like the problem is ill-posed");
        case P2S_GCV_SINGULAR: return p2s_set_error(P2S_ERR_GCV_SINGULAR, "singular matrix");
        case P2S_GCV_MAX_EVALS:
            return p2s_set_error(P2S_ERR_GCV_NO_MINIMUM, "Unable to find minimum of the GCV function: Maximum number of function calls reached.");
        default: return p2s_set_error(P2S_ERR_GCV_NO_MINIMUM, "Unable to find minimum of the GCV function: NaN result encountered.");
        }
    }
    if (lam_out)
        for (const P2sGcvRun &r : sorted) lam_out[(int64_t)r.start * S + r.col] = r.lam;
    return P2S_OK;
}

int p2s_loess_host(p2s_ctx *ctx, int64_t n_frames, int32_t n_cols, const double *data, int32_t k, int64_t min_run, double *out) {
    if (!ctx) return p2s_set_error(P2S_ERR_INVALID_ARG, "null context");
    if (n_frames < 0 || n_cols < 0) return p2s_set_error(P2S_ERR_INVALID_ARG, "bad shape: n_frames=%lld n_cols=%d", (long long)n_frames, n_cols);
    if (k < 2 || k > 8191) return p2s_set_error(P2S_ERR_INVALID_ARG, "LOESS filter: window of %d samples: supported 2..8191", k);
    if (min_run <= k)
        return p2s_set_error(P2S_ERR_INVALID_ARG, "LOESS filter: min_run=%lld must exceed the window of %d samples", (long long)min_run, k);
    if (n_frames == 0 || n_cols == 0) return P2S_OK;
    if (!data || !out) return p2s_set_error(P2S_ERR_INVALID_ARG, "null pointer");
    const size_t total = (size_t)n_frames * n_cols, bytes = total * sizeof(double);
    for (size_t i = 0; i < total; ++i)
        if (std::isinf(data[i]))
            return p2s_set_error(P2S_ERR_INVALID_ARG, "LOESS filter: the data hold an infinity (statsmodels' answer for one has not been recorded)");

    // the interior window: tricube weights of the distances 0 .. k / 2 - 1 with h = k / 2, normalised by their sum
    // over both sides
    const int m = k / 2;
    std::vector<double> wn(m);
    double sum = 0.0;
    for (int d = m - 1; d >= 1; --d) { wn[d] = loess_tricube((double)d, (double)m); sum += 2.0 * wn[d]; }
    wn[0] = 1.0;
    sum += 1.0;
    for (int d = 0; d < m; ++d) wn[d] /= sum;

    P2sLoessArgs f{};
    f.n_frames = n_frames; f.n_cols = n_cols; f.k = k; f.min_run = min_run;
    HIP_TRY(hipSetDevice(ctx->device));
    Stage st{ctx};
    P2S_TRY(st.upload(f.in, data, bytes));
    P2S_TRY(st.alloc(f.out, bytes));
    P2S_TRY(st.upload(f.wn, wn.data(), (size_t)m * sizeof(double)));
    hipLaunchKernelGGL(p2s_loess_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, ctx->stream, f);
    HIP_TRY(hipGetLastError());
    P2S_TRY(st.down(out, f.out, bytes));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    return P2S_OK;
}

int p2s_trc_metrics_host(p2s_ctx *ctx, int64_t n_frames, int32_t n_markers, const double *xyz, int32_t n_bones,
                         const int32_t *bones, double *bone_len, double *bone_stats, double *accel, int64_t *missing) {
    if (!ctx) return p2s_set_error(P2S_ERR_INVALID_ARG, "null context");
    if (n_frames < 0 || n_markers < 0 || n_bones < 0) return p2s_set_error(P2S_ERR_INVALID_ARG, "bad shape");
    if (n_frames == 0 || (n_markers == 0 && n_bones == 0)) return P2S_OK;
    if (!xyz || (n_bones && (!bones || !bone_len || !bone_stats)) || (n_markers && (!accel || !missing)))
        return p2s_set_error(P2S_ERR_INVALID_ARG, "null pointer");
    for (int i = 0; i < 2 * n_bones; ++i)
        if (bones[i] < 0 || bones[i] >= n_markers) return p2s_set_error(P2S_ERR_INVALID_ARG, "bone %d names marker %d of %d", i / 2, bones[i], n_markers);
    const size_t xyz_b = (size_t)n_frames * n_markers * 3 * sizeof(double);
    const size_t len_b = (size_t)n_bones * n_frames * sizeof(double);
    const size_t acc_b = (size_t)n_markers * (n_frames > 2 ? n_frames - 2 : 0) * sizeof(double);
    HIP_TRY(hipSetDevice(ctx->device));
    P2sMetricsArgs m{};
    m.n_frames = n_frames; m.n_markers = n_markers; m.n_bones = n_bones;
    Stage st{ctx};
    unsigned char *aux;                                    // one block: bones [n_bones][2] i32, bone_stats [n_bones][3], missing [n_markers]
    P2S_TRY(st.upload(m.xyz, xyz, xyz_b));
    P2S_TRY(st.alloc(m.bone_len, len_b));
    P2S_TRY(st.alloc(m.accel, acc_b));
    P2S_TRY(st.alloc(aux, (size_t)n_bones * 32 + (size_t)n_markers * 8));
    m.bones = (const int32_t *)aux;
    m.bone_stats = (double *)(aux + (size_t)n_bones * 8);
    m.missing = (int64_t *)(aux + (size_t)n_bones * 32);
    P2S_TRY(st.up(aux, bones, (size_t)n_bones * 8));
    hipLaunchKernelGGL(p2s_trc_metrics_kernel, dim3((unsigned)(n_bones + n_markers)), dim3(256), 0, ctx->stream, m);
    HIP_TRY(hipGetLastError());
    P2S_TRY(st.down(bone_len, m.bone_len, len_b));
    P2S_TRY(st.down(bone_stats, m.bone_stats, (size_t)n_bones * 24));
    P2S_TRY(st.down(accel, m.accel, acc_b));
    P2S_TRY(st.down(missing, m.missing, (size_t)n_markers * 8));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    return P2S_OK;
}

}  // extern "C"
