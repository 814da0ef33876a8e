// p2s_sync.hip -- the synchronization stage on gfx950: vertical speeds of every camera and their time-lagged Pearson
// correlation with the reference camera's (synchronize_cams_all, synchronization.py:1346-1612).  fp64 throughout.
//
// Speeds (:1541-1575, vert_speed :1271-1288), three launches:
//   p2s_sync_columns_kernel  one lane per (camera, coordinate column), consecutive lanes = consecutive columns of the
//                            camera's row-major [frame][column] block: interpolate_zeros_nans(col, 'linear') (scipy
//                            interp1d, linear, fill_value 'extrapolate', same slope expression), bfill().ffill(), then
//                            signal.filtfilt(b, a, col) over the whole column when the camera has more than
//                            3 (len(b) - 1) frames (the reference's own check; scipy's padlen is 3 len(b));
//   p2s_sync_speed_kernel    one thread per frame: diff of every y column, NaN -> 2x the second row's diff (fillna),
//                            sum of |.| with pandas' skipna (NaN skipped, all-NaN row -> 0);
//   p2s_sync_sum_kernel      one lane per camera: filtfilt of that sum under the same rule.
// The recurrences are sequential in time; the work is small (a few ms for 8 x 36 000 frames), latency-bound.
//
// Lagged Pearson (time_lagged_cross_corr :1291-1343), the O(N^2) part:
//   p2s_pearson_kernel       one wave per (signal, group of kLagsPerWave consecutive lags).  The lanes stride over the
//                            union of the group's pair ranges; every reference sample is loaded once for the group and
//                            the compared signal's samples of the group's lags are neighbours (one cache line).  Two
//                            passes as np.corrcoef: means over the pairs whose values are both not NaN (pandas' notna),
//                            then the centred sums; r = sxy / f / sqrt(sxx / f) / sqrt(syy / f), f = n - 1, clipped to
//                            [-1, 1]; NaN with fewer than 2 pairs or a centred sum of 0.  Both signals stay in L2
//                            (2 x 288 KB at 36 000 frames).
//   p2s_pearson_argmax_kernel one workgroup per signal: np.argmax of the r list (first maximum, or first NaN if any) and
//                            np.nanmax (NaN when every r is NaN).
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <math.h>

#include <vector>

#include "p2s_ctx.h"
#include "p2s_iir.h"

// synchronization speeds and their time-lagged Pearson correlation (synchronization.py:1271-1343, 1541-1575)
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

namespace {

__device__ __forceinline__ bool good_sample(double v) { return (v == v) && (v != 0.0); }

// scipy.signal.filtfilt(b, a, x) with its defaults (padtype 'odd', padlen = 3 (N + 1), lfilter_zi start) on the L
// samples x[0], x[S], ...; out may alias x (x is only read in the forward pass).  work: L + 2 padlen samples, stride S.
template <int N>
__device__ void filtfilt_column(const P2sSyncArgs &a, const double *x, double *out, double *work, int64_t L, int64_t S) {
    const int64_t pad = a.padlen;
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
        if (i >= pad && i < pad + L) out[(i - pad) * S] = y;
    }
}

// interp1d(..., kind='linear', fill_value='extrapolate')(i) for a missing sample i: slope between the good samples lo
// and hi, evaluated as scipy's _call_linear does.
__device__ __forceinline__ double interp_at(const double *x, int64_t S, int64_t lo, int64_t hi, int64_t i) {
#pragma clang fp contract(off)
    const double ylo = x[lo * S], yhi = x[hi * S];
    const double slope = (yhi - ylo) / (double)(hi - lo);
    return slope * (double)(i - lo) + ylo;
}

template <int N>
__global__ void __launch_bounds__(64) p2s_sync_columns_kernel(const P2sSyncArgs a) {
    const int64_t lane = (int64_t)blockIdx.x * 64 + threadIdx.x;
    if (lane >= (int64_t)a.n_cams * a.n_cols) return;
    const int c = (int)(lane / a.n_cols), j = (int)(lane % a.n_cols);
    const int64_t S = a.n_cols, r0 = a.row0[c], L = a.row0[c + 1] - r0;
    const double *x = a.coords + r0 * S + j;
    double *out = a.filled + r0 * S + j;

    // interpolate_zeros_nans (common.py:669-715, N = inf): only with more than 4 good samples
    int64_t G = 0, g0 = -1, g1 = -1, gl1 = -1, gl = -1;
    for (int64_t f = 0; f < L; ++f)
        if (good_sample(x[f * S])) {
            if (G == 0) g0 = f; else if (G == 1) g1 = f;
            gl1 = gl; gl = f;
            ++G;
        }
    if (G <= 4) {
        for (int64_t f = 0; f < L; ++f) out[f * S] = x[f * S];
    } else {
        int64_t prev = -1, f = 0;
        while (f < L) {
            if (good_sample(x[f * S])) { out[f * S] = x[f * S]; prev = f++; continue; }
            int64_t r = f + 1;                                   // the missing run [f, r)
            while (r < L && !good_sample(x[r * S])) ++r;
            const int64_t lo = prev < 0 ? g0 : (r >= L ? gl1 : prev);
            const int64_t hi = prev < 0 ? g1 : (r >= L ? gl : r);
            for (int64_t i = f; i < r; ++i) out[i * S] = interp_at(x, S, lo, hi, i);
            f = r;
        }
    }
    // bfill().ffill()
    double carry = __builtin_nan("");
    for (int64_t f = L - 1; f >= 0; --f) {
        const double v = out[f * S];
        if (v != v) out[f * S] = carry; else carry = v;
    }
    carry = __builtin_nan("");
    for (int64_t f = 0; f < L; ++f) {
        const double v = out[f * S];
        if (v != v) out[f * S] = carry; else carry = v;
    }
    if (L > a.filter_above) filtfilt_column<N>(a, out, out, a.work + (r0 + (int64_t)2 * a.padlen * c) * S + j, L, S);
}

__global__ void __launch_bounds__(256) p2s_sync_speed_kernel(const P2sSyncArgs a) {
    const int64_t gr = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (gr >= a.row0[a.n_cams]) return;
    int c = 0;
    while (a.row0[c + 1] <= gr) ++c;
    const int64_t S = a.n_cols, r0 = a.row0[c], f = gr - r0;
    const double *v = a.filled + r0 * S;
    double sum = 0.0;
    for (int k = 1; k < a.n_cols; k += 2) {
        double d = f >= 1 ? v[f * S + k] - v[(f - 1) * S + k] : __builtin_nan("");
        if (d != d) d = (v[S + k] - v[k]) * 2.0;                // df_diff.fillna(df_diff.iloc[1] * 2)
        if (d == d) sum += fabs(d);
    }
    a.speed[gr] = sum;
}

template <int N>
__global__ void __launch_bounds__(64) p2s_sync_sum_kernel(const P2sSyncArgs a) {
    const int c = blockIdx.x * 64 + threadIdx.x;
    if (c >= a.n_cams) return;
    const int64_t r0 = a.row0[c], L = a.row0[c + 1] - r0;
    if (L > a.filter_above) filtfilt_column<N>(a, a.speed + r0, a.speed + r0, a.speed_work + r0 + (int64_t)2 * a.padlen * c, L, 1);
}

// ---------------------------------------------------------------------------------------------------------------------
constexpr int kLagsPerWave = 8;

__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m, 64);
    return v;
}

__global__ void __launch_bounds__(256) p2s_pearson_kernel(const P2sPearsonArgs a) {
    const int s = blockIdx.y;
    const int lane = threadIdx.x & 63;
    const int64_t t0 = ((int64_t)blockIdx.x * 4 + (threadIdx.x >> 6)) * kLagsPerWave;
    if (t0 >= a.n_lags) return;                                 // whole waves leave together
    const double *y = a.sig + a.sig0[s];
    const int64_t ny = a.sig0[s + 1] - a.sig0[s];
    const int64_t M = a.n_ref < ny ? a.n_ref : ny;              // Series.align(join='inner') on 0..n-1 indices
    int64_t lo[kLagsPerWave], hi[kLagsPerWave];
#pragma unroll
    for (int j = 0; j < kLagsPerWave; ++j) {
        const int64_t lag = a.lag_lo + t0 + j;
        lo[j] = lag > 0 ? lag : 0;
        hi[j] = ny + lag < M ? ny + lag : M;
        if (t0 + j >= a.n_lags || hi[j] < lo[j]) hi[j] = lo[j];   // no pairs
    }
    int64_t ulo = INT64_MAX, uhi = 0;                           // union of the group's pair ranges
#pragma unroll
    for (int j = 0; j < kLagsPerWave; ++j)
        if (hi[j] > lo[j]) { ulo = lo[j] < ulo ? lo[j] : ulo; uhi = hi[j] > uhi ? hi[j] : uhi; }
    if (ulo > uhi) ulo = uhi;
    const int64_t lag0 = a.lag_lo + t0;

    double n[kLagsPerWave], sx[kLagsPerWave], sy[kLagsPerWave];
#pragma unroll
    for (int j = 0; j < kLagsPerWave; ++j) n[j] = sx[j] = sy[j] = 0.0;
    for (int64_t i = ulo + lane; i < uhi; i += 64) {
        const double xv = a.ref[i];
        if (xv != xv) continue;
#pragma unroll
        for (int j = 0; j < kLagsPerWave; ++j) {
            if (i < lo[j] || i >= hi[j]) continue;
            const double yv = y[i - lag0 - j];
            if (yv != yv) continue;
            n[j] += 1.0; sx[j] += xv; sy[j] += yv;
        }
    }
    double mx[kLagsPerWave], my[kLagsPerWave];
#pragma unroll
    for (int j = 0; j < kLagsPerWave; ++j) {
        n[j] = wave_sum(n[j]);
        mx[j] = wave_sum(sx[j]) / n[j];
        my[j] = wave_sum(sy[j]) / n[j];
    }
    double sxx[kLagsPerWave], syy[kLagsPerWave], sxy[kLagsPerWave];
#pragma unroll
    for (int j = 0; j < kLagsPerWave; ++j) sxx[j] = syy[j] = sxy[j] = 0.0;
    for (int64_t i = ulo + lane; i < uhi; i += 64) {
        const double xv = a.ref[i];
        if (xv != xv) continue;
#pragma unroll
        for (int j = 0; j < kLagsPerWave; ++j) {
            if (i < lo[j] || i >= hi[j]) continue;
            const double yv = y[i - lag0 - j];
            if (yv != yv) continue;
            const double dx = xv - mx[j], dy = yv - my[j];
            sxx[j] += dx * dx; syy[j] += dy * dy; sxy[j] += dx * dy;
        }
    }
#pragma unroll
    for (int j = 0; j < kLagsPerWave; ++j) {
        const double cxx = wave_sum(sxx[j]), cyy = wave_sum(syy[j]), cxy = wave_sum(sxy[j]);
        if (lane != 0 || t0 + j >= a.n_lags) continue;
        double r = __builtin_nan("");
        if (n[j] >= 2.0) {
            const double inv = 1.0 / (n[j] - 1.0);              // np.cov: c *= 1 / fact
            r = cxy * inv / sqrt(cxx * inv) / sqrt(cyy * inv);   // np.corrcoef: c /= stddev[:, None]; c /= stddev[None, :]
            if (r == r) r = fmin(1.0, fmax(-1.0, r));           // np.clip(c, -1, 1)
        }
        a.r[(int64_t)s * a.n_lags + t0 + j] = r;
    }
}

__global__ void __launch_bounds__(256) p2s_pearson_argmax_kernel(const P2sPearsonArgs a) {
    __shared__ double best_v[256];
    __shared__ int64_t best_t[256], nan_t[256];
    const int s = blockIdx.x, tid = threadIdx.x;
    const double *r = a.r + (int64_t)s * a.n_lags;
    double bv = -INFINITY;
    int64_t bt = INT64_MAX, nt = INT64_MAX;
    for (int64_t t = tid; t < a.n_lags; t += 256) {
        const double v = r[t];
        if (v != v) { if (nt == INT64_MAX) nt = t; }
        else if (bt == INT64_MAX || v > bv) { bv = v; bt = t; }
    }
    best_v[tid] = bv; best_t[tid] = bt; nan_t[tid] = nt;
    __syncthreads();
    for (int h = 128; h >= 1; h >>= 1) {
        if (tid < h) {
            const double ov = best_v[tid + h];
            const int64_t ot = best_t[tid + h];
            if (ot != INT64_MAX && (best_t[tid] == INT64_MAX || ov > best_v[tid] || (ov == best_v[tid] && ot < best_t[tid]))) {
                best_v[tid] = ov; best_t[tid] = ot;
            }
            if (nan_t[tid + h] < nan_t[tid]) nan_t[tid] = nan_t[tid + h];
        }
        __syncthreads();
    }
    if (tid == 0) {
        a.argmax[s] = nan_t[0] != INT64_MAX ? nan_t[0] : best_t[0];
        a.max_corr[s] = best_t[0] != INT64_MAX ? best_v[0] : __builtin_nan("");
    }
}

}  // namespace

static hipError_t p2s_launch_sync_speeds(const P2sSyncArgs &a, hipStream_t s) {
    const int64_t lanes = (int64_t)a.n_cams * a.n_cols, rows = a.total_rows;
    if (rows == 0) return hipSuccess;
    const unsigned grid_c = (unsigned)((lanes + 63) / 64), grid_r = (unsigned)((rows + 255) / 256);
    const unsigned grid_s = (unsigned)((a.n_cams + 63) / 64);
    switch (a.n_order) {
#define P2S_SYNC_CASE(N)                                                                                   \
    case N:                                                                                                \
        if (lanes) hipLaunchKernelGGL((p2s_sync_columns_kernel<N>), dim3(grid_c), dim3(64), 0, s, a);      \
        hipLaunchKernelGGL(p2s_sync_speed_kernel, dim3(grid_r), dim3(256), 0, s, a);                       \
        hipLaunchKernelGGL((p2s_sync_sum_kernel<N>), dim3(grid_s), dim3(64), 0, s, a);                     \
        break;
    P2S_SYNC_CASE(1) P2S_SYNC_CASE(2) P2S_SYNC_CASE(3) P2S_SYNC_CASE(4)
    P2S_SYNC_CASE(5) P2S_SYNC_CASE(6) P2S_SYNC_CASE(7) P2S_SYNC_CASE(8)
#undef P2S_SYNC_CASE
    default: return hipErrorInvalidValue;
    }
    return hipGetLastError();
}

static hipError_t p2s_launch_pearson(const P2sPearsonArgs &a, hipStream_t s) {
    if (a.n_sig == 0 || a.n_lags == 0) return hipSuccess;
    const int64_t groups = (a.n_lags + kLagsPerWave - 1) / kLagsPerWave;
    hipLaunchKernelGGL(p2s_pearson_kernel, dim3((unsigned)((groups + 3) / 4), (unsigned)a.n_sig), dim3(256), 0, s, a);
    hipLaunchKernelGGL(p2s_pearson_argmax_kernel, dim3((unsigned)a.n_sig), dim3(256), 0, s, a);
    return hipGetLastError();
}

// ---- C-ABI entry points (include/p2s.h) ----------------------------------------------------------------------------
extern "C" {

int p2s_sync_speeds_host(p2s_ctx *ctx, int32_t n_cams, const int64_t *n_frames, int32_t n_cols, const double *coords,
                         int32_t n_coef, const double *b, const double *a, const double *zi, double *speeds) {
    if (!ctx) return p2s_set_error(P2S_ERR_INVALID_ARG, "null context");
    if (n_cams < 0 || n_cols < 0 || (n_cols & 1)) return p2s_set_error(P2S_ERR_INVALID_ARG, "bad shape: n_cams=%d n_cols=%d (x, y pairs)", n_cams, n_cols);
    if (n_coef < 2 || n_coef > P2S_MAX_FILTER_ORDER + 1)
        return p2s_set_error(P2S_ERR_INVALID_ARG, "filter with %d coefficients: supported 2..%d", n_coef, P2S_MAX_FILTER_ORDER + 1);
    if (n_cams == 0) return P2S_OK;
    if (!n_frames || !b || !a || !zi || !speeds) return p2s_set_error(P2S_ERR_INVALID_ARG, "null pointer");
    if (!(a[0] == 1.0)) return p2s_set_error(P2S_ERR_INVALID_ARG, "a[0] must be 1 (scipy.signal.butter normalises it)");
    P2sSyncArgs f{};
    f.n_cams = n_cams; f.n_cols = n_cols; f.n_order = n_coef - 1;
    f.padlen = 3 * n_coef;                                   // scipy.signal.filtfilt's default
    f.filter_above = 3 * (n_coef - 1);                       // synchronization.py:1539, 1567, 1584
    for (int i = 0; i < n_coef; ++i) { f.b[i] = b[i]; f.a[i] = a[i]; }
    for (int i = 0; i < n_coef - 1; ++i) f.zi[i] = zi[i];
    std::vector<int64_t> row0((size_t)n_cams + 1, 0);
    for (int c = 0; c < n_cams; ++c) {
        const int64_t L = n_frames[c];
        if (L < 2 || L > ((int64_t)1 << 31)) return p2s_set_error(P2S_ERR_INVALID_ARG, "camera %d: %lld frames (2 .. 2^31 supported)", c, (long long)L);
        if (L > f.filter_above && L <= f.padlen)
            return p2s_set_error(P2S_ERR_SYNC_PADLEN, "The length of the input vector x must be greater than padlen, which is %d.", f.padlen);
        row0[(size_t)c + 1] = row0[(size_t)c] + L;
    }
    const int64_t rows = row0[(size_t)n_cams];
    if (n_cols > 0 && !coords) return p2s_set_error(P2S_ERR_INVALID_ARG, "null coords");
    f.total_rows = rows;
    const int64_t wrows = rows + (int64_t)2 * f.padlen * n_cams;
    const size_t cbytes = (size_t)rows * n_cols * sizeof(double), wbytes = (size_t)wrows * n_cols * sizeof(double);
    // one block: speed [rows], speed_work [wrows], row0 [n_cams + 1]
    const size_t sw_off = (size_t)rows * sizeof(double), r0_off = sw_off + (size_t)wrows * sizeof(double);
    const size_t r0_b = row0.size() * sizeof(int64_t);
    HIP_TRY(hipSetDevice(ctx->device));
    Stage st{ctx};
    char *aux;
    P2S_TRY(st.alloc(f.coords, cbytes + 16));
    P2S_TRY(st.up(f.coords, coords, cbytes));
    P2S_TRY(st.alloc(f.filled, cbytes + 16));
    P2S_TRY(st.alloc(f.work, wbytes + 16));
    P2S_TRY(st.alloc(aux, r0_off + r0_b));
    f.speed = (double *)aux; f.speed_work = (double *)(aux + sw_off); f.row0 = (const int64_t *)(aux + r0_off);
    P2S_TRY(st.up(f.row0, row0.data(), r0_b));
    HIP_TRY(p2s_launch_sync_speeds(f, ctx->stream));
    P2S_TRY(st.down(speeds, f.speed, (size_t)rows * sizeof(double)));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    return P2S_OK;
}

int p2s_lagged_pearson_host(p2s_ctx *ctx, const double *ref, int64_t n_ref, int32_t n_sig, const double *sig,
                            const int64_t *sig_len, int64_t lag_lo, int64_t lag_hi, double *r, int64_t *argmax,
                            double *max_corr) {
    if (!ctx) return p2s_set_error(P2S_ERR_INVALID_ARG, "null context");
    if (n_ref < 0 || n_sig < 0 || n_ref > ((int64_t)1 << 31)) return p2s_set_error(P2S_ERR_INVALID_ARG, "bad shape: n_ref=%lld n_sig=%d", (long long)n_ref, n_sig);
    if (lag_hi <= lag_lo || lag_hi - lag_lo > ((int64_t)1 << 31) || lag_lo < -((int64_t)1 << 40) || lag_hi > ((int64_t)1 << 40))
        return p2s_set_error(P2S_ERR_INVALID_ARG, "empty or too large lag range [%lld, %lld)", (long long)lag_lo, (long long)lag_hi);
    if (n_sig == 0) return P2S_OK;
    if (!sig_len || !r || !argmax || !max_corr || (n_ref > 0 && !ref)) return p2s_set_error(P2S_ERR_INVALID_ARG, "null pointer");
    std::vector<int64_t> sig0((size_t)n_sig + 1, 0);
    for (int i = 0; i < n_sig; ++i) {
        if (sig_len[i] < 0 || sig_len[i] > ((int64_t)1 << 31)) return p2s_set_error(P2S_ERR_INVALID_ARG, "signal %d: bad length", i);
        sig0[(size_t)i + 1] = sig0[(size_t)i] + sig_len[i];
    }
    const int64_t total = sig0[(size_t)n_sig];
    if (total > 0 && !sig) return p2s_set_error(P2S_ERR_INVALID_ARG, "null signals");
    P2sPearsonArgs p{};
    p.n_ref = n_ref; p.lag_lo = lag_lo; p.n_lags = lag_hi - lag_lo; p.n_sig = n_sig;
    // one input block: ref [n_ref + 1], sig [total + 1], sig0 [n_sig + 1]; one result block: argmax [n_sig], max_corr [n_sig]
    const size_t sig_off = (size_t)(n_ref + 1) * sizeof(double), s0_off = sig_off + (size_t)(total + 1) * sizeof(double);
    const size_t s0_b = sig0.size() * sizeof(int64_t), r_bytes = (size_t)n_sig * p.n_lags * sizeof(double);
    HIP_TRY(hipSetDevice(ctx->device));
    Stage st{ctx};
    char *in;
    P2S_TRY(st.alloc(in, s0_off + s0_b));
    P2S_TRY(st.alloc(p.r, r_bytes));
    P2S_TRY(st.alloc(p.argmax, (size_t)n_sig * 16));
    p.ref = (const double *)in; p.sig = (const double *)(in + sig_off); p.sig0 = (const int64_t *)(in + s0_off);
    p.max_corr = (double *)(p.argmax + n_sig);
    P2S_TRY(st.up(p.ref, ref, (size_t)n_ref * sizeof(double)));
    P2S_TRY(st.up(p.sig, sig, (size_t)total * sizeof(double)));
    P2S_TRY(st.up(p.sig0, sig0.data(), s0_b));
    HIP_TRY(p2s_launch_pearson(p, ctx->stream));
    P2S_TRY(st.down(r, p.r, r_bytes));
    P2S_TRY(st.down(argmax, p.argmax, (size_t)n_sig * 8));
    P2S_TRY(st.down(max_corr, p.max_corr, (size_t)n_sig * 8));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    return P2S_OK;
}

}  // extern "C"
