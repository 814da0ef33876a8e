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

#include "p2s_internal.h"
#include "p2s_iir.h"

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

hipError_t p2s_launch_sync_speeds(const P2sSyncArgs &a, hipStream_t s) {
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

hipError_t p2s_launch_pearson(const P2sPearsonArgs &a, hipStream_t s) {
    if (a.n_sig == 0 || a.n_lags == 0) return hipSuccess;
    const int64_t groups = (a.n_lags + kLagsPerWave - 1) / kLagsPerWave;
    hipLaunchKernelGGL(p2s_pearson_kernel, dim3((unsigned)((groups + 3) / 4), (unsigned)a.n_sig), dim3(256), 0, s, a);
    hipLaunchKernelGGL(p2s_pearson_argmax_kernel, dim3((unsigned)a.n_sig), dim3(256), 0, s, a);
    return hipGetLastError();
}
