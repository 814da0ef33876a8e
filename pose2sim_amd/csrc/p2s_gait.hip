// p2s_gait.hip -- gait events from a filtered .trc (Utilities/trc_gaitevents.py) and the exact peak finder it needs.
//
//   scipy.signal.find_peaks(x, prominence=p) for every column of a table at once (_local_maxima_1d and _peak_prominences
//   with wlen=None, scipy 1.15.3), bit for bit: peak indices, prominences, left and right bases
//     fp_summary_kernel      per block of 256 samples: max, min, the first and last position of the min, NaN -> max = NaN
//     fp_maxima_kernel       one lane per sample: the left edge of a plateau that is a local maximum marks its midpoint
//     fp_count_kernel, fp_scan_kernel, fp_gather_kernel   ordered compaction of the marks: count per tile, exclusive
//                            scan, write -- no atomic decides a position
//     fp_prominence_kernel   one lane per local maximum: the two scans for its bases, stepping over whole blocks whose
//                            summary says they cannot end the scan; keep = prominence >= p
//     fp_count_kernel, fp_scan_kernel, fp_emit_kernel     the same compaction over the kept maxima
//   The columns stand back to back and every index is a position in that one run ("flat"); a block of 256 flat samples
//   may straddle two columns, and a scan steps over a block only when the block lies inside the range it may look at.
//
//   the contact signals of the two threshold methods, a batch of (file, foot) columns of unequal length at once
//     gait_height_kernel     gait_events_height_coords :430-433: scipy.signal.filtfilt(b, a, (factor x)[1:]) over the
//                            WHOLE column, one lane per column (the recurrence of p2s_iir.h, none of p2s_butter_kernel's
//                            run cutting: zeros are data and a NaN makes the column NaN, as in scipy)
//     gait_speed_kernel      gait_events_fwd_vel :520-525: diff / dt, samples of the wrong sign (and NaN) zeroed, abs, [1:]
//     gait_gauss_kernel      :527 gaussian_filter1d(., 5) = correlate1d with scipy's weights, mode 'reflect'
//     gait_runs_kernel       signal < threshold and start_end_true_seq :116-133: one workgroup per column walks it 256
//                            samples at a time, a scan of the rising and falling edges gives every event its place
//
// Contraction is off for the whole file: prominence is one subtraction, the filters must round as scipy's C loops do.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>
#include <cstring>
#include <vector>

#include "p2s_ctx.h"
#include "p2s_iir.h"

#pragma clang fp contract(off)

#define P2S_GAIT_HEIGHT 0
#define P2S_GAIT_VELOCITY 1
#define P2S_GAIT_MAX_RADIUS 4095

struct FpSummary {
    double mx, mn;               // over the block's samples; mx is NaN when the block holds a NaN (it then ends every scan)
    int32_t first, last;         // the first and the last position (within the block) of a sample equal to mn
};

struct P2sPeaksArgs {
    const double *x;             // [n_cols][n_rows] columns back to back
    FpSummary *sum;              // [n_blocks]
    uint8_t *mark;               // [total] 1: a local maximum (the midpoint of its plateau)
    uint32_t *tile_count;        // [max(n_blocks, cand_tiles)]: one compaction after the other
    long long *tile_off;         // the same size
    long long *n_cand, *n_kept;  // totals of the two compactions
    long long *cand;             // [max_cand] flat index of every local maximum, ascending
    double *cand_prom;           // [max_cand]
    int32_t *cand_lb, *cand_rb;  // [max_cand] bases as rows
    uint8_t *cand_keep;          // [max_cand]
    int64_t *out_peak, *out_lb, *out_rb;   // [capacity] rows
    double *out_prom;            // [capacity]
    int32_t *col_count;          // [n_cols] kept peaks per column (zeroed by the caller)
    int64_t n_rows, total, n_blocks, max_cand, capacity;
    const double *min_prom;      // [n_cols] the prominence bound of every column; NULL: every local maximum is kept
    int32_t n_cols;
};

struct P2sGaitArgs {
    const double *in;            // [max_rows][n_cols] row-major: column c holds col_len[c] samples, the rest is padding
    double *sig;                 // [max_rows - 1][n_cols] the filtered signal: col_len[c] - 1 samples
    double *work;                // height: [max_rows - 1 + 2 padlen][n_cols] forward pass; velocity: [max_rows - 1][n_cols] speeds
    const int64_t *col_len;      // [n_cols]
    const double *dt, *threshold, *factor;   // [n_cols]
    const double *w;             // velocity: 2 radius + 1 weights
    int32_t *on, *off;           // [n_cols][capacity]
    int32_t *n_on, *n_off;       // [n_cols]
    uint8_t *first_low;          // [n_cols] signal[0] < threshold
    int64_t max_rows, capacity;
    int32_t n_cols, method, n_order, padlen, radius, sign;
    double b[P2S_MAX_FILTER_ORDER + 1], a[P2S_MAX_FILTER_ORDER + 1], zi[P2S_MAX_FILTER_ORDER];
};

namespace {

constexpr int FB = 256;                  // samples per summary block and per compaction tile

// exclusive scan of `mine` over a workgroup of 256 lanes; total in every lane.  wave_total: 4 words of LDS.
__device__ __forceinline__ uint32_t block_scan_256(uint32_t mine, uint32_t *wave_total, uint32_t &total) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    uint32_t incl = mine;
    for (int m = 1; m < 64; m <<= 1) {
        const uint32_t up = (uint32_t)__shfl_up((int)incl, m);
        if (lane >= m) incl += up;
    }
    __syncthreads();                                              // wave_total of an earlier round has been read
    if (lane == 63) wave_total[wave] = incl;
    __syncthreads();
    uint32_t before = incl - mine;
    total = 0;
    for (int w = 0; w < 4; ++w) {
        if (w < wave) before += wave_total[w];
        total += wave_total[w];
    }
    return before;
}

// ---- find_peaks ---------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(FB) fp_summary_kernel(const P2sPeaksArgs a) {
    __shared__ double s_mx[4], s_mn[4];
    __shared__ int s_first[4], s_last[4], s_nan[4];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int64_t i = (int64_t)blockIdx.x * FB + tid;
    const bool in = i < a.total;
    const double v = in ? a.x[i] : 0.0;
    const bool is_nan = in && v != v;
    const bool use = in && !is_nan;
    double mx = use ? v : -__builtin_inf(), mn = use ? v : __builtin_inf();
    for (int m = 32; m >= 1; m >>= 1) {
        mx = fmax(mx, __shfl_xor(mx, m));
        mn = fmin(mn, __shfl_xor(mn, m));
    }
    const unsigned long long any_nan = __ballot(is_nan);
    if (lane == 0) { s_mx[wave] = mx; s_mn[wave] = mn; s_nan[wave] = any_nan != 0ULL; }
    __syncthreads();
    mx = fmax(fmax(s_mx[0], s_mx[1]), fmax(s_mx[2], s_mx[3]));
    mn = fmin(fmin(s_mn[0], s_mn[1]), fmin(s_mn[2], s_mn[3]));
    const bool nan_block = s_nan[0] | s_nan[1] | s_nan[2] | s_nan[3];
    const unsigned long long at_min = __ballot(use && v == mn);
    if (lane == 0) {
        s_first[wave] = at_min ? 64 * wave + (__ffsll((long long)at_min) - 1) : FB;
        s_last[wave] = at_min ? 64 * wave + (63 - __clzll((long long)at_min)) : -1;
    }
    __syncthreads();
    if (tid == 0) {
        FpSummary s;
        s.mx = nan_block ? __longlong_as_double(0x7ff8000000000000LL) : mx;
        s.mn = mn;
        s.first = min(min(s_first[0], s_first[1]), min(s_first[2], s_first[3]));
        s.last = max(max(s_last[0], s_last[1]), max(s_last[2], s_last[3]));
        a.sum[blockIdx.x] = s;
    }
}

// _local_maxima_1d: sample i (1 <= i <= n - 2) with x[i - 1] < x[i] opens a plateau; i_ahead runs over the samples equal
// to x[i] while i_ahead < n - 1; a smaller sample right after them makes (i + i_ahead - 1) // 2 a peak.  Whole blocks of
// samples equal to x[i] are stepped over by their summary (min == max == x[i], no NaN).
__global__ void __launch_bounds__(FB) fp_maxima_kernel(const P2sPeaksArgs a) {
    const int64_t g = (int64_t)blockIdx.x * FB + threadIdx.x;
    if (g >= a.total) return;
    const int64_t col = g / a.n_rows, row = g - col * a.n_rows;
    if (row < 1 || row > a.n_rows - 2) return;
    const double v = a.x[g];
    if (!(a.x[g - 1] < v)) return;
    const int64_t i_max = col * a.n_rows + a.n_rows - 1;          // the column's last sample
    int64_t ia = g + 1;
    while (ia < i_max) {
        if ((ia & (FB - 1)) == 0 && ia + FB <= i_max) {           // the block's samples are all below i_max
            const FpSummary s = a.sum[ia >> 8];
            if (s.mx == v && s.mn == v) { ia += FB; continue; }
        }
        if (!(a.x[ia] == v)) break;
        ++ia;
    }
    if (a.x[ia] < v) a.mark[(g + ia - 1) / 2] = 1;               // plateaus are disjoint: one writer per midpoint
}

// ordered compaction, used twice: over the marks of all samples (n = total) and over the keep flags of the local maxima
// (n = *n_dev, known only on the device: the grid covers max_cand and the tiles past n leave at once)
__global__ void __launch_bounds__(FB) fp_count_kernel(const uint8_t *flag, int64_t n, const long long *n_dev, uint32_t *tile_count) {
    __shared__ uint32_t wave_total[4];
    if (n_dev) n = *n_dev;
    const int64_t i = (int64_t)blockIdx.x * FB + threadIdx.x;
    if ((int64_t)blockIdx.x * FB >= n) return;                    // uniform over the workgroup
    uint32_t total;
    block_scan_256(i < n && flag[i] ? 1u : 0u, wave_total, total);
    if (threadIdx.x == 0) tile_count[blockIdx.x] = total;
}

// tile_off <- exclusive scan of tile_count over ceil(n / 256) tiles; *n_out <- the total.  One workgroup.
__global__ void __launch_bounds__(1024) fp_scan_kernel(const uint32_t *tile_count, long long *tile_off, int64_t n, const long long *n_dev,
                                                        long long *n_out) {
    __shared__ uint32_t wave_total[16];
    if (n_dev) n = *n_dev;
    const int64_t n_tiles = (n + FB - 1) / FB;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    unsigned long long carry = 0;
    for (int64_t base = 0; base < n_tiles; base += 1024) {
        const int64_t i = base + tid;
        const uint32_t mine = i < n_tiles ? tile_count[i] : 0u;
        uint32_t incl = mine;
        for (int m = 1; m < 64; m <<= 1) {
            const uint32_t up = (uint32_t)__shfl_up((int)incl, m);
            if (lane >= m) incl += up;
        }
        __syncthreads();                                          // wave_total of the previous round has been read
        if (lane == 63) wave_total[wave] = incl;
        __syncthreads();
        unsigned long long before = carry + (incl - mine), total = 0;
        for (int w = 0; w < 16; ++w) {
            if (w < wave) before += wave_total[w];
            total += wave_total[w];
        }
        if (i < n_tiles) tile_off[i] = (long long)before;
        carry += total;
    }
    if (tid == 0) *n_out = (long long)carry;
}

__global__ void __launch_bounds__(FB) fp_gather_kernel(const P2sPeaksArgs a) {
    __shared__ uint32_t wave_total[4];
    const int64_t i = (int64_t)blockIdx.x * FB + threadIdx.x;
    const bool on = i < a.total && a.mark[i];
    uint32_t total;
    const uint32_t before = block_scan_256(on ? 1u : 0u, wave_total, total);
    const int64_t at = (int64_t)a.tile_off[blockIdx.x] + before;
    if (on && at < a.max_cand) a.cand[at] = i;                   // at < max_cand always: a column has at most (n - 1) / 2 maxima
}

// _peak_prominences, wlen=None: from the peak leftwards while x[i] <= x[peak] (a larger sample or a NaN ends the scan),
// the smallest sample met and the position nearest to the peak that holds it; the same rightwards; prominence =
// x[peak] - max(left_min, right_min).  A block that lies wholly inside the column on the scan's way and whose max is
// <= x[peak] cannot end the scan: its min and that min's nearest position come from the summary.
__global__ void __launch_bounds__(64) fp_prominence_kernel(const P2sPeaksArgs a) {
    const int64_t e = (int64_t)blockIdx.x * 64 + threadIdx.x;
    if (e >= *a.n_cand) return;
    const int64_t p = a.cand[e];
    const int64_t col = p / a.n_rows, lo = col * a.n_rows, hi = lo + a.n_rows - 1;
    const double xp = a.x[p];
    double lmin = xp, rmin = xp;
    int64_t lb = p, rb = p;
    int64_t i = p - 1;
    while (i >= lo) {
        if ((i & (FB - 1)) == FB - 1 && i - (FB - 1) >= lo) {
            const FpSummary s = a.sum[i >> 8];
            if (s.mx <= xp) {
                if (s.mn < lmin) { lmin = s.mn; lb = (i - (FB - 1)) + s.last; }
                i -= FB;
                continue;
            }
        }
        const double v = a.x[i];
        if (!(v <= xp)) break;
        if (v < lmin) { lmin = v; lb = i; }
        --i;
    }
    i = p + 1;
    while (i <= hi) {
        if ((i & (FB - 1)) == 0 && i + (FB - 1) <= hi) {
            const FpSummary s = a.sum[i >> 8];
            if (s.mx <= xp) {
                if (s.mn < rmin) { rmin = s.mn; rb = i + s.first; }
                i += FB;
                continue;
            }
        }
        const double v = a.x[i];
        if (!(v <= xp)) break;
        if (v < rmin) { rmin = v; rb = i; }
        ++i;
    }
    const double prom = xp - (rmin > lmin ? rmin : lmin);
    a.cand_prom[e] = prom;
    a.cand_lb[e] = (int32_t)(lb - lo);
    a.cand_rb[e] = (int32_t)(rb - lo);
    a.cand_keep[e] = !a.min_prom || a.min_prom[col] <= prom;      // scipy: pmin <= prominences, false for a NaN
}

__global__ void __launch_bounds__(FB) fp_emit_kernel(const P2sPeaksArgs a) {
    __shared__ uint32_t wave_total[4];
    const int64_t n = *a.n_cand;
    if ((int64_t)blockIdx.x * FB >= n) return;                    // uniform over the workgroup
    const int64_t e = (int64_t)blockIdx.x * FB + threadIdx.x;
    const bool on = e < n && a.cand_keep[e];
    uint32_t total;
    const uint32_t before = block_scan_256(on ? 1u : 0u, wave_total, total);
    if (!on) return;
    const int64_t at = (int64_t)a.tile_off[blockIdx.x] + before;
    const int64_t p = a.cand[e], col = p / a.n_rows;
    atomicAdd(&a.col_count[col], 1);                              // an integer count: the order of arrival does not matter
    if (at < a.capacity) {
        a.out_peak[at] = p - col * a.n_rows;
        a.out_prom[at] = a.cand_prom[e];
        a.out_lb[at] = a.cand_lb[e];
        a.out_rb[at] = a.cand_rb[e];
    }
}

// ---- contact signals ------------------------------------------------------------------------------------------------------
// scipy.signal.filtfilt(b, a, x) with its defaults (padtype 'odd', padlen = 3 max(len(a), len(b)), lfilter_zi start) on
// x = (factor * column)[1:], the whole of it.  The host refuses a column with len(x) <= padlen, as scipy does.
template <int N>
__global__ void __launch_bounds__(64) gait_height_kernel(const P2sGaitArgs a) {
    const int col = blockIdx.x * 64 + threadIdx.x;
    if (col >= a.n_cols) return;
    const int64_t S = a.n_cols, L = a.col_len[col] - 1, pad = a.padlen;
    if (L <= pad) return;
    const double fac = a.factor[col];
    const double *x = a.in + S + col;                             // the column from its second sample
    double *work = a.work + col, *out = a.sig + col;
    const double x0 = x[0] * fac, xl = x[(L - 1) * S] * fac;
    const int64_t E = L + 2 * pad;
    auto ext = [&](int64_t i) -> double {
        if (i < pad) return 2.0 * x0 - x[(pad - i) * S] * fac;
        if (i < pad + L) return x[(i - pad) * S] * fac;
        return 2.0 * xl - x[(L - 2 - (i - pad - L)) * S] * fac;
    };
    double z[N];
    const double e0 = ext(0);
#pragma unroll
    for (int k = 0; k < N; ++k) z[k] = a.zi[k] * e0;
    int64_t i = 0;
    for (; i < pad; ++i) work[i * S] = iir_step<N>(a.b, a.a, z, ext(i));
    for (; i + 8 <= pad + L; i += 8) {                            // eight loads in flight ahead of the recurrence
        double v[8];
#pragma unroll
        for (int k = 0; k < 8; ++k) v[k] = x[(i + k - pad) * S];
#pragma unroll
        for (int k = 0; k < 8; ++k) work[(i + k) * S] = iir_step<N>(a.b, a.a, z, v[k] * fac);
    }
    for (; i < E; ++i) work[i * S] = iir_step<N>(a.b, a.a, z, ext(i));
    const double y0 = work[(E - 1) * S];
#pragma unroll
    for (int k = 0; k < N; ++k) z[k] = a.zi[k] * y0;
    i = E - 1;
    for (; i >= pad + L; --i) (void)iir_step<N>(a.b, a.a, z, work[i * S]);
    for (; i - 7 >= pad; i -= 8) {
        double v[8];
#pragma unroll
        for (int k = 0; k < 8; ++k) v[k] = work[(i - k) * S];
#pragma unroll
        for (int k = 0; k < 8; ++k) out[(i - k - pad) * S] = iir_step<N>(a.b, a.a, z, v[k]);
    }
    for (; i >= pad; --i) out[(i - pad) * S] = iir_step<N>(a.b, a.a, z, work[i * S]);
}

// speed[k] = |v| where v = (factor x[k + 1] - factor x[k]) / dt has the sign of the direction, else 0 (pandas' where:
// a NaN fails the comparison and becomes 0)
__global__ void __launch_bounds__(256) gait_speed_kernel(const P2sGaitArgs a) {
    const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int64_t S = a.n_cols;
    if (idx >= (a.max_rows - 1) * S) return;
    const int64_t k = idx / S, c = idx - k * S;
    if (k >= a.col_len[c] - 1) return;
    const double fac = a.factor[c];
    const double v = (a.in[idx + S] * fac - a.in[idx] * fac) / a.dt[c];
    const bool keep = a.sign < 0 ? v < 0.0 : v > 0.0;
    a.work[idx] = keep ? fabs(v) : 0.0;
}

// correlate1d(speed, weights, mode='reflect') as p2s_gauss_kernel adds it: centre tap, then the pairs from the far end
__global__ void __launch_bounds__(256) gait_gauss_kernel(const P2sGaitArgs a) {
    const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int64_t S = a.n_cols;
    if (idx >= (a.max_rows - 1) * S) return;
    const int64_t f = idx / S, c = idx - f * S, F = a.col_len[c] - 1;
    if (f >= F) return;
    const int r = a.radius;
    auto at = [&](int64_t i) -> double {                           // 'reflect': d c b a | a b c d | d c b a
        while (i < 0 || i >= F) i = (i < 0) ? -i - 1 : 2 * F - 1 - i;
        return a.work[i * S + c];
    };
    double acc = a.work[idx] * a.w[r];
    for (int k = -r; k < 0; ++k) acc += (at(f + k) + at(f - k)) * a.w[k + r];
    a.sig[idx] = acc;
}

// low = signal < threshold; start_end_true_seq: on = the samples i >= 1 with low[i] and not low[i - 1] (the reference
// takes index 0 off the list), off = i - 1 for the samples i >= 1 with low[i - 1] and not low[i] (its -1 is dropped).
__global__ void __launch_bounds__(FB) gait_runs_kernel(const P2sGaitArgs a) {
    __shared__ uint32_t wave_total[4];
    const int col = blockIdx.x, tid = threadIdx.x;
    const int64_t S = a.n_cols, L = a.col_len[col] - 1;
    const double thr = a.threshold[col];
    const double *s = a.sig + col;
    int32_t *on = a.on + (int64_t)col * a.capacity, *off = a.off + (int64_t)col * a.capacity;
    uint32_t n_on = 0, n_off = 0;
    for (int64_t base = 0; base < L; base += FB) {                // uniform trip count
        const int64_t i = base + tid;
        bool rise = false, fall = false;
        if (i >= 1 && i < L) {
            const bool cur = s[i * S] < thr, prev = s[(i - 1) * S] < thr;
            rise = cur && !prev;
            fall = prev && !cur;
        }
        uint32_t total;
        const uint32_t before = block_scan_256((rise ? 1u : 0u) | (fall ? 0x10000u : 0u), wave_total, total);
        if (rise && n_on + (before & 0xffffu) < a.capacity) on[n_on + (before & 0xffffu)] = (int32_t)i;
        if (fall && n_off + (before >> 16) < a.capacity) off[n_off + (before >> 16)] = (int32_t)(i - 1);
        n_on += total & 0xffffu;
        n_off += total >> 16;
    }
    if (tid == 0) {
        a.n_on[col] = (int32_t)n_on;
        a.n_off[col] = (int32_t)n_off;
        a.first_low[col] = L >= 1 && s[0] < thr;
    }
}

}  // namespace

static hipError_t p2s_launch_find_peaks(const P2sPeaksArgs &a, hipStream_t s) {
    const unsigned blocks = (unsigned)a.n_blocks, cand_tiles = (unsigned)((a.max_cand + FB - 1) / FB);
    hipLaunchKernelGGL(fp_summary_kernel, dim3(blocks), dim3(FB), 0, s, a);
    hipLaunchKernelGGL(fp_maxima_kernel, dim3(blocks), dim3(FB), 0, s, a);
    hipLaunchKernelGGL(fp_count_kernel, dim3(blocks), dim3(FB), 0, s, (const uint8_t *)a.mark, a.total, (const long long *)nullptr, a.tile_count);
    hipLaunchKernelGGL(fp_scan_kernel, dim3(1), dim3(1024), 0, s, (const uint32_t *)a.tile_count, a.tile_off, a.total, (const long long *)nullptr, a.n_cand);
    hipLaunchKernelGGL(fp_gather_kernel, dim3(blocks), dim3(FB), 0, s, a);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    if (a.max_cand > 0) {
        hipLaunchKernelGGL(fp_prominence_kernel, dim3((unsigned)((a.max_cand + 63) / 64)), dim3(64), 0, s, a);
        hipLaunchKernelGGL(fp_count_kernel, dim3(cand_tiles), dim3(FB), 0, s, (const uint8_t *)a.cand_keep, (int64_t)0, (const long long *)a.n_cand, a.tile_count);
    }
    hipLaunchKernelGGL(fp_scan_kernel, dim3(1), dim3(1024), 0, s, (const uint32_t *)a.tile_count, a.tile_off, (int64_t)0, (const long long *)a.n_cand, a.n_kept);
    if (a.max_cand > 0) hipLaunchKernelGGL(fp_emit_kernel, dim3(cand_tiles), dim3(FB), 0, s, a);
    return hipGetLastError();
}

static hipError_t p2s_launch_gait(const P2sGaitArgs &a, hipStream_t s) {
    const unsigned grid_c = (unsigned)((a.n_cols + 63) / 64);
    const int64_t cells = (a.max_rows - 1) * a.n_cols;
    if (a.method == P2S_GAIT_HEIGHT) {
        switch (a.n_order) {
        case 1: hipLaunchKernelGGL((gait_height_kernel<1>), dim3(grid_c), dim3(64), 0, s, a); break;
        case 2: hipLaunchKernelGGL((gait_height_kernel<2>), dim3(grid_c), dim3(64), 0, s, a); break;
        case 3: hipLaunchKernelGGL((gait_height_kernel<3>), dim3(grid_c), dim3(64), 0, s, a); break;
        case 4: hipLaunchKernelGGL((gait_height_kernel<4>), dim3(grid_c), dim3(64), 0, s, a); break;
        case 5: hipLaunchKernelGGL((gait_height_kernel<5>), dim3(grid_c), dim3(64), 0, s, a); break;
        case 6: hipLaunchKernelGGL((gait_height_kernel<6>), dim3(grid_c), dim3(64), 0, s, a); break;
        case 7: hipLaunchKernelGGL((gait_height_kernel<7>), dim3(grid_c), dim3(64), 0, s, a); break;
        case 8: hipLaunchKernelGGL((gait_height_kernel<8>), dim3(grid_c), dim3(64), 0, s, a); break;
        default: return hipErrorInvalidValue;
        }
    } else if (cells > 0) {
        const unsigned grid_e = (unsigned)((cells + 255) / 256);
        hipLaunchKernelGGL(gait_speed_kernel, dim3(grid_e), dim3(256), 0, s, a);
        hipLaunchKernelGGL(gait_gauss_kernel, dim3(grid_e), dim3(256), 0, s, a);
    }
    hipLaunchKernelGGL(gait_runs_kernel, dim3((unsigned)a.n_cols), dim3(FB), 0, s, a);
    return hipGetLastError();
}

// ---- C-ABI entry points (include/p2s.h) ----------------------------------------------------------------------------
extern "C" {

int p2s_find_peaks_host(p2s_ctx *ctx, int64_t n_rows, int32_t n_cols, const double *data, const double *prominence, int64_t capacity, int64_t *peaks, double *prominences, int64_t *left_bases,
                        int64_t *right_bases, int32_t *col_counts, int64_t *n_peaks) {
    if (!ctx) return p2s_set_error(P2S_ERR_INVALID_ARG, "null context");
    if (n_rows < 1 || n_rows >= ((int64_t)1 << 31) || n_cols < 1)
        return p2s_set_error(P2S_ERR_INVALID_ARG, "bad shape: %lld rows, %d columns; expected 1 .. 2^31 - 1 rows and at least 1 column", (long long)n_rows, n_cols);
    if ((int64_t)n_cols * n_rows > ((int64_t)1 << 36)) return p2s_set_error(P2S_ERR_INVALID_ARG, "%lld samples are too many", (long long)n_cols * n_rows);
    if (!data || !col_counts || !n_peaks) return p2s_set_error(P2S_ERR_INVALID_ARG, "null argument");
    if (capacity < 0 || (capacity > 0 && (!peaks || !prominences || !left_bases || !right_bases)))
        return p2s_set_error(P2S_ERR_INVALID_ARG, "capacity=%lld without room", (long long)capacity);
    P2sPeaksArgs a{};
    a.n_rows = n_rows; a.n_cols = n_cols;
    a.total = n_rows * n_cols;
    a.n_blocks = (a.total + FB - 1) / FB;
    a.max_cand = (int64_t)n_cols * ((n_rows - 1) / 2);           // peaks are separated by a smaller sample, none at the ends
    a.capacity = capacity;
    const int64_t tiles = std::max<int64_t>(a.n_blocks, (a.max_cand + FB - 1) / FB);
    const size_t mc = (size_t)a.max_cand, cap = (size_t)capacity;
    Layout lay;                                                   // tile_off, then n_cand and n_kept right behind it
    const size_t o_toff = lay.add(((size_t)tiles + 2) * 8), o_mp = lay.add((size_t)n_cols * 8), o_tc = lay.add((size_t)tiles * 4), o_cc = lay.add((size_t)n_cols * 4);
    HIP_TRY(hipSetDevice(ctx->device));
    Stage st{ctx};
    char *sm, *cd, *ob;
    P2S_TRY(st.upload(a.x, data, (size_t)a.total * sizeof(double)));
    P2S_TRY(st.alloc(a.sum, (size_t)a.n_blocks * sizeof(FpSummary)));
    P2S_TRY(st.alloc(a.mark, (size_t)a.total));
    P2S_TRY(st.alloc(sm, lay.bytes));
    P2S_TRY(st.alloc(cd, mc * 25 + 16));                          // cand i64, prom f64, lb, rb i32, keep u8
    P2S_TRY(st.alloc(ob, cap * 32 + 16));                         // peak, lb, rb i64, prom f64
    a.tile_off = (long long *)(sm + o_toff);
    a.n_cand = a.tile_off + tiles; a.n_kept = a.n_cand + 1;
    a.tile_count = (uint32_t *)(sm + o_tc);
    if (prominence) {
        P2S_TRY(st.up(sm + o_mp, prominence, (size_t)n_cols * 8));
        a.min_prom = (const double *)(sm + o_mp);
    }
    a.col_count = (int32_t *)(sm + o_cc);
    a.cand = (long long *)cd;
    a.cand_prom = (double *)(cd + mc * 8);
    a.cand_lb = (int32_t *)(cd + mc * 16); a.cand_rb = a.cand_lb + mc;
    a.cand_keep = (uint8_t *)(cd + mc * 24);
    a.out_peak = (int64_t *)ob; a.out_lb = a.out_peak + cap; a.out_rb = a.out_lb + cap;
    a.out_prom = (double *)(a.out_rb + cap);
    HIP_TRY(hipMemsetAsync(a.mark, 0, (size_t)a.total, ctx->stream));
    HIP_TRY(hipMemsetAsync(a.col_count, 0, (size_t)n_cols * 4, ctx->stream));
    P2S_TRY(st.time_begin());
    HIP_TRY(p2s_launch_find_peaks(a, ctx->stream));
    P2S_TRY(st.time_end());
    long long found = 0;
    P2S_TRY(st.down(&found, a.n_kept, 8));
    P2S_TRY(st.down(col_counts, a.col_count, (size_t)n_cols * 4));
    P2S_TRY(st.finish(P2S_TIMED_GAIT));                           // `found` is host memory: alive until here
    const size_t n_copy = (size_t)std::min<int64_t>(found, capacity);
    if (n_copy > 0) {
        P2S_TRY(st.down(peaks, a.out_peak, n_copy * 8));
        P2S_TRY(st.down(left_bases, a.out_lb, n_copy * 8));
        P2S_TRY(st.down(right_bases, a.out_rb, n_copy * 8));
        P2S_TRY(st.down(prominences, a.out_prom, n_copy * 8));
        HIP_TRY(hipStreamSynchronize(ctx->stream));
    }
    *n_peaks = found;
    return P2S_OK;
}

int p2s_gait_contacts_host(p2s_ctx *ctx, int32_t method, int32_t n_cols, int64_t max_rows, const int64_t *col_len,
                           const double *data, const double *dt, const double *threshold, const double *factor,
                           int32_t sign, int32_t n_coef, const double *b, const double *a, const double *zi,
                           int32_t n_weights, const double *weights, double *signal, int64_t event_capacity, int32_t *on,
                           int32_t *off, int32_t *n_on, int32_t *n_off, uint8_t *first_low) {
    if (!ctx) return p2s_set_error(P2S_ERR_INVALID_ARG, "null context");
    if (method != P2S_GAIT_HEIGHT && method != P2S_GAIT_VELOCITY) return p2s_set_error(P2S_ERR_INVALID_ARG, "unknown method %d", method);
    if (n_cols < 1 || max_rows < 1 || max_rows >= ((int64_t)1 << 31))
        return p2s_set_error(P2S_ERR_INVALID_ARG, "bad shape: %d columns of at most %lld rows; expected at least 1 column and 1 .. 2^31 - 1 rows", n_cols, (long long)max_rows);
    if (!col_len || !data || !dt || !threshold || !factor || !n_on || !n_off || !first_low) return p2s_set_error(P2S_ERR_INVALID_ARG, "null argument");
    if (event_capacity < 0 || (event_capacity > 0 && (!on || !off))) return p2s_set_error(P2S_ERR_INVALID_ARG, "event_capacity=%lld without room", (long long)event_capacity);
    if (sign != 1 && sign != -1) return p2s_set_error(P2S_ERR_INVALID_ARG, "sign=%d; expected 1 or -1", sign);
    P2sGaitArgs g{};
    g.method = method; g.n_cols = n_cols; g.max_rows = max_rows; g.capacity = event_capacity; g.sign = sign;
    if (method == P2S_GAIT_HEIGHT) {
        if (n_coef < 2 || n_coef > P2S_MAX_FILTER_ORDER + 1)
            return p2s_set_error(P2S_ERR_INVALID_ARG, "filter with %d coefficients: supported 2..%d", n_coef, P2S_MAX_FILTER_ORDER + 1);
        if (!b || !a || !zi) return p2s_set_error(P2S_ERR_INVALID_ARG, "null filter coefficients");
        if (!(a[0] == 1.0)) return p2s_set_error(P2S_ERR_INVALID_ARG, "a[0] must be 1 (scipy.signal.butter normalises it)");
        g.n_order = n_coef - 1; g.padlen = 3 * n_coef;
        for (int i = 0; i < n_coef; ++i) { g.b[i] = b[i]; g.a[i] = a[i]; }
        for (int i = 0; i < n_coef - 1; ++i) g.zi[i] = zi[i];
    } else {
        if (n_weights < 1 || n_weights % 2 != 1 || n_weights > 2 * P2S_GAIT_MAX_RADIUS + 1 || !weights)
            return p2s_set_error(P2S_ERR_INVALID_ARG, "velocity method: 2 radius + 1 weights, radius <= %d", P2S_GAIT_MAX_RADIUS);
        g.radius = n_weights / 2;
    }
    for (int32_t c = 0; c < n_cols; ++c) {
        if (col_len[c] < 1 || col_len[c] > max_rows)
            return p2s_set_error(P2S_ERR_INVALID_ARG, "column %d has %lld rows; expected 1 .. max_rows = %lld", c, (long long)col_len[c], (long long)max_rows);
        if (method == P2S_GAIT_HEIGHT && col_len[c] - 1 <= g.padlen)
            return p2s_set_error(P2S_ERR_INVALID_ARG, "The length of the input vector x must be greater than padlen, which is %d.", g.padlen);
        if (method == P2S_GAIT_VELOCITY && !(dt[c] == dt[c])) return p2s_set_error(P2S_ERR_INVALID_ARG, "column %d: dt is NaN", c);
    }
    const size_t nc = (size_t)n_cols, cells = (size_t)(max_rows - 1) * nc, cap = (size_t)event_capacity;
    const size_t work_rows = (size_t)(max_rows - 1) + (method == P2S_GAIT_HEIGHT ? 2 * (size_t)g.padlen : 0);
    const size_t nw = method == P2S_GAIT_VELOCITY ? (size_t)n_weights : 0;
    Layout lay;                                                   // `host_small` goes up as one: what the caller gave
    const size_t o_len = lay.add(nc * 8), o_dt = lay.add(nc * 8), o_thr = lay.add(nc * 8), o_fac = lay.add(nc * 8), o_w = lay.add(nw * 8), up_b = lay.bytes;
    const size_t o_non = lay.add(nc * 4), o_noff = lay.add(nc * 4), o_first = lay.add(nc);   // and what the kernels count
    std::vector<char> host_small(up_b);
    memcpy(host_small.data() + o_len, col_len, nc * 8);
    memcpy(host_small.data() + o_dt, dt, nc * 8);
    memcpy(host_small.data() + o_thr, threshold, nc * 8);
    memcpy(host_small.data() + o_fac, factor, nc * 8);
    if (nw) memcpy(host_small.data() + o_w, weights, nw * 8);
    HIP_TRY(hipSetDevice(ctx->device));
    Stage st{ctx};
    char *sm;
    P2S_TRY(st.upload(g.in, data, (size_t)max_rows * nc * sizeof(double)));
    P2S_TRY(st.alloc(g.sig, cells * sizeof(double)));
    P2S_TRY(st.alloc(g.work, work_rows * nc * sizeof(double)));
    P2S_TRY(st.alloc(sm, lay.bytes));
    P2S_TRY(st.alloc(g.on, 2 * nc * cap * 4 + 16));
    P2S_TRY(st.up(sm, host_small.data(), up_b));
    g.off = g.on + nc * cap;
    g.col_len = (const int64_t *)(sm + o_len);
    g.dt = (const double *)(sm + o_dt); g.threshold = (const double *)(sm + o_thr); g.factor = (const double *)(sm + o_fac);
    g.w = (const double *)(sm + o_w);
    g.n_on = (int32_t *)(sm + o_non); g.n_off = (int32_t *)(sm + o_noff);
    g.first_low = (uint8_t *)(sm + o_first);
    P2S_TRY(st.time_begin());
    HIP_TRY(p2s_launch_gait(g, ctx->stream));
    P2S_TRY(st.time_end());
    P2S_TRY(st.down(signal, g.sig, cells * sizeof(double)));
    P2S_TRY(st.down(n_on, g.n_on, nc * 4));
    P2S_TRY(st.down(n_off, g.n_off, nc * 4));
    P2S_TRY(st.down(first_low, g.first_low, nc));
    P2S_TRY(st.down(on, g.on, nc * cap * 4));
    P2S_TRY(st.down(off, g.off, nc * cap * 4));
    return st.finish(P2S_TIMED_GAIT);                             // `host_small` is host memory: alive until here
}

int p2s_gait_kernel_ms(p2s_ctx *ctx, float *elapsed_ms) {
    return p2s_kernel_ms_query(ctx, P2S_TIMED_GAIT, "neither p2s_find_peaks_host nor p2s_gait_contacts_host", elapsed_ms);
}

}  // extern "C"
