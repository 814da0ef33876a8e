// p2s_confidence.hip -- 2D confidence statistics (Utilities/pose_confidence_analyze.py:118-219) and the primitive they
// need: np.mean and np.std of a long column, bit for bit.  float64 end to end.
//
//   conf_transpose_kernel  the cameras' tables [frames][K] -> one contiguous column per (camera, keypoint), NaN kept
//   conf_compact_kernel    per column: the non-NaN entries in frame order (stable), their count m, min and max, the five
//                          band counts (compute_band_distribution :157-190) and the counts below up to 8 thresholds
//                          (compute_statistics :152, simulate_threshold :193-219)
//   conf_mean_std_kernel   per column: np.mean and np.std of the compacted entries, summed in NumPy's order
//   order_stats_kernel     (p2s_jitter.hip) per column: np.percentile's two neighbours for 5, 25, 50, 75 and 95 %
//   conf_finish_kernel     median, percentile interpolation -> stats [column][9]
//
// NumPy's sum.  np.add.reduce of m contiguous doubles starts from +0.0 and adds, left to right, the sums of consecutive
// chunks of 8192 entries (the ufunc buffer).  A chunk's sum is pairwise(a, n): n <= 128 is a leaf -- below 8 terms a plain
// loop from 0.0; else eight accumulators r[j] = a[j], r[j] += a[i + j] over the whole blocks of 8,
// ((r0+r1)+(r2+r3))+((r4+r5)+(r6+r7)), then the tail one by one -- and a longer run splits at n2 = n / 2 rounded down to
// a multiple of 8.  The tree's shape depends on n alone, it is at most 7 levels deep and has at most 128 leaves (every
// leaf of a split run has 64 terms or more), so a chunk is one step of a workgroup of 1024 lanes: 128 slots of 8 lanes, a
// slot's number read as the path from the root (most significant bit first).  A slot whose path ends on a leaf before
// its bits run out stands for that leaf only when the bits left over are 0: the leftmost leaf of every subtree sits on the
// subtree's own slot, so "the slot at s + stride holds a leaf" is "the right subtree at this level exists".  Lane j of a
// slot is accumulator r[j]; the fixed combine is a butterfly over lane distance 1, 2, 4 (a + b is b + a, so both sides
// hold the reference's bits); the levels are lane distance 8, 16, 32 and then the sixteen waves' values through LDS.
// np.mean = sum / m; np.std = sqrt(sum((x - mean) * (x - mean)) / m), each operation rounded once: floating-point
// contraction is off for this whole file and the root is the correctly rounded __dsqrt_rn.  No floating-point atomic
// anywhere: two runs give the same bytes.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>
#include <vector>

#include "p2s_ctx.h"
#include "p2s_npsum.h"                       // CT, CW, cf_sum: np.add.reduce

#pragma clang fp contract(off)

#define P2S_CONF_MAX_K 64
#define P2S_CONF_MAX_THRESHOLDS 8
#define P2S_CONF_BANDS 5
#define P2S_CONF_STATS 9         // mean, median, std, min, max, p5, p25, p75, p95
#define P2S_CONF_QUANTILES 5     // 5, 25, 50, 75, 95 %: two neighbours each
struct P2sConfArgs {
    const double *tables;        // [frames][K], cameras back to back (the transposition's input)
    const int64_t *frame_off;    // [C + 1]
    double *cols;                // one column per (camera, keypoint): camera c's K columns of F_c entries from K * frame_off[c]
    const int64_t *col_off;      // [n_cols] first element of every column in cols and valid, or NULL: col * n_rows
    const int64_t *col_len;      // [n_cols] entries of every column, or NULL: n_rows
    double *valid;               // the columns' non-NaN entries, each at its column's offset
    int64_t *m;                  // [n_cols] non-NaN entries
    const double *thresholds;    // [n_thr]
    int64_t *below;              // [n_thr][n_cols] entries < threshold, or NULL
    int64_t *bands;              // [n_cols][5], or NULL
    double *minmax;              // [n_cols][2]
    double *mean_std;            // [n_cols][2]
    const double *fractions;     // [5] 0.05, 0.25, 0.5, 0.75, 0.95
    const double *order;         // [n_cols][10] the entries at np.percentile's lo and hi of every fraction
    double *stats;               // [n_cols][9]
    int64_t n_rows, max_frames;
    int32_t C, K, n_cols, n_thr;
};

namespace {

constexpr int TF = 64;                   // frames per workgroup of the transposition
constexpr int UNR = 4;                   // entries per lane and round of the compaction: UNR * CW = 64 wave counts, one wave's scan

__device__ __forceinline__ double cf_nan() { return __longlong_as_double(0x7ff8000000000000LL); }
__device__ __forceinline__ double cf_inf() { return __longlong_as_double(0x7ff0000000000000LL); }

// ---- [frames][K] -> columns ------------------------------------------------------------------------------------------
// A workgroup reads 64 frames of one camera back to back (64 K doubles) and stores K runs of 512 bytes.
__global__ void __launch_bounds__(256) conf_transpose_kernel(const P2sConfArgs a) {
    __shared__ double tile[P2S_CONF_MAX_K][TF + 1];
    const int c = blockIdx.y, K = a.K;
    const int64_t f_base = a.frame_off[c];
    const int64_t F = a.frame_off[c + 1] - f_base;
    const int64_t t0 = (int64_t)blockIdx.x * TF;
    if (t0 >= F) return;                                          // uniform over the workgroup
    const int nf = (int)(F - t0 < TF ? F - t0 : TF);
    const double *src = a.tables + (f_base + t0) * K;
    for (int i = threadIdx.x; i < nf * K; i += 256) tile[i % K][i / K] = src[i];
    __syncthreads();
    double *dst = a.cols + f_base * K;
    for (int i = threadIdx.x; i < K * TF; i += 256) {
        const int k = i / TF, j = i % TF;
        if (j < nf) dst[k * F + t0 + j] = tile[k][j];
    }
}

// ---- stable compaction, counts, min and max -----------------------------------------------------------------------------
// One workgroup per column walks it 4096 entries a round: entry base + u * 1024 + tid, u < 4.  A wave's ballot gives
// every lane its place among the wave's entries; the 64 (u, wave) totals are scanned by every wave for itself (one
// entry a lane), and a running carry places the round.  Counts are integers, kept per lane and added up at the end.
constexpr int N_COUNTS = P2S_CONF_BANDS + P2S_CONF_MAX_THRESHOLDS;
__global__ void __launch_bounds__(CT) conf_compact_kernel(const P2sConfArgs a) {
    __shared__ uint32_t wave_count[2][UNR * CW];
    __shared__ uint32_t wave_sums[CW][N_COUNTS];
    __shared__ double wave_lo[CW], wave_hi[CW];
    __shared__ double thr[P2S_CONF_MAX_THRESHOLDS];
    const int col = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int64_t off = a.col_off ? a.col_off[col] : (int64_t)col * a.n_rows;
    const int64_t n = a.col_len ? a.col_len[col] : a.n_rows;
    const double *x = a.cols + off;
    double *y = a.valid + off;
    const int n_thr = a.below ? a.n_thr : 0;
    if (tid < P2S_CONF_MAX_THRESHOLDS) thr[tid] = tid < n_thr ? a.thresholds[tid] : cf_nan();   // nothing is below NaN
    __syncthreads();
    uint32_t cnt[N_COUNTS];
    for (int i = 0; i < N_COUNTS; ++i) cnt[i] = 0u;
    double lo = cf_inf(), hi = -cf_inf();
    const unsigned long long lanes_below = (1ULL << lane) - 1ULL;
    int64_t carry = 0;                                            // entries kept so far; the same in every lane
    int par = 0;
    for (int64_t base = 0; base < n; base += UNR * CT, par ^= 1) {   // uniform trip count: the ballots need every lane
        double v[UNR];
        uint32_t place[UNR];
#pragma unroll
        for (int u = 0; u < UNR; ++u) {
            const int64_t i = base + u * CT + tid;
            v[u] = i < n ? x[i] : cf_nan();
            const unsigned long long b = __ballot(v[u] == v[u]);
            place[u] = (uint32_t)__popcll(b & lanes_below);
            if (lane == 0) wave_count[par][u * CW + wave] = (uint32_t)__popcll(b);
        }
        __syncthreads();                                          // the other half of wave_count is free: every wave has
        const uint32_t mine = wave_count[par][lane];              // passed this barrier since it last read it
        uint32_t incl = mine;
        for (int s = 1; s < 64; s <<= 1) {
            const uint32_t up = (uint32_t)__shfl_up((int)incl, s);
            if (lane >= s) incl += up;
        }
        const uint32_t excl = incl - mine;
#pragma unroll
        for (int u = 0; u < UNR; ++u) {
            const uint32_t before = (uint32_t)__shfl((int)excl, u * CW + wave);
            const double w = v[u];
            if (w == w) {
                y[carry + before + place[u]] = w;                 // carry + before + place < m <= n: inside the column
                lo = fmin(lo, w); hi = fmax(hi, w);
                cnt[0] += w >= 0.0 && w < 0.4;                    // CONFIDENCE_BANDS :42-48
                cnt[1] += w >= 0.4 && w < 0.6;
                cnt[2] += w >= 0.6 && w < 0.8;
                cnt[3] += w >= 0.8 && w <= 1.0;                   // 'high' is closed above: 1.0 counts here and in the next
                cnt[4] += w >= 1.0 && w < cf_inf();
#pragma unroll
                for (int t = 0; t < P2S_CONF_MAX_THRESHOLDS; ++t) cnt[P2S_CONF_BANDS + t] += w < thr[t];
            }
        }
        carry += (uint32_t)__shfl((int)incl, 63);
    }
    // the lanes' counts and extremes -> the column's
#pragma unroll
    for (int i = 0; i < N_COUNTS; ++i) {
        uint32_t s = cnt[i];                                      // a lane holds at most 2^21, a wave at most 2^27
        for (int d = 32; d >= 1; d >>= 1) s += (uint32_t)__shfl_xor((int)s, d);
        if (lane == 0) wave_sums[wave][i] = s;
    }
    for (int d = 32; d >= 1; d >>= 1) {
        lo = fmin(lo, __shfl_xor(lo, d));
        hi = fmax(hi, __shfl_xor(hi, d));
    }
    if (lane == 0) { wave_lo[wave] = lo; wave_hi[wave] = hi; }
    __syncthreads();
    if (tid < N_COUNTS) {
        int64_t s = 0;
        for (int w = 0; w < CW; ++w) s += wave_sums[w][tid];
        if (tid < P2S_CONF_BANDS) { if (a.bands) a.bands[(int64_t)col * P2S_CONF_BANDS + tid] = s; }
        else if (tid - P2S_CONF_BANDS < n_thr) a.below[(int64_t)(tid - P2S_CONF_BANDS) * a.n_cols + col] = s;
    }
    if (tid == 0) {
        for (int w = 1; w < CW; ++w) { lo = fmin(lo, wave_lo[w]); hi = fmax(hi, wave_hi[w]); }
        a.m[col] = carry;
        a.minmax[2 * (int64_t)col] = carry ? lo : cf_nan();
        a.minmax[2 * (int64_t)col + 1] = carry ? hi : cf_nan();
    }
}

// ---- np.mean, np.std (np.add.reduce: cf_sum of p2s_npsum.h) --------------------------------------------------------------
__global__ void __launch_bounds__(CT) conf_mean_std_kernel(const P2sConfArgs a) {
    __shared__ CfShared s;
    const int col = blockIdx.x;
    const double *x = a.valid + (a.col_off ? a.col_off[col] : (int64_t)col * a.n_rows);
    const int64_t m = a.m[col];
    const double mean = cf_sum<false>(s, x, m, 0.0) / (double)m;
    const double var = cf_sum<true>(s, x, m, mean) / (double)m;
    if (threadIdx.x == 0) {
        a.mean_std[2 * (int64_t)col] = m ? mean : cf_nan();
        a.mean_std[2 * (int64_t)col + 1] = m ? __dsqrt_rn(var) : cf_nan();
    }
}

// ---- median, percentiles -----------------------------------------------------------------------------------------------
// np.percentile, method 'linear': vi = (m - 1) * fraction, g = vi - floor(vi), d = s[hi] - s[lo]; s[lo] + d * g, replaced
// by s[hi] - d * (1 - g) where g >= 0.5.  np.median: the mean of the one or two middle entries, added to +0.0.
__global__ void conf_finish_kernel(const P2sConfArgs a) {
    const int col = blockIdx.x * blockDim.x + threadIdx.x;
    if (col >= a.n_cols) return;
    const int64_t m = a.m[col];
    double *out = a.stats + (int64_t)col * P2S_CONF_STATS;
    if (m == 0) {
        for (int i = 0; i < P2S_CONF_STATS; ++i) out[i] = cf_nan();
        return;
    }
    const double *q = a.order + (int64_t)col * 2 * P2S_CONF_QUANTILES;
    double pct[P2S_CONF_QUANTILES];
    for (int i = 0; i < P2S_CONF_QUANTILES; ++i) {
        const double vi = (double)(m - 1) * a.fractions[i];
        const double g = vi - floor(vi);
        const double lo = q[2 * i], hi = q[2 * i + 1], d = hi - lo;
        pct[i] = g >= 0.5 ? hi - d * (1.0 - g) : lo + d * g;
    }
    const double mid = 0.0 + q[4];                                // fraction 0.5: lo = (m - 1) / 2, hi = m / 2 when m is even
    out[0] = a.mean_std[2 * (int64_t)col];
    out[1] = (m & 1) ? mid : (mid + q[5]) / 2.0;
    out[2] = a.mean_std[2 * (int64_t)col + 1];
    out[3] = a.minmax[2 * (int64_t)col];
    out[4] = a.minmax[2 * (int64_t)col + 1];
    out[5] = pct[0]; out[6] = pct[1]; out[7] = pct[3]; out[8] = pct[4];
}

hipError_t launch_columns(const P2sConfArgs &a, hipStream_t s) {  // compaction, then mean and std
    if (a.n_cols == 0) return hipSuccess;
    hipLaunchKernelGGL(conf_compact_kernel, dim3((unsigned)a.n_cols), dim3(CT), 0, s, a);
    hipLaunchKernelGGL(conf_mean_std_kernel, dim3((unsigned)a.n_cols), dim3(CT), 0, s, a);
    return hipGetLastError();
}

hipError_t launch_confidence(const P2sConfArgs &a, hipStream_t s) {
    const unsigned tiles = (unsigned)((a.max_frames + TF - 1) / TF);
    hipLaunchKernelGGL(conf_transpose_kernel, dim3(tiles, (unsigned)a.C), dim3(256), 0, s, a);
    hipError_t e = launch_columns(a, s);
    if (e != hipSuccess) return e;
    P2sOrderArgs o{};
    o.data = a.valid; o.col_off = a.col_off; o.col_len = a.m;     // the compacted columns: m entries, none NaN
    o.fractions = a.fractions;
    o.out = const_cast<double *>(a.order);
    o.n_cols = a.n_cols; o.n_ranks = 2 * P2S_CONF_QUANTILES;
    if ((e = p2s_launch_order_stats(o, s)) != hipSuccess) return e;
    hipLaunchKernelGGL(conf_finish_kernel, dim3((unsigned)((a.n_cols + 63) / 64)), dim3(64), 0, s, a);
    return hipGetLastError();
}

}  // namespace

hipError_t p2s_launch_column_moments(const double *cols, double *valid, int64_t n_rows, int32_t n_cols, int64_t *m, double *minmax,
                                     double *mean_std, hipStream_t s) {   // also p2s_idswitch.hip
    P2sConfArgs a{};
    a.cols = const_cast<double *>(cols); a.valid = valid; a.m = m; a.minmax = minmax; a.mean_std = mean_std;
    a.n_rows = n_rows; a.n_cols = n_cols;
    return launch_columns(a, s);
}

// ---- C-ABI entry points (include/p2s.h) ----------------------------------------------------------------------------
extern "C" {

int p2s_column_mean_std_host(p2s_ctx *ctx, int64_t n_rows, int32_t n_cols, const double *data, double *mean, double *std,
                             int64_t *counts) {
    if (!ctx) return p2s_set_error(P2S_ERR_INVALID_ARG, "null context");
    if (n_rows < 0 || n_rows >= ((int64_t)1 << 31) || n_cols < 0)
        return p2s_set_error(P2S_ERR_INVALID_ARG, "bad shape: %lld rows, %d columns", (long long)n_rows, n_cols);
    if (n_cols == 0) return P2S_OK;
    if (n_rows > 0 && !data) return p2s_set_error(P2S_ERR_INVALID_ARG, "null argument");
    const size_t nc = (size_t)n_cols, data_b = (size_t)n_rows * nc * sizeof(double);
    HIP_TRY(hipSetDevice(ctx->device));
    P2sConfArgs a{};
    a.n_rows = n_rows; a.n_cols = n_cols;
    Stage st{ctx};
    const double *d_data;
    P2S_TRY(st.upload(d_data, data, data_b));
    a.cols = const_cast<double *>(d_data);
    P2S_TRY(st.alloc(a.valid, data_b));
    P2S_TRY(st.alloc(a.m, nc * 40));                              // m [nc] i64, min and max [nc][2], mean and std [nc][2]
    a.minmax = (double *)(a.m + nc);
    a.mean_std = a.minmax + 2 * nc;
    HIP_TRY(launch_columns(a, ctx->stream));
    std::vector<double> ms(2 * nc);
    P2S_TRY(st.down(ms.data(), a.mean_std, 2 * nc * sizeof(double)));
    P2S_TRY(st.down(counts, a.m, nc * sizeof(int64_t)));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    for (size_t c = 0; c < nc; ++c) {
        if (mean) mean[c] = ms[2 * c];
        if (std) std[c] = ms[2 * c + 1];
    }
    return P2S_OK;
}

int p2s_confidence_stats_host(p2s_ctx *ctx, int32_t n_cams, const int64_t *n_frames, int32_t n_kpts, const double *tables,
                              int32_t n_thresholds, const double *thresholds, double *stats, int64_t *counts, int64_t *below,
                              int64_t *bands) {
    if (!ctx) return p2s_set_error(P2S_ERR_INVALID_ARG, "null context");
    P2S_TRY(p2s_check_n_cams(n_cams));
    if (n_kpts < 1 || n_kpts > P2S_CONF_MAX_K) return p2s_set_error(P2S_ERR_INVALID_ARG, "n_kpts=%d outside [1, %d]", n_kpts, P2S_CONF_MAX_K);
    if (n_thresholds < 0 || n_thresholds > P2S_CONF_MAX_THRESHOLDS)
        return p2s_set_error(P2S_ERR_INVALID_ARG, "n_thresholds=%d outside [0, %d]", n_thresholds, P2S_CONF_MAX_THRESHOLDS);
    if (!n_frames || !tables || (n_thresholds > 0 && !thresholds)) return p2s_set_error(P2S_ERR_INVALID_ARG, "null argument");
    const size_t C = (size_t)n_cams, K = (size_t)n_kpts, nc = C * K, T = (size_t)n_thresholds;
    Layout lay;                                                   // `tab` goes up as one: what the host knows
    const size_t o_foff = lay.add((C + 1) * 8), o_coff = lay.add(nc * 8), o_clen = lay.add(nc * 8), o_frac = lay.add(P2S_CONF_QUANTILES * 8),
                 o_thr = lay.add(P2S_CONF_MAX_THRESHOLDS * 8), tab_b = lay.bytes;
    // and what the kernels leave on the device
    const size_t o_m = lay.add(nc * 8), o_below = lay.add(P2S_CONF_MAX_THRESHOLDS * nc * 8), o_bands = lay.add(P2S_CONF_BANDS * nc * 8), o_mm = lay.add(2 * nc * 8),
                 o_ms = lay.add(2 * nc * 8), o_ord = lay.add(2 * P2S_CONF_QUANTILES * nc * 8), o_stats = lay.add(P2S_CONF_STATS * nc * 8);
    std::vector<char> tab(tab_b);
    int64_t *frame_off = (int64_t *)(tab.data() + o_foff), *col_off = (int64_t *)(tab.data() + o_coff), *col_len = (int64_t *)(tab.data() + o_clen);
    P2sFrames fr;
    P2S_TRY(fr.build(n_cams, n_frames, 1, (int64_t)1 << 33, frame_off));
    const int64_t frames = fr.frames, max_frames = fr.max_frames;
    for (size_t c = 0; c < C; ++c)
        for (size_t k = 0; k < K; ++k) {
            col_off[c * K + k] = (int64_t)K * frame_off[c] + (int64_t)k * n_frames[c];
            col_len[c * K + k] = n_frames[c];
        }
    double *up_frac = (double *)(tab.data() + o_frac), *up_thr = (double *)(tab.data() + o_thr);
    const double fractions[P2S_CONF_QUANTILES] = {5 / 100.0, 25 / 100.0, 50 / 100.0, 75 / 100.0, 95 / 100.0};   // np.percentile: q / 100
    for (int i = 0; i < P2S_CONF_QUANTILES; ++i) up_frac[i] = fractions[i];
    for (size_t t = 0; t < P2S_CONF_MAX_THRESHOLDS; ++t) up_thr[t] = t < T ? thresholds[t] : 0.0;
    const size_t table_b = (size_t)frames * K * sizeof(double);
    HIP_TRY(hipSetDevice(ctx->device));
    P2sConfArgs a{};
    Stage st{ctx};
    char *sm;
    P2S_TRY(st.upload(a.tables, tables, table_b));
    P2S_TRY(st.alloc(a.cols, table_b));
    P2S_TRY(st.alloc(a.valid, table_b));
    P2S_TRY(st.alloc(sm, lay.bytes));
    P2S_TRY(st.up(sm, tab.data(), tab_b));
    a.frame_off = (const int64_t *)(sm + o_foff); a.col_off = (const int64_t *)(sm + o_coff); a.col_len = (const int64_t *)(sm + o_clen);
    a.fractions = (const double *)(sm + o_frac); a.thresholds = (const double *)(sm + o_thr);
    a.m = (int64_t *)(sm + o_m); a.below = (int64_t *)(sm + o_below); a.bands = (int64_t *)(sm + o_bands);
    a.minmax = (double *)(sm + o_mm); a.mean_std = (double *)(sm + o_ms);
    a.order = (const double *)(sm + o_ord); a.stats = (double *)(sm + o_stats);
    a.max_frames = max_frames;
    a.C = n_cams; a.K = n_kpts; a.n_cols = (int32_t)nc; a.n_thr = n_thresholds;
    P2S_TRY(st.time_begin());
    HIP_TRY(launch_confidence(a, ctx->stream));
    P2S_TRY(st.time_end());
    P2S_TRY(st.down(stats, a.stats, P2S_CONF_STATS * nc * 8));
    P2S_TRY(st.down(counts, a.m, nc * 8));
    P2S_TRY(st.down(below, a.below, T * nc * 8));
    P2S_TRY(st.down(bands, a.bands, P2S_CONF_BANDS * nc * 8));
    return st.finish(P2S_TIMED_CONFIDENCE);                       // `tab` is host memory: alive until here
}

int p2s_confidence_kernel_ms(p2s_ctx *ctx, float *elapsed_ms) { return p2s_kernel_ms_query(ctx, P2S_TIMED_CONFIDENCE, "p2s_confidence_stats_host", elapsed_ms); }

}  // extern "C"
