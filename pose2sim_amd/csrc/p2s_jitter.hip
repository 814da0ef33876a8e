// p2s_jitter.hip -- 2D keypoint jitter analysis (Utilities/keypoint_jitter_analyze.py:143-325) and the exact column order
// statistic it needs.  float64 end to end: every number must be the reference's bit for bit.
//
//   jitter_frames_kernel   per frame: frame-to-frame displacement of every keypoint (compute_displacements :143-166), the
//                          bounding box of the valid keypoints, its area (compute_bb_areas :198-223) and whether it comes
//                          within 10 px of the image border (classify_pattern :252-260)
//   order_stats_kernel     per column: the values at given ranks among the non-NaN entries (np.nanmedian :188, :294)
//   jitter_thresholds_kernel  medians -> thresholds (detect_jitter :188-191)
//   jitter_events_kernel<0>   event mask, counts per (camera, keypoint), events per tile of 256 rows
//   scan_tiles_kernel         exclusive scan of the tile counts
//   jitter_events_kernel<1>   the event list (camera, frame, keypoint, pattern) in np.argwhere order, cameras in order
//
// Bit equality.  dx*dx + dy*dy must be rn(rn(dx*dx) + rn(dy*dy)) as NumPy computes it: floating-point contraction is off
// for this whole file (an FMA would change the last bit), and the square root is the correctly rounded __dsqrt_rn.
// Everything else is comparisons, exact order statistics, one subtraction pair and product (the area), one sum and
// halving (the median) and one product (the threshold), none of which the compiler may fuse with contraction off.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>
#include <vector>

#include "p2s_ctx.h"

#pragma clang fp contract(off)

// 2D keypoint jitter analysis (Utilities/keypoint_jitter_analyze.py:143-325).  Cameras back to back:
// camera c holds frames frame_off[c] .. frame_off[c + 1] and one displacement row fewer than frames, so its first row
// among all rows is frame_off[c] - c.
#define P2S_JITTER_KPTS 26
struct P2sJitterArgs {
    const double *series;        // [frames][26][3] (x, y, confidence)
    const int64_t *frame_off;    // [C + 1]
    const int64_t *tile_base;    // [C + 1] first 256-row tile of every camera
    double *disp;                // per camera [26][rows]: column-major, for the order statistics
    double *area;                // [frames] box area, NaN with fewer than 2 valid keypoints
    uint8_t *edge;               // [frames] 1: the box comes within 10 px of the image border
    const double *stats;         // [C][27][2] the two middle values of the 26 displacement columns and the area column
    const int64_t *stat_counts;  // [C][27] their non-NaN counts
    double *medians, *thresholds;   // [C][26]
    double *med_area;            // [C]
    uint8_t *mask;               // [rows][26]
    int32_t *counts;             // [C][26] events per keypoint (zeroed by the caller)
    uint32_t *tile_count;        // [n_tiles]
    long long *tile_off;         // [n_tiles] exclusive scan of tile_count
    long long *n_events;
    int32_t *events;             // [event_capacity][4] camera, frame, keypoint, pattern (0 A, 1 C, 2 D, 3 E)
    int64_t event_capacity;
    int64_t n_tiles, max_frames;
    double multiplier, x_edge, y_edge;   // width - 10, height - 10
    int32_t C;
};

namespace {

constexpr int JK = P2S_JITTER_KPTS;      // 26 keypoints, (x, y, confidence) each: 624 contiguous bytes per frame
constexpr int FT = 64;                   // frames per workgroup of the per-frame pass
constexpr int RUN = 8;                   // consecutive frames per 32-lane group (8 groups x 8 frames = FT)
constexpr int ET = 256;                  // displacement rows per workgroup of the event kernels
constexpr double CONF_THRESHOLD = 0.1;   // keypoint_jitter_analyze.py:42
constexpr double EDGE_MARGIN = 10.0;     // :45
constexpr double LOW_CONF = 0.3;         // :268

__device__ __forceinline__ double jt_nan() { return __longlong_as_double(0x7ff8000000000000LL); }
__device__ __forceinline__ double jt_inf() { return __longlong_as_double(0x7ff0000000000000LL); }

// ---- per-frame pass -------------------------------------------------------------------------------------------------
// A frame belongs to a group of 32 lanes (lane k < 26 holds keypoint k: the group's loads cover the frame's 624 bytes
// back to back), and a group walks RUN consecutive frames carrying the previous frame in registers, so a frame is read
// once (plus one frame per run).  The box is reduced across the group with shuffles and ballots.  The displacements of
// the workgroup's 64 frames are transposed through LDS so that every keypoint's column gets one contiguous run.
__global__ void __launch_bounds__(256) jitter_frames_kernel(const P2sJitterArgs a) {
    __shared__ double tile[JK][FT + 1];
    const int c = blockIdx.y;
    const int64_t f_base = a.frame_off[c];
    const int64_t F = a.frame_off[c + 1] - f_base;
    const int64_t t0 = (int64_t)blockIdx.x * FT;
    if (t0 >= F) return;                                         // uniform over the workgroup
    const int g = threadIdx.x >> 5, k = threadIdx.x & 31;
    const int half_shift = (g & 1) * 32;                         // the group's half of the wave's ballot
    const bool lane_on = k < JK;
    const double *src = a.series + f_base * (JK * 3) + k * 3;
    const int64_t f0 = t0 + (int64_t)g * RUN;
    double px = jt_nan(), py = jt_nan();
    bool pvalid = false;
    if (lane_on && f0 >= 1 && f0 - 1 < F) {
        const double *p = src + (f0 - 1) * (JK * 3);
        px = p[0]; py = p[1];
        pvalid = p[2] > CONF_THRESHOLD;                          // a NaN confidence fails the test
    }
    for (int j = 0; j < RUN; ++j) {
        const int64_t f = f0 + j;
        const bool in = lane_on && f < F;
        double x = jt_nan(), y = jt_nan(), cf = jt_nan();
        if (in) {
            const double *p = src + f * (JK * 3);
            x = p[0]; y = p[1]; cf = p[2];
        }
        const bool valid = in && cf > CONF_THRESHOLD;
        // every lane of the wave takes part in the ballots and shuffles: nothing below is under a divergent branch
        const int n_valid = __popc((unsigned)(__ballot(valid) >> half_shift));
        const bool nan_x = (unsigned)(__ballot(valid && x != x) >> half_shift) != 0u;
        const bool nan_y = (unsigned)(__ballot(valid && y != y) >> half_shift) != 0u;
        double x_lo = valid ? x : jt_inf(), x_hi = valid ? x : -jt_inf();
        double y_lo = valid ? y : jt_inf(), y_hi = valid ? y : -jt_inf();
#pragma unroll
        for (int m = 16; m >= 1; m >>= 1) {
            x_lo = fmin(x_lo, __shfl_xor(x_lo, m, 32));
            x_hi = fmax(x_hi, __shfl_xor(x_hi, m, 32));
            y_lo = fmin(y_lo, __shfl_xor(y_lo, m, 32));
            y_hi = fmax(y_hi, __shfl_xor(y_hi, m, 32));
        }
        if (nan_x) x_lo = x_hi = jt_nan();                       // ndarray.min / max propagate NaN
        if (nan_y) y_lo = y_hi = jt_nan();
        if (k == 0 && f < F) {
            const bool box = n_valid >= 2;
            a.area[f_base + f] = box ? (x_hi - x_lo) * (y_hi - y_lo) : jt_nan();
            a.edge[f_base + f] = box && (x_lo < EDGE_MARGIN || y_lo < EDGE_MARGIN || x_hi > a.x_edge || y_hi > a.y_edge);
        }
        double d = jt_nan();
        if (valid && pvalid) {
            const double dx = x - px, dy = y - py;
            d = __dsqrt_rn(dx * dx + dy * dy);
        }
        if (lane_on) tile[k][g * RUN + j] = d;                    // frame t0 + g*RUN + j = displacement row (that frame - 1)
        px = x; py = y; pvalid = valid;
    }
    __syncthreads();
    const int64_t R = F - 1;
    double *dst = a.disp + JK * (f_base - c);                    // camera c's columns: [JK][R]
    for (int i = threadIdx.x; i < JK * FT; i += 256) {
        const int kk = i / FT, j = i % FT;
        const int64_t r = t0 + j - 1;
        if (r >= 0 && r < R) dst[kk * R + r] = tile[kk][j];
    }
}

// ---- exact order statistics of a column -------------------------------------------------------------------------------
// One workgroup per column.  A double maps to a 64-bit key whose unsigned order is the order of the values (-0.0 before
// +0.0); NaN entries are skipped.  Most-significant-digit radix select, 8 bits a pass: a histogram of the current digit
// over the entries whose higher digits equal the prefix found so far, then the bin holding the rank.  The histogram of
// the first digit does not depend on the rank and is kept; its total is the non-NaN count.  Ranks that fall on the value
// just found reuse it, and the rank right after it takes one pass (the smallest larger key), so a median costs 8 or 9
// passes over a column that stays in L2.
//
// Histogram: one private copy per wave in LDS.  Displacements span a few binades, so the first digits of a whole wave
// fall on two or three bins, and 64 atomic adds to one LDS word serialise.  Two rounds of aggregation come first: the
// first pending lane's digit is broadcast, the lanes that hold it are counted with a ballot, one lane adds the count.
// What is left -- nothing for a constant column, most lanes for well-spread digits -- goes through ds_add_u32.
constexpr int OS_THREADS = 1024, OS_WAVES = OS_THREADS / 64;

__device__ __forceinline__ uint64_t os_key(double v) {
    const uint64_t b = (uint64_t)__double_as_longlong(v);
    return b ^ ((b >> 63) ? ~0ULL : 0x8000000000000000ULL);
}
__device__ __forceinline__ double os_value(uint64_t key) {
    return __longlong_as_double((long long)((key >> 63) ? key ^ 0x8000000000000000ULL : ~key));
}

__device__ __forceinline__ void os_hist_add(uint32_t *h, bool on, uint32_t digit, int lane) {
    unsigned long long todo = __ballot(on);
    for (int round = 0; round < 2 && todo != 0ULL; ++round) {    // todo is wave-uniform
        const int leader = __ffsll((long long)todo) - 1;
        const uint32_t d0 = (uint32_t)__shfl((int)digit, leader);
        const unsigned long long same = __ballot(on && digit == d0);
        if (lane == leader) atomicAdd(&h[d0], (uint32_t)__popcll(same));
        if (digit == d0) on = false;
        todo &= ~same;
    }
    if (on) atomicAdd(&h[digit], 1u);
}

struct OsShared {
    uint32_t hist[OS_WAVES][256];
    uint32_t first[256];                 // the first digit's histogram, kept for every rank
    uint32_t bins[256];
    unsigned long long wave_min[OS_WAVES];
    uint32_t wave_cnt[OS_WAVES];
    uint32_t digit, before, in_bin;      // what os_pick found
};

// bins <- the histogram of digit (key >> shift) & 255 over the non-NaN entries with (key >> (shift + 8)) == prefix
// (every non-NaN entry when shift == 56).  Called by the whole workgroup.
__device__ void os_histogram(OsShared &s, const double *x, int64_t n, int shift, uint64_t prefix) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    for (int i = tid; i < OS_WAVES * 256; i += OS_THREADS) (&s.hist[0][0])[i] = 0u;
    __syncthreads();
    for (int64_t base = 0; base < n; base += OS_THREADS) {       // uniform trip count: the ballots need every lane
        const int64_t i = base + tid;
        bool on = i < n;
        uint32_t digit = 0;
        if (on) {
            const double v = x[i];
            const uint64_t key = os_key(v);
            on = v == v && ((key >> shift) >> 8) == prefix;      // shift == 56: 0 == 0
            digit = (uint32_t)(key >> shift) & 255u;
        }
        os_hist_add(s.hist[wave], on, digit, lane);
    }
    __syncthreads();
    if (tid < 256) {
        uint32_t t = 0;
        for (int w = 0; w < OS_WAVES; ++w) t += s.hist[w][tid];
        s.bins[tid] = t;
    }
    __syncthreads();
}

// The bin of `bins` that holds 0-based position `rank` (rank < sum of bins): digit, entries before it, entries in it.
// Wave 0 scans (4 bins a lane); the whole workgroup calls and reads the result after the barrier.
__device__ void os_pick(OsShared &s, const uint32_t *bins, uint32_t rank) {
    if (threadIdx.x < 64) {
        const int lane = threadIdx.x;
        uint32_t b[4], sum = 0;
        for (int i = 0; i < 4; ++i) { b[i] = bins[4 * lane + i]; sum += b[i]; }
        uint32_t incl = sum;
        for (int m = 1; m < 64; m <<= 1) {
            const uint32_t up = (uint32_t)__shfl_up((int)incl, m);
            if (lane >= m) incl += up;
        }
        uint32_t before = incl - sum;
        if (rank >= before && rank < incl) {                     // exactly one lane
            int i = 0;
            while (rank >= before + b[i]) { before += b[i]; ++i; }
            s.digit = 4 * lane + i; s.before = before; s.in_bin = b[i];
        }
    }
    __syncthreads();
}

__global__ void __launch_bounds__(OS_THREADS) order_stats_kernel(const P2sOrderArgs a) {
    __shared__ OsShared s;
    const int col = blockIdx.x, tid = threadIdx.x;
    const double *x = a.data + (a.col_off ? a.col_off[col] : (int64_t)col * a.n_rows);
    const int64_t n = a.col_len ? a.col_len[col] : a.n_rows;
    const int n_ranks = (a.ranks || a.fractions) ? a.n_ranks : 2;
    double *out = a.out + (int64_t)col * n_ranks;

    os_histogram(s, x, n, 56, 0);
    if (tid < 256) s.first[tid] = s.bins[tid];
    __syncthreads();
    uint32_t m = 0;                                               // non-NaN count; the same in every thread
    for (int i = 0; i < 256; ++i) m += s.first[i];
    if (tid == 0 && a.counts) a.counts[col] = (int64_t)m;

    bool have = false;                                            // the last value found: its key, how many entries are
    uint64_t key = 0;                                             // smaller (less) and how many equal it (equal)
    uint32_t less = 0, equal = 0;
    for (int j = 0; j < n_ranks; ++j) {
        int64_t r;
        if (a.fractions) {                                        // np.percentile's lo, hi around (m - 1) * fraction
            const int64_t lo = (int64_t)floor((double)((int64_t)m - 1) * a.fractions[j >> 1]);
            r = (j & 1) ? (lo + 1 < (int64_t)m ? lo + 1 : (int64_t)m - 1) : lo;
        } else if (a.ranks) { r = a.ranks[j]; if (r < 0) r += m; }   // negative: counted from the top
        else r = j == 0 ? ((int64_t)m - 1) / 2 : (int64_t)m / 2;  // the two middle positions (equal when m is odd)
        if (m == 0 || r < 0 || r >= (int64_t)m) {
            if (tid == 0) out[j] = jt_nan();
            continue;
        }
        if (have && r >= less && r < (int64_t)less + equal) {
            // the same value again
        } else if (have && r == (int64_t)less + equal) {
            // the next larger value: the smallest key above the last one
            // and how many entries hold it
            unsigned long long best = ~0ULL;
            uint32_t n_best = 0;
            for (int64_t i = tid; i < n; i += OS_THREADS) {
                const double v = x[i];
                const uint64_t kk = os_key(v);
                if (v == v && kk > key) {
                    if (kk < best) { best = kk; n_best = 1; }
                    else if (kk == best) ++n_best;
                }
            }
            for (int mm = 32; mm >= 1; mm >>= 1) {
                const unsigned long long o = __shfl_xor(best, mm);
                const uint32_t on = (uint32_t)__shfl_xor((int)n_best, mm);
                if (o < best) { best = o; n_best = on; }
                else if (o == best) n_best += on;
            }
            __syncthreads();                                      // wave_min of an earlier rank has been read
            if ((tid & 63) == 0) { s.wave_min[tid >> 6] = best; s.wave_cnt[tid >> 6] = n_best; }
            __syncthreads();
            best = s.wave_min[0]; n_best = s.wave_cnt[0];
            for (int w = 1; w < OS_WAVES; ++w) {
                if (s.wave_min[w] < best) { best = s.wave_min[w]; n_best = s.wave_cnt[w]; }
                else if (s.wave_min[w] == best) n_best += s.wave_cnt[w];
            }
            key = best; less += equal; equal = n_best;            // r < m, so a larger entry exists
        } else {
            __syncthreads();                                      // s.digit .. of an earlier rank have been read
            os_pick(s, s.first, (uint32_t)r);
            uint64_t prefix = s.digit;
            uint32_t rr = (uint32_t)r - s.before, before_all = s.before, in_bin = s.in_bin;
            for (int shift = 48; shift >= 0; shift -= 8) {
                os_histogram(s, x, n, shift, prefix);
                os_pick(s, s.bins, rr);
                prefix = (prefix << 8) | s.digit;
                rr -= s.before; before_all += s.before; in_bin = s.in_bin;
                __syncthreads();                                  // everyone has read the pick before the next one
            }
            key = prefix; less = before_all; equal = in_bin; have = true;
        }
        if (tid == 0) out[j] = os_value(key);
    }
}

// ---- thresholds, events -------------------------------------------------------------------------------------------
// stats [C][JK + 1][2]: the two middle values of the 26 displacement columns and of the area column.  NumPy's median of
// an even count is the mean of the two, add.reduce then / 2; with an odd count both ranks name the same entry, which
// is the median.
__global__ void jitter_thresholds_kernel(const P2sJitterArgs a) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= a.C * (JK + 1)) return;
    const int c = i / (JK + 1), k = i % (JK + 1);
    const int64_t m = a.stat_counts[i];
    // np.mean adds the entries to +0.0 (so a median of -0.0 entries is +0.0); contraction is off, the sum is kept
    const double lo = 0.0 + a.stats[2 * i];
    const double med = m == 0 ? jt_nan() : (m & 1) ? lo : (lo + a.stats[2 * i + 1]) / 2.0;
    if (k == JK) {
        a.med_area[c] = med;
    } else {
        a.medians[c * JK + k] = med;
        a.thresholds[c * JK + k] = med == 0.0 ? 10.0 : med * a.multiplier;   // detect_jitter :190-191
    }
}

// classify_pattern :226-271 at displacement row r (frame r + 1): 0 = A, 1 = C, 2 = D, 3 = E
__device__ __forceinline__ int jitter_pattern(const P2sJitterArgs &a, int c, int64_t f_abs, int k) {
    if (a.edge[f_abs]) return 0;
    const double area = a.area[f_abs], med = a.med_area[c];
    if (area == area && med == med && area < med * 0.5) return 1;
    if (a.series[(f_abs * JK + k) * 3 + 2] < LOW_CONF) return 2;
    return 3;
}

// A tile is 256 consecutive displacement rows of one camera, one row per lane: for every keypoint the lanes read 256
// consecutive doubles of its column.  SCATTER = false: the mask bytes [row][JK], the counts per (camera, keypoint) and
// the tile's event count.  SCATTER = true: with the exclusive scan of the tile counts, every event goes to its place in
// np.argwhere order (row-major over (row, keypoint)) behind the events of the earlier cameras -- no atomic cursor.
template <bool SCATTER>
__global__ void __launch_bounds__(ET) jitter_events_kernel(const P2sJitterArgs a) {
    __shared__ double thr[JK];
    __shared__ uint32_t kcount[JK];
    __shared__ uint32_t wave_total[ET / 64];
    __shared__ uint8_t bytes[ET * JK];
    const int c = blockIdx.y, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int64_t f_base = a.frame_off[c];
    const int64_t R = a.frame_off[c + 1] - f_base - 1;
    const int64_t r0 = (int64_t)blockIdx.x * ET;
    if (r0 >= R) return;                                          // uniform over the workgroup
    if (tid < JK) { thr[tid] = a.thresholds[c * JK + tid]; kcount[tid] = 0u; }
    __syncthreads();
    const int64_t row_base = f_base - c;                          // camera c's first row among all rows
    const double *col = a.disp + JK * row_base;
    const int64_t r = r0 + tid;
    const bool in = r < R;
    uint32_t bits = 0;
    for (int k = 0; k < JK; ++k) {
        const bool ev = in && col[k * R + r] > thr[k];            // NaN on either side: no event
        bits |= (uint32_t)ev << k;
        if (!SCATTER) {
            bytes[tid * JK + k] = ev;
            const unsigned long long b = __ballot(ev);
            if (lane == 0 && b) atomicAdd(&kcount[k], (uint32_t)__popcll(b));
        }
    }
    // exclusive scan of the rows' event counts over the workgroup
    const uint32_t mine = __popc(bits);
    uint32_t incl = mine;
    for (int m = 1; m < 64; m <<= 1) {
        const uint32_t up = (uint32_t)__shfl_up((int)incl, m);
        if (lane >= m) incl += up;
    }
    if (lane == 63) wave_total[wave] = incl;
    __syncthreads();
    uint32_t before = incl - mine, total = 0;
    for (int w = 0; w < ET / 64; ++w) {
        if (w < wave) before += wave_total[w];
        total += wave_total[w];
    }
    const int64_t tile = a.tile_base[c] + blockIdx.x;
    if (!SCATTER) {
        if (tid == 0) a.tile_count[tile] = total;
        if (tid < JK && kcount[tid]) atomicAdd(&a.counts[c * JK + tid], (int32_t)kcount[tid]);   // integer: order-free
        const int64_t n_bytes = (R - r0 < ET ? R - r0 : ET) * JK;
        uint8_t *dst = a.mask + (row_base + r0) * JK;
        for (int64_t i = tid; i < n_bytes; i += ET) dst[i] = bytes[i];
    } else {
        int64_t at = (int64_t)a.tile_off[tile] + before;
        while (bits) {
            const int k = __ffs((int)bits) - 1;
            bits &= bits - 1;
            if (at < a.event_capacity)
                reinterpret_cast<int4 *>(a.events)[at] = make_int4(c, (int)(r + 1), k, jitter_pattern(a, c, f_base + r + 1, k));
            ++at;
        }
    }
}

// tile_off <- exclusive scan of tile_count; n_events <- the total.  One workgroup walks the tiles 1024 at a time.
__global__ void __launch_bounds__(1024) scan_tiles_kernel(const P2sJitterArgs a) {
    __shared__ uint32_t wave_total[16];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    unsigned long long carry = 0;
    for (int64_t base = 0; base < a.n_tiles; base += 1024) {
        const int64_t i = base + tid;
        const uint32_t mine = i < a.n_tiles ? a.tile_count[i] : 0u;
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
        if (i < a.n_tiles) a.tile_off[i] = (long long)before;
        carry += total;
    }
    if (tid == 0) *a.n_events = (long long)carry;
}

}  // namespace

hipError_t p2s_launch_order_stats(const P2sOrderArgs &a, hipStream_t s) {   // also p2s_confidence.hip
    if (a.n_cols == 0) return hipSuccess;
    hipLaunchKernelGGL(order_stats_kernel, dim3((unsigned)a.n_cols), dim3(OS_THREADS), 0, s, a);
    return hipGetLastError();
}

static hipError_t p2s_launch_jitter(const P2sJitterArgs &a, const P2sOrderArgs &o, hipStream_t s) {
    const unsigned frame_tiles = (unsigned)((a.max_frames + FT - 1) / FT);
    hipLaunchKernelGGL(jitter_frames_kernel, dim3(frame_tiles, (unsigned)a.C), dim3(256), 0, s, a);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    if ((e = p2s_launch_order_stats(o, s)) != hipSuccess) return e;
    hipLaunchKernelGGL(jitter_thresholds_kernel, dim3((unsigned)((a.C * (JK + 1) + 63) / 64)), dim3(64), 0, s, a);
    if (a.max_frames > 1) {
        const unsigned row_tiles = (unsigned)((a.max_frames - 1 + ET - 1) / ET);
        hipLaunchKernelGGL((jitter_events_kernel<false>), dim3(row_tiles, (unsigned)a.C), dim3(ET), 0, s, a);
        hipLaunchKernelGGL(scan_tiles_kernel, dim3(1), dim3(1024), 0, s, a);
        hipLaunchKernelGGL((jitter_events_kernel<true>), dim3(row_tiles, (unsigned)a.C), dim3(ET), 0, s, a);
    } else {
        hipLaunchKernelGGL(scan_tiles_kernel, dim3(1), dim3(1024), 0, s, a);   // no rows: zero events
    }
    return hipGetLastError();
}

// ---- C-ABI entry points (include/p2s.h) ----------------------------------------------------------------------------
extern "C" {

int p2s_column_order_stats_host(p2s_ctx *ctx, int64_t n_rows, int32_t n_cols, const double *data, int32_t n_ranks,
                                const int64_t *ranks, double *out, int64_t *counts) {
    if (!ctx) return p2s_set_error(P2S_ERR_INVALID_ARG, "null context");
    if (n_rows < 0 || n_rows >= ((int64_t)1 << 31) || n_cols < 0 || n_ranks < 0)
        return p2s_set_error(P2S_ERR_INVALID_ARG, "bad shape: %lld rows, %d columns, %d ranks", (long long)n_rows, n_cols, n_ranks);
    if (n_cols == 0) return P2S_OK;
    if ((n_rows > 0 && !data) || (n_ranks > 0 && (!ranks || !out))) return p2s_set_error(P2S_ERR_INVALID_ARG, "null argument");
    const size_t data_b = (size_t)n_rows * n_cols * sizeof(double);
    const size_t rank_b = (size_t)n_ranks * sizeof(int64_t), out_b = (size_t)n_cols * n_ranks * sizeof(double);
    const size_t cnt_b = (size_t)n_cols * sizeof(int64_t);
    HIP_TRY(hipSetDevice(ctx->device));
    P2sOrderArgs a{};
    a.n_rows = n_rows; a.n_cols = n_cols; a.n_ranks = n_ranks;
    Stage st{ctx};
    P2S_TRY(st.upload(a.data, data, data_b));
    P2S_TRY(st.upload(a.ranks, ranks, rank_b));
    P2S_TRY(st.alloc(a.counts, cnt_b + out_b));                   // one block, the 8-byte counts first: both parts stay aligned
    a.out = (double *)(a.counts + n_cols);
    HIP_TRY(p2s_launch_order_stats(a, ctx->stream));
    P2S_TRY(st.down(out, a.out, out_b));
    P2S_TRY(st.down(counts, a.counts, cnt_b));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    return P2S_OK;
}

int p2s_jitter_host(p2s_ctx *ctx, int32_t n_cams, const int64_t *n_frames, const double *series, double multiplier,
                    double image_width, double image_height, double *displacements, double *areas, double *medians,
                    double *thresholds, double *median_area, uint8_t *mask, int32_t *counts, int64_t event_capacity,
                    int32_t *events, int64_t *n_events) {
    if (!ctx) return p2s_set_error(P2S_ERR_INVALID_ARG, "null context");
    P2S_TRY(p2s_check_n_cams(n_cams));
    if (!n_frames || !series) return p2s_set_error(P2S_ERR_INVALID_ARG, "null argument");
    if (event_capacity < 0 || (event_capacity > 0 && !events)) return p2s_set_error(P2S_ERR_INVALID_ARG, "event_capacity=%lld without room", (long long)event_capacity);
    constexpr int K = P2S_JITTER_KPTS, NS = K + 1;
    const size_t C = (size_t)n_cams;
    Layout lay;                                                   // `tab` goes up as one: the host's tables
    const size_t o_foff = lay.add((C + 1) * 8), o_tbase = lay.add((C + 1) * 8), o_coff = lay.add(C * NS * 8), o_clen = lay.add(C * NS * 8), tab_b = lay.bytes;
    std::vector<char> tab(tab_b);
    int64_t *frame_off = (int64_t *)(tab.data() + o_foff), *tile_base = (int64_t *)(tab.data() + o_tbase);
    int64_t *col_off = (int64_t *)(tab.data() + o_coff), *col_len = (int64_t *)(tab.data() + o_clen);
    P2sFrames fr;
    P2S_TRY(fr.build(n_cams, n_frames, 1, (int64_t)1 << 33, frame_off));
    const int64_t frames = fr.frames, max_frames = fr.max_frames, rows = frames - n_cams;
    tile_base[0] = 0;
    for (size_t c = 0; c < C; ++c) {                              // displacement columns, then the areas, in one allocation
        const int64_t R = n_frames[c] - 1;
        tile_base[c + 1] = tile_base[c] + (R + 255) / 256;
        for (int k = 0; k < K; ++k) { col_off[c * NS + k] = K * (frame_off[c] - (int64_t)c) + k * R; col_len[c * NS + k] = R; }
        col_off[c * NS + K] = K * rows + frame_off[c];
        col_len[c * NS + K] = n_frames[c];
    }
    const int64_t n_tiles = tile_base[C];
    const size_t series_b = (size_t)frames * K * 3 * sizeof(double), disp_b = (size_t)rows * K * sizeof(double);
    const size_t area_b = (size_t)frames * sizeof(double);
    // and what stays on the device: the columns' two middle values and non-NaN counts, what the kernels derive from them
    const size_t o_stats = lay.add(C * NS * 16), o_scnt = lay.add(C * NS * 8), o_med = lay.add(C * K * 8), o_thr = lay.add(C * K * 8),
                 o_marea = lay.add(C * 8), o_nev = lay.add(8), o_cnt = lay.add(C * K * 4);
    HIP_TRY(hipSetDevice(ctx->device));
    P2sJitterArgs a{};
    Stage st{ctx};
    char *sm;
    P2S_TRY(st.upload(a.series, series, series_b));
    P2S_TRY(st.alloc(a.disp, disp_b + area_b));
    P2S_TRY(st.alloc(sm, lay.bytes));
    P2S_TRY(st.alloc(a.tile_off, (size_t)n_tiles * 16 + 16));
    P2S_TRY(st.alloc(a.mask, (size_t)rows * K + 16));
    P2S_TRY(st.alloc(a.edge, (size_t)frames));
    P2S_TRY(st.alloc(a.events, (size_t)event_capacity * 16 + 16));
    P2S_TRY(st.up(sm, tab.data(), tab_b));
    a.frame_off = (const int64_t *)(sm + o_foff);
    a.tile_base = (const int64_t *)(sm + o_tbase);
    a.area = a.disp + (size_t)rows * K;
    a.stats = (const double *)(sm + o_stats);
    a.stat_counts = (const int64_t *)(sm + o_scnt);
    a.medians = (double *)(sm + o_med);
    a.thresholds = (double *)(sm + o_thr);
    a.med_area = (double *)(sm + o_marea);
    a.n_events = (long long *)(sm + o_nev);
    a.counts = (int32_t *)(sm + o_cnt);
    a.tile_count = (uint32_t *)((char *)a.tile_off + (size_t)n_tiles * 8 + 8);
    a.event_capacity = event_capacity;
    a.n_tiles = n_tiles; a.max_frames = max_frames;
    a.multiplier = multiplier; a.x_edge = image_width - 10.0; a.y_edge = image_height - 10.0;
    a.C = n_cams;
    P2sOrderArgs o{};
    o.data = a.disp;
    o.col_off = (const int64_t *)(sm + o_coff);
    o.col_len = (const int64_t *)(sm + o_clen);
    o.out = (double *)(sm + o_stats);
    o.counts = (int64_t *)(sm + o_scnt);
    o.n_cols = n_cams * NS; o.n_ranks = 2;                        // ranks NULL: the two middle positions
    HIP_TRY(hipMemsetAsync(a.counts, 0, C * K * 4, ctx->stream));
    P2S_TRY(st.time_begin());
    HIP_TRY(p2s_launch_jitter(a, o, ctx->stream));
    P2S_TRY(st.time_end());
    long long found = 0;
    P2S_TRY(st.down(&found, a.n_events, 8));
    P2S_TRY(st.down(displacements, a.disp, disp_b));
    P2S_TRY(st.down(areas, a.area, area_b));
    P2S_TRY(st.down(medians, a.medians, C * K * 8));
    P2S_TRY(st.down(thresholds, a.thresholds, C * K * 8));
    P2S_TRY(st.down(median_area, a.med_area, C * 8));
    P2S_TRY(st.down(mask, a.mask, (size_t)rows * K));
    P2S_TRY(st.down(counts, a.counts, C * K * 4));
    P2S_TRY(st.finish(P2S_TIMED_JITTER));                         // `tab` and `found` are host memory: alive until here
    const int64_t n_copy = std::min<int64_t>(found, event_capacity);
    if (n_copy > 0) {
        P2S_TRY(st.down(events, a.events, (size_t)n_copy * 16));
        HIP_TRY(hipStreamSynchronize(ctx->stream));
    }
    if (n_events) *n_events = found;
    return P2S_OK;
}

int p2s_jitter_kernel_ms(p2s_ctx *ctx, float *elapsed_ms) { return p2s_kernel_ms_query(ctx, P2S_TIMED_JITTER, "p2s_jitter_host", elapsed_ms); }

}  // extern "C"
