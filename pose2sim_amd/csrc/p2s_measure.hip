// p2s_measure.hip -- body measurements from .trc tables (common.py:378-455 and :715-1034, the .trc half of
// kinematics.py:278-304), and the primitive they need: a segmented stable sort of float64 keys.  A batch of files of
// unequal length is one call, and no count comes back to the host between the steps.
//
//   ms_speed_kernel      per frame: nansum over the markers of ||Q[i] - Q[i - 1]|| (row 0 is 0), the sort key (the speed,
//                        NaN where it is not above the file's close_to_zero_speed) and the count of frames above it
//   sort                 the frames of every file by speed
//   ms_select_kernel     n_sel = int(n_above * (1 - fastest_frames_to_remove_percent)), or every frame in file order when
//                        no speed is above the bound
//   ms_angle_kernel      mean_angles of the selected rows; the count of angles below the limit
//   sort                 the selected rows of every file by angle
//   ms_keep_kernel       the rows with angle < limit in their order when there are 50 or more, else the first 50 rows by
//                        angle (Series.nsmallest: NaN angles last, in their order, and kept when fewer than 50 rows have
//                        an angle); every frame of the file when no row is left
//   ms_length_kernel     nansum(d * d) per kept row and marker pair, and whether a pair has any non-NaN difference
//   ms_height_kernel     sqrt (inf for a pair whose differences are all NaN), row heights and row leg lengths
//   sort                 every (file, column) over the kept rows
//   ms_trim_kernel       np.mean(np.sort(x)[int(n * p / 2) : int(n * (1 - p / 2))]), np.mean(x) when the slice is empty
//
// The sort.  A key is the double's bits made monotone (sign flipped, negative values inverted), -0.0 first turned into
// +0.0 and every NaN into the largest word: NumPy's order -inf < ... < -0.0 = +0.0 < ... < inf < NaN.  Records are compared
// as (key, index in the segment): the indices are distinct, so the order is total and the result is the stable order
// whatever the algorithm.  ms_tile_sort_kernel sorts tiles of ST = 1024 records in LDS (a bitonic network over the next
// power of two of the tile's fill, the padding above every record); ms_merge_kernel doubles the sorted runs, one record
// per lane and step: its place is its offset in its own run plus the number of records of the sibling run below it, a
// binary search.  A run is a whole number of tiles, so a tile has one sibling.  Segment lengths are read from device
// memory; the grid and the number of merge rounds come from the capacities, which the host knows.
//
// Numbers.  Speeds, lengths, heights and trimmed means are sums, products and correctly rounded roots in NumPy's order
// (contraction off): bit for bit.  The angles go through atan2 and compare to a tolerance.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>

#include <algorithm>
#include <vector>

#include "p2s_ctx.h"
#include "p2s_npsum.h"                       // CT, cf_sum: np.add.reduce

#pragma clang fp contract(off)

#define P2S_MEASURE_ROLES 10                 // RShoulder LShoulder RHip LHip Hip Neck RKnee LKnee RAnkle LAnkle
#define P2S_MEASURE_HEIGHT_PAIRS 9
#define P2S_MEASURE_MAX_PAIRS 1024

struct MsSort {
    const double *src;           // the keys: column c's segment f at c * col_stride + row_off[f]
    const int64_t *row_off;      // [n_seg]
    const int32_t *seg_len;      // [n_seg] on the device; at most the capacity the tiles were laid out for
    const int32_t *tile_seg;     // [n_tiles] the segment of every tile
    const int32_t *tile_idx;     // [n_tiles] and its number inside the segment
    int64_t col_stride;
    uint64_t *key[2];            // ping-pong records
    uint32_t *idx[2];
    int32_t *order;              // out: the stable order of every segment
    double *sorted;              // out: src in that order, or NULL
};

struct MsArgs {
    const double *data;          // the tables back to back, [n_rows][3 n_markers] each
    const int64_t *tab_off;      // [n_files] first element of every table
    const int64_t *row_off;      // [n_files] first row of every file among all rows
    const double *head_factor;   // [n_files]
    const double *speed_thr;     // [n_files]
    const int32_t *n_rows, *n_mk, *flags;
    const int32_t *n_speed;      // [n_files] the speeds sum over the first n_speed markers
    const int32_t *roles;        // [n_files][10]
    const int32_t *pairs;        // [n_files][n_pairs][2]
    const int32_t *tile_seg, *tile_idx;
    double keep_fraction, angle_limit, half_trim;
    int64_t N;                   // rows of all files
    int32_t n_files, n_pairs, n_cols;   // n_cols = n_pairs + 2: the pairs, the heights, the leg lengths
    double *speed, *key1, *ang;  // [N]
    double *vals, *sorted;       // [n_cols][N]
    double *means;               // [n_files][n_cols]
    int32_t *order1, *order2, *kept_pos, *kept_frame;   // [N]
    int32_t *n_pos, *n_sel, *n_lt, *n_kept, *branch;   // [n_files]
    int32_t *has_value;          // [n_files][n_pairs]
};

struct MsTrim {
    const double *vals, *sorted; // column c's segment f at c * col_stride + row_off[f]
    const int64_t *row_off;
    const int32_t *seg_len;
    double *means;               // [n_seg][n_cols]
    int64_t col_stride;
    double half_trim;
};

namespace {

constexpr int ST = 1024;                 // records per sort tile
constexpr int SB = 256;                  // lanes per workgroup of the tile kernels: ST / SB records per lane
constexpr int MS_IDENTITY = 0x100;       // branch word, device side only: the selected rows are the frames in file order

__device__ __forceinline__ double ms_nan() { return __longlong_as_double(0x7ff8000000000000LL); }
__device__ __forceinline__ double ms_inf() { return __longlong_as_double(0x7ff0000000000000LL); }

__device__ __forceinline__ uint64_t ms_key(double v) {
    if (v != v) return ~0ull;
    uint64_t b = (uint64_t)__double_as_longlong(v);
    if (b == 0x8000000000000000ull) b = 0;
    return (b >> 63) ? ~b : (b | 0x8000000000000000ull);
}

__device__ __forceinline__ bool ms_less(uint64_t ka, uint32_t ia, uint64_t kb, uint32_t ib) { return ka < kb || (ka == kb && ia < ib); }

// the tile of this workgroup: its segment, first record, the segment's length and first element
struct MsTile {
    int seg;
    int64_t t0, n, base;
};
__device__ __forceinline__ MsTile ms_tile(const int32_t *tile_seg, const int32_t *tile_idx, const int64_t *row_off, const int32_t *seg_len) {
    MsTile t;
    t.seg = tile_seg[blockIdx.x];
    t.t0 = (int64_t)tile_idx[blockIdx.x] * ST;
    t.n = seg_len[t.seg];
    t.base = row_off[t.seg];
    return t;
}

// ---- the sort -----------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(SB) ms_tile_sort_kernel(const MsSort a) {
    __shared__ uint64_t sk[ST];
    __shared__ uint32_t si[ST];
    const MsTile t = ms_tile(a.tile_seg, a.tile_idx, a.row_off, a.seg_len);
    if (t.t0 >= t.n) return;                                      // the whole workgroup
    const int tid = threadIdx.x;
    const int cnt = (int)(t.n - t.t0 < ST ? t.n - t.t0 : ST);
    const int64_t at = (int64_t)blockIdx.y * a.col_stride + t.base + t.t0;
    int P = 2;
    while (P < cnt) P <<= 1;
    for (int e = tid; e < P; e += SB) {
        sk[e] = e < cnt ? ms_key(a.src[at + e]) : ~0ull;
        si[e] = e < cnt ? (uint32_t)(t.t0 + e) : 0xffffffffu;     // indices stay below 2^31: the padding is above every record
    }
    __syncthreads();
    for (int k = 2; k <= P; k <<= 1) {
        for (int j = k >> 1; j > 0; j >>= 1) {
            for (int q = tid; q < P / 2; q += SB) {
                const int lo = ((q & ~(j - 1)) << 1) | (q & (j - 1)), hi = lo | j;
                const uint64_t k0 = sk[lo], k1 = sk[hi];
                const uint32_t i0 = si[lo], i1 = si[hi];
                const bool up = (lo & k) == 0;
                if (ms_less(k1, i1, k0, i0) == up) { sk[lo] = k1; sk[hi] = k0; si[lo] = i1; si[hi] = i0; }
            }
            __syncthreads();
        }
    }
    for (int e = tid; e < cnt; e += SB) {
        a.key[0][at + e] = sk[e];
        a.idx[0][at + e] = si[e];
    }
}

__global__ void __launch_bounds__(SB) ms_merge_kernel(const MsSort a, int from, int64_t w) {
    const MsTile t = ms_tile(a.tile_seg, a.tile_idx, a.row_off, a.seg_len);
    if (t.t0 >= t.n) return;
    const int64_t col = (int64_t)blockIdx.y * a.col_stride + t.base;
    const uint64_t *K = a.key[from] + col;
    const uint32_t *I = a.idx[from] + col;
    uint64_t *Kd = a.key[from ^ 1] + col;
    uint32_t *Id = a.idx[from ^ 1] + col;
    for (int u = 0; u < ST / SB; ++u) {
        const int64_t e = t.t0 + threadIdx.x + u * SB;
        if (e >= t.n) break;
        const int64_t p0 = e / (2 * w) * (2 * w);
        const int64_t mid = p0 + w < t.n ? p0 + w : t.n, end = p0 + 2 * w < t.n ? p0 + 2 * w : t.n;
        const uint64_t k = K[e];
        const uint32_t i = I[e];
        const bool left = e < mid;
        int64_t lo = left ? mid : p0, hi = left ? end : mid;      // the sibling run; records are distinct
        while (lo < hi) {
            const int64_t m = lo + (hi - lo) / 2;
            if (ms_less(K[m], I[m], k, i)) lo = m + 1;
            else hi = m;
        }
        const int64_t pos = left ? e + (lo - mid) : lo + (e - mid);   // inside [p0, end)
        Kd[pos] = k;
        Id[pos] = i;
    }
}

__global__ void __launch_bounds__(SB) ms_order_kernel(const MsSort a, int from) {
    const MsTile t = ms_tile(a.tile_seg, a.tile_idx, a.row_off, a.seg_len);
    if (t.t0 >= t.n) return;
    const int64_t col = (int64_t)blockIdx.y * a.col_stride + t.base;
    for (int u = 0; u < ST / SB; ++u) {
        const int64_t e = t.t0 + threadIdx.x + u * SB;
        if (e >= t.n) break;
        const uint32_t i = a.idx[from][col + e];
        a.order[col + e] = (int32_t)i;
        if (a.sorted) a.sorted[col + e] = a.src[col + i];
    }
}

// ---- np.mean of the trimmed slice ------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(CT) ms_trim_kernel(const MsTrim a) {
    __shared__ CfShared s;
    const int seg = blockIdx.x;
    const int64_t n = a.seg_len[seg], col = (int64_t)blockIdx.y * a.col_stride + a.row_off[seg];
    const int64_t lo = (int64_t)((double)n * a.half_trim), hi = (int64_t)((double)n * (1.0 - a.half_trim));
    const bool whole = hi <= lo;                                  // an empty slice: the mean of the array as it came
    const double *x = whole ? a.vals + col : a.sorted + col + lo;
    const int64_t m = whole ? n : hi - lo;
    const double mean = cf_sum<false>(s, x, m, 0.0) / (double)m;
    if (threadIdx.x == 0) a.means[(int64_t)seg * gridDim.y + blockIdx.y] = m ? mean : ms_nan();
}

// ---- speeds, angles, the selection -------------------------------------------------------------------------------------
__device__ __forceinline__ void ms_count(int32_t *counter, bool on) {
    const unsigned long long b = __ballot(on);
    if ((threadIdx.x & 63) == 0 && b) atomicAdd(counter, (int32_t)__popcll(b));
}

__global__ void __launch_bounds__(SB) ms_speed_kernel(const MsArgs a) {
    const MsTile t = ms_tile(a.tile_seg, a.tile_idx, a.row_off, a.n_rows);
    const int f = t.seg, K = a.n_mk[f], n_speed = a.n_speed[f];
    const double *tab = a.data + a.tab_off[f];
    const double thr = a.speed_thr[f];
    for (int u = 0; u < ST / SB; ++u) {                           // t.t0 < t.n: the tiles were laid out for n_rows
        const int64_t i = t.t0 + threadIdx.x + u * SB;
        bool above = false;
        if (i < t.n) {
            double sum = 0.0;
            if (i > 0) {
                const double *p = tab + i * 3 * K, *q = p - 3 * K;
                for (int m = 0; m < n_speed; ++m) {
                    const double dx = p[3 * m] - q[3 * m], dy = p[3 * m + 1] - q[3 * m + 1], dz = p[3 * m + 2] - q[3 * m + 2];
                    const double norm = __dsqrt_rn((dx * dx + dy * dy) + dz * dz);
                    if (norm == norm) sum = sum + norm;
                }
            }
            above = sum > thr;
            a.speed[t.base + i] = sum;
            a.key1[t.base + i] = above ? sum : ms_nan();
        }
        ms_count(a.n_pos + f, above);
    }
}

__global__ void ms_select_kernel(const MsArgs a) {
    const int f = blockIdx.x * blockDim.x + threadIdx.x;
    if (f >= a.n_files) return;
    const int32_t n = a.n_rows[f], above = a.n_pos[f];
    if (!(a.flags[f] & P2S_MEASURE_SPEED)) {
        a.n_sel[f] = n;
        a.branch[f] = MS_IDENTITY;
    } else if (above == 0) {
        a.n_sel[f] = n;
        a.branch[f] = MS_IDENTITY | P2S_MEASURE_ALL_SLOW;
    } else {
        a.n_sel[f] = (int32_t)((double)above * a.keep_fraction);
        a.branch[f] = 0;
    }
}

// A marker's coordinates in a row; K is the mid-shoulder and K + 1 the mid-hip, (right + left) / 2.
__device__ __forceinline__ void ms_point(const double *row, int K, const int32_t *role, int m, double &x, double &y, double &z) {
    if (m < K) {
        x = row[3 * m]; y = row[3 * m + 1]; z = row[3 * m + 2];
    } else {
        const int r = role[m == K ? 0 : 2], l = role[m == K ? 1 : 3];
        x = (row[3 * r] + row[3 * l]) / 2.0; y = (row[3 * r + 1] + row[3 * l + 1]) / 2.0; z = (row[3 * r + 2] + row[3 * l + 2]) / 2.0;
    }
}

// points_to_angles on 3-D vectors u, v in degrees, then fixed_angles' offset, factor and wrap, then abs
__device__ __forceinline__ double ms_angle(double ux, double uy, double uz, double vx, double vy, double vz, double offset, double factor) {
    const double cx = uy * vz - uz * vy, cy = uz * vx - ux * vz, cz = ux * vy - uy * vx;
    const double dot = (ux * vx + uy * vy) + uz * vz;
    double ang = atan2(__dsqrt_rn((cx * cx + cy * cy) + cz * cz), dot) * (180.0 / 3.14159265358979323846);
    ang = (ang + offset) * factor;
    if (ang > 180.0) ang = ang - 360.0;
    if (ang < -180.0) ang = ang + 360.0;
    return fabs(ang);
}

__global__ void __launch_bounds__(SB) ms_angle_kernel(const MsArgs a) {
    const MsTile t = ms_tile(a.tile_seg, a.tile_idx, a.row_off, a.n_sel);
    const int f = t.seg;
    if (t.t0 >= t.n) return;
    if (!(a.flags[f] & P2S_MEASURE_ANGLES)) {                     // no angles asked for: NaN, which is also what the caller reads
        for (int u = 0; u < ST / SB; ++u) {
            const int64_t k = t.t0 + threadIdx.x + u * SB;
            if (k < t.n) a.ang[t.base + k] = ms_nan();
        }
        return;
    }
    const int K = a.n_mk[f], identity = a.branch[f] & MS_IDENTITY;
    const double *tab = a.data + a.tab_off[f];
    const int32_t *role = a.roles + (int64_t)f * P2S_MEASURE_ROLES;
    const int hip = role[4] >= 0 ? role[4] : K + 1, neck = role[5] >= 0 ? role[5] : K;
    for (int u = 0; u < ST / SB; ++u) {
        const int64_t k = t.t0 + threadIdx.x + u * SB;
        bool below = false;
        if (k < t.n) {
            const int64_t frame = identity ? k : a.order1[t.base + k];
            const double *row = tab + frame * 3 * K;
            double hx, hy, hz, nx, ny, nz, sum = 0.0;
            ms_point(row, K, role, hip, hx, hy, hz);
            ms_point(row, K, role, neck, nx, ny, nz);
            for (int side = 0; side < 2; ++side) {                // knees: ankle - knee against hip - knee, -180
                const double *an = row + 3 * role[8 + side], *kn = row + 3 * role[6 + side], *hp = row + 3 * role[2 + side];
                sum = sum + ms_angle(an[0] - kn[0], an[1] - kn[1], an[2] - kn[2], hp[0] - kn[0], hp[1] - kn[1], hp[2] - kn[2], -180.0, 1.0);
            }
            for (int side = 0; side < 2; ++side) {                // hips: hip - knee against neck - mid-hip, times -1
                const double *kn = row + 3 * role[6 + side], *hp = row + 3 * role[2 + side];
                sum = sum + ms_angle(hp[0] - kn[0], hp[1] - kn[1], hp[2] - kn[2], nx - hx, ny - hy, nz - hz, 0.0, -1.0);
            }
            const double mean = sum / 4.0;
            a.ang[t.base + k] = mean;
            below = mean < a.angle_limit;
        }
        ms_count(a.n_lt + f, below);
    }
}

// exclusive scan of `mine` over the SB lanes; the total in every lane.  wave_total: SB / 64 words of LDS.
__device__ __forceinline__ uint32_t ms_block_scan(uint32_t mine, uint32_t *wave_total, uint32_t &total) {
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
    for (int w = 0; w < SB / 64; ++w) {
        if (w < wave) before += wave_total[w];
        total += wave_total[w];
    }
    return before;
}

__global__ void __launch_bounds__(SB) ms_keep_kernel(const MsArgs a) {
    __shared__ uint32_t wave_total[SB / 64];
    const int f = blockIdx.x, tid = threadIdx.x;
    const int64_t base = a.row_off[f];
    const int32_t n = a.n_rows[f], n_sel = a.n_sel[f], fl = a.flags[f];
    int32_t branch = a.branch[f];
    const int identity = branch & MS_IDENTITY;
    int32_t *pos = a.kept_pos + base, *frame = a.kept_frame + base;
    const int32_t *order1 = a.order1 + base;
    int32_t kept;
    if (!(fl & P2S_MEASURE_RESTRICT)) {
        kept = n_sel;
        for (int32_t k = tid; k < n_sel; k += SB) { pos[k] = k; frame[k] = identity ? k : order1[k]; }
    } else if (a.n_lt[f] >= 50) {
        uint32_t done = 0;
        for (int32_t k0 = 0; k0 < n_sel; k0 += SB) {              // k0 + tid stays below 2^31 + 256: compared as int64
            const int64_t k = (int64_t)k0 + tid;
            const bool on = k < n_sel && a.ang[base + k] < a.angle_limit;
            uint32_t total;
            const uint32_t before = ms_block_scan(on ? 1u : 0u, wave_total, total);
            if (on) { pos[done + before] = (int32_t)k; frame[done + before] = identity ? (int32_t)k : order1[k]; }
            done += total;
            if (n_sel - k0 <= SB) break;
        }
        kept = (int32_t)done;
    } else {
        branch |= P2S_MEASURE_FEW_SMALL_ANGLES;
        kept = n_sel < 50 ? n_sel : 50;                           // NaN angles sort last and fill up: Series.nsmallest keeps them
        if (tid < kept) { const int32_t k = a.order2[base + tid]; pos[tid] = k; frame[tid] = identity ? k : order1[k]; }
    }
    if (kept == 0) {
        branch |= P2S_MEASURE_ALL_DATA;
        kept = n;
        for (int32_t i = tid; i < n; i += SB) { pos[i] = i; frame[i] = i; }
    }
    if (tid == 0) { a.n_kept[f] = kept; a.branch[f] = branch & ~MS_IDENTITY; }
}

// ---- lengths, heights ------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(SB) ms_length_kernel(const MsArgs a) {
    const MsTile t = ms_tile(a.tile_seg, a.tile_idx, a.row_off, a.n_kept);
    if (t.t0 >= t.n) return;
    const int f = t.seg, K = a.n_mk[f];
    const double *tab = a.data + a.tab_off[f];
    const int32_t *role = a.roles + (int64_t)f * P2S_MEASURE_ROLES, *pairs = a.pairs + (int64_t)f * a.n_pairs * 2;
    for (int u = 0; u < ST / SB; ++u) {
        const int64_t j = t.t0 + threadIdx.x + u * SB;
        if (j >= t.n) break;
        const double *row = tab + (int64_t)a.kept_frame[t.base + j] * 3 * K;
        for (int p = 0; p < a.n_pairs; ++p) {
            const int m0 = pairs[2 * p], m1 = pairs[2 * p + 1];
            double ss = 0.0;
            if (m0 >= 0 && m1 >= 0) {
                double x0, y0, z0, x1, y1, z1;
                ms_point(row, K, role, m0, x0, y0, z0);
                ms_point(row, K, role, m1, x1, y1, z1);
                const double dx = x1 - x0, dy = y1 - y0, dz = z1 - z0;
                const double sx = dx * dx, sy = dy * dy, sz = dz * dz;
                ss = ((sx == sx ? sx : 0.0) + (sy == sy ? sy : 0.0)) + (sz == sz ? sz : 0.0);
                if (dx == dx || dy == dy || dz == dz) a.has_value[(int64_t)f * a.n_pairs + p] = 1;
            }
            a.vals[(int64_t)p * a.N + t.base + j] = ss;
        }
    }
}

__global__ void __launch_bounds__(SB) ms_height_kernel(const MsArgs a) {
    const MsTile t = ms_tile(a.tile_seg, a.tile_idx, a.row_off, a.n_kept);
    if (t.t0 >= t.n) return;
    const int f = t.seg, fl = a.flags[f];
    const int32_t *pairs = a.pairs + (int64_t)f * a.n_pairs * 2, *has = a.has_value + (int64_t)f * a.n_pairs;
    for (int u = 0; u < ST / SB; ++u) {
        const int64_t j = t.t0 + threadIdx.x + u * SB;
        if (j >= t.n) break;
        double h[P2S_MEASURE_HEIGHT_PAIRS] = {};
        for (int p = 0; p < a.n_pairs; ++p) {
            double *v = a.vals + (int64_t)p * a.N + t.base + j;
            double len = 0.0;
            if (pairs[2 * p] >= 0 && pairs[2 * p + 1] >= 0) len = has[p] ? __dsqrt_rn(*v) : ms_inf();
            *v = len;
            if (p < P2S_MEASURE_HEIGHT_PAIRS) h[p] = len;
        }
        if (fl & P2S_MEASURE_FEET_CONST) h[0] = h[1] = 0.10;
        const double shanks = (h[2] + h[3]) / 2.0, thighs = (h[4] + h[5]) / 2.0;
        a.vals[(int64_t)a.n_pairs * a.N + t.base + j] = (fl & P2S_MEASURE_HEIGHT) ? ((((h[0] + h[1]) / 2.0 + shanks) + thighs) + (h[6] + h[7]) / 2.0) + h[8] * a.head_factor[f] : ms_nan();
        a.vals[(int64_t)(a.n_pairs + 1) * a.N + t.base + j] = (fl & P2S_MEASURE_LEG) ? shanks + thighs : ms_nan();
    }
}

}  // namespace

// tile_sort, the merge rounds the longest capacity needs, the order (and the sorted values)
static hipError_t p2s_launch_sort(const MsSort &s, int64_t n_tiles, int n_cols, int64_t max_len, hipStream_t st) {
    const dim3 grid((unsigned)n_tiles, (unsigned)n_cols);
    hipLaunchKernelGGL(ms_tile_sort_kernel, grid, dim3(SB), 0, st, s);
    int from = 0;
    for (int64_t w = ST; w < max_len; w *= 2, from ^= 1) hipLaunchKernelGGL(ms_merge_kernel, grid, dim3(SB), 0, st, s, from, w);
    hipLaunchKernelGGL(ms_order_kernel, grid, dim3(SB), 0, st, s, from);
    return hipGetLastError();
}

// Segment offsets and the tile table for segments of `len` records (each 1 .. 2^31 - 1, checked by the caller).
static void ms_tiles(int64_t n_seg, const int64_t *len, std::vector<int64_t> &row_off, std::vector<int32_t> &tile_seg, std::vector<int32_t> &tile_idx, int64_t &total, int64_t &longest) {
    row_off.resize((size_t)n_seg);
    total = longest = 0;
    for (int64_t s = 0; s < n_seg; ++s) {
        row_off[(size_t)s] = total;
        total += len[s];
        longest = std::max(longest, len[s]);
        for (int64_t t = 0; t * ST < len[s]; ++t) { tile_seg.push_back((int32_t)s); tile_idx.push_back((int32_t)t); }
    }
}

static int ms_check_segments(int64_t n_seg, const int64_t *seg_len) {
    // 2^21 segments and 2^33 rows: at most 2^21 workgroups of 1024 lanes and fewer than 2^24 tiles of 256, below HIP's 2^32 threads a grid
    if (n_seg < 1 || n_seg > ((int64_t)1 << 21)) return p2s_set_error(P2S_ERR_INVALID_ARG, "%lld segments; expected 1 .. 2^21", (long long)n_seg);
    if (!seg_len) return p2s_set_error(P2S_ERR_INVALID_ARG, "null argument");
    int64_t total = 0;
    for (int64_t s = 0; s < n_seg; ++s) {
        if (seg_len[s] < 1 || seg_len[s] >= ((int64_t)1 << 31))
            return p2s_set_error(P2S_ERR_INVALID_ARG, "segment %lld has %lld rows; expected 1 .. 2^31 - 1", (long long)s, (long long)seg_len[s]);
        total += seg_len[s];
        if (total > ((int64_t)1 << 33)) return p2s_set_error(P2S_ERR_INVALID_ARG, "more than 2^33 rows in one call");
    }
    return P2S_OK;
}

// What p2s_stable_argsort_host and p2s_trimmed_means_host share: the keys up, the sort.
struct MsColumns {
    MsSort s{};
    std::vector<int64_t> row_off;
    std::vector<int32_t> tile_seg, tile_idx, len32;
    int64_t total = 0, longest = 0;
    char *small = nullptr, *rec = nullptr;
    int run(p2s_ctx *ctx, Stage &st, int64_t n_seg, const int64_t *seg_len, const double *data, bool want_sorted) {
        ms_tiles(n_seg, seg_len, row_off, tile_seg, tile_idx, total, longest);
        len32.resize((size_t)n_seg);
        for (int64_t i = 0; i < n_seg; ++i) len32[(size_t)i] = (int32_t)seg_len[i];
        const size_t ns = (size_t)n_seg, nt = tile_seg.size(), n = (size_t)total;
        Layout sm;
        const size_t o_off = sm.add(ns * 8), o_len = sm.add(ns * 4), o_ts = sm.add(nt * 4), o_ti = sm.add(nt * 4);
        std::vector<char> host(sm.bytes);
        memcpy(host.data() + o_off, row_off.data(), ns * 8);
        memcpy(host.data() + o_len, len32.data(), ns * 4);
        memcpy(host.data() + o_ts, tile_seg.data(), nt * 4);
        memcpy(host.data() + o_ti, tile_idx.data(), nt * 4);
        Layout rc;
        const size_t o_k0 = rc.add(n * 8), o_k1 = rc.add(n * 8), o_i0 = rc.add(n * 4), o_i1 = rc.add(n * 4), o_ord = rc.add(n * 4), o_sorted = rc.add(want_sorted ? n * 8 : 0);
        P2S_TRY(st.upload(s.src, data, n * sizeof(double)));
        P2S_TRY(st.upload(small, host.data(), sm.bytes));
        P2S_TRY(st.alloc(rec, rc.bytes));
        HIP_TRY(hipStreamSynchronize(ctx->stream));               // `host` is this function's: uploaded before it returns
        s.row_off = (const int64_t *)(small + o_off);
        s.seg_len = (const int32_t *)(small + o_len);
        s.tile_seg = (const int32_t *)(small + o_ts);
        s.tile_idx = (const int32_t *)(small + o_ti);
        s.col_stride = 0;
        s.key[0] = (uint64_t *)(rec + o_k0); s.key[1] = (uint64_t *)(rec + o_k1);
        s.idx[0] = (uint32_t *)(rec + o_i0); s.idx[1] = (uint32_t *)(rec + o_i1);
        s.order = (int32_t *)(rec + o_ord);
        s.sorted = want_sorted ? (double *)(rec + o_sorted) : nullptr;
        P2S_TRY(st.time_begin());
        HIP_TRY(p2s_launch_sort(s, (int64_t)nt, 1, longest, ctx->stream));
        return P2S_OK;
    }
};

// ---- C-ABI entry points (include/p2s.h) ----------------------------------------------------------------------------
extern "C" {

int p2s_stable_argsort_host(p2s_ctx *ctx, int64_t n_segments, const int64_t *seg_len, const double *data, int32_t *order) {
    if (!ctx) return p2s_set_error(P2S_ERR_INVALID_ARG, "null context");
    P2S_TRY(ms_check_segments(n_segments, seg_len));
    if (!data || !order) return p2s_set_error(P2S_ERR_INVALID_ARG, "null argument");
    HIP_TRY(hipSetDevice(ctx->device));
    Stage st{ctx};
    MsColumns c;
    P2S_TRY(c.run(ctx, st, n_segments, seg_len, data, false));
    P2S_TRY(st.time_end());
    P2S_TRY(st.down(order, c.s.order, (size_t)c.total * 4));
    return st.finish(P2S_TIMED_MEASURE);
}

int p2s_trimmed_means_host(p2s_ctx *ctx, int64_t n_segments, const int64_t *seg_len, const double *data, double half_trim, double *means) {
    if (!ctx) return p2s_set_error(P2S_ERR_INVALID_ARG, "null context");
    P2S_TRY(ms_check_segments(n_segments, seg_len));
    if (!data || !means) return p2s_set_error(P2S_ERR_INVALID_ARG, "null argument");
    if (!(half_trim >= 0.0 && half_trim <= 0.5)) return p2s_set_error(P2S_ERR_INVALID_ARG, "half_trim=%g; expected trimmed_extrema_percent / 2 in [0, 0.5]", half_trim);
    HIP_TRY(hipSetDevice(ctx->device));
    Stage st{ctx};
    MsColumns c;
    P2S_TRY(c.run(ctx, st, n_segments, seg_len, data, true));
    MsTrim t{};
    double *d_means;
    P2S_TRY(st.alloc(d_means, (size_t)n_segments * 8));
    t.vals = c.s.src; t.sorted = c.s.sorted; t.row_off = c.s.row_off; t.seg_len = c.s.seg_len;
    t.means = d_means; t.col_stride = 0; t.half_trim = half_trim;
    hipLaunchKernelGGL(ms_trim_kernel, dim3((unsigned)n_segments, 1), dim3(CT), 0, ctx->stream, t);
    HIP_TRY(hipGetLastError());
    P2S_TRY(st.time_end());
    P2S_TRY(st.down(means, d_means, (size_t)n_segments * 8));
    return st.finish(P2S_TIMED_MEASURE);
}

int p2s_body_measure_host(p2s_ctx *ctx, int32_t n_files, const int64_t *n_rows, const int32_t *n_markers, const double *data,
                          const int32_t *flags, const int32_t *roles, int32_t n_pairs, const int32_t *pairs,
                          const double *head_factor, const double *speed_threshold, const int32_t *n_speed_markers, double keep_fraction,
                          double angle_limit, double half_trim, double *sum_speeds, double *angles, int32_t *n_selected, int32_t *kept_pos,
                          int32_t *kept_frame, int32_t *n_kept, int32_t *branch, double *row_heights, double *row_values,
                          double *means) {
    if (!ctx) return p2s_set_error(P2S_ERR_INVALID_ARG, "null context");
    if (n_files < 1 || n_pairs < 0 || n_pairs > P2S_MEASURE_MAX_PAIRS)
        return p2s_set_error(P2S_ERR_INVALID_ARG, "bad shape: %d files, %d pairs; expected at least 1 file and 0 .. %d pairs", n_files, n_pairs, P2S_MEASURE_MAX_PAIRS);
    if (!n_rows || !n_markers || !data || !flags || !roles || (n_pairs > 0 && !pairs) || !head_factor || !speed_threshold || !n_selected ||
        !kept_pos || !kept_frame || !n_kept || !branch || !means)
        return p2s_set_error(P2S_ERR_INVALID_ARG, "null argument");
    P2S_TRY(ms_check_segments(n_files, n_rows));
    if (!(keep_fraction >= 0.0 && keep_fraction <= 1.0)) return p2s_set_error(P2S_ERR_INVALID_ARG, "keep_fraction=%g; expected 1 - fastest_frames_to_remove_percent in [0, 1]", keep_fraction);
    if (!(half_trim >= 0.0 && half_trim <= 0.5)) return p2s_set_error(P2S_ERR_INVALID_ARG, "half_trim=%g; expected trimmed_extrema_percent / 2 in [0, 0.5]", half_trim);
    if (!(angle_limit == angle_limit)) return p2s_set_error(P2S_ERR_INVALID_ARG, "angle_limit is NaN");
    const size_t nf = (size_t)n_files, np = (size_t)n_pairs, ncol = np + 2;
    std::vector<int64_t> tab_off(nf);
    std::vector<int32_t> n_speed(nf);
    int64_t cells = 0;
    bool any_restrict = false;
    for (int32_t f = 0; f < n_files; ++f) {
        const int32_t K = n_markers[f], fl = flags[f];
        const int32_t *role = roles + (size_t)f * P2S_MEASURE_ROLES, *pr = pairs + (size_t)f * np * 2;
        if (K < 1 || K > (1 << 20)) return p2s_set_error(P2S_ERR_INVALID_ARG, "file %d has %d markers; expected 1 .. 2^20", f, K);
        if (fl & ~P2S_MEASURE_FLAGS) return p2s_set_error(P2S_ERR_INVALID_ARG, "file %d: unknown flags 0x%x", f, fl);
        if ((fl & P2S_MEASURE_RESTRICT) && !(fl & P2S_MEASURE_ANGLES)) return p2s_set_error(P2S_ERR_INVALID_ARG, "file %d: P2S_MEASURE_RESTRICT without P2S_MEASURE_ANGLES", f);
        if (!(speed_threshold[f] == speed_threshold[f]) || !(head_factor[f] == head_factor[f])) return p2s_set_error(P2S_ERR_INVALID_ARG, "file %d: NaN speed threshold or head factor", f);
        for (int r = 0; r < P2S_MEASURE_ROLES; ++r)
            if (role[r] < -1 || role[r] >= K) return p2s_set_error(P2S_ERR_INVALID_ARG, "file %d: marker index %d of role %d out of range (%d markers)", f, role[r], r, K);
        if (fl & P2S_MEASURE_ANGLES)
            for (int r = 0; r < P2S_MEASURE_ROLES; ++r)
                if (r != 4 && r != 5 && !(r < 2 && role[5] >= 0) && role[r] < 0)          // the shoulders only stand in for a missing Neck
                    return p2s_set_error(P2S_ERR_INVALID_ARG, "file %d: the angles need role %d", f, r);
        for (size_t p = 0; p < 2 * np; ++p) {
            if (pr[p] < -1 || pr[p] > K + 1) return p2s_set_error(P2S_ERR_INVALID_ARG, "file %d: marker index %d of pair %zu out of range (%d markers)", f, pr[p], p / 2, K);
            if (pr[p] >= K && (role[2 * (pr[p] - K)] < 0 || role[2 * (pr[p] - K) + 1] < 0))
                return p2s_set_error(P2S_ERR_INVALID_ARG, "file %d: pair %zu uses a midpoint whose two markers are not given", f, p / 2);
        }
        if (fl & (P2S_MEASURE_HEIGHT | P2S_MEASURE_LEG)) {
            const int first = (fl & P2S_MEASURE_HEIGHT) && !(fl & P2S_MEASURE_FEET_CONST) ? 0 : 2, last = (fl & P2S_MEASURE_HEIGHT) ? P2S_MEASURE_HEIGHT_PAIRS : 6;
            if (n_pairs < last) return p2s_set_error(P2S_ERR_INVALID_ARG, "file %d: heights and leg lengths need the first %d pairs", f, last);
            for (int p = first; p < last; ++p)
                if (pr[2 * p] < 0 || pr[2 * p + 1] < 0) return p2s_set_error(P2S_ERR_INVALID_ARG, "file %d: pair %d is needed and not given", f, p);
        }
        n_speed[(size_t)f] = n_speed_markers ? n_speed_markers[f] : K;
        if (n_speed[(size_t)f] < 0 || n_speed[(size_t)f] > K) return p2s_set_error(P2S_ERR_INVALID_ARG, "file %d: %d speed markers out of range (%d markers)", f, n_speed[(size_t)f], K);
        any_restrict = any_restrict || (fl & P2S_MEASURE_RESTRICT);
        tab_off[(size_t)f] = cells;
        cells += n_rows[f] * 3 * K;
        if (cells > ((int64_t)1 << 36)) return p2s_set_error(P2S_ERR_INVALID_ARG, "more than 2^36 coordinates in one call");
    }
    std::vector<int64_t> row_off;
    std::vector<int32_t> tile_seg, tile_idx, rows32(nf);
    int64_t N, longest;
    ms_tiles(n_files, n_rows, row_off, tile_seg, tile_idx, N, longest);
    if ((int64_t)ncol * N > ((int64_t)1 << 33) || (int64_t)ncol * (int64_t)tile_seg.size() >= ((int64_t)1 << 24) || (int64_t)ncol * n_files >= ((int64_t)1 << 22))
        return p2s_set_error(P2S_ERR_INVALID_ARG, "%d files, %lld rows x %zu columns are too many for one call", n_files, (long long)N, ncol);
    for (size_t f = 0; f < nf; ++f) rows32[f] = (int32_t)n_rows[f];
    const size_t nt = tile_seg.size(), n = (size_t)N, M = ncol * n;

    Layout sm;                                                    // what the host knows
    const size_t o_tab = sm.add(nf * 8), o_row = sm.add(nf * 8), o_head = sm.add(nf * 8), o_thr = sm.add(nf * 8), o_n = sm.add(nf * 4),
                 o_k = sm.add(nf * 4), o_ns = sm.add(nf * 4), o_fl = sm.add(nf * 4), o_role = sm.add(nf * P2S_MEASURE_ROLES * 4), o_pair = sm.add(nf * np * 8),
                 o_ts = sm.add(nt * 4), o_ti = sm.add(nt * 4);
    std::vector<char> host(sm.bytes);
    memcpy(host.data() + o_tab, tab_off.data(), nf * 8);
    memcpy(host.data() + o_row, row_off.data(), nf * 8);
    memcpy(host.data() + o_head, head_factor, nf * 8);
    memcpy(host.data() + o_thr, speed_threshold, nf * 8);
    memcpy(host.data() + o_n, rows32.data(), nf * 4);
    memcpy(host.data() + o_k, n_markers, nf * 4);
    memcpy(host.data() + o_ns, n_speed.data(), nf * 4);
    memcpy(host.data() + o_fl, flags, nf * 4);
    memcpy(host.data() + o_role, roles, nf * P2S_MEASURE_ROLES * 4);
    if (np) memcpy(host.data() + o_pair, pairs, nf * np * 8);
    memcpy(host.data() + o_ts, tile_seg.data(), nt * 4);
    memcpy(host.data() + o_ti, tile_idx.data(), nt * 4);
    Layout fp;                                                    // doubles
    const size_t o_speed = fp.add(n * 8), o_key1 = fp.add(n * 8), o_ang = fp.add(n * 8), o_vals = fp.add(M * 8), o_sorted = fp.add(M * 8), o_means = fp.add(nf * ncol * 8);
    Layout rc;                                                    // the sort's records
    const size_t o_k0 = rc.add(M * 8), o_k1 = rc.add(M * 8), o_i0 = rc.add(M * 4), o_i1 = rc.add(M * 4), o_ord3 = rc.add(M * 4);
    Layout in;                                                    // counters first: one memset
    const size_t o_cnt = in.add(nf * 5 * 4), o_has = in.add(nf * np * 4);
    const size_t zero_bytes = in.bytes;
    const size_t o_ord1 = in.add(n * 4), o_ord2 = in.add(n * 4), o_pos = in.add(n * 4), o_frame = in.add(n * 4);

    HIP_TRY(hipSetDevice(ctx->device));
    Stage st{ctx};
    char *d_sm, *d_fp, *d_rc, *d_in;
    MsArgs a{};
    P2S_TRY(st.upload(a.data, data, (size_t)cells * sizeof(double)));
    P2S_TRY(st.upload(d_sm, host.data(), sm.bytes));
    P2S_TRY(st.alloc(d_fp, fp.bytes));
    P2S_TRY(st.alloc(d_rc, rc.bytes));
    P2S_TRY(st.alloc(d_in, in.bytes));
    HIP_TRY(hipMemsetAsync(d_in, 0, zero_bytes, ctx->stream));
    a.tab_off = (const int64_t *)(d_sm + o_tab); a.row_off = (const int64_t *)(d_sm + o_row);
    a.head_factor = (const double *)(d_sm + o_head); a.speed_thr = (const double *)(d_sm + o_thr);
    a.n_rows = (const int32_t *)(d_sm + o_n); a.n_mk = (const int32_t *)(d_sm + o_k); a.n_speed = (const int32_t *)(d_sm + o_ns); a.flags = (const int32_t *)(d_sm + o_fl);
    a.roles = (const int32_t *)(d_sm + o_role); a.pairs = (const int32_t *)(d_sm + o_pair);
    a.tile_seg = (const int32_t *)(d_sm + o_ts); a.tile_idx = (const int32_t *)(d_sm + o_ti);
    a.keep_fraction = keep_fraction; a.angle_limit = angle_limit; a.half_trim = half_trim;
    a.N = N; a.n_files = n_files; a.n_pairs = n_pairs; a.n_cols = (int32_t)ncol;
    a.speed = (double *)(d_fp + o_speed); a.key1 = (double *)(d_fp + o_key1); a.ang = (double *)(d_fp + o_ang);
    a.vals = (double *)(d_fp + o_vals); a.sorted = (double *)(d_fp + o_sorted); a.means = (double *)(d_fp + o_means);
    int32_t *cnt = (int32_t *)(d_in + o_cnt);
    a.n_pos = cnt; a.n_sel = cnt + nf; a.n_lt = cnt + 2 * nf; a.n_kept = cnt + 3 * nf; a.branch = cnt + 4 * nf;
    a.has_value = (int32_t *)(d_in + o_has);
    a.order1 = (int32_t *)(d_in + o_ord1); a.order2 = (int32_t *)(d_in + o_ord2);
    a.kept_pos = (int32_t *)(d_in + o_pos); a.kept_frame = (int32_t *)(d_in + o_frame);
    MsSort s{};
    s.row_off = a.row_off; s.tile_seg = a.tile_seg; s.tile_idx = a.tile_idx; s.col_stride = N;
    s.key[0] = (uint64_t *)(d_rc + o_k0); s.key[1] = (uint64_t *)(d_rc + o_k1);
    s.idx[0] = (uint32_t *)(d_rc + o_i0); s.idx[1] = (uint32_t *)(d_rc + o_i1);
    const dim3 tiles((unsigned)nt), files((unsigned)n_files);
    hipStream_t q = ctx->stream;
    P2S_TRY(st.time_begin());
    hipLaunchKernelGGL(ms_speed_kernel, tiles, dim3(SB), 0, q, a);
    s.src = a.key1; s.seg_len = a.n_rows; s.order = a.order1; s.sorted = nullptr;
    HIP_TRY(p2s_launch_sort(s, (int64_t)nt, 1, longest, q));
    hipLaunchKernelGGL(ms_select_kernel, dim3((unsigned)((n_files + 63) / 64)), dim3(64), 0, q, a);
    hipLaunchKernelGGL(ms_angle_kernel, tiles, dim3(SB), 0, q, a);
    if (any_restrict) {                                           // order2 is read by the files that restrict alone
        s.src = a.ang; s.seg_len = a.n_sel; s.order = a.order2;
        HIP_TRY(p2s_launch_sort(s, (int64_t)nt, 1, longest, q));
    }
    hipLaunchKernelGGL(ms_keep_kernel, files, dim3(SB), 0, q, a);
    if (n_pairs > 0) hipLaunchKernelGGL(ms_length_kernel, tiles, dim3(SB), 0, q, a);
    hipLaunchKernelGGL(ms_height_kernel, tiles, dim3(SB), 0, q, a);
    s.src = a.vals; s.seg_len = a.n_kept; s.order = (int32_t *)(d_rc + o_ord3); s.sorted = a.sorted;
    HIP_TRY(p2s_launch_sort(s, (int64_t)nt, (int)ncol, longest, q));
    MsTrim t{};
    t.vals = a.vals; t.sorted = a.sorted; t.row_off = a.row_off; t.seg_len = a.n_kept; t.means = a.means; t.col_stride = N; t.half_trim = half_trim;
    hipLaunchKernelGGL(ms_trim_kernel, dim3((unsigned)n_files, (unsigned)ncol), dim3(CT), 0, q, t);
    HIP_TRY(hipGetLastError());
    P2S_TRY(st.time_end());
    P2S_TRY(st.down(sum_speeds, a.speed, n * 8));
    P2S_TRY(st.down(angles, a.ang, n * 8));
    P2S_TRY(st.down(n_selected, a.n_sel, nf * 4));
    P2S_TRY(st.down(kept_pos, a.kept_pos, n * 4));
    P2S_TRY(st.down(kept_frame, a.kept_frame, n * 4));
    P2S_TRY(st.down(n_kept, a.n_kept, nf * 4));
    P2S_TRY(st.down(branch, a.branch, nf * 4));
    P2S_TRY(st.down(row_heights, a.vals + np * n, n * 8));
    P2S_TRY(st.down(row_values, a.vals, M * 8));
    P2S_TRY(st.down(means, a.means, nf * ncol * 8));
    return st.finish(P2S_TIMED_MEASURE);                          // `host` is host memory: alive until here
}

int p2s_measure_kernel_ms(p2s_ctx *ctx, float *elapsed_ms) {
    return p2s_kernel_ms_query(ctx, P2S_TIMED_MEASURE, "none of p2s_stable_argsort_host, p2s_trimmed_means_host and p2s_body_measure_host", elapsed_ms);
}

}  // extern "C"
