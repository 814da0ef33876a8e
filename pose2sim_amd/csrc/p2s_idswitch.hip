// p2s_idswitch.hip -- frame-to-frame person matching (Utilities/id_switch_analyze.py:47-145, 148-291, 364-388) and the
// assignment solver it needs.  float64 end to end: every number must be the reference's bit for bit.
//
//   ids_filter_kernel      per frame: the persons parse_frame_people keeps (some confidence above 0), their count and their
//                          stable list; per tile of 256 frames the last frame that holds a person
//   cam_tile_scan_kernel   (p2s_scan.h) per camera: exclusive scan of the tiles' values -- a running maximum (the last frame
//                          with a person before the tile) or a running sum (the matched distances before the tile)
//   cam_prev_kernel        (p2s_scan.h) per frame: the last earlier frame with a person (analyze_camera's prev_people) and
//                          the number of empty frames since (its zero_count)
//   ids_match_kernel       per frame with persons and a previous frame: the cost matrix (compute_match_cost), scipy's
//                          linear_sum_assignment (p2s_lsap.h), the matched distances in previous-person order, the numbers
//                          of unmatched previous and current persons
//   ids_count_kernel, ids_gather_kernel   the matched distances of a camera, compacted in frame order into one column
//   conf_compact_kernel, conf_mean_std_kernel (p2s_confidence.hip), order_stats_kernel (p2s_jitter.hip), ids_finish_kernel
//                          np.mean, np.median, np.percentile 95 and 99, min and max of every camera's column
//   lsap_kernel            linear_sum_assignment alone, on a batch of matrices of one shape
//
// Frames to lanes.  A frame is one workgroup of one wave.  The costs are parallel: lane p takes the pair (p / Q, p % Q) of
// the P previous and Q current persons (pairs beyond 64 in further rounds), walks the 26 keypoints and keeps the distances
// of the shared ones in its column of an LDS table, so that the mean can be summed in np.add.reduce's order once their
// number is known.  The solver is sequential: lane 0 runs it on the matrix the lanes left in LDS, its work arrays in LDS
// too (indexed at run time: registers would spill to scratch).  A typical frame holds 1 to 4 persons, so the solver's
// turn is a few dozen operations and the kernel is bound by the latency of its dependent loads, not by arithmetic; one
// wave a workgroup keeps the LDS per frame small enough for several frames a CU.
//
// Bit equality.  dx*dx + dy*dy must be rn(rn(dx*dx) + rn(dy*dy)): floating-point contraction is off for this whole file
// and the root is the correctly rounded __dsqrt_rn.  The mean of m distances is np.add.reduce's sum -- below 8 entries a
// plain loop from 0.0, else eight accumulators r[j] = d[j], r[j] += d[i + j] over the whole blocks of 8,
// ((r0+r1)+(r2+r3))+((r4+r5)+(r6+r7)), then the tail one by one -- and one division by m.  Counts and offsets are
// integers and every sum of them is a scan: no atomic of any kind, two runs give the same bytes.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>

#include <algorithm>
#include <vector>

#include "p2s_ctx.h"
#include "p2s_lsap.h"
#include "p2s_npsum_small.h"
#include "p2s_scan.h"

#pragma clang fp contract(off)

#define P2S_IDS_KPTS 26
#define P2S_IDS_VALUES (3 * P2S_IDS_KPTS)
#define P2S_IDS_TABLES 7         // count, prev, zero_run, n_matched, n_lost, n_appeared, flag
#define P2S_IDS_STATS 6          // mean, median, p95, p99, min, max
#define P2S_IDS_QUANTILES 3      // 50, 95, 99 %: two neighbours each
struct P2sIdsArgs {
    const double *persons;       // [N][26][3] every listed person of every frame, cameras back to back
    const int64_t *person_off;   // [frames + 1] first person of every frame (frames of all cameras back to back)
    const int64_t *frame_off;    // [C + 1]
    int32_t *valid_list;         // [N] from person_off[f]: the kept persons of frame f, as indices into the frame's list
    int32_t *count, *prev, *zero_run, *n_matched, *n_lost, *n_appeared, *flag;   // [frames] each
    int64_t *tile_value;         // [C][tiles] what cam_tile_scan_kernel scans
    int64_t *tile_before;        // [C][tiles] its result
    int64_t *n_dist;             // [C] the running sum's total: matched distances of the camera
    double *stage;               // [N] from person_off[f]: the matched distances of frame f
    double *table;               // [C][n_rows] the cameras' distances in frame order, NaN behind them
    double *valid;               // [C][n_rows] the columns' non-NaN entries (conf_compact_kernel)
    int64_t *m;                  // [C] what that compaction counted (= n_dist)
    double *minmax, *mean_std;   // [C][2] each
    const double *fractions;     // [3] 0.5, 0.95, 0.99
    double *order;               // [C][6] the entries at np.percentile's lo and hi of every fraction
    double *stats;               // [C][6]
    int64_t n_rows, max_frames;
    int32_t C, tiles;
};

struct P2sLsapArgs {
    const double *cost;          // [n][n_rows][n_cols]
    int32_t *row_ind, *col_ind;  // [n][min(n_rows, n_cols)]
    int32_t *status;             // [n] P2S_LSAP_*
    int64_t n;
    int32_t n_rows, n_cols;
};

namespace {

constexpr int TILE = CAM_TILE;           // frames per workgroup of the per-frame passes: the shared scan's tile, 256
constexpr int FLAG_TOO_MANY = 4;         // more than 32 kept persons in the frame or in its previous one: not matched

__device__ __forceinline__ double ids_nan() { return __longlong_as_double(0x7ff8000000000000LL); }

// OpMax, OpSum, wave_scan and block_scan_exclusive: p2s_scan.h

// ---- the person filter ---------------------------------------------------------------------------------------------------
// parse_frame_people :67-74: a person is dropped when every confidence is NaN or none is above 0 -- that is, kept when
// some confidence is above 0.  One lane a frame; a tile's value is its last frame with a kept person, -1 without one.
__global__ void __launch_bounds__(TILE) ids_filter_kernel(const P2sIdsArgs a) {
    __shared__ int64_t part[TILE / 64];
    const int c = blockIdx.y, tid = threadIdx.x;
    const int64_t f_base = a.frame_off[c], F = a.frame_off[c + 1] - f_base;
    const int64_t t0 = (int64_t)blockIdx.x * TILE;
    if (t0 >= F) return;                                          // uniform over the workgroup
    const int64_t f = t0 + tid;
    int64_t key = -1;
    if (f < F) {
        const int64_t p0 = a.person_off[f_base + f], p1 = a.person_off[f_base + f + 1];
        int32_t n = 0;
        for (int64_t p = p0; p < p1; ++p) {
            const double *v = a.persons + p * P2S_IDS_VALUES;
            bool any = false;
            for (int k = 0; k < P2S_IDS_KPTS; ++k) any |= v[3 * k + 2] > 0.0;
            if (any) a.valid_list[p0 + n++] = (int32_t)(p - p0);   // n <= p - p0: inside the frame's own run
        }
        a.count[f_base + f] = n;
        if (n > 0) key = f;
    }
    int64_t last;
    (void)block_scan_exclusive<OpMax>(key, part, &last);
    if (tid == 0) a.tile_value[(int64_t)c * a.tiles + blockIdx.x] = last;
}

// The scan of the tiles of a camera and the previous frame of every frame -- prev[f], and zero_run[f]: analyze_camera's
// zero_count when it reaches frame f -- are cam_tile_scan_kernel and cam_prev_kernel of p2s_scan.h.

// ---- cost matrix and assignment -------------------------------------------------------------------------------------------
struct MatchShared {
    double dist[P2S_IDS_KPTS][64];       // lane l's distances in dist[.][l]: no two lanes on one bank
    double cost[P2S_LSAP_MAX * P2S_LSAP_MAX];
    P2sLsapWork work;
    int row_ind[P2S_LSAP_MAX], col_ind[P2S_LSAP_MAX];
};

// compute_match_cost :77-97 of two persons' [26][3]; d = the calling lane's column of MatchShared::dist
__device__ __forceinline__ double match_cost(const double *pa, const double *pb, double (*d)[64], int lane) {
    int m = 0;
    for (int k = 0; k < P2S_IDS_KPTS; ++k) {
        if (pa[3 * k + 2] > 0.1 && pb[3 * k + 2] > 0.1) {         // CONF_THRESHOLD, both
            const double dx = pa[3 * k] - pb[3 * k], dy = pa[3 * k + 1] - pb[3 * k + 1];
            d[m++][lane] = __dsqrt_rn(dx * dx + dy * dy);         // m <= 26 entries
        }
    }
    if (m < 3) return 1e9;                                        // MIN_VALID_KP
    return p2s_np_sum_below_128<64>(&d[0][lane], m) / (double)m;
}

__global__ void __launch_bounds__(64) ids_match_kernel(const P2sIdsArgs a) {
    __shared__ MatchShared s;
    const int c = blockIdx.y, lane = threadIdx.x;
    const int64_t f_base = a.frame_off[c], F = a.frame_off[c + 1] - f_base;
    const int64_t f = blockIdx.x;
    if (f >= F) return;                                           // uniform over the workgroup
    const int64_t gf = f_base + f;
    const int Q = a.count[gf], pv = a.prev[gf];
    const int P = pv >= 0 && Q > 0 ? a.count[f_base + pv] : 0;
    int flag = 0, n_matched = 0;
    if (P > P2S_LSAP_MAX || Q > P2S_LSAP_MAX) {
        flag = FLAG_TOO_MANY;
    } else if (P > 0 && Q > 0) {                                  // match_people :119-145
        const int64_t a0 = a.person_off[f_base + pv], b0 = a.person_off[gf];
        for (int pair = lane; pair < P * Q; pair += 64) {
            const int i = pair / Q, j = pair % Q;                 // cost_matrix[i, j]: previous person i, current person j
            const double *pa = a.persons + (a0 + a.valid_list[a0 + i]) * P2S_IDS_VALUES;
            const double *pb = a.persons + (b0 + a.valid_list[b0 + j]) * P2S_IDS_VALUES;
            s.cost[pair] = match_cost(pa, pb, s.dist, lane);      // pair < 32 * 32
        }
        __syncthreads();
        if (lane == 0) {
            flag = p2s_lsap_solve(P, Q, s.cost, s.work, s.row_ind, s.col_ind);
            if (flag == P2S_LSAP_OK) {
                const int n = P < Q ? P : Q;
                for (int k = 0; k < n; ++k) {                     // ascending previous person
                    const double d = s.cost[s.row_ind[k] * Q + s.col_ind[k]];
                    if (d < 1e9) a.stage[b0 + n_matched++] = d;   // n_matched <= Q <= the frame's own run
                }
            }
        }
    }
    if (lane == 0) {
        const bool matched = flag == 0 && P > 0 && Q > 0;
        a.n_matched[gf] = n_matched;
        a.n_lost[gf] = matched ? P - n_matched : 0;
        a.n_appeared[gf] = matched ? Q - n_matched : 0;
        a.flag[gf] = flag;
    }
}

// ---- the distances of a camera, in frame order ---------------------------------------------------------------------------
__global__ void __launch_bounds__(TILE) ids_count_kernel(const P2sIdsArgs a) {
    __shared__ int64_t part[TILE / 64];
    const int c = blockIdx.y, tid = threadIdx.x;
    const int64_t f_base = a.frame_off[c], F = a.frame_off[c + 1] - f_base;
    const int64_t t0 = (int64_t)blockIdx.x * TILE;
    if (t0 >= F) return;
    const int64_t f = t0 + tid;
    int64_t total;
    (void)block_scan_exclusive<OpSum>(f < F ? a.n_matched[f_base + f] : 0, part, &total);
    if (tid == 0) a.tile_value[(int64_t)c * a.tiles + blockIdx.x] = total;
}

__global__ void __launch_bounds__(TILE) ids_gather_kernel(const P2sIdsArgs a) {
    __shared__ int64_t part[TILE / 64];
    const int c = blockIdx.y, tid = threadIdx.x;
    const int64_t f_base = a.frame_off[c], F = a.frame_off[c + 1] - f_base;
    const int64_t t0 = (int64_t)blockIdx.x * TILE;
    if (t0 >= F) return;
    const int64_t f = t0 + tid;
    const int n = f < F ? a.n_matched[f_base + f] : 0;
    const int64_t at = a.tile_before[(int64_t)c * a.tiles + blockIdx.x] + block_scan_exclusive<OpSum>(n, part, nullptr);
    if (n > 0) {
        const double *src = a.stage + a.person_off[f_base + f];
        double *dst = a.table + (int64_t)c * a.n_rows + at;       // at + n <= n_dist[c] <= the camera's persons <= n_rows
        for (int k = 0; k < n; ++k) dst[k] = src[k];
    }
}

__global__ void ids_fill_nan_kernel(double *x, int64_t n) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) x[i] = ids_nan();
}

// compute_distance_stats :379-388.  np.percentile, method 'linear', and np.median as conf_finish_kernel forms them.
__global__ void ids_finish_kernel(const P2sIdsArgs a) {
    const int c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= a.C) return;
    const int64_t m = a.m[c];
    double *out = a.stats + (int64_t)c * P2S_IDS_STATS;
    if (m == 0) {
        for (int i = 0; i < P2S_IDS_STATS; ++i) out[i] = ids_nan();
        return;
    }
    const double *q = a.order + (int64_t)c * 2 * P2S_IDS_QUANTILES;
    double pct[P2S_IDS_QUANTILES];
    for (int i = 0; i < P2S_IDS_QUANTILES; ++i) {
        const double vi = (double)(m - 1) * a.fractions[i];
        const double g = vi - floor(vi);
        const double lo = q[2 * i], hi = q[2 * i + 1], d = hi - lo;
        pct[i] = g >= 0.5 ? hi - d * (1.0 - g) : lo + d * g;
    }
    const double mid = 0.0 + q[0];
    out[0] = a.mean_std[2 * (int64_t)c];
    out[1] = (m & 1) ? mid : (mid + q[1]) / 2.0;
    out[2] = pct[1]; out[3] = pct[2];
    out[4] = a.minmax[2 * (int64_t)c];
    out[5] = a.minmax[2 * (int64_t)c + 1];
}

hipError_t launch_id_switch(const P2sIdsArgs &a, hipStream_t s) {
    const dim3 tiles((unsigned)a.tiles, (unsigned)a.C);
    const int64_t cells = (int64_t)a.C * a.n_rows;
    hipLaunchKernelGGL(ids_fill_nan_kernel, dim3((unsigned)((cells + 255) / 256)), dim3(256), 0, s, a.table, cells);
    CamScanArgs sc{a.frame_off, a.count, a.tile_value, a.tile_before, a.prev, a.zero_run, nullptr, a.C, a.tiles};
    if (a.max_frames > 0) {
        hipLaunchKernelGGL(ids_filter_kernel, tiles, dim3(TILE), 0, s, a);
        hipLaunchKernelGGL(cam_tile_scan_kernel<OpMax>, dim3((unsigned)a.C), dim3(1024), 0, s, sc);   // the running maximum has no total to keep
        hipLaunchKernelGGL(cam_prev_kernel, tiles, dim3(TILE), 0, s, sc);
        hipLaunchKernelGGL(ids_match_kernel, dim3((unsigned)a.max_frames, (unsigned)a.C), dim3(64), 0, s, a);
        hipLaunchKernelGGL(ids_count_kernel, tiles, dim3(TILE), 0, s, a);
    }
    sc.totals = a.n_dist;
    hipLaunchKernelGGL(cam_tile_scan_kernel<OpSum>, dim3((unsigned)a.C), dim3(1024), 0, s, sc);   // no frame at all: n_dist = 0
    if (a.max_frames > 0) hipLaunchKernelGGL(ids_gather_kernel, tiles, dim3(TILE), 0, s, a);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    // the statistics: one column a camera
    if ((e = p2s_launch_column_moments(a.table, a.valid, a.n_rows, a.C, a.m, a.minmax, a.mean_std, s)) != hipSuccess) return e;
    P2sOrderArgs o{};
    o.data = a.valid; o.col_len = a.m; o.n_rows = a.n_rows;       // the compacted columns: m entries, none NaN
    o.fractions = a.fractions;
    o.out = a.order;
    o.n_cols = a.C; o.n_ranks = 2 * P2S_IDS_QUANTILES;
    if ((e = p2s_launch_order_stats(o, s)) != hipSuccess) return e;
    hipLaunchKernelGGL(ids_finish_kernel, dim3((unsigned)((a.C + 63) / 64)), dim3(64), 0, s, a);
    return hipGetLastError();
}

// ---- linear_sum_assignment alone -----------------------------------------------------------------------------------------
// One matrix a workgroup of one wave: the lanes bring the matrix into LDS, lane 0 solves, the lanes store the answer.
struct LsapShared {
    double cost[P2S_LSAP_MAX * P2S_LSAP_MAX];
    P2sLsapWork work;
    int row_ind[P2S_LSAP_MAX], col_ind[P2S_LSAP_MAX];
    int status;
};

__global__ void __launch_bounds__(64) lsap_kernel(const P2sLsapArgs a) {
    __shared__ LsapShared s;
    const int lane = threadIdx.x, cells = a.n_rows * a.n_cols, n = a.n_rows < a.n_cols ? a.n_rows : a.n_cols;
    const int64_t b = blockIdx.x;
    for (int i = lane; i < cells; i += 64) s.cost[i] = a.cost[b * cells + i];   // cells <= 32 * 32
    __syncthreads();
    if (lane == 0) s.status = p2s_lsap_solve(a.n_rows, a.n_cols, s.cost, s.work, s.row_ind, s.col_ind);
    __syncthreads();
    const bool ok = s.status == P2S_LSAP_OK;
    if (lane < n) {                                               // n <= 32
        a.row_ind[b * n + lane] = ok ? s.row_ind[lane] : -1;
        a.col_ind[b * n + lane] = ok ? s.col_ind[lane] : -1;
    }
    if (lane == 0) a.status[b] = s.status;
}

}  // namespace

// ---- C-ABI entry points (include/p2s.h) ----------------------------------------------------------------------------
extern "C" {

int p2s_id_switch_host(p2s_ctx *ctx, int32_t n_cams, const int64_t *n_frames, const int64_t *person_off, const double *persons,
                       int32_t *tables, int32_t *kept, double *distances, int64_t *n_distances, double *stats) {
    if (!ctx) return p2s_set_error(P2S_ERR_INVALID_ARG, "null context");
    P2S_TRY(p2s_check_n_cams(n_cams));
    if (!n_frames || !person_off) return p2s_set_error(P2S_ERR_INVALID_ARG, "null argument");
    const size_t C = (size_t)n_cams;
    Layout lay;                                                   // `head` goes up as one: frame_off, np.percentile's fractions
    const size_t o_foff = lay.add((C + 1) * 8), o_frac = lay.add(P2S_IDS_QUANTILES * 8), head_b = lay.bytes;
    std::vector<char> head(head_b);
    int64_t *frame_off = (int64_t *)(head.data() + o_foff), N;
    P2sFrames fr;
    P2S_TRY(fr.build(n_cams, n_frames, 0, ((int64_t)1 << 31) - 1, frame_off));
    P2S_TRY(fr.persons(person_off, persons, N));
    const int64_t frames = fr.frames, max_frames = fr.max_frames;
    int64_t n_rows = 1;                                           // the longest camera's persons: room for its distances
    for (size_t c = 0; c < C; ++c) n_rows = std::max(n_rows, person_off[frame_off[c + 1]] - person_off[frame_off[c]]);
    const double fractions[P2S_IDS_QUANTILES] = {50 / 100.0, 95 / 100.0, 99 / 100.0};   // np.percentile: q / 100
    memcpy(head.data() + o_frac, fractions, sizeof fractions);
    const int64_t tiles = std::max<int64_t>((max_frames + TILE - 1) / TILE, 1);
    const size_t n_poff = (size_t)frames + 1, n_tile = C * (size_t)tiles;
    const size_t o_poff = lay.add(n_poff * 8), o_tv = lay.add(n_tile * 8), o_tb = lay.add(n_tile * 8), o_nd = lay.add(C * 8), o_m = lay.add(C * 8),
                 o_mm = lay.add(2 * C * 8), o_ms = lay.add(2 * C * 8), o_ord = lay.add(2 * P2S_IDS_QUANTILES * C * 8), o_stats = lay.add(P2S_IDS_STATS * C * 8);
    const size_t cells = C * (size_t)n_rows;
    HIP_TRY(hipSetDevice(ctx->device));
    P2sIdsArgs a{};
    Stage st{ctx};
    char *sm;
    int32_t *ints;
    P2S_TRY(st.upload(a.persons, persons, (size_t)N * P2S_IDS_VALUES * sizeof(double)));
    P2S_TRY(st.alloc(sm, lay.bytes));
    P2S_TRY(st.up(sm, head.data(), head_b));
    P2S_TRY(st.up(sm + o_poff, person_off, n_poff * 8));
    P2S_TRY(st.alloc(ints, ((size_t)P2S_IDS_TABLES * frames + N) * sizeof(int32_t)));
    P2S_TRY(st.alloc(a.stage, (size_t)N * sizeof(double)));
    P2S_TRY(st.alloc(a.table, cells * sizeof(double)));
    P2S_TRY(st.alloc(a.valid, cells * sizeof(double)));
    a.frame_off = (const int64_t *)(sm + o_foff); a.fractions = (const double *)(sm + o_frac); a.person_off = (const int64_t *)(sm + o_poff);
    a.tile_value = (int64_t *)(sm + o_tv); a.tile_before = (int64_t *)(sm + o_tb); a.n_dist = (int64_t *)(sm + o_nd); a.m = (int64_t *)(sm + o_m);
    a.minmax = (double *)(sm + o_mm); a.mean_std = (double *)(sm + o_ms); a.order = (double *)(sm + o_ord); a.stats = (double *)(sm + o_stats);
    a.count = ints; a.prev = ints + frames; a.zero_run = ints + 2 * frames; a.n_matched = ints + 3 * frames;
    a.n_lost = ints + 4 * frames; a.n_appeared = ints + 5 * frames; a.flag = ints + 6 * frames;
    a.valid_list = ints + (size_t)P2S_IDS_TABLES * frames;
    a.n_rows = n_rows; a.max_frames = max_frames; a.C = n_cams; a.tiles = (int32_t)tiles;
    P2S_TRY(st.time_begin());
    HIP_TRY(launch_id_switch(a, ctx->stream));
    P2S_TRY(st.time_end());
    std::vector<int64_t> nd(C);
    std::vector<double> table(distances ? cells : 0);
    P2S_TRY(st.down(tables, ints, (size_t)P2S_IDS_TABLES * frames * sizeof(int32_t)));
    P2S_TRY(st.down(kept, a.valid_list, (size_t)N * sizeof(int32_t)));
    P2S_TRY(st.down(nd.data(), a.n_dist, C * 8));
    P2S_TRY(st.down(stats, a.stats, P2S_IDS_STATS * C * 8));
    if (distances) P2S_TRY(st.down(table.data(), a.table, cells * sizeof(double)));
    P2S_TRY(st.finish(P2S_TIMED_ID_SWITCH));                      // `head` and person_off are host memory: alive until here
    int64_t at = 0;                                               // the cameras' distances back to back
    for (size_t c = 0; c < C; ++c) {
        if (n_distances) n_distances[c] = nd[c];
        if (distances) std::copy(table.begin() + c * n_rows, table.begin() + c * n_rows + nd[c], distances + at);
        at += nd[c];
    }
    return P2S_OK;
}

int p2s_lsap_host(p2s_ctx *ctx, int64_t n, int32_t n_rows, int32_t n_cols, const double *cost, int32_t *row_ind, int32_t *col_ind,
                  int32_t *status) {
    if (n < 0 || n >= ((int64_t)1 << 31) || n_rows < 1 || n_rows > P2S_LSAP_MAX || n_cols < 1 || n_cols > P2S_LSAP_MAX)
        return p2s_set_error(P2S_ERR_INVALID_ARG, "bad shape: %lld matrices of %d x %d; expected 1 .. %d rows and columns", (long long)n,
                             n_rows, n_cols, P2S_LSAP_MAX);
    if (n == 0) return P2S_OK;
    if (!cost || !row_ind || !col_ind || !status) return p2s_set_error(P2S_ERR_INVALID_ARG, "null argument");
    const size_t cells = (size_t)n_rows * n_cols, k = (size_t)std::min(n_rows, n_cols);
    if (!ctx) {                                                   // p2s_lsap.h compiled for the host
        P2sLsapWork work;
        int rows[P2S_LSAP_MAX], cols[P2S_LSAP_MAX];
        for (int64_t b = 0; b < n; ++b) {
            status[b] = p2s_lsap_solve(n_rows, n_cols, cost + b * cells, work, rows, cols);
            for (size_t i = 0; i < k; ++i) {
                row_ind[b * k + i] = status[b] == P2S_LSAP_OK ? rows[i] : -1;
                col_ind[b * k + i] = status[b] == P2S_LSAP_OK ? cols[i] : -1;
            }
        }
        return P2S_OK;
    }
    HIP_TRY(hipSetDevice(ctx->device));
    P2sLsapArgs a{};
    a.n = n; a.n_rows = n_rows; a.n_cols = n_cols;
    Stage st{ctx};
    P2S_TRY(st.upload(a.cost, cost, (size_t)n * cells * sizeof(double)));
    P2S_TRY(st.alloc(a.row_ind, (size_t)n * (2 * k + 1) * sizeof(int32_t)));
    a.col_ind = a.row_ind + n * k; a.status = a.col_ind + n * k;
    hipLaunchKernelGGL(lsap_kernel, dim3((unsigned)n), dim3(64), 0, ctx->stream, a);
    HIP_TRY(hipGetLastError());
    P2S_TRY(st.down(row_ind, a.row_ind, (size_t)n * k * sizeof(int32_t)));
    P2S_TRY(st.down(col_ind, a.col_ind, (size_t)n * k * sizeof(int32_t)));
    P2S_TRY(st.down(status, a.status, (size_t)n * sizeof(int32_t)));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    return P2S_OK;
}

int p2s_id_switch_kernel_ms(p2s_ctx *ctx, float *elapsed_ms) { return p2s_kernel_ms_query(ctx, P2S_TIMED_ID_SWITCH, "p2s_id_switch_host", elapsed_ms); }

}  // extern "C"
