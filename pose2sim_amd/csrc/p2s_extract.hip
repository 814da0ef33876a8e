// p2s_extract.hip -- the primary-person selection of Utilities/pose_extract_person.py:37-87 (_select_person, the rule of
// p2s_json_select_tracked_person) for every camera at once, as a prefix scan instead of a loop over the frames.
//
// Why it is a scan.  Whether a frame selects anybody does not depend on earlier choices: a frame with a candidate always
// selects one.  So the previous selecting frame of every frame is a running maximum, and what frame f chooses is a function
// of which candidate that previous frame chose: map[f][j], at most 32 entries of one byte.  Functions compose
// associatively; the choices are the prefix composition of the maps along the camera, and all the arithmetic -- distances,
// square roots, np.mean in NumPy's order -- happens before the scan, in parallel over (frame, previous candidate, candidate).
//
//   ext_person_kernel      per person: the number of confidences above the threshold and the candidate flag
//   ext_frame_kernel       per frame: its candidates in list order, their count, the fallback choice (the first candidate
//                          with the most confidences); per tile of 256 frames the last frame with a candidate
//   cam_tile_scan_kernel   (p2s_scan.h) per camera: running maximum over those tiles
//   cam_prev_kernel        (p2s_scan.h) per frame: the last earlier frame with a candidate
//   ext_map_kernel         per frame, one wave: map[f][j] for every candidate j of the previous selecting frame.  A frame
//                          without candidates gets the identity, a frame with one candidate and the first selecting frame
//                          of a camera a constant map
//   ext_tile_agg_kernel    per tile of T = 32 frames: the composition of its maps, walked once per entry state, 32 lanes wide
//   ext_agg_scan_kernel    per camera, one workgroup: the state on entry of every tile (composition is a gather)
//   ext_walk_kernel        per tile: walked again from its true entry state; writes `chosen`
//
// The hand-off between the phases is the launch boundary: no workgroup waits for another inside a launch, there is no
// flag, no look-back and no atomic.  Bit equality as in p2s_idswitch.hip: contraction is off for this file, the root is
// __dsqrt_rn, the sum is p2s_npsum_small.h's.  T is discussed in DESIGN.md 4.17.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>
#include <vector>

#include "p2s_ctx.h"
#include "p2s_npsum_small.h"
#include "p2s_scan.h"

#pragma clang fp contract(off)

#define P2S_EXT_MAX_CAND 32
#define P2S_EXT_MAX_KPTS 127

struct P2sExtArgs {
    const double *persons;       // [N][K][3]
    const int64_t *person_off;   // [frames + 1]
    const int64_t *frame_off;    // [C + 1]
    int32_t *pinfo;              // [N] confidences above the threshold; bit 16: a candidate
    int32_t *cand_list;          // [N] from person_off[f]: the candidates of frame f, as indices into the frame's run
    int32_t *count, *prev, *chosen;   // [frames]
    uint8_t *fallback;           // [frames] the fallback choice, as a position in the frame's candidate list
    uint8_t *map;                // [frames][32]
    uint8_t *agg;                // [C][tiles][32] the composed map of every tile
    uint8_t *entry;              // [C][tiles] the state on entry of every tile
    int64_t *tile_value, *tile_before;   // [C][ptiles] the running maximum's tiles
    double thr;
    int64_t N;
    int32_t C, K, ptiles, tiles;
};

namespace {

constexpr int TILE = CAM_TILE;           // frames per workgroup of the per-frame passes: the shared scan's tile, 256
constexpr int T = 32;                    // frames per tile of the map scan: one lane of a 32-lane group each
constexpr int GROUPS = 8;                // tiles per workgroup of the two walks
constexpr int MC = P2S_EXT_MAX_CAND;

__device__ __forceinline__ double ext_inf() { return __longlong_as_double(0x7ff0000000000000LL); }

__global__ void __launch_bounds__(256) ext_person_kernel(const P2sExtArgs a) {
    const int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (p >= a.N) return;
    const double *v = a.persons + p * 3 * a.K;
    int cnt = 0, cand = 0;
    for (int k = 0; k < a.K; ++k) {
        const double x = v[3 * k], cf = v[3 * k + 2];
        const int above = cf > a.thr;
        cnt += above;
        cand |= above && x == x;
    }
    a.pinfo[p] = cnt | (cand << 16);                              // cnt <= 127
}

__global__ void __launch_bounds__(TILE) ext_frame_kernel(const P2sExtArgs a) {
    __shared__ int64_t part[TILE / 64];
    const int c = blockIdx.y, tid = threadIdx.x;
    const int64_t f_base = a.frame_off[c], F = a.frame_off[c + 1] - f_base;
    const int64_t t0 = (int64_t)blockIdx.x * TILE;
    if (t0 >= F) return;                                          // uniform over the workgroup
    const int64_t f = t0 + tid;
    int64_t key = -1;
    if (f < F) {
        const int64_t p0 = a.person_off[f_base + f], p1 = a.person_off[f_base + f + 1];
        int32_t n = 0, most = -1, fb = 0;
        for (int64_t p = p0; p < p1; ++p) {
            const int32_t info = a.pinfo[p];
            if (info >> 16) {
                a.cand_list[p0 + n] = (int32_t)(p - p0);          // n <= p - p0: inside the frame's own run
                if ((info & 0xffff) > most) { most = info & 0xffff; fb = n; }
                ++n;
            }
        }
        a.count[f_base + f] = n;
        a.fallback[f_base + f] = (uint8_t)(fb < MC ? fb : 0);
        if (n > 0) key = f;
    }
    int64_t last;
    (void)block_scan_exclusive<OpMax>(key, part, &last);
    if (tid == 0) a.tile_value[(int64_t)c * a.ptiles + blockIdx.x] = last;
}

// ---- the transition map of a frame ---------------------------------------------------------------------------------------
// One workgroup of one wave a frame.  Lane p takes the pair (p / Q, p % Q) of the P candidates of the previous selecting
// frame and the Q of this one (pairs beyond 64 in further rounds), walks the keypoints and keeps the distances of the shared
// ones in its column of the LDS table, so that the mean can be summed in np.add.reduce's order once their number is known.
// Lane j then takes the strictly smallest mean of its row, the first on ties, round by round.
__global__ void __launch_bounds__(64) ext_map_kernel(const P2sExtArgs a) {
    extern __shared__ double dist[];                              // [K + 1][64]: lane l's distances in dist[. * 64 + l]
    const int c = blockIdx.y, lane = threadIdx.x;
    const int64_t f_base = a.frame_off[c], F = a.frame_off[c + 1] - f_base;
    const int64_t f = blockIdx.x;
    if (f >= F) return;                                           // uniform over the workgroup
    const int64_t gf = f_base + f;
    const int Q = a.count[gf], pv = a.prev[gf];
    const int P = pv >= 0 ? a.count[f_base + pv] : 0;
    uint8_t *m = a.map + gf * MC;
    const int fb = a.fallback[gf];
    if (Q == 0) {                                                 // nobody selected: the state passes through
        if (lane < MC) m[lane] = (uint8_t)lane;
        return;
    }
    if (Q == 1 || P == 0 || Q > MC || P > MC) {                   // the only candidate; no earlier choice: the fallback.
        if (lane < MC) m[lane] = (uint8_t)(Q == 1 || P == 0 ? (Q == 1 ? 0 : fb) : 0);   // (beyond 32: refused by the caller)
        return;
    }
    const int64_t a0 = a.person_off[f_base + pv], b0 = a.person_off[gf];
    const int K = a.K;
    const double thr = a.thr;
    double best = ext_inf();
    int found = -1;
    double *round_cost = dist + K * 64;                           // the means of the round's 64 pairs
    for (int first = 0; first < P * Q; first += 64) {             // uniform trip count
        const int pair = first + lane;
        if (pair < P * Q) {
            const int j = pair / Q, i = pair % Q;                 // previous candidate j, candidate i
            const double *pa = a.persons + (a0 + a.cand_list[a0 + j]) * 3 * K;
            const double *pb = a.persons + (b0 + a.cand_list[b0 + i]) * 3 * K;
            int n = 0;
            for (int k = 0; k < K; ++k) {
                const double ax = pa[3 * k], bx = pb[3 * k];
                if (pa[3 * k + 2] > thr && ax == ax && pb[3 * k + 2] > thr && bx == bx) {
                    const double dx = bx - ax, dy = pb[3 * k + 1] - pa[3 * k + 1];
                    dist[n++ * 64 + lane] = __dsqrt_rn(dx * dx + dy * dy);   // n <= K entries
                }
            }
            round_cost[lane] = n == 0 ? ext_inf() : p2s_np_sum_below_128<64>(dist + lane, n) / (double)n;
        }
        __syncthreads();
        // lane j takes its row's pairs of this round, in rising i over the rounds: the first of equal means stays
        if (lane < P) {
            const int lo = lane * Q > first ? lane * Q : first, hi = (lane + 1) * Q < first + 64 ? (lane + 1) * Q : first + 64;
            for (int q = lo; q < hi; ++q) {                       // q - first in [0, 64), q < P * Q
                const double d = round_cost[q - first];
                if (d < best) { best = d; found = q - lane * Q; } // strictly smaller: NaN and inf never win
            }
        }
        __syncthreads();                                          // round_cost may be written again
    }
    if (lane < MC) m[lane] = (uint8_t)(lane < P && found >= 0 ? found : fb);   // < Q <= 32; states of P and beyond are never entered
}

// ---- the scan of the maps --------------------------------------------------------------------------------------------------
// The maps of the T frames of tile t of camera c into the group's LDS rows: lane l brings frame t * T + l, the identity
// beyond the camera's last frame.
__device__ __forceinline__ void ext_stage_tile(const P2sExtArgs &a, int64_t f_base, int64_t F, int64_t t, int l, uint8_t (*rows)[MC]) {
    const int64_t f = t * T + l;
    uint4 lo = make_uint4(0x03020100u, 0x07060504u, 0x0b0a0908u, 0x0f0e0d0cu);
    uint4 hi = make_uint4(0x13121110u, 0x17161514u, 0x1b1a1918u, 0x1f1e1d1cu);
    if (f < F) {
        const uint4 *src = (const uint4 *)(a.map + (f_base + f) * MC);   // 32-byte rows of a 256-byte aligned buffer
        lo = src[0];
        hi = src[1];
    }
    uint4 *dst = (uint4 *)rows[l];
    dst[0] = lo;
    dst[1] = hi;
}

__global__ void __launch_bounds__(GROUPS * 32) ext_tile_agg_kernel(const P2sExtArgs a) {
    __shared__ __attribute__((aligned(16))) uint8_t rows[GROUPS][T][MC];
    const int c = blockIdx.y, g = threadIdx.x >> 5, l = threadIdx.x & 31;
    const int64_t f_base = a.frame_off[c], F = a.frame_off[c + 1] - f_base;
    const int64_t t = (int64_t)blockIdx.x * GROUPS + g;
    ext_stage_tile(a, f_base, F, t, l, rows[g]);
    __syncthreads();
    int s = l;                                                    // lane l walks the tile from entry state l
    for (int i = 0; i < T; ++i) s = rows[g][i][s];                // every entry of a map is below 32
    if (t < a.tiles) a.agg[((int64_t)c * a.tiles + t) * MC + l] = (uint8_t)s;
}

__global__ void __launch_bounds__(1024) ext_agg_scan_kernel(const P2sExtArgs a) {
    __shared__ uint8_t chunk_map[32][MC];
    const int c = blockIdx.x, g = threadIdx.x >> 5, l = threadIdx.x & 31;
    const int64_t F = a.frame_off[c + 1] - a.frame_off[c];
    const int64_t nt = (F + T - 1) / T;                           // <= a.tiles
    const int64_t per = (nt + 31) / 32;                           // tiles a group of 32 lanes
    const int64_t t_lo = g * per < nt ? g * per : nt, t_hi = t_lo + per < nt ? t_lo + per : nt;
    const uint8_t *agg = a.agg + (int64_t)c * a.tiles * MC;
    int s = l;
    for (int64_t t = t_lo; t < t_hi; ++t) s = agg[t * MC + s];
    chunk_map[g][l] = (uint8_t)s;
    __syncthreads();
    int e = 0;                                                    // the first selecting frame's map is constant: any state will do
    for (int gg = 0; gg < g; ++gg) e = chunk_map[gg][e];
    if (l == 0)
        for (int64_t t = t_lo; t < t_hi; ++t) {
            a.entry[(int64_t)c * a.tiles + t] = (uint8_t)e;
            e = agg[t * MC + e];
        }
}

__global__ void __launch_bounds__(GROUPS * 32) ext_walk_kernel(const P2sExtArgs a) {
    __shared__ __attribute__((aligned(16))) uint8_t rows[GROUPS][T][MC];
    __shared__ uint8_t state[GROUPS][T];
    const int c = blockIdx.y, g = threadIdx.x >> 5, l = threadIdx.x & 31;
    const int64_t f_base = a.frame_off[c], F = a.frame_off[c + 1] - f_base;
    const int64_t t = (int64_t)blockIdx.x * GROUPS + g;
    ext_stage_tile(a, f_base, F, t, l, rows[g]);
    __syncthreads();
    if (l == 0 && t * T < F) {                                    // t * T < F: t < the camera's tiles <= a.tiles
        int s = a.entry[(int64_t)c * a.tiles + t];
        for (int i = 0; i < T; ++i) {
            s = rows[g][i][s];
            state[g][i] = (uint8_t)s;
        }
    }
    __syncthreads();
    const int64_t f = t * T + l;
    if (f < F) {
        const int64_t gf = f_base + f;
        // a frame with candidates: its map's entries are positions in its own candidate list, below its count
        a.chosen[gf] = a.count[gf] > 0 ? a.cand_list[a.person_off[gf] + state[g][l]] : -1;
    }
}

hipError_t launch_track_select(const P2sExtArgs &a, int64_t max_frames, hipStream_t s) {
    if (max_frames == 0) return hipSuccess;
    const dim3 ptiles((unsigned)a.ptiles, (unsigned)a.C);
    const dim3 wtiles((unsigned)((a.tiles + GROUPS - 1) / GROUPS), (unsigned)a.C);
    if (a.N > 0) hipLaunchKernelGGL(ext_person_kernel, dim3((unsigned)((a.N + 255) / 256)), dim3(256), 0, s, a);
    const CamScanArgs sc{a.frame_off, a.count, a.tile_value, a.tile_before, a.prev, nullptr, nullptr, a.C, a.ptiles};
    hipLaunchKernelGGL(ext_frame_kernel, ptiles, dim3(TILE), 0, s, a);
    hipLaunchKernelGGL(cam_tile_scan_kernel<OpMax>, dim3((unsigned)a.C), dim3(1024), 0, s, sc);
    hipLaunchKernelGGL(cam_prev_kernel, ptiles, dim3(TILE), 0, s, sc);
    hipLaunchKernelGGL(ext_map_kernel, dim3((unsigned)max_frames, (unsigned)a.C), dim3(64), ((size_t)a.K + 1) * 64 * sizeof(double), s, a);   // at most 64 KiB
    hipLaunchKernelGGL(ext_tile_agg_kernel, wtiles, dim3(GROUPS * 32), 0, s, a);
    hipLaunchKernelGGL(ext_agg_scan_kernel, dim3((unsigned)a.C), dim3(1024), 0, s, a);
    hipLaunchKernelGGL(ext_walk_kernel, wtiles, dim3(GROUPS * 32), 0, s, a);
    return hipGetLastError();
}

}  // namespace

// ---- C-ABI entry points (include/p2s.h) ----------------------------------------------------------------------------
extern "C" {

int p2s_track_select_host(p2s_ctx *ctx, int32_t n_cams, const int64_t *n_frames, const int64_t *person_off, const double *persons,
                          int32_t n_kpts, double conf_threshold, int32_t *chosen, int32_t *n_candidates, int32_t *prev) {
    if (!ctx) return p2s_set_error(P2S_ERR_INVALID_ARG, "null context");
    P2S_TRY(p2s_check_n_cams(n_cams));
    if (n_kpts < 1 || n_kpts > P2S_EXT_MAX_KPTS) return p2s_set_error(P2S_ERR_INVALID_ARG, "n_kpts=%d outside [1, %d]", n_kpts, P2S_EXT_MAX_KPTS);
    if (!n_frames || !person_off) return p2s_set_error(P2S_ERR_INVALID_ARG, "null argument");
    const size_t C = (size_t)n_cams;
    std::vector<int64_t> frame_off(C + 1);
    P2sFrames fr;
    int64_t N;
    P2S_TRY(fr.build(n_cams, n_frames, 0, ((int64_t)1 << 31) - 1, frame_off.data()));
    P2S_TRY(fr.persons(person_off, persons, N));
    const int64_t frames = fr.frames, max_frames = fr.max_frames;
    // more than 32 candidates need more than 32 listed persons: only such a frame is counted here
    const int64_t values = 3 * (int64_t)n_kpts;
    for (size_t c = 0; c < C; ++c)
        for (int64_t f = frame_off[c]; f < frame_off[c + 1]; ++f) {
            if (person_off[f + 1] - person_off[f] <= P2S_EXT_MAX_CAND) continue;
            int64_t n = 0;
            for (int64_t p = person_off[f]; p < person_off[f + 1]; ++p) {
                const double *v = persons + p * values;
                bool cand = false;
                for (int k = 0; k < n_kpts && !cand; ++k) cand = v[3 * k + 2] > conf_threshold && v[3 * k] == v[3 * k];
                n += cand;
            }
            if (n > P2S_EXT_MAX_CAND)
                return p2s_set_error(P2S_ERR_INVALID_ARG, "camera %zu, frame %lld has %lld candidates; at most %d are supported", c,
                                     (long long)(f - frame_off[c]), (long long)n, P2S_EXT_MAX_CAND);
        }
    const int64_t ptiles = std::max<int64_t>((max_frames + TILE - 1) / TILE, 1), tiles = std::max<int64_t>((max_frames + T - 1) / T, 1);
    Layout lw, lb;                                                // 8-byte words; bytes
    const size_t n_ptile = C * (size_t)ptiles, n_tile = C * (size_t)tiles;
    const size_t o_foff = lw.add((C + 1) * 8), o_poff = lw.add(((size_t)frames + 1) * 8), o_tv = lw.add(n_ptile * 8), o_tb = lw.add(n_ptile * 8);
    const size_t o_map = lb.add((size_t)frames * MC), o_agg = lb.add(n_tile * MC), o_entry = lb.add(n_tile), o_fb = lb.add((size_t)frames);
    HIP_TRY(hipSetDevice(ctx->device));
    P2sExtArgs a{};
    Stage st{ctx};
    char *words;
    int32_t *ints;
    uint8_t *bytes;
    P2S_TRY(st.upload(a.persons, persons, (size_t)N * values * sizeof(double)));
    P2S_TRY(st.alloc(words, lw.bytes));
    P2S_TRY(st.up(words + o_foff, frame_off.data(), (C + 1) * 8));
    P2S_TRY(st.up(words + o_poff, person_off, ((size_t)frames + 1) * 8));
    P2S_TRY(st.alloc(ints, (2 * (size_t)N + 3 * (size_t)frames) * sizeof(int32_t)));
    P2S_TRY(st.alloc(bytes, lb.bytes));
    a.frame_off = (const int64_t *)(words + o_foff); a.person_off = (const int64_t *)(words + o_poff);
    a.tile_value = (int64_t *)(words + o_tv); a.tile_before = (int64_t *)(words + o_tb);
    a.count = ints; a.prev = ints + frames; a.chosen = ints + 2 * frames; a.pinfo = ints + 3 * frames; a.cand_list = a.pinfo + N;
    a.map = bytes + o_map; a.agg = bytes + o_agg; a.entry = bytes + o_entry; a.fallback = bytes + o_fb;
    a.thr = conf_threshold; a.N = N; a.C = n_cams; a.K = n_kpts; a.ptiles = (int32_t)ptiles; a.tiles = (int32_t)tiles;
    P2S_TRY(st.time_begin());
    HIP_TRY(launch_track_select(a, max_frames, ctx->stream));
    P2S_TRY(st.time_end());
    P2S_TRY(st.down(n_candidates, a.count, (size_t)frames * sizeof(int32_t)));
    P2S_TRY(st.down(prev, a.prev, (size_t)frames * sizeof(int32_t)));
    P2S_TRY(st.down(chosen, a.chosen, (size_t)frames * sizeof(int32_t)));
    return st.finish(P2S_TIMED_TRACK_SELECT);                     // frame_off and person_off are host memory: alive until here
}

int p2s_track_select_kernel_ms(p2s_ctx *ctx, float *elapsed_ms) { return p2s_kernel_ms_query(ctx, P2S_TIMED_TRACK_SELECT, "p2s_track_select_host", elapsed_ms); }

}  // extern "C"
