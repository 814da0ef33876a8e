// p2s_timeline.hip -- the rows of Utilities/confidence_timeline.py:89-130 for every camera folder at once: one row per
// (frame, person, keypoint) in the reference's order, and the same confidences grouped per (keypoint, person) -- its
// `grouped`, the series of the scatter plot.  Integers and copied doubles only.
//
//   tl_count_kernel        per tile of 256 files of a camera: the rows its files contribute, K a valid person
//   cam_tile_scan_kernel   (p2s_scan.h) per camera: the tiles' rows scanned along the camera; then, the cameras' totals
//                          taken as the tiles of one long camera, the same kernel once more: row_off
//   tl_rows_kernel         per tile: the first row of every file (a workgroup scan on top of the tile's entry), then one
//                          lane a person: its file by a search of the tile's person offsets in LDS, its rank among the
//                          file's valid persons counted in the lane, its K rows written
//   tl_series_kernel<0>    per (series, tile): the files of the tile in which entry p of the list is valid
//   cam_tile_scan_kernel   per series along its camera's files, then over the series' lengths: series_off
//   tl_series_kernel<1>    per (series, tile): the position of every such file in the series, frame and K confidences
//
// Why the series are a scan.  Whether a listed person yields rows depends on the length of its list alone, not on the
// keypoint: the series of (slot, person p) of a camera holds one entry for every file whose entry p is valid, in file
// order, for every slot alike.  So a file's position in the series of p is the exclusive sum, down the camera's files,
// of column p of a files x P_c table of 0 / 1, P_c the camera's longest list -- the scan the rows use, with (camera,
// person index) pairs where the rows have cameras.  No atomic decides a position: the order is the scan's.
// ctx == NULL runs the same functions on the host, file after file: the logic is checked without a GPU.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>
#include <vector>

#include "p2s_ctx.h"
#include "p2s_scan.h"

#define TL_HD __host__ __device__ inline
#define P2S_TL_MAX_K 26

struct P2sTlArgs {
    const int64_t *file_off;     // [C + 1]
    const int64_t *person_base;  // [n_files + 1]
    const uint8_t *valid;        // [N]
    const double *conf;          // [N][K]
    const int64_t *series_files; // [S + 1] the series as the scan's cameras: series q has the files of its camera
    const int64_t *people_off;   // [C + 1] the first series of every camera: the running sum of P_c
    const int32_t *series_cam;   // [S]
    int64_t *tv_rows, *tb_rows;  // [C][tiles] rows of every tile of files; rows of the camera before the tile
    int64_t *cam_rows;           // [C]
    int64_t *row_off;            // [C + 1]
    int64_t *tv_ser, *tb_ser;    // [S][tiles]
    int64_t *ser_len;            // [S]
    int64_t *series_off;         // [S + 1]
    int32_t *frame, *person, *slot;   // [K * n_valid]
    double *confidence;          // [K * n_valid]
    int32_t *series_frame;       // [n_valid]
    double *series_conf;         // [K][n_valid]
    int64_t n_valid, S;
    int32_t C, K, tiles;
};

namespace {

constexpr int TILE = CAM_TILE;           // files of a tile, lanes of its workgroup

// Valid persons of file gf (an index among the files of all cameras).
TL_HD int64_t tl_file_valid(const P2sTlArgs &a, int64_t gf) {
    int64_t n = 0;
    for (int64_t i = a.person_base[gf]; i < a.person_base[gf + 1]; ++i) n += a.valid[i];
    return n;
}

// The K rows of the valid person i, entry p of the list of its camera's file f, from `row` on.
TL_HD void tl_write_person(const P2sTlArgs &a, int64_t i, int64_t f, int64_t p, int64_t row) {
    const double *cf = a.conf + i * a.K;
    for (int k = 0; k < a.K; ++k) {                               // row + k < row_off[C] = K * n_valid: the counts are the scan's
        a.frame[row + k] = (int32_t)f;
        a.person[row + k] = (int32_t)p;
        a.slot[row + k] = k;
        a.confidence[row + k] = cf[k];
    }
}

// Entry p of file gf: the person's index when the file lists it and it is valid, else -1.
TL_HD int64_t tl_series_person(const P2sTlArgs &a, int64_t gf, int64_t p) {
    const int64_t b = a.person_base[gf];
    return p < a.person_base[gf + 1] - b && a.valid[b + p] ? b + p : -1;
}

TL_HD void tl_write_series(const P2sTlArgs &a, int64_t i, int64_t f, int64_t pos) {      // pos < series_off[S] = n_valid
    a.series_frame[pos] = (int32_t)f;
    for (int k = 0; k < a.K; ++k) a.series_conf[k * a.n_valid + pos] = a.conf[i * a.K + k];
}

// ---- rows ------------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(TILE) tl_count_kernel(const P2sTlArgs a) {
    __shared__ int64_t part[TILE / 64];
    const int c = blockIdx.y, tid = threadIdx.x;
    const int64_t f_base = a.file_off[c], F = a.file_off[c + 1] - f_base;
    const int64_t t0 = (int64_t)blockIdx.x * TILE;
    if (t0 >= F) return;                                          // uniform over the workgroup
    const int64_t f = t0 + tid;
    int64_t total;
    (void)block_scan_exclusive<OpSum>(f < F ? a.K * tl_file_valid(a, f_base + f) : 0, part, &total);
    if (tid == 0) a.tv_rows[(int64_t)c * a.tiles + blockIdx.x] = total;
}

__global__ void __launch_bounds__(TILE) tl_rows_kernel(const P2sTlArgs a) {
    __shared__ int64_t part[TILE / 64];
    __shared__ int64_t pb[TILE + 1], first_row[TILE];
    const int c = blockIdx.y, tid = threadIdx.x;
    const int64_t f_base = a.file_off[c], F = a.file_off[c + 1] - f_base;
    const int64_t t0 = (int64_t)blockIdx.x * TILE;
    if (t0 >= F) return;                                          // uniform over the workgroup
    const int nf = (int)(F - t0 < TILE ? F - t0 : TILE);
    const int64_t gf = f_base + t0 + tid;
    if (tid < nf) pb[tid] = a.person_base[gf];
    if (tid == 0) pb[nf] = a.person_base[f_base + t0 + nf];
    const int64_t before = block_scan_exclusive<OpSum>(tid < nf ? a.K * tl_file_valid(a, gf) : 0, part, nullptr);
    first_row[tid] = a.row_off[c] + a.tb_rows[(int64_t)c * a.tiles + blockIdx.x] + before;
    __syncthreads();
    for (int64_t i = pb[0] + tid; i < pb[nf]; i += TILE) {        // the tile's persons stand back to back
        if (!a.valid[i]) continue;
        int lo = 0, hi = nf;                                      // pb[lo] <= i < pb[hi]
        while (hi - lo > 1) {
            const int mid = (lo + hi) >> 1;
            if (pb[mid] <= i) lo = mid; else hi = mid;
        }
        int64_t rank = 0;
        for (int64_t j = pb[lo]; j < i; ++j) rank += a.valid[j];
        tl_write_person(a, i, t0 + lo, i - pb[lo], first_row[lo] + rank * a.K);
    }
}

// ---- series ----------------------------------------------------------------------------------------------------------------
// Workgroup q * tiles + t takes tile t of series q: person index q - people_off[c] of camera c = series_cam[q].
template <bool WRITE> __global__ void __launch_bounds__(TILE) tl_series_kernel(const P2sTlArgs a) {
    __shared__ int64_t part[TILE / 64];
    const int64_t q = blockIdx.x / (unsigned)a.tiles, t = blockIdx.x % (unsigned)a.tiles;
    const int c = a.series_cam[q], tid = threadIdx.x;
    const int64_t p = q - a.people_off[c];
    const int64_t f_base = a.file_off[c], F = a.file_off[c + 1] - f_base;
    const int64_t t0 = t * TILE;
    if (t0 >= F) return;                                          // uniform over the workgroup
    const int64_t f = t0 + tid;
    const int64_t i = f < F ? tl_series_person(a, f_base + f, p) : -1;
    int64_t total;
    const int64_t before = block_scan_exclusive<OpSum>(i >= 0, part, &total);
    if (!WRITE) {
        if (tid == 0) a.tv_ser[q * a.tiles + t] = total;
    } else if (i >= 0) {
        tl_write_series(a, i, f, a.series_off[q] + a.tb_ser[q * a.tiles + t] + before);
    }
}

// A scan of n values into their n + 1 offsets: the values as the tiles of one camera of n * CAM_TILE frames (`span`,
// {0, n * CAM_TILE} on the device), the total as that camera's.
void launch_offsets(const int64_t *span, int64_t *values, int64_t *offsets, int64_t n, hipStream_t s) {
    const CamScanArgs sc{span, nullptr, values, offsets, nullptr, nullptr, offsets + n, 1, (int32_t)n};
    hipLaunchKernelGGL(cam_tile_scan_kernel<OpSum>, dim3(1), dim3(1024), 0, s, sc);
}

hipError_t launch_timeline(const P2sTlArgs &a, const int64_t *span_cams, const int64_t *span_series, hipStream_t s) {
    const dim3 grid((unsigned)a.tiles, (unsigned)a.C);
    hipLaunchKernelGGL(tl_count_kernel, grid, dim3(TILE), 0, s, a);
    const CamScanArgs rows{a.file_off, nullptr, a.tv_rows, a.tb_rows, nullptr, nullptr, a.cam_rows, a.C, a.tiles};
    hipLaunchKernelGGL(cam_tile_scan_kernel<OpSum>, dim3((unsigned)a.C), dim3(1024), 0, s, rows);
    launch_offsets(span_cams, a.cam_rows, a.row_off, a.C, s);
    hipLaunchKernelGGL(tl_rows_kernel, grid, dim3(TILE), 0, s, a);
    const dim3 sgrid((unsigned)(a.S * a.tiles));
    if (a.S > 0) {
        hipLaunchKernelGGL(tl_series_kernel<false>, sgrid, dim3(TILE), 0, s, a);
        const CamScanArgs ser{a.series_files, nullptr, a.tv_ser, a.tb_ser, nullptr, nullptr, a.ser_len, (int32_t)a.S, a.tiles};
        hipLaunchKernelGGL(cam_tile_scan_kernel<OpSum>, dim3((unsigned)a.S), dim3(1024), 0, s, ser);
    }
    launch_offsets(span_series, a.ser_len, a.series_off, a.S, s);
    if (a.S > 0) hipLaunchKernelGGL(tl_series_kernel<true>, sgrid, dim3(TILE), 0, s, a);
    return hipGetLastError();
}

// ---- the same passes on the host -------------------------------------------------------------------------------------------
void host_timeline(const P2sTlArgs &a) {
    int64_t row = 0, pos = 0, q = 0;
    for (int c = 0; c < a.C; ++c) {
        a.row_off[c] = row;
        for (int64_t gf = a.file_off[c]; gf < a.file_off[c + 1]; ++gf)
            for (int64_t b = a.person_base[gf], i = b; i < a.person_base[gf + 1]; ++i)
                if (a.valid[i]) {
                    tl_write_person(a, i, gf - a.file_off[c], i - b, row);
                    row += a.K;
                }
    }
    a.row_off[a.C] = row;
    for (int c = 0; c < a.C; ++c)
        for (int64_t p = 0; p < a.people_off[c + 1] - a.people_off[c]; ++p, ++q) {
            a.series_off[q] = pos;
            for (int64_t gf = a.file_off[c]; gf < a.file_off[c + 1]; ++gf) {
                const int64_t i = tl_series_person(a, gf, p);
                if (i >= 0) tl_write_series(a, i, gf - a.file_off[c], pos++);
            }
        }
    a.series_off[a.S] = pos;
}

}  // namespace

// ---- C-ABI entry points (include/p2s.h) ----------------------------------------------------------------------------
extern "C" {

int p2s_timeline_rows_host(p2s_ctx *ctx, int32_t n_cams, const int64_t *file_off, const int64_t *person_base, const uint8_t *valid,
                           int32_t n_kpts, const double *conf, int64_t n_rows, int64_t n_series, int64_t *row_off, int32_t *frame,
                           int32_t *person, int32_t *slot, double *confidence, int64_t *n_people, int64_t *series_off,
                           int32_t *series_frame, double *series_conf) {
    P2S_TRY(p2s_check_n_cams(n_cams));
    if (n_kpts < 1 || n_kpts > P2S_TL_MAX_K) return p2s_set_error(P2S_ERR_INVALID_ARG, "n_kpts=%d outside [1, %d]", n_kpts, P2S_TL_MAX_K);
    if (!file_off || !person_base || !row_off || !n_people || !series_off) return p2s_set_error(P2S_ERR_INVALID_ARG, "null argument");
    if (file_off[0] != 0) return p2s_set_error(P2S_ERR_INVALID_ARG, "file_off must start at 0");
    const size_t C = (size_t)n_cams, K = (size_t)n_kpts;
    std::vector<int64_t> n_files(C), foff(C + 1), people_off(C + 1, 0);
    for (size_t c = 0; c < C; ++c) n_files[c] = file_off[c + 1] - file_off[c];     // a negative one is refused by build()
    P2sFrames fr;
    int64_t N;
    P2S_TRY(fr.build(n_cams, n_files.data(), 0, ((int64_t)1 << 31) - 2, foff.data()));
    P2S_TRY(fr.persons(person_base, valid, N));
    if (N > 0 && !conf) return p2s_set_error(P2S_ERR_INVALID_ARG, "null argument");
    // what the outputs' sizes and the series' grid depend on: the valid persons, the longest list of every camera
    int64_t n_valid = 0;
    for (int64_t i = 0; i < N; ++i) n_valid += valid[i] != 0;
    for (size_t c = 0; c < C; ++c) {
        int64_t most = 0;
        for (int64_t f = foff[c]; f < foff[c + 1]; ++f) most = std::max(most, person_base[f + 1] - person_base[f]);
        people_off[c + 1] = people_off[c] + most;
    }
    const int64_t S = people_off[C], tiles = std::max<int64_t>((fr.max_frames + TILE - 1) / TILE, 1);
    if (n_rows != (int64_t)K * n_valid || n_series != S)
        return p2s_set_error(P2S_ERR_INVALID_ARG, "n_rows=%lld, n_series=%lld; the input holds %lld rows and %lld series", (long long)n_rows,
                             (long long)n_series, (long long)((int64_t)K * n_valid), (long long)S);
    if (n_valid > 0 && (!frame || !person || !slot || !confidence || !series_frame || !series_conf))
        return p2s_set_error(P2S_ERR_INVALID_ARG, "null argument");
    if (S * tiles >= ((int64_t)1 << 31)) return p2s_set_error(P2S_ERR_INVALID_ARG, "%lld series of %lld tiles are too many", (long long)S, (long long)tiles);
    for (size_t c = 0; c < C; ++c) n_people[c] = people_off[c + 1] - people_off[c];
    std::vector<int64_t> series_files((size_t)S + 1, 0);
    std::vector<int32_t> series_cam((size_t)S);
    for (size_t c = 0; c < C; ++c)
        for (int64_t q = people_off[c]; q < people_off[c + 1]; ++q) {
            series_cam[(size_t)q] = (int32_t)c;
            series_files[(size_t)q + 1] = series_files[(size_t)q] + n_files[c];
        }
    P2sTlArgs a{};
    a.n_valid = n_valid; a.S = S; a.C = n_cams; a.K = n_kpts; a.tiles = (int32_t)tiles;
    if (!ctx) {                                                   // the same functions on the host
        a.file_off = foff.data(); a.person_base = person_base; a.valid = valid; a.conf = conf; a.people_off = people_off.data();
        a.row_off = row_off; a.frame = frame; a.person = person; a.slot = slot; a.confidence = confidence;
        a.series_off = series_off; a.series_frame = series_frame; a.series_conf = series_conf;
        host_timeline(a);
        return P2S_OK;
    }
    const size_t n_tiles = C * (size_t)tiles, s_tiles = (size_t)S * (size_t)tiles, nv = (size_t)n_valid, nf = (size_t)fr.frames;
    const int64_t spans[4] = {0, (int64_t)C * CAM_TILE, 0, S * CAM_TILE};
    Layout lw, li, ld;                                            // 8-byte words; int32; the doubles that go down
    const size_t o_foff = lw.add((C + 1) * 8), o_pb = lw.add((nf + 1) * 8), o_sf = lw.add(((size_t)S + 1) * 8), o_po = lw.add((C + 1) * 8),
                 o_span = lw.add(sizeof spans), o_scam = lw.add((size_t)S * 4);
    const size_t o_tvr = lw.add(n_tiles * 8), o_tbr = lw.add(n_tiles * 8), o_cr = lw.add(C * 8), o_roff = lw.add((C + 1) * 8),
                 o_tvs = lw.add(s_tiles * 8), o_tbs = lw.add(s_tiles * 8), o_sl = lw.add((size_t)S * 8), o_soff = lw.add(((size_t)S + 1) * 8);
    const size_t o_frame = li.add(K * nv * 4), o_person = li.add(K * nv * 4), o_slot = li.add(K * nv * 4), o_sfr = li.add(nv * 4);
    const size_t o_conf = ld.add(K * nv * 8), o_sconf = ld.add(K * nv * 8);
    HIP_TRY(hipSetDevice(ctx->device));
    Stage st{ctx};
    char *w, *ints, *dbl;
    P2S_TRY(st.upload(a.valid, valid, (size_t)N));
    P2S_TRY(st.upload(a.conf, conf, (size_t)N * K * 8));
    P2S_TRY(st.alloc(w, lw.bytes));
    P2S_TRY(st.up(w + o_foff, foff.data(), (C + 1) * 8));
    P2S_TRY(st.up(w + o_pb, person_base, (nf + 1) * 8));
    P2S_TRY(st.up(w + o_sf, series_files.data(), ((size_t)S + 1) * 8));
    P2S_TRY(st.up(w + o_po, people_off.data(), (C + 1) * 8));
    P2S_TRY(st.up(w + o_span, spans, sizeof spans));
    P2S_TRY(st.up(w + o_scam, series_cam.data(), (size_t)S * 4));
    P2S_TRY(st.alloc(ints, li.bytes));
    P2S_TRY(st.alloc(dbl, ld.bytes));
    a.file_off = (const int64_t *)(w + o_foff); a.person_base = (const int64_t *)(w + o_pb); a.series_files = (const int64_t *)(w + o_sf);
    a.people_off = (const int64_t *)(w + o_po); a.series_cam = (const int32_t *)(w + o_scam);
    a.tv_rows = (int64_t *)(w + o_tvr); a.tb_rows = (int64_t *)(w + o_tbr); a.cam_rows = (int64_t *)(w + o_cr); a.row_off = (int64_t *)(w + o_roff);
    a.tv_ser = (int64_t *)(w + o_tvs); a.tb_ser = (int64_t *)(w + o_tbs); a.ser_len = (int64_t *)(w + o_sl); a.series_off = (int64_t *)(w + o_soff);
    a.frame = (int32_t *)(ints + o_frame); a.person = (int32_t *)(ints + o_person); a.slot = (int32_t *)(ints + o_slot);
    a.series_frame = (int32_t *)(ints + o_sfr);
    a.confidence = (double *)(dbl + o_conf); a.series_conf = (double *)(dbl + o_sconf);
    const int64_t *span = (const int64_t *)(w + o_span);
    P2S_TRY(st.time_begin());
    HIP_TRY(launch_timeline(a, span, span + 2, ctx->stream));
    P2S_TRY(st.time_end());
    P2S_TRY(st.down(row_off, a.row_off, (C + 1) * 8));
    P2S_TRY(st.down(frame, a.frame, K * nv * 4));
    P2S_TRY(st.down(person, a.person, K * nv * 4));
    P2S_TRY(st.down(slot, a.slot, K * nv * 4));
    P2S_TRY(st.down(confidence, a.confidence, K * nv * 8));
    P2S_TRY(st.down(series_off, a.series_off, ((size_t)S + 1) * 8));
    P2S_TRY(st.down(series_frame, a.series_frame, nv * 4));
    P2S_TRY(st.down(series_conf, a.series_conf, K * nv * 8));
    return st.finish(P2S_TIMED_TIMELINE);                         // the offsets and tables are host memory: alive until here
}

int p2s_timeline_kernel_ms(p2s_ctx *ctx, float *elapsed_ms) { return p2s_kernel_ms_query(ctx, P2S_TIMED_TIMELINE, "p2s_timeline_rows_host", elapsed_ms); }

}  // extern "C"
