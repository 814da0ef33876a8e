// p2s_scan.h -- scans of one int64 a lane over a wave and over a workgroup, with the running maximum and the running sum
// as operators, and on top of them the two kernels that scan along the frames of every camera (the tiles' values, then
// "the last earlier frame that holds something"): what p2s_idswitch.hip and p2s_extract.hip share.
#ifndef P2S_SCAN_H
#define P2S_SCAN_H

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace {

struct OpMax {
    static __device__ __forceinline__ int64_t identity() { return -1; }
    static __device__ __forceinline__ int64_t apply(int64_t a, int64_t b) { return a > b ? a : b; }
};
struct OpSum {
    static __device__ __forceinline__ int64_t identity() { return 0; }
    static __device__ __forceinline__ int64_t apply(int64_t a, int64_t b) { return a + b; }
};

// Inclusive scan over the lanes of a wave.
template <typename Op> __device__ __forceinline__ int64_t wave_scan(int64_t v, int lane) {
    for (int s = 1; s < 64; s <<= 1) {
        const int64_t up = __shfl_up(v, s);
        if (lane >= s) v = Op::apply(v, up);
    }
    return v;
}

// Exclusive scan over the workgroup's lanes (whole waves, at most 16 of them); *total gets the value over all lanes.
// `part` is LDS for one value a wave; called by every lane, two barriers.
template <typename Op> __device__ int64_t block_scan_exclusive(int64_t mine, int64_t *part, int64_t *total) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, n_waves = (int)(blockDim.x >> 6);
    const int64_t incl = wave_scan<Op>(mine, lane);
    int64_t before = __shfl_up(incl, 1);
    if (lane == 0) before = Op::identity();
    __syncthreads();                                              // part of an earlier call has been read
    if (lane == 63) part[wave] = incl;
    __syncthreads();
    int64_t all = Op::identity();
    for (int w = 0; w < n_waves; ++w) {
        if (w < wave) before = Op::apply(part[w], before);
        all = Op::apply(all, part[w]);
    }
    if (total) *total = all;
    return before;
}

// ---- the scan along the frames of every camera ---------------------------------------------------------------------------
// The frames of camera c are frame_off[c] .. frame_off[c + 1], in tiles of CAM_TILE frames, one workgroup a tile.  The
// stage's own first pass leaves one value a tile in tile_value; cam_tile_scan_kernel scans them per camera into
// tile_before, and a per-frame pass picks its tile's entry up from there.
constexpr int CAM_TILE = 256;

struct CamScanArgs {
    const int64_t *frame_off;    // [C + 1]
    const int32_t *count;        // [frames] cam_prev_kernel: a frame with count > 0 is one to be found
    int64_t *tile_value;         // [C][tiles]
    int64_t *tile_before;        // [C][tiles] the exclusive scan of tile_value along the camera
    int32_t *prev;               // [frames] the last earlier frame of the camera with count > 0, -1 without one
    int32_t *zero_run;           // [frames] the frames between the two, f - 1 - prev[f]; may be NULL
    int64_t *totals;             // [C] the scan's value over all tiles of the camera; may be NULL
    int32_t C, tiles;
};

template <typename Op> __global__ void __launch_bounds__(1024) cam_tile_scan_kernel(const CamScanArgs a) {
    __shared__ int64_t part[16];
    const int c = blockIdx.x, tid = threadIdx.x;
    const int64_t F = a.frame_off[c + 1] - a.frame_off[c];
    const int64_t nt = (F + CAM_TILE - 1) / CAM_TILE;             // <= a.tiles
    const int64_t *in = a.tile_value + (int64_t)c * a.tiles;
    int64_t *out = a.tile_before + (int64_t)c * a.tiles;
    int64_t carry = Op::identity();
    for (int64_t base = 0; base < nt; base += 1024) {             // uniform trip count
        const int64_t i = base + tid;
        int64_t total;
        const int64_t before = block_scan_exclusive<Op>(i < nt ? in[i] : Op::identity(), part, &total);
        if (i < nt) out[i] = Op::apply(carry, before);
        carry = Op::apply(carry, total);
    }
    if (tid == 0 && a.totals) a.totals[c] = carry;
}

// With tile_before the running maximum (OpMax) of the tiles' last frame with count > 0.
__global__ void __launch_bounds__(CAM_TILE) cam_prev_kernel(const CamScanArgs a) {
    __shared__ int64_t part[CAM_TILE / 64];
    const int c = blockIdx.y, tid = threadIdx.x;
    const int64_t f_base = a.frame_off[c], F = a.frame_off[c + 1] - f_base;
    const int64_t t0 = (int64_t)blockIdx.x * CAM_TILE;
    if (t0 >= F) return;                                          // uniform over the workgroup
    const int64_t f = t0 + tid;
    const int64_t key = f < F && a.count[f_base + f] > 0 ? f : -1;
    int64_t before = block_scan_exclusive<OpMax>(key, part, nullptr);
    before = OpMax::apply(before, a.tile_before[(int64_t)c * a.tiles + blockIdx.x]);
    if (f < F) {
        a.prev[f_base + f] = (int32_t)before;
        if (a.zero_run) a.zero_run[f_base + f] = (int32_t)(f - 1 - before);
    }
}

}  // namespace

#endif
