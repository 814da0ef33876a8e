// p2s_scan.h -- scans of one int64 a lane over a wave and over a workgroup, with the running maximum and the running sum
// as operators: what the per-frame passes of p2s_idswitch.hip and p2s_extract.hip share.
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

}  // namespace

#endif
