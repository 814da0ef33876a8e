// p2s_passes.h -- ordered sums over the points of a call, on the device or on the host: what the stages that iterate
// (p2s_refine.hip, p2s_relpose.hip) share.  A pass has `rows` rows (blockIdx.y: a camera, a camera pair) and a.parts
// workgroups along the points (blockIdx.x); a lane adds W values over its points in order, a wave its lanes by the xor
// butterfly, a workgroup its waves in order.  That leaves partials [row][W][parts], which the caller adds up: in order
// on the host (p2s_sum_parts), or with rf_sum_kernel.  No floating-point atomic: two runs agree bit for bit.
//
// A pass is a type F with  static bool skip(const A &a, int row)              a row that is left out (P2sPassAll: none)
//                          static void point(const A &a, int row, int64_t n, double *acc)     acc [W] += point n's terms
// over an args struct A with N, tiles, parts and partials.  p2s_pass runs it as p2s_pass_kernel or, ctx == NULL, as
// p2s_pass_host: the same F, the points of a part in the kernel's order.
#ifndef P2S_PASSES_H
#define P2S_PASSES_H

#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>

#include "p2s_ctx.h"

namespace {

// The workgroup's (T lanes) sum of W values a lane: lanes by the butterfly, waves in order; out[i * stride] for value i.
template <int W, int T> __device__ void p2s_block_sum(double (&acc)[W], double *lds, double *out, int64_t stride) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
#pragma unroll
    for (int i = 0; i < W; ++i) {
        double v = acc[i];
        for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m, 64);
        if (lane == 0) lds[wave * W + i] = v;
    }
    __syncthreads();
    if (tid < W) {
        double s = 0.0;
        for (int w = 0; w < T / 64; ++w) s += lds[w * W + tid];
        out[tid * stride] = s;
    }
}

struct P2sPassAll {
    template <typename A> __host__ __device__ static bool skip(const A &, int) { return false; }
};

template <int W, int T, typename F, typename A> __global__ void __launch_bounds__(T) p2s_pass_kernel(const A a) {
    __shared__ double lds[(T / 64) * W];
    const int row = blockIdx.y;
    if (F::skip(a, row)) return;                                     // uniform over the workgroup
    double acc[W];
#pragma unroll
    for (int i = 0; i < W; ++i) acc[i] = 0.0;
    for (int64_t t = blockIdx.x; t < a.tiles; t += a.parts) {        // uniform trip count
        const int64_t n = t * T + threadIdx.x;
        if (n < a.N) F::point(a, row, n, acc);
    }
    p2s_block_sum<W, T>(acc, lds, a.partials + (int64_t)row * W * a.parts + blockIdx.x, a.parts);
}

template <int W, int T, typename F, typename A> void p2s_pass_host(const A &a, int rows) {
    for (int row = 0; row < rows; ++row) {
        if (F::skip(a, row)) continue;
        for (int part = 0; part < a.parts; ++part) {
            double acc[W] = {};
            for (int64_t t = part; t < a.tiles; t += a.parts)
                for (int64_t n = t * T; n < std::min<int64_t>(a.N, (t + 1) * T); ++n) F::point(a, row, n, acc);
            for (int i = 0; i < W; ++i) a.partials[((int64_t)row * W + i) * a.parts + part] = acc[i];
        }
    }
}

// The pass F over `rows` rows into a.partials: a launch on ctx's stream, or on the host at once.
template <int W, int T, typename F, typename A> int p2s_pass(p2s_ctx *ctx, const A &a, int rows) {
    if (!ctx) {
        p2s_pass_host<W, T, F>(a, rows);
        return P2S_OK;
    }
    hipLaunchKernelGGL((p2s_pass_kernel<W, T, F, A>), dim3((unsigned)a.parts, (unsigned)rows), dim3(T), 0, ctx->stream, a);
    HIP_TRY(hipGetLastError());
    return P2S_OK;
}

// sums [count] of the host's partials [count][parts]: the parts in order.
inline void p2s_sum_parts(const double *partials, size_t count, int parts, double *sums) {
    for (size_t i = 0; i < count; ++i) {
        double s = 0.0;
        for (int part = 0; part < parts; ++part) s += partials[i * parts + part];
        sums[i] = s;
    }
}

// The same on the device, in another order: one wave a value, lane l adds the partial sums l, l + 64, .. in order, the
// lanes by the butterfly.
__global__ void __launch_bounds__(64) rf_sum_kernel(const double *partials, double *sums, int parts) {
    const double *p = partials + (int64_t)blockIdx.x * parts;
    double v = 0.0;
    for (int i = threadIdx.x; i < parts; i += 64) v += p[i];
    for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m, 64);
    if (threadIdx.x == 0) sums[blockIdx.x] = v;
}

}  // namespace

#endif
