// p2s_iir.h -- the IIR recurrence shared by the zero-phase filters of p2s_filter.hip (Butterworth on .trc columns) and
// p2s_sync.hip (Butterworth on the synchronization speeds).
#ifndef P2S_IIR_H
#define P2S_IIR_H

#include <hip/hip_runtime.h>

#define P2S_MAX_FILTER_ORDER 8

// One sample of scipy's lfilter (direct form II transposed, a[0] = 1): y = z[0] + b[0] x, then
// z[k] = z[k+1] + b[k+1] x - a[k+1] y.  Same operation order as scipy's C loop and no contraction, so that the result
// matches scipy.signal.filtfilt to rounding.  b, a: N + 1 coefficients.
template <int N>
__device__ __forceinline__ double iir_step(const double *b, const double *a, double (&z)[N], double x) {
#pragma clang fp contract(off)
    const double y = z[0] + b[0] * x;
#pragma unroll
    for (int k = 0; k < N - 1; ++k) z[k] = (z[k + 1] + x * b[k + 1]) - y * a[k + 1];
    z[N - 1] = x * b[N] - y * a[N];
    return y;
}

#endif
