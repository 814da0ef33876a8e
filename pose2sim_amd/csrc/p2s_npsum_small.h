// p2s_npsum_small.h -- np.add.reduce over fewer than 128 contiguous float64 entries (NumPy's pairwise_sum below its
// block of 128), bit for bit, for the host and for one lane of a kernel: what the tracked-person selection of
// p2s_ingest.cpp, the match cost of p2s_idswitch.hip and the transition maps of p2s_extract.hip share.  The order: a plain
// loop from 0.0 below 8 entries; else eight running sums r[j] = a[j], r[j] += a[i + j] over the whole blocks of eight,
// ((r0+r1)+(r2+r3))+((r4+r5)+(r6+r7)), then the tail one by one.  STRIDE is the distance between two entries: 1 for a
// plain array, 64 for a lane's column of an LDS table [n][64].
#ifndef P2S_NPSUM_SMALL_H
#define P2S_NPSUM_SMALL_H

#if defined(__HIP__)
#define P2S_NPSUM_HD __host__ __device__ inline __attribute__((always_inline))
#else
#define P2S_NPSUM_HD inline
#endif

template <int STRIDE> P2S_NPSUM_HD double p2s_np_sum_below_128(const double *a, int n) {
    if (n < 8) {
        double r = 0.0;
        for (int i = 0; i < n; ++i) r = r + a[i * STRIDE];
        return r;
    }
    double r[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) r[j] = a[j * STRIDE];
    const int whole = n - n % 8;
    for (int i = 8; i < whole; i += 8) {
#pragma unroll
        for (int j = 0; j < 8; ++j) r[j] = r[j] + a[(i + j) * STRIDE];
    }
    double res = ((r[0] + r[1]) + (r[2] + r[3])) + ((r[4] + r[5]) + (r[6] + r[7]));
    for (int i = whole; i < n; ++i) res = res + a[i * STRIDE];
    return res;
}

#endif
