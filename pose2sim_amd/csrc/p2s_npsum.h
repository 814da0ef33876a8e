// p2s_npsum.h -- np.add.reduce of a contiguous run of doubles, bit for bit, by one workgroup of 1024 lanes: what
// p2s_confidence.hip (np.mean, np.std) and p2s_measure.hip (the trimmed means) share.  The summation order is described
// at the head of p2s_confidence.hip.  Floating-point contraction is off for every file that includes this.
#ifndef P2S_NPSUM_H
#define P2S_NPSUM_H

#include <hip/hip_runtime.h>
#include <stdint.h>

#pragma clang fp contract(off)

namespace {

constexpr int CT = 1024, CW = CT / 64;   // lanes and waves of the per-column workgroups
constexpr int CHUNK = 8192;              // NumPy's ufunc buffer
constexpr int LEAF = 128;                // pairwise summation's block
constexpr int DEPTH = 7;                 // levels below the root of a chunk's tree: 2^7 slots of 8 lanes = CT

// ---- np.add.reduce ---------------------------------------------------------------------------------------------------
struct CfShared {
    double part[2][CW];
    int part_on[2][CW];
    double total;
};

template <bool SQ> __device__ __forceinline__ double cf_term(double v, double mean) {
    if (!SQ) return v;
    const double d = v - mean;
    return d * d;
}

// One level of the tree: the node on this lane takes the node `dist` lanes up when that one exists.  Called by whole
// waves; what the lanes of a right-hand node compute is never read again.
__device__ __forceinline__ void cf_level(double &r, int on, int lane, int dist) {
    const double other = __shfl_xor(r, dist);
    const int other_on = __shfl_xor(on, dist);
    if (!(lane & dist) && other_on) r = r + other;
}

// np.add.reduce over f(x[0 .. m)), f = identity or the squared deviation from `mean`.  Called by the whole workgroup;
// every lane gets the sum.
template <bool SQ> __device__ double cf_sum(CfShared &s, const double *x, int64_t m, double mean) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int slot = tid >> 3, j = tid & 7;
    double total = 0.0;                                           // wave 0, lane 0 keeps it
    int par = 0;
    for (int64_t c0 = 0; c0 < m; c0 += CHUNK, par ^= 1) {
        // this slot's leaf: walk the path
        int nn = (int)(m - c0 < CHUNK ? m - c0 : CHUNK), at = 0, on = 1;
        for (int d = 0; d < DEPTH; ++d) {
            if (nn <= LEAF) { on = (slot & ((1 << (DEPTH - d)) - 1)) == 0; break; }
            int n2 = nn / 2;
            n2 -= n2 % 8;
            if ((slot >> (DEPTH - 1 - d)) & 1) { at += n2; nn -= n2; }
            else nn = n2;
        }
        // nn <= 128 here: a run of 8192 or fewer halves to 64 + 15 at most in seven steps
        const double *p = x + c0 + at;                            // at + nn <= the chunk's length: inside the column
        const int whole = nn - nn % 8;
        double r = 0.0;
        if (on) {
            if (nn < 8) {
                for (int i = 0; i < nn; ++i) r = r + cf_term<SQ>(p[i], mean);
            } else {
                r = cf_term<SQ>(p[j], mean);
                for (int i = 8; i < whole; i += 8) r = r + cf_term<SQ>(p[i + j], mean);
            }
        }
        double b = r;                                             // ((r0+r1)+(r2+r3))+((r4+r5)+(r6+r7)) on every lane of the slot
        b = b + __shfl_xor(b, 1);
        b = b + __shfl_xor(b, 2);
        b = b + __shfl_xor(b, 4);
        if (on && nn >= 8) {
            r = b;
            for (int i = whole; i < nn; ++i) r = r + cf_term<SQ>(p[i], mean);
        }
        cf_level(r, on, lane, 8);
        cf_level(r, on, lane, 16);
        cf_level(r, on, lane, 32);
        if (lane == 0) { s.part[par][wave] = r; s.part_on[par][wave] = on; }
        __syncthreads();                                          // the other half of part is free: wave 0 has passed this
        if (wave == 0) {                                          // barrier since it last read it
            double v = lane < CW ? s.part[par][lane] : 0.0;
            const int v_on = lane < CW ? s.part_on[par][lane] : 0;
            cf_level(v, v_on, lane, 1);
            cf_level(v, v_on, lane, 2);
            cf_level(v, v_on, lane, 4);
            cf_level(v, v_on, lane, 8);
            total = total + v;                                    // the chunks' sums one after the other
        }
    }
    if (tid == 0) s.total = total;
    __syncthreads();
    total = s.total;
    __syncthreads();                                              // s.total and part may be written again
    return total;
}

}  // namespace

#endif
