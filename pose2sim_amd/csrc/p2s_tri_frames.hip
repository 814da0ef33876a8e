// p2s_tri_frames.hip -- robust triangulation with PER-FRAME cameras (moving and / or zooming rigs) for gfx950: the
// per-unit contract of p2s_tri_fused.hip (triangulation_from_best_cameras, triangulation.py:363-604, pinhole branch, no
// L/R swap, 2..16 cameras), except that unit (block b, keypoint k) uses the projection matrices of calibration frame
// block_frame[b] out of a device table P[Fc][C][12].
//
// One calibration frame per wave.  The host cuts the blocks into runs of equal frame (block_frame must not decrease, so
// a frame's blocks are consecutive) and every run into waves of up to 64 units; a wave reads {first unit, units, frame}
// from the plan, and `P + frame * C * 12` is wave-uniform: the matrices stay scalar loads through the constant address
// space and SGPR operands of the fp64 FMAs, exactly as the static kernels' helpers expect them.  The price is the lane
// fill, units of a frame / 64 rounded up: 26 of 64 lanes (41 %) at one person x 26 keypoints, 133 of 192 (69 %) at 133
// (DESIGN.md section 4.24 has the figures of the alternative, tiles of 64 units across frames with per-lane matrices).
//
// Level 0 and the camera-subset search run in the same wave and launch, as in p2s_tri_fused.hip: the units whose
// level-0 error exceeds the threshold are parked in LDS slots (one per lane, so a wave never runs out of them) and the
// wave walks their levels in lock step, groups of G lanes per pending unit, subsets in itertools.combinations order out
// of a table, np.nanargmin's order through better_candidate, the break at the first level under the threshold.  No fp32
// screen: every candidate is solved and measured in fp64 by accum_camera, smallest_eigvec and camera_distance of
// p2s_tri_dev.h.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <math.h>

#include <algorithm>
#include <vector>

#include "p2s_ctx.h"
#include "p2s_tri_dev.h"
#include "p2s_tri_frames.h"

namespace {

// One wave's share of a call: `count` (1..64) consecutive units from `unit0` (index within the chunk), all of
// calibration frame `frame`.
struct P2sFrameWave {
    uint32_t unit0, count, frame, pad;
};

struct P2sFramesArgs {
    const void *xyl;             // whole tensor [n_blocks][C][K][3]
    const double *P;             // [Fc][C][12]
    const P2sFrameWave *waves;   // this chunk's waves, one per workgroup
    double *Q;
    float *err;
    uint8_t *n_excl;
    uint32_t *mask;
    unsigned long long *stats;
    const uint16_t *sub_tab;     // camera subsets by level (p2s_subset_table)
    const uint32_t *sub_off;
    int64_t block0;              // first block of this chunk
    int32_t K, C, min_cams;
    double thr, lik_thr;
};

// One frame's matrices, [C][12]: wave-uniform, read through the constant address space.
typedef const __attribute__((address_space(4))) double *pmat_cptr;

// camera_distance and camera_distance_exact read nothing of a P2sCam but P, its first member.
__device__ __forceinline__ cam_cptr as_cam(pmat_cptr Pw, int c) { return (cam_cptr)(Pw + 12 * c); }

template <typename T, int CT>
struct alignas(16) FSlot {
    double N[10];
    double err;
    double q[3];
    uint32_t nan, zero, S, owner;          // owner = lane that streamed the unit
    T o[CT * 3];                           // x, y, likelihood per camera
};

template <typename T, int CT>
__device__ __forceinline__ void frames_load_obs(const P2sFramesArgs &a, int C, uint32_t b, uint32_t k, RegObs<T, CT> &obs) {
    const unsigned char *chunk = reinterpret_cast<const unsigned char *>(a.xyl) +
                                 (size_t)a.block0 * (size_t)C * (size_t)a.K * 3u * sizeof(T);
    const uint32_t voff = (b * (uint32_t)(C * a.K) + k) * (uint32_t)(3 * sizeof(T));   // < 2^31: chunked on the host
    const uint32_t cam_stride = (uint32_t)a.K * (uint32_t)(3 * sizeof(T));
#pragma unroll
    for (int c = 0; c < CT; ++c) {
        if (c < C) {
            const T *p = reinterpret_cast<const T *>(chunk + (size_t)c * cam_stride + voff);
            obs.x[c] = __builtin_nontemporal_load(p);
            obs.y[c] = __builtin_nontemporal_load(p + 1);
            obs.w[c] = __builtin_nontemporal_load(p + 2);
        } else {
            obs.x[c] = obs.y[c] = obs.w[c] = (T)0;
        }
    }
}

// classify_and_accumulate of p2s_tri_dev.h on a frame's matrices.
template <typename T, int CT, typename OBS>
__device__ __forceinline__ void frames_classify_and_accumulate(pmat_cptr Pw, int C, const OBS &o, double N[10],
                                                                uint32_t &nanmask, uint32_t &zeromask) {
    for_each_cam<CT>(C, [&](int c) {
        T x, y, w;
        o.rawT(c, x, y, w);
        const bool isn = !(w == w) || ((double)w < o.lik_thr) || !finite_xy(x, y);
        const bool isz = (w == (T)0) && !isn;
        nanmask |= isn ? (1u << c) : 0u;
        zeromask |= isz ? (1u << c) : 0u;
        const bool ok = !(isn || isz);
        accum_camera<1>(N, Pw + 12 * c, (double)(ok ? x : (T)0), (double)(ok ? y : (T)0), (double)(ok ? w : (T)0));
    });
}

// mean_error of p2s_tri_dev.h (pinhole) on a frame's matrices.
template <int CT, typename OBS>
__device__ __forceinline__ double frames_mean_error(pmat_cptr Pw, int C, const OBS &o, uint32_t kept, const double q[3]) {
    double sum = 0.0;
    bool irregular = false;
    for_each_cam<CT>(C, [&](int c) {
        double x, y, w;
        o.raw(c, x, y, w);
        const bool k = (kept >> c) & 1u;
        bool reg;
        const double d = camera_distance<false>(as_cam(Pw, c), q, x, y, reg);
        irregular = irregular || (k && !reg);
        sum += k ? d : 0.0;
    });
    if (__any(irregular)) {                        // rare: some wanted camera is degenerate / NaN
        double sum2 = 0.0;
        for_each_cam<CT>(C, [&](int c) {
            double x, y, w;
            o.raw(c, x, y, w);
            const double d = camera_distance_exact(as_cam(Pw, c), q[0], q[1], q[2], x, y);
            sum2 += ((kept >> c) & 1u) ? d : 0.0;
        });
        sum = irregular ? sum2 : sum;
    }
    return sum * fast_rcp((double)__popc(kept));   // no camera kept -> NaN, as np.mean([])
}

template <typename T, int CT>
__global__ void __launch_bounds__(64) p2s_tri_frames_kernel(const P2sFramesArgs a) {
    typedef FSlot<T, CT> slot_t;
    __shared__ __align__(16) unsigned char smem[sizeof(slot_t) * 64];
    __shared__ __align__(16) double sP[CT * 12];
    __shared__ uint32_t sList[64];
    // results of the wave's units; the searching units overwrite theirs level by level
    __shared__ double sQ[64 * 3];
    __shared__ uint32_t sE[64];
    __shared__ uint32_t sM[64];
    __shared__ uint8_t sX[64];
    slot_t *slots = reinterpret_cast<slot_t *>(smem);

    const int C = a.C;
    const int K = a.K;
    const int lane = threadIdx.x;
    const P2sFrameWave *wv = a.waves + blockIdx.x;
    const uint32_t unit0 = (uint32_t)__builtin_amdgcn_readfirstlane((int)wv->unit0);
    const uint32_t count = (uint32_t)__builtin_amdgcn_readfirstlane((int)wv->count);
    const uint32_t frame = (uint32_t)__builtin_amdgcn_readfirstlane((int)wv->frame);
    const double *Pg = a.P + (size_t)frame * (size_t)(C * 12);
    pmat_cptr Pw = (pmat_cptr)Pg;
    const bool active = (uint32_t)lane < count;
    const uint32_t u = unit0 + (active ? (uint32_t)lane : 0u);        // a lane beyond the last unit works on the first one
    const double thr = a.thr;
    const uint32_t allmask = (1u << C) - 1u;                         // C <= 16
    const unsigned long long lt = (1ull << lane) - 1ull;
    for (int i = lane; i < C * 12; i += 64) sP[i] = Pg[i];

    // ---- level 0 (triangulation.py:404-505 with nb_cams_off = 0) --------------------------------------------------------
    int n_hard = 0;
    {
        RegObs<T, CT> obs;
        obs.lik_thr = a.lik_thr;
        frames_load_obs<T, CT>(a, C, u / (uint32_t)K, u % (uint32_t)K, obs);
        double N[10];
#pragma unroll
        for (int i = 0; i < 10; ++i) N[i] = 0.0;
        uint32_t nanmask = 0, zeromask = 0;
        frames_classify_and_accumulate<T, CT>(Pw, C, obs, N, nanmask, zeromask);
        const uint32_t dmask = nanmask | zeromask;
        const uint32_t valid = allmask & ~dmask;
        const int V = __popc(dmask);
        const int Lmax = active ? C - a.min_cams - V : -1;              // last level that runs (:408, :437-441)
        double q[3];
        smallest_eigvec(N, q);
        if (C - V < 2) { q[0] = d_nan(); q[1] = d_nan(); q[2] = d_nan(); }   // common.py:347: fewer than 4 rows
        const double e = frames_mean_error<CT>(Pw, C, obs, valid, q);
        const bool ran = Lmax >= 0;                                     // else no level completes (:595-596)
        const bool ok = ran && (e <= thr);                              // :600-602
        sQ[lane * 3 + 0] = ok ? q[0] : d_nan();
        sQ[lane * 3 + 1] = ok ? q[1] : d_nan();
        sQ[lane * 3 + 2] = ok ? q[2] : d_nan();
        sE[lane] = __float_as_uint(ok ? (float)e : __builtin_nanf(""));
        sM[lane] = ran ? nanmask : allmask;
        sX[lane] = (uint8_t)(ran ? V : C);
        const bool need = (Lmax >= 1) && (e > thr);                     // goes on to level 1
        const unsigned long long hard = __ballot(need);
        if (need) {
            slot_t &s = slots[__popcll(hard & lt)];
#pragma unroll
            for (int i = 0; i < 10; ++i) s.N[i] = N[i];
            s.nan = nanmask; s.zero = zeromask; s.owner = (uint32_t)lane;
#pragma unroll
            for (int c = 0; c < CT; ++c) { s.o[3 * c] = obs.x[c]; s.o[3 * c + 1] = obs.y[c]; s.o[3 * c + 2] = obs.w[c]; }
        }
        n_hard = __popcll(hard);
    }

    // ---- camera-subset search over the parked units: lane s looks after slot s ------------------------------------------
    if (n_hard != 0) {
        uint32_t st_evals = 0, st_passes = 0;
        wsync();
        bool cont = lane < n_hard;                                      // this lane's slot goes on to `level`
        const slot_t &mine = slots[cont ? lane : 0];
        const uint32_t m_nan = mine.nan, m_d = mine.nan | mine.zero, m_valid = allmask & ~m_d;
        const int m_V = __popc(m_d), m_Lmax = C - a.min_cams - m_V, m_owner = (int)mine.owner;
        for (int level = 1;; ++level) {
            const unsigned long long pend = __ballot(cont);
            if (pend == 0ull) break;
            const int npend = __popcll(pend);
            if (cont) sList[__popcll(pend & lt)] = (uint32_t)lane;
            wsync();
            const uint32_t sub0 = a.sub_off[level];
            const uint32_t nsub = a.sub_off[level + 1] - sub0;
            int lg = 2;
            {
                uint32_t best_cost = 0xffffffffu;
                for (int l = 2; l <= 6; ++l) {
                    const uint32_t passes = (((uint32_t)npend << l) + 63u) >> 6;
                    const uint32_t rounds = (nsub + (1u << l) - 1u) >> l;
                    const uint32_t cost = passes * rounds;
                    if (cost <= best_cost) { best_cost = cost; lg = l; }
                }
            }
            const int G = 1 << lg, groups = 64 >> lg;
            const int grp = lane >> lg, lig = lane & (G - 1);
            for (int p0 = 0; p0 < npend; p0 += groups) {
                const bool has = p0 + grp < npend;
                const slot_t &s = slots[has ? sList[p0 + grp] : sList[p0]];
                const uint32_t o_d = s.nan | s.zero, o_valid = allmask & ~o_d;
                SlotObs<T> sobs{s.o, a.lik_thr};
                double be = kInf, bq0 = d_nan(), bq1 = d_nan(), bq2 = d_nan();
                uint32_t brank = kNone, bS = 0;
                for (uint32_t r0 = 0; r0 < nsub; r0 += G) {
                    const uint32_t r = r0 + lig;
                    bool go = has && (r < nsub);
                    uint32_t S = 0;
                    if (go) {
                        S = (uint32_t)a.sub_tab[sub0 + r];
                        go = first_padding(S, o_d);                         // quirk Q1 duplicates
                    }
                    if (!__any(go)) continue;
                    st_evals += (uint32_t)__popcll(__ballot(go)); ++st_passes;
                    const uint32_t Rreal = S & o_valid;
                    const uint32_t kept = o_valid & ~Rreal;
                    const int nkept = __popc(kept);
                    double Ns[10];
#pragma unroll
                    for (int i = 0; i < 10; ++i) Ns[i] = s.N[i];
                    for (uint32_t rr = go ? Rreal : 0u; __any(rr != 0u); rr &= rr - 1) {
                        const bool on = rr != 0u;
                        const int c = on ? __builtin_ctz(rr) : 0;
                        const T x = s.o[3 * c], y = s.o[3 * c + 1], w = s.o[3 * c + 2];
                        accum_camera<-1>(Ns, sP + c * 12, (double)(on ? x : (T)0), (double)(on ? y : (T)0),
                                         (double)(on ? w : (T)0));
                    }
                    double q[3];
                    smallest_eigvec(Ns, q);
                    if (nkept < 2) { q[0] = d_nan(); q[1] = d_nan(); q[2] = d_nan(); }
                    // the matrices are scalar loads at their point of use: an opaque copy of the pointer keeps the
                    // compiler from hoisting all of them out of the loops
                    pmat_cptr P_here = Pw;
                    asm volatile("" : "+s"(P_here));
                    const double e = frames_mean_error<CT>(P_here, C, sobs, kept, q);
                    // (a lane meets its candidates in rising rank: a lower error wins, and a number replaces a NaN --
                    // np.nanargmin, triangulation.py:500-503)
                    if (go && (brank == kNone || e < be || (be != be && e == e))) { be = e; bq0 = q[0]; bq1 = q[1]; bq2 = q[2]; brank = r; bS = S; }
                }
                double ge = be;
                uint32_t grank = brank;
                for (int off = G >> 1; off > 0; off >>= 1) {
                    const double oe = __shfl_xor(ge, off, 64);
                    const uint32_t orank = (uint32_t)__shfl_xor((int)grank, off, 64);
                    const bool take = better_candidate(oe, orank, ge, grank);
                    if (take) { ge = oe; grank = orank; }
                }
                grank = (uint32_t)__shfl((int)grank, lane & ~(G - 1), 64);
                if (has && brank != kNone && brank == grank) {
                    slot_t &d = slots[sList[p0 + grp]];
                    d.err = be; d.q[0] = bq0; d.q[1] = bq1; d.q[2] = bq2; d.S = bS;
                }
            }
            wsync();
            if (cont) {
                const slot_t &s = slots[lane];
                const double e = s.err;
                const uint32_t bS = s.S;
                const bool ok = e <= thr;
                cont = (e > thr) && (level + 1 <= m_Lmax);
                sQ[m_owner * 3 + 0] = ok ? s.q[0] : d_nan();
                sQ[m_owner * 3 + 1] = ok ? s.q[1] : d_nan();
                sQ[m_owner * 3 + 2] = ok ? s.q[2] : d_nan();
                sE[m_owner] = __float_as_uint(ok ? (float)e : __builtin_nanf(""));
                sM[m_owner] = m_nan | bS;
                sX[m_owner] = (uint8_t)(m_V + __popc(bS & m_valid));   // :436 counts NaN or zero
            }
            wsync();
        }
        if (a.stats && lane == 0) {
            unsigned long long *st = a.stats + (size_t)(blockIdx.x % P2S_STAT_SHARDS) * P2S_STAT_STRIDE;
            atomicAdd(st + 0, (unsigned long long)n_hard);
            atomicAdd(st + 1, (unsigned long long)st_evals);
            atomicAdd(st + 2, (unsigned long long)st_passes);
        }
    }

    // ---- results (triangulation.py:588-604) --------------------------------------------------------------------------------
    wsync();
    if (active) {
        const int64_t gu = a.block0 * K + (int64_t)u;
        a.Q[gu * 3 + 0] = sQ[lane * 3 + 0];
        a.Q[gu * 3 + 1] = sQ[lane * 3 + 1];
        a.Q[gu * 3 + 2] = sQ[lane * 3 + 2];
        a.err[gu] = __uint_as_float(sE[lane]);
        a.mask[gu] = sM[lane];
        a.n_excl[gu] = sX[lane];
    }
}

template <typename T, int CT>
hipError_t launch_frames(const P2sFramesArgs &a, unsigned grid, hipStream_t s) {
    hipLaunchKernelGGL((p2s_tri_frames_kernel<T, CT>), dim3(grid), dim3(64), 0, s, a);
    return hipGetLastError();
}

hipError_t launch_frames_any(const P2sFramesArgs &a, int dtype, unsigned grid, hipStream_t s) {
    if (dtype == P2S_F32) {
        if (a.C <= 4) return launch_frames<float, 4>(a, grid, s);
        if (a.C <= 8) return launch_frames<float, 8>(a, grid, s);
        return launch_frames<float, 16>(a, grid, s);
    }
    if (a.C <= 4) return launch_frames<double, 4>(a, grid, s);
    if (a.C <= 8) return launch_frames<double, 8>(a, grid, s);
    return launch_frames<double, 16>(a, grid, s);
}

// Everything that can be refused without looking at block_frame; `what` says where the operands live.
int frames_check(p2s_ctx *ctx, int64_t n_cal_frames, int32_t n_cams, const void *P, int64_t n_blocks, int32_t K, int32_t dtype,
                 const void *xyl, const void *block_frame, const p2s_tri_params *p, const void *Q, const void *err,
                 const void *n_excl, const void *mask, const char *what) {
    if (!ctx) return p2s_set_error(P2S_ERR_INVALID_ARG, "null context");
    if (!p) return p2s_set_error(P2S_ERR_INVALID_ARG, "null params");
    if (n_cams < 2 || n_cams > 16)
        return p2s_set_error(P2S_ERR_INVALID_ARG, "n_cams=%d outside [2, 16]: per-frame cameras are triangulated with 2 to 16 cameras", n_cams);
    if (p->undistort_points) return p2s_set_error(P2S_ERR_INVALID_ARG, "undistort_points is not supported with per-frame cameras");
    if (p->handle_lr_swap) return p2s_set_error(P2S_ERR_INVALID_ARG, "handle_lr_swap is not supported with per-frame cameras");
    if (n_cal_frames < 1) return p2s_set_error(P2S_ERR_INVALID_ARG, "n_cal_frames=%lld: at least one calibration frame is needed", (long long)n_cal_frames);
    if (n_cal_frames >= ((int64_t)1 << 31)) return p2s_set_error(P2S_ERR_INVALID_ARG, "n_cal_frames=%lld is too many", (long long)n_cal_frames);
    if (n_blocks < 0 || K <= 0) return p2s_set_error(P2S_ERR_INVALID_ARG, "bad shape: n_blocks=%lld K=%d", (long long)n_blocks, K);
    if (dtype != P2S_F32 && dtype != P2S_F64) return p2s_set_error(P2S_ERR_INVALID_ARG, "dtype must be P2S_F32 or P2S_F64");
    if (p->min_cameras < 1) return p2s_set_error(P2S_ERR_INVALID_ARG, "min_cameras must be >= 1 (got %d)", p->min_cameras);
    if (!(p->reproj_error_threshold == p->reproj_error_threshold))
        return p2s_set_error(P2S_ERR_INVALID_ARG, "reproj_error_threshold is NaN");
    if (n_blocks * (int64_t)K >= (int64_t)1 << 40) return p2s_set_error(P2S_ERR_INVALID_ARG, "too many units");
    if ((int64_t)n_cams * K * 3 * 8 > ((int64_t)1 << 26)) return p2s_set_error(P2S_ERR_INVALID_ARG, "K=%d too large", K);
    if (n_blocks > 0 && (!P || !xyl || !block_frame || !Q || !err || !n_excl || !mask))
        return p2s_set_error(P2S_ERR_INVALID_ARG, "null %s pointer", what);
    return P2S_OK;
}

// block_frame on the host: every entry in [0, Fc), never decreasing.
int frames_check_map(const int64_t *bf, int64_t n_blocks, int64_t n_cal_frames) {
    for (int64_t b = 0; b < n_blocks; ++b) {
        if (bf[b] < 0 || bf[b] >= n_cal_frames)
            return p2s_set_error(P2S_ERR_INVALID_ARG, "block_frame[%lld]=%lld outside [0, %lld)", (long long)b, (long long)bf[b],
                                 (long long)n_cal_frames);
        if (b > 0 && bf[b] < bf[b - 1])
            return p2s_set_error(P2S_ERR_INVALID_ARG, "block_frame decreases at block %lld (%lld after %lld): the blocks of one calibration frame must be consecutive",
                                 (long long)b, (long long)bf[b], (long long)bf[b - 1]);
    }
    return P2S_OK;
}

// The launches of one call; every operand is on the device but bf, the checked host copy of block_frame.  A chunk keeps
// the kernel's 32-bit byte offsets below 2^31.  The stream is idle when the plan goes up (the previous call's kernels
// may still be reading the plan buffer otherwise) and nothing is read back after the first launch.
int frames_run(p2s_ctx *ctx, int32_t C, const double *d_P, int64_t n_blocks, int32_t K, int32_t dtype, const void *d_xyl,
               const int64_t *bf, const p2s_tri_params *params, double *d_Q, float *d_err, uint8_t *d_n_excl,
               uint32_t *d_excl_mask) {
    const int64_t blk_bytes = (int64_t)C * K * 3 * (dtype == P2S_F32 ? 4 : 8);
    const int64_t chunk_blocks = std::max<int64_t>(1, ((int64_t)1 << 31) / blk_bytes - 1);
    // the plan: per chunk, every run of equal frame cut into waves of up to 64 units
    std::vector<P2sFrameWave> plan;
    std::vector<size_t> chunk_start;
    for (int64_t b0 = 0; b0 < n_blocks; b0 += chunk_blocks) {
        chunk_start.push_back(plan.size());
        const int64_t b1 = std::min(n_blocks, b0 + chunk_blocks);
        for (int64_t b = b0; b < b1;) {
            int64_t e = b + 1;
            while (e < b1 && bf[e] == bf[b]) ++e;
            const int64_t u0 = (b - b0) * K, u1 = (e - b0) * K;
            for (int64_t u = u0; u < u1; u += 64)
                plan.push_back(P2sFrameWave{(uint32_t)u, (uint32_t)std::min<int64_t>(64, u1 - u), (uint32_t)bf[b], 0u});
            b = e;
        }
    }
    chunk_start.push_back(plan.size());

    HIP_TRY(hipStreamSynchronize(ctx->stream));
    const size_t tab_bytes = sizeof(uint16_t) << 16;
    std::vector<uint16_t> tab;
    std::vector<uint32_t> off;
    if (ctx->frames_sub_cams != C) {
        ctx->frames_sub_cams = 0;
        P2S_TRY(ctx->frames_sub.ensure(tab_bytes + sizeof(uint32_t) * 18));
        P2S_TRY(p2s_poison(ctx, ctx->frames_sub));
        p2s_subset_table(C, tab, off);
        HIP_TRY(hipMemcpyAsync(ctx->frames_sub.p, tab.data(), tab.size() * sizeof(uint16_t), hipMemcpyHostToDevice, ctx->stream));
        HIP_TRY(hipMemcpyAsync((char *)ctx->frames_sub.p + tab_bytes, off.data(), off.size() * sizeof(uint32_t), hipMemcpyHostToDevice, ctx->stream));
    }
    P2S_TRY(ctx->frames_plan.ensure(plan.size() * sizeof(P2sFrameWave)));
    P2S_TRY(p2s_poison(ctx, ctx->frames_plan));
    HIP_TRY(hipMemcpyAsync(ctx->frames_plan.p, plan.data(), plan.size() * sizeof(P2sFrameWave), hipMemcpyHostToDevice, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));                        // plan, tab and off may go
    ctx->frames_sub_cams = C;

    P2sFramesArgs a{};
    a.xyl = d_xyl; a.P = d_P;
    a.Q = d_Q; a.err = d_err; a.n_excl = d_n_excl; a.mask = d_excl_mask;
    a.stats = ctx->d_stats;
    a.sub_tab = (const uint16_t *)ctx->frames_sub.p;
    a.sub_off = (const uint32_t *)((const char *)ctx->frames_sub.p + tab_bytes);
    a.K = K; a.C = C;
    a.min_cams = params->min_cameras;
    a.thr = params->reproj_error_threshold;
    a.lik_thr = params->likelihood_threshold;
    for (size_t i = 0; i + 1 < chunk_start.size(); ++i) {
        a.block0 = (int64_t)i * chunk_blocks;
        a.waves = (const P2sFrameWave *)ctx->frames_plan.p + chunk_start[i];
        HIP_TRY(launch_frames_any(a, dtype, (unsigned)(chunk_start[i + 1] - chunk_start[i]), ctx->stream));
    }
    return P2S_OK;
}

}  // namespace

extern "C" {

int p2s_triangulate_frames_device(p2s_ctx *ctx, int64_t n_cal_frames, int32_t n_cams, const double *d_P, int64_t n_blocks,
                                  int32_t n_kpts, int32_t dtype, const void *d_xyl, const int64_t *d_block_frame,
                                  const p2s_tri_params *params, double *d_Q, float *d_err, uint8_t *d_n_excl,
                                  uint32_t *d_excl_mask) {
    P2S_TRY(frames_check(ctx, n_cal_frames, n_cams, d_P, n_blocks, n_kpts, dtype, d_xyl, d_block_frame, params, d_Q, d_err,
                         d_n_excl, d_excl_mask, "device"));
    if (n_blocks == 0) return P2S_OK;
    HIP_TRY(hipSetDevice(ctx->device));
    std::vector<int64_t> bf((size_t)n_blocks);
    HIP_TRY(hipMemcpyAsync(bf.data(), d_block_frame, (size_t)n_blocks * 8, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    P2S_TRY(frames_check_map(bf.data(), n_blocks, n_cal_frames));
    return frames_run(ctx, n_cams, d_P, n_blocks, n_kpts, dtype, d_xyl, bf.data(), params, d_Q, d_err, d_n_excl, d_excl_mask);
}

int p2s_triangulate_frames_host(p2s_ctx *ctx, int64_t n_cal_frames, int32_t n_cams, const double *P, int64_t n_blocks,
                                int32_t n_kpts, int32_t dtype, const void *xyl, const int64_t *block_frame,
                                const p2s_tri_params *params, double *Q, float *err, uint8_t *n_excl, uint32_t *excl_mask) {
    P2S_TRY(frames_check(ctx, n_cal_frames, n_cams, P, n_blocks, n_kpts, dtype, xyl, block_frame, params, Q, err, n_excl,
                         excl_mask, "host"));
    if (n_blocks == 0) return P2S_OK;
    P2S_TRY(frames_check_map(block_frame, n_blocks, n_cal_frames));
    const size_t elem = dtype == P2S_F32 ? 4 : 8;
    const size_t n_units = (size_t)n_blocks * n_kpts;
    HIP_TRY(hipSetDevice(ctx->device));
    Stage st{ctx};
    const void *d_xyl;
    const double *d_P;
    double *d_Q;
    float *d_err;
    uint8_t *d_nexcl;
    uint32_t *d_mask;
    P2S_TRY(st.upload(d_P, P, (size_t)n_cal_frames * n_cams * 12 * 8));
    P2S_TRY(st.upload(d_xyl, xyl, (size_t)n_blocks * n_cams * n_kpts * 3 * elem));
    P2S_TRY(st.alloc(d_Q, n_units * 24));
    P2S_TRY(st.alloc(d_err, n_units * 4));
    P2S_TRY(st.alloc(d_nexcl, n_units));
    P2S_TRY(st.alloc(d_mask, n_units * 4));
    P2S_TRY(frames_run(ctx, n_cams, d_P, n_blocks, n_kpts, dtype, d_xyl, block_frame, params, d_Q, d_err, d_nexcl, d_mask));
    P2S_TRY(st.down(Q, d_Q, n_units * 24));
    P2S_TRY(st.down(err, d_err, n_units * 4));
    P2S_TRY(st.down(n_excl, d_nexcl, n_units));
    P2S_TRY(st.down(excl_mask, d_mask, n_units * 4));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    return P2S_OK;
}

}  // extern "C"
