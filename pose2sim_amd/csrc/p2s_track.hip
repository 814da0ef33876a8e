// p2s_track.hip -- person tracking across the frames of multi-person triangulation (triangulation.py:823-874 around
// common.py:1037-1136, sort_people_sports2d with scores=None): which detection every person slot takes, frame after
// frame.  float64 end to end; the only computed number is the mean keypoint distance, and it is NumPy's bit for bit.
//
//   track_kernel   one workgroup of 256 lanes a trial, a loop over the trial's frames inside it
//
// The recurrence.  The state S [32][K][3] holds the last non-NaN value of every coordinate of every slot; n of its rows
// are live, the others NaN.  Frame f with detections C [P][K][3]: dist[i][j] = mean over the keypoints of
// sqrt(nansum((C[j][k] - S[i][k])**2)) with NaN and +inf turned into 1e10, scipy's linear_sum_assignment on the n x P
// matrix (p2s_lsap.h), pairs above max_dist dropped, the detections left over appended as new slots in ascending order,
// and S takes the placed detections' non-NaN values.  The absolute frame 0 is not matched: the slots take the detections
// in their own order.  n only grows; a frame that would pass 32 slots ends the trial (status).
//
// Lanes.  S and the frame's detections live in LDS.  The n * P * K keypoint distances are spread over the lanes into an
// LDS table D [pair][K], `rp` pairs a round (as many as the LDS left over holds; one round for every usual shape); then
// one lane a pair sums its K distances in np.add.reduce's order (p2s_npsum_small.h below 129 entries, one pairwise split
// above) and divides by K.  Lane 0 solves the assignment on the matrix in LDS, its work arrays in LDS too, and places
// the detections; all lanes then update S and write the frame's outputs.  Barriers per frame: 2 a round, 1 after the
// solve, 1 after the update, 1 after the next frame's detections are in LDS -- 5 with one round.
//
// Latency.  The frames depend on each other, so the loop is a chain of LDS round trips, barriers and one serial solve;
// no global load sits in it: the next frame's P * K * 3 values are requested into registers (12 a lane, 3 072 values)
// before the current frame's work starts and go to LDS after it.  Only what a larger frame holds beyond that is loaded
// where it is stored.  ids, matched_dist, n_slots and Q_rows are stored and never read back.
//
// Bit equality.  Contraction is off for this file: (a - b)**2 is rn(d * d), the three squares are added from 0.0 in
// order (a NaN square is skipped: nansum adds 0.0 to a non-negative sum), the root is the correctly rounded one.
// ctx == NULL runs the same functions on the host (track_host): the restatement is checked against NumPy without a GPU.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include <string.h>

#include <algorithm>
#include <vector>

#include "p2s_ctx.h"
#include "p2s_lsap.h"
#include "p2s_npsum_small.h"

#pragma clang fp contract(off)

#define P2S_TRK_MAX_SLOTS P2S_LSAP_MAX
#define P2S_TRK_MAX_KPTS_DEVICE 240      // one pairwise split gives two runs of at most 128: K / 2 + 8 <= 128
#define P2S_TRK_HD __host__ __device__ inline

struct P2sTrackArgs {
    const double *Q;             // [N][P][K][3] the frames of all trials back to back
    const int64_t *frame_off;    // [T + 1]
    const int64_t *first_frame;  // [T] absolute number of every trial's first frame
    const double *state_in;      // [T][32][K][3] or NULL: every trial starts with P slots of NaN
    const int32_t *n_state_in;   // [T] live rows of state_in
    int32_t *ids;                // [N][P]
    double *Q_rows;              // [N][P][K][3]
    double *matched;             // [N][P]
    int32_t *n_slots;            // [N]
    double *state_out;           // [T][32][K][3]
    int32_t *n_state_out;        // [T]
    int32_t *status;             // [T][2]
    double max_dist;
    int32_t has_max, P, K, rp;   // rp: pairs a round of the distance table
};

namespace {

constexpr int TT = 256;                  // lanes of a trial's workgroup
constexpr int NPRE = 12;                 // values of the next frame a lane keeps in registers
constexpr int MAXS = P2S_TRK_MAX_SLOTS;

P2S_TRK_HD double trk_nan() {
    const uint64_t bits = 0x7ff8000000000000ULL;
    double v;
    memcpy(&v, &bits, sizeof v);
    return v;
}

// sqrt(np.nansum((c - s)**2)) of one keypoint
P2S_TRK_HD double trk_kpt_dist(const double *c, const double *s) {
    double acc = 0.0;
    for (int i = 0; i < 3; ++i) {
        const double d = c[i] - s[i], sq = d * d;
        if (sq == sq) acc = acc + sq;
    }
#if defined(__HIP_DEVICE_COMPILE__)
    return __dsqrt_rn(acc);
#else
    return sqrt(acc);
#endif
}

// np.add.reduce over n contiguous entries: NumPy's pairwise_sum, at most DEPTH splits deep
template <int DEPTH> P2S_TRK_HD double trk_np_sum(const double *a, int n) {
    if constexpr (DEPTH > 0) {
        if (n > 128) {
            int n2 = n / 2;
            n2 -= n2 % 8;
            return trk_np_sum<DEPTH - 1>(a, n2) + trk_np_sum<DEPTH - 1>(a + n2, n - n2);
        }
    }
    return p2s_np_sum_below_128<1>(a, n);
}

// The same sum on the host at any length: plain recursion (a template of every depth takes the compiler half an hour)
double trk_np_sum_host(const double *a, int n) {
    if (n <= 128) return p2s_np_sum_below_128<1>(a, n);
    int n2 = n / 2;
    n2 -= n2 % 8;
    return trk_np_sum_host(a, n2) + trk_np_sum_host(a + n2, n - n2);
}

// np.nan_to_num(np.nanmean(d), nan=1e10, posinf=1e10) from the sum of a pair's K keypoint distances, none of them NaN
P2S_TRK_HD double trk_pair_cost(double sum, int K) {
    const double mean = sum / (double)K;
    return (mean != mean || mean == __builtin_huge_val()) ? 1e10 : mean;
}

// The slots of a frame that is not matched (the absolute frame 0, or a state without slots): detection p in slot p.
P2S_TRK_HD int trk_place_identity(int n, int P, int *slot_det, double *slot_dist) {
    for (int i = 0; i < MAXS; ++i) { slot_det[i] = i < P ? i : -1; slot_dist[i] = trk_nan(); }
    return n > P ? n : P;
}

// The slots after the assignment: the kept pairs, then the detections left over as new slots.  -> the new slot count, -1
// when it would pass 32.
P2S_TRK_HD int trk_place(int n, int P, const double *cost, int n_pairs, const int *row_ind, const int *col_ind, int has_max,
                         double max_dist, int *slot_det, double *slot_dist) {
    for (int i = 0; i < MAXS; ++i) { slot_det[i] = -1; slot_dist[i] = trk_nan(); }
    uint32_t taken = 0;
    for (int k = 0; k < n_pairs; ++k) {
        const int r = row_ind[k], c = col_ind[k];                 // r < n <= 32, c < P <= 32
        const double d = cost[r * P + c];
        if (!has_max || d <= max_dist) { slot_det[r] = c; slot_dist[r] = d; taken |= (uint32_t)1 << c; }
    }
    for (int c = 0; c < P; ++c) {
        if ((taken >> c) & 1) continue;
        if (n == MAXS) return -1;
        slot_det[n++] = c;
    }
    return n;
}

struct TrkCtl {
    P2sLsapWork work;
    double slot_dist[MAXS];
    int row_ind[MAXS], col_ind[MAXS], slot_det[MAXS];
    int n_new, flag;
};

// LDS of a trial's workgroup: S, the frame's detections, the distance table of rp pairs, the cost matrix, TrkCtl
size_t trk_lds_bytes(int P, int K, int rp) {
    return ((size_t)MAXS * 3 * K + (size_t)P * 3 * K + (size_t)rp * K + MAXS * MAXS) * sizeof(double) + sizeof(TrkCtl);
}

__global__ void __launch_bounds__(TT) track_kernel(const P2sTrackArgs a) {
    extern __shared__ double trk_lds[];
    const int tid = threadIdx.x, P = a.P, K = a.K, K3 = 3 * K, PK3 = P * K3;
    double *S = trk_lds, *C = S + MAXS * K3, *D = C + PK3, *cost = D + (size_t)a.rp * K;
    TrkCtl &ctl = *reinterpret_cast<TrkCtl *>(cost + MAXS * MAXS);
    const int64_t t = blockIdx.x, f0 = a.frame_off[t], F = a.frame_off[t + 1] - f0, first = a.first_frame[t];
    int n = a.state_in ? a.n_state_in[t] : P;
    const bool bad_state = n < 0 || n > MAXS;                     // device pointers are not checked by the host
    if (bad_state) n = 0;
    for (int idx = tid; idx < MAXS * K3; idx += TT)
        S[idx] = a.state_in && idx < n * K3 ? a.state_in[t * MAXS * K3 + idx] : trk_nan();
    const double *src = a.Q + f0 * PK3;                           // frame fi at src + fi * PK3, fi < F
    if (F > 0)
        for (int idx = tid; idx < PK3; idx += TT) C[idx] = src[idx];
    __syncthreads();
    int stopped = 0;
    for (int64_t fi = 0; fi < F; ++fi) {
        // the next frame on its way while this one is worked on
        double pre[NPRE];
        const double *nxt = src + (fi + 1) * PK3;
        const bool more = fi + 1 < F;
#pragma unroll
        for (int r = 0; r < NPRE; ++r) {
            const int idx = tid + r * TT;
            pre[r] = more && idx < PK3 ? nxt[idx] : 0.0;
        }
        const bool match = first + fi != 0 && n > 0;
        if (match) {
            const int pairs = n * P;                              // <= 32 * 32
            for (int p0 = 0; p0 < pairs; p0 += a.rp) {
                const int cnt = pairs - p0 < a.rp ? pairs - p0 : a.rp;
                for (int idx = tid; idx < cnt * K; idx += TT) {
                    const int ps = idx / K, k = idx - ps * K, pair = p0 + ps, i = pair / P, j = pair - i * P;
                    D[idx] = trk_kpt_dist(C + (j * K + k) * 3, S + (i * K + k) * 3);   // idx < rp * K
                }
                __syncthreads();
                for (int ps = tid; ps < cnt; ps += TT) cost[p0 + ps] = trk_pair_cost(trk_np_sum<1>(D + ps * K, K), K);
                __syncthreads();
            }
        }
        if (tid == 0) {
            int n_new, flag = bad_state ? -1 : 0;
            if (bad_state) {
                n_new = -1;
            } else if (match) {
                flag = p2s_lsap_solve(n, P, cost, ctl.work, ctl.row_ind, ctl.col_ind);
                n_new = flag != P2S_LSAP_OK ? -1
                                            : trk_place(n, P, cost, n < P ? n : P, ctl.row_ind, ctl.col_ind, a.has_max, a.max_dist,
                                                        ctl.slot_det, ctl.slot_dist);
            } else {
                n_new = trk_place_identity(n, P, ctl.slot_det, ctl.slot_dist);
            }
            ctl.n_new = n_new; ctl.flag = flag;
        }
        __syncthreads();
        const int n_new = ctl.n_new;
        if (n_new < 0) {                                          // uniform over the workgroup
            if (tid == 0) { a.status[2 * t] = (int32_t)(fi + 1); a.status[2 * t + 1] = ctl.flag; }
            stopped = 1;
            break;
        }
        const int64_t gf = f0 + fi;
        for (int idx = tid; idx < n_new * K3; idx += TT) {        // n_new >= P
            const int i = idx / K3, e = idx - i * K3, j = ctl.slot_det[i];
            const double v = j >= 0 ? C[j * K3 + e] : trk_nan();
            if (v == v) S[idx] = v;                               // a new slot's row was NaN
            if (i < P && a.Q_rows) a.Q_rows[gf * PK3 + idx] = v;
        }
        if (tid < P) {
            if (a.ids) a.ids[gf * P + tid] = ctl.slot_det[tid];
            if (a.matched) a.matched[gf * P + tid] = ctl.slot_dist[tid];
        }
        if (tid == 0 && a.n_slots) a.n_slots[gf] = n_new;
        n = n_new;
        __syncthreads();
        if (more) {
#pragma unroll
            for (int r = 0; r < NPRE; ++r) {
                const int idx = tid + r * TT;
                if (idx < PK3) C[idx] = pre[r];
            }
            for (int idx = tid + NPRE * TT; idx < PK3; idx += TT) C[idx] = nxt[idx];
        }
        __syncthreads();
    }
    if (a.state_out)
        for (int idx = tid; idx < MAXS * K3; idx += TT) a.state_out[t * MAXS * K3 + idx] = S[idx];
    if (tid == 0) {
        if (a.n_state_out) a.n_state_out[t] = n;
        if (!stopped) { a.status[2 * t] = bad_state && F == 0 ? 1 : 0; a.status[2 * t + 1] = bad_state && F == 0 ? -1 : 0; }
    }
}

// The same recurrence on the host, one trial after the other.
void track_host(const P2sTrackArgs &a, int64_t T) {
    const int P = a.P, K = a.K, K3 = 3 * K, PK3 = P * K3;
    std::vector<double> S((size_t)MAXS * K3), D((size_t)K), cost(MAXS * MAXS), slot_dist(MAXS);
    std::vector<int> row_ind(MAXS), col_ind(MAXS), slot_det(MAXS);
    P2sLsapWork work;
    for (int64_t t = 0; t < T; ++t) {
        const int64_t f0 = a.frame_off[t], F = a.frame_off[t + 1] - f0, first = a.first_frame[t];
        int n = a.state_in ? a.n_state_in[t] : P;
        for (int idx = 0; idx < MAXS * K3; ++idx) S[idx] = a.state_in && idx < n * K3 ? a.state_in[t * MAXS * K3 + idx] : trk_nan();
        int32_t status[2] = {0, 0};
        for (int64_t fi = 0; fi < F; ++fi) {
            const int64_t gf = f0 + fi;
            const double *C = a.Q + gf * PK3;
            int n_new, flag = 0;
            if (first + fi != 0 && n > 0) {
                for (int i = 0; i < n; ++i)
                    for (int j = 0; j < P; ++j) {
                        for (int k = 0; k < K; ++k) D[k] = trk_kpt_dist(C + (j * K + k) * 3, S.data() + (i * K + k) * 3);
                        cost[i * P + j] = trk_pair_cost(trk_np_sum_host(D.data(), K), K);
                    }
                flag = p2s_lsap_solve(n, P, cost.data(), work, row_ind.data(), col_ind.data());
                n_new = flag != P2S_LSAP_OK ? -1
                                            : trk_place(n, P, cost.data(), std::min(n, P), row_ind.data(), col_ind.data(), a.has_max,
                                                        a.max_dist, slot_det.data(), slot_dist.data());
            } else {
                n_new = trk_place_identity(n, P, slot_det.data(), slot_dist.data());
            }
            if (n_new < 0) { status[0] = (int32_t)(fi + 1); status[1] = flag; break; }
            for (int idx = 0; idx < n_new * K3; ++idx) {
                const int i = idx / K3, e = idx - i * K3, j = slot_det[i];
                const double v = j >= 0 ? C[j * K3 + e] : trk_nan();
                if (v == v) S[idx] = v;
                if (i < P && a.Q_rows) a.Q_rows[gf * PK3 + idx] = v;
            }
            for (int p = 0; p < P; ++p) {
                if (a.ids) a.ids[gf * P + p] = slot_det[p];
                if (a.matched) a.matched[gf * P + p] = slot_dist[p];
            }
            if (a.n_slots) a.n_slots[gf] = n_new;
            n = n_new;
        }
        if (a.state_out) std::copy(S.begin(), S.end(), a.state_out + t * MAXS * K3);
        if (a.n_state_out) a.n_state_out[t] = n;
        a.status[2 * t] = status[0]; a.status[2 * t + 1] = status[1];
    }
}

// What both entry points check of the shape, and the frames of all trials: N.
int track_check(int64_t n_trials, const int64_t *frame_off, const int64_t *first_frame, int32_t P, int32_t K, const void *Q,
                const void *state_in, const void *n_state_in, const void *status, int64_t &N) {
    if (n_trials < 0 || n_trials >= ((int64_t)1 << 31)) return p2s_set_error(P2S_ERR_INVALID_ARG, "n_trials=%lld outside [0, 2^31 - 1]", (long long)n_trials);
    if (P < 1 || P > MAXS) return p2s_set_error(P2S_ERR_INVALID_ARG, "n_persons=%d outside [1, %d]", P, MAXS);
    if (K < 1 || K > (1 << 20)) return p2s_set_error(P2S_ERR_INVALID_ARG, "n_kpts=%d outside [1, 2^20]", K);
    N = 0;
    if (n_trials == 0) return P2S_OK;
    if (!frame_off || !first_frame || !status || (state_in && !n_state_in)) return p2s_set_error(P2S_ERR_INVALID_ARG, "null argument");
    if (frame_off[0] != 0) return p2s_set_error(P2S_ERR_INVALID_ARG, "frame_off must start at 0");
    for (int64_t t = 0; t < n_trials; ++t)
        if (frame_off[t + 1] < frame_off[t]) return p2s_set_error(P2S_ERR_INVALID_ARG, "frame_off must not decrease (trial %lld)", (long long)t);
    N = frame_off[n_trials];
    if (N >= ((int64_t)1 << 31)) return p2s_set_error(P2S_ERR_INVALID_ARG, "%lld frames are too many", (long long)N);
    if (N > 0 && !Q) return p2s_set_error(P2S_ERR_INVALID_ARG, "null argument");
    return P2S_OK;
}

int track_check_states(int64_t n_trials, const int32_t *n_state_in) {
    for (int64_t t = 0; t < n_trials; ++t)
        if (n_state_in[t] < 0 || n_state_in[t] > MAXS)
            return p2s_set_error(P2S_ERR_INVALID_ARG, "trial %lld starts with %d slots; expected 0 .. %d", (long long)t, n_state_in[t], MAXS);
    return P2S_OK;
}

// The pairs a round that the device's LDS leaves room for, the workgroup's LDS with them; a shape that does not fit is
// refused.
int track_geometry(p2s_ctx *ctx, int32_t P, int32_t K, int32_t &rp, size_t &lds) {
    int limit = 0;
    HIP_TRY(hipDeviceGetAttribute(&limit, hipDeviceAttributeMaxSharedMemoryPerBlock, ctx->device));
    const size_t fixed = trk_lds_bytes(P, K, 0), row = (size_t)K * sizeof(double);
    if (K > P2S_TRK_MAX_KPTS_DEVICE || fixed + row > (size_t)limit)
        return p2s_set_error(P2S_ERR_INVALID_ARG, "n_persons=%d, n_kpts=%d need %zu bytes of LDS and at most %d keypoints; the device gives a workgroup %d bytes",
                             P, K, fixed + row, P2S_TRK_MAX_KPTS_DEVICE, limit);
    rp = (int32_t)std::min<size_t>(((size_t)limit - fixed) / row, (size_t)MAXS * P);
    lds = trk_lds_bytes(P, K, rp);
    return P2S_OK;
}

hipError_t launch_track(const P2sTrackArgs &a, int64_t T, size_t lds, hipStream_t s) {
    hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(&track_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(track_kernel, dim3((unsigned)T), dim3(TT), lds, s, a);
    return hipGetLastError();
}

}  // namespace

// ---- C-ABI entry points (include/p2s.h) ----------------------------------------------------------------------------
extern "C" {

int p2s_track_persons_host(p2s_ctx *ctx, int64_t n_trials, const int64_t *frame_off, const int64_t *first_frame, int32_t n_persons,
                           int32_t n_kpts, const double *Q, int32_t has_max_dist, double max_dist, const double *state_in,
                           const int32_t *n_state_in, int32_t *ids, double *Q_rows, double *matched_dist, int32_t *n_slots,
                           double *state_out, int32_t *n_state_out, int32_t *status) {
    int64_t N;
    P2S_TRY(track_check(n_trials, frame_off, first_frame, n_persons, n_kpts, Q, state_in, n_state_in, status, N));
    P2sTrackArgs a{};
    a.has_max = has_max_dist != 0; a.max_dist = max_dist; a.P = n_persons; a.K = n_kpts;
    int32_t rp = 0;
    size_t lds = 0;
    if (ctx) {
        HIP_TRY(hipSetDevice(ctx->device));
        P2S_TRY(track_geometry(ctx, n_persons, n_kpts, rp, lds));
    }
    if (n_trials == 0) return P2S_OK;
    if (state_in) P2S_TRY(track_check_states(n_trials, n_state_in));
    const size_t T = (size_t)n_trials, K3 = 3 * (size_t)n_kpts, PK3 = (size_t)n_persons * K3, SK3 = (size_t)MAXS * K3;
    if (!ctx) {                                                   // the same functions on the host
        a.Q = Q; a.frame_off = frame_off; a.first_frame = first_frame; a.state_in = state_in; a.n_state_in = n_state_in;
        a.ids = ids; a.Q_rows = Q_rows; a.matched = matched_dist; a.n_slots = n_slots; a.state_out = state_out;
        a.n_state_out = n_state_out; a.status = status;
        track_host(a, n_trials);
        return P2S_OK;
    }
    Layout in, out;
    const size_t i_foff = in.add((T + 1) * 8), i_first = in.add(T * 8), i_n = in.add(state_in ? T * 4 : 0), i_state = in.add(state_in ? T * SK3 * 8 : 0);
    const size_t o_status = out.add(T * 2 * 4), o_ids = out.add(ids ? (size_t)N * n_persons * 4 : 0), o_rows = out.add(Q_rows ? (size_t)N * PK3 * 8 : 0),
                 o_dist = out.add(matched_dist ? (size_t)N * n_persons * 8 : 0), o_slots = out.add(n_slots ? (size_t)N * 4 : 0),
                 o_state = out.add(state_out ? T * SK3 * 8 : 0), o_n = out.add(n_state_out ? T * 4 : 0);
    Stage st{ctx};
    char *din, *dout;
    P2S_TRY(st.upload(a.Q, Q, (size_t)N * PK3 * sizeof(double)));
    P2S_TRY(st.alloc(din, in.bytes));
    P2S_TRY(st.up(din + i_foff, frame_off, (T + 1) * 8));
    P2S_TRY(st.up(din + i_first, first_frame, T * 8));
    if (state_in) {
        P2S_TRY(st.up(din + i_n, n_state_in, T * 4));
        P2S_TRY(st.up(din + i_state, state_in, T * SK3 * 8));
    }
    P2S_TRY(st.alloc(dout, out.bytes));
    a.frame_off = (const int64_t *)(din + i_foff); a.first_frame = (const int64_t *)(din + i_first);
    a.n_state_in = state_in ? (const int32_t *)(din + i_n) : nullptr; a.state_in = state_in ? (const double *)(din + i_state) : nullptr;
    a.status = (int32_t *)(dout + o_status);
    a.ids = ids ? (int32_t *)(dout + o_ids) : nullptr; a.Q_rows = Q_rows ? (double *)(dout + o_rows) : nullptr;
    a.matched = matched_dist ? (double *)(dout + o_dist) : nullptr; a.n_slots = n_slots ? (int32_t *)(dout + o_slots) : nullptr;
    a.state_out = state_out ? (double *)(dout + o_state) : nullptr; a.n_state_out = n_state_out ? (int32_t *)(dout + o_n) : nullptr;
    a.rp = rp;
    P2S_TRY(st.time_begin());
    HIP_TRY(launch_track(a, n_trials, lds, ctx->stream));
    P2S_TRY(st.time_end());
    P2S_TRY(st.down(status, a.status, T * 2 * 4));
    P2S_TRY(st.down(ids, a.ids, (size_t)N * n_persons * 4));
    P2S_TRY(st.down(Q_rows, a.Q_rows, (size_t)N * PK3 * 8));
    P2S_TRY(st.down(matched_dist, a.matched, (size_t)N * n_persons * 8));
    P2S_TRY(st.down(n_slots, a.n_slots, (size_t)N * 4));
    P2S_TRY(st.down(state_out, a.state_out, T * SK3 * 8));
    P2S_TRY(st.down(n_state_out, a.n_state_out, T * 4));
    return st.finish(P2S_TIMED_TRACK_PERSONS);                    // frame_off, first_frame and the state are host memory: alive until here
}

int p2s_track_persons_device(p2s_ctx *ctx, int64_t n_trials, const int64_t *frame_off, const int64_t *first_frame, int32_t n_persons,
                             int32_t n_kpts, const double *d_Q, int32_t has_max_dist, double max_dist, const double *d_state_in,
                             const int32_t *d_n_state_in, int32_t *d_ids, double *d_Q_rows, double *d_matched_dist, int32_t *d_n_slots,
                             double *d_state_out, int32_t *d_n_state_out, int32_t *d_status) {
    if (!ctx) return p2s_set_error(P2S_ERR_INVALID_ARG, "null context");
    int64_t N;
    P2S_TRY(track_check(n_trials, frame_off, first_frame, n_persons, n_kpts, d_Q, d_state_in, d_n_state_in, d_status, N));
    HIP_TRY(hipSetDevice(ctx->device));
    int32_t rp;
    size_t lds;
    P2S_TRY(track_geometry(ctx, n_persons, n_kpts, rp, lds));
    if (n_trials == 0) return P2S_OK;
    // frame_off and first_frame describe the shape, as n_blocks does for p2s_triangulate_device: HOST arrays, kept by the
    // context until the next call so that the caller may free its own at once
    const size_t T = (size_t)n_trials;
    ctx->track_meta.assign(frame_off, frame_off + T + 1);
    ctx->track_meta.insert(ctx->track_meta.end(), first_frame, first_frame + T);
    Stage st{ctx};
    int64_t *meta;
    P2S_TRY(st.upload(meta, ctx->track_meta.data(), (2 * T + 1) * 8));
    P2sTrackArgs a{};
    a.Q = d_Q; a.frame_off = meta; a.first_frame = meta + T + 1; a.state_in = d_state_in; a.n_state_in = d_n_state_in;
    a.ids = d_ids; a.Q_rows = d_Q_rows; a.matched = d_matched_dist; a.n_slots = d_n_slots; a.state_out = d_state_out;
    a.n_state_out = d_n_state_out; a.status = d_status;
    a.has_max = has_max_dist != 0; a.max_dist = max_dist; a.P = n_persons; a.K = n_kpts; a.rp = rp;
    HIP_TRY(launch_track(a, n_trials, lds, ctx->stream));
    return P2S_OK;
}

int p2s_track_persons_kernel_ms(p2s_ctx *ctx, float *elapsed_ms) { return p2s_kernel_ms_query(ctx, P2S_TIMED_TRACK_PERSONS, "p2s_track_persons_host", elapsed_ms); }

}  // extern "C"
