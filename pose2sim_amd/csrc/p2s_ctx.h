// p2s_ctx.h -- the per-GPU context behind include/p2s.h's opaque p2s_ctx, and what the C-ABI entry points (p2s_api.hip
// and the tail of every stage's kernel file) share to use it: HIP_TRY / P2S_TRY, the grow-only Scratch buffer, Stage,
// which hands a *_host call its device buffers and times its kernels (one slot of p2s_ctx::kernel_ms a stage, read
// back by p2s_kernel_ms_query), Layout, which carves one block into arrays, Block, which keeps that block on the device
// or on the host, and the checked frame and person offsets of the per-camera analysis stages (P2sFrames).
#ifndef P2S_CTX_H
#define P2S_CTX_H

#include <hip/hip_runtime.h>
#include <string.h>

#include <vector>

#include "p2s.h"
#include "p2s_error.h"
#include "p2s_internal.h"

#define HIP_TRY(expr)                                                                                       \
    do {                                                                                                    \
        hipError_t e_ = (expr);                                                                             \
        if (e_ != hipSuccess)                                                                               \
            return p2s_set_error(e_ == hipErrorOutOfMemory ? P2S_ERR_OOM : P2S_ERR_HIP, "%s failed: %s", #expr, \
                                 hipGetErrorString(e_));                                                    \
    } while (0)

#define P2S_TRY(expr)                                                                                       \
    do {                                                                                                    \
        const int rc_ = (expr);                                                                             \
        if (rc_ != P2S_OK) return rc_;                                                                      \
    } while (0)

struct Scratch {
    void *p = nullptr;
    size_t bytes = 0;
    int ensure(size_t n) {
        if (n <= bytes) return P2S_OK;
        release();
        hipError_t e = hipMalloc(&p, n);
        if (e != hipSuccess) return p2s_set_error(P2S_ERR_OOM, "hipMalloc(%zu) failed: %s", n, hipGetErrorString(e));
        bytes = n;
        return P2S_OK;
    }
    void release() {
        if (p) (void)hipFree(p);
        p = nullptr;
        bytes = 0;
    }
};

#define P2S_N_SLOTS 8

// The stages that time their own kernels: one slot of p2s_ctx::kernel_ms each.
enum { P2S_TIMED_REPROJ, P2S_TIMED_JITTER, P2S_TIMED_CONFIDENCE, P2S_TIMED_ID_SWITCH, P2S_TIMED_GAIT, P2S_TIMED_MEASURE,
       P2S_TIMED_TRACK_SELECT, P2S_TIMED_TRACK_PERSONS, P2S_TIMED_GAPS, P2S_TIMED_TIMELINE, P2S_TIMED_REFINE, P2S_TIMED_RELPOSE,
       P2S_TIMED_FLOOR, P2S_N_TIMED };

struct p2s_ctx {
    int device = 0;
    hipStream_t own_stream = nullptr;
    hipStream_t stream = nullptr;
    P2sCam *d_cams = nullptr;
    uint32_t *d_binom = nullptr;
    uint32_t binom[33 * 33] = {};                    // the host's copy of d_binom: C(n, k) at [n * 33 + k], filled at creation
    int n_cams = 0;
    bool full_calib = false;     // K, dist, R, T, newK were provided
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    hipEvent_t ev_stage[2] = {nullptr, nullptr};     // around the kernels of the *_host call that times itself
    float kernel_ms[P2S_N_TIMED] = {-1.0f, -1.0f, -1.0f, -1.0f, -1.0f, -1.0f, -1.0f, -1.0f, -1.0f, -1.0f, -1.0f, -1.0f, -1.0f};   // the last call's kernel time of every P2S_TIMED_* stage; -1: has not run
    hipStream_t side_stream = nullptr;               // search kernels run here, beside the next chunk's streaming pass
    hipEvent_t ev_k1[2] = {nullptr, nullptr}, ev_k2[2] = {nullptr, nullptr};
    Scratch slot[P2S_N_SLOTS];                       // staging of the *_host calls (Stage): no role, no owner between calls
    std::vector<int64_t> track_meta;                 // p2s_track_persons_device: the host copy of its frame offsets, while they go up
    Scratch wl_rec, wl_count;
    Scratch deep_entries, deep_ctl, deep_sched, deep_partials;   // deep levels of the search (p2s_tri_deep.hip)
    uint32_t deep_min_subsets = P2S_DEEP_MIN_SUBSETS;            // 0 = every level stays in the search kernel's wave
    unsigned long long *d_stats = nullptr;           // P2S_N_STATS counters (p2s_get_tri_stats)
    unsigned long long *d_assoc_stats = nullptr;     // 4 counters (p2s_get_assoc_stats)
    uint16_t *d_sub_tab = nullptr;                   // camera subsets by level (fused kernel), built with the calibration
    uint32_t *d_sub_off = nullptr;
    // p2s_tri_frames.hip (per-frame cameras), independent of the static calibration above: the subset table of the last
    // call's camera count (frames_sub_cams; the level offsets follow 2^16 table entries) and the wave plan of one call
    Scratch frames_sub, frames_plan;
    int frames_sub_cams = 0;
    // p2s_set_tuning: experiments and tests only, never read from the environment
    int tri_path = P2S_TRI_PATH_AUTO;
    int force_tiled = 0, no_overlap = 0, job = 0;
    uint32_t max_subsets = P2S_MAX_SUBSETS_PER_LEVEL;
    int debug_mode = 0;                              // honoured by a -DP2S_DIAG build only
    int assoc_form = P2S_ASSOC_FORM_AUTO;
    int deep_prune = 1;                              // p2s_tri_deep.hip: exact pruning of the deep levels' evaluations
    int pool_singles_pct = 8;                        // p2s_tri_fused.hip: share of the tiles that the last workgroups take one at a time
    int screen = 1;                                  // p2s_tri_pool.hip: fp32 screen of the camera-subset candidates
    int gaps_ws_kb = P2S_GAPS_WORKSPACE_KB;          // p2s_gaps.hip: cap of the spline kinds' workspace
    int pool_tiles = 5;                              // p2s_tri_pool.hip: tiles a wave streams before it searches their pooled failures (2..6)
    int poison = -1;                                 // 0..255: p2s_poison fills every context-owned buffer with this byte before a call uses it
};

// Every subset of n_cams <= 16 cameras as a bit mask, level by level in itertools.combinations order
// (triangulation.py:411): what the lanes of the one-launch kernels index by (level, rank); 2^n_cams entries, level k
// starts at off[k], off has n_cams + 2 entries.
inline void p2s_subset_table(int n_cams, std::vector<uint16_t> &tab, std::vector<uint32_t> &off) {
    tab.clear();
    off.assign(n_cams + 2, 0);
    tab.reserve((size_t)1 << n_cams);
    for (int k = 0; k <= n_cams; ++k) {
        off[k] = (uint32_t)tab.size();
        std::vector<int> idx(k);
        for (int i = 0; i < k; ++i) idx[i] = i;
        for (;;) {
            uint32_t m = 0;
            for (int i = 0; i < k; ++i) m |= 1u << idx[i];
            tab.push_back((uint16_t)m);
            int i = k - 1;
            while (i >= 0 && idx[i] == n_cams - k + i) --i;
            if (i < 0) break;
            ++idx[i];
            for (int j = i + 1; j < k; ++j) idx[j] = idx[j - 1] + 1;
        }
    }
    off[n_cams + 1] = (uint32_t)tab.size();
}

// P2S_TUNE_POISON_STAGING (tests only).  What an earlier call left in a staging slot or in one of the six role buffers of
// the work-list triangulation (wl_rec, wl_count, deep_entries / ctl / sched / partials) is garbage by contract; with the
// switch on, that garbage is this byte over the buffer's whole capacity, put there on ctx->stream before anything of the
// call that asked for the buffer.  No buffer is exempt: none of them holds content meant to outlive a call.  Off is one
// branch.
inline int p2s_poison(p2s_ctx *ctx, const Scratch &s) {
    if (ctx->poison >= 0 && s.p) HIP_TRY(hipMemsetAsync(s.p, ctx->poison, s.bytes, ctx->stream));
    return P2S_OK;
}

// Device buffers of one *_host call.  The i-th buffer the call asks for is ctx->slot[i]: two pointers of one call never
// share a slot, a slot only grows (hipFree / hipMalloc on growth alone), and what an earlier call left in it is garbage
// (p2s_poison, above, makes it the same garbage every time for the tests).
// A buffer is never NULL (at least 16 bytes); copies of 0 bytes and downloads to a NULL host pointer are skipped.
struct Stage {
    p2s_ctx *ctx;
    int used = 0;
    template <typename T> int alloc(T *&d, size_t bytes) {
        if (used == P2S_N_SLOTS) return p2s_set_error(P2S_ERR_INVALID_ARG, "more than %d staging buffers in one call", P2S_N_SLOTS);
        Scratch &s = ctx->slot[used++];
        P2S_TRY(s.ensure(bytes > 16 ? bytes : 16));
        P2S_TRY(p2s_poison(ctx, s));
        d = (T *)s.p;
        return P2S_OK;
    }
    int up(const void *d, const void *h, size_t bytes) const {        // async, into a buffer (or a part of one) of this call
        if (bytes) HIP_TRY(hipMemcpyAsync((void *)d, h, bytes, hipMemcpyHostToDevice, ctx->stream));
        return P2S_OK;
    }
    template <typename T> int upload(T *&d, const void *h, size_t bytes) {
        P2S_TRY(alloc(d, bytes));
        return up(d, h, bytes);
    }
    int down(void *h, const void *d, size_t bytes) const {
        if (h && bytes) HIP_TRY(hipMemcpyAsync(h, d, bytes, hipMemcpyDeviceToHost, ctx->stream));
        return P2S_OK;
    }
    // A call that times itself: time_begin, its launches, time_end, its downloads, finish(P2S_TIMED_*).
    int time_begin() const {
        HIP_TRY(hipEventRecord(ctx->ev_stage[0], ctx->stream));
        return P2S_OK;
    }
    int time_end() const {
        HIP_TRY(hipEventRecord(ctx->ev_stage[1], ctx->stream));
        return P2S_OK;
    }
    int finish(int which) const {                                     // the stream's work is done when this returns
        HIP_TRY(hipStreamSynchronize(ctx->stream));
        HIP_TRY(hipEventElapsedTime(&ctx->kernel_ms[which], ctx->ev_stage[0], ctx->ev_stage[1]));
        return P2S_OK;
    }
};

// The body of every p2s_*_kernel_ms.  `who` names what has to run first: one entry point ("<who> has not run on this
// context"), or a phrase over several that carries its own negation ("neither a nor b", "none of a, b and c": "<who>
// has run on this context").
inline int p2s_kernel_ms_query(p2s_ctx *ctx, int which, const char *who, float *out) {
    if (!ctx || !out) return p2s_set_error(P2S_ERR_INVALID_ARG, "null argument");
    if (ctx->kernel_ms[which] < 0.0f)
        return p2s_set_error(P2S_ERR_INVALID_ARG, "%s has %srun on this context", who, strchr(who, ' ') ? "" : "not ");
    *out = ctx->kernel_ms[which];
    return P2S_OK;
}

// One block of arrays, each at a multiple of 16 bytes: add() hands out the offsets in bytes, a host block and a device
// block carved by the same calls match, and what is added first is a prefix that goes up as one copy.
struct Layout {
    size_t bytes = 0;
    size_t add(size_t n) {
        const size_t at = bytes;
        bytes += (n + 15) / 16 * 16;
        return at;
    }
};

// One Layout block of a call that runs the same code on the device or, ctx == NULL, on the host: a Stage buffer there, the
// host's own memory here.  put and get copy into and out of it (on the device async: what they name lives until wait());
// the timer does nothing on the host.
struct Block {
    Stage st;
    char *p = nullptr;
    std::vector<char> host;
    int alloc(size_t bytes) {
        if (st.ctx) return st.alloc(p, bytes);
        host.resize(bytes);
        p = host.data();
        return P2S_OK;
    }
    int put(void *d, const void *h, size_t bytes) const {
        if (st.ctx) return st.up(d, h, bytes);
        if (bytes) memcpy(d, h, bytes);
        return P2S_OK;
    }
    int put_wait(void *d, const void *h, size_t bytes) const {        // h may change when this returns
        P2S_TRY(put(d, h, bytes));
        return wait();
    }
    int get(void *h, const void *d, size_t bytes) const {             // a NULL h is skipped
        if (st.ctx) return st.down(h, d, bytes);
        if (h && bytes) memcpy(h, d, bytes);
        return P2S_OK;
    }
    int wait() const {
        if (st.ctx) HIP_TRY(hipStreamSynchronize(st.ctx->stream));
        return P2S_OK;
    }
    int time_begin() const { return st.ctx ? st.time_begin() : P2S_OK; }
    int time_end() const { return st.ctx ? st.time_end() : P2S_OK; }
    int finish(int which) const { return st.ctx ? st.finish(which) : P2S_OK; }
};

// The cameras of a per-camera analysis call (jitter, confidence, id_switch, track_select), frames back to back.
inline int p2s_check_n_cams(int32_t n_cams) {
    if (n_cams < 1 || n_cams > 65535) return p2s_set_error(P2S_ERR_INVALID_ARG, "n_cams=%d outside [1, 65535]", n_cams);
    return P2S_OK;
}

struct P2sFrames {
    int64_t frames = 0, max_frames = 0;
    // frame_off [n_cams + 1] from the cameras' frame counts, each min_frames (0 or 1) .. 2^31 - 1 and at most max_total
    // together.  frame_off is the caller's storage: it goes up, so it has to live until the stream is synchronized.
    int build(int32_t n_cams, const int64_t *n_frames, int min_frames, int64_t max_total, int64_t *frame_off) {
        frame_off[0] = 0;
        for (size_t c = 0; c < (size_t)n_cams; ++c) {
            if (n_frames[c] < min_frames || n_frames[c] >= ((int64_t)1 << 31))
                return p2s_set_error(P2S_ERR_INVALID_ARG, "camera %zu has %lld frames; expected %d .. 2^31 - 1", c, (long long)n_frames[c], min_frames);
            frame_off[c + 1] = frame_off[c] + n_frames[c];
            if (n_frames[c] > max_frames) max_frames = n_frames[c];
        }
        frames = frame_off[n_cams];
        if (frames > max_total) return p2s_set_error(P2S_ERR_INVALID_ARG, "%lld frames are too many", (long long)frames);
        return P2S_OK;
    }
    // person_off [frames + 1], the first person of every one of these frames, and the persons it indexes: their number.
    int persons(const int64_t *person_off, const void *persons, int64_t &N) const {
        if (person_off[0] != 0) return p2s_set_error(P2S_ERR_INVALID_ARG, "person_off must start at 0");
        for (int64_t f = 0; f < frames; ++f)
            if (person_off[f + 1] < person_off[f]) return p2s_set_error(P2S_ERR_INVALID_ARG, "person_off must not decrease (frame %lld)", (long long)f);
        N = person_off[frames];
        if (N >= ((int64_t)1 << 31)) return p2s_set_error(P2S_ERR_INVALID_ARG, "%lld persons are too many", (long long)N);
        if (N > 0 && !persons) return p2s_set_error(P2S_ERR_INVALID_ARG, "null argument");
        return P2S_OK;
    }
};

#endif
