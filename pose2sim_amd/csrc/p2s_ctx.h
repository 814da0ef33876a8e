// p2s_ctx.h -- the per-GPU context behind include/p2s.h's opaque p2s_ctx, and what the C-ABI entry points (p2s_api.hip
// and the tail of every stage's kernel file) share to use it: HIP_TRY / P2S_TRY, the grow-only Scratch buffer, and
// Stage, which hands a *_host call its device buffers.
#ifndef P2S_CTX_H
#define P2S_CTX_H

#include <hip/hip_runtime.h>

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
    float reproj_kernel_ms = -1.0f;                  // p2s_reproject_kernel_ms: the last call's kernel time
    float jitter_kernel_ms = -1.0f;                  // p2s_jitter_kernel_ms
    float confidence_kernel_ms = -1.0f;              // p2s_confidence_kernel_ms
    float id_switch_kernel_ms = -1.0f;               // p2s_id_switch_kernel_ms
    float gait_kernel_ms = -1.0f;                    // p2s_gait_kernel_ms
    float measure_kernel_ms = -1.0f;                 // p2s_measure_kernel_ms
    float track_select_kernel_ms = -1.0f;            // p2s_track_select_kernel_ms
    hipStream_t side_stream = nullptr;               // search kernels run here, beside the next chunk's streaming pass
    hipEvent_t ev_k1[2] = {nullptr, nullptr}, ev_k2[2] = {nullptr, nullptr};
    Scratch slot[P2S_N_SLOTS];                       // staging of the *_host calls (Stage): no role, no owner between calls
    Scratch wl_rec, wl_count;
    Scratch deep_entries, deep_ctl, deep_sched, deep_partials;   // deep levels of the search (p2s_tri_deep.hip)
    uint32_t deep_min_subsets = P2S_DEEP_MIN_SUBSETS;            // 0 = every level stays in the search kernel's wave
    unsigned long long *d_stats = nullptr;           // P2S_N_STATS counters (p2s_get_tri_stats)
    unsigned long long *d_assoc_stats = nullptr;     // 4 counters (p2s_get_assoc_stats)
    uint16_t *d_sub_tab = nullptr;                   // camera subsets by level (fused kernel), built with the calibration
    uint32_t *d_sub_off = nullptr;
    // p2s_set_tuning: experiments and tests only, never read from the environment
    int tri_path = P2S_TRI_PATH_AUTO;
    int force_tiled = 0, no_overlap = 0, job = 0;
    uint32_t max_subsets = P2S_MAX_SUBSETS_PER_LEVEL;
    int debug_mode = 0;                              // honoured by a -DP2S_DIAG build only
    int assoc_form = P2S_ASSOC_FORM_AUTO;
    int deep_prune = 1;                              // p2s_tri_deep.hip: exact pruning of the deep levels' evaluations
    int pool_singles_pct = 8;                        // p2s_tri_fused.hip: share of the tiles that the last workgroups take one at a time
    int screen = 1;                                  // p2s_tri_pool.hip: fp32 screen of the camera-subset candidates
    int pool_tiles = 5;                              // p2s_tri_pool.hip: tiles a wave streams before it searches their pooled failures (2..6)
};

// Device buffers of one *_host call.  The i-th buffer the call asks for is ctx->slot[i]: two pointers of one call never
// share a slot, a slot only grows (hipFree / hipMalloc on growth alone), and what an earlier call left in it is garbage.
// A buffer is never NULL (at least 16 bytes); copies of 0 bytes and downloads to a NULL host pointer are skipped.
struct Stage {
    p2s_ctx *ctx;
    int used = 0;
    template <typename T> int alloc(T *&d, size_t bytes) {
        if (used == P2S_N_SLOTS) return p2s_set_error(P2S_ERR_INVALID_ARG, "more than %d staging buffers in one call", P2S_N_SLOTS);
        Scratch &s = ctx->slot[used++];
        P2S_TRY(s.ensure(bytes > 16 ? bytes : 16));
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
};

#endif
