// p2s_api.hip -- the part of the extern "C" boundary declared in include/p2s.h that belongs to no stage: the life of
// the per-GPU context (p2s_ctx.h), its calibration, tuning, counters and timing, and the error slot.  The entry points
// of every stage live at the end of the file that holds its kernels (p2s_tri.hip, p2s_assoc.hip, p2s_filter.hip,
// p2s_sync.hip, p2s_reproj.hip, p2s_jitter.hip).  No torch types, no exceptions across the ABI.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <cstdlib>
#include <string>
#include <vector>

#include "p2s_ctx.h"

namespace {

thread_local std::string g_last_error;

constexpr size_t kStatBytes = sizeof(unsigned long long) * P2S_STAT_SHARDS * P2S_STAT_STRIDE;

void fill_binom(uint32_t *b) {
    for (int n = 0; n < 33; ++n)
        for (int k = 0; k < 33; ++k) {
            unsigned long long v;
            if (k > n) v = 0;
            else if (k == 0 || k == n) v = 1;
            else v = (unsigned long long)b[(n - 1) * 33 + k - 1] + b[(n - 1) * 33 + k];
            b[n * 33 + k] = (uint32_t)std::min<unsigned long long>(v, 0xfffffffeull);
        }
}

}  // namespace

// p2s_error.h: the error slot of every translation unit.
int p2s_set_error(int code, const char *fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    g_last_error = buf;
    return code;
}

extern "C" {

int p2s_version(void) { return 100; }

const char *p2s_last_error(void) { return g_last_error.c_str(); }

int p2s_device_count(int *count) {
    if (!count) return p2s_set_error(P2S_ERR_INVALID_ARG, "null count");
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess) {
        (void)hipGetLastError();
        n = 0;
    }
    *count = n;
    return P2S_OK;
}

// everything p2s_create allocates; what a failed step leaves behind is p2s_destroy's to free
static int init_ctx(p2s_ctx *c) {
    HIP_TRY(hipStreamCreateWithFlags(&c->own_stream, hipStreamNonBlocking));
    c->stream = c->own_stream;
    HIP_TRY(hipMalloc((void **)&c->d_cams, sizeof(P2sCam) * P2S_MAX_CAMS));
    HIP_TRY(hipMalloc((void **)&c->d_binom, sizeof(uint32_t) * 33 * 33));
    fill_binom(c->binom);
    HIP_TRY(hipMemcpy(c->d_binom, c->binom, sizeof c->binom, hipMemcpyHostToDevice));
    HIP_TRY(hipMalloc((void **)&c->d_stats, kStatBytes));
    HIP_TRY(hipMemset(c->d_stats, 0, kStatBytes));
    HIP_TRY(hipMalloc((void **)&c->d_assoc_stats, kStatBytes));
    HIP_TRY(hipMemset(c->d_assoc_stats, 0, kStatBytes));
    HIP_TRY(hipEventCreate(&c->ev0));
    HIP_TRY(hipEventCreate(&c->ev1));
    HIP_TRY(hipEventCreate(&c->ev_stage[0]));
    HIP_TRY(hipEventCreate(&c->ev_stage[1]));
    HIP_TRY(hipStreamCreateWithFlags(&c->side_stream, hipStreamNonBlocking));
    for (int i = 0; i < 2; ++i) {
        HIP_TRY(hipEventCreateWithFlags(&c->ev_k1[i], hipEventDisableTiming));
        HIP_TRY(hipEventCreateWithFlags(&c->ev_k2[i], hipEventDisableTiming));
    }
    return P2S_OK;
}

int p2s_create(int device_id, p2s_ctx **out) {
    if (!out) return p2s_set_error(P2S_ERR_INVALID_ARG, "null out");
    *out = nullptr;
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n <= 0) {
        (void)hipGetLastError();
        return p2s_set_error(P2S_ERR_NO_DEVICE, "no HIP device visible: the triangulation engine has no CPU fallback");
    }
    if (device_id < 0 || device_id >= n) return p2s_set_error(P2S_ERR_INVALID_ARG, "device %d out of range (%d devices)", device_id, n);
    HIP_TRY(hipSetDevice(device_id));
    p2s_ctx *c = new p2s_ctx();
    c->device = device_id;
    const int rc = init_ctx(c);
    if (rc != P2S_OK) {
        p2s_destroy(c);           // leaves the error text alone
        return rc;
    }
    *out = c;
    return P2S_OK;
}

int p2s_destroy(p2s_ctx *ctx) {
    if (!ctx) return P2S_OK;
    (void)hipSetDevice(ctx->device);
    (void)hipStreamSynchronize(ctx->stream);
    for (Scratch &s : ctx->slot) s.release();
    ctx->wl_rec.release(); ctx->wl_count.release();
    ctx->deep_entries.release(); ctx->deep_ctl.release(); ctx->deep_sched.release(); ctx->deep_partials.release();
    ctx->frames_sub.release(); ctx->frames_plan.release();
    if (ctx->d_cams) (void)hipFree(ctx->d_cams);
    if (ctx->d_binom) (void)hipFree(ctx->d_binom);
    if (ctx->d_stats) (void)hipFree(ctx->d_stats);
    if (ctx->d_assoc_stats) (void)hipFree(ctx->d_assoc_stats);
    if (ctx->d_sub_tab) (void)hipFree(ctx->d_sub_tab);
    if (ctx->d_sub_off) (void)hipFree(ctx->d_sub_off);
    if (ctx->ev0) (void)hipEventDestroy(ctx->ev0);
    if (ctx->ev1) (void)hipEventDestroy(ctx->ev1);
    for (int i = 0; i < 2; ++i)
        if (ctx->ev_stage[i]) (void)hipEventDestroy(ctx->ev_stage[i]);
    if (ctx->own_stream) (void)hipStreamDestroy(ctx->own_stream);
    if (ctx->side_stream) { (void)hipStreamSynchronize(ctx->side_stream); (void)hipStreamDestroy(ctx->side_stream); }
    for (int i = 0; i < 2; ++i) {
        if (ctx->ev_k1[i]) (void)hipEventDestroy(ctx->ev_k1[i]);
        if (ctx->ev_k2[i]) (void)hipEventDestroy(ctx->ev_k2[i]);
    }
    delete ctx;
    return P2S_OK;
}

int p2s_set_stream(p2s_ctx *ctx, void *hip_stream) {
    if (!ctx) return p2s_set_error(P2S_ERR_INVALID_ARG, "null context");
    ctx->stream = (hipStream_t)hip_stream;   // NULL = HIP's default stream
    return P2S_OK;
}

int p2s_synchronize(p2s_ctx *ctx) {
    if (!ctx) return p2s_set_error(P2S_ERR_INVALID_ARG, "null context");
    HIP_TRY(hipSetDevice(ctx->device));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    return P2S_OK;
}

int p2s_set_calibration(p2s_ctx *ctx, int32_t n_cams, const double *P, const double *Kmat, const double *dist,
                        const double *Rmat, const double *T, const double *newK) {
    if (!ctx) return p2s_set_error(P2S_ERR_INVALID_ARG, "null context");
    if (n_cams < 1 || n_cams > P2S_MAX_CAMS) return p2s_set_error(P2S_ERR_INVALID_ARG, "n_cams=%d outside [1, %d]", n_cams, P2S_MAX_CAMS);
    if (!P) return p2s_set_error(P2S_ERR_INVALID_ARG, "null P");
    const bool full = Kmat && dist && Rmat && T && newK;
    if (!full && (Kmat || dist || Rmat || T || newK))
        return p2s_set_error(P2S_ERR_INVALID_ARG, "K, dist, R, T and optim_K must be given together or all be NULL");
    std::vector<P2sCam> cams(P2S_MAX_CAMS);
    std::memset(cams.data(), 0, sizeof(P2sCam) * P2S_MAX_CAMS);
    for (int c = 0; c < n_cams; ++c) {
        P2sCam &cam = cams[c];
        std::memcpy(cam.P, P + 12 * c, sizeof cam.P);
        for (int i = 0; i < 12; ++i) cam.Pf[i] = (float)cam.P[i];
        if (!full) continue;
        const double *K = Kmat + 9 * c;
        cam.fx = K[0]; cam.fy = K[4]; cam.cx = K[2]; cam.cy = K[5];
        cam.ifx = 1.0 / cam.fx; cam.ify = 1.0 / cam.fy;
        std::memcpy(cam.k, dist + 5 * c, sizeof cam.k);
        std::memcpy(cam.R, Rmat + 9 * c, sizeof cam.R);
        std::memcpy(cam.T, T + 3 * c, sizeof cam.T);
        std::memcpy(cam.nk, newK + 9 * c, sizeof cam.nk);
        // inverse of K (general 3x3, as numpy.linalg.inv at common.py:282) by cofactors
        const double a = K[0], b = K[1], cc = K[2], d = K[3], e = K[4], f = K[5], g = K[6], h = K[7], i = K[8];
        const double det = a * (e * i - f * h) - b * (d * i - f * g) + cc * (d * h - e * g);
        const double id = 1.0 / det;
        cam.iK[0] = (e * i - f * h) * id; cam.iK[1] = (cc * h - b * i) * id; cam.iK[2] = (b * f - cc * e) * id;
        cam.iK[3] = (f * g - d * i) * id; cam.iK[4] = (a * i - cc * g) * id; cam.iK[5] = (cc * d - a * f) * id;
        cam.iK[6] = (d * h - e * g) * id; cam.iK[7] = (b * g - a * h) * id; cam.iK[8] = (a * e - b * d) * id;
        for (int r = 0; r < 3; ++r)
            cam.center[r] = -(cam.R[0 * 3 + r] * cam.T[0] + cam.R[1 * 3 + r] * cam.T[1] + cam.R[2 * 3 + r] * cam.T[2]);
    }
    HIP_TRY(hipSetDevice(ctx->device));
    HIP_TRY(hipMemcpy(ctx->d_cams, cams.data(), sizeof(P2sCam) * P2S_MAX_CAMS, hipMemcpyHostToDevice));
    // every subset of the n_cams cameras as a bit mask, level by level in itertools.combinations order
    // (triangulation.py:411): what the fused kernel's lanes index by (level, rank); 2^C entries, C <= 16
    if (n_cams <= 16) {
        std::vector<uint16_t> tab;
        std::vector<uint32_t> off;
        p2s_subset_table(n_cams, tab, off);
        if (!ctx->d_sub_tab) HIP_TRY(hipMalloc((void **)&ctx->d_sub_tab, sizeof(uint16_t) << 16));
        if (!ctx->d_sub_off) HIP_TRY(hipMalloc((void **)&ctx->d_sub_off, sizeof(uint32_t) * 18));
        HIP_TRY(hipMemcpy(ctx->d_sub_tab, tab.data(), tab.size() * sizeof(uint16_t), hipMemcpyHostToDevice));
        HIP_TRY(hipMemcpy(ctx->d_sub_off, off.data(), off.size() * sizeof(uint32_t), hipMemcpyHostToDevice));
    }
    ctx->n_cams = n_cams;
    ctx->full_calib = full;
    return P2S_OK;
}

// sum of the shards of one counter block (d_stats or d_assoc_stats) after the context's work has finished
static int read_stats(p2s_ctx *ctx, unsigned long long *d, int n, uint64_t *out, int32_t reset) {
    if (!ctx || !out) return p2s_set_error(P2S_ERR_INVALID_ARG, "null argument");
    HIP_TRY(hipSetDevice(ctx->device));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    if (ctx->side_stream) HIP_TRY(hipStreamSynchronize(ctx->side_stream));
    std::vector<unsigned long long> h((size_t)P2S_STAT_SHARDS * P2S_STAT_STRIDE);
    HIP_TRY(hipMemcpy(h.data(), d, kStatBytes, hipMemcpyDeviceToHost));
    for (int i = 0; i < n; ++i) {
        out[i] = 0;
        for (int sh = 0; sh < P2S_STAT_SHARDS; ++sh) out[i] += h[(size_t)sh * P2S_STAT_STRIDE + i];
    }
    if (reset) HIP_TRY(hipMemset(d, 0, kStatBytes));
    return P2S_OK;
}

int p2s_get_tri_stats(p2s_ctx *ctx, uint64_t *out, int32_t reset) {
    return read_stats(ctx, ctx ? ctx->d_stats : nullptr, P2S_N_STATS, out, reset);
}

int p2s_get_assoc_stats(p2s_ctx *ctx, uint64_t *out, int32_t reset) {
    return read_stats(ctx, ctx ? ctx->d_assoc_stats : nullptr, 4, out, reset);
}

int p2s_set_tuning(p2s_ctx *ctx, int32_t key, int32_t value) {
    if (!ctx) return p2s_set_error(P2S_ERR_INVALID_ARG, "null context");
    switch (key) {
    case P2S_TUNE_TRI_PATH:
        if (value != P2S_TRI_PATH_AUTO && value != P2S_TRI_PATH_WORKLIST && value != P2S_TRI_PATH_ONE_TILE &&
            value != P2S_TRI_PATH_POOLED && value != P2S_TRI_PATH_TWO_TILES)
            return p2s_set_error(P2S_ERR_INVALID_ARG, "unknown triangulation path %d", value);
        ctx->tri_path = value;
        return P2S_OK;
    case P2S_TUNE_FORCE_TILED: ctx->force_tiled = value ? 1 : 0; return P2S_OK;
    case P2S_TUNE_NO_OVERLAP: ctx->no_overlap = value ? 1 : 0; return P2S_OK;
    case P2S_TUNE_SEARCH_JOB:
        if (value != 0 && (value < 8 || value > 64)) return p2s_set_error(P2S_ERR_INVALID_ARG, "search job size %d outside [8, 64]", value);
        ctx->job = value;
        return P2S_OK;
    case P2S_TUNE_MAX_SUBSETS:
        if (value < 1) return p2s_set_error(P2S_ERR_INVALID_ARG, "max subsets per level must be >= 1");
        ctx->max_subsets = (uint32_t)value;
        return P2S_OK;
    case P2S_TUNE_DEEP_MIN_SUBSETS:
        if (value < 0) return p2s_set_error(P2S_ERR_INVALID_ARG, "deep-level threshold must be >= 0");
        ctx->deep_min_subsets = (uint32_t)value;
        return P2S_OK;
    case P2S_TUNE_DEEP_PRUNE: ctx->deep_prune = value ? 1 : 0; return P2S_OK;
    case P2S_TUNE_POOL_SINGLES_PCT:
        if (value < 0 || value > 100) return p2s_set_error(P2S_ERR_INVALID_ARG, "percentage outside [0, 100]");
        ctx->pool_singles_pct = value;
        return P2S_OK;
    case P2S_TUNE_SCREEN: ctx->screen = value ? 1 : 0; return P2S_OK;
    case P2S_TUNE_POOL_TILES:
        if (value < 2 || value > 6) return p2s_set_error(P2S_ERR_INVALID_ARG, "tiles per wave outside [2, 6]");
        ctx->pool_tiles = value;
        return P2S_OK;
    case P2S_TUNE_GAPS_WORKSPACE_KB:
        if (value < 1) return p2s_set_error(P2S_ERR_INVALID_ARG, "workspace cap must be >= 1 KiB");
        ctx->gaps_ws_kb = value;
        return P2S_OK;
    case P2S_TUNE_POISON_STAGING:
        if (value < -1 || value > 255) return p2s_set_error(P2S_ERR_INVALID_ARG, "poison byte %d outside -1 (off), 0 .. 255", value);
        ctx->poison = value;
        return P2S_OK;
    case P2S_TUNE_ASSOC_FORM:
        if (value != P2S_ASSOC_FORM_AUTO && value != P2S_ASSOC_FORM_GENERAL)
            return p2s_set_error(P2S_ERR_INVALID_ARG, "unknown association kernel form %d", value);
        ctx->assoc_form = value;
        return P2S_OK;
    case P2S_TUNE_DIAG_MODE:
#ifdef P2S_DIAG
        ctx->debug_mode = value;
        return P2S_OK;
#else
        return p2s_set_error(P2S_ERR_INVALID_ARG, "kernel diagnostics need a -DP2S_DIAG build of the library");
#endif
    default: return p2s_set_error(P2S_ERR_INVALID_ARG, "unknown tuning key %d", key);
    }
}

int p2s_timing_begin(p2s_ctx *ctx) {
    if (!ctx) return p2s_set_error(P2S_ERR_INVALID_ARG, "null context");
    HIP_TRY(hipSetDevice(ctx->device));
    HIP_TRY(hipEventRecord(ctx->ev0, ctx->stream));
    return P2S_OK;
}

int p2s_timing_end(p2s_ctx *ctx, float *elapsed_ms) {
    if (!ctx || !elapsed_ms) return p2s_set_error(P2S_ERR_INVALID_ARG, "null argument");
    HIP_TRY(hipSetDevice(ctx->device));
    HIP_TRY(hipEventRecord(ctx->ev1, ctx->stream));
    HIP_TRY(hipEventSynchronize(ctx->ev1));
    HIP_TRY(hipEventElapsedTime(elapsed_ms, ctx->ev0, ctx->ev1));
    return P2S_OK;
}

}  // extern "C"
