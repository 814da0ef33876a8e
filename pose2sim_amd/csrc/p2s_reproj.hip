// p2s_reproj.hip -- 3D markers onto the image planes: the per (frame, marker, camera) arithmetic of
// Utilities/reproj_from_trc_calib.py:446-475 (reprojection() or cv2.projectPoints, np.round(decimals=1), the
// in-image test on the rounded values).
//
// A memory-bound element-wise kernel: one lane per (frame, marker) unit, the camera loop inside so that the unit's
// point is read once (24 B); the camera constants are wave-uniform (scalar loads) unless the cameras change per frame;
// consecutive lanes store consecutive 16-byte (x, y) pairs into each camera plane.  Traffic per unit: 24 B read,
// 16 B per camera written (32 B with the unrounded plane).  Nothing is reused, so nothing is staged in LDS.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <cstring>
#include <vector>

#include "p2s_ctx.h"
#include "p2s_tri_dev.h"      // project_distorted: the cv2.projectPoints restatement the triangulation kernels use

// 3D markers onto the image planes (Utilities/reproj_from_trc_calib.py:446-475)
struct P2sReprojArgs {
    const double *Q;             // [n_frames][K][3], Z-up (X, Y, Z); NaN = missing
    const double *P;             // plain mode: [C][Fp][12]
    const P2sCam *cams;          // distorted mode: [C] (R, T, fx, fy, cx, cy, k read); NULL = plain mode
    const double *sizes;         // [C][2] width, height
    double *uv_raw;              // [C][n_frames][K][2] unrounded pixels, or NULL
    double *uv;                  // [C][n_frames][K][2] rounded to one decimal, NaN outside the image
    int64_t n_units;             // n_frames * K
    int64_t Fp;                  // 1, or n_frames: one projection matrix per frame
    int32_t K, C;
};

namespace {

// Read-only for the whole launch and indexed by the camera alone: through the constant address space these become
// scalar loads and SGPR operands, like the cameras of the triangulation kernels (cam_cptr).
typedef const __attribute__((address_space(4))) double *const_dptr;

// np.round(v, decimals=1) = rint(v * 10) / 10 (ties to even), then the reference's mask: both NaN unless
// 0 <= x < width and 0 <= y < height on the ROUNDED values.  NaN and infinities fail the comparisons.
__device__ __forceinline__ double2 round_and_mask(double u, double v, double w, double h) {
    const double ru = rint(u * 10.0) / 10.0, rv = rint(v * 10.0) / 10.0;
    const bool ok = (ru >= 0.0) && (ru < w) && (rv >= 0.0) && (rv < h);
    return ok ? make_double2(ru, rv) : make_double2(d_nan(), d_nan());
}

// reprojection() (reproj_from_trc_calib.py:183-201): x = P0.q / P2.q, y = P1.q / P2.q with q = (X, Y, Z, 1).  PT is a
// constant-address-space pointer (static cameras) or a global one (one matrix per frame).
template <typename PT>
__device__ __forceinline__ void project_pinhole(PT P, const double q[3], double &x, double &y) {
    const double n0 = fma(P[0], q[0], fma(P[1], q[1], fma(P[2], q[2], P[3])));
    const double n1 = fma(P[4], q[0], fma(P[5], q[1], fma(P[6], q[2], P[7])));
    const double z = fma(P[8], q[0], fma(P[9], q[1], fma(P[10], q[2], P[11])));
    x = n0 / z;
    y = n1 / z;
}

template <int MODE>   // 0: plain, one P per camera; 1: plain, one P per camera and frame; 2: distorted, static cameras
__global__ void __launch_bounds__(256) p2s_reproject_kernel(const P2sReprojArgs a) {
    const int64_t u = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (u >= a.n_units) return;
    const double q[3] = {a.Q[3 * u], a.Q[3 * u + 1], a.Q[3 * u + 2]};
    const int64_t f = u / a.K;
    cam_cptr cams = (cam_cptr)a.cams;
    const_dptr sizes = (const_dptr)a.sizes;
    for (int c = 0; c < a.C; ++c) {
        double x, y;
        if (MODE == 2) {
            project_distorted(cams + c, q, x, y);
        } else if (MODE == 0) {
            project_pinhole((const_dptr)a.P + (int64_t)c * 12, q, x, y);
        } else {
            project_pinhole(a.P + ((int64_t)c * a.Fp + f) * 12, q, x, y);
        }
        const int64_t o = (int64_t)c * a.n_units + u;
        if (a.uv_raw) reinterpret_cast<double2 *>(a.uv_raw)[o] = make_double2(x, y);
        reinterpret_cast<double2 *>(a.uv)[o] = round_and_mask(x, y, sizes[2 * c], sizes[2 * c + 1]);
    }
}

}  // namespace

static hipError_t p2s_launch_reproject(const P2sReprojArgs &a, hipStream_t s) {
    if (a.n_units == 0 || a.C == 0) return hipSuccess;
    const int64_t blocks = (a.n_units + 255) / 256;
    if (blocks > 0x7fffffffLL) return hipErrorInvalidValue;
    const dim3 grid((unsigned)blocks), block(256);
    if (a.cams)
        hipLaunchKernelGGL((p2s_reproject_kernel<2>), grid, block, 0, s, a);
    else if (a.Fp != 1)
        hipLaunchKernelGGL((p2s_reproject_kernel<1>), grid, block, 0, s, a);
    else
        hipLaunchKernelGGL((p2s_reproject_kernel<0>), grid, block, 0, s, a);
    return hipGetLastError();
}

// ---- C-ABI entry points (include/p2s.h) ----------------------------------------------------------------------------
extern "C" {

int p2s_reproject_host(p2s_ctx *ctx, int64_t n_frames, int32_t n_markers, const double *Q, int32_t n_cams, int64_t n_frames_p,
                       const double *P, const double *Kmat, const double *dist, const double *Rmat, const double *T,
                       const double *sizes, int32_t flags, double *uv_raw, double *uv) {
    if (!ctx) return p2s_set_error(P2S_ERR_INVALID_ARG, "null context");
    if (n_frames < 0 || n_markers < 0) return p2s_set_error(P2S_ERR_INVALID_ARG, "bad shape: %lld frames, %d markers", (long long)n_frames, n_markers);
    if (n_cams < 1 || n_cams > P2S_MAX_CAMS) return p2s_set_error(P2S_ERR_INVALID_ARG, "n_cams=%d outside [1, %d]", n_cams, P2S_MAX_CAMS);
    if (flags & ~P2S_REPROJ_DISTORTED) return p2s_set_error(P2S_ERR_INVALID_ARG, "unknown flags 0x%x", flags);
    const bool distorted = (flags & P2S_REPROJ_DISTORTED) != 0;
    if (distorted) {
        if (n_frames_p != 1)
            return p2s_set_error(P2S_ERR_INVALID_ARG, "distorted projection takes static cameras: n_frames_p=%lld, expected 1", (long long)n_frames_p);
        if (!Kmat || !dist || !Rmat || !T) return p2s_set_error(P2S_ERR_INVALID_ARG, "distorted projection needs K, dist, R and T");
    } else {
        if (n_frames_p != 1 && n_frames_p != n_frames)
            return p2s_set_error(P2S_ERR_INVALID_ARG, "n_frames_p=%lld is neither 1 nor n_frames=%lld", (long long)n_frames_p, (long long)n_frames);
        if (!P) return p2s_set_error(P2S_ERR_INVALID_ARG, "null P");
    }
    if (!sizes) return p2s_set_error(P2S_ERR_INVALID_ARG, "null sizes");
    if (!uv) return p2s_set_error(P2S_ERR_INVALID_ARG, "null uv");
    const int64_t n_units = n_frames * (int64_t)n_markers;
    ctx->kernel_ms[P2S_TIMED_REPROJ] = 0.0f;                      // nothing to project: the call has run, in no time
    if (n_units == 0) return P2S_OK;
    if (!Q) return p2s_set_error(P2S_ERR_INVALID_ARG, "null Q");
    if (n_units > ((int64_t)1 << 38) / n_cams) return p2s_set_error(P2S_ERR_INVALID_ARG, "%lld units x %d cameras is too large", (long long)n_units, n_cams);
    const size_t q_b = (size_t)n_units * 3 * sizeof(double);
    const size_t out_b = (size_t)n_units * n_cams * 2 * sizeof(double);
    HIP_TRY(hipSetDevice(ctx->device));
    P2sReprojArgs a{};
    a.n_units = n_units; a.Fp = n_frames_p; a.K = n_markers; a.C = n_cams;
    Stage st{ctx};
    std::vector<P2sCam> cams;
    if (distorted) {
        cams.resize((size_t)n_cams);
        std::memset(cams.data(), 0, sizeof(P2sCam) * (size_t)n_cams);
        for (int c = 0; c < n_cams; ++c) {
            P2sCam &cam = cams[(size_t)c];
            const double *K = Kmat + 9 * c;
            cam.fx = K[0]; cam.fy = K[4]; cam.cx = K[2]; cam.cy = K[5];     // the skew term is ignored, as in cv2.projectPoints
            std::memcpy(cam.k, dist + 5 * c, sizeof cam.k);
            std::memcpy(cam.R, Rmat + 9 * c, sizeof cam.R);
            std::memcpy(cam.T, T + 3 * c, sizeof cam.T);
        }
        P2S_TRY(st.upload(a.cams, cams.data(), sizeof(P2sCam) * (size_t)n_cams));
    } else {
        P2S_TRY(st.upload(a.P, P, (size_t)n_cams * n_frames_p * 12 * sizeof(double)));
    }
    P2S_TRY(st.upload(a.sizes, sizes, (size_t)n_cams * 2 * sizeof(double)));
    P2S_TRY(st.upload(a.Q, Q, q_b));
    P2S_TRY(st.alloc(a.uv, out_b));
    if (uv_raw) P2S_TRY(st.alloc(a.uv_raw, out_b));
    P2S_TRY(st.time_begin());
    HIP_TRY(p2s_launch_reproject(a, ctx->stream));
    P2S_TRY(st.time_end());
    P2S_TRY(st.down(uv, a.uv, out_b));
    P2S_TRY(st.down(uv_raw, a.uv_raw, out_b));
    return st.finish(P2S_TIMED_REPROJ);                  // `cams` is pageable host memory: alive until here
}

int p2s_reproject_kernel_ms(p2s_ctx *ctx, float *elapsed_ms) { return p2s_kernel_ms_query(ctx, P2S_TIMED_REPROJ, "p2s_reproject_host", elapsed_ms); }

}  // extern "C"
