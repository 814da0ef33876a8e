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

#include "p2s_internal.h"
#include "p2s_tri_dev.h"      // project_distorted: the cv2.projectPoints restatement the triangulation kernels use

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

hipError_t p2s_launch_reproject(const P2sReprojArgs &a, hipStream_t s) {
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
