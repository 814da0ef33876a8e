"""scipy restatement of Engine.refine_extrinsics (include/p2s.h): the live reference of
tests/test_refine_gpu.py and tests/test_refine_host.py, and the builder of their cases.  Test infrastructure, not a
fallback: the package never imports it.

The cost is the contract's: weights s = l for l >= lik_thr and finite (x, y, l), points with fewer than min_cams such
observations or a NaN start dropped, residuals s (proj - obs) per component, scipy's loss='huber' with f_scale = delta.
least_squares minimises it over the free camera parameters (rotation vectors and translations of the cameras 1 .. C - 1
without the held coordinate of camera 1) and all kept points, from the same start, with its own finite-difference
Jacobian: nothing here shares a derivative with the kernels."""
import numpy as np
from scipy.optimize import least_squares

import rigs
from pose2sim_amd import cvmath, synth


# The bounds of the tests: 100 x the worst figure of its kind measured on the MI355X over the cases of
# tests/test_refine_gpu.py (DESIGN.md 4.21 lists them; the library's host path in tests/test_refine_host.py stays inside
# the same figures), and never beyond what makes a result another minimum (a relative cost difference of 1e-6) or no
# recovery (1e-6 m at zero noise).  The margin covers other seeds and another summation order.
COST_REL_BOUND = 5e-12      # |cost - cost_oracle| / cost_oracle; worst measured 4.7e-14 (ring, 2 cameras)
CENTRE_BOUND = 5e-5         # m, camera centres against the oracle's; worst measured 4.9e-7 (stadium: where the oracle stops)
POINT_BOUND = 2.5e-5        # m, kept points against the oracle's; worst measured 2.5e-7 (overhead)
ZERO_NOISE_BOUND = 8e-13    # m, camera centres and points against the truth at zero noise; worst measured 8.0e-15
assert COST_REL_BOUND <= 1e-6 and ZERO_NOISE_BOUND <= 1e-6


def held_coord(R, t):
    """argmax_j |(t1 - R1 R0^T t0)_j|, the first index on ties."""
    R, t = np.asarray(R, dtype=np.float64).reshape(-1, 3, 3), np.asarray(t, dtype=np.float64).reshape(-1, 3)
    b = t[1] - R[1] @ R[0].T @ t[0]
    return int(np.argmax(np.abs(b)))


def centres(R, t):
    R, t = np.asarray(R, dtype=np.float64).reshape(-1, 3, 3), np.asarray(t, dtype=np.float64).reshape(-1, 3)
    return -np.einsum('cji,cj->ci', R, t)


def as_points(xyl):
    """[F..., C, K, 3] -> [N = prod(F...) * K][C][3]."""
    xyl = np.asarray(xyl, dtype=np.float64)
    Cn, Kn = xyl.shape[-3], xyl.shape[-2]
    return np.moveaxis(xyl.reshape(-1, Cn, Kn, 3), 1, 2).reshape(-1, Cn, 3)


def weights(xyl, X0, lik_thr=0.3, min_cams=2):
    """s [N][C] and kept [N] of the contract."""
    o = as_points(xyl)
    with np.errstate(invalid='ignore'):
        ok = np.isfinite(o).all(axis=-1) & (o[..., 2] >= lik_thr) & (o[..., 2] > 0)
    s = np.where(ok, o[..., 2], 0.0)
    kept = (ok.sum(axis=1) >= max(2, min_cams)) & ~np.isnan(np.asarray(X0, dtype=np.float64).reshape(-1, 3)).any(axis=1)
    s[~kept] = 0.0
    return s, kept


def project(K, R, t, X):
    """[C][N][2] pinhole pixels of X [N][3] (no skew: u = fx x / z + cx) and the depths [C][N]."""
    Xc = np.einsum('cij,nj->cni', R, X) + t[:, None, :]
    z = Xc[..., 2]
    uv = np.stack([K[:, 0, 0, None] * Xc[..., 0] / z + K[:, 0, 2, None], K[:, 1, 1, None] * Xc[..., 1] / z + K[:, 1, 2, None]], axis=-1)
    return uv, z


def residuals(xyl, s, K, R, t, X):
    """e [N][C][2] = s (proj - obs), 0 where s = 0."""
    o = as_points(xyl)
    uv, _ = project(K, R, t, np.nan_to_num(X))
    e = np.swapaxes(uv, 0, 1) - np.nan_to_num(o[..., :2])
    return np.where(s[..., None] > 0, s[..., None] * e, 0.0)


def huber_cost(e, delta):
    """sum of delta^2 rho((e / delta)^2), rho(z) = z for z <= 1, else 2 sqrt(z) - 1."""
    z = (np.asarray(e) / delta) ** 2
    return float(np.sum(delta ** 2 * np.where(z <= 1, z, 2 * np.sqrt(z) - 1)))


def cost(xyl, K, R, t, X, X0=None, lik_thr=0.3, delta=3.0, min_cams=2):
    K, R, t = (np.asarray(v, dtype=np.float64) for v in (K, R, t))
    s, _ = weights(xyl, X if X0 is None else X0, lik_thr, min_cams)
    return huber_cost(residuals(xyl, s, K, R, t, np.asarray(X, dtype=np.float64).reshape(-1, 3)), delta)


def refine(xyl, K, R, t, X0, lik_thr=0.3, delta=3.0, min_cams=2, tol=1e-14, max_nfev=4000):
    """-> (R [C][3][3], t [C][3], X [N][3] with NaN for dropped points, cost, result of least_squares)."""
    K, R, t = (np.array(v, dtype=np.float64) for v in (K, R, t))
    R, t = R.reshape(-1, 3, 3), t.reshape(-1, 3)
    X0 = np.array(X0, dtype=np.float64).reshape(-1, 3)
    Cn = len(K)
    s, kept = weights(xyl, X0, lik_thr, min_cams)
    o = as_points(xyl)
    ok, sk = np.nan_to_num(o[kept][..., :2]), s[kept]
    j = held_coord(R, t)
    free = np.ones((Cn, 6), dtype=bool)
    free[0] = False
    free[1, 3 + j] = False
    cam0 = np.concatenate([np.stack([cvmath.rodrigues_from_matrix(R[c]) for c in range(Cn)]), t], axis=1)

    def unpack(p):
        cam = cam0.copy()
        cam[free] = p[:free.sum()]
        Rm = np.stack([cvmath.rodrigues(cam[c, :3]) for c in range(Cn)])
        Rm[0] = R[0]
        return Rm, cam[:, 3:], p[free.sum():].reshape(-1, 3)

    def fun(p):
        Rm, tm, X = unpack(p)
        uv, _ = project(K, Rm, tm, X)
        e = sk[..., None] * (np.swapaxes(uv, 0, 1) - ok)
        return e[sk > 0].ravel()

    p0 = np.concatenate([cam0[free], X0[kept].ravel()])
    res = least_squares(fun, p0, loss='huber', f_scale=delta, x_scale='jac', xtol=tol, ftol=tol, gtol=tol, max_nfev=max_nfev)
    Rm, tm, Xk = unpack(res.x)
    X = np.full_like(X0, np.nan)
    X[kept] = Xk
    return Rm, tm, X, huber_cost(fun(res.x), delta), res


def triangulate_dlt(xyl, K, R, t, lik_thr=0.3, min_cams=2):
    """Weighted DLT of every point from its observations of weight > 0 (the start of the cases): [N][3], NaN when fewer
    than min_cams cameras see it."""
    K, R, t = (np.asarray(v, dtype=np.float64) for v in (K, R, t))
    o = as_points(xyl)
    with np.errstate(invalid='ignore'):
        ok = np.isfinite(o).all(axis=-1) & (o[..., 2] >= lik_thr) & (o[..., 2] > 0)
    P = K @ np.concatenate([R.reshape(-1, 3, 3), t.reshape(-1, 3, 1)], axis=2)
    X = np.full((len(o), 3), np.nan)
    for n in range(len(o)):
        cs = np.flatnonzero(ok[n])
        if len(cs) < max(2, min_cams):
            continue
        rows = []
        for c in cs:
            x, y, l = o[n, c]
            rows += [l * (P[c, 0] - x * P[c, 2]), l * (P[c, 1] - y * P[c, 2])]
        q = np.linalg.svd(np.array(rows))[2][-1]
        X[n] = q[:3] / q[3]
    return X


def make_case(family='ring', C=4, F=5, Kp=13, seed=0, noise_px=0.5, p_outlier=0.05, outlier_px=80.0, lik=(0.1, 1.0), rot_deg=1.5,
              trans_m=0.04, lik_thr=0.3, dtype=np.float64, distortion='none'):
    """One refinement case on a rig of `family`: dict with xyl [F][C][Kp][3], K, the true R, t and points, the perturbed
    R0, t0 (camera 0 and the held coordinate of camera 1 at the truth) and the start X0 (weighted DLT through the perturbed
    cameras).  lik = None: every likelihood is 1."""
    cams = rigs.make_rig(family, C, seed, distortion)
    scale, offset = rigs.scene(family)
    Q = (synth.make_points3d(F, 1, Kp, seed=seed) * scale + offset)[:, 0]                 # [F][Kp][3]
    rng = np.random.default_rng(seed + 4242)
    K = np.array(cams['K'], dtype=np.float64)
    R = np.array(cams['R_mat'], dtype=np.float64)
    t = np.array(cams['T'], dtype=np.float64)
    xyl = np.empty((F, C, Kp, 3))
    for c in range(C):
        uv = cvmath.project_points(Q.reshape(-1, 3), R[c], t[c], K[c], cams['dist'][c]).reshape(F, Kp, 2)
        uv = uv + rng.normal(0.0, 1.0, uv.shape) * noise_px
        out = rng.random((F, Kp)) < p_outlier
        ang, mag = rng.uniform(0, 2 * np.pi, (F, Kp)), rng.uniform(0.0, outlier_px, (F, Kp))
        uv = uv + out[..., None] * np.stack([mag * np.cos(ang), mag * np.sin(ang)], axis=-1)
        xyl[:, c, :, :2] = uv
        xyl[:, c, :, 2] = 1.0 if lik is None else rng.uniform(lik[0], lik[1], (F, Kp))
    xyl = xyl.astype(dtype)
    j = held_coord(R, t)
    R0, t0 = R.copy(), t.copy()
    for c in range(1, C):
        axis = rng.normal(size=3)
        axis /= np.linalg.norm(axis)
        R0[c] = cvmath.rodrigues(axis * np.deg2rad(rot_deg) * rng.uniform(0.5, 1.0)) @ R[c]
        d = rng.normal(size=3)
        d *= trans_m * rng.uniform(0.5, 1.0) / np.linalg.norm(d)
        if c == 1:
            d[j] = 0.0
        t0[c] = t[c] + d
    assert held_coord(R0, t0) == j, 'the perturbation moved the gauge'
    X0 = triangulate_dlt(xyl, K, R0, t0, lik_thr)
    return {'xyl': xyl, 'K': K, 'R': R, 't': t, 'Q': Q.reshape(-1, 3), 'R0': R0, 't0': t0, 'X0': X0, 'cams': cams, 'held': j,
            'lik_thr': lik_thr}
