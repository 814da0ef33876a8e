"""Stand-in for the two filterpy names the reference's filtering module uses (filterpy.kalman.KalmanFilter and
filterpy.common.Q_discrete_white_noise), written from the published Kalman filter and Rauch-Tung-Striebel equations.

filterpy is not importable where the goldens are recorded.  make_golden_kalman.py puts this module in its place, so that
the reference's own set-up code (initial state, F, H, P, R, Q, the `smooth` test, the splitting into runs) runs unchanged
and only the recursion is this file's.  The recursion is in turn checked against an exact multiprecision solve
(tests/kalman_exact.py, tests/test_kalman_host.py).  General in dim_x / dim_z, plain matrix products and np.linalg.inv;
the state may be the 1-D array the reference assigns or a column vector.

    predict:   x <- F x (+ B u),  P <- F P F^T + Q
    update:    y = z - H x,  S = H P H^T + R,  K = P H^T S^-1,  x <- x + K y,
               P <- (I - K H) P (I - K H)^T + K R K^T                                   (Joseph form)
    smoother:  for k = n-2 .. 0:  Pp = F P_k F^T + Q,  C = P_k F^T Pp^-1,
               x_k <- x_k + C (x_{k+1} - F x_k),  P_k <- P_k + C (P_{k+1} - Pp) C^T
"""
import math

import numpy as np


class KalmanFilter:
    def __init__(self, dim_x, dim_z, dim_u=0):
        self.dim_x, self.dim_z, self.dim_u = dim_x, dim_z, dim_u
        self.x = np.zeros((dim_x, 1))
        self.P = np.eye(dim_x)
        self.Q = np.eye(dim_x)
        self.B = None
        self.F = np.eye(dim_x)
        self.H = np.zeros((dim_z, dim_x))
        self.R = np.eye(dim_z)

    def _measurement(self, z):
        z = np.asarray(z, dtype=np.float64).reshape(-1)
        if z.size != self.dim_z:
            raise ValueError(f'measurement of {z.size} values for dim_z = {self.dim_z}')
        return z if np.ndim(self.x) == 1 else z.reshape(self.dim_z, 1)

    def predict(self, u=None):
        F = np.asarray(self.F, dtype=np.float64)
        self.x = F @ self.x
        if self.B is not None and u is not None:
            self.x = self.x + np.asarray(self.B) @ u
        self.P = F @ self.P @ F.T + self.Q

    def update(self, z):
        H, R = np.asarray(self.H, dtype=np.float64), np.asarray(self.R, dtype=np.float64)
        residual = self._measurement(z) - H @ self.x
        PHt = self.P @ H.T
        gain = PHt @ np.linalg.inv(H @ PHt + R)
        self.x = self.x + gain @ residual
        keep = np.eye(self.dim_x) - gain @ H
        self.P = keep @ self.P @ keep.T + gain @ R @ gain.T

    def batch_filter(self, zs):
        """predict, then update, per measurement -> (means, covariances, means after predict, covariances after predict)."""
        n = len(zs)
        means = np.zeros((n,) + np.shape(self.x))
        covs = np.zeros((n, self.dim_x, self.dim_x))
        means_p, covs_p = means.copy(), covs.copy()
        for i, z in enumerate(zs):
            self.predict()
            means_p[i], covs_p[i] = self.x, self.P
            self.update(z)
            means[i], covs[i] = self.x, self.P
        return means, covs, means_p, covs_p

    def rts_smoother(self, Xs, Ps):
        """-> (smoothed means, smoothed covariances, smoother gains, predicted covariances)."""
        F = np.asarray(self.F, dtype=np.float64)
        n = len(Xs)
        xs, cov = np.array(Xs, dtype=np.float64), np.array(Ps, dtype=np.float64)
        gains, predicted = np.zeros_like(cov), np.zeros_like(cov)
        for k in range(n - 2, -1, -1):
            predicted[k] = F @ cov[k] @ F.T + self.Q
            gains[k] = cov[k] @ F.T @ np.linalg.inv(predicted[k])
            xs[k] = xs[k] + gains[k] @ (xs[k + 1] - F @ xs[k])
            cov[k] = cov[k] + gains[k] @ (cov[k + 1] - predicted[k]) @ gains[k].T
        return xs, cov, gains, predicted


def Q_discrete_white_noise(dim, dt=1., var=1., block_size=1):
    """Process noise of a discrete white-noise input w (variance var) that enters the highest derivative and is held over
    one step: the state moves by g w, so Q = var * g g^T, one block per coordinate.  dim 3 (position, velocity,
    acceleration): g = [dt^2/2, dt, 1]; dim 4 adds jerk; dim 2 is the piecewise-constant acceleration model on
    (position, velocity), g = [dt^2/2, dt]."""
    if dim == 2:
        g = np.array([dt ** 2 / 2, dt])
    elif dim in (3, 4):
        g = np.array([dt ** (dim - 1 - i) / math.factorial(dim - 1 - i) for i in range(dim)])
    else:
        raise ValueError('dim must be 2, 3 or 4')
    return np.kron(np.eye(block_size), np.outer(g, g) * var)
