"""TEST INFRASTRUCTURE -- the exact answer of kalman_filter_1d's model, by one dense linear solve in multiprecision.

The reference (Pose2Sim/filtering.py:316-434) sets up, for every run z_1..z_N of >= 4 samples that are neither NaN nor 0,
a constant-acceleration model of one coordinate and hands it to filterpy's recursion.  The model is linear and Gaussian:

    x_0 ~ N(x_init, P0)                 x_init = [z_1, z_2 - z_1, z_3 - 2 z_2 + z_1] (differences NOT divided by dt, :342-351)
                                        P0 = measurement_noise * I                       (:376, filterpy's P starts as I)
    x_k = F x_{k-1} + g w_k             F = [[1, dt, dt^2/2], [0, 1, dt], [0, 0, 1]],  g = [dt^2/2, dt, 1]
    w_k ~ N(0, process_noise^2)         Q_discrete_white_noise(3, dt, var) = var * g g^T: rank one
    z_k = x_k[0] + v_k                  v_k ~ N(0, measurement_noise^2);  measurement_noise = 20, process_noise = 20 * trust_ratio

so what batch_filter + rts_smoother compute is the posterior mean of the positions x_k[0] given all of z_1..z_N, and what
batch_filter alone gives at sample k is the posterior mean of x_k[0] given z_1..z_k.  filterpy predicts before it updates,
so z_1 is observed at x_1 = F x_0 + g w_1, not at x_0.

Q is singular, so the unknowns are not the states but theta = [x_0 - x_init, w_1 .. w_N] (3 + N independent Gaussians).
With F^m = [[1, m dt, (m dt)^2 / 2], ...] the position at sample k is linear in theta:

    x_k[0] = (F^k x_0)[0] + sum_{j <= k} (F^(k-j) g)[0] w_j,
    (F^m)[0, :] = [1, m dt, (m dt)^2 / 2],   (F^m g)[0] = dt^2/2 + m dt^2 + (m dt)^2/2 = ((m + 1) dt)^2 / 2,

i.e. positions = A theta + c with c = (F^k x_init)[0], and the posterior mean of theta solves the normal equations

    (A^T A / R + diag(1/P0, 1/P0, 1/P0, 1/var, ..., 1/var)) theta = A^T (z - c) / R.

No recursion, no covariance propagation, 60 significant digits: a statement of the operation that shares nothing with the
float64 predict / update / smooth loops it is compared with.  Cost grows as N^3 (about 4 s at 80 samples, 30 s at 160).
"""
import mpmath as mp
import numpy as np

DIGITS = 60
MEASUREMENT_NOISE = 20


def initial_state(z):
    """The reference's initial state (:342-351): repeated np.diff of the run with derivate_array's default dt = 1."""
    z = np.asarray(z, dtype=np.float64)
    d1 = np.diff(z)
    return [z[0], d1[0], np.diff(d1)[0]]


def _system(z, frame_rate, trust_ratio, x_init):
    n = len(z)
    dt = mp.mpf(1) / int(frame_rate)
    A = mp.zeros(n, 3 + n)
    c = mp.zeros(n, 1)
    x0 = [mp.mpf(float(v)) for v in x_init]
    for k in range(1, n + 1):
        row = [mp.mpf(1), k * dt, (k * dt) ** 2 / 2]
        for i in range(3):
            A[k - 1, i] = row[i]
        c[k - 1] = row[0] * x0[0] + row[1] * x0[1] + row[2] * x0[2]
        for j in range(1, k + 1):
            A[k - 1, 2 + j] = ((k - j + 1) * dt) ** 2 / 2
    zz = mp.matrix([mp.mpf(float(v)) for v in z]) - c
    var = mp.mpf((MEASUREMENT_NOISE * int(trust_ratio)) ** 2)
    return A, c, zz, var


def _solve(A, c, zz, var, n):
    """Posterior means of the first n positions given the first n samples."""
    A, c, zz = A[:n, :3 + n], c[:n, :], zz[:n, :]
    R = mp.mpf(MEASUREMENT_NOISE ** 2)
    prior = mp.diag([mp.mpf(1) / MEASUREMENT_NOISE] * 3 + [1 / var] * n)
    At = A.T
    theta = mp.lu_solve(At * A / R + prior, At * zz / R)
    return A * theta + c


def posterior_means(z, frame_rate, trust_ratio, smoothed, x_init=None):
    """One run z (no NaN, no 0, at least 3 samples unless x_init is given).  smoothed: E[x_k[0] | z_1..z_N] for every k
    (filter + RTS smoother); otherwise E[x_k[0] | z_1..z_k] (the filter alone, one solve per prefix).  -> float64 [N]."""
    z = np.asarray(z, dtype=np.float64)
    with mp.workdps(DIGITS):
        A, c, zz, var = _system(z, frame_rate, trust_ratio, initial_state(z) if x_init is None else x_init)
        if smoothed:
            return np.array([float(v) for v in _solve(A, c, zz, var, len(z))])
        return np.array([float(_solve(A, c, zz, var, n)[n - 1]) for n in range(1, len(z) + 1)])


def first_filtered_sample(z, frame_rate, trust_ratio, x_init):
    """Closed form of the filter's first output: one predict and one scalar update from x_init (float64 in, mp inside)."""
    with mp.workdps(DIGITS):
        dt = mp.mpf(1) / int(frame_rate)
        x = [mp.mpf(float(v)) for v in x_init]
        var = mp.mpf((MEASUREMENT_NOISE * int(trust_ratio)) ** 2)
        pred = x[0] + dt * x[1] + dt ** 2 / 2 * x[2]
        # (F P0 F^T + Q)[0, 0] with P0 = measurement_noise * I
        p00 = MEASUREMENT_NOISE * (1 + dt ** 2 + dt ** 4 / 4) + var * dt ** 4 / 4
        gain = p00 / (p00 + MEASUREMENT_NOISE ** 2)
        return float(pred + gain * (mp.mpf(float(z[0])) - pred))


def smoothing_is_on(smooth):
    """The reference's `smooth == True` after `smooth = int(...)` (:395, :418): only 1 (or True) smooths."""
    return int(smooth) == 1


def column(col, frame_rate, trust_ratio, smooth):
    """kalman_filter_1d's answer for a whole column: every run of >= 4 samples that are neither NaN nor 0 replaced by
    its exact posterior means, every other sample left as it is."""
    out = np.array(col, dtype=np.float64)
    start = None
    for i in range(len(out) + 1):
        usable = i < len(out) and not np.isnan(out[i]) and out[i] != 0
        if usable and start is None:
            start = i
        elif not usable and start is not None:
            if i - start >= 4:
                out[start:i] = posterior_means(out[start:i], frame_rate, trust_ratio, smoothing_is_on(smooth))
            start = None
    return out
