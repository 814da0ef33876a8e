"""TEST INFRASTRUCTURE -- a stand-in for statsmodels.nonparametric.smoothers_lowess.lowess, which is not importable here.

The reference's loess_filter_1d (filtering.py:532-558) calls lowess(run, frame_indices, is_sorted=True, frac=nb/len(run),
it=0).  This module restates, in plain NumPy and in the algorithm's own order of operations, the three routines of
statsmodels' _lowess.pyx that such a call goes through -- update_neighborhood, calculate_weights, calculate_y_fit -- for
it = 0 and delta = 0, as published and as remembered: statsmodels itself has never run here, so everything recorded
through this module is parity-unpinned against statsmodels.  What pins it instead is tests/loess_exact.py, a 60-digit
solve of the definition that shares nothing with these loops.

The two details that cannot be looked up -- which of two equally distant neighbours stays in the window, and the rule
by which the window slides -- only decide whether a sample at distance exactly `radius` is in the window, where the
tricube weight is exactly 0.
"""
import numpy as np


def _update_neighborhood(x, i, n, left_end, right_end):
    """Slide the window [left_end, right_end) to the right while the next sample is nearer to x[i] than the leftmost."""
    while right_end < n and x[i] > (x[left_end] + x[right_end]) / 2.0:
        left_end += 1
        right_end += 1
    radius = max(x[i] - x[left_end], x[right_end - 1] - x[i])
    return left_end, right_end, radius


def _calculate_weights(x, i, left_end, right_end, radius):
    """Tricube weights of the window, normalised to sum 1; reg_ok is False when no regression can be made."""
    dist = np.abs(x[left_end:right_end] - x[i]) / radius
    w = 1.0 - dist * dist * dist
    w = w * w * w
    w[dist >= 1.0] = 0.0
    total = 0.0
    for v in w:
        total += v
    if total <= 0.0 or np.count_nonzero(w) < 2:          # a single non-zero weight: the fit is the sample itself
        return False, w
    return True, w / total


def _calculate_y_fit(x, y, i, weights, left_end, right_end, reg_ok):
    if not reg_ok:
        return y[i]
    xs, ys = x[left_end:right_end], y[left_end:right_end]
    sum_weighted_x = 0.0
    for w, xj in zip(weights, xs):
        sum_weighted_x += w * xj
    weighted_sqdev_x = 0.0
    for w, xj in zip(weights, xs):
        weighted_sqdev_x += w * (xj - sum_weighted_x) ** 2
    fit = 0.0
    for w, xj, yj in zip(weights, xs, ys):
        p_i_j = w * (1.0 + (x[i] - sum_weighted_x) * (xj - sum_weighted_x) / weighted_sqdev_x)
        fit += p_i_j * yj
    return fit


def lowess(endog, exog, frac=2.0 / 3.0, it=3, delta=0.0, xvals=None, is_sorted=False, missing='drop', return_sorted=True):
    if it != 0 or delta != 0.0 or xvals is not None:
        raise NotImplementedError('the stand-in covers it=0, delta=0, xvals=None: what the filtering stage calls')
    y = np.asarray(endog, dtype=np.float64)
    x = np.asarray(exog, dtype=np.float64)
    if x.ndim != 1 or y.shape != x.shape:
        raise ValueError('exog and endog must be vectors of one length')
    if not 0 <= frac <= 1:
        raise ValueError('Lowess `frac` must be in the range [0,1]!')
    if not (np.isfinite(x).all() and np.isfinite(y).all()):
        raise NotImplementedError('the stand-in takes finite data only')
    if not is_sorted:
        order = np.argsort(x, kind='stable')
        x, y = x[order], y[order]
    n = len(x)
    k = int(frac * n + 1e-10)
    if k < 2:
        raise NotImplementedError('a window of fewer than 2 samples has radius 0')
    y_fit = np.zeros(n)
    left_end, right_end = 0, k
    for i in range(n):
        left_end, right_end, radius = _update_neighborhood(x, i, n, left_end, right_end)
        reg_ok, weights = _calculate_weights(x, i, left_end, right_end, radius)
        y_fit[i] = _calculate_y_fit(x, y, i, weights, left_end, right_end, reg_ok)
    if not return_sorted:
        raise NotImplementedError('the stand-in returns the sorted (x, fit) columns only')
    return np.column_stack([x, y_fit])
