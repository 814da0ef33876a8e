"""TEST INFRASTRUCTURE -- host mirror of p2s_loess_kernel (pose2sim_amd/csrc/p2s_filter.hip) in NumPy.

Splits every column into its runs of consecutive non-NaN samples and gives, for the runs that are long enough, the same
closed form as the kernel in the same centred arithmetic (u = j - i): away from a run's ends the fixed FIR filter with
the normalised tricube weights, at its ends the weighted least-squares line at u = 0 from the five centred sums.  It is
pinned to the reference's recorded outputs and to the exact values by tests/test_loess_host.py.
"""
import numpy as np

from pose2sim_amd.engine import loess_window
from test_filter_oracle import OracleFilterEngine


def interior_weights(k):
    """[k // 2] weights by distance of the symmetric window (h = k // 2), normalised over both sides."""
    m = k // 2
    w = (1.0 - (np.arange(m) / m) ** 3) ** 3
    return w / (w[0] + 2.0 * w[1:].sum())


def loess_run(y, k):
    """One run y (no NaN) of more than k samples."""
    y = np.asarray(y, dtype=np.float64)
    L, m = len(y), k // 2
    assert 2 <= k < L
    out = y.copy()
    wn = interior_weights(k)
    first, last = m, L - k + m                       # the samples whose window [i - m, i - m + k) is not clamped
    if m == 1:
        pass                                         # one non-zero weight: the sample itself
    else:
        full = np.concatenate([wn[:0:-1], wn])       # distances -(m - 1) .. m - 1
        win = np.lib.stride_tricks.sliding_window_view(y, 2 * m - 1)
        out[first:last + 1] = win[first - (m - 1):last - (m - 1) + 1] @ full
    # the samples whose window is clamped to the run's first k samples, then those clamped to its last k
    for idx, lo in ((np.arange(first), 0), (np.arange(last + 1, L), L - k)):
        if idx.size == 0:
            continue
        u = (np.arange(lo, lo + k)[None, :] - idx[:, None]).astype(np.float64)
        h = np.maximum(idx - lo, lo + k - 1 - idx).astype(np.float64)[:, None]
        keep = np.abs(u) < h
        w = np.where(keep, (1.0 - (np.abs(u) / h) ** 3) ** 3, 0.0)
        v = y[lo:lo + k][None, :]
        s0, s1, s2, t0, t1 = w.sum(1), (w * u).sum(1), (w * u * u).sum(1), (w * v).sum(1), (w * u * v).sum(1)
        with np.errstate(divide='ignore', invalid='ignore'):
            ubar, ybar = s1 / s0, t0 / s0
            fit = ybar - ((t1 - ubar * t0) / (s2 - s1 * ubar)) * ubar
        out[idx] = np.where(keep.sum(1) >= 2, fit, y[idx])      # one non-zero weight: the sample itself
    return out


def loess_columns(data, nb_values_used):
    """Engine.loess for a [n_frames][n_cols] matrix."""
    k, min_run = loess_window(nb_values_used)
    out = np.array(data, dtype=np.float64)
    assert out.ndim == 2
    for c in range(out.shape[1]):
        col = out[:, c]
        good = np.where(~np.isnan(col))[0]
        if good.size == 0:
            continue
        for seq in np.split(good, np.where(np.diff(good) > 1)[0] + 1):
            if len(seq) >= min_run:
                col[seq] = loess_run(col[seq], k)
    return out


class NumpyLoessEngine(OracleFilterEngine):
    """OracleFilterEngine (Hampel etc.) plus Engine.loess restated in NumPy."""

    def loess(self, data, nb_values_used):
        return loess_columns(data, nb_values_used)
