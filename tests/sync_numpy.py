"""A NumPy / SciPy restatement of the synchronization engine entries (Engine.sync_speeds, Engine.lagged_pearson): the
CPU model the goldens pin and the GPU kernels are checked against, and a test double of Engine for the stage."""
import numpy as np
from scipy import signal


def interpolate_column(col):
    """interpolate_zeros_nans(col, 'linear') (common.py:669-715): linear interpolation of NaN / 0 samples with
    extrapolation at the ends, as scipy interp1d evaluates it; untouched with 4 good samples or fewer."""
    col = np.array(col, dtype=np.float64)
    good = np.flatnonzero(~(np.isnan(col) | (col == 0)))
    if len(good) <= 4:
        return col
    miss = np.flatnonzero(np.isnan(col) | (col == 0))
    idx = np.clip(np.searchsorted(good, miss), 1, len(good) - 1)
    lo, hi = good[idx - 1], good[idx]
    slope = (col[hi] - col[lo]) / (hi - lo).astype(np.float64)
    col[miss] = slope * (miss - lo).astype(np.float64) + col[lo]
    return col


def bfill_ffill(col):
    col = np.array(col, dtype=np.float64)
    for order in (slice(None, None, -1), slice(None)):
        view = col[order]
        carry = np.nan
        for i in range(len(view)):
            if np.isnan(view[i]):
                view[i] = carry
            else:
                carry = view[i]
    return col


def speeds(coords, b, a):
    """Per camera: columns interpolated, filled, filtered (more than 3 (len(b) - 1) frames), the sum of |diff| of the y
    columns (NaN -> 2x the second row's diff, NaN skipped), that sum filtered under the same rule."""
    padlen = 3 * (max(len(a), len(b)) - 1)
    out = []
    for cam in coords:
        cam = np.asarray(cam, dtype=np.float64)
        n = cam.shape[0]
        filled = np.column_stack([bfill_ffill(interpolate_column(cam[:, j])) for j in range(cam.shape[1])]) if cam.shape[1] else cam
        if n > padlen and cam.shape[1]:
            filled = signal.filtfilt(b, a, filled, axis=0)
        y = filled[:, 1::2]
        d = np.full_like(y, np.nan)
        d[1:] = y[1:] - y[:-1]
        d = np.where(np.isnan(d), 2 * (y[1] - y[0]), d)
        s = np.nansum(np.abs(d), axis=1) if y.shape[1] else np.zeros(n)
        if n > padlen:
            s = signal.filtfilt(b, a, s)
        out.append(s)
    return out


def pearson(x, y):
    """np.corrcoef of the pairs where neither value is NaN (Series.corr); NaN with fewer than 2 pairs."""
    ok = ~(np.isnan(x) | np.isnan(y))
    x, y = x[ok], y[ok]
    if len(x) < 2:
        return np.nan
    with np.errstate(divide='ignore', invalid='ignore'):
        return float(np.corrcoef(x, y)[0, 1])


def lagged_pearson(ref, signals, lag_lo, lag_hi):
    """-> (r [n_sig][n_lags], np.argmax of each row, np.nanmax of each row (NaN when all NaN))."""
    ref = np.asarray(ref, dtype=np.float64)
    n_lags = lag_hi - lag_lo
    r = np.full((len(signals), n_lags), np.nan)
    for s, sig in enumerate(signals):
        sig = np.asarray(sig, dtype=np.float64)
        m = min(len(ref), len(sig))
        for t in range(n_lags):
            lag = lag_lo + t
            lo, hi = max(lag, 0), min(m, len(sig) + lag)
            if hi > lo:
                r[s, t] = pearson(ref[lo:hi], sig[lo - lag:hi - lag])
    arg = np.array([int(np.argmax(row)) for row in r], dtype=np.int64)
    mx = np.array([np.nan if np.isnan(row).all() else np.nanmax(row) for row in r])
    return r, arg, mx


class NumpySyncEngine:
    """Engine.sync_speeds / Engine.lagged_pearson on the CPU."""

    def sync_speeds(self, coords, b, a, zi):
        padlen = 3 * (max(len(a), len(b)) - 1)
        for cam in coords:
            if padlen < len(cam) <= 3 * len(b):
                raise ValueError(f'The length of the input vector x must be greater than padlen, which is {3 * len(b)}.')
        return speeds(coords, b, a)

    def lagged_pearson(self, ref, signals, lag_lo, lag_hi):
        return lagged_pearson(ref, signals, lag_lo, lag_hi)
