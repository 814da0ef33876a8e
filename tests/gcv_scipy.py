"""The GCV smoothing-spline filter restated with SciPy's public make_smoothing_spline: the model the gcv_spline tests
check against (tests/test_gcv_spline_host.py uses it as a test double of Engine.gcv_spline, the GPU tests as the
yardstick of seeded inputs the goldens do not cover).

With x = arange(n) the reference's normalised-axis GCV search (filtering.py:163-181) searches on the very arrays
make_smoothing_spline builds, so make_smoothing_spline(x, y) finds the reference's lambda; it is read by wrapping
scipy's _compute_optimal_gcv_parameter for the call, and the fit is redone with lambda * smoothing_factor.
"""
import numpy as np


def runs(col):
    """Index arrays of the runs of valid samples (not NaN, not 0) of col."""
    good = np.flatnonzero(~(np.isnan(col) | (col == 0)))
    return np.split(good, np.flatnonzero(np.diff(good) > 1) + 1) if len(good) else []


def gcv_lambda(x, y):
    """The lambda make_smoothing_spline(x, y) chooses by GCV."""
    import scipy.interpolate._bsplines as bs
    from scipy.interpolate import make_smoothing_spline
    found = []
    orig = bs._compute_optimal_gcv_parameter

    def wrapped(*args):
        found.append(orig(*args))
        return found[-1]
    bs._compute_optimal_gcv_parameter = wrapped
    try:
        make_smoothing_spline(x, y)
    finally:
        bs._compute_optimal_gcv_parameter = orig
    return found[0]


def gcv_spline_columns(data, cutoff='auto', smoothing_factor=1.0, frame_rate=None, lam_override=None):
    """gcv_spline_filter_1d on every column of data [n_frames][n_cols] -> (out, lam) as Engine.gcv_spline returns them.
    lam_override [n_frames][n_cols] (optional): fit 'auto' runs with this lambda (at the run's first sample) instead of
    searching -- the fit alone, for inputs too long for SciPy's Python-loop search."""
    from scipy.interpolate import make_smoothing_spline
    data = np.asarray(data, dtype=np.float64)
    out = data.copy()
    lam_out = np.full(data.shape, np.nan)
    sf = float(smoothing_factor)
    for c in range(data.shape[1]):
        col = out[:, c]
        for seq in runs(col):
            if len(seq) < 2:
                continue
            y = col[seq]
            x = np.arange(len(seq))
            if cutoff == 'auto':
                med = np.median(y)
                mad = np.median(np.abs(y - med))
                mad = mad if mad > 0 else 1.0
                y_norm = 1 + (y - med) / (1.4826 * mad)
                if lam_override is not None:
                    lam = lam_override[seq[0], c]
                else:
                    if len(seq) <= 4:
                        raise ValueError('``x`` and ``y`` length must be at least 5')
                    lam = gcv_lambda(x, y_norm) * sf
                s = make_smoothing_spline(x, y_norm, lam=lam)(x)
                col[seq] = (s - 1) * (1.4826 * mad) + med
            else:
                lam = (frame_rate / (2 * np.pi * float(cutoff))) ** 4
                lam *= sf
                col[seq] = make_smoothing_spline(x, y, lam=lam)(x)
            lam_out[seq[0], c] = lam
    return out, lam_out
