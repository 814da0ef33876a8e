"""TEST INFRASTRUCTURE -- the exact answer of loess_filter_1d's definition, in multiprecision.

The reference (Pose2Sim/filtering.py:532-558) replaces every run y_0..y_{L-1} of L > nb_values_used consecutive non-NaN
samples by lowess(run, frame_indices, frac=nb/L, it=0): with k = int(nb/L*L + 1e-10), the value at sample i is

    a + b x_i,   (a, b) = argmin sum_j w_j (y_j - a - b x_j)^2,   w_j = (1 - (|x_j - x_i| / h)^3)^3 for |x_j - x_i| < h, else 0,

h being the distance from x_i to its k-th nearest sample of the run (the sample itself counts as the first).  The
abscissae are consecutive frame indices, so only differences of them enter.  Neighbours are chosen by distance < h: a
sample at distance exactly h has weight 0 whichever way a tie between two of them is broken.  With a single non-zero
weight the line is not determined and the value is y_i.

Here the 2 x 2 normal equations are solved per sample at 60 digits and rounded to float64 once: a statement of the
operation that shares nothing with the float64 loops it is compared with.
"""
import mpmath as mp
import numpy as np

DIGITS = 60


def window(nb_values_used, run_length):
    """statsmodels' k = int(frac * n + 1e-10) for the reference's frac = nb / len(run)."""
    return int(nb_values_used / run_length * run_length + 1e-10)


def run(y, k):
    """One run y (no NaN) of more than k samples -> float64 [L], the local linear fit at every sample."""
    y = np.asarray(y, dtype=np.float64)
    L = len(y)
    assert 2 <= k < L
    out = np.empty(L)
    with mp.workdps(DIGITS):
        ym = [mp.mpf(float(v)) for v in y]
        cache = {}
        for i in range(L):
            h = sorted(abs(j - i) for j in range(L))[k - 1]
            near = [j for j in range(max(0, i - h + 1), min(L, i + h)) if abs(j - i) < h]
            if len(near) < 2:
                out[i] = y[i]
                continue
            s0 = s1 = s2 = t0 = t1 = mp.mpf(0)
            for j in near:
                d = abs(j - i)
                w = cache.get((d, h))
                if w is None:
                    w = cache[(d, h)] = (1 - (mp.mpf(d) / h) ** 3) ** 3
                u = j - i
                s0 += w; s1 += w * u; s2 += w * u * u
                t0 += w * ym[j]; t1 += w * u * ym[j]
            out[i] = float((s2 * t0 - s1 * t1) / (s0 * s2 - s1 * s1))      # the intercept: the line at u = 0
    return out


def runs(col, nb_values_used):
    """The index sequences the reference filters: runs of consecutive non-NaN samples longer than nb_values_used."""
    col = np.asarray(col, dtype=np.float64)
    good = np.where(~np.isnan(col))[0]
    if good.size == 0:
        return []
    return [s for s in np.split(good, np.where(np.diff(good) > 1)[0] + 1) if len(s) > nb_values_used]


def column(col, nb_values_used):
    """loess_filter_1d's answer for a whole column: every filtered run replaced by its exact fit, the rest left alone."""
    out = np.array(col, dtype=np.float64)
    for seq in runs(out, nb_values_used):
        out[seq] = run(out[seq], window(nb_values_used, len(seq)))
    return out
