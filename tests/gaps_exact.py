"""TEST INFRASTRUCTURE -- the interpolating splines of scipy's interp1d kinds 'slinear', 'quadratic' and 'cubic', solved
in multiprecision.

interp1d(x, y, kind) with order k = 1, 2, 3 is make_interp_spline(x, y, k) (scipy 1.15.3, interpolate/_bsplines.py): the
spline s = sum_j c_j B_j of degree k on the knot vector

    k = 1   x_0, x_0, x_1, ..., x_{n-1}, x_{n-1}                             (_augknt: the coefficients are the samples)
    k = 2   x_0 (3 times), (x_i + x_{i+1}) / 2 for i = 1 .. n-3, x_{n-1} (3 times)          (_not_a_knot, even k)
    k = 3   x_0 (4 times), x_2, ..., x_{n-3}, x_{n-1} (4 times)                              (_not_a_knot, odd k)

that takes the values s(x_i) = y_i, i = 0 .. n-1; with fill_value='extrapolate' the first and the last polynomial piece
go on beyond x_0 and x_{n-1}.  The knots are computed as scipy computes them, in float64 (they are part of the
definition); from there on everything is 60-digit arithmetic: the B-splines by the Cox-de Boor recursion, the n x n
collocation system by banded elimination, the value by de Boor's triangular scheme on the coefficients.  The result is
rounded to float64 once: a statement of the operation that shares nothing with the float64 code it is compared with.
"""
import mpmath as mp
import numpy as np

DIGITS = 60
ORDER = {'slinear': 1, 'quadratic': 2, 'cubic': 3}


def knots(x, k):
    """make_interp_spline's knot vector for the abscissae x (float64, increasing, at least k + 2 of them)."""
    x = np.asarray(x, dtype=np.float64)
    if k == 1:
        return np.r_[x[0], x, x[-1]]
    t = x.copy() if k % 2 == 1 else (x[1:] + x[:-1]) / 2
    k2 = (k + 1) // 2 if k % 2 == 1 else k // 2
    return np.r_[(x[0],) * (k + 1), t[k2:-k2], (x[-1],) * (k + 1)]


def _interval(t, k, n, x):
    """The piece that x is evaluated on: t[ell] <= x < t[ell + 1] within [k, n - 1], the end pieces beyond the ends."""
    ell = int(np.searchsorted(t, x, side='right')) - 1
    return min(max(ell, k), n - 1)


def _basis(tm, k, ell, x):
    """B_{ell-k} .. B_{ell} at x by the Cox-de Boor recursion on the piece ell (0 / 0 = 0)."""
    N = [mp.mpf(1)]                                               # degree 0: the one spline that lives on the piece
    for p in range(1, k + 1):
        new = [mp.mpf(0)] * (p + 1)
        for r in range(p):                                        # N[r] = B_{ell-p+1+r, p-1}
            j = ell - p + 1 + r
            span = tm[j + p] - tm[j]
            if span != 0:
                new[r] += (tm[j + p] - x) / span * N[r]           # its share of B_{j-1, p}
                new[r + 1] += (x - tm[j]) / span * N[r]           # and of B_{j, p}
        N = new
    return N


def coefficients(x, y, k):
    """The n B-spline coefficients (mpf) of the interpolating spline, and its knots (mpf)."""
    x = np.asarray(x, dtype=np.float64)
    n = len(x)
    t = knots(x, k)
    tm = [mp.mpf(float(v)) for v in t]
    rows, rhs = [], [mp.mpf(float(v)) for v in y]
    if k == 1:                                                    # B_j(x_i) = 1 for j = i, else 0
        return rhs, tm, t
    for i in range(n):                                            # row i: columns ell - k .. ell
        ell = _interval(t, k, n, x[i])
        rows.append((ell - k, _basis(tm, k, ell, mp.mpf(float(x[i])))))
    # banded elimination on dense band rows: A[i] maps column -> value
    A = [{lo + m: v for m, v in enumerate(vals) if v != 0} for lo, vals in rows]
    for i in range(n):
        piv = A[i].get(i, mp.mpf(0))
        assert piv != 0, 'zero pivot: the collocation matrix is totally positive, this cannot happen'
        for r in range(i + 1, min(n, i + k + 1)):
            a = A[r].pop(i, None)
            if a is None:
                continue
            f = a / piv
            for col, v in A[i].items():
                if col > i:
                    A[r][col] = A[r].get(col, mp.mpf(0)) - f * v
            rhs[r] -= f * rhs[i]
    c = [mp.mpf(0)] * n
    for i in range(n - 1, -1, -1):
        s = rhs[i]
        for col, v in A[i].items():
            if col > i:
                s -= v * c[col]
        c[i] = s / A[i][i]
    return c, tm, t


def evaluate(x, y, kind, x_new):
    """interp1d(x, y, kind, fill_value='extrapolate')(x_new), exact to float64's last bit: float64 [len(x_new)]."""
    k = ORDER[kind]
    n = len(x)
    out = np.empty(len(x_new))
    with mp.workdps(DIGITS):
        c, tm, t = coefficients(x, y, k)
        for q, xv in enumerate(np.asarray(x_new, dtype=np.float64)):
            ell = _interval(t, k, n, xv)
            xm = mp.mpf(float(xv))
            d = [c[ell - k + j] for j in range(k + 1)]            # de Boor's triangular scheme
            for r in range(1, k + 1):
                for j in range(k, r - 1, -1):
                    lo, hi = tm[j + ell - k], tm[j + 1 + ell - r]
                    alpha = (xm - lo) / (hi - lo)
                    d[j] = (1 - alpha) * d[j - 1] + alpha * d[j]
            out[q] = float(d[k])
    return out


def column(vals, labels, kind):
    """The exact interpolant of one column at its bad samples (NaN or 0): (positions, values), or None when the column has
    4 or fewer good samples."""
    vals = np.asarray(vals, dtype=np.float64)
    good = ~(np.isnan(vals) | (vals == 0))
    if int(good.sum()) <= 4:
        return None
    bad_pos = np.flatnonzero(~good)
    labels = np.asarray(labels, dtype=np.float64)
    return bad_pos, evaluate(labels[good], vals[good], kind, labels[bad_pos])
