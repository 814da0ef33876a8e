"""TEST INFRASTRUCTURE -- the natural cubic smoothing spline of gcv_spline_filter_1d and its GCV criterion, solved in
multiprecision, with the cases and the bounds of tests/test_gcv_exact_host.py and tests/test_gcv_exact_gpu.py.

The spline s through the samples y_0 .. y_{n-1} at x = 0 .. n-1 minimises sum (y_i - s(x_i))^2 + lambda int s''^2.  In
Reinsch's form (Reinsch 1967; Green & Silverman 1994, 2.3) its values at the samples are

    s = y - lambda Q g,      (R + lambda Q^T Q) g = Q^T y

with Q [n][n-2] the second differences (column j holds 1, -2, 1 in the rows j, j+1, j+2) and R [n-2][n-2] tridiagonal
(2/3 on the diagonal, 1/6 beside it): one symmetric positive definite 5-band system in the second derivatives g, solved
here by a banded L D L^T in 60-digit arithmetic.  The influence matrix is A = I - lambda Q (R + lambda Q^T Q)^-1 Q^T,
so tr A = n - lambda tr((R + lambda Q^T Q)^-1 Q^T Q), one banded solve per column of Q^T Q, and

    GCV(lambda) = (|y - s|^2 / n) / (1 - tr A / n)^2        (Craven & Wahba 1979).

Nothing here is shared with the kernel or with scipy's make_smoothing_spline, which both work in the B-spline basis
(X + lambda E) c = y with a pivoted band LU and get the trace from a banded Cholesky factor's inverse bands.
"""
import functools

import mpmath as mp
import numpy as np

DIGITS = 60

# ---- the bounds, with what was measured next to them ------------------------------------------------------------------
BAR_FIXED, BAR_LAM = 1e-9, 1e-4            # the project's bars of tests/test_gcv_spline_gpu.py
LOOSEST_BAR = 1e-6                         # its loosest (the 'auto' bar): scipy itself must stay inside it on every case
EPS = 2.0 ** -52
KERNEL_FACTOR = 8                          # d_kernel <= 8 max(d_scipy, 2^-52): another summation order, the rounding of
#                                            the exact result (the rule of tests/test_gaps_gpu.py's spline kinds)
SEARCH_FACTOR, XATOL = 4, 1e-5             # |lam_kernel - lam*| <= 4 max(|lam_scipy - lam*|, xatol): both sides run the
#                                            same Brent iteration on criterion values that differ in rounding, and either
#                                            may stop anywhere in a final bracket a few tol1 wide
# scipy's distance to fit() over the ladder's rows with lambda <= 6.4, every scale and run length: worst measured
# 3.5e-15 (lambda 6.4, n = 65, the mm scale); the bound is 100 x that
FIT_VS_SCIPY_SMALL = 3.5e-13


def _mpf(v):
    return mp.mpf(float(v))


def _factor(m, lam):
    """L D L^T of R + lambda Q^T Q [m][m] (diagonals 2/3 + 6 lambda, 1/6 - 4 lambda, lambda): d, e = L[i+1][i],
    f = L[i+2][i]."""
    a, b, c = mp.mpf(2) / 3 + 6 * lam, mp.mpf(1) / 6 - 4 * lam, lam
    d, e, f = [None] * m, [mp.mpf(0)] * m, [mp.mpf(0)] * m
    for i in range(m):
        di = a
        if i >= 1:
            di -= e[i - 1] ** 2 * d[i - 1]
        if i >= 2:
            di -= f[i - 2] ** 2 * d[i - 2]
        d[i] = di
        if i + 1 < m:
            e[i] = (b - (f[i - 1] * e[i - 1] * d[i - 1] if i >= 1 else 0)) / di
        if i + 2 < m:
            f[i] = c / di
    return d, e, f


def _solve(fac, rhs, first=0):
    """(R + lambda Q^T Q)^-1 rhs; rhs is zero before index `first`."""
    d, e, f = fac
    m = len(d)
    z = list(rhs)
    for i in range(max(first, 0) + 1, m):
        z[i] -= e[i - 1] * z[i - 1]
        if i >= 2:
            z[i] -= f[i - 2] * z[i - 2]
    for i in range(m):
        z[i] /= d[i]
    for i in range(m - 2, -1, -1):
        z[i] -= e[i] * z[i + 1]
        if i + 2 < m:
            z[i] -= f[i] * z[i + 2]
    return z


def _fit(ym, lam, fac=None):
    n = len(ym)
    m = n - 2
    fac = fac or _factor(m, lam)
    g = _solve(fac, [ym[j] - 2 * ym[j + 1] + ym[j + 2] for j in range(m)])
    s = list(ym)
    for j in range(m):
        v = lam * g[j]
        s[j] -= v
        s[j + 1] += 2 * v
        s[j + 2] -= v
    return s


def fit(y, lam):
    """The smoothing spline of the float64 samples y (n >= 3) with the float64 lambda >= 0, at the samples: n mpf."""
    with mp.workdps(DIGITS):
        return _fit([_mpf(v) for v in y], _mpf(lam))


def _gcv(ym, lam):
    n = len(ym)
    m = n - 2
    fac = _factor(m, lam)
    s = _fit(ym, lam, fac)
    numer = sum((a - b) ** 2 for a, b in zip(ym, s)) / n
    tr = mp.mpf(0)                                               # tr((R + lambda Q^T Q)^-1 Q^T Q)
    stencil = (1, -4, 6, -4, 1)
    for j in range(m):
        col = [mp.mpf(0)] * m
        for k, v in enumerate(stencil):
            if 0 <= j - 2 + k < m:
                col[j - 2 + k] = mp.mpf(v)
        tr += _solve(fac, col, j - 2)[j]
    t = lam * tr / n                                             # 1 - tr A / n
    return numer / (t * t)


def gcv(y, lam):
    """The GCV criterion of the float64 samples y at lambda > 0: mpf."""
    with mp.workdps(DIGITS):
        return _gcv([_mpf(v) for v in y], mp.mpf(lam))


def local_minimiser(y, lo, hi, tol=1e-9):
    """The minimiser of gcv(y, .) on [lo, hi] by golden section, to tol: float.  (A local minimiser when the criterion
    is unimodal on the bracket; interior_minimum() checks what the tests need of it.)"""
    with mp.workdps(DIGITS):
        ym = [_mpf(v) for v in y]
        g = (mp.sqrt(5) - 1) / 2
        a, b = mp.mpf(lo), mp.mpf(hi)
        x1, x2 = b - g * (b - a), a + g * (b - a)
        f1, f2 = _gcv(ym, x1), _gcv(ym, x2)
        while b - a > tol:
            if f1 <= f2:
                b, x2, f2 = x2, x1, f1
                x1 = b - g * (b - a)
                f1 = _gcv(ym, x1)
            else:
                a, x1, f1 = x1, x2, f2
                x2 = a + g * (b - a)
                f2 = _gcv(ym, x2)
        return float((a + b) / 2)


def interior_minimum(y, lam_star):
    """lam_star lies in [1e-3 n, 0.9 n] and the criterion is larger at both ends of a bracket of +-1 % around it."""
    n = len(y)
    if not 1e-3 * n <= lam_star <= 0.9 * n:
        return False
    mid = gcv(y, lam_star)
    return gcv(y, 0.99 * lam_star) > mid and gcv(y, 1.01 * lam_star) > mid


def normalise(y):
    """filtering.py:277-281 in float64, as the reference and the host do it: (y_norm, med, scale)."""
    y = np.asarray(y, dtype=np.float64)
    med = np.median(y)
    mad = np.median(np.abs(y - med))
    mad = mad if mad > 0 else 1.0
    return 1 + (y - med) / (1.4826 * mad), med, 1.4826 * mad


def auto_fit(y, lam):
    """The 'auto' output for the lambda of the final fit: the exact spline of the float64 y_norm, denormalised in mp."""
    y_norm, med, scale = normalise(y)
    with mp.workdps(DIGITS):
        return [(s - 1) * _mpf(scale) + _mpf(med) for s in _fit([_mpf(v) for v in y_norm], _mpf(lam))]


def distance(a, exact, y):
    """max |a - exact| / max(1, max |y|) over the run: float."""
    with mp.workdps(DIGITS):
        return float(max(abs(_mpf(u) - v) for u, v in zip(a, exact)) / max(1.0, float(np.abs(y).max())))


def kernel_bar(d_scipy):
    return KERNEL_FACTOR * max(d_scipy, EPS)


def scipy_fit(y, lam):
    from scipy.interpolate import make_smoothing_spline
    x = np.arange(len(y))
    return make_smoothing_spline(x, np.asarray(y, dtype=np.float64), lam=lam)(x)


def scipy_auto_fit(y, lam):
    """make_smoothing_spline(x, y_norm, lam=lam), denormalised: the reference's 'auto' output for a given final lambda."""
    y_norm, med, scale = normalise(y)
    return (scipy_fit(y_norm, lam) - 1) * scale + med


# ---- the cases --------------------------------------------------------------------------------------------------------
# (frame_rate, cut_off_frequency, smoothing_factor) as a configuration gives them; lambda = (rate / (2 pi fc))^4 sf
LADDER = [(30, 14.0, 1),        # 0.0135: no row swap at the ends of the LU
          (60, 6, 1),           # 6.4
          (120, 2.5, 1),        # 3.4e3, a float cut-off
          (240, 1, 1),          # 2.1e6
          (240, 1, 20),         # 4.3e7
          (1000, 1, 1),         # 6.4e8
          (60, 6, 0),           # 0: the output equals the input to rounding
          (60, 6, 0.5)]         # 3.2
RUN_LENGTHS = (5, 6, 7, 8, 9, 63, 64, 65, 257)
SCALES = ('m', 'mm', '1e5')     # about 1.2 m, about 1500 mm, 1e5 + a 0.3 signal
AUTO_LENGTHS = (5, 6, 7, 8, 9, 12, 31, 64, 257, 2000)
AUTO_FACTORS = (0.5, 1, 10)
SIGNALS = ('noise', 'smooth', 'sinus')
# the seeds with which 'noise' ends at the upper end of the search interval and 'sinus' inside it (scipy's search;
# test_gcv_exact_host.py asserts what the tests rely on); 0 where not listed
SEEDS = {('noise', 5): 1, ('noise', 7): 2, ('noise', 8): 1, ('noise', 9): 1, ('noise', 12): 1, ('noise', 64): 2, ('sinus', 8): 2}
# 'auto' cases whose GCV minimum is interior: (signal, n, seed)
SEARCH_CASES = (('noise', 9, 4), ('sinus', 5, 0), ('sinus', 7, 0), ('sinus', 12, 0), ('sinus', 31, 0), ('sinus', 64, 0))
# and the two boundary signals: lambda ends at the search interval's upper / lower end
BOUNDARY_CASES = tuple((sig, n, SEEDS.get((sig, n), 0)) for sig in ('noise', 'smooth') for n in (5, 8, 12, 64))


def ladder_lambda(rate, cutoff, sf):
    """filtering.py:301-304: the same two operations in the same order."""
    lam = (rate / (2 * np.pi * float(cutoff))) ** 4
    lam *= sf
    return lam


def signal(kind, n, seed=0):
    """A run of n samples, metres around 1.2: 'noise' (GCV ends at the upper end of (0, n)), 'smooth' (a noise-free
    sinusoid: the lower end), 'sinus' (a noisy sinusoid)."""
    rng = np.random.default_rng([20, SIGNALS.index(kind), n, seed])
    t = np.arange(n) / 60.0
    wave = 0.3 * np.sin(2 * np.pi * rng.uniform(0.5, 1.5) * t + rng.uniform(0, 6))
    if kind == 'noise':
        return 1.2 + 0.05 * rng.normal(size=n)
    if kind == 'smooth':
        return 1.2 + wave
    return 1.2 + wave + 0.01 * rng.normal(size=n)


def ladder_run(scale, n):
    y = signal('sinus', n, seed=1 + SCALES.index(scale))
    if scale == 'mm':
        return 1500.0 + 1000.0 * (y - 1.2)
    if scale == '1e5':
        return 1e5 + (y - 1.2)
    return y


def columns(runs_):
    """The runs as NaN-padded columns of one matrix, run k starting at frame k % 3: (data, [(col, start, n)])."""
    F = max(len(y) for y in runs_) + 2
    data = np.full((F, len(runs_)), np.nan)
    where = []
    for c, y in enumerate(runs_):
        data[c % 3:c % 3 + len(y), c] = y
        where.append((c, c % 3, len(y)))
    return data, where


@functools.lru_cache(maxsize=None)
def ladder_matrix():
    """Every scale and run length of the ladder: (data, where, [(scale, n)])."""
    keys = [(s, n) for s in SCALES for n in RUN_LENGTHS]
    data, where = columns([ladder_run(s, n) for s, n in keys])
    data.setflags(write=False)
    return data, where, keys


@functools.lru_cache(maxsize=None)
def ladder_exact(row):
    """For LADDER[row]: [(y, exact fit, scipy's fit or the exception it raised, d_scipy)] per column of ladder_matrix()."""
    lam = ladder_lambda(*LADDER[row])
    data, where, _ = ladder_matrix()
    out = []
    for c, start, n in where:
        y = data[start:start + n, c]
        exact = fit(y, lam)
        try:
            ref = scipy_fit(y, lam)
            out.append((y, exact, ref, distance(ref, exact, y)))
        except Exception as e:                                   # noqa: BLE001 -- the host test reports it
            out.append((y, exact, e, np.inf))
    return out


def wave_layout(n_short):
    """One run of 2000 samples followed by n_short runs of 5 to 9 samples, dealt to three columns and separated by
    zeros and NaN in turn: (data, [(col, start, n)]).  The first wave's storage is sized by a run 200 times longer than
    its neighbours', and with more than 63 short runs a second wave starts at the work offset of lane 64."""
    rng = np.random.default_rng([21, n_short])
    lens = [5 + k % 5 for k in range(n_short)]
    F = 2000 + 1 + sum(ln + 1 for ln in lens[0::3])
    data = np.full((F, 3), np.nan)
    data[:2000, 0] = signal('sinus', 2000, seed=5)
    where = [(0, 0, 2000)]
    top = [2001, 0, 0]
    for k, ln in enumerate(lens):
        c = k % 3
        data[top[c]:top[c] + ln, c] = signal('sinus', ln, seed=100 + k) + rng.uniform(-0.2, 0.2)
        where.append((c, top[c], ln))
        top[c] += ln
        data[top[c], c] = 0.0 if k % 2 else np.nan
        top[c] += 1
    return data, where


def auto_run(kind, n):
    """The run of the 'auto' fit cases."""
    return signal(kind, n, SEEDS.get((kind, n), 0))


@functools.lru_cache(maxsize=None)
def search_case(kind, n, seed):
    """An 'auto' case: (y, y_norm, lam_scipy, lam_star or None).  lam_star (SEARCH_CASES only) is the exact minimiser on
    a bracket of +-1 % around scipy's value."""
    from gcv_scipy import gcv_lambda
    y = signal(kind, n, seed)
    y_norm = normalise(y)[0]
    lam_scipy = float(gcv_lambda(np.arange(n), y_norm))
    lam_star = local_minimiser(y_norm, 0.99 * lam_scipy, 1.01 * lam_scipy) if (kind, n, seed) in SEARCH_CASES else None
    return y, y_norm, lam_scipy, lam_star
