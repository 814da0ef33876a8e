"""p2s_gcv_spline_kernel on the MI355X against the exact smoothing spline of tests/gcv_exact.py (60-digit Reinsch form),
through Engine.gcv_spline.  SciPy's make_smoothing_spline, the float64 algorithm the kernel follows, is the yardstick
rather than the reference: on every run

    d_kernel <= 8 max(d_scipy, 2^-52)

d_kernel and d_scipy being the distances of the kernel's and of SciPy's output to the exact fit, relative to
max(1, max |y|) of the run.  The lambda ladder goes from 0 to 6.4e8 (where SciPy itself is 5e-7 from the truth), the run
lengths from 5 samples up, at three data scales; the 'auto' search is held to the exact local minimiser of the GCV
criterion.  tests/test_gcv_exact_host.py pins the exact solve and the conditions on these cases."""
import numpy as np
import pytest

import gcv_exact as gx

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def engine():
    from pose2sim_amd.engine import Engine
    return Engine(0)


def _untouched(data, out, where):
    """The samples outside the filtered runs bit for bit, the NaN pattern everywhere."""
    f = np.zeros(data.shape, dtype=bool)
    for c, start, n in where:
        f[start:start + n, c] = True
    assert np.array_equal(np.isnan(out), np.isnan(data))
    assert np.array_equal(out[~f], data[~f], equal_nan=True)


def _lam_pattern(lam, where):
    want = np.zeros(lam.shape, dtype=bool)
    for c, start, _ in where:
        want[start, c] = True
    assert np.array_equal(~np.isnan(lam), want)


@pytest.mark.parametrize('row', range(len(gx.LADDER)))
def test_fixed_cutoff_ladder(engine, row):
    rate, cutoff, sf = gx.LADDER[row]
    data, where, keys = gx.ladder_matrix()
    out, lam = engine.gcv_spline(data, cutoff, sf, rate)
    _untouched(data, out, where)
    _lam_pattern(lam, where)
    want = gx.ladder_lambda(rate, cutoff, sf)
    failed = []
    print(f'\nladder {gx.LADDER[row]}: lambda {want:.6g}')
    for (c, start, n), (scale, _), (y, exact, ref, d_scipy) in zip(where, keys, gx.ladder_exact(row)):
        d_kernel = gx.distance(out[start:start + n, c], exact, y)
        ok = d_kernel <= gx.kernel_bar(d_scipy) and lam[start, c] == want
        apart = np.abs(out[start:start + n, c] - ref).max() / max(1.0, np.abs(y).max())     # for the record, not held
        print(f'  {scale:>3} n {n:3d}: d_scipy {d_scipy:.3e}  d_kernel {d_kernel:.3e}  bar {gx.kernel_bar(d_scipy):.3e}  '
              f'kernel to scipy {apart:.3e}  lam {lam[start, c]!r}{"" if ok else "  <-- FAILS"}')
        if not ok:
            failed.append((scale, n))
    assert not failed, failed


@pytest.mark.parametrize('n_short', (0, 62, 63, 64, 128))
def test_wave_layout(engine, n_short):
    """A run of 2000 samples and n_short runs of 5 to 9: 1, 63, 64, 65 and 129 lanes, cut-off 6 at 60 fps."""
    data, where = gx.wave_layout(n_short)
    out, lam = engine.gcv_spline(data, 6, 1.0, 60)
    _untouched(data, out, where)
    _lam_pattern(lam, where)
    want = gx.ladder_lambda(60, 6, 1.0)
    worst, failed = (0.0, 0.0), []
    for k, (c, start, n) in enumerate(where):
        y = data[start:start + n, c]
        exact = gx.fit(y, want)
        d_scipy, d_kernel = gx.distance(gx.scipy_fit(y, want), exact, y), gx.distance(out[start:start + n, c], exact, y)
        worst = max(worst, (d_kernel, d_scipy))
        if not (d_kernel <= gx.kernel_bar(d_scipy) and lam[start, c] == want):
            failed.append((k, c, start, n, d_scipy, d_kernel))
    print(f'\n{len(where)} runs: worst d_kernel {worst[0]:.3e} (d_scipy there {worst[1]:.3e}); the run of 2000: '
          f'd_kernel {gx.distance(out[:2000, 0], gx.fit(data[:2000, 0], want), data[:2000, 0]):.3e}')
    assert not failed, failed


@pytest.fixture(scope='module')
def auto_matrix():
    keys = [(kind, n) for kind in gx.SIGNALS for n in gx.AUTO_LENGTHS]
    data, where = gx.columns([gx.auto_run(kind, n) for kind, n in keys])
    return data, where, keys


@pytest.mark.parametrize('sf', gx.AUTO_FACTORS)
def test_auto_fit(engine, auto_matrix, sf):
    """The solver of the 'auto' mode: the output against the exact spline of the normalised run with the kernel's own
    lambda, denormalised, SciPy's fit with that lambda as the yardstick."""
    data, where, keys = auto_matrix
    out, lam = engine.gcv_spline(data, 'auto', sf, 60)
    _untouched(data, out, where)
    _lam_pattern(lam, where)
    failed = []
    print(f"\n'auto', smoothing factor {sf}")
    for (c, start, n), (kind, _) in zip(where, keys):
        y, lk = data[start:start + n, c], lam[start, c]
        assert 0 < lk <= n * sf, (kind, n, lk)
        exact = gx.auto_fit(y, lk)
        d_scipy, d_kernel = gx.distance(gx.scipy_auto_fit(y, lk), exact, y), gx.distance(out[start:start + n, c], exact, y)
        ok = d_kernel <= gx.kernel_bar(d_scipy)
        print(f'  {kind:>6} n {n:4d}: lambda {lk:.9g}  d_scipy {d_scipy:.3e}  d_kernel {d_kernel:.3e}{"" if ok else "  <-- FAILS"}')
        if not ok:
            failed.append((kind, n))
    assert not failed, failed


@pytest.mark.parametrize('sf', (1, 0.5, 10))
def test_auto_search(engine, sf):
    """The search: the interior cases against the exact local minimiser of GCV, the two boundary signals against SciPy."""
    cases = gx.SEARCH_CASES + gx.BOUNDARY_CASES
    data, where = gx.columns([gx.search_case(*k)[0] for k in cases])
    _, lam = engine.gcv_spline(data, 'auto', sf, 60)
    failed = []
    print(f"\n'auto' search, smoothing factor {sf}")
    for (c, start, n), key in zip(where, cases):
        _, _, lam_scipy, lam_star = gx.search_case(*key)
        lk = lam[start, c] / sf
        if lam_star is not None:
            bar = gx.SEARCH_FACTOR * max(abs(lam_scipy - lam_star), gx.XATOL)
            ok = abs(lk - lam_star) <= bar
            print(f'  {key[0]:>6} n {n:2d}: lambda* {lam_star:.9f}  scipy {lam_scipy:.9f} ({abs(lam_scipy - lam_star):.2e})  '
                  f'kernel {lk:.9f} ({abs(lk - lam_star):.2e})  bar {bar:.1e}{"" if ok else "  <-- FAILS"}')
        else:
            ok = abs(lk - lam_scipy) <= gx.BAR_LAM * max(1.0, lam_scipy)
            print(f'  {key[0]:>6} n {n:2d}: scipy {lam_scipy:.9g}  kernel {lk:.9g}{"" if ok else "  <-- FAILS"}')
        if not ok:
            failed.append(key)
    assert not failed, failed


def test_two_calls_return_the_same_bytes(engine):
    data = gx.ladder_matrix()[0]
    for cutoff, sf in ((6, 1.0), (1, 20.0), ('auto', 1.0)):
        a, b = engine.gcv_spline(data, cutoff, sf, 240), engine.gcv_spline(data, cutoff, sf, 240)
        assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes()
