"""The exact GCV smoothing spline of tests/gcv_exact.py pinned on the CPU: against SciPy where SciPy is accurate, against
the reference's recorded outputs and lambdas (tests/golden/gcv_units.npz), and the conditions the GPU tests
(tests/test_gcv_exact_gpu.py) rely on, for every case they use."""
import os

import numpy as np
import pytest

import gcv_exact as gx
from gcv_scipy import runs


@pytest.fixture(scope='module')
def gold(golden_dir):
    return np.load(os.path.join(golden_dir, 'gcv_units.npz'))


def test_fit_against_scipy_at_small_lambda():
    """lambda <= 6.4, where make_smoothing_spline loses a few ulps at the most."""
    worst = (0.0, None)
    for row in range(len(gx.LADDER)):
        lam = gx.ladder_lambda(*gx.LADDER[row])
        if lam > 6.5:
            continue
        for (scale, n), (y, exact, ref, d) in zip(gx.ladder_matrix()[2], gx.ladder_exact(row)):
            assert not isinstance(ref, Exception), (lam, scale, n, ref)
            worst = max(worst, (d, (lam, scale, n)))
    print(f'\nfit against scipy, lambda <= 6.4: worst distance {worst[0]:.3e} at (lambda, scale, n) = {worst[1]}')
    assert worst[0] <= gx.FIT_VS_SCIPY_SMALL


def test_fit_at_lambda_zero_is_the_input():
    y = gx.ladder_run('mm', 9)
    assert gx.distance(y, gx.fit(y, 0.0), y) == 0.0


def test_fit_against_the_recorded_fixed_cutoff_outputs(gold):
    worst, count = 0.0, 0
    for i in range(int(gold['n_cols'])):
        auto, sf, cutoff, rate = gold[f'col{i}_prm']
        if auto:
            continue
        col, ref, lam = gold[f'col{i}_in'], gold[f'col{i}_out'], gold[f'col{i}_lam']
        for seq in runs(col):
            if len(seq) < 5:
                continue
            exact = np.array([float(v) for v in gx.fit(col[seq], lam[seq[0]])])
            dev = (np.abs(ref[seq] - exact) / np.maximum(1.0, np.abs(ref[seq]))).max()
            assert dev <= gx.BAR_FIXED, (i, len(seq), dev)
            worst, count = max(worst, dev), count + 1
    print(f'\nfit against {count} recorded fixed cut-off runs: worst {worst:.3e}')
    assert count >= 20


def test_local_minimiser_against_the_recorded_lambdas(gold):
    """Every 'auto' run of the goldens with n <= 64 that is not on a straight line and has an interior minimum."""
    rows = []
    for i in range(int(gold['n_cols'])):
        auto, sf, cutoff, rate = gold[f'col{i}_prm']
        if not auto:
            continue
        col, lam, free = gold[f'col{i}_in'], gold[f'col{i}_lam'], gold[f'col{i}_lam_free']
        for seq in runs(col):
            n = len(seq)
            if n < 5 or n > 64 or free[seq[0]] == 1.0:
                continue
            rec = lam[seq[0]] / sf
            if not 1e-3 * n <= rec <= 0.9 * n:
                continue
            y_norm = gx.normalise(col[seq])[0]
            star = gx.local_minimiser(y_norm, 0.99 * rec, 1.01 * rec)
            if not gx.interior_minimum(y_norm, star):
                continue
            rows.append((i, n, rec, star))
    print()
    for i, n, rec, star in rows:
        print(f'column {i:2d} n {n:2d}: recorded lambda / sf {rec:.9f}, exact minimiser {star:.9f}, apart {abs(rec - star):.2e}')
    assert len(rows) >= 10
    for i, n, rec, star in rows:
        assert abs(rec - star) <= gx.BAR_LAM * max(1.0, rec), (i, n)


@pytest.mark.parametrize('row', range(len(gx.LADDER)))
def test_ladder_conditions(row):
    """SciPy does not raise and stays within the project's loosest bar of the exact fit on every ladder case."""
    lam = gx.ladder_lambda(*gx.LADDER[row])
    worst = 0.0
    for (scale, n), (y, exact, ref, d) in zip(gx.ladder_matrix()[2], gx.ladder_exact(row)):
        assert not isinstance(ref, Exception), (scale, n, ref)
        assert d < gx.LOOSEST_BAR, (scale, n, d)
        worst = max(worst, d)
    print(f'\nladder {gx.LADDER[row]}: lambda {lam:.4g}, scipy\'s worst distance to the exact fit {worst:.3e}')


@pytest.mark.parametrize('n_short', (0, 62, 63, 64, 128))
def test_wave_layout_cases(n_short):
    data, where = gx.wave_layout(n_short)
    got = sorted((c, int(seq[0]), len(seq)) for c in range(data.shape[1]) for seq in runs(data[:, c]))
    assert got == sorted(where) and len(where) == n_short + 1
    assert where[0][2] == 2000 and all(5 <= n <= 9 for _, _, n in where[1:])
    if n_short:
        assert {n for _, _, n in where[1:]} == {5, 6, 7, 8, 9}
        gaps = [data[s + n, c] for c, s, n in where[1:]]
        assert any(v == 0.0 for v in gaps) and any(np.isnan(v) for v in gaps)


@pytest.mark.parametrize('kind,n,seed', gx.SEARCH_CASES)
def test_search_cases_have_an_interior_minimum(kind, n, seed):
    y, y_norm, lam_scipy, lam_star = gx.search_case(kind, n, seed)
    print(f'\n{kind} n {n}: scipy lambda {lam_scipy:.9f}, exact minimiser {lam_star:.9f}, apart {abs(lam_scipy - lam_star):.2e}')
    assert gx.interior_minimum(y_norm, lam_star)
    assert abs(lam_scipy - lam_star) < 0.005 * lam_star            # inside the bracket, not at its ends


@pytest.mark.parametrize('kind,n,seed', gx.BOUNDARY_CASES)
def test_boundary_cases_end_at_the_interval_ends(kind, n, seed):
    """SciPy does not raise; noise ends at the upper end of (0, n), the noise-free signal at the lower."""
    lam = gx.search_case(kind, n, seed)[2]
    print(f'\n{kind} n {n}: scipy lambda {lam:.9g}')
    assert (n - 1e-4 < lam < n) if kind == 'noise' else (0 < lam < 1e-4)


def test_auto_cases_scipy_conditions():
    """The 'auto' fit cases at scipy's own lambda: scipy does not raise and is within the loosest bar of auto_fit."""
    worst = 0.0
    for kind in gx.SIGNALS:
        for n in gx.AUTO_LENGTHS[:-2]:                               # the search of 257 and 2000 samples is the GPU test's
            y, _, lam, _ = gx.search_case(kind, n, gx.SEEDS.get((kind, n), 0))
            d = gx.distance(gx.scipy_auto_fit(y, lam), gx.auto_fit(y, lam), y)
            assert d < gx.LOOSEST_BAR, (kind, n, d)
            worst = max(worst, d)
    print(f"\n'auto' cases, scipy's fit at scipy's lambda: worst distance {worst:.3e}")
