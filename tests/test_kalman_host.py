"""The Kalman filter of the filtering stage on CPU, pinned to the reference and to an exact posterior solve.

tests/golden/kalman_units.npz (<- make_golden_kalman.py) holds columns run through the reference's own kalman_filter_1d
and files written by its filter_all, with filterpy's recursion replaced by tests/golden/filterpy_standin.py (filterpy has
never run here), and next to each column the exact posterior means of the same model (tests/kalman_exact.py, one dense
solve at 60 digits).  Checked here: the stand-in and the stored exact values against a fresh exact solve (the goldens'
provenance), the reference outputs against the exact values, oracle/filtering_ref.kalman_filter_1d against both, the
initial state, the `smooth` values, and filter_all with the oracle engine against the recorded file text.

Bars: the project's 1e-9 relative to max(1, |value|) with identical NaN pattern for the oracle (tests/test_filter_gpu.py
holds the kernel to the same); 1e-10 for the recorded reference outputs and the stand-in against the exact solve (the
limit the generator refuses to exceed; measured: 2.6e-15).  Every recorded column and file is compared."""
import logging
import os
import sys

import numpy as np
import pytest

import kalman_exact
from oracle import filtering_ref as fr
from test_filter_oracle import OracleFilterEngine

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden'))
import filterpy_standin  # noqa: E402

TOL = 1e-9                     # the project's bar (test_filter_gpu.TOL)
REFERENCE_TOL = 1e-10          # the reference's float64 recursion against the exact solve
SMOOTH_VALUES = {'True': True, 'False': False, '1': 1, '0': 0, '2': 2}


@pytest.fixture(scope='module')
def gold(golden_dir):
    return np.load(os.path.join(golden_dir, 'kalman_units.npz'))


@pytest.fixture
def work_dir():
    """A scratch directory whose path does not contain 'filt' (filter_all skips every .trc whose path does)."""
    import shutil
    import tempfile
    from pathlib import Path
    d = tempfile.mkdtemp(prefix='p2s_kal_')
    yield Path(d)
    shutil.rmtree(d, ignore_errors=True)


def _case(g, i):
    rate, trust = (int(v) for v in g[f'col{i}_prm'])
    return g[f'col{i}_in'], rate, trust, SMOOTH_VALUES[str(g[f'col{i}_smooth'])]


def _distance(got, want, what):
    assert got.shape == want.shape and np.array_equal(np.isnan(got), np.isnan(want)), f'{what}: NaN pattern'
    ok = ~np.isnan(want)
    return float((np.abs(got[ok] - want[ok]) / np.maximum(1.0, np.abs(want[ok]))).max()) if ok.any() else 0.0


def _close(got, want, what, tol=TOL):
    d = _distance(got, want, what)
    assert d <= tol, f'{what}: {d:.3e}'
    return d


def _runs(col):
    good = np.where(~(np.isnan(col) | (col == 0)))[0]
    return [s for s in np.split(good, np.where(np.diff(good) > 1)[0] + 1) if len(s) >= 4]


def _standin_column(col, rate, trust, smoothed):
    """The model of kalman_exact's docstring handed to the stand-in, run by run."""
    out = np.array(col, dtype=np.float64)
    dt = 1 / rate
    for seq in _runs(out):
        f = filterpy_standin.KalmanFilter(dim_x=3, dim_z=1)
        f.x = np.array(kalman_exact.initial_state(out[seq]))
        f.F = np.array([[1, dt, dt * dt / 2], [0, 1, dt], [0, 0, 1]])
        f.H = np.array([[1.0, 0.0, 0.0]])
        f.P = np.eye(3) * 20
        f.R = np.array([[400.0]])
        f.Q = filterpy_standin.Q_discrete_white_noise(3, dt=dt, var=(20 * trust) ** 2)
        means, covs, _, _ = f.batch_filter(out[seq])
        if smoothed:
            means = f.rts_smoother(means, covs)[0]
        out[seq] = means[:, 0]
    return out


def test_fixture_covers_what_it_should(gold):
    g = gold
    cases = [_case(g, i) for i in range(int(g['n_cols']))]
    combos = {(rate, trust) for _, rate, trust, _ in cases}
    assert {(r, t) for r in (25, 30, 60, 120, 240) for t in (1, 20, 500, 5000)} <= combos
    assert {str(g[f'col{i}_smooth']) for i in range(len(cases))} == set(SMOOTH_VALUES)
    run_lengths = set()
    for col, *_ in cases:
        good = np.where(~(np.isnan(col) | (col == 0)))[0]
        run_lengths |= {len(s) for s in np.split(good, np.where(np.diff(good) > 1)[0] + 1)}
    assert {0, 1, 2, 3, 4, 5, 6, 100} <= run_lengths and max(run_lengths) == 100
    assert any(np.isnan(c).all() for c, *_ in cases) and any(len(c) < 4 for c, *_ in cases)
    assert any(np.isnan(c).any() and (c == 0).any() for c, *_ in cases)
    assert any(np.nanmin(c) < -100 for c, *_ in cases if not np.isnan(c).all()) and any(np.nanmax(c) > 100 for c, *_ in cases if not np.isnan(c).all())
    for i in range(len(cases)):
        assert f'col{i}_out' in g.files and f'col{i}_exact' in g.files, i


PROVENANCE_COLUMNS = (1, 6, 7, 19, 22, 24, 34, 35)


def test_standin_and_stored_exact_values_against_a_fresh_exact_solve(gold):
    """The goldens' provenance: on a handful of columns (filter and smoother, 25 to 240 fps, trust 1 to 5000, both
    scales, a column of short runs split by NaN) the exact solve is recomputed here; the stored exact values must equal it
    bit for bit, and the stand-in -- set up by this test from the model, not by the reference -- must meet it."""
    g = gold
    seen = set()
    for i in PROVENANCE_COLUMNS:
        col, rate, trust, smooth = _case(g, i)
        smoothed = kalman_exact.smoothing_is_on(smooth)
        exact = kalman_exact.column(col, rate, trust, smooth)
        assert np.array_equal(exact, g[f'col{i}_exact'], equal_nan=True), i
        d = _close(_standin_column(col, rate, trust, smoothed), exact, f'stand-in, column {i}', REFERENCE_TOL)
        print(f'column {i}: {rate} fps, trust {trust}, smooth {smooth!r}: |stand-in - exact| = {d:.2e}')
        seen.add(smoothed)
    assert seen == {True, False}


def test_reference_outputs_against_the_exact_values(gold):
    g = gold
    worst = 0.0
    for i in range(int(g['n_cols'])):
        col, out, exact = g[f'col{i}_in'], g[f'col{i}_out'], g[f'col{i}_exact']
        worst = max(worst, _close(out, exact, f'reference output, column {i}', REFERENCE_TOL))
        filtered = np.zeros(len(col), dtype=bool)
        for seq in _runs(col):
            filtered[seq] = True
        assert np.array_equal(out[~filtered], col[~filtered], equal_nan=True), i
        assert np.array_equal(exact[~filtered], col[~filtered], equal_nan=True), i
    print(f'worst |reference - exact| = {worst:.2e}')


def test_oracle_against_every_golden_column(gold):
    """oracle/filtering_ref.kalman_filter_1d against what the reference's code returned and against the exact values."""
    g = gold
    for i in range(int(g['n_cols'])):
        col, rate, trust, smooth = _case(g, i)
        got = fr.kalman_filter_1d(col, rate, trust, smooth)
        what = f'column {i} ({rate} fps, trust {trust}, smooth {smooth!r})'
        d_ref = _distance(got, g[f'col{i}_out'], what)
        d_exact = _distance(got, g[f'col{i}_exact'], what)
        print(f'{what}: |oracle - reference| = {d_ref:.2e}, |oracle - exact| = {d_exact:.2e}')
        assert d_ref <= TOL and d_exact <= TOL, f'{what}: {d_ref:.3e} from the reference, {d_exact:.3e} from the exact values'
        filtered = np.zeros(len(col), dtype=bool)
        for seq in _runs(col):
            filtered[seq] = True
        assert np.array_equal(got[~filtered], col[~filtered], equal_nan=True), what


def initial_state_cases(g):
    """Filter-only fixture columns at 25 and 240 fps whose first run has >= 4 samples -> (column index, run, rate, trust)."""
    out = []
    for i in range(int(g['n_cols'])):
        col, rate, trust, smooth = _case(g, i)
        runs = _runs(col)
        if rate in (25, 240) and not kalman_exact.smoothing_is_on(smooth) and runs:
            out.append((i, col[runs[0]], rate, trust))
    assert {c[2] for c in out} == {25, 240}
    return out


def check_initial_state(first_sample, z, rate, trust, what):
    """The first filtered sample of a filter-only run is one predict and one update from x_init: it must equal the closed
    form for the reference's x_init = [z0, z1 - z0, z2 - 2 z1 + z0] (differences not divided by dt), which is also the
    exact solve on the 1-sample prefix.  Where the signal moves, the state divided by dt and dt^2 gives another number."""
    x_init = [z[0], z[1] - z[0], (z[2] - z[1]) - (z[1] - z[0])]
    want = kalman_exact.first_filtered_sample(z, rate, trust, x_init)
    prefix = kalman_exact.posterior_means(z[:1], rate, trust, False, x_init=x_init)[0]
    assert abs(want - prefix) <= 1e-13 * max(1.0, abs(want)), what
    divided = kalman_exact.first_filtered_sample(z, rate, trust, [x_init[0], x_init[1] * rate, x_init[2] * rate * rate])
    if z[1] != z[0]:
        assert abs(divided - want) > 1000 * TOL * max(1.0, abs(want)), f'{what}: the pin cannot tell the two states apart'
    d = abs(first_sample - want) / max(1.0, abs(want))
    assert d <= TOL, f'{what}: first filtered sample {d:.3e} from the closed form ({abs(first_sample - divided) / max(1.0, abs(want)):.3e} from the divided state)'


def test_initial_state_of_the_oracle(gold):
    for i, z, rate, trust in initial_state_cases(gold):
        got = fr.kalman_filter_1d(z, rate, trust, False)
        check_initial_state(got[0], z, rate, trust, f'oracle, column {i} ({rate} fps, trust {trust})')


def test_smooth_values_through_the_host_mirror(gold):
    """filtering.kalman_filter sends smoothing on only for True / 1, as the reference's `smooth == True` on int(smooth)
    does (:395, :418): 2 filters without smoothing."""
    from pose2sim_amd import filtering
    g = gold
    i = 0
    col, rate, trust, _ = _case(g, i)
    data = np.stack([col, col[::-1]], axis=1)
    got = {repr(s): filtering.kalman_filter(data, rate, trust, s, engine=OracleFilterEngine()) for s in (True, False, 1, 0, 2)}
    for c in range(2):
        _close(got['True'][:, c], fr.kalman_filter_1d(data[:, c], rate, trust, True), 'smoother')
        _close(got['False'][:, c], fr.kalman_filter_1d(data[:, c], rate, trust, False), 'filter')
    _close(got['True'][:, 0], g[f'col{i}_exact'], 'smoother against the exact values')
    assert np.abs(got['True'] - got['False']).max() > 1e-6
    assert np.array_equal(got['1'], got['True']) and np.array_equal(got['0'], got['False'])
    assert np.array_equal(got['2'], got['False'])
    for j in range(int(g['n_cols'])):                   # and every recorded column with its own recorded value
        col, rate, trust, smooth = _case(g, j)
        got = filtering.kalman_filter(col.reshape(-1, 1), rate, trust, smooth, engine=OracleFilterEngine())[:, 0]
        _close(got, g[f'col{j}_out'], f'column {j}, smooth {smooth!r}')


def _write_trial(root, g, i):
    trial = root / f'trial{i}'
    (trial / 'pose-3d').mkdir(parents=True)
    (trial / 'pose-3d' / str(g[f'file{i}_name'])).write_text(str(g[f'file{i}_text']))
    return trial, kalman_config(str(trial), int(g[f'file{i}_rate']), int(g[f'file{i}_trust']), bool(g[f'file{i}_smooth']))


def kalman_config(trial, rate, trust, smooth):
    return {'project': {'project_dir': trial, 'frame_rate': rate, 'frame_range': 'auto'}, 'pose': {'vid_img_extension': 'mp4'},
            'filtering': {'type': 'kalman', 'filter': True, 'reject_outliers': False, 'make_c3d': False,
                          'kalman': {'trust_ratio': trust, 'smooth': smooth}}}


def compare_trc_text(got_text, want_text, what, tol=TOL):
    """Header lines and frame / time columns exactly, coordinates within tol, empty fields in the same places."""
    got, want = got_text.split('\n'), want_text.split('\n')
    assert got[:5] == want[:5] and len(got) == len(want), what
    worst = 0.0
    for gl, wl in zip(got[5:], want[5:]):
        gf, wf = gl.split('\t'), wl.split('\t')
        assert gf[:2] == wf[:2] and len(gf) == len(wf), what
        a = np.array([float(v) if v else np.nan for v in gf[2:]])
        b = np.array([float(v) if v else np.nan for v in wf[2:]])
        worst = max(worst, _close(a, b, what, tol))
    return worst


def test_filter_all_kalman_against_the_recorded_files(work_dir, gold):
    from pose2sim_amd import filtering
    g = gold
    smooths = set()
    for i in range(int(g['n_files'])):
        trial, cfg = _write_trial(work_dir, g, i)
        paths = filtering.filter_all(cfg, engine=OracleFilterEngine())
        assert [os.path.basename(p) for p in paths] == [str(g[f'file{i}_out_name'])]
        d = compare_trc_text(open(paths[0]).read(), str(g[f'file{i}_out_text']), f'file {i}')
        print(f'file {i}: worst coordinate {d:.2e} from the recorded text')
        smooths.add(cfg['filtering']['kalman']['smooth'])
    assert smooths == {True, False}


def test_smooth_2_filters_and_still_reports_a_smoother(work_dir, gold, caplog):
    """smooth = 2: the numbers are the filter's alone (the reference compares int(smooth) with True), the report still
    says "smoother" (its log line tests plain truthiness, :685)."""
    from pose2sim_amd import filtering, trc
    g = gold
    trial, cfg = _write_trial(work_dir, g, 1)
    assert cfg['filtering']['kalman']['smooth'] is False
    cfg['filtering']['kalman']['smooth'] = 2
    with caplog.at_level(logging.INFO):
        paths = filtering.filter_all(cfg, engine=OracleFilterEngine())
    assert '--> Filter type: Kalman smoother. Measurements trusted 20 times as much as previous data' in caplog.text
    compare_trc_text(open(paths[0]).read(), str(g['file1_out_text']), 'smooth = 2 against the filter-only file')
    data = trc.load_trc(paths[0])[2]
    cfg['filtering']['kalman']['smooth'] = 1
    os.remove(paths[0])
    smoothed = trc.load_trc(filtering.filter_all(cfg, engine=OracleFilterEngine())[0])[2]
    assert np.nanmax(np.abs(smoothed - data)) > 1e-6
