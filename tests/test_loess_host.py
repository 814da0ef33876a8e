"""The loess filter type on CPU, pinned to the reference's own code and to an exact solve of the definition.

tests/golden/loess_units.npz (<- make_golden_loess.py) holds columns run through the reference's own loess_filter_1d and
files written by its filter_all, with statsmodels' lowess replaced by tests/golden/statsmodels_standin.py (statsmodels has
never run here: all of this is parity-unpinned against it), and next to each column the exact values of the definition
(tests/loess_exact.py, the weighted least-squares line of every sample at 60 digits).  Checked here: the stand-in and the
stored exact values against a fresh exact solve (the goldens' provenance), the reference outputs against the exact
values, the host mirror of the kernel (tests/loess_numpy.py) against both, filter_all with the mirror as engine against
the recorded files, the report line, the `LOESS` key, the refusal of nb_values_used < 2, Pose2Sim.filtering() on a
Config.toml that says type = 'loess', and the C-ABI entry's declaration, export and binding.

Bars: the project's 1e-9 relative to max(1, |value|) with identical NaN pattern for the mirror (tests/test_loess_gpu.py
holds the kernel to the same), copied samples bit-equal; 1e-10 for the recorded reference outputs and the stand-in
against the exact solve (the limit the generator refuses to exceed; measured: 9.7e-12 at frame 98 765, where the
stand-in's sums over absolute frame indices lose about frame index x eps; the mirror's centred sums stay below 1e-14)."""
import logging
import os
import sys
import types

import numpy as np
import pytest

import loess_exact
from loess_numpy import NumpyLoessEngine, interior_weights, loess_columns
from test_filter_oracle import OracleFilterEngine
from test_kalman_host import compare_trc_text

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden'))
import statsmodels_standin  # noqa: E402

TOL = 1e-9                     # the project's bar (test_filter_gpu.TOL)
REFERENCE_TOL = 1e-10          # the reference's float64 sums against the exact solve
NB_VALUES = (2, 3, 4, 5, 5.5, 6, 30, 31, 257)


@pytest.fixture(scope='module')
def gold(golden_dir):
    return np.load(os.path.join(golden_dir, 'loess_units.npz'))


@pytest.fixture
def work_dir():
    """A scratch directory whose path does not contain 'filt' (filter_all skips every .trc whose path does)."""
    import shutil
    import tempfile
    from pathlib import Path
    d = tempfile.mkdtemp(prefix='p2s_loess_')
    yield Path(d)
    shutil.rmtree(d, ignore_errors=True)


def nb_of(g, i):
    nb = float(g[f'col{i}_nb'])
    return int(nb) if nb == int(nb) else nb


def distance(got, want, what):
    assert got.shape == want.shape and np.array_equal(np.isnan(got), np.isnan(want)), f'{what}: NaN pattern'
    ok = ~np.isnan(want)
    return float((np.abs(got[ok] - want[ok]) / np.maximum(1.0, np.abs(want[ok]))).max()) if ok.any() else 0.0


def filtered_mask(col, nb):
    mask = np.zeros(len(col), dtype=bool)
    for seq in loess_exact.runs(col, nb):
        mask[seq] = True
    return mask


def check_column(got, g, i, who):
    """`got` for golden column i: within TOL of the reference's output and of the exact values, copied samples bit-equal."""
    col, nb = g[f'col{i}_in'], nb_of(g, i)
    what = f'{who}, column {i} (nb_values_used {nb}, {len(col)} frames)'
    d_ref, d_exact = distance(got, g[f'col{i}_out'], what), distance(got, g[f'col{i}_exact'], what)
    assert d_ref <= TOL and d_exact <= TOL, f'{what}: {d_ref:.3e} from the reference, {d_exact:.3e} from the exact values'
    copied = ~filtered_mask(col, nb)
    assert np.array_equal(got[copied], col[copied], equal_nan=True), what
    return d_ref, d_exact


def test_fixture_covers_what_it_should(gold):
    g = gold
    n = int(g['n_cols'])
    assert {nb_of(g, i) for i in range(n)} == set(NB_VALUES)
    for nb in NB_VALUES:
        n0 = int(np.floor(nb))
        cols = [g[f'col{i}_in'] for i in range(n) if nb_of(g, i) == nb]
        lengths, at_first, at_last, zero_inside = set(), False, False, False
        for col in cols:
            good = np.where(~np.isnan(col))[0]
            for seq in (np.split(good, np.where(np.diff(good) > 1)[0] + 1) if good.size else []):
                lengths.add(len(seq))
                if len(seq) > nb:
                    at_first |= seq[0] == 0
                    at_last |= seq[-1] == len(col) - 1
                    zero_inside |= bool((col[seq] == 0).any())
        assert {n0, n0 + 1} <= lengths and max(lengths) <= 400, nb
        assert at_first and at_last and zero_inside, nb
        assert {1, n0 + 1} <= {len(c) for c in cols}, nb
        values = [c[~np.isnan(c)] for c in cols if not np.isnan(c).all()]
        assert any(v.min() < -100 for v in values) and any(0 < v.max() < 100 for v in values), nb      # scales -1000 and 1
    cols = [g[f'col{i}_in'] for i in range(n)]
    assert any(np.isnan(c).all() for c in cols)
    assert any(len(c) > 99000 for c in cols) and max(len(c) for c in cols) <= 100000
    gaps = 0
    for c in cols:
        isn = np.isnan(c)
        gaps += int((isn[1:-1] & ~isn[:-2] & ~isn[2:]).sum())
    assert gaps >= len(NB_VALUES)                       # runs split by one NaN
    for i in range(n):
        assert f'col{i}_out' in g.files and f'col{i}_exact' in g.files, i
    assert {str(g[f'file{i}_key']) for i in range(int(g['n_files']))} == {'loess', 'LOESS'}


PROVENANCE_COLUMNS = (0, 7, 13, 18, 24, 31, 37, 42, 52, 55)


def test_standin_and_stored_exact_values_against_a_fresh_exact_solve(gold):
    """The goldens' provenance: on a handful of columns (every parity of k, both scales, zeros, a run at frame 99 000) the
    exact solve is recomputed here; the stored exact values must equal it bit for bit, and the stand-in -- called by this
    test run by run, not by the reference -- must meet it."""
    g = gold
    for i in PROVENANCE_COLUMNS:
        col, nb = g[f'col{i}_in'], nb_of(g, i)
        exact = loess_exact.column(col, nb)
        assert np.array_equal(exact, g[f'col{i}_exact'], equal_nan=True), i
        got = col.copy()
        for seq in loess_exact.runs(col, nb):
            got[seq] = statsmodels_standin.lowess(col[seq], seq, is_sorted=True, frac=nb / len(seq), it=0)[:, 1]
        d = distance(got, exact, f'stand-in, column {i}')
        print(f'column {i}: nb_values_used {nb}: |stand-in - exact| = {d:.2e}')
        assert d <= REFERENCE_TOL, (i, d)


def test_reference_outputs_against_the_exact_values(gold):
    g = gold
    worst = 0.0
    for i in range(int(g['n_cols'])):
        col, out, exact, nb = g[f'col{i}_in'], g[f'col{i}_out'], g[f'col{i}_exact'], nb_of(g, i)
        d = distance(out, exact, f'reference output, column {i}')
        assert d <= REFERENCE_TOL, (i, d)
        worst = max(worst, d)
        copied = ~filtered_mask(col, nb)
        assert np.array_equal(out[copied], col[copied], equal_nan=True), i
        assert np.array_equal(exact[copied], col[copied], equal_nan=True), i
    print(f'worst |reference - exact| = {worst:.2e}')


def test_mirror_against_every_golden_column(gold):
    """tests/loess_numpy.py (the kernel's arithmetic in NumPy) against what the reference's code returned and against the
    exact values.  Measured: worst 9.7e-12 from the reference (its own distance from exact at frame 98 765), 8.5e-15 from
    the exact values."""
    g = gold
    worst_ref = worst_exact = 0.0
    for i in range(int(g['n_cols'])):
        got = loess_columns(g[f'col{i}_in'].reshape(-1, 1), nb_of(g, i))[:, 0]
        d_ref, d_exact = check_column(got, g, i, 'mirror')
        worst_ref, worst_exact = max(worst_ref, d_ref), max(worst_exact, d_exact)
    print(f'worst: {worst_ref:.2e} from the reference, {worst_exact:.2e} from the exact values')


def test_interior_window_is_a_fixed_fir(gold):
    """Away from a run's ends the window is symmetric and the fit is the tricube-weighted mean: the mirror's table
    against the exact values, for odd and even k."""
    rng = np.random.default_rng(11)
    for k in (4, 5, 6, 7, 30, 31):
        y = rng.normal(0, 1, 3 * k)
        exact = loess_exact.run(y, k)
        wn = interior_weights(k)
        m = k // 2
        assert abs(wn[0] + 2 * wn[1:].sum() - 1.0) <= 4e-16
        for i in range(m, len(y) - k + m + 1):
            fir = sum(wn[abs(u)] * y[i + u] for u in range(-(m - 1), m))
            assert abs(fir - exact[i]) <= 1e-13 * max(1.0, abs(exact[i])), (k, i)


def loess_config(trial, rate, nb, key='loess'):
    return {'project': {'project_dir': trial, 'frame_rate': rate, 'frame_range': 'auto'}, 'pose': {'vid_img_extension': 'mp4'},
            'filtering': {'type': 'loess', 'filter': True, 'reject_outliers': False, 'make_c3d': False, key: {'nb_values_used': nb}}}


def write_trial(root, g, i):
    trial = root / f'trial{i}'
    (trial / 'pose-3d').mkdir(parents=True)
    (trial / 'pose-3d' / str(g[f'file{i}_name'])).write_text(str(g[f'file{i}_text']))
    return trial, loess_config(str(trial), int(g[f'file{i}_rate']), int(g[f'file{i}_nb']), str(g[f'file{i}_key']))


def test_filter_all_loess_against_the_recorded_files(work_dir, gold, caplog):
    """filter_all with the mirror as engine writes the reference's file name, and its text: header lines, frame and time
    columns and empty fields exactly.  The coordinates are compared as parsed values within TOL, not byte for byte: the
    reference's text holds the stand-in's sums over absolute frame indices, the mirror's sums are centred, and the last
    of the 17 digits written differs in most fields (the count is printed)."""
    from pose2sim_amd import filtering
    g = gold
    keys = set()
    for i in range(int(g['n_files'])):
        trial, cfg = write_trial(work_dir, g, i)
        caplog.clear()
        with caplog.at_level(logging.INFO):
            paths = filtering.filter_all(cfg, engine=NumpyLoessEngine())
        assert [os.path.basename(p) for p in paths] == [str(g[f'file{i}_out_name'])]
        assert paths[0].endswith('_filt_loess.trc')
        got, want = open(paths[0]).read(), str(g[f'file{i}_out_text'])
        d = compare_trc_text(got, want, f'file {i}', TOL)
        same = sum(a == b for a, b in zip(got.split('\n'), want.split('\n')))
        print(f'file {i}: worst coordinate {d:.2e} from the recorded text; {same} of {len(want.splitlines())} lines byte-equal')
        assert [r.getMessage() for r in caplog.records if r.getMessage().startswith('--> Filter type')] == \
            [f"--> Filter type: LOESS. Number of values used: {int(g[f'file{i}_nb'])}"]
        keys.add(str(g[f'file{i}_key']))
    assert keys == {'loess', 'LOESS'}                   # the `LOESS` key is read as the reference reads it


def test_recap_line_is_the_reference_text():
    from pose2sim_amd.filtering import _TYPE_LINES
    line = _TYPE_LINES['loess']
    assert line({'loess': {'nb_values_used': 5}}) == '--> Filter type: LOESS. Number of values used: 5'
    assert line({'LOESS': {'nb_values_used': 5.5}}) == '--> Filter type: LOESS. Number of values used: 5.5'
    assert line({'loess': {'nb_values_used': 7}, 'LOESS': {'nb_values_used': 9}}) == '--> Filter type: LOESS. Number of values used: 7'


def test_the_loess_key_wins_over_the_LOESS_key(gold):
    from pose2sim_amd import filtering
    data = gold['col18_in'].reshape(-1, 1)
    fcfg = {'loess': {'nb_values_used': 5}, 'LOESS': {'nb_values_used': 3}}
    got = filtering._apply('loess', fcfg, data, 60, NumpyLoessEngine())
    assert np.array_equal(got, loess_columns(data, 5), equal_nan=True)
    got = filtering._apply('loess', {'LOESS': {'nb_values_used': 3}}, data, 60, NumpyLoessEngine())
    assert np.array_equal(got, loess_columns(data, 3), equal_nan=True)


@pytest.mark.parametrize('nb', [1, 1.9, 0, -3, float('nan')])
def test_a_window_of_fewer_than_two_samples_raises(nb, work_dir, gold):
    from pose2sim_amd import filtering
    from pose2sim_amd.engine import loess_window
    with pytest.raises(ValueError):
        loess_window(nb)
    with pytest.raises(ValueError):
        filtering.loess_filter(np.ones((8, 2)), nb, engine=NumpyLoessEngine())
    trial, cfg = write_trial(work_dir, gold, 0)
    cfg['filtering']['loess']['nb_values_used'] = nb
    with pytest.raises(ValueError):
        filtering.filter_all(cfg, engine=NumpyLoessEngine())
    assert [f for f in os.listdir(trial / 'pose-3d') if 'filt' in f] == []


def test_window_and_shortest_run_follow_the_reference():
    """k = int(nb + 1e-10) is statsmodels' int(frac * n + 1e-10) for the reference's frac = nb / n at every run length, and
    the shortest filtered run is the first length > nb."""
    from pose2sim_amd.engine import loess_window
    for nb in NB_VALUES + (7, 2.5, 1001, 8191):
        k, min_run = loess_window(nb)
        assert min_run == int(np.floor(nb)) + 1 and k == int(np.floor(nb))
        for L in range(min_run, min_run + 2000):
            assert loess_exact.window(nb, L) == k, (nb, L)


def test_an_engine_without_loess_is_refused(work_dir, gold):
    from pose2sim_amd import filtering
    trial, cfg = write_trial(work_dir, gold, 0)
    with pytest.raises(NotImplementedError):
        filtering.filter_all(cfg, engine=OracleFilterEngine())
    assert [f for f in os.listdir(trial / 'pose-3d') if 'filt' in f] == []


def test_a_library_without_the_entry_is_refused():
    from pose2sim_amd.engine import Engine
    eng = Engine.__new__(Engine)
    eng._lib, eng._h = types.SimpleNamespace(), None
    with pytest.raises(NotImplementedError, match='p2s_loess_host'):
        eng.loess(np.ones((8, 1)), 5)


def test_pose2sim_filtering_runs_a_loess_config(work_dir, gold, monkeypatch):
    """Pose2Sim.filtering() on a trial whose Config.toml says type = 'loess' writes the reference's file (coordinates as
    parsed values within TOL, see test_filter_all_loess_against_the_recorded_files)."""
    from pose2sim_amd import Pose2Sim, filtering
    trial, _ = write_trial(work_dir, gold, 0)
    (trial / 'Config.toml').write_text('[project]\nframe_rate = 60\nframe_range = []\n\n[pose]\nvid_img_extension = "mp4"\n\n'
                                       '[logging]\nuse_custom_logging = true\n\n'
                                       '[filtering]\ntype = "loess"\nfilter = true\nreject_outliers = false\nmake_c3d = false\n'
                                       '[filtering.loess]\nnb_values_used = 5\n')
    monkeypatch.setattr(filtering, '_make_engine', lambda: NumpyLoessEngine())
    monkeypatch.chdir(trial)
    Pose2Sim.filtering()
    out = trial / 'pose-3d' / str(gold['file0_out_name'])
    compare_trc_text(out.read_text(), str(gold['file0_out_text']), 'Pose2Sim.filtering()', TOL)


def test_the_entry_is_declared_exported_and_optional():
    import ctypes
    from pose2sim_amd import _lib
    name = 'p2s_loess_host'
    assert name in _lib.OPTIONAL and name in _lib.SIGNATURES
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    header = open(os.path.join(root, 'include', 'p2s.h')).read()
    assert f'int {name}(p2s_ctx *ctx, int64_t n_frames, int32_t n_cols, const double *data, int32_t k, int64_t min_run,' in header
    assert hasattr(ctypes.CDLL(_lib.LIB_PATH), name)


def test_no_filter_type_is_refused_any_more():
    from pose2sim_amd import filtering
    assert not hasattr(filtering, 'REFUSED_TYPES')
    assert set(filtering._TYPE_LINES) == {'butterworth', 'butterworth_on_speed', 'gaussian', 'median', 'one_euro', 'kalman', 'gcv_spline', 'loess'}
