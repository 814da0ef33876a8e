"""The gap steps after triangulation without a GPU: tests/gaps_numpy.py's mirror against postproc.py and against columns
recorded from the reference (tests/golden/gaps_units.npz <- make_golden_gaps.py), the 60-digit solve of tests/gaps_exact.py
against scipy, csrc/p2s_gaps.hip compiled for the host (ctx == NULL runs the functions the kernels run) against all of
them, and triangulation.finish_persons_engine with host doubles of the engine against finish_person."""
import ctypes
import logging
import os

import numpy as np
import pytest

import gaps_exact
import gaps_numpy as gn
from pose2sim_amd import _lib, engine, postproc, triangulation

HOST_CASES = [(F, C) for F in (5, 6, 63, 64, 65, 257) for C in (1, 3, 8)] + [(1025, 6), (4099, 5)]


@pytest.mark.parametrize('F,C', HOST_CASES)
def test_mirror_is_postproc(F, C):
    coords, labels = gn.case(F, C)
    for kind in gn.KINDS:
        for max_gap in gn.MAX_GAPS:
            got, status = gn.interpolate(coords, labels, max_gap, kind)
            cols = np.flatnonzero(status == 0)                    # a person with such a column stays on the host as a whole
            with np.errstate(all='ignore'):
                want = postproc.interpolate_gaps(coords[:, cols].copy(), labels, max_gap, kind)
            assert gn.same(got[:, cols], want), (kind, max_gap)
            assert gn.same(got[:, status != 0], coords[:, status != 0])
            assert bool(status.any()) == (kind in gn.SPLINE_KINDS and C > gn.WITH_INF and F >= 6)
    for table in gn.fill_inputs(F, C):
        for how in ('last_value', 'zeros', 'nan', None):
            assert gn.same(gn.fill(table, how), postproc.fill_gaps(table.copy(), how))
    x = gn.fill_inputs(F, C)[1]
    for max_gap in gn.MAX_GAPS:
        for first, last in ((-1, F), (1, F - 2), (F // 3, F - F // 4)):
            assert gn.runs(x, first, last, max_gap) == postproc.gap_spans(x, first, last, max_gap)


def test_generator_plants_what_it_promises():
    coords, labels = gn.case(4099, 8)
    bad = gn.bad_samples(coords)
    assert (~bad[:, gn.FIVE_GOOD]).sum() == 5 and (~bad[:, gn.FOUR_GOOD]).sum() == 4 and np.isnan(coords[:, gn.ALL_NAN]).all()
    assert np.isinf(coords[:, gn.WITH_INF]).sum() == 1 and bad[0, 0] and bad[-1, 0] and not (bad[0, 5] and bad[-1, 5])
    assert np.isnan(coords).any() and (coords == 0).any() and np.signbit(coords[coords == 0]).any() and not np.signbit(coords[coords == 0]).all()
    assert (np.diff(labels) == 2).sum() == 1
    for c in (0, 5, 6, 7):
        pos = np.flatnonzero(bad[:, c])
        lengths = set(gn.bad_runs(labels, pos)[1].tolist())
        assert set(gn.EXACT_RUNS) <= lengths, (c, lengths)
        assert all(bad[k - 1, c] and bad[k, c] for k in range(gn.TILE, 4099, gn.TILE))
        step = 4099 // 2
        assert bad[step - 1, c] and bad[step, c]                  # one run by position, two by label
    assert (~gn.bad_samples(gn.case(5, 1)[0])).sum() == 4 and (~gn.bad_samples(gn.case(6, 1)[0])).sum() == 5


def test_mirror_equals_the_golden(golden_dir):
    gn.check_golden(gn.interpolate, golden_dir)


def test_exact_solve_agrees_with_scipy_to_d_ref(golden_dir):
    """The recorded exact values are what gaps_exact computes here, and scipy (the mirror) is d_ref away from them --
    recorded and recomputed: the reference's interp1d is this machine's."""
    n = 0
    for i, z, kind in gn.golden_cases(golden_dir):
        if kind not in gn.SPLINE_KINDS:
            continue
        col, index = z[f'c{i}_col'], z[f'c{i}_index']
        patch = gaps_exact.column(col, index, kind)
        if patch is None:
            assert np.isnan(z[f'c{i}_exact']).all()
            continue
        assert np.array_equal(z[f'c{i}_exact'][patch[0]], patch[1])
        scipy_values = gn.interpolants(col[:, None], index, kind)[0][1]
        took = np.isfinite(z[f'c{i}_out'][patch[0]])
        d = np.abs(scipy_values[took] - patch[1][took]).max() if took.any() else 0.0
        assert d == float(z[f'c{i}_d_ref']), (i, kind, d)
        assert d <= 1e-9 * max(1.0, float(z[f'c{i}_scale']))      # scipy is right to rounding, and so is the exact solve
        n += 1
    assert n >= 20


def test_exact_knots_are_scipys():
    from scipy.interpolate import make_interp_spline
    x = np.array([3.0, 4, 6, 7, 11, 12, 13, 17])
    for k in (1, 2, 3):
        assert np.array_equal(gaps_exact.knots(x, k), make_interp_spline(x, np.ones(8), k=k).t)


# ---- csrc/p2s_gaps.hip on the host ---------------------------------------------------------------------------------------------
def test_library_exports_the_new_symbols():
    new = {'p2s_interpolate_gaps', 'p2s_fill_gaps', 'p2s_gap_runs', 'p2s_gaps_kernel_ms'}
    assert new <= _lib.OPTIONAL and new <= set(_lib.SIGNATURES)
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    header = open(os.path.join(root, 'include', 'p2s.h')).read()
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name in new:
        assert f'int {name}(' in header and hasattr(lib, name), name


def test_host_path_golden(golden_dir):
    gn.check_golden(engine.interpolate_gaps_host, golden_dir)


@pytest.mark.parametrize('kind', gn.KINDS)
@pytest.mark.parametrize('F,C', HOST_CASES)
def test_host_path_generated(F, C, kind):
    gn.check_interpolation(engine.interpolate_gaps_host, F, C, kind)


@pytest.mark.parametrize('F,C', HOST_CASES)
def test_host_path_fill_and_runs(F, C):
    gn.check_fill(engine.fill_gaps_host, F, C)
    gn.check_runs(engine.gap_runs_host, F, C)


def test_generated_cases_left_out_of_the_exact_comparison():
    """At most 1 column in 20 of the GPU test's cases may be left out of the value comparison (scipy's own answer is not
    finite there): counted here on the columns themselves, without solving anything."""
    for F in gn.LENGTHS:
        for C in gn.COLUMNS:
            coords = gn.case(F, C)[0]
            out = sum(bool(gn.column_status(coords[:, c], 'cubic')) for c in range(C))
            assert out * 20 <= C, (F, C, out)


def test_host_path_refuses_and_writes_nothing():
    lib = _lib.load()
    ptr = lambda a: a.ctypes.data_as(ctypes.c_void_p)                # noqa: E731
    x, labels = np.ones((4, 2)), np.arange(4, dtype=np.int64)
    out, status, table = np.full((4, 2), 7.0), np.full(2, 7, dtype=np.int32), np.full((4, 4), 7, dtype=np.int32)
    count, over = ctypes.c_int64(7), ctypes.c_int32(7)
    interp = lambda F, C, lab, kind: lib.p2s_interpolate_gaps(None, F, C, ptr(x), ptr(lab), 3.0, kind, ptr(out), ptr(status))   # noqa: E731
    for args, text in (((0, 2, labels, 1), 'n_frames=0 outside [1, 2^30]'), ((4, 0, labels, 1), 'n_cols=0 outside [1, 65535]'),
                       ((4, 2, labels, 5), 'unknown interpolation kind 5'), ((4, 2, labels, -1), 'unknown interpolation kind -1'),
                       ((4, 2, np.array([0, 1, 1, 2], dtype=np.int64), 1), 'labels must increase (frame 2)'),
                       ((4, 2, np.array([0, 3, 2, 4], dtype=np.int64), 4), 'labels must increase (frame 2)')):
        assert interp(*args) == _lib.P2S_ERR_INVALID_ARG and lib.p2s_last_error().decode() == text
    assert lib.p2s_fill_gaps(None, 0, 2, ptr(x), 1, ptr(out)) == _lib.P2S_ERR_INVALID_ARG
    assert lib.p2s_fill_gaps(None, 4, -1, ptr(x), 1, ptr(out)) == _lib.P2S_ERR_INVALID_ARG
    assert lib.p2s_gap_runs(None, 0, 2, ptr(x), 0, 4, 3.0, 4, ptr(table), ctypes.byref(count), ctypes.byref(over)) == _lib.P2S_ERR_INVALID_ARG
    assert lib.p2s_gap_runs(None, 4, 2, ptr(x), 0, 4, 3.0, -1, ptr(table), ctypes.byref(count), ctypes.byref(over)) == _lib.P2S_ERR_INVALID_ARG
    assert (out == 7).all() and (status == 7).all() and (table == 7).all() and count.value == 7 and over.value == 7
    with pytest.raises(_lib.P2sError, match='unknown interpolation kind'):
        engine.interpolate_gaps_host(x, labels, 3, 'nearest')


def test_host_path_reports_a_table_that_is_too_small():
    x = gn.fill_inputs(257, 8)[1]
    full = gn.runs_table(x, -1, 257, 20)
    assert len(full) > 10
    table, count, over = engine.gap_runs_host(x, -1, 257, 20, raw=True)
    assert np.array_equal(table, full) and count == len(full) and not over
    table, count, over = engine.gap_runs_host(x, -1, 257, 20, capacity=len(full), raw=True)
    assert np.array_equal(table, full) and not over
    for cap in (0, 3, len(full) - 1):
        table, count, over = engine.gap_runs_host(x, -1, 257, 20, capacity=cap, raw=True)
        assert over and count == len(full) and np.array_equal(table, full[:cap])
    with pytest.raises(_lib.P2sError, match='do not fit'):
        engine.gap_runs_host(x, -1, 257, 20, capacity=3)


# ---- the stage -----------------------------------------------------------------------------------------------------------------
KPTS = ('Hip', 'Knee', 'Ankle', 'Toe')


def _trial(tmp_path, name, kind='cubic', fill='last_value'):
    """A trial of 2 persons, 140 frames from frame 7, 4 keypoints: the tables, the per-frame means and the settings."""
    F, P, K3 = 140, 2, 3 * len(KPTS)
    table = gn.case(F, P * K3 + 5)[0][:, 5:]                      # past the columns with a planted peculiarity
    coords = [np.ascontiguousarray(table[:, n * K3:(n + 1) * K3]) for n in range(P)]
    rng = np.random.default_rng(5)
    err, excl = rng.uniform(1, 5, (F, P)), rng.uniform(0, 2, (F, P))
    err[:6, 0] = np.nan; err[100:104, 1] = np.nan; err[131:, 1] = np.nan
    root = tmp_path / name / 'trial'
    os.makedirs(root)
    settings = {'interpolation': kind, 'max_gap': 20, 'remove_incomplete_frames': False, 'sections_to_keep': 'largest', 'min_chunk_size': 10,
                'fill_large_gaps_with': fill, 'show_interp_indices': True, 'make_c3d': False}
    config = {'project': {'project_dir': str(root), 'multi_person': True, 'frame_rate': 60}}
    return coords, err, excl, np.arange(7, 7 + F), settings, config


def _facts(people, root):
    out = []
    for p in people:
        text = open(p.trc_path, 'rb').read() if p.trc_path else b''
        out.append((p.start, p.end, p.kept, os.path.relpath(p.trc_path, root) if p.trc_path else '', text, p.err_mean, p.excl_mean,
                    p.interpolated, p.not_interpolated))
    return out


class OldEngine:
    """An engine from before the gap calls."""


@pytest.mark.parametrize('kind,fill', [('cubic', 'last_value'), ('linear', 'zeros'), ('slinear', 'nan'), ('none', 'last_value'), ('nearest', 'zeros')])
def test_finish_persons_engine_is_finish_person(tmp_path, caplog, kind, fill):
    """The same .trc bytes, PersonTrial fields and log lines with the mirror behind the engine's method names, with an
    engine without the calls, and with one that reports a status for a column of person 1 -- whatever runs the steps."""
    results = []
    doubles = (None, gn.HostEngine(), OldEngine(), gn.HostEngine(status_columns=(3 * len(KPTS) + 2,)))
    for i, eng in enumerate(doubles):
        coords, err, excl, frames, settings, config = _trial(tmp_path, f'run{i}', kind, fill)
        caplog.clear()
        with caplog.at_level(logging.INFO):
            if eng is None:
                people = [triangulation.finish_person(n, coords[n], err[:, n], excl[:, n], frames, settings, config, KPTS, True) for n in range(2)]
            else:
                people = triangulation.finish_persons_engine(eng, coords, err, excl, frames, settings, config, KPTS, True)
        root = str(tmp_path / f'run{i}')
        results.append((_facts(people, root), [(r.levelno, r.getMessage().replace(root, '<root>')) for r in caplog.records]))
    want = results[0]
    assert len(want[0]) == 2 and all(f[2] and f[4] for f in want[0]) and want[0][0][0] == 6 and want[0][1][1] == 100
    assert any(any(want[0][n][8]) for n in range(2)) and (kind != 'none' or any(any(want[0][n][7]) for n in range(2)))    # spans to report
    for got in results[1:]:
        assert got == want
    known = kind in ('none',) + triangulation.GAP_KINDS_ENGINE
    assert doubles[1].calls == {'interpolate_gaps': int(known and kind != 'none'), 'fill_gaps': 2 * known, 'gap_runs': 2 * known}
    assert doubles[3].calls == ({'interpolate_gaps': 1, 'fill_gaps': 1, 'gap_runs': 1} if known and kind != 'none' else doubles[1].calls)


def test_engine_without_the_entries_refuses():
    class Old:
        pass
    eng = engine.Engine.__new__(engine.Engine)
    eng._lib, eng._h = Old(), None
    with pytest.raises(NotImplementedError):
        eng.interpolate_gaps(np.ones((5, 1)), np.arange(5), 3, 'linear')
    with pytest.raises(NotImplementedError):
        eng.fill_gaps(np.ones((5, 1)), 'zeros')
    with pytest.raises(NotImplementedError):
        eng.gap_runs(np.ones((5, 1)), 0, 5, 3)
    with pytest.raises(NotImplementedError):
        eng.gaps_kernel_ms()
