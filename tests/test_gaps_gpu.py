"""The gap steps after triangulation on the GPU (csrc/p2s_gaps.hip): the recorded columns and the generated cases of
tests/gaps_numpy.py through a context.  Kinds None and 'linear', fill_gaps and gap_runs are compared exactly; the spline
kinds with scipy within the project's 1e-7 m and, up to 257 frames, within 8 x max(d_ref, 2^-52 scale), d_ref being scipy's
own distance to the 60-digit solve of tests/gaps_exact.py.  Then the workspace cap, the refusals, a table that is too
small, the stage timer, and the stage with and without the kernels."""
import ast
import ctypes as C
import logging
import os
import sys

import numpy as np
import pytest

import gaps_numpy as gn
from pose2sim_amd import _lib, triangulation
from pose2sim_amd.engine import Engine

pytestmark = pytest.mark.gpu

SHAPES = [(F, Cn) for F in gn.LENGTHS for Cn in gn.COLUMNS]


@pytest.fixture(scope='module')
def engine():
    import __graft_entry__ as entry
    entry.build_hip()
    eng = Engine(0)
    yield eng
    eng.close()


def test_recorded_columns(engine, golden_dir):
    gn.check_golden(engine.interpolate_gaps, golden_dir, verbose=True)


@pytest.mark.parametrize('kind', gn.KINDS)
@pytest.mark.parametrize('F,Cn', SHAPES)
def test_generated_cases(engine, F, Cn, kind):
    """Every max_gap of (1, 20, inf) on the case of F frames and Cn columns."""
    compared, left_out = gn.check_interpolation(engine.interpolate_gaps, F, Cn, kind, verbose=True)
    assert left_out * 20 <= Cn


@pytest.mark.parametrize('F,Cn', SHAPES)
def test_fill_gaps_and_gap_runs(engine, F, Cn):
    gn.check_fill(engine.fill_gaps, F, Cn)
    gn.check_runs(engine.gap_runs, F, Cn)


def test_columns_go_through_a_capped_workspace_in_chunks(engine):
    """20 000 frames x 6 columns, 'cubic': a column's rows take 7 x 8 x 20 000 bytes = 1 094 KiB, so a cap of 2 400 KiB holds
    2 columns and the 6 go in 3 chunks -- the same bits as in one."""
    F, Cn = 20000, 6
    coords, labels = gn.case(F, Cn)
    want, status = gn.interpolate(coords, labels, 20, 'cubic', gn.case_patches(F, Cn, 'cubic'))
    whole, st_whole = engine.interpolate_gaps(coords, labels, 20, 'cubic')
    engine.set_tuning(Engine.TUNE_GAPS_WORKSPACE_KB, 2400)
    try:
        chunked, st_chunked = engine.interpolate_gaps(coords, labels, 20, 'cubic')
    finally:
        engine.set_tuning(Engine.TUNE_GAPS_WORKSPACE_KB, 256 * 1024)
    assert gn.same(chunked, whole) and np.array_equal(st_chunked, st_whole) and np.array_equal(st_whole, status)
    assert status[gn.WITH_INF] == gn.NONFINITE and status.sum() == gn.NONFINITE
    assert np.array_equal(np.isnan(whole), np.isnan(want))
    took = gn.bad_samples(coords) & np.isfinite(want)
    assert took.sum() > 1000
    gn.assert_within_project_bar(whole[took], want[took], 'chunks')
    with pytest.raises(_lib.P2sError, match='workspace cap'):
        engine.set_tuning(Engine.TUNE_GAPS_WORKSPACE_KB, 0)


def test_refusals_write_nothing(engine):
    lib = engine._lib
    ptr = lambda a: a.ctypes.data_as(C.c_void_p)                    # noqa: E731
    x, labels = np.ones((4, 2)), np.arange(4, dtype=np.int64)
    out, status, table = np.full((4, 2), 7.0), np.full(2, 7, dtype=np.int32), np.full((4, 4), 7, dtype=np.int32)
    count, over = C.c_int64(7), C.c_int32(7)
    interp = lambda F, Cn, lab, kind: lib.p2s_interpolate_gaps(engine._h, F, Cn, ptr(x), ptr(lab), 3.0, kind, ptr(out), ptr(status))   # noqa: E731
    for args, text in (((0, 2, labels, 1), 'n_frames=0 outside [1, 2^30]'), ((4, 0, labels, 1), 'n_cols=0 outside [1, 65535]'),
                       ((4, 2, labels, 5), 'unknown interpolation kind 5'),
                       ((4, 2, np.array([0, 1, 1, 2], dtype=np.int64), 1), 'labels must increase (frame 2)'),
                       ((4, 2, np.array([0, 3, 2, 4], dtype=np.int64), 4), 'labels must increase (frame 2)')):
        assert interp(*args) == _lib.P2S_ERR_INVALID_ARG and lib.p2s_last_error().decode() == text
    assert lib.p2s_fill_gaps(engine._h, 0, 2, ptr(x), 1, ptr(out)) == _lib.P2S_ERR_INVALID_ARG
    assert lib.p2s_fill_gaps(engine._h, 4, 0, ptr(x), 1, ptr(out)) == _lib.P2S_ERR_INVALID_ARG
    assert lib.p2s_gap_runs(engine._h, 0, 2, ptr(x), 0, 4, 3.0, 4, ptr(table), C.byref(count), C.byref(over)) == _lib.P2S_ERR_INVALID_ARG
    assert lib.p2s_gap_runs(engine._h, 4, 2, ptr(x), 0, 4, 3.0, -1, ptr(table), C.byref(count), C.byref(over)) == _lib.P2S_ERR_INVALID_ARG
    assert (out == 7).all() and (status == 7).all() and (table == 7).all() and count.value == 7 and over.value == 7
    with pytest.raises(_lib.P2sError, match='unknown interpolation kind'):
        engine.interpolate_gaps(x, labels, 3, 'nearest')


def test_a_table_that_is_too_small_reports_overflow(engine):
    x = gn.case(1025, 78)[0]
    full = gn.runs_table(x, -1, 1025, 20)
    assert len(full) > 1000
    table, count, over = engine.gap_runs(x, -1, 1025, 20, raw=True)
    assert np.array_equal(table, full) and count == len(full) and not over
    for cap in (0, 3, len(full) - 1, len(full)):
        table, count, over = engine.gap_runs(x, -1, 1025, 20, capacity=cap, raw=True)
        assert over == (cap < len(full)) and count == len(full) and np.array_equal(table, full[:cap])
    with pytest.raises(_lib.P2sError, match='do not fit'):
        engine.gap_runs(x, -1, 1025, 20, capacity=3)


def test_kernel_time(engine):
    fresh = Engine(0)
    with pytest.raises(_lib.P2sError, match='none of p2s_interpolate_gaps, p2s_fill_gaps and p2s_gap_runs has run on this context'):
        fresh.gaps_kernel_ms()
    fresh.close()
    coords, labels = gn.case(257, 3)
    engine.interpolate_gaps(coords, labels, 20, 'cubic')
    assert engine.gaps_kernel_ms() > 0.0
    engine.fill_gaps(coords, 'last_value')
    assert engine.gaps_kernel_ms() > 0.0
    engine.gap_runs(coords, -1, 257, 20)
    assert engine.gaps_kernel_ms() > 0.0


def test_stage_with_and_without_the_kernels(engine, golden_dir, tmp_path, monkeypatch, caplog):
    """The recorded trials through triangulate_all with the gap kernels and with the three Engine methods refusing (the
    host functions): the same .trc bytes and the same log, with 'linear' interpolation (bit for bit) and every filler."""
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden'))
    import e2e_common as ec
    from pose2sim_amd import skeletons
    z = np.load(os.path.join(golden_dir, 'e2e_trc.npz'), allow_pickle=False)
    ids, _, _ = skeletons.keypoints('HALPE_26')
    calls = []
    real = {name: getattr(Engine, name) for name in ('interpolate_gaps', 'fill_gaps', 'gap_runs')}

    def counted(name):
        def method(self, *args, **kwargs):
            calls.append(name)
            return real[name](self, *args, **kwargs)
        return method

    def refusing(self, *args, **kwargs):
        calls.append('refused')
        raise NotImplementedError

    for name, filler in (('multi', 'last_value'), ('single_opts', 'zeros')):
        tri = {str(k): ast.literal_eval(str(v)) for k, v in zip(z[f'{name}_tri_keys'], z[f'{name}_tri_vals'])}
        tri.update(interpolation='linear', fill_large_gaps_with=filler, show_interp_indices=True)
        cams = ec.cams_from_arrays(z, f'{name}_')
        people = ec.people_from_xyl(z[f'{name}_xyl'], ids, 26)
        runs = []
        for how in ('kernels', 'host'):
            for method in real:
                monkeypatch.setattr(Engine, method, counted(method) if how == 'kernels' else refusing)
            del calls[:]
            root = str(tmp_path / f'{name}_{how}')
            trial = ec.write_trial(root, 'trial_' + name, cams, people, json_subdir=str(z[f'{name}_json_subdir']))
            cfg = ec.base_config(trial, bool(z[f'{name}_multi']), **tri)
            monkeypatch.chdir(root)
            caplog.clear()
            with caplog.at_level(logging.INFO):
                paths = triangulation.triangulate_all(cfg)
            texts = {os.path.basename(p): open(p, 'rb').read() for p in paths if p}
            runs.append((texts, [(r.levelno, r.getMessage().replace(root, '<root>')) for r in caplog.records], list(calls)))
        n_files = len(runs[0][0])
        assert n_files >= 1 and runs[0][0] == runs[1][0]
        assert runs[0][1] == runs[1][1] and len(runs[0][1]) > 10
        assert runs[0][2].count('interpolate_gaps') == 1 and runs[0][2].count('fill_gaps') == n_files and runs[0][2].count('gap_runs') == n_files
        assert runs[1][2] == ['refused']
