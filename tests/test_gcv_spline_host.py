"""The gcv_spline filter type on CPU: filtering.filter_all with a SciPy-backed test double of Engine.gcv_spline
(tests/gcv_scipy.py) must write the reference's .trc files byte for byte (tests/golden/gcv_units.npz <-
make_golden_gcv.py), log its recap line, and fail where the reference fails."""
import logging
import os

import numpy as np
import pytest

from gcv_scipy import gcv_spline_columns
from test_filter_oracle import OracleFilterEngine


class ScipyGcvEngine(OracleFilterEngine):
    """OracleFilterEngine (Hampel etc.) plus Engine.gcv_spline restated with make_smoothing_spline."""

    def gcv_spline(self, data, cutoff, smoothing_factor, frame_rate):
        return gcv_spline_columns(data, cutoff, smoothing_factor, frame_rate)


@pytest.fixture(scope='module')
def gold(golden_dir):
    return np.load(os.path.join(golden_dir, 'gcv_units.npz'))


def _text(gold, key):
    """A .trc text of the goldens (stored as its UTF-8 bytes)."""
    return gold[key].tobytes().decode('utf-8')


@pytest.fixture
def work_dir():
    """A scratch directory whose path does not contain 'filt' (the reference skips every .trc whose path does)."""
    import shutil
    import tempfile
    from pathlib import Path
    d = tempfile.mkdtemp(prefix='p2s_gcv_')
    yield Path(d)
    shutil.rmtree(d, ignore_errors=True)


def _trial(tmp_path, gold, i):
    cutoff, sf, reject, rate, frame_range = (str(v) for v in gold[f'file{i}_prm'])
    trial = tmp_path / f'trial{i}'
    (trial / 'pose-3d').mkdir(parents=True)
    (trial / 'pose-3d' / str(gold[f'file{i}_name'])).write_text(_text(gold, f'file{i}_text'))
    cfg = {'project': {'project_dir': str(trial), 'frame_rate': int(rate),
                       'frame_range': 'auto' if frame_range == 'auto' else [int(v) for v in frame_range.strip('[]').split(',')]},
           'pose': {'vid_img_extension': 'mp4'},
           'filtering': {'type': 'gcv_spline', 'filter': True, 'reject_outliers': reject == 'True', 'make_c3d': False,
                         'gcv_spline': {'cut_off_frequency': cutoff if cutoff == 'auto' else int(cutoff), 'smoothing_factor': float(sf)}}}
    return trial, cfg


def test_the_scipy_model_is_the_reference_on_every_golden_column(gold):
    """The double itself: bit for bit the reference's gcv_spline_filter_1d, lambdas included."""
    for i in range(int(gold['n_cols'])):
        auto, sf, cutoff, rate = gold[f'col{i}_prm']
        out, lam = gcv_spline_columns(gold[f'col{i}_in'][:, None], 'auto' if auto else int(cutoff), sf, int(rate))
        assert np.array_equal(out[:, 0], gold[f'col{i}_out'], equal_nan=True), i
        assert np.array_equal(lam[:, 0], gold[f'col{i}_lam'], equal_nan=True), i


def test_filter_all_writes_the_reference_files(work_dir, gold, caplog):
    from pose2sim_amd import filtering
    for i in range(int(gold['n_files'])):
        trial, cfg = _trial(work_dir, gold, i)
        caplog.clear()
        with caplog.at_level(logging.INFO):
            paths = filtering.filter_all(cfg, engine=ScipyGcvEngine())
        assert [os.path.basename(p) for p in paths] == [str(gold[f'file{i}_out_name'])], i
        assert open(paths[0]).read() == _text(gold, f'file{i}_out_text'), i
        assert [r.getMessage() for r in caplog.records if r.getMessage().startswith('--> Filter type')] == [str(gold[f'file{i}_recap'])], i


def test_recap_lines_are_the_reference_text():
    from pose2sim_amd.filtering import _TYPE_LINES
    line = _TYPE_LINES['gcv_spline']
    assert line({'gcv_spline': {'cut_off_frequency': 'auto', 'smoothing_factor': 2}}) == \
        '--> Filter type: Generalized Cross-Validation Spline. Optimal parameters automatically estimated with smoothing factor 2.0.'
    assert line({}) == \
        '--> Filter type: Generalized Cross-Validation Spline. Optimal parameters automatically estimated with smoothing factor 1.0.'
    assert line({'gcv_spline': {'cut_off_frequency': 6, 'smoothing_factor': 1.0}}) == \
        '--> Filter type: Generalized Cross-Validation Spline. Cut-off frequency {gcv_filter_cutoff} Hz.'


@pytest.mark.parametrize('mode', ['short_auto', 'short_fixed'])
def test_a_run_of_three_samples_raises_and_writes_nothing(work_dir, gold, mode):
    from pose2sim_amd import filtering
    trial, cfg = _trial(work_dir, gold, 0)
    name = str(gold['file0_name'])
    path = trial / 'pose-3d' / name
    lines = path.read_text().split('\n')
    rows = [r.split('\t') for r in lines[5:] if r]
    for k, v in enumerate(gold['short_in'][:len(rows)]):        # a run of 3 samples in marker 1's X column
        rows[k][2] = '' if np.isnan(v) else repr(float(v))
    path.write_text('\n'.join(lines[:5] + ['\t'.join(r) for r in rows]) + '\n')
    if mode == 'short_fixed':
        cfg['filtering']['gcv_spline']['cut_off_frequency'] = 6
    with pytest.raises(ValueError) as e:
        filtering.filter_all(cfg, engine=ScipyGcvEngine())
    assert type(e.value).__name__ == str(gold[f'{mode}_type']) and str(e.value) == str(gold[f'{mode}_msg'])
    assert [f for f in os.listdir(trial / 'pose-3d') if 'filt' in f] == []


def test_loess_is_still_refused(work_dir, gold):
    from pose2sim_amd import filtering
    trial, cfg = _trial(work_dir, gold, 0)
    cfg['filtering']['type'] = 'loess'
    with pytest.raises(NotImplementedError):
        filtering.filter_all(cfg, engine=ScipyGcvEngine())


def test_an_engine_without_gcv_spline_is_refused(work_dir, gold):
    from pose2sim_amd import filtering
    trial, cfg = _trial(work_dir, gold, 1)
    with pytest.raises(NotImplementedError):
        filtering.filter_all(cfg, engine=OracleFilterEngine())
    assert [f for f in os.listdir(trial / 'pose-3d') if 'filt' in f] == []


def test_pose2sim_filtering_runs_a_gcv_spline_config(work_dir, gold, monkeypatch):
    """Pose2Sim.filtering() on a trial whose Config.toml says type = 'gcv_spline' writes the reference's file."""
    from pose2sim_amd import Pose2Sim, filtering
    trial, _ = _trial(work_dir, gold, 0)
    (trial / 'Config.toml').write_text('[project]\nframe_rate = 60\nframe_range = []\n\n[pose]\nvid_img_extension = "mp4"\n\n'
                                       '[logging]\nuse_custom_logging = true\n\n'
                                       '[filtering]\ntype = "gcv_spline"\nfilter = true\nreject_outliers = false\nmake_c3d = false\n'
                                       '[filtering.gcv_spline]\ncut_off_frequency = "auto"\nsmoothing_factor = 1.0\n')
    monkeypatch.setattr(filtering, '_make_engine', lambda: ScipyGcvEngine())
    monkeypatch.chdir(trial)
    Pose2Sim.filtering()
    out = trial / 'pose-3d' / str(gold['file0_out_name'])
    assert out.read_text() == _text(gold, 'file0_out_text')
