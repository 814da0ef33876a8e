"""The synchronization stage on CPU: the NumPy restatement of the engine entries (tests/sync_numpy.py) against the
reference's goldens (tests/golden/sync_units.npz <- make_golden_sync.py), and the stage with that restatement as its
Engine: offsets, pose-sync/ tree, log lines and exceptions of every recorded case.  Also the native host pieces that
need no GPU: the person choice of the JSON gather and the file copy."""
import json
import logging
import os
import shutil
import stat
import tempfile

import numpy as np
import pytest

import sync_trials as st
from sync_numpy import NumpySyncEngine, lagged_pearson


@pytest.fixture(scope='module')
def gold(golden_dir):
    return np.load(os.path.join(golden_dir, 'sync_units.npz'))


def trial_of(gold, name):
    return {k: gold[f'trial{name}_{k}'] for k in ('xy', 'lik', 'n_frames', 'n_persons', 'kind', 'trunc')}


def cases(gold, errors=False):
    return [n for n in range(int(gold['n_cases'])) if (f'case{n}_error' in gold) == errors]


@pytest.fixture
def work_dir():
    d = os.path.realpath(tempfile.mkdtemp(prefix='p2s_sync_'))
    yield d
    shutil.rmtree(d, ignore_errors=True)


class _Lines(logging.Handler):
    def __init__(self):
        super().__init__()
        self.lines = []

    def emit(self, record):
        self.lines.append(record.getMessage())


class RecordingEngine(NumpySyncEngine):
    """The NumPy restatement, keeping what the stage asked for."""

    def sync_speeds(self, coords, b, a, zi):
        self.speeds = super().sync_speeds(coords, b, a, zi)
        return self.speeds

    def lagged_pearson(self, ref, signals, lag_lo, lag_hi):
        self.pearson = super().lagged_pearson(ref, signals, lag_lo, lag_hi)
        return self.pearson


def run_case(gold, n, work_dir, engine):
    """Write case n's trial, run the stage -> (error or None, log lines with the trial's directory as <TMP>, trial dir)."""
    from pose2sim_amd import synchronization
    trial_dir = os.path.join(work_dir, 'trial')
    st.write_trial(trial_of(gold, str(gold[f'case{n}_trial'])), os.path.join(trial_dir, 'pose'))
    cfg = st.sync_config(trial_dir, **json.loads(str(gold[f'case{n}_config'])))
    root = logging.getLogger()
    level = root.level
    root.setLevel(logging.INFO)
    h = _Lines()
    root.addHandler(h)
    err = None
    try:
        synchronization.synchronize_cams_all(cfg, engine=engine)
    except Exception as e:                                                   # noqa: BLE001
        err = e
    finally:
        root.removeHandler(h)
        root.setLevel(level)
    return err, [line.replace(work_dir, '<TMP>') for line in h.lines], trial_dir


def check_against_gold(gold, n, engine, lines, trial_dir):
    """Speeds, r curves, offsets, log lines and the pose-sync/ tree of case n."""
    name = str(gold[f'case{n}_name'])
    assert lines == json.loads(str(gold[f'case{n}_logs'])), name
    r, _, _ = engine.pearson
    calls = int(gold[f'case{n}_n_calls'])
    assert r.shape[0] == calls
    ref = gold[f'case{n}_speed_ref']
    scale = max(1.0, float(np.nanmax(np.abs(ref))))
    assert any(len(s) == len(ref) and np.allclose(s, ref, rtol=0, atol=1e-9 * scale) for s in engine.speeds), name
    for k in range(calls):
        want = gold[f'case{n}_speed{k}']
        assert any(len(s) == len(want) and np.allclose(s, want, rtol=0, atol=1e-9 * max(1.0, float(np.nanmax(np.abs(want)))))
                   for s in engine.speeds), (name, k)
        assert np.array_equal(np.isnan(r[k]), np.isnan(gold[f'case{n}_r{k}'])), (name, k)
        assert np.allclose(r[k], gold[f'case{n}_r{k}'], rtol=0, atol=1e-9, equal_nan=True), (name, k)
    listing = json.loads(str(gold[f'case{n}_listing']))
    sync_dir = os.path.join(trial_dir, 'pose-sync')
    assert sorted(d for d in os.listdir(sync_dir) if os.path.isdir(os.path.join(sync_dir, d))) == sorted(listing)
    for d, files in listing.items():
        assert sorted(os.listdir(os.path.join(sync_dir, d))) == files, (name, d)


def test_numpy_pearson_is_the_reference_on_the_golden_speeds(gold):
    """The restatement of time_lagged_cross_corr on the reference's own speed series: r within 1e-9, same argmax."""
    for n in cases(gold):
        ref = gold[f'case{n}_speed_ref']
        half = int(len(ref) / 2)
        for k in range(int(gold[f'case{n}_n_calls'])):
            r, arg, mx = lagged_pearson(ref, [gold[f'case{n}_speed{k}']], -half, half)
            want = gold[f'case{n}_r{k}']
            assert np.allclose(r[0], want, rtol=0, atol=1e-9, equal_nan=True)
            assert arg[0] == np.argmax(want)
            section, _ = gold[f'case{n}_section{k}']
            if not np.isnan(want).all():
                assert half - arg[0] == section


@pytest.mark.parametrize('n', range(11))
def test_stage_reproduces_the_reference(gold, work_dir, n):
    """synchronize_cams_all with the NumPy engine: the reference's speeds, r curves, log lines and pose-sync/ listing."""
    assert n in cases(gold)
    engine = RecordingEngine()
    err, lines, trial_dir = run_case(gold, n, work_dir, engine)
    assert err is None, err
    check_against_gold(gold, n, engine, lines, trial_dir)


def test_stage_copies_are_byte_identical_with_the_source_mode(gold, work_dir):
    """pose-sync/ files are the sources' bytes under their renumbered names, with shutil.copy's permission bits."""
    n = 0
    trial_dir = os.path.join(work_dir, 'trial')
    st.write_trial(trial_of(gold, str(gold[f'case{n}_trial'])), os.path.join(trial_dir, 'pose'))
    src = os.path.join(trial_dir, 'pose', 'cam02_json', 'cam02_000010.json')
    os.chmod(src, 0o640)
    from pose2sim_amd import synchronization
    offsets = synchronization.synchronize_cams_all(st.sync_config(trial_dir), engine=NumpySyncEngine())
    assert offsets == [0, -7, 12, -25]
    dst = os.path.join(trial_dir, 'pose-sync', 'cam02_json', f'cam02_{10 + 7:06d}.json')
    assert open(dst, 'rb').read() == open(src, 'rb').read()
    assert stat.S_IMODE(os.stat(dst).st_mode) == 0o640
    # offset 0: frame 0 is not copied (its new number is not > 0); cam04 (offset -25) starts at 25
    assert 'cam01_000000.json' not in os.listdir(os.path.join(trial_dir, 'pose-sync', 'cam01_json'))
    assert min(os.listdir(os.path.join(trial_dir, 'pose-sync', 'cam04_json'))) == 'cam04_000025.json'


@pytest.mark.parametrize('k', range(5))
def test_stage_raises_what_the_reference_raised(gold, work_dir, k):
    errs = cases(gold, errors=True)
    assert len(errs) == 5
    n = errs[k]
    err, lines, _ = run_case(gold, n, work_dir, NumpySyncEngine())
    want_type, want_msg = (str(v) for v in gold[f'case{n}_error'])
    assert err is not None and type(err).__name__ == want_type, (gold[f'case{n}_name'], err)
    if want_type == 'UnboundLocalError':
        assert 'search_around_frames' in str(err)                  # the wording is the interpreter's
    else:
        assert str(err) == want_msg
        assert lines == json.loads(str(gold[f'case{n}_logs']))


def test_gui_mode_is_refused(work_dir):
    from pose2sim_amd import synchronization
    with pytest.raises(NotImplementedError, match='synchronization_gui'):
        synchronization.synchronize_cams_all(st.sync_config(work_dir, synchronization_gui=True), engine=NumpySyncEngine())


def test_pose2sim_entry_runs_the_stage(gold, work_dir, monkeypatch):
    """Pose2Sim.synchronization() (no longer a stub) writes pose-sync/ with the reference's listing."""
    from pose2sim_amd import Pose2Sim, synchronization
    monkeypatch.setattr(synchronization, '_make_engine', NumpySyncEngine)
    n = 0
    trial_dir = os.path.join(work_dir, 'trial')
    st.write_trial(trial_of(gold, 'A'), os.path.join(trial_dir, 'pose'))
    cfg = st.sync_config(trial_dir)
    cfg['logging'] = {'use_custom_logging': True}
    Pose2Sim.synchronization(cfg)
    listing = json.loads(str(gold[f'case{n}_listing']))
    for d, files in listing.items():
        assert sorted(os.listdir(os.path.join(trial_dir, 'pose-sync', d))) == files


def reference_person_choice(path, ids, thr):
    """convert_json2pandas's try block (synchronization.py:1203-1240, synchronization_gui false), restated with its
    comprehension as written: the keypoints of every person are indexed before the `in p` test."""
    try:
        people = json.load(open(path))['people']
        areas = [(kp[:, 0].max() - kp[:, 0].min()) * (kp[:, 1].max() - kp[:, 1].min()) if 'pose_keypoints_2d' in p else 0
                 for p in people
                 for kp in [np.array([p['pose_keypoints_2d'][3 * i:3 * i + 3] for i in ids])]]
        chosen = people[np.argmax(areas)]
        data = np.array([chosen['pose_keypoints_2d'][3 * i:3 * i + 3] for i in ids])
        return np.array([j if j[2] > thr else [np.nan] * 3 for j in data], dtype=np.float64)
    except Exception:                                                                   # noqa: BLE001
        return np.full((len(ids), 3), np.nan)


def test_gather_chooses_the_reference_person(gold, work_dir):
    """p2s_json_gather_largest_person on the multi-person trial (distractors, persons without a list, empty files,
    truncated lists, files without "people"), against the reference's rule."""
    from pose2sim_amd import skeletons
    from pose2sim_amd.ingest import JsonBatch
    ids, _, _ = skeletons.keypoints('HALPE_26')
    trial = trial_of(gold, 'B')
    dirs = st.write_trial(trial, work_dir)
    paths = [os.path.join(work_dir, d, f) for d in dirs for f in sorted(os.listdir(os.path.join(work_dir, d)))]
    with JsonBatch(paths) as batch:
        got = batch.gather_largest_person(ids, 0.4)
    kinds = set(int(k) for k in trial['kind'].ravel())
    assert kinds == {0, 1, 2, 3, 4}
    for i, p in enumerate(paths):
        assert np.array_equal(got[i], reference_person_choice(p, ids, 0.4), equal_nan=True), p
    assert np.isnan(got).all(axis=(1, 2)).sum() > 0


def test_gather_tie_and_nan_rules(work_dir):
    """np.argmax's rules for the chosen person: the first of equal areas, the first NaN area."""
    from pose2sim_amd.ingest import JsonBatch
    a = [10, 10, 0.9, 20, 30, 0.9]                           # area 100
    b = [110, 10, 0.8, 120, 20, 0.8]                         # area 100 (tie: the first wins)
    c = [float('nan'), 0, 0.7, 5, 5, 0.7]                    # NaN area
    docs = {'tie.json': [a, b], 'nan_second.json': [a, c, b], 'nan_first.json': [c, a]}
    paths = []
    for name, people in docs.items():
        with open(os.path.join(work_dir, name), 'w') as fh:
            json.dump({'people': [{'pose_keypoints_2d': p} for p in people]}, fh)
        paths.append(os.path.join(work_dir, name))
    with JsonBatch(paths) as batch:
        got = batch.gather_largest_person([0, 1], 0.5)
    for i, p in enumerate(paths):
        assert np.array_equal(got[i], reference_person_choice(p, [0, 1], 0.5), equal_nan=True), p
    assert got[0][0][0] == 10 and np.isnan(got[1][0][0]) and np.isnan(got[2][0][0])


def test_copy_files_keeps_bytes_and_mode(work_dir):
    from pose2sim_amd.ingest import copy_files
    pairs = []
    for i, mode in enumerate((0o600, 0o644, 0o755)):
        src = os.path.join(work_dir, f's{i}.json')
        with open(src, 'wb') as fh:
            fh.write(bytes(range(256)) * (i * 300 + 1))
        os.chmod(src, mode)
        pairs.append((src, os.path.join(work_dir, f'd{i}.json')))
    with open(pairs[0][1], 'w') as fh:
        fh.write('an older, longer file that the copy must truncate' * 100)
    copy_files(pairs)
    for (src, dst), mode in zip(pairs, (0o600, 0o644, 0o755)):
        assert open(dst, 'rb').read() == open(src, 'rb').read()
        assert stat.S_IMODE(os.stat(dst).st_mode) == mode
    with pytest.raises(OSError, match='missing'):
        copy_files([(os.path.join(work_dir, 'missing.json'), os.path.join(work_dir, 'x.json'))])
