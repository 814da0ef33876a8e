"""The jitter utility without a GPU: the NumPy restatement (tests/jitter_numpy.py) against the goldens recorded from the
reference (tests/golden/jitter_units.npz) bit for bit, pose2sim_amd.keypoint_jitter_analyze on that restatement against
the recorded files, printed text and errors byte for byte, the native person selection (host code) against the recorded
series and against a NumPy statement of the rule on random people, the command line and the refusals.  Nothing here has
a tolerance."""
import json
import os

import numpy as np
import pytest

import jitter_numpy as jn
from pose2sim_amd import _lib
from pose2sim_amd import keypoint_jitter_analyze as kj


@pytest.fixture(scope='module')
def gold(golden_dir):
    return np.load(os.path.join(golden_dir, 'jitter_units.npz'))


ALL = json.loads(str(np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'jitter_units.npz'))['cases']))
ERROR_CASES = [n for n in ALL if n.startswith('error_')]
assert len(ALL) == 12 and len(ERROR_CASES) == 3


def same(a, b):
    """Equal bit for bit up to the payload of a NaN: values, NaN pattern, and the sign of everything that is not NaN."""
    a, b = np.asarray(a), np.asarray(b)
    if a.shape != b.shape or not np.array_equal(a, b, equal_nan=a.dtype.kind == 'f'):
        return False
    if a.dtype.kind != 'f':
        return True
    ok = ~np.isnan(a)
    return np.array_equal(np.signbit(a[ok]), np.signbit(b[ok]))


def lay_out(gold, name, work):
    """Write the case's inputs into `work` -> (pose_dir, keyword arguments)."""
    for d in json.loads(str(gold[f'{name}__folders'])):
        os.makedirs(os.path.join(work, d), exist_ok=True)
    for rel, text in json.loads(str(gold[f'{name}__files'])).items():
        os.makedirs(os.path.dirname(os.path.join(work, rel)), exist_ok=True)
        with open(os.path.join(work, rel), 'w') as fh:
            fh.write(text)
    args = json.loads(str(gold[f'{name}__args']))
    if 'output' in args:
        args['output'] = os.path.join(work, args['output'])
    if 'image_size' in args:
        args['image_size'] = tuple(args['image_size'])
    return os.path.join(work, str(gold[f'{name}__pose_dir'])), args


def recorded_series(gold, name):
    return [gold[f'{name}__{c}__series'] for c in range(int(gold[f'{name}__n_cams']))]


def check_engine_on_case(gold, name, engine, report=print):
    """engine.jitter on the recorded series of every camera of the case, each table against the recording."""
    series = recorded_series(gold, name)
    if not series:
        return
    args = json.loads(str(gold[f'{name}__args']))
    res = engine.jitter(series, args.get('multiplier', 5.0), tuple(args.get('image_size', (1920, 1080))))
    events = json.loads(str(gold[f'{name}__events']))
    want = [[c, e['frame'], e['keypoint_idx'], 'ACDE'.index(e['pattern'])] for c, evs in enumerate(events) for e in evs]
    report(f'{name}: {len(series)} cameras, {len(want)} events, per pattern {jn.pattern_counts(res["events"])}')
    for c in range(len(series)):
        for key, mine in (('displacements', 'displacements'), ('areas', 'bb_areas'), ('medians', 'medians'), ('thresholds', 'thresholds'),
                          ('mask', 'jitter_mask'), ('median_area', 'median_bb_area')):
            assert same(gold[f'{name}__{c}__{key}'], res[mine][c]), (name, c, key)
        assert np.array_equal(res['counts'][c], gold[f'{name}__{c}__mask'].sum(axis=0)), (name, c, 'counts')
    assert np.array_equal(res['events'], np.array(want, dtype=np.int32).reshape(-1, 4)), (name, 'events')


def run_case(gold, name, work, engine, capsys):
    """The utility on `engine` in `work` (the working directory, as in the recording): files written, their text, what was
    printed and the error, against the recording, the recording's folder replaced by `work`."""
    pose_dir, args = lay_out(gold, name, work)
    root = str(gold['work_root']) + '/' + name
    error = json.loads(str(gold[f'{name}__error']))
    before = {os.path.join(r, f) for r, _, fs in os.walk(work) for f in fs}
    cwd = os.getcwd()
    os.chdir(work)
    capsys.readouterr()
    try:
        if error is None:
            result = kj.analyze_jitter(pose_dir, engine=engine, **args)
        else:
            kind = {'ValueError': ValueError, 'FileNotFoundError': FileNotFoundError}[error[0]]
            with pytest.raises(kind) as caught:
                kj.analyze_jitter(pose_dir, engine=engine, **args)
            assert str(caught.value) == error[1].replace(root, work)
            result = None
    finally:
        os.chdir(cwd)
    assert capsys.readouterr().out == str(gold[f'{name}__printed']).replace(root, work)
    written = {}
    for r, _, fs in os.walk(work):
        for f in fs:
            p = os.path.join(r, f)
            if p not in before:
                with open(p, encoding='utf-8', newline='') as fh:
                    written[os.path.relpath(p, work)] = fh.read()
    want = {rel: text.replace(root, work) for rel, text in json.loads(str(gold[f'{name}__written'])).items()}
    assert sorted(written) == sorted(want)
    for rel in want:
        assert written[rel] == want[rel], rel
    return result


@pytest.mark.parametrize('name', ALL)
def test_numpy_restatement_reproduces_the_reference(gold, name, capsys):
    with capsys.disabled():
        check_engine_on_case(gold, name, jn.NumpyJitterEngine())


@pytest.mark.parametrize('name', ALL)
def test_utility_writes_the_recorded_files(gold, tmp_path, name, capsys):
    result = run_case(gold, name, str(tmp_path), jn.NumpyJitterEngine(), capsys)
    if result is not None:                                           # the returned dictionary: the reference's internal one
        events = json.loads(str(gold[f'{name}__events']))
        assert len(result) == len(events)
        for c, cam in enumerate(result.values()):                    # insertion order = folder order
            assert same(cam['keypoints_series'], gold[f'{name}__{c}__series'])
            assert cam['n_frames'] == len(gold[f'{name}__{c}__series'])
            assert json.dumps(cam['events']) == json.dumps(events[c])      # repr floats: exact, NaN included
            for key in ('displacements', 'thresholds', 'medians'):
                assert same(cam[key], gold[f'{name}__{c}__{key}'])
            assert same(cam['jitter_mask'], gold[f'{name}__{c}__mask'])


def test_fixture_covers_what_it_claims(gold):
    tally = dict.fromkeys('ACDE', 0)
    for name in ALL:
        for evs in json.loads(str(gold[f'{name}__events'])):
            for e in evs:
                tally[e['pattern']] += 1
    assert min(tally.values()) >= 20, tally
    sp = 'special'
    assert gold[f'{sp}__0__medians'][3] == 0.0 and gold[f'{sp}__0__thresholds'][3] == 10.0        # a median of exactly 0
    assert gold[f'{sp}__0__mask'][[19, 20, 32, 33], 3].all()         # 25 px there and back, twice
    assert not gold[f'{sp}__0__mask'][[43, 44], 3].any()             # the 6 px jump stays below 10
    at_border = {e['frame'] for e in json.loads(str(gold[f'{sp}__events']))[0] if e['pattern'] == 'A'}
    assert {14, 17, 22, 25} <= at_border                             # left, right, top, bottom
    assert np.isnan(gold[f'{sp}__0__medians'][7]) and np.isnan(gold[f'{sp}__0__displacements'][:, 7]).all()
    assert np.isnan(gold[f'{sp}__0__series'][[3, 8]]).all()          # a short list alone, no valid keypoint: no candidate
    assert not np.isnan(gold[f'{sp}__0__series'][[2, 4, 5]]).all(axis=(1, 2)).any()
    assert np.isnan(gold[f'{sp}__0__areas'][[5, 6, 10, 11, 12]]).all()
    assert np.isnan(gold[f'{sp}__0__series'][10, 2, 2])
    assert gold['one_frame__0__displacements'].shape == (0, 26) and np.isnan(gold['one_frame__0__medians']).all()
    lengths = {len(gold[f'four_cameras_lengths__{c}__series']) for c in range(4)}
    assert len(lengths) == 4


@pytest.mark.parametrize('name', ALL)
def test_native_selection_reproduces_the_recorded_series(gold, tmp_path, name):
    """p2s_json_select_tracked_person on every camera folder of every case, against the series the reference selected."""
    pose_dir, _ = lay_out(gold, name, str(tmp_path))
    series = recorded_series(gold, name)
    try:
        dirs = kj.find_camera_dirs(pose_dir)
    except FileNotFoundError:
        assert name == 'error_no_folders'
        return
    for c, d in enumerate(dirs):
        if c < len(series):
            assert same(kj.load_keypoints_series(d), series[c]), (name, c)
        else:                                                        # the camera the reference stopped at
            with pytest.raises((ValueError, FileNotFoundError)):
                kj.load_keypoints_series(d)
            break


def numpy_choice(people, prev):
    """The selection rule on people [P][26][3] (all candidates), in plain NumPy with np.mean -> index."""
    if prev is not None:
        best, best_d = None, np.inf
        pv = (prev[:, 2] > 0.1) & ~np.isnan(prev[:, 0])
        for i, kp in enumerate(people):
            both = pv & (kp[:, 2] > 0.1) & ~np.isnan(kp[:, 0])
            if both.any():
                d = np.mean(np.sqrt(((kp[both, :2] - prev[both, :2]) ** 2).sum(axis=1)))
                if d < best_d:
                    best, best_d = i, d
        if best is not None:
            return best
    return int(np.argmax([(kp[:, 2] > 0.1).sum() for kp in people]))


def test_native_selection_sums_in_numpy_order(tmp_path):
    """Near-ties: every frame holds two persons at almost the same mean distance from the previous choice (one is the other
    with its keypoints permuted, so the sums differ by rounding alone, or not at all).  The native choice must be np.mean's."""
    from pose2sim_amd.ingest import JsonBatch
    rng = np.random.default_rng(3)
    prev, files, want = None, [], []
    for f in range(400):
        a = np.concatenate([rng.uniform(100, 900, (26, 2)), rng.uniform(0.05, 1.0, (26, 1))], axis=1)
        a[rng.random(26) < 0.1, 0] = np.nan
        people = [a]
        if f:
            off = a[:, :2] - prev[:, :2]
            perm = rng.permutation(26)
            b = a.copy()
            b[:, :2] = prev[:, :2] + off[perm] * (1 + (f % 3 == 0) * 1e-15)
            b[:, 2] = np.where(a[perm, 2] > 0.1, 0.9, 0.05)
            people = [a, b] if f % 2 else [b, a]
        i = numpy_choice(people, prev)
        want.append(people[i])
        prev = people[i]
        path = os.path.join(str(tmp_path), f'{f:04d}.json')
        with open(path, 'w') as fh:
            json.dump({'people': [{'pose_keypoints_2d': [float(v) for v in p.ravel()]} for p in people]}, fh)
        files.append(path)
    with JsonBatch(files) as batch:
        series, status, detail = batch.select_tracked_person(26, 0.1)
    assert (status == _lib.P2S_TRACK_SELECTED).all()
    assert same(series, np.array(want))


def write(path, text):
    with open(path, 'w') as fh:
        fh.write(text)
    return path


GOOD = json.dumps({'people': [{'pose_keypoints_2d': [100.0 + k for k in range(78)]}]})


def test_selection_statuses(tmp_path):
    from pose2sim_amd.ingest import JsonBatch
    t = str(tmp_path)
    many = json.dumps({'people': [{'pose_keypoints_2d': [1.0] * 78}, {'pose_keypoints_2d': [2.0] * 81}]})
    docs = [GOOD, '{"version": 1.3}', '{"people": []}', '{"people": null}', json.dumps({'people': [{'pose_keypoints_2d': [0.0] * 78}]}),
            many, 'not json', '[1, 2]', '{"people": 5}', '{"people": [7]}', json.dumps({'people': [{'pose_keypoints_2d': [1.0] * 77 + [None]}]}),
            json.dumps({'people': [{'pose_keypoints_2d': ['a'] * 78}]}), json.dumps({'people': [{'pose_keypoints_2d': 3}]}),
            json.dumps({'people': [{'pose_keypoints_2d': [1.0, True] * 39}]})]
    files = [write(os.path.join(t, f'{i:02d}.json'), d) for i, d in enumerate(docs)] + [os.path.join(t, 'missing.json')]
    with JsonBatch(files) as batch:
        series, status, detail = batch.select_tracked_person(26, 0.1)
    L = _lib
    assert list(status) == [L.P2S_TRACK_SELECTED, L.P2S_TRACK_NO_PEOPLE, L.P2S_TRACK_NO_PEOPLE, L.P2S_TRACK_NO_PEOPLE, L.P2S_TRACK_NO_CANDIDATE,
                            L.P2S_TRACK_LONG_LIST, L.P2S_TRACK_BAD_FILE, L.P2S_TRACK_BAD_CONTENT, L.P2S_TRACK_BAD_CONTENT, L.P2S_TRACK_BAD_CONTENT,
                            L.P2S_TRACK_BAD_CONTENT, L.P2S_TRACK_BAD_CONTENT, L.P2S_TRACK_BAD_CONTENT, L.P2S_TRACK_SELECTED, L.P2S_TRACK_BAD_FILE]
    assert detail[5] == 81
    assert np.array_equal(series[0].ravel(), 100.0 + np.arange(78)) and np.isnan(series[1:13]).all()
    assert np.array_equal(series[13].ravel(), [1.0, 1.0] * 39)       # true reads as 1.0, as np.array makes it


@pytest.mark.parametrize('text', ['not json', '[1, 2]', '{"people": [7]}',
                                  json.dumps({'people': [{'pose_keypoints_2d': [1.0] * 77 + [None]}]}),
                                  json.dumps({'people': [{'pose_keypoints_2d': ['a'] * 78}]})])
def test_inputs_outside_the_contract_raise_and_write_nothing(tmp_path, text):
    cam = os.path.join(str(tmp_path), 'pose', 'cam01_json')
    os.makedirs(cam)
    write(os.path.join(cam, '000.json'), GOOD)
    bad = write(os.path.join(cam, '001.json'), text)
    out = os.path.join(str(tmp_path), 'out')
    with pytest.raises(ValueError, match='001.json') as caught:
        kj.analyze_jitter(os.path.join(str(tmp_path), 'pose'), output=out, engine=jn.NumpyJitterEngine())
    assert bad in str(caught.value)
    assert not os.path.exists(out)


def test_main_parses_the_reference_options(monkeypatch):
    seen = {}
    monkeypatch.setattr(kj, 'analyze_jitter', lambda **a: seen.update(a))
    monkeypatch.setattr('sys.argv', ['keypoint_jitter_analyze', '-p', 'some/pose', '-o', 'where', '--multiplier', '3.5', '--no-plot',
                                     '--image-width', '1280', '--image-height', '720'])
    kj.main()
    assert seen == {'pose_dir': 'some/pose', 'output': 'where', 'multiplier': 3.5, 'no_plot': True, 'image_size': (1280, 720)}
    seen.clear()
    monkeypatch.setattr('sys.argv', ['keypoint_jitter_analyze', '--pose-dir', 'p'])
    kj.main()
    assert seen == {'pose_dir': 'p', 'output': None, 'multiplier': 5.0, 'no_plot': False, 'image_size': (1920, 1080)}
    monkeypatch.setattr('sys.argv', ['keypoint_jitter_analyze'])
    with pytest.raises(SystemExit):
        kj.main()


def test_defaults_are_the_references():
    import inspect
    sig = inspect.signature(kj.analyze_jitter)
    assert [(n, p.default) for n, p in sig.parameters.items()][:5] == [
        ('pose_dir', inspect.Parameter.empty), ('output', None), ('multiplier', 5.0), ('no_plot', False), ('image_size', (1920, 1080))]
    assert len(kj.KEYPOINT_NAMES) == 26 and kj.KEYPOINT_NAMES[0] == 'Nose' and kj.KEYPOINT_NAMES[-1] == 'RHeel'


def test_engine_without_the_entries_refuses():
    """An Engine whose library lacks the new entry points raises NotImplementedError, as reproject does."""
    from pose2sim_amd.engine import Engine
    from pose2sim_amd.ingest import JsonBatch

    class Old:
        pass
    eng = Engine.__new__(Engine)
    eng._lib, eng._h = Old(), None
    with pytest.raises(NotImplementedError):
        eng.jitter([np.zeros((2, 26, 3))])
    with pytest.raises(NotImplementedError):
        eng.column_order_stats(np.zeros((2, 2)), [0])
    with pytest.raises(NotImplementedError):
        eng.jitter_kernel_ms()
    batch = JsonBatch.__new__(JsonBatch)
    batch._lib, batch._h, batch.n_files = Old(), None, 0
    with pytest.raises(NotImplementedError):
        batch.select_tracked_person()


def test_new_entries_are_optional_for_an_older_library():
    assert {'p2s_column_order_stats_host', 'p2s_jitter_host', 'p2s_jitter_kernel_ms', 'p2s_json_select_tracked_person'} <= _lib.OPTIONAL


def test_no_gpu_means_the_utility_raises(gold, tmp_path):
    """There is no CPU fallback: with the default engine and no GPU the utility raises before it writes."""
    if _lib.device_count() > 0:
        return                                                       # covered by tests/test_jitter_gpu.py
    pose_dir, args = lay_out(gold, 'two_frames', str(tmp_path))
    with pytest.raises(_lib.P2sError):
        kj.analyze_jitter(pose_dir, **args)
    assert not os.path.exists(args['output'])
