"""The confidence utility without a GPU: the NumPy stand-in (tests/confidence_numpy.py) against the goldens recorded from the
reference (tests/golden/confidence_units.npz) bit for bit, pose2sim_amd.pose_confidence_analyze on that stand-in against
the recorded files, printed text and errors byte for byte, the native loading (host code) against the recorded tables,
the command line and the refusals.  Nothing here has a tolerance."""
import json
import os

import numpy as np
import pytest

import confidence_numpy as cn
from pose2sim_amd import _lib
from pose2sim_amd import pose_confidence_analyze as pc
from test_jitter_host import same

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'confidence_units.npz')
ALL = json.loads(str(np.load(GOLDEN)['cases']))
ERROR_CASES = [n for n in ALL if n.startswith('error_')]
assert len(ALL) == 9 and len(ERROR_CASES) == 4
ERRORS = {'IndexError': IndexError, 'KeyError': KeyError, 'FileNotFoundError': FileNotFoundError}


@pytest.fixture(scope='module')
def gold():
    return np.load(GOLDEN)


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
    return os.path.join(work, str(gold[f'{name}__pose_dir'])), args


def recorded_tables(gold, name):
    return [gold[f'{name}__{c}__table'] for c in range(len(json.loads(str(gold[f'{name}__cameras']))))]


def check_engine_on_case(gold, name, engine, report=print):
    """engine.confidence_stats on the recorded tables of the case, every table against the recording."""
    tables = recorded_tables(gold, name)
    if not tables:
        return
    threshold = json.loads(str(gold[f'{name}__args'])).get('threshold', 0.4)
    ths = [float(t) for t in gold[f'{name}__sim_thresholds']]
    res = engine.confidence_stats(tables, ths)
    want = gold[f'{name}__stats']
    report(f'{name}: {len(tables)} cameras, thresholds {ths}, {int(res["counts"].sum())} entries, {int((res["counts"] == 0).sum())} empty columns')
    assert same(res['stats'], want[:, :, :9]), (name, 'stats')
    assert same(res['below_rate'][ths.index(threshold)], want[:, :, 9]), (name, 'below_threshold_rate')
    assert np.array_equal(res['counts'], np.array([(~np.isnan(t)).sum(axis=0) for t in tables])), (name, 'counts')
    assert res['bands'].dtype == np.int64 and np.array_equal(res['bands'], gold[f'{name}__band_counts']), (name, 'bands')
    assert same(res['band_rate'], gold[f'{name}__band_rates']), (name, 'band rates')
    sim = np.where(res['counts'][None] == 0, 0.0, res['below_rate'])
    assert same(sim, gold[f'{name}__sim']), (name, 'threshold simulation')


def run_case(gold, name, work, engine, capsys):
    """The utility on `engine` in `work`: files written, their text, what was printed, the error and the returned
    dictionary, against the recording, the recording's folder replaced by `work`."""
    pose_dir, args = lay_out(gold, name, work)
    root = str(gold['work_root']) + '/' + name
    error = json.loads(str(gold[f'{name}__error']))
    before = {os.path.join(r, f) for r, _, fs in os.walk(work) for f in fs}
    capsys.readouterr()
    if error is None:
        result = pc.analyze_confidence(pose_dir, engine=engine, **args)
    else:
        with pytest.raises(ERRORS[error[0]]) as caught:
            pc.analyze_confidence(pose_dir, engine=engine, **args)
        assert type(caught.value) is ERRORS[error[0]] and str(caught.value) == error[1].replace(root, work)
        result = None
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
    if result is not None:
        check_result(gold, name, result)
    return result


def check_result(gold, name, result):
    """The returned dictionary: the reference's keys, Python floats and ints, the recorded bits."""
    cams = json.loads(str(gold[f'{name}__cameras']))
    assert list(result) == ['statistics', 'band_distribution', 'threshold_simulation']
    st, bd, sim = result['statistics'], result['band_distribution'], result['threshold_simulation']
    assert list(st) == cams and list(bd) == cams
    stat_names = cn.STATS + ('below_threshold_rate',)
    for c, cam in enumerate(cams):
        assert list(st[cam]) == list(range(26)) and list(bd[cam]) == list(range(26))
        for k in range(26):
            assert list(st[cam][k]) == list(stat_names) and all(type(v) is float for v in st[cam][k].values())
            assert same([st[cam][k][s] for s in stat_names], gold[f'{name}__stats'][c, k]), (cam, k)
            assert list(bd[cam][k]) == ['low', 'danger', 'medium', 'high', 'very_high']
            assert all(type(b['count']) is int and type(b['rate']) is float for b in bd[cam][k].values())
            assert [b['count'] for b in bd[cam][k].values()] == list(gold[f'{name}__band_counts'][c, k])
            assert same([b['rate'] for b in bd[cam][k].values()], gold[f'{name}__band_rates'][c, k])
    assert list(sim) == list(gold[f'{name}__sim_thresholds'])
    for t, th in enumerate(sim):
        assert list(sim[th]) == cams
        for c, cam in enumerate(cams):
            assert all(type(v) is float for v in sim[th][cam].values())
            assert same([sim[th][cam][k] for k in range(26)], gold[f'{name}__sim'][t, c])


@pytest.mark.parametrize('name', ALL)
def test_numpy_stand_in_reproduces_the_reference(gold, name, capsys):
    with capsys.disabled():
        check_engine_on_case(gold, name, cn.NumpyConfidenceEngine())


@pytest.mark.parametrize('name', ALL)
def test_utility_writes_the_recorded_files(gold, tmp_path, name, capsys):
    run_case(gold, name, str(tmp_path), cn.NumpyConfidenceEngine(), capsys)


@pytest.mark.parametrize('name', ALL)
def test_native_loading_reproduces_the_recorded_tables(gold, tmp_path, name):
    pose_dir, _ = lay_out(gold, name, str(tmp_path))
    tables = recorded_tables(gold, name)
    if not tables:
        with pytest.raises(tuple(ERRORS.values())):
            pc.load_pose_data(pose_dir)
        return
    loaded = pc.load_pose_data(pose_dir)
    assert list(loaded) == json.loads(str(gold[f'{name}__cameras']))
    for table, want in zip(loaded.values(), tables):
        assert same(table, want)


def test_fixture_covers_what_it_claims(gold):
    sp = gold['special_values__0__table']
    assert [int((~np.isnan(sp[:, k])).sum()) for k in range(8)] == [1, 2, 7, 8, 9, 127, 128, 129]
    assert np.isnan(sp[:, 12]).all() and not np.isnan(sp[:, 11]).all(axis=0) and np.isnan(sp[[50, 51]]).all()
    assert {0.4, 0.6, 0.8, 1.0} <= set(sp[:, 8]) and (sp[:, 9] > 1).any() and (sp[:, 10] < 0).any() and (sp[:, 10] == 0).any()
    bands = gold['special_values__band_counts'][0]
    assert bands[8, 4] == (sp[:, 8] == 1.0).sum() > 0 and bands[8, 3] == ((sp[:, 8] >= 0.8) & (sp[:, 8] <= 1.0)).sum()
    assert bands[10].sum() == (sp[:, 10] >= 0).sum() < (~np.isnan(sp[:, 10])).sum()
    assert np.isnan(gold['special_values__stats'][0, 12]).all() and (gold['special_values__band_rates'][0, 12] == 0).all()
    assert gold['special_values__sim_thresholds'][0] == 0.3 and list(gold['four_cameras__sim_thresholds']) == [0.4, 0.45, 0.5, 0.6]
    assert json.loads(str(gold['four_cameras__cameras'])) == ['cam01', 'cam02_v2', 'cam03', 'cam04']
    assert len({len(gold[f'four_cameras__{c}__table']) for c in range(4)}) == 4
    assert np.isnan(gold['four_cameras__2__table']).all() and np.isnan(gold['four_cameras__stats'][2]).all()
    assert (gold['four_cameras__sim'][:, 2] == 0).all() and 'nan' in str(gold['four_cameras__printed'])
    first = json.loads(json.loads(str(gold['three_cameras_lengths__files']))['pose/cam01_json/frame_0000.json'])['people']
    assert len(first) == 2 and first[1]['pose_keypoints_2d'][0] > first[0]['pose_keypoints_2d'][0]
    assert same(gold['three_cameras_lengths__0__table'][0], first[0]['pose_keypoints_2d'][2::3])
    long_list = json.loads(json.loads(str(gold['long_lists_threshold_07__files']))['pose/cam1_json/img_0.json'])['people'][0]
    assert len(long_list['pose_keypoints_2d']) == 399
    assert 'confidence_analysis' in ''.join(json.loads(str(gold['one_camera_default_output__written'])))


def write(path, text):
    with open(path, 'w') as fh:
        fh.write(text)
    return path


GOOD = json.dumps({'people': [{'pose_keypoints_2d': [0.25 + k for k in range(78)]}]})


@pytest.mark.parametrize('text', ['not json', '', json.dumps({'people': [{'pose_keypoints_2d': ['a'] * 78}]}),
                                  json.dumps({'people': [{'pose_keypoints_2d': [1.0] * 77 + [[2.0]]}]})])
def test_inputs_outside_the_contract_raise_and_write_nothing(tmp_path, text, capsys):
    cam = os.path.join(str(tmp_path), 'pose', 'cam01_json')
    os.makedirs(cam)
    write(os.path.join(cam, '000.json'), GOOD)
    bad = write(os.path.join(cam, '001.json'), text)
    out = os.path.join(str(tmp_path), 'out')
    with pytest.raises(ValueError, match='001.json') as caught:
        pc.analyze_confidence(os.path.join(str(tmp_path), 'pose'), output=out, engine=cn.NumpyConfidenceEngine())
    assert bad in str(caught.value)
    assert not os.path.exists(out)
    assert capsys.readouterr().out.count('\n') == 1                   # the 'Loading pose data' line alone


def test_unreadable_file_raises(tmp_path):
    cam = os.path.join(str(tmp_path), 'pose', 'cam01_json')
    os.makedirs(cam)
    write(os.path.join(cam, '000.json'), GOOD)
    os.symlink(os.path.join(cam, 'nowhere'), os.path.join(cam, '001.json'))     # listed, but it cannot be opened
    with pytest.raises(ValueError, match='001.json'):
        pc.analyze_confidence(os.path.join(str(tmp_path), 'pose'), engine=cn.NumpyConfidenceEngine())
    assert not os.path.exists(os.path.join(str(tmp_path), 'pose', 'confidence_analysis'))


def test_first_person_and_long_lists(tmp_path):
    """people[0] is used whatever follows it; a list of more than 78 numbers is cut to 26 keypoints."""
    cam = os.path.join(str(tmp_path), 'cam1_json')
    os.makedirs(cam)
    write(os.path.join(cam, 'a.json'), json.dumps({'people': [{'pose_keypoints_2d': [0.5] * 78}, {'pose_keypoints_2d': [9.0] * 78}]}))
    write(os.path.join(cam, 'b.json'), json.dumps({'people': [{'pose_keypoints_2d': [float(i) for i in range(399)]}, {'no': 'list'}]}))
    write(os.path.join(cam, 'c.json'), '{"people": null}')
    table = pc.load_pose_data(str(tmp_path))['cam1']
    assert np.array_equal(table[0], np.full(26, 0.5)) and np.array_equal(table[1], np.arange(2.0, 78.0, 3.0)) and np.isnan(table[2]).all()


def test_main_parses_the_reference_options(monkeypatch):
    seen = {}
    monkeypatch.setattr(pc, 'analyze_confidence', lambda **a: seen.update(a))
    monkeypatch.setattr('sys.argv', ['pose_confidence_analyze', '-p', 'some/pose', '-t', '0.55', '-o', 'where', '--no-plot'])
    pc.main()
    assert seen == {'pose_dir': 'some/pose', 'threshold': 0.55, 'output': 'where', 'no_plot': True}
    seen.clear()
    monkeypatch.setattr('sys.argv', ['pose_confidence_analyze', '--pose-dir', 'p'])
    pc.main()
    assert seen == {'pose_dir': 'p', 'threshold': 0.4, 'output': None, 'no_plot': False}
    monkeypatch.setattr('sys.argv', ['pose_confidence_analyze'])
    with pytest.raises(SystemExit):
        pc.main()


def test_defaults_are_the_references():
    import inspect
    sig = inspect.signature(pc.analyze_confidence)
    assert [(n, p.default) for n, p in sig.parameters.items()] == [
        ('pose_dir', inspect.Parameter.empty), ('threshold', 0.4), ('output', None), ('no_plot', False), ('engine', None)]
    assert pc.N_KPTS == 26 and pc.N_PROBLEM == 6


def test_engine_without_the_entries_refuses():
    """An Engine whose library lacks the new entry points raises NotImplementedError, as jitter does."""
    from pose2sim_amd.engine import Engine

    class Old:
        pass
    eng = Engine.__new__(Engine)
    eng._lib, eng._h = Old(), None
    with pytest.raises(NotImplementedError):
        eng.confidence_stats([np.zeros((2, 26))])
    with pytest.raises(NotImplementedError):
        eng.column_mean_std(np.zeros((2, 2)))
    with pytest.raises(NotImplementedError):
        eng.confidence_kernel_ms()


def test_new_entries_are_declared_exported_and_optional():
    import ctypes
    new = {'p2s_column_mean_std_host', 'p2s_confidence_stats_host', 'p2s_confidence_kernel_ms'}
    assert new <= _lib.OPTIONAL and new <= set(_lib.SIGNATURES)
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    header = open(os.path.join(root, 'include', 'p2s.h')).read()
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name in new:
        assert f'int {name}(' in header and hasattr(lib, name), name


def test_no_gpu_means_the_utility_raises(gold, tmp_path):
    """There is no CPU fallback: with the default engine and no GPU the utility raises before it writes."""
    if _lib.device_count() > 0:
        return                                                       # covered by tests/test_confidence_gpu.py
    pose_dir, args = lay_out(gold, 'special_values', str(tmp_path))
    with pytest.raises(_lib.P2sError):
        pc.analyze_confidence(pose_dir, **args)
    assert not os.path.exists(args['output'])
