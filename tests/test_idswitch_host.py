"""The ID switch utility without a GPU: pose2sim_amd.id_switch_analyze on the NumPy / scipy stand-in (tests/idswitch_numpy.py)
against the goldens recorded from the reference (tests/golden/idswitch_units.npz) -- the returned dictionary element for
element, the three files and the printed text byte for byte, the errors by type and message -- the native ingest's
person_id reader on the recorded files, and csrc/p2s_lsap.h compiled for the host against scipy's own
linear_sum_assignment, ties included.  Nothing here has a tolerance."""
import ctypes
import json
import os

import numpy as np
import pytest
from scipy.optimize import linear_sum_assignment

import idswitch_numpy as isn
from pose2sim_amd import _lib
from pose2sim_amd import id_switch_analyze as ids
from test_jitter_host import same

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'idswitch_units.npz')
ALL = json.loads(str(np.load(GOLDEN)['cases']))
ERROR_CASES = [n for n in ALL if n.startswith('error_')]
assert len(ALL) == 14 and len(ERROR_CASES) == 9
ERRORS = {e.__name__: e for e in (KeyError, ValueError, TypeError, AttributeError, ZeroDivisionError, FileNotFoundError)}
RESULT_KEYS = ['events', 'match_distances', 'detection_counts', 'person_id_values', 'n_frames', 'n_errors', 'distance_stats', 'pattern_counts']
# every shape from 1 x 1 to 8 x 8, the large and the lopsided ones, and sizes between: around 8 and 16, nearly square both ways
SHAPES = [(r, c) for r in range(1, 9) for c in range(1, 9)] + [(32, 32), (1, 32), (32, 1), (32, 20), (20, 32)]
SHAPES += [(8, 9), (9, 8), (9, 9), (13, 17), (17, 13), (16, 16), (31, 32), (32, 31)]
KINDS = ('continuous', 'integers 0 to 2', 'continuous, 40 % at 1e9', 'integers, 40 % at 1e9', 'all 1e9')


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
    if 'output_dir' in args:
        args['output_dir'] = os.path.join(work, args['output_dir'])
    return os.path.join(work, str(gold[f'{name}__pose_dir'])), args


def recorded_result(gold, name):
    """The recorded dictionary with detection_counts' keys back in place (0, 1, 2, '3+'), or None for an error case."""
    result = json.loads(str(gold[f'{name}__result']))
    if result is not None:
        for res in result.values():
            res['detection_counts'] = {k: v for k, v in res['detection_counts']}
    return result


def check_result(result, want):
    """The reference's keys in its order, Python ints, floats and strings, the recorded values and bits."""
    assert list(result) == list(want)
    for cam in want:
        got, ref = result[cam], want[cam]
        assert list(got) == RESULT_KEYS
        assert got['events'] == ref['events'] and all(list(a) == list(b) for a, b in zip(got['events'], ref['events']))
        assert all(type(v) is type(w) for a, b in zip(got['events'], ref['events']) for v, w in zip(a.values(), b.values()))
        assert all(type(d) is float for d in got['match_distances']) and same(got['match_distances'], ref['match_distances']), cam
        for key in ('detection_counts', 'person_id_values', 'pattern_counts', 'distance_stats'):
            assert list(got[key].items()) == list(ref[key].items()), (cam, key)
            assert [type(v) for v in got[key].values()] == [type(v) for v in ref[key].values()], (cam, key)
        assert same(list(got['distance_stats'].values()), list(ref['distance_stats'].values())), cam
        assert (got['n_frames'], got['n_errors']) == (ref['n_frames'], ref['n_errors']) and type(got['n_frames']) is int and type(got['n_errors']) is int


def run_case(gold, name, work, engine, capsys, monkeypatch):
    """The utility on `engine` in `work` (the working directory too: the default output folder is relative): the files
    written, what was printed, the error and the returned dictionary against the recording, its folder replaced by `work`."""
    pose_dir, args = lay_out(gold, name, work)
    root = str(gold['work_root']) + '/' + name
    error = json.loads(str(gold[f'{name}__error']))
    before = {os.path.join(r, f) for r, _, fs in os.walk(work) for f in fs}
    monkeypatch.chdir(work)
    capsys.readouterr()
    if error is None:
        result = ids.analyze_id_switches(pose_dir, engine=engine, **args)
        assert capsys.readouterr().out == str(gold[f'{name}__printed']).replace(root, work)
        check_result(result, recorded_result(gold, name))
    else:
        with pytest.raises(ERRORS[error[0]]) as caught:
            ids.analyze_id_switches(pose_dir, engine=engine, **args)
        assert type(caught.value) is ERRORS[error[0]] and str(caught.value) == error[1].replace(root, work)
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


def engine_tables_of_case(gold, name, work, engine):
    """engine.id_switch on the case's cameras as the utility loads them -> (its result, the loaded cameras)."""
    pose_dir, _ = lay_out(gold, name, work)
    cams = [ids.load_camera(d) for d in sorted(ids.Path(pose_dir).glob('cam*_json'))]
    return engine.id_switch([(cam['persons'], cam['offsets']) for cam in cams]), cams


def check_engine_on_case(gold, name, work, engine, report=print):
    """The engine's tables, distances and statistics on a recorded case against the recording and against the stand-in."""
    want = recorded_result(gold, name)
    res, cams = engine_tables_of_case(gold, name, work, engine)
    ref = isn.NumpyIdSwitchEngine().id_switch([(cam['persons'], cam['offsets']) for cam in cams])
    report(f'{name}: {len(cams)} cameras, {[len(cam["offsets"]) - 1 for cam in cams]} frames, {[len(d) for d in res["distances"]]} distances')
    for c, cam_name in enumerate(want):
        assert same(res['distances'][c], want[cam_name]['match_distances']), (name, cam_name)
        stats = want[cam_name]['distance_stats']
        if stats['count']:
            assert same(res['stats'][c], [stats[k] for k in isn.STATS]), (name, cam_name)
        else:
            assert np.isnan(res['stats'][c]).all()
        for key in isn.TABLES + ('kept',):
            assert np.array_equal(res[key][c], ref[key][c]), (name, cam_name, key)
        lost = sum(1 for e in want[cam_name]['events'] if e['event_type'] == 'person_lost')
        assert int(res['n_lost'][c].sum()) == lost and int(res['n_matched'][c].sum()) == len(want[cam_name]['match_distances'])


@pytest.mark.parametrize('name', ALL)
def test_utility_on_the_stand_in_reproduces_the_reference(gold, tmp_path, name, capsys, monkeypatch):
    run_case(gold, name, str(tmp_path), isn.NumpyIdSwitchEngine(), capsys, monkeypatch)


@pytest.mark.parametrize('name', [n for n in ALL if n not in ERROR_CASES])
def test_stand_in_tables_reproduce_the_reference(gold, tmp_path, name, capsys):
    with capsys.disabled():
        check_engine_on_case(gold, name, str(tmp_path), isn.NumpyIdSwitchEngine())


def test_person_ids_of_the_recorded_files(gold, tmp_path):
    from pose2sim_amd.ingest import JsonBatch
    pose_dir, _ = lay_out(gold, 'one_camera_default_output', str(tmp_path))
    files = sorted(os.path.join(pose_dir, 'cam01_json', f) for f in os.listdir(os.path.join(pose_dir, 'cam01_json')))
    with JsonBatch(files) as batch:
        texts, kinds = batch.person_ids()
    want = []
    for f in files:
        with open(f) as fh:
            want += [json.dumps(p['person_id']).encode() if 'person_id' in p else None for p in json.load(fh)['people']]
    assert texts == want and {None, b'[-1]', b'[3]', b'7', b'[1.0]'} == set(texts)
    assert (kinds == _lib.P2S_JSON_DOC_PEOPLE).all()


def test_person_ids_raw_text_and_file_kinds(tmp_path):
    from pose2sim_amd.ingest import JsonBatch
    kp = json.dumps([0.5] * 78)
    texts = ['{"people": [{"person_id": [ -1,\n 2 ], "pose_keypoints_2d": %s}, {"pose_keypoints_2d": %s, "person_id": 1, "person_id": "a\\"b"}, {}]}' % (kp, kp),
             '{"version": 1}', '{"people": null}', '{"people": 5}', '[1]', '"s"', '12', '-1.5e3', 'true', 'null', 'NaN', 'nope', '{"people": []}']
    files = []
    for i, text in enumerate(texts):
        files.append(os.path.join(str(tmp_path), f'{i:02d}.json'))
        with open(files[-1], 'w') as fh:
            fh.write(text)
    with JsonBatch(files) as batch:
        ids_, kinds = batch.person_ids()
    assert ids_ == [b'[ -1,\n 2 ]', b'"a\\"b"', None]                      # the raw text; a repeated key takes the last value
    assert list(kinds) == [0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 7, -1, 0]
    assert [_lib.P2S_JSON_DOC_TYPES[k] for k in kinds[4:11]] == [type(json.loads(t)).__name__ for t in texts[4:11]]


def lsap_host(cost):
    """csrc/p2s_lsap.h compiled for the host: p2s_lsap_host without a context."""
    cost = np.ascontiguousarray(cost, dtype=np.float64)
    n, k = len(cost), min(cost.shape[1:])
    rows, cols, status = np.empty((n, k), dtype=np.int32), np.empty((n, k), dtype=np.int32), np.empty(n, dtype=np.int32)
    _lib.check(_lib.load().p2s_lsap_host(None, n, cost.shape[1], cost.shape[2], cost.ctypes.data_as(ctypes.c_void_p),
                                         rows.ctypes.data_as(ctypes.c_void_p), cols.ctypes.data_as(ctypes.c_void_p),
                                         status.ctypes.data_as(ctypes.c_void_p)))
    return rows, cols, status


def lsap_matrices(shape, kind, n=24):
    """n seeded matrices of the shape; ties are the rule for the integer kinds and for the entries at 1e9."""
    rng = np.random.default_rng(1000 * shape[0] + shape[1])
    cost = rng.uniform(0.0, 100.0, (n,) + shape) if kind.startswith('continuous') else rng.integers(0, 3, (n,) + shape).astype(np.float64)
    if '40 %' in kind:
        cost[rng.random(cost.shape) < 0.4] = 1e9
    if kind == 'all 1e9':
        cost[:] = 1e9
    return cost


def check_lsap(solve, shape, kind):
    cost = lsap_matrices(shape, kind)
    rows, cols = solve(cost)
    for b, m in enumerate(cost):
        r, c = linear_sum_assignment(m)
        assert np.array_equal(rows[b], r) and np.array_equal(cols[b], c), (shape, kind, b)


@pytest.mark.parametrize('kind', KINDS)
def test_lsap_header_on_the_host_equals_scipy(kind):
    for shape in SHAPES:
        check_lsap(lambda cost: lsap_host(cost)[:2], shape, kind)


def test_lsap_refuses_what_scipy_refuses():
    cost = np.ones((3, 2, 3))
    cost[1, 0, 1] = np.nan
    cost[2, 1] = np.inf
    rows, cols, status = lsap_host(cost)
    assert list(status) == [0, 1, 2] and (rows[1:] == -1).all() and (cols[1:] == -1).all()
    for m, code in ((cost[1], 1), (cost[2], 2)):
        with pytest.raises(ValueError) as caught:
            linear_sum_assignment(m)
        assert str(caught.value) == _lib.P2S_LSAP_ERRORS[code]
    neg = np.ones((1, 2, 2))
    neg[0, 0, 0] = -np.inf
    assert lsap_host(neg)[2][0] == 1
    with pytest.raises(_lib.P2sError, match='expected 1 .. 32 rows and columns'):
        lsap_host(np.zeros((1, 33, 2)))


def test_pattern_classification_is_the_references_and_linear():
    """The stack gives the reference's marks where its backward search reaches past the resumed event's own gap."""
    def ev(frame, kind, gap=''):
        return {'frame': frame, 'event_type': kind, 'prev_count': 0, 'curr_count': 0, 'match_distance': '', 'gap_frames': gap, 'pattern': ''}
    events = [ev(5, 'no_detection'), ev(50, 'detection_resumed', 45), ev(60, 'no_detection'), ev(62, 'detection_resumed', 2),
              ev(70, 'detection_resumed', 3), ev(80, 'detection_resumed', 4)]
    out, counts = ids.classify_patterns(events, fps=30)
    assert [e['pattern'] for e in out] == ['A', 'D', 'A', 'A', 'A', 'A'] and counts == {'A': 3, 'B': 0, 'C': 0, 'D': 1}
    import time
    many = [ev(2 * i, 'detection_resumed' if i % 2 else 'person_lost', 2 if i % 2 else '') for i in range(200000)]
    t0 = time.perf_counter()                                          # no no_detection to find: the reference's search
    _, counts = ids.classify_patterns(many, fps=30)                   # walks back to the start for every resumed event
    assert time.perf_counter() - t0 < 5.0 and counts == {'A': 100000, 'B': 0, 'C': 0, 'D': 100000}


def test_more_than_32_valid_persons_are_refused(tmp_path):
    cam = os.path.join(str(tmp_path), 'pose', 'cam01_json')
    os.makedirs(cam)
    one = {'pose_keypoints_2d': [0.5] * 78}
    for i, n in enumerate((32, 33)):
        with open(os.path.join(cam, f'{i}.json'), 'w') as fh:
            json.dump({'people': [one] * n}, fh)
    out = os.path.join(str(tmp_path), 'out')
    with pytest.raises(ValueError, match='1.json holds 33 valid persons'):
        ids.analyze_id_switches(os.path.join(str(tmp_path), 'pose'), output_dir=out, engine=isn.NumpyIdSwitchEngine())
    assert not os.path.exists(out)


def test_main_parses_the_reference_options(monkeypatch):
    seen = {}
    monkeypatch.setattr(ids, 'analyze_id_switches', lambda **a: seen.update(a))
    monkeypatch.setattr('sys.argv', ['id_switch_analyze', '-p', 'some/pose', '-o', 'where', '--fps', '60'])
    ids.main()
    assert seen == {'pose_dir': 'some/pose', 'output_dir': 'where', 'fps': 60}
    seen.clear()
    monkeypatch.setattr('sys.argv', ['id_switch_analyze', '--pose-dir', 'p'])
    ids.main()
    assert seen == {'pose_dir': 'p', 'output_dir': None, 'fps': 30}
    monkeypatch.setattr('sys.argv', ['id_switch_analyze'])
    with pytest.raises(SystemExit):
        ids.main()


def test_engine_without_the_entries_refuses():
    from pose2sim_amd.engine import Engine

    class Old:
        pass
    eng = Engine.__new__(Engine)
    eng._lib, eng._h = Old(), None
    with pytest.raises(NotImplementedError):
        eng.id_switch([(np.zeros((1, 26, 3)), [0, 1])])
    with pytest.raises(NotImplementedError):
        eng.lsap(np.zeros((2, 2)))
    with pytest.raises(NotImplementedError):
        eng.id_switch_kernel_ms()


def test_new_entries_are_declared_exported_and_optional():
    new = {'p2s_lsap_host', 'p2s_id_switch_host', 'p2s_id_switch_kernel_ms', 'p2s_json_person_ids'}
    assert new <= _lib.OPTIONAL and new <= set(_lib.SIGNATURES)
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    header = open(os.path.join(root, 'include', 'p2s.h')).read()
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name in new:
        assert f'int {name}(' in header and hasattr(lib, name), name


def test_no_gpu_means_the_utility_raises(gold, tmp_path):
    """There is no CPU fallback: with the default engine and no GPU the utility raises before it writes."""
    if _lib.device_count() > 0:
        return                                                       # covered by tests/test_idswitch_gpu.py
    pose_dir, args = lay_out(gold, 'shared_keypoints', str(tmp_path))
    with pytest.raises(_lib.P2sError):
        ids.analyze_id_switches(pose_dir, **args)
    assert not os.path.exists(args['output_dir'])
