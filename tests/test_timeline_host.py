"""The confidence timeline without a GPU: pose2sim_amd.confidence_timeline on the library's host path (ctx == NULL) against
the goldens recorded from the reference (tests/golden/timeline_units.npz) -- CSV bytes, printed lines with the time masked,
exceptions in type and text --, the NumPy mirror (tests/timeline_numpy.py) against the same goldens, the host path against
the mirror on seeded shapes, the native float text against repr(), the command line and the refusals.  Nothing here has a
tolerance."""
import ctypes
import json
import os
import re
import struct

import numpy as np
import pytest

import timeline_numpy as tn
from pose2sim_amd import _lib
from pose2sim_amd import confidence_timeline as ct
from pose2sim_amd import engine as eng

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'timeline_units.npz')
ALL = json.loads(str(np.load(GOLDEN)['cases']))
ERROR_CASES = [n for n in ALL if n.startswith('error_')]
assert len(ALL) == 12 and len(ERROR_CASES) == 5
ERRORS = {'ValueError': ValueError, 'FileNotFoundError': FileNotFoundError, 'TypeError': TypeError, 'AttributeError': AttributeError}
ELAPSED = re.compile(r'in \d+\.\d+s\.')
HEADER = b'frame,person,keypoint,confidence\r\n'


@pytest.fixture(scope='module')
def gold():
    return np.load(GOLDEN)


def lay_out(gold, name, work):
    """Write the case's inputs into `work` -> (json_dir, keypoints, output_dir, thresholds)."""
    args = json.loads(str(gold[f'{name}__args']))
    for d in args['folders']:
        os.makedirs(os.path.join(work, d), exist_ok=True)
    for rel, text in json.loads(str(gold[f'{name}__files'])).items():
        with open(os.path.join(work, rel), 'w') as fh:
            fh.write(text)
    return os.path.join(work, args['json_dir']), args['keypoints'], os.path.join(work, args['output']), args['thresholds']


def run_case(gold, name, work, engine, capsys):
    """The utility on `engine` in `work` against the recording, the recording's folder replaced by `work`."""
    json_dir, keypoints, output, thresholds = lay_out(gold, name, work)
    root = str(gold['work_root']) + '/' + name
    error = json.loads(str(gold[f'{name}__error']))
    capsys.readouterr()
    if error is None:
        result = ct.process(json_dir, keypoints, output, thresholds, engine=engine)
    else:
        with pytest.raises(ERRORS[error[0]]) as caught:
            ct.process(json_dir, keypoints, output, thresholds, engine=engine)
        assert type(caught.value) is ERRORS[error[0]] and str(caught.value) == error[1].replace(root, work)
        result = None
    printed = capsys.readouterr()
    want = [line for line in str(gold[f'{name}__printed']).replace(root, work).splitlines(True) if not line.startswith('  PNG: ')]
    assert ELAPSED.sub('in <t>s.', printed.out) == ''.join(want)
    assert printed.err == str(gold[f'{name}__stderr']).replace(root, work)
    assert os.path.isdir(output) == bool(gold[f'{name}__folder_made'])
    csv_path = os.path.join(output, 'confidence_timeline.csv')
    assert os.path.exists(csv_path) == bool(gold[f'{name}__has_csv'])
    if result is None:
        return None
    assert os.listdir(output) == ['confidence_timeline.csv']              # no PNG
    with open(csv_path, 'rb') as fh:
        assert fh.read() == bytes(gold[f'{name}__csv'])
    check_result(result, bytes(gold[f'{name}__csv']))
    return result


def check_result(result, data):
    """The returned dictionary against the CSV's own rows: the row arrays, and the series as the reference groups them."""
    assert list(result) == ['frame', 'person', 'keypoint', 'confidence', 'names', 'series']
    rows = [line.split(',') for line in data.decode().split('\r\n')[1:-1]]
    assert [int(r[0]) for r in rows] == result['frame'].tolist() and [int(r[1]) for r in rows] == result['person'].tolist()
    assert [r[2] for r in rows] == [result['names'][k] for k in result['keypoint']]
    assert [r[3] for r in rows] == [repr(float(v)) for v in result['confidence']]
    grouped = {}
    for frame, person, name, conf in rows:
        grouped.setdefault((name, int(person)), ([], []))
        grouped[(name, int(person))][0].append(int(frame))
        grouped[(name, int(person))][1].append(conf)
    assert list(result['series']) == list(grouped)                         # the reference's keys, in its order
    for key, (frames, confs) in grouped.items():
        assert result['series'][key][0].tolist() == frames and [repr(float(v)) for v in result['series'][key][1]] == confs, key


@pytest.mark.parametrize('name', ALL)
def test_utility_on_the_host_path_writes_the_recorded_bytes(gold, tmp_path, name, capsys):
    run_case(gold, name, str(tmp_path), tn.HostTimelineEngine(), capsys)


@pytest.mark.parametrize('name', [n for n in ALL if n not in ERROR_CASES])
def test_numpy_mirror_reproduces_the_reference(gold, name):
    args = json.loads(str(gold[f'{name}__args']))
    files = json.loads(str(gold[f'{name}__files']))
    names = list(dict.fromkeys(args['keypoints']))
    person_base, valid, conf = tn.arrays_from_documents([files[k] for k in sorted(files)], [ct.HALPE_26_INDICES[n] for n in names])
    res = tn.timeline_rows([0, len(files)], person_base, valid, conf)
    assert tn.csv_bytes(res, names) == bytes(gold[f'{name}__csv'])


def test_keypoint_table_is_the_references(gold):
    names = json.loads(str(gold['halpe_names']))
    assert ct.HALPE_26_INDICES == {n: i for i, n in enumerate(names)} and list(ct.HALPE_26_INDICES) == names
    assert ct.N_KEYPOINTS == int(gold['n_keypoints']) == 26


def test_fixture_covers_what_it_claims(gold):
    files = {n: json.loads(str(gold[f'{n}__files'])) for n in ALL}
    assert len(files['one_file_one_person']) == 1 and len(files['files_257_three_persons']) == 257
    people = [len(json.loads(t).get('people', [])) for _, t in sorted(files['mixed_people_all_keypoints'].items()) if 'f06' not in _]
    assert {0, 1, 3, 6} <= set(people)
    mixed = bytes(gold['mixed_people_all_keypoints__csv']).decode()
    assert '\r\n5,1,Nose,' in mixed and '\r\n5,0,' not in mixed and '\r\n4,' not in mixed and '\r\n6,' not in mixed and '\r\n7,2,RHeel,' in mixed
    assert '\r\n7,1,' not in mixed and '\r\n10,2,' in mixed and 'f06.json' in str(gold['mixed_people_all_keypoints__stderr'])
    assert len(json.loads(files['mixed_people_all_keypoints']['cam01_json/f08.json'])['people'][0]['pose_keypoints_2d']) == 399
    assert bytes(gold['no_valid_entry__csv']) == HEADER
    special = bytes(gold['special_confidences__csv']).decode()
    for text in (',1.0\r', ',0.0\r', ',0.1\r', ',1e-05\r', ',1.5\r', ',nan\r', ',0.30000000000000004\r'):
        assert text in special, text
    assert '"pose_keypoints_2d": [100, 50, 1, ' in files['special_confidences']['cam01_json/s00.json'] and 'NaN' in files['special_confidences']['cam01_json/s05.json']
    assert 'Keypoints: Neck, Nose, Neck, LHeel' in str(gold['name_given_twice__printed'])
    assert [json.loads(str(gold[f'{n}__error']))[0] for n in ERROR_CASES] == ['ValueError', 'FileNotFoundError', 'TypeError', 'AttributeError', 'AttributeError']
    assert [bool(gold[f'{n}__folder_made']) for n in ERROR_CASES] == [False, False, True, True, True]
    assert os.path.getsize(GOLDEN) < 1000000


# (files of every camera, longest list of every camera, K): one tile, the tile's edge, two tiles and one file; a camera
# without files between two others; cameras whose lists are empty
SHAPES = (((1,), (1,), 1), ((255, 0, 257), (2, 5, 7), 4), ((256, 513, 3), (1, 7, 0), 26), ((5,), (0,), 3), ((300, 2), (3, 3), 2))


@pytest.mark.parametrize('n_files,most,K', SHAPES)
def test_host_path_equals_the_mirror(n_files, most, K):
    case = tn.seeded_case(n_files, most, K, seed=sum(n_files) + K)
    tn.assert_same(eng.timeline_rows_host(*case), tn.timeline_rows(*case))


def test_host_path_with_no_valid_person():
    file_off, person_base, valid, conf = tn.seeded_case((40, 300), (3, 2), 4, seed=3, p_valid=(0.0, 0.5))
    got = eng.timeline_rows_host(file_off, person_base, valid, conf)
    tn.assert_same(got, tn.timeline_rows(file_off, person_base, valid, conf))
    assert got['row_off'][1] == 0 and got['n_people'][0] == 3 and list(got['series_off'][:4]) == [0, 0, 0, 0]


def native_csv(tmp_path, values):
    """The confidence column of the native CSV of one row a value, as text."""
    n = len(values)
    path = os.path.join(str(tmp_path), 'floats.csv')
    eng.write_timeline_csv(path, np.arange(n), np.zeros(n), np.zeros(n), values, ['Nose'])
    with open(path, 'rb') as fh:
        lines = fh.read().split(b'\r\n')
    assert lines[0] + b'\r\n' == HEADER and lines[-1] == b'' and len(lines) == n + 2
    for i, line in enumerate(lines[1:-1]):
        assert line.startswith(b'%d,0,Nose,' % i)
    return [line.split(b',')[3].decode() for line in lines[1:-1]]


def test_native_float_text_is_repr_on_the_listed_values(tmp_path):
    values = [0.1, 1.0, 1e16, 9999999999999998.0, 1e-05, 0.0001, 5e-324, 1.7976931348623157e308, 0.30000000000000004, -0.0,
              float('nan'), float('inf'), float('-inf')]
    assert native_csv(tmp_path, np.array(values)) == [repr(v) for v in values]
    assert native_csv(tmp_path, np.array([-float('nan'), 123456789012345.6, 1234567890123456.8, 1e15, 1e-4, 9.999e-05])) \
        == ['nan', '123456789012345.6', '1234567890123456.8', '1000000000000000.0', '0.0001', '9.999e-05']


def test_native_float_text_is_repr_on_random_bit_patterns(tmp_path):
    bits = np.random.default_rng(2026).integers(0, 1 << 64, 10000, dtype=np.uint64)
    values = bits.view(np.float64)
    assert np.isnan(values).any() and (np.abs(values[~np.isnan(values)]) < 1e-300).any()
    got = native_csv(tmp_path, values)
    want = [repr(struct.unpack('<d', struct.pack('<Q', int(b)))[0]) for b in bits]
    assert got == want


def test_native_writer_in_blocks_equals_csv_writer(tmp_path):
    """More rows than one formatting block, on one thread and on several."""
    case = tn.seeded_case((7000,), (4,), 5, seed=8)
    res = tn.timeline_rows(*case)
    names = ['Nose', 'LEye', 'REye', 'LEar', 'REar']
    assert len(res['frame']) > 2 * 16384
    for threads in (1, 5):
        path = os.path.join(str(tmp_path), f't{threads}.csv')
        eng.write_timeline_csv(path, res['frame'], res['person'], res['slot'], res['confidence'], names, n_threads=threads)
        with open(path, 'rb') as fh:
            assert fh.read() == tn.csv_bytes(res, names)


def test_native_writer_refusals(tmp_path):
    path = os.path.join(str(tmp_path), 'x.csv')
    with pytest.raises(_lib.P2sError, match='slot 1 of 1'):
        eng.write_timeline_csv(path, [0], [0], [1], [0.5], ['Nose'])
    with pytest.raises(_lib.P2sError, match='would quote'):
        eng.write_timeline_csv(path, [0], [0], [0], [0.5], ['No,se'])
    assert not os.path.exists(path)
    with pytest.raises(ValueError):
        eng.write_timeline_csv(path, [0, 1], [0], [0], [0.5], ['Nose'])


def write_folder(folder, seed, n_files=7, most=3):
    """A small folder of the golden generator's kind, written by the test."""
    rng = np.random.default_rng(seed)
    os.makedirs(folder)
    for f in range(n_files):
        people = []
        for _ in range(int(rng.integers(0, most + 1))):
            n = 78 if rng.random() < 0.7 else 75
            people.append({'person_id': [-1], 'pose_keypoints_2d': [float(v) for v in np.round(rng.uniform(0.0, 1.0, n), 3)]})
        with open(os.path.join(folder, f'{f:03d}.json'), 'w') as fh:
            fh.write(json.dumps({'version': 1.3, 'people': people}) if f != 4 else 'not json')
    return folder


def test_several_folders_in_one_call_equal_separate_calls(tmp_path, capsys):
    root = str(tmp_path)
    dirs = [write_folder(os.path.join(root, f'cam{c}_json'), 10 + c, n_files=5 + 3 * c) for c in range(3)]
    names = ['Neck', 'RHeel', 'Neck']
    engine = tn.HostTimelineEngine()
    together = ct.confidence_timelines(dirs, names, [os.path.join(root, f'all{c}') for c in range(3)], engine=engine)
    quiet = ct.confidence_timelines(dirs, names, engine=engine)
    assert capsys.readouterr().out.count('Done.') == 3
    assert sorted(os.listdir(root)) == ['all0', 'all1', 'all2', 'cam0_json', 'cam1_json', 'cam2_json']     # None writes nothing
    for c, d in enumerate(dirs):
        one = ct.process(d, names, os.path.join(root, f'one{c}'), None, engine=engine)
        with open(os.path.join(root, f'one{c}', 'confidence_timeline.csv'), 'rb') as a, open(os.path.join(root, f'all{c}', 'confidence_timeline.csv'), 'rb') as b:
            data = a.read()
            assert data == b.read() and len(data) > len(HEADER)
        for res in (together[c], quiet[c]):
            assert res['names'] == one['names'] == ['Neck', 'RHeel'] and list(res['series']) == list(one['series'])
            for key in ('frame', 'person', 'keypoint', 'confidence'):
                assert tn.same(res[key], one[key]), key
            for key in one['series']:
                assert tn.same(res['series'][key][0], one['series'][key][0]) and tn.same(res['series'][key][1], one['series'][key][1])
        check_result(one, data)


GOOD = json.dumps({'people': [{'pose_keypoints_2d': [0.25 + k for k in range(78)]}]})


@pytest.mark.parametrize('text', [json.dumps({'people': [{'pose_keypoints_2d': ['a'] * 78}]}), json.dumps({'people': [{'pose_keypoints_2d': [1.0] * 77 + [[2.0]]}]}),
                                  json.dumps({'people': [3]}), json.dumps({'people': 'abc'}), json.dumps({'people': [{'pose_keypoints_2d': 5}]}),
                                  json.dumps({'people': [{'pose_keypoints_2d': [None] * 78}]}), b'\xff\xfe{}'])
def test_inputs_outside_the_contract_raise_and_write_nothing(tmp_path, text, capsys):
    cam = os.path.join(str(tmp_path), 'cam01_json')
    os.makedirs(cam)
    with open(os.path.join(cam, '000.json'), 'w') as fh:
        fh.write(GOOD)
    bad = os.path.join(cam, '001.json')
    with open(bad, 'wb') as fh:
        fh.write(text if isinstance(text, bytes) else text.encode())
    out = os.path.join(str(tmp_path), 'out')
    with pytest.raises(ValueError, match='001.json') as caught:
        ct.process(cam, ['Nose'], out, None, engine=tn.HostTimelineEngine())
    assert bad in str(caught.value) and not os.path.exists(out)
    printed = capsys.readouterr()
    assert printed.out == '' and printed.err == ''


def test_unreadable_file_raises(tmp_path):
    cam = os.path.join(str(tmp_path), 'cam01_json')
    os.makedirs(cam)
    with open(os.path.join(cam, '000.json'), 'w') as fh:
        fh.write(GOOD)
    os.symlink(os.path.join(cam, 'nowhere'), os.path.join(cam, '001.json'))     # listed, but it cannot be opened
    with pytest.raises(ValueError, match='001.json'):
        ct.process(cam, ['Nose'], os.path.join(str(tmp_path), 'out'), None, engine=tn.HostTimelineEngine())
    assert not os.path.exists(os.path.join(str(tmp_path), 'out'))


def test_main_parses_the_reference_options(monkeypatch, tmp_path, capsys):
    seen = []
    monkeypatch.setattr(ct, 'process', lambda *a: seen.append(a))
    folder = str(tmp_path)
    monkeypatch.setattr('sys.argv', ['confidence_timeline', '-j', folder + '/'])
    ct.main()
    assert seen.pop() == (folder + '/', ['Nose', 'Neck', 'RShoulder', 'LShoulder'], folder + '_conf_timeline', None)
    monkeypatch.setattr('sys.argv', ['confidence_timeline', '--json_dir', folder, '-k', 'Nose, RHeel', '-o', 'where', '-t', '0.3, 0.5'])
    ct.main()
    assert seen.pop() == (folder, ['Nose', 'RHeel'], 'where', [0.3, 0.5])
    for argv, text in ((['-j', folder + '/missing'], f'Error: Input directory not found: {folder}/missing\n'),
                       (['-j', folder, '-t', '0.3,x'], 'Error: Invalid threshold value: 0.3,x\n')):
        monkeypatch.setattr('sys.argv', ['confidence_timeline'] + argv)
        with pytest.raises(SystemExit) as caught:
            ct.main()
        assert caught.value.code == 1 and capsys.readouterr().err == text and not seen
    monkeypatch.setattr('sys.argv', ['confidence_timeline'])
    with pytest.raises(SystemExit):
        ct.main()


def test_signatures_are_the_references():
    import inspect
    assert [(n, p.default) for n, p in inspect.signature(ct.process).parameters.items()] == [
        ('json_dir', inspect.Parameter.empty), ('keypoint_names', inspect.Parameter.empty), ('output_dir', inspect.Parameter.empty),
        ('thresholds', inspect.Parameter.empty), ('engine', None)]
    assert [(n, p.default) for n, p in inspect.signature(ct.confidence_timelines).parameters.items()] == [
        ('json_dirs', inspect.Parameter.empty), ('keypoint_names', inspect.Parameter.empty), ('output_dirs', None), ('engine', None)]


def test_engine_input_checks_raise_value_error():
    file_off, person_base, valid, conf = tn.seeded_case((4, 3), (2, 2), 3, seed=1)
    for args in (([0, 5, 4], person_base, valid, conf), ([1, 4, 7], person_base, valid, conf), (file_off, person_base[:-1], valid, conf),
                 (file_off, person_base[::-1], valid, conf), (file_off, person_base, valid[:-1], conf), (file_off, person_base, valid, conf[:-1]),
                 (file_off, person_base, valid, conf[:, :0]), (file_off, person_base, valid, np.zeros((len(valid), 27))),
                 (file_off, person_base, valid, conf[:, 0])):
        with pytest.raises(ValueError):
            eng.timeline_rows_host(*args)


def test_library_refuses_other_sizes():
    """The C entry point checks the caller's n_rows and n_series against the input before it writes."""
    lib = _lib.load()
    file_off, person_base = np.array([0, 1], dtype=np.int64), np.array([0, 1], dtype=np.int64)
    valid, conf = np.ones(1, dtype=np.uint8), np.zeros((1, 2))
    ptr = lambda a: a.ctypes.data_as(ctypes.c_void_p)                       # noqa: E731
    outs = [np.zeros(8, dtype=np.int64) for _ in range(9)]
    for n_rows, n_series in ((1, 1), (2, 2)):
        rc = lib.p2s_timeline_rows_host(None, 1, ptr(file_off), ptr(person_base), ptr(valid), 2, ptr(conf), n_rows, n_series, *[ptr(o) for o in outs])
        assert rc == _lib.P2S_ERR_INVALID_ARG and b'2 rows and 1 series' in lib.p2s_last_error()
    assert not any(o.any() for o in outs)


def test_engine_without_the_entries_refuses():
    """An Engine whose library lacks the new entry points raises NotImplementedError, as its siblings do."""
    class Old:
        pass
    engine = eng.Engine.__new__(eng.Engine)
    engine._lib, engine._h = Old(), None
    with pytest.raises(NotImplementedError):
        engine.timeline_rows([0, 0], [0], [], np.zeros((0, 1)))
    with pytest.raises(NotImplementedError):
        engine.timeline_kernel_ms()


def test_new_entries_are_declared_exported_and_optional():
    new = {'p2s_timeline_rows_host', 'p2s_timeline_kernel_ms', 'p2s_timeline_write_csv'}
    assert new <= _lib.OPTIONAL and new <= set(_lib.SIGNATURES)
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    header = open(os.path.join(root, 'include', 'p2s.h')).read()
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name in new:
        assert f'int {name}(' in header and hasattr(lib, name), name


def test_module_runs_as_a_script_and_refuses_without_a_gpu(gold, tmp_path):
    """python -m pose2sim_amd.confidence_timeline -j <folder>: there is no CPU fallback, so without a GPU it ends with the
    library's error before anything is written; with one, tests/test_timeline_gpu.py checks the bytes."""
    import subprocess
    import sys
    json_dir, _, _, _ = lay_out(gold, 'six_persons_single_keypoint', str(tmp_path))
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    run = subprocess.run([sys.executable, '-m', 'pose2sim_amd.confidence_timeline', '-j', json_dir, '-k', 'RHeel'], cwd=root, capture_output=True, text=True)
    out = json_dir + '_conf_timeline'
    if _lib.device_count() > 0:
        assert run.returncode == 0, run.stderr
        with open(os.path.join(out, 'confidence_timeline.csv'), 'rb') as fh:
            assert fh.read() == bytes(gold['six_persons_single_keypoint__csv'])
    else:
        assert run.returncode != 0 and 'P2sError' in run.stderr and not os.path.exists(out)
