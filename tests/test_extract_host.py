"""The primary-person extraction without a GPU: pose2sim_amd.pose_extract_person on the NumPy restatement
(tests/extract_numpy.py) against the goldens recorded from the reference (tests/golden/extract_units.npz) -- files byte for
byte, printed text with the seconds masked, warnings, exceptions and the files written before them --, the restatement
against the native host selection (JsonBatch.select_tracked_person, pinned to the reference by tests/test_jitter_host.py),
the native writer against json.dump, the parser's integer-token flag and the refusals.  Nothing here has a tolerance."""
import functools
import json
import os
import re

import numpy as np
import pytest

import extract_numpy as en
from test_jitter_host import numpy_choice
from pose2sim_amd import _lib
from pose2sim_amd import pose_extract_person as pe

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'extract_units.npz')
ALL = json.loads(str(np.load(GOLD)['cases']))
ERROR_CASES = [n for n in ALL if n.startswith('error_')]
assert len(ALL) == 19 and len(ERROR_CASES) == 7
ERRORS = {'TypeError': TypeError, 'ValueError': ValueError, 'AttributeError': AttributeError, 'FileNotFoundError': FileNotFoundError,
          'SystemExit': SystemExit}
SECONDS = re.compile(r'processed in \d+\.\ds\.')


@pytest.fixture(scope='module')
def gold():
    return np.load(GOLD)


def lay_out(gold, name, work):
    for d in json.loads(str(gold[f'{name}__folders'])):
        os.makedirs(os.path.join(work, d), exist_ok=True)
    for rel, text in json.loads(str(gold[f'{name}__files'])).items():
        os.makedirs(os.path.dirname(os.path.join(work, rel)), exist_ok=True)
        with open(os.path.join(work, rel), 'w') as fh:
            fh.write(text)
    return json.loads(str(gold[f'{name}__call']))


def run_case(gold, name, work, engine, capsys, monkeypatch):
    """The utility on `engine` in `work` (the working directory, as in the recording): every file outside the input folder,
    what was printed, the warnings and the error against the recording, the recording's folder replaced by `work`."""
    call = lay_out(gold, name, work)
    root = str(gold['work_root']) + '/' + name
    error = json.loads(str(gold[f'{name}__error']))
    monkeypatch.chdir(work)
    capsys.readouterr()

    def run():
        if call['mode'] == 'main':
            monkeypatch.setattr(pe, 'process', functools.partial(pe.process, engine=engine))
            monkeypatch.setattr('sys.argv', ['pose_extract_person'] + call['argv'])
            pe.main()
        else:
            pe.process(os.path.join(work, call['input']), os.path.join(work, call['output']), engine=engine)
    if error is None:
        run()
    else:
        with pytest.raises(ERRORS[error[0]]) as caught:
            run()
        assert type(caught.value).__name__ == error[0]
        assert str(caught.value) == error[1].replace(root, work)
    printed = capsys.readouterr()
    assert SECONDS.sub('processed in #s.', printed.out) == SECONDS.sub('processed in #s.', str(gold[f'{name}__printed']).replace(root, work))
    lines = [ln for ln in printed.err.splitlines() if ln.startswith(('Warning:', 'Error:'))]
    assert lines == [ln.replace(root, work) for ln in json.loads(str(gold[f'{name}__stderr']))]
    inside = os.path.join(work, call['input'].rstrip('/')) + os.sep
    found = {}
    for r, _, fs in os.walk(work):
        for f in fs:
            p = os.path.join(r, f)
            if not p.startswith(inside):
                with open(p, encoding='utf-8', newline='') as fh:
                    found[os.path.relpath(p, work)] = fh.read()
    want = json.loads(str(gold[f'{name}__found']))
    assert sorted(found) == sorted(want)
    for rel in want:
        assert found[rel] == want[rel], rel


@pytest.mark.parametrize('name', ALL)
def test_utility_reproduces_the_recorded_case(gold, tmp_path, name, capsys, monkeypatch):
    run_case(gold, name, str(tmp_path), en.NumpyExtractEngine(), capsys, monkeypatch)


def test_fixture_covers_what_it_claims(gold):
    found = json.loads(str(gold['all_integer__found']))
    assert all(re.search(r'"pose_keypoints_2d": \[\d+, \d+, 1, ', t) for t in found.values())
    mixed = json.loads(str(gold['integer_one_float__found']))
    assert any('300.5' in t and '1.0, ' in t for t in mixed.values()) and any('"pose_keypoints_2d": [700, ' in t for t in mixed.values())
    odd = ''.join(json.loads(str(gold['nan_infinity__found'])).values())
    assert 'NaN' in odd and '-Infinity' in odd and ' Infinity' in odd
    assert json.loads(str(gold['bad_file_between__found']))['out/f003.json'] == '{"version": 1.3, "people": []}'
    assert len(json.loads(str(gold['bad_file_between__stderr']))) == 1
    for name in ('error_people_null', 'error_133_keypoints', 'error_top_level_list', 'error_person_number'):
        assert sorted(json.loads(str(gold[f'{name}__found']))) == ['out/f000.json', 'out/f001.json', 'out/f002.json']   # written before the raise
    assert 'cam02_json_person/f000.json' in json.loads(str(gold['main_trailing_slash__found']))
    kept = json.loads(str(gold['main_existing_output__found']))
    assert kept['out/old.json'] == '{"kept": true}' and kept['out/f001.json'] != 'overwritten'
    assert json.loads(str(gold['error_main_missing_input__error'])) == ['SystemExit', '1']


# ---- the restatement against the native host selection ---------------------------------------------------------------
def staged_camera(files):
    """-> (persons, offsets, people index of every staged person, (status, detail) of the host selection)."""
    from pose2sim_amd.ingest import JsonBatch
    with JsonBatch(files) as batch:
        _, status, detail = batch.select_tracked_person(26, 0.1)
        lengths = batch.person_lengths
        file_of = np.repeat(np.arange(len(files)), np.maximum(batch.counts, 0))
        rows = np.flatnonzero(lengths == 78)
        index = (rows - batch.person_base[file_of[rows]]).astype(np.int32)
        persons, _ = batch.gather_people(file_of[rows], index, 78)
    offsets = np.concatenate([[0], np.cumsum(np.bincount(file_of[rows], minlength=len(files)))])
    return persons.reshape(-1, 26, 3), offsets, index, status, detail


def check_against_host_selection(files):
    persons, offsets, index, status, detail = staged_camera(files)
    bad = np.flatnonzero(status < 0)
    n = int(bad[0]) if len(bad) else len(files)                      # the reference's run ends at the first such file
    res = en.NumpyExtractEngine().track_select([(persons[:offsets[n]], offsets[:n + 1])])
    chosen = res['chosen'][0]
    selected = status[:n] == _lib.P2S_TRACK_SELECTED
    assert np.array_equal(chosen >= 0, selected)
    assert np.array_equal(index[offsets[:n][selected] + chosen[selected]], detail[:n][selected])
    return int(selected.sum())


@pytest.mark.parametrize('name', ALL)
def test_restatement_chooses_what_the_host_selection_chooses(gold, tmp_path, name):
    call = lay_out(gold, name, str(tmp_path))
    files = sorted(os.path.join(str(tmp_path), rel) for rel in json.loads(str(gold[f'{name}__files'])) if rel.startswith(call['input'].rstrip('/') + '/')
                   and rel.endswith('.json'))
    if files:
        check_against_host_selection(files)


def test_restatement_and_host_selection_agree_on_ties(tmp_path):
    """400 frames of three persons: one near the previous choice, one the same distances away with its keypoints permuted (the
    sums differ by rounding alone, or not at all), one an exact copy of one of them (an exact tie: the first listed wins)."""
    rng = np.random.default_rng(11)
    prev, files = None, []
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
            people = [a, b, (a if f % 5 else b).copy()]
            people = [people[i] for i in rng.permutation(3)]
        prev = people[numpy_choice(people, prev)]                    # the rule in plain NumPy: the next frame's ties are about this one
        path = os.path.join(str(tmp_path), f'{f:04d}.json')
        with open(path, 'w') as fh:
            json.dump({'people': [{'pose_keypoints_2d': [float(v) for v in p.ravel()]} for p in people]}, fh)
        files.append(path)
    assert check_against_host_selection(files) == 400


def test_track_select_of_several_cameras_and_extract_persons(gold, tmp_path, capsys):
    """Two folders in one call write what one call each writes."""
    names = ('two_crossing', 'three_crossing')
    for n in names:
        lay_out(gold, n, os.path.join(str(tmp_path), n))
    ins = [os.path.join(str(tmp_path), n, 'cam01_json') for n in names]
    outs = [os.path.join(str(tmp_path), n, 'both') for n in names]
    for o in outs:
        os.makedirs(o)
    report = pe.extract_persons(ins, outs, engine=en.NumpyExtractEngine())
    assert len(report) == 2 and capsys.readouterr().out.count('Done. 60 frames processed') == 2
    for n, o in zip(names, outs):
        want = json.loads(str(gold[f'{n}__found']))
        assert sorted(os.listdir(o)) == sorted(os.path.basename(r) for r in want)
        for rel, text in want.items():
            with open(os.path.join(o, os.path.basename(rel))) as fh:
                assert fh.read() == text
        assert report[names.index(n)][0] == 60


# ---- the writer ---------------------------------------------------------------------------------------------------------
def reference_document(values, kind):
    if kind == 0:
        return json.dumps({'version': 1.3, 'people': []})
    kp = np.array(values, dtype=np.float64 if kind == 1 else np.int64).reshape(26, 3)
    return json.dumps({'version': 1.3, 'people': [{'person_id': [-1], 'pose_keypoints_2d': kp.flatten().tolist(), 'face_keypoints_2d': [],
                                                   'hand_left_keypoints_2d': [], 'hand_right_keypoints_2d': [], 'pose_keypoints_3d': [],
                                                   'face_keypoints_3d': [], 'hand_left_keypoints_3d': [], 'hand_right_keypoints_3d': []}]})


def test_writer_writes_json_dumps_text(tmp_path):
    from pose2sim_amd.ingest import write_person_files
    rng = np.random.default_rng(5)
    n = 300
    kind = rng.integers(0, 3, n).astype(np.int8)
    values = np.zeros((n, 78))
    special = np.array([-0.0, 1e22, 1e21, 1e16, 5e-324, 1.7976931348623157e308, 0.1, 1 / 3, 123456789.12345678, 1e-5, 9.999e-5, np.nan, np.inf, -np.inf])
    for i in range(n):
        if kind[i] == 2:
            values[i] = rng.integers(-2 ** 53, 2 ** 53, 78).astype(np.float64)
            values[i, :4] = [0, -1, 10000000000, -2.0 ** 63]
        else:
            values[i] = rng.normal(0, 1, 78) * 10.0 ** rng.integers(-12, 14, 78)
            where = rng.random(78) < 0.3
            values[i, where] = rng.choice(special, int(where.sum()))
    paths = [os.path.join(str(tmp_path), f'{i:03d}.json') for i in range(n)]
    assert write_person_files(paths, values, kind).all()
    for i in range(n):
        with open(paths[i], newline='') as fh:
            assert fh.read() == reference_document(values[i], kind[i]), i
    missing = os.path.join(str(tmp_path), 'no', 'such', 'folder.json')
    assert list(write_person_files([paths[0], missing], values[:2], [0, 0])) == [True, False]


@pytest.mark.parametrize('value', [0.5, 2.0 ** 63, -2.0 ** 64, np.nan, np.inf])
def test_writer_refuses_what_is_no_int64(tmp_path, value):
    from pose2sim_amd.ingest import write_person_files
    values = np.zeros((2, 78))
    values[1, 77] = value
    paths = [os.path.join(str(tmp_path), 'a.json'), os.path.join(str(tmp_path), 'b.json')]
    with pytest.raises(_lib.P2sError, match='not an integer within int64'):
        write_person_files(paths, values, [1, 2])
    assert not os.path.exists(paths[0])                              # refused before anything is written
    with pytest.raises(_lib.P2sError):
        write_person_files(paths, values, [1, 3])


# ---- the parser's flags ---------------------------------------------------------------------------------------------------
def flags_of(tmp_path, lists):
    from pose2sim_amd.ingest import JsonBatch
    path = os.path.join(str(tmp_path), 'flags.json')
    with open(path, 'w') as fh:
        fh.write('{"people": [' + ', '.join('{"pose_keypoints_2d": [' + text + ']}' for text in lists) + ']}')
    with JsonBatch([path]) as batch:
        return batch.person_flags().tolist(), batch.person_lengths.tolist()


def test_integer_token_flag(tmp_path):
    L = _lib
    flags, lengths = flags_of(tmp_path, ['1', '1.0', '1e0', '-0', '10000000000', '1, 2, 3.0', '1, NaN', '1, Infinity', '-Infinity, 2', '',
                                         '9007199254740992', '9007199254740993', '1, 99999999999999999999, 2', '1, null', '1, true', '1, "a"', '1, [2]',
                                         '1.5, 99999999999999999999'])
    ints = [bool(f & L.P2S_JSON_PERSON_ALL_INTS) for f in flags]
    assert ints == [True, False, False, True, True, False, False, False, False, False, True, True, True, False, False, False, False, False]
    big = [bool(f & L.P2S_JSON_PERSON_BIG_INT) for f in flags]
    assert big == [False] * 11 + [True, True, False, False, False, False, True]    # an integer token, whatever stands beside it
    assert flags[13] & L.P2S_JSON_PERSON_HAS_NULL and flags[14] & L.P2S_JSON_PERSON_HAS_BOOL
    assert lengths[15] == L.P2S_JSON_PERSON_NOT_NUMERIC and lengths[16] == L.P2S_JSON_PERSON_NOT_NUMERIC


def test_person_shape_flags(tmp_path):
    from pose2sim_amd.ingest import JsonBatch
    path = os.path.join(str(tmp_path), 'shapes.json')
    with open(path, 'w') as fh:
        fh.write('{"people": [7, {"pose_keypoints_2d": 3}, {}, {"pose_keypoints_2d": [1]}]}')
    with JsonBatch([path]) as batch:
        flags = batch.person_flags().tolist()
    L = _lib
    assert flags == [L.P2S_JSON_PERSON_NOT_OBJECT, L.P2S_JSON_PERSON_BAD_LIST, 0, L.P2S_JSON_PERSON_ALL_INTS]


# ---- refusals ---------------------------------------------------------------------------------------------------------------
GOOD = json.dumps({'people': [{'pose_keypoints_2d': [100.0 + k for k in range(78)]}]})


@pytest.mark.parametrize('numbers', ['"a", ' * 77 + '1', '1, ' * 77 + 'null', '1, ' * 77 + 'true', '1, ' * 77 + '[1]', '1, ' * 77 + '99999999999999999999',
                                     '1, ' * 77 + '9007199254740993', 'null'])
def test_lists_outside_the_contract_raise_and_write_nothing(tmp_path, numbers):
    cam, out = os.path.join(str(tmp_path), 'cam'), os.path.join(str(tmp_path), 'out')
    os.makedirs(cam), os.makedirs(out)
    for i, text in enumerate((GOOD, '{"people": [{"pose_keypoints_2d": [' + numbers + ']}]}', GOOD)):
        with open(os.path.join(cam, f'{i:03d}.json'), 'w') as fh:
            fh.write(text)
    with pytest.raises(ValueError, match='001.json'):
        pe.process(cam, out, engine=en.NumpyExtractEngine())
    assert os.listdir(out) == []


def test_other_exceptions_of_open_and_load_propagate(tmp_path):
    cam, out = os.path.join(str(tmp_path), 'cam'), os.path.join(str(tmp_path), 'out')
    os.makedirs(cam), os.makedirs(out)
    for i, data in enumerate((GOOD.encode(), b'{"people": "\xff"}', GOOD.encode())):
        with open(os.path.join(cam, f'{i:03d}.json'), 'wb') as fh:
            fh.write(data)
    with pytest.raises(UnicodeDecodeError):
        pe.process(cam, out, engine=en.NumpyExtractEngine())
    assert os.listdir(out) == ['000.json']


def test_main_parses_the_reference_options(monkeypatch, tmp_path):
    seen = []
    monkeypatch.setattr(pe, 'process', lambda i, o: seen.append((i, o)))
    cam = os.path.join(str(tmp_path), 'cam_json')
    os.makedirs(cam)
    monkeypatch.setattr('sys.argv', ['pose_extract_person', '--input', cam + '/', '--output', os.path.join(str(tmp_path), 'a', 'b')])
    pe.main()
    monkeypatch.setattr('sys.argv', ['pose_extract_person', '-i', cam + '//'])
    pe.main()
    assert seen == [(cam + '/', os.path.join(str(tmp_path), 'a', 'b')), (cam + '//', cam + '_person')]
    assert os.path.isdir(os.path.join(str(tmp_path), 'a', 'b')) and os.path.isdir(cam + '_person')
    monkeypatch.setattr('sys.argv', ['pose_extract_person'])
    with pytest.raises(SystemExit):
        pe.main()


def test_engine_without_the_entries_refuses():
    from pose2sim_amd.engine import Engine
    from pose2sim_amd.ingest import JsonBatch

    class Old:
        pass
    eng = Engine.__new__(Engine)
    eng._lib, eng._h = Old(), None
    with pytest.raises(NotImplementedError):
        eng.track_select([(np.zeros((1, 26, 3)), [0, 1])])
    with pytest.raises(NotImplementedError):
        eng.track_select_kernel_ms()
    batch = JsonBatch.__new__(JsonBatch)
    batch._lib, batch._h, batch.n_files, batch.person_base = Old(), None, 0, np.zeros(1, dtype=np.int64)
    with pytest.raises(NotImplementedError):
        batch.person_flags()
    assert {'p2s_track_select_host', 'p2s_track_select_kernel_ms', 'p2s_json_person_flags', 'p2s_write_person_files'} <= _lib.OPTIONAL


def test_no_gpu_means_the_utility_raises(gold, tmp_path):
    """There is no CPU fallback: with the default engine and no GPU the utility raises before it writes."""
    if _lib.device_count() > 0:
        return                                                       # covered by tests/test_extract_gpu.py
    call = lay_out(gold, 'one_file', str(tmp_path))
    out = os.path.join(str(tmp_path), call['output'])
    with pytest.raises(_lib.P2sError):
        pe.process(os.path.join(str(tmp_path), call['input']), out)
    assert os.listdir(out) == []
