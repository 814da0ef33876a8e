"""The reprojection utility without a GPU: the NumPy restatement (tests/reproj_numpy.py) against the goldens recorded from
the reference (tests/golden/reproj_units.npz), pose2sim_amd.reproj_from_trc_calib on that restatement against the recorded
files, the refusals, and the native OpenPose writer (host code) against json.dumps."""
import hashlib
import json
import os

import numpy as np
import pandas as pd
import pytest

import reproj_numpy as rn
from pose2sim_amd import reproj_from_trc_calib as rp

RAW_TOL = 1e-9          # px: the project's bar for float64 kernels


@pytest.fixture(scope='module')
def gold(golden_dir):
    return np.load(os.path.join(golden_dir, 'reproj_units.npz'))


def case_names(gold):
    return json.loads(str(gold['cases']))


def all_case_names():
    return case_names(np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'reproj_units.npz')))


ALL = all_case_names()
ARRAY_CASES = [n for n in ALL if n not in ('error_no_format', 'error_no_format_markerset', 'error_ragged_frames')]
assert len(ALL) == 22 and len(ARRAY_CASES) == 19


def lay_out(gold, name, work):
    """Write the case's inputs into `work` -> the utility's keyword arguments."""
    for rel in json.loads(str(gold[f'{name}__premade'])):
        os.makedirs(os.path.join(work, rel))
    trc_path, toml_path = os.path.join(work, str(gold[f'{name}__trc_name'])), os.path.join(work, 'Calib.toml')
    with open(trc_path, 'w') as fh:
        fh.write(str(gold[f'{name}__trc']))
    with open(toml_path, 'w') as fh:
        fh.write(str(gold[f'{name}__toml']))
    args = json.loads(str(gold[f'{name}__args']))
    if args.get('output_file_root'):
        args['output_file_root'] = os.path.join(work, args['output_file_root'])
        os.makedirs(os.path.dirname(args['output_file_root']))
    return {'input_trc_file': trc_path, 'input_calib_file': toml_path, 'openpose': False, 'deeplabcut': False, 'mmpose': False,
            'markerset': None, 'undistort_points': False, 'output_file_root': None, **args}


def engine_inputs(gold, name, work):
    """The arrays the utility hands to Engine.reproject for this case: (Q, keyword arguments)."""
    kw = lay_out(gold, name, work)
    _, _, Q = rp.read_markers(kw['input_trc_file'])
    cams = rp.read_cameras(kw['input_calib_file'])
    P, _ = rp.projection_matrices(cams)
    sizes = np.array([c['S'] for c in cams])
    F = len(Q) if P.shape[1] == 1 else min(P.shape[1], len(Q))
    if kw['undistort_points']:
        cal = {'K': [c['K'] for c in cams], 'dist': [c['dist'] for c in cams], 'T': [c['T'] for c in cams],
               'R_mat': [rp.cvmath.rodrigues(c['R']) for c in cams]}
        return Q[:F], {'cal': cal, 'sizes': sizes}
    return Q[:F], {'P': P[:, :F], 'sizes': sizes}


def check_arrays(gold, name, uv, uv_raw):
    raw, table = gold[f'{name}__raw'], gold[f'{name}__table']
    assert uv_raw.shape == raw.shape and uv.shape == table.shape
    finite = np.isfinite(raw)
    assert np.array_equal(np.isfinite(uv_raw), finite)
    worst = float(np.abs(uv_raw[finite] - raw[finite]).max()) if finite.any() else 0.0
    print(f'{name}: {finite.sum()} values, worst |raw - reference| = {worst:.3e} px')
    assert worst <= RAW_TOL
    assert np.array_equal(np.isnan(uv), np.isnan(table)), 'NaN pattern of the rounded table'
    keep = ~np.isnan(table)
    assert np.array_equal(uv[keep], table[keep])
    assert np.array_equal(np.signbit(uv[keep]), np.signbit(table[keep])), 'negative zero'
    return worst


def relocate(text, old, new):
    return text.replace(old, new)


def mmpose_expected(text, old_dir, new_dir):
    """The recorded MMPose document moved to new_dir: names substituted, ids recomputed from them by the md5 rule."""
    doc = json.loads(text)
    ids = {}
    for img in doc['images']:
        img['file_name'] = relocate(img['file_name'], old_dir, new_dir)
        ids[img['id']] = int(hashlib.md5(img['file_name'].encode()).hexdigest(), 16) % 10 ** 12
        img['id'] = ids[img['id']]
    names = {img['id']: img['file_name'] for img in doc['images']}
    for ann in doc['annotations']:
        ann['image_id'] = ids[ann['image_id']]
        ann['id'] = int(hashlib.md5(('person0' + names[ann['image_id']]).encode()).hexdigest(), 16) % 10 ** 12
    return doc


def same_json(a, b):
    """Equal as parsed JSON, ints and floats kept apart and floats compared exactly."""
    if type(a) is not type(b):
        return False
    if isinstance(a, dict):
        return list(a) == list(b) and all(same_json(a[k], b[k]) for k in a)
    if isinstance(a, list):
        return len(a) == len(b) and all(same_json(x, y) for x, y in zip(a, b))
    return a == b


def run_case(gold, name, work, engine, capsys, monkeypatch):
    """The utility on `engine` in `work`, DataFrame.to_hdf switched off as in the recording; compares folders, files, what
    was printed and, for the error cases, the exception's type and message with the recording."""
    kw = lay_out(gold, name, work)
    monkeypatch.setattr(pd.DataFrame, 'to_hdf', lambda self, *a, **k: None)
    before = {os.path.join(r, f) for r, _, fs in os.walk(work) for f in fs}
    error = json.loads(str(gold[f'{name}__error']))
    capsys.readouterr()
    if error is None:
        rp.reproj_from_trc_calib_func(engine=engine, **kw)
    else:
        with pytest.raises(Exception) as info:
            rp.reproj_from_trc_calib_func(engine=engine, **kw)
        old_dir = os.path.join(str(gold['work_root']), name)
        assert [type(info.value).__name__, str(info.value)] == [error[0], relocate(error[1], old_dir, work)]
    old_dir = os.path.join(str(gold['work_root']), name)
    assert capsys.readouterr().out == relocate(str(gold[f'{name}__printed']), old_dir, work)
    expected = json.loads(str(gold[f'{name}__files']))
    found, folders = {}, []
    for r, ds, fs in os.walk(work):
        folders += [os.path.relpath(os.path.join(r, x), work) for x in ds]
        found.update({os.path.relpath(os.path.join(r, f), work): os.path.join(r, f) for f in fs if os.path.join(r, f) not in before})
    assert sorted(folders) == json.loads(str(gold[f'{name}__folders']))
    assert sorted(found) == sorted(expected)
    for rel, text in expected.items():
        with open(found[rel], 'rb') as fh:
            got = fh.read()
        if rel.endswith('_mmpose.json'):
            assert same_json(json.loads(got), mmpose_expected(text, old_dir, work)), rel
        elif rel.endswith('.csv'):
            assert got == relocate(text, old_dir, work).encode(), rel
        else:
            assert got == text.encode(), rel
    return error


@pytest.mark.parametrize('name', ARRAY_CASES)
def test_numpy_restatement_reproduces_the_reference(gold, tmp_path, name, capsys):
    Q, kw = engine_inputs(gold, name, str(tmp_path))
    uv, uv_raw = rn.reproject(Q, raw=True, **kw)
    with capsys.disabled():
        check_arrays(gold, name, uv, uv_raw)


def test_fixture_holds_no_rounding_tie(gold):
    """What makes element-for-element equality of the rounded tables a fair demand on a kernel with reordered sums."""
    n = 0
    for name in ARRAY_CASES:
        raw = gold[f'{name}__raw']
        t = raw[np.isfinite(raw)] * 10
        assert (np.abs(t - np.floor(t) - 0.5) > 1e-6).all(), name
        n += t.size
    assert n > 10000


def test_border_markers_sit_on_both_sides_of_every_border(gold):
    """static4 plants markers a few hundredths of a pixel either side of the borders of camera 1: the mask is taken on the
    rounded values, so -0.04 stays (as -0.0) and width - 0.04 goes."""
    raw, table = gold['static4__raw'][0, 0], gold['static4__table'][0, 0]
    tags = dict(zip(('L_in', 'L_out', 'R_out', 'R_in', 'T_in', 'T_out', 'B_out', 'B_in'), range(28, 36)))
    for tag, k in tags.items():
        assert np.isnan(table[k]).all() == tag.endswith('_out'), (tag, raw[k], table[k])
    assert table[tags['L_in'], 0] == 0 and np.signbit(table[tags['L_in'], 0])
    assert raw[tags['R_out'], 0] < 1920 and raw[tags['L_in'], 0] < 0


@pytest.mark.parametrize('name', ALL)
def test_utility_writes_the_recorded_files(gold, tmp_path, name, capsys, monkeypatch):
    error = run_case(gold, name, str(tmp_path), rn.NumpyReprojEngine(), capsys, monkeypatch)
    if name.startswith('error_no_format'):
        assert error[1] == rp.NO_FORMAT


def test_no_format_raises_the_recorded_message(gold, tmp_path):
    error = json.loads(str(gold['error_no_format__error']))
    with pytest.raises(ValueError) as info:
        rp.reproj_from_trc_calib_func(engine=rn.NumpyReprojEngine(), **lay_out(gold, 'error_no_format', str(tmp_path)))
    assert [type(info.value).__name__, str(info.value)] == error


@pytest.mark.parametrize('markerset', rp.NAMED_MARKERSETS)
def test_named_markersets_are_refused(gold, tmp_path, markerset):
    kw = lay_out(gold, 'static2', str(tmp_path))
    with pytest.raises(NotImplementedError, match='markerset'):
        rp.reproj_from_trc_calib_func(engine=rn.NumpyReprojEngine(), **{**kw, 'markerset': markerset})
    assert not os.path.exists(os.path.join(str(tmp_path), 'trial_reproj'))


@pytest.mark.parametrize('name', ['zooming', 'moving', 'zooming_moving'])
def test_distortion_with_per_frame_cameras_is_refused(gold, tmp_path, name):
    kw = lay_out(gold, name, str(tmp_path))
    with pytest.raises(NotImplementedError, match='static cameras'):
        rp.reproj_from_trc_calib_func(engine=rn.NumpyReprojEngine(), **{**kw, 'undistort_points': True})


def rewrite_trc(path, edit):
    with open(path) as fh:
        lines = fh.read().split('\n')
    edit(lines)
    with open(path, 'w') as fh:
        fh.write('\n'.join(lines))


def test_marker_count_that_disagrees_with_the_label_row_is_refused(gold, tmp_path):
    kw = lay_out(gold, 'static2', str(tmp_path))

    def fewer(lines):
        facts = lines[2].split('\t')
        facts[3] = '20'
        lines[2] = '\t'.join(facts)
    rewrite_trc(kw['input_trc_file'], fewer)
    with pytest.raises(ValueError, match='NumMarkers is 20 but the label row names 26 markers'):
        rp.reproj_from_trc_calib_func(engine=rn.NumpyReprojEngine(), **kw)


def test_marker_named_twice_is_refused(gold, tmp_path):
    kw = lay_out(gold, 'static2', str(tmp_path))
    rewrite_trc(kw['input_trc_file'], lambda lines: lines.__setitem__(3, lines[3].replace('M05', 'M04')))
    with pytest.raises(NotImplementedError, match='names a marker twice'):
        rp.reproj_from_trc_calib_func(engine=rn.NumpyReprojEngine(), **kw)


def test_deeplabcut_without_pytables_ends_before_any_csv(gold, tmp_path):
    """DataFrame.to_hdf comes first, as in the reference: without pytables pandas raises ImportError and no csv exists."""
    import importlib.util
    kw = {**lay_out(gold, 'static2', str(tmp_path)), 'deeplabcut': True}
    csvs = lambda: [f for _, _, fs in os.walk(str(tmp_path)) for f in fs if f.endswith('.csv')]     # noqa: E731
    if importlib.util.find_spec('tables') is None:
        with pytest.raises(ImportError):
            rp.reproj_from_trc_calib_func(engine=rn.NumpyReprojEngine(), **kw)
        assert not csvs()
    else:
        rp.reproj_from_trc_calib_func(engine=rn.NumpyReprojEngine(), **kw)
        assert len(csvs()) == 2


def test_main_parses_the_reference_options(gold, tmp_path, monkeypatch):
    kw = lay_out(gold, 'static2', str(tmp_path))
    seen = {}
    monkeypatch.setattr(rp, 'reproj_from_trc_calib_func', lambda **a: seen.update(a))
    monkeypatch.setattr('sys.argv', ['reproj_from_trc_calib', '-t', kw['input_trc_file'], '-c', kw['input_calib_file'], '-o', '-d', '-m',
                                     '-u', '-s', 'custom', '-O', 'out'])
    rp.main()
    assert seen == {'input_trc_file': kw['input_trc_file'], 'input_calib_file': kw['input_calib_file'], 'openpose': True,
                    'deeplabcut': True, 'mmpose': True, 'undistort_points': True, 'markerset': 'custom', 'output_file_root': 'out'}


def test_engine_without_the_entry_refuses(monkeypatch):
    """An Engine whose library lacks p2s_reproject_host raises NotImplementedError, as gcv_spline does."""
    from pose2sim_amd.engine import Engine

    class Old:
        pass
    eng = Engine.__new__(Engine)
    eng._lib, eng._h = Old(), None
    with pytest.raises(NotImplementedError, match='p2s_reproject_host'):
        eng.reproject(np.zeros((1, 1, 3)), P=np.zeros((1, 1, 3, 4)), sizes=np.ones((1, 2)))


# ---- the native OpenPose writer: host code, runs without a GPU ---------------------------------------------------------------
def native_files(tmp_path, uv, marker_index=None, root='t', n_threads=0):
    from pose2sim_amd.engine import write_openpose_files
    dirs = [os.path.join(str(tmp_path), f'cam{c + 1:02d}_json') for c in range(uv.shape[0])]
    for d in dirs:
        os.mkdir(d)
    assert write_openpose_files(dirs, root, uv, marker_index, n_threads) == uv.shape[0] * uv.shape[1]
    for c, d in enumerate(dirs):
        assert sorted(os.listdir(d)) == [f'{root}_cam{c + 1:02d}_openpose_{f:04d}.json' for f in range(uv.shape[1])]
        for f in range(uv.shape[1]):
            with open(os.path.join(d, f'{root}_cam{c + 1:02d}_openpose_{f:04d}.json'), 'rb') as fh:
                yield c, f, fh.read()


@pytest.mark.parametrize('name', ['static4', 'distorted8', 'one_marker', 'one_frame'])
def test_native_openpose_writer_on_the_golden_tables(gold, tmp_path, name):
    uv = gold[f'{name}__table']
    idx = range(uv.shape[2])
    for c, f, got in native_files(tmp_path, uv):
        assert got == rn.openpose_text(uv[c, f], idx).encode()


def test_native_openpose_writer_on_seeded_tables(tmp_path):
    rng = np.random.default_rng(77)
    uv = np.round(rng.uniform(-5, 1925, (3, 150, 17, 2)), 1)
    uv[rng.random(uv.shape[:3]) < 0.15] = np.nan
    uv[0, 0, 1, 0] = np.nan                                      # x alone missing
    uv[0, 0, 2, 1] = np.nan                                      # y alone missing
    uv[1, 3] = np.nan                                            # a frame without a marker
    uv[2, 0, :6] = [[0.0, 100.0], [1919.9, -0.0], [-0.0, -0.0], [0.1, 1e-5], [1e16, 123456.7], [1e-4, 5e-324]]
    order = rng.permutation(17)[:11].astype(np.int32)
    for c, f, got in native_files(tmp_path, uv, order, root='a b.c', n_threads=5):
        assert got == rn.openpose_text(uv[c, f], order).encode()
        assert json.loads(got)['people'][0]['person_id'] == [-1]


def test_native_openpose_writer_reports_a_missing_folder(tmp_path):
    from pose2sim_amd.engine import P2sError, write_openpose_files
    os.mkdir(os.path.join(str(tmp_path), 'a'))
    with pytest.raises(P2sError, match='cannot write'):
        write_openpose_files([os.path.join(str(tmp_path), 'a'), os.path.join(str(tmp_path), 'missing')], 'r', np.zeros((2, 3, 2, 2)))
    assert len(os.listdir(os.path.join(str(tmp_path), 'a'))) == 3
    with pytest.raises(P2sError, match='names marker'):
        write_openpose_files([os.path.join(str(tmp_path), 'a')], 'r', np.zeros((1, 3, 2, 2)), [0, 2])


# ---- closed loop with the triangulation: the tolerance of the GPU test is derived here, on the CPU ---------------------------
LIK_THR, ERR_THR, MIN_CAMS = 0.3, 15.0, 2
# Worst |reported error - mean pixel distance to the reprojection of the reported point| found on the CPU between
# oracle/triangulation_ref.py and reproj_numpy on the workloads below: with the oracle's float64 error, and with that error
# rounded to float32, the type Engine.triangulate reports it in (errors reach the 15 px threshold; 15 x 2^-24 = 8.9e-7).
# The GPU test (test_reproj_gpu.py) allows ten times the second figure, for reordered float64 sums and fused multiply-adds.
CLOSED_LOOP_CPU_WORST_F64 = 1.1e-13
CLOSED_LOOP_CPU_WORST_F32 = 4.76e-7


def closed_loop_workload(C, F, seed):
    from pose2sim_amd import synth
    return synth.make_config(F, C, 26, 1, seed=seed, p_lowlik=0.1, p_outlier=0.08)


def closed_loop_mean_distance(xyl, mask, uv_raw, lik_thr=LIK_THR):
    """xyl [B][C][K][3] float32, mask [B][K] excluded-camera bits, uv_raw [C][B][K][2] -> [B][K]: the unweighted mean over the
    kept cameras (likelihood at or above the threshold and not 0, not excluded) of the pixel distance between the
    observation and the projection (oracle/triangulation_ref.py:63-67, 127)."""
    obs = np.asarray(xyl, dtype=np.float64)
    proj = np.transpose(uv_raw, (1, 0, 2, 3))
    bits = (np.asarray(mask, dtype=np.uint32)[:, None, :] >> np.arange(obs.shape[1], dtype=np.uint32)[None, :, None]) & 1
    with np.errstate(invalid='ignore'):
        kept = (obs[..., 2] >= lik_thr) & (obs[..., 2] != 0) & (bits == 0)
        d = np.sqrt((obs[..., 0] - proj[..., 0]) ** 2 + (obs[..., 1] - proj[..., 1]) ** 2)
        return np.where(kept, d, 0.0).sum(axis=1) / kept.sum(axis=1)


@pytest.mark.parametrize('C,F', [(4, 12), (8, 8), (16, 3)])
def test_closed_loop_tolerance_is_derived_on_the_cpu(C, F, capsys):
    from oracle import triangulation_ref as tr
    wl = closed_loop_workload(C, F, seed=100 + C)
    Q, err, _, mask = tr.triangulate_batch(wl['xyl'], wl['P'], None, list(range(26)), LIK_THR, ERR_THR, MIN_CAMS)
    xyl, Q, err, mask = wl['xyl'].reshape(F, C, 26, 3), Q.reshape(F, 26, 3), err.reshape(F, 26), mask.reshape(F, 26)
    uv_raw = rn.project_plain(Q, np.array(wl['P']))
    mine = closed_loop_mean_distance(xyl, mask, uv_raw)
    ok = ~np.isnan(err)
    assert ok.sum() > 0.8 * ok.size
    d64 = float(np.abs(mine[ok] - err[ok]).max())
    d32 = float(np.abs(mine[ok] - err[ok].astype(np.float32).astype(np.float64)).max())
    with capsys.disabled():
        print(f'closed loop on the CPU, {C} cameras, {ok.sum()} units: worst difference {d64:.3e} px (float64 error), '
              f'{d32:.3e} px (error rounded to float32)')
    # the recorded worst cases, with room for another BLAS build's summation order
    assert d64 <= 2 * CLOSED_LOOP_CPU_WORST_F64 and d32 <= 1.01 * CLOSED_LOOP_CPU_WORST_F32
