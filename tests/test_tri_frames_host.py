"""Per-frame calibrations without a GPU: the reader that the reprojection utility and triangulation share, against the
calibrations and pixels recorded from the reference (tests/golden/reproj_units.npz), mixed and ragged rigs, and the
refusals of the stages that take static cameras only."""
import ctypes as C
import os
import re
import sys

import numpy as np
import pytest

import moving_rig

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden'))
import e2e_common as ec  # noqa: E402

from pose2sim_amd import _lib, calib, personAssociation, synth, triangulation  # noqa: E402
from pose2sim_amd import reproj_from_trc_calib as rp  # noqa: E402

RECORDED = ['zooming', 'moving', 'zooming_moving']
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_entry_points_are_declared_exported_and_bound():
    """include/p2s_tri_frames.h against the library and against _lib's table of it, as tests/test_lib_abi.py holds include/p2s.h."""
    import __graft_entry__ as entry
    entry.build_hip()
    txt = open(os.path.join(ROOT, 'include', 'p2s_tri_frames.h')).read()
    syms = set(re.findall(r'\b(p2s_[a-z_0-9]+)\s*\(', re.sub(r'/\*.*?\*/', '', txt, flags=re.S)))
    assert syms == {'p2s_triangulate_frames_host', 'p2s_triangulate_frames_device'} == set(_lib.TRI_FRAMES_SIGNATURES) and syms <= _lib.OPTIONAL
    assert not syms & (set(_lib.SIGNATURES) | set(_lib.FLOOR_SIGNATURES))
    lib = C.CDLL(_lib.LIB_PATH)
    assert all(hasattr(lib, name) for name in syms)
    bound = _lib.load()
    for name in syms:
        assert getattr(bound, name).argtypes == _lib.TRI_FRAMES_SIGNATURES[name][1]
    # the two calls take the same operands, and as many as the header declares
    for name in syms:
        declared = re.search(name + r'\s*\((.*?)\);', re.sub(r'/\*.*?\*/', '', txt, flags=re.S), flags=re.S).group(1)
        assert len(declared.split(',')) == len(_lib.TRI_FRAMES_SIGNATURES[name][1]) == 14
    assert 'p2s_tri_frames.hip' in entry.HIP_SOURCES


@pytest.fixture(scope='module')
def gold(golden_dir):
    return np.load(os.path.join(golden_dir, 'reproj_units.npz'))


def write_case(gold, name, folder):
    toml_path, trc_path = os.path.join(folder, 'Calib.toml'), os.path.join(folder, str(gold[f'{name}__trc_name']))
    with open(toml_path, 'w') as fh:
        fh.write(str(gold[f'{name}__toml']))
    with open(trc_path, 'w') as fh:
        fh.write(str(gold[f'{name}__trc']))
    return toml_path, trc_path


@pytest.mark.parametrize('name', RECORDED)
def test_shared_reader_on_the_recorded_calibrations(gold, tmp_path, name):
    """calib.frame_projections gives the utility's matrices, frame-major, and they project the .trc onto the recorded pixels."""
    toml_path, trc_path = write_case(gold, name, str(tmp_path))
    assert calib.is_per_frame(toml_path)
    P, cams = calib.frame_projections(toml_path)
    P_util, per_frame = rp.projection_matrices(rp.read_cameras(toml_path))
    assert per_frame and P.shape == (P_util.shape[1], P_util.shape[0], 3, 4)
    assert np.array_equal(P, P_util.transpose(1, 0, 2, 3))
    assert len(cams) == P.shape[1]
    _, _, Q = rp.read_markers(trc_path)
    raw = gold[f'{name}__raw']                                              # [C][F][K][2]
    F = raw.shape[1]
    h = np.einsum('fcij,fkj->cfki', P[:F], np.concatenate([Q[:F], np.ones(Q[:F].shape[:2] + (1,))], axis=-1))
    assert np.abs(h[..., :2] / h[..., 2:3] - raw).max() <= 1e-9


def static_toml(path, C=4, seed=3):
    cams = synth.make_cameras(C, seed=seed)
    calib.write_calibration_toml(path, cams)
    return cams


def test_static_file_is_not_per_frame(tmp_path):
    path = str(tmp_path / 'Calib.toml')
    cams = static_toml(path)
    assert not calib.is_per_frame(path)
    assert triangulation.load_frame_calibration(path, False, False) is None
    P, _ = calib.frame_projections(path)                                    # one frame, the static matrices
    assert P.shape == (1, 4, 3, 4) and np.allclose(P[0], np.array(calib.computeP(path)), rtol=0, atol=1e-9)
    assert len(calib.retrieve_calib_params(path)['K']) == len(cams['K'])


def test_mixed_rig_broadcasts_its_static_cameras(tmp_path):
    path = str(tmp_path / 'Calib.toml')
    rig = moving_rig.make_rig(4, 9, seed=2, static=(1, 3))
    moving_rig.write_toml(path, rig)
    assert calib.is_per_frame(path)
    P, cams = calib.frame_projections(path)
    assert P.shape == (9, 4, 3, 4)
    assert np.abs(P - rig['P']).max() < 1e-8                                 # through the Rodrigues vector and back
    for c in (1, 3):
        assert cams[c]['K'].ndim == 2 and all(np.array_equal(P[f, c], P[0, c]) for f in range(9))
    for c in (0, 2):
        assert cams[c]['K'].ndim == 3 and not np.array_equal(P[1, c], P[0, c])
    # the utility keeps the reference's behaviour on such a file: NumPy's refusal of the ragged list
    with pytest.raises(ValueError):
        rp.projection_matrices(rp.read_cameras(path))


def test_ragged_frame_counts_are_refused(tmp_path, gold):
    path = str(tmp_path / 'Calib.toml')
    moving_rig.write_toml(path, moving_rig.make_rig(3, 8, seed=2), frames={2: 5})
    with pytest.raises(ValueError, match=r'different numbers of calibration frames: \[5, 8\]'):
        calib.frame_projections(path)
    with open(path, 'w') as fh:
        fh.write(str(gold['error_ragged_frames__toml']))
    with pytest.raises(ValueError, match='different numbers of calibration frames'):
        calib.frame_projections(path)


def test_triangulation_skips_the_four_table_names(tmp_path):
    """calib.camera_keys picks the tables for triangulation; the utility skips 'metadata' alone."""
    path = str(tmp_path / 'Calib.toml')
    moving_rig.write_toml(path, moving_rig.make_rig(3, 4, seed=2))
    with open(path, 'a') as fh:
        fh.write('\n[capture_volume]\nsize = [ 1.0, 2.0]\n')
    assert calib.frame_projections(path)[0].shape == (4, 3, 3, 4)
    with pytest.raises(KeyError):
        rp.read_cameras(path)


def session(tmp_path, n_cal_frames, n_files, C=4, **tri):
    """A session whose Calib.toml holds n_cal_frames frames of a moving rig and whose pose folders hold n_files frames."""
    os.makedirs(str(tmp_path), exist_ok=True)
    root = str(tmp_path / 'session')
    toml_path = str(tmp_path / 'rig.toml')
    moving_rig.write_toml(toml_path, moving_rig.make_rig(C, n_cal_frames, seed=4))
    people = [[[np.zeros(26 * 3)] for _ in range(C)] for _ in range(n_files)]
    trial = ec.write_trial(root, 'trial', None, people, calib_text=open(toml_path).read())
    return ec.base_config(trial, False, **tri)


def test_static_only_entry_points_refuse_in_words(tmp_path):
    cfg = session(tmp_path, 6, 6)
    toml_path = calib.find_calibration_file(os.path.dirname(cfg['project']['project_dir']))
    for fn in (calib.computeP, calib.retrieve_calib_params):
        with pytest.raises(NotImplementedError, match='per-frame cameras'):
            fn(toml_path)
    for multi_person in (False, True):
        cfg['project']['multi_person'] = multi_person
        with pytest.raises(NotImplementedError, match='per-frame cameras'):
            personAssociation.associate_all(cfg)


def test_short_calibration_is_refused_before_any_device_work(tmp_path, monkeypatch):
    cfg = session(tmp_path, 10, 12)
    monkeypatch.setattr(triangulation, '_make_engine', lambda: pytest.fail('an engine was asked for'))
    with pytest.raises(ValueError, match=r'ends at frame 12 but the calibration holds 10 frames'):
        triangulation.triangulate_all(cfg)
    cfg['project']['frame_range'] = [3, 11]
    with pytest.raises(ValueError, match=r'ends at frame 11 but the calibration holds 10 frames'):
        triangulation.triangulate_all(cfg)


def test_options_that_take_static_cameras_only(tmp_path, monkeypatch):
    monkeypatch.setattr(triangulation, '_make_engine', lambda: pytest.fail('an engine was asked for'))
    with pytest.raises(NotImplementedError, match='undistort_points with moving or zooming cameras') as distort:
        triangulation.triangulate_all(session(tmp_path / 'a', 6, 6, undistort_points=True))
    assert str(distort.value) == calib.UNDISTORT_PER_FRAME                    # the utility's words
    with pytest.raises(NotImplementedError, match='handle_LR_swap with moving or zooming cameras'):
        triangulation.triangulate_all(session(tmp_path / 'b', 6, 6, handle_LR_swap=True))
    monkeypatch.setattr(triangulation.parallel, 'dist_info', lambda: (1, 2))
    with pytest.raises(NotImplementedError, match='more than one rank'):
        triangulation.triangulate_all(session(tmp_path / 'c', 6, 6))


def test_the_utility_refuses_distortion_in_the_same_words(gold, tmp_path):
    toml_path, trc_path = write_case(gold, 'moving', str(tmp_path))
    with pytest.raises(NotImplementedError) as refusal:
        rp.reproj_from_trc_calib_func(engine=object(), input_trc_file=trc_path, input_calib_file=toml_path, openpose=True,
                                      undistort_points=True)
    assert str(refusal.value) == calib.UNDISTORT_PER_FRAME


def test_recap_factor_is_the_mean_over_the_frame_range(tmp_path):
    rig = moving_rig.make_rig(3, 12, seed=6)
    path = str(tmp_path / 'Calib.toml')
    moving_rig.write_toml(path, rig)
    first = calib.load_toml(path)[rig['names'][0]]
    per_frame = np.linalg.norm(rig['T'][:, 0], axis=1) / rig['K'][:, 0, 0, 0]
    assert per_frame.std() > 0.01 * per_frame.mean()                         # the rule matters on this rig
    for f_range in ([0, 12], [4, 9], [11, 12]):
        want = per_frame[f_range[0]:f_range[1]].mean()
        assert abs(triangulation.recap_px_to_m(first, f_range) - want) <= 1e-12 * want
    # a static camera: the present value, whatever the range
    static_toml(path)
    first = calib.load_toml(path)['cam01']
    want = float(np.sqrt(np.sum(np.array(first['translation']) ** 2))) / first['matrix'][0][0]
    assert triangulation.recap_px_to_m(first, [0, 500]) == want
    # zooming only: |T| is one number, fx one per frame
    zoom = {'translation': [0.0, 3.0, 4.0], 'matrix': [[[1000.0 * (f + 1), 0, 0], [0, 1000.0, 0], [0, 0, 1]] for f in range(4)]}
    assert triangulation.recap_px_to_m(zoom, [1, 3]) == pytest.approx(np.mean([5.0 / 2000.0, 5.0 / 3000.0]), rel=1e-15)
