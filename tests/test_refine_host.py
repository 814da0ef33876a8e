"""What of the extrinsics refinement needs no GPU: the oracle itself, the gauge, the library's host path (ctx == NULL runs the
kernels' per-point functions pass after pass), its refusals, the TOML round trip and the command line."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import refine_scipy as rs
import rigs
from pose2sim_amd import _lib, calib, calib_refine, cvmath, engine

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_entry_points_are_bound_as_optional():
    new = {'p2s_refine_extrinsics_host', 'p2s_refine_kernel_ms', 'p2s_refine_held_coord'}
    assert new <= _lib.OPTIONAL and new <= set(_lib.SIGNATURES)
    txt = open(os.path.join(ROOT, 'include', 'p2s.h')).read()
    defs = {m.group(1): int(m.group(2)) for m in re.finditer(r'#define\s+(P2S_REFINE_[A-Z_]+)\s+(\d+)', txt)}
    assert defs == {'P2S_REFINE_TILE': _lib.P2S_REFINE_TILE, 'P2S_REFINE_MAX_PARTS': _lib.P2S_REFINE_MAX_PARTS}
    assert C.sizeof(_lib.RefineParams) == 32 and C.sizeof(_lib.RefineReport) == 48 + 2 * 8 * _lib.P2S_MAX_CAMS


def test_oracle_recovers_the_true_cameras_at_zero_noise():
    cs = rs.make_case('ring', 3, seed=1, noise_px=0.0, p_outlier=0.0, lik=None)
    start = np.abs(rs.centres(cs['R0'], cs['t0']) - rs.centres(cs['R'], cs['t'])).max()
    R, t, X, cost, _ = rs.refine(cs['xyl'], cs['K'], cs['R0'], cs['t0'], cs['X0'])
    dc = np.abs(rs.centres(R, t) - rs.centres(cs['R'], cs['t'])).max()
    print(f'oracle at zero noise: centres {start:.3e} m -> {dc:.3e} m from the truth, cost {cost:.3e}')
    assert start > 1e-2 and dc <= rs.ZERO_NOISE_BOUND
    assert np.array_equal(R[0], cs['R'][0]) and np.array_equal(t[0], cs['t'][0]) and t[1][cs['held']] == cs['t'][1][cs['held']]


def test_gauge_takes_the_first_index_on_ties():
    eye = np.stack([np.eye(3), np.eye(3)])
    for t1, j in (((1.0, 1.0, 0.5), 0), ((0.5, 1.0, 1.0), 1), ((-1.0, 1.0, 1.0), 0), ((0.5, -1.0, 1.0), 1), ((1.0, 1.0, 1.0), 0),
                  ((0.0, 0.0, 2.0), 2), ((0.0, 0.0, 0.0), 0)):
        t = np.array([(0.0, 0.0, 0.0), t1])
        assert engine.refine_held_coord(eye, t) == j == rs.held_coord(eye, t), t1
    # the baseline counts, not camera 1's translation: both cameras 10 m from the origin along x, 1 m apart along y
    t = np.array([(10.0, 0.0, 0.0), (10.0, 1.0, 0.0)])
    assert engine.refine_held_coord(eye, t) == 1 == rs.held_coord(eye, t)
    with pytest.raises(_lib.P2sError, match='must be finite'):
        engine.refine_held_coord(eye, np.array([(0.0, 0.0, 0.0), (np.nan, 1.0, 1.0)]))


@pytest.mark.parametrize('family', ['ring', 'overhead', 'one_side', 'stadium'])
def test_gauge_is_invariant_to_rescaling_about_camera_0(family):
    cams = rigs.make_rig(family, 4, seed=2)
    R, t = np.array(cams['R_mat']), np.array(cams['T'])
    j = rs.held_coord(R, t)
    assert engine.refine_held_coord(R, t) == j
    c = rs.centres(R, t)
    for alpha in (1e-3, 0.25, 3.0, 1e3):
        cs = c[0] + alpha * (c - c[0])
        ts = -np.einsum('cij,cj->ci', R, cs)
        assert engine.refine_held_coord(R, ts) == j == rs.held_coord(R, ts), alpha


@pytest.mark.parametrize('family, C', [('ring', 4), ('stadium', 4), ('ring', 2)])
def test_host_path_against_the_oracle(family, C):
    """The per-point functions of the kernels, run by the library on the host, reach the oracle's minimum."""
    cs = rs.make_case(family, C, seed=C)
    Ro, to, Xo, co, _ = rs.refine(cs['xyl'], cs['K'], cs['R0'], cs['t0'], cs['X0'])
    R, t, X, rep = engine.refine_extrinsics_host(cs['xyl'], cs['K'], cs['R0'], cs['t0'], cs['X0'])
    rel = (rep['cost_after'] - co) / co
    dc = np.abs(rs.centres(R, t) - rs.centres(Ro, to)).max()
    dx = np.nanmax(np.abs(X.reshape(-1, 3) - Xo))
    print(f'{family} {C} on the host: cost {rep["cost_before"]:.6f} -> {rep["cost_after"]:.9f}, oracle {co:.9f}, relative difference {rel:.3e}; '
          f'centres within {dc:.3e} m, points within {dx:.3e} m; {rep["iterations"]} trials, {rep["accepted"]} accepted')
    assert abs(rel) <= rs.COST_REL_BOUND and dc <= rs.CENTRE_BOUND and dx <= rs.POINT_BOUND
    assert np.array_equal(np.isnan(X.reshape(-1, 3)), np.isnan(Xo))
    assert np.array_equal(R[0], cs['R0'][0]) and np.array_equal(t[0], cs['t0'][0]) and t[1][rep['held_coord']] == cs['t0'][1][rep['held_coord']]
    assert rep['held_coord'] == cs['held'] and rep['cost_after'] <= rep['cost_before']
    # the cost it reports is the contract's, by the oracle's own cost function at the returned cameras and points
    assert abs(rs.cost(cs['xyl'], cs['K'], R, t, X, X0=cs['X0']) - rep['cost_after']) <= 1e-12 * co
    again = engine.refine_extrinsics_host(cs['xyl'], cs['K'], cs['R0'], cs['t0'], cs['X0'])
    assert all(a.tobytes() == b.tobytes() for a, b in zip((R, t, X), again[:3]))


def test_refusals_without_a_device():
    cs = rs.make_case('ring', 3, seed=0)

    def call(**kw):
        a = {k: np.array(cs[k]) for k in ('xyl', 'K', 'R0', 't0', 'X0')}
        a.update(kw)
        return engine.refine_extrinsics_host(a['xyl'], a['K'], a['R0'], a['t0'], a['X0'], **{k: v for k, v in kw.items() if k == 'huber_px'})

    with pytest.raises(_lib.P2sError, match=r'n_cams=1 outside \[2, 32\]'):
        call(xyl=cs['xyl'][:, :1], K=cs['K'][:1], R0=cs['R0'][:1], t0=cs['t0'][:1])
    with pytest.raises(_lib.P2sError, match=r'n_cams=33 outside \[2, 32\]'):
        call(xyl=np.tile(cs['xyl'], (1, 11, 1, 1)), K=np.tile(cs['K'], (11, 1, 1)), R0=np.tile(cs['R0'], (11, 1, 1)), t0=np.tile(cs['t0'], (11, 1)))
    for key, text in (('K', 'camera 1: K and R must be finite'), ('R0', 'camera 1: K and R must be finite'), ('t0', 'camera 1: t must be finite')):
        v = np.array(cs[key])
        v[1].flat[-1] = np.nan
        with pytest.raises(_lib.P2sError, match=text):
            call(**{key: v})
    x = np.array(cs['xyl'])
    x[:, 2, :, 0] = np.nan
    with pytest.raises(_lib.P2sError, match='camera 2 has no kept observation'):
        call(xyl=x)
    x[:, 1, :, 1] = np.inf
    with pytest.raises(_lib.P2sError, match='no kept point'):
        call(xyl=x)
    t = np.array(cs['t0'])
    t[2, 2] = -t[2, 2]
    with pytest.raises(_lib.P2sError, match=r'point \d+ lies behind camera 2 at entry'):
        call(t0=t)
    with pytest.raises(_lib.P2sError, match='huber_px must be positive'):
        call(huber_px=0.0)
    with pytest.raises(_lib.P2sError, match='K, R and t hold'):
        call(K=cs['K'][:2])


def test_refined_calibration_round_trips_through_toml(tmp_path):
    cams = rigs.make_rig('ring', 4, seed=5, distortion='mild5')
    cs = rs.make_case('ring', 4, seed=5)
    refined = {k: list(v) for k, v in cams.items()}
    refined['R_mat'] = list(cs['R0'])
    refined['R'] = [cvmath.rodrigues_from_matrix(R) for R in cs['R0']]
    refined['T'] = list(cs['t0'])
    path = str(tmp_path / 'refined.toml')
    calib.write_calibration_toml(path, refined, adjusted=True, error=1.25)
    meta = calib.load_toml(path)['metadata']
    assert meta['adjusted'] is True and meta['error'] == 1.25
    back = calib.retrieve_calib_params(path)
    for k in ('K', 'dist', 'S', 'optim_K'):
        assert all(np.array_equal(a, b) for a, b in zip(back[k], cams[k])), k
    assert back['names'] == cams['names']
    assert max(np.abs(a - b).max() for a, b in zip(back['R_mat'], cs['R0'])) < 1e-14
    assert all(np.array_equal(a, b) for a, b in zip(back['T'], cs['t0']))
    # the present callers' output is what it was
    old = str(tmp_path / 'plain.toml')
    calib.write_calibration_toml(old, cams)
    assert open(old).read().endswith('[metadata]\nadjusted = false\nerror = 0.0\n')


def test_undistortion_leaves_pinhole_cameras_alone():
    cams = rigs.make_rig('ring', 3, seed=1)
    xyl = np.random.default_rng(0).uniform(0.0, 1000.0, (2, 3, 5, 3))
    xyl[0, 1, 2] = np.nan
    assert np.array_equal(calib_refine.undistorted(cams, xyl), xyl, equal_nan=True)
    lens = rigs.make_rig('ring', 3, seed=1, distortion='mild5')
    out = calib_refine.undistorted(lens, xyl)
    assert np.array_equal(out[..., 2], xyl[..., 2], equal_nan=True) and np.isnan(out[0, 1, 2]).all()
    c = 2
    back = cvmath.project_points(np.concatenate([(out[1, c, :, :2] - lens['K'][c][:2, 2]) / np.diag(lens['K'][c])[:2], np.ones((5, 1))], axis=1),
                                 np.eye(3), np.zeros(3), lens['K'][c], lens['dist'][c])
    assert np.abs(back - xyl[1, c, :, :2]).max() < 2e-3              # float32 pixels in and out


def test_command_line_arguments():
    a = calib_refine.parse_args(['-c', 'Calib.toml', '-p', 'pose'])
    assert (a.calib, a.pose, a.output, a.likelihood, a.huber, a.min_cams, a.keypoints, a.pose_model, a.frames) == \
        ('Calib.toml', 'pose', None, 0.3, 3.0, 2, None, 'HALPE_26', None)
    a = calib_refine.parse_args(['--calib', 'c.toml', '--pose', 'p', '-o', 'out.toml', '--likelihood', '0.5', '--huber', '2', '--min-cams', '3',
                                 '--keypoints', 'Nose, Neck,RHip', '--frames', '10', '20'])
    assert (a.output, a.likelihood, a.huber, a.min_cams, a.keypoints, a.frames) == ('out.toml', 0.5, 2.0, 3, ['Nose', 'Neck', 'RHip'], [10, 20])
    for bad in (['-p', 'pose'], ['-c', 'c.toml'], ['-c', 'c', '-p', 'p', '--huber', '0'], ['-c', 'c', '-p', 'p', '--min-cams', '1'],
                ['-c', 'c', '-p', 'p', '--keypoints', ' , ']):
        with pytest.raises(SystemExit):
            calib_refine.parse_args(bad)
    ids, names = calib_refine.select_keypoints('HALPE_26', ['Nose', 'Neck'])
    all_ids, all_names = calib_refine.select_keypoints('HALPE_26')
    assert names == ['Nose', 'Neck'] and ids == [all_ids[all_names.index('Nose')], all_ids[all_names.index('Neck')]] and len(all_ids) == 26
    with pytest.raises(ValueError, match='no keypoint named Elbow'):
        calib_refine.select_keypoints('HALPE_26', ['Nose', 'Elbow'])


def test_trial_reader_takes_the_first_person_in_natural_folder_order(tmp_path):
    from pose2sim_amd import poseio
    ids, _ = calib_refine.select_keypoints('HALPE_26', ['Nose', 'Neck'])
    rng = np.random.default_rng(0)
    people = rng.uniform(1.0, 100.0, (3, 4, 2, 26, 3)).astype(np.float32)          # [camera][frame][person]
    for c, name in enumerate(('cam2_json', 'cam10_json', 'cam1_json')):
        os.makedirs(tmp_path / name)
        for f in range(4):
            if (c, f) != (1, 2):                                                    # a missing file reads as NaN
                poseio.write_openpose_json(str(tmp_path / name / f'a_{f:03d}.json'), list(people[c, f]))
    os.makedirs(tmp_path / 'videos')
    xyl, dirs = calib_refine.read_trial(str(tmp_path), ids)
    assert dirs == ['cam1_json', 'cam2_json', 'cam10_json'] and xyl.shape == (4, 3, 2, 3)
    for c, src in enumerate((2, 0, 1)):
        for f in range(4):
            want = np.full((2, 3), np.nan) if (src, f) == (1, 2) else people[src, f, 0][ids]
            assert np.array_equal(xyl[f, c], want, equal_nan=True)
    assert calib_refine.read_trial(str(tmp_path), ids, frame_range=(1, 3))[0].shape == (2, 3, 2, 3)
    with pytest.raises(ValueError, match='2 or more are needed'):
        calib_refine.read_trial(str(tmp_path / 'cam1_json'), ids)
