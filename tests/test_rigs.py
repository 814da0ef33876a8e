"""The rigs and likelihood patterns of tests/rigs.py, and the case list of tests/test_tri_screen_gpu.py (no GPU)."""
import numpy as np

import rigs
from test_tri_screen_gpu import CASES


def test_case_list_covers_the_kernel():
    """Every family, mode and kernel instantiation of the pooled kernel is in the screen-on-against-off list."""
    assert {c[0] for c in CASES} == set(rigs.RIGS) and {c[1] for c in CASES} == set(rigs.LIK_MODES)
    assert {c[2] for c in CASES} >= {3, 4, 6, 8, 9, 12, 16}
    assert {c[3] for c in CASES} == {1.0, 15.0, 60.0} and {c[4] for c in CASES} == {0.0, 0.01, 0.3}
    assert {c[5] for c in CASES} == {2, 3, 4}
    assert {c[6] for c in CASES if c[2] in (6, 8)} == {2, 5, 6}
    assert all((c[6] is None) == (c[2] not in (6, 8)) for c in CASES)
    assert {c[0] for c in CASES if c[1] == 'clamped'} == set(rigs.RIGS)
    assert any(c[7] for c in CASES)
    assert len(set(CASES)) == len(CASES)


def _project(P, Q):
    h = np.einsum('ij,nj->ni', P, np.c_[Q, np.ones(len(Q))])
    return h[:, :2] / h[:, 2:], h[:, 2]


def test_every_rig_sees_its_scene():
    """Pinhole cameras (dist 0) that have the whole scene in front of them, at the distances and focal lengths promised."""
    for fam in rigs.RIGS:
        wl = rigs.make_workload(fam, 9, 200, 26, seed=5)
        cams, Q = wl['cams'], wl['Q3d'].reshape(-1, 3)
        assert len(wl['P']) == 9 and all(not np.any(d) for d in cams['dist'])
        for c, P in enumerate(wl['P']):
            R = cams['R_mat'][c]
            assert np.allclose(R @ R.T, np.eye(3), atol=1e-9) and np.isclose(np.linalg.det(R), 1.0)
            _, z = _project(P, Q)
            assert (z > 0).all(), f'{fam}: camera {c} has scene points behind it'
        f = np.array([k[0, 0] for k in cams['K']])
        if fam == 'stadium':
            assert f.min() >= 4000 and f.max() <= 8000
        if fam == 'mixed':
            assert f.min() >= 500 and f.max() <= 6000 and f.max() / f.min() > 3
        if fam == 'uhd':
            assert max(s[0] for s in cams['S']) == 7680 and np.nanmax(np.abs(wl['xyl'][..., :2])) > 4000


def test_far_origin_straddles_the_screen_guard():
    wl = rigs.make_workload('far_origin', 6, 500, 26, seed=3)
    r = np.linalg.norm(wl['Q3d'], axis=-1)
    assert r.min() > 25.0 and r.max() < 32.0 and (r > 30.0).any() and (r < 30.0).any()


def test_close_rig_scale():
    wl = rigs.make_workload('close', 6, 200, 26, seed=3)
    Q = wl['Q3d'].reshape(-1, 3)
    assert np.ptp(Q, axis=0).max() < 0.4
    for c, P in enumerate(wl['P']):
        _, z = _project(P, Q)
        ratio = wl['cams']['K'][c][0, 0] / z
        assert 0.6 <= z.min() and z.max() <= 1.5 and 1300 < np.median(ratio) < 3000


def test_overhead_cameras_look_down():
    cams = rigs.make_rig('overhead', 6, seed=1)
    down = [c for c in range(6) if cams['R_mat'][c][2] @ np.array([0.0, 0.0, -1.0]) > 0.999]
    assert down == [1, 4]


def test_one_side_arc():
    cams = rigs.make_rig('one_side', 8, seed=1)
    pos = np.array([-cams['R_mat'][c].T @ cams['T'][c] for c in range(8)])
    ang = np.degrees(np.arctan2(pos[:, 1], pos[:, 0]))
    assert np.ptp(ang) <= 62.0


def test_likelihood_modes():
    F, C, K = 300, 6, 26
    low = rigs.make_workload('ring', C, F, K, lik='low', seed=2)['xyl'][..., 2]
    frac = np.nanmean((low >= 1e-3) & (low <= 0.05))
    assert 0.4 < frac < 0.6
    z = rigs.make_workload('ring', C, F, K, lik='zeros', seed=2)['xyl']
    exact0 = (z == 0).all(axis=-1)
    assert 0.03 < exact0.mean() < 0.07
    hl = rigs.make_workload('ring', C, F, K, lik='heavy_light', seed=2)
    w = hl['xyl'][:, 0, :, :, 2]                                   # [F][C][K]
    n_heavy = (w == 1.0).sum(axis=1)
    assert set(np.unique(n_heavy)) == {1, 2}
    light = w[w != 1.0]
    assert light.min() >= 1e-3 and light.max() <= 1e-2
    # the heavy cameras are the gross outliers, the light ones accurate
    uv = np.stack([np.asarray(_project(np.asarray(P), hl['Q3d'].reshape(-1, 3))[0]).reshape(F, K, 2) for P in hl['P']], 1)
    d = np.linalg.norm(hl['xyl'][:, 0, :, :, :2] - uv, axis=-1)
    assert d[w == 1.0].min() > 50.0 and np.median(d[w != 1.0]) < 3.0


def test_duplicate_camera():
    wl = rigs.make_workload('mixed', 5, 50, 26, seed=4, dup=True)
    assert np.array_equal(wl['P'][0], wl['P'][1])
    assert np.array_equal(wl['xyl'][:, :, 0], wl['xyl'][:, :, 1], equal_nan=True)
    assert not np.array_equal(wl['P'][0], wl['P'][2])
