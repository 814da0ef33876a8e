"""The rigs and likelihood patterns of tests/rigs.py, and the case list of tests/test_tri_screen_gpu.py (no GPU)."""
import numpy as np
import pytest

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


def test_default_distortion_is_the_pinhole_rig():
    for fam in rigs.RIGS:
        a, b = rigs.make_workload(fam, 6, 30, 26, seed=8), rigs.make_workload(fam, 6, 30, 26, seed=8, distortion='none')
        assert a['xyl'].tobytes() == b['xyl'].tobytes()
        assert all(np.array_equal(p, q) for p, q in zip(a['P'], b['P']))
        assert all(not np.any(d) for d in b['cams']['dist'])


@pytest.mark.parametrize('profile', rigs.DISTORTIONS[1:])
def test_distortion_profiles(profile):
    """Coefficient ranges and term counts, lenses laid out on each camera's own sensor, optim_K and P built from them."""
    from pose2sim_amd import cvmath, synth
    for fam in rigs.RIGS:
        wl = rigs.make_workload(fam, 9, 12, 26, seed=6, distortion=profile)
        cams, pin = wl['cams'], rigs.make_rig(fam, 9, seed=6)
        for c in range(9):
            d, Kc, size = cams['dist'][c], cams['K'][c], tuple(int(s) for s in cams['S'][c])
            assert np.array_equal(cams['S'][c], pin['S'][c]) and np.array_equal(cams['T'][c], pin['T'][c])
            assert len(d) == (4 if profile == 'pincushion' else 5)
            assert np.array_equal(cams['optim_K'][c], cvmath.get_optimal_new_camera_matrix(Kc, d, size, 1.0))
            assert np.allclose(cams['inv_K'][c] @ Kc, np.eye(3), atol=1e-12)
            rc = rigs.corner_radius(Kc, size)
            if profile == 'mild5':
                assert abs(d[0]) <= 0.1 and abs(d[1]) <= 0.05 and abs(d[2]) <= 1e-3 and abs(d[3]) <= 1e-3 and 0 < abs(d[4]) <= 0.02
                assert np.array_equal(Kc, pin['K'][c])
            elif profile == 'pincushion':
                assert 0.1 <= d[0] <= 0.25 and 0 <= d[1] <= 0.05 and np.array_equal(Kc, pin['K'][c])
            elif profile == 'wide':
                assert -0.32 <= d[0] <= -0.25 and 0.06 <= d[1] <= 0.12 and -0.02 <= d[4] <= -0.005 and abs(d[2]) <= 2e-3 >= abs(d[3])
                assert abs(Kc[0, 0] / (0.5 * size[0]) - 1) <= 0.03 and 1.1 < rc * rc < 1.5
                # the forward model r -> r cdist(r) rises all the way to the image corner: d(r cdist)/dr > 0 there
                slope, r_corner = rigs.forward_slope_to_corner(Kc, d, size)
                assert r_corner is not None and slope > 0, (fam, c, d)
                assert 1 + 3 * d[0] * r_corner ** 2 + 5 * d[1] * r_corner ** 4 + 7 * d[4] * r_corner ** 6 > 0
                assert (rigs.radial(d, np.linspace(0, r_corner, 500) ** 2) > 0).all()
            else:
                assert abs(Kc[0, 0] / (0.47 * size[0]) - 1) <= 0.03
                # 1 + k1 r^2 + k2 r^4 + k3 r^6 turns negative inside the image, in its outer part
                r = np.linspace(0, rc, 2000)
                neg = np.flatnonzero(rigs.radial(d, r * r) < 0)
                assert neg.size and 0.75 * rc < r[neg[0]] < 0.95 * rc, (fam, c, d)
                assert abs(cams['optim_K'][c][0, 0] / Kc[0, 0] - 1) < 0.08 and abs(cams['optim_K'][c][1, 1] / Kc[1, 1] - 1) < 0.08
        assert all(np.array_equal(p, q) for p, q in zip(wl['P'], synth.projection_matrices(cams, undistort=True)))
        assert not any(np.array_equal(p, q) for p, q in zip(wl['P'], synth.projection_matrices(cams, undistort=False)))
        if fam == 'uhd':
            assert {int(s[0]) for s in cams['S']} == {3840, 7680}
            assert np.nanmax(wl['xyl'][..., 0]) > 2000


def test_observations_go_through_the_distorted_model():
    """Noise-free observations of a pincushion rig, undistorted as the reference does, land on the projections through P."""
    from pose2sim_amd import cvmath
    wl = rigs.make_workload('uhd', 5, 40, 26, seed=9, distortion='pincushion', p_outlier=0.0, noise_px=0.0)
    cams, Q = wl['cams'], wl['Q3d'].reshape(-1, 3)
    for c in range(5):
        obs = wl['xyl'][:, 0, c, :, :2].reshape(-1, 2)
        seen = np.isfinite(obs[:, 0])
        und = cvmath.undistort_points(obs[seen], cams['K'][c], cams['dist'][c], cams['optim_K'][c])
        uv, _ = _project(np.asarray(wl['P'][c]), Q[seen])
        pin = cvmath.project_points(Q[seen], cams['R_mat'][c], cams['T'][c], cams['K'][c], np.zeros(4))
        assert np.abs(und - uv).max() < 0.02                        # float32 pixels at up to 7.7 k: 5e-4 px each way
        assert np.abs(obs[seen] - pin).max() > 1.0                  # and not on the pinhole projections


def test_fallback_counts():
    """The NumPy walk of the five iterations: no exit without a lens or inside a wide lens, a first-iteration exit for a pixel
    beyond the zero of the radial polynomial, a later one for a pixel whose iterates cross it."""
    cams = rigs.make_rig('ring', 2, seed=1, distortion='runaway')
    K0, d0 = cams['K'][0], cams['dist'][0]
    r = np.linspace(0, rigs.corner_radius(K0, cams['S'][0]), 4000)
    r_zero = r[np.flatnonzero(rigs.radial(d0, r * r) < 0)[0]]
    xyl = np.full((3, 1, 2, 1, 3), np.nan)
    xyl[0, 0, 0, 0] = [K0[0, 2] + 1.02 * r_zero * K0[0, 0], K0[1, 2], 1.0]          # beyond the zero
    xyl[1, 0, 0, 0] = [K0[0, 2] + 0.9 * r_zero * K0[0, 0], K0[1, 2], 1.0]           # inside it, past the fold: iterates run away
    xyl[2, 0, 0, 0] = [K0[0, 2] + 0.2 * r_zero * K0[0, 0], K0[1, 2], 1.0]           # near the centre: converges
    assert rigs.fallback_counts(xyl[0:1], cams) == (1, 0)
    assert rigs.fallback_counts(xyl[1:2], cams) == (0, 1)
    assert rigs.fallback_counts(xyl[2:3], cams) == (0, 0)
    assert rigs.fallback_counts(xyl, cams) == (1, 1)
    for profile in ('none', 'mild5', 'wide', 'pincushion'):
        wl = rigs.make_workload('ring', 4, 30, 26, seed=2, distortion=profile)
        assert rigs.fallback_counts(wl['xyl'], wl['cams']) == (0, 0)
    # ... and the walk is cvmath's: the fallback keeps the undistorted guess x0
    from pose2sim_amd import cvmath
    x, y = cvmath.undistort_normalized(xyl[:2, 0, 0, 0, 0], xyl[:2, 0, 0, 0, 1], K0, d0)
    assert np.array_equal(x, (xyl[:2, 0, 0, 0, 0] - K0[0, 2]) * (1.0 / K0[0, 0]))
