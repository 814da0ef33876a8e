"""Engine.refine_extrinsics on the GPU (csrc/p2s_refine.hip) against the scipy oracle of tests/refine_scipy.py and, at zero
noise, against the ground truth.  Every test prints its figures before it asserts; DESIGN.md 4.21 holds what was measured
and where the bounds of refine_scipy come from."""
import functools
import os

import numpy as np
import pytest

import refine_scipy as rs
from pose2sim_amd import _lib, calib, calib_refine, poseio, synth

pytestmark = pytest.mark.gpu

TILE, MAX_PARTS = _lib.P2S_REFINE_TILE, _lib.P2S_REFINE_MAX_PARTS
ORACLE_CASES = [('ring', 4), ('overhead', 4), ('one_side', 4), ('stadium', 4), ('ring', 2), ('ring', 3), ('ring', 8)]


@pytest.fixture(scope='module')
def engine():
    from pose2sim_amd.engine import Engine
    return Engine(0)


@functools.lru_cache(maxsize=None)
def oracle_case(family, C, F=5, Kp=13, dtype='float64', structure=False, min_cams=2):
    """The case and the oracle's answer, computed once (read-only for the tests)."""
    cs = rs.make_case(family, C, F=F, Kp=Kp, seed=C, dtype=np.dtype(dtype))
    if structure:
        rng = np.random.default_rng(5)
        x, X0 = cs['xyl'], cs['X0']                              # [F][C][Kp][3]
        for k in range(4):                                        # points seen by exactly min_cams cameras
            off = rng.permutation(C)[min_cams:]
            x[0, off, k, 2] = 0.05
        x[1, 1:, 0, 2] = 0.0                                      # seen by one camera only
        x[1, :, 1, 0] = np.nan                                    # by none: no finite x
        X0[2 * Kp + 3] = np.nan                                   # no start
        X0[2 * Kp + 4, 1] = np.nan
        cs['X0'] = np.where(np.isnan(X0).any(axis=1, keepdims=True), np.nan, X0)
    cs['oracle'] = rs.refine(cs['xyl'], cs['K'], cs['R0'], cs['t0'], cs['X0'], min_cams=min_cams)
    for v in cs.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return cs


def run(engine, cs, **kw):
    return engine.refine_extrinsics(cs['xyl'], cs['K'], cs['R0'], cs['t0'], cs['X0'], **kw)


def check_against_oracle(label, cs, out, scale=1.0):
    R, t, X, rep = out
    Ro, to, Xo, co, _ = cs['oracle']
    rel = (rep['cost_after'] - scale * co) / (scale * co)
    dc = np.abs(rs.centres(R, t) - rs.centres(Ro, to)).max()
    print(f'{label}: cost {rep["cost_before"]:.6f} -> {rep["cost_after"]:.9f}, oracle {scale * co:.9f}, relative difference {rel:.3e}; '
          f'centres within {dc:.3e} m of the oracle\'s; {rep["iterations"]} trials, {rep["accepted"]} accepted, {rep["kept_points"]} points')
    assert rep['cost_after'] <= rep['cost_before']
    assert abs(rel) <= rs.COST_REL_BOUND
    assert dc <= rs.CENTRE_BOUND
    return rel, dc


@pytest.mark.parametrize('family, C', ORACLE_CASES, ids=[f'{f}-{c}' for f, c in ORACLE_CASES])
def test_against_the_oracle(engine, family, C):
    cs = oracle_case(family, C)
    out = run(engine, cs)
    check_against_oracle(f'{family} {C}', cs, out)
    # the points too: those the oracle kept, where it put them
    X, Xo = out[2].reshape(-1, 3), cs['oracle'][2]
    assert np.array_equal(np.isnan(X), np.isnan(Xo))
    dx = np.nanmax(np.abs(X - Xo))
    print(f'{family} {C}: points within {dx:.3e} m of the oracle\'s')
    assert dx <= rs.POINT_BOUND


def test_32_cameras(engine):
    """The largest reduced system (185 unknowns, 560 rows of workgroups): 20 points keep scipy's Jacobian within seconds."""
    cs = oracle_case('ring', 32, F=2, Kp=10)
    check_against_oracle('ring 32', cs, run(engine, cs))


@pytest.mark.parametrize('copies', [5, 13])
def test_tiles_against_the_oracle(engine, copies):
    """The ring-4 case with every point `copies` times: the cost is `copies` x the oracle's and its minimum the oracle's,
    over 2 and 4 workgroup passes (325 and 845 points)."""
    cs = dict(oracle_case('ring', 4))
    assert copies * 65 > (copies // 4) * TILE
    cs['xyl'] = np.tile(cs['xyl'], (copies, 1, 1, 1))
    cs['X0'] = np.tile(cs['X0'], (copies, 1))
    check_against_oracle(f'ring 4 x {copies}', cs, run(engine, cs), scale=float(copies))


def exact_case(n_points, C=3, seed=3):
    """n_points noise-free observations of likelihood 1 through the true cameras; start: the truth moved by ~2 cm."""
    F = -(-n_points // 13)
    cs = rs.make_case('ring', C, F=1, Kp=13, seed=seed, noise_px=0.0, p_outlier=0.0, lik=None)
    Q = synth.make_points3d(F, 1, 13, seed=seed)[:, 0].reshape(-1, 3)[:n_points]
    uv, _ = rs.project(cs['K'], cs['R'], cs['t'], Q)                 # [C][N][2]
    xyl = np.ones((n_points, C, 1, 3))
    xyl[:, :, 0, :2] = np.swapaxes(uv, 0, 1)
    cs['xyl'], cs['Q'] = xyl, Q
    cs['X0'] = Q + np.random.default_rng(seed).normal(0.0, 0.02, Q.shape)
    return cs


BOUNDARY_POINTS = [8, TILE - 1, TILE, TILE + 1, 3 * TILE + 1, MAX_PARTS * TILE + 1]


@pytest.mark.parametrize('n_points', BOUNDARY_POINTS)
def test_exact_recovery_across_tiles(engine, n_points):
    """Zero noise, no outliers, likelihood 1: the refined cameras are the true ones, at point counts on both sides of every
    boundary of the build: one pass, one more point, several passes, more passes than partial sums."""
    cs = exact_case(n_points)
    R, t, X, rep = run(engine, cs)
    dc = np.abs(rs.centres(R, t) - rs.centres(cs['R'], cs['t'])).max()
    dx = np.abs(X.reshape(-1, 3) - cs['Q']).max()
    print(f'{n_points} points: centres within {dc:.3e} m of the truth, points within {dx:.3e} m; cost {rep["cost_before"]:.3e} -> '
          f'{rep["cost_after"]:.3e} in {rep["iterations"]} trials')
    assert rep['kept_points'] == n_points
    assert dc <= rs.ZERO_NOISE_BOUND and dx <= rs.ZERO_NOISE_BOUND


def test_exact_recovery_on_a_rig_case(engine):
    cs = rs.make_case('ring', 3, seed=1, noise_px=0.0, p_outlier=0.0, lik=None)
    R, t, X, rep = run(engine, cs)
    dc = np.abs(rs.centres(R, t) - rs.centres(cs['R'], cs['t'])).max()
    print(f'zero noise, ring 3: centres within {dc:.3e} m of the truth; {rep["iterations"]} trials')
    assert dc <= rs.ZERO_NOISE_BOUND


@pytest.mark.parametrize('min_cams', [2, 3])
def test_structure(engine, min_cams):
    """Points seen by exactly min_cams cameras count; points seen by fewer, or without a start, are ignored and come back NaN."""
    cs = oracle_case('ring', 4, structure=True, min_cams=min_cams)
    out = run(engine, cs, min_cams=min_cams)
    check_against_oracle(f'structure, min_cams {min_cams}', cs, out)
    X, Xo = out[2].reshape(-1, 3), cs['oracle'][2]
    _, kept = rs.weights(cs['xyl'], cs['X0'], 0.3, min_cams)
    assert out[3]['kept_points'] == kept.sum() < len(kept)
    assert np.array_equal(np.isnan(X).all(axis=1), ~kept) and np.array_equal(np.isnan(X), np.isnan(Xo))
    assert not kept[13] and not kept[14] and not kept[2 * 13 + 3] and not kept[2 * 13 + 4]


def test_float32_observations(engine):
    cs = oracle_case('ring', 4, dtype='float32')
    assert cs['xyl'].dtype == np.float32
    check_against_oracle('ring 4, float32', cs, run(engine, cs))


def test_determinism(engine):
    """Two calls on the same input return the same bits: no sum depends on the order the workgroups finish in."""
    cs = dict(oracle_case('ring', 4))
    cs['xyl'] = np.tile(cs['xyl'], (13, 1, 1, 1))
    cs['X0'] = np.tile(cs['X0'], (13, 1))
    a, b = run(engine, cs), run(engine, cs)
    for x, y in zip(a[:3], b[:3]):
        assert x.tobytes() == y.tobytes()
    for k in a[3]:
        assert np.asarray(a[3][k]).tobytes() == np.asarray(b[3][k]).tobytes(), k


def test_max_iter_zero_returns_the_input(engine):
    cs = oracle_case('ring', 4)
    R, t, X, rep = run(engine, cs, max_iter=0)
    assert np.array_equal(R, cs['R0']) and np.array_equal(t, cs['t0'])
    assert np.array_equal(X.reshape(-1, 3), cs['X0'], equal_nan=True)
    assert rep['cost_after'] == rep['cost_before'] and rep['iterations'] == 0 and rep['accepted'] == 0
    c0 = rs.cost(cs['xyl'], cs['K'], cs['R0'], cs['t0'], cs['X0'])
    print(f'cost at the input {rep["cost_before"]:.9f}, oracle\'s cost function {c0:.9f}')
    assert abs(rep['cost_before'] - c0) <= 1e-12 * c0                # the same sum of ~500 terms in another order
    assert np.array_equal(rep['rms_before'], rep['rms_after'])
    assert engine.refine_kernel_ms() >= 0.0


def test_refusals(engine):
    """Everything here is refused on the host or right after the weights are known, before any refinement kernel runs."""
    cs = oracle_case('ring', 4)
    P2sError = _lib.P2sError

    def call(**kw):
        a = {k: np.array(cs[k]) for k in ('xyl', 'K', 'R0', 't0', 'X0')}
        a.update(kw)
        return engine.refine_extrinsics(a['xyl'], a['K'], a['R0'], a['t0'], a['X0'])

    with pytest.raises(P2sError, match=r'n_cams=1 outside \[2, 32\]'):
        call(xyl=cs['xyl'][:, :1], K=cs['K'][:1], R0=cs['R0'][:1], t0=cs['t0'][:1])
    with pytest.raises(P2sError, match=r'n_cams=33 outside \[2, 32\]'):
        call(xyl=np.tile(cs['xyl'], (1, 9, 1, 1))[:, :33], K=np.tile(cs['K'], (9, 1, 1))[:33], R0=np.tile(cs['R0'], (9, 1, 1))[:33],
             t0=np.tile(cs['t0'], (9, 1))[:33])
    for key, text in (('K', 'camera 2: K and R must be finite'), ('R0', 'camera 2: K and R must be finite'), ('t0', 'camera 2: t must be finite')):
        for bad in (np.nan, np.inf):
            v = np.array(cs[key])
            v[2].flat[0] = bad
            with pytest.raises(P2sError, match=text):
                call(**{key: v})
    x = np.array(cs['xyl'])
    x[:, 3, :, 2] = 0.1
    with pytest.raises(P2sError, match='camera 3 has no kept observation'):
        call(xyl=x)
    x = np.array(cs['xyl'])
    x[..., 2] = 0.2
    with pytest.raises(P2sError, match='no kept point'):
        call(xyl=x)
    with pytest.raises(P2sError, match='no kept point'):
        call(X0=np.full_like(cs['X0'], np.nan))
    t = np.array(cs['t0'])
    t[1, 2] = -t[1, 2]                                               # the scene behind camera 1
    with pytest.raises(P2sError, match=r'point \d+ lies behind camera 1 at entry'):
        call(t0=t)
    with pytest.raises(P2sError, match='X0 holds'):
        call(X0=cs['X0'][:-1])


def _mean_triangulation_error(engine, calib_file, xyl):
    """Mean reprojection error (px) of the trial's triangulation with undistortion, as the triangulation stage computes it."""
    from pose2sim_amd.engine import Engine
    cams = calib.retrieve_calib_params(calib_file)
    engine.set_calibration(calib.computeP(calib_file, undistort=True), cams)
    err = engine.triangulate(xyl, Engine.tri_params(1e6, 0.3, 2, undistort=True))[1]
    return float(np.nanmean(err))


def test_refine_calibration_end_to_end(engine, tmp_path):
    """A synthetic trial on lenses with distortion, written with the project's writers: the refined TOML loads, says
    adjusted = true, keeps the intrinsics, and triangulates the trial with a lower reprojection error than the perturbed one."""
    cs = rs.make_case('ring', 4, F=5, Kp=26, seed=11, distortion='mild5')
    cams = {k: list(v) for k, v in cs['cams'].items()}
    cams['R_mat'] = list(cs['R0'])
    cams['R'] = [calib_refine.cvmath.rodrigues_from_matrix(R) for R in cs['R0']]
    cams['T'] = list(cs['t0'])
    perturbed = str(tmp_path / 'Calib_perturbed.toml')
    calib.write_calibration_toml(perturbed, cams)
    pose = tmp_path / 'pose'
    for c, name in enumerate(cams['names']):
        os.makedirs(pose / f'{name}_json')
        for f in range(5):
            poseio.write_openpose_json(str(pose / f'{name}_json' / f'trial_{f:06d}.json'), [cs['xyl'][f, c].astype(np.float32)])
    out, report = calib_refine.refine_calibration(perturbed, str(pose), engine=engine)
    assert out == str(tmp_path / 'Calib_perturbed_refined.toml') and os.path.exists(out)
    assert calib.load_toml(out)['metadata']['adjusted'] is True
    new = calib.retrieve_calib_params(out)
    for k in ('K', 'dist', 'S'):
        assert all(np.array_equal(a, b) for a, b in zip(new[k], cams[k])), k
    assert new['names'] == cams['names']
    xyl = cs['xyl'].astype(np.float32)[:, None]
    before, after = _mean_triangulation_error(engine, perturbed, xyl), _mean_triangulation_error(engine, out, xyl)
    d0 = np.abs(rs.centres(cs['R0'], cs['t0']) - rs.centres(cs['R'], cs['t'])).max()
    d1 = np.abs(rs.centres(new['R_mat'], new['T']) - rs.centres(cs['R'], cs['t'])).max()
    print(f'mean triangulation reprojection error {before:.3f} px -> {after:.3f} px; cost {report["cost_before"]:.1f} -> {report["cost_after"]:.1f}; '
          f'centres {d0:.3f} m -> {d1:.3f} m from the truth')
    assert report['cost_after'] < report['cost_before']
    assert after < before
