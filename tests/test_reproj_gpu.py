"""The reprojection kernel and the whole utility on the MI355X, through the C-ABI: against the goldens recorded from the
reference (tests/golden/reproj_units.npz), against the NumPy restatement on large seeded shapes, and in a closed loop with
the triangulation kernels.  Every test prints its figure (worst difference, share of values near a rounding tie,
kernel time) before it asserts; DESIGN.md 4.11 holds the bounds and where they come from."""
import ctypes as C

import numpy as np
import pytest

import reproj_numpy as rn
from test_reproj_host import (ALL, ARRAY_CASES, CLOSED_LOOP_CPU_WORST_F32, ERR_THR, LIK_THR, MIN_CAMS, RAW_TOL, check_arrays,
                              closed_loop_mean_distance, closed_loop_workload, engine_inputs, gold, run_case)  # noqa: F401

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def engine():
    from pose2sim_amd.engine import Engine
    return Engine(0)


@pytest.mark.parametrize('name', ARRAY_CASES)
def test_kernel_reproduces_the_reference(gold, engine, tmp_path, name, capsys):   # noqa: F811
    Q, kw = engine_inputs(gold, name, str(tmp_path))
    uv, uv_raw = engine.reproject(Q, raw=True, **kw)
    with capsys.disabled():
        check_arrays(gold, name, uv, uv_raw)
    assert np.array_equal(engine.reproject(Q, **kw), uv, equal_nan=True), 'the call without uv_raw'


@pytest.mark.parametrize('name', ALL)
def test_utility_on_the_gpu_writes_the_recorded_files(gold, engine, tmp_path, name, capsys, monkeypatch):   # noqa: F811
    run_case(gold, name, str(tmp_path), engine, capsys, monkeypatch)


def large_scene(F, K, Cn, seed, distort):
    from pose2sim_amd import synth
    cams = synth.make_cameras(Cn, seed=seed, distort=distort)
    rng = np.random.default_rng(seed)
    Q = np.ascontiguousarray(synth.make_points3d(F, 1, K, seed=seed)[:, 0])
    Q[rng.random((F, K)) < 0.02] = np.nan
    Q[rng.random((F, K)) < 0.03] *= 1.7                           # pushed out of some images, still in front of every camera
    return cams, Q, np.array(cams['S'])


def check_large(engine, Q, kw, capsys):
    ref, ref_raw = rn.reproject(Q, raw=True, **kw)
    uv, uv_raw = engine.reproject(Q, raw=True, **kw)
    finite = np.isfinite(ref_raw)
    assert np.array_equal(np.isfinite(uv_raw), finite)
    worst = float(np.abs(uv_raw[finite] - ref_raw[finite]).max())
    t = ref_raw * 10
    with np.errstate(invalid='ignore'):
        clear = ~(np.abs(t - np.floor(t) - 0.5) <= 1e-6)             # NaN and infinite values count as clear
    clear = (clear[..., 0] & clear[..., 1])[..., None] & np.ones(2, dtype=bool)
    left_out = 1.0 - clear.mean()
    with capsys.disabled():
        print(f'{uv.shape}: worst |raw - restatement| = {worst:.3e} px, {int((~clear).sum())} of {clear.size} values within 1e-6 of a '
              f'rounding tie ({left_out:.2e}), kernel {engine.reproject_kernel_ms():.3f} ms')
    assert worst <= RAW_TOL
    assert left_out <= 1e-5
    assert np.array_equal(np.isnan(uv[clear]), np.isnan(ref[clear]))
    keep = clear & ~np.isnan(ref)
    assert np.array_equal(uv[keep], ref[keep])


def test_large_plain_static(engine, capsys):
    cams, Q, sizes = large_scene(20000, 133, 16, 301, False)
    from pose2sim_amd import synth
    check_large(engine, Q, {'P': np.array(synth.projection_matrices(cams))[:, None], 'sizes': sizes}, capsys)


def test_large_plain_per_frame(engine, capsys):
    from pose2sim_amd import synth
    F = 20000
    cams, Q, sizes = large_scene(F, 133, 8, 302, False)
    P = np.array(synth.projection_matrices(cams))
    rng = np.random.default_rng(302)
    P = P[:, None] * (1 + rng.normal(0, 1e-3, (8, F, 3, 4)))       # one matrix per camera and frame
    check_large(engine, Q, {'P': P, 'sizes': sizes}, capsys)


def test_large_distorted(engine, capsys):
    cams, Q, sizes = large_scene(20000, 26, 8, 303, True)
    check_large(engine, Q, {'cal': cams, 'sizes': sizes}, capsys)


@pytest.mark.parametrize('Cn,F', [(4, 400), (8, 300), (16, 150)])
def test_closed_loop_with_the_triangulation_kernels(engine, Cn, F, capsys):
    """For every triangulated unit, the mean pixel distance between its kept observations and the new kernel's projection of
    the triangulation kernel's own 3D point is the reprojection error the triangulation reported.  Tolerance: ten times
    the worst difference of the same comparison on the CPU (test_reproj_host.py), the error being reported in float32."""
    from pose2sim_amd.engine import Engine
    wl = closed_loop_workload(Cn, F, seed=200 + Cn)
    tri = Engine(0)
    tri.set_calibration(wl['P'])
    Q, err, _, mask = tri.triangulate(wl['xyl'], Engine.tri_params(ERR_THR, LIK_THR, MIN_CAMS))
    tri.close()
    xyl, Q, err, mask = wl['xyl'].reshape(F, Cn, 26, 3), Q.reshape(F, 26, 3), err.reshape(F, 26), mask.reshape(F, 26)
    _, uv_raw = engine.reproject(Q, P=np.array(wl['P']), sizes=np.array(wl['cams']['S']), raw=True)
    mine = closed_loop_mean_distance(xyl, mask, uv_raw)
    ok = ~np.isnan(err)
    assert ok.sum() > 0.8 * ok.size
    assert np.isnan(uv_raw[:, ~ok]).all()
    worst = float(np.abs(mine[ok] - err[ok].astype(np.float64)).max())
    with capsys.disabled():
        print(f'closed loop, {Cn} cameras, {ok.sum()} units: worst |reported error - mean distance| = {worst:.3e} px '
              f'(allowed {10 * CLOSED_LOOP_CPU_WORST_F32:.2e})')
    assert worst <= 10 * CLOSED_LOOP_CPU_WORST_F32


def test_argument_errors_come_back_as_status_and_message(engine):
    from pose2sim_amd import _lib
    lib, h = engine._lib, engine._h
    F, K, Cn = 4, 3, 2
    Q, P, sizes = np.zeros((F, K, 3)), np.zeros((Cn, 1, 12)), np.full((Cn, 2), 100.0)
    Km, d, R, T = np.zeros((Cn, 9)), np.zeros((Cn, 5)), np.zeros((Cn, 9)), np.zeros((Cn, 3))
    uv = np.zeros((Cn, F, K, 2))
    p = lambda a: a.ctypes.data_as(C.c_void_p)                      # noqa: E731
    ok = dict(F=F, K=K, Q=p(Q), C=Cn, Fp=1, P=p(P), Km=p(Km), d=p(d), R=p(R), T=p(T), sizes=p(sizes), flags=0, raw=None, uv=p(uv))

    def call(**change):
        a = {**ok, **change}
        rc = lib.p2s_reproject_host(h, a['F'], a['K'], a['Q'], a['C'], a['Fp'], a['P'], a['Km'], a['d'], a['R'], a['T'], a['sizes'],
                                    a['flags'], a['raw'], a['uv'])
        return rc, (lib.p2s_last_error() or b'').decode()

    assert call()[0] == 0
    assert call(flags=_lib.P2S_REPROJ_DISTORTED)[0] == 0
    for change, text in (({'Fp': 3}, 'neither 1 nor n_frames'), ({'Fp': F, 'flags': 1}, 'static cameras'), ({'uv': None}, 'null uv'),
                         ({'C': 0}, 'n_cams=0'), ({'C': 33}, 'n_cams=33'), ({'P': None}, 'null P'), ({'Q': None}, 'null Q'),
                         ({'sizes': None}, 'null sizes'), ({'flags': 1, 'Km': None}, 'needs K, dist, R and T'), ({'flags': 6}, 'unknown flags'),
                         ({'F': -1}, 'bad shape')):
        rc, msg = call(**change)
        assert rc == _lib.P2S_ERR_INVALID_ARG and text in msg, (change, rc, msg)
    assert lib.p2s_reproject_host(None, F, K, p(Q), Cn, 1, p(P), None, None, None, None, p(sizes), 0, None, p(uv)) == _lib.P2S_ERR_INVALID_ARG
    assert call(F=0)[0] == 0                                        # nothing to do is not an error
