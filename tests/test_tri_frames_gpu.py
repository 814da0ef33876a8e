"""Triangulation with per-frame cameras (csrc/p2s_tri_frames.hip) on the GPU, at the bars of tests/test_tri_gpu.py: 3D within
1e-7 m of the C oracle run frame by frame with that frame's matrices, identical camera selections (n_excl, mask, NaN
pattern), the error within 2e-6 relative.  The rig of tests/moving_rig.py pans, tilts, drifts and zooms every camera in
every frame, so a unit triangulated with any other frame's matrices is metres away from its expectation."""
import json
import os
import sys

import numpy as np
import pytest

import moving_rig
from test_tri_gpu import TOL_E, TOL_Q, _compare  # noqa: F401 -- TOL_E is the bar _compare holds the error to

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden'))
import e2e_common as ec  # noqa: E402

pytestmark = pytest.mark.gpu

LIK_THR, THR = 0.3, 15.0


@pytest.fixture(scope='module')
def engine():
    import __graft_entry__ as entry
    entry.build_hip()
    from pose2sim_amd.engine import Engine
    eng = Engine(0)
    yield eng
    eng.close()


def oracle_frames(xyl, P, frames, min_cams):
    """The C oracle frame by frame: row i of xyl with the matrices of calibration frame frames[i]."""
    from oracle import tri_oracle
    K = xyl.shape[-2]
    out = [tri_oracle.triangulate_batch(xyl[i], P[f], None, list(range(K)), LIK_THR, THR, min_cams) for i, f in enumerate(frames)]
    return tuple(np.stack([o[j] for o in out]) for j in range(4))


def assert_covers(ref, what, heavy=False):
    """The oracle's answer itself holds what the case is about: units with 0, 1 and >= 2 excluded cameras and a unit that
    is not triangulated (heavy: three or more excluded as well)."""
    _, er, nr, _ = ref
    done = ~np.isnan(er)
    for want, have in (('n_excl 0', (nr[done] == 0).any()), ('n_excl 1', (nr == 1).any()), ('n_excl >= 2', (nr >= 2).any()),
                       ('a NaN unit', (~done).any())):
        assert have, f'{what}: the oracle has no unit with {want}'
    if heavy:
        assert (nr[done] >= 3).any(), f'{what}: the oracle has no triangulated unit with n_excl >= 3'


# C, K, persons, F, float64, min_cameras, seed.  min_cameras is chosen per camera count so that the oracle's own answer holds
# every class assert_covers asks for under make_config's default contamination (5 % low likelihoods, 3 % outliers, 1 %
# missing cameras): with 8 cameras and min_cameras 2 a unit ends untriangulated only when 7 cameras fail at once (1e-8 a
# unit), with min_cameras 5 or 6 when 3 or 4 do.  Two cameras run with min_cameras 1: with 2 a unit that loses a camera
# does not run at all and is reported with both excluded, so n_excl 1 cannot occur.  The seeds are ones at which the
# oracle alone satisfies assert_covers, found on the CPU.
CASES = [
    (2, 26, 1, 64, False, 1, 0),
    (3, 1, 1, 200, False, 2, 1),
    (4, 5, 1, 37, False, 2, 1),
    (8, 26, 1, 120, False, 5, 0),
    (8, 26, 2, 60, False, 6, 0),
    (6, 133, 1, 24, False, 2, 14),
    (16, 26, 1, 40, False, 13, 0),
    (8, 26, 1, 50, True, 6, 0),
]

_workloads = {}


def workload(case, **contamination):
    """The observations, matrices and the oracle's answer of a case, computed once."""
    key = (case, tuple(sorted(contamination.items())))
    if key not in _workloads:
        C, K, Pn, F, f64, min_cams, seed = case
        wl = moving_rig.make_workload(F, C, K, Pn, seed=seed, dtype=np.float64 if f64 else np.float32, **contamination)
        wl['ref'] = oracle_frames(wl['xyl'], wl['P'], range(F), min_cams)
        _workloads[key] = wl
    return _workloads[key]


@pytest.mark.parametrize('case', CASES, ids=lambda c: 'C{}-K{}-P{}-F{}-{}'.format(c[0], c[1], c[2], c[3], 'f64' if c[4] else 'f32'))
def test_every_unit_against_the_oracle_frame_by_frame(engine, case):
    wl = workload(case)
    assert_covers(wl['ref'], str(case))
    assert wl['xyl'].dtype == (np.float64 if case[4] else np.float32)
    got = engine.triangulate_frames(wl['xyl'], wl['P'], engine.tri_params(THR, LIK_THR, case[5]))
    dq = _compare(*got, *wl['ref'], what=str(case))
    print(f'{case}: worst |dQ| = {dq:.3e} m')


HEAVY_SEED = 63         # 120 frames: one unit in 3 120 ends untriangulated at min_cameras 2 (7 of 8 cameras must fail)


@pytest.mark.parametrize('min_cams', [2, 4])
def test_heavy_contamination_descends_several_levels(engine, min_cams):
    """A quarter of the detections are outliers: units descend several levels and some end untriangulated."""
    case = (8, 26, 1, 120, False, min_cams, HEAVY_SEED)
    wl = workload(case, p_outlier=0.25)
    assert_covers(wl['ref'], f'heavy, min_cameras {min_cams}', heavy=True)
    engine.tri_stats(reset=True)
    got = engine.triangulate_frames(wl['xyl'], wl['P'], engine.tri_params(THR, LIK_THR, min_cams))
    _compare(*got, *wl['ref'], what=f'heavy, min_cameras {min_cams}')
    st = engine.tri_stats(reset=True)
    assert st['subsets_evaluated'] >= st['search_units'] > 0 and st['passes'] > 0


def test_block_frame_with_offset_skips_and_repeats(engine):
    """Blocks [3, 3, 7, 7, 8, 8, 20, 20, 20, 39]: an offset, skipped frames, persons sharing a frame, a lone block."""
    wl = workload(CASES[3])
    frames = [3, 3, 7, 7, 8, 8, 20, 20, 20, 39]
    xyl = np.ascontiguousarray(wl['xyl'][:len(frames), 0])                   # [blocks][C][K][3]: any observations will do
    ref = oracle_frames(xyl, wl['P'], frames, 2)
    got = engine.triangulate_frames(xyl, wl['P'], engine.tri_params(THR, LIK_THR, 2), block_frame=frames)
    _compare(*got, *ref, what='block_frame')
    # the same observations with the default map are another problem altogether
    other = oracle_frames(xyl, wl['P'], range(len(frames)), 2)
    both = ~np.isnan(ref[1]) & ~np.isnan(other[1])
    assert both.any() and np.abs(ref[0][both] - other[0][both]).max() > 1e3 * TOL_Q


@pytest.mark.parametrize('C,F', [(8, 300), (16, 60)])
def test_static_rig_repeated_equals_the_static_path(engine, C, F):
    from pose2sim_amd import synth
    wl = synth.make_config(F, C, 26, 1, seed=11)
    P = np.array(wl['P'])
    prm = engine.tri_params(THR, LIK_THR, 2)
    engine.set_calibration(P)
    want = engine.triangulate(wl['xyl'], prm)
    got = engine.triangulate_frames(wl['xyl'], np.broadcast_to(P, (F,) + P.shape), prm)
    assert (~np.isnan(want[1])).any() and (want[2] >= 1).any()
    _compare(*got, *want, what=f'static {C} x 26 x {F}')
    # and the static calibration is still in place
    again = engine.triangulate(wl['xyl'], prm)
    assert all(np.array_equal(a, b, equal_nan=True) for a, b in zip(want, again))


@pytest.mark.parametrize('name', ['zooming', 'moving', 'zooming_moving'])
def test_reference_projections_closed_loop(engine, golden_dir, tmp_path, name):
    """The pixels the reference projected through a per-frame calibration, unrounded, triangulate back to the .trc's points."""
    from pose2sim_amd import calib
    from pose2sim_amd import reproj_from_trc_calib as rp
    gold = np.load(os.path.join(golden_dir, 'reproj_units.npz'))
    toml_path, trc_path = str(tmp_path / 'Calib.toml'), str(tmp_path / str(gold[f'{name}__trc_name']))
    with open(toml_path, 'w') as fh:
        fh.write(str(gold[f'{name}__toml']))
    with open(trc_path, 'w') as fh:
        fh.write(str(gold[f'{name}__trc']))
    P, _ = calib.frame_projections(toml_path)
    _, _, Q = rp.read_markers(trc_path)
    raw = gold[f'{name}__raw']                                              # [C][F][K][2]
    Cn, F, K, _ = raw.shape
    assert len(P) >= F and P.shape[1] == Cn and np.isfinite(raw).all()
    xyl = np.ones((F, Cn, K, 3), dtype=np.float64)
    xyl[..., :2] = raw.transpose(1, 0, 2, 3)
    Qg, err, nex, _ = engine.triangulate_frames(xyl, P, engine.tri_params(THR, LIK_THR, 2))
    dq = np.abs(Qg - Q[:F]).max()
    print(f'{name}: worst |dQ| = {dq:.3e} m, worst error {err.max():.3e} px')
    assert dq <= TOL_Q
    assert (nex == 0).all() and err.max() < 1e-6


def test_device_entry_point_equals_the_host_one(engine):
    """Device memory comes from the HIP runtime directly (hipMalloc through ctypes), no torch in this process."""
    import ctypes as C
    from pose2sim_amd.engine import P2S_F32
    case = CASES[3]
    wl = workload(case)
    Cn, K, _, F = case[:4]
    prm = engine.tri_params(THR, LIK_THR, case[5])
    want = engine.triangulate_frames(wl['xyl'], wl['P'], prm)
    hip = C.CDLL('libamdhip64.so')
    hip.hipMalloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t]
    hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    hip.hipFree.argtypes = [C.c_void_p]
    n = F * K
    inputs = {'x': np.ascontiguousarray(wl['xyl']), 'P': np.ascontiguousarray(wl['P']), 'bf': np.arange(F, dtype=np.int64)}
    got = {'Q': np.full((n, 3), 7.0), 'err': np.full(n, 7.0, dtype=np.float32), 'nex': np.full(n, 7, dtype=np.uint8),
           'mask': np.full(n, 7, dtype=np.uint32)}
    d = {k: C.c_void_p() for k in (*inputs, *got)}
    try:
        for k, host in (*inputs.items(), *got.items()):
            assert hip.hipMalloc(C.byref(d[k]), host.nbytes) == 0
            assert hip.hipMemcpy(d[k], host.ctypes.data_as(C.c_void_p), host.nbytes, 1) == 0              # host -> device
        engine.triangulate_frames_device(F, Cn, d['P'].value, F, K, P2S_F32, d['x'].value, d['bf'].value, prm, d['Q'].value,
                                         d['err'].value, d['nex'].value, d['mask'].value)
        engine.synchronize()
        for k, host in got.items():
            assert hip.hipMemcpy(host.ctypes.data_as(C.c_void_p), d[k], host.nbytes, 2) == 0              # device -> host
    finally:
        for ptr in d.values():
            hip.hipFree(ptr)
    for g, w in zip(got.values(), want):
        assert np.array_equal(g.reshape(-1), w.reshape(-1), equal_nan=True)


def test_refusals_leave_the_outputs_alone(engine):
    import ctypes as C
    from pose2sim_amd import _lib
    from pose2sim_amd.engine import P2S_F32, _ptr
    F, Cn, K = 6, 4, 5
    wl = moving_rig.make_workload(F, Cn, K, seed=1)
    xyl, P = np.ascontiguousarray(wl['xyl'][:, 0]), np.ascontiguousarray(wl['P'])
    bf = np.arange(F, dtype=np.int64)
    out = {'Q': np.full((F, K, 3), 7.0), 'err': np.full((F, K), 7.0, dtype=np.float32), 'nex': np.full((F, K), 7, dtype=np.uint8),
           'mask': np.full((F, K), 7, dtype=np.uint32)}
    ok = dict(Fc=F, C=Cn, P=P, nb=F, xyl=xyl, bf=bf, prm=engine.tri_params(THR, LIK_THR, 2))

    def call(**change):
        a = {**ok, **change}
        P17 = a['P'] if a['C'] <= Cn else np.zeros((F, a['C'], 12))
        return engine._lib.p2s_triangulate_frames_host(engine._h, a['Fc'], a['C'], _ptr(P17), a['nb'], K, P2S_F32, _ptr(a['xyl']),
                                                       _ptr(a['bf']), C.byref(a['prm']), _ptr(out['Q']), _ptr(out['err']),
                                                       _ptr(out['nex']), _ptr(out['mask']))

    refusals = [
        (dict(C=1), r'n_cams=1 outside \[2, 16\]'),
        (dict(C=17), r'n_cams=17 outside \[2, 16\]'),
        (dict(prm=engine.tri_params(THR, LIK_THR, 2, undistort=True)), 'undistort_points is not supported with per-frame cameras'),
        (dict(prm=engine.tri_params(THR, LIK_THR, 2, lr_swap=True)), 'handle_lr_swap is not supported with per-frame cameras'),
        (dict(bf=np.array([0, 1, 2, 3, 4, 6], dtype=np.int64)), r'block_frame\[5\]=6 outside \[0, 6\)'),
        (dict(bf=np.array([-1, 1, 2, 3, 4, 5], dtype=np.int64)), r'block_frame\[0\]=-1 outside \[0, 6\)'),
        (dict(bf=np.array([0, 1, 3, 2, 4, 5], dtype=np.int64)), r'block_frame decreases at block 3 \(2 after 3\)'),
        (dict(Fc=0), 'n_cal_frames=0'),
        (dict(xyl=None), 'null host pointer'),
        (dict(P=None), 'null host pointer'),
        (dict(bf=None), 'null host pointer'),
    ]
    for change, text in refusals:
        rc = call(**change)
        assert rc == -1, change                                                # P2S_ERR_INVALID_ARG
        with pytest.raises(_lib.P2sError, match=text):
            _lib.check(rc)
        assert all((v == 7).all() for v in out.values()), change
    # nothing to do is no error, and launches nothing
    assert call(nb=0, xyl=None, bf=None) == 0
    assert all((v == 7).all() for v in out.values())
    # and the call as it stands is a good one
    assert call() == 0
    assert not (out['Q'] == 7).any() and not (out['nex'] == 7).any()


def test_the_stage_writes_the_per_frame_oracles_points(engine, tmp_path):
    """Pose2Sim's triangulation stage on a session with a per-frame Calib.toml: .trc frame f holds what the oracle finds
    with calibration frame f, and not what it finds with frame f + 1.  The .trc prints every coordinate as repr(), which
    loses nothing, so the file adds no error of its own and the bar is the kernel's, TOL_Q."""
    from pose2sim_amd import calib, poseio, skeletons, synth, trc, triangulation
    from pose2sim_amd import reproj_from_trc_calib as rp
    C, Fc, f0, f1 = 4, 40, 5, 35
    root = str(tmp_path / 'session')
    trial = os.path.join(root, 'trial')
    cfg = ec.base_config(trial, False, interpolation='none')
    cfg['project']['frame_range'] = [f0, f1]
    ids, names, _ = skeletons.keypoints(cfg['pose']['pose_model'], cfg)
    K = max(ids) + 1
    rig = moving_rig.make_rig(C, Fc, seed=5)
    os.makedirs(os.path.join(root, 'calibration'))
    open(os.path.join(root, 'Config.toml'), 'w').close()
    toml_path = os.path.join(root, 'calibration', 'Calib.toml')
    moving_rig.write_toml(toml_path, rig)
    P, _ = calib.frame_projections(toml_path)
    assert P.shape == (Fc, C, 3, 4) and np.abs(P - rig['P']).max() < 1e-6
    Q3d = synth.make_points3d(Fc, 1, K, seed=5)
    xyl = moving_rig.make_observations(Q3d, P, seed=5, dtype=np.float64, p_lowlik=0.0, p_outlier=0.0, p_missing_cam=0.0)
    uv = np.ascontiguousarray(xyl[:, 0, :, :, :2].transpose(1, 0, 2, 3))       # [C][F][K][2]
    cam_dirs = [os.path.join(trial, 'pose', f'cam{c + 1:02d}_json') for c in range(C)]
    for d in cam_dirs:
        os.makedirs(d)
    engine.write_openpose_files(cam_dirs, 'trial', uv)

    paths = triangulation.triangulate_all(cfg)
    assert len(paths) == 1 and paths[0].endswith(f'trial_{f0}-{f1 - 1}.trc')
    frames, _, _, markers, _ = trc.load_trc(paths[0])
    assert list(frames) == list(range(f0, f1)) and markers == list(names)
    _, _, Q_file = rp.read_markers(paths[0])

    pose_dir, json_dirs, json_files = triangulation.select_pose_inputs(trial)
    obs = poseio.load_observations(pose_dir, json_dirs, poseio.frame_file_map(json_files), (f0, f1), ids, 1)
    right = oracle_frames(obs, P, range(f0, f1), 2)
    shifted = oracle_frames(obs, P, range(f0 + 1, f1 + 1), 2)
    assert not np.isnan(right[0]).any() and not np.isnan(shifted[0]).any()
    assert np.abs(right[0] - shifted[0]).max(axis=(1, 2, 3)).min() > 1e3 * TOL_Q, 'the two expectations must be told apart'
    assert np.abs(Q_file - right[0][:, 0]).max() <= TOL_Q
    assert np.abs(Q_file - shifted[0][:, 0]).max(axis=(1, 2)).min() > 1e3 * TOL_Q
    print(json.dumps({'worst_dQ': float(np.abs(Q_file - right[0][:, 0]).max())}))


def stages_with_the_frames(size):
    """Every stage of tests/engine_reuse_cases.py at this size, with the two per-frame calls in the middle of them: the same
    observations (two persons a frame) through a rig that moves and zooms; the device call on memory of the HIP runtime's own."""
    import ctypes as C
    import engine_reuse_cases as erc
    from pose2sim_amd import synth
    from pose2sim_amd.engine import Engine, P2S_F32
    Ft, Cn, K = size[0], erc.C, erc.K
    xyl = synth.make_config(Ft, Cn, K, 2, seed=7, p_lowlik=0.1, p_outlier=0.08)['xyl']
    P_frames = np.ascontiguousarray(moving_rig.make_rig(Cn, Ft, seed=7)['P'])
    prm = Engine.tri_params(THR, LIK_THR, 2)

    def on_device(e):
        hip = C.CDLL('libamdhip64.so')
        hip.hipMalloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t]
        hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
        hip.hipFree.argtypes = [C.c_void_p]
        n = Ft * 2 * K
        inputs = {'x': np.ascontiguousarray(xyl), 'P': P_frames, 'bf': np.repeat(np.arange(Ft, dtype=np.int64), 2)}
        out = {'Q': np.empty((n, 3)), 'err': np.empty(n, dtype=np.float32), 'nex': np.empty(n, dtype=np.uint8), 'mask': np.empty(n, dtype=np.uint32)}
        d = {k: C.c_void_p() for k in (*inputs, *out)}
        try:
            for k, host in (*inputs.items(), *out.items()):
                assert hip.hipMalloc(C.byref(d[k]), host.nbytes) == 0
            for k, host in inputs.items():
                assert hip.hipMemcpy(d[k], host.ctypes.data_as(C.c_void_p), host.nbytes, 1) == 0          # host -> device
            e.triangulate_frames_device(Ft, Cn, d['P'].value, Ft * 2, K, P2S_F32, d['x'].value, d['bf'].value, prm, d['Q'].value,
                                        d['err'].value, d['nex'].value, d['mask'].value)
            e.synchronize()
            for k, host in out.items():
                assert hip.hipMemcpy(host.ctypes.data_as(C.c_void_p), d[k], host.nbytes, 2) == 0         # device -> host
        finally:
            for ptr in d.values():
                hip.hipFree(ptr)
        return tuple(out.values())

    listed = erc.stages(size)
    mine = [('triangulate_frames', lambda e: e.triangulate_frames(xyl, P_frames, prm)), ('triangulate_frames_device', on_device)]
    return listed[:len(listed) // 2] + mine + listed[len(listed) // 2:]


@pytest.fixture(scope='module')
def fresh():
    """{(size, name): result}: the two per-frame calls on an Engine of its own that has run nothing else, and once more on it;
    the other stages' fresh results are tests/test_engine_reuse_gpu.py's business, here they only fill and poison the buffers."""
    import engine_reuse_cases as erc
    out = {}
    for size in (erc.SMALL, erc.LARGE):
        for name, call in stages_with_the_frames(size):
            if name.startswith('triangulate_frames'):
                eng = erc.new_engine()
                out[size, name] = tuple(call(eng))
                again = tuple(call(eng))
                eng.close()
                assert all(np.array_equal(a, b, equal_nan=a.dtype.kind == 'f') for a, b in zip(out[size, name], again))
    return out


@pytest.mark.parametrize('poison', [None, 0xFF, 0x3F])
def test_one_engine_through_every_stage_with_the_frames_among_them(fresh, poison):
    """The run of tests/test_engine_reuse_gpu.py with the two per-frame calls as two more stages: one engine through every stage
    at the small shapes, at three times the frames (every slot, the plan and the subset table's buffer grow or are reused), at
    the small shapes again in reverse order, as the calls left the buffers and with every buffer filled with 0xFF or 0x3F
    before the call that asked for it.  The per-frame results must be those of a fresh engine, bit for bit; the host call is
    also the device call's answer."""
    import engine_reuse_cases as erc
    from pose2sim_amd.engine import Engine
    eng = erc.new_engine()
    if poison is not None:
        eng.set_tuning(Engine.TUNE_POISON_STAGING, poison)
    differing, ran = [], 0
    for rnd, (size, order) in enumerate(((erc.SMALL, 1), (erc.LARGE, 1), (erc.SMALL, -1))):
        for name, call in stages_with_the_frames(size)[::order]:
            got = tuple(call(eng))
            if not name.startswith('triangulate_frames'):
                continue
            ran += 1
            want = fresh[size, name]
            for index, (g, w) in enumerate(zip(got, want)):
                if not (g.dtype == w.dtype and g.shape == w.shape and np.array_equal(g, w, equal_nan=g.dtype.kind == 'f')):
                    differing.append((poison, rnd, name, index))
    eng.close()
    assert differing == [] and ran == 6
    for size in (erc.SMALL, erc.LARGE):
        host, device = fresh[size, 'triangulate_frames'], fresh[size, 'triangulate_frames_device']
        assert all(np.array_equal(h.reshape(-1), d.reshape(-1), equal_nan=True) for h, d in zip(host, device))
