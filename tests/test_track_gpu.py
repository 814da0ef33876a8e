"""Person tracking across frames on the GPU (csrc/p2s_track.hip): the cases of tests/track_cases.py through a context,
every comparison exact; the refusals, the device entry point chained after p2s_triangulate_device, and the stage with and
without the kernel."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

import track_cases as tc
import track_numpy as tn
from pose2sim_amd import _lib, synth, triangulation
from pose2sim_amd.engine import P2S_F32, Engine, TrackShapeError

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def engine():
    import __graft_entry__ as entry
    entry.build_hip()
    eng = Engine(0)
    yield eng
    eng.close()


def test_recorded_single_steps(engine, golden_dir):
    tc.check_golden_steps(engine.track_persons_3d, golden_dir)


def test_generated_trials_match_the_mirror(engine):
    tc.check_generated(engine.track_persons_3d)
    assert engine.track_persons_kernel_ms() > 0.0


def test_overflow_is_reported_and_32_slots_are_not(engine):
    tc.check_overflow(engine.track_persons_3d)


def test_chunks_join_through_the_state(engine):
    tc.check_chunks(engine.track_persons_3d)


def test_ties_and_degenerate_frames(engine):
    tc.check_degenerate(engine.track_persons_3d)


def test_more_pairs_than_one_round_holds(engine):
    """COCO_133 with as many persons as the LDS takes: the distance table holds a few pairs only, so a frame's pairs go
    through it in several rounds.  The person count is found by asking: the limit is the device's."""
    P = 2
    while True:
        try:
            engine.track_persons_3d(np.zeros((1, P + 1, 133, 3)))
        except TrackShapeError:
            break
        P += 1
    assert 2 <= P < 32
    Q = tn.make_trial(10, P, 133, 0.05, seed=11)
    want = tn.replay(Q, 0, 1.0)
    assert want[3].max() > P
    got = engine.track_persons_3d(Q, first_frame=0, max_dist=1.0)
    assert not got[5].any()
    tc.assert_same_run(got, want, what='rounds')


def test_refusals_write_nothing(engine):
    lib = engine._lib
    ptr = lambda a: a.ctypes.data_as(C.c_void_p)                    # noqa: E731
    off, first = np.array([0, 1], dtype=np.int64), np.zeros(1, dtype=np.int64)
    ids, status = np.full(33, 7, dtype=np.int32), np.full(2, 7, dtype=np.int32)
    K_big = 240                                                      # with 32 persons 193 K + 1 024 doubles: 370 KB, beyond any LDS
    for P, K, text in ((0, 26, 'n_persons=0 outside [1, 32]'), (33, 26, 'n_persons=33 outside [1, 32]'), (32, K_big, None), (1, 241, None)):
        Q = np.zeros((1, max(P, 1), K, 3))
        rc = lib.p2s_track_persons_host(engine._h, 1, ptr(off), ptr(first), P, K, ptr(Q), 0, 0.0, None, None, ptr(ids), None, None, None, None, None,
                                        ptr(status))
        assert rc == _lib.P2S_ERR_INVALID_ARG, (P, K)
        message = lib.p2s_last_error().decode()
        assert message == text if text else ('bytes of LDS' in message and f'n_kpts={K}' in message), message
    assert (ids == 7).all() and (status == 7).all()
    with pytest.raises(TrackShapeError):
        engine.track_persons_3d(np.zeros((2, 32, K_big, 3)))
    with pytest.raises(TrackShapeError):
        engine.track_persons_3d_device([0, 1], 0, 33, 26, 0, d_status=0)
    assert lib.p2s_track_persons_device(None, 1, ptr(off), ptr(first), 3, 26, None, 0, 0.0, None, None, None, None, None, None, None, None,
                                        None) == _lib.P2S_ERR_INVALID_ARG and lib.p2s_last_error().decode() == 'null context'
    fresh = Engine(0)
    with pytest.raises(_lib.P2sError, match='p2s_track_persons_host has not run on this context'):
        fresh.track_persons_kernel_ms()
    fresh.close()


def test_device_entry_after_triangulate_device(engine):
    """track_persons_3d_device on the buffer triangulate_device filled: the ids of track_persons_3d on its host copy.
    Three persons on the ring rig of tests/rigs.py, 30 frames, the detection order shuffled in every frame."""
    import rigs
    F, P, Cn, K = 30, 3, 6, 26
    cams = rigs.make_rig('ring', Cn, seed=3)
    scale, offset = rigs.scene('ring')
    Q3d = synth.make_points3d(F, P, K, seed=3) * scale + offset
    Q3d += np.array([[-1.5, 0, 0], [0, 0, 0], [1.5, 0, 0]])[None, :, None, :]
    xyl = synth.make_observations(Q3d, cams, seed=3, noise_px=1.0, p_outlier=0.02)
    rng = np.random.default_rng(3)
    xyl = np.ascontiguousarray(np.stack([x[rng.permutation(P)] for x in xyl]), dtype=np.float32)
    assert xyl.shape == (F, P, Cn, K, 3)
    engine.set_calibration(synth.projection_matrices(cams))
    prm = engine.tri_params(15.0, 0.3, 2)
    Q = engine.triangulate(xyl, prm)[0]
    want = engine.track_persons_3d(Q, first_frame=0, max_dist=1.0)
    assert tn.reordered_share(want[1]) >= 0.5 and not want[5].any()
    tc.assert_same_run(want, tn.replay(Q, 0, 1.0), what='host copy')
    hip = C.CDLL('libamdhip64.so')
    hip.hipMalloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t]
    hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    hip.hipFree.argtypes = [C.c_void_p]
    n = F * P * K
    sizes = {'x': xyl.nbytes, 'Q': n * 24, 'err': n * 4, 'nex': n, 'mask': n * 4, 'ids': F * P * 4, 'rows': n * 24, 'status': 8}
    d = {k: C.c_void_p() for k in sizes}
    try:
        for k, size in sizes.items():
            assert hip.hipMalloc(C.byref(d[k]), size) == 0
        assert hip.hipMemcpy(d['x'], xyl.ctypes.data_as(C.c_void_p), xyl.nbytes, 1) == 0           # host -> device
        engine.triangulate_device(F * P, K, P2S_F32, d['x'].value, None, prm, d['Q'].value, d['err'].value, d['nex'].value, d['mask'].value)
        engine.track_persons_3d_device([0, F], 0, P, K, d['Q'].value, max_dist=1.0, d_ids=d['ids'].value, d_Q_rows=d['rows'].value,
                                       d_status=d['status'].value)
        engine.synchronize()
        ids, rows, status = np.empty((F, P), dtype=np.int32), np.empty((F, P, K, 3)), np.empty(2, dtype=np.int32)
        for host, k in ((ids, 'ids'), (rows, 'rows'), (status, 'status')):
            assert hip.hipMemcpy(host.ctypes.data_as(C.c_void_p), d[k], host.nbytes, 2) == 0      # device -> host
    finally:
        for p in d.values():
            hip.hipFree(p)
    assert not status.any() and tc.same(ids, want[1]) and tc.same(rows, want[0])


def test_stage_with_and_without_the_kernel(engine, golden_dir, tmp_path, monkeypatch, caplog):
    """A multi-person trial through triangulate_all with the kernel and with Engine.track_persons_3d refusing (the host
    loop): the same .trc bytes and the same log."""
    import ast
    import logging
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden'))
    import e2e_common as ec
    from pose2sim_amd import skeletons
    z = np.load(os.path.join(golden_dir, 'e2e_trc.npz'), allow_pickle=False)
    name = next(str(n) for n in z['cases'] if bool(z[f'{n}_multi']))
    tri = {str(k): ast.literal_eval(str(v)) for k, v in zip(z[f'{name}_tri_keys'], z[f'{name}_tri_vals'])}
    ids, _, _ = skeletons.keypoints('HALPE_26')
    cams = ec.cams_from_arrays(z, f'{name}_')
    people = ec.people_from_xyl(z[f'{name}_xyl'], ids, 26)
    calls = []
    real = Engine.track_persons_3d

    def counted(self, *args, **kwargs):
        calls.append(1)
        return real(self, *args, **kwargs)

    def refusing(self, *args, **kwargs):
        calls.append(0)
        raise NotImplementedError

    runs = []
    for how in (counted, refusing):
        monkeypatch.setattr(Engine, 'track_persons_3d', how)
        root = str(tmp_path / how.__name__)
        trial = ec.write_trial(root, 'trial_' + name, cams, people, json_subdir=str(z[f'{name}_json_subdir']))
        cfg = ec.base_config(trial, True, **tri)
        monkeypatch.chdir(root)
        caplog.clear()
        with caplog.at_level(logging.INFO):
            paths = triangulation.triangulate_all(cfg)
        texts = {os.path.basename(p): open(p, 'rb').read() for p in paths if p}
        runs.append((texts, [(r.levelno, r.getMessage().replace(root, '<root>')) for r in caplog.records]))
    assert calls == [1, 0] and len(runs[0][0]) >= 2
    assert runs[0][0] == runs[1][0]
    assert runs[0][1] == runs[1][1] and len(runs[0][1]) > 10
