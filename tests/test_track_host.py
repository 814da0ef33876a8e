"""Person tracking across frames, csrc/p2s_track.hip compiled for the host: p2s_track_persons_host without a context runs
the functions the kernel runs, so the restatement of the reference's loop (triangulation.py:823-874, common.py:1037-1136)
is checked here against NumPy and scipy bit for bit, without a GPU.  The cases are tests/track_cases.py's."""
import ctypes
import os

import numpy as np
import pytest

import track_cases as tc
import track_numpy as tn
from pose2sim_amd import _lib, engine, triangulation

run = engine.track_persons_3d_host


def test_recorded_single_steps(golden_dir):
    tc.check_golden_steps(run, golden_dir)


def test_generated_trials_match_the_mirror():
    tc.check_generated(run)


def test_overflow_is_reported_and_32_slots_are_not():
    tc.check_overflow(run)


def test_chunks_join_through_the_state():
    tc.check_chunks(run)


def test_ties_and_degenerate_frames():
    tc.check_degenerate(run)


def test_host_path_refuses_bad_shapes():
    """Without a context there is no LDS limit: only the person count and the layout are refused, and nothing is written."""
    lib = _lib.load()
    ptr = lambda a: a.ctypes.data_as(ctypes.c_void_p)                # noqa: E731
    off, first, Q = np.array([0, 1], dtype=np.int64), np.zeros(1, dtype=np.int64), np.zeros((1, 33, 2, 3))
    ids, status = np.full(33, 7, dtype=np.int32), np.full(2, 7, dtype=np.int32)

    def call(T, off, P, K, status_ptr=None):
        return lib.p2s_track_persons_host(None, T, ptr(off), ptr(first), P, K, ptr(Q), 0, 0.0, None, None, ptr(ids), None, None, None,
                                          None, None, ptr(status) if status_ptr is None else status_ptr)
    for P in (0, 33, -1):
        assert call(1, off, P, 2) == _lib.P2S_ERR_INVALID_ARG
        assert lib.p2s_last_error().decode() == f'n_persons={P} outside [1, 32]'
    assert call(1, off, 3, 0) == _lib.P2S_ERR_INVALID_ARG and lib.p2s_last_error().decode() == 'n_kpts=0 outside [1, 2^20]'
    assert call(-1, off, 3, 2) == _lib.P2S_ERR_INVALID_ARG
    assert call(1, np.array([1, 2], dtype=np.int64), 3, 2) == _lib.P2S_ERR_INVALID_ARG and lib.p2s_last_error().decode() == 'frame_off must start at 0'
    assert call(2, np.array([0, 2, 1], dtype=np.int64), 3, 2) == _lib.P2S_ERR_INVALID_ARG
    assert lib.p2s_last_error().decode() == 'frame_off must not decrease (trial 1)'
    assert call(1, off, 3, 2, status_ptr=ctypes.c_void_p()) == _lib.P2S_ERR_INVALID_ARG and lib.p2s_last_error().decode() == 'null argument'
    assert (ids == 7).all() and (status == 7).all()
    with pytest.raises(engine.TrackShapeError):
        run(np.zeros((2, 33, 2, 3)))
    n_in, state = np.array([33], dtype=np.int32), np.zeros((1, 32, 2, 3))      # a state of more than 32 rows cannot come from a call
    rc = lib.p2s_track_persons_host(None, 1, ptr(off), ptr(first), 3, 2, ptr(Q), 0, 0.0, ptr(state), ptr(n_in), None, None, None, None,
                                    None, None, ptr(status))
    assert rc == _lib.P2S_ERR_INVALID_ARG and lib.p2s_last_error().decode() == 'trial 0 starts with 33 slots; expected 0 .. 32'
    assert (status == 7).all()


def test_the_stage_falls_back_to_the_host_loop():
    """triangulation.track_persons_engine: the engine's answer when it has one, the host loop's otherwise -- the same arrays."""
    Q, max_dist, want = tc.generated(3, 5)
    over, over_dist, _ = tc.generated(-1, 0)

    class HostEngine:
        calls = 0

        def track_persons_3d(self, Q, first_frame=0, max_dist=None, state=None):
            HostEngine.calls += 1
            return run(Q, first_frame, max_dist, state)

    class OldEngine:
        def track_persons_3d(self, *args, **kwargs):
            raise NotImplementedError

    class SmallEngine:
        def track_persons_3d(self, *args, **kwargs):
            raise engine.TrackShapeError('does not fit')

    host = triangulation.track_persons(Q, (5, 5 + len(Q)), True, max_dist)
    for eng in (HostEngine(), OldEngine(), SmallEngine(), object()):
        rows, ids = triangulation.track_persons_engine(eng, Q, (5, 5 + len(Q)), True, max_dist)
        assert tc.same(rows, host[0]) and tc.same(ids, host[1]) and ids.dtype == host[1].dtype
    assert HostEngine.calls == 1
    # more than 32 slots: the status sends the stage to the host loop, which has no limit
    host = triangulation.track_persons(over, (0, len(over)), True, over_dist)
    rows, ids = triangulation.track_persons_engine(HostEngine(), over, (0, len(over)), True, over_dist)
    assert HostEngine.calls == 2 and tc.same(rows, host[0]) and tc.same(ids, host[1])
    # single-person trials never reach the engine
    rows, ids = triangulation.track_persons_engine(HostEngine(), Q, (5, 5 + len(Q)), False, max_dist)
    assert HostEngine.calls == 2 and rows is Q


def test_engine_without_the_entries_refuses():
    class Old:
        pass
    eng = engine.Engine.__new__(engine.Engine)
    eng._lib, eng._h = Old(), None
    with pytest.raises(NotImplementedError):
        eng.track_persons_3d(np.zeros((1, 2, 3, 3)))
    with pytest.raises(NotImplementedError):
        eng.track_persons_3d_device([0, 1], 0, 2, 3, 0, d_status=0)
    with pytest.raises(NotImplementedError):
        eng.track_persons_kernel_ms()


def test_new_entries_are_declared_exported_and_optional():
    new = {'p2s_track_persons_host', 'p2s_track_persons_device', 'p2s_track_persons_kernel_ms'}
    assert new <= _lib.OPTIONAL and new <= set(_lib.SIGNATURES)
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    header = open(os.path.join(root, 'include', 'p2s.h')).read()
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name in new:
        assert f'int {name}(' in header and hasattr(lib, name), name
    assert _lib.P2S_TRACK_MAX_SLOTS == _lib.P2S_LSAP_MAX == 32 and tn.OVERFLOW[1] <= 32
