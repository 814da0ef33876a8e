"""Body measurements without a device: the NumPy restatement (tests/measure_numpy.py) behind pose2sim_amd.measurements
reproduces every case recorded from the reference (tests/golden/measure_units.npz), the argument and marker fall-back
logic of the module, and the library's exports."""
import ctypes as C
import json
import logging
import os
import sys

import numpy as np
import pandas as pd
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import measure_numpy  # noqa: E402
from pose2sim_amd import _lib, measurements  # noqa: E402

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'measure_units.npz')
ANGLE_TOL = 1e-9            # degrees: the project's bar for values that go through libm


class Golden:
    def __init__(self):
        self.z = np.load(GOLDEN)
        meta = json.loads(bytes(self.z['meta']).decode())
        self.cases, self.trimmed = meta['cases'], meta['trimmed']
        self._frames = {}

    def text(self, trial):
        return bytes(self.z['trial_' + trial]).decode()

    def frame(self, trial):
        if trial not in self._frames:
            self._frames[trial] = measure_numpy.read_trc_text(self.text(trial))
        return self._frames[trial]

    def arr(self, i, key):
        name = f'c{i}_{key}'
        return self.z[name] if name in self.z.files else None


class Capture(logging.Handler):
    def __init__(self):
        super().__init__(level=logging.DEBUG)
        self.records = []

    def emit(self, record):
        self.records.append([record.levelname, record.getMessage()])


def same_bits(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.int64) if a.ndim else a.reshape(1).view(np.int64),
                                                  b.view(np.int64) if b.ndim else b.reshape(1).view(np.int64))


def same_numbers(a, b):
    """Bit for bit, any NaN equal to any NaN (the sign and payload of a NaN are not part of the contract)."""
    a, b = np.asarray(a, dtype=np.float64).reshape(-1), np.asarray(b, dtype=np.float64).reshape(-1)
    if a.shape != b.shape or not np.array_equal(np.isnan(a), np.isnan(b)):
        return False
    ok = ~np.isnan(a)
    return same_bits(a[ok], b[ok])


def run_case(G, i, engine, tmp_path):
    """One golden case through pose2sim_amd.measurements on `engine` -> checked against the record."""
    case = G.cases[i]
    Q_coords, markers = G.frame(case['trial'])
    kw = dict(case['kwargs'])
    func = case['func']
    cap = Capture()
    root = logging.getLogger()
    root.addHandler(cap)
    old = root.level
    root.setLevel(logging.DEBUG)
    exc, ret = '', None
    seen = {}
    real = engine.body_measure

    def spy(*a, **k):
        out = real(*a, **k)
        seen['res'] = out[0]
        return out
    engine.body_measure = spy
    try:
        if func == 'best_coords_for_measurements':
            ret = measurements.best_coords_for_measurements(Q_coords, markers, engine=engine, **kw)
        elif func == 'compute_height':
            ret = measurements.compute_height(Q_coords, markers, engine=engine, **kw)
        elif func == 'compute_leg_length':
            path = os.path.join(tmp_path, case['trial'] + '.trc')
            if not os.path.exists(path):
                with open(path, 'w') as fh:
                    fh.write(G.text(case['trial']))
            ret = measurements.compute_leg_length(path, engine=engine, **kw)
        elif func == 'mean_angles':
            ret = measurements.mean_angles(Q_coords, engine=engine)
        elif func == 'segment_lengths':
            ret = measurements.segment_lengths(Q_coords, markers, kw.pop('pairs'), engine=engine, **kw)
    except Exception as e:                                    # noqa: BLE001  the type is what is compared
        exc = type(e).__name__
    finally:
        engine.body_measure = real
        root.removeHandler(cap)
        root.setLevel(old)
    name = case['name']
    assert exc == case['exc'], f'{name}: raised {exc or "nothing"}, the reference {case["exc"] or "nothing"}'
    assert cap.records == case['logs'], f'{name}: log records differ'
    if exc:
        return
    if func == 'best_coords_for_measurements':
        assert [str(c) for c in ret.columns] == case['columns'], name
        assert np.array_equal(np.asarray(ret.index, dtype=np.int64), G.arr(i, 'index')), f'{name}: kept rows differ'
        assert measure_numpy.frame_digest(ret) == case['digest'], f'{name}: the frame differs'
        if G.arr(i, 'values') is not None:
            assert same_numbers(ret.to_numpy(), G.arr(i, 'values')), name
        res = seen['res']
        if G.arr(i, 'sum_speeds') is not None:
            assert same_bits(res['sum_speeds'], G.arr(i, 'sum_speeds')), f'{name}: speeds differ'
        if G.arr(i, 'ang_mean') is not None:
            want = G.arr(i, 'ang_mean')
            assert len(want) == res['n_selected'] and np.array_equal(np.isnan(want), np.isnan(res['angles'])), name
            d = np.abs(res['angles'] - want)
            assert not (d > ANGLE_TOL).any(), f'{name}: angles differ by {np.nanmax(d)} degrees'
    elif func == 'mean_angles':
        want = G.arr(i, 'ret')
        assert np.array_equal(np.isnan(want), np.isnan(ret)), name
        assert not (np.abs(ret - want) > ANGLE_TOL).any(), f'{name}: angles differ by {np.nanmax(np.abs(ret - want))} degrees'
    else:
        assert same_numbers(ret, G.arr(i, 'ret')), f'{name}: {ret!r} against {G.arr(i, "ret")!r}'
        if G.arr(i, 'rows') is not None:
            assert same_numbers(seen['res']['row_heights'], G.arr(i, 'rows')), f'{name}: row heights differ'


@pytest.fixture(scope='module')
def G():
    return Golden()


def test_golden_holds_the_cases_the_feature_names(G):
    assert os.path.getsize(GOLDEN) < (1 << 20)
    excs = {c['exc'] for c in G.cases}
    assert {'', 'ValueError', 'KeyError'} <= excs
    logs = {m for c in G.cases for _, m in c['logs']}
    for msg in (measurements.MSG_ALL_SLOW, measurements.MSG_ALL_DATA, measurements.MSG_NO_HEEL, measurements.MSG_NO_HEAD,
                measurements.MSG_HEIGHT_LOG, measurements.MSG_LEG_LOG, measurements.MSG_NO_ANGLES.format(45)):
        assert msg in logs, msg
    lengths = {len(G.text(t).split('\n')) - 6 for t in {c['trial'] for c in G.cases}}
    assert {1, 2, 49, 50, 51, 300, 1500} <= lengths
    assert any(np.isinf(G.arr(i, 'ret')).any() for i, c in enumerate(G.cases) if c['func'] == 'compute_height' and not c['exc'])


def test_numpy_restatement_reproduces_every_golden_case(G, tmp_path):
    engine = measure_numpy.NumpyEngine()
    for i in range(len(G.cases)):
        run_case(G, i, engine, str(tmp_path))


def test_numpy_trimmed_mean_is_the_references(G):
    for i, t in enumerate(G.trimmed):
        got = measurements.trimmed_mean(G.z[f't{i}_x'], t['p'], engine=measure_numpy.NumpyEngine())
        assert same_numbers(got, G.z[f't{i}_ret']), t


def test_duplicate_and_misplaced_names_are_refused(G):
    Q, markers = G.frame('len_2')
    engine = measure_numpy.NumpyEngine()
    twice = pd.concat((Q, Q['Nose']), axis=1)
    with pytest.raises(ValueError, match='unique'):
        measurements.compute_height(twice, markers + ['Nose'], engine=engine)
    with pytest.raises(ValueError, match='unique'):
        measurements.segment_lengths(Q, markers + ['Nose'], [('Nose', 'Hip')], engine=engine)
    with pytest.raises(ValueError, match='three columns'):
        measurements.best_coords_for_measurements(Q.iloc[:, :-1], markers, engine=engine)
    with pytest.raises(ValueError, match='unique'):
        measurements.best_coords_for_measurements(Q, [m for m in markers if m != 'Hip'], engine=engine)
    with pytest.raises(KeyError):
        measurements.best_coords_for_measurements(Q, markers + ['Tail'], engine=engine)
    with pytest.raises(ValueError, match='1-D'):
        measurements.trimmed_mean(np.zeros((2, 2)), engine=engine)
    assert np.isnan(measurements.trimmed_mean([], engine=engine))


def check_named_markers_alone_are_summed(G, engine):
    """keypoints_names may be a part of the frame's markers in another order: the speeds sum over them, in that order."""
    Q, markers = G.frame('walk_px')
    part = [m for m in markers[::-1] if not m.endswith(('Eye', 'Ear', 'Wrist'))]
    seen = {}
    real = engine.body_measure

    def spy(*a, **k):
        seen['res'] = real(*a, **k)[0]
        return [seen['res']]
    engine.body_measure = spy
    try:
        kept = measurements.best_coords_for_measurements(Q, part, close_to_zero_speed=40, engine=engine)
        height = measurements.compute_height(Q, part, close_to_zero_speed=40, engine=engine)
    finally:
        engine.body_measure = real
    speeds = measure_numpy.pandas_sum_speeds(Q, part)
    assert same_bits(seen['res']['sum_speeds'], speeds)
    assert not same_bits(speeds, measure_numpy.pandas_sum_speeds(Q, markers))
    assert list(kept.columns[:Q.shape[1]]) == list(Q.columns) and list(kept.columns[-3:]) == ['MidShoulder'] * 3
    rows = Q.to_numpy()
    assert all((rows == r).all(axis=1).any() for r in kept.to_numpy()[:, :Q.shape[1]])
    return kept, height


def test_named_markers_alone_are_summed(G):
    kept, height = check_named_markers_alone_are_summed(G, measure_numpy.NumpyEngine())
    assert 50 <= len(kept) < 150 and 600 < height < 760       # pixels at 400 a metre


def test_marker_fallbacks_choose_the_flags(G):
    P = measurements._Plan
    Q, markers = G.frame('len_2')
    full = P(Q, markers, height=True, leg=True)
    assert full.flags == (_lib.P2S_MEASURE_SPEED | _lib.P2S_MEASURE_ANGLES | _lib.P2S_MEASURE_RESTRICT | _lib.P2S_MEASURE_HEIGHT | _lib.P2S_MEASURE_LEG)
    assert full.head_factor == 1.008 and not full.add_hip and full.roles[4] == markers.index('Hip') and full.roles[5] == markers.index('Neck')
    assert full.pairs[8] == (len(markers), markers.index('Head'))

    def drop(*names):
        keep = [m for m in markers if m not in names]
        return Q[keep], keep
    p = P(*drop('Hip', 'Neck', 'Head', 'RHeel'), height=True, leg=True)
    assert p.add_hip and p.roles[4] == -1 and p.roles[5] == -1 and p.head == 'Nose' and p.head_factor == 1.5
    assert p.flags & _lib.P2S_MEASURE_FEET_CONST and p.flags & _lib.P2S_MEASURE_HEIGHT and p.pairs[0] == (-1, -1)
    p = P(*drop('LKnee'), height=True, leg=True)
    assert not p.angles_ok and not p.body_ok and not p.leg_ok
    assert p.flags == _lib.P2S_MEASURE_SPEED
    p = P(*drop('LShoulder'), height=True)
    assert isinstance(p.error, KeyError)
    p = P(Q, markers, pairs=[('Nose', 'Hip'), ('Nose', 'Tail')])
    assert isinstance(p.pair_error, ValueError) and p.pairs[9:] == [(-1, -1), (-1, -1)]


def test_measure_batch_equals_the_loop_on_the_host(G, tmp_path):
    engine = measure_numpy.NumpyEngine()
    trials = ['walk_px', 'no_rknee', 'len_1', 'no_rshoulder', 'crouch_nan_knees', 'deep_px']
    paths = []
    for t in trials:
        paths.append(os.path.join(str(tmp_path), t + '.trc'))
        with open(paths[-1], 'w') as fh:
            fh.write(G.text(t))
    speeds = [50, 0.2, 0.2, 0.2, 0.2, 50]
    pairs = [('RKnee', 'RAnkle'), ('LHip', 'LKnee')]
    batch = measurements.measure_batch(paths, pairs=pairs, engine=engine, close_to_zero_speed=speeds)
    check_batch_against_loop(batch, paths, speeds, pairs, engine)


def check_batch_against_loop(batch, paths, speeds, pairs, engine):
    from pose2sim_amd import trc

    def outcome(fn):
        try:
            return fn()
        except (ValueError, KeyError) as e:
            return e

    def same(a, b):
        return type(a) is type(b) if isinstance(a, Exception) or isinstance(b, Exception) else same_numbers(a, b)
    assert len(batch) == len(paths)
    for path, speed, got in zip(paths, speeds, batch):
        Q, _, _, markers, header = trc.read_trc(path)
        assert same(got['height'], outcome(lambda: measurements.compute_height(Q, markers, close_to_zero_speed=speed, engine=engine))), path
        assert same(got['leg_length'], outcome(lambda: measurements.compute_leg_length(path, close_to_zero_speed=speed, engine=engine))), path
        kept = outcome(lambda: measurements.best_coords_for_measurements(Q, markers, 0.1, speed, 45, engine=engine))
        seg = kept if isinstance(kept, Exception) else outcome(lambda: measurements.segment_lengths(kept, markers, pairs, engine=engine))
        assert same(got['segment_lengths'], seg), path
        assert got['units'] == header[2].split('\t')[4]
        if not isinstance(kept, Exception):
            assert len(got['frames_kept']) == len(kept)
            assert np.array_equal(Q.to_numpy()[got['frames_kept']], kept.to_numpy()[:, :Q.shape[1]], equal_nan=True)


def test_library_exports_the_measurement_entry_points():
    lib = C.CDLL(_lib.LIB_PATH)
    for name in ('p2s_stable_argsort_host', 'p2s_trimmed_means_host', 'p2s_body_measure_host', 'p2s_measure_kernel_ms'):
        assert hasattr(lib, name), name
        assert name in _lib.SIGNATURES
    header = open(os.path.join(os.path.dirname(_lib.__file__), '..', 'include', 'p2s.h')).read()
    for name, value in (('P2S_MEASURE_SPEED', _lib.P2S_MEASURE_SPEED), ('P2S_MEASURE_ANGLES', _lib.P2S_MEASURE_ANGLES),
                        ('P2S_MEASURE_RESTRICT', _lib.P2S_MEASURE_RESTRICT), ('P2S_MEASURE_FEET_CONST', _lib.P2S_MEASURE_FEET_CONST),
                        ('P2S_MEASURE_HEIGHT', _lib.P2S_MEASURE_HEIGHT), ('P2S_MEASURE_LEG', _lib.P2S_MEASURE_LEG),
                        ('P2S_MEASURE_ALL_SLOW', _lib.P2S_MEASURE_ALL_SLOW), ('P2S_MEASURE_FEW_SMALL_ANGLES', _lib.P2S_MEASURE_FEW_SMALL_ANGLES),
                        ('P2S_MEASURE_ALL_DATA', _lib.P2S_MEASURE_ALL_DATA)):
        assert f'#define {name} {value}\n' in header, name
