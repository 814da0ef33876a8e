"""The kernels of csrc/p2s_measure.hip and pose2sim_amd.measurements on the MI355X, through the C-ABI.

Engine.stable_argsort against np.argsort(kind='stable') and Engine.trimmed_means against the reference's trimmed_mean
(restated in tests/measure_numpy.py, recorded in tests/golden/measure_units.npz): bit for bit.  Every golden case through
pose2sim_amd.measurements on the device: kept rows, speeds, heights, lengths and scalars bit for bit, frames, log texts and
exception types equal, angles within 1e-9 degrees (they go through atan2; the generator keeps them 1e-6 away from the
limit and from each other where their order decides).  measure_batch against the loop over the single-file functions, a
36 000 x 26 table against the NumPy restatement, and the refusals of the entry points."""
import ctypes as C
import os

import numpy as np
import pytest

import measure_numpy
from pose2sim_amd import _lib, measurements
from test_measure_host import (ANGLE_TOL, Golden, check_batch_against_loop, check_named_markers_alone_are_summed, run_case, same_bits,
                               same_numbers)

pytestmark = pytest.mark.gpu

TILE = 1024                      # records a workgroup sorts in LDS (ST of p2s_measure.hip)
PAST_ONE_TILE = TILE + 1         # one merge round
PAST_ONE_ROUND = 2 * TILE + 1    # a second round, whose last run is a single record
LENGTHS = (1, 2, 63, 64, 65, 255, 256, 257, PAST_ONE_TILE, PAST_ONE_ROUND, 4 * TILE + 3)
FUNCS = ('best_coords_for_measurements', 'compute_height', 'compute_leg_length', 'mean_angles', 'segment_lengths')


@pytest.fixture(scope='module')
def engine():
    from pose2sim_amd.engine import Engine
    return Engine(0)


@pytest.fixture(scope='module')
def G():
    return Golden()


def key_sets(n, rng):
    tiny = np.float64(5e-324)
    sets = {'equal': np.full(n, 1.5), 'two': rng.integers(0, 2, n).astype(np.float64),
            'zeros': np.where(rng.random(n) < 0.5, 0.0, -0.0),
            'denormal': rng.integers(-3, 4, n) * tiny,
            'inf': rng.choice([-np.inf, np.inf, 0.0, 1.0], n),
            'nan': np.where(rng.random(n) < 0.3, np.nan, np.round(rng.normal(0, 1, n), 1)),
            'negative': -np.abs(np.round(rng.normal(0, 3, n), 1)),
            'mixed': rng.choice([np.nan, -np.nan, -np.inf, np.inf, -0.0, 0.0, tiny, -tiny, 1.0, -1.0, 2.5], n)}
    return sets


def test_stable_argsort_equals_numpy(engine):
    rng = np.random.default_rng(11)
    columns = [keys for n in LENGTHS for keys in key_sets(n, rng).values()]
    got = engine.stable_argsort(columns)                     # one batch of unequal lengths, length 1 included
    for keys, order in zip(columns, got):
        assert order.dtype == np.int64
        assert np.array_equal(order, np.argsort(keys, kind='stable')), (len(keys), keys[:8])
    for n in (1, PAST_ONE_TILE):                             # and a call of its own
        keys = key_sets(n, rng)['nan']
        assert np.array_equal(engine.stable_argsort([keys])[0], np.argsort(keys, kind='stable'))


def test_stable_argsort_of_a_long_column_with_ties(engine):
    rng = np.random.default_rng(12)
    walk = np.round(np.cumsum(rng.normal(0, 1, 36000)), 0)
    short = np.round(np.cumsum(rng.normal(0, 1, 5000)), 0)
    got = engine.stable_argsort([walk, np.array([3.0]), short])
    for keys, order in zip((walk, np.array([3.0]), short), got):
        assert np.array_equal(order, np.argsort(keys, kind='stable'))
    assert len(np.unique(walk)) < 2000                       # many ties


def test_trimmed_means_equal_the_references(engine, G):
    rng = np.random.default_rng(13)
    for p in (0, 0.1, 0.5, 0.999, 1.0):
        columns = [np.round(rng.normal(1.7, 0.05, n), 3) for n in LENGTHS] + [np.round(np.cumsum(rng.normal(0, 1, 36000)), 0)]
        columns += [np.array([1.0, np.inf, 2.0, 0.5]), np.array([1.0, np.nan, 2.0, 0.5, 7.0]), np.array([np.inf, -np.inf, 1.0])]
        got = engine.trimmed_means(columns, p)
        with np.errstate(all='ignore'):
            for x, mean in zip(columns, got):
                assert same_numbers(mean, measure_numpy.trimmed_mean(x, p)), (len(x), p)
        empty = [int(len(x) * (p / 2)) >= int(len(x) * (1 - p / 2)) for x in columns]
        assert any(empty) == (p > 0) and (p < 1.0 or all(empty))      # the slice that comes out empty: one entry, or p = 1
    for i, t in enumerate(G.trimmed):                        # what the reference itself returned
        assert same_numbers(measurements.trimmed_mean(G.z[f't{i}_x'], t['p'], engine=engine), G.z[f't{i}_ret']), t


@pytest.mark.parametrize('func', FUNCS)
def test_golden_cases_on_the_device(engine, G, func, tmp_path):
    mine = [i for i, c in enumerate(G.cases) if c['func'] == func]
    assert mine
    for i in mine:
        run_case(G, i, engine, str(tmp_path))


def test_measure_batch_equals_the_loop(engine, G, tmp_path):
    trials = ['walk_m', 'body_1500', 'no_rshoulder', 'len_51', 'no_rknee', 'len_1', 'stand_px']     # 300, 1 500, 51 and 1 frames
    speeds = [0.2, 0.2, 0.2, 50, 0.2, 0.2, 50]
    paths = []
    for t in trials:
        paths.append(os.path.join(str(tmp_path), t + '.trc'))
        with open(paths[-1], 'w') as fh:
            fh.write(G.text(t))
    pairs = [('RKnee', 'RAnkle'), ('LHip', 'LKnee'), ('Nose', 'RHip')]
    batch = measurements.measure_batch(paths, pairs=pairs, engine=engine, close_to_zero_speed=speeds)
    assert isinstance(batch[2]['height'], KeyError) and isinstance(batch[4]['height'], ValueError)   # two files raise in mid-batch
    assert [b['branch'] for b in batch] == ['selected', 'selected', None, 'few_small_angles', 'selected', 'few_small_angles', 'few_small_angles']
    check_batch_against_loop(batch, paths, speeds, pairs, engine)


def test_named_markers_alone_are_summed(engine, G):
    kept, height = check_named_markers_alone_are_summed(G, engine)
    want_kept, want_height = check_named_markers_alone_are_summed(G, measure_numpy.NumpyEngine())
    assert kept.equals(want_kept) and same_numbers(height, want_height)


def test_long_table_against_numpy(engine):
    rng = np.random.default_rng(14)
    names = ['Nose', 'LEye', 'REye', 'LEar', 'REar', 'LShoulder', 'RShoulder', 'LElbow', 'RElbow', 'LWrist', 'RWrist', 'LHip', 'RHip',
             'LKnee', 'RKnee', 'LAnkle', 'RAnkle', 'Head', 'Neck', 'Hip', 'LBigToe', 'RBigToe', 'LSmallToe', 'RSmallToe', 'LHeel', 'RHeel']
    n = 36000
    stand = {'Hip': (0, 0.92, 0), 'Hip_': (0, 0.92, 0.1), 'Knee_': (0.02, 0.5, 0.1), 'Ankle_': (0, 0.08, 0.1), 'Heel_': (-0.05, 0.02, 0.1),
             'BigToe_': (0.16, 0.01, 0.1), 'SmallToe_': (0.13, 0.01, 0.14), 'Neck': (0.02, 1.44, 0), 'Shoulder_': (0.02, 1.42, 0.18),
             'Elbow_': (0.02, 1.12, 0.2), 'Wrist_': (0.05, 0.86, 0.2), 'Head': (0.02, 1.7, 0), 'Nose': (0.12, 1.59, 0), 'Eye_': (0.1, 1.63, 0.03),
             'Ear_': (0.03, 1.61, 0.07)}
    rest = np.array([stand[m] if m in stand else np.array(stand[m[1:] + '_']) * (1, 1, 1 if m[0] == 'R' else -1) for m in names]).reshape(1, 78)
    sigma = 0.004 * (0.6 + 0.8 * rng.random((n, 1)))            # frames below and above close_to_zero_speed
    table = np.round(rest + 0.02 * np.cumsum(rng.normal(0, 1, (n, 78)), axis=0) / np.sqrt(np.arange(1, n + 1))[:, None]
                     + sigma * rng.normal(0, 1, (n, 78)), 3)
    table[rng.random((n, 26)).repeat(3, axis=1) < 0.01] = np.nan
    roles = [names.index(m) for m in _lib.P2S_MEASURE_ROLES]
    K = len(names)
    pairs = [(names.index(a), names.index(b)) for a, b in measurements.HEIGHT_PAIRS] + [(K, names.index('Head')), (K + 1, names.index('Nose'))]
    flags = (_lib.P2S_MEASURE_SPEED | _lib.P2S_MEASURE_ANGLES | _lib.P2S_MEASURE_RESTRICT | _lib.P2S_MEASURE_HEIGHT | _lib.P2S_MEASURE_LEG)
    kw = dict(close_to_zero_speed=0.2, fastest_frames_to_remove_percent=0.1, trimmed_extrema_percent=0.5)
    want = measure_numpy.NumpyEngine().body_measure([table], [roles], [pairs], [flags], large_hip_knee_angles=45, **kw)[0]
    ok = want['angles'][~np.isnan(want['angles'])]
    limit = round(float(np.median(ok)), 2)                   # about half of the rows pass
    while np.abs(ok - limit).min() <= 1e-6:                  # a condition on the input: the limit keeps clear of every angle
        limit += 0.01
    want = measure_numpy.NumpyEngine().body_measure([table], [roles], [pairs], [flags], large_hip_knee_angles=limit, **kw)[0]
    assert (ok < limit).sum() >= 50 and 1000 < want['n_selected'] < n and len(want['kept_frame']) < want['n_selected']
    got = engine.body_measure([table], [roles], [pairs], [flags], large_hip_knee_angles=limit, row_values=True, **kw)[0]
    print(f'measure_kernel_ms for {n} x 26: {engine.measure_kernel_ms():.3f} ms; {want["n_selected"]} rows by speed, {len(want["kept_frame"])} kept')
    assert same_bits(got['sum_speeds'], want['sum_speeds'])
    assert got['n_selected'] == want['n_selected']
    assert np.array_equal(np.isnan(got['angles']), np.isnan(want['angles']))
    assert not (np.abs(got['angles'] - want['angles']) > ANGLE_TOL).any()
    assert np.array_equal(got['kept_pos'], want['kept_pos']) and np.array_equal(got['kept_frame'], want['kept_frame'])
    assert same_numbers(got['row_values'], want['row_values']) and same_numbers(got['row_heights'], want['row_heights'])
    assert same_numbers(got['lengths'], want['lengths']) and same_numbers(got['height'], want['height']) and same_numbers(got['leg_length'], want['leg_length'])
    assert (got['all_slow'], got['few_small_angles'], got['all_data']) == (False, False, False)


def test_abi_refusals(engine):
    from pose2sim_amd.engine import Engine
    lib, h = engine._lib, engine._h
    ptr = lambda a: a.ctypes.data_as(C.c_void_p)    # noqa: E731
    ms = C.c_float(0)

    def refused(rc, text):
        assert rc == _lib.P2S_ERR_INVALID_ARG
        assert text in lib.p2s_last_error().decode(), lib.p2s_last_error()

    fresh = Engine(0)
    refused(lib.p2s_measure_kernel_ms(fresh._h, C.byref(ms)), 'has run on this context')
    fresh.close()
    refused(lib.p2s_measure_kernel_ms(None, C.byref(ms)), 'null argument')
    refused(lib.p2s_measure_kernel_ms(h, None), 'null argument')

    x = np.arange(8.0)
    lens, order, means = np.array([5, 3], dtype=np.int64), np.zeros(8, dtype=np.int32), np.zeros(2)
    sort, trim = lib.p2s_stable_argsort_host, lib.p2s_trimmed_means_host
    refused(sort(None, 2, ptr(lens), ptr(x), ptr(order)), 'null context')
    refused(sort(h, 0, ptr(lens), ptr(x), ptr(order)), 'segments')
    refused(sort(h, (1 << 21) + 1, ptr(lens), ptr(x), ptr(order)), 'segments; expected 1 .. 2^21')
    refused(trim(h, (1 << 21) + 1, ptr(lens), ptr(x), 0.25, ptr(means)), 'segments; expected 1 .. 2^21')
    refused(sort(h, 2, None, ptr(x), ptr(order)), 'null argument')
    refused(sort(h, 2, ptr(lens), None, ptr(order)), 'null argument')
    refused(sort(h, 2, ptr(lens), ptr(x), None), 'null argument')
    refused(sort(h, 2, ptr(np.array([5, 0], dtype=np.int64)), ptr(x), ptr(order)), 'segment 1 has 0 rows')
    refused(sort(h, 2, ptr(np.array([1 << 31, 3], dtype=np.int64)), ptr(x), ptr(order)), 'segment 0 has 2147483648 rows')
    refused(trim(None, 2, ptr(lens), ptr(x), 0.25, ptr(means)), 'null context')
    refused(trim(h, 2, ptr(lens), ptr(x), 0.25, None), 'null argument')
    refused(trim(h, 2, ptr(np.array([-1, 3], dtype=np.int64)), ptr(x), 0.25, ptr(means)), 'segment 0 has -1 rows')
    for bad in (-0.01, 0.51, float('nan')):
        refused(trim(h, 2, ptr(lens), ptr(x), bad, ptr(means)), 'half_trim')
    assert sort(h, 2, ptr(lens), ptr(x), ptr(order)) == 0 and order.tolist() == [0, 1, 2, 3, 4, 0, 1, 2]
    assert lib.p2s_measure_kernel_ms(h, C.byref(ms)) == 0 and ms.value >= 0.0

    K, n = 12, 6
    table = np.random.default_rng(1).normal(0, 1, (n, 3 * K))
    rows, mk = np.array([n], dtype=np.int64), np.array([K], dtype=np.int32)
    roles = np.arange(10, dtype=np.int32).reshape(1, 10)
    pairs = np.array([[i, i + 1] for i in range(9)], dtype=np.int32).reshape(1, 9, 2)
    head, thr = np.array([1.008]), np.array([0.2])
    every = np.array([_lib.P2S_MEASURE_SPEED | _lib.P2S_MEASURE_ANGLES | _lib.P2S_MEASURE_RESTRICT | _lib.P2S_MEASURE_HEIGHT | _lib.P2S_MEASURE_LEG], dtype=np.int32)
    i32 = lambda: np.zeros(n, dtype=np.int32)    # noqa: E731
    out = dict(speeds=np.zeros(n), angles=np.zeros(n), n_sel=i32(), pos=i32(), frame=i32(), n_kept=i32(), branch=i32(), heights=np.zeros(n),
               means=np.zeros(11))

    def call(ctx=h, n_files=1, n_rows=rows, n_mk=mk, data=table, flags=every, roles=roles, n_pairs=9, pairs=pairs, head=head, thr=thr,
             n_speed=None, keep=0.9, limit=45.0, half=0.25, means=out['means'], n_kept=out['n_kept']):
        p = lambda a: None if a is None else ptr(a)    # noqa: E731
        return lib.p2s_body_measure_host(ctx, n_files, p(n_rows), p(n_mk), p(data), p(flags), p(roles), n_pairs, p(pairs), p(head), p(thr),
                                         p(n_speed), keep, limit, half, ptr(out['speeds']), ptr(out['angles']), ptr(out['n_sel']), ptr(out['pos']),
                                         ptr(out['frame']), p(n_kept), ptr(out['branch']), ptr(out['heights']), None, p(means))

    def i32a(v):
        return np.array(v, dtype=np.int32)

    refused(call(ctx=None), 'null context')
    refused(call(n_files=0), 'bad shape')
    refused(call(n_pairs=-1), 'bad shape')
    refused(call(n_pairs=1025), 'bad shape')
    for name in ('n_rows', 'n_mk', 'data', 'flags', 'roles', 'pairs', 'head', 'thr', 'means', 'n_kept'):
        refused(call(**{name: None}), 'null argument')
    refused(call(n_rows=np.array([0], dtype=np.int64)), 'segment 0 has 0 rows')
    refused(call(n_rows=np.array([1 << 31], dtype=np.int64)), 'segment 0 has 2147483648 rows')
    refused(call(n_mk=i32a([0])), 'markers')
    refused(call(flags=i32a([64])), 'unknown flags')
    refused(call(flags=i32a([_lib.P2S_MEASURE_RESTRICT])), 'without P2S_MEASURE_ANGLES')
    bad_roles = roles.copy()
    bad_roles[0, 3] = K
    refused(call(roles=bad_roles), 'out of range')
    bad_roles[0, 3] = -2
    refused(call(roles=bad_roles), 'out of range')
    bad_roles[0, 3] = -1
    refused(call(roles=bad_roles), 'the angles need role 3')
    bad_pairs = pairs.copy()
    bad_pairs[0, 4, 1] = K + 2
    refused(call(pairs=bad_pairs), 'out of range')
    bad_pairs[0, 4, 1] = -2
    refused(call(pairs=bad_pairs), 'out of range')
    bad_pairs[0, 4, 1] = -1
    refused(call(pairs=bad_pairs), 'pair 4 is needed')
    bad_pairs[0, 4, 1] = K + 1
    refused(call(pairs=bad_pairs, roles=bad_roles, flags=i32a([0])), 'midpoint')
    refused(call(n_pairs=8), 'need the first 9 pairs')
    refused(call(n_speed=i32a([K + 1])), 'speed markers out of range')
    refused(call(n_speed=i32a([-1])), 'speed markers out of range')
    for bad in (-0.1, 1.1, float('nan')):
        refused(call(keep=bad), 'keep_fraction')
    for bad in (-0.1, 0.6, float('nan')):
        refused(call(half=bad), 'half_trim')
    refused(call(limit=float('nan')), 'angle_limit')
    refused(call(thr=np.array([np.nan])), 'NaN speed threshold')
    assert call() == 0 and 1 <= out['n_kept'][0] <= n
