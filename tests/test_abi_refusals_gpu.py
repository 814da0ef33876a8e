"""Refusals of the downstream stages' C-ABI entry points, through the raw library with a live context: the return code
and the exact p2s_last_error() text.  Every case returns before anything is launched or copied; the texts are the ones
the library has always given (callers match on some of them), written out here rather than read from its source."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

INVALID, GCV_SHORT_RUN, SYNC_PADLEN = -1, -6, -10


def P(a):
    return a.ctypes.data_as(C.c_void_p)


f8 = lambda *shape: np.ones(shape)                                  # noqa: E731
i8 = lambda *v: np.array(v, dtype=np.int64)                         # noqa: E731
B, A, ZI = np.array([0.2, 0.4, 0.2]), np.array([1.0, -0.5, 0.3]), np.array([0.8, -0.1])
A_BAD = np.array([2.0, -0.5, 0.3])
NAN_DATA = np.array([[1.0, 2.0], [np.nan, 3.0], [4.0, 5.0]])
SHORT_RUN = np.array([[1.0], [2.0], [3.0], [np.nan], [np.nan], [np.nan], [np.nan], [np.nan]])
INF_RUN = np.array([[1.0], [2.0], [np.inf], [4.0], [5.0], [6.0]])
OUT = np.empty(64)                                                  # room for any output of the cases below
IOUT = np.empty(64, dtype=np.int64)
IDS_OUT = (P(IOUT), P(IOUT), P(OUT), P(IOUT), P(OUT))                # tables, kept, distances, n_distances, stats
CONF_OUT = (P(OUT), P(IOUT), P(IOUT), P(IOUT))                      # stats, counts, below, bands
TS_OUT = (P(IOUT), P(IOUT), P(IOUT))                                # chosen, n_candidates, prev

# (entry point, arguments after the context, return code, message)
CASES = [
    ('p2s_butterworth_host', (4, 2, P(f8(4, 2)), 1, P(B), P(A), P(ZI), P(OUT)), INVALID, 'filter with 1 coefficients: supported 2..9'),
    ('p2s_butterworth_host', (4, 2, P(f8(4, 2)), 3, P(B), P(A_BAD), P(ZI), P(OUT)), INVALID, 'a[0] must be 1 (scipy.signal.butter normalises it)'),
    ('p2s_butterworth_host', (-1, 2, None, 3, P(B), P(A), P(ZI), None), INVALID, 'bad shape: n_frames=-1 n_cols=2'),
    ('p2s_filter_columns_host', (99, 4, 2, P(f8(4, 2)), P(f8(1)), 1, P(OUT)), INVALID, 'unknown column filter 99'),
    ('p2s_filter_columns_host', (1, 4, 2, P(f8(4, 2)), P(f8(2)), 2, P(OUT)), INVALID, 'Hampel filter: params = {n_sigma}'),
    ('p2s_filter_columns_host', (3, 3, 2, P(NAN_DATA), P(np.array([3.0])), 1, P(OUT)), INVALID,
     "median filter: the data hold NaN (scipy.signal.medfilt's answer for them is not defined)"),
    ('p2s_gcv_spline_host', (8, 1, P(SHORT_RUN), 1, 0.0, 1.0, P(OUT), None), GCV_SHORT_RUN, '``x`` and ``y`` length must be at least 5'),
    ('p2s_gcv_spline_host', (6, 1, P(INF_RUN), 1, 0.0, 1.0, P(OUT), None), INVALID, 'array must not contain infs or NaNs'),
    ('p2s_gcv_spline_host', (-1, 2, None, 1, 0.0, 1.0, None, None), INVALID, 'bad shape: n_frames=-1 n_cols=2'),
    ('p2s_trc_metrics_host', (2, -1, None, 0, None, None, None, None, None), INVALID, 'bad shape'),
    ('p2s_trc_metrics_host', (2, 3, P(f8(2, 3, 3)), 1, P(np.array([0, 7], dtype=np.int32)), P(OUT), P(OUT), P(OUT), P(IOUT)), INVALID,
     'bone 0 names marker 7 of 3'),
    ('p2s_sync_speeds_host', (1, P(i8(40)), 3, P(f8(40, 3)), 3, P(B), P(A), P(ZI), P(OUT)), INVALID, 'bad shape: n_cams=1 n_cols=3 (x, y pairs)'),
    ('p2s_sync_speeds_host', (1, P(i8(40)), 2, P(f8(40, 2)), 10, P(B), P(A), P(ZI), P(OUT)), INVALID, 'filter with 10 coefficients: supported 2..9'),
    ('p2s_sync_speeds_host', (1, P(i8(8)), 2, P(f8(8, 2)), 3, P(B), P(A), P(ZI), P(OUT)), SYNC_PADLEN,
     'The length of the input vector x must be greater than padlen, which is 9.'),
    ('p2s_lagged_pearson_host', (P(f8(8)), 8, 1, P(f8(8)), P(i8(8)), 5, 5, P(OUT), P(IOUT), P(OUT)), INVALID, 'empty or too large lag range [5, 5)'),
    ('p2s_lagged_pearson_host', (P(f8(8)), 8, 1, P(f8(8)), P(i8(-2)), -2, 3, P(OUT), P(IOUT), P(OUT)), INVALID, 'signal 0: bad length'),
    ('p2s_reproject_host', (5, 2, P(f8(5, 2, 3)), 2, 3, P(f8(2, 3, 12)), None, None, None, None, P(f8(2, 2)), 0, None, P(OUT)), INVALID,
     'n_frames_p=3 is neither 1 nor n_frames=5'),
    ('p2s_reproject_host', (5, 2, P(f8(5, 2, 3)), 2, 1, P(f8(2, 1, 12)), None, None, None, None, P(f8(2, 2)), 4, None, P(OUT)), INVALID, 'unknown flags 0x4'),
    ('p2s_reproject_host', (5, 2, P(f8(5, 2, 3)), 2, 5, None, P(f8(2, 9)), P(f8(2, 5)), P(f8(2, 9)), P(f8(2, 3)), P(f8(2, 2)), 1, None, P(OUT)), INVALID,
     'distorted projection takes static cameras: n_frames_p=5, expected 1'),
    ('p2s_column_order_stats_host', (4, 2, P(f8(2, 4)), -1, None, None, None), INVALID, 'bad shape: 4 rows, 2 columns, -1 ranks'),
    ('p2s_column_order_stats_host', (4, 2, None, 1, P(i8(0)), P(OUT), None), INVALID, 'null argument'),
    ('p2s_jitter_host', (1, P(i8(3)), P(f8(3, 26, 3)), 5.0, 1920.0, 1080.0) + (None,) * 7 + (8, None, None), INVALID, 'event_capacity=8 without room'),
    ('p2s_jitter_host', (0, P(i8(3)), P(f8(3, 26, 3)), 5.0, 1920.0, 1080.0) + (None,) * 7 + (0, None, None), INVALID, 'n_cams=0 outside [1, 65535]'),
    ('p2s_jitter_host', (1, P(i8(0)), P(f8(3, 26, 3)), 5.0, 1920.0, 1080.0) + (None,) * 7 + (0, None, None), INVALID,
     'camera 0 has 0 frames; expected 1 .. 2^31 - 1'),
    # p2s_id_switch_host(n_cams, n_frames, person_off, persons, tables, kept, distances, n_distances, stats)
    ('p2s_id_switch_host', (0, P(i8(1)), P(i8(0, 1)), P(f8(1, 26, 3))) + IDS_OUT, INVALID, 'n_cams=0 outside [1, 65535]'),
    ('p2s_id_switch_host', (65536, P(i8(1)), P(i8(0, 1)), P(f8(1, 26, 3))) + IDS_OUT, INVALID, 'n_cams=65536 outside [1, 65535]'),
    ('p2s_id_switch_host', (1, None, P(i8(0, 1)), P(f8(1, 26, 3))) + IDS_OUT, INVALID, 'null argument'),
    ('p2s_id_switch_host', (1, P(i8(1)), None, P(f8(1, 26, 3))) + IDS_OUT, INVALID, 'null argument'),
    ('p2s_id_switch_host', (1, P(i8(-1)), P(i8(0, 1)), P(f8(1, 26, 3))) + IDS_OUT, INVALID, 'camera 0 has -1 frames; expected 0 .. 2^31 - 1'),
    ('p2s_id_switch_host', (2, P(i8(1, 2 ** 31)), P(i8(0, 1)), P(f8(1, 26, 3))) + IDS_OUT, INVALID,
     'camera 1 has 2147483648 frames; expected 0 .. 2^31 - 1'),
    ('p2s_id_switch_host', (2, P(i8(2 ** 31 - 1, 1)), P(i8(0, 1)), P(f8(1, 26, 3))) + IDS_OUT, INVALID, '2147483648 frames are too many'),
    ('p2s_id_switch_host', (1, P(i8(1)), P(i8(1, 2)), P(f8(2, 26, 3))) + IDS_OUT, INVALID, 'person_off must start at 0'),
    ('p2s_id_switch_host', (1, P(i8(2)), P(i8(0, 2, 1)), P(f8(2, 26, 3))) + IDS_OUT, INVALID, 'person_off must not decrease (frame 1)'),
    ('p2s_id_switch_host', (1, P(i8(1)), P(i8(0, 2 ** 31)), P(f8(1, 26, 3))) + IDS_OUT, INVALID, '2147483648 persons are too many'),
    ('p2s_id_switch_host', (1, P(i8(1)), P(i8(0, 1)), None) + IDS_OUT, INVALID, 'null argument'),
    # p2s_confidence_stats_host(n_cams, n_frames, n_kpts, tables, n_thresholds, thresholds, stats, counts, below, bands)
    ('p2s_confidence_stats_host', (0, P(i8(2)), 3, P(f8(2, 3)), 1, P(f8(1))) + CONF_OUT, INVALID, 'n_cams=0 outside [1, 65535]'),
    ('p2s_confidence_stats_host', (1, P(i8(2)), 0, P(f8(2, 3)), 1, P(f8(1))) + CONF_OUT, INVALID, 'n_kpts=0 outside [1, 64]'),
    ('p2s_confidence_stats_host', (1, P(i8(2)), 65, P(f8(2, 65)), 1, P(f8(1))) + CONF_OUT, INVALID, 'n_kpts=65 outside [1, 64]'),
    ('p2s_confidence_stats_host', (1, P(i8(2)), 3, P(f8(2, 3)), -1, P(f8(1))) + CONF_OUT, INVALID, 'n_thresholds=-1 outside [0, 8]'),
    ('p2s_confidence_stats_host', (1, P(i8(2)), 3, P(f8(2, 3)), 9, P(f8(9))) + CONF_OUT, INVALID, 'n_thresholds=9 outside [0, 8]'),
    ('p2s_confidence_stats_host', (1, None, 3, P(f8(2, 3)), 1, P(f8(1))) + CONF_OUT, INVALID, 'null argument'),
    ('p2s_confidence_stats_host', (1, P(i8(2)), 3, None, 1, P(f8(1))) + CONF_OUT, INVALID, 'null argument'),
    ('p2s_confidence_stats_host', (1, P(i8(2)), 3, P(f8(2, 3)), 1, None) + CONF_OUT, INVALID, 'null argument'),
    ('p2s_confidence_stats_host', (2, P(i8(2, 0)), 3, P(f8(2, 3)), 1, P(f8(1))) + CONF_OUT, INVALID, 'camera 1 has 0 frames; expected 1 .. 2^31 - 1'),
    ('p2s_confidence_stats_host', (1, P(i8(2 ** 31)), 3, P(f8(2, 3)), 1, P(f8(1))) + CONF_OUT, INVALID,
     'camera 0 has 2147483648 frames; expected 1 .. 2^31 - 1'),
    ('p2s_confidence_stats_host', (5, P(i8(*[2 ** 31 - 1] * 5)), 1, P(f8(2, 1)), 0, None) + CONF_OUT, INVALID, '10737418235 frames are too many'),
    # p2s_column_mean_std_host(n_rows, n_cols, data, mean, std, counts)
    ('p2s_column_mean_std_host', (-1, 2, P(f8(2, 4)), P(OUT), P(OUT), P(IOUT)), INVALID, 'bad shape: -1 rows, 2 columns'),
    ('p2s_column_mean_std_host', (2 ** 31, 2, P(f8(2, 4)), P(OUT), P(OUT), P(IOUT)), INVALID, 'bad shape: 2147483648 rows, 2 columns'),
    ('p2s_column_mean_std_host', (4, -1, P(f8(2, 4)), P(OUT), P(OUT), P(IOUT)), INVALID, 'bad shape: 4 rows, -1 columns'),
    ('p2s_column_mean_std_host', (4, 2, None, P(OUT), P(OUT), P(IOUT)), INVALID, 'null argument'),
    # (new cases go at the end: a case's position is part of its test id)
    # p2s_track_select_host(n_cams, n_frames, person_off, persons, n_kpts, conf_threshold, chosen, n_candidates, prev): the frame
    # and person offsets are id_switch's, with its messages
    ('p2s_track_select_host', (0, P(i8(1)), P(i8(0, 1)), P(f8(1, 26, 3)), 26, 0.1) + TS_OUT, INVALID, 'n_cams=0 outside [1, 65535]'),
    ('p2s_track_select_host', (65536, P(i8(1)), P(i8(0, 1)), P(f8(1, 26, 3)), 26, 0.1) + TS_OUT, INVALID, 'n_cams=65536 outside [1, 65535]'),
    ('p2s_track_select_host', (1, P(i8(1)), P(i8(0, 1)), P(f8(1, 26, 3)), 0, 0.1) + TS_OUT, INVALID, 'n_kpts=0 outside [1, 127]'),
    ('p2s_track_select_host', (1, P(i8(1)), P(i8(0, 1)), P(f8(1, 128, 3)), 128, 0.1) + TS_OUT, INVALID, 'n_kpts=128 outside [1, 127]'),
    ('p2s_track_select_host', (1, None, P(i8(0, 1)), P(f8(1, 26, 3)), 26, 0.1) + TS_OUT, INVALID, 'null argument'),
    ('p2s_track_select_host', (1, P(i8(1)), None, P(f8(1, 26, 3)), 26, 0.1) + TS_OUT, INVALID, 'null argument'),
    ('p2s_track_select_host', (1, P(i8(-1)), P(i8(0, 1)), P(f8(1, 26, 3)), 26, 0.1) + TS_OUT, INVALID, 'camera 0 has -1 frames; expected 0 .. 2^31 - 1'),
    ('p2s_track_select_host', (2, P(i8(1, 2 ** 31)), P(i8(0, 1)), P(f8(1, 26, 3)), 26, 0.1) + TS_OUT, INVALID,
     'camera 1 has 2147483648 frames; expected 0 .. 2^31 - 1'),
    ('p2s_track_select_host', (2, P(i8(2 ** 31 - 1, 1)), P(i8(0, 1)), P(f8(1, 26, 3)), 26, 0.1) + TS_OUT, INVALID, '2147483648 frames are too many'),
    ('p2s_track_select_host', (1, P(i8(1)), P(i8(1, 2)), P(f8(2, 26, 3)), 26, 0.1) + TS_OUT, INVALID, 'person_off must start at 0'),
    ('p2s_track_select_host', (1, P(i8(2)), P(i8(0, 2, 1)), P(f8(2, 26, 3)), 26, 0.1) + TS_OUT, INVALID, 'person_off must not decrease (frame 1)'),
    ('p2s_track_select_host', (1, P(i8(1)), P(i8(0, 2 ** 31)), P(f8(1, 26, 3)), 26, 0.1) + TS_OUT, INVALID, '2147483648 persons are too many'),
    ('p2s_track_select_host', (1, P(i8(1)), P(i8(0, 1)), None, 26, 0.1) + TS_OUT, INVALID, 'null argument'),
]
KEEP = [B, A, ZI, A_BAD, NAN_DATA, SHORT_RUN, INF_RUN, OUT, IOUT]    # the temporaries above are kept alive by ctypes' own references


@pytest.fixture(scope='module')
def lib():
    from pose2sim_amd import _lib
    return _lib.load()


@pytest.fixture(scope='module')
def ctx(lib):
    h = C.c_void_p()
    assert lib.p2s_create(0, C.byref(h)) == 0, lib.p2s_last_error()
    yield h
    lib.p2s_destroy(h)


@pytest.mark.parametrize('name, args, code, text', CASES, ids=[f'{c[0]}-{i}' for i, c in enumerate(CASES)])
def test_refusal_with_a_live_context(lib, ctx, name, args, code, text):
    assert getattr(lib, name)(ctx, *args) == code
    assert lib.p2s_last_error().decode() == text


@pytest.mark.parametrize('name', sorted({c[0] for c in CASES}))
def test_null_context_is_refused(lib, name):
    args = next(c[1] for c in CASES if c[0] == name)
    assert getattr(lib, name)(None, *args) == INVALID
    assert lib.p2s_last_error().decode() == 'null context'


def test_lsap_refuses_a_bad_shape(lib, ctx):
    """p2s_lsap_host solves on the host without a context, by design: its refusals are the same with and without one."""
    cost, out = f8(1, 33, 33), np.empty(64, dtype=np.int32)
    for h in (ctx, None):
        for n, n_rows, n_cols in ((1, 33, 2), (1, 2, 33), (1, 0, 2), (1, 2, 0), (-1, 2, 2), (2 ** 31, 2, 2)):
            assert lib.p2s_lsap_host(h, n, n_rows, n_cols, P(cost), P(out), P(out), P(out)) == INVALID
            assert lib.p2s_last_error().decode() == f'bad shape: {n} matrices of {n_rows} x {n_cols}; expected 1 .. 32 rows and columns'
        for args in ((None, P(out), P(out), P(out)), (P(cost), None, P(out), P(out)), (P(cost), P(out), None, P(out)), (P(cost), P(out), P(out), None)):
            assert lib.p2s_lsap_host(h, 1, 2, 2, *args) == INVALID and lib.p2s_last_error().decode() == 'null argument'
        assert lib.p2s_lsap_host(h, 0, 2, 2, None, None, None, None) == 0                # no matrix: nothing to do


def test_kernel_times_refuse_until_their_own_stage_has_run(lib):
    """The seven stages that time their kernels share one pair of events; each query still answers for its own stage alone,
    and for gait and measure, which keep several entry points behind one query, any of them arms it."""
    from pose2sim_amd.engine import Engine
    P34 = np.array([[[1000.0, 0, 960, 0], [0, 1000.0, 540, 0], [0, 0, 1, 4.0]]])
    person = (np.full((2, 26, 3), 0.5), [0, 1, 2])                    # one camera of 2 frames with one person each
    filt = dict(b=[0.5, 0.5], a=[1.0, 0.0], zi=[0.5])
    table = np.arange(60.0).reshape(2, 30) % 7.0                     # 2 rows of 10 markers
    # (the query, what its refusal names, the smallest call of every entry point of that stage)
    stages = (('p2s_reproject_kernel_ms', 'p2s_reproject_host has not', (lambda e: e.reproject(np.zeros((3, 2, 3)), P=P34, sizes=np.array([[1920.0, 1080.0]])),)),
              ('p2s_jitter_kernel_ms', 'p2s_jitter_host has not', (lambda e: e.jitter([np.ones((4, 26, 3))]),)),
              ('p2s_confidence_kernel_ms', 'p2s_confidence_stats_host has not', (lambda e: e.confidence_stats([np.full((4, 26), 0.5)]),)),
              ('p2s_id_switch_kernel_ms', 'p2s_id_switch_host has not', (lambda e: e.id_switch([person]),)),
              ('p2s_gait_kernel_ms', 'neither p2s_find_peaks_host nor p2s_gait_contacts_host has',
               (lambda e: e.find_peaks(np.array([[0.0], [1.0], [0.0], [2.0], [0.0]])),
                lambda e: e.gait_contacts([np.arange(9.0)], 'height_coordinates', 1.0, 4.0, **filt))),
              ('p2s_measure_kernel_ms', 'none of p2s_stable_argsort_host, p2s_trimmed_means_host and p2s_body_measure_host has',
               (lambda e: e.stable_argsort([[2.0, 1.0, 3.0]]),
                lambda e: e.trimmed_means([[2.0, 1.0, 3.0]]),
                lambda e: e.body_measure([table], [[-1] * 10], np.zeros((1, 0, 2)), 0))),
              ('p2s_track_select_kernel_ms', 'p2s_track_select_host has not', (lambda e: e.track_select([person]),)))
    ms = C.c_float(0)
    for query, _, _ in stages:
        assert getattr(lib, query)(None, C.byref(ms)) == INVALID and lib.p2s_last_error().decode() == 'null argument'

    def refuses(eng, query, who):
        return getattr(lib, query)(eng._h, C.byref(ms)) == INVALID and lib.p2s_last_error().decode() == f'{who} run on this context'

    def answers(eng, query):
        ms.value = -1.0
        return getattr(lib, query)(eng._h, C.byref(ms)) == 0 and ms.value >= 0.0

    for first, (armed, _, runs) in enumerate(stages):
        for run_first in runs:                                       # every entry point as the first call of a fresh context
            eng = Engine(0)
            assert all(refuses(eng, query, who) for query, who, _ in stages)
            run_first(eng)
            assert answers(eng, armed)
            for query, who, _ in stages:                             # another stage's call does not count
                assert query == armed or refuses(eng, query, who), (armed, query)
            for n, (_, _, others) in enumerate(stages):              # the others one by one: what has run answers, the rest refuses
                if n != first:
                    others[-1](eng)
                done = set(range(n + 1)) | {first}
                for k, (query, who, _) in enumerate(stages):
                    assert answers(eng, query) if k in done else refuses(eng, query, who), (first, n, query)
            assert all(answers(eng, query) for query, _, _ in stages)
            eng.close()
