"""The kernels of csrc/p2s_gait.hip and pose2sim_amd.trc_gaitevents on the MI355X, through the C-ABI.

Engine.find_peaks against the scipy results recorded in tests/golden/gait_units.npz: bit for bit.  Engine.gait_contacts
against scipy's filtfilt / gaussian_filter1d on the same column (tests/gait_scipy.py): 1e-9 relative to max(1, |value|),
the bar of tests/test_filter_gpu.py for the same recurrences; its runs against start_end_true_seq on scipy's signal for
the golden trials, whose samples the generator keeps 1e-6 away from the threshold.  The utility end to end against what
the reference returned, printed and wrote.

A NaN sample and the forward_velocity signal: the reference's `where(speed > 0, other=0)` turns a NaN speed into 0 before
the Gaussian, so the filtered signal holds no NaN; the test compares with that, scipy and pandas on the same column."""
import ctypes as C

import numpy as np
import pytest
from scipy import signal

import gait_scipy as gs
from pose2sim_amd import _lib
from pose2sim_amd import trc as p2s_trc
from pose2sim_amd import trc_gaitevents as tg
from test_gait_host import BAD, BY_NAME, ERRORS, G, GOOD, same_result

pytestmark = pytest.mark.gpu

FP_NAMES = [str(n) for n in G['fp_names']]
REL = 1e-9


@pytest.fixture(scope='module')
def engine():
    from pose2sim_amd.engine import Engine
    return Engine(0)


def same_floats(got, want):
    """Equal values, NaN where the other has NaN, the same sign on zeros."""
    got, want = np.asarray(got), np.asarray(want)
    return got.shape == want.shape and np.array_equal(got, want, equal_nan=True) and np.array_equal(np.signbit(got[got == 0]), np.signbit(want[want == 0]))


def recorded(name, key):
    counts = G[f'fp_{name}_{key}_counts']
    off = np.concatenate([[0], np.cumsum(counts)])
    parts = [G[f'fp_{name}_{key}_{f}'] for f in ('peaks', 'prom', 'lb', 'rb')]
    return [tuple(p[off[c]:off[c + 1]] for p in parts) for c in range(len(counts))]


def check_columns(got, want, tag):
    assert len(got) == len(want), tag
    for c, (g, w) in enumerate(zip(got, want)):
        assert g[0].dtype == np.int64 and np.array_equal(g[0], w[0]), (tag, c, 'peaks', g[0], w[0])
        assert same_floats(g[1], w[1]), (tag, c, 'prominences', g[1], w[1])
        assert np.array_equal(g[2], w[2]), (tag, c, 'left bases', g[2], w[2])
        assert np.array_equal(g[3], w[3]), (tag, c, 'right bases', g[3], w[3])


@pytest.mark.parametrize('key', ['none', 'zero', 'mid', 'inf'])
@pytest.mark.parametrize('name', FP_NAMES)
def test_find_peaks_equals_scipy(engine, name, key):
    x = G[f'fp_{name}_x']
    p = {'none': None, 'zero': 0, 'mid': float(G[f'fp_{name}_mid']), 'inf': np.inf}[key]
    want = recorded(name, key)
    if key == 'inf' and not np.isinf(x).any():                       # only a peak of infinite prominence passes inf <= prominence
        assert all(len(w[0]) == 0 for w in want)
    check_columns(engine.find_peaks(x, prominence=p), want, (name, key))


def test_find_peaks_takes_strided_tables_and_a_bound_per_column(engine):
    x = G['fp_wide_x']
    bounds = np.where(np.arange(x.shape[1]) % 2 == 0, 0.0, float(G['fp_wide_mid']))
    want = [w for pair in zip(recorded('wide', 'zero')[::2], recorded('wide', 'mid')[1::2]) for w in pair] + [recorded('wide', 'zero')[64]]
    check_columns(engine.find_peaks(np.asfortranarray(x), prominence=bounds), want, 'per column')
    check_columns(engine.find_peaks(x[::-1][::-1][:, ::3], prominence=0), recorded('wide', 'zero')[::3], 'strided')


def test_find_peaks_past_one_round_of_the_tile_scan(engine, capsys):
    """36 000 x 9 samples: 1 266 tiles, more than the 1 024 the scan takes a round; columns of plateaus, a rising
    sawtooth (every left scan runs to the column's start over the block summaries) and smooth waves."""
    rng = np.random.default_rng(5)
    n = 36000
    x = np.round(np.cumsum(rng.normal(0, 1, (n, 9)), axis=0), 1)
    x[:, 7] = np.arange(n) + 10.0 * (np.arange(n) % 2)
    x[:, 8] = np.sin(np.arange(n) / 300.0) + 0.01 * np.sin(np.arange(n) / 3.0)
    got = engine.find_peaks(x, prominence=0.5)
    ms = engine.gait_kernel_ms()
    with capsys.disabled():
        print(f'find_peaks {n} x 9: {sum(len(g[0]) for g in got)} peaks kept, kernels {ms:.3f} ms')
    check_columns(got, [gs.peaks_of_column(x[:, c], 0.5) for c in range(9)], 'large')


def test_find_peaks_capacity_protocol(engine):
    """The first call too small, through the C ABI: the total and the counts are right, the first `capacity` peaks are
    written, and nothing past them."""
    lib = _lib.load()
    x = G['fp_wide_x']
    cols = np.ascontiguousarray(x.T)
    want = recorded('wide', 'none')
    total = sum(len(w[0]) for w in want)
    ptr = lambda a: a.ctypes.data_as(C.c_void_p)    # noqa: E731
    counts, found = np.zeros(x.shape[1], dtype=np.int32), C.c_int64(-1)
    assert lib.p2s_find_peaks_host(engine._h, x.shape[0], x.shape[1], ptr(cols), None, 0, None, None, None, None, ptr(counts), C.byref(found)) == 0
    assert found.value == total and np.array_equal(counts, [len(w[0]) for w in want])
    cap = 100
    peaks, lb, rb = (np.full(cap + 8, -7, dtype=np.int64) for _ in range(3))
    prom = np.full(cap + 8, -7.0)
    counts[:] = 0
    assert lib.p2s_find_peaks_host(engine._h, x.shape[0], x.shape[1], ptr(cols), None, cap, ptr(peaks), ptr(prom), ptr(lb), ptr(rb),
                                   ptr(counts), C.byref(found)) == 0
    assert found.value == total > cap and np.array_equal(counts, [len(w[0]) for w in want])
    flat = [np.concatenate([w[k] for w in want]) for k in range(4)]
    assert np.array_equal(peaks[:cap], flat[0][:cap]) and same_floats(prom[:cap], flat[1][:cap])
    assert np.array_equal(lb[:cap], flat[2][:cap]) and np.array_equal(rb[:cap], flat[3][:cap])
    assert (peaks[cap:] == -7).all() and (prom[cap:] == -7.0).all() and (lb[cap:] == -7).all() and (rb[cap:] == -7).all()
    # Engine.find_peaks repeats the call by itself: 'wide' holds more peaks than its first capacity of 45500 / 16
    assert total > x.size // 16


# ---- contact signals ------------------------------------------------------------------------------------------------------
def butter_for(dt, cutoff=10):
    b, a = signal.butter(4 / 2, cutoff * dt * 2, 'low', analog=False)
    return b, a, signal.lfilter_zi(b, a)


def close(got, want):
    got, want = np.asarray(got), np.asarray(want)
    if got.shape != want.shape or not np.array_equal(np.isnan(got), np.isnan(want)):
        return False
    ok = ~np.isnan(want)
    fin = ok & np.isfinite(want)
    return np.array_equal(got[ok & ~fin], want[ok & ~fin]) and bool(np.all(np.abs(got[fin] - want[fin]) <= REL * np.maximum(1.0, np.abs(want[fin]))))


def toe_like(n, seed):
    rng = np.random.default_rng(seed)
    t = np.arange(n) / 60.0
    return 0.03 + 0.1 * np.sin(2 * np.pi * t / 1.1 + seed) ** 2 + 0.5 * t * (seed % 3) + rng.normal(0, 0.003, n)


def check_runs(sig_ref, thr, on, off, first, tag):
    low = sig_ref < thr
    assert first == bool(len(low) and low[0]), tag
    if len(low) == 0 or low.all():
        assert len(on) == 0 and len(off) == 0, tag
        return
    want_on, want_off = gs.runs_of(sig_ref, thr)
    assert on.tolist() == want_on and off.tolist() == want_off, (tag, on, want_on, off, want_off)


def test_height_signal_on_short_and_unequal_columns(engine):
    dt = 1 / 60
    b, a, zi = butter_for(dt)
    lens = [11, 12, 11, 300, 77, 12]                                   # 10 after the drop: the shortest filtfilt takes at order 2
    cols = [toe_like(n, s) for s, n in enumerate(lens)]
    cols[4][20] = 0.0                                                   # a zero is data
    thr = [6.0, 6.0, 4.0, 6.0, 8.0, 100.0]
    sigs, on, off, first = engine.gait_contacts(cols, 'height_coordinates', dt=dt, threshold=thr, factor=100.0, b=b, a=a, zi=zi)
    for c, col in enumerate(cols):
        want = gs.contact_signal(col, 'height_coordinates', dt, 100.0, b=b, a=a)
        assert len(sigs[c]) == lens[c] - 1 and close(sigs[c], want), (c, np.abs(sigs[c] - want).max())
        check_runs(want, thr[c], on[c], off[c], first[c], c)
    assert first[5] and len(off[5]) == 0                                # all below: what start_end_true_seq raises on
    with pytest.raises(ValueError, match='greater than padlen, which is 9'):
        engine.gait_contacts([toe_like(10, 1), toe_like(40, 2)], 'height_coordinates', dt=dt, threshold=6.0, b=b, a=a, zi=zi)


def test_height_signal_with_a_nan_is_all_nan(engine):
    dt = 1 / 60
    b, a, zi = butter_for(dt)
    cols = [toe_like(120, 3), toe_like(120, 4)]
    cols[0][60] = np.nan
    sigs, on, off, first = engine.gait_contacts(cols, 'height_coordinates', dt=dt, threshold=6.0, factor=100.0, b=b, a=a, zi=zi)
    assert np.isnan(sigs[0]).all() and len(on[0]) == 0 and len(off[0]) == 0 and not first[0]
    assert np.isnan(gs.contact_signal(cols[0], 'height_coordinates', dt, 100.0, b=b, a=a)).all()
    assert close(sigs[1], gs.contact_signal(cols[1], 'height_coordinates', dt, 100.0, b=b, a=a))


@pytest.mark.parametrize('sign', [1, -1])
def test_velocity_signal_on_short_and_unequal_columns(engine, sign):
    lens = [2, 4, 21, 22, 42, 300, 2, 130]                             # 1, 3, 20, 21, 41 after the drop: radius 20 reflects
    cols = [sign * np.cumsum(np.abs(toe_like(n, s))) * (1 + s) for s, n in enumerate(lens)]   # more than once on the short ones
    cols[5][::7] -= sign * 0.3                                          # steps against the direction: zeroed
    cols[7][60] = np.nan                                                # NaN speeds become 0, as pandas' where makes them
    dts = np.array([1 / 60, 1 / 50, 1 / 60, 1 / 100, 1 / 60, 1 / 120, 1 / 60, 1 / 60])
    thr = np.array([1.0, 2.0, 5.0, 20.0, 8.0, 30.0, 1e9, 12.0])
    fac = np.array([1.0, 10.0, 1.0, 1.0, 1.0, 1.0, 1.0, 1.0])
    sigs, on, off, first = engine.gait_contacts(cols, 'forward_velocity', dt=dts, threshold=thr, factor=fac, sign=sign, weights=tg.gaussian_weights())
    for c, col in enumerate(cols):
        want = gs.contact_signal(col, 'forward_velocity', dts[c], fac[c], sign=sign)
        assert len(sigs[c]) == lens[c] - 1 and close(sigs[c], want), (c, sigs[c], want)
        check_runs(want, thr[c], on[c], off[c], first[c], c)
    assert not np.isnan(sigs[7]).any()
    assert first[6] and len(off[6]) == 0


THRESHOLD_CASES = [n for n in GOOD if BY_NAME[n]['args'].get('method', 'height_coordinates') != 'forward_coordinates']


@pytest.mark.parametrize('name', THRESHOLD_CASES)
def test_runs_of_the_golden_trials_equal_start_end_true_seq(engine, name, tmp_path):
    case = BY_NAME[name]
    cfg = tg.resolve_args(dict(case['args'], trc_path=gs.write_trial(G, case['trial'], tmp_path)))
    prep = tg._prepare(cfg, cfg['trc_path'])
    kw = dict(dt=prep['dt'], threshold=prep['threshold'], factor=prep['factor'])
    if cfg['method'] == 'height_coordinates':
        b, a, zi = prep['filter']
        sigs, on, off, first = engine.gait_contacts(prep['columns'], cfg['method'], b=b, a=a, zi=zi, **kw)
    else:
        b = a = None
        sigs, on, off, first = engine.gait_contacts(prep['columns'], cfg['method'], sign=prep['sign'], weights=tg.gaussian_weights(), **kw)
    for c, col in enumerate(prep['columns']):
        want = gs.contact_signal(col, cfg['method'], prep['dt'], prep['factor'], sign=prep['sign'], b=b, a=a)
        assert close(sigs[c], want), (c, np.abs(sigs[c] - want).max())
        assert np.abs(want - prep['threshold']).min() > 1e-6 * max(1.0, abs(prep['threshold']))     # the generator's margin
        check_runs(want, prep['threshold'], on[c], off[c], first[c], c)


# ---- the utility ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', GOOD + BAD)
def test_utility_reproduces_the_reference(engine, name, tmp_path, capsys):
    case = BY_NAME[name]
    path = gs.write_trial(G, case['trial'], tmp_path)
    args = dict(case['args'], trc_path=path, plot=False, engine=engine)
    if case['error']:
        with pytest.raises(ERRORS[case['error']]) as info:
            tg.trc_gaitevents_func(**args)
        assert type(info.value) is ERRORS[case['error']]
        assert not (tmp_path / 'gaitevents.txt').exists()
    else:
        assert same_result(tg.trc_gaitevents_func(**args), case['result'])
        assert open(tmp_path / 'gaitevents.txt', 'rb').read() == case['file'].encode()
    assert capsys.readouterr().out == case['console']


@pytest.mark.parametrize('method', tg.METHODS)
def test_batch_equals_the_loop(engine, method, tmp_path, capsys):
    """Files of unequal length (300, 400, 300 and 200 frames) in one device call; the last one raises, after the reports
    of the others."""
    trials = ['walk_m', 'walk_noisy', 'walk_m', 'stand']
    cases = [BY_NAME[f'{t}-{method}-gait'] for t in trials[:3]] + [BY_NAME[next(n for n in BAD if n.startswith(f'stand-{method}'))]]
    paths = [gs.write_trial(G, t, tmp_path) for t in trials]
    args = dict(cases[0]['args'], engine=engine, plot=False)
    res = tg.trc_gaitevents_batch(paths[:3], **args)
    assert len(res) == 3 and all(same_result(r, c['result']) for r, c in zip(res, cases))
    assert capsys.readouterr().out == ''.join(c['console'] for c in cases[:3])
    assert open(tmp_path / 'gaitevents.txt').read() == ''.join(c['file'] for c in cases[:3])
    (tmp_path / 'gaitevents.txt').unlink()
    one = tg.trc_gaitevents_batch(paths[1:2], **args)                   # a batch of one file
    assert len(one) == 1 and same_result(one[0], cases[1]['result'])
    assert open(tmp_path / 'gaitevents.txt').read() == cases[1]['file']
    (tmp_path / 'gaitevents.txt').unlink()
    capsys.readouterr()
    with pytest.raises(IndexError):                                     # the second file raises
        tg.trc_gaitevents_batch([paths[0], paths[3], paths[1]], **args)
    motion = cases[3]['args']['motion_type']
    assert capsys.readouterr().out == cases[0]['console'] + cases[3]['console'].replace(f'Motion type: {motion}', 'Motion type: gait')
    assert open(tmp_path / 'gaitevents.txt').read() == cases[0]['file']


def test_time_column_is_the_one_pandas_parses(tmp_path):
    path = gs.write_trial(G, 'walk_mm', tmp_path)
    import pandas as pd
    want = pd.read_csv(path, sep='\t', skiprows=4, encoding='utf-8').iloc[:, 1]
    assert np.array_equal(p2s_trc.read_trc(path)[2].to_numpy(), want.to_numpy())


# ---- refusals: arguments the entry points reject before any launch -------------------------------------------------------------
def test_abi_refusals(engine):
    lib = _lib.load()
    h = engine._h
    ptr = lambda a: a.ctypes.data_as(C.c_void_p)    # noqa: E731
    x = np.zeros((4, 8))
    counts, found = np.zeros(4, dtype=np.int32), C.c_int64(0)
    out = np.zeros(16, dtype=np.int64)
    prom = np.zeros(16)

    def refused(rc, text):
        assert rc == _lib.P2S_ERR_INVALID_ARG
        assert text in lib.p2s_last_error().decode(), lib.p2s_last_error()

    fp = lib.p2s_find_peaks_host
    refused(fp(None, 8, 4, ptr(x), None, 0, None, None, None, None, ptr(counts), C.byref(found)), 'null context')
    refused(fp(h, 0, 4, ptr(x), None, 0, None, None, None, None, ptr(counts), C.byref(found)), 'bad shape')
    refused(fp(h, -1, 4, ptr(x), None, 0, None, None, None, None, ptr(counts), C.byref(found)), 'bad shape')
    refused(fp(h, 8, 0, ptr(x), None, 0, None, None, None, None, ptr(counts), C.byref(found)), 'bad shape')
    refused(fp(h, 1 << 31, 1, ptr(x), None, 0, None, None, None, None, ptr(counts), C.byref(found)), 'bad shape')
    refused(fp(h, 8, 4, None, None, 0, None, None, None, None, ptr(counts), C.byref(found)), 'null argument')
    refused(fp(h, 8, 4, ptr(x), None, 0, None, None, None, None, None, C.byref(found)), 'null argument')
    refused(fp(h, 8, 4, ptr(x), None, 0, None, None, None, None, ptr(counts), None), 'null argument')
    refused(fp(h, 8, 4, ptr(x), None, -1, ptr(out), ptr(prom), ptr(out), ptr(out), ptr(counts), C.byref(found)), 'without room')
    refused(fp(h, 8, 4, ptr(x), None, 16, ptr(out), None, ptr(out), ptr(out), ptr(counts), C.byref(found)), 'without room')

    lens = np.array([8, 8, 8, 8], dtype=np.int64)
    one = np.ones(4)
    b, a, zi = butter_for(1 / 60)
    w = tg.gaussian_weights()
    n_on, n_off, first = np.zeros(4, dtype=np.int32), np.zeros(4, dtype=np.int32), np.zeros(4, dtype=np.uint8)
    gc = lib.p2s_gait_contacts_host

    def call(ctx=h, method=1, n_cols=4, max_rows=8, col_len=lens, data=x, dt=one, thr=one, fac=one, sign=1, n_coef=0, bb=None, aa=None, zz=None,
             n_w=len(w), ww=w, cap=0, non=n_on, noff=n_off, fl=first):
        p = lambda v: None if v is None else ptr(v)    # noqa: E731
        return gc(ctx, method, n_cols, max_rows, p(col_len), p(data), p(dt), p(thr), p(fac), sign, n_coef, p(bb), p(aa), p(zz), n_w, p(ww),
                  None, cap, None, None, p(non), p(noff), p(fl))

    assert call() == 0                                                  # the baseline the refusals depart from
    refused(call(ctx=None), 'null context')
    refused(call(method=2), 'unknown method')
    refused(call(n_cols=0), 'bad shape')
    refused(call(max_rows=0), 'bad shape')
    refused(call(max_rows=-3), 'bad shape')
    for name in ('col_len', 'data', 'dt', 'thr', 'fac', 'non', 'noff', 'fl'):
        refused(call(**{name: None}), 'null argument')
    refused(call(cap=-1), 'without room')
    refused(call(cap=4), 'without room')                                # room announced, no buffers
    refused(call(sign=0), 'sign=0')
    refused(call(n_w=4), 'velocity method')
    refused(call(n_w=0), 'velocity method')
    refused(call(ww=None), 'velocity method')
    refused(call(col_len=np.array([8, 9, 8, 8], dtype=np.int64)), 'column 1 has 9 rows')
    refused(call(col_len=np.array([8, 8, 0, 8], dtype=np.int64)), 'column 2 has 0 rows')
    refused(call(method=0, n_coef=1, bb=b, aa=a, zz=zi), 'supported 2..9')
    refused(call(method=0, n_coef=10, bb=b, aa=a, zz=zi), 'supported 2..9')
    refused(call(method=0, n_coef=3, bb=None, aa=a, zz=zi), 'null filter coefficients')
    refused(call(method=0, n_coef=3, bb=b, aa=a * 2, zz=zi), 'a[0] must be 1')
    refused(call(method=0, n_coef=3, bb=b, aa=a, zz=zi), 'greater than padlen, which is 9')   # 7 samples after the drop

    ms = C.c_float(0)
    refused(lib.p2s_gait_kernel_ms(None, C.byref(ms)), 'null argument')
    refused(lib.p2s_gait_kernel_ms(h, None), 'null argument')
    assert lib.p2s_gait_kernel_ms(h, C.byref(ms)) == 0 and ms.value >= 0.0


def test_kernel_ms_needs_a_call_first():
    from pose2sim_amd.engine import Engine
    fresh = Engine(0)
    with pytest.raises(_lib.P2sError, match='has run on this context'):
        fresh.gait_kernel_ms()
    fresh.find_peaks(np.array([[0.0], [1.0], [0.0]]))
    assert fresh.gait_kernel_ms() >= 0.0
    fresh.close()
