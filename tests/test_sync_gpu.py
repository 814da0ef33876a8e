"""The synchronization kernels on the MI355X: Engine.sync_speeds / Engine.lagged_pearson against the reference's goldens
and the NumPy restatement (tests/sync_numpy.py), and the whole stage end to end."""
import os

import numpy as np
import pytest

import sync_trials as st
from sync_numpy import pearson, speeds
from test_sync_host import cases, check_against_gold, run_case

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def gold(golden_dir):
    return np.load(os.path.join(golden_dir, 'sync_units.npz'))


@pytest.fixture(scope='module')
def engine():
    from pose2sim_amd.engine import Engine
    return Engine(0)


class Recording:
    def __init__(self, engine):
        self.engine = engine

    def sync_speeds(self, coords, b, a, zi):
        self.speeds = self.engine.sync_speeds(coords, b, a, zi)
        return self.speeds

    def lagged_pearson(self, ref, signals, lag_lo, lag_hi):
        self.pearson = self.engine.lagged_pearson(ref, signals, lag_lo, lag_hi)
        return self.pearson


@pytest.fixture(scope='module')
def margins(gold):
    """Per golden r curve: the gap between its best and second-best r.  A deviation of 1e-9 cannot move the argmax
    when the gap is wider than 2e-9 (or when the curve's argmax is a NaN, which the NaN pattern decides)."""
    out = {}
    for n in cases(gold):
        for k in range(int(gold[f'case{n}_n_calls'])):
            r = gold[f'case{n}_r{k}']
            if np.isnan(r).any():
                out[(n, k)] = np.inf
                continue
            top = np.sort(r)[-2:]
            out[(n, k)] = top[1] - top[0]
    return out


def test_golden_margins_allow_the_tolerance(margins):
    assert all(m > 2e-9 for m in margins.values()), margins


@pytest.mark.parametrize('n', range(11))
def test_stage_on_the_gpu_reproduces_the_reference(gold, engine, tmp_path, margins, n):
    """Both C entries through the stage: speeds within 1e-9 max|speed|, r within 1e-9, identical offsets, log lines and
    pose-sync/ listing."""
    rec = Recording(engine)
    work = os.path.realpath(str(tmp_path))
    err, lines, trial_dir = run_case(gold, n, work, rec)
    assert err is None, err
    check_against_gold(gold, n, rec, lines, trial_dir)
    _, argmax, _ = rec.pearson
    for k in range(int(gold[f'case{n}_n_calls'])):
        assert argmax[k] == np.argmax(gold[f'case{n}_r{k}'])


@pytest.mark.parametrize('k', range(5))
def test_stage_on_the_gpu_raises_what_the_reference_raised(gold, engine, tmp_path, k):
    n = cases(gold, errors=True)[k]
    err, _, _ = run_case(gold, n, os.path.realpath(str(tmp_path)), engine)
    want_type, want_msg = (str(v) for v in gold[f'case{n}_error'])
    assert type(err).__name__ == want_type
    if want_type != 'UnboundLocalError':
        assert str(err) == want_msg


def _speed_signal(rng, n, nan_frac=0.0, zero_runs=0):
    s = np.abs(np.cumsum(rng.normal(0, 1, n))) + rng.gamma(2.0, 1.0, n)
    for _ in range(zero_runs):
        a = int(rng.integers(0, max(1, n - 10)))
        s[a:a + int(rng.integers(2, 60))] = 0.0
    if nan_frac:
        s[rng.random(n) < nan_frac] = np.nan
    return s


def _check_lags(engine, ref, sigs, lag_lo, lag_hi, picks=None):
    r, arg, mx = engine.lagged_pearson(ref, sigs, lag_lo, lag_hi)
    n_lags = lag_hi - lag_lo
    picks = range(n_lags) if picks is None else picks
    for s, sig in enumerate(sigs):
        m = min(len(ref), len(sig))
        for t in picks:
            lag = lag_lo + t
            lo, hi = max(lag, 0), min(m, len(sig) + lag)
            want = pearson(ref[lo:hi], sig[lo - lag:hi - lag]) if hi > lo else np.nan
            assert np.isnan(r[s, t]) == np.isnan(want), (s, t, r[s, t], want)
            if not np.isnan(want):
                assert abs(r[s, t] - want) <= 1e-9, (s, t, r[s, t], want)
        assert arg[s] == np.argmax(r[s])
        assert (np.isnan(mx[s]) and np.isnan(r[s]).all()) or mx[s] == np.nanmax(r[s])
    return r, arg, mx


def test_pearson_against_numpy_on_seeded_signals(engine):
    rng = np.random.default_rng(5)
    for n_ref, lens, nan_frac, zeros in ((1, [1, 3], 0, 0), (2, [2, 1, 5], 0, 0), (17, [9, 17, 40], 0.1, 1),
                                         (300, [300, 250, 420, 1], 0.05, 3), (1000, [640, 1000], 0.0, 5)):
        ref = _speed_signal(rng, n_ref, nan_frac, zeros)
        sigs = [_speed_signal(rng, n, nan_frac, zeros) for n in lens]
        half = max(1, n_ref // 2)
        _check_lags(engine, ref, sigs, -half - 3, half + 3)          # beyond the ends: 0 and 1 pairs, then none


def test_pearson_long_signals_on_sampled_lags(engine):
    """Lengths up to 70 000 (the full curve against a sample of lags, the argmax against the whole curve)."""
    rng = np.random.default_rng(6)
    ref = _speed_signal(rng, 70000, 0.01, 20)
    sigs = [_speed_signal(rng, 70000, 0.01, 20), _speed_signal(rng, 52001, 0.0, 5)]
    picks = sorted(set(rng.integers(0, 70000, 60).tolist()) | {0, 1, 34999, 35000, 69998, 69999})
    _check_lags(engine, ref, sigs, -35000, 35000, picks)


def test_pearson_nan_first_argmax(engine):
    """A constant-zero stretch gives NaN r at the lags that see only it; np.argmax then picks the first NaN."""
    rng = np.random.default_rng(8)
    ref = rng.gamma(2.0, 1.0, 100)
    sig = np.r_[rng.gamma(2.0, 1.0, 40), np.zeros(60)]          # lags <= -40 see only the zeros
    r, arg, mx = _check_lags(engine, ref, [sig], -50, 50)
    assert np.isnan(r[0][:11]).all() and not np.isnan(r[0][11:]).any() and arg[0] == 0
    assert not np.isnan(mx[0])
    r, arg, mx = engine.lagged_pearson(np.zeros(30), [np.ones(30)], -15, 15)
    assert np.isnan(r).all() and arg[0] == 0 and np.isnan(mx[0])


def test_speeds_against_numpy_on_seeded_columns(engine):
    """Interpolation (<= 4 good samples: untouched), fill, filter (short cameras unfiltered), speed sums."""
    from scipy import signal
    rng = np.random.default_rng(7)
    b, a = signal.butter(2, 6 / 15, 'low')
    zi = signal.lfilter_zi(b, a)
    coords = []
    for n in (2, 5, 6, 10, 64, 333, 5000):
        c = 500 + np.cumsum(rng.normal(0, 3, (n, 8)), axis=0)
        c[rng.random((n, 8)) < 0.08] = np.nan
        c[rng.random((n, 8)) < 0.02] = 0.0
        if n > 10:
            c[:, 3] = np.nan                                            # an all-NaN y column
            c[rng.permutation(n)[:n - 3], 5] = np.nan                   # 3 good samples: left as is
            c[:7, 1] = np.nan                                           # leading gap: extrapolated
            c[-5:, 7] = 0.0                                             # trailing zeros: extrapolated
        coords.append(c)
    got = engine.sync_speeds(coords, b, a, zi)
    want = speeds(coords, b, a)
    for g, w in zip(got, want):
        assert g.shape == w.shape
        assert np.allclose(g, w, rtol=0, atol=1e-9 * max(1.0, float(np.nanmax(np.abs(w))))), np.abs(g - w).max()
    with pytest.raises(ValueError, match='padlen, which is 9'):
        engine.sync_speeds([np.ones((8, 2))], b, a, zi)


def test_planted_offsets_are_recovered_at_5000_frames(engine, tmp_path):
    from pose2sim_amd import synchronization
    shifts = [0, 7, -12, 25]
    trial = st.make_trial(21, [5000] * 4, shifts)
    trial_dir = os.path.join(str(tmp_path), 'trial')
    st.write_trial(trial, os.path.join(trial_dir, 'pose'))
    offsets = synchronization.synchronize_cams_all(st.sync_config(trial_dir), engine=engine)
    assert offsets == [-s for s in shifts]
    listing = sorted(os.listdir(os.path.join(trial_dir, 'pose-sync', 'cam04_json')))
    assert listing[0] == 'cam04_000025.json' and len(listing) == 5000


def test_sync_plot_is_written(gold, engine, tmp_path):
    pytest.importorskip('matplotlib')
    from pose2sim_amd import synchronization
    trial_dir = os.path.join(str(tmp_path), 'trial')
    st.write_trial({k: gold[f'trialC_{k}'] for k in ('xy', 'lik', 'n_frames', 'n_persons', 'kind', 'trunc')},
                   os.path.join(trial_dir, 'pose'))
    cfg = st.sync_config(trial_dir, save_sync_plots=True, display_sync_plots=True)
    synchronization.synchronize_cams_all(cfg, engine=engine)
    for name in ('sync_cam02_vs_cam01.png', 'sync_cam02_vs_cam03.png'):
        assert os.path.getsize(os.path.join(trial_dir, 'pose-sync', name)) > 1000
