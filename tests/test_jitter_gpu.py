"""The jitter kernels, the exact column order statistic and the whole utility on the MI355X, through the C-ABI: against
the goldens recorded from the reference (tests/golden/jitter_units.npz), against np.sort on adversarial columns, and
against the NumPy restatement on large seeded series.  There is no tolerance: every array, NaN pattern, sign and the
event list must be equal.  Every test prints its figures (events per pattern, kernel time) before it asserts."""
import time

import numpy as np
import pytest

import jitter_numpy as jn
from test_jitter_host import ALL, check_engine_on_case, gold, run_case, same  # noqa: F401

pytestmark = pytest.mark.gpu

LARGE = ((3, 108000, 2024), (8, 36000, 2025))            # (cameras, frames, seed): tests/golden/make_golden_jitter.py checks
                                                          # that each holds at least 100 events of every pattern


@pytest.fixture(scope='module')
def engine():
    from pose2sim_amd.engine import Engine
    return Engine(0)


@pytest.mark.parametrize('name', ALL)
def test_kernels_reproduce_the_reference(gold, engine, name, capsys):   # noqa: F811
    with capsys.disabled():
        check_engine_on_case(gold, name, engine)


@pytest.mark.parametrize('name', ALL)
def test_utility_on_the_gpu_writes_the_recorded_files(gold, engine, tmp_path, name, capsys):   # noqa: F811
    run_case(gold, name, str(tmp_path), engine, capsys)


def adversarial_columns(n, rng):
    """-> [n][12]: one column per kind, NaN sprinkled over most of them."""
    tiny = np.float64(5e-324)
    cols = [rng.normal(0, 1, n),                                                      # well spread
            np.full(n, np.nan),                                                       # all NaN
            np.full(n, 3.25),                                                         # all equal
            rng.choice([1.5, -2.0], n),                                               # two distinct values
            rng.integers(0, 7, n) * tiny,                                             # subnormals and zero
            rng.choice([1.7e308, -1.7e308, 1e300, np.inf, -np.inf], n),               # huge values
            -np.abs(rng.normal(0, 1e-3, n)),                                          # negative only
            rng.choice([-0.0, -1.0, -1e-300], n),                                     # negative zero among negatives
            np.zeros(n),                                                              # zeros
            np.floor(rng.uniform(0, 4, n)) + rng.choice([0.0, 2.0 ** -52], n),        # heavy duplicates one ulp apart
            np.abs(rng.normal(3, 2, n)).astype(np.float32).astype(np.float64),        # what a displacement column looks like
            rng.permutation(n).astype(np.float64)]                                    # every value once
    a = np.stack(cols, axis=1)
    for c in (0, 3, 4, 5, 9, 10):
        a[rng.random(n) < 0.2, c] = np.nan
    return a


@pytest.mark.parametrize('n', [1, 2, 63, 64, 65, 4097, 1000003])
def test_column_order_stats_against_sort(engine, n, capsys):
    rng = np.random.default_rng(n)
    a = adversarial_columns(n, rng)
    ranks = np.array([0, 1, -1, -2, n // 2, (n - 1) // 2, n // 3, -(n // 4) - 1, n - 1, -n, n, -n - 1, 5, 5, 6, 4], dtype=np.int64)
    t0 = time.perf_counter()
    out, counts = engine.column_order_stats(a, ranks)
    dt = time.perf_counter() - t0
    with capsys.disabled():
        print(f'column_order_stats: {n} rows x {a.shape[1]} columns x {len(ranks)} ranks in {dt * 1e3:.1f} ms with the copies')
    for c in range(a.shape[1]):
        s = np.sort(a[~np.isnan(a[:, c]), c])
        m = len(s)
        assert counts[c] == m, (n, c)
        want = np.array([s[r] if -m <= r < m else np.nan for r in ranks])
        assert np.array_equal(out[c], want, equal_nan=True), (n, c, out[c], want)
        if c != 7:                                                    # np.sort leaves -0.0 and +0.0 in input order
            ok = ~np.isnan(want)
            assert np.array_equal(np.signbit(out[c][ok]), np.signbit(want[ok])), (n, c)
    # both middle ranks at once give np.nanmedian
    for c in range(a.shape[1]):
        m = int(counts[c])
        if m == 0:
            continue
        two, _ = engine.column_order_stats(a[:, c:c + 1], [(m - 1) // 2, m // 2])
        with np.errstate(over='ignore', invalid='ignore'):
            med = np.mean(two[0, :1] if m % 2 else two[0])            # np.median: the mean of the middle entries, which
                                                                      # adds them to +0.0 (a median of -0.0 is +0.0)
            assert same(med, np.nanmedian(a[:, c])), (n, c)


def test_negative_zero_orders_before_positive_zero(engine):
    out, counts = engine.column_order_stats(np.array([[0.0], [-0.0], [np.nan], [1.0], [-0.0]]), [0, 1, 2, 3, 4])
    assert counts[0] == 4 and np.array_equal(out[0, :4], [0.0, 0.0, 0.0, 1.0]) and np.isnan(out[0, 4])
    assert list(np.signbit(out[0, :4])) == [True, True, False, False]


def test_column_order_stats_16m_rows(engine, capsys):
    """2^24 + 1 rows: past every 24-bit count."""
    n = (1 << 24) + 1
    rng = np.random.default_rng(7)
    a = rng.normal(0, 1, n).astype(np.float32).astype(np.float64)[:, None]
    a[::5] = np.nan
    out, counts = engine.column_order_stats(a, [0, (n // 2), -1])
    s = np.sort(a[~np.isnan(a)])
    with capsys.disabled():
        print(f'column_order_stats: {n} rows, {counts[0]} not NaN')
    assert counts[0] == len(s)
    assert np.array_equal(out[0], [s[0], s[n // 2], s[-1]])


@pytest.mark.parametrize('C,F,seed', LARGE)
def test_large_seeded_series_equal_the_restatement(engine, C, F, seed, capsys):
    series = [jn.seeded_series(F, seed * 100 + c) for c in range(C)]
    ref = jn.NumpyJitterEngine().jitter(series)
    engine.jitter(series)                                             # warm-up: code objects, allocations
    t0 = time.perf_counter()
    res = engine.jitter(series)
    call = time.perf_counter() - t0
    ms = engine.jitter_kernel_ms()
    with capsys.disabled():
        print(f'jitter {C} x {F}: {len(res["events"])} events, per pattern {jn.pattern_counts(res["events"])}; kernels {ms:.3f} ms, '
              f'call with the copies {call * 1e3:.1f} ms')
    assert min(jn.pattern_counts(ref['events']).values()) >= 100
    for c in range(C):
        for key in ('displacements', 'bb_areas', 'medians', 'thresholds', 'median_bb_area', 'jitter_mask', 'counts'):
            assert same(ref[key][c], res[key][c]), (c, key)
    assert np.array_equal(ref['events'], res['events'])


def test_event_list_larger_than_the_first_capacity(engine):
    """More events than the first call has room for: the second call returns them all, in order."""
    rng = np.random.default_rng(11)
    s = np.concatenate([rng.uniform(100, 1800, (20000, 26, 2)), np.full((20000, 26, 1), 0.9)], axis=2)
    s[::2, :, :2] = s[0, :, :2]                                       # every other frame the same: the median is large, but
    res = engine.jitter([s], multiplier=0.5)                          # half of it is below most jumps
    ref = jn.NumpyJitterEngine().jitter([s], multiplier=0.5)
    assert len(ref['events']) > (1 << 18)
    assert np.array_equal(ref['events'], res['events'])
    assert same(ref['jitter_mask'][0], res['jitter_mask'][0])
