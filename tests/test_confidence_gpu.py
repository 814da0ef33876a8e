"""The confidence kernels, np.mean / np.std of long columns and the whole utility on the MI355X, through the C-ABI: against the
goldens recorded from the reference (tests/golden/confidence_units.npz), against NumPy itself on columns of every length
at which the summation tree changes shape, and against the NumPy stand-in on large seeded tables.  There is no tolerance:
every array, NaN pattern and sign must be equal.  Every test prints its figures before it asserts."""
import time

import numpy as np
import pytest

import confidence_numpy as cn
from test_confidence_host import ALL, check_engine_on_case, gold, run_case  # noqa: F401
from test_jitter_host import same

pytestmark = pytest.mark.gpu

LARGE = ((3, 108000, 2024), (8, 36000, 2025))            # (cameras, frames, seed): the tables of tests/test_jitter_gpu.py
# valid entries per column: around every size at which np.add.reduce changes its path -- the plain loop (< 8), one block of
# eight accumulators with and without a tail, the first split (129) and where its halves get a tail, powers of two, the
# 8192-entry chunks with a remainder of 1, 7, 8 and 9, two and three chunks, a last chunk of 129, and a long column
COUNTS = (1, 2, 7, 8, 9, 15, 16, 17, 127, 128, 129, 135, 136, 137, 255, 256, 257, 1023, 1024, 1025, 8191, 8192, 8193, 8199, 8200,
          8201, 16383, 16384, 16385, 24705, 36000)
KINDS = ('three decimals', 'full precision', 'constant', 'all NaN', 'cancellation')


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


def columns(m, rng):
    """-> [rows][5], one column per kind of KINDS with m entries each (none in 'all NaN') among rows = m + m // 9 + 1: about
    one row in ten is NaN, at other rows in every column."""
    rows = m + m // 9 + 1
    values = [np.round(rng.uniform(0.0, 1.0, m), 3), rng.uniform(0.0, 1.0, m), np.full(m, 0.4), None,
              rng.choice([1e8, 1.0, -1e8, 1e-3], m)]     # a wrong summation order shows in the leading digits here
    a = np.full((rows, len(KINDS)), np.nan)
    for c, v in enumerate(values):
        if v is not None:
            a[np.sort(rng.choice(rows, m, replace=False)), c] = v
    return a


@pytest.mark.parametrize('m', COUNTS)
def test_column_mean_std_against_numpy(engine, m, capsys):
    a = columns(m, np.random.default_rng(m))
    mean, std, counts = engine.column_mean_std(a)
    valid = [a[:, c][~np.isnan(a[:, c])] for c in range(a.shape[1])]
    want_mean = np.array([np.mean(v) if len(v) else np.nan for v in valid])
    want_std = np.array([np.std(v) if len(v) else np.nan for v in valid])
    with capsys.disabled():
        print(f'column_mean_std m = {m}, {len(a)} rows: mean {mean.tolist()} (NumPy {want_mean.tolist()}), std {std.tolist()} (NumPy {want_std.tolist()})')
    assert list(counts) == [m, m, m, 0, m]
    assert same(mean, want_mean), [KINDS[c] for c in range(5) if not same(mean[c], want_mean[c])]
    assert same(std, want_std), [KINDS[c] for c in range(5) if not same(std[c], want_std[c])]


@pytest.mark.parametrize('m', COUNTS)
def test_percentiles_and_medians_against_numpy(engine, m, capsys):
    """The same columns as one camera's table: np.median, np.percentile, min, max, the counts below the thresholds and per band."""
    a = columns(m, np.random.default_rng(m))
    ths = (0.4, 0.5, 1e-3, -1.0, 1e8)
    res = engine.confidence_stats([a], ths)
    ref = cn.NumpyConfidenceEngine().confidence_stats([a], ths)
    with capsys.disabled():
        print(f'confidence_stats m = {m}: median {res["stats"][0, :, 1].tolist()}, p5 {res["stats"][0, :, 5].tolist()}, p95 {res["stats"][0, :, 8].tolist()}')
    for key in ref:
        assert same(ref[key], res[key]), key


def test_empty_and_single_row_tables(engine):
    mean, std, counts = engine.column_mean_std(np.zeros((0, 3)))
    assert np.isnan(mean).all() and np.isnan(std).all() and list(counts) == [0, 0, 0]
    mean, std, counts = engine.column_mean_std(np.array([[-0.0, np.nan, 2.5]]))
    assert same(mean, [0.0, np.nan, 2.5]) and same(std, [0.0, np.nan, 0.0]) and list(counts) == [1, 0, 1]   # -0.0 is added to +0.0
    one = np.array([[0.4] + [np.nan] * 63])                           # the widest table, one frame
    res, ref = engine.confidence_stats([one]), cn.NumpyConfidenceEngine().confidence_stats([one])
    for key in ref:
        assert same(ref[key], res[key]), key


@pytest.mark.parametrize('K', (1, 2, 25, 63, 64))
def test_tables_of_other_widths_equal_the_stand_in(engine, K, capsys):
    """Cameras of 1, 65 and 4097 frames, no multiple of the transposition's 64-frame tile, at widths on the edges of its
    [64][65] LDS tile; three-decimal values, about one entry in ten NaN, at other frames in every column."""
    rng = np.random.default_rng(K)
    tables = [np.round(rng.uniform(0.0, 1.0, (F, K)), 3) for F in (1, 65, 4097)]
    for t in tables:
        t[rng.random(t.shape) < 0.1] = np.nan
    tables[0][0, 0] = 0.4                                             # the one-frame camera keeps an entry, on a band's edge
    ths = (0.4, 0.6)
    ref = cn.NumpyConfidenceEngine().confidence_stats(tables, ths)
    res = engine.confidence_stats(tables, ths)
    with capsys.disabled():
        print(f'confidence_stats K = {K}, frames (1, 65, 4097): entries {res["counts"].sum(axis=1).tolist()} (NumPy {ref["counts"].sum(axis=1).tolist()}), '
              f'mean of the last column {res["stats"][:, -1, 0].tolist()} (NumPy {ref["stats"][:, -1, 0].tolist()})')
    assert (ref['counts'][1:] > 0).all() and (ref['counts'][1:] < np.array([65, 4097])[:, None]).all()     # every long column has NaN to skip
    for key in ref:
        assert res[key].dtype == ref[key].dtype and same(ref[key], res[key]), key


def test_refusals(engine):
    from pose2sim_amd._lib import P2sError
    for tables, ths, text in (([np.zeros((2, 65))], (0.4,), r'n_kpts=65 outside \[1, 64\]'),
                              ([np.zeros((2, 26))], (0.1,) * 9, r'n_thresholds=9 outside \[0, 8\]')):
        with pytest.raises(P2sError, match=text):
            engine.confidence_stats(tables, ths)
    with pytest.raises(P2sError, match='same K'):
        engine.confidence_stats([np.zeros((2, 26)), np.zeros((0, 26))])
    from pose2sim_amd.engine import Engine
    with pytest.raises(P2sError, match='p2s_confidence_stats_host has not run on this context'):
        Engine(0).confidence_kernel_ms()


@pytest.mark.parametrize('C,F,seed', LARGE)
def test_large_seeded_tables_equal_the_stand_in(engine, C, F, seed, capsys):
    tables = cn.seeded_tables(C, F, seed)
    ths = (0.4, 0.5, 0.6)
    ref = cn.NumpyConfidenceEngine().confidence_stats(tables, ths)
    first = engine.confidence_stats(tables, ths)                      # warm-up: code objects, allocations
    t0 = time.perf_counter()
    res = engine.confidence_stats(tables, ths)
    call = time.perf_counter() - t0
    ms = engine.confidence_kernel_ms()
    with capsys.disabled():
        print(f'confidence {C} x {F}: {int(res["counts"].sum())} entries of {C * F * 26}; kernels {ms:.3f} ms, call with the copies {call * 1e3:.1f} ms')
    assert (ref['counts'] < F).all() and (ref['counts'] > 0.9 * F).all()      # the compaction has work to do
    for key in ref:
        assert same(ref[key], res[key]), key
        assert first[key].tobytes() == res[key].tobytes(), key         # two runs, the same bytes
