"""GPU parity of p2s_loess_kernel through the C-ABI (p2s_loess_host, Engine.loess): against the goldens recorded through
the reference's own loess_filter_1d with a stand-in for statsmodels' lowess, against the exact values stored next to them
(tests/golden/loess_units.npz, tests/test_loess_host.py), and against the kernel's NumPy mirror (tests/loess_numpy.py) on
seeded matrices at the shapes where indexing can break.

Bars: filtered samples within 1e-9 relative to max(1, |value|) with identical NaN pattern (kernel and mirror do the same
centred sums in a different order: in practice 1e-14), copied samples bit-identical.  statsmodels itself has never run
here; nothing in this file is parity with statsmodels."""
import ctypes as C
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

TOL = 1e-9
WINDOWS = (2, 3, 4, 5, 30, 257)
N_COLS = (1, 63, 64, 65, 79)


@pytest.fixture(scope='module')
def engine():
    import __graft_entry__ as entry
    entry.build_hip()
    from pose2sim_amd.engine import Engine
    eng = Engine(0)
    yield eng
    eng.close()


@pytest.fixture(scope='module')
def gold(golden_dir):
    return np.load(os.path.join(golden_dir, 'loess_units.npz'))


def _distance(got, want, what):
    assert got.shape == want.shape and np.array_equal(np.isnan(got), np.isnan(want)), f'{what}: NaN pattern'
    ok = ~np.isnan(want)
    return float((np.abs(got[ok] - want[ok]) / np.maximum(1.0, np.abs(want[ok]))).max()) if ok.any() else 0.0


def _close(got, want, what):
    d = _distance(got, want, what)
    assert d <= TOL, f'{what}: {d:.3e}'
    return d


def test_golden_columns(engine, gold):
    """Engine.loess on every column of loess_units.npz: within TOL of what the reference's own loess_filter_1d returned
    (lowess replaced by the stand-in) and of the exact values; samples outside the filtered runs bit-identical to the
    input.  Measured on an MI355X: worst 9.7e-12 from the reference's outputs (the stand-in's own distance from exact at
    frame 98 765), 8.2e-14 from the exact values."""
    import test_loess_host as host
    g = gold
    worst_ref = worst_exact = 0.0
    for i in range(int(g['n_cols'])):
        got = engine.loess(g[f'col{i}_in'].reshape(-1, 1), host.nb_of(g, i))[:, 0]
        d_ref, d_exact = host.check_column(got, g, i, 'kernel')
        print(f'column {i}: |kernel - reference| = {d_ref:.2e}, |kernel - exact| = {d_exact:.2e}')
        worst_ref, worst_exact = max(worst_ref, d_ref), max(worst_exact, d_exact)
    print(f'worst: {worst_ref:.2e} from the reference, {worst_exact:.2e} from the exact values')


def test_golden_columns_in_one_launch(engine, gold):
    """The columns of one nb_values_used side by side in one matrix, padded with NaN to a common length: neighbouring
    threads must not disturb each other."""
    import test_loess_host as host
    g = gold
    groups = {}
    for i in range(int(g['n_cols'])):
        if len(g[f'col{i}_in']) <= 1000:
            groups.setdefault(host.nb_of(g, i), []).append(i)
    assert set(groups) == set(host.NB_VALUES)
    for nb, members in groups.items():
        L = max(len(g[f'col{i}_in']) for i in members)
        data = np.full((L, len(members)), np.nan)
        for c, i in enumerate(members):
            data[:len(g[f'col{i}_in']), c] = g[f'col{i}_in']
        got = engine.loess(data, nb)
        for c, i in enumerate(members):
            n = len(g[f'col{i}_in'])
            host.check_column(got[:n, c], g, i, f'kernel, in a group of {len(members)}')
            assert np.isnan(got[n:, c]).all()


def seeded_matrix(n_frames, n_cols, seed):
    """Coordinates at scale 1 and -1000 with a few NaN and exact zeros per column, some columns without any, column 7
    all NaN."""
    rng = np.random.default_rng(seed)
    t = np.arange(n_frames)[:, None] / 60.0
    scale = np.where(np.arange(n_cols) % 3 == 1, -1000.0, 1.0)[None, :]
    data = scale * (1.2 + 0.4 * np.sin(2 * np.pi * 1.1 * t + rng.uniform(0, 6, (1, n_cols))) + 0.05 * np.sin(2 * np.pi * 7 * t)
                    + rng.normal(0, 0.005, (n_frames, n_cols)))
    holes = rng.random((n_frames, n_cols)) < 3.0 / max(n_frames, 3)
    holes[:, ::5] = False
    data[holes] = np.nan
    data[rng.random((n_frames, n_cols)) < 0.004] = 0.0
    if n_cols > 7:
        data[:, 7] = np.nan
    return data


@pytest.fixture(scope='module')
def matrix():
    return seeded_matrix(700, 79, 31)


@pytest.fixture(scope='module')
def mirror(matrix):
    """The mirror's answer for the 700 x 79 matrix, once per window; columns are independent, so the answer for its
    first n columns is the first n columns of this."""
    from loess_numpy import loess_columns
    return {k: loess_columns(matrix, k) for k in WINDOWS}


@pytest.mark.parametrize('k', WINDOWS)
def test_matrix_against_the_mirror(engine, matrix, mirror, k):
    """700 frames x 1 / 63 / 64 / 65 / 79 columns: rows that are no multiple of the workgroup, an all-NaN column beside
    full ones, runs of every length."""
    want = mirror[k]
    assert (want != matrix)[~np.isnan(matrix)].any() or k <= 3        # it did filter (k = 2 and 3 fit their samples exactly)
    for n_cols in N_COLS:
        data = np.ascontiguousarray(matrix[:, :n_cols])
        got = engine.loess(data, k)
        _close(got, want[:, :n_cols], f'k = {k}, 700 x {n_cols}')
        copied = want[:, :n_cols] == data
        assert np.array_equal(got[copied], data[copied]), (k, n_cols)
    full = engine.loess(matrix, k)
    assert np.isnan(full[:, 7]).all() and not np.isnan(full[:, 5]).any()
    assert np.array_equal(full, engine.loess(matrix, k), equal_nan=True)      # the same call twice: bit for bit


@pytest.mark.parametrize('k', WINDOWS + (1001,))
def test_shortest_matrices(engine, k):
    """n_frames = k + 1 (every window clamped at both ends of the only run that can be filtered) and n_frames = 1."""
    from loess_numpy import loess_columns
    widths = N_COLS if k < 100 else (1, 64, 65)
    data = seeded_matrix(k + 1, max(widths), 100 + k)
    data[:, ::5] = np.abs(data[:, ::5]) + 0.5                      # the columns without NaN: one run of k + 1 samples
    want = loess_columns(data, k)
    assert (want[:, 0] != data[:, 0]).any() or k <= 3
    for n_cols in widths:
        part = np.ascontiguousarray(data[:, :n_cols])
        _close(engine.loess(part, k), want[:, :n_cols], f'k = {k}, {k + 1} x {n_cols}')
        one = np.ascontiguousarray(data[:1, :n_cols])
        assert np.array_equal(engine.loess(one, k), one, equal_nan=True)


def test_windows_that_outrun_a_workgroup(engine):
    """k = 1001 on 1 500 frames: a window covers four workgroups' spans of a one-column matrix; with three columns, a full
    one, one split at frame 1 200 (a run of 1 200 and one of 299 samples, left alone) and an all-NaN one."""
    from loess_numpy import loess_columns
    data = seeded_matrix(1500, 3, 77)
    data[:, 0] = np.abs(data[:, 0]) + 0.5
    data[:, 1] = -1000.0 * data[::-1, 0]
    data[1200, 1] = np.nan
    data[:, 2] = np.nan
    want = loess_columns(data, 1001)
    got = engine.loess(data, 1001)
    _close(got, want, 'k = 1001, 1500 x 3')
    assert np.array_equal(got[1201:, 1], data[1201:, 1]) and (got[:1200, 1] != data[:1200, 1]).all()
    first = np.ascontiguousarray(data[:, :1])
    _close(engine.loess(first, 1001), want[:, :1], 'k = 1001, 1500 x 1')
    assert np.array_equal(got, engine.loess(data, 1001), equal_nan=True)


@pytest.mark.parametrize('n_cols', [1, 64, 65])
def test_runs_that_end_and_start_at_a_workgroup_boundary(engine, n_cols):
    """A workgroup takes 256 consecutive elements of the row-major matrix.  One run ends exactly at the last element of
    a workgroup, another starts exactly at the first element of one; each is k + 3 samples long."""
    from loess_numpy import loess_columns
    k = 5
    n_frames = 256 * 6 // n_cols + 12
    data = np.nan_to_num(np.abs(seeded_matrix(n_frames, n_cols, 5 + n_cols)), nan=0.75) + 0.5
    f, c = divmod(256 * 3 - 1, n_cols)                              # the last element of the third workgroup
    assert f >= k + 3
    data[f + 1, c] = np.nan
    data[f - (k + 3), c] = np.nan
    f2, c2 = divmod(256 * 5, n_cols)                                # the first element of the sixth workgroup
    assert f2 + k + 3 < n_frames and (c2 != c or f2 > f + 2)
    data[f2 - 1, c2] = np.nan
    data[f2 + k + 3, c2] = np.nan
    want = loess_columns(data, k)
    assert (want[f - (k + 2):f + 1, c] != data[f - (k + 2):f + 1, c]).any() and (want[f2:f2 + k + 3, c2] != data[f2:f2 + k + 3, c2]).any()
    _close(engine.loess(data, k), want, f'boundary runs, {n_frames} x {n_cols}')


@pytest.mark.parametrize('k, every', [(5, 4), (5, 6), (30, 7), (2, 3)])
def test_no_run_qualifies(engine, k, every):
    """An isolated NaN every few frames leaves runs of at most k samples: the output is the input bit for bit."""
    data = seeded_matrix(300, 65, 9)
    data[::every] = np.nan
    assert every - 1 <= k
    got = engine.loess(data, k)
    assert np.array_equal(got, data, equal_nan=True)
    assert np.array_equal(got.view(np.int64), data.view(np.int64))


def test_filter_all_loess_on_the_gpu(engine, gold):
    """filter_all with type = 'loess' (key `loess`, and key `LOESS` with the first frame at 17) against the text the
    reference wrote: header lines and frame / time columns exactly, coordinates within TOL."""
    import shutil
    import tempfile
    from pathlib import Path
    import test_loess_host as host
    from pose2sim_amd import filtering
    g = gold
    root = tempfile.mkdtemp(prefix='p2s_loess_')
    try:
        for i in range(int(g['n_files'])):
            trial, cfg = host.write_trial(Path(root), g, i)
            paths = filtering.filter_all(cfg, engine=engine)
            assert [os.path.basename(p) for p in paths] == [str(g[f'file{i}_out_name'])]
            d = host.compare_trc_text(open(paths[0]).read(), str(g[f'file{i}_out_text']), f'file {i}', TOL)
            print(f'file {i}: worst coordinate {d:.2e} from the recorded text')
    finally:
        shutil.rmtree(root, ignore_errors=True)


# ---- refusals of p2s_loess_host, through the raw library with a live context -------------------------------------------------
INVALID = -1


def P(a):
    return a.ctypes.data_as(C.c_void_p)


DATA = np.arange(1.0, 17.0).reshape(8, 2)
PLUS_INF, MINUS_INF = DATA.copy(), DATA.copy()
PLUS_INF[3, 1], MINUS_INF[7, 0] = np.inf, -np.inf
SENTINEL = -12345.5
OUT = np.full(16, SENTINEL)
INF_TEXT = "LOESS filter: the data hold an infinity (statsmodels' answer for one has not been recorded)"

# (arguments after the context: n_frames, n_cols, data, k, min_run, out; return code; message)
CASES = [
    ((-1, 2, None, 5, 6, None), INVALID, 'bad shape: n_frames=-1 n_cols=2'),
    ((8, -2, None, 5, 6, None), INVALID, 'bad shape: n_frames=8 n_cols=-2'),
    ((8, 2, None, 5, 6, P(OUT)), INVALID, 'null pointer'),
    ((8, 2, P(DATA), 5, 6, None), INVALID, 'null pointer'),
    ((8, 2, P(DATA), 1, 6, P(OUT)), INVALID, 'LOESS filter: window of 1 samples: supported 2..8191'),
    ((8, 2, P(DATA), 0, 6, P(OUT)), INVALID, 'LOESS filter: window of 0 samples: supported 2..8191'),
    ((8, 2, P(DATA), -3, 6, P(OUT)), INVALID, 'LOESS filter: window of -3 samples: supported 2..8191'),
    ((8, 2, P(DATA), 8192, 8193, P(OUT)), INVALID, 'LOESS filter: window of 8192 samples: supported 2..8191'),
    ((8, 2, P(DATA), 5, 5, P(OUT)), INVALID, 'LOESS filter: min_run=5 must exceed the window of 5 samples'),
    ((8, 2, P(DATA), 5, 0, P(OUT)), INVALID, 'LOESS filter: min_run=0 must exceed the window of 5 samples'),
    ((0, 2, None, 1, 6, None), INVALID, 'LOESS filter: window of 1 samples: supported 2..8191'),     # parameters are checked for an empty shape too
    ((8, 2, P(PLUS_INF), 5, 6, P(OUT)), INVALID, INF_TEXT),
    ((8, 2, P(MINUS_INF), 5, 6, P(OUT)), INVALID, INF_TEXT),
]


@pytest.fixture(scope='module')
def lib(engine):
    from pose2sim_amd import _lib
    return _lib.load()


@pytest.mark.parametrize('args, code, text', CASES, ids=[f'loess-{i}' for i in range(len(CASES))])
def test_refusal_with_a_live_context(lib, engine, args, code, text):
    """Every refusal returns its code and message before anything is copied or launched; `out` is left untouched."""
    OUT[:] = SENTINEL
    assert lib.p2s_loess_host(engine._h, *args) == code
    assert lib.p2s_last_error().decode() == text
    assert (OUT == SENTINEL).all()


def test_null_context_is_refused(lib):
    assert lib.p2s_loess_host(None, 8, 2, P(DATA), 5, 6, P(OUT)) == INVALID
    assert lib.p2s_last_error().decode() == 'null context'


def test_an_empty_shape_is_no_error(lib, engine):
    OUT[:] = SENTINEL
    for n_frames, n_cols in ((0, 2), (8, 0), (0, 0)):
        assert lib.p2s_loess_host(engine._h, n_frames, n_cols, None, 5, 6, None) == 0
        assert lib.p2s_loess_host(engine._h, n_frames, n_cols, P(DATA), 5, 6, P(OUT)) == 0
    assert (OUT == SENTINEL).all()
    assert engine.loess(np.empty((0, 3)), 5).shape == (0, 3) and engine.loess(np.empty((4, 0)), 5).shape == (4, 0)


def test_engine_refuses_a_window_below_two(engine):
    with pytest.raises(ValueError):
        engine.loess(np.ones((8, 2)), 1.5)
