"""TEST INFRASTRUCTURE -- a NumPy / scipy mirror of csrc/p2s_gaps.hip's three entry points, written from
pose2sim_amd/postproc.py (_interpolate_column, fill_gaps, gap_spans), and the generator of the cases that the host and
GPU tests share.

The mirror keeps the two halves of the interpolation apart: `interpolants` evaluates scipy's interp1d at every bad
sample of every column (the expensive half, one pass per kind), `interpolate` then turns the runs longer than max_gap
into NaN.  A case is therefore interpolated once per kind whatever the max_gap values it is tested with.
"""
import numpy as np
from scipy import interpolate as sp_interpolate

KINDS = (None, 'linear', 'slinear', 'quadratic', 'cubic')
SPLINE_KINDS = {'slinear': 1, 'quadratic': 2, 'cubic': 3}
NONFINITE = 1                                                     # P2S_GAPS_NONFINITE

LENGTHS = (5, 6, 63, 64, 65, 257, 1025, 4099)                    # either side of a wave and of a 256-sample tile; several tiles
COLUMNS = (1, 3, 78, 130)                                        # 130: more columns than two waves of lanes
MAX_GAPS = (1, 20, np.inf)
TILE = 256


def bad_samples(coords):
    return np.isnan(coords) | (coords == 0)


def column_status(col, kind):
    """What the kernels report for a column: nonzero when a spline kind meets +-inf among more than 4 good samples."""
    good = ~bad_samples(col)
    return NONFINITE if kind in SPLINE_KINDS and good.sum() > 4 and not np.isfinite(col[good]).all() else 0


def interpolants(coords, labels, kind):
    """Per column: None (4 or fewer good samples, or a status), else (positions of the bad samples, interp1d there)."""
    out = []
    for c in range(coords.shape[1]):
        vals = coords[:, c]
        good = ~bad_samples(vals)
        if int(good.sum()) <= 4 or column_status(vals, kind):
            out.append(None)
            continue
        bad_pos = np.flatnonzero(~good)
        if not bad_pos.size:
            out.append((bad_pos, vals[:0]))
            continue
        if kind is None:
            f = sp_interpolate.interp1d(labels[good], vals[good], kind='linear', bounds_error=False, assume_sorted=True)
        else:
            f = sp_interpolate.interp1d(labels[good], vals[good], kind=kind, fill_value='extrapolate', bounds_error=False, assume_sorted=True)
        with np.errstate(all='ignore'):
            out.append((bad_pos, f(labels[bad_pos])))
    return out


def bad_runs(labels, bad_pos):
    """(first index into bad_pos, length) of every run of bad samples with consecutive labels."""
    if not bad_pos.size:
        return np.zeros(0, dtype=np.int64), np.zeros(0, dtype=np.int64)
    starts = np.concatenate(([0], np.flatnonzero(np.diff(labels[bad_pos]) > 1) + 1))
    return starts, np.diff(np.concatenate((starts, [bad_pos.size])))


def interpolate(coords, labels, max_gap, kind, patches=None):
    """Engine.interpolate_gaps: (out, status).  patches: interpolants(coords, labels, kind), when already computed."""
    coords = np.asarray(coords, dtype=np.float64)
    labels = np.asarray(labels, dtype=np.int64)
    patches = interpolants(coords, labels, kind) if patches is None else patches
    out = coords.copy()
    status = np.array([column_status(coords[:, c], kind) for c in range(coords.shape[1])], dtype=np.int32)
    for c, patch in enumerate(patches):
        if patch is None:
            continue
        bad_pos, new = patch[0], patch[1].copy()
        starts, lengths = bad_runs(labels, bad_pos)
        for s0, ln in zip(starts, lengths):
            if ln > max_gap:
                new[s0:s0 + ln] = np.nan
        out[bad_pos, c] = new
    return out, status


def fill(coords, how):
    """Engine.fill_gaps."""
    out = np.array(coords, dtype=np.float64)
    if how not in ('last_value', 'zeros'):
        return out
    rows = np.arange(out.shape[0])
    for c in range(out.shape[1]):
        col = out[:, c]
        missing = np.isnan(col)
        if how == 'last_value' and missing.any() and not missing.all():
            last = np.maximum.accumulate(np.where(missing, -1, rows))
            first = int(np.argmin(missing))
            col[missing] = col[np.where(last >= 0, last, first)[missing]]
            missing = np.isnan(col)
        col[missing | (col == np.inf)] = 0
    return out


def runs_table(x, first, last, max_gap):
    """p2s_gap_runs's table: rows (column, start, end, long) by column, then by position."""
    rows = []
    for k in range(x.shape[1]):
        pos = np.flatnonzero((x[:, k] == 0) | ~np.isfinite(x[:, k]))
        pos = pos[(pos > first) & (pos < last)]
        for r in np.split(pos, np.flatnonzero(np.diff(pos) > 1) + 1):
            if len(r):
                rows.append((k, r[0], r[-1], int(len(r) > max_gap)))
    return np.array(rows, dtype=np.int32).reshape(-1, 4)


def runs(x, first, last, max_gap):
    """Engine.gap_runs: (done, left) as postproc.gap_spans returns them."""
    done, left = [[] for _ in range(x.shape[1])], [[] for _ in range(x.shape[1])]
    for k, a, b, is_long in runs_table(x, first, last, max_gap).tolist():
        (left if is_long else done)[k].append(f'{a}:{b}')
    return done, left


class HostEngine:
    """The mirror behind the engine's method names: a host double for triangulation.finish_persons_engine."""

    def __init__(self, status_columns=()):
        self.status_columns = tuple(status_columns)
        self.calls = {'interpolate_gaps': 0, 'fill_gaps': 0, 'gap_runs': 0}

    def interpolate_gaps(self, coords, labels, max_gap, kind):
        self.calls['interpolate_gaps'] += 1
        out, status = interpolate(coords, labels, max_gap, kind)
        for c in self.status_columns:
            out[:, c], status[c] = np.asarray(coords)[:, c], NONFINITE
        return out, status

    def fill_gaps(self, coords, how):
        self.calls['fill_gaps'] += 1
        return fill(coords, how)

    def gap_runs(self, x, first, last, max_gap):
        self.calls['gap_runs'] += 1
        return runs(np.asarray(x), first, last, max_gap)


# ---- the cases ----------------------------------------------------------------------------------------------------------------
# Column c of a case of length F is made from (F, c) alone: the case of 130 columns holds the case of 78 as its first
# columns, and what is computed for a column (its interpolants, its exact solve) serves every case that holds it.
FIVE_GOOD, FOUR_GOOD, ALL_NAN, WITH_INF = 1, 2, 3, 4             # the columns with a planted peculiarity (when the case has them)
EXACT_RUNS = (1, 2, 20, 21)                                      # runs of exactly max_gap and max_gap + 1 samples, max_gap 1 and 20


def case_labels(F):
    """Frame numbers from an offset, with one step of 2 in the middle (a bad run across it is two runs)."""
    labels = np.arange(F, dtype=np.int64) + 11
    if F >= 6:
        labels[F // 2:] += 1
    return labels


def _column(F, c):
    rng = np.random.default_rng(1000 * F + c)
    col = np.cumsum(rng.normal(0, 0.01, F)) + rng.uniform(-2, 2)
    col[col == 0] = 1e-3
    bad = np.zeros(F, dtype=bool)
    if c == ALL_NAN:
        return np.full(F, np.nan)
    if c in (FIVE_GOOD, FOUR_GOOD):
        bad[:] = True
        bad[rng.choice(F, size=min(F, 5 if c == FIVE_GOOD else 4), replace=False)] = False
    elif F < 8:
        bad[rng.integers(0, F)] = True                            # F = 5 leaves 4 good samples, F = 6 leaves 5
    else:
        if F >= 16:
            for s in np.flatnonzero(rng.random(F) < 0.02):
                bad[s:s + int(rng.integers(1, 4))] = True
        if c % 2 == 0:                                            # gaps at both ends: extrapolation
            bad[:int(rng.integers(1, 3))] = True
            bad[F - int(rng.integers(1, 3)):] = True
        bad[F // 2 - 1:F // 2 + 1] = True                         # across the label step
        keep_out = {F // 2 - 1, F // 2}
        for k in range(TILE, F, TILE):                            # across every tile boundary
            lo, hi = k - 1 - (k // TILE + c) % 3, k + 1 + (k // TILE + c) % 2
            bad[lo:hi] = True
            keep_out.update(range(lo, hi))
        at = 4
        for length in EXACT_RUNS:                                 # runs of exactly these lengths, good samples around them
            while at + length + 1 < F - 3 and any(p in keep_out for p in range(at - 1, at + length + 1)):
                at += 1
            if at + length + 1 >= F - 3:
                break
            bad[at - 1], bad[at + length] = False, False
            bad[at:at + length] = True
            keep_out.update(range(at - 1, at + length + 1))
            at += length + 2
    kind_of_bad = rng.integers(0, 3, F)
    col[bad] = np.where(kind_of_bad[bad] == 0, np.nan, np.where(kind_of_bad[bad] == 1, 0.0, -0.0))
    if c == WITH_INF:
        col[rng.choice(np.flatnonzero(~bad))] = np.inf
    return col


def make_case(F, C):
    """(coords [F][C], labels [F]) with, where F and C leave room: gaps at both ends, runs of exactly 1, 2, 20 and 21 bad
    samples, NaN, 0 and -0.0 as bad samples, a column of exactly 5 good samples, one of exactly 4, one all NaN, one with
    +inf among its good samples, a bad run across the step of 2 in the labels and one across every multiple of 256."""
    return np.stack([_column(F, c) for c in range(C)], axis=1), case_labels(F)


def same(a, b):
    return a.shape == b.shape and np.array_equal(a, b, equal_nan=True)


# ---- what the host and the GPU tests check, with the entry point under test as an argument -----------------------------------
_columns, _patches, _exact = {}, {}, {}
EXACT_UP_TO = 257                                                # rows: beyond, a 60-digit solve of every column takes too long
EPS = 2.0 ** -52


def case(F, C):
    """make_case(F, C), every column made once."""
    for c in range(C):
        if (F, c) not in _columns:
            _columns[F, c] = _column(F, c)
    return np.stack([_columns[F, c] for c in range(C)], axis=1), case_labels(F)


def case_patches(F, C, kind):
    """interpolants() of case(F, C), every column interpolated once per kind."""
    coords, labels = case(F, C)
    for c in range(C):
        if (F, c, kind) not in _patches:
            _patches[F, c, kind] = interpolants(coords[:, c:c + 1], labels, kind)[0]
    return [_patches[F, c, kind] for c in range(C)]


def case_exact(F, c, kind):
    """The 60-digit interpolant of column c of the cases of length F at its bad samples, solved once."""
    import gaps_exact
    if (F, c, kind) not in _exact:
        coords, labels = case(F, c + 1)
        _exact[F, c, kind] = gaps_exact.column(coords[:, c], labels, kind)[1]
    return _exact[F, c, kind]


def spline_bound(d_ref, scale):
    """The issue's bar for a spline kind: 8 x max(scipy's own distance to the exact solve, one ulp of the column's scale)."""
    return 8 * max(d_ref, EPS * scale)


def assert_within_project_bar(got, want, what):
    """tests/test_tri_gpu.py:_compare: 1e-7 m for data within 100 m, 1e-9 relative beyond."""
    d = np.abs(got - want)
    near = np.abs(want) <= 100.0
    assert not d[near].size or d[near].max() <= 1e-7, f'{what}: {d[near].max()} m from scipy'
    assert (d[~near] <= 1e-9 * np.abs(want[~near])).all(), f'{what}: beyond 100 m, relative {np.max(d[~near] / np.abs(want[~near]))}'


def check_interpolation(run, F, C, kind, verbose=False):
    """run(coords, labels, max_gap, kind) -> (out, status) on case(F, C) at every max_gap of MAX_GAPS.  Kinds None and
    'linear': the mirror's bits.  Spline kinds: the mirror's NaN pattern and untouched samples, scipy's values within the
    project's bar, and at F <= 257 within 8 x max(d_ref, 2^-52 scale) per column, d_ref = max |scipy - exact| over the
    samples compared.  -> (columns compared, columns left out because scipy's own answer is not finite there)."""
    coords, labels = case(F, C)
    patches = case_patches(F, C, kind)
    compared = left_out = 0
    for max_gap in MAX_GAPS:
        want, status = interpolate(coords, labels, max_gap, kind, patches)
        got, got_status = run(coords, labels, max_gap, kind)
        assert np.array_equal(got_status, status), (F, C, kind, max_gap)
        if kind not in SPLINE_KINDS:
            assert same(got, want), (F, C, kind, max_gap, np.argwhere(~((got == want) | (np.isnan(got) & np.isnan(want))))[:4])
            continue
        assert np.array_equal(np.isnan(got), np.isnan(want)), (F, C, kind, max_gap)
        good = ~bad_samples(coords)
        assert np.array_equal(got[good], coords[good])
        for c, patch in enumerate(patches):
            if patch is None:
                assert same(got[:, c], coords[:, c])
                left_out += max_gap == MAX_GAPS[0] and bool(status[c])
                continue
            pos = patch[0]
            kept = np.isfinite(want[pos, c])
            if not np.isfinite(patch[1]).all():
                left_out += max_gap == MAX_GAPS[0]
                continue
            compared += max_gap == MAX_GAPS[0]
            if not kept.any():
                continue
            g, w = got[pos, c][kept], want[pos, c][kept]
            assert_within_project_bar(g, w, f'F={F} column {c} {kind} max_gap={max_gap}')
            if F <= EXACT_UP_TO:
                exact = case_exact(F, c, kind)[kept]
                d_ref, scale = np.abs(w - exact).max(), np.abs(coords[good[:, c], c]).max()
                d = np.abs(g - w).max()
                if verbose:
                    print(f'F={F} c={c} {kind} max_gap={max_gap}: |kernel - scipy| {d:.3e}  d_ref {d_ref:.3e}  bound {spline_bound(d_ref, scale):.3e}')
                assert d <= spline_bound(d_ref, scale), (F, c, kind, max_gap, d, d_ref, scale)
    return compared, left_out


def golden_cases(golden_dir):
    import os
    z = np.load(os.path.join(golden_dir, 'gaps_units.npz'), allow_pickle=False)
    for i in range(int(z['n_cases'])):
        kind = str(z[f'c{i}_kind'])
        yield i, z, (None if kind == 'none' else kind)


def check_golden(run, golden_dir, verbose=False):
    """The recorded columns of the reference's interpolate_zeros_nans: None and 'linear' bit for bit; the spline kinds
    within the project's bar of the reference and within 8 x max(d_ref, 2^-52 scale) of the recorded exact solve."""
    n = {k: 0 for k in KINDS}
    for i, z, kind in golden_cases(golden_dir):
        col, index, N, want = z[f'c{i}_col'], z[f'c{i}_index'], float(z[f'c{i}_N']), z[f'c{i}_out']
        got, status = run(col[:, None], index, N, kind)
        got = got[:, 0]
        assert not status.any()
        n[kind] += 1
        if kind not in SPLINE_KINDS:
            assert same(got, want), (i, kind)
            continue
        assert np.array_equal(np.isnan(got), np.isnan(want)), (i, kind)
        took = bad_samples(col) & np.isfinite(want)
        assert np.array_equal(got[~bad_samples(col)], col[~bad_samples(col)])
        if (~bad_samples(col)).sum() <= 4:                        # untouched: its bad samples are what they were
            assert same(got, col) and same(want, col)
            continue
        if not took.any():
            continue
        assert_within_project_bar(got[took], want[took], f'golden {i} {kind}')
        d, bound = np.abs(got[took] - z[f'c{i}_exact'][took]).max(), spline_bound(float(z[f'c{i}_d_ref']), float(z[f'c{i}_scale']))
        if verbose:
            print(f'golden {i} {kind}: |kernel - exact| {d:.3e}  d_ref {float(z[f"c{i}_d_ref"]):.3e}  bound {bound:.3e}')
        assert d <= bound, (i, kind, d, bound)
    assert min(n.values()) >= 5, n


def fill_inputs(F, C):
    """The case's table as it is, and as the interpolation leaves it, with +-inf planted."""
    coords, labels = case(F, C)
    filled = interpolate(coords, labels, 20, 'linear', case_patches(F, C, 'linear'))[0]
    filled[F // 2, 0], filled[F - 1, C - 1] = np.inf, -np.inf
    return coords, filled


def check_fill(run, F, C):
    for table in fill_inputs(F, C):
        for how in ('last_value', 'zeros', 'nan', None):
            before = table.copy()
            got = run(table, how)
            assert same(got, fill(table, how)), (F, C, how)
            assert same(table, before)


def check_runs(run, F, C):
    x = fill_inputs(F, C)[1]
    for max_gap in MAX_GAPS:
        for first, last in ((-1, F), (1, F - 2), (F // 3, F - F // 4)):
            assert run(x, first, last, max_gap) == runs(x, first, last, max_gap), (F, C, max_gap, first, last)
