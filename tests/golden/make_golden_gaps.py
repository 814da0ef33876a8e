"""Unit-level goldens of the gap interpolation, recorded from the reference's own interpolate_zeros_nans
(common.py:669-712): the five kinds (no kind at all, 'linear', 'slinear', 'quadratic', 'cubic') on a handful of columns
each, with gap limits, zeros, -0.0 and NaN as bad samples, gaps at both ends, a step of 2 in the index inside a bad run,
short columns and, for the linear kinds, +inf among the good samples.  For the spline kinds the 60-digit solve of
tests/gaps_exact.py is recorded beside the reference's answer, with d_ref = max |reference - exact| over the samples the
reference interpolated and scale = max |y| over the good samples.  -> gaps_units.npz"""
import os
import sys
import warnings

import numpy as np
import pandas as pd

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import ref_shim  # noqa: E402
import gaps_exact  # noqa: E402

KINDS = ['none', 'linear', 'slinear', 'quadratic', 'cubic']


def gen():
    common = ref_shim.load()[0]
    rng = np.random.default_rng(419)
    out, n = {}, 0
    for case in range(50):
        kind = KINDS[case % 5]
        L = [5, 6, 9, 40, 64, 65, 130, 257, 300, 520][case // 5]
        start = int(rng.integers(0, 50))
        col = np.cumsum(rng.normal(0, 0.01, L)) + rng.uniform(-2, 2)
        bad = rng.random(L) < rng.choice([0.05, 0.15, 0.4])
        if L > 30:
            g0 = int(rng.integers(2, L - 25))
            bad[g0:g0 + int(rng.integers(3, 23))] = True
            if case % 2:
                bad[:int(rng.integers(1, 4))] = True               # extrapolation at the start
                bad[-int(rng.integers(1, 4)):] = True              # ... and at the end
        else:
            bad[:] = False
            bad[rng.integers(0, L)] = True
        index = np.arange(start, start + L)
        if L > 8:
            index[L // 3:] += 1                                    # a step of 2 in the index, inside a bad run
            bad[L // 3 - 1:L // 3 + 1] = True
        which = rng.integers(0, 3, L)
        col[bad] = np.where(which[bad] == 0, np.nan, np.where(which[bad] == 1, 0.0, -0.0))
        if kind in ('none', 'linear') and L > 60 and case % 2 == 0:
            col[rng.choice(np.flatnonzero(~bad))] = np.inf
        N = [1, 3, 20, np.inf][(case // 5) % 4]
        s = pd.Series(col, index=index)
        with warnings.catch_warnings():
            warnings.simplefilter('ignore')
            res = common.interpolate_zeros_nans(s.copy()) if kind == 'none' else common.interpolate_zeros_nans(s.copy(), N, kind)
        res = np.asarray(res, dtype=float)
        out[f'c{n}_col'] = col; out[f'c{n}_index'] = index; out[f'c{n}_kind'] = np.array(kind)
        out[f'c{n}_N'] = np.array(np.inf if kind == 'none' else N); out[f'c{n}_out'] = res
        if kind in gaps_exact.ORDER:
            good = ~(np.isnan(col) | (col == 0))
            exact = np.full(L, np.nan)
            patch = gaps_exact.column(col, index, kind)
            if patch is not None:
                exact[patch[0]] = patch[1]
            took = ~good & np.isfinite(res) & np.isfinite(exact)
            out[f'c{n}_exact'] = exact
            out[f'c{n}_d_ref'] = np.array(np.abs(res[took] - exact[took]).max() if took.any() else 0.0)
            out[f'c{n}_scale'] = np.array(np.abs(col[good]).max())
        n += 1
    out['n_cases'] = np.array(n)
    path = os.path.join(HERE, 'gaps_units.npz')
    np.savez_compressed(path, **out)
    print('wrote gaps_units.npz:', n, 'columns,', os.path.getsize(path), 'bytes')


if __name__ == '__main__':
    gen()
