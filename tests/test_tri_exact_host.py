"""What tests/test_tri_exact_gpu.py rests on, checked without a GPU.  Nothing here runs the code under test: it validates the
references and the inputs.

1. the float64 SVD restatement (tri_exact.candidates) stays within 1e-9 m of the exact point on every compared unit, so its
   errors may stand for the exact ones where subsets are ranked;
2. the NumPy float64 model of the kernels' arithmetic (level-0 normal matrix in camera order, the winner's excluded cameras
   subtracted, numpy.linalg.eigh) stays within 4 e_cond of the exact point, and tri_exact.K is eight times its worst ratio,
   rounded up to a power of two;
3. at most 2 % of a case's searching units are ambiguous (tests/test_tri_exact_gpu.analyse), and at least 64 of the 520
   units of every case search;
4. the case list holds at least three cases in which K e_cond exceeds 1e-7 m for more than 10 % of the units (the bar is
   the conditioning there) and three in which it never does (the bar is test_tri_gpu's);
5. oracle/tri_oracle matches the exact point within 1e-9 m and picks the same subsets outside the ambiguous units.
"""
import math
import multiprocessing
import os

import numpy as np
import pytest

import tri_exact
from test_tri_exact_gpu import AMBIGUOUS_CAP, CASES, F, KP, analyse, case_id, make_case, oracle_run, workload_key

SVD_BAR_M = 1e-9
MODEL_BAR = 4.0

# one analysis per workload: the paths share them
WORKLOADS = []
for _c in CASES:
    if workload_key(_c) not in [workload_key(w) for w in WORKLOADS]:
        WORKLOADS.append(_c)


def _summarise(i):
    case = WORKLOADS[i]
    wl, x = make_case(case)
    units = analyse(case, wl, x)
    Qo, eo, no, mo = (a.reshape((F * KP,) + a.shape[3:]) for a in oracle_run(case, wl, x, threads=1))
    rows = []
    for u, r in enumerate(units):
        won = r['kept'] is not None
        row = {'searching': r['searching'], 'ambiguous': r['ambiguous'], 'won': won, 'complete': r['walk']['complete'],
               'oracle_nan': bool(np.isnan(eo[u])), 'oracle_n': int(no[u])}
        if won:
            model = tri_exact.model_point(r['unit'], r['kept'])
            row.update(d_svd=float(np.abs(r['q_svd'] - r['q']).max()), d_model=float(np.abs(model - r['q']).max()),
                       econd=r['econd'], tol=r['tol'], n_excl=int(len(r['kept']) - r['kept'].sum()),
                       d_oracle=float(np.abs(Qo[u] - r['q']).max()) if not np.isnan(eo[u]) else np.nan,
                       oracle_kept=bool(np.isnan(eo[u])) or bool((tri_exact.kept_of(mo[u], no[u], r['unit'].valid) == r['kept']).all()))
        rows.append(row)
    return rows


@pytest.fixture(scope='module')
def summaries():
    """The reference walk, one exact solve per triangulated unit, the model and the C oracle on every workload, on the CPUs
    this process may use (at most 16)."""
    n = max(1, min(16, len(os.sched_getaffinity(0)), len(WORKLOADS)))
    with multiprocessing.get_context('fork').Pool(n) as pool:
        out = pool.map(_summarise, range(len(WORKLOADS)), chunksize=1)
    return dict(zip((case_id(c) for c in WORKLOADS), out))


def _won(rows):
    return [r for r in rows if r['won']]


def test_svd_restatement_is_exact_to_1e_9_m(summaries):
    worst = 0.0
    for name, rows in summaries.items():
        d = max((r['d_svd'] for r in _won(rows)), default=0.0)
        print(f'{name}: float64 SVD within {d:.2e} m of the exact point on {len(_won(rows))} units')
        worst = max(worst, d)
    assert worst <= SVD_BAR_M


def test_model_ratio_and_K(summaries):
    worst = 0.0
    for name, rows in summaries.items():
        ratio = max((r['d_model'] / r['econd'] for r in _won(rows)), default=0.0)
        d = max((r['d_model'] for r in _won(rows)), default=0.0)
        print(f'{name}: the float64 normal-equations model is within {d:.2e} m of the exact point, worst |dq| / e_cond {ratio:.2f}')
        worst = max(worst, ratio)
    print(f'worst |dq| / e_cond over all cases: {worst:.3f}; tri_exact.MODEL_WORST_RATIO {tri_exact.MODEL_WORST_RATIO}, K {tri_exact.K:g}')
    assert worst <= MODEL_BAR
    # the recorded ratio may move in its last digits with the LAPACK build; K must be what the rule gives for either
    assert tri_exact.K == 2.0 ** math.ceil(math.log2(8.0 * tri_exact.MODEL_WORST_RATIO))
    assert tri_exact.K == 2.0 ** math.ceil(math.log2(8.0 * worst))


def test_ambiguous_units_are_rare(summaries):
    for name, rows in summaries.items():
        search = [r for r in rows if r['searching']]
        amb = sum(r['ambiguous'] for r in search)
        print(f'{name}: {len(search)} of {len(rows)} units search, {amb} of them ambiguous '
              f'({100.0 * amb / max(1, len(search)):.2f} %), {sum(not r["complete"] for r in rows)} past the enumeration cap')
        assert amb <= AMBIGUOUS_CAP * len(search), name
        assert len(search) >= 64, name               # a tile's worth of lanes: the pooled kernel's waves pool several units


def test_case_list_covers_both_regimes(summaries):
    above, never = 0, 0
    for name, rows in summaries.items():
        share = float(np.mean([tri_exact.K * r['econd'] > 1e-7 for r in _won(rows)]))
        print(f'{name}: K e_cond > 1e-7 m on {100.0 * share:.1f} % of the units')
        above += share > 0.10
        never += share == 0.0
    assert above >= 3 and never >= 3, (above, never)


def test_c_oracle_against_the_exact_point(summaries):
    for name, rows in summaries.items():
        d = [r['d_oracle'] for r in _won(rows) if r['oracle_kept'] and not r['oracle_nan']]
        print(f'{name}: oracle/tri_oracle within {max(d, default=0.0):.2e} m of the exact point on {len(d)} units')
        assert max(d, default=0.0) <= SVD_BAR_M, name
        for u, r in enumerate(rows):
            if r['ambiguous'] or not r['complete']:
                continue
            assert r['oracle_nan'] == (not r['won']), f'{name}: unit {u}'
            if r['won']:
                assert r['oracle_kept'] and r['oracle_n'] == r['n_excl'], f'{name}: unit {u}'
