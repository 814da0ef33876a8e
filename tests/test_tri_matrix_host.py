"""What tests/test_tri_matrix_gpu.py rests on, checked without a GPU: its case list covers the kernels, its `runaway`
workloads do leave the undistortion through the `icdist < 0` exit, and the two CPU oracles -- the NumPy restatement of the
reference (oracle/triangulation_ref.py) and the C oracle the GPU test compares with (oracle/tri_oracle.c) -- agree on a
reduced copy (20 frames) of every case of up to 12 cameras, at the bars of test_tri_gpu._compare.  A workload on which the
references disagree with each other would be no test of a kernel."""
import multiprocessing
import os

import numpy as np
import pytest

import rigs
from test_tri_matrix_gpu import CASES, K, LIK_THR, camera_class, case_id, fused_applies, make_case, oracle_run, swap_table

REDUCED_FRAMES = 20
FRAMES_PER_TASK = 4
HOST_CASES = [c for c in CASES if c[2] <= 12]


def test_case_list_covers_the_kernels():
    """All eight (dtype, undistort, swap) combinations on the work-list path in every camera-count class, both camera counts
    of every class, every rig family and every distortion profile with undistortion at least twice, the pairs and the
    runaway cases the module's header names, every path where it applies, the tiled level 0 at up to 8 cameras."""
    combos = {(f64, und, sw) for f64 in (False, True) for und in (False, True) for sw in (False, True)}
    for cls, counts in enumerate(((5, 8), (11, 16), (20, 32))):
        mine = [c for c in CASES if camera_class(c[2]) == cls]
        assert {c[3:6] for c in mine if c[6] == 'worklist' and not c[9]} == combos
        assert {c[2] for c in mine} == set(counts)
        assert sum(c[6] == 'auto' for c in mine) == 1
    assert all(c[1] in rigs.SCATTER and (c[1] != 'none') == c[4] for c in CASES)
    und = [c for c in CASES if c[4]]
    for fam in rigs.RIGS:
        assert sum(c[0] == fam for c in und) >= 2, fam
        assert any(c[0] == fam for c in CASES if not c[4]), fam
    for prof in ('mild5', 'wide', 'pincushion', 'runaway'):
        assert sum(c[1] == prof for c in und) >= 2, prof
    pairs = {(c[0], c[1]) for c in und}
    assert {('uhd', 'wide'), ('far_origin', 'mild5'), ('stadium', 'pincushion'), ('close', 'wide')} <= pairs
    assert any(c[1] == 'runaway' and c[2] == 8 and not c[3] for c in CASES)
    assert any(c[1] == 'runaway' and c[2] == 20 and c[3] for c in CASES)
    # float32 with undistortion at 9-16 cameras, without swap (direct<16>, U = true) and with it; float64 with swap above 8
    # cameras; float64 with undistortion and swap together
    assert any(not c[3] and c[4] and not c[5] and 9 <= c[2] <= 16 and c[6] == 'worklist' for c in CASES)
    assert any(not c[3] and c[4] and c[5] and 9 <= c[2] <= 16 for c in CASES)
    assert any(c[3] and c[5] and c[2] > 8 for c in CASES) and any(c[3] and c[4] and c[5] for c in CASES)
    # the one-launch kernels: only where they apply, in both forms, float32 in both of their classes, float64 in its one
    fused = [c for c in CASES if c[6] in ('onetile', 'twotiles')]
    assert all(fused_applies(c[2], c[3], c[4], c[5]) for c in fused)
    assert {(c[6], c[3], camera_class(c[2])) for c in fused} == {(p, f64, cls) for p in ('onetile', 'twotiles')
                                                                 for f64, cls in ((False, 0), (False, 1), (True, 0))}
    assert any(c[9] and c[2] <= 8 for c in CASES) and all(c[6] == 'worklist' for c in CASES if c[9])
    assert {c[7] for c in CASES} == {6.0, 15.0, 60.0}
    assert {c[8] for c in CASES if c[2] <= 16} == {2, 3, 4} and all(c[8] == c[2] - 4 for c in CASES if c[2] > 16 and c[8] != 2)
    assert [(c[2], c[8], c[10]) for c in CASES if c[2] > 16 and c[8] == 2] == [(32, 2, 0.01)]
    assert len(set(CASES)) == len(CASES)


@pytest.mark.parametrize('case', [c for c in CASES if c[1] == 'runaway'], ids=case_id)
def test_runaway_cases_take_the_fallback(case):
    """Observations of the full-size workload leave the undistortion at the first iteration (the observed pixel is already
    beyond the zero of 1 + k1 r^2 + k2 r^4 + k3 r^6) and at a later one (an iterate crosses it)."""
    wl, x, x64 = make_case(case)
    first, later = rigs.fallback_counts(x64, wl['cams'])
    n = int(np.isfinite(x64[..., 0]).sum())
    print(f'{case_id(case)}: of {n} observations {first} take the icdist < 0 exit at the first iteration, {later} at a later one')
    assert first > 0
    assert later > 0


def _numpy_oracle(task):
    from oracle import triangulation_ref as tr
    i, lo, hi = task
    fam, prof, C, f64, und, sw, path, thr, mc, tiled, _ = HOST_CASES[i]
    wl, x, x64 = make_case(HOST_CASES[i], REDUCED_FRAMES)
    with np.errstate(all='ignore'):
        return i, lo, tr.triangulate_batch(x64[lo:hi], wl['P'], wl['cams'] if und else None, swap_table(), LIK_THR, thr, mc, sw, und)


@pytest.fixture(scope='module')
def numpy_oracle_results():
    """The NumPy restatement on every reduced case, a few frames per task, on the CPUs this process may use (at most 16)."""
    tasks = [(i, lo, min(lo + FRAMES_PER_TASK, REDUCED_FRAMES)) for i in range(len(HOST_CASES))
             for lo in range(0, REDUCED_FRAMES, FRAMES_PER_TASK)]
    n = max(1, min(16, len(os.sched_getaffinity(0))))
    with multiprocessing.get_context('fork').Pool(n) as pool:
        parts = pool.map(_numpy_oracle, tasks, chunksize=1)
    out = {}
    for i, lo, res in sorted(parts, key=lambda p: (p[0], p[1])):
        out.setdefault(i, []).append(res)
    return {i: tuple(np.concatenate([r[j] for r in rs]) for j in range(4)) for i, rs in out.items()}


@pytest.mark.parametrize('i', range(len(HOST_CASES)), ids=[case_id(c) for c in HOST_CASES])
def test_the_oracles_agree_on_the_reduced_case(numpy_oracle_results, i):
    from test_tri_gpu import _compare
    case = HOST_CASES[i]
    wl, x, x64 = make_case(case, REDUCED_FRAMES)
    Qc, ec, nc, mc = oracle_run(case, wl, x64, threads=2)
    Qn, en, nn, mn = numpy_oracle_results[i]
    assert Qn.shape == Qc.shape == (REDUCED_FRAMES, 1, K, 3)
    dq = _compare(Qc, ec, nc, mc, Qn, en, nn, mn, case_id(case))
    if case[1] == 'runaway':
        first, later = rigs.fallback_counts(x64, wl['cams'])
        print(f'{case_id(case)}: fallback exits {first} + {later}')
        assert first > 0
    print(f'{case_id(case)}: {int(np.isfinite(en).sum())} of {en.size} units triangulated, worst |dQ| {dq:.2e} m')
