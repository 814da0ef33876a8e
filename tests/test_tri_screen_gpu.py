"""The pooled triangulation kernel's fp32 screen (p2s_tri_pool.hip, tier A) on rigs and likelihoods it was not tuned on.

The screen drops a camera subset when its fp32 reprojection error, less a margin, cannot be the level's minimum; a wrong
drop changes the chosen cameras, the point and the error without any other sign.  Every case runs the pooled kernel
twice, screen on and screen off (every candidate evaluated in fp64), and asserts that Q, err, n_excl and mask are the
same bytes.  No oracle is involved there, so the conditioning of the reference's SVD does not matter.  The cases cover
every rig family and likelihood mode of tests/rigs.py, every instantiation of the kernel (3-4 cameras: 4-camera slots,
not exact and exact; 6 and 8: 8-camera slots with 2, 5 and 6 tiles pooled per wave; 9, 12 and 16: 16-camera slots,
observations taken eight at a time, fp64 normal matrix kept in the slot), thresholds of 1, 15 and 60 px, likelihood
thresholds of 0, 0.01 and 0.3 and min_cameras 2-4.  The low-likelihood cases hold 52 k units each: a NumPy model of the
unguarded screen wrongly dropped about one winner per 13 k searching units there.

The `clamped` case of every rig family is also checked unit by unit against the C oracle with the bars of
test_tri_gpu._compare.  The `low`, `zeros` and `heavy_light` cases are not: at a weight ratio of 1e-6 between the
cameras of a unit (likelihood 1e-3 against 1) the oracle's SVD of A is still within 1e-9 m of the exact point
(tests/test_tri_exact_host.py), but the kernel solves the normal equations A^T A, whose error there may pass the flat
1e-7 m bar (tests/sweeps/fuzz_params.py raises such likelihoods for the same reason).  That error is bounded unit by unit
by K e_cond in tests/test_tri_exact_gpu.py, against an exact multiprecision solve; here, screen on against screen off is
the bar.
"""
import os

import numpy as np
import pytest

import rigs

pytestmark = pytest.mark.gpu

F, K = 2000, 26                                      # 52 k units per case

# (rig family, likelihood mode, cameras, thr px, lik_thr, min_cameras, tiles per wave (6-8 cameras only), camera 1 = camera 0)
# (heavy_light runs with lik_thr 0: a threshold of 0.01 removes its light cameras and nothing is left to search; what the
# list covers is checked without a GPU by tests/test_rigs.py)
CASES = [
    ('ring', 'clamped', 8, 15.0, 0.3, 2, 5, False),
    ('ring', 'low', 8, 15.0, 0.0, 2, 5, False),
    ('ring', 'low', 8, 15.0, 0.01, 3, 2, False),
    ('ring', 'heavy_light', 8, 15.0, 0.0, 2, 6, False),
    ('ring', 'low', 16, 15.0, 0.0, 3, None, False),
    ('ring', 'heavy_light', 12, 15.0, 0.0, 2, None, False),
    ('ring', 'zeros', 4, 1.0, 0.3, 2, None, False),
    ('ring', 'clamped', 16, 60.0, 0.3, 4, None, True),
    ('ring', 'low', 3, 15.0, 0.0, 2, None, False),
    ('ring', 'heavy_light', 16, 15.0, 0.0, 4, None, True),
    ('uhd', 'clamped', 6, 15.0, 0.3, 2, 2, False),
    ('uhd', 'low', 8, 60.0, 0.0, 3, 5, False),
    ('uhd', 'heavy_light', 4, 15.0, 0.0, 2, None, False),
    ('uhd', 'low', 12, 15.0, 0.01, 4, None, False),
    ('uhd', 'zeros', 9, 60.0, 0.3, 3, None, False),
    ('far_origin', 'clamped', 8, 15.0, 0.3, 2, 5, False),
    ('far_origin', 'low', 8, 15.0, 0.0, 2, 5, False),
    ('far_origin', 'low', 6, 1.0, 0.0, 2, 6, False),
    ('far_origin', 'heavy_light', 8, 60.0, 0.0, 3, 2, False),
    ('far_origin', 'low', 16, 15.0, 0.0, 2, None, False),
    ('far_origin', 'heavy_light', 3, 15.0, 0.0, 2, None, False),
    ('far_origin', 'zeros', 12, 15.0, 0.3, 4, None, True),
    ('stadium', 'clamped', 12, 15.0, 0.3, 3, None, False),
    ('stadium', 'low', 4, 15.0, 0.0, 2, None, False),
    ('stadium', 'heavy_light', 16, 60.0, 0.0, 4, None, False),
    ('stadium', 'zeros', 6, 1.0, 0.3, 2, 5, False),
    ('stadium', 'low', 8, 15.0, 0.01, 2, 6, False),
    ('stadium', 'heavy_light', 9, 15.0, 0.0, 2, None, False),
    ('close', 'clamped', 4, 15.0, 0.3, 3, None, True),
    ('close', 'low', 6, 15.0, 0.0, 2, 2, False),
    ('close', 'heavy_light', 8, 15.0, 0.0, 2, 5, False),
    ('close', 'zeros', 16, 15.0, 0.3, 2, None, False),
    ('close', 'low', 9, 60.0, 0.01, 3, None, False),
    ('one_side', 'clamped', 8, 60.0, 0.3, 4, 6, False),
    ('one_side', 'low', 3, 1.0, 0.0, 2, None, False),
    ('one_side', 'heavy_light', 6, 15.0, 0.0, 3, 5, False),
    ('one_side', 'low', 12, 15.0, 0.0, 2, None, False),
    ('one_side', 'zeros', 4, 15.0, 0.3, 2, None, False),
    ('overhead', 'clamped', 9, 15.0, 0.3, 2, None, False),
    ('overhead', 'low', 6, 15.0, 0.0, 2, 5, True),
    ('overhead', 'heavy_light', 8, 15.0, 0.0, 2, 2, False),
    ('overhead', 'zeros', 3, 15.0, 0.3, 2, None, False),
    ('overhead', 'low', 16, 60.0, 0.01, 4, None, False),
    ('mixed', 'clamped', 16, 15.0, 0.3, 2, None, False),
    ('mixed', 'low', 8, 15.0, 0.0, 2, 5, False),
    ('mixed', 'heavy_light', 12, 60.0, 0.0, 3, None, False),
    ('mixed', 'zeros', 6, 60.0, 0.3, 4, 6, False),
    ('mixed', 'low', 4, 1.0, 0.0, 2, None, True),
]


def _case_id(c):
    fam, lik, C, thr, lt, mc, tiles, dup = c
    return f'{fam}-{lik}-C{C}-thr{thr:g}-lik{lt:g}-min{mc}' + (f'-t{tiles}' if tiles else '') + ('-dup' if dup else '')


@pytest.fixture(scope='module')
def engines():
    """The pooled kernel with the screen on and with it off."""
    import __graft_entry__ as entry
    entry.build_hip()
    from pose2sim_amd.engine import Engine
    out = {}
    for screen in (1, 0):
        eng = Engine(0)
        eng.set_tuning(Engine.TUNE_TRI_PATH, Engine.TRI_PATH_POOLED)
        eng.set_tuning(Engine.TUNE_SCREEN, screen)
        out[screen] = eng
    yield out
    for eng in out.values():
        eng.close()


def _level0_point(xyl_u, P, lik_thr):
    """fp64 DLT point of all valid cameras of one unit (x, y, likelihood per camera) -- the screen's centre c0."""
    N = np.zeros((4, 4))
    for c, (x, y, w) in enumerate(np.asarray(xyl_u, dtype=np.float64)):
        if not (np.isfinite(x) and np.isfinite(y) and np.isfinite(w)) or w < lik_thr or w == 0.0:
            continue
        A = (P[c][0] - x * P[c][2]) * w
        B = (P[c][1] - y * P[c][2]) * w
        N += np.outer(A, A) + np.outer(B, B)
    v = np.linalg.eigh(N)[1][:, 0]
    return v[:3] / v[3] if v[3] != 0 else np.full(3, np.nan)


def _describe(bad, wl, on, off, C, lik_thr):
    P = [np.asarray(p, dtype=np.float64) for p in wl['P']]
    x = wl['xyl'][:, 0].transpose(0, 2, 1, 3).reshape(-1, C, 3)      # [unit][camera][x, y, lik]
    lines = []
    for u in bad[:8]:
        w = x[u, :, 2]
        valid = np.isfinite(w) & np.isfinite(x[u, :, 0]) & np.isfinite(x[u, :, 1]) & (w >= lik_thr) & (w != 0)
        vbits = int(sum(1 << c for c in range(C) if valid[c]))
        c0 = _level0_point(x[u], P, lik_thr)
        wmin = float(w[valid].min()) if valid.any() else float('nan')
        lines.append(f'  frame {u // K} kpt {u % K}: C={C} valid={vbits:#0{C + 2}b} '
                     f'n_excl {int(on[2].reshape(-1)[u])}/{int(off[2].reshape(-1)[u])} '
                     f'mask {int(on[3].reshape(-1)[u]):#x}/{int(off[3].reshape(-1)[u]):#x} '
                     f'err {float(on[1].reshape(-1)[u]):.6g}/{float(off[1].reshape(-1)[u]):.6g} (on/off) '
                     f'|c0| {np.linalg.norm(c0):.2f} m, smallest likelihood {wmin:.3g}')
    return '\n'.join(lines)


@pytest.mark.parametrize('case', CASES, ids=[_case_id(c) for c in CASES])
def test_screen_on_equals_screen_off(engines, case):
    from pose2sim_amd.engine import Engine
    fam, lik, C, thr, lik_thr, min_cams, tiles, dup = case
    seed = 1000 + CASES.index(case)
    wl = rigs.make_workload(fam, C, F, K, lik=lik, seed=seed, dup=dup)
    outs, stats = {}, {}
    for screen, eng in engines.items():
        eng.set_tuning(Engine.TUNE_POOL_TILES, tiles or 5)
        eng.set_calibration(wl['P'])
        eng.tri_stats(reset=True)
        outs[screen] = eng.triangulate(wl['xyl'], eng.tri_params(thr, lik_thr, min_cams))
        stats[screen] = eng.tri_stats(reset=True)
    on, off = outs[1], outs[0]
    differ = np.zeros(F * K, dtype=bool)
    for a, b in zip(on, off):
        a = np.ascontiguousarray(a).reshape(F * K, -1).view(np.uint8).reshape(F * K, -1)
        b = np.ascontiguousarray(b).reshape(F * K, -1).view(np.uint8).reshape(F * K, -1)
        differ |= (a != b).any(axis=1)
    bad = np.flatnonzero(differ)
    assert bad.size == 0, (f'{_case_id(case)}: {bad.size} of {F * K} units differ between screen on and off '
                           f'(searching units {stats[0]["search_units"]}); the first {min(8, bad.size)}:\n'
                           + _describe(bad, wl, on, off, C, lik_thr))
    for a, b in zip(on, off):
        assert a.tobytes() == b.tobytes()
    # the pooled kernel did run and search, and with the screen off every candidate went to fp64
    assert stats[1]['screened_subsets'] > 0, stats
    assert stats[0]['screened_subsets'] == stats[0]['subsets_evaluated'], stats[0]
    assert stats[1]['subsets_evaluated'] <= stats[0]['subsets_evaluated']
    print(f'{_case_id(case)}: {stats[0]["search_units"]} searching units, '
          f'{stats[1]["subsets_evaluated"]} of {stats[0]["subsets_evaluated"]} subsets evaluated in fp64')
    if lik == 'clamped':
        from oracle import tri_oracle
        from test_tri_gpu import _compare, oracle_threads
        threads = oracle_threads(16)
        Qr, er, nr, mr = tri_oracle.triangulate_batch(wl['xyl'].astype(np.float64), wl['P'], None, list(range(K)), lik_thr, thr,
                                                      min_cams, threads=threads)
        _compare(*on, Qr, er, nr, mr, _case_id(case))
