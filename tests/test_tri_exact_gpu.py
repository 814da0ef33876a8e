"""Every triangulation kernel against the exact weighted-DLT point on uneven likelihoods (tests/tri_exact.py).

The `low`, `zeros` and `heavy_light` likelihood modes of tests/rigs.py put weight ratios of 1e-3 .. 1e-6 between the cameras
of one unit.  The kernels solve the normal equations N = A^T A (p2s_tri_dev.h: accum_camera, smallest_eigvec with its
stopping rule, the `weak` refinement step, and the search's downdate by accum_camera<-1>), the reference and the oracles take
the SVD of A; on such inputs the two differ by the normal-equations error, which no other test bounds.  Here every unit a
kernel triangulates is compared, for the camera subset the kernel itself reports (mask, n_excl), with

  point    |Q - exact_point(kept)|_inf <= bar_u = max(tol_u, K e_cond_u): tol_u is test_tri_gpu's bar (1e-7 m within 100 m
           of the origin, 1e-9 |Q| beyond), e_cond_u the first-order eigenvector perturbation bound of tri_exact's header and
           K the constant that tests/test_tri_exact_host.py derives from a NumPy model of the arithmetic -- never from a
           kernel.  A kernel as good as an fp64 eigen-solve of its normal matrix can be stays inside; a wrong root, an
           unsettled iteration, a refinement that does not fire or a downdate that has cancelled the remaining cameras away
           does not
  error    |err - exact_error| <= TOL_E max(1, err) + J_u bar_u (J_u: tri_exact.jacobian_norm over the kept cameras)
  subset   with m_u = 2 (TOL_E max(1, err) + J_u bar_u): no candidate of the winning level has a float64 SVD error below
           err - m_u, none of a shallower level one below thr - m_u, err <= thr + m_u; a unit the kernel left NaN has no
           candidate below thr less the candidate's own margin at any level down to min_cameras.  At most the first three
           levels past level 0 are enumerated; a unit that would need more is held to the first two checks only (printed)
  oracle   NaN pattern and n_excl equal to oracle/tri_oracle's outside the ambiguous units (a level's best error within the
           margin of the threshold, or of the winning level's second best: tests/test_tri_exact_host.py caps them at 2 %)

Cases: 20 frames x 26 keypoints = 520 units (eight full tiles and a partial one); every unit of a `heavy_light` case and
94 - 147 of the 520 of the others search (tests/test_tri_exact_host.py asks for 64: one per lane of a tile), so the pooled
kernel's waves pool several units.  lik_thr is 0 for `heavy_light` (header of test_tri_screen_gpu.py) and `low`,
0.3 for `zeros` and `clamped`; thr 15 px.  The pooled cases take float32 input; float64 inputs get
test_tri_matrix_gpu.make_case's seeded +-1e-4 px so that the float64 kernels run.  The exact solve takes about 3 s of host
time per case (mpmath at 60 digits, one 4 x 4 eigen-decomposition per unit) and runs on every unit.
"""
import numpy as np
import pytest

import rigs
import tri_exact

pytestmark = pytest.mark.gpu

F, KP = 20, 26
THR = 15.0
LIK_THR = {'heavy_light': 0.0, 'low': 0.0, 'zeros': 0.3, 'clamped': 0.3}
LEVELS_PAST_0 = 3
AMBIGUOUS_CAP = 0.02

# (path, rig family, likelihood mode, cameras, min_cameras, float64 input, TUNE_POOL_TILES, TUNE_FORCE_TILED)
CASES = [
    ('pooled', 'far_origin', 'heavy_light', 3, 2, False, None, False),
    ('pooled', 'uhd', 'heavy_light', 4, 2, False, None, False),
    ('pooled', 'one_side', 'low', 3, 2, False, None, False),
    ('pooled', 'close', 'zeros', 6, 2, False, 2, False),
    ('pooled', 'far_origin', 'heavy_light', 8, 2, False, 5, False),
    ('pooled', 'far_origin', 'low', 8, 3, False, 6, False),
    ('pooled', 'mixed', 'heavy_light', 12, 3, False, None, False),
    ('pooled', 'stadium', 'heavy_light', 16, 4, False, None, False),
    ('pooled', 'ring', 'low', 16, 3, False, None, False),
    ('pooled', 'ring', 'clamped', 8, 2, False, None, False),                       # the control
    ('worklist', 'far_origin', 'heavy_light', 8, 2, False, None, False),           # direct<8>
    ('worklist', 'stadium', 'heavy_light', 16, 4, False, None, False),             # direct<16>
    ('worklist', 'far_origin', 'low', 11, 2, True, None, False),                   # tiled level 0
    ('worklist', 'far_origin', 'heavy_light', 5, 2, True, None, True),
    ('worklist', 'ring', 'heavy_light', 20, 16, False, None, False),               # and again with the deep rounds
    ('onetile', 'far_origin', 'heavy_light', 8, 2, False, None, False),
    ('twotiles', 'uhd', 'low', 5, 2, True, None, False),
]

# rigs.make_workload's seed per (family, mode, cameras); a workload with more than AMBIGUOUS_CAP ambiguous units gets
# another one (tests/test_tri_exact_host.py::test_ambiguous_units_are_rare).
SEEDS = {('far_origin', 'heavy_light', 3): 12}               # seed 11: 11 of 520 searching units ambiguous (2.1 %)
DEFAULT_SEED = 11


def case_id(c):
    path, fam, lik, C, mc, f64, tiles, tiled = c
    return (f'{path}-{fam}-{lik}-C{C}-min{mc}-{"f64" if f64 else "f32"}' + (f'-t{tiles}' if tiles else '')
            + ('-tiled' if tiled else ''))


def workload_key(c):
    return c[1], c[2], c[3], c[4], c[5]


def make_case(case):
    """(wl, x): rigs.make_workload's dict and the observations as the engine gets them."""
    path, fam, lik, C, mc, f64, tiles, tiled = case
    wl = rigs.make_workload(fam, C, F, KP, lik=lik, seed=SEEDS.get((fam, lik, C), DEFAULT_SEED))
    x = wl['xyl']
    if f64:
        x64 = x.astype(np.float64)
        x = x64 + np.random.default_rng(5).uniform(-1e-4, 1e-4, x.shape) * (x64 != 0)
    return wl, x


def analyse(case, wl, x):
    """What both this test and the host test need of every unit, by the reference's own walk (tri_exact.reference_walk) and
    one exact solve of its winner: list of dicts with
      unit, walk, n0
      searching      level 0 fails and a level 1 exists
      kept, q, lam, econd, bar, tol, jac, m, q_svd, err_svd    of the accepted subset (None / absent for a failed unit)
      ambiguous      some level's best error lies within its margin of the threshold, or the winning level's second-best
                     error (over the subsets that keep other cameras) within m_u of the best"""
    path, fam, lik, C, mc, f64, tiles, tiled = case
    out = []
    for unit, obs in zip(tri_exact.units_of(wl['P'], x, LIK_THR[lik]), _per_unit(x)):
        walk = tri_exact.reference_walk(unit, THR, mc, LEVELS_PAST_0)
        n0 = tri_exact.n0_norm(unit)
        r = {'unit': unit, 'obs': obs, 'walk': walk, 'n0': n0, 'kept': None, 'ambiguous': False, 'exact': {},
             'searching': bool(walk['levels']) and not walk['levels'][0]['err'][tri_exact.best_of(walk['levels'][0])] <= THR
             and tri_exact.max_level(unit, mc) >= 1}
        for level, cand in enumerate(walk['levels']):
            b = tri_exact.best_of(cand)
            e = float(cand['err'][b])
            if not np.isfinite(e):
                continue
            if walk['won'] == (level, b):
                r.update(solve(r, cand['kept'][b]))
                r.update(kept=cand['kept'][b], q_svd=cand['Q'][b], err_svd=e)
                m = r['m'] = tri_exact.margin(unit, r['kept'], r['q'], e, r['bar'])
                other = (cand['kept'] != cand['kept'][b]).any(axis=1) & ~np.isnan(cand['err'])
                if other.any() and cand['err'][other].min() - e <= m:
                    r['ambiguous'] = True
            else:
                m = candidate_margin(unit, n0, cand, b)
            if abs(e - THR) <= m:
                r['ambiguous'] = True
        out.append(r)
    return out


def _per_unit(x):
    return np.asarray(x)[:, 0].transpose(0, 2, 1, 3).reshape(F * KP, -1, 3)


def solve(r, kept):
    """The exact point of the subset `kept` of the unit of r and what hangs on it; one mpmath solve per subset."""
    key = tuple(np.flatnonzero(kept))
    if key not in r['exact']:
        unit = r['unit']
        q, lam = tri_exact.exact_point(unit.P, r['obs'], kept)
        econd = tri_exact.e_cond(r['n0'], lam, q)
        bar, tol = tri_exact.point_bar(q, econd)
        r['exact'][key] = {'q': q, 'lam': lam, 'econd': econd, 'bar': bar, 'tol': tol,
                           'jac': tri_exact.jacobian_norm(unit, kept, q)}
    return r['exact'][key]


def candidate_margin(unit, n0, cand, i):
    """The margin of a candidate that is not the winner, with e_cond from the float64 singular values (tri_exact.svd_e_cond)."""
    q, e = cand['Q'][i], float(cand['err'][i])
    if not (np.isfinite(q).all() and np.isfinite(e)):
        return 0.0
    bar, _ = tri_exact.point_bar(q, tri_exact.svd_e_cond(n0, cand['sv'][i], q))
    return tri_exact.margin(unit, cand['kept'][i], q, e, bar)


def oracle_run(case, wl, x, threads):
    from oracle import tri_oracle
    path, fam, lik, C, mc, f64, tiles, tiled = case
    return tri_oracle.triangulate_batch(np.asarray(x, dtype=np.float64), wl['P'], None, list(range(KP)), LIK_THR[lik], THR, mc,
                                        threads=threads)


def _triangulate(case, wl, x, deep_min=None):
    from pose2sim_amd.engine import Engine
    path, fam, lik, C, mc, f64, tiles, tiled = case
    eng = Engine(0)
    try:
        eng.set_tuning(Engine.TUNE_TRI_PATH, {'pooled': Engine.TRI_PATH_POOLED, 'worklist': Engine.TRI_PATH_WORKLIST,
                                              'onetile': Engine.TRI_PATH_ONE_TILE, 'twotiles': Engine.TRI_PATH_TWO_TILES}[path])
        if tiles:
            eng.set_tuning(Engine.TUNE_POOL_TILES, tiles)
        if tiled:
            eng.set_tuning(Engine.TUNE_FORCE_TILED, 1)
        if deep_min is not None:
            eng.set_tuning(Engine.TUNE_DEEP_MIN_SUBSETS, deep_min)
        eng.set_calibration(wl['P'])
        eng.tri_stats(reset=True)
        out = eng.triangulate(x, eng.tri_params(THR, LIK_THR[lik], mc))
        return out, eng.tri_stats(reset=True)
    finally:
        eng.close()


def check_case(case, got, units, oracle, what):
    """Prints the case's line and returns the failures (strings) of one kernel run against the exact solve."""
    from test_tri_gpu import TOL_E
    path, fam, lik, C, mc, f64, tiles, tiled = case
    Q = got[0].reshape(-1, 3)
    err = got[1].reshape(-1).astype(np.float64)
    nex, mask = got[2].reshape(-1), got[3].reshape(-1)
    er, nr = oracle[1].reshape(-1), oracle[2].reshape(-1)
    fails = []
    rows = []          # per compared unit: |dQ|, e_cond, bar, tol, |dQ| of the float64 SVD, error difference
    n_capped = 0
    for u, r in enumerate(units):
        unit = r['unit']
        if not r['ambiguous']:
            if np.isnan(err[u]) != np.isnan(er[u]):
                fails.append(f'unit {u}: NaN pattern differs from the C oracle (kernel err {err[u]}, oracle {er[u]})')
            elif int(nex[u]) != int(nr[u]):
                fails.append(f'unit {u}: n_excl {int(nex[u])}, C oracle {int(nr[u])}')
        top = tri_exact.max_level(unit, mc)
        if np.isnan(err[u]):
            assert np.isnan(Q[u]).all()
            n_capped += top > LEVELS_PAST_0
            for level in range(min(top, LEVELS_PAST_0) + 1):
                cand = _level(r, level)
                for i in np.flatnonzero(cand['err'] < THR):
                    if cand['err'][i] < THR - candidate_margin(unit, r['n0'], cand, i):
                        fails.append(f'unit {u}: left NaN, but level {level} subset {cand["removed"][i]} has error {cand["err"][i]:.6f}')
                        break
            continue
        kept = tri_exact.kept_of(mask[u], nex[u], unit.valid)
        s = solve(r, kept)
        dq = float(np.abs(Q[u] - s['q']).max())
        ee = tri_exact.exact_error(s['q'], unit, kept)
        de = abs(err[u] - ee)
        level = int((unit.valid & ~kept).sum())
        cand = _level(r, level) if level <= LEVELS_PAST_0 else None
        dq_svd = np.nan
        if cand is not None:
            same = np.flatnonzero((cand['kept'] == kept).all(axis=1))
            dq_svd = float(np.abs(cand['Q'][same[0]] - s['q']).max())
        rows.append((dq, s['econd'], s['bar'], s['tol'], dq_svd, de))
        if not dq <= s['bar']:
            fails.append(f'unit {u}: |dQ| {dq:.3e} m > bar {s["bar"]:.3e} (tol {s["tol"]:.1e}, e_cond {s["econd"]:.3e}, ratio '
                         f'{dq / s["econd"]:.1f}), kept {np.flatnonzero(kept)}, level {level}')
        if not de <= TOL_E * max(1.0, err[u]) + s['jac'] * s['bar']:
            fails.append(f'unit {u}: err {err[u]:.7f} px, exact {ee:.7f} px')
        m = tri_exact.margin(unit, kept, s['q'], err[u], s['bar'])
        if not err[u] <= THR + m:
            fails.append(f'unit {u}: accepted at {err[u]:.6f} px > thr + {m:.2e}')
        if cand is None:
            n_capped += 1
            continue
        if cand['err'].min() < err[u] - m:
            i = int(np.argmin(cand['err']))
            fails.append(f'unit {u}: level {level} subset {cand["removed"][i]} has error {cand["err"][i]:.7f} < {err[u]:.7f} - {m:.2e}')
        for lv in range(level):
            c2 = _level(r, lv)
            if np.nanmin(np.where(np.isnan(c2['err']), np.inf, c2['err'])) < THR - m:
                fails.append(f'unit {u}: won at level {level}, but level {lv} has a subset at {np.nanmin(c2["err"]):.6f} px')
                break
    a = np.array(rows).reshape(-1, 6)
    over = a[:, 0] > 1e-7
    n_search = sum(r['searching'] for r in units)
    with np.errstate(invalid='ignore', divide='ignore'):
        ratio = float((a[:, 0] / a[:, 1]).max()) if len(a) else 0.0
    print(f'EXACT | {what} | {len(a)} | {n_search} | {a[:, 0].max() if len(a) else 0.0:.2e} | {ratio:.2f} | '
          f'{100.0 * float((tri_exact.K * a[:, 1] > a[:, 3]).mean()) if len(a) else 0.0:.1f} % | '
          f'{int(over.sum())} (SVD: {np.nanmax(a[over, 4]) if over.any() and not np.isnan(a[over, 4]).all() else 0.0:.1e}) | '
          f'{a[:, 5].max() if len(a) else 0.0:.2e} | {sum(r["ambiguous"] for r in units)} | {int(n_capped)}')
    return fails


def _level(r, level):
    """The candidates of one level of the unit of r, from the walk where it went that far."""
    cache = r.setdefault('cand', {})
    if level not in cache:
        lv = r['walk']['levels']
        cache[level] = lv[level] if level < len(lv) else tri_exact.candidates(r['unit'], level)
    return cache[level]


HEADER = ('EXACT | case | units compared | searching | worst |dQ| m | worst |dQ| / e_cond | K e_cond > tol_u | units with |dQ| > 1e-7 m '
          '(float64 SVD on those) | worst |d err| px | ambiguous | past the enumeration cap')


@pytest.mark.parametrize('case', CASES, ids=[case_id(c) for c in CASES])
def test_kernels_against_the_exact_point(case):
    import __graft_entry__ as entry
    entry.build_hip()
    from test_tri_gpu import oracle_threads
    path, fam, lik, C, mc, f64, tiles, tiled = case
    wl, x = make_case(case)
    assert (x.dtype == np.float64) == f64
    if f64:
        assert (x.astype(np.float32).astype(np.float64) != x).any()               # the float64 kernels do run
    got, stats = _triangulate(case, wl, x)
    units = analyse(case, wl, x)
    oracle = oracle_run(case, wl, x, oracle_threads(16))
    print(HEADER)
    fails = check_case(case, got, units, oracle, case_id(case))
    assert stats['search_units'] > 0, stats
    if C >= 17:
        # the deep rounds (p2s_tri_deep.hip) from 100 subsets per level on
        deep, dstats = _triangulate(case, wl, x, deep_min=100)
        assert dstats['subsets_evaluated'] > 0, dstats
        fails += check_case(case, deep, units, oracle, case_id(case) + '-deep100')
    assert not fails, f'{case_id(case)}: {len(fails)} failure(s); the first {min(10, len(fails))}:\n' + '\n'.join(fails[:10])
