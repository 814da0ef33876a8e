"""The work-list and one-launch triangulation kernels on distorted rigs: every template combination against the C oracle.

tests/test_tri_screen_gpu.py proves the pooled kernel on the eight rig families of tests/rigs.py; everything else in
triangulation -- undistortion, the L/R swap, 17-32 cameras, float64 observations, i.e. p2s_tri_level0_direct_kernel<T, U, L,
8 | 16>, p2s_tri_level0_kernel, p2s_tri_search_kernel, p2s_deep_eval_kernel<T, U, L> and the kernels of p2s_tri_fused.hip --
only ever saw synth.make_cameras' ring at 1080p with four small distortion terms.  CASES is the product of

  (dtype, undistort, lr_swap)   all eight combinations, in each of
  the camera-count classes      5 | 8 (direct<8>; two cases again with TUNE_FORCE_TILED), 11 | 16 (direct<16> for float32
                                without swap, the tiled level 0 otherwise), 20 | 32 (tiled level 0 and the deep rounds,
                                min_cameras = C - 4; one C = 32 case with min_cameras = 2 and 1 % outliers)
  the path                      TRI_PATH_WORKLIST for each of those; ONE_TILE and TWO_TILES where p2s_tri_fused.hip applies
                                (pinhole, no swap, float32 up to 16 cameras, float64 up to 8); AUTO once per class

with the rig families and the distortion profiles of tests/rigs.py (mild5, wide, pincushion, runaway) dealt over the cases:
every family and every profile runs with undistortion at least twice, among them uhd x wide (one float32 ulp of an
undistorted 4K / 8K coordinate is 2.4e-4 - 4.9e-4 px and moves a point by more than the 1e-7 m bar), far_origin x mild5,
stadium x pincushion, close x wide and four runaway cases whose observations leave undistort_point through the
`icdist < 0` exit.  Pinhole cases bring the work-list and one-launch paths to the eight geometries the pooled kernel passed.

Every unit of every case (300 frames x HALPE_26 = 7.8 k) is compared with oracle/tri_oracle through test_tri_gpu._compare at
its bars.  The likelihoods are rigs' `clamped` mode with a threshold of 0.3: at very low likelihoods the kernel's solve of the
normal equations may leave the flat 1e-7 m bar (header of test_tri_screen_gpu.py); tests/test_tri_exact_gpu.py covers those.

Thresholds follow the profile.  With undistortion the reference compares the UNDISTORTED observation with the reprojection
through the ORIGINAL K and distortion (triangulation.py:473, quirk Q4), so a unit's error is about the mean displacement of
its observations under undistortion: a few px for mild5 and runaway lenses, 10 - 20 px for pincushion, 25 - 40 px for `wide`
at 1080p (optim_K is 0.7 K there) and twice to four times that on the uhd rig.  A case whose units all fail its threshold
checks NaN against NaN, so `wide` runs at 60 px, pincushion at 15 or 60 px, and uhd x wide at 8 cameras with min_cameras = 2,
where every unit searches and four in five find a subset of cameras that passes.  tests/test_tri_matrix_host.py checks
without a GPU that the list covers what is promised above and that the two oracles agree on these workloads.
"""
import numpy as np
import pytest

import rigs

pytestmark = pytest.mark.gpu

F, K = 300, 26
LIK_THR = 0.3
PATHS = ('worklist', 'onetile', 'twotiles', 'auto')

# (rig family, distortion profile, cameras, float64 input, undistort, lr_swap, path, thr px, min_cameras, TUNE_FORCE_TILED,
#  outlier rate)
CASES = [
    # 5 | 8 cameras: p2s_tri_level0_direct_kernel<T, U, L, 8>
    ('ring', 'none', 5, False, False, False, 'worklist', 15.0, 2, False, 0.06),
    ('uhd', 'wide', 8, False, True, False, 'worklist', 60.0, 2, False, 0.06),
    ('far_origin', 'none', 8, False, False, True, 'worklist', 6.0, 3, False, 0.06),
    ('ring', 'runaway', 8, False, True, True, 'worklist', 15.0, 2, False, 0.06),
    ('stadium', 'none', 8, True, False, False, 'worklist', 15.0, 4, False, 0.06),
    ('close', 'wide', 5, True, True, False, 'worklist', 60.0, 2, False, 0.06),
    ('close', 'none', 5, True, False, True, 'worklist', 15.0, 2, False, 0.06),
    ('far_origin', 'mild5', 8, True, True, True, 'worklist', 6.0, 3, False, 0.06),
    # ... and the tiled level-0 kernel at the same camera counts
    ('far_origin', 'pincushion', 8, False, True, True, 'worklist', 15.0, 2, True, 0.06),
    ('ring', 'wide', 5, True, True, False, 'worklist', 60.0, 2, True, 0.06),
    # 11 | 16 cameras: direct<16> for float32 without swap, the tiled level 0 otherwise
    ('one_side', 'none', 11, False, False, False, 'worklist', 6.0, 2, False, 0.06),
    ('stadium', 'pincushion', 16, False, True, False, 'worklist', 15.0, 3, False, 0.06),
    ('overhead', 'none', 16, False, False, True, 'worklist', 15.0, 4, False, 0.06),
    ('overhead', 'mild5', 11, False, True, True, 'worklist', 15.0, 2, False, 0.06),
    ('mixed', 'none', 16, True, False, False, 'worklist', 15.0, 3, False, 0.06),
    ('mixed', 'pincushion', 11, True, True, False, 'worklist', 15.0, 4, False, 0.06),
    ('uhd', 'none', 11, True, False, True, 'worklist', 6.0, 2, False, 0.06),
    ('one_side', 'runaway', 16, True, True, True, 'worklist', 60.0, 3, False, 0.06),
    # 20 | 32 cameras, min_cameras = C - 4: tiled level 0 and the deep rounds
    ('ring', 'none', 20, False, False, False, 'worklist', 15.0, 16, False, 0.04),
    ('close', 'mild5', 32, False, True, False, 'worklist', 15.0, 28, False, 0.04),
    ('stadium', 'none', 32, False, False, True, 'worklist', 6.0, 28, False, 0.02),
    ('mixed', 'wide', 20, False, True, True, 'worklist', 60.0, 16, False, 0.02),
    ('far_origin', 'none', 32, True, False, False, 'worklist', 6.0, 28, False, 0.02),
    ('overhead', 'runaway', 20, True, True, False, 'worklist', 15.0, 16, False, 0.02),
    ('one_side', 'none', 20, True, False, True, 'worklist', 15.0, 16, False, 0.02),
    ('uhd', 'pincushion', 32, True, True, True, 'worklist', 60.0, 28, False, 0.02),
    # 32 cameras down to two, 1 % outliers
    ('stadium', 'mild5', 32, False, True, True, 'worklist', 15.0, 2, False, 0.01),
    # the dispatch itself, once per class
    ('overhead', 'none', 8, False, False, False, 'auto', 15.0, 2, False, 0.06),
    ('one_side', 'wide', 11, False, True, False, 'auto', 60.0, 3, False, 0.06),
    ('close', 'none', 20, False, False, True, 'auto', 15.0, 16, False, 0.02),
    # the one-launch kernels of p2s_tri_fused.hip where they apply
    ('mixed', 'none', 8, False, False, False, 'onetile', 15.0, 2, False, 0.06),
    ('uhd', 'none', 5, False, False, False, 'twotiles', 6.0, 3, False, 0.06),
    ('far_origin', 'none', 16, False, False, False, 'onetile', 6.0, 4, False, 0.06),
    ('close', 'none', 11, False, False, False, 'twotiles', 15.0, 2, False, 0.06),
    ('overhead', 'none', 5, True, False, False, 'onetile', 15.0, 2, False, 0.06),
    ('one_side', 'none', 8, True, False, False, 'twotiles', 6.0, 4, False, 0.06),
    # direct<16> with undistortion on a runaway lens: at 16 cameras and 60 px a scattered observation stays in the winning
    # subset of some units, so where the `icdist < 0` exit leaves it decides their exclusion counts (at 8 cameras it never does)
    ('far_origin', 'runaway', 16, False, True, False, 'worklist', 60.0, 4, False, 0.06),
]


def camera_class(C):
    return 0 if C <= 8 else 1 if C <= 16 else 2


def fused_applies(C, f64, undistort, lr_swap):
    """p2s_tri_fused_supports: pinhole, no swap, float32 up to 16 cameras, float64 up to 8."""
    return not undistort and not lr_swap and C <= (8 if f64 else 16)


def case_id(c):
    fam, prof, C, f64, und, sw, path, thr, mc, tiled, _ = c
    return (f'{fam}-{prof}-C{C}-{"f64" if f64 else "f32"}{"-undistort" if und else ""}{"-swap" if sw else ""}-{path}'
            f'-thr{thr:g}-min{mc}' + ('-tiled' if tiled else ''))


def swap_table():
    from pose2sim_amd import skeletons
    return skeletons.keypoints('HALPE_26')[2]


def make_case(case, frames=F):
    """The workload of one case: (wl, x, x64) -- rigs.make_workload's dict, the observations as the engine gets them (float32,
    or float64 values that are not float32-representable: a seeded +-1e-4 px on every coordinate) and as the oracles do."""
    fam, prof, C, f64, und, sw, path, thr, mc, tiled, p_out = case
    assert (prof != 'none') == und
    wl = rigs.make_workload(fam, C, frames, K, seed=2000 + CASES.index(case), p_outlier=p_out, distortion=prof,
                            p_lr_swap=0.02 if sw else 0.0, swap_idx=swap_table() if sw else None)
    x = wl['xyl']
    x64 = x.astype(np.float64)
    if f64:
        rng = np.random.default_rng(5)
        x64 = x64 + rng.uniform(-1e-4, 1e-4, x.shape) * (x64 != 0)
        x = x64
    return wl, x, x64


def oracle_run(case, wl, x64, threads):
    from oracle import tri_oracle
    fam, prof, C, f64, und, sw, path, thr, mc, tiled, _ = case
    return tri_oracle.triangulate_batch(x64, wl['P'], wl['cams'] if und else None, swap_table(), LIK_THR, thr, mc, sw, und,
                                        threads=threads)


def searching_units(x64, er, nr, C, min_cams):
    """(units that went past level 0, units that went past level 1) by the oracle's exclusion counts.  A unit with fewer
    valid cameras than min_cameras runs no level at all and is neither."""
    with np.errstate(invalid='ignore'):
        lik = x64[..., 2]
        invalid = (np.isnan(lik) | (lik < LIK_THR) | (lik == 0)).sum(axis=-2).reshape(-1)
    attempted = C - invalid >= min_cams
    extra = np.asarray(nr).reshape(-1) - invalid
    failed = np.isnan(np.asarray(er).reshape(-1))
    return int((attempted & ((extra >= 1) | failed)).sum()), int((attempted & (extra >= 2)).sum())


def _triangulate(case, wl, x, deep_min=None):
    from pose2sim_amd.engine import Engine
    fam, prof, C, f64, und, sw, path, thr, mc, tiled, _ = case
    eng = Engine(0)
    try:
        eng.set_tuning(Engine.TUNE_TRI_PATH, {'worklist': Engine.TRI_PATH_WORKLIST, 'onetile': Engine.TRI_PATH_ONE_TILE,
                                              'twotiles': Engine.TRI_PATH_TWO_TILES, 'auto': Engine.TRI_PATH_AUTO}[path])
        if tiled:
            eng.set_tuning(Engine.TUNE_FORCE_TILED, 1)
        if deep_min is not None:
            eng.set_tuning(Engine.TUNE_DEEP_MIN_SUBSETS, deep_min)
        eng.set_calibration(wl['P'], wl['cams'] if und else None)
        eng.tri_stats(reset=True)
        out = eng.triangulate(x, eng.tri_params(thr, LIK_THR, mc, und, sw), swap_table() if sw else None)
        return out, eng.tri_stats(reset=True)
    finally:
        eng.close()


@pytest.mark.parametrize('case', CASES, ids=[case_id(c) for c in CASES])
def test_kernel_matrix_against_the_oracle(case):
    import __graft_entry__ as entry
    entry.build_hip()
    from test_tri_gpu import _compare, oracle_threads
    fam, prof, C, f64, und, sw, path, thr, mc, tiled, _ = case
    wl, x, x64 = make_case(case)
    assert (x.dtype == np.float64) == f64
    if f64:
        assert (x64.astype(np.float32).astype(np.float64) != x64).any()          # the float64 kernels do run
    got, stats = _triangulate(case, wl, x)
    Qr, er, nr, mr = oracle_run(case, wl, x64, oracle_threads(16))
    n_search, n_deeper = searching_units(x64, er, nr, C, mc)
    both = ~np.isnan(er.reshape(-1)) & ~np.isnan(got[1].reshape(-1))
    dq = np.abs(got[0].reshape(-1, 3) - Qr.reshape(-1, 3)).max(axis=1)[both]
    de = (np.abs(got[1].reshape(-1).astype(np.float64) - er.reshape(-1)) / np.maximum(1.0, np.abs(er.reshape(-1))))[both]
    fb = rigs.fallback_counts(x64, wl['cams']) if und else (0, 0)
    print(f'MATRIX | {fam} | {prof} | {C} | {"f64" if f64 else "f32"}{" U" if und else ""}{" L" if sw else ""} | '
          f'{path}{" tiled" if tiled else ""} | thr {thr:g} min {mc} | {n_search} | {dq.max() if dq.size else 0.0:.2e} | '
          f'{de.max() if de.size else 0.0:.2e} | triangulated {int(both.sum())} of {F * K} | fallback exits {fb[0]} + {fb[1]}')
    _compare(*got, Qr, er, nr, mr, case_id(case))
    if prof == 'runaway':
        assert fb[0] > 0
    if C >= 17:
        # the deep rounds (p2s_tri_deep.hip) from 100 subsets per level on: the same bits, and they did run
        deep, dstats = _triangulate(case, wl, x, deep_min=100)
        for a, b, what in zip(got, deep, ('Q', 'err', 'n_excl', 'mask')):
            assert a.tobytes() == b.tobytes(), f'{case_id(case)}: {what} changes with TUNE_DEEP_MIN_SUBSETS = 100'
        assert stats['subsets_evaluated'] > 0 and dstats['subsets_evaluated'] > 0, (stats, dstats)
        assert n_deeper > 0, f'{case_id(case)}: no unit went past level 1'
