"""What of the extrinsics from scratch needs no GPU: the mirror against the truth, the library's host path (ctx == NULL runs
the kernels' per-hypothesis and per-point functions) against the mirror, the assembly on exact pair poses, the refusals,
the samples and the command line."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import relpose_numpy as rn
import rigs
from pose2sim_amd import _lib, engine
from pose2sim_amd import calib_from_keypoints as cfk
from test_relpose_gpu import compare_hypotheses, compare_results, sliced

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# (family, cameras, noise px, outliers, hypotheses, centres m, ||R - R_true||_F): what the start may be off by.  The last
# two are not tolerances of arithmetic but of the method on 20 frames: Engine.refine_extrinsics reaches the oracle's minimum
# from 4 cm and 1.5 degrees on every family and, in test_relpose_gpu.py, from each of these starts; the
# figures are 3 x what these seeds give (printed), so that another seed of the same case stays inside.
TABLE = [('ring', 2, 0.5, 0.05, 512, 0.005, 0.004), ('ring', 3, 0.5, 0.05, 512, 0.05, 0.02), ('ring', 4, 0.5, 0.05, 512, 0.35, 0.12),
         ('overhead', 4, 0.5, 0.05, 512, 0.09, 0.045), ('one_side', 4, 0.5, 0.05, 512, 0.10, 0.03), ('stadium', 4, 0.5, 0.05, 512, 7.0, 0.3),
         ('ring', 8, 1.5, 0.15, 512, 0.2, 0.07), ('ring', 4, 1.5, 0.30, 1024, 1.0, 0.4)]


def start_error(case, R, T):
    Ra, ca, ct = rn.align(R, T, case['R'], case['t'])
    return float(np.abs(ca - ct).max()), float(max(np.linalg.norm(Ra[c] - case['R'][c]) for c in range(len(Ra))))


def test_entry_points_are_bound_as_optional():
    new = {'p2s_relative_poses_host', 'p2s_relpose_kernel_ms'}
    assert new <= _lib.OPTIONAL and new <= set(_lib.SIGNATURES)
    txt = open(os.path.join(ROOT, 'include', 'p2s.h')).read()
    defs = {m.group(1): int(m.group(2)) for m in re.finditer(r'#define\s+(P2S_RELPOSE_[A-Z_]+)\s+(\d+)', txt)}
    assert defs == {'P2S_RELPOSE_TILE': _lib.P2S_RELPOSE_TILE, 'P2S_RELPOSE_MAX_CHUNKS': _lib.P2S_RELPOSE_MAX_CHUNKS,
                    'P2S_RELPOSE_MAX_PARTS': _lib.P2S_RELPOSE_MAX_PARTS, 'P2S_RELPOSE_MIN_SAMPLE': _lib.P2S_RELPOSE_MIN_SAMPLE,
                    'P2S_RELPOSE_MAX_SAMPLE': _lib.P2S_RELPOSE_MAX_SAMPLE}
    assert len(_lib.SIGNATURES['p2s_relative_poses_host'][1]) == 25 and C.sizeof(C.c_void_p) == 8


def test_mirror_recovers_the_cameras_exactly_at_zero_noise():
    cs = rn.walk_case('ring', 3, 8, 13, seed=3, noise_px=0.0)
    xn, us, pairs, smp, thr2 = rn.inputs(cs, H=64)
    ref = rn.relative_poses(xn, us, pairs, smp, thr2)
    dc, dr = start_error(cs, *rn.cameras(3, xn, pairs, ref))
    print(f'mirror at zero noise: centres {dc:.3e} m, rotations {dr:.3e} from the truth')
    assert dc <= rn.ZERO_NOISE_C and dr <= rn.ZERO_NOISE_R and (ref['inliers'] == 104).all() and (ref['front'] == 104).all()


@pytest.mark.parametrize('family, Cn, noise, p_out, H, c_max, r_max', TABLE)
def test_mirror_and_host_path_against_the_truth(family, Cn, noise, p_out, H, c_max, r_max):
    """The start that the mirror's pair poses assemble to lies within reach of the refinement; the library's host path gives
    the mirror's winners, refits, counts and masks, and its E, R, t and costs within the bounds."""
    cs = rn.walk_case(family, Cn, 20, 13, seed=Cn, noise_px=noise, p_outlier=p_out)
    xn, us, pairs, smp, thr2 = rn.inputs(cs, H=H)
    ref = rn.relative_poses(xn, us, pairs, smp, thr2)
    dc, dr = start_error(cs, *rn.cameras(Cn, xn, pairs, ref))
    got = engine.relative_poses_host(xn, us, pairs, smp, thr2)
    dch, drh = start_error(cs, *rn.cameras(Cn, xn, pairs, got))
    print(f'{family} {Cn}, {noise} px, {p_out:.0%} outliers: start centres {dc:.3e} m, rotations {dr:.3e} ({np.degrees(dr / np.sqrt(2)):.2f} deg) '
          f'from the truth; host path {dch:.3e} m, {drh:.3e}; inliers {ref["inliers"].min()} .. {ref["inliers"].max()}')
    assert dc <= c_max and dr <= r_max and dch <= c_max and drh <= r_max
    assert rn.winners_are_clear(ref), 'two best costs too close'
    assert rn.no_point_at_the_threshold(ref) and ref['near_final'].min() > rn.COST_REL_BOUND
    for k in ('winner', 'refits', 'inliers', 'front', 'mask'):
        assert np.array_equal(got[k], ref[k]), k
    dE = np.abs(rn.match_sign(got['E'], ref['E']) - ref['E']).max()
    dR, dt = np.abs(got['R'] - ref['R']).max(), np.abs(got['t'] - ref['t']).max()
    dcost = (np.abs(got['cost'] - ref['cost']) / ref['cost']).max()
    print(f'    host path against the mirror: E {dE:.2e}, R {dR:.2e}, t {dt:.2e}, cost {dcost:.2e} relative')
    assert dE <= rn.WIN_E_BOUND and dR <= rn.RT_BOUND and dt <= rn.RT_BOUND and dcost <= rn.RESULT_COST_REL_BOUND


@pytest.mark.parametrize('Cn, N, H, m, seed', [(32, 1025, 8, 8, 15)])
def test_host_path_passes_of_more_tiles_than_parts(Cn, N, H, m, seed):
    """496 pairs at 1025 points: the per-point passes take 3 parts over 5 tiles (2, 2 and 1 of them); the refits leave pairs
    out of a pass and keep others in."""
    xn, us, pairs, smp, thr2 = sliced(Cn, N, H, m, seed)
    ref = rn.relative_poses(xn, us, pairs, smp, thr2)
    got = engine.relative_poses_host(xn, us, pairs, smp, thr2, all_hypotheses=True)
    assert -(-N // _lib.P2S_RELPOSE_TILE) == 5 and len(pairs) == 496
    assert rn.winners_are_clear(ref) and (ref['winner'] >= 0).all()
    assert np.bincount(ref['refits'], minlength=4).min() > 0                  # pairs with 0, 1, 2 and 3 refits kept
    tag = f'host path, C {Cn} (P {len(pairs)}), N {N}, H {H}, m {m}'
    compare_hypotheses(got, ref, xn, us, pairs, thr2, tag)
    compare_results(got, ref, tag)


def test_host_path_every_hypothesis_and_its_own_refusals():
    cs = rn.walk_case('ring', 3, 5, 13, seed=5)
    xn, us, pairs, _, thr2 = rn.inputs(cs, H=1)
    us[2, 5:] = False                                   # camera 2: five points, fewer than a sample
    us[0, 7] = False
    xn[1, 9] = np.nan                                   # usable, and not a number
    smp = cfk.draw_samples(us & np.isfinite(xn).all(axis=-1), pairs, 40, 8, seed=1)
    smp[0, 3, 5] = smp[0, 3, 1]                         # a repeated index
    smp[0, 4, 0] = 65                                   # past the end
    smp[0, 5, 2] = -1
    smp[0, 6, 7] = 7                                    # not usable in camera 0
    smp[0, 7, 7] = 9                                    # NaN in camera 1
    ref = rn.relative_poses(xn, us, pairs, smp, thr2)
    got = engine.relative_poses_host(xn, us, pairs, smp, thr2, all_hypotheses=True)
    assert (smp[1:] == -1).all() and (got['winner'][1:] == -1).all() and np.isnan(got['E'][1:]).all() and np.isnan(got['cost'][1:]).all()
    assert not got['mask'][1:].any() and not got['inliers'][1:].any() and not got['front'][1:].any() and np.isnan(got['R'][1:]).all()
    assert np.isinf(got['hyp_cost'][0, 3:8]).all() and not got['hyp_inliers'][0, 3:8].any() and np.isnan(got['hyp_E'][0, 3:8]).all()
    assert np.isfinite(got['hyp_cost'][0, :3]).all() and np.isfinite(got['hyp_cost'][0, 8:]).all()
    assert not got['mask'][0, 7] and not got['mask'][0, 9]
    compared = ref['hyp_cond'][0] >= rn.COND_FLOOR
    assert np.array_equal(got['hyp_inliers'], ref['hyp_inliers']) and got['winner'][0] == ref['winner'][0]
    dE = np.abs(rn.match_sign(got['hyp_E'][0], ref['hyp_E'][0]) - ref['hyp_E'][0]).max(axis=(-2, -1))
    assert np.nanmax((dE * ref['hyp_cond'][0])[compared]) <= rn.HYP_E_SCALED_BOUND


def test_scoring_on_a_stride_of_the_points():
    cs = rn.walk_case('ring', 2, 40, 13, seed=2)
    xn, us, pairs, smp, thr2 = rn.inputs(cs, H=32)
    ref = rn.relative_poses(xn, us, pairs, smp, thr2, score_points=100)
    got = engine.relative_poses_host(xn, us, pairs, smp, thr2, all_hypotheses=True, score_points=100)
    assert ref['hyp_inliers'].max() <= 100 < ref['inliers'][0]
    for k in ('hyp_inliers', 'winner', 'refits', 'inliers', 'front', 'mask'):
        assert np.array_equal(got[k], ref[k]), k
    assert abs(got['cost'][0] - ref['cost'][0]) <= rn.RESULT_COST_REL_BOUND * ref['cost'][0]


def exact_pairs(case, pairs, usable, withheld=()):
    """Exact pair poses with every mutually usable point an inlier; nothing for the pairs in `withheld`."""
    R, t = rn.pair_truth(case['R'], case['t'], pairs)
    mask = np.array([usable[a] & usable[b] for a, b in pairs])
    for p in withheld:
        R[p], t[p], mask[p] = np.nan, np.nan, False
    return {'R': R, 't': t, 'mask': mask, 'inliers': mask.sum(axis=1)}


def test_assembly_on_exact_pair_poses():
    for family, Cn in (('ring', 4), ('overhead', 4), ('stadium', 5)):
        cs = rn.walk_case(family, Cn, 8, 13, seed=1, noise_px=0.0)
        xn, us, pairs, _, _ = rn.inputs(cs, H=1)
        res = exact_pairs(cs, pairs, us)
        R, T, X, edges = cfk.assemble(Cn, xn, pairs, res['R'], res['t'], res['inliers'], res['mask'])
        dc, dr = start_error(cs, R, T)
        print(f'{family} {Cn}: assembled from exact pairs, centres {dc:.3e} m, rotations {dr:.3e}')
        assert dc <= rn.ZERO_NOISE_C and dr <= rn.ZERO_NOISE_R and np.array_equal(R[0], np.eye(3)) and not T[0].any()
        assert np.isclose(np.linalg.norm(T[edges[0][1]]), 1.0, atol=1e-14) and np.isfinite(X).all()


def test_assembly_chains_through_the_tree():
    """Camera 0 shares enough points with camera 1 only: the tree has to go 0 - 1 - ..., and the scale of the later edges comes
    from points that cameras 0 and 1 placed."""
    cs = rn.walk_case('ring', 4, 10, 13, seed=7, noise_px=0.0)
    xn, us, pairs, _, _ = rn.inputs(cs, H=1)
    us[0, 52:] = False                                  # camera 0: the first 52 points
    us[2, :32] = False                                  # cameras 2 and 3: from point 32 on, 20 in common with camera 0
    us[3, :32] = False
    res = exact_pairs(cs, pairs, us)
    assert [int(res['inliers'][p]) for p in range(3)] == [52, 20, 20]
    R, T, X, edges = cfk.assemble(4, xn, pairs, res['R'], res['t'], res['inliers'], res['mask'], min_inliers=30)
    assert edges[0][:2] == (0, 1) and all(a != 0 for a, _, _, _, _ in edges[1:]) and all(k >= 20 for *_, k in edges[1:])
    dc, dr = start_error(cs, R, T)
    assert dc <= rn.ZERO_NOISE_C and dr <= rn.ZERO_NOISE_R
    # a camera that no edge reaches is named
    res = exact_pairs(cs, pairs, us, withheld=[2, 4, 5])
    names = ['north', 'east', 'south', 'west']
    with pytest.raises(ValueError, match='^west: no camera pair with 30 or more inliers'):
        cfk.assemble(4, xn, pairs, res['R'], res['t'], res['inliers'], res['mask'], min_inliers=30, names=names)


def test_refusals_without_a_device():
    cs = rn.walk_case('ring', 3, 5, 13, seed=0)
    xn, us, pairs, smp, thr2 = rn.inputs(cs, H=4)

    def call(**kw):
        a = dict(xn=xn, usable=us, pairs=pairs, samples=smp, thr2=thr2)
        a.update(kw)
        return engine.relative_poses_host(a['xn'], a['usable'], a['pairs'], a['samples'], a['thr2'], **{k: v for k, v in kw.items() if k == 'rounds'})

    with pytest.raises(_lib.P2sError, match=r'n_cams=1 outside \[2, 32\]'):
        call(xn=xn[:1], usable=us[:1])
    with pytest.raises(_lib.P2sError, match=r'n_cams=33 outside \[2, 32\]'):
        call(xn=np.tile(xn, (11, 1, 1)), usable=np.tile(us, (11, 1)))
    for m in (7, 17):
        with pytest.raises(_lib.P2sError, match=rf'sample_size={m} outside \[8, 16\]'):
            call(samples=np.zeros((3, 4, m), dtype=np.int32))
    with pytest.raises(_lib.P2sError, match='n_hyp=0'):
        call(samples=np.zeros((3, 0, 8), dtype=np.int32))
    for bad in ((1, 1), (0, 3), (-1, 2)):
        with pytest.raises(_lib.P2sError, match='pair 1 names the cameras'):
            call(pairs=np.array([(0, 1), bad, (1, 2)]))
    for bad in (0.0, -1e-6, np.nan, np.inf):
        with pytest.raises(_lib.P2sError, match='thr2 of pair 2 must be positive and finite'):
            call(thr2=np.array([1e-5, 1e-5, bad]))
    with pytest.raises(_lib.P2sError, match='rounds=-1'):
        call(rounds=-1)
    with pytest.raises(_lib.P2sError, match='usable has shape'):
        call(usable=us[:, :-1])
    with pytest.raises(_lib.P2sError, match='samples has shape'):
        call(samples=smp[:2])
    assert call(rounds=0)['refits'].max() == 0


def test_draw_samples_gives_distinct_usable_indices_and_is_reproducible():
    rng = np.random.default_rng(0)
    usable = rng.random((3, 5000)) < 0.7
    usable[2, 9:] = False                               # pairs with camera 2: a handful of points
    usable[2, :9] = usable[0, :9] = True
    usable[1, :9] = [1, 1, 1, 0, 1, 1, 0, 1, 1]         # (1, 2): seven, fewer than a sample
    pairs = cfk.all_pairs(3)
    for m in (8, 16):
        s = cfk.draw_samples(usable, pairs, 300, m, seed=11)
        assert s.shape == (3, 300, m) and s.dtype == np.int32 and np.array_equal(s, cfk.draw_samples(usable, pairs, 300, m, seed=11))
        assert not np.array_equal(s, cfk.draw_samples(usable, pairs, 300, m, seed=12))
        for p, (a, b) in enumerate(pairs):
            if (usable[a] & usable[b]).sum() < m:
                assert (s[p] == -1).all()
                continue
            assert (usable[a][s[p]] & usable[b][s[p]]).all()
            assert (np.diff(np.sort(s[p], axis=1), axis=1) > 0).all()
    assert (cfk.draw_samples(usable, pairs, 300, 8, seed=11)[1] >= 0).all() and len(np.unique(cfk.draw_samples(usable, pairs, 300, 8)[0])) > 1000


def test_normalised_coordinates_undo_the_lens_and_the_intrinsics():
    cams = rigs.make_rig('ring', 3, seed=1, distortion='mild5')
    cs = rn.walk_case('ring', 3, 4, 5, seed=1, noise_px=0.0, distortion='mild5')
    cs['xyl'][1, 2, 3, 2] = 0.2
    cs['xyl'][2, 0, 1, 0] = np.nan
    xn, usable = cfk.normalised(cams, cs['xyl'], 0.3)
    assert xn.shape == (3, 20, 2) and not usable[2, 1 * 5 + 3] and not usable[0, 2 * 5 + 1] and usable.sum() == 58 and np.isnan(xn[~usable]).all()
    Xc = np.einsum('cij,nj->cni', cs['R'], cs['Q']) + cs['t'][:, None, :]
    assert np.abs(xn - Xc[..., :2] / Xc[..., 2:])[usable].max() < 1e-5      # five fixed-point iterations of the undistortion


def test_command_line_arguments():
    a = cfk.parse_args(['-c', 'K.toml', '-p', 'pose'])
    assert (a.calib, a.pose, a.output, a.baseline, a.height, a.threshold, a.hypotheses, a.sample_size, a.score_points, a.seed, a.likelihood,
            a.huber, a.min_cams, a.keypoints, a.pose_model, a.frames) == ('K.toml', 'pose', None, None, None, 4.0, 4096, 8, 16384, 0, 0.3, 3.0, 2,
                                                                          None, 'HALPE_26', None)
    a = cfk.parse_args(['--calib', 'k.toml', '--pose', 'p', '-o', 'out.toml', '--baseline', 'cam01', 'cam03', '2.5', '--threshold', '3',
                        '--hypotheses', '1024', '--sample-size', '12', '--seed', '7', '--likelihood', '0.5', '--huber', '2',
                        '--keypoints', 'Nose, Neck', '--frames', '10', '20', '--score-points', '0'])
    assert (a.output, a.baseline, a.threshold, a.hypotheses, a.sample_size, a.seed, a.likelihood, a.huber, a.keypoints, a.frames, a.score_points) == \
        ('out.toml', ('cam01', 'cam03', 2.5), 3.0, 1024, 12, 7, 0.5, 2.0, ['Nose', 'Neck'], [10, 20], 0)
    assert cfk.parse_args(['-c', 'c', '-p', 'p', '--height', '1.8']).height == 1.8
    for bad in (['-p', 'pose'], ['-c', 'c.toml'], ['-c', 'c', '-p', 'p', '--baseline', 'a', 'b', '1', '--height', '1.7'],
                ['-c', 'c', '-p', 'p', '--baseline', 'a', 'a', '1'], ['-c', 'c', '-p', 'p', '--baseline', 'a', 'b', 'x'],
                ['-c', 'c', '-p', 'p', '--baseline', 'a', 'b', '0'], ['-c', 'c', '-p', 'p', '--height', '0'], ['-c', 'c', '-p', 'p', '--threshold', '0'],
                ['-c', 'c', '-p', 'p', '--sample-size', '7'], ['-c', 'c', '-p', 'p', '--sample-size', '17'], ['-c', 'c', '-p', 'p', '--hypotheses', '0'],
                ['-c', 'c', '-p', 'p', '--keypoints', ' , ']):
        with pytest.raises(SystemExit):
            cfk.parse_args(bad)
