"""Engine.relative_poses and calib_from_keypoints on the MI355X against the NumPy mirror (tests/relpose_numpy.py), the truth
and Engine.refine_extrinsics started from the true cameras.

The bounds, what they are 100 x of, and why a hypothesis' difference is weighted by its conditioning are in
tests/relpose_numpy.py; DESIGN.md 4.22 lists the figures of every case."""
import os

import numpy as np
import pytest

import refine_scipy as rs
import relpose_numpy as rn
from pose2sim_amd import calib, calib_refine, poseio
from pose2sim_amd import calib_from_keypoints as cfk
from pose2sim_amd.engine import Engine

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def eng():
    e = Engine(0)
    yield e
    e.close()


def sliced(Cn, N, H, m, seed, family='ring'):
    """The first N points of a walk: (xn, usable, pairs, samples, thr2).  N = 8: every likelihood is 1, so that the 8 count."""
    cs = rn.walk_case(family, Cn, -(-N // 13), 13, seed=seed, lik=None if N == 8 else (0.1, 1.0))
    xn, us, pairs, _, thr2 = rn.inputs(cs, H=1)
    xn, us = np.ascontiguousarray(xn[:, :N]), np.ascontiguousarray(us[:, :N])
    return xn, us, pairs, cfk.draw_samples(us, pairs, H, m, seed), thr2


def compare_hypotheses(got, ref, xn, us, pairs, thr2, tag):
    """Every hypothesis of a case against the mirror; -> the worst figures."""
    cond, fin = ref['hyp_cond'], np.isfinite(ref['hyp_cost'])
    compared = fin & (cond >= rn.COND_FLOOR)
    share = 1.0 - compared[fin].mean() if fin.any() else 0.0
    assert share <= rn.COND_SHARE, f'{tag}: {share:.3%} of the hypotheses are below the conditioning floor'
    assert rn.no_point_at_the_threshold(ref), f'{tag}: a point of the mirror lies at the threshold'
    assert np.array_equal(np.isfinite(got['hyp_cost']), fin) and np.array_equal(np.isnan(got['hyp_E']), np.isnan(ref['hyp_E']))
    assert np.array_equal(got['hyp_inliers'], ref['hyp_inliers']), tag
    dE = np.abs(rn.match_sign(got['hyp_E'], ref['hyp_E']) - ref['hyp_E']).max(axis=(-2, -1))
    dc = np.abs(got['hyp_cost'] - ref['hyp_cost']) / np.where(fin, ref['hyp_cost'], 1.0)
    ok = rn.counts(xn, us)
    ds = 0.0                                              # the scoring kernel alone: the mirror scores the device's E
    for p, (a, b) in enumerate(pairs):
        both = ok[a] & ok[b]
        for h in np.flatnonzero(fin[p]):
            c, i, _ = rn.score(got['hyp_E'][p, h], xn[a][both], xn[b][both], thr2[p])
            assert i == got['hyp_inliers'][p, h]
            ds = max(ds, abs(c - got['hyp_cost'][p, h]) / c)
    worst = (float((dE * cond)[compared].max(initial=0.0)), float((dc * cond)[compared].max(initial=0.0)), ds)
    print(f'{tag}: {int(compared.sum())} of {int(fin.sum())} hypotheses compared, lambda_2 / lambda_max from {cond[compared].min(initial=1):.1e}; '
          f'E {dE[compared].max(initial=0.0):.2e}, x lambda_2 / lambda_max {worst[0]:.2e}; cost {dc[compared].max(initial=0.0):.2e} relative, '
          f'x lambda_2 / lambda_max {worst[1]:.2e}; cost of the device\'s E {worst[2]:.2e} relative')
    assert worst[0] <= rn.HYP_E_SCALED_BOUND and worst[1] <= rn.HYP_COST_SCALED_BOUND and worst[2] <= rn.COST_REL_BOUND, tag
    return worst


def compare_results(got, ref, tag, clear=None):
    """The pairs' results against the mirror's.  A pair that is not `clear` (the mirror's two best costs lie within their bounds
    of each other) only has to take one of those two.  A result that is a hypothesis as it stands (no refit kept) of a
    lambda_2 / lambda_max below RESULT_COND_FLOOR is held to the hypotheses' weighted bounds, every other one to the caps."""
    P = len(ref['winner'])
    clear = np.ones(P, dtype=bool) if clear is None else clear
    assert np.array_equal(got['winner'] >= 0, ref['winner'] >= 0)
    cond = np.array([ref['hyp_cond'][p, ref['winner'][p]] if ref['winner'][p] >= 0 else 1.0 for p in range(P)])[clear]
    got, ref = ({k: v[clear] for k, v in r.items() if k in ('winner', 'refits', 'inliers', 'front', 'mask', 'E', 'R', 't', 'cost')} for r in (got, ref))
    for k in ('winner', 'refits', 'inliers', 'front', 'mask'):
        assert np.array_equal(got[k], ref[k]), (tag, k)
    v = ref['winner'] >= 0
    assert np.isnan(got['E'][~v]).all() and np.isnan(got['R'][~v]).all() and np.isnan(got['t'][~v]).all() and np.isnan(got['cost'][~v]).all()
    if not v.any():
        return
    dE = np.abs(rn.match_sign(got['E'][v], ref['E'][v]) - ref['E'][v]).max(axis=(-2, -1))
    dR, dt = np.abs(got['R'][v] - ref['R'][v]).max(axis=(-2, -1)), np.abs(got['t'][v] - ref['t'][v]).max(axis=-1)
    dcost = np.abs(got['cost'][v] - ref['cost'][v]) / ref['cost'][v]
    weighted = (ref['refits'][v] == 0) & (cond[v] < rn.RESULT_COND_FLOOR)
    w, s = cond[v][weighted], ~weighted
    print(f'{tag}: {int(s.sum())} results E {dE[s].max(initial=0):.2e}, R {dR[s].max(initial=0):.2e}, t {dt[s].max(initial=0):.2e}, cost '
          f'{dcost[s].max(initial=0):.2e} relative; {int(weighted.sum())} unrefitted hypotheses of a low lambda_2 / lambda_max, x that: E '
          f'{(dE[weighted] * w).max(initial=0):.2e}, R {(dR[weighted] * w).max(initial=0):.2e}, t {(dt[weighted] * w).max(initial=0):.2e}, cost '
          f'{(dcost[weighted] * w).max(initial=0):.2e}; refits {got["refits"][v].tolist()[:8]}')
    assert max(dE[s].max(initial=0), dR[s].max(initial=0), dt[s].max(initial=0)) <= rn.WIN_E_BOUND and dcost[s].max(initial=0) <= rn.RESULT_COST_REL_BOUND, tag
    assert (dE[weighted] * w).max(initial=0) <= rn.HYP_E_SCALED_BOUND and (dcost[weighted] * w).max(initial=0) <= rn.HYP_COST_SCALED_BOUND, tag
    assert max((dR[weighted] * w).max(initial=0), (dt[weighted] * w).max(initial=0)) <= rn.RT_SCALED_BOUND, tag
    assert np.abs(np.linalg.norm(got['t'][v], axis=1) - 1).max() < 1e-14 and np.abs(np.linalg.det(got['R'][v]) - 1).max() < 1e-13


# N around the 64 lanes of a wave and the 256 points of a pass; 257 and 700 are past a single chunk (2 cameras: the points
# are cut into chunks of a pass each); H around a wave and the 256 hypotheses of a workgroup; every sample size's ends;
# 32 cameras at 1025 points: the per-point passes take 3 parts over 5 tiles (2, 2 and 1 of them), and the refits leave
# pairs out of a pass and keep others in (0, 1, 2 and 3 refits kept)
SHAPES = [(2, 8, 64, 8, 1), (2, 63, 64, 8, 2), (2, 64, 64, 8, 3), (2, 65, 64, 8, 4), (2, 257, 64, 8, 5), (2, 700, 64, 8, 6),
          (2, 65, 1, 8, 7), (2, 65, 63, 8, 8), (2, 65, 65, 8, 9), (2, 65, 257, 8, 10), (2, 130, 64, 12, 11), (2, 130, 64, 16, 12),
          (3, 65, 64, 8, 13), (32, 40, 8, 8, 14), (32, 1025, 8, 8, 15)]


@pytest.mark.parametrize('Cn, N, H, m, seed', SHAPES)
def test_every_hypothesis_against_the_mirror(eng, Cn, N, H, m, seed):
    xn, us, pairs, smp, thr2 = sliced(Cn, N, H, m, seed)
    ref = rn.relative_poses(xn, us, pairs, smp, thr2)
    got = eng.relative_poses(xn, us, pairs, smp, thr2, all_hypotheses=True)
    tag = f'C {Cn} (P {len(pairs)}), N {N}, H {H}, m {m}'
    compare_hypotheses(got, ref, xn, us, pairs, thr2, tag)
    if N > 8:                                             # 8 points: every sample is the same 8, and every cost a tie
        clear, best = rn.clear_winners(ref)
        assert clear.all() if Cn < 32 else clear.mean() >= 0.95, 'the two best costs are too close'
        assert all(got['winner'][p] in best[p] for p in np.flatnonzero(~clear))
        compare_results(got, ref, tag, clear)
    assert eng.relpose_kernel_ms() > 0


def test_unusable_points_nan_short_pairs_and_refused_samples(eng):
    xn, us, pairs, _, thr2 = sliced(3, 300, 1, 8, 21)
    us[2, 5:] = False                                   # camera 2: five points, fewer than a sample
    us[0, 7::9] = False
    xn[1, 9::11] = np.nan                               # usable, and not a number
    smp = cfk.draw_samples(us & np.isfinite(xn).all(axis=-1), pairs, 70, 8, seed=1)
    smp[0, 3, 5] = smp[0, 3, 1]                         # a repeated index
    smp[0, 4, 0] = 300                                  # past the end
    smp[0, 5, 2] = -1
    smp[0, 6, 7] = 7                                    # not usable in camera 0
    smp[0, 69, 7] = 9                                   # NaN in camera 1
    ref = rn.relative_poses(xn, us, pairs, smp, thr2)
    got = eng.relative_poses(xn, us, pairs, smp, thr2, all_hypotheses=True)
    compare_hypotheses(got, ref, xn, us, pairs, thr2, 'refusals')
    compare_results(got, ref, 'refusals')
    assert (got['winner'][1:] == -1).all() and not got['mask'][1:].any() and got['winner'][0] >= 0
    assert np.isinf(got['hyp_cost'][0, [3, 4, 5, 6, 69]]).all() and np.isnan(got['hyp_E'][0, [3, 4, 5, 6, 69]]).all()
    assert np.isinf(got['hyp_cost'][1:]).all() and not got['mask'][0, 7::9].any() and not got['mask'][0, 9::11].any()


@pytest.fixture(scope='module')
def ring4():
    cs = rn.walk_case('ring', 4, 20, 13, seed=4)
    inp = rn.inputs(cs, H=512)
    return cs, inp, rn.relative_poses(*inp)


def test_winner_refits_and_decomposition(eng, ring4):
    cs, (xn, us, pairs, smp, thr2), ref = ring4
    assert rn.winners_are_clear(ref) and ref['near_final'].min() > rn.COST_REL_BOUND
    assert 0 < ref['refits'].sum() < 3 * len(pairs)       # refits kept and refits refused
    compare_results(eng.relative_poses(xn, us, pairs, smp, thr2), ref, 'ring 4, H 512')
    # scoring on a stride of the points, refits on all
    ref = rn.relative_poses(xn, us, pairs, smp, thr2, score_points=100)
    got = eng.relative_poses(xn, us, pairs, smp, thr2, all_hypotheses=True, score_points=100)
    assert np.array_equal(got['hyp_inliers'], ref['hyp_inliers']) and ref['hyp_inliers'].max() <= 100 < ref['inliers'].min()
    compare_results(got, ref, 'ring 4, H 512, 100 points scored')


def test_two_calls_return_the_same_bytes(eng, ring4):
    _, (xn, us, pairs, smp, thr2), _ = ring4
    a = eng.relative_poses(xn, us, pairs, smp, thr2, all_hypotheses=True)
    b = eng.relative_poses(xn, us, pairs, smp, thr2, all_hypotheses=True)
    assert sorted(a) == sorted(b) and len(a) == 12
    for k in a:
        assert a[k].tobytes() == b[k].tobytes(), k
    xn2, us2, pairs2, smp2, thr22 = sliced(2, 700, 257, 8, 6)                       # chunks of points, two workgroups of hypotheses
    a, b = (eng.relative_poses(xn2, us2, pairs2, smp2, thr22, all_hypotheses=True) for _ in range(2))
    for k in a:
        assert a[k].tobytes() == b[k].tobytes(), k
    xn3, us3, pairs3, smp3, thr23 = sliced(32, 1025, 8, 8, 15)                      # more tiles than parts, an uneven last part
    a, b = (eng.relative_poses(xn3, us3, pairs3, smp3, thr23, all_hypotheses=True) for _ in range(2))
    for k in a:
        assert a[k].tobytes() == b[k].tobytes(), k


@pytest.mark.parametrize('N', [104, 255, 256, 257])
def test_zero_noise_recovers_the_cameras(eng, N):
    cs = rn.walk_case('ring', 3, 8 if N == 104 else 20, 13, seed=3, noise_px=0.0)
    xn, us, pairs, _, thr2 = rn.inputs(cs, H=1)
    xn, us = np.ascontiguousarray(xn[:, :N]), np.ascontiguousarray(us[:, :N])
    got = eng.relative_poses(xn, us, pairs, cfk.draw_samples(us, pairs, 64, 8, 0), thr2)
    assert (got['inliers'] == N).all() and (got['front'] == N).all() and got['mask'].all()
    Ra, ca, ct = rn.align(*rn.cameras(3, xn, pairs, got), cs['R'], cs['t'])
    dr, dc = max(np.linalg.norm(Ra[c] - cs['R'][c]) for c in range(3)), np.abs(ca - ct).max()
    print(f'zero noise, N {N}: rotations {dr:.2e}, centres {dc:.2e} m from the truth')
    assert dr <= rn.ZERO_NOISE_R and dc <= rn.ZERO_NOISE_C


E2E = [('ring', 2, 0.5, 0.05), ('ring', 3, 0.5, 0.05), ('ring', 4, 0.5, 0.05), ('overhead', 4, 0.5, 0.05), ('one_side', 4, 0.5, 0.05),
       ('stadium', 4, 0.5, 0.05), ('ring', 8, 1.5, 0.15)]


@pytest.mark.parametrize('family, Cn, noise, p_out', E2E)
def test_end_to_end_reaches_the_minimum_of_the_true_start(eng, family, Cn, noise, p_out):
    cs = rn.walk_case(family, Cn, 20, 13, seed=Cn, noise_px=noise, p_outlier=p_out)
    _, cams, rep = cfk.calibrate_from_keypoints(cs['cams'], cs['xyl'], hypotheses=512, engine=eng)
    truth, rep_t = calib_refine.refine_extrinsics(cs['cams'], cs['xyl'], engine=eng)
    Rs, cstart, ct = rn.align(rep['start']['R_mat'], rep['start']['T'], cs['R'], cs['t'])
    rel = (rep['cost_after'] - rep_t['cost_after']) / rep_t['cost_after']
    _, c, cref = rn.align(cams['R_mat'], cams['T'], truth['R_mat'], truth['T'])
    dc = np.abs(c - cref).max()
    print(f'{family} {Cn}: start {np.abs(cstart - ct).max():.3e} m and {max(np.linalg.norm(Rs[i] - cs["R"][i]) for i in range(Cn)):.3e} from the '
          f'truth; cost {rep["cost_after"]:.9f}, from the true cameras {rep_t["cost_after"]:.9f}, relative difference {rel:.2e}; centres {dc:.2e} m')
    assert rep['kept_points'] == rep_t['kept_points']
    assert abs(rel) <= rs.COST_REL_BOUND and dc <= rs.CENTRE_BOUND
    assert np.array_equal(cams['R_mat'][0], np.eye(3)) and not np.asarray(cams['T'][0]).any()


def test_from_openpose_folders_with_lenses_and_a_baseline(eng, tmp_path):
    cs = rn.walk_case('ring', 3, 20, 26, seed=9, distortion='mild5')
    names = cs['cams']['names']
    for c, name in enumerate(names):
        os.makedirs(tmp_path / 'pose' / f'{name}_json')
        for f in range(20):
            poseio.write_openpose_json(str(tmp_path / 'pose' / f'{name}_json' / f'walk_{f:04d}.json'), [cs['xyl'][f, c]])
    wrong = {k: list(v) for k, v in cs['cams'].items()}
    wrong['R_mat'], wrong['R'], wrong['T'] = [np.eye(3)] * 3, [np.zeros(3)] * 3, [np.zeros(3)] * 3      # the extrinsics are not read
    toml = str(tmp_path / 'intrinsics.toml')
    calib.write_calibration_toml(toml, wrong)
    out, cams, rep = cfk.calibrate_from_keypoints(toml, str(tmp_path / 'pose'), baseline=(names[0], names[2], 2.5), hypotheses=512, engine=eng)
    assert out == str(tmp_path / 'intrinsics_keypoints.toml') and calib.load_toml(out)['metadata']['adjusted'] is True
    back = calib.retrieve_calib_params(out)
    assert back['names'] == names and all(np.array_equal(a, b) for a, b in zip(back['K'], cs['cams']['K']))
    c = cfk.centres(back)
    assert abs(np.linalg.norm(c[0] - c[2]) - 2.5) < 1e-12
    Ra, ca, ct = rn.align(back['R_mat'], back['T'], cs['R'], cs['t'])
    print(f'from folders: centres {np.abs(ca - ct).max():.3e} m, rotations {max(np.linalg.norm(Ra[i] - cs["R"][i]) for i in range(3)):.3e} from '
          f'the truth, RMS {rep["rms_after"]}')
