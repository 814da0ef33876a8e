"""Engine.fit_planes and calib_align_floor on the MI355X against the NumPy mirror (tests/floor_numpy.py) and the truth of
synthetic walks.  The cases, the comparisons and the bounds are those of tests/test_floor_host.py, which runs them on the
library's host path; DESIGN.md 4.23 lists the figures of every case."""
import numpy as np
import pytest

import floor_numpy as fn
from pose2sim_amd import _lib, calib, trc
from pose2sim_amd import calib_align_floor as caf
from pose2sim_amd import calib_from_keypoints as cfk

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def eng():
    from pose2sim_amd.engine import Engine
    e = Engine(0)
    yield e
    e.close()


@pytest.mark.parametrize('B, N, H, seed', fn.HYP_CASES)
def test_every_hypothesis_and_result_against_the_mirror(eng, B, N, H, seed):
    """Every hypothesis, none excluded: counts equal, planes and costs within the bounds, weighted by the sine the mirror computes;
    then winner, refits kept, mask, plane, centroid and evals."""
    inp, ref = fn.hyp_case(B, N, H, seed)
    assert fn.winners_are_clear(ref) and fn.no_point_at_the_threshold(ref)
    got = eng.fit_planes(*inp, all_hypotheses=True)
    fn.compare_hypotheses(got, ref, inp, f'gpu B {B} N {N} H {H}')
    fn.compare_results(got, ref, f'gpu B {B} N {N} H {H}')
    assert eng.floor_kernel_ms() > 0


def test_structure(eng):
    fn.check_structure(eng.fit_planes)


def test_walks_against_the_mirror(eng):
    kept = []
    for F, seed, straight in fn.WALK_CASES:
        case, inp, ref = fn.walk_case(F, seed, straight)
        assert fn.winners_are_clear(ref) and fn.no_point_at_the_threshold(ref)
        got = eng.fit_planes(*inp, all_hypotheses=True)
        fn.compare_hypotheses(got, ref, inp, f'gpu walk {F}')
        fn.compare_results(got, ref, f'gpu walk {F}')
        angle = np.degrees(np.arccos(min(1.0, got['plane'][0, :3] @ case['up'])))
        mirror = np.degrees(np.arccos(min(1.0, ref['plane'][0, :3] @ case['up'])))
        print(f'walk of {F} frames: {angle:.4f} degrees from the true up, the mirror {mirror:.4f}')
        kept.append(int(got['refits'][0]))
    cases, inp, ref = fn.walks_batch()
    assert fn.winners_are_clear(ref) and fn.no_point_at_the_threshold(ref)
    got = eng.fit_planes(*inp, all_hypotheses=True)
    fn.compare_hypotheses(got, ref, inp, 'gpu walks, one call')
    fn.compare_results(got, ref, 'gpu walks, one call')
    assert max(kept) >= 1 and min(kept) < 3                                     # a refit is kept, and one is refused


def test_two_calls_return_the_same_bytes(eng):
    for inp in (fn.walks_batch()[1], fn.hyp_case(3, 700, 257, 5)[0], fn.hyp_case(1, 3, 1, 0)[0]):
        assert fn.same_bytes(eng.fit_planes(*inp, all_hypotheses=True), eng.fit_planes(*inp, all_hypotheses=True))


def test_refusals(eng):
    fn.check_refusals(eng.fit_planes, _lib.P2sError)


@pytest.mark.parametrize('N', fn.ZERO_NOISE_N)
def test_zero_noise_against_the_truth(eng, N):
    fn.check_zero_noise(eng.fit_planes, N)


def differences(got, want):
    """The indices of the arrays of `got` that are not `want`'s in dtype, shape, bits or NaN positions; [-1]: another number of them."""
    if len(got) != len(want):
        return [-1]
    return [i for i, (g, w) in enumerate(zip(got, want))
            if not (g.dtype == w.dtype and g.shape == w.shape and np.array_equal(g, w, equal_nan=g.dtype.kind == 'f'))]


def stages_with_the_floor(size):
    """Every stage of tests/engine_reuse_cases.py at this size, with fit_planes in the middle of them: one point past a wave
    at the small size, one past P2S_FLOOR_TILE at the large one."""
    import engine_reuse_cases as erc
    floor = fn.random_problem(2, 65 if size == erc.SMALL else 257, 65, seed=size[1])
    listed = erc.stages(size)
    return listed[:len(listed) // 2] + [('fit_planes', lambda e: erc.flat(e.fit_planes(*floor, all_hypotheses=True)))] + listed[len(listed) // 2:]


@pytest.fixture(scope='module')
def fresh():
    """{(size, name): result}: every call on an Engine of its own that has run nothing else."""
    import engine_reuse_cases as erc
    out = {}
    for size in (erc.SMALL, erc.LARGE):
        for name, call in stages_with_the_floor(size):
            e = erc.new_engine()
            out[size, name] = tuple(call(e))
            e.close()
    return out


@pytest.mark.parametrize('poison', [None, 0xFF, 0x3F])
def test_one_engine_through_every_stage_with_the_floor_among_them(fresh, poison):
    """The run of tests/test_engine_reuse_gpu.py with fit_planes as one more stage: one engine through every stage at the small
    shapes, at three times the frames (every slot grows), at the small shapes again in reverse order (every slot holds the stale
    tail of a larger call of another stage), as the calls left the buffers and with every buffer filled with 0xFF or 0x3F before
    each call.  Every result -- fit_planes' after the other stages, the other stages' after fit_planes -- must equal, bit for
    bit and NaN for NaN, that of a fresh Engine."""
    import engine_reuse_cases as erc
    from pose2sim_amd.engine import Engine
    eng = erc.new_engine()
    if poison is not None:
        eng.set_tuning(Engine.TUNE_POISON_STAGING, poison)
    differing, ran = [], 0
    for rnd, (size, order) in enumerate(((erc.SMALL, 1), (erc.LARGE, 1), (erc.SMALL, -1))):
        for name, call in stages_with_the_floor(size)[::order]:
            ran += name == 'fit_planes'
            for index in differences(tuple(call(eng)), fresh[size, name]):
                differing.append((poison, rnd, name, index))
                print('differs (poison, round, stage, array):', differing[-1])
    eng.close()
    assert differing == [] and ran == 3


def triangulated_world(eng, cams, xyl):
    return caf.triangulated(cams, xyl, engine=eng)


def check_world(X, walk, threshold=0.03):
    """X [F][K][3], the walk without noise seen through aligned cameras: the stance feet within the threshold of Z = 0, the hips
    above, the walk along +Y."""
    assert np.isfinite(X).all()
    assert np.abs(X[:, fn.FEET][walk['stance']][:, 2]).max() < threshold and X[:, :3, 2].min() > 0.8
    hips = X[:, 0, :2] - X[:, 0, :2].mean(axis=0)
    cov = hips.T @ hips
    angle = np.degrees(0.5 * np.arctan2(2 * cov[0, 1], cov[1, 1] - cov[0, 0]))
    print(f'the walk runs {X[-1, 0, 1] - X[0, 0, 1]:.2f} m along +Y, its principal axis {angle:.3f} degrees from Y')
    assert X[-1, 0, 1] - X[0, 0, 1] > 2.5 and abs(angle) < 2.0                  # fn.check_frame's 2 degrees


def test_align_calibration_end_to_end(eng, tmp_path):
    """A ring of 4 whose world was rotated and shifted off the floor: after align_calibration the true walk, triangulated
    through the written cameras, stands on Z = 0 and runs along +Y; the device's frame against the mirror pipeline's."""
    off, xyl, xyl_clean, walk = fn.rig_case()
    before = triangulated_world(eng, off, xyl_clean)
    assert np.abs(before[:, fn.FEET][walk['stance']][:, 2]).max() > 0.1         # the premise: this world is not on the floor
    path = str(tmp_path / 'Calib_off.toml')
    calib.write_calibration_toml(path, off)
    assert caf.align_calibration(off, xyl, keypoints=fn.KEYPOINTS, engine=eng)[0] is None          # dict and array: nothing written
    out, cams, rep = caf.align_calibration(off, xyl, str(tmp_path / 'Calib_floor.toml'), keypoints=fn.KEYPOINTS, engine=eng)
    back = calib.retrieve_calib_params(out)
    assert calib.load_toml(out)['metadata']['adjusted'] is True and len(back['K']) == 4
    check_world(triangulated_world(eng, back, xyl_clean), walk)
    # the mirror pipeline on the same triangulation
    X = triangulated_world(eng, off, xyl)
    pts, ok, ref, traj, offset = caf.plane_inputs(X, fn.KEYPOINTS)
    inp = (pts[None], ok[None], ref[None], caf.draw_triples(ok, 1024, 0)[None], 0.03)
    mirror = fn.fit_planes(*inp)
    assert fn.winners_are_clear(mirror) and fn.no_point_at_the_threshold(mirror) and rep['winner'] == mirror['winner'][0]
    Am, bm = caf.frame_of_plane(mirror['plane'][0], mirror['centroid'][0], traj)
    angle, mirror_angle = (np.degrees(np.arccos(min(1.0, float(r @ walk['up_off'])))) for r in (rep['A'][2], Am[2]))
    print(f'frame against the mirror pipeline: A {np.abs(rep["A"] - Am).max():.3e}, b {np.abs(rep["b"] - bm).max():.3e} m; '
          f'{angle:.4f} degrees from the true up, the mirror {mirror_angle:.4f}')
    assert np.abs(rep['A'] - Am).max() <= fn.RESULT_FRAME_BOUND and np.abs(rep['b'] - bm).max() <= fn.RESULT_FRAME_BOUND


def test_calibrate_from_keypoints_with_the_floor(eng, tmp_path):
    """calibrate_from_keypoints(floor=True) is floor=False followed by align_calibration, and its world is on the floor."""
    off, xyl, xyl_clean, walk = fn.rig_case()
    names = off['names']
    c = cfk.centres(off)
    kw = dict(baseline=(names[0], names[1], float(np.linalg.norm(c[0] - c[1]))), keypoints=fn.KEYPOINTS, hypotheses=512, engine=eng)
    out, floored, rep = cfk.calibrate_from_keypoints(off, xyl, str(tmp_path / 'Calib_keypoints.toml'), floor=True, **kw)
    _, plain, _ = cfk.calibrate_from_keypoints(off, xyl, floor=False, **kw)
    _, aligned, rep2 = caf.align_calibration(plain, xyl, keypoints=fn.KEYPOINTS, engine=eng)
    assert np.array_equal(plain['R_mat'][0], np.eye(3)) and 'floor' in rep                            # camera 0's world without the floor
    for c in range(4):                                                                               # the same calls on the same engine
        assert np.array_equal(floored['R_mat'][c], aligned['R_mat'][c]) and np.array_equal(floored['T'][c], aligned['T'][c])
    assert rep['floor']['winner'] == rep2['winner']
    back = calib.retrieve_calib_params(out)
    check_world(triangulated_world(eng, back, xyl_clean), walk)


def test_align_trc_against_the_mirror_pipeline(eng, tmp_path):
    F, seed, straight = fn.WALK_CASES[2]
    case, inp, ref = fn.walk_case(F, seed, straight)
    path = trc.write_trc(str(tmp_path), 'walk', np.arange(F), case['X'].reshape(F, -1), case['names'], 60)
    out, A, b, rep = caf.align_trc(path, hypotheses=256, seed=seed, engine=eng)
    Am, bm = caf.frame_of_plane(ref['plane'][0], ref['centroid'][0], caf.plane_inputs(case['X'], case['names'])[3])
    assert rep['winner'] == ref['winner'][0] and rep['refits'] == ref['refits'][0]
    print(f'align_trc against the mirror pipeline: A {np.abs(A - Am).max():.3e}, b {np.abs(b - bm).max():.3e} m')
    assert np.abs(A - Am).max() <= fn.RESULT_FRAME_BOUND and np.abs(b - bm).max() <= fn.RESULT_FRAME_BOUND
    fn.check_frame(case, A, b)
    coords = trc.load_trc(out)[2]
    assert np.abs(caf.zup_markers(coords) - (case['X'] @ A.T + b)).max() < 1e-12
    batch = caf.align_trc_batch([path, path], [str(tmp_path / 'a.trc'), str(tmp_path / 'b.trc')], hypotheses=256, seed=seed, engine=eng)
    for _, A2, b2, rep2 in batch:
        assert rep2['winner'] == rep['winner'] and np.abs(A2 - A).max() <= fn.RESULT_FRAME_BOUND and np.abs(b2 - b).max() <= fn.RESULT_FRAME_BOUND
