"""What of the floor alignment needs no GPU: the library's host path (ctx == NULL runs the kernels' per-hypothesis and per-point
functions) against the NumPy mirror on the cases and bounds of tests/test_floor_gpu.py, the mirror against the truth,
floor_frame and align_trc through the host path, the samples and the command line."""
import ctypes as C
import logging
import os
import re

import numpy as np
import pytest

import floor_numpy as fn
from pose2sim_amd import _lib, engine, trc
from pose2sim_amd import calib_align_floor as caf

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def fit(*args, **kw):
    return engine.fit_planes_host(*args, **kw)


def test_entry_points_are_declared_exported_and_bound_as_optional():
    """include/p2s_floor.h against the library and against _lib's table of it, as tests/test_lib_abi.py holds include/p2s.h."""
    txt = open(os.path.join(ROOT, 'include', 'p2s_floor.h')).read()
    defs = {m.group(1): int(m.group(2)) for m in re.finditer(r'#define\s+(P2S_FLOOR_[A-Z_]+)\s+(\d+)', txt)}
    assert defs == {'P2S_FLOOR_TILE': _lib.P2S_FLOOR_TILE, 'P2S_FLOOR_MAX_CHUNKS': _lib.P2S_FLOOR_MAX_CHUNKS, 'P2S_FLOOR_MAX_PARTS': _lib.P2S_FLOOR_MAX_PARTS}
    syms = set(re.findall(r'\b(p2s_[a-z_0-9]+)\s*\(', re.sub(r'/\*.*?\*/', '', txt, flags=re.S)))
    assert syms == {'p2s_fit_planes_host', 'p2s_floor_kernel_ms'} == set(_lib.FLOOR_SIGNATURES) and syms <= _lib.OPTIONAL
    assert not syms & set(_lib.SIGNATURES)
    lib = C.CDLL(_lib.LIB_PATH)
    assert all(hasattr(lib, name) for name in syms)
    bound = _lib.load()
    assert bound.p2s_fit_planes_host.argtypes == _lib.FLOOR_SIGNATURES['p2s_fit_planes_host'][1]
    assert 'p2s_floor.hip' in open(os.path.join(ROOT, '__graft_entry__.py')).read()


@pytest.mark.parametrize('B, N, H, seed', fn.HYP_CASES)
def test_every_hypothesis_and_result_against_the_mirror(B, N, H, seed):
    inp, ref = fn.hyp_case(B, N, H, seed)
    assert fn.winners_are_clear(ref) and fn.no_point_at_the_threshold(ref)
    got = fit(*inp, all_hypotheses=True)
    fn.compare_hypotheses(got, ref, inp, f'host B {B} N {N} H {H}')
    fn.compare_results(got, ref, f'host B {B} N {N} H {H}')
    assert B == 1 or len(set(fn.counts(inp[0], inp[1]).sum(axis=1))) == B       # different counts of usable points


def test_structure():
    fn.check_structure(fit)


def test_walks_against_the_mirror_and_the_truth():
    """Winner, refits kept, mask, plane, centroid and evals of the walks, alone and as the problems of one call; the mirror's
    own angle to the true up beside them."""
    kept = []
    for F, seed, straight in fn.WALK_CASES:
        case, inp, ref = fn.walk_case(F, seed, straight)
        assert fn.winners_are_clear(ref) and fn.no_point_at_the_threshold(ref)
        got = fit(*inp, all_hypotheses=True)
        fn.compare_hypotheses(got, ref, inp, f'host walk {F}')
        fn.compare_results(got, ref, f'host walk {F}')
        angle = np.degrees(np.arccos(min(1.0, ref['plane'][0, :3] @ case['up'])))
        feet = ((case['world'] - case['b']) @ case['A'])[:, fn.FEET][case['stance']]             # the true stance feet, given frame
        off = np.abs(feet @ ref['plane'][0, :3] - ref['plane'][0, 3]).max()
        print(f'walk of {F} frames: the mirror is {angle:.3f} degrees from the true up, the true stance feet at most {off * 1000:.2f} mm from its plane')
        # the method on 1 cm noise, not a bound of arithmetic: 1 cm over a band of 0.11 m of 250 inliers and more is 0.3 degrees
        assert angle < 1.0 and off < 0.03
        kept.append(int(ref['refits'][0]))
    cases, inp, ref = fn.walks_batch()
    assert fn.winners_are_clear(ref) and fn.no_point_at_the_threshold(ref)
    fn.compare_results(fit(*inp), ref, 'host walks, one call')
    assert max(kept) >= 1 and min(kept) < 3                                     # a refit is kept, and one is refused


def test_two_calls_return_the_same_bytes():
    _, inp, _ = fn.walks_batch()
    assert fn.same_bytes(fit(*inp, all_hypotheses=True), fit(*inp, all_hypotheses=True))


def test_refusals():
    fn.check_refusals(fit, _lib.P2sError)


@pytest.mark.parametrize('N', fn.ZERO_NOISE_N)
def test_zero_noise_against_the_truth(N):
    fn.check_zero_noise(fit, N)


def test_draw_triples():
    usable = np.arange(50) % 3 != 0
    s = caf.draw_triples(usable, 300, seed=5)
    assert s.shape == (300, 3) and s.dtype == np.int32 and usable[s].all() and (np.sort(s, axis=1)[:, 1:] != np.sort(s, axis=1)[:, :-1]).all()
    assert np.array_equal(s, caf.draw_triples(usable, 300, seed=5)) and not np.array_equal(s, caf.draw_triples(usable, 300, seed=6))
    few = caf.draw_triples(np.arange(10) < 5, 40, seed=0)
    assert (few < 5).all() and (np.sort(few, axis=1)[:, 1:] != np.sort(few, axis=1)[:, :-1]).all()
    assert (caf.draw_triples(np.arange(10) < 2, 4) == -1).all()


def test_floor_frame_on_walks(caplog):
    for F, seed, straight in fn.WALK_CASES[1:]:
        case, inp, ref = fn.walk_case(F, seed, straight)
        with caplog.at_level(logging.WARNING):
            caplog.clear()
            A, b, rep = caf.floor_frame(case['X'], case['names'], hypotheses=256, seed=seed, host=True)
        assert rep['winner'] == ref['winner'][0] and rep['inliers'] == ref['inliers'][0]           # the same samples: fn.inputs draws them so
        fn.check_frame(case, A, b)
        narrow = rep['band'] < 10 * 0.03
        assert narrow == straight and ('band' in caplog.text) == narrow, rep['band']              # the straight walk's roll is warned of


def test_floor_frame_with_ankles_and_without_feet():
    case, _, _ = fn.walk_case(*fn.WALK_CASES[2])
    names = [{'LHeel': 'LAnkle', 'RHeel': 'RAnkle'}.get(n, n) for n in case['names']]
    keep = [i for i, n in enumerate(names) if 'Toe' not in n]
    X = case['X'][:, keep].copy()
    for n in ('LAnkle', 'RAnkle'):
        X[:, [names[i] for i in keep].index(n)] += 0.08 * case['up']              # the ankles, 8 cm over the floor
    A, b, rep = caf.floor_frame(X, [names[i] for i in keep], hypotheses=256, seed=2, ankle_height=0.08, host=True)
    assert rep['offset'] == 0.08
    fn.check_frame(case, A, b)
    with pytest.raises(ValueError, match='no floor without feet'):
        caf.floor_frame(X[:, :3], ['Hip', 'RHip', 'LHip'], host=True)
    with pytest.raises(ValueError, match='which side of the floor is up'):
        caf.floor_frame(X[:, -2:], ['LAnkle', 'RAnkle'], host=True)


def test_moved_cameras_see_the_moved_world():
    off, _, _, walk = fn.rig_case()
    rng = np.random.default_rng(0)
    A, b = fn.random_rotation(rng), rng.normal(size=3)
    moved = caf.moved_cameras(off, A, b)
    x = rng.normal(size=(5, 3))
    for c in range(4):
        assert np.abs((x @ off['R_mat'][c].T + off['T'][c]) - ((x @ A.T + b) @ moved['R_mat'][c].T + moved['T'][c])).max() < 1e-12


def test_align_trc_and_batch(tmp_path):
    """align_trc on written files against the mirror pipeline; a session's files as the problems of one call."""
    paths, walks = [], []
    for F, seed, straight in fn.WALK_CASES[1:]:
        case, inp, ref = fn.walk_case(F, seed, straight)
        frames = np.arange(10, 10 + F)
        paths.append(trc.write_trc(str(tmp_path), f'walk{F}', frames, case['X'].reshape(F, -1), case['names'], 60))
        walks.append((case, inp, ref, seed))
    for path, (case, inp, ref, seed) in zip(paths, walks):
        out, A, b, rep = caf.align_trc(path, hypotheses=256, seed=seed, host=True)
        assert out == os.path.splitext(path)[0] + '_floor.trc' and rep['winner'] == ref['winner'][0]
        Am, bm = caf.frame_of_plane(ref['plane'][0], ref['centroid'][0], caf.plane_inputs(case['X'], case['names'])[3])
        print(f'align_trc against the mirror pipeline: A {np.abs(A - Am).max():.3e}, b {np.abs(b - bm).max():.3e} m')
        assert np.abs(A - Am).max() <= fn.RESULT_FRAME_BOUND and np.abs(b - bm).max() <= fn.RESULT_FRAME_BOUND
        frames, time_col, coords, markers, header = trc.load_trc(out)
        f0, t0, c0, m0, h0 = trc.load_trc(path)
        assert markers == m0 and np.array_equal(frames, f0) and np.array_equal(time_col, t0) and header[1:] == h0[1:]
        assert [ln.split('\t')[:2] for ln in open(out).read().split('\n')[5:]] == [ln.split('\t')[:2] for ln in open(path).read().split('\n')[5:]]
        assert header[0].split('\t')[-1].strip() == os.path.basename(out)
        new = caf.zup_markers(coords)
        assert np.abs(new - (case['X'] @ A.T + b)).max() < 1e-12
        fn.check_frame(case, A, b)
        # through the reference's zup2yup the file runs along +X, has +Y up and +Z to the right
        stored = coords.reshape(len(coords), -1, 3)
        assert np.median(stored[-5:, 0, 0]) - np.median(stored[:5, 0, 0]) > 2.5 and np.median(stored[:, 0, 1]) > 0.8   # medians: the file holds the noisy walk
        assert (stored[:, case['names'].index('RHip'), 2] - stored[:, case['names'].index('LHip'), 2]).mean() > 0.1   # 0.2 m apart, across a heading that turns by up to 56 degrees
    outs = [str(tmp_path / f'b{i}.trc') for i in range(2)]
    batch = caf.align_trc_batch(paths, outs, hypotheses=256, seed=1, host=True)
    for (out, A, b, rep), path in zip(batch, paths):
        _, A1, b1, rep1 = caf.align_trc(path, str(tmp_path / 'single.trc'), hypotheses=256, seed=1, host=True)
        assert rep['winner'] == rep1['winner'] and np.abs(A - A1).max() <= fn.RESULT_FRAME_BOUND and np.abs(b - b1).max() <= fn.RESULT_FRAME_BOUND
        assert os.path.exists(out)


def test_command_line():
    args = caf.parse_args(['-c', 'Calib.toml', '-p', 'pose'])
    assert (args.threshold, args.hypotheses, args.seed, args.output, args.trc) == (0.03, 1024, 0, None, None)
    assert caf.parse_args(['--trc', 'a.trc', 'b.trc']).trc == ['a.trc', 'b.trc']
    for bad in (['-c', 'Calib.toml'], ['-p', 'pose'], ['-c', 'C.toml', '-p', 'pose', '--trc', 'a.trc'], ['--trc', 'a.trc', '--threshold', '0'],
                ['--trc', 'a.trc', '--hypotheses', '0']):
        with pytest.raises(SystemExit):
            caf.parse_args(bad)
    from pose2sim_amd import calib_from_keypoints as cfk
    args = cfk.parse_args(['-c', 'a.toml', '-p', 'pose', '--floor', '--height', '1.7', '--floor-threshold', '0.02', '--floor-hypotheses', '64'])
    assert args.floor and (args.floor_threshold, args.floor_hypotheses, args.ankle_height) == (0.02, 64, 0.08)
    assert not cfk.parse_args(['-c', 'a.toml', '-p', 'pose']).floor
    for bad in (['--floor'], ['--floor', '--height', '1.7', '--floor-threshold', '0']):        # an arbitrary scale has no metres
        with pytest.raises(SystemExit):
            cfk.parse_args(['-c', 'a.toml', '-p', 'pose'] + bad)
    with pytest.raises(ValueError, match='needs a baseline or a height'):
        cfk.calibrate_from_keypoints({'K': []}, np.zeros((1, 2, 1, 3)), floor=True)


def test_a_trc_that_is_not_in_metres_is_refused(tmp_path):
    case, _, _ = fn.walk_case(*fn.WALK_CASES[0])
    F = len(case['X'])
    path = trc.write_trc(str(tmp_path), 'walk', np.arange(F), case['X'].reshape(F, -1), case['names'], 60)
    assert trc.units(trc.load_trc(path)[4]) == 'm'
    lines = open(path).read().split('\n')
    lines[2] = '\t'.join('mm' if v == 'm' else v for v in lines[2].split('\t'))
    open(path, 'w').write('\n'.join(lines))
    with pytest.raises(ValueError, match='is in mm'):
        caf.align_trc(path, host=True)
    assert not os.path.exists(os.path.splitext(path)[0] + '_floor.trc')
