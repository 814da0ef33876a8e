"""GPU parity of the association kernel (rays + affinity + matchSVT) through the C-ABI.

Against the frames recorded from the reference (tests/golden/assoc_frames.npz): the thresholded
matchSVT matrix within 1e-7 and, from it, IDENTICAL proposals (person_index_per_cam on the host).
"""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden'))
from pose2sim_amd import synth  # noqa: E402
from pose2sim_amd._lib import P2sError  # noqa: E402

import assoc_hard as ah
from test_oracle_golden import _assoc_groups, assoc_frames_of

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module', params=['auto', 'general'])
def engine(request):
    """'auto': frames of up to 32 detections take the symmetric one-wave kernel; 'general': the kernel that assumes
    no symmetry and accumulates V at every size -- two implementations of matchSVT against the same references."""
    import __graft_entry__ as entry
    entry.build_hip()
    from pose2sim_amd.engine import Engine
    eng = Engine(0)
    if request.param == 'general':
        eng.set_tuning(Engine.TUNE_ASSOC_FORM, Engine.ASSOC_FORM_GENERAL)
    yield eng
    eng.close()


def _pack(frames, C, Kj):
    n_persons = np.array([[len(p) for p in per_cam] for per_cam in frames], dtype=np.int32).reshape(len(frames), C)
    rows = [np.asarray(p, dtype=np.float64).reshape(Kj, 3) for per_cam in frames for people in per_cam for p in people]
    kpts = np.array(rows).reshape(-1, Kj, 3) if rows else np.zeros((0, Kj, 3))
    return n_persons, kpts


def test_golden_frames(engine, golden_dir):
    from pose2sim_amd import personAssociation as pa
    worst = 0.0
    for i, g in _assoc_groups(golden_dir):
        cal, frames = assoc_frames_of(g)
        C, Kj = int(g['C']), int(g['Kj'])
        P = [np.hstack([cal['K'][c], np.zeros((3, 1))]) @ np.vstack([np.hstack([cal['R_mat'][c], cal['T'][c].reshape(3, 1)]), [0, 0, 0, 1]]) for c in range(C)]
        engine.set_calibration(P, cal)
        n_persons, kpts = _pack(frames, C, Kj)
        prm = engine.assoc_params(float(g['recon_thr']), float(g['min_aff']), int(g['min_cams']))
        aff = engine.associate(n_persons, kpts, prm)
        for f in range(len(frames)):
            N = int(n_persons[f].sum())
            ref = g['result'][f, :N, :N]
            d = np.abs(aff[f, :N, :N] - ref).max() if N else 0.0
            worst = max(worst, d)
            assert d <= 1e-7, (i, f, d)
            cum = np.cumsum([0] + list(n_persons[f]))
            props = pa.person_index_per_cam(aff[f, :N, :N].copy(), cum, int(g['min_cams']))
            k = int(g['n_props'][f])
            props = np.asarray(props, dtype=float).reshape(-1, C) if np.asarray(props).size else np.zeros((0, C))
            assert props.shape[0] == k and np.array_equal(props, g['proposals'][f, :k], equal_nan=True), (i, f)
    print(f'association: worst |d affinity| = {worst:.3e}')


def test_counters(engine, golden_dir):
    """p2s_get_assoc_stats: one count per frame with detections, passes within max_iter, a plausible operation count."""
    i, g = next(iter(_assoc_groups(golden_dir)))
    cal, frames = assoc_frames_of(g)
    C, Kj = int(g['C']), int(g['Kj'])
    P = [np.hstack([cal['K'][c], np.zeros((3, 1))]) @ np.vstack([np.hstack([cal['R_mat'][c], cal['T'][c].reshape(3, 1)]), [0, 0, 0, 1]]) for c in range(C)]
    engine.set_calibration(P, cal)
    n_persons, kpts = _pack(frames, C, Kj)
    engine.assoc_stats(reset=True)
    engine.associate(n_persons, kpts, engine.assoc_params(float(g['recon_thr']), float(g['min_aff']), int(g['min_cams']), max_iter=7))
    st = engine.assoc_stats(reset=True)
    nonempty = int((n_persons.sum(axis=1) > 0).sum())
    assert st['frames'] == nonempty
    assert nonempty <= st['admm_passes'] <= 7 * nonempty
    assert st['admm_passes'] <= st['jacobi_sweeps'] <= 40 * st['admm_passes']
    N = n_persons.sum(axis=1).astype(np.int64)
    assert st['fp64_flops'] >= int((N ** 3).sum())          # at least one product per frame
    assert engine.assoc_stats()['frames'] == 0


def test_edge_frames(engine):
    """No detections at all, a single detection, one camera only."""
    from oracle import association_ref as ar
    from pose2sim_amd import synth
    cams = synth.make_cameras(4, seed=5)
    P = synth.projection_matrices(cams)
    engine.set_calibration(P, cams)
    rng = np.random.default_rng(0)
    Kj = 26
    person = rng.uniform(100, 900, (Kj, 3)); person[:, 2] = 0.8
    frames = [[[], [], [], []], [[person.ravel()], [], [], []], [[person.ravel(), person.ravel() + 3], [], [], []]]
    n_persons, kpts = _pack(frames, 4, Kj)
    prm = engine.assoc_params(0.1, 0.2, 2)
    aff = engine.associate(n_persons, kpts, prm)
    cal = {'inv_K': cams['inv_K'], 'R_mat': cams['R_mat'], 'T': cams['T']}
    for f, per_cam in enumerate(frames):
        N = int(n_persons[f].sum())
        _, ref, _ = ar.associate_frame(per_cam, cal, 0.1, 0.2, 2)
        if N:
            assert np.abs(aff[f, :N, :N] - ref).max() <= 1e-9


def _every_order(engine, max_iter, f64):
    from oracle import association_ref as ar
    from pose2sim_amd.engine import P2S_F32, P2S_F64, as_packed
    C, Pn, Kj = 10, 5, 26
    cams = synth.make_cameras(C, seed=21)
    P = synth.projection_matrices(cams)
    xyl = synth.make_observations(synth.make_points3d(48, Pn, Kj, seed=22), cams, seed=22, p_missing_cam=0.0, p_outlier=0.0)   # [F][Pn][C][K][3]
    cal = {'inv_K': cams['inv_K'], 'R_mat': cams['R_mat'], 'T': cams['T']}
    rng = np.random.default_rng(23)
    frames = []
    for total in range(1, 49):
        counts = np.zeros(C, dtype=int)
        for _ in range(total):                            # spread `total` detections over the cameras, at most Pn each
            c = rng.choice(np.flatnonzero(counts < Pn))
            counts[c] += 1
        # float64: the float32 numbers shifted off the float32 grid, the oracle reads the same
        frames.append([[(np.nan_to_num(xyl[total - 1, p, c]).astype(np.float32).astype(np.float64) + (1e-9 if f64 else 0.0)).ravel()
                        for p in rng.permutation(Pn)[:counts[c]]] for c in range(C)])
    engine.set_calibration(P, cams)
    min_aff = 0.2 if max_iter == 20 else -1.0
    prm = engine.assoc_params(0.1, min_aff, 2, max_iter=max_iter)
    worst = 0.0
    for lo, hi in ((0, 16), (0, 32), (0, 48)):            # largest frame of the call: 16, 32, 48 detections
        n_persons, kpts = _pack(frames[lo:hi], C, Kj)
        kpts = kpts if f64 else kpts.astype(np.float32)
        assert as_packed(kpts)[1] == (P2S_F64 if f64 else P2S_F32)
        aff = engine.associate(n_persons, kpts, prm)
        for f, per_cam in enumerate(frames[lo:hi]):
            N = int(n_persons[f].sum())
            cum = np.cumsum([0] + [len(p) for p in per_cam])
            ref = ar.match_svt(ar.affinity_matrix(per_cam, cal, cum, 0.1), cum, max_iter=max_iter)
            if max_iter == 20:
                ref = np.where(ref < min_aff, 0.0, ref)
            d = float(np.abs(aff[f, :N, :N] - ref).max())
            worst = max(worst, d)
            assert d <= 1e-9, (hi, N, d)
    print(f'orders 1..48, {"float64" if f64 else "float32"}, max_iter {max_iter}: worst |d| = {worst:.3e}')


@pytest.mark.parametrize('max_iter', [20, 3])
def test_every_matrix_order(engine, max_iter):
    """Frames of 1 .. 48 detections (odd and even orders, empty cameras, one frame per order, up to
    P2S_MAX_PERSONS_TOTAL): the symmetric one-wave kernel up to 32 -- its 16-row form when the largest frame of a call
    has at most 16 -- and the general kernel above, against the oracle; converged result and the continuous iterate
    after 3 passes.  float32 keypoints."""
    _every_order(engine, max_iter, False)


@pytest.mark.parametrize('max_iter', [20, 3])
def test_every_matrix_order_float64(engine, max_iter):
    """The same orders through the float64 instantiations (keypoints that are not float32-representable, as a JSON
    file's numbers usually are not)."""
    _every_order(engine, max_iter, True)


def test_partial_iterations_match_oracle(engine, golden_dir):
    """The converged matchSVT result is binary; stopping the ADMM loop after 1, 2, 3 and 5 iterations
    exposes the continuous iterates (SVD-thresholded values), compared with the oracle at 1e-9."""
    from oracle import association_ref as ar
    worst = 0.0
    for i, g in _assoc_groups(golden_dir):
        if i not in (1, 2):
            continue
        cal, frames = assoc_frames_of(g)
        frames = frames[:12]
        C, Kj = int(g['C']), int(g['Kj'])
        P = [np.hstack([cal['K'][c], np.zeros((3, 1))]) @ np.vstack([np.hstack([cal['R_mat'][c], cal['T'][c].reshape(3, 1)]), [0, 0, 0, 1]]) for c in range(C)]
        engine.set_calibration(P, cal)
        n_persons, kpts = _pack(frames, C, Kj)
        for it in (1, 2, 3, 5):
            prm = engine.assoc_params(float(g['recon_thr']), -1.0, int(g['min_cams']), max_iter=it)
            aff = engine.associate(n_persons, kpts, prm)
            for f, per_cam in enumerate(frames):
                N = int(n_persons[f].sum())
                cum = np.cumsum([0] + [len(p) for p in per_cam])
                a0 = ar.affinity_matrix(per_cam, cal, cum, float(g['recon_thr']))
                ref = ar.match_svt(a0, cum, max_iter=it)
                d = np.abs(aff[f, :N, :N] - ref).max() if N else 0.0
                worst = max(worst, d)
                assert d <= 1e-9, (i, it, f, d)
    assert worst > 0.0          # the comparison was on continuous values
    print(f'partial iterations: worst |d| = {worst:.3e}')


# ---- hard frames (tests/assoc_hard.py; the fixture itself is checked on the CPU by tests/test_assoc_hard_host.py) ----
def _prepare(engine, frames, cams, Kj, f64):
    from pose2sim_amd.engine import P2S_F32, P2S_F64, as_packed
    engine.set_calibration(synth.projection_matrices(cams), cams)
    n_persons, kpts = _pack(frames, len(cams['K']), Kj)
    kpts = kpts if f64 else kpts.astype(np.float32)
    assert as_packed(kpts)[1] == (P2S_F64 if f64 else P2S_F32)
    return n_persons, kpts


def _deviations(aff, n_persons, refs):
    """Per frame |kernel - oracle| over the N x N block.  Neither side holds a NaN (so the NaN patterns are identical:
    empty) and everything outside the block is exactly 0."""
    out = []
    for f, ref in enumerate(refs):
        N = int(n_persons[f].sum())
        assert ref.shape == (N, N) and not np.isnan(ref).any(), f
        assert not np.isnan(aff[f]).any(), f
        outside = aff[f].copy()
        outside[:N, :N] = 0.0
        assert not outside.any(), f
        out.append(float(np.abs(aff[f, :N, :N] - ref).max()) if N else 0.0)
    return out


@pytest.mark.parametrize('Kj, f64', [(k, False) for k in ah.KJ_ALL] + [(k, True) for k in ah.KJ_F64])
def test_affinity_alone_at_every_keypoint_count(engine, Kj, f64):
    """max_iter = 0: rays, affinity and circular constraint alone, on hard frames (NaN joints of every kind, zero
    likelihoods, ghosts, a blank person, one camera only) of 1 .. 135 keypoints.  Three calls per keypoint count, the
    largest frame in <= 16, 17 .. 32 and 33 .. 48 detections and N falling to 1 within each, so that the chunk of joints
    the ray stage holds at a time is larger than Kj, equal to it, smaller, and leaves a last chunk of one joint
    (test_assoc_hard_host.py::test_affinity_frames_reach_every_chunk_size); recon_thr 0.05, 0.1 and 0.3 spread over
    the cases.  1e-9 on every entry, no NaN on either side, exact zeros outside the N x N block.
    Measured on an MI355X: worst 9.8e-14 (both forms, float32 and float64)."""
    worst = []
    for k, (_, _, lo, hi) in enumerate(ah.SIZE_CLASSES):
        frames, cams, thr, refs = ah.affinity_call(Kj, k, f64)
        n_persons, kpts = _prepare(engine, frames, cams, Kj, f64)
        assert lo <= n_persons.sum(axis=1).max() <= hi and n_persons.sum(axis=1).min() == 1
        aff = engine.associate(n_persons, kpts, engine.assoc_params(thr, -1.0, 2, max_iter=0))
        worst.append(max(_deviations(aff, n_persons, refs)))
    print(f'affinity alone, Kj {Kj}, {"float64" if f64 else "float32"}: worst |d| = ' + ', '.join(f'{w:.3e}' for w in worst) +
          ' (largest frame <= 16, <= 32, <= 48)')
    assert max(worst) <= 1e-9, worst


@pytest.mark.parametrize('Kj, C, n_per_cam', [(26, 3, 2), (26, 8, 4), (133, 3, 2), (133, 8, 4)])
def test_every_joint_counts_once(engine, Kj, C, n_per_cam):
    """One frame per joint j, every likelihood 0 but joint j's: the affinity hangs on that joint alone.  A kernel that
    drops a joint of a chunk finds distance 0 there (affinity 1), one that reads a neighbour finds another distance.
    6 and 32 detections per frame: large and small chunks.  max_iter = 0, 1e-9 against the oracle.
    Measured on an MI355X: worst 5.4e-14 (both forms)."""
    frames, cams, refs = ah.one_hot_call(Kj, C, n_per_cam)
    n_persons, kpts = _prepare(engine, frames, cams, Kj, False)
    aff = engine.associate(n_persons, kpts, engine.assoc_params(0.1, -1.0, 2, max_iter=0))
    dev = _deviations(aff, n_persons, refs)
    print(f'one live joint, Kj {Kj}, N {C * n_per_cam}: worst |d| = {max(dev):.3e}')
    # the fixture discriminates: the frames differ from each other, and each holds affinities strictly between 0 and 1
    assert np.stack(refs).std(axis=0).max() > 0.01
    assert all(((r > 0) & (r < 1)).any() for r in refs)
    assert max(dev) <= 1e-9, int(np.argmax(dev))


HARD_CASES = [(i, False) for i in range(len(ah.HARD_SHAPES))] + [(i, True) for i in ah.HARD_F64]


@pytest.mark.parametrize('shape, f64', HARD_CASES)
def test_hard_frames_after_every_pass_count(engine, shape, f64):
    """Noisy frames (6 px, 20 % outliers, NaN and zero-likelihood joints, ghosts, a blank person, two people 25 cm
    apart) that are still non-binary after 20 passes: mu is doubled and halved on the way, the Jacobi iteration is warm
    started 19 times and the symmetric form's shift follows a grown Y.  The uncut iterate after at most 1, 2, 3, 5 and 20
    passes within 1e-9 of the oracle's, and as many ADMM passes as the oracle made, its early break included.
    Measured on an MI355X: worst 1.6e-14, 2.9e-14, 5.0e-14, 1.2e-13 and 1.4e-12 after 1, 2, 3, 5 and 20 passes, the pass
    counts equal (symmetric form on the four shapes up to 32 detections, general form on (10, 4, 26, 48)).  The general form
    gave NaN on the rank-deficient frames of the other shapes -- the null-column underflow of jacobi_svd_t, fixed in
    csrc/p2s_assoc.hip with these tests; the figures above were taken before that fix, which does not touch those paths."""
    C, Pn, Kj, n_cap, thr = ah.HARD_SHAPES[shape]
    frames, cams, thr, _, refs = ah.hard_call(shape, f64)
    n_persons, kpts = _prepare(engine, frames, cams, Kj, f64)
    worst, passes, want = {}, {}, {}
    for it in ah.PASS_COUNTS:
        engine.assoc_stats(reset=True)
        aff = engine.associate(n_persons, kpts, engine.assoc_params(thr, -1.0, 2, max_iter=it))
        st = engine.assoc_stats(reset=True)
        assert st['frames'] == len(frames)
        worst[it] = max(_deviations(aff, n_persons, [r[it][0] for r in refs]))
        passes[it], want[it] = st['admm_passes'], sum(r[it][1] for r in refs)
    print(f'hard frames {ah.HARD_SHAPES[shape]}, {"float64" if f64 else "float32"}: worst |d| after ' +
          ', '.join(f'{it} passes {w:.3e}' for it, w in worst.items()) + f'; ADMM passes {passes}, the oracle\'s {want}')
    assert max(worst.values()) <= 1e-9, worst
    assert worst[20] > 0.0          # the comparison was on continuous values
    assert passes == want


@pytest.mark.parametrize('shape, f64', HARD_CASES)
def test_hard_frames_give_the_oracles_proposals(engine, shape, f64):
    """The same frames through the product's setting (min_affinity 0.2, 20 passes): person_index_per_cam on the kernel's
    matrix gives the oracle's proposals.  A frame is left out only when the ORACLE's own uncut matrix has an entry within
    1e-7 of the cut or the two largest kept entries of some (row, camera block) within 1e-7 of each other -- 100 x the
    matrix bar, and at most 1 frame in 20 (the oracle alone meets that: test_assoc_hard_host.py).
    Measured on an MI355X: 0 of 16 frames left out in every shape, cut matrix within 1.4e-12."""
    from oracle import association_ref as ar
    from pose2sim_amd import personAssociation as pa
    C, Pn, Kj, n_cap, thr = ah.HARD_SHAPES[shape]
    frames, cams, thr, _, refs = ah.hard_call(shape, f64)
    n_persons, kpts = _prepare(engine, frames, cams, Kj, f64)
    aff = engine.associate(n_persons, kpts, engine.assoc_params(thr, ah.MIN_AFFINITY, ah.MIN_CAMS, max_iter=20))
    left_out, different, worst = 0, [], 0.0
    for f, per_cam in enumerate(frames):
        N, cum, X = int(n_persons[f].sum()), ah.cum_of(per_cam), refs[f][20][0]
        if not ah.proposals_decided(X, cum):
            left_out += 1
            continue
        cut = np.where(X < ah.MIN_AFFINITY, 0.0, X)
        worst = max(worst, float(np.abs(aff[f, :N, :N] - cut).max()))
        want = np.asarray(ar.proposals_from_affinity(cut, cum, ah.MIN_CAMS), dtype=float)
        got = np.asarray(pa.person_index_per_cam(aff[f, :N, :N].copy(), cum, ah.MIN_CAMS), dtype=float)
        want = want.reshape(-1, C) if want.size else np.zeros((0, C))
        got = got.reshape(-1, C) if got.size else np.zeros((0, C))
        if got.shape != want.shape or not np.array_equal(got, want, equal_nan=True):
            different.append(f)
    print(f'hard frames {ah.HARD_SHAPES[shape]}, {"float64" if f64 else "float32"}: {left_out} of {len(frames)} frames left out, '
          f'different proposals in {different}, worst |d| of the cut matrix {worst:.3e}')
    assert 20 * left_out <= len(frames)
    assert not different and worst <= 1e-9


def test_association_refusals(engine):
    """p2s_associate_host through the raw library on a calibrated context: the return code and the exact p2s_last_error()
    text of everything it refuses, each before a launch (the frame counter stays 0)."""
    import ctypes as C
    from pose2sim_amd import _lib
    lib = _lib.load()
    cams = synth.make_cameras(2, seed=3)
    engine.set_calibration(synth.projection_matrices(cams), cams)
    engine.assoc_stats(reset=True)
    INVALID, NO_CALIB, Kj = -1, -4, 2
    ptr = lambda a: a.ctypes.data_as(C.c_void_p)                    # noqa: E731
    kpts, out = np.ones((7, Kj, 3), dtype=np.float32), np.zeros((2, 50, 50))
    good = dict(n_frames=2, n_max=6, dtype=0, n_persons=[[1, 1], [2, 3]], offsets=[0, 2, 7], thr=0.1, max_iter=20)

    def call(ctx, **kw):
        a = dict(good, **kw)
        n_persons, offsets = np.array(a['n_persons'], dtype=np.int32), np.array(a['offsets'], dtype=np.int64)
        prm = engine.assoc_params(a['thr'], 0.2, 2, max_iter=a['max_iter'])
        return lib.p2s_associate_host(ctx, a['n_frames'], Kj, a['n_max'], a['dtype'], ptr(n_persons), ptr(offsets), ptr(kpts),
                                      C.byref(prm), ptr(out))
    cases = [
        (dict(n_max=50), 'n_max=50 outside [1, 48]'),
        (dict(n_max=0), 'n_max=0 outside [1, 48]'),
        (dict(dtype=2), 'dtype must be P2S_F32 or P2S_F64'),
        (dict(thr=0.0), 'reconstruction_error_threshold must be > 0'),
        (dict(thr=float('nan')), 'reconstruction_error_threshold must be > 0'),
        (dict(max_iter=-1), 'max_iter < 0'),
        (dict(n_max=4), 'frame 1 has 5 detections > n_max=4'),
        (dict(offsets=[0, 3, 7]), 'offsets[1] does not match n_persons'),
        (dict(offsets=[0, 2, 8]), 'offsets[F] does not match n_persons'),
        (dict(n_persons=[[1, 1], [-1, 3]], offsets=[0, 2, 4]), 'negative person count'),
        (dict(n_max=5), 'n_max must be even (pad the affinity stride)'),
        (dict(n_frames=-1), 'bad shape'),
    ]
    for kw, text in cases:
        assert call(engine._h, **kw) == INVALID, kw
        assert lib.p2s_last_error().decode() == text, kw
    fresh = C.c_void_p()
    assert lib.p2s_create(0, C.byref(fresh)) == 0, lib.p2s_last_error()
    try:
        assert call(fresh) == NO_CALIB
        assert lib.p2s_last_error().decode() == 'association needs K, R and T in p2s_set_calibration'
    finally:
        lib.p2s_destroy(fresh)
    prm = engine.assoc_params(0.1, 0.2, 2)
    assert lib.p2s_associate_host(engine._h, 0, Kj, 6, 0, None, None, None, C.byref(prm), None) == 0      # no frames: P2S_OK
    assert engine.assoc_stats()['frames'] == 0
    assert call(engine._h) == 0 and engine.assoc_stats(reset=True)['frames'] == 2                         # and the good call runs


# ---- single-person mode ---------------------------------------------------------------------------
def _single_inputs(per_frame, kid):
    n_persons = np.array([[len(p) for p in per_cam] for per_cam in per_frame], dtype=np.int32)
    tracked = np.array([np.asarray(p)[kid * 3:kid * 3 + 3] for per_cam in per_frame for people in per_cam for p in people],
                       dtype=np.float64).reshape(-1, 3)
    return n_persons, tracked


def _check_single(comb, err, Q, want_comb, want_err, want_Q, tag):
    """Identical person / camera choice; error within 1e-6 px (a 1e-10 m change of Q moves a pixel error by
    ~1e-7 px at these focal lengths / distances); Q within 1e-7 m (north_star)."""
    for f in range(len(err)):
        wc = np.where(np.isnan(want_comb[f]), -1, want_comb[f]).astype(np.int32)
        assert np.array_equal(comb[f], wc), (tag, f, comb[f], wc)
        if np.isinf(want_err[f]):
            assert np.isinf(err[f]) and np.isnan(Q[f]).all(), (tag, f)
            continue
        assert abs(err[f] - want_err[f]) <= 1e-6 * max(1.0, abs(want_err[f])), (tag, f, err[f], want_err[f])
        assert np.allclose(Q[f], want_Q[f], rtol=0, atol=1e-7), (tag, f, Q[f], want_Q[f])


@pytest.mark.gpu
def test_single_person_matches_reference_goldens(engine, golden_dir):
    """Per-frame best error / combination / 3D point recorded from the reference's
    best_persons_and_cameras_combination (tests/golden/make_golden_e2e_single.py)."""
    from test_oracle_golden import single_frames_of
    z = np.load(os.path.join(golden_dir, 'e2e_single.npz'))
    for name in [str(n) for n in z['cases']]:
        P, frames = single_frames_of(z, name)
        eng = engine
        eng.set_calibration(np.array(P))
        n_persons, tracked = _single_inputs(frames, 18)
        comb, err, Q = eng.associate_single(n_persons, tracked, float(z[f'{name}_thr']), 0.3, int(z[f'{name}_min_cams']))
        _check_single(comb, err, Q, z[f'{name}_best_comb'], z[f'{name}_best_err'], z[f'{name}_best_Q'], name)


@pytest.mark.gpu
@pytest.mark.parametrize('C,min_cams,thr,seed', [(3, 2, 8.0, 1), (4, 2, 4.0, 2), (6, 3, 6.0, 3), (8, 4, 5.0, 4), (5, 2, 0.5, 5)])
def test_single_person_matches_oracle_on_random_trials(engine, C, min_cams, thr, seed):
    """More cameras, tighter thresholds (deeper camera-removal levels, more than 64 combinations per
    frame, frames where nothing qualifies) against the pinned oracle."""
    _random_single_trial(engine, C, min_cams, thr, seed, False)


@pytest.mark.gpu
@pytest.mark.parametrize('C,min_cams,thr,seed', [(3, 2, 8.0, 1), (4, 2, 4.0, 2), (6, 3, 6.0, 3), (8, 4, 5.0, 4), (5, 2, 0.5, 5)])
def test_single_person_float32_matches_oracle_on_random_trials(engine, C, min_cams, thr, seed):
    """The same trials with the keypoints rounded to float32: the float32 instantiation of the kernel (the one the
    product takes for float32-representable JSON numbers), the oracle on the same rounded numbers."""
    _random_single_trial(engine, C, min_cams, thr, seed, True)


def _random_single_trial(engine, C, min_cams, thr, seed, f32):
    from e2e_common import make_single_scene
    from oracle import association_single_ref as sr
    from pose2sim_amd.engine import P2S_F32, P2S_F64, as_packed
    cams, frames = make_single_scene(24, C, 26, 100 + seed, n_distract=3 if C <= 5 else 1)
    if f32:
        frames = [[[np.asarray(p, dtype=np.float32).astype(np.float64) for p in people] for people in per_cam] for per_cam in frames]
    P = synth.projection_matrices(cams)
    eng = engine
    eng.set_calibration(np.array(P))
    n_persons, tracked = _single_inputs(frames, 18)
    assert as_packed(tracked)[1] == (P2S_F32 if f32 else P2S_F64)
    comb, err, Q = eng.associate_single(n_persons, tracked, thr, 0.3, min_cams)
    want_c, want_e, want_q = [], [], []
    for per_cam in frames:
        e, cb, q = sr.best_persons_and_cameras(per_cam, sr.persons_combinations([len(p) for p in per_cam]), P, 18, thr,
                                               min_cams, 0.3)
        want_c.append(cb); want_e.append(e); want_q.append(q)
    _check_single(comb, err, Q, np.array(want_c), np.array(want_e), np.array(want_q), f'C{C}' + (' f32' if f32 else ''))


def _planted_frame(P, counts, true_pos, rng, noise=1.0, bad_cam=None, dup=None):
    """One frame of the tracked keypoint: camera c holds counts[c] detections, the person of interest at true_pos[c] and
    distractors 400-800 px away from it (so that a combination below a threshold of a few px is made of the person
    only).  bad_cam: that camera's detection of the person is 300 px off, so nothing qualifies until it is switched off.
    dup = (camera, index): a second, identical detection of the person there (an exact tie between two combinations)."""
    X = np.array([rng.uniform(-0.5, 0.5), rng.uniform(-0.5, 0.5), rng.uniform(0.8, 1.6), 1.0])
    per_cam = []
    for c, n in enumerate(counts):
        h = P[c] @ X
        uv = h[:2] / h[2] + rng.normal(0, noise, 2)
        if c == bad_cam:
            a = rng.uniform(0, 2 * np.pi)
            uv = uv + 300.0 * np.array([np.cos(a), np.sin(a)])
        me = np.array([uv[0], uv[1], rng.uniform(0.5, 1.0)])
        people = []
        for i in range(n):
            if i == true_pos[c] or (dup is not None and dup == (c, i)):
                people.append(me.copy())
            else:
                a = rng.uniform(0, 2 * np.pi)
                people.append(np.array([*(uv + rng.uniform(400, 800) * np.array([np.cos(a), np.sin(a)])), rng.uniform(0.5, 1.0)]))
        per_cam.append(people)
    return per_cam


def _digits(index, counts):
    """Mixed-radix digits of a combination index (itertools.product order: the last camera varies fastest)."""
    out = []
    for n in reversed(counts):
        out.append(index % n)
        index //= n
    return out[::-1]


@pytest.mark.gpu
@pytest.mark.parametrize('f32', [False, True])
def test_single_person_planted_frames(engine, f32):
    """The person of interest planted among far-away distractors, so that the combination the reference's scan stops at
    is known: the first one below the threshold at index 63, 64, 65, 127, 128 and 6560 (the last of 3^8); nothing below
    the threshold at level 0 and the first qualifying combination of level 1 past a pass boundary; exact ties between two
    combinations of one 64-lane pass (min_cameras = C: level 0 only, every combination looked at, the earliest wins);
    16 detections on a camera (P2S_MAX_PERSONS_PER_CAM); 12 cameras of 2 detections (4 096 combinations).  float32 and
    float64 numbers, both against the oracle."""
    from oracle import association_single_ref as sr
    from pose2sim_amd.engine import P2S_F32, P2S_F64, as_packed
    rng = np.random.default_rng(61 + f32)
    c8, c16, c12 = [3] * 8, [16, 3, 2, 16], [2] * 12
    first_below = [(c8, _digits(i, c8), {}) for i in (63, 64, 65, 127, 128, 6560) for _ in range(2)]
    level1 = []
    for first in (64, 100, 200, 2000):                   # camera 0 off: the first qualifying combination has its digit 0
        pos = _digits(first, c8)
        pos[0] = int(rng.integers(1, 3))
        level1.append((c8, pos, dict(bad_cam=0)))
    level1 += [(c8, _digits(i, c8), dict(bad_cam=7)) for i in (69, 129)]
    ties = []
    for counts in ([2, 2, 4, 4], [4, 4, 2, 2], [1, 4, 4, 4]):
        for _ in range(6):
            pos = [int(rng.integers(0, n)) for n in counts]
            c = int(rng.choice([i for i, n in enumerate(counts) if n > 1]))
            other = int(rng.choice([i for i in range(counts[c]) if i != pos[c]]))
            ties.append((counts, pos, dict(noise=2.0, dup=(c, other))))
    groups = [  # (cameras' seed, C, thr, min_cameras, frames)
        (31, 8, 8.0, 2, first_below + level1),
        (32, 4, 0.2, 4, ties),
        (33, 4, 8.0, 2, [(c16, _digits(i, c16), {}) for i in (1535, 1534, 770, 15)]),
        (34, 12, 8.0, 2, [(c12, _digits(i, c12), {}) for i in (4095, 2049, 63, 64)]),
    ]
    for seed, C, thr, min_cams, specs in groups:
        cams = synth.make_cameras(C, seed=seed)
        P = [np.asarray(p) for p in synth.projection_matrices(cams)]
        engine.set_calibration(np.array(P))
        frames = [_planted_frame(P, counts, pos, rng, **kw) for counts, pos, kw in specs]
        if f32:
            frames = [[[np.asarray(p, dtype=np.float32).astype(np.float64) for p in people] for people in per_cam] for per_cam in frames]
        n_persons, tracked = _single_inputs(frames, 0)
        assert as_packed(tracked)[1] == (P2S_F32 if f32 else P2S_F64)
        comb, err, Q = engine.associate_single(n_persons, tracked, thr, 0.3, min_cams)
        want_c, want_e, want_q = [], [], []
        for per_cam in frames:
            e, cb, q = sr.best_persons_and_cameras(per_cam, sr.persons_combinations([len(p) for p in per_cam]), P, 0, thr,
                                                   min_cams, 0.3)
            want_c.append(cb); want_e.append(e); want_q.append(q)
        _check_single(comb, err, Q, np.array(want_c), np.array(want_e), np.array(want_q), f'planted C{C} thr {thr}')
        assert np.isfinite(err).all()                   # every planted frame has a solution


@pytest.mark.gpu
def test_single_person_edge_cases(engine):
    cams = synth.make_cameras(4, seed=9)
    eng = engine
    eng.set_calibration(np.array(synth.projection_matrices(cams)))
    # no frames; a frame with no detections at all; a frame with one camera only
    comb, err, Q = eng.associate_single(np.zeros((0, 4), np.int32), np.zeros((0, 3)), 10.0, 0.3, 2)
    assert comb.shape == (0, 4) and err.shape == (0,)
    n_persons = np.array([[0, 0, 0, 0], [1, 0, 0, 0]], dtype=np.int32)
    comb, err, Q = eng.associate_single(n_persons, np.array([[100.0, 100.0, 0.9]]), 10.0, 0.3, 2)
    assert (comb == -1).all() and np.isinf(err).all() and np.isnan(Q).all()
    with pytest.raises(P2sError):
        eng.associate_single(np.full((1, 4), 17, np.int32), np.zeros((68, 3)), 10.0, 0.3, 2)
    # 3^12 combinations x 4083 camera subsets in the worst case: refused before anything is launched
    cams12 = synth.make_cameras(12, seed=9)
    eng.set_calibration(np.array(synth.projection_matrices(cams12)))
    with pytest.raises(P2sError, match='evaluations exceed'):
        eng.associate_single(np.full((1, 12), 3, np.int32), np.zeros((36, 3)), 10.0, 0.3, 2)
