"""Hard frames for the multi-person association kernels -- TEST INFRASTRUCTURE, NumPy only, no GPU.

What the recorded and the clean synthetic frames never hold: noisy keypoints (6 px, 20 % outliers, 20 % low likelihoods),
joints with NaN in x, y, the likelihood or all three, likelihoods of exactly 0, persons a camera does not see, ghost
detections, a blank (all-NaN) person, two people 25 cm apart, a frame with one camera only, odd and even orders from 1 up to
a cap, and every keypoint count from 1 to 135.  tests/test_assoc_hard_host.py checks that the generators deliver all that
and that the oracle is well conditioned on it; tests/test_assoc_gpu.py runs both kernels on it.

Two things are kept out on purpose: two identical detections in one camera and more than one blank
person per frame give exact ties that np.argmax breaks by 1e-13 rounding noise in the reference as well, and a negative
likelihood makes the reference's sqrt a NaN on which numpy.linalg.svd raises.  The generator asserts all three.

The oracle's results for the cases the tests share are computed once per process (functools.lru_cache) and handed out
read-only.
"""
import contextlib
import functools

import numpy as np

from oracle import association_ref as ar
from pose2sim_amd import synth

NAN_KINDS = ((0,), (1,), (2,), (0, 1, 2))          # a joint's NaN: x only, y only, likelihood only, all three
RECON_THRS = (0.05, 0.1, 0.3)

# test_affinity_alone_at_every_keypoint_count: every Kj with three calls whose largest frame is in <= 16, 17..32, 33..48
KJ_ALL = (1, 2, 3, 7, 8, 17, 25, 26, 33, 133, 135)
KJ_F64 = (1, 26, 133)
SIZE_CLASSES = ((6, 4, 1, 16), (10, 5, 17, 32), (12, 6, 33, 48))      # (cameras, persons, smallest and largest N of the class)
AFFINITY_FRAMES = 12
AFFINITY_SEED = 3000

# test_hard_frames_*: (cameras, persons, Kj, n_cap, recon_thr); float64 as well for HARD_F64
HARD_SHAPES = ((3, 2, 17, 16, 0.1), (4, 3, 26, 16, 0.05), (6, 4, 26, 32, 0.1), (8, 4, 133, 32, 0.3), (10, 4, 26, 48, 0.1),
               (8, 5, 7, 48, 0.1))
HARD_F64 = (1, 4)
HARD_FRAMES = 16
HARD_SEEDS = (411, 412, 413, 414, 415, 416)
PASS_COUNTS = (1, 2, 3, 5, 20)
MIN_AFFINITY, MIN_CAMS, MARGIN = 0.2, 2, 1e-7


def cal_of(cams):
    return {'inv_K': cams['inv_K'], 'R_mat': cams['R_mat'], 'T': cams['T']}


def cum_of(per_cam):
    return np.cumsum([0] + [len(p) for p in per_cam])


def _scene(C, Pn, Kj, F, seed):
    """Cameras and the noisy projections [F][Pn][C][Kj][3] (float32) of Pn people, person 1 25 cm beside person 0."""
    cams = synth.make_cameras(C, seed=seed)
    Q = synth.make_points3d(F, Pn, Kj, seed=seed + 1)
    if Pn >= 2:
        Q[:, 1] = Q[:, 0] + np.array([0.25, 0.0, 0.0]) + np.random.default_rng(seed + 3).normal(0, 0.05, (1, Kj, 3))
    xyl = synth.make_observations(Q, cams, seed=seed + 2, noise_px=6.0, p_outlier=0.2, p_lowlik=0.2, p_missing_cam=0.0)
    return cams, xyl


def _same(a, b):
    return np.array_equal(a, b, equal_nan=True)


def hard_frames_with_info(C, Pn, Kj, F, seed, n_cap, recon_case=0, f64=False, spread=False):
    """-> (frames, cams, info).  frames[f][c] = list of flat [x0, y0, l0, x1, ...] detections (what _pack of
    tests/test_assoc_gpu.py and the oracle take); info[f] = the kinds ('person', 'ghost', 'blank') of frame f's detections
    in packed order.

    recon_case picks the random stream of everything drawn per detection (NaN, zeros, unseen persons, ghosts, order), so
    that the calls of one scene with different thresholds do not repeat each other's frames; f64 moves the float32
    numbers off the float32 grid by 1e-9 without drawing anything else (zero likelihoods stay exactly 0); spread caps
    frame f at a count that falls evenly from n_cap (frame 0) to 1 (the last frame) instead of at n_cap."""
    cams, xyl = _scene(C, Pn, Kj, F, seed)
    rng = np.random.default_rng([seed, recon_case])
    shift = 1e-9 if f64 else 0.0
    n_nan = 0                                                     # the four kinds of NaN joint take turns
    frames, info = [], []
    for f in range(F):
        blank_cam = int(rng.integers(C)) if rng.random() < 0.25 else -1   # at most ONE blank person per frame
        if spread and f == 0:
            blank_cam = 0                                         # one where no trimming reaches it
        per_cam = []
        for c in range(C):
            people = []
            for p in rng.permutation(Pn):
                if rng.random() < 0.25:
                    continue                                      # this camera does not see the person
                k = xyl[f, p, c].astype(np.float64) + shift
                whole = k.copy()
                k[rng.random(Kj) < 0.1, 2] = 0.0
                for j in np.flatnonzero(rng.random(Kj) < 0.1):
                    k[j, list(NAN_KINDS[n_nan % 4])] = np.nan
                    n_nan += 1
                if np.isnan(k).all():                             # (a few joints only) that would be a second blank person
                    k[0] = whole[0]
                people.append(('person', k.ravel()))
            if rng.random() < 0.3:
                g = np.stack([rng.uniform(0, 1920, Kj), rng.uniform(0, 1080, Kj), rng.uniform(0.05, 0.5, Kj)], axis=1)
                people.append(('ghost', (g.astype(np.float32).astype(np.float64) + shift).ravel()))
            if c == blank_cam:
                people.append(('blank', np.full(Kj * 3, np.nan)))
            per_cam.append([people[i] for i in rng.permutation(len(people))])
        frames.append(per_cam)
    if F >= 2:                                                    # one frame with detections in a single camera only
        keep = int(np.argmax([len(p) for p in frames[1]]))
        frames[1] = [p if c == keep else [] for c, p in enumerate(frames[1])]
    for f in range(F):                                            # trim by dropping the last detections
        cap = n_cap - (f * (n_cap - 1)) // max(1, F - 1) if spread else n_cap
        _drop_last(frames[f], sum(len(p) for p in frames[f]) - cap)
    if not any(sum(len(p) for p in per_cam) % 2 for per_cam in frames):   # one frame with N odd
        _drop_last(frames[min(2, F - 1)], 1)
    for per_cam in frames:
        assert sum(kind == 'blank' or bool(np.isnan(k).all()) for p in per_cam for kind, k in p) <= 1
        for people in per_cam:
            assert not any(_same(a[1], b[1]) for i, a in enumerate(people) for b in people[:i]), 'identical detections in a camera'
            assert all(not (k[2::3] < 0).any() for _, k in people), 'negative likelihood'
        info.append([kind for p in per_cam for kind, _ in p])
    return [[[k for _, k in p] for p in per_cam] for per_cam in frames], cams, info


def _drop_last(per_cam, count):
    for people in reversed(per_cam):
        while count > 0 and people:
            people.pop()
            count -= 1


def hard_frames(C, Pn, Kj, F, seed, n_cap, recon_case=0, f64=False, spread=False):
    frames, cams, _ = hard_frames_with_info(C, Pn, Kj, F, seed, n_cap, recon_case, f64, spread)
    return frames, cams


def one_hot_frames(C, Kj, n_per_cam, joints, seed):
    """One frame per joint index j of `joints`: n_per_cam persons in each of C cameras, every likelihood 0 but joint
    j's (0.3 .. 1.0), noisy projections (one pose for the whole call: the frames differ by the live joint, its likelihood
    and the order of the persons), no NaN.  The affinity of a pair then hangs on joint j alone: a kernel that skips it
    finds distance 0 (affinity 1), one that reads a neighbour finds that neighbour's distance."""
    cams, xyl = _scene(C, n_per_cam, Kj, 1, seed)
    rng = np.random.default_rng([seed, 1])
    frames = []
    for j in joints:
        per_cam = []
        for c in range(C):
            people = []
            for p in rng.permutation(n_per_cam):
                k = xyl[0, p, c].astype(np.float64)
                assert not np.isnan(k).any()
                k[:, 2] = 0.0
                k[j, 2] = float(np.float32(rng.uniform(0.3, 1.0)))
                people.append(k.ravel())
            per_cam.append(people)
        frames.append(per_cam)
    return frames, cams


@contextlib.contextmanager
def rays_joint_by_joint():
    """While it is open, oracle.association_ref.rays_of_person is evaluated one joint at a time -- by the oracle's own
    function, whose rows do not depend on each other -- and every distinct (camera, x, y, likelihood) only once.  The
    133 frames of a one-hot call repeat 131 of 133 joints of every person; this keeps the oracle's Python loop over them
    to a second instead of half a minute, with bit-identical results (test_assoc_hard_host.py compares)."""
    whole, memo = ar.rays_of_person, {}

    def rays(kpts, inv_K, R_mat, T):
        kp = np.asarray(kpts, dtype=np.float64).reshape(-1, 3)
        out = np.empty((len(kp), 7))
        for i, key in enumerate(map(tuple, kp.tolist())):
            row = memo.get((id(inv_K), key))
            if row is None:
                row = memo[id(inv_K), key] = whole(kp[i], inv_K, R_mat, T)[0]
            out[i] = row
        return out
    ar.rays_of_person = rays
    try:
        yield
    finally:
        ar.rays_of_person = whole


def match_svt_counted(affinity, cum, max_iter):
    """oracle.association_ref.match_svt and the passes it made (its early break included): one SVT per pass, counted by a
    wrapper around the oracle's own singular_value_threshold for the length of the call."""
    svt, calls = ar.singular_value_threshold, [0]

    def counting(M, t):
        calls[0] += 1
        return svt(M, t)
    ar.singular_value_threshold = counting
    try:
        X = ar.match_svt(affinity, cum, max_iter=max_iter)
    finally:
        ar.singular_value_threshold = svt
    return X, calls[0]


def proposals_decided(uncut, cum, min_affinity=MIN_AFFINITY, margin=MARGIN):
    """False where a deviation far below `margin` could change the proposals of this matrix: an entry within `margin` of
    the min_affinity cut, or the two largest kept entries of some (row, camera block) within `margin` of each other."""
    if uncut.size and np.abs(uncut - min_affinity).min() <= margin:
        return False
    kept = np.where(uncut < min_affinity, 0.0, uncut)
    for r in range(kept.shape[0]):
        for c in range(len(cum) - 1):
            b = np.sort(kept[r, cum[c]:cum[c + 1]])
            if len(b) >= 2 and b[-1] > 0 and b[-1] - b[-2] <= margin:
                return False
    return True


def _frozen(a):
    a.flags.writeable = False
    return a


def affinity_seed(Kj, k):
    return AFFINITY_SEED + 10 * Kj + k


def affinity_thr(i_kj, k):
    """recon_thr of keypoint count KJ_ALL[i_kj], size class k: the three thresholds spread over the cases."""
    return RECON_THRS[(i_kj + k) % 3]


@functools.lru_cache(maxsize=None)
def affinity_call(Kj, k, f64):
    """One call of test_affinity_alone_at_every_keypoint_count -> (frames, cams, thr, refs): 12 hard frames with N falling
    from the class limit to 1, refs[f] = the oracle's affinity after the circular constraint with a zero diagonal."""
    C, Pn, _, n_cap = SIZE_CLASSES[k]
    thr = affinity_thr(KJ_ALL.index(Kj), k)
    frames, cams = hard_frames(C, Pn, Kj, AFFINITY_FRAMES, affinity_seed(Kj, k), n_cap, recon_case=RECON_THRS.index(thr), f64=f64, spread=True)
    cal = cal_of(cams)
    refs = []
    for per_cam in frames:
        cum = cum_of(per_cam)
        refs.append(_frozen(ar.match_svt(ar.affinity_matrix(per_cam, cal, cum, thr), cum, max_iter=0)))
    return frames, cams, thr, refs


@functools.lru_cache(maxsize=None)
def one_hot_call(Kj, C, n_per_cam):
    """One call of test_every_joint_counts_once -> (frames, cams, refs), a frame per joint, recon_thr 0.1."""
    frames, cams = one_hot_frames(C, Kj, n_per_cam, range(Kj), 2000 + Kj + C)
    cal = cal_of(cams)
    refs = []
    with rays_joint_by_joint():
        for per_cam in frames:
            cum = cum_of(per_cam)
            refs.append(_frozen(ar.match_svt(ar.affinity_matrix(per_cam, cal, cum, 0.1), cum, max_iter=0)))
    return frames, cams, refs


@functools.lru_cache(maxsize=None)
def hard_call(shape, f64):
    """Hard shape HARD_SHAPES[shape] -> (frames, cams, thr, affinity, refs): affinity[f] = the oracle's affinity matrix of
    frame f, refs[f][max_iter] = (the oracle's uncut matchSVT matrix after at most max_iter passes, the passes made) for
    max_iter 0 and PASS_COUNTS."""
    C, Pn, Kj, n_cap, thr = HARD_SHAPES[shape]
    frames, cams = hard_frames(C, Pn, Kj, HARD_FRAMES, HARD_SEEDS[shape], n_cap, f64=f64)
    cal = cal_of(cams)
    affinity, refs = [], []
    for per_cam in frames:
        cum = cum_of(per_cam)
        A = _frozen(ar.affinity_matrix(per_cam, cal, cum, thr))
        affinity.append(A)
        refs.append({it: (lambda X, n: (_frozen(X), n))(*match_svt_counted(A, cum, it)) for it in (0,) + PASS_COUNTS})
    return frames, cams, thr, affinity, refs
