"""NumPy restatement of Engine.fit_planes (include/p2s_floor.h): the live reference of tests/test_floor_gpu.py and
tests/test_floor_host.py, the builder of their cases and the holder of their bounds.  Test infrastructure, not a fallback:
the package never imports it.

The contract is restated with np.cross and np.linalg.eigh: nothing here shares an eigen-solver or a summation order with the
kernels.  The frame that calib_align_floor assembles from a plane (frame_of_plane) has no second implementation; the tests hold
it against the truth of the synthetic walks."""
import functools

import numpy as np

# The bounds of the tests: 100 x the worst figure of its kind measured against this mirror over the cases of
# tests/test_floor_gpu.py (DESIGN.md 4.23 lists them), under the cap on relative costs (1e-9).  The figures of the library's
# host path came first; the MI355X's replaced or confirmed them.
#
# A hypothesis' normal is a normalised cross product: its rounding error is eps / sin(angle of the sample's two edges), and d
# = n . p0 follows it with the size of the coordinates.  So every hypothesis is compared, none excluded, with its difference
# weighted by the sine that the mirror computes itself; the scoring alone is held to a bound of its own by letting the mirror
# score the library's plane.
# figure: worst measured on (the library's host path, the MI355X)
HYP_PLANE_SCALED_BOUND = 4.2e-14  # max |plane - plane_mirror| x sin; (2.34e-16, 4.13e-16)
HYP_COST_SCALED_BOUND = 6.0e-13   # |cost - cost_mirror| / (cost_mirror + thr^2) x sin, each side its own plane; (5.83e-15, 5.95e-15)
COST_REL_BOUND = 5.4e-13          # |cost - mirror's cost of the library's plane| / (cost + thr^2) of a hypothesis (the scoring alone); (5.22e-15, 5.34e-15)
RESULT_COST_REL_BOUND = 1.3e-13   # |cost - cost_mirror| / (cost_mirror + THR_FLOOR^2) of a problem's result; (1.29e-15, 4.36e-16)
RESULT_PLANE_BOUND = 5.2e-13      # max |plane - plane_mirror| of a result (n without a unit, d in m); (3.21e-15, 5.19e-15)
RESULT_CENTROID_BOUND = 1.2e-13   # m; (1.11e-15, 1.11e-15)
RESULT_EVALS_REL_BOUND = 2.3e-13  # |evals - evals_mirror| / evals_mirror[2]; (2.01e-15, 2.28e-15)
RESULT_FRAME_BOUND = 9.5e-13      # max |A - A_mirror|, |b - b_mirror| (m) of the frame assembled from a result; (9.44e-15 through a .trc, 3.15e-15)
# zero noise: 100 x the mirror's own worst error against the truth over ZERO_NOISE_N
ZERO_NOISE_NORMAL = 3.4e-14       # max |n - n_true|; the mirror's worst 3.33e-16; the library's (3.33e-16, 3.33e-16)
ZERO_NOISE_OFFSET = 3.1e-14       # m, |d - d_true|; the mirror's worst 3.05e-16; the library's (3.05e-16, 3.05e-16)
ZERO_NOISE_FRAME = 1.6e-13        # max |A - A_true|, |b - b_true| of the assembled frame; the mirror's worst 1.55e-15; the library's (6.11e-16, 3.33e-16)
THR_FLOOR = 0.01     # the smallest thr of a case, m: no_point_at_the_threshold divides an absolute bound on s by it
assert max(COST_REL_BOUND, RESULT_COST_REL_BOUND) <= 1e-9


def counts(points, usable):
    return np.asarray(usable, dtype=bool) & np.isfinite(np.asarray(points, dtype=np.float64)).all(axis=-1)


def hypothesis(pts, ok, ref, smp):
    """(plane [4], sin of the angle between the sample's edges) of the contract; NaN and 0 for a sample that is refused."""
    N = len(pts)
    bad = np.full(4, np.nan), 0.0
    if len(set(smp.tolist())) < 3 or (smp < 0).any() or (smp >= N).any() or not ok[smp].all():
        return bad
    p0, p1, p2 = pts[smp]
    with np.errstate(all='ignore'):
        c = np.cross(p1 - p0, p2 - p0)
        length = np.sqrt(c @ c)
        if not (np.isfinite(length) and length > 0):
            return bad
        n = c / length
        d = n @ p0
        s = n @ ref - d
        if not np.isfinite(s) or s == 0:
            return bad
        if s < 0:
            n, d = -n, -d
        return np.append(n, d), float(length / (np.linalg.norm(p1 - p0) * np.linalg.norm(p2 - p0)))


def signed(plane, x):
    with np.errstate(all='ignore'):
        return x @ plane[:3] - plane[3]


def score(plane, x, thr):
    """(cost, inliers, below, s) of the contract; +inf and 0 for a plane that is not finite."""
    s = signed(plane, x)
    if not np.isfinite(plane).all():
        return np.inf, 0, 0, s
    q = s * s
    with np.errstate(invalid='ignore'):
        return float(np.sum(np.where(q < thr * thr, q, np.where(q >= thr * thr, thr * thr, 0.0)))), int(np.sum(q < thr * thr)), int(np.sum(s < -thr)), s


def moments(x, ref):
    """(m, S): the mean about ref and the scatter over the count of the points x."""
    u = x - ref
    m = u.mean(axis=0)
    return m, (u[:, :, None] * u[:, None, :]).mean(axis=0) - np.outer(m, m)


def refit(x, ref):
    """The plane of the contract's refit on the inliers x, None when it is not finite or holds ref."""
    m, S = moments(x, ref)
    n = np.linalg.eigh(S)[1][:, 0]
    d = n @ (ref + m)
    s = n @ ref - d
    if not np.isfinite(np.append(n, d)).all() or not np.isfinite(s) or s == 0:
        return None
    return np.append(n, d) * (-1.0 if s < 0 else 1.0)


def fit_planes(points, usable, ref, samples, thr, rounds=3):
    """The contract, problem after problem.  Besides the library's outputs: hyp_sin [B][H] (0 for a refused sample), margin [B]
    (second best cost - best), near [B][H] and near_final [B]: the smallest | |s| - thr | / thr over the points."""
    points = np.asarray(points, dtype=np.float64)
    ok = counts(points, usable)
    samples = np.asarray(samples)
    B, H, _ = samples.shape
    N = points.shape[1]
    thr = np.broadcast_to(np.asarray(thr, dtype=np.float64), (B,))
    ref = np.asarray(ref, dtype=np.float64)
    out = {'plane': np.full((B, 4), np.nan), 'cost': np.full(B, np.nan), 'inliers': np.zeros(B, dtype=np.int32), 'below': np.zeros(B, dtype=np.int32),
           'winner': np.full(B, -1, dtype=np.int32), 'refits': np.zeros(B, dtype=np.int32), 'centroid': np.full((B, 3), np.nan),
           'evals': np.full((B, 3), np.nan), 'mask': np.zeros((B, N), dtype=bool), 'hyp_plane': np.full((B, H, 4), np.nan),
           'hyp_cost': np.full((B, H), np.inf), 'hyp_inliers': np.zeros((B, H), dtype=np.int32), 'hyp_sin': np.zeros((B, H)),
           'margin': np.full(B, np.inf), 'near': np.full((B, H), np.inf), 'near_final': np.full(B, np.inf)}
    for b in range(B):
        idx = np.flatnonzero(ok[b])
        x = points[b][idx]
        for h in range(H):
            plane, sin = hypothesis(points[b], ok[b], ref[b], samples[b, h])
            out['hyp_plane'][b, h], out['hyp_sin'][b, h] = plane, sin
            cost, inl, _, s = score(plane, x, thr[b])
            out['hyp_cost'][b, h], out['hyp_inliers'][b, h] = cost, inl
            if len(s) and np.isfinite(plane).all():
                out['near'][b, h] = np.min(np.abs(np.abs(s) - thr[b])) / thr[b]
        w = int(np.argmin(out['hyp_cost'][b]))
        if len(idx) < 3 or not np.isfinite(out['hyp_cost'][b, w]):
            continue
        out['winner'][b] = w
        if H > 1:
            out['margin'][b] = np.partition(out['hyp_cost'][b], 1)[1] - out['hyp_cost'][b, w]
        plane = out['hyp_plane'][b, w]
        cost, inl, below, s = score(plane, x, thr[b])
        for _ in range(rounds):
            if inl < 3:
                break
            trial = refit(x[s * s < thr[b] ** 2], ref[b])
            if trial is None:
                break
            ct, it, bt, st = score(trial, x, thr[b])
            if not ct < cost:
                break
            plane, cost, inl, below, s = trial, ct, it, bt, st
            out['refits'][b] += 1
        i = s * s < thr[b] ** 2
        out['plane'][b], out['cost'][b], out['inliers'][b], out['below'][b] = plane, cost, inl, below
        out['near_final'][b] = np.min(np.abs(np.abs(s) - thr[b])) / thr[b]
        out['mask'][b, idx[i]] = True
        m, S = moments(x[i], ref[b])
        out['centroid'][b], out['evals'][b] = ref[b] + m, np.linalg.eigvalsh(S)
    return out


def clear_winners(ref):
    """[B] bool: the mirror's two best costs of the problem differ by more than the bounds of both, so that no other winner
    lies within them."""
    B = len(ref['winner'])
    clear = np.ones(B, dtype=bool)
    for b in range(B):
        c, sin = ref['hyp_cost'][b], np.maximum(ref['hyp_sin'][b], 1e-300)
        fin = np.flatnonzero(np.isfinite(c))
        if len(fin) < 2:
            continue
        h0, h1 = fin[np.argsort(c[fin], kind='stable')[:2]]
        clear[b] = c[h1] - c[h0] > HYP_COST_SCALED_BOUND * ((c[h0] + 1.0) / sin[h0] + (c[h1] + 1.0) / sin[h1])   # 1.0 > thr^2
    return clear


def winners_are_clear(ref):
    return bool(clear_winners(ref).all())


def no_point_at_the_threshold(ref):
    """No point of a hypothesis of the mirror, nor of a result, has its |s| within that plane's bound of thr: a plane that
    differs by HYP_PLANE_SCALED_BOUND / sin in each of its four numbers moves s by at most (|x|_1 + 1) times that, and the
    cases' coordinates stay below 10 m."""
    fin = np.isfinite(ref['hyp_cost']) & (ref['hyp_sin'] > 0)
    hyp = (ref['near'][fin] > 31 * HYP_PLANE_SCALED_BOUND / ref['hyp_sin'][fin] / THR_FLOOR).all()
    return bool(hyp and (ref['near_final'] > 31 * RESULT_PLANE_BOUND / THR_FLOOR).all())

# ---- the cases ------------------------------------------------------------------------------------------------------------------
KEYPOINTS = ['Hip', 'RHip', 'LHip', 'Neck', 'Head', 'RBigToe', 'RSmallToe', 'RHeel', 'LBigToe', 'LSmallToe', 'LHeel']   # of HALPE_26
FEET = [KEYPOINTS.index(n) for n in ('LHeel', 'RHeel', 'LBigToe', 'RBigToe', 'LSmallToe', 'RSmallToe')]


def random_rotation(rng, tilt=None):
    """A rotation by `tilt` radians about a random axis (None: a uniformly random rotation)."""
    if tilt is None:
        Q = np.linalg.qr(rng.normal(size=(3, 3)))[0]
        return Q * np.sign(np.linalg.det(Q))
    k = rng.normal(size=3)
    k /= np.linalg.norm(k)
    Kx = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    return np.eye(3) + np.sin(tilt) * Kx + (1 - np.cos(tilt)) * Kx @ Kx


def path(u, straight):
    """The walk's line on the floor at arc parameter u (m along Y): (x, y) and the unit heading."""
    x, dx = (np.zeros_like(u), np.zeros_like(u)) if straight else (0.7 * np.sin(2 * np.pi * u / 3.0), 0.7 * 2 * np.pi / 3.0 * np.cos(2 * np.pi * u / 3.0))
    head = np.stack([dx, np.ones_like(u)], axis=-1)
    return np.stack([x, u], axis=-1), head / np.linalg.norm(head, axis=-1, keepdims=True)


def floor_case(F=240, seed=0, noise_m=0.01, p_outlier=0.05, straight=False, tilt=None, length=3.0, stride=1.2, stance=0.6, lift=0.12):
    """A walk of F frames over the floor Z = 0 of its own world (Y the direction of the walk, from -length / 2 to +length / 2),
    feet in stance (flat on the floor, a share `stance` of the cycle) and swing (lifted by up to `lift`), given in a frame
    that is rotated (by `tilt` rad about a random axis, None: any rotation) and shifted: dict with X [F][K][3] of KEYPOINTS in
    the given frame, 'world' the same without noise in the walk's world, the truth (A, b) with world = A x + b, 'up' and 'd'
    (the floor n . x = d in the given frame), and 'stance' [F][6] for the columns FEET."""
    rng = np.random.default_rng(seed)
    u = np.linspace(-length / 2, length / 2, F)
    W = np.zeros((F, len(KEYPOINTS), 3))
    c, head = path(u, straight)
    side = np.stack([head[:, 1], -head[:, 0]], axis=-1)                       # to the right of the heading
    for name, lateral, z in (('Hip', 0.0, 0.92), ('RHip', 0.1, 0.92), ('LHip', -0.1, 0.92), ('Neck', 0.0, 1.45), ('Head', 0.0, 1.7)):
        W[:, KEYPOINTS.index(name), :2] = c + lateral * side
        W[:, KEYPOINTS.index(name), 2] = z + 0.02 * np.sin(4 * np.pi * (u + length / 2) / stride)
    on_floor = np.zeros((F, 6), dtype=bool)
    for s, (prefix, lateral) in enumerate((('R', 0.1), ('L', -0.1))):
        cycle = (u + length / 2) / stride + 0.5 * s + 0.25
        k, phi = np.floor(cycle), cycle - np.floor(cycle)
        swing = np.clip((phi - stance) / (1 - stance), 0.0, 1.0)               # 0 during stance
        at = (k - 0.5 * s - 0.25 + swing) * stride - length / 2 + 0.3          # where the foot stands, or is on its way to
        fc, fh = path(at, straight)
        fs = np.stack([fh[:, 1], -fh[:, 0]], axis=-1)
        z = lift * np.sin(np.pi * swing)
        for name, ahead, out in (('Heel', -0.05, 0.0), ('BigToe', 0.17, -0.02), ('SmallToe', 0.14, 0.04)):
            j = KEYPOINTS.index(prefix + name)
            W[:, j, :2] = fc + ahead * fh + (lateral + out * np.sign(lateral)) * fs
            W[:, j, 2] = z * (1.0 if name == 'Heel' else 0.6)
            on_floor[:, FEET.index(j)] = swing == 0
    R0, t0 = random_rotation(rng, tilt), rng.uniform(-1.0, 1.0, 3) * (0.0 if tilt == 0 else 1.0)
    X = W @ R0.T + t0                                                          # x = R0 w + t0: w = R0^T x - R0^T t0
    if noise_m > 0:
        X = X + rng.normal(0.0, noise_m, X.shape)
        bad = rng.random(X.shape[:2]) < p_outlier
        X = X + bad[..., None] * rng.uniform(-0.8, 0.8, X.shape) / np.sqrt(3.0)
    up = R0[:, 2]
    return {'X': X, 'world': W, 'A': R0.T, 'b': -R0.T @ t0, 'up': up, 'd': float(up @ t0), 'stance': on_floor, 'names': list(KEYPOINTS)}


def inputs(cases, H=256, seed=0, thr=0.03):
    """What Engine.fit_planes takes for a list of floor_case walks, as calib_align_floor.floor_frames builds it: (points,
    usable, ref, samples, thr)."""
    from pose2sim_amd import calib_align_floor as caf
    ins = [caf.plane_inputs(c['X'], c['names']) for c in cases]
    B, N = len(ins), max(len(i[0]) for i in ins)
    points, usable, samples = np.zeros((B, N, 3)), np.zeros((B, N), dtype=bool), np.empty((B, H, 3), dtype=np.int32)
    for p, (pts, ok, _, _, _) in enumerate(ins):
        points[p, :len(pts)], usable[p, :len(pts)] = np.where(ok[:, None], pts, 0.0), ok
        samples[p] = caf.draw_triples(ok, H, seed)
    return points, usable, np.array([i[2] for i in ins]), samples, np.broadcast_to(np.asarray(thr, dtype=np.float64), (B,)).copy()


def random_problem(B, N, H, seed, thr=(0.03,), p_unusable=0.1, p_nan=0.03):
    """B problems of N points each near a tilted plane (two thirds on it with 1 cm noise, the rest up to 0.5 m above), with
    unusable points and NaN coordinates, a different share in every problem, and H samples of any three different points (so
    some name points that do not count): (points, usable, ref, samples, thr)."""
    rng = np.random.default_rng(seed)
    points, usable = np.empty((B, N, 3)), np.ones((B, N), dtype=bool)
    ref, samples = np.empty((B, 3)), np.empty((B, H, 3), dtype=np.int32)
    for b in range(B):
        R0, t0 = random_rotation(rng), rng.uniform(-1, 1, 3)
        w = np.stack([rng.uniform(-1.5, 1.5, N), rng.uniform(-1.5, 1.5, N), np.where(rng.random(N) < 0.67, rng.normal(0, 0.01, N), rng.uniform(0, 0.5, N))], axis=1)
        points[b] = w @ R0.T + t0
        ref[b] = R0 @ np.array([0.0, 0.0, 0.9]) + t0
        if N > 3:
            usable[b] = rng.random(N) >= p_unusable * (b + 1)
            points[b][rng.random(N) < p_nan * (b + 1), rng.integers(0, 3)] = np.nan
        samples[b] = np.argsort(rng.random((H, N)), axis=1)[:, :3] if N >= 3 else 0
    return points, usable, ref, samples, np.resize(np.asarray(thr, dtype=np.float64), B)


def zero_noise_case(N, seed):
    """Zero noise: N points, the first two thirds on the plane z = 0.25 of their own world, the others 0.125 m and more above
    it, all given in a rotated and shifted frame, where they lie on the plane to rounding.  -> (points [1][N][3], ref [1][3],
    truth plane [4], inliers [N] bool, the hips' trajectory [F][3] along the world's Y, truth (A, b) of frame_of_plane)."""
    rng = np.random.default_rng(seed)
    on = np.arange(N) < max(3, 2 * N // 3)
    w = np.stack([rng.uniform(-1.5, 1.5, N), np.linspace(-1.5, 1.5, N), np.where(on, 0.25, 0.375 + rng.uniform(0, 0.4, N))], axis=1)
    R0, t0 = random_rotation(rng), rng.uniform(-1, 1, 3)
    traj = np.stack([np.zeros(9), np.linspace(-1.0, 1.0, 9), np.full(9, 1.25)], axis=1)
    up, heading = R0[:, 2], R0[:, 1]
    plane = np.append(up, up @ t0 + 0.25)
    A = np.stack([np.cross(heading, up), heading, up])
    origin = (np.append(w[on, :2].mean(axis=0), 0.25)) @ R0.T + t0
    return (w @ R0.T + t0)[None], (np.array([0.0, 0.0, 1.25]) @ R0.T + t0)[None], plane, on, traj @ R0.T + t0, (A, -A @ origin)


# ---- the cases of both test files, each with the mirror's answer, built once --------------------------------------------------
# (B, N, H, seed): N = one sample, a wave less one, a wave, one past it, one past a tile, several chunks; H likewise
HYP_CASES = [(1, 3, 1, 0), (1, 63, 63, 1), (1, 64, 64, 2), (3, 65, 65, 3), (1, 257, 257, 4), (3, 700, 257, 5), (3, 257, 64, 6)]
THRS = (0.03, 0.02, 0.05)
# (frames, seed, straight): walks of floor_case, 6 foot points a frame
WALK_CASES = [(43, 0, False), (120, 1, True), (240, 2, False)]
ZERO_NOISE_N = (8, 255, 256, 257, 32769)


@functools.lru_cache(maxsize=None)
def hyp_case(B, N, H, seed):
    inp = random_problem(B, N, H, seed, THRS)
    return inp, fit_planes(*inp)


@functools.lru_cache(maxsize=None)
def walk_case(F, seed, straight, H=256):
    case = floor_case(F, seed, straight=straight)
    inp = inputs([case], H=H, seed=seed)
    return case, inp, fit_planes(*inp)


@functools.lru_cache(maxsize=None)
def walks_batch():
    """The three walks as the problems of one call, with a thr each."""
    cases = [floor_case(F, seed, straight=straight) for F, seed, straight in WALK_CASES]
    inp = inputs(cases, H=256, seed=7, thr=THRS)
    return cases, inp, fit_planes(*inp)


def same_bytes(a, b):
    return sorted(a) == sorted(b) and all(a[k].dtype == b[k].dtype and a[k].tobytes() == b[k].tobytes() for k in a)


def compare_hypotheses(got, ref, inp, label):
    """Every hypothesis of the library against the mirror's, none excluded -> the figures measured."""
    points, usable, _, _, thr = inp
    ok = counts(points, usable)
    assert np.array_equal(np.isnan(got['hyp_plane']), np.isnan(ref['hyp_plane'])), label
    assert np.array_equal(np.isinf(got['hyp_cost']), np.isinf(ref['hyp_cost'])) and not np.isnan(got['hyp_cost']).any(), label
    fin = np.isfinite(ref['hyp_cost'])
    sin = ref['hyp_sin'][fin]
    dp = float((np.abs(got['hyp_plane'][fin] - ref['hyp_plane'][fin]).max(axis=-1, initial=0.0) * sin).max(initial=0.0))
    # relative to cost + thr^2: the three points of the sample itself have an s of pure rounding, and where nothing else is
    # scored (N = 3) so is the whole cost
    floor = (thr * thr)[:, None]
    dc = float((np.abs(got['hyp_cost'][fin] - ref['hyp_cost'][fin]) / (ref['hyp_cost'] + floor)[fin] * sin).max(initial=0.0))
    own = 0.0
    for b, h in zip(*np.nonzero(fin)):
        cost = score(got['hyp_plane'][b, h], points[b][ok[b]], thr[b])[0]
        own = max(own, abs(got['hyp_cost'][b, h] - cost) / (cost + thr[b] ** 2))
    print(f'{label}: hypotheses |plane - mirror| x sin {dp:.3e}, |cost - mirror| / cost x sin {dc:.3e}, scoring alone {own:.3e}; smallest sin {sin.min(initial=1.0):.2e}')
    assert np.array_equal(got['hyp_inliers'], ref['hyp_inliers']), label
    assert dp <= HYP_PLANE_SCALED_BOUND and dc <= HYP_COST_SCALED_BOUND and own <= COST_REL_BOUND, label
    return dp, dc, own


def compare_results(got, ref, label):
    """The results of the library against the mirror's -> the figures measured."""
    for k in ('winner', 'refits', 'inliers', 'below', 'mask'):
        assert np.array_equal(got[k], ref[k]), (label, k, got[k], ref[k])
    has = ref['winner'] >= 0
    for k in ('plane', 'cost', 'centroid', 'evals'):
        assert np.array_equal(np.isnan(got[k]), np.isnan(ref[k])) and np.isnan(ref[k][~has]).all(), (label, k)
    dp = float(np.abs(got['plane'][has] - ref['plane'][has]).max(initial=0.0))
    dc = float((np.abs(got['cost'][has] - ref['cost'][has]) / (ref['cost'][has] + THR_FLOOR ** 2)).max(initial=0.0))
    dm = float(np.abs(got['centroid'][has] - ref['centroid'][has]).max(initial=0.0))
    de = float((np.abs(got['evals'][has] - ref['evals'][has]) / ref['evals'][has][:, 2:]).max(initial=0.0))
    print(f'{label}: results |plane - mirror| {dp:.3e}, |cost - mirror| / cost {dc:.3e}, centroid {dm:.3e} m, evals {de:.3e} of the largest')
    assert dp <= RESULT_PLANE_BOUND and dc <= RESULT_COST_REL_BOUND and dm <= RESULT_CENTROID_BOUND and de <= RESULT_EVALS_REL_BOUND, label
    return dp, dc, dm, de


def structure_case():
    """Two problems by hand, on integer coordinates so that every figure is exact: the 8 points of a 3 x 3 grid on the floor z
    = 0 without its centre, two points above, an unusable point and one with a NaN, and a sample of every kind that is refused;
    ref stands over (0, 0).  Problem 1 has the same points and two of them usable.  -> (inputs, what each sample is)."""
    floor = [(x, y, 0.0) for x in (0.0, 1.0, 2.0) for y in (0.0, 1.0, 2.0) if (x, y) != (1.0, 1.0)]          # 0 .. 7
    pts = np.array(floor + [(0.0, 0.0, 2.0), (1.0, 1.0, 0.0), (2.0, 2.0, 0.0), (1.0, 2.0, 1.0)])             # 8: above; 9: unusable; 10: NaN; 11: above
    pts[10, 1] = np.nan
    usable = np.ones((2, 12), dtype=bool)
    usable[0, 9] = False
    usable[1, 2:] = False
    kinds = [('repeated index', (0, 0, 1)), ('index past the last', (0, 1, 12)), ('negative index', (-1, 0, 1)), ('unusable point', (0, 1, 9)),
             ('NaN point', (0, 2, 10)), ('first of two equal', (0, 2, 5)), ('second of two equal', (5, 0, 2)), ('collinear', (0, 1, 2)),
             ('ref in the plane', (0, 3, 8)), ('through a point above', (0, 1, 11)), ('third equal', (7, 5, 2))]
    samples = np.array([[k[1] for k in kinds]] * 2, dtype=np.int32)
    ref = np.array([[0.0, 0.0, 1.0], [0.0, 0.0, 1.0]])                  # the points 0, 3 and 8 span the plane y = 0, which holds ref
    return (np.stack([pts, pts]), usable, ref, samples, np.array([0.25, 0.25])), [k[0] for k in kinds]


def check_structure(fit):
    inp, kinds = structure_case()
    ref = fit_planes(*inp)
    got = fit(*inp, all_hypotheses=True)
    refused = [i for i, k in enumerate(kinds) if k in ('repeated index', 'index past the last', 'negative index', 'unusable point', 'NaN point',
                                                       'collinear', 'ref in the plane')]
    for res in (ref, got):
        assert np.isnan(res['hyp_plane'][0, refused]).all() and np.isinf(res['hyp_cost'][0, refused]).all() and not res['hyp_inliers'][0, refused].any()
        first, second, third = kinds.index('first of two equal'), kinds.index('second of two equal'), kinds.index('third equal')
        assert res['hyp_cost'][0, first] == res['hyp_cost'][0, second] == res['hyp_cost'][0, third] == 2 * 0.25 ** 2   # the two points above
        assert res['winner'][0] == first and res['inliers'][0] == 8 and res['below'][0] == 0
        assert np.array_equal(res['plane'][0], [0.0, 0.0, 1.0, 0.0]) and res['mask'][0].tolist() == [True] * 8 + [False] * 3 + [False]
        # two counting points: no error, nothing found; every sample of it names a point that does not count, or too few
        assert res['winner'][1] == -1 and np.isnan(res['plane'][1]).all() and np.isnan(res['cost'][1]) and np.isnan(res['centroid'][1]).all()
        assert np.isnan(res['evals'][1]).all() and res['inliers'][1] == res['below'][1] == res['refits'][1] == 0 and not res['mask'][1].any()
        assert np.isinf(res['hyp_cost'][1]).all() and np.isnan(res['hyp_plane'][1]).all()
    assert np.array_equal(got['hyp_inliers'], ref['hyp_inliers'])
    assert np.array_equal(got['hyp_plane'], ref['hyp_plane'], equal_nan=True) and np.array_equal(got['hyp_cost'], ref['hyp_cost'])   # exact on integers
    compare_results(got, ref, 'structure')


def check_refusals(fit, error):
    """Each invalid argument is refused with its message (argument checks only)."""
    import pytest
    (points, usable, ref, samples, thr), _ = hyp_case(3, 65, 65, 3)
    with pytest.raises(error, match='n_problems=0'):
        fit(points[:0], usable[:0], ref[:0], samples[:0], thr[:0])
    with pytest.raises(error, match='n_points=0'):
        fit(points[:, :0], usable[:, :0], ref, samples, thr)
    with pytest.raises(error, match='n_hyp=0'):
        fit(points, usable, ref, samples[:, :0], thr)
    with pytest.raises(error, match='rounds=-1 is negative'):
        fit(points, usable, ref, samples, thr, rounds=-1)
    for bad in (0.0, -0.03, np.inf, np.nan):
        with pytest.raises(error, match='thr of problem 1 must be positive and finite'):
            fit(points, usable, ref, samples, [0.03, bad, 0.03])
    for bad in (np.nan, np.inf):
        r = ref.copy()
        r[2, 1] = bad
        with pytest.raises(error, match='ref of problem 2 is not finite'):
            fit(points, usable, r, samples, thr)


def check_zero_noise(fit, N):
    """Points exactly on and above a known plane: the normal, the offset and the assembled frame against the truth; the same of
    the mirror, whose error sets the bound -> (the library's figures, the mirror's)."""
    from pose2sim_amd import calib_align_floor as caf
    points, ref, plane, on, traj, (A, b) = zero_noise_case(N, seed=N)
    samples = caf.draw_triples(on | ~on, 64, seed=N)[None]
    out = []
    for name, res in (('library', fit(points, on[None] | True, ref, samples, 0.03)), ('mirror', fit_planes(points, on[None] | True, ref, samples, 0.03))):
        assert res['winner'][0] >= 0 and res['inliers'][0] == on.sum() and res['below'][0] == 0 and np.array_equal(res['mask'][0], on), name
        Ag, bg = caf.frame_of_plane(res['plane'][0], res['centroid'][0], traj)
        fig = (float(np.abs(res['plane'][0, :3] - plane[:3]).max()), float(abs(res['plane'][0, 3] - plane[3])), float(max(np.abs(Ag - A).max(), np.abs(bg - b).max())))
        print(f'zero noise, N = {N}, {name}: normal {fig[0]:.3e}, offset {fig[1]:.3e} m, frame {fig[2]:.3e} from the truth')
        out.append(fig)
    assert out[0][0] <= ZERO_NOISE_NORMAL and out[0][1] <= ZERO_NOISE_OFFSET and out[0][2] <= ZERO_NOISE_FRAME
    return out


# ---- end to end: a rig whose world is off the floor ---------------------------------------------------------------------------
def observed(cams, X):
    """X [F][K][3] in the world of `cams` -> xyl [F][C][K][3], likelihood 1 (pinhole rigs)."""
    from pose2sim_amd import cvmath
    F, K = X.shape[:2]
    xyl = np.ones((F, len(cams['K']), K, 3))
    for c in range(len(cams['K'])):
        xyl[:, c, :, :2] = cvmath.project_points(X.reshape(-1, 3), np.asarray(cams['R_mat'][c]), np.asarray(cams['T'][c]), np.asarray(cams['K'][c]),
                                                 cams['dist'][c]).reshape(F, K, 2)
    return xyl


@functools.lru_cache(maxsize=None)
def rig_case(seed=4, F=240):
    """rigs.make_rig('ring', 4) with its world rotated by 0.4 rad and shifted off the floor, and a floor_case walk (1 cm noise and
    outliers in 3D) seen by its cameras: (the calibration off the floor, xyl of the noisy walk, xyl of the walk without noise, the
    walk, with 'up_off': the true up in the world off the floor)."""
    import rigs
    from pose2sim_amd import calib_align_floor as caf
    rng = np.random.default_rng(seed)
    rig = rigs.make_rig('ring', 4, seed)
    walk = floor_case(F, seed, tilt=0)                                          # in the rig's own world: Z up, the floor Z = 0
    A0 = random_rotation(rng, 0.4)
    off = caf.moved_cameras(rig, A0, rng.uniform(-1.0, 1.0, 3))
    walk['up_off'] = A0[:, 2]                                                   # the true up in the world that is off the floor
    return off, observed(rig, walk['X']), observed(rig, walk['world']), walk


def check_frame(case, A, b, threshold=0.03):
    """(A, b) is rigid and puts the walk's noise-free stance feet within the threshold of Z = 0, the hips above and the walk
    along +Y: Y within 2 degrees of the principal axis of the noise-free hips on the true floor (the noise of the case, 1 cm
    and 5 % outliers on three hip keypoints over 43 frames and more, turns that axis by a few tenths of a degree), X = Y x Z."""
    given = (case['world'] - case['b']) @ case['A']                               # world = A_true x + b_true
    new = given @ A.T + b
    assert abs(np.linalg.det(A) - 1) < 1e-12 and np.abs(A @ A.T - np.eye(3)).max() < 1e-12
    assert np.abs(np.cross(A[1], A[2]) - A[0]).max() < 1e-12
    assert np.abs(new[:, FEET][case['stance']][:, 2]).max() < threshold and new[:, :3, 2].min() > 0.8
    hips = case['world'][:, 0, :2] - case['world'][:, 0, :2].mean(axis=0)
    axis = np.linalg.eigh(hips.T @ hips)[1][:, -1]
    axis = np.append(axis * np.sign(axis[1]), 0.0) @ case['A']                    # in the given frame
    angle = np.degrees(np.arccos(min(1.0, float(axis @ A[1]))))
    print(f'heading {angle:.3f} degrees from the principal axis of the true hips, walk of {new[-1, 0, 1] - new[0, 0, 1]:.2f} m along +Y')
    assert angle < 2.0 and new[-1, 0, 1] - new[0, 0, 1] > 2.5
