"""NumPy restatement of Engine.relative_poses (include/p2s.h): the live reference of
tests/test_relpose_gpu.py and tests/test_relpose_host.py, the builder of their cases and the holder of their bounds.  Test
infrastructure, not a fallback: the package never imports it.

The contract is restated with np.linalg.eigh and np.linalg.svd: nothing here shares an eigen-solver, a decomposition or a
summation order with the kernels.  The host-side assembly of the pair poses (calib_from_keypoints.assemble) has no second
implementation: `cameras` runs it on this mirror's pair poses and the tests hold the result against the true cameras after
the similarity alignment `align`."""
import numpy as np

import rigs
from pose2sim_amd import calib_from_keypoints as cfk
from pose2sim_amd import cvmath, synth

# The bounds of the tests: 100 x the worst figure of its kind measured on the MI355X over the cases of
# tests/test_relpose_gpu.py (DESIGN.md 4.22 lists them), the device against this mirror, under the caps the feature was
# specified with (1e-9 relative on costs, 1e-9 on the pairs' E).  The library's host path stays inside the same figures.
#
# A hypothesis' E is an eigenvector of A^T A, and eigh here as the Jacobi sweeps there deliver it to eps x lambda_max /
# lambda_2, no better: of 8 correspondences the ratio lambda_2 / lambda_max is below 1e-3 in 70 % of the samples of these rigs
# and reaches 1e-9.  Its cost follows E with a factor of about 2 / sqrt(thr2) (d is the square of a residual of the size of the
# threshold).  So every hypothesis is compared, with its difference weighted by the mirror's own lambda_2 / lambda_max; the
# scoring itself is held to the cap by letting the mirror score the library's E.
COND_FLOOR = 1e-10          # hypotheses of a lambda_2 / lambda_max below it are not compared (E, cost): none in the cases so far
COND_SHARE = 0.02           # ... and may be at most this share of a case
HYP_E_SCALED_BOUND = 1.1e-13     # max |E - E_mirror| x lambda_2 / lambda_max (sign matched); worst measured 1.06e-15 (32 cameras)
HYP_COST_SCALED_BOUND = 6.2e-12  # |cost - cost_mirror| / cost_mirror x lambda_2 / lambda_max, each side its own E; worst measured 6.15e-14
COST_REL_BOUND = 2.6e-12    # |cost - mirror's cost of the library's E| / cost of a hypothesis (the scoring kernel alone); worst measured 2.58e-14
RESULT_COST_REL_BOUND = 1e-9  # |cost - cost_mirror| / cost_mirror of a pair's result: the cap; 100 x the worst measured, 9.9e-11 (32 cameras), is above it
RESULT_COND_FLOOR = 1e-4    # a pair's result that is a hypothesis as it stands (no refit kept) of a lambda_2 / lambda_max below this is
                            # held to the hypotheses' weighted bounds, not to the caps: 100 x 6e-14 / 1e-4 is the cap on costs
WIN_E_BOUND = 4.5e-10       # max |E - E_mirror|, |R - R_mirror|, |t - t_mirror| of every other result; worst measured 3.2e-12, 4.5e-12, 1.8e-12
RT_BOUND = WIN_E_BOUND
RT_SCALED_BOUND = 6.1e-14   # |R - R_mirror|, |t - t_mirror| x lambda_2 / lambda_max of the former; worst measured 6.1e-16
ZERO_NOISE_R = 2.9e-13      # ||R - R_true||_F of the assembled cameras at zero noise; worst measured 2.9e-15
ZERO_NOISE_C = 2.2e-12      # m, their centres against the truth; worst measured 2.13e-14
assert max(COST_REL_BOUND, RESULT_COST_REL_BOUND, WIN_E_BOUND, RT_BOUND, ZERO_NOISE_R, ZERO_NOISE_C) <= 1e-9


def clear_winners(ref):
    """[P] bool: the mirror's two best costs of the pair differ by more than the bounds of both, so that no other winner lies
    within them; and [P][2] the two best hypotheses."""
    P = len(ref['winner'])
    clear, best = np.ones(P, dtype=bool), np.full((P, 2), -1)
    for p in range(P):
        c, cond = ref['hyp_cost'][p], np.maximum(ref['hyp_cond'][p], 1e-300)
        fin = np.flatnonzero(np.isfinite(c))
        if len(fin) < 2:
            continue
        h0, h1 = best[p] = fin[np.argsort(c[fin], kind='stable')[:2]]
        clear[p] = c[h1] - c[h0] > HYP_COST_SCALED_BOUND * (c[h0] / cond[h0] + c[h1] / cond[h1])
    return clear, best


def winners_are_clear(ref):
    return bool(clear_winners(ref)[0].all())


def no_point_at_the_threshold(ref):
    """No scored point of a hypothesis of the mirror has its d within that hypothesis' cost bound of thr2."""
    fin = np.isfinite(ref['hyp_cost']) & (ref['hyp_cond'] > 0)
    return bool((ref['near'][fin] > HYP_COST_SCALED_BOUND / ref['hyp_cond'][fin]).all())


def counts(xn, usable):
    xn = np.asarray(xn, dtype=np.float64)
    return np.asarray(usable, dtype=bool) & np.isfinite(xn).all(axis=-1)


def normalisation(x):
    """(s, c): x' = s (x - c) has its centroid at 0 and an RMS distance of sqrt 2."""
    c = x.mean(axis=0)
    return np.sqrt(2.0 / np.mean(np.sum((x - c) ** 2, axis=1))), c


def solve(xa, xb, sa, ca, sb, cb):
    """E from correspondences under given normalisations; -> (E, lambda_2 / lambda_max of A^T A)."""
    a, b = sa * (xa - ca), sb * (xb - cb)
    ah, bh = np.concatenate([a, np.ones((len(a), 1))], axis=1), np.concatenate([b, np.ones((len(b), 1))], axis=1)
    A = (bh[:, :, None] * ah[:, None, :]).reshape(-1, 9)
    lam, vec = np.linalg.eigh(A.T @ A)
    Fn = vec[:, 0].reshape(3, 3)
    Ta = np.array([[sa, 0, -sa * ca[0]], [0, sa, -sa * ca[1]], [0, 0, 1.0]])
    Tb = np.array([[sb, 0, -sb * cb[0]], [0, sb, -sb * cb[1]], [0, 0, 1.0]])
    F = Tb.T @ Fn @ Ta
    if not np.isfinite(F).all():
        return np.full((3, 3), np.nan), 0.0
    U, s, Vt = np.linalg.svd(F)
    if not s[1] > 0:
        return np.full((3, 3), np.nan), 0.0
    return U @ np.diag([1.0, 1.0, 0.0]) @ Vt, lam[1] / lam[-1]


def hypothesis(xa, xb):
    with np.errstate(all='ignore'):
        return solve(xa, xb, *normalisation(xa), *normalisation(xb))


def sampson(E, xa, xb):
    ah, bh = np.concatenate([xa, np.ones((len(xa), 1))], axis=1), np.concatenate([xb, np.ones((len(xb), 1))], axis=1)
    Ea, Eb = ah @ E.T, bh @ E
    with np.errstate(all='ignore'):
        return np.sum(bh * Ea, axis=1) ** 2 / (Ea[:, 0] ** 2 + Ea[:, 1] ** 2 + Eb[:, 0] ** 2 + Eb[:, 1] ** 2)


def score(E, xa, xb, thr2):
    """(cost, inliers, d) of the contract; +inf and 0 for an E that is not finite."""
    d = sampson(E, xa, xb)
    if not np.isfinite(E).all():
        return np.inf, 0, d
    with np.errstate(invalid='ignore'):
        return float(np.sum(np.where(d < thr2, d, np.where(d >= thr2, thr2, 0.0)))), int(np.sum(d < thr2)), d


def decompose(E):
    """The four (R, t) of E in the contract's order."""
    U, _, Vt = np.linalg.svd(E)
    if np.linalg.det(U) < 0:
        U[:, 2] *= -1
    if np.linalg.det(Vt) < 0:
        Vt[2] *= -1
    W = np.array([[0.0, -1, 0], [1, 0, 0], [0, 0, 1]])
    Ra, Rb, t = U @ W @ Vt, U @ W.T @ Vt, U[:, 2] / np.linalg.norm(U[:, 2])
    if t[np.argmax(np.abs(t))] < 0:
        t = -t
    if np.trace(Rb) > np.trace(Ra):
        Ra, Rb = Rb, Ra
    return [(Ra, t), (Ra, -t), (Rb, t), (Rb, -t)]


def in_front(R, t, xa, xb):
    ah, bh = np.concatenate([xa, np.ones((len(xa), 1))], axis=1), np.concatenate([xb, np.ones((len(xb), 1))], axis=1)
    r = ah @ R.T
    c, d = np.cross(bh, r), np.cross(bh, t[None, :])
    with np.errstate(all='ignore'):
        za = -np.sum(c * d, axis=1) / np.sum(c * c, axis=1)
    return (za > 0) & (za * r[:, 2] + t[2] > 0)


def relative_poses(xn, usable, pairs, samples, thr2, rounds=3, score_points=0):
    """The contract, pair after pair.  Besides the library's outputs: hyp_cond [P][H] (lambda_2 / lambda_max, 0 for a refused
    sample), margin [P] (second best cost - best), near [P][H] and near_final [P]: the smallest |d - thr2| / thr2 over the
    scored points, front_all [P][4]."""
    xn = np.asarray(xn, dtype=np.float64)
    ok = counts(xn, usable)
    pairs, samples = np.asarray(pairs).reshape(-1, 2), np.asarray(samples)
    P, H, m = samples.shape
    N = xn.shape[1]
    thr2 = np.broadcast_to(np.asarray(thr2, dtype=np.float64), (P,))
    most = max(int((ok[a] & ok[b]).sum()) for a, b in pairs)
    S = score_points if 0 < score_points < most else 0
    out = {'E': np.full((P, 3, 3), np.nan), 'R': np.full((P, 3, 3), np.nan), 't': np.full((P, 3), np.nan), 'cost': np.full(P, np.nan),
           'inliers': np.zeros(P, dtype=np.int32), 'front': np.zeros(P, dtype=np.int32), 'winner': np.full(P, -1, dtype=np.int32),
           'refits': np.zeros(P, dtype=np.int32), 'mask': np.zeros((P, N), dtype=bool), 'hyp_E': np.full((P, H, 3, 3), np.nan),
           'hyp_cost': np.full((P, H), np.inf), 'hyp_inliers': np.zeros((P, H), dtype=np.int32), 'hyp_cond': np.zeros((P, H)),
           'margin': np.full(P, np.inf), 'near': np.full((P, H), np.inf), 'near_final': np.full(P, np.inf),
           'front_all': np.zeros((P, 4), dtype=np.int32)}
    for p, (a, b) in enumerate(pairs):
        both = ok[a] & ok[b]
        idx = np.flatnonzero(both)
        k = len(idx)
        sc = idx if not S or k <= S else idx[(np.arange(S) * k) // S]
        xa, xb = xn[a][sc], xn[b][sc]
        for h in range(H):
            smp = samples[p, h]
            if len(set(smp.tolist())) < m or (smp < 0).any() or (smp >= N).any() or not both[smp].all():
                continue
            E, cond = hypothesis(xn[a][smp], xn[b][smp])
            out['hyp_E'][p, h], out['hyp_cond'][p, h] = E, cond
            cost, inl, d = score(E, xa, xb, thr2[p])
            out['hyp_cost'][p, h], out['hyp_inliers'][p, h] = cost, inl
            if len(d) and np.isfinite(E).all():
                out['near'][p, h] = np.nanmin(np.abs(d - thr2[p])) / thr2[p]
        w = int(np.argmin(out['hyp_cost'][p]))
        if k < m or not np.isfinite(out['hyp_cost'][p, w]):
            continue
        out['winner'][p] = w
        if H > 1:
            out['margin'][p] = np.partition(out['hyp_cost'][p], 1)[1] - out['hyp_cost'][p, w]
        E = out['hyp_E'][p, w]
        xa, xb = xn[a][idx], xn[b][idx]
        cost, inl, d = score(E, xa, xb, thr2[p])
        for _ in range(rounds):
            if inl < 8:
                break
            i = d < thr2[p]
            n = i.sum()
            ca, cb = xa[i].sum(axis=0) / n, xb[i].sum(axis=0) / n
            va, vb = (xa[i] ** 2).sum() / n - ca @ ca, (xb[i] ** 2).sum() / n - cb @ cb
            if not (va > 0 and vb > 0):
                break
            Et, _ = solve(xa[i], xb[i], np.sqrt(2.0 / va), ca, np.sqrt(2.0 / vb), cb)
            ct, it, dt = score(Et, xa, xb, thr2[p])
            if not ct < cost:
                break
            E, cost, inl, d = Et, ct, it, dt
            out['refits'][p] += 1
        out['E'][p], out['cost'][p], out['inliers'][p] = E, cost, inl
        out['near_final'][p] = np.nanmin(np.abs(d - thr2[p])) / thr2[p]
        i = d < thr2[p]
        out['mask'][p, idx[i]] = True
        cand = decompose(E)
        out['front_all'][p] = [int(in_front(R, t, xa[i], xb[i]).sum()) for R, t in cand]
        best = int(np.argmax(out['front_all'][p]))
        out['R'][p], out['t'][p], out['front'][p] = cand[best][0], cand[best][1], out['front_all'][p, best]
    return out


def match_sign(E, Eref):
    """E or -E, whichever is nearer Eref (per matrix of a stack)."""
    s = np.sign(np.sum(E * Eref, axis=(-2, -1), keepdims=True))
    return np.where(s < 0, -E, E)


def cameras(C, xn, pairs, res, min_inliers=30):
    """The assembled world cameras (R [C][3][3], T [C][3]) of pair results."""
    return cfk.assemble(C, xn, pairs, res['R'], res['t'], res['inliers'], res['mask'], min_inliers)[:2]


def align(R, T, Rt, Tt):
    """The cameras (R, T) in the true cameras' world: the similarity that takes camera 0 to the true camera 0 and the mean
    distance of the centres from camera 0 to the true one.  -> (R [C][3][3], centres [C][3], true centres)."""
    R, T, Rt, Tt = (np.asarray(v, dtype=np.float64) for v in (R, T, Rt, Tt))
    c, ct = -np.einsum('cji,cj->ci', R, T), -np.einsum('cji,cj->ci', Rt, Tt)
    Q = Rt[0].T @ R[0]                                            # world -> true world
    s = np.linalg.norm(ct[1:] - ct[0], axis=1).mean() / np.linalg.norm(c[1:] - c[0], axis=1).mean()
    return R @ Q.T, ct[0] + s * (c - c[0]) @ Q.T, ct


def pair_truth(R, T, pairs):
    """The exact pair poses X_b = R X_a + t (|t| = 1) of world cameras."""
    Rp, tp = [], []
    for a, b in pairs:
        Rab = R[b] @ R[a].T
        tab = T[b] - Rab @ T[a]
        Rp.append(Rab)
        tp.append(tab / np.linalg.norm(tab))
    return np.array(Rp), np.array(tp)


def walk_case(family='ring', C=4, F=20, Kp=13, seed=0, noise_px=0.5, p_outlier=0.05, outlier_px=80.0, lik=(0.1, 1.0), distortion='none'):
    """A person who stands somewhere else in the 3 x 3 m area in every frame: dict with xyl [F][C][Kp][3], the rig `cams` and
    its true K, R, t.  Noise, outliers and likelihoods as in refine_scipy.make_case; noise_px == 0: likelihood 1, no outliers."""
    cams = rigs.make_rig(family, C, seed, distortion)
    scale, offset = rigs.scene(family)
    Q = synth.make_points3d(F, 1, Kp, seed=seed)[:, 0]                                     # [F][Kp][3]
    rng = np.random.default_rng(seed + 2718)
    Q[..., :2] += (rng.uniform(-1.5, 1.5, (F, 2)) - Q[..., :2].mean(axis=1))[:, None, :]    # the frame's root somewhere else
    Q = Q * scale + offset
    K = np.array(cams['K'], dtype=np.float64)
    R = np.array(cams['R_mat'], dtype=np.float64)
    t = np.array(cams['T'], dtype=np.float64)
    xyl = np.empty((F, C, Kp, 3))
    for c in range(C):
        uv = cvmath.project_points(Q.reshape(-1, 3), R[c], t[c], K[c], cams['dist'][c]).reshape(F, Kp, 2)
        if noise_px > 0:
            uv = uv + rng.normal(0.0, 1.0, uv.shape) * noise_px
            out = rng.random((F, Kp)) < p_outlier
            ang, mag = rng.uniform(0, 2 * np.pi, (F, Kp)), rng.uniform(0.0, outlier_px, (F, Kp))
            uv = uv + out[..., None] * np.stack([mag * np.cos(ang), mag * np.sin(ang)], axis=-1)
        xyl[:, c, :, :2] = uv
        xyl[:, c, :, 2] = 1.0 if (lik is None or noise_px == 0) else rng.uniform(lik[0], lik[1], (F, Kp))
    return {'xyl': xyl, 'cams': cams, 'K': K, 'R': R, 't': t, 'Q': Q.reshape(-1, 3)}


def inputs(case, H=512, m=8, seed=0, thr_px=4.0, lik_thr=0.3):
    """What Engine.relative_poses takes for a walk_case: (xn, usable, pairs, samples, thr2), as initial_extrinsics builds it."""
    cams = case['cams']
    C = len(cams['K'])
    xn, usable = cfk.normalised(cams, case['xyl'], lik_thr)
    pairs = cfk.all_pairs(C)
    f = np.array([[cams['K'][c][0][0], cams['K'][c][1][1]] for c in range(C)])
    thr2 = np.array([(thr_px / np.mean([f[a], f[b]])) ** 2 for a, b in pairs])
    return xn, usable, pairs, cfk.draw_samples(usable, pairs, H, m, seed), thr2
