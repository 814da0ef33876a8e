"""Extrinsics from scratch: the cameras' rotations and translations from the 2D keypoints of a person who walks through
the volume, given the intrinsics alone.

The reference names this (`extrinsics_method = 'keypoints'`) and answers it with NotImplementedError
(calibration.py:969-971, :998-999).  calib_refine repairs a calibration that is nearly right; this module needs none.
Every camera pair gets a relative pose by hypothesise and score (Engine.relative_poses, csrc/p2s_relpose.hip, DESIGN.md
4.22: normalised 8-point hypotheses, MSAC on the Sampson distance, refits on the inliers, cheirality), the pairs are
assembled along a maximum spanning tree of their inlier counts, and the result starts calib_refine's bundle adjustment.

What the data must be: ONE person who MOVES THROUGH the volume.  A person who stays within a few decimetres gives a point
cloud that is flat as seen from 5 m, the two-view geometry is then close to weak perspective, and no pair is recovered.
The world frame of the result is camera 0's (R = I, t = 0); with floor = True (--floor) it is put on the floor the person walks
on instead, Z up and Y along the walk (calib_align_floor), which needs a scale in metres and is refused without one.  The scale comes from
a known baseline, from the person's height, or is arbitrary (first baseline = 1).  cv2.findEssentialMat has never run next to this
code and nothing here is pinned to it.

    python -m pose2sim_amd.calib_from_keypoints -c Intrinsics.toml -p pose [-o Calib.toml] [--baseline cam01 cam02 2.5 |
                                                --height 1.75] [--floor [--floor-threshold 0.03] [--floor-hypotheses 1024]] [--threshold 4] [--hypotheses 4096] [--sample-size 8] [--seed 0]
                                                [--likelihood 0.3] [--huber 3] [--keypoints Nose,Neck,...] [--pose-model HALPE_26]
"""
import argparse
import logging
import os

import numpy as np

from . import calib, calib_refine, cvmath

WIDE_START_THR = 300.0     # px: the reprojection threshold of the first refinement's start points (a 2 degree start is ~50 px)
MOVED_M, MOVED_RAD = 1e-6, 1e-7   # share of the first baseline / rotation beyond which the first refinement "moved the cameras"


def normalised(cams, xyl, lik_thr=0.3):
    """xyl [F..., C, K, 3] -> (xn [C][N][2] normalised pinhole coordinates, usable [C][N], N = frames x K in calib_refine's
    point order): lenses undone, K^-1 applied; usable where the observation is finite and its likelihood lik_thr or more."""
    xyl = calib_refine.undistorted(cams, xyl)
    C, Kn = xyl.shape[-3], xyl.shape[-2]
    o = np.moveaxis(xyl.reshape(-1, C, Kn, 3), 1, 0).reshape(C, -1, 3)
    with np.errstate(invalid='ignore'):
        usable = np.isfinite(o).all(axis=-1) & (o[..., 2] >= lik_thr) & (o[..., 2] > 0)
    xn = np.empty(o.shape[:2] + (2,))
    for c in range(C):
        Ki = np.linalg.inv(np.asarray(cams['K'][c], dtype=np.float64))
        h = np.nan_to_num(o[c, :, :2]) @ Ki[:, :2].T + Ki[:, 2]
        xn[c] = h[:, :2] / h[:, 2:]
    xn[~usable] = np.nan
    return xn, usable


def all_pairs(C):
    return np.array([(a, b) for a in range(C) for b in range(a + 1, C)], dtype=np.int32).reshape(-1, 2)


def draw_samples(usable, pairs, H, m, seed=0):
    """samples [P][H][m] int32: per pair H rows of m distinct indices of points usable in both cameras, from
    default_rng(seed); -1 throughout for a pair with fewer than m such points."""
    usable = np.asarray(usable, dtype=bool)
    rng = np.random.default_rng(seed)
    out = np.full((len(pairs), H, m), -1, dtype=np.int32)
    for p, (a, b) in enumerate(np.asarray(pairs)):
        idx = np.flatnonzero(usable[a] & usable[b])
        k = len(idx)
        if k < m:
            continue
        if k <= 4 * m * m:                                   # few points: the first m of a random order
            rows = np.argsort(rng.random((H, k)), axis=1)[:, :m]
        else:                                                # many: draw, and redraw the rows that repeat an index
            rows = rng.integers(0, k, (H, m))
            while True:
                s = np.sort(rows, axis=1)
                bad = np.flatnonzero((s[:, 1:] == s[:, :-1]).any(axis=1))
                if not len(bad):
                    break
                rows[bad] = rng.integers(0, k, (len(bad), m))
        out[p] = idx[rows]
    return out


def triangulate_pair(Ra, ta, Rb, tb, xa, xb):
    """Linear two-view triangulation of normalised correspondences [n][2] through X_c = R_c X + t_c: X [n][3]."""
    Pa, Pb = np.hstack([Ra, ta.reshape(3, 1)]), np.hstack([Rb, tb.reshape(3, 1)])
    A = np.stack([xa[:, 0, None] * Pa[2] - Pa[0], xa[:, 1, None] * Pa[2] - Pa[1], xb[:, 0, None] * Pb[2] - Pb[0],
                  xb[:, 1, None] * Pb[2] - Pb[1]], axis=1)
    q = np.linalg.svd(A)[2][:, -1]
    with np.errstate(divide='ignore', invalid='ignore'):
        return q[:, :3] / q[:, 3:]


def assemble(C, xn, pairs, R, t, inliers, mask, min_inliers=30, names=None):
    """World cameras from pair poses X_b = R X_a + t (|t| = 1): a maximum spanning tree over the pairs' inlier counts grown
    from camera 0, the world frame.  The first edge fixes the unit baseline; a later camera c, reached from the placed camera
    a, takes the scale s = median over the edge's inliers with a known point X of the least-squares solution of
    x_c x (R_c X + R_ac t_a + s t_ac) = 0; the edge's other inliers are triangulated once c is placed.
    -> (R [C][3][3], T [C][3], X [N][3] with NaN for points never triangulated, edges [(a, c, pair, scale, known)])."""
    pairs = np.asarray(pairs)
    names = names or [f'camera {c}' for c in range(C)]
    Rw, Tw = np.full((C, 3, 3), np.nan), np.full((C, 3), np.nan)
    Rw[0], Tw[0] = np.eye(3), 0.0
    X = np.full((xn.shape[1], 3), np.nan)
    placed, edges = {0}, []
    order = sorted(range(len(pairs)), key=lambda p: (-int(inliers[p]), p))
    while len(placed) < C:
        for p in order:
            a, b = (int(v) for v in pairs[p])
            if inliers[p] < min_inliers or (a in placed) == (b in placed) or not np.isfinite(R[p]).all():
                continue
            Rac, tac = (R[p], t[p]) if a in placed else (R[p].T, -R[p].T @ t[p])
            if b in placed:
                a, b = b, a                                  # a is placed, b is new: X_b = Rac X_a + s tac
            m = np.asarray(mask[p], dtype=bool)
            Rb = Rac @ Rw[a]
            if not edges:
                s, known = 1.0, 0
            else:
                k = m & np.isfinite(X[:, 0])
                known = int(k.sum())
                if known == 0:
                    continue                                 # nothing ties this edge's scale to what is placed
                xh = np.concatenate([xn[b][k], np.ones((known, 1))], axis=1)
                u = np.cross(xh, X[k] @ Rb.T + Rac @ Tw[a])
                v = np.cross(xh, tac[None, :])
                s = float(np.median(-(u * v).sum(axis=1) / (v * v).sum(axis=1)))
                if not s > 0:
                    continue
            Rw[b], Tw[b] = Rb, Rac @ Tw[a] + s * tac
            new = m & ~np.isfinite(X[:, 0])
            Xn = triangulate_pair(Rw[a], Tw[a], Rw[b], Tw[b], xn[a][new], xn[b][new])
            front = ((Xn @ Rw[a].T + Tw[a])[:, 2] > 0) & ((Xn @ Rw[b].T + Tw[b])[:, 2] > 0) & np.isfinite(Xn).all(axis=1)
            Xn[~front] = np.nan
            X[new] = Xn
            placed.add(b)
            edges.append((a, b, int(p), s, known))
            break
        else:
            missing = [names[c] for c in range(C) if c not in placed]
            raise ValueError(f'{", ".join(missing)}: no camera pair with {min_inliers} or more inliers and a point in common with the placed '
                             f'cameras reaches it; the person has to walk through the volume that this camera shares with another')
    return Rw, Tw, X, edges


def initial_extrinsics(cams, xyl, lik_thr=0.3, thr_px=4.0, hypotheses=4096, sample_size=8, score_points=16384, seed=0, rounds=3,
                       min_inliers=30, engine=None):
    """cams: the dict of calib.retrieve_calib_params (its extrinsics are not read); xyl [F..., C, K, 3] of one person.
    -> (cams with 'R', 'R_mat' and 'T' in camera 0's frame, the first tree edge's baseline 1; info: the pairs' results of
    Engine.relative_poses, 'pairs', 'edges' and the points 'X' of the assembly)."""
    from .engine import Engine
    xyl = np.asarray(xyl)
    C = len(cams['K'])
    if xyl.ndim < 3 or xyl.shape[-3] != C or xyl.shape[-1] != 3:
        raise ValueError(f'xyl has shape {xyl.shape}; expected [..., {C}, K, 3]')
    xn, usable = normalised(cams, xyl, lik_thr)
    pairs = all_pairs(C)
    f = np.array([[cams['K'][c][0][0], cams['K'][c][1][1]] for c in range(C)], dtype=np.float64)
    thr2 = np.array([(thr_px / np.mean([f[a], f[b]])) ** 2 for a, b in pairs])
    samples = draw_samples(usable, pairs, int(hypotheses), int(sample_size), seed)
    eng = engine if engine is not None else Engine(0)
    res = eng.relative_poses(xn, usable, pairs, samples, thr2, rounds=rounds, score_points=score_points)
    names = list(cams['names']) if 'names' in cams else None
    Rw, Tw, X, edges = assemble(C, xn, pairs, res['R'], res['t'], res['inliers'], res['mask'], min_inliers, names)
    for a, b, p, s, known in edges:
        logging.info(f'  {names[a] if names else a} -> {names[b] if names else b}: {res["inliers"][p]} inliers, {res["front"][p]} in front of both '
                     f'cameras, baseline {s:.4f} from {known} placed points')
    out = {k: list(v) for k, v in cams.items()}
    out['R_mat'] = [Rw[c] for c in range(C)]
    out['R'] = [cvmath.rodrigues_from_matrix(Rw[c]) for c in range(C)]
    out['T'] = [Tw[c] for c in range(C)]
    res.update(pairs=pairs, edges=edges, X=X)
    return out, res


def centres(cams):
    R, T = np.asarray(cams['R_mat'], dtype=np.float64), np.asarray(cams['T'], dtype=np.float64)
    return -np.einsum('cji,cj->ci', R, T)


def rescaled(cams, s):
    """The calibration with the world scaled by s about camera 0's centre (the rotations stay)."""
    c = centres(cams)
    R = np.asarray(cams['R_mat'], dtype=np.float64)
    out = {k: list(v) for k, v in cams.items()}
    out['T'] = [-R[i] @ (c[0] + s * (c[i] - c[0])) for i in range(len(R))]
    return out


def calibrate_from_keypoints(calib_toml, pose_dir, out_toml=None, baseline=None, height=None, keypoints=None, frame_range=None,
                             pose_model='HALPE_26', lik_thr=0.3, thr_px=4.0, hypotheses=4096, sample_size=8, score_points=16384, seed=0,
                             huber_px=3.0, min_cams=2, max_iter=100, ftol=1e-12, min_inliers=30, engine=None, floor=False, floor_threshold=0.03,
                             floor_hypotheses=1024, ankle_height=0.08):
    """Extrinsics of the cameras of calib_toml (its intrinsics and lenses are kept, its extrinsics ignored) from the keypoints
    under pose_dir, written in the reference's schema with adjusted = true to out_toml (default: <calib_toml>_keypoints.toml).
    calib_toml may be the dict of calib.retrieve_calib_params and pose_dir an array xyl [F..., C, K, 3]: nothing is written
    without an out_toml then.  Scale: baseline = (camera name a, camera name b, metres), or height = the person's, in metres
    (measurements.compute_height on the triangulated trial; needs the keypoints of pose_model), or neither: the first tree
    edge's baseline is 1 and a warning says so.  floor = True puts the world on the floor under the person's feet after the scale
    step (calib_align_floor.floor_frame on the triangulated trial with floor_threshold (m), floor_hypotheses and ankle_height; the
    report gains 'floor'); it needs a baseline or a height, since an arbitrary scale has no metres, and is refused without.  -> (out_toml or None, cams, report of the last refinement with the tree's 'edges', the assembled 'start' and its 'rms_start')."""
    from .engine import Engine
    if baseline is not None and height is not None:
        raise ValueError('give a baseline or a height, not both')
    if floor and baseline is None and height is None:
        raise ValueError('floor = True needs a baseline or a height: the floor is looked for with a threshold in metres')
    from_file = not isinstance(calib_toml, dict)
    cams = calib.retrieve_calib_params(calib_toml) if from_file else calib_toml
    ids, kp_names = calib_refine.select_keypoints(pose_model, keypoints)
    if isinstance(pose_dir, (str, os.PathLike)):
        xyl, json_dirs = calib_refine.read_trial(pose_dir, ids, frame_range)
        if len(json_dirs) != len(cams['K']):
            raise ValueError(f'{calib_toml} holds {len(cams["K"])} cameras, {pose_dir} {len(json_dirs)} camera folders')
    else:
        xyl = np.asarray(pose_dir)
    names = list(cams['names']) if 'names' in cams else [f'cam_{c + 1:02d}' for c in range(len(cams['K']))]
    if baseline is not None:
        na, nb, metres = baseline
        if na not in names or nb not in names or na == nb or not float(metres) > 0:
            raise ValueError(f'baseline {baseline!r}: expected two different cameras of {", ".join(names)} and a positive length')
    eng = engine if engine is not None else Engine(0)
    logging.info('Relative poses of the camera pairs, assembled from camera 0:')
    start, info = initial_extrinsics(cams, xyl, lik_thr=lik_thr, thr_px=thr_px, hypotheses=hypotheses, sample_size=sample_size,
                                     score_points=score_points, seed=seed, min_inliers=min_inliers, engine=eng)
    kw = dict(lik_thr=lik_thr, huber_px=huber_px, min_cams=min_cams, max_iter=max_iter, ftol=ftol, engine=eng)
    refined, report = calib_refine.refine_extrinsics(start, xyl, start_thr=WIDE_START_THR, **kw)
    rms_start = report['rms_before']
    moved = np.abs(centres(refined) - centres(start)).max() > MOVED_M or \
        max(np.abs(a - b).max() for a, b in zip(refined['R_mat'], start['R_mat'])) > MOVED_RAD
    if moved:
        refined, report = calib_refine.refine_extrinsics(refined, xyl, **kw)
    if baseline is not None:
        c = centres(refined)
        refined = rescaled(refined, float(metres) / np.linalg.norm(c[names.index(na)] - c[names.index(nb)]))
    elif height is not None:
        import pandas as pd
        from . import measurements
        R, T = np.asarray(refined['R_mat'], dtype=np.float64), np.asarray(refined['T'], dtype=np.float64)
        K = np.asarray(refined['K'], dtype=np.float64)
        und = calib_refine.undistorted(refined, xyl)
        eng.set_calibration([K[c] @ np.hstack([R[c], T[c].reshape(3, 1)]) for c in range(len(K))])
        Q = eng.triangulate(und, Engine.tri_params(15.0, lik_thr, max(2, int(min_cams))))[0]
        Q = Q.reshape(-1, Q.shape[-2] * 3)
        table = pd.DataFrame(Q, columns=[n for n in kp_names for _ in range(3)])
        measured = float(measurements.compute_height(table, kp_names, engine=eng))
        if not measured > 0:
            raise ValueError(f'the height of the triangulated person is {measured}; no scale can be taken from it')
        refined = rescaled(refined, float(height) / measured)
    else:
        logging.warning('No baseline and no height given: the scale of the calibration is arbitrary (the first baseline is 1).')
    report = dict(report, edges=info['edges'], rms_start=rms_start, start=start)
    if floor:
        from . import calib_align_floor
        A, b, report['floor'] = calib_align_floor.floor_frame(calib_align_floor.triangulated(refined, xyl, lik_thr, min_cams, eng), kp_names,
                                                              hypotheses=floor_hypotheses, threshold=floor_threshold, seed=seed,
                                                              ankle_height=ankle_height, engine=eng)
        refined = calib_align_floor.moved_cameras(refined, A, b)
    logging.info(f'Extrinsics from {report["kept_points"]} points, cost {report["cost_after"]:.6g}.')
    for c, name in enumerate(names):
        logging.info(f'  {name}: weighted RMS reprojection error {rms_start[c]:.3f} px at the assembled start -> {report["rms_after"][c]:.3f} px')
    if out_toml is None and from_file:
        out_toml = os.path.splitext(calib_toml)[0] + '_keypoints.toml'
    if out_toml is not None:
        error = float(np.sqrt(np.mean(np.square(report['rms_after']))))
        calib.write_calibration_toml(out_toml, refined, adjusted=True, error=error)
        logging.info(f'Calibration written to {out_toml}.')
    return out_toml, refined, report


def parse_args(argv=None):
    parser = argparse.ArgumentParser(prog='python -m pose2sim_amd.calib_from_keypoints',
                                     description='Extrinsics from the 2D keypoints of a person walking through the volume; intrinsics given.')
    parser.add_argument('-c', '--calib', required=True, help='calibration .toml with the intrinsics (its extrinsics are ignored)')
    parser.add_argument('-p', '--pose', required=True, help='pose folder of the trial: one <camera>_json folder a camera')
    parser.add_argument('-o', '--output', default=None, help='calibration to write (default: <calib>_keypoints.toml)')
    parser.add_argument('--baseline', nargs=3, default=None, metavar=('A', 'B', 'M'), help='cameras A and B are M metres apart')
    parser.add_argument('--height', type=float, default=None, help="the person's height, m")
    parser.add_argument('--floor', action='store_true', help='put the world frame on the floor the person walks on: Z up, Y along the walk (needs --baseline or --height)')
    parser.add_argument('--floor-threshold', type=float, default=0.03, help='--floor: inlier distance from the floor, m')
    parser.add_argument('--floor-hypotheses', type=int, default=1024, help='--floor: triples of foot points that are tried')
    parser.add_argument('--ankle-height', type=float, default=0.08, help='--floor: height of the ankles over the floor, m (models without heels and toes)')
    parser.add_argument('--threshold', type=float, default=4.0, help='inlier threshold of the Sampson distance, px')
    parser.add_argument('--hypotheses', type=int, default=4096, help='hypotheses a camera pair')
    parser.add_argument('--sample-size', type=int, default=8, help='correspondences a hypothesis (8 .. 16)')
    parser.add_argument('--score-points', type=int, default=16384, help='points a pair at most that the hypotheses are scored on')
    parser.add_argument('--seed', type=int, default=0, help='seed of the samples: the same seed gives the same calibration')
    parser.add_argument('--likelihood', type=float, default=0.3, help='observations below this likelihood do not count')
    parser.add_argument('--huber', type=float, default=3.0, help='delta of the Huber loss of the refinement, px')
    parser.add_argument('--min-cams', type=int, default=2, help='cameras a point needs in the refinement')
    parser.add_argument('--keypoints', default=None, help='comma-separated keypoint names (default: all of the model)')
    parser.add_argument('--pose-model', default='HALPE_26', help='skeleton the JSON files follow')
    parser.add_argument('--frames', type=int, nargs=2, default=None, metavar=('FIRST', 'END'), help='frame range [FIRST, END)')
    args = parser.parse_args(argv)
    if args.keypoints is not None:
        args.keypoints = [k.strip() for k in args.keypoints.split(',') if k.strip()]
        if not args.keypoints:
            parser.error('--keypoints names no keypoint')
    if args.baseline is not None:
        if args.height is not None:
            parser.error('--baseline and --height exclude each other')
        try:
            args.baseline = (args.baseline[0], args.baseline[1], float(args.baseline[2]))
        except ValueError:
            parser.error('--baseline takes two camera names and a length in metres')
        if not args.baseline[2] > 0 or args.baseline[0] == args.baseline[1]:
            parser.error('--baseline needs two different cameras and a positive length')
    if args.floor and args.baseline is None and args.height is None:
        parser.error('--floor needs --baseline or --height: the floor is looked for with a threshold in metres')
    if not args.floor_threshold > 0 or args.floor_hypotheses < 1 or args.ankle_height < 0:
        parser.error('--floor-threshold must be positive, --floor-hypotheses 1 or more, --ankle-height 0 or more')
    if args.height is not None and not args.height > 0:
        parser.error('--height must be positive')
    if not args.threshold > 0 or not args.huber > 0:
        parser.error('--threshold and --huber must be positive')
    if args.hypotheses < 1 or not 8 <= args.sample_size <= 16 or args.min_cams < 2:
        parser.error('--hypotheses must be 1 or more, --sample-size 8 .. 16, --min-cams 2 or more')
    return args


def main(argv=None):
    args = parse_args(argv)
    logging.basicConfig(format='%(message)s', level=logging.INFO)
    calibrate_from_keypoints(args.calib, args.pose, args.output, baseline=args.baseline, height=args.height, keypoints=args.keypoints,
                             frame_range=args.frames, pose_model=args.pose_model, lik_thr=args.likelihood, thr_px=args.threshold,
                             hypotheses=args.hypotheses, sample_size=args.sample_size, score_points=args.score_points, seed=args.seed,
                             huber_px=args.huber, min_cams=args.min_cams, floor=args.floor, floor_threshold=args.floor_threshold,
                             floor_hypotheses=args.floor_hypotheses, ankle_height=args.ankle_height)


if __name__ == '__main__':
    main()
