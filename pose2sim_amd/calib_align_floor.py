"""The world frame on the floor: Z up from the plane under the feet of a walking person, Y along the walk.

calib_from_keypoints leaves the world in camera 0's frame, and a board that stood askew leaves it tilted; the .trc writer
(the reference's zup2yup), trc_gaitevents' defaults and OpenSim all take the calibration's Z as "up".  The floor is the
dominant plane of the foot keypoints of a walk: the feet rest on it during stance and are above it during swing.  It is
found by hypothesise and score (Engine.fit_planes, csrc/p2s_floor.hip, DESIGN.md 4.23: planes through sampled triples, MSAC
on the signed distance, refits on the inliers), oriented by the hips, and the heading is the principal axis of the hips'
trajectory on it.  Through zup2yup the .trc then runs along +X, has +Y up and +Z to the right.

What the data must be: ONE person who WALKS, in metres (a calibration of arbitrary scale has no 3 cm).  A walk along one
straight line whose feet stay within a narrow band fixes the plane's roll about that line badly; a warning says so.

    python -m pose2sim_amd.calib_align_floor -c Calib.toml -p pose [-o Calib_floor.toml] [--threshold 0.03] [--hypotheses 1024]
                                             [--seed 0] [--likelihood 0.3] [--pose-model HALPE_26] [--ankle-height 0.08]
    python -m pose2sim_amd.calib_align_floor --trc a.trc b.trc ...            (writes <name>_floor.trc beside each)
"""
import argparse
import logging
import os

import numpy as np

from . import calib, calib_refine, cvmath, trc

FEET = ('LHeel', 'RHeel', 'LBigToe', 'RBigToe', 'LSmallToe', 'RSmallToe')
ANKLES = ('LAnkle', 'RAnkle')
HIPS = ('LHip', 'RHip', 'Hip')
NECK = ('Neck',)
REPROJ_THR = 15.0          # px: the reprojection threshold of the triangulation that feeds the plane
NARROW_BAND = 10.0         # thresholds: an inlier band narrower than this lets the plane roll by threshold / extent, 0.1 rad


def draw_triples(usable, H, seed=0):
    """samples [H][3] int32: H rows of 3 distinct indices of usable points, from default_rng(seed); -1 throughout with fewer
    than 3 such points (calib_from_keypoints.draw_samples for one problem and m = 3)."""
    idx = np.flatnonzero(np.asarray(usable, dtype=bool))
    rng = np.random.default_rng(seed)
    k = len(idx)
    if k < 3:
        return np.full((H, 3), -1, dtype=np.int32)
    if k <= 36:                                              # few points: the first 3 of a random order
        rows = np.argsort(rng.random((H, k)), axis=1)[:, :3]
    else:                                                    # many: draw, and redraw the rows that repeat an index
        rows = rng.integers(0, k, (H, 3))
        while True:
            s = np.sort(rows, axis=1)
            bad = np.flatnonzero((s[:, 1:] == s[:, :-1]).any(axis=1))
            if not len(bad):
                break
            rows[bad] = rng.integers(0, k, (len(bad), 3))
    return idx[rows].astype(np.int32)


def plane_inputs(X, names, ankle_height=0.08):
    """X [F][K][3] of one person -> (points [N][3] of the foot keypoints, usable [N], ref [3], trajectory [F][3] of the
    ref keypoints' mean, offset: how far the floor lies below the plane of these points)."""
    X = np.asarray(X, dtype=np.float64)
    names = list(names)
    if X.ndim != 3 or X.shape[1] != len(names) or X.shape[2] != 3:
        raise ValueError(f'X has shape {X.shape}; expected [F][{len(names)}][3]')
    feet, offset = [names.index(n) for n in FEET if n in names], 0.0
    if not feet:
        feet, offset = [names.index(n) for n in ANKLES if n in names], float(ankle_height)
    if not feet:
        raise ValueError(f'none of {", ".join(FEET + ANKLES)} among the keypoints: no floor without feet')
    above = [names.index(n) for n in HIPS if n in names] or [names.index(n) for n in NECK if n in names]
    if not above:
        raise ValueError(f'none of {", ".join(HIPS + NECK)} among the keypoints: nothing says which side of the floor is up')
    points = X[:, feet].reshape(-1, 3)
    usable = np.isfinite(points).all(axis=1)
    traj = X[:, above]
    seen = np.isfinite(traj).all(axis=2)                                       # [F][len(above)]
    with np.errstate(invalid='ignore', divide='ignore'):
        traj = np.where(seen[..., None], traj, 0.0).sum(axis=1) / seen.sum(axis=1)[:, None]   # NaN where no ref keypoint is seen
    good = np.isfinite(traj).all(axis=1)
    if not good.any():
        raise ValueError(f'{", ".join(names[i] for i in above)}: not seen in any frame')
    return points, usable, traj[good].mean(axis=0), traj, offset


def frame_of_plane(plane, centroid, traj, offset=0.0):
    """The rigid map x' = A x + b into the world of the floor n . x = d - offset: Z' = n, the origin the centroid dropped
    onto the floor, Y' the principal axis of the trajectory projected on the floor, its sign that of the first-to-last
    displacement (exactly 0: its largest coordinate positive), X' = Y' x Z'."""
    n, d = np.asarray(plane[:3], dtype=np.float64), float(plane[3]) - float(offset)
    traj = np.asarray(traj, dtype=np.float64)
    traj = traj[np.isfinite(traj).all(axis=1)]
    flat = traj - np.outer(traj @ n - d, n)
    dev = flat - flat.mean(axis=0)
    y = np.linalg.eigh(dev.T @ dev)[1][:, -1]
    y = y - (y @ n) * n
    y /= np.linalg.norm(y)
    along = float((flat[-1] - flat[0]) @ y)
    if along < 0 or (along == 0 and y[np.argmax(np.abs(y))] < 0):
        y = -y
    A = np.stack([np.cross(y, n), y, n])
    origin = np.asarray(centroid, dtype=np.float64)
    origin = origin - (origin @ n - d) * n
    return A, -A @ origin


def floor_frames(Xs, names, hypotheses=1024, threshold=0.03, seed=0, rounds=3, ankle_height=0.08, engine=None, host=False):
    """floor_frame for several persons or trials in one call of Engine.fit_planes: Xs a list of [F][K][3], names the
    keypoint names of each (or one list for all).  -> [(A, b, report)]."""
    from . import engine as engine_module
    if names and isinstance(names[0], str):
        names = [names] * len(Xs)
    if not len(Xs) or len(names) != len(Xs):
        raise ValueError('one list of keypoint names a trial is needed, and a trial at least')
    ins = [plane_inputs(X, nm, ankle_height) for X, nm in zip(Xs, names)]
    B, N, H = len(ins), max(len(i[0]) for i in ins), int(hypotheses)
    points, usable = np.zeros((B, N, 3)), np.zeros((B, N), dtype=bool)
    samples = np.empty((B, H, 3), dtype=np.int32)
    for p, (pts, ok, _, _, _) in enumerate(ins):
        points[p, :len(pts)], usable[p, :len(pts)] = np.where(ok[:, None], pts, 0.0), ok
        samples[p] = draw_triples(ok, H, seed)
    ref = np.array([i[2] for i in ins])
    if host:
        fit = engine_module.fit_planes_host
    else:
        fit = (engine if engine is not None else engine_module.Engine(0)).fit_planes
    res = fit(points, usable, ref, samples, float(threshold), rounds=rounds)
    out = []
    for p, (pts, ok, _, traj, offset) in enumerate(ins):
        rep = {k: res[k][p] for k in ('plane', 'cost', 'inliers', 'below', 'winner', 'refits', 'centroid', 'evals')}
        rep.update(mask=res['mask'][p, :len(pts)], points=int(ok.sum()), offset=offset, threshold=float(threshold))
        if rep['winner'] < 0:
            raise ValueError(f'trial {p}: no plane through {rep["points"]} foot points; the person has to be seen walking')
        with np.errstate(invalid='ignore'):
            rep['band'] = float(np.sqrt(max(rep['evals'][1], 0.0)))
        if rep['band'] < NARROW_BAND * threshold:
            logging.warning(f'The feet on the floor lie within a band of {rep["band"]:.3f} m (RMS) about one line: the floor may roll about '
                            f'that line by up to {threshold / max(rep["band"], 1e-12):.2f} rad.  A walk with a turn in it fixes that.')
        if rep['below'] > rep['inliers'] / 10:
            logging.warning(f'{rep["below"]} foot points lie more than {threshold} m below the plane of {rep["inliers"]}: this may not be the floor.')
        A, b = frame_of_plane(rep['plane'], rep['centroid'], traj, offset)
        rep.update(A=A, b=b)
        logging.info(f'Floor from {rep["inliers"]} of {rep["points"]} foot points (hypothesis {rep["winner"]}, {rep["refits"]} refits kept), '
                     f'RMS distance {np.sqrt(max(rep["evals"][0], 0.0)) * 1000:.1f} mm.')
        out.append((A, b, rep))
    return out


def floor_frame(X, names, hypotheses=1024, threshold=0.03, seed=0, rounds=3, ankle_height=0.08, engine=None, host=False):
    """X [F][K][3]: one person's keypoints `names` in any frame, metres.  -> (A [3][3], b [3], report): x' = A x + b is the
    point in the world whose Z = 0 is the floor, whose Z points up and whose Y is the heading of the walk.  The floor is the
    plane of the heels and toes (of the ankles, ankle_height above it, for a model without them) found by
    Engine.fit_planes from `hypotheses` triples of default_rng(seed) with the inlier distance `threshold` (m); host = True
    runs the library's host path instead (no GPU: for checking it).  report: the plane, cost, inliers, below, winner,
    refits, centroid, evals and mask of fit_planes, 'band' (m), 'A' and 'b'."""
    return floor_frames([X], [list(names)], hypotheses, threshold, seed, rounds, ankle_height, engine, host)[0]


def moved_cameras(cams, A, b):
    """The calibration `cams` for the world x' = A x + b: R' = R A^T, t' = t - R A^T b."""
    out = {k: list(v) for k, v in cams.items()}
    R = [np.asarray(r, dtype=np.float64) @ A.T for r in cams['R_mat']]
    out['R_mat'] = R
    out['R'] = [cvmath.rodrigues_from_matrix(r) for r in R]
    out['T'] = [np.asarray(t, dtype=np.float64) - r @ b for r, t in zip(R, cams['T'])]
    return out


def triangulated(cams, xyl, lik_thr=0.3, min_cams=2, engine=None):
    """xyl [F][C][K][3] -> X [F][K][3] through the cameras `cams` (lenses undone first), NaN where fewer than min_cams
    cameras agree within REPROJ_THR px."""
    from .engine import Engine
    eng = engine if engine is not None else Engine(0)
    R, T = np.asarray(cams['R_mat'], dtype=np.float64), np.asarray(cams['T'], dtype=np.float64)
    K = np.asarray(cams['K'], dtype=np.float64)
    und = calib_refine.undistorted(cams, xyl)
    eng.set_calibration([K[c] @ np.hstack([R[c], T[c].reshape(3, 1)]) for c in range(len(K))])
    Q = eng.triangulate(und, Engine.tri_params(REPROJ_THR, lik_thr, max(2, int(min_cams))))[0]
    return Q.reshape(-1, Q.shape[-2], 3)


def align_calibration(calib_toml, pose_dir, out_toml=None, keypoints=None, frame_range=None, pose_model='HALPE_26', lik_thr=0.3,
                      min_cams=2, hypotheses=1024, threshold=0.03, seed=0, ankle_height=0.08, engine=None):
    """The calibration calib_toml with its world put on the floor that the person under pose_dir walks on: the trial is
    triangulated through it, floor_frame finds the floor, and the cameras are written in the reference's schema with
    adjusted = true to out_toml (default: <calib_toml>_floor.toml).  calib_toml may be the dict of
    calib.retrieve_calib_params and pose_dir an array xyl [F..., C, K, 3]: nothing is written without an out_toml then.
    -> (out_toml or None, cams, report of floor_frame)."""
    from .engine import Engine
    from_file = not isinstance(calib_toml, dict)
    cams = calib.retrieve_calib_params(calib_toml) if from_file else calib_toml
    ids, kp_names = calib_refine.select_keypoints(pose_model, keypoints)
    if isinstance(pose_dir, (str, os.PathLike)):
        xyl, json_dirs = calib_refine.read_trial(pose_dir, ids, frame_range)
        if len(json_dirs) != len(cams['K']):
            raise ValueError(f'{calib_toml} holds {len(cams["K"])} cameras, {pose_dir} {len(json_dirs)} camera folders')
    else:
        xyl = np.asarray(pose_dir)
    if xyl.shape[-2] != len(kp_names):
        raise ValueError(f'xyl has {xyl.shape[-2]} keypoints; {len(kp_names)} are named')
    eng = engine if engine is not None else Engine(0)
    X = triangulated(cams, xyl, lik_thr, min_cams, eng)
    A, b, report = floor_frame(X, kp_names, hypotheses, threshold, seed, ankle_height=ankle_height, engine=eng)
    out = moved_cameras(cams, A, b)
    if out_toml is None and from_file:
        out_toml = os.path.splitext(calib_toml)[0] + '_floor.toml'
    if out_toml is not None:
        calib.write_calibration_toml(out_toml, out, adjusted=True)
        logging.info(f'Calibration written to {out_toml}.')
    return out_toml, out, report


def zup_markers(coords):
    """The stored (Y-up) columns [F][3 K] of a .trc as [F][K][3] in the Z-up frame they were written from (zup2yup undone)."""
    c = np.asarray(coords, dtype=np.float64).reshape(len(coords), -1, 3)
    return c[..., [2, 0, 1]]


def align_trc_batch(trc_paths, out_paths=None, hypotheses=1024, threshold=0.03, seed=0, ankle_height=0.08, engine=None, host=False):
    """align_trc for the files of a session: their planes are the problems of one Engine.fit_planes call.  A file whose Units
    field is not m is refused.  -> [(out_path, A, b, report)]."""
    trc_paths = list(trc_paths)
    if out_paths is None:
        out_paths = [os.path.splitext(p)[0] + '_floor.trc' for p in trc_paths]
    if len(out_paths) != len(trc_paths):
        raise ValueError('one output path a .trc file is needed')
    loaded = [trc.load_trc(p) for p in trc_paths]
    for src, (_, _, _, _, header) in zip(trc_paths, loaded):
        if trc.units(header) != 'm':
            raise ValueError(f'{src} is in {trc.units(header) or "no named unit"}; the floor is looked for with a threshold in metres: convert the file to m')
    Xs = [zup_markers(coords) for _, _, coords, _, _ in loaded]
    frames = floor_frames(Xs, [markers for _, _, _, markers, _ in loaded], hypotheses, threshold, seed, 3, ankle_height, engine, host)
    out = []
    for src, path, (frame_col, _, _, markers, header), X, (A, b, report) in zip(trc_paths, out_paths, loaded, Xs, frames):
        moved = (X @ A.T + b).reshape(len(X), -1)
        trc.write_like(path, header, frame_col, trc.time_column(src), moved[:, trc.yup_columns(len(markers))])
        logging.info(f'{path}: on the floor, along +X, +Y up.')
        out.append((path, A, b, report))
    return out


def align_trc(trc_path, out_path=None, **kw):
    """The Y-up file trc_path re-expressed in the frame of the floor its person walks on (floor_frame on its markers after
    the inverse of zup2yup), written to out_path (default: <trc_path>_floor.trc): the walk along +X, +Y up, +Z to the right.
    -> (out_path, A, b, report), (A, b) in the Z-up frame."""
    return align_trc_batch([trc_path], None if out_path is None else [out_path], **kw)[0]


def parse_args(argv=None):
    parser = argparse.ArgumentParser(prog='python -m pose2sim_amd.calib_align_floor',
                                     description='Put the world frame of a calibration, or of .trc files, on the floor a person walks on.')
    parser.add_argument('-c', '--calib', default=None, help='calibration .toml to align')
    parser.add_argument('-p', '--pose', default=None, help='pose folder of the trial: one <camera>_json folder a camera')
    parser.add_argument('-o', '--output', default=None, help='calibration to write (default: <calib>_floor.toml)')
    parser.add_argument('--trc', nargs='+', default=None, help='.trc files to align instead (each writes <name>_floor.trc)')
    parser.add_argument('--threshold', type=float, default=0.03, help='inlier distance from the floor, m')
    parser.add_argument('--hypotheses', type=int, default=1024, help='triples of foot points that are tried')
    parser.add_argument('--seed', type=int, default=0, help='seed of the triples: the same seed gives the same frame')
    parser.add_argument('--likelihood', type=float, default=0.3, help='observations below this likelihood do not count')
    parser.add_argument('--min-cams', type=int, default=2, help='cameras a triangulated point needs')
    parser.add_argument('--ankle-height', type=float, default=0.08, help='height of the ankles over the floor, m (models without heels and toes)')
    parser.add_argument('--pose-model', default='HALPE_26', help='skeleton the JSON files follow')
    parser.add_argument('--frames', type=int, nargs=2, default=None, metavar=('FIRST', 'END'), help='frame range [FIRST, END)')
    args = parser.parse_args(argv)
    if (args.trc is None) == (args.calib is None) or (args.calib is not None and args.pose is None):
        parser.error('give --calib with --pose, or --trc')
    if not args.threshold > 0 or args.hypotheses < 1 or args.min_cams < 2 or args.ankle_height < 0:
        parser.error('--threshold must be positive, --hypotheses 1 or more, --min-cams 2 or more, --ankle-height 0 or more')
    return args


def main(argv=None):
    args = parse_args(argv)
    logging.basicConfig(format='%(message)s', level=logging.INFO)
    kw = dict(hypotheses=args.hypotheses, threshold=args.threshold, seed=args.seed, ankle_height=args.ankle_height)
    if args.trc is not None:
        align_trc_batch(args.trc, **kw)
    else:
        align_calibration(args.calib, args.pose, args.output, frame_range=args.frames, pose_model=args.pose_model, lik_thr=args.likelihood,
                          min_cams=args.min_cams, **kw)


if __name__ == '__main__':
    main()
