"""Refinement of a calibration's extrinsics from the 2D keypoints of a recorded trial.

The reference names this (`extrinsics_method = 'keypoints'`) and answers it with NotImplementedError
(calibration.py:969-971, :998-999).  Here the cameras' rotations and translations are bundle-adjusted on the trial's
keypoints -- the robust reprojection error over all cameras and all 3D points jointly, intrinsics and distortion held,
camera 0 and the scale of the input calibration kept -- by Engine.refine_extrinsics (csrc/p2s_refine.hip).

    python -m pose2sim_amd.calib_refine -c Calib.toml -p pose [-o Calib_refined.toml] [--likelihood 0.3] [--huber 3]
                                        [--min-cams 2] [--keypoints Nose,Neck,...] [--pose-model HALPE_26]
"""
import argparse
import logging
import os

import numpy as np

from . import calib, cvmath, poseio, skeletons


def undistorted(cams, xyl):
    """xyl [..., C, K, 3] with the pixels of every camera that has a lens taken to the pinhole model of its own K
    (cv2.undistortPoints with newK = K); float64, likelihoods and NaN untouched."""
    out = np.array(xyl, dtype=np.float64)
    for c in range(out.shape[-3]):
        dist = np.asarray(cams['dist'][c], dtype=np.float64)
        if np.any(dist != 0):
            K = np.asarray(cams['K'][c], dtype=np.float64)
            out[..., c, :, :2] = cvmath.undistort_points(out[..., c, :, :2], K, dist, K)
    return out


def refine_extrinsics(cams, xyl, lik_thr=0.3, huber_px=3.0, min_cams=2, max_iter=100, ftol=1e-12, start_thr=50.0, engine=None):
    """cams: the dict of calib.retrieve_calib_params; xyl [F..., C, K, 3] pixels and likelihoods of one person.
    -> (cams with refined 'R' (Rodrigues vectors), 'R_mat' and 'T', report of Engine.refine_extrinsics).
    The start points come from Engine.triangulate through the input cameras with the same lik_thr and min_cams and the
    reprojection threshold start_thr (px): observations its search excludes do not pull the start."""
    from .engine import Engine
    xyl = np.asarray(xyl)
    C = len(cams['K'])
    if xyl.ndim < 3 or xyl.shape[-3] != C or xyl.shape[-1] != 3:
        raise ValueError(f'xyl has shape {xyl.shape}; expected [..., {C}, K, 3]')
    if any(np.any(np.asarray(cams['dist'][c]) != 0) for c in range(C)):
        xyl = undistorted(cams, xyl)
    K = np.asarray(cams['K'], dtype=np.float64).reshape(C, 3, 3)
    R = np.asarray(cams['R_mat'], dtype=np.float64).reshape(C, 3, 3)
    T = np.asarray(cams['T'], dtype=np.float64).reshape(C, 3)
    eng = engine if engine is not None else Engine(0)
    eng.set_calibration([K[c] @ np.hstack([R[c], T[c].reshape(3, 1)]) for c in range(C)])
    X0 = eng.triangulate(xyl, Engine.tri_params(start_thr, lik_thr, max(2, int(min_cams))))[0]
    Rn, Tn, _, report = eng.refine_extrinsics(xyl, K, R, T, X0.reshape(-1, 3), lik_thr=lik_thr, huber_px=huber_px, min_cams=min_cams,
                                              max_iter=max_iter, ftol=ftol)
    out = {k: list(v) for k, v in cams.items()}
    out['R_mat'] = [Rn[c] for c in range(C)]
    out['R'] = [cvmath.rodrigues_from_matrix(Rn[c]) for c in range(C)]
    out['T'] = [Tn[c] for c in range(C)]
    return out, report


def read_trial(pose_dir, keypoints_ids, frame_range=None):
    """The first person of every file of the camera folders of pose_dir (the reference's natural folder order), through
    the native ingest: xyl [F][C][K][3], NaN where a file, person or keypoint is missing."""
    _, json_dirs = poseio.list_json_dirs(pose_dir)
    if len(json_dirs) < 2:
        raise ValueError(f'{pose_dir} holds {len(json_dirs)} camera folders with "json" in their name; 2 or more are needed')
    names = poseio.list_json_files(pose_dir, json_dirs)
    maps = poseio.frame_file_map(names)
    frames = sorted(set().union(*[set(m) for m in maps]))
    if not frames:
        raise ValueError(f'no JSON files under {pose_dir}')
    f_range = (frames[0], frames[-1] + 1) if frame_range is None else (int(frame_range[0]), int(frame_range[1]))
    return poseio.load_observations(pose_dir, json_dirs, maps, f_range, keypoints_ids, 1)[:, 0], json_dirs


def select_keypoints(pose_model, keypoints=None):
    """(ids in the JSON lists, names) of the model's keypoints, or of those named in `keypoints`."""
    ids, names, _ = skeletons.keypoints(pose_model)
    if keypoints:
        missing = [k for k in keypoints if k not in names]
        if missing:
            raise ValueError(f'{pose_model} has no keypoint named {", ".join(missing)}')
        ids = [ids[names.index(k)] for k in keypoints]
        names = list(keypoints)
    return list(ids), list(names)


def log_report(report, names):
    logging.info(f'Extrinsics refined on {report["kept_points"]} points: cost {report["cost_before"]:.6g} -> {report["cost_after"]:.6g} '
                 f'in {report["iterations"]} iterations ({report["accepted"]} accepted), coordinate {"xyz"[report["held_coord"]]} of '
                 f'{names[1]}\'s translation held.')
    for c, name in enumerate(names):
        logging.info(f'  {name}: weighted RMS reprojection error {report["rms_before"][c]:.3f} px -> {report["rms_after"][c]:.3f} px')


def refine_calibration(calib_toml, pose_dir, out_toml=None, keypoints=None, frame_range=None, pose_model='HALPE_26', lik_thr=0.3,
                       huber_px=3.0, min_cams=2, max_iter=100, ftol=1e-12, engine=None):
    """Refine the extrinsics of calib_toml on the keypoints under pose_dir (a single-person or associated trial) and write
    them, in the reference's schema with adjusted = true, to out_toml (default: <calib_toml>_refined.toml).
    -> (out_toml, report)."""
    cams = calib.retrieve_calib_params(calib_toml)
    ids, _ = select_keypoints(pose_model, keypoints)
    xyl, json_dirs = read_trial(pose_dir, ids, frame_range)
    if len(json_dirs) != len(cams['K']):
        raise ValueError(f'{calib_toml} holds {len(cams["K"])} cameras, {pose_dir} {len(json_dirs)} camera folders')
    refined, report = refine_extrinsics(cams, xyl, lik_thr=lik_thr, huber_px=huber_px, min_cams=min_cams, max_iter=max_iter, ftol=ftol,
                                        engine=engine)
    if out_toml is None:
        out_toml = os.path.splitext(calib_toml)[0] + '_refined.toml'
    error = float(np.sqrt(np.mean(np.square(report['rms_after']))))
    calib.write_calibration_toml(out_toml, refined, adjusted=True, error=error)
    log_report(report, refined['names'])
    logging.info(f'Calibration written to {out_toml}.')
    return out_toml, report


def parse_args(argv=None):
    parser = argparse.ArgumentParser(prog='python -m pose2sim_amd.calib_refine',
                                     description='Refine the extrinsics of a calibration on the 2D keypoints of a trial.')
    parser.add_argument('-c', '--calib', required=True, help='calibration .toml to refine')
    parser.add_argument('-p', '--pose', required=True, help='pose folder of the trial: one <camera>_json folder a camera')
    parser.add_argument('-o', '--output', default=None, help='refined .toml (default: <calib>_refined.toml)')
    parser.add_argument('--likelihood', type=float, default=0.3, help='observations below this likelihood do not count')
    parser.add_argument('--huber', type=float, default=3.0, help='delta of the Huber loss, px')
    parser.add_argument('--min-cams', type=int, default=2, help='cameras a point needs')
    parser.add_argument('--keypoints', default=None, help='comma-separated keypoint names (default: all of the model)')
    parser.add_argument('--pose-model', default='HALPE_26', help='skeleton the JSON files follow')
    parser.add_argument('--frames', type=int, nargs=2, default=None, metavar=('FIRST', 'END'), help='frame range [FIRST, END)')
    args = parser.parse_args(argv)
    if args.keypoints is not None:
        args.keypoints = [k.strip() for k in args.keypoints.split(',') if k.strip()]
        if not args.keypoints:
            parser.error('--keypoints names no keypoint')
    if not args.huber > 0:
        parser.error('--huber must be positive')
    if args.min_cams < 2:
        parser.error('--min-cams must be 2 or more')
    return args


def main(argv=None):
    args = parse_args(argv)
    logging.basicConfig(format='%(message)s', level=logging.INFO)
    refine_calibration(args.calib, args.pose, args.output, keypoints=args.keypoints, frame_range=args.frames, pose_model=args.pose_model,
                       lik_thr=args.likelihood, huber_px=args.huber, min_cams=args.min_cams)


if __name__ == '__main__':
    main()
