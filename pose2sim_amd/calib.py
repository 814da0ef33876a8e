"""Calibration TOML -> camera parameters and projection matrices.

Restates retrieve_calib_params (common.py:254-288) and computeP (common.py:291-324) on top of
``tomli`` (the reference uses ``toml``) and the camera model in cvmath.py.  Schema written by
calibration.py:1504-1533: one table per camera with name, size, matrix, distortions, rotation
(Rodrigues vector), translation, fisheye; tables named metadata / capture_volume / charuco /
checkerboard are skipped.
"""
import glob
import os

import numpy as np
import tomli

from . import cvmath

_SKIP = ('metadata', 'capture_volume', 'charuco', 'checkerboard')


def load_toml(path):
    with open(path, 'rb') as f:
        return tomli.load(f)


def camera_keys(calib):
    return [c for c in calib.keys() if c not in _SKIP and isinstance(calib[c], dict)]


# ---- per-frame cameras (Utilities/reproj_from_trc_calib.py:86-141): a camera table whose matrix is [Fc][3][3] zooms, one
# whose rotation and translation are [Fc][3] moves.  One reader for the reprojection utility and for triangulation.
PER_FRAME_REFUSAL = 'per-frame cameras (a moving or zooming rig: matrix [F][3][3], rotation / translation [F][3])'
UNDISTORT_PER_FRAME = 'undistort_points with moving or zooming cameras: the distorted projection takes static cameras only'


def read_cameras(calib_path, keys=None):
    """-> per camera: size, K ([3][3] or [Fc][3][3]), dist, rotation vector(s), translation(s).  keys picks the tables
    out of the parsed file (camera_keys for triangulation); by default every table but 'metadata', the rule of the
    reference's reprojection utility."""
    tables = load_toml(calib_path)
    names = [k for k in tables if k != 'metadata'] if keys is None else keys(tables)
    cams = []
    for key in names:
        t = tables[key]
        cams.append({'S': np.array(t['size'], dtype=np.float64), 'K': np.array(t['matrix'], dtype=np.float64),
                     'dist': np.array(t['distortions'], dtype=np.float64), 'R': np.array(t['rotation'], dtype=np.float64),
                     'T': np.array(t['translation'], dtype=np.float64)})
    return cams


def camera_frames(cam):
    """Calibration frames of one camera of read_cameras; None for a static one."""
    zooming, moving = cam['K'].ndim == 3, cam['R'].ndim == 2
    return len(cam['K']) if zooming else len(cam['R']) if moving else None


def camera_projections(cam):
    """[Fp][3][4] = [K | 0] [[R, T], [0, 1]] of one camera: Fp = 1 for a static one, else one matrix per calibration
    frame of a zooming (K per frame) and / or moving (rotation and translation per frame) camera."""
    zooming, moving = cam['K'].ndim == 3, cam['R'].ndim == 2
    per_frame = []
    for f in range(camera_frames(cam) or 1):
        K = cam['K'][f] if zooming else cam['K']
        rvec, T = (cam['R'][f], cam['T'][f]) if moving else (cam['R'], cam['T'])
        H = np.block([[cvmath.rodrigues(rvec), T.reshape(3, 1)], [np.zeros(3), 1]])
        per_frame.append(np.block([K, np.zeros((3, 1))]) @ H)
    return per_frame


def projection_matrices(cams):
    """P [C][Fp][3][4] and whether any camera is per-frame, as the reprojection utility takes them."""
    P = [camera_projections(cam) for cam in cams]
    # cameras with different frame counts: NumPy refuses the ragged list here, as in the reference
    return np.array(P).reshape(len(P), -1, 3, 4), any(camera_frames(c) is not None for c in cams)


def is_per_frame(calib_file):
    """Whether some camera of the calibration (camera_keys) moves or zooms."""
    return any(camera_frames(c) is not None for c in read_cameras(calib_file, camera_keys))


def frame_projections(calib_file):
    """The calibration for triangulation with per-frame cameras: P [Fc][C][3][4] over the tables of camera_keys, the static
    cameras of a mixed rig repeated for every frame (Fc = 1 when all are static), and the cameras of read_cameras.
    Cameras with different frame counts are refused."""
    cams = read_cameras(calib_file, camera_keys)
    counts = sorted({camera_frames(c) for c in cams} - {None})
    if len(counts) > 1:
        raise ValueError(f'the cameras of {calib_file} have different numbers of calibration frames: {counts}')
    Fc = counts[0] if counts else 1
    P = np.empty((Fc, len(cams), 3, 4), dtype=np.float64)
    for c, cam in enumerate(cams):
        P[:, c] = np.array(camera_projections(cam))         # [1][3][4] of a static camera is broadcast
    return P, cams


def _refuse_per_frame(calib, what):
    for cam in camera_keys(calib):
        if np.ndim(calib[cam]['matrix']) == 3 or np.ndim(calib[cam]['rotation']) == 2:
            raise NotImplementedError(f'{what}: {PER_FRAME_REFUSAL} are served by calib.frame_projections and '
                                      'Engine.triangulate_frames only')


def retrieve_calib_params(calib_file):
    """common.py:254-288 (+ camera names, used by the recap at triangulation.py:284)."""
    calib = load_toml(calib_file)
    _refuse_per_frame(calib, 'retrieve_calib_params')
    out ={'S': [], 'K': [], 'dist': [], 'inv_K': [], 'optim_K': [], 'R': [], 'R_mat': [], 'T': [], 'names': []}
    for cam in camera_keys(calib):
        S = np.array(calib[cam]['size'], dtype=np.float64)
        K = np.array(calib[cam]['matrix'], dtype=np.float64)
        dist = np.array(calib[cam]['distortions'], dtype=np.float64)
        size = [int(s) for s in S]
        out['S'].append(S)
        out['K'].append(K)
        out['dist'].append(dist)
        out['optim_K'].append(cvmath.get_optimal_new_camera_matrix(K, dist, size, 1, size))
        out['inv_K'].append(np.linalg.inv(K))
        R = np.array(calib[cam]['rotation'], dtype=np.float64)
        out['R'].append(R)
        out['R_mat'].append(cvmath.rodrigues(R))
        out['T'].append(np.array(calib[cam]['translation'], dtype=np.float64))
        out['names'].append(calib[cam].get('name') if calib[cam].get('name') else cam)
    return out


def computeP(calib_file, undistort=False):
    """common.py:291-324: P = [K | 0] . [[R, T], [0, 1]] per camera (optim_K when undistorting)."""
    calib = load_toml(calib_file)
    _refuse_per_frame(calib, 'computeP')
    P = []
    for cam in camera_keys(calib):
        K = np.array(calib[cam]['matrix'], dtype=np.float64)
        if undistort:
            S = np.array(calib[cam]['size'])
            dist = np.array(calib[cam]['distortions'], dtype=np.float64)
            size = [int(s) for s in S]
            K = cvmath.get_optimal_new_camera_matrix(K, dist, size, 1, size)
        Kh = np.block([K, np.zeros(3).reshape(3, 1)])
        R = cvmath.rodrigues(np.array(calib[cam]['rotation'], dtype=np.float64))
        T = np.array(calib[cam]['translation'], dtype=np.float64)
        H = np.block([[R, T.reshape(3, 1)], [np.zeros(3), 1]])
        P.append(Kh @ H)
    return P


def find_calibration_file(session_dir):
    """triangulation.py:698-706 / personAssociation.py:677-685: newest *.toml of the first
    directory whose name contains 'calib'; same exception types and messages."""
    try:
        calib_dir = [os.path.join(session_dir, c) for c in os.listdir(session_dir)
                     if os.path.isdir(os.path.join(session_dir, c)) and 'calib' in c.lower()][0]
    except Exception:
        raise Exception('No .toml calibration direcctory found.')
    try:
        calib_files = glob.glob(os.path.join(calib_dir, '*.toml'))
        calib_file = max(calib_files, key=os.path.getctime)
    except Exception:
        raise Exception(f'No .toml calibration file found in the {calib_dir}.')
    return calib_file


def write_calibration_toml(path, cams, adjusted=False, error=0.0):
    """Write a calibration in the schema of calibration.py:1504-1533 (used by tests / demos, and by calib_refine with
    adjusted=True)."""
    with open(path, 'w') as f:
        for c in range(len(cams['K'])):
            name = cams['names'][c] if 'names' in cams else f'cam_{c + 1:02d}'
            K = np.asarray(cams['K'][c])
            f.write(f'[{name}]\n')
            f.write(f'name = "{name}"\n')
            f.write(f'size = [ {float(cams["S"][c][0])!r}, {float(cams["S"][c][1])!r}]\n')
            rows = ', '.join('[ ' + ', '.join(repr(float(v)) for v in row) + ']' for row in K)
            f.write(f'matrix = [ {rows}]\n')
            f.write('distortions = [ ' + ', '.join(repr(float(v)) for v in np.asarray(cams['dist'][c]).ravel()) + ']\n')
            f.write('rotation = [ ' + ', '.join(repr(float(v)) for v in np.asarray(cams['R'][c]).ravel()) + ']\n')
            f.write('translation = [ ' + ', '.join(repr(float(v)) for v in np.asarray(cams['T'][c]).ravel()) + ']\n')
            f.write('fisheye = false\n\n')
        f.write(f'[metadata]\nadjusted = {"true" if adjusted else "false"}\nerror = {float(error)!r}\n')
