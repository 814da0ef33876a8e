"""A .trc back onto the image planes: mirror of Pose2Sim/Utilities/reproj_from_trc_calib.py.

3D markers and a calibration TOML in; per-camera 2D keypoints out, as OpenPose JSON folders (-o), a COCO / MMPose JSON
(-m) or DeepLabCut csv / h5 tables (-d).  Everything per (frame, marker, camera) -- the projection, the rounding to one
decimal, the out-of-image mask -- is one call of the HIP engine (Engine.reproject, csrc/p2s_reproj.hip), and the
OpenPose files come from its native writer; there is no NumPy path for either.  The MMPose and DeepLabCut writers (one
file per camera) stay on the host.

The reference's contract is kept, including what looks accidental (each item is recorded in tests/golden/reproj_units.npz):
* the output root defaults to the .trc path with '.trc' replaced by '_reproj'; camera folders are cam<position>_json, not
  the calibration's names; the folder creation stops at the first folder that already exists;
* frames are numbered from 0 by row; with per-frame cameras the number of frames is min(calibration frames, rows);
  cameras with different frame counts end in NumPy's ValueError for a ragged list; with a camera folder missing the
  call ends in FileNotFoundError after the earlier cameras' files;
* only the table named 'metadata' is skipped in the calibration (calib.camera_keys skips four names; this utility follows
  the reference's rule for this file);
* DeepLabCut: DataFrame.to_hdf runs before any csv is written, so without pytables pandas' ImportError ends the call.

Refused with NotImplementedError: undistort_points together with per-frame cameras (the reference hands the whole
per-frame rotation array to cv2.projectPoints), the marker sets halpe26 / halpeplus / biocvplus (their orders are
name tables of the reference's program; the default, the file's own order, covers the .trc files this engine writes),
and a .trc that names a marker twice (the reference lets pandas rename the columns).  A NumMarkers that disagrees with the
label row is refused with ValueError: the engine's tables are rectangular, [frames][markers].  Neither happens in a .trc
this project or the reference writes.
With undistort_points the arithmetic is cvmath.project_points, this project's restatement of cv2.projectPoints: parity
with OpenCV itself is unpinned, as everywhere in this project.
"""
import argparse
import errno
import hashlib
import json
import os
import warnings

import numpy as np
import pandas as pd

from . import calib, cvmath, trc

NAMED_MARKERSETS = ('halpe26', 'halpeplus', 'biocvplus')
NO_FORMAT = 'Output_format must be specified either "openpose" (-o), "deeplabcut" (-d), or "mmpose" (-m)'
BBOX_PADDING = 0.05


def main():
    parser = argparse.ArgumentParser(description='Reproject the markers of a .trc file onto the cameras of a calibration file')
    parser.add_argument('-t', '--input_trc_file', required=True, help='.trc file with the 3D markers')
    parser.add_argument('-c', '--input_calib_file', required=True, help='calibration .toml file')
    for short, name, what in (('-o', 'openpose', 'one OpenPose json file per camera and frame'),
                              ('-d', 'deeplabcut', 'DeepLabCut csv and h5 tables, one per camera'),
                              ('-m', 'mmpose', 'one COCO / MMPose json file per camera'),
                              ('-u', 'undistort_points', 'project with the distortion coefficients')):
        parser.add_argument(short, '--' + name, required=False, action='store_true', help=what)
    parser.add_argument('-s', '--markerset', required=False, help='marker order; only the file\'s own order is available')
    parser.add_argument('-O', '--output_file_root', required=False, help='output folder (default: <trc>_reproj)')
    reproj_from_trc_calib_func(**vars(parser.parse_args()))


def name_id(name, digits=12):
    """int(md5(name)) mod 10^digits: the image and annotation ids of the MMPose file."""
    return int(hashlib.md5(name.encode()).hexdigest(), 16) % 10 ** digits


def read_markers(trc_path):
    """-> (marker names from the label row, NumMarkers from the header, Q [rows][K][3] in the Z-up frame)."""
    _, _, coords, names, header = trc.load_trc(trc_path)
    facts = dict(zip(header[1].rstrip('\n').split('\t'), header[2].rstrip('\n').split('\t')))
    n_markers = int(float(facts['NumMarkers']))
    if n_markers != len(names):
        raise ValueError(f'NumMarkers is {n_markers} but the label row names {len(names)} markers')
    # a row holds (Y, Z, X) per marker (trc.yup_columns): back to (X, Y, Z)
    Q = coords.reshape(len(coords), len(names), 3)[:, :, [2, 0, 1]]
    return names, n_markers, np.ascontiguousarray(Q)


def read_cameras(calib_path):
    """Every table but 'metadata' -> per camera: size, K ([3][3] or [Fp][3][3]), dist, rotation vector(s), translation(s)
    (calib.read_cameras, the reader triangulation shares)."""
    return calib.read_cameras(calib_path)


projection_matrices = calib.projection_matrices


def labels_table(uv_cam, image_names, markers):
    """The DeepLabCut table of one camera: rows = image names, four-level columns scorer / individuals / bodyparts / coords."""
    columns = pd.MultiIndex.from_product([['DavidPagnon'], ['person0'], markers, ['x', 'y']],
                                         names=['scorer', 'individuals', 'bodyparts', 'coords'])
    return pd.DataFrame(uv_cam.reshape(len(image_names), -1), index=pd.MultiIndex.from_product([image_names]), columns=columns)


def mmpose_document(uv_cam, image_names, size, markerset, marker_index):
    """The COCO / MMPose dictionary of one camera from uv_cam [F][K][2]."""
    w, h = int(size[0]), int(size[1])
    doc = {'info': {'description': f'Bedlam Pose {markerset}', 'url': 'https://github.com/davidpagnon/bedlam_pose', 'version': '0.1',
                    'year': 2024, 'contributor': 'David Pagnon', 'date_created': '2024/08/14'},
           'licenses': [{'url': 'https://bedlam.is.tue.mpg.de/license.html', 'id': 1, 'name': 'Non-commercial scientific research purposes'},
                        {'url': 'https://creativecommons.org/licenses/by/4.0/deed.en', 'id': 2, 'name': 'Attribution License'}],
           'images': [], 'annotations': [], 'categories': [{'id': 1, 'name': 'person'}]}
    for f, name in enumerate(image_names):
        image_id = name_id(name)
        doc['images'].append({'file_name': name, 'height': h, 'width': w, 'id': image_id, 'license': 1})
        keypoints = []
        for k in marker_index:
            x, y = uv_cam[f, k]
            keypoints += [0.0, 0.0, 0] if (np.isnan(x) or np.isnan(y)) else [float(x), float(y), 2]
        with warnings.catch_warnings():
            warnings.simplefilter('ignore', RuntimeWarning)         # a frame without a visible marker: all-NaN minima
            x0, y0 = np.nanmin(uv_cam[f, :, 0]), np.nanmin(uv_cam[f, :, 1])
            x1, y1 = np.nanmax(uv_cam[f, :, 0]), np.nanmax(uv_cam[f, :, 1])
        bw, bh = np.round(x1 - x0, decimals=1), np.round(y1 - y0, decimals=1)
        pad = BBOX_PADDING
        bbox = [max(0, x0 - bw * pad), max(0, y0 - bh * pad),
                bw * (1 + pad * 2) if x1 + bw * pad < w else bw * (1 + pad),
                bh * (1 + pad * 2) if y1 + bh * pad < h else bh * (1 + pad)]
        if np.isnan(bbox).any():
            continue
        doc['annotations'].append({'keypoints': keypoints, 'num_keypoints': len(marker_index), 'bbox': bbox,
                                   'id': name_id('person0' + name), 'image_id': image_id, 'category_id': 1,
                                   'segmentation': [[x0, y0, x0, y1, x1, y1, x1, y0]],
                                   'area': np.round(bw * bh, decimals=1), 'iscrowd': 0})
    return doc


def reproj_from_trc_calib_func(engine=None, **args):
    """input_trc_file, input_calib_file, openpose / deeplabcut / mmpose (at least one), markerset, undistort_points,
    output_file_root: the reference's arguments.  engine: an Engine (default: one on GPU 0)."""
    trc_path = os.path.realpath(args.get('input_trc_file'))
    calib_path = os.path.realpath(args.get('input_calib_file'))
    formats = {k: args.get(k) for k in ('openpose', 'deeplabcut', 'mmpose')}
    markerset = args.get('markerset')
    undistort = args.get('undistort_points')
    out_root = args.get('output_file_root')
    if out_root is None:
        out_root = trc_path.replace('.trc', '_reproj')
    if not any(formats.values()):
        raise ValueError(NO_FORMAT)
    if markerset in NAMED_MARKERSETS:
        raise NotImplementedError(f'markerset {markerset!r}: the named marker orders are not part of this project; leave it out to '
                                  'keep the order of the .trc file')
    if engine is None:
        from .filtering import _make_engine
        engine = _make_engine()

    markers, n_markers, Q = read_markers(trc_path)
    if len(set(markers)) != len(markers):
        raise NotImplementedError('the .trc file names a marker twice')
    stem = os.path.splitext(os.path.basename(trc_path))[0]
    cams = read_cameras(calib_path)
    P, per_frame = projection_matrices(cams)
    if undistort and per_frame:
        raise NotImplementedError(calib.UNDISTORT_PER_FRAME)
    sizes = np.array([cam['S'][:2] for cam in cams], dtype=np.float64).reshape(len(cams), 2)

    reproj_dir = os.path.realpath(out_root)
    cam_dirs = [os.path.join(reproj_dir, f'cam{c + 1:02d}_json') for c in range(len(cams))]
    if not os.path.exists(reproj_dir):
        os.mkdir(reproj_dir)
    for cam_dir in cam_dirs:                # stops at the first folder that cannot be made, e.g. one that exists
        try:
            os.mkdir(cam_dir)
        except Exception:
            break

    n_frames = len(Q) if P.shape[1] == 1 else min(P.shape[1], len(Q))
    image_names = [os.path.join(os.path.splitext(trc_path)[0], f'img_{f:03d}.jpg') for f in range(n_frames)]
    if undistort:
        cal = {'K': [c['K'] for c in cams], 'dist': [c['dist'] for c in cams], 'T': [c['T'] for c in cams],
               'R_mat': [cvmath.rodrigues(c['R']) for c in cams]}
        uv = engine.reproject(Q[:n_frames], cal=cal, sizes=sizes)
    else:
        uv = engine.reproject(Q[:n_frames], P=P[:, :n_frames], sizes=sizes)
    marker_index = np.arange(n_markers, dtype=np.int32)

    if formats['deeplabcut']:
        tables = [labels_table(uv[c], image_names, markers) for c in range(len(cams))]
        for c, cam_dir in enumerate(cam_dirs):
            tables[c].to_hdf(os.path.join(cam_dir, f'{stem}_cam_{c + 1:02d}_dlc.h5'), index=True, key='reprojected_points')
        for c, cam_dir in enumerate(cam_dirs):
            tables[c].to_csv(os.path.join(cam_dir, f'{stem}_cam_{c + 1:02d}_dlc.csv'), sep=',', index=True, lineterminator='\n')
    if formats['mmpose']:
        for c, cam_dir in enumerate(cam_dirs):
            with open(os.path.join(cam_dir, f'{stem}_cam_{c + 1:02d}_mmpose.json'), 'w') as fh:
                json.dump(mmpose_document(uv[c], image_names, sizes[c], markerset, marker_index), fh)
    if formats['openpose']:
        # the reference writes camera by camera and stops with FileNotFoundError at the first camera without a folder
        n_ready = next((c for c, cam_dir in enumerate(cam_dirs) if not os.path.isdir(cam_dir)), len(cam_dirs))
        engine.write_openpose_files(cam_dirs[:n_ready], stem, uv[:n_ready], marker_index)
        if n_ready < len(cam_dirs):
            raise FileNotFoundError(errno.ENOENT, os.strerror(errno.ENOENT),
                                    os.path.join(cam_dirs[n_ready], f'{stem}_cam{n_ready + 1:02d}_openpose_0000.json'))
    print(f'Reprojected points saved at {out_root}.')


if __name__ == '__main__':
    main()
