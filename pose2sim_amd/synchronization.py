"""Synchronization stage: drop-in for the reference's ``synchronize_cams_all(config_dict)`` (synchronization.py:1346-1612)
for cameras that were not genlocked.

What runs where:

* reading the JSON files and choosing the person of every file (convert_json2pandas :1185-1250) .... host threads,
  p2s_json_parse + p2s_json_gather_largest_person
* interpolation, bfill / ffill, Butterworth filter, vertical speeds, filter of their sum (:1562-1585) ... p2s_sync_*
  kernels (Engine.sync_speeds)
* the lagged Pearson correlation of every camera with the reference camera, its argmax (:1291-1343) ... p2s_pearson
  kernels (Engine.lagged_pearson), every camera and every lag in one launch
* renaming and copying the JSON files into pose-sync/ (:1602-1612) ................................. host threads,
  p2s_copy_files (bytes and permission bits, as shutil.copy)

The interactive person picker (``synchronization_gui = true``) is a GUI matter and is refused with NotImplementedError.
Every other input gives the reference's offsets, pose-sync/ tree, log lines and exceptions.
"""
import fnmatch
import glob
import logging
import os
import re

import numpy as np

from . import poseio, skeletons
from . import trc as trc_mod


def _make_engine():
    from .engine import Engine
    return Engine(int(os.environ.get('LOCAL_RANK', '0')))


def _unbound_search_windows():
    """The UnboundLocalError the reference meets (:1537) when approx_time_maxspeed is neither a list nor 'auto', with
    this interpreter's own wording."""
    def meet():
        search_around_frames  # noqa: F821,B018
        search_around_frames = None  # noqa: F841
    try:
        meet()
    except UnboundLocalError as err:
        return err
    raise AssertionError('unreachable')


def _frame_rate(fps, project_dir, vid_img_extension):
    """:1396-1416: the configured rate, or for 'auto' the first video's (the 60-fps warning text and a value of 30 when it
    cannot be read).  The warning about a missing videos/ directory is logged whatever the rate."""
    video_dir = os.path.join(project_dir, 'videos')
    found = _glob(video_dir, vid_img_extension)
    if not found:
        try:
            for sub in os.listdir(video_dir):
                if os.path.isdir(os.path.join(video_dir, sub)):
                    found.append(_glob(os.path.join(video_dir, sub), vid_img_extension))
        except Exception:
            logging.warning(f'No video files nor image directories found in {video_dir}.')
    if fps != 'auto':
        return fps
    rate = trc_mod.mp4_frame_rate(found[0]) if found and isinstance(found[0], str) else None
    if not rate:
        logging.warning('Cannot read video. Frame rate will be set to 60 fps.')
        return 30
    return round(rate)


def _glob(directory, extension):
    return glob.glob(os.path.join(directory, '*' + extension))


def _considered_names(keypoints_to_consider, names):
    """:1500-1508 -> the names, or raises the reference's ValueError."""
    if keypoints_to_consider == 'right':
        return [n for n in names if n.startswith('R') or n.startswith('right')]
    if keypoints_to_consider == 'left':
        return [n for n in names if n.startswith('L') or n.startswith('left')]
    if keypoints_to_consider == 'all':
        return list(names)
    if not isinstance(keypoints_to_consider, list):
        raise ValueError('keypoints_to_consider should be "all", "right", "left", or a list of keypoint names.\n'
                         '                        If you specified keypoints, make sure that they exist in your pose_model.')
    return keypoints_to_consider


def _search_windows(approx_time_maxspeed, lag_range, fps, nb_frames_per_cam, f_range, cam_nb):
    """:1478-1496: [start, end) frames of every camera (None: approx_time_maxspeed is neither a list nor 'auto')."""
    if isinstance(approx_time_maxspeed, list):
        if len(approx_time_maxspeed) == 1 and cam_nb > 1:
            approx_time_maxspeed *= cam_nb                   # in place, as the reference (the config's list grows)
        windows = []
        for i, frame in enumerate(int(fps * t) for t in approx_time_maxspeed):
            lo, hi = frame - lag_range, frame + lag_range
            start, end = max(int(lo), 0), min(int(hi), nb_frames_per_cam[i] + f_range[0])
            if start != lo:
                logging.warning(f'Frame range start adjusted for camera {i}: {lo} -> {start}')
            if end != hi:
                logging.warning(f'Frame range end adjusted for camera {i}: {hi} -> {end}')
            windows.append([start, end])
        return windows
    if approx_time_maxspeed == 'auto':
        return [[f_range[0], f_range[0] + n] for n in nb_frames_per_cam]
    return None


def _save_plot(path, ref_speed, cam_speed, lags, r, argmax, offset, max_corr, ref_cam_name, cam_name):
    """The figure of time_lagged_cross_corr (:1320-1333), drawn from the engine's r curve without pyplot (never shown,
    never blocking)."""
    from matplotlib.figure import Figure
    fig = Figure()
    ax = fig.subplots(2, 1)
    ax[0].plot(np.arange(len(ref_speed)), ref_speed, label=f'Reference: {ref_cam_name}')
    ax[0].plot(np.arange(len(cam_speed)), cam_speed, label=f'Compared: {cam_name}')
    ax[0].set(xlabel='Frame', ylabel='Speed (px/frame)')
    ax[0].legend()
    ax[1].plot(lags, r)
    ax[1].axvline(np.ceil(len(r) / 2) + lags[0], color='k', linestyle='--')
    ax[1].axvline(argmax + lags[0], color='r', linestyle='--', label='Peak synchrony')
    ax[1].annotate(f'Max correlation={np.round(max_corr, 2)}', xy=(0.05, 0.9), xycoords='axes fraction')
    ax[1].set(title=f'Offset = {offset} frames', xlabel='Offset (frames)', ylabel='Pearson r')
    ax[1].legend()
    fig.tight_layout()
    fig.savefig(path)


def synchronize_cams_all(config_dict, engine=None):
    """Offsets of every camera against the one with the fewest JSON files, from the correlation of their vertical
    keypoint speeds, and the renumbered copies of every JSON file in pose-sync/."""
    project_dir = config_dict.get('project').get('project_dir')
    pose_dir = os.path.realpath(os.path.join(project_dir, 'pose'))
    sync_dir = os.path.abspath(os.path.join(pose_dir, '..', 'pose-sync'))
    os.makedirs(sync_dir, exist_ok=True)
    sync_cfg = config_dict.get('synchronization')
    if sync_cfg.get('synchronization_gui'):
        raise NotImplementedError('synchronization_gui = true (the interactive person picker) is outside the scope of this '
                                  'engine; set it to false, or run that stage with the reference.')
    pose_model = config_dict.get('pose').get('pose_model')
    frame_range = config_dict.get('project').get('frame_range')
    save_plots = sync_cfg.get('save_sync_plots', True)
    keypoints_to_consider = sync_cfg.get('keypoints_to_consider')
    approx_time_maxspeed = sync_cfg.get('approx_time_maxspeed')
    time_range_around_maxspeed = sync_cfg.get('time_range_around_maxspeed')
    likelihood_threshold = sync_cfg.get('likelihood_threshold')
    filter_cutoff = int(sync_cfg.get('filter_cutoff'))
    filter_order = int(sync_cfg.get('filter_order'))

    fps = _frame_rate(config_dict.get('project').get('frame_rate'), project_dir, config_dict['pose']['vid_img_extension'])
    lag_range = time_range_around_maxspeed * fps
    keypoints_ids, keypoints_names, _ = skeletons.keypoints(pose_model, config_dict)

    # the cameras' JSON directories and files (:1440-1456)
    try:
        listed = next(os.walk(pose_dir))[1]
        os.listdir(os.path.join(pose_dir, listed[0]))[0]
    except Exception:
        raise ValueError(f'No json files found in {pose_dir} subdirectories. Make sure you run Pose2Sim.poseEstimation() first.')
    json_dirs_names = [d for d in poseio.sort_stringlist_by_last_number(listed) if 'json' in d]
    json_files_names = [poseio.sort_stringlist_by_last_number(fnmatch.filter(os.listdir(os.path.join(pose_dir, d)), '*.json'))
                        for d in json_dirs_names]
    nb_frames_per_cam = [len(files) for files in json_files_names]
    cam_nb = len(json_dirs_names)
    cam_names = [d.split('_')[0] for d in json_dirs_names]
    f_range = [0, min(nb_frames_per_cam)] if frame_range in ('all', 'auto', []) else frame_range

    windows = _search_windows(approx_time_maxspeed, lag_range, fps, nb_frames_per_cam, f_range, cam_nb)
    considered = _considered_names(keypoints_to_consider, keypoints_names)

    logging.info('Synchronizing...')
    from scipy import signal
    b, a = signal.butter(int(filter_order / 2), filter_cutoff / (fps / 2), 'low', analog=False)
    zi = signal.lfilter_zi(b, a)
    if windows is None:
        raise _unbound_search_windows()
    in_window = [[f for f in files if poseio.frame_of(f) in range(*w)] for files, w in zip(json_files_names, windows)]
    if any(not files for files in in_window):
        raise ValueError(f'No json files found within the specified frame range ({frame_range}) at the times '
                         f'{approx_time_maxspeed} +/- {time_range_around_maxspeed} s.')
    positions = [p for p, name in enumerate(keypoints_names) if name in considered]

    if isinstance(approx_time_maxspeed, list):
        logging.info(f'Synchronization is calculated around the times {approx_time_maxspeed} +/- {time_range_around_maxspeed} s.')
    else:
        logging.info('Synchronization is calculated on the whole sequence. This may take a while.')
    logging.info(f'\nKeypoints used to compute the best synchronization offset: {considered}.')
    logging.info(f'These keypoints are filtered with a Butterworth filter (cut-off frequency: {filter_cutoff} Hz, order: {filter_order}).')
    logging.info(f'They are removed when their likelihood is below {likelihood_threshold}.\n')

    # person of every file, per camera (one parse of every file of every window)
    from .ingest import JsonBatch
    paths = [os.path.join(pose_dir, d, f) for d, files in zip(json_dirs_names, in_window) for f in files]
    with JsonBatch(paths) as batch:
        xyl = batch.gather_largest_person(keypoints_ids, likelihood_threshold)
    per_cam = np.split(xyl, np.cumsum([len(files) for files in in_window])[:-1])

    padlen = 3 * (max(len(a), len(b)) - 1)
    coords = []
    for i, cam in enumerate(per_cam):
        if np.isnan(cam).all():
            msg = ('No valid coordinates found in the JSON files. There may be a mismatch between the "pose_model" specified '
                   'for pose estimation and for synchronization. If not, make sure that your likelihood_threshold for '
                   'synchronization is not set too high.')
            logging.error(msg)
            raise ValueError(msg)
        n = cam.shape[0]
        if n > padlen:
            if n <= 3 * max(len(a), len(b)):
                raise ValueError(f'The length of the input vector x must be greater than padlen, which is {3 * max(len(a), len(b))}.')
        else:
            logging.warning(f'Camera {i}: insufficient number of samples ({n} < {padlen + 1}) to apply the Butterworth filter. '
                            'Data will remain unfiltered.')
        coords.append(np.ascontiguousarray(cam[:, positions, :2].reshape(n, -1)))
    for i, cam in enumerate(coords):
        n = cam.shape[0]
        if n < 2:
            raise IndexError('single positional indexer is out-of-bounds')            # df_diff.iloc[1], :1284
        if n <= padlen:
            # unfiltered, the columns keep their labels 2 p, 2 p + 1 and vert_speed reads labels 1, 3, ... (:1285)
            missing = [2 * k + 1 for k in range(len(positions)) if positions[k] != k]
            if missing:
                raise KeyError(missing[0])
            logging.warning(f'Camera {i}: insufficient number of samples ({n} < {padlen + 1}) to apply the Butterworth filter. '
                            'Data will remain unfiltered.')

    engine = engine or _make_engine()
    speeds = engine.sync_speeds(coords, b, a, zi)

    # offsets against the camera with the fewest files (:1588-1600)
    ref_cam_id = nb_frames_per_cam.index(min(nb_frames_per_cam))
    ref_cam_name = cam_names[ref_cam_id]
    half = int(len(coords[ref_cam_id]) / 2)
    others = [c for c in range(cam_nb) if c != ref_cam_id]
    r, argmax, max_corr = engine.lagged_pearson(speeds[ref_cam_id], [speeds[c] for c in others], -half, half)
    offset = [0] * cam_nb
    logging.info('')
    plotting = bool(save_plots)
    if plotting:
        try:
            import matplotlib  # noqa: F401
        except ImportError:
            logging.warning('matplotlib is not importable: the synchronization plots are not saved.')
            plotting = False
    for j, cam_id in enumerate(others):
        cam_name = cam_names[cam_id]
        if np.isnan(r[j]).all():
            section, corr = 0, 0
        else:
            section, corr = int(half - argmax[j]), np.float64(max_corr[j])
            if plotting:
                _save_plot(os.path.join(sync_dir, f'sync_{ref_cam_name}_vs_{cam_name}.png'), speeds[ref_cam_id], speeds[cam_id],
                           np.arange(-half, half), r[j], int(argmax[j]), section, corr, ref_cam_name, cam_name)
        offset_cam = section - (windows[ref_cam_id][0] - windows[cam_id][0])
        if isinstance(approx_time_maxspeed, list):
            logging.info(f'--> Camera {ref_cam_name} and {cam_name}: {offset_cam} frames offset ({section} on the selected section), correlation {round(corr, 2)}.')
        else:
            logging.info(f'--> Camera {ref_cam_name} and {cam_name}: {offset_cam} frames offset, correlation {round(corr, 2)}.')
        offset[cam_id] = offset_cam
    if save_plots:
        logging.info(f'Synchronization plots saved in {sync_dir}.')

    # every file of every camera, renumbered by its offset, into pose-sync/ (:1602-1612)
    pairs = []
    for d, name in enumerate(json_dirs_names):
        os.makedirs(os.path.join(sync_dir, name), exist_ok=True)
        for f in json_files_names[d]:
            parts = re.split(r'(\d+)', f)
            parts[-2] = f'{int(parts[-2]) - offset[d]:06d}'
            if int(parts[-2]) > 0:
                pairs.append((os.path.join(pose_dir, name, f), os.path.join(sync_dir, name, ''.join(parts))))
    from .ingest import copy_files
    copy_files(pairs)
    logging.info(f'Synchronized json files saved in {sync_dir}.')
    return offset
