"""2D confidence analysis: mirror of Pose2Sim/Utilities/pose_confidence_analyze.py.

Per camera and keypoint, over the frames that hold a person: mean, median, standard deviation, extremes and the 5 / 25 / 75 /
95 % percentiles of the detector's confidence, the share below the likelihood threshold, the share in each of five bands
(below 0.4, 0.4-0.6 "danger", 0.6-0.8, 0.8-1.0, 1.0 and above) and the share a higher threshold would exclude.  Written:
confidence_statistics.csv, confidence_band_distribution.csv and the console report.

The JSON files of a camera are parsed in one batch by the native ingest (JsonBatch); every statistic comes from one call
of the HIP engine for all cameras (Engine.confidence_stats, csrc/p2s_confidence.hip), float64 and bit for bit the
reference's: np.mean and np.std are summed in NumPy's own order on the GPU, the percentiles are exact order statistics.
There is no NumPy path for them.  The host forms the rates (a count divided by a count) and the report's averages over
26 or fewer numbers (np.nanmean of the cameras' means, np.mean of 26 rates), as the reference does.

Kept from the reference, each recorded in tests/golden/confidence_units.npz: only folders named cam*_json are cameras; the
camera name is the folder name with every '_json' removed; the person is the FIRST one listed, not a tracked one; a list
longer than 78 numbers is cut to 26 keypoints, a shorter one raises IndexError, a person without the list KeyError; a
confidence of exactly 1.0 counts in two bands, a negative one in none; all cameras are loaded before anything but the
first line is printed.  The two PNG heatmaps are not produced, with or without no_plot: the numbers they are drawn from
are in the returned dictionary.

Outside the reference's contract, refused with ValueError naming the file before anything is written: an unreadable or
non-JSON file, a keypoint list holding anything but numbers.
"""
import argparse
import csv
import glob
import os
import warnings
from pathlib import Path

import numpy as np

from . import _lib
from .keypoint_jitter_analyze import KEYPOINT_NAMES, N_KPTS

DEFAULT_THRESHOLD = 0.4
SIMULATED_THRESHOLDS = (0.4, 0.5, 0.6)
STAT_NAMES = ('mean', 'median', 'std', 'min', 'max', 'p5', 'p25', 'p75', 'p95')     # the engine's order
BANDS = (('low', '<0.4'), ('danger', '0.4-0.6'), ('medium', '0.6-0.8'), ('high', '0.8-1.0'), ('very_high', '>1.0'))   # the engine's order
BAND_NAMES = [name for name, _ in BANDS]
N_PROBLEM = max(1, N_KPTS // 4)
N_HOT_SPOTS = 10


def camera_name(cam_dir):
    return Path(cam_dir).name.replace('_json', '')


def load_confidences(cam_json_dir):
    """-> [n_files][26]: the confidences of the first person of every file of the camera, NaN rows where there is none."""
    from .ingest import JsonBatch
    files = sorted(glob.glob(os.path.join(glob.escape(str(cam_json_dir)), '*.json')))
    if not files:
        raise FileNotFoundError(f'No JSON files found in {cam_json_dir}')
    table = np.full((len(files), N_KPTS), np.nan)
    with JsonBatch(files) as batch:
        has_person = batch.counts > 0
        first = batch.person_lengths[batch.person_base[:-1][has_person]]      # of people[0] of the files that hold one
        # the first file the reference, or the parser, would stop at
        stop = (batch.counts == _lib.P2S_JSON_UNREADABLE)
        stop[has_person] |= first < 3 * N_KPTS
        if stop.any():
            i = int(np.flatnonzero(stop)[0])
            if batch.counts[i] == _lib.P2S_JSON_UNREADABLE:
                raise ValueError(f'{files[i]} cannot be read as JSON')
            length = int(batch.person_lengths[batch.person_base[i]])
            if length == _lib.P2S_JSON_PERSON_NOT_NUMERIC:
                raise ValueError(f'{files[i]} does not hold OpenPose people with lists of numbers')
            if length == _lib.P2S_JSON_PERSON_NO_LIST:
                raise KeyError('pose_keypoints_2d')
            raise IndexError('list index out of range')
        rows = np.flatnonzero(has_person)
        if len(rows):
            values, _ = batch.gather_people(rows, np.zeros(len(rows), dtype=np.int32), 3 * N_KPTS)
            table[rows] = values[:, 2::3]
    return table


def load_pose_data(pose_dir):
    """-> {camera name: [n_frames][26]} of the cam*_json folders of pose_dir, in sorted folder order."""
    pose_dir = Path(pose_dir)
    cam_dirs = sorted(pose_dir.glob('cam*_json'))
    if not cam_dirs:
        raise FileNotFoundError(f'No cam*_json directories found in {pose_dir}')
    return {camera_name(d): load_confidences(d) for d in cam_dirs}


def results(res, names, thresholds, threshold):
    """The reference's three dictionaries, Python floats and ints, from Engine.confidence_stats' tables."""
    t0 = thresholds.index(threshold)
    statistics, band_dist = {}, {}
    for c, cam in enumerate(names):
        statistics[cam], band_dist[cam] = {}, {}
        for k in range(res['stats'].shape[1]):
            s = dict(zip(STAT_NAMES, (float(v) for v in res['stats'][c, k])))
            s['below_threshold_rate'] = float(res['below_rate'][t0, c, k])    # NaN without entries
            statistics[cam][k] = s
            band_dist[cam][k] = {b: {'count': int(res['bands'][c, k, i]), 'rate': float(res['band_rate'][c, k, i])}
                                 for i, b in enumerate(BAND_NAMES)}
    empty = res['counts'] == 0
    sim = {th: {cam: {k: 0.0 if empty[c, k] else float(res['below_rate'][t, c, k]) for k in range(empty.shape[1])}
                for c, cam in enumerate(names)} for t, th in enumerate(thresholds)}
    return statistics, band_dist, sim


def format_report(n_frames, statistics, band_dist, threshold_sim, threshold):
    cameras = sorted(statistics)
    kpts = range(N_KPTS)
    out = ['=== 2D Keypoint Confidence Analysis ===',
           f'Cameras: {len(cameras)} ({", ".join(cameras)})',
           f'Total frames: {sum(n_frames.values())}',
           f'Threshold: {threshold}', '',
           '--- Analysis 1: Mean Confidence per Camera x Keypoint ---']
    head = f'{"Keypoint":<14}' + ''.join(f'{c:>8}' for c in cameras) + f'{"avg":>8}'
    out += [head, '-' * len(head)]
    means = [[statistics[c][k]['mean'] for c in cameras] for k in kpts]
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')                               # a keypoint no camera ever saw: nan
        avgs = [np.nanmean(row) for row in means]
    for k in kpts:
        out.append(f'{KEYPOINT_NAMES[k]:<14}' + ''.join(f'{m:>8.3f}' for m in means[k]) + f'{avgs[k]:>8.3f}')
    out += ['', f'--- Low Confidence Keypoints (bottom {N_PROBLEM}) ---']
    for k in sorted(kpts, key=lambda k: avgs[k])[:N_PROBLEM]:             # stable: the first keypoint on ties
        per_cam = '  '.join(f'{c}={m:.3f}' for c, m in zip(cameras, means[k]))
        out.append(f'  {KEYPOINT_NAMES[k]:<14} avg={avgs[k]:.3f}  ({per_cam})')
    out += ['', '--- Analysis 2: Confidence Band Distribution (per camera, all keypoints) ---']
    head = f'{"Camera":<8}' + ''.join(f'{label:>10}' for _, label in BANDS)
    out += [head, '-' * len(head)]
    for c in cameras:
        per_band = [sum(band_dist[c][k][b]['count'] for k in kpts) for b in BAND_NAMES]
        total = sum(per_band)                                         # a confidence of 1.0 is in it twice
        out.append(f'{c:<8}' + ''.join(f'{(n / total * 100 if total > 0 else 0):>9.1f}%' for n in per_band))
    out += ['', f'--- Danger Zone (0.4-0.6) Hot Spots (top {N_HOT_SPOTS}) ---']
    spots = [(c, k, band_dist[c][k]['danger']['rate']) for c in cameras for k in kpts]
    for c, k, rate in sorted((s for s in spots if s[2] > 0), key=lambda s: -s[2])[:N_HOT_SPOTS]:
        out.append(f'  {c}:{KEYPOINT_NAMES[k]:<14} {rate * 100:>5.1f}%')
    out += ['', '--- Threshold Simulation ---']
    ordered = sorted(threshold_sim)
    base = ordered[0] if ordered else threshold
    for th in ordered:
        if th == base:
            continue
        parts = []
        for c in cameras:
            gain = np.mean([threshold_sim[th][c][k] for k in kpts]) - np.mean([threshold_sim[base][c][k] for k in kpts])
            parts.append(f'{c}: +{gain * 100:.1f}%')
        out.append(f'  {base} -> {th}  additional exclusion:  {", ".join(parts)}')
    out.append('')
    return '\n'.join(out)


def save_csv(statistics, band_dist, output_dir):
    output_dir = Path(output_dir)
    output_dir.mkdir(parents=True, exist_ok=True)
    path = output_dir / 'confidence_statistics.csv'
    columns = STAT_NAMES + ('below_threshold_rate',)
    with open(path, 'w', newline='') as fh:
        writer = csv.writer(fh)
        writer.writerow(('camera', 'keypoint') + columns)
        for cam in sorted(statistics):
            for k, name in enumerate(KEYPOINT_NAMES):
                writer.writerow([cam, name] + [f'{statistics[cam][k][col]:.4f}' for col in columns])
    print(f'Statistics CSV saved: {path}')
    path = output_dir / 'confidence_band_distribution.csv'
    with open(path, 'w', newline='') as fh:
        writer = csv.writer(fh)
        writer.writerow(['camera', 'keypoint'] + [f'{b}_{what}' for b in BAND_NAMES for what in ('count', 'rate')])
        for cam in sorted(band_dist):
            for k, name in enumerate(KEYPOINT_NAMES):
                cells = band_dist[cam][k]
                writer.writerow([cam, name] + [v for b in BAND_NAMES for v in (cells[b]['count'], f'{cells[b]["rate"]:.4f}')])
    print(f'Band distribution CSV saved: {path}')


def analyze_confidence(pose_dir, threshold=DEFAULT_THRESHOLD, output=None, no_plot=False, engine=None):
    """-> {'statistics': {camera: {keypoint index: {'mean', 'median', 'std', 'min', 'max', 'p5', 'p25', 'p75', 'p95',
    'below_threshold_rate'}}}, 'band_distribution': {camera: {keypoint index: {band: {'count', 'rate'}}}},
    'threshold_simulation': {threshold: {camera: {keypoint index: share excluded}}}}, as the reference returns it.
    no_plot is accepted and changes nothing: no figure is drawn.  engine: an Engine (default: Engine(0))."""
    pose_dir = Path(pose_dir)
    output_dir = pose_dir / 'confidence_analysis' if output is None else Path(output)
    print(f'Loading pose data from {pose_dir} ...')
    tables = load_pose_data(pose_dir)
    thresholds = sorted({threshold, *SIMULATED_THRESHOLDS})
    if engine is None:
        from .engine import Engine
        engine = Engine(0)
    names = list(tables)
    res = engine.confidence_stats([tables[n] for n in names], thresholds)
    for name in names:
        print(f'  {name}: {len(tables[name])} frames')
    statistics, band_dist, threshold_sim = results(res, names, thresholds, threshold)
    print(format_report({n: len(t) for n, t in tables.items()}, statistics, band_dist, threshold_sim, threshold))
    save_csv(statistics, band_dist, output_dir)
    return {'statistics': statistics, 'band_distribution': band_dist, 'threshold_simulation': threshold_sim}


def main():
    parser = argparse.ArgumentParser(description='Analyze the confidence of 2D pose estimates per camera and keypoint: finds the '
                                                 'cameras and keypoints too uncertain, or too close to the threshold, to triangulate well.')
    parser.add_argument('-p', '--pose-dir', required=True, help='pose folder holding the cam*_json camera folders')
    parser.add_argument('-t', '--threshold', type=float, default=DEFAULT_THRESHOLD, help=f'likelihood threshold in use (default: {DEFAULT_THRESHOLD})')
    parser.add_argument('-o', '--output', default=None, help='output folder (default: <pose_dir>/confidence_analysis/)')
    parser.add_argument('--no-plot', action='store_true', help='accepted; no figure is drawn either way')
    args = parser.parse_args()
    analyze_confidence(pose_dir=args.pose_dir, threshold=args.threshold, output=args.output, no_plot=args.no_plot)


if __name__ == '__main__':
    main()
