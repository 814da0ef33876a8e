"""2D keypoint jitter analysis: mirror of Pose2Sim/Utilities/keypoint_jitter_analyze.py.

Per camera and keypoint: the frame-to-frame displacement of the tracked person, a threshold from the column's median
(median x multiplier, 10 px where the median is 0), and the list of the jumps above it, each with a guessed cause --
A the person's box touches the image border, C the box is less than half its median area, D the keypoint's confidence
is below 0.3, E none of these.  Written: jitter_events.csv, phase1_results.md and the console report.

The JSON files of a camera are parsed in one batch by the native ingest and the person is chosen there
(JsonBatch.select_tracked_person); every number after that -- displacements, box areas, the exact medians, thresholds,
the event mask, the ordered event list and its patterns -- comes from one call of the HIP engine for all cameras
(Engine.jitter, csrc/p2s_jitter.hip), float64 and bit for bit the reference's.  There is no NumPy path.

Kept from the reference, each recorded in tests/golden/jitter_units.npz: the folder search (cam*_json, then *_json, then
the folder itself); the camera name with every '_json' removed when the folder name ends in it; frames numbered by the
position of the file in the sorted listing; cameras reported in sorted-name order but events in folder order; a
keypoint list longer than 78 numbers ends the run with NumPy's reshape ValueError; phase1_results.md goes beside a
folder named test_results and inside any other.  The four PNG figures are not produced, with or without no_plot: the
arrays they are drawn from are in the returned dictionary.

Outside the reference's contract, refused with ValueError naming the file before anything is written: an unreadable or
non-JSON file, a top level that is not an object, a 'people' value that is neither a list nor null, a person that is
not an object, a keypoint list holding anything but numbers.
"""
import argparse
import csv
import glob
import os
from pathlib import Path

import numpy as np

from . import _lib

KEYPOINT_NAMES = ('Nose LEye REye LEar REar LShoulder RShoulder LElbow RElbow LWrist RWrist LHip RHip LKnee RKnee LAnkle RAnkle '
                  'Head Neck Hip LBigToe RBigToe LSmallToe RSmallToe LHeel RHeel').split()   # HALPE_26 in JSON order
N_KPTS = len(KEYPOINT_NAMES)
CONF_THRESHOLD = 0.1
DEFAULT_MULTIPLIER = 5.0
DEFAULT_IMAGE_SIZE = (1920, 1080)
DEFAULT_OUTPUT = 'docs/012_2d_keypoint_jitter/test_results'
PATTERNS = 'ACDE'                                # the engine's pattern codes 0..3
PATTERN_NAMES = {'A': 'Out-of-frame', 'C': 'Small BB', 'D': 'Low confidence', 'E': 'Other'}
CSV_HEADER = ['camera', 'frame', 'keypoint', 'keypoint_idx', 'displacement', 'confidence', 'threshold', 'median_displacement',
              'pattern']


def find_camera_dirs(pose_dir):
    """-> the camera folders of pose_dir, in the reference's order of preference."""
    pose_dir = Path(pose_dir)
    for pattern in ('cam*_json', '*_json'):
        found = sorted(pose_dir.glob(pattern))
        if found:
            return found
    if list(pose_dir.glob('*.json')):
        return [pose_dir]
    raise FileNotFoundError(f'No JSON directories found in {pose_dir}')


def camera_name(cam_dir):
    name = Path(cam_dir).name
    return name.replace('_json', '') if name.endswith('_json') else name


def load_keypoints_series(cam_json_dir):
    """-> [n_files][26][3] (x, y, confidence) of the person tracked through the camera's files, NaN where there is none."""
    from .ingest import JsonBatch
    files = sorted(glob.glob(os.path.join(str(cam_json_dir), '*.json')))
    if not files:
        raise FileNotFoundError(f'No JSON files found in {cam_json_dir}')
    with JsonBatch(files) as batch:
        series, status, detail = batch.select_tracked_person(N_KPTS, CONF_THRESHOLD)
    bad = np.flatnonzero(status < 0)
    if len(bad):
        i = int(bad[0])
        if status[i] == _lib.P2S_TRACK_LONG_LIST:
            raise ValueError(f'cannot reshape array of size {int(detail[i])} into shape ({N_KPTS},3)')
        what = 'cannot be read as JSON' if status[i] == _lib.P2S_TRACK_BAD_FILE else 'does not hold OpenPose people with lists of numbers'
        raise ValueError(f'{files[i]} {what}')
    return series


def camera_result(res, c, series):
    """The reference's per-camera dictionary from the engine's tables for camera c."""
    ev = res['events']
    ev = ev[ev[:, 0] == c]
    frames, kpts = ev[:, 1].astype(np.int64), ev[:, 2].astype(np.int64)
    disp, thr, med = res['displacements'][c], res['thresholds'][c], res['medians'][c]
    d, cf = disp[frames - 1, kpts], series[frames, kpts, 2]
    events = [{'frame': int(f), 'keypoint': KEYPOINT_NAMES[k], 'keypoint_idx': int(k), 'displacement': float(dv),
               'confidence': float(cv), 'threshold': float(thr[k]), 'median_displacement': float(med[k]), 'pattern': PATTERNS[p]}
              for f, k, dv, cv, p in zip(frames, kpts, d, cf, ev[:, 3])]
    return {'n_frames': len(series), 'events': events, 'jitter_mask': res['jitter_mask'][c], 'displacements': disp,
            'thresholds': thr, 'medians': med, 'keypoints_series': series,
            'bb_areas': res['bb_areas'][c], 'median_bb_area': res['median_bb_area'][c], 'counts': res['counts'][c]}


def format_report(cam_results, multiplier):
    cameras = sorted(cam_results)
    counts = {c: [int(n) for n in cam_results[c]['counts']] for c in cameras}
    out = ['=== 2D Keypoint Jitter Analysis ===',
           f'Cameras: {len(cameras)} ({", ".join(cameras)})',
           f'Total frames: {sum(cam_results[c]["n_frames"] for c in cameras)}',
           f'Jitter threshold multiplier: {multiplier}', '',
           '--- Jitter Count per Camera x Keypoint ---']
    head = f'{"Keypoint":<14}' + ''.join(f'{c:>8}' for c in cameras) + f'{"total":>8}'
    out += [head, '-' * len(head)]
    totals = [sum(counts[c][k] for c in cameras) for k in range(N_KPTS)]
    for k, name in enumerate(KEYPOINT_NAMES):
        out.append(f'{name:<14}' + ''.join(f'{counts[c][k]:>8}' for c in cameras) + f'{totals[k]:>8}')
    n_events = sum(totals)
    out += [f'{"TOTAL":<14}' + ''.join(f'{len(cam_results[c]["events"]):>8}' for c in cameras) + f'{n_events:>8}', '',
            '--- Pattern Distribution ---']
    per_pattern = dict.fromkeys(PATTERNS, 0)
    for c in cameras:
        for e in cam_results[c]['events']:
            per_pattern[e['pattern']] += 1
    for p in PATTERNS:
        share = per_pattern[p] / n_events * 100 if n_events > 0 else 0
        out.append(f'  {p} ({PATTERN_NAMES[p]}): {per_pattern[p]} ({share:.1f}%)')
    out += [f'  Total: {n_events}', '', '--- Top 5 Problematic Keypoints ---']
    for k in sorted(range(N_KPTS), key=lambda k: -totals[k])[:5]:         # stable: the first keypoint on ties
        per_cam = '  '.join(f'{c}={counts[c][k]}' for c in cameras)
        out.append(f'  {KEYPOINT_NAMES[k]:<14} total={totals[k]}  ({per_cam})')
    out += ['', '--- Median Displacement & Threshold (px) ---']
    head = f'{"Keypoint":<14}' + ''.join(f'{c + "-med":>10}{c + "-thr":>10}' for c in cameras)
    out += [head, '-' * len(head)]
    for k, name in enumerate(KEYPOINT_NAMES):
        out.append(f'{name:<14}' + ''.join(f'{cam_results[c]["medians"][k]:>10.1f}{cam_results[c]["thresholds"][k]:>10.1f}' for c in cameras))
    out.append('')
    return '\n'.join(out)


def save_csv(all_events, output_dir):
    output_dir = Path(output_dir)
    output_dir.mkdir(parents=True, exist_ok=True)
    path = output_dir / 'jitter_events.csv'
    with open(path, 'w', newline='') as fh:
        writer = csv.writer(fh)
        writer.writerow(CSV_HEADER)
        for cam, e in all_events:
            writer.writerow([cam, e['frame'], e['keypoint'], e['keypoint_idx'], f'{e["displacement"]:.1f}', f'{e["confidence"]:.3f}',
                             f'{e["threshold"]:.1f}', f'{e["median_displacement"]:.1f}', e['pattern']])
    print(f'CSV saved: {path}')


def save_report_md(cam_results, multiplier, output_dir):
    output_dir = Path(output_dir)
    path = (output_dir.parent if output_dir.name == 'test_results' else output_dir) / 'phase1_results.md'
    cameras = sorted(cam_results)
    n_events = sum(len(cam_results[c]['events']) for c in cameras)
    lines = ['# 012 Phase 1 分析結果: 2Dキーポイント暴れ分析', '', '## 1. データ概要', '']
    lines += [f'- {c}: {cam_results[c]["n_frames"]} frames' for c in cameras]
    lines += [f'- キーポイント数: {N_KPTS} (HALPE_26)', f'- 暴れ閾値倍率: {multiplier}', '',
              '## 2. 分析結果サマリ', '', f'暴れ検出イベント合計: **{n_events}**', '',
              '```', format_report(cam_results, multiplier), '```', '',
              '## 3. プロット画像', '',
              '- `test_results/jitter_heatmap.png`: カメラ×キーポイント暴れ頻度ヒートマップ',
              '- `test_results/jitter_confidence_dist.png`: 暴れ時 vs 通常時のconfidence分布',
              '- `test_results/jitter_pattern_dist.png`: 原因パターン別分布',
              '- `test_results/jitter_timeseries_top3.png`: 暴れ上位3キーポイントの移動量時系列', '',
              '## 4. 考察', '', '（テスト実行後に記入）', '']
    with open(path, 'w', encoding='utf-8') as fh:
        fh.write('\n'.join(lines))
    print(f'Report saved: {path}')


def analyze_jitter(pose_dir, output=None, multiplier=DEFAULT_MULTIPLIER, no_plot=False, image_size=DEFAULT_IMAGE_SIZE, engine=None):
    """-> {camera name: {'n_frames', 'events', 'jitter_mask', 'displacements', 'thresholds', 'medians', 'keypoints_series',
    and 'bb_areas', 'median_bb_area', 'counts'}}, the dictionary the reference builds internally (it returns None).
    no_plot is accepted and changes nothing: no figure is drawn.  engine: an Engine (default: Engine(0))."""
    pose_dir = Path(pose_dir)
    output_dir = Path(DEFAULT_OUTPUT if output is None else output)
    cam_dirs = find_camera_dirs(pose_dir)
    # every camera is read first and analysed in one call; a camera that cannot be read ends the run where the reference
    # ends it, after the lines of the cameras before it
    loaded, error = [], None
    for d in cam_dirs:
        try:
            loaded.append(load_keypoints_series(d))
        except (FileNotFoundError, ValueError) as e:
            error = e
            break
    res = None
    if loaded:
        if engine is None:
            from .engine import Engine
            engine = Engine(0)
        res = engine.jitter(loaded, multiplier, image_size)
    print(f'Loading pose data from {pose_dir} ...')
    cam_results, all_events = {}, []
    for c, d in enumerate(cam_dirs):
        name = camera_name(d)
        print(f'\nAnalyzing {name} ...')
        if c == len(loaded):
            raise error
        cam_results[name] = result = camera_result(res, c, loaded[c])
        all_events += [(name, e) for e in result['events']]
        print(f'  {name}: {result["n_frames"]} frames, {len(result["events"])} jitter events')
    print('\n' + format_report(cam_results, multiplier))
    save_csv(all_events, output_dir)
    save_report_md(cam_results, multiplier, output_dir)
    return cam_results


def main():
    parser = argparse.ArgumentParser(description='Analyze 2D keypoint jitter (frame-to-frame displacement anomalies): detects the '
                                                 'jumps and guesses their cause.')
    parser.add_argument('-p', '--pose-dir', required=True, help='folder holding *_json camera folders, or the JSON files themselves')
    parser.add_argument('-o', '--output', default=None, help=f'output folder (default: {DEFAULT_OUTPUT}/)')
    parser.add_argument('--multiplier', type=float, default=DEFAULT_MULTIPLIER, help=f'threshold = median x this (default: {DEFAULT_MULTIPLIER})')
    parser.add_argument('--no-plot', action='store_true', help='accepted; no figure is drawn either way')
    parser.add_argument('--image-width', type=int, default=DEFAULT_IMAGE_SIZE[0], help=f'image width in pixels (default: {DEFAULT_IMAGE_SIZE[0]})')
    parser.add_argument('--image-height', type=int, default=DEFAULT_IMAGE_SIZE[1], help=f'image height in pixels (default: {DEFAULT_IMAGE_SIZE[1]})')
    args = parser.parse_args()
    analyze_jitter(pose_dir=args.pose_dir, output=args.output, multiplier=args.multiplier, no_plot=args.no_plot,
                   image_size=(args.image_width, args.image_height))


if __name__ == '__main__':
    main()
