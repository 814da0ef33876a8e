"""ID switch analysis: mirror of Pose2Sim/Utilities/id_switch_analyze.py.

Per camera, over the frames in file order: how many persons the detector reports, and whether they keep their identity
from frame to frame -- every frame's persons are matched to those of the last earlier frame that held one by the
Hungarian assignment over the mean keypoint distance.  Reported: persons lost and appearing, count changes, gaps without
detections and their A / C / D patterns, the distribution of the matched distances and of the person_id values.  Written:
id_switch_events.csv and match_distances.csv into the output folder, phase1_results.md (UTF-8) into its parent, and the
console lines, all byte for byte the reference's; the tqdm progress bars are not reproduced.

The JSON files of a camera are parsed in one batch by the native ingest (JsonBatch); the person filter, the previous-frame
scan, the cost matrices, scipy's linear_sum_assignment and the distance statistics come from one call of the HIP engine
for all cameras (Engine.id_switch, csrc/p2s_idswitch.hip), float64 and bit for bit the reference's.  There is no NumPy or
scipy path for them.  The host counts integers, forms the rates and percentages, turns the per-frame integers into the
event list, classifies the patterns (pattern A's backward search with a stack instead of the reference's rescan: linear
in the number of events, the same marks) and formats text.

Kept from the reference, each recorded in tests/golden/idswitch_units.npz: only folders named cam*_json are cameras; the
camera name is the folder name with every '_json' removed; the files are taken in sorted order and `frame` is the position
in that order; a person without 'pose_keypoints_2d' (the {} entries personAssociation writes included) raises KeyError, a
list that is not 78 numbers ValueError, 'people': null TypeError, a document that is not an object AttributeError; a file
that cannot be read or is not JSON counts in n_errors, keeps its frame index, resets nothing and prints the WARNING line
with json's own message (the host reads such a file again to word it; the message is json's, byte for byte); a person is
dropped when no confidence is above 0; a keypoint takes part in a cost when both confidences are above 0.1, fewer than 3
of them cost 1e9; a frame without persons does not replace the previous persons; detection_resumed is emitted even after
leading empty frames; person_id is str() of the JSON value, '[-1]' when absent, counted in first-seen order; a NaN
coordinate on a shared keypoint raises scipy's ValueError; a camera whose every file is unreadable divides by zero.

Outside the reference's contract: more than 32 kept persons in one frame is refused with ValueError naming the file before
anything is written; a person that is no object, or whose list holds anything but numbers, raises KeyError / ValueError.
"""
import argparse
import csv
import json
from pathlib import Path

import numpy as np

from . import _lib

N_VALUES = 78
MAX_PERSONS = _lib.P2S_LSAP_MAX
EVENT_TYPES = ('count_change', 'person_lost', 'person_appeared', 'no_detection', 'detection_resumed')


def camera_name(cam_dir):
    return Path(cam_dir).name.replace('_json', '')


def _abort_of_file(kind):
    """The exception the reference ends with on a parsed file without a usable person list, or None."""
    if kind == _lib.P2S_JSON_DOC_PEOPLE_NULL:
        return TypeError("'NoneType' object is not iterable")
    if kind == _lib.P2S_JSON_DOC_PEOPLE_OTHER:
        return TypeError("'people' is not a list")
    if kind in _lib.P2S_JSON_DOC_TYPES:
        return AttributeError(f"'{_lib.P2S_JSON_DOC_TYPES[kind]}' object has no attribute 'get'")
    return None


def _abort_of_person(length, path):
    if length == _lib.P2S_JSON_PERSON_NO_LIST:
        return KeyError('pose_keypoints_2d')
    if length == _lib.P2S_JSON_PERSON_NOT_NUMERIC:
        return ValueError(f'{path} does not hold OpenPose people with lists of numbers')
    return ValueError(f'cannot reshape array of size {length} into shape (26,3)')


def load_camera(cam_dir):
    """-> dict: 'files', 'persons' [N][26][3] and 'offsets' [n + 1] of the n readable files before the first one the
    reference stops at, 'frame_of' [n] their positions among the files, 'unreadable' positions, 'ids' the persons'
    person_id texts, 'abort' the exception that file raises or None."""
    from .ingest import JsonBatch
    files = sorted(Path(cam_dir).glob('*.json'))
    if not files:
        raise FileNotFoundError(f'No JSON files found in {cam_dir}')
    with JsonBatch([str(f) for f in files]) as batch:
        ids, kinds = batch.person_ids()
        base = batch.person_base
        stop, abort = len(files), None
        bad_kind = np.flatnonzero(kinds > _lib.P2S_JSON_DOC_NO_PEOPLE_KEY)
        bad_person = np.flatnonzero(batch.person_lengths != N_VALUES)
        if len(bad_kind):
            stop, abort = int(bad_kind[0]), _abort_of_file(int(kinds[bad_kind[0]]))
        if len(bad_person):
            i = int(np.searchsorted(base, bad_person[0], side='right')) - 1
            if i < stop:
                stop, abort = i, _abort_of_person(int(batch.person_lengths[bad_person[0]]), files[i])
        listed = kinds[:stop] >= _lib.P2S_JSON_DOC_PEOPLE                 # readable: a list, or no 'people' key at all
        frame_of = np.flatnonzero(listed)
        n_persons = int(base[stop])
        file_index = np.repeat(np.arange(stop), np.diff(base[:stop + 1]))
        persons, _ = batch.gather_people(file_index, np.arange(n_persons) - base[file_index], N_VALUES)
    return {'files': files, 'persons': persons.reshape(-1, 26, 3), 'offsets': np.append(base[frame_of], n_persons).astype(np.int64),
            'frame_of': frame_of, 'unreadable': np.flatnonzero(~listed), 'ids': ids[:n_persons], 'abort': abort}


def parse_warning(cam_name, frame_idx, path):
    """The reference's WARNING line for a file the ingest could not parse: json's own wording, from reading it again."""
    try:
        with open(path) as f:
            json.load(f)
    except (json.JSONDecodeError, IOError) as e:
        return f'WARNING: {cam_name} frame {frame_idx}: JSON parse error: {e}'
    raise _lib.P2sError(f'{path}: the native parser refuses a file json.load accepts')


def events_of_camera(frame_of, counts, prev, zero_run, n_lost, n_appeared):
    """The reference's event list from the per-frame integers (analyze_camera :204-279), frames in order."""
    counts, prev = np.asarray(counts), np.asarray(prev)
    with_prev = prev >= 0
    prev_count = np.where(with_prev, counts[np.maximum(prev, 0)], 0)
    empty = counts == 0
    resumed = ~empty & (np.asarray(zero_run) > 0)
    matched = ~empty & with_prev
    busy = (empty & with_prev & (np.asarray(zero_run) == 0)) | resumed | (matched & ((prev_count != counts) | (np.asarray(n_lost) > 0) | (np.asarray(n_appeared) > 0)))
    events = []

    def add(frame, kind, before, now, gap=''):
        events.append({'frame': frame, 'event_type': kind, 'prev_count': before, 'curr_count': now, 'match_distance': '',
                       'gap_frames': gap, 'pattern': ''})
    for f in np.flatnonzero(busy).tolist():
        frame, now, before = int(frame_of[f]), int(counts[f]), int(prev_count[f])
        if now == 0:
            add(frame, 'no_detection', before, 0)
            continue
        if resumed[f]:
            add(frame, 'detection_resumed', 0, now, int(zero_run[f]))
        if not with_prev[f]:
            continue
        if before != now:
            add(frame, 'count_change', before, now)
        for _ in range(int(n_lost[f])):
            add(frame, 'person_lost', before, now)
        for _ in range(int(n_appeared[f])):
            add(frame, 'person_appeared', before, now)
    return events


def classify_patterns(events, fps=30):
    """classify_patterns :294-361.  Pattern A marks, for every detection_resumed after a gap of at most fps frames, the
    nearest earlier no_detection that is still unmarked: those are kept on a stack while walking the events once."""
    pattern_counts = {'A': 0, 'B': 0, 'C': 0, 'D': 0}
    unmarked = []
    for e in events:
        if e['event_type'] == 'no_detection':
            unmarked.append(e)
        elif e['event_type'] == 'detection_resumed':
            gap = e.get('gap_frames', 0)
            if isinstance(gap, int) and gap <= fps:
                e['pattern'] = 'A'
                pattern_counts['A'] += 1
                if unmarked:
                    unmarked.pop()['pattern'] = 'A'
    changes = [e for e in events if e['event_type'] == 'count_change']
    for e1, e2 in zip(changes, changes[1:]):
        if abs(e2['frame'] - e1['frame']) <= 10 and (e1['curr_count'] - e1['prev_count']) * (e2['curr_count'] - e2['prev_count']) < 0:
            for e in (e1, e2):
                if e['pattern'] == '':
                    e['pattern'] = 'C'
                    pattern_counts['C'] += 1
    for e in events:
        if e['pattern'] == '' and e['event_type'] in EVENT_TYPES:
            e['pattern'] = 'D'
            pattern_counts['D'] += 1
    return events, pattern_counts


def person_id_values(ids, kept):
    """{str(person_id): occurrences} over the kept persons, in first-seen order; '[-1]' where the key is absent."""
    words, out = {None: '[-1]'}, {}
    for p in np.asarray(kept).tolist():
        text = ids[p]
        if text not in words:
            words[text] = str(json.loads(text))
        word = words[text]
        out[word] = out.get(word, 0) + 1
    return out


def format_report(cam_results, fps):
    lines = ['# 011 IDスイッチ分析結果（Phase 1）', '', '## 1. データ概要', '', f'- フレームレート: {fps} fps', f'- カメラ数: {len(cam_results)}']
    ordered = sorted(cam_results.items())
    for cam, res in ordered:
        lines.append(f'- {cam}: {res["n_frames"]} フレーム (エラー: {res["n_errors"]})')
    lines += ['', '## 2. 検出人数の分布', '', '| カメラ | 0人 | 1人 | 2人 | 3人+ |', '|--------|-----|-----|-----|------|']
    for cam, res in ordered:
        dc = res['detection_counts']
        total = res['n_frames'] - res['n_errors']
        lines.append(f'| {cam} | {dc[0]} ({dc[0]/total*100:.1f}%) | {dc[1]} ({dc[1]/total*100:.1f}%) '
                     f'| {dc[2]} ({dc[2]/total*100:.1f}%) | {dc["3+"]} ({dc["3+"]/total*100:.1f}%) |')
    lines += ['', '## 3. person_idの分布', '']
    for cam, res in ordered:
        lines.append(f'- {cam}: {res["person_id_values"]}')
    lines += ['', '## 4. フレーム間マッチング距離の分布', '', '| カメラ | サンプル数 | 平均 | 中央値 | 95%ile | 99%ile | 最小 | 最大 |',
              '|--------|-----------|------|--------|--------|--------|------|------|']
    for cam, res in ordered:
        ds = res['distance_stats']
        lines.append(f'| {cam} | {ds["count"]} | {ds["mean"]:.1f} | {ds["median"]:.1f} | {ds["p95"]:.1f} | {ds["p99"]:.1f} '
                     f'| {ds["min"]:.1f} | {ds["max"]:.1f} |')
    lines += ['', '## 5. イベントパターン分類', '', f'- パターンA: 一時的消失→再出現（{fps}フレーム={fps/fps:.0f}秒以内）',
              '- パターンB: 人数変動なし・マッチング距離異常（※Phase 1では未使用: 閾値が未決定のため）',
              '- パターンC: 段階的な人数変動（10フレーム以内の増減反転）', '- パターンD: その他', '',
              '| カメラ | A | B | C | D | 合計イベント |', '|--------|---|---|---|---|------------|']
    for cam, res in ordered:
        pc = res['pattern_counts']
        lines.append(f'| {cam} | {pc["A"]} | {pc["B"]} | {pc["C"]} | {pc["D"]} | {sum(pc.values())} |')
    lines += ['', '## 6. イベントタイプ別集計', '']
    for cam, res in ordered:
        event_types = {}
        for e in res['events']:
            event_types[e['event_type']] = event_types.get(e['event_type'], 0) + 1
        lines.append(f'### {cam}')
        lines += [f'- {et}: {count}' for et, count in sorted(event_types.items())]
        lines.append('')
    lines += ['## 7. マッチング失敗率', '', 'マッチング失敗 = person_lost + person_appeared イベント（人物の出現・消失）', '']
    for cam, res in ordered:
        n_lost = sum(1 for e in res['events'] if e['event_type'] == 'person_lost')
        n_appeared = sum(1 for e in res['events'] if e['event_type'] == 'person_appeared')
        total = res['n_frames'] - res['n_errors']
        lines.append(f'- {cam}: 消失={n_lost} ({n_lost/total*100:.2f}%), 出現={n_appeared} ({n_appeared/total*100:.2f}%)')
    lines.append('')
    return '\n'.join(lines)


def save_events_csv(cam_results, output_dir):
    output_dir = Path(output_dir)
    output_dir.mkdir(parents=True, exist_ok=True)
    path = output_dir / 'id_switch_events.csv'
    with open(path, 'w', newline='') as f:
        writer = csv.writer(f)
        writer.writerow(['camera', 'frame', 'event_type', 'prev_person_count', 'curr_person_count', 'match_distance', 'gap_frames', 'pattern'])
        for cam in sorted(cam_results):
            for e in cam_results[cam]['events']:
                writer.writerow([cam, e['frame'], e['event_type'], e['prev_count'], e['curr_count'], e['match_distance'], e['gap_frames'], e['pattern']])
    print(f'Events CSV saved: {path}')
    return path


def save_distance_csv(cam_results, output_dir):
    output_dir = Path(output_dir)
    output_dir.mkdir(parents=True, exist_ok=True)
    path = output_dir / 'match_distances.csv'
    with open(path, 'w', newline='') as f:
        writer = csv.writer(f)
        writer.writerow(['camera', 'distance'])
        for cam in sorted(cam_results):
            for d in cam_results[cam]['match_distances']:
                writer.writerow([cam, f'{d:.2f}'])
    print(f'Distance CSV saved: {path}')
    return path


def camera_result(cam, res, c, fps):
    """The reference's result dictionary of camera c from Engine.id_switch's tables: Python ints and floats."""
    counts = res['counts'][c]
    n_by_count = np.bincount(np.minimum(counts, 3), minlength=4)
    distances = [float(d) for d in res['distances'][c]]
    if distances:
        stats = dict(zip(('mean', 'median', 'p95', 'p99', 'min', 'max'), (float(v) for v in res['stats'][c])))
        stats['count'] = len(distances)
    else:
        stats = {k: 0.0 for k in ('mean', 'median', 'p95', 'p99', 'min', 'max', 'count')}
    events = events_of_camera(cam['frame_of'], counts, res['prev'][c], res['zero_run'][c], res['n_lost'][c], res['n_appeared'][c])
    events, pattern_counts = classify_patterns(events, fps=fps)
    return {'events': events, 'match_distances': distances,
            'detection_counts': {0: int(n_by_count[0]), 1: int(n_by_count[1]), 2: int(n_by_count[2]), '3+': int(n_by_count[3])},
            'person_id_values': person_id_values(cam['ids'], res['kept'][c]), 'n_frames': len(cam['files']),
            'n_errors': len(cam['unreadable']), 'distance_stats': stats, 'pattern_counts': pattern_counts}


def analyze_id_switches(pose_dir, output_dir=None, fps=30, engine=None):
    """-> {camera: {'events', 'match_distances', 'detection_counts', 'person_id_values', 'n_frames', 'n_errors',
    'distance_stats', 'pattern_counts'}}, as the reference returns it.  engine: an Engine (default: Engine(0))."""
    pose_dir = Path(pose_dir)
    output_dir = Path('docs/011_id_switch_analysis/test_results') if output_dir is None else Path(output_dir)
    cam_dirs = sorted(pose_dir.glob('cam*_json'))
    if not cam_dirs:
        raise FileNotFoundError(f'No cam*_json directories found in {pose_dir}')
    print(f'Analyzing ID switches in {pose_dir}')
    print(f'Found {len(cam_dirs)} cameras: {[d.name for d in cam_dirs]}')
    print(f'FPS: {fps}')
    print()
    # every camera up to the first file the reference stops at, in one call of the engine
    names, cams, pending = [], [], None
    for cam_dir in cam_dirs:
        names.append(camera_name(cam_dir))
        try:
            cams.append(load_camera(cam_dir))
        except FileNotFoundError as e:
            pending = e
            break
        if cams[-1]['abort'] is not None:
            break
    if cams:
        if engine is None:
            from .engine import Engine
            engine = Engine(0)
        res = engine.id_switch([(cam['persons'], cam['offsets']) for cam in cams])
        for c, cam in enumerate(cams):
            crowded = np.flatnonzero(res['counts'][c] > MAX_PERSONS)
            if len(crowded):
                raise ValueError(f'{cam["files"][cam["frame_of"][crowded[0]]]} holds {int(res["counts"][c][crowded[0]])} valid persons; '
                                 f'at most {MAX_PERSONS} a frame are matched')
    cam_results = {}
    for c, name in enumerate(names):
        print(f'Processing {name}...')
        if c == len(cams):
            raise pending
        cam = cams[c]
        refused = np.flatnonzero(res['flags'][c])
        stop = cam['frame_of'][refused[0]] if len(refused) else len(cam['files'])
        for i in cam['unreadable'].tolist():
            if i < stop:
                print(parse_warning(name, i, cam['files'][i]))
        if len(refused):
            raise ValueError(_lib.P2S_LSAP_ERRORS[int(res['flags'][c][refused[0]])])
        if cam['abort'] is not None:
            raise cam['abort']
        result = cam_results[name] = camera_result(cam, res, c, fps)
        ds, dc = result['distance_stats'], result['detection_counts']
        print(f'  Frames: {result["n_frames"]}, Errors: {result["n_errors"]}')
        print(f'  Detection: 0={dc[0]}, 1={dc[1]}, 2={dc[2]}, 3+={dc["3+"]}')
        print(f'  Match distances: mean={ds["mean"]:.1f}, median={ds["median"]:.1f}, p95={ds["p95"]:.1f}, p99={ds["p99"]:.1f}')
        print(f'  Events: {len(result["events"])}')
        print(f'  Patterns: {result["pattern_counts"]}')
        print()
    report = format_report(cam_results, fps)
    output_dir.mkdir(parents=True, exist_ok=True)
    report_path = output_dir.parent / 'phase1_results.md'
    with open(report_path, 'w', encoding='utf-8') as f:
        f.write(report)
    print(f'Report saved: {report_path}')
    save_events_csv(cam_results, output_dir)
    save_distance_csv(cam_results, output_dir)
    print()
    print(report)
    return cam_results


def main():
    parser = argparse.ArgumentParser(description='Analyze tracking ID switches in 2D pose estimation outputs. '
                                                 'Quantifies detection count changes and frame-to-frame person matching.')
    parser.add_argument('-p', '--pose-dir', required=True, help='Pose directory path containing cam*_json subdirectories.')
    parser.add_argument('-o', '--output-dir', default=None, help='Output directory path. Default: docs/011_id_switch_analysis/test_results/')
    parser.add_argument('--fps', type=int, default=30, help='Frame rate (default: 30). Used for pattern A gap threshold.')
    args = parser.parse_args()
    analyze_id_switches(pose_dir=args.pose_dir, output_dir=args.output_dir, fps=args.fps)


if __name__ == '__main__':
    main()
