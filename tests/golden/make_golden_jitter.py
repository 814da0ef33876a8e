"""Goldens of the 2D keypoint jitter utility, recorded through the reference's own code -> jitter_units.npz

Every case runs Pose2Sim/Utilities/keypoint_jitter_analyze.py:analyze_jitter (imported through ref_shim; the module needs
none of its stand-ins) with no_plot=True on OpenPose JSON folders written here, and stores

* the input files as text and the arguments (paths relative to the folder the case ran in);
* per camera, in folder order: the selected series, the displacements, the box areas (compute_bb_areas on the captured
  series), their median, the medians, the thresholds and the mask -- analyze_camera's result, captured as it returns;
* the events with their camera names, as JSON (repr floats: exact);
* the text of every file written and where, what was printed, and for the error cases the exception's type and message.

Cases: 1, 3 and 4 cameras named cam*_json; folders that only match *_json (one holds '_json' twice); a bare folder of
JSON files; cameras of different lengths; file names whose lexicographic order is not their numeric order; frames
without a 'people' key, with an empty list, with null; two and three persons that cross, listed in shuffled order, the
tracked one sometimes with fewer valid keypoints than the others (gen() checks that the proximity rule and the
most-valid rule disagree on at least one recorded frame, and that a multi-person frame follows an all-NaN stretch); a
person with a short list; a keypoint that never moves (median exactly 0: threshold 10); a keypoint that is never valid
(all-NaN column); frames with one and with no valid keypoint; NaN confidences and coordinates; a box at each of the four
borders; a non-default image size and multiplier; the default output folder, one named test_results and one that is not;
2-frame and 1-frame inputs; a 133-keypoint list in the second camera (ValueError); no folders and no files
(FileNotFoundError).

The person selection needs no margin condition: the native selection sums the distances in np.mean's own order (DESIGN.md
4.12), so even a near-tie falls the same way.  gen() asserts that each of A, C, D and E occurs at least 20 times over the
recorded cases and at least 100 times in the large seeded series of tests/test_jitter_gpu.py under the restatement
(tests/jitter_numpy.py).  The file is written with fixed zip time stamps: running this script again reproduces it byte for
byte.  It also prints the time of the reference's own arithmetic on 6 000 frames, one CPU core.
"""
import contextlib
import importlib
import io
import json
import os
import shutil
import sys
import tempfile
import time
import warnings
import zipfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import ref_shim  # noqa: E402

import jitter_numpy as jn  # noqa: E402

WORK = os.path.join(os.path.realpath(tempfile.gettempdir()), 'jitter_golden_work')      # fixed: the printed lines hold it
LARGE = ((3, 108000, 2024), (8, 36000, 2025))            # (cameras, frames, seed) of the large seeded series


def load_reference():
    ref_shim.install()
    return importlib.import_module('Pose2Sim.Utilities.keypoint_jitter_analyze')


def save_npz(path, arrays):
    """np.savez_compressed with fixed time stamps, so that the same arrays give the same bytes."""
    with zipfile.ZipFile(path, 'w', zipfile.ZIP_DEFLATED) as zf:
        for key, val in arrays.items():
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.asanyarray(val), allow_pickle=False)
            info = zipfile.ZipInfo(key + '.npy', date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            zf.writestr(info, buf.getvalue())


def large_series(C, F, seed):
    return [jn.seeded_series(F, seed * 100 + c) for c in range(C)]


def person(values):
    """values [26][3] or a flat list -> a 'people' entry; NaN is written as the NaN literal json.load accepts."""
    flat = [float(v) for v in np.asarray(values, dtype=np.float64).ravel()]
    return {'person_id': [-1], 'pose_keypoints_2d': flat}


def document(people):
    return json.dumps({'version': 1.3, 'people': people})


def camera_files(F, seed, n_persons=1, image_size=(1920, 1080), stem='frame_{:04d}', gaps=(), p_weak=0.0):
    """-> {file name: text}: n_persons seeded persons per frame in shuffled order; frames in `gaps` alternate between no
    'people' key, an empty list and null; with p_weak the first person loses six keypoints' confidence in a frame."""
    rng = np.random.default_rng(seed + 7)
    tracks = [jn.seeded_series(F, seed * 10 + n, image_size, period=2.5 * F + 40 * n, p_low=0.15, p_outlier=0.03, decimals=2)
              for n in range(n_persons)]
    files = {}
    for f in range(F):
        name = stem.format(f) + '.json'
        if f in gaps:
            files[name] = ('{"version": 1.3}', document([]), '{"version": 1.3, "people": null}')[f % 3]
            continue
        people = []
        for n in rng.permutation(n_persons):
            kp = tracks[n][f].copy()
            if np.isnan(kp).all():
                continue                                  # this person is missing from the frame
            if n == 0 and rng.random() < p_weak:
                kp[rng.choice(26, 6, replace=False), 2] = 0.05
            people.append(person(kp))
        files[name] = document(people)
    return files


def special_camera():
    """One hand-made camera for the corner cases (see the module docstring)."""
    rng = np.random.default_rng(99)
    base = np.stack([rng.uniform(700, 1100, 26), rng.uniform(300, 800, 26), np.full(26, 0.8)], axis=1)
    base[0, :2], base[1, :2] = (700.0, 300.0), (1100.0, 800.0)   # the corners of the box, up to the noise
    files = {}
    F = 48
    for f in range(F):
        kp = base.copy()
        kp[:, :2] += np.round(rng.normal(0, 1.0, (26, 2)), 2)
        kp[3, :2] = base[3, :2]                           # keypoint 3 never moves: median 0, threshold 10 ...
        if f in (20, 33):
            kp[3, 0] += 25.0                              # ... and two jumps above it
        if f == 44:
            kp[3, 0] += 6.0                               # ... one below it
        kp[7, 2] = 0.0                                    # keypoint 7 is never valid: an all-NaN column
        if f in (5, 6):
            kp[:, 2] = 0.05
            kp[11, 2] = 0.9                               # one valid keypoint: a candidate, but no box
        if f == 8:
            kp[:, 2] = 0.05                               # none: no candidate
        if f in (10, 11):
            kp[2, 2] = np.nan                             # NaN confidence
            kp[4, 0] = np.nan                             # NaN x of a valid keypoint: the box is NaN
        if f == 12:
            kp[5, 1] = np.nan                             # NaN y
        if f in (14, 15):
            kp[:, 0] -= 695.0                             # box at the left border
            kp[9, 0] += 40.0 * (f - 14)
        if f in (17, 18):
            kp[:, 0] += 815.0                             # right
            kp[9, 0] -= 40.0 * (f - 17)
        if f in (22, 23):
            kp[:, 1] -= 295.0                             # top
            kp[9, 1] += 40.0 * (f - 22)
        if f in (25, 26):
            kp[:, 1] += 275.0                             # bottom
            kp[9, 1] -= 40.0 * (f - 25)
        if f in (30, 31, 32):
            kp[:, :2] = kp[:, :2].mean(axis=0) + 0.3 * (kp[:, :2] - kp[:, :2].mean(axis=0))   # a small box
            kp[13, 0] += 30.0 * (f - 30)
        if f in (36, 37):
            kp[15, 2] = 0.2                               # low confidence and a jump
            kp[15, 0] += 35.0 * (f - 35)
        if f in (40, 41):
            kp[16, 0] += 45.0 * (f - 39)                  # a plain jump
        kp = np.round(kp, 2)
        people = [person(kp)]
        if f == 2:
            people = [person(kp.ravel()[:51]), person(kp)]                     # a short list beside a full one
        if f == 3:
            people = [person(kp.ravel()[:51])]                                 # a short list alone: no candidate
        if f == 4:
            people = [{'person_id': [-1]}, person(kp)]                         # no list at all: length 0
        files[f'f{f:03d}.json'] = document(people)
    return files


def cases():
    """-> list of dicts: name, files {relative path: text}, folders (made even when empty), pose_dir, args, cwd-relative."""
    out = []

    def add(name, cams, pose_dir='pose', folders=(), **args):
        files = {f'{pose_dir}/{cam}/{fn}' if cam else f'{pose_dir}/{fn}': text for cam, fs in cams.items() for fn, text in fs.items()}
        out.append({'name': name, 'files': files, 'folders': [pose_dir] + [f'{pose_dir}/{d}' for d in folders], 'pose_dir': pose_dir, 'args': args})

    add('one_camera_default_output', {'cam01_json': camera_files(150, 1, gaps=(40, 41, 42))})
    add('three_cameras', {f'cam{c + 1:02d}_json': camera_files(100, 10 + c, n_persons=2, gaps=range(50, 56), p_weak=0.4) for c in range(3)},
        output='results')
    add('four_cameras_lengths', {f'cam{c + 1}_json': camera_files(F, 20 + c, n_persons=3, image_size=(1280, 720), gaps=range(20, 24), p_weak=0.4)
                                 for c, F in enumerate((60, 45, 30, 50))}, output='deep/er/test_results', multiplier=3.5, image_size=[1280, 720])
    add('star_json_folders', {'right_json_v2_json': camera_files(40, 31), 'left_json': camera_files(40, 32, n_persons=2), 'notes': {}},
        folders=['notes'], output='out')
    add('bare_folder', {'': camera_files(40, 33)}, pose_dir='session_json', output='out', multiplier=2.0)
    add('lexicographic_names', {'cam01_json': camera_files(25, 34, stem='img_{}')}, output='out')
    add('special', {'cam01_json': special_camera()}, output='test_results')
    add('two_frames', {'cam01_json': camera_files(2, 35)}, output='out')
    add('one_frame', {'cam01_json': camera_files(1, 36), 'cam02_json': camera_files(1, 37)}, output='out')
    long_cam = camera_files(6, 38)
    long_cam['frame_0003.json'] = document([person(np.round(np.random.default_rng(5).uniform(0.2, 900, 399), 2))])
    add('error_133_keypoints', {'cam01_json': camera_files(6, 39), 'cam02_json': long_cam}, output='out')
    add('error_no_folders', {}, output='out')
    add('error_no_files', {'cam01_json': camera_files(5, 40), 'cam02_json': {}}, folders=['cam02_json'], output='out')
    return out


def lay_out(case, work):
    shutil.rmtree(work, ignore_errors=True)
    os.makedirs(work)
    for d in case['folders']:
        os.makedirs(os.path.join(work, d), exist_ok=True)
    for rel, text in case['files'].items():
        os.makedirs(os.path.dirname(os.path.join(work, rel)), exist_ok=True)
        with open(os.path.join(work, rel), 'w') as fh:
            fh.write(text)


def run_reference(ref, case, selections):
    """Runs the utility in WORK/<name> (the working directory, for the default output); -> (per-camera results, files
    written {relative path: text}, printed text, (error type, message) or None)."""
    work = os.path.join(WORK, case['name'])
    lay_out(case, work)
    args = dict(case['args'])
    if 'output' in args:
        args['output'] = os.path.join(work, args['output'])
    if 'image_size' in args:
        args['image_size'] = tuple(args['image_size'])
    captured, error, printed = [], None, io.StringIO()
    real_camera, real_select = ref.analyze_camera, ref._select_person

    def analyze_camera(*a, **k):
        captured.append(real_camera(*a, **k))
        return captured[-1]

    def select(people, prev):
        chosen = real_select(people, prev)
        selections.append((people, prev, chosen))
        return chosen
    ref.analyze_camera, ref._select_person = analyze_camera, select
    before = {os.path.join(r, f) for r, _, fs in os.walk(work) for f in fs}
    cwd = os.getcwd()
    os.chdir(work)
    try:
        with contextlib.redirect_stdout(printed), contextlib.redirect_stderr(io.StringIO()), warnings.catch_warnings():
            warnings.simplefilter('ignore')
            ref.analyze_jitter(os.path.join(work, case['pose_dir']), no_plot=True, **args)
    except Exception as e:
        error = (type(e).__name__, str(e))
    finally:
        os.chdir(cwd)
        ref.analyze_camera, ref._select_person = real_camera, real_select
    written = {}
    for r, _, fs in os.walk(work):
        for f in fs:
            p = os.path.join(r, f)
            if p not in before:
                with open(p, encoding='utf-8', newline='') as fh:
                    written[os.path.relpath(p, work)] = fh.read()
    return captured, written, printed.getvalue(), error


def rules_disagree(people, prev, chosen):
    """A frame with several candidates and an earlier choice, where the chosen person is not the most-valid one."""
    cands = [np.array(p.get('pose_keypoints_2d', [])) for p in people]
    cands = [k.reshape(26, 3) for k in cands if k.size == 78]
    cands = [k for k in cands if ((k[:, 2] > 0.1) & ~np.isnan(k[:, 0])).any()]
    if len(cands) < 2 or prev is None or chosen is None:
        return False
    most = max(cands, key=lambda k: (k[:, 2] > 0.1).sum())
    return not np.array_equal(most, chosen, equal_nan=True)


def time_reference(ref):
    series = jn.seeded_series(6000, 1)
    t0 = time.perf_counter()
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        d = ref.compute_displacements(series)
        areas = ref.compute_bb_areas(series)
        med_area = np.nanmedian(areas)
        mask, thr, med = ref.detect_jitter(d, 5.0)
        patterns = [ref.classify_pattern(f, k, series, areas, med_area) for f, k in np.argwhere(mask)]
    dt = time.perf_counter() - t0
    tally = {p: patterns.count(p) for p in 'ACDE'}
    print(f'reference arithmetic, one core, 6 000 frames x 26 keypoints: {dt:.3f} s ({dt / 6000 * 1e6:.1f} us per frame), events {tally}')


def gen(timing=True):
    ref = load_reference()
    out = {'work_root': np.array(WORK)}
    names, tally = [], dict.fromkeys('ACDE', 0)
    selections, n_frames_total = [], 0
    after_gap = False
    for case in cases():
        n = case['name']
        names.append(n)
        first = len(selections)
        results, written, printed, error = run_reference(ref, case, selections)
        out[f'{n}__files'] = np.array(json.dumps(case['files'], sort_keys=True))
        out[f'{n}__folders'] = np.array(json.dumps(case['folders']))
        out[f'{n}__pose_dir'] = np.array(case['pose_dir'])
        out[f'{n}__args'] = np.array(json.dumps(case['args'], sort_keys=True))
        out[f'{n}__written'] = np.array(json.dumps(written, sort_keys=True))
        out[f'{n}__printed'] = np.array(printed)
        out[f'{n}__error'] = np.array(json.dumps(error))
        out[f'{n}__n_cams'] = np.array(len(results))
        events = []
        for c, r in enumerate(results):
            with warnings.catch_warnings():
                warnings.simplefilter('ignore')
                areas = ref.compute_bb_areas(r['keypoints_series'])
                med_area = np.nanmedian(areas)
            out[f'{n}__{c}__series'] = r['keypoints_series']
            out[f'{n}__{c}__displacements'] = r['displacements']
            out[f'{n}__{c}__areas'] = areas
            out[f'{n}__{c}__median_area'] = np.array(med_area)
            out[f'{n}__{c}__medians'] = r['medians']
            out[f'{n}__{c}__thresholds'] = r['thresholds']
            out[f'{n}__{c}__mask'] = r['jitter_mask']
            events.append(r['events'])
            n_frames_total += r['n_frames']
            for e in r['events']:
                tally[e['pattern']] += 1
            # a multi-person frame right after frames without a selection
            nan_rows = np.isnan(r['keypoints_series']).all(axis=(1, 2))
            after_gap |= bool(np.any(nan_rows[:-1] & ~nan_rows[1:]))
        out[f'{n}__events'] = np.array(json.dumps(events))
        shutil.rmtree(os.path.join(WORK, n))
        print(f'{n}: {len(results)} cameras, {sum(len(e) for e in events)} events, {len(selections) - first} selections, error {error}')
    disagree = sum(rules_disagree(*s) for s in selections)
    assert disagree >= 1, 'no frame where the proximity rule and the most-valid rule disagree'
    assert after_gap, 'no selection after an all-NaN stretch'
    assert min(tally.values()) >= 20, tally
    out['cases'] = np.array(json.dumps(names))
    path = os.path.join(HERE, 'jitter_units.npz')
    save_npz(path, out)
    print(f'{len(names)} cases, {n_frames_total} frames, events per pattern {tally}, {disagree} frames where the two selection rules '
          f'disagree; {os.path.getsize(path)} bytes -> {path}')
    for C, F, seed in LARGE:
        res = jn.NumpyJitterEngine().jitter(large_series(C, F, seed))
        counts = jn.pattern_counts(res['events'])
        assert min(counts.values()) >= 100, counts
        print(f'large seeded series {C} x {F}: events per pattern {counts}')
    if timing:
        time_reference(ref)
    shutil.rmtree(WORK, ignore_errors=True)


if __name__ == '__main__':
    gen(timing='--no-timing' not in sys.argv)
