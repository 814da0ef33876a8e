"""Goldens of the ID switch utility, recorded through the reference's own code -> idswitch_units.npz

Every case runs Pose2Sim/Utilities/id_switch_analyze.py:analyze_id_switches (imported through ref_shim; the module needs
numpy, scipy and tqdm only) on OpenPose JSON folders written here, and stores

* the input files as text and the arguments (paths relative to the folder the case ran in);
* the returned dictionary as JSON (detection_counts as a list of pairs: its keys are 0, 1, 2 and '3+');
* the text of the three written files and where they went, what was printed (tqdm writes to stderr: not kept), and for the
  error cases the exception's type and message.

Cases: 1, 3 and 4 cameras of different lengths; a folder named cam02_json_v2_json and one that is no camera; frames with
0, 1, 2, 3 and 5 persons; leading, trailing and inner empty runs shorter than, equal to and longer than fps, at fps 30 and
60; a gap preceded by an unreadable file, an unreadable first file; persons dropped by the filter (confidences all NaN,
all zero, all negative); pairs with exactly 2, 3, 7, 8, 9 and 26 shared keypoints, a confidence of exactly 0.1, a frame
where every pair costs 1e9, more previous than current persons and the reverse, two persons swapping their list order;
count changes 9, 10 and 11 frames apart in the same and in opposite directions; person_id as [-1], [3], 7, [1.0] and
absent; the default and an explicit output folder; a person without the list and a {} entry (KeyError), a 77-number list
(ValueError), 'people': null (TypeError), a document that is a list (AttributeError), a NaN coordinate on a shared keypoint
(ValueError from scipy), a camera whose every file is unreadable (ZeroDivisionError), no cam*_json folder and a camera
folder without files (FileNotFoundError); a crowd: one camera whose frames rise from 3 to 32 persons and fall again, pairs of
more than 64 costs and of 32 x 32, about one confidence in ten below 0.1, a person the filter drops listed first among 32
others, the list reversed from one frame to the next, an empty frame in between.

The file is written with fixed zip time stamps: running this script again reproduces it byte for byte.  It also prints
the time of the reference's own arithmetic (match_people) per frame at 1, 3 and 8 persons, one CPU core.
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

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import ref_shim  # noqa: E402

from make_golden_jitter import save_npz  # noqa: E402

WORK = os.path.join(os.path.realpath(tempfile.gettempdir()), 'idswitch_golden_work')   # fixed: the printed lines hold it
SHARED_COUNTS = (2, 3, 7, 8, 9, 26)
ABSENT = 'absent'


def load_reference():
    ref_shim.install()
    return importlib.import_module('Pose2Sim.Utilities.id_switch_analyze')


def body(cx, cy, conf=0.9, digits=1, wobble=None):
    """[26][3]: a fixed stick figure around (cx, cy); wobble: a generator for a little noise."""
    k = np.arange(26)
    xy = np.stack([cx + 20.0 * np.cos(0.7 * k) + 3.0 * (k % 5), cy + 35.0 * np.sin(0.45 * k) + 2.0 * (k % 7)], axis=1)
    if wobble is not None:
        xy = xy + wobble.normal(0, 0.8, xy.shape)
    return np.concatenate([np.round(xy, digits), np.full((26, 1), conf)], axis=1)


def person(kp, pid=(-1,)):
    entry = {} if pid == ABSENT else {'person_id': list(pid) if isinstance(pid, tuple) else pid}
    entry['pose_keypoints_2d'] = [float(v) for v in np.asarray(kp, dtype=np.float64).reshape(-1)]
    return entry


def document(people):
    return json.dumps({'version': 1.3, 'people': people})


def walkers(F, counts, seed, ids=((-1,), (-1,), (-1,), (-1,), (-1,)), swap=(), dropped=None, digits=1):
    """{file name: text} of F frames; counts[f] persons in frame f, person k walking right from its own start.  swap: frames
    whose list order is reversed; dropped {frame: kind}: an extra person the filter drops, listed first."""
    rng = np.random.default_rng(seed)
    files = {}
    for f in range(F):
        people = [person(body(150.0 + 330.0 * k + 1.5 * f, 400.0 + 40.0 * k, conf=round(0.6 + 0.05 * k, 2), digits=digits, wobble=rng), ids[k])
                  for k in range(counts[f])]
        if f in swap:
            people.reverse()
        if dropped and f in dropped:
            ghost = body(900.0, 500.0)
            ghost[:, 2] = {'nan': np.nan, 'zero': 0.0, 'negative': -0.5}[dropped[f]]
            people.insert(0, person(ghost))
        files[f'frame_{f:04d}.json'] = document(people)
    return files


def run_lengths(*runs):
    """(count, length) pairs -> the per-frame counts."""
    return [c for c, n in runs for _ in range(n)]


def shared_camera():
    """One hand-made camera: pairs with a chosen number of shared keypoints, in full-precision coordinates."""
    rng = np.random.default_rng(7)

    def full(cx, cy, n_conf_a):
        kp = body(cx, cy)
        kp[:, :2] = kp[:, :2] + rng.uniform(-1, 1, (26, 2))          # full precision
        kp[n_conf_a:, 2] = 0.05                                      # keypoints n_conf_a .. 25 take no part
        return kp
    frames = []
    for n in SHARED_COUNTS:                                          # two frames per count: one pair with n shared keypoints
        frames += [[person(full(400, 400, 26))], [person(full(403, 401, n))]]
    # a confidence of exactly 0.1 does not count: three above it and one on it -> 3 shared; two above and one on it -> 2
    edge = full(406, 402, 4)
    edge[3, 2] = 0.1
    frames.append([person(edge)])
    edge2 = full(408, 403, 3)
    edge2[2, 2] = 0.1
    frames.append([person(edge2)])
    # every pair costs 1e9: two persons against two without shared keypoints
    far = [full(300, 300, 26), full(900, 300, 26)]
    none = [full(300, 300, 26), full(900, 300, 26)]
    for kp in none:
        kp[:, 2] = np.where(np.arange(26) < 2, 0.9, 0.05)
    frames += [[person(k) for k in far], [person(k) for k in none]]
    # more previous than current persons, and the reverse; a tie between two identical candidates
    frames.append([person(full(300 + 250 * k, 300, 26)) for k in range(5)])
    frames.append([person(full(300 + 250 * k + 2, 301, 26)) for k in (3, 1)])
    frames.append([person(full(300 + 250 * k + 3, 302, 26)) for k in (0, 1, 2, 3, 4)])
    twin = full(500, 500, 26)
    frames += [[person(twin), person(twin)], [person(twin), person(twin), person(twin)]]
    return {f'f{f:03d}.json': document(people) for f, people in enumerate(frames)}


CROWD_COUNTS = (3, 8, 9, 12, 0, 20, 20, 32, 32, 32, 31, 13)


def crowd_camera():
    """{file name: text}: CROWD_COUNTS persons a frame, six to a row, walking right; about one confidence in ten is below the
    threshold.  Frame 8 lists its 32 persons in reverse; frames 6 and 9 list a person with zero confidence first."""
    rng = np.random.default_rng(40)
    files = {}
    for f, n in enumerate(CROWD_COUNTS):
        people = []
        for k in range(n):
            kp = body(150.0 + 300.0 * (k % 6) + 1.5 * f, 200.0 + 150.0 * (k // 6), conf=round(0.5 + 0.01 * k, 2), wobble=rng)
            kp[rng.random(26) < 0.1, 2] = 0.05
            people.append(person(kp))
        if f == 8:
            people.reverse()
        if f in (6, 9):
            ghost = body(900.0, 500.0)
            ghost[:, 2] = 0.0
            people.insert(0, person(ghost))
        files[f'frame_{f:04d}.json'] = document(people)
    return files


def cases():
    """-> list of dicts: name, files {relative path: text}, folders (made even when empty), pose_dir, args."""
    out = []

    def add(name, cams, pose_dir='pose', folders=(), **args):
        files = {f'{pose_dir}/{cam}/{fn}': text for cam, fs in cams.items() for fn, text in fs.items()}
        out.append({'name': name, 'files': files, 'folders': [pose_dir] + [f'{pose_dir}/{d}' for d in folders], 'pose_dir': pose_dir, 'args': args})

    ids = ((-1,), (3,), 7, (1.0,), ABSENT)
    # leading run, inner runs of 5 (< fps), 30 (= fps) and 31 (> fps) frames, every person count, a trailing run
    counts = run_lengths((0, 4), (1, 6), (0, 5), (2, 6), (0, 30), (3, 5), (0, 31), (5, 4), (1, 3), (2, 3), (0, 6))
    add('one_camera_default_output', {'cam01_json': walkers(len(counts), counts, 1, ids=ids, swap=(17, 18, 53), dropped={7: 'nan', 8: 'zero', 9: 'negative', 30: 'zero'})})
    # count changes 9, 10 and 11 frames apart, in opposite and in the same direction
    steps = run_lengths((1, 5), (2, 9), (1, 12), (2, 10), (1, 12), (2, 11), (1, 12), (2, 9), (3, 12), (2, 10), (1, 12), (2, 10), (3, 11), (2, 4))
    gaps60 = run_lengths((2, 3), (0, 59), (2, 3), (0, 60), (1, 3), (0, 61), (2, 3))
    add('three_cameras_fps60', {'cam01_json': walkers(len(steps), steps, 2), 'cam02_json': walkers(len(gaps60), gaps60, 3, swap=(63,)),
                                'cam03_json': walkers(40, run_lengths((0, 3), (3, 37)), 4, ids=ids, swap=range(10, 40, 3))},
        fps=60, output_dir='results')
    # unreadable files: before a gap, as the first file, inside a run; a folder with two '_json', one that is no camera
    broken = walkers(30, run_lengths((2, 8), (0, 6), (2, 16)), 5)
    broken['frame_0007.json'] = 'not json'
    broken['frame_0020.json'] = '{"version": 1.3, "people": ['
    first = walkers(20, run_lengths((1, 10), (2, 10)), 6)
    first['frame_0000.json'] = ''
    nokey = walkers(12, run_lengths((1, 12)), 8)
    nokey['frame_0005.json'] = '{"version": 1.3}'                      # no 'people' key: a frame without persons
    add('four_cameras_unreadable', {'cam01_json': broken, 'cam02_json_v2_json': first, 'cam03_json': walkers(25, run_lengths((0, 25)), 7),
                                    'cam04_json': nokey, 'other_json': walkers(3, [1, 1, 1], 9), 'notes': {}},
        folders=['notes'], output_dir='deep/er/out')
    add('shared_keypoints', {'cam1_json': shared_camera()}, output_dir='out', fps=30)

    def with_file(seed, name, text):
        files = walkers(8, run_lengths((2, 8)), seed)
        files[name] = text
        return files
    one = json.loads(walkers(1, [1], 20)['frame_0000.json'])['people'][0]
    add('error_no_key', {'cam01_json': walkers(5, [1] * 5, 21), 'cam02_json': with_file(22, 'frame_0004.json', document([one, {'person_id': [-1]}]))}, output_dir='out')
    add('error_empty_entry', {'cam01_json': with_file(23, 'frame_0003.json', document([{}, one]))}, output_dir='out')
    short = dict(one, pose_keypoints_2d=one['pose_keypoints_2d'][:77])
    add('error_77_numbers', {'cam01_json': with_file(24, 'frame_0002.json', document([one, short]))}, output_dir='out')
    add('error_people_null', {'cam01_json': with_file(25, 'frame_0005.json', '{"version": 1.3, "people": null}')}, output_dir='out')
    add('error_document_is_a_list', {'cam01_json': with_file(26, 'frame_0001.json', '[{"people": []}]')}, output_dir='out')
    nan = json.loads(json.dumps(one))
    nan['pose_keypoints_2d'][3 * 4] = float('nan')
    add('error_nan_coordinate', {'cam01_json': with_file(27, 'frame_0006.json', document([nan, one]))}, output_dir='out')
    add('error_all_unreadable', {'cam01_json': walkers(4, [1] * 4, 28), 'cam02_json': {'a.json': 'x', 'b.json': '{'}}, output_dir='out')
    add('error_no_folders', {'left_json': walkers(3, [1] * 3, 29)}, output_dir='out')
    add('error_no_files', {'cam01_json': walkers(3, [1] * 3, 30), 'cam02_json': {}}, folders=['cam02_json'], output_dir='out')
    add('crowd', {'cam01_json': crowd_camera()}, output_dir='out')    # last: the cases before it keep their place in the file
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


def encode_result(result):
    """The returned dictionary as JSON: floats keep their bits (repr), the int and str keys of detection_counts their type."""
    return json.dumps({cam: dict(res, detection_counts=[[k, v] for k, v in res['detection_counts'].items()]) for cam, res in result.items()})


def run_reference(ref, case):
    """Runs the utility in WORK/<name> (the working directory: the default output folder is relative) -> (returned dictionary
    or None, files written {relative path: text}, printed text, (error type, message) or None)."""
    work = os.path.join(WORK, case['name'])
    lay_out(case, work)
    args = dict(case['args'])
    if 'output_dir' in args:
        args['output_dir'] = os.path.join(work, args['output_dir'])
    error, result, printed = None, None, io.StringIO()
    before = {os.path.join(r, f) for r, _, fs in os.walk(work) for f in fs}
    cwd = os.getcwd()
    os.chdir(work)
    try:
        with contextlib.redirect_stdout(printed), contextlib.redirect_stderr(io.StringIO()), warnings.catch_warnings():
            warnings.simplefilter('ignore')
            result = ref.analyze_id_switches(os.path.join(work, case['pose_dir']), **args)
    except Exception as e:
        error = (type(e).__name__, str(e))
    finally:
        os.chdir(cwd)
    written = {}
    for r, _, fs in os.walk(work):
        for f in fs:
            p = os.path.join(r, f)
            if p not in before:
                with open(p, encoding='utf-8', newline='') as fh:
                    written[os.path.relpath(p, work)] = fh.read()
    return result, written, printed.getvalue(), error


def time_reference(ref):
    rng = np.random.default_rng(0)
    for n in (1, 3, 8):
        frames = [[body(200.0 + 150 * k + f, 400.0, wobble=rng) for k in range(n)] for f in range(200)]
        t0 = time.perf_counter()
        for a, b in zip(frames, frames[1:]):
            ref.match_people(a, b)
        dt = (time.perf_counter() - t0) / (len(frames) - 1)
        print(f'reference arithmetic (match_people), one core, {n} persons: {dt * 1e6:.0f} us per frame')


def gen(timing=True):
    ref = load_reference()
    out = {'work_root': np.array(WORK)}
    names = []
    for case in cases():
        n = case['name']
        names.append(n)
        result, written, printed, error = run_reference(ref, case)
        out[f'{n}__files'] = np.array(json.dumps(case['files'], sort_keys=True))
        out[f'{n}__folders'] = np.array(json.dumps(case['folders']))
        out[f'{n}__pose_dir'] = np.array(case['pose_dir'])
        out[f'{n}__args'] = np.array(json.dumps(case['args'], sort_keys=True))
        out[f'{n}__written'] = np.array(json.dumps(written, sort_keys=True))
        out[f'{n}__printed'] = np.array(printed)
        out[f'{n}__error'] = np.array(json.dumps(error))
        out[f'{n}__result'] = np.array('null' if result is None else encode_result(result))
        shutil.rmtree(os.path.join(WORK, n))
        events = {} if result is None else {cam: len(res['events']) for cam, res in result.items()}
        print(f'{n}: events {events}, {len(written)} files written, error {error}')
        assert (result is None) == n.startswith('error_'), n
    check_claims(out)
    out['cases'] = np.array(json.dumps(names))
    path = os.path.join(HERE, 'idswitch_units.npz')
    save_npz(path, out)
    size, conf = os.path.getsize(path), os.path.getsize(os.path.join(HERE, 'confidence_units.npz'))
    assert size < 1.5 * conf, (size, conf)
    print(f'{len(names)} cases; {size} bytes (confidence_units.npz: {conf}) -> {path}')
    if timing:
        time_reference(ref)
    shutil.rmtree(WORK, ignore_errors=True)


def check_claims(out):
    """What the docstring claims, on the recorded results."""
    def result(name):
        return json.loads(str(out[f'{name}__result']))
    one = result('one_camera_default_output')['cam01']
    assert [k for k, _ in one['detection_counts']] == [0, 1, 2, '3+'] and all(v > 0 for _, v in one['detection_counts'])
    assert list(one['person_id_values']) == ['[-1]', '[3]', '7', '[1.0]'] and one['n_errors'] == 0
    gaps = [e['gap_frames'] for e in one['events'] if e['event_type'] == 'detection_resumed']
    assert gaps == [4, 5, 30, 31] and [e['pattern'] for e in one['events'] if e['event_type'] == 'detection_resumed'] == ['A', 'A', 'A', 'D']
    assert sum(v for _, v in one['detection_counts']) == one['n_frames']
    assert 'docs/011_id_switch_analysis/test_results/id_switch_events.csv' in json.loads(str(out['one_camera_default_output__written']))
    three = result('three_cameras_fps60')
    assert [three[c]['n_frames'] for c in three] == [139, 192, 40]
    changes = [e for e in three['cam01']['events'] if e['event_type'] == 'count_change']
    assert sorted({b['frame'] - a['frame'] for a, b in zip(changes, changes[1:])}) == [9, 10, 11, 12]
    assert {e['pattern'] for e in changes} == {'C', 'D'}
    assert [e['gap_frames'] for e in three['cam02']['events'] if e['event_type'] == 'detection_resumed'] == [59, 60, 61]
    assert [e['pattern'] for e in three['cam02']['events'] if e['event_type'] == 'detection_resumed'] == ['A', 'A', 'D']
    assert len(three['cam03']['person_id_values']) == 3
    four = result('four_cameras_unreadable')
    assert list(four) == ['cam01', 'cam02_v2', 'cam03', 'cam04'] and [four[c]['n_errors'] for c in four] == [2, 1, 0, 0]
    assert four['cam03']['distance_stats']['count'] == 0.0 and four['cam03']['events'] == []
    assert str(out['four_cameras_unreadable__printed']).count('WARNING: ') == 3
    shared = result('shared_keypoints')['cam1']
    assert any(e['event_type'] == 'person_lost' for e in shared['events']) and any(e['event_type'] == 'person_appeared' for e in shared['events'])
    errors = {n: json.loads(str(out[f'{n}__error']))[0] for n in [k[:-7] for k in out if k.endswith('__error')] if n.startswith('error_')}
    assert errors == {'error_no_key': 'KeyError', 'error_empty_entry': 'KeyError', 'error_77_numbers': 'ValueError', 'error_people_null': 'TypeError',
                      'error_document_is_a_list': 'AttributeError', 'error_nan_coordinate': 'ValueError', 'error_all_unreadable': 'ZeroDivisionError',
                      'error_no_folders': 'FileNotFoundError', 'error_no_files': 'FileNotFoundError'}, errors
    assert json.loads(str(out['error_nan_coordinate__error']))[1] == 'matrix contains invalid numeric entries'
    # the crowd: some frame pair has P * Q > 64 and a 32 x 32 pair occurs; every previous or current person finds a partner
    crowd = result('crowd')['cam01']
    files = json.loads(str(out['crowd__files']))
    kept = [sum(any(c > 0 for c in p['pose_keypoints_2d'][2::3]) for p in json.loads(files[name])['people']) for name in sorted(files)]
    listed = [len(json.loads(files[name])['people']) for name in sorted(files)]
    assert tuple(kept) == CROWD_COUNTS and max(listed) == 33 and crowd['n_errors'] == 0
    present = [n for n in kept if n > 0]
    pairs = list(zip(present, present[1:]))
    assert any(p * q > 64 for p, q in pairs) and (32, 32) in pairs and max(p * q for p, q in pairs) == 1024
    assert len(crowd['match_distances']) == sum(min(p, q) for p, q in pairs) and max(crowd['match_distances']) < 1e9


if __name__ == '__main__':
    gen(timing='--no-timing' not in sys.argv)
