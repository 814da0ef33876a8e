"""Goldens of the 2D confidence utility, recorded through the reference's own code -> confidence_units.npz

Every case runs Pose2Sim/Utilities/pose_confidence_analyze.py:analyze_confidence (imported through ref_shim; the module
needs none of its stand-ins, and matplotlib only for the heatmaps) with no_plot=True on OpenPose JSON folders written
here, and stores

* the input files as text and the arguments (paths relative to the folder the case ran in);
* the camera names and the tables load_pose_data returned, in its order;
* every statistic as float64 [C][26][10] (mean, median, std, min, max, p5, p25, p75, p95, below_threshold_rate), the band
  counts and rates [C][26][5], the simulated thresholds and their shares [T][C][26] -- the returned dictionary;
* the text of both CSV files and where they went, what was printed, and for the error cases the exception's type and
  message.

Cases: 1, 3 and 4 cameras of different lengths; a folder named cam02_json_v2_json; a camera whose every frame is empty;
frames without a 'people' key, with an empty list, with null; two persons of which the first listed is the smaller one; a
133-keypoint list; confidences of exactly 0.4, 0.6, 0.8 and 1.0, above 1, 0.0 and negative, a NaN literal; a constant
column of seven times 0.4 and a long one; columns with 1, 2, 7, 8, 9, 127, 128 and 129 valid frames and one with none;
thresholds 0.4 (default), 0.5, 0.45 (four simulated thresholds), 0.3 (it becomes the base) and 0.7; the default and an
explicit output folder; a 77-number list (IndexError), a person without the list (KeyError), no cam*_json folder and a
camera folder without files (FileNotFoundError).  No column holds both -0.0 and +0.0.

The file is written with fixed zip time stamps: running this script again reproduces it byte for byte.  It also prints
the time of the reference's own arithmetic on 6 000 frames x 26 keypoints, one CPU core.
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

WORK = os.path.join(os.path.realpath(tempfile.gettempdir()), 'confidence_golden_work')   # fixed: the printed lines hold it
STATS = ('mean', 'median', 'std', 'min', 'max', 'p5', 'p25', 'p75', 'p95', 'below_threshold_rate')
BANDS = ('low', 'danger', 'medium', 'high', 'very_high')
VALID_COUNTS = (1, 2, 7, 8, 9, 127, 128, 129)              # of the special camera's first columns
EMPTY_FRAMES = (50, 51)                                   # of its 135 frames hold no person


def load_reference():
    ref_shim.install()
    return importlib.import_module('Pose2Sim.Utilities.pose_confidence_analyze')


def person(conf, n_kpts=26, scale=1.0):
    """A 'people' entry with the given confidences (short coordinates keep the text small); NaN is written as the literal."""
    flat = []
    for k in range(n_kpts):
        flat += [round(100.0 * scale + k, 1), round(50.0 * scale + 2 * k, 1), float(conf[k]) if k < len(conf) else 0.5]
    return {'person_id': [-1], 'pose_keypoints_2d': flat}


def document(people):
    return json.dumps({'version': 1.3, 'people': people})


def confidences(F, rng):
    """[F][26] rounded to 3 decimals: mostly high, a danger-zone share that differs per keypoint, a few low ones."""
    conf = rng.uniform(0.62, 0.99, (F, 26))
    danger = rng.random((F, 26)) < np.linspace(0.02, 0.45, 26)[None, :]
    conf[danger] = rng.uniform(0.4, 0.6, int(danger.sum()))
    low = rng.random((F, 26)) < 0.06
    conf[low] = rng.uniform(0.01, 0.4, int(low.sum()))
    return np.round(conf, 3)


def camera_files(F, seed, gaps=(), second_person=False, n_kpts=26, stem='frame_{:04d}'):
    rng = np.random.default_rng(seed)
    conf = confidences(F, rng)
    files = {}
    for f in range(F):
        name = stem.format(f) + '.json'
        if f in gaps:
            files[name] = ('{"version": 1.3}', document([]), '{"version": 1.3, "people": null}')[f % 3]
            continue
        people = [person(conf[f], n_kpts)]
        if second_person and f % 3 == 0:                      # a larger, more confident person listed second: not used
            people.append(person(np.minimum(np.round(conf[f] + 0.2, 3), 1.0), n_kpts, scale=4.0))
        files[name] = document(people)
    return files


def empty_camera(F):
    return {f'frame_{f:04d}.json': ('{"version": 1.3}', document([]), '{"version": 1.3, "people": null}')[f % 3] for f in range(F)}


def special_camera():
    """One hand-made camera for the corner cases (see the module docstring)."""
    rng = np.random.default_rng(99)
    F = 135
    conf = confidences(F, rng)
    for k, n in enumerate(VALID_COUNTS):                      # columns 0..7: n valid frames at scattered places
        gone = np.ones(F, dtype=bool)
        gone[rng.choice(np.setdiff1d(np.arange(F), EMPTY_FRAMES), n, replace=False)] = False
        conf[gone, k] = np.nan
    conf[~np.isnan(conf[:, 2]), 2] = 0.4                      # seven times 0.4
    conf[:, 8] = np.resize([0.4, 0.6, 0.8, 1.0, 0.6, 1.0, 0.8], F)   # the band edges
    conf[:, 9] = np.round(rng.uniform(0.95, 1.6, F), 3)       # above 1
    conf[::9, 9] = 1.0
    conf[:, 10] = rng.choice([0.0, -0.25, 0.1, 0.399], F)     # zero and negative
    conf[:, 11] = 0.4                                         # a long constant column
    conf[:, 12] = np.nan                                      # never valid, in frames that hold a person
    conf[rng.random(F) < 0.3, 13] = np.nan                    # NaN literals among ordinary values
    files = {}
    for f in range(F):
        files[f'f{f:03d}.json'] = document([]) if f in EMPTY_FRAMES else document([person(conf[f])])
    return files


def cases():
    """-> list of dicts: name, files {relative path: text}, folders (made even when empty), pose_dir, args, cwd-relative."""
    out = []

    def add(name, cams, pose_dir='pose', folders=(), **args):
        files = {f'{pose_dir}/{cam}/{fn}': text for cam, fs in cams.items() for fn, text in fs.items()}
        out.append({'name': name, 'files': files, 'folders': [pose_dir] + [f'{pose_dir}/{d}' for d in folders], 'pose_dir': pose_dir, 'args': args})

    add('one_camera_default_output', {'cam01_json': camera_files(150, 1, gaps=(40, 41, 42))})
    add('three_cameras_lengths', {f'cam{c + 1:02d}_json': camera_files(F, 10 + c, gaps=range(20, 26), second_person=True)
                                  for c, F in enumerate((120, 90, 60))}, threshold=0.5, output='results')
    add('four_cameras', {'cam01_json': camera_files(60, 20), 'cam02_json_v2_json': camera_files(45, 21, gaps=(0, 44)),
                         'cam03_json': empty_camera(30), 'cam04_json': camera_files(50, 23, second_person=True),
                         'other_json': camera_files(3, 24), 'notes': {}},
        folders=['notes'], threshold=0.45, output='deep/er/out')
    add('special_values', {'cam01_json': special_camera()}, threshold=0.3, output='out')
    add('long_lists_threshold_07', {'cam1_json': camera_files(40, 30, n_kpts=133, stem='img_{}'), 'cam2_json': camera_files(25, 31)},
        threshold=0.7, output='out')
    short = camera_files(6, 40)
    doc = json.loads(short['frame_0003.json'])
    doc['people'][0]['pose_keypoints_2d'] = doc['people'][0]['pose_keypoints_2d'][:77]
    short['frame_0003.json'] = json.dumps(doc)
    add('error_77_numbers', {'cam01_json': camera_files(6, 41), 'cam02_json': short}, output='out')
    no_key = camera_files(6, 42)
    no_key['frame_0002.json'] = document([{'person_id': [-1]}, person(np.full(26, 0.9))])
    add('error_no_key', {'cam01_json': no_key}, output='out')
    add('error_no_folders', {'left_json': camera_files(3, 43)}, output='out')
    add('error_no_files', {'cam01_json': camera_files(5, 44), 'cam02_json': {}}, folders=['cam02_json'], output='out')
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


def run_reference(ref, case):
    """Runs the utility in WORK/<name> -> (returned dictionary or None, loaded tables {name: table}, files written
    {relative path: text}, printed text, (error type, message) or None)."""
    work = os.path.join(WORK, case['name'])
    lay_out(case, work)
    args = dict(case['args'])
    if 'output' in args:
        args['output'] = os.path.join(work, args['output'])
    loaded, error, result, printed = {}, None, None, io.StringIO()
    real_load = ref.load_pose_data

    def load(*a, **k):
        loaded.update(real_load(*a, **k))
        return loaded
    ref.load_pose_data = load
    before = {os.path.join(r, f) for r, _, fs in os.walk(work) for f in fs}
    cwd = os.getcwd()
    os.chdir(work)
    try:
        with contextlib.redirect_stdout(printed), contextlib.redirect_stderr(io.StringIO()), warnings.catch_warnings():
            warnings.simplefilter('ignore')
            result = ref.analyze_confidence(os.path.join(work, case['pose_dir']), no_plot=True, **args)
    except Exception as e:
        error = (type(e).__name__, str(e))
    finally:
        os.chdir(cwd)
        ref.load_pose_data = real_load
    written = {}
    for r, _, fs in os.walk(work):
        for f in fs:
            p = os.path.join(r, f)
            if p not in before:
                with open(p, encoding='utf-8', newline='') as fh:
                    written[os.path.relpath(p, work)] = fh.read()
    return result, loaded, written, printed.getvalue(), error


def time_reference(ref):
    import jitter_numpy as jn
    table = {'cam01': np.ascontiguousarray(jn.seeded_series(6000, 1)[:, :, 2])}
    t0 = time.perf_counter()
    ref.compute_statistics(table, 0.4)
    ref.compute_band_distribution(table)
    ref.simulate_threshold(table, [0.4, 0.5, 0.6])
    dt = time.perf_counter() - t0
    print(f'reference arithmetic, one core, 6 000 frames x 26 keypoints: {dt:.3f} s ({dt / 6000 * 1e6:.1f} us per frame)')


def gen(timing=True):
    ref = load_reference()
    out = {'work_root': np.array(WORK)}
    names, n_frames_total = [], 0
    for case in cases():
        n = case['name']
        names.append(n)
        result, loaded, written, printed, error = run_reference(ref, case)
        out[f'{n}__files'] = np.array(json.dumps(case['files'], sort_keys=True))
        out[f'{n}__folders'] = np.array(json.dumps(case['folders']))
        out[f'{n}__pose_dir'] = np.array(case['pose_dir'])
        out[f'{n}__args'] = np.array(json.dumps(case['args'], sort_keys=True))
        out[f'{n}__written'] = np.array(json.dumps(written, sort_keys=True))
        out[f'{n}__printed'] = np.array(printed)
        out[f'{n}__error'] = np.array(json.dumps(error))
        cams = list(loaded) if result is not None else []
        out[f'{n}__cameras'] = np.array(json.dumps(cams))
        for c, cam in enumerate(cams):
            out[f'{n}__{c}__table'] = loaded[cam]
            n_frames_total += len(loaded[cam])
        if result is not None:
            st, bd, sim = result['statistics'], result['band_distribution'], result['threshold_simulation']
            assert list(st) == cams and all(type(v) is float for v in st[cams[0]][0].values())
            out[f'{n}__stats'] = np.array([[[st[cam][k][s] for s in STATS] for k in range(26)] for cam in cams], dtype=np.float64)
            out[f'{n}__band_counts'] = np.array([[[bd[cam][k][b]['count'] for b in BANDS] for k in range(26)] for cam in cams], dtype=np.int64)
            out[f'{n}__band_rates'] = np.array([[[bd[cam][k][b]['rate'] for b in BANDS] for k in range(26)] for cam in cams], dtype=np.float64)
            out[f'{n}__sim_thresholds'] = np.array(list(sim), dtype=np.float64)
            out[f'{n}__sim'] = np.array([[[sim[th][cam][k] for k in range(26)] for cam in cams] for th in sim], dtype=np.float64)
        shutil.rmtree(os.path.join(WORK, n))
        print(f'{n}: cameras {cams}, {len(written)} files written, error {error}')
    # what the docstring claims
    sp = out['special_values__0__table']
    assert [int((~np.isnan(sp[:, k])).sum()) for k in range(8)] == list(VALID_COUNTS) and np.isnan(sp[:, 12]).all()
    ones = int((sp[:, 8] == 1.0).sum())                          # exactly 1.0: in 'high' and in 'very_high'
    assert ones > 0 and out['special_values__band_counts'][0, 8, 4] == ones
    assert out['special_values__band_counts'][0, 8, 3] == int(((sp[:, 8] >= 0.8) & (sp[:, 8] <= 1.0)).sum())
    assert out['special_values__band_counts'][0, 10].sum() == int((sp[:, 10] >= 0).sum()) < int((~np.isnan(sp[:, 10])).sum())   # negatives: in no band
    for k in range(26):
        col = sp[:, k][~np.isnan(sp[:, k])]
        zeros = col[col == 0]
        assert len(set(np.signbit(zeros))) <= 1
    assert np.isnan(out['four_cameras__2__table']).all() and np.isnan(out['four_cameras__stats'][2]).all()
    assert (out['four_cameras__band_rates'][2] == 0).all() and (out['four_cameras__sim'][:, 2] == 0).all()
    assert len(out['four_cameras__sim_thresholds']) == 4 and out['special_values__sim_thresholds'][0] == 0.3
    assert json.loads(str(out['four_cameras__cameras'])) == ['cam01', 'cam02_v2', 'cam03', 'cam04']
    out['cases'] = np.array(json.dumps(names))
    path = os.path.join(HERE, 'confidence_units.npz')
    save_npz(path, out)
    size, jitter = os.path.getsize(path), os.path.getsize(os.path.join(HERE, 'jitter_units.npz'))
    assert size < jitter, (size, jitter)
    print(f'{len(names)} cases, {n_frames_total} frames; {size} bytes (jitter_units.npz: {jitter}) -> {path}')
    if timing:
        time_reference(ref)
    shutil.rmtree(WORK, ignore_errors=True)


if __name__ == '__main__':
    gen(timing='--no-timing' not in sys.argv)
