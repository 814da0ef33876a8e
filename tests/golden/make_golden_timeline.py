"""Goldens of the confidence timeline utility, recorded through the reference's own code -> timeline_units.npz

Every case runs Pose2Sim/Utilities/confidence_timeline.py:process (imported through ref_shim; matplotlib draws its PNG
with the Agg backend into the work folder, where it stays) on an OpenPose JSON folder written here, and stores

* the input files as text, the folders made, and the arguments (paths relative to the folder the case ran in);
* the bytes of confidence_timeline.csv;
* what was printed on stdout, the elapsed figure masked, and on stderr (the progress bar is taken out of the module for
  the run: its text holds rates and times);
* for the error cases the exception's type and message, and whether the output folder existed afterwards;
* the reference's keypoint table as the list of its names in index order, and N_KEYPOINTS.

Cases: 1 file and 257 files; 0, 1, 3 and 6 persons in a file; an empty 'people' list and no 'people' key; a file whose only
person has 77 numbers; person 0 too short and person 1 valid; an entry without 'pose_keypoints_2d'; a 133-keypoint list;
a file in the middle of a folder that does not decode; a folder in which no entry is valid (a CSV of the header alone); the
default keypoints, a single one, all 26, a name given twice, an unknown name (ValueError before the folder is made);
confidences 1 (an integer), 0, 0.1, 1e-05, 1.5, a NaN literal and a 17-digit value; an empty folder (FileNotFoundError,
raised before an unknown name is noticed); 'people': null (TypeError), a top level that is a list and one that is a
number (AttributeError), each in the middle of a folder.

The file is written with fixed zip time stamps: running this script again reproduces it byte for byte.  It also prints
the reference's time per frame on 6 000 frames x 3 persons x 4 keypoints, one CPU core.
"""
import contextlib
import importlib
import io
import json
import os
import re
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

WORK = os.path.join(os.path.realpath(tempfile.gettempdir()), 'timeline_golden_work')   # fixed: the printed lines hold it
DEFAULT = ['Nose', 'Neck', 'RShoulder', 'LShoulder']
ELAPSED = re.compile(r'in \d+\.\d+s\.')


def load_reference():
    ref_shim.install()
    ref = importlib.import_module('Pose2Sim.Utilities.confidence_timeline')
    ref.tqdm = lambda files, **kwargs: files
    return ref


def person(conf, n_kpts=26, n_numbers=None, integers=False):
    """A 'people' entry with the confidences `conf` (one value for all, or one a keypoint), short coordinates."""
    conf = np.broadcast_to(np.asarray(conf, dtype=object), (n_kpts,))
    flat = []
    for k in range(n_kpts):
        flat += [100 + k, 50 + 2 * k, conf[k]] if integers else [100.5 + k, 50.0 + 2 * k, conf[k]]
    return {'person_id': [-1], 'pose_keypoints_2d': flat[:n_numbers]}


def document(people):
    return json.dumps({'version': 1.3, 'people': people})


def seeded_folder(F, seed, most, stem='frame_{:05d}'):
    """F files of 0 .. most persons, confidences of three decimals."""
    rng = np.random.default_rng(seed)
    files = {}
    for f in range(F):
        n = int(rng.integers(0, most + 1)) if f else most
        files[stem.format(f) + '.json'] = document([person([float(v) for v in np.round(rng.uniform(0.0, 1.0, 26), 3)]) for _ in range(n)])
    return files


def mixed_folder():
    rng = np.random.default_rng(5)

    def conf():
        return [float(v) for v in np.round(rng.uniform(0.0, 1.0, 26), 3)]
    return {
        'f00.json': document([person(conf())]),
        'f01.json': document([]),
        'f02.json': document([person(conf()) for _ in range(3)]),
        'f03.json': '{"version": 1.3}',
        'f04.json': document([person(conf(), n_numbers=77)]),
        'f05.json': document([person(conf(), n_numbers=77), person(conf())]),
        'f06.json': '{"version": 1.3, "people": [',
        'f07.json': document([person(conf()), {'person_id': [-1]}, person(conf())]),
        'f08.json': document([person([float(v) for v in np.round(rng.uniform(0.0, 1.0, 133), 3)], n_kpts=133), person(conf())]),
        'f09.json': document([person(conf()) for _ in range(6)]),
        'f10.json': document([{'person_id': [-1], 'pose_keypoints_2d': []}, person(conf(), n_numbers=3), person(conf())]),
    }


def special_folder():
    values = [1, 0, 0.1, 1e-05, 1.5, float('nan'), 0.30000000000000004, 0.1 + 0.7, 1e-4, 123456.789, 1e16, 1.0, 0.0, 2]
    return {f's{i:02d}.json': document([person(v, integers=isinstance(v, int)), person(values[(i + 1) % len(values)])]) for i, v in enumerate(values)}


def broken_folder(text):
    files = seeded_folder(5, 9, 2, stem='b{}')
    files['b2.json'] = text
    return files


def cases():
    """-> list of dicts: name, files {relative path: text}, json_dir, keypoints, output (relative), thresholds."""
    out = []

    def add(name, files, keypoints=DEFAULT, output='out', thresholds=None, json_dir='cam01_json'):
        out.append({'name': name, 'files': {f'{json_dir}/{fn}': text for fn, text in files.items()}, 'folders': [json_dir],
                    'json_dir': json_dir, 'keypoints': list(keypoints), 'output': output, 'thresholds': thresholds})

    add('one_file_one_person', {'only.json': document([person(0.875)])})
    add('files_257_three_persons', seeded_folder(257, 1, 3), thresholds=[0.3, 0.5])
    add('mixed_people_all_keypoints', mixed_folder(), keypoints=list(REF_NAMES), output='deep/er/out')
    add('six_persons_single_keypoint', seeded_folder(9, 2, 6), keypoints=['RHeel'])
    add('no_valid_entry', {'a.json': document([]), 'b.json': document([person(0.5, n_numbers=77)]), 'c.json': '{"version": 1.3}',
                           'd.json': document([{'person_id': [3]}])})
    add('name_given_twice', seeded_folder(4, 3, 2), keypoints=['Neck', 'Nose', 'Neck', 'LHeel'])
    add('special_confidences', special_folder(), keypoints=['Nose', 'RHeel'])
    add('error_unknown_name', seeded_folder(2, 4, 1), keypoints=['Nose', 'Elbow'])
    add('error_empty_folder', {}, keypoints=['Elbow'])
    add('error_people_null', broken_folder('{"version": 1.3, "people": null}'))
    add('error_top_level_list', broken_folder('[{"people": []}]'))
    add('error_top_level_number', broken_folder('1.5'))
    return out


def lay_out(case, work):
    shutil.rmtree(work, ignore_errors=True)
    os.makedirs(work)
    for d in case['folders']:
        os.makedirs(os.path.join(work, d), exist_ok=True)
    for rel, text in case['files'].items():
        with open(os.path.join(work, rel), 'w') as fh:
            fh.write(text)


def run_reference(ref, case):
    """-> (CSV bytes or None, stdout, stderr, (error type, message) or None, the output folder exists)."""
    work = os.path.join(WORK, case['name'])
    lay_out(case, work)
    output = os.path.join(work, case['output'])
    printed, warned, error = io.StringIO(), io.StringIO(), None
    try:
        with contextlib.redirect_stdout(printed), contextlib.redirect_stderr(warned), warnings.catch_warnings():
            warnings.simplefilter('ignore')                           # matplotlib's, about a plot without points
            assert ref.process(os.path.join(work, case['json_dir']), case['keypoints'], output, case['thresholds']) is None
    except Exception as e:
        error = (type(e).__name__, str(e))
    csv_path = os.path.join(output, 'confidence_timeline.csv')
    data = None
    if os.path.exists(csv_path):
        with open(csv_path, 'rb') as fh:
            data = fh.read()
    return data, ELAPSED.sub('in <t>s.', printed.getvalue()), warned.getvalue(), error, os.path.isdir(output)


def time_reference(ref):
    work = os.path.join(WORK, 'timing')
    case = {'folders': ['cam'], 'files': {f'cam/{fn}': text for fn, text in seeded_folder(6000, 77, 3).items()}}
    for rel, text in case['files'].items():                           # three persons in every file
        doc = json.loads(text)
        while len(doc['people']) < 3:
            doc['people'].append(person(0.5))
        case['files'][rel] = json.dumps(doc)
    lay_out(case, work)
    t0 = time.perf_counter()
    with contextlib.redirect_stdout(io.StringIO()), contextlib.redirect_stderr(io.StringIO()):
        ref.process(os.path.join(work, 'cam'), DEFAULT, os.path.join(work, 'out'), None)
    dt = time.perf_counter() - t0
    print(f'reference process(), one core, 6 000 frames x 3 persons x 4 keypoints: {dt:.2f} s ({dt / 6000 * 1e6:.0f} us per frame)')


def gen(timing=True):
    global REF_NAMES
    ref = load_reference()
    REF_NAMES = sorted(ref.HALPE_26_INDICES, key=ref.HALPE_26_INDICES.get)
    assert sorted(ref.HALPE_26_INDICES.values()) == list(range(26))
    out = {'work_root': np.array(WORK), 'halpe_names': np.array(json.dumps(REF_NAMES)), 'n_keypoints': np.array(ref.N_KEYPOINTS)}
    names = []
    for case in cases():
        n = case['name']
        names.append(n)
        data, printed, warned, error, made = run_reference(ref, case)
        out[f'{n}__files'] = np.array(json.dumps(case['files'], sort_keys=True))
        out[f'{n}__args'] = np.array(json.dumps({k: case[k] for k in ('json_dir', 'keypoints', 'output', 'thresholds', 'folders')}, sort_keys=True))
        out[f'{n}__csv'] = np.frombuffer(data if data is not None else b'', dtype=np.uint8)
        out[f'{n}__has_csv'] = np.array(data is not None)
        out[f'{n}__printed'] = np.array(printed)
        out[f'{n}__stderr'] = np.array(warned)
        out[f'{n}__error'] = np.array(json.dumps(error))
        out[f'{n}__folder_made'] = np.array(made)
        print(f'{n}: {len(case["files"])} files, CSV {None if data is None else len(data)} bytes, error {error}, output folder made: {made}')
    # what the docstring claims
    assert bytes(out['no_valid_entry__csv']) == b'frame,person,keypoint,confidence\r\n'
    special = bytes(out['special_confidences__csv']).decode()
    for text in (',1.0\r', ',0.0\r', ',0.1\r', ',1e-05\r', ',1.5\r', ',nan\r', ',0.30000000000000004\r', ',0.7999999999999999\r', ',0.0001\r', ',1e+16\r', ',2.0\r'):
        assert text in special, text
    assert 'f06.json' in str(out['mixed_people_all_keypoints__stderr']) and '\n10,2,Nose,' in bytes(out['mixed_people_all_keypoints__csv']).decode()
    assert '\n5,1,Nose,' in bytes(out['mixed_people_all_keypoints__csv']).decode() and '\n5,0,' not in bytes(out['mixed_people_all_keypoints__csv']).decode()
    twice = bytes(out['name_given_twice__csv']).decode().split('\r\n')
    assert [r.split(',')[2] for r in twice[1:4]] == ['Neck', 'Nose', 'LHeel'] and 'Keypoints: Neck, Nose, Neck, LHeel' in str(out['name_given_twice__printed'])
    errors = {n: json.loads(str(out[f'{n}__error'])) for n in names if n.startswith('error_')}
    assert [e[0] for e in errors.values()] == ['ValueError', 'FileNotFoundError', 'TypeError', 'AttributeError', 'AttributeError'], errors
    assert not out['error_unknown_name__folder_made'] and not out['error_empty_folder__folder_made'] and out['error_people_null__folder_made']
    out['cases'] = np.array(json.dumps(names))
    path = os.path.join(HERE, 'timeline_units.npz')
    save_npz(path, out)
    size = os.path.getsize(path)
    assert size < 1000000, size
    print(f'{len(names)} cases; {size} bytes -> {path}')
    if timing:
        time_reference(ref)
    shutil.rmtree(WORK, ignore_errors=True)


if __name__ == '__main__':
    gen(timing='--no-timing' not in sys.argv)
