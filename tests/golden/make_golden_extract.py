"""Goldens of the primary-person extraction, recorded through the reference's own code -> extract_units.npz

Every case runs Pose2Sim/Utilities/pose_extract_person.py (imported through ref_shim; its progress bar replaced by the plain
iterator) -- process(), or main() with a command line -- on OpenPose JSON folders written here, and stores the input files
as text, the call, every file found outside the input folder afterwards as text, stdout (its seconds field set to 0.0), the
Warning / Error lines of stderr,
and the exception's type and message.

Cases: two and three persons that cross, listed in shuffled order, with gaps (no 'people' key, an empty list) and the
tracked person sometimes weaker than the others; the hand-made corner-case camera of make_golden_jitter.py (a short list
beside a full one, no list, one and no valid keypoint, NaN values); an all-integer list; an integer list with one float;
NaN and Infinity values; a file that is not JSON between two multi-person frames; "people": null, a 133-keypoint list, a
top-level list and a person that is a number, each in the middle of a run; a short list beside a full one; a frame whose
candidates share no keypoint with the previous choice; main() on an input path with a trailing '/' and no -o; main() with
an existing output folder that holds files; process() with a missing output folder; a 1-file folder; a folder without JSON
files; a missing input folder for main().

gen() asserts that the proximity rule and the most-valid rule disagree on at least one recorded frame, and that at least
one recorded frame's choice changes when the previous choice is swapped for another candidate of that previous frame: a
selection that forgot its state could not reproduce these files.  The file is written with fixed zip time stamps: running
this script again reproduces it byte for byte.  It also prints the time of the reference's process() per 1 000 frames.
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

from make_golden_jitter import camera_files, document, lay_out, person, rules_disagree, save_npz, special_camera  # noqa: E402

WORK = os.path.join(os.path.realpath(tempfile.gettempdir()), 'extract_golden_work')     # fixed: the printed lines hold it


def load_reference():
    ref_shim.install()
    ref = importlib.import_module('Pose2Sim.Utilities.pose_extract_person')
    ref.tqdm = lambda it, **kwargs: it                       # no progress bar: stderr holds the warnings alone
    return ref


def base_person(seed, shift=0.0):
    rng = np.random.default_rng(seed)
    kp = np.stack([rng.uniform(600, 900, 26) + shift, rng.uniform(300, 800, 26), rng.uniform(0.3, 0.95, 26)], axis=1)
    return np.round(kp, 2)


def two_people(f, order=True):
    """Two persons 300 px apart that drift slowly; listed A, B or B, A."""
    a, b = base_person(1, 2.0 * f), base_person(2, 300.0 - 2.0 * f)
    return [person(a), person(b)] if order else [person(b), person(a)]


def int_person(seed, shift=0):
    rng = np.random.default_rng(seed)
    vals = np.stack([rng.integers(600, 900, 26) + shift, rng.integers(300, 800, 26), np.ones(26, dtype=np.int64)], axis=1)
    return {'person_id': [-1], 'pose_keypoints_2d': [int(v) for v in vals.ravel()]}


def run_of(special, at=3, F=7):
    """F two-person frames named f000.json ..., the file at `at` replaced by the text `special`."""
    files = {f'f{f:03d}.json': document(two_people(f, order=f % 2 == 0)) for f in range(F)}
    files[f'f{at:03d}.json'] = special
    return files


def cases():
    out = []

    def add(name, files, mode='process', input_dir='cam01_json', output='out', argv=None, folders=(), extra=None, make_input=True):
        all_files = {f'{input_dir.rstrip("/")}/{fn}': text for fn, text in files.items()}
        all_files.update(extra or {})
        out.append({'name': name, 'files': all_files, 'folders': [input_dir.rstrip('/')] * make_input + list(folders), 'mode': mode,
                    'input': input_dir, 'output': output, 'argv': argv})

    add('two_crossing', camera_files(60, 1, n_persons=2, gaps=(21, 22, 24, 25), p_weak=0.4), folders=['out'])
    add('three_crossing', camera_files(60, 2, n_persons=3, gaps=(30, 31, 33), p_weak=0.4), folders=['out'])
    add('special', special_camera(), folders=['out'])
    ints = {f'f{f:03d}.json': json.dumps({'version': 1.3, 'people': [int_person(3, f), int_person(4, 200 - f)][::1 if f % 2 else -1]}) for f in range(6)}
    add('all_integer', ints, folders=['out'])
    mixed = {}
    for f in range(6):
        a, b = int_person(3, f), int_person(4, 200 - f)
        a['pose_keypoints_2d'][40] = 300.5                   # one float: the whole list is written as floats
        b['pose_keypoints_2d'][0] = 700                      # all integers beside it
        if f >= 3:
            a['pose_keypoints_2d'] = a['pose_keypoints_2d'][:51]   # a short list: the all-integer person is taken from here on
        mixed[f'f{f:03d}.json'] = json.dumps({'version': 1.3, 'people': [b, a] if f % 2 else [a, b]})
    add('integer_one_float', mixed, folders=['out'])
    odd = {}
    for f in range(6):
        a, b = base_person(5, f), base_person(6, 250.0 - f)
        a[3, 0] = np.nan                                     # NaN x of a confident keypoint
        a[4, 2] = np.nan                                     # NaN confidence
        a[5, 1], a[5, 2] = np.inf, 0.05                      # infinite coordinates of keypoints that are not valid
        a[6, 0], a[6, 2] = -np.inf, 0.05
        a[7, 2] = np.inf                                     # an infinite confidence is above the threshold
        if f == 0:
            b[10:14, 2] = 0.05                               # the first choice is A, by the number of confidences
        if f == 3:
            b[8, 1] = np.nan                                 # a NaN y: that mean is NaN
        odd[f'f{f:03d}.json'] = document([person(a), person(b)] if f % 2 else [person(b), person(a)])
    add('nan_infinity', odd, folders=['out'])
    add('bad_file_between', run_of('{bad'), folders=['out'])
    add('error_people_null', run_of('{"version": 1.3, "people": null}'), folders=['out'])
    long_list = document([person(base_person(7)), person(np.round(np.random.default_rng(5).uniform(0.2, 900, 399), 2))])
    add('error_133_keypoints', run_of(long_list), folders=['out'])
    add('error_top_level_list', run_of('[1, 2]'), folders=['out'])
    add('error_person_number', run_of('{"version": 1.3, "people": [7]}'), folders=['out'])
    short = run_of(document([person(base_person(1, 6.0).ravel()[:51]), person(base_person(2, 294.0)), person(base_person(1, 6.0))]))
    add('short_beside_full', short, folders=['out'])
    apart = {}
    for f in range(6):
        a, b = base_person(1, 2.0 * f), base_person(2, 300.0 - 2.0 * f)
        if f == 0:
            b[:, 2] = 0.05                                   # one candidate: A, valid on the first half only
            a[13:, 2] = 0.05
        if f == 1:
            a[:13, 2] = 0.05                                 # both valid on the second half only: nothing shared with the choice
            b[:13, 2] = 0.05
            b[20, 2] = 0.05                                  # A has more confidences: the fallback takes it, listed second
        apart[f'f{f:03d}.json'] = document([person(b), person(a)])
    add('no_shared_keypoint', apart, folders=['out'])
    add('main_trailing_slash', run_of(document([])), mode='main', input_dir='cam02_json/', output=None, argv=['-i', 'cam02_json/'])
    add('main_existing_output', run_of(document(two_people(3))), mode='main', argv=['-i', 'cam01_json', '-o', 'out'], folders=['out'],
        extra={'out/old.json': '{"kept": true}', 'out/f001.json': 'overwritten'})
    add('error_process_missing_output', run_of(document(two_people(3))), output='nowhere/out')
    add('one_file', {'only.json': document(two_people(0))}, folders=['out'])
    add('error_no_json', {}, folders=['out'], extra={'cam01_json/readme.txt': 'no frames'})
    add('error_main_missing_input', {}, mode='main', input_dir='absent_json', argv=['-i', 'absent_json'], output=None, make_input=False)
    return out


def run_reference(ref, case, selections):
    work = os.path.join(WORK, case['name'])
    lay_out(case, work)
    error, printed, errors = None, io.StringIO(), io.StringIO()
    real_select = ref._select_person

    def select(people, prev):
        chosen = real_select(people, prev)
        selections.append((people, prev, chosen))
        return chosen
    ref._select_person = select
    cwd, argv = os.getcwd(), sys.argv
    os.chdir(work)
    try:
        with contextlib.redirect_stdout(printed), contextlib.redirect_stderr(errors), warnings.catch_warnings():
            warnings.simplefilter('ignore')
            if case['mode'] == 'main':
                sys.argv = ['pose_extract_person'] + case['argv']
                ref.main()
            else:
                ref.process(os.path.join(work, case['input']), os.path.join(work, case['output']))
    except BaseException as e:                               # SystemExit included
        error = (type(e).__name__, str(e))
    finally:
        os.chdir(cwd)
        sys.argv = argv
        ref._select_person = real_select
    inside = os.path.join(work, case['input'].rstrip('/')) + os.sep
    found = {}
    for r, _, fs in os.walk(work):
        for f in fs:
            p = os.path.join(r, f)
            if not p.startswith(inside):
                with open(p, encoding='utf-8', newline='') as fh:
                    found[os.path.relpath(p, work)] = fh.read()
    lines = [ln for ln in errors.getvalue().splitlines() if ln.startswith(('Warning:', 'Error:'))]
    return found, printed.getvalue(), lines, error


def candidates_of(people):
    c = [np.array(p.get('pose_keypoints_2d', [])) for p in people if isinstance(p, dict)]
    c = [k.reshape(26, 3) for k in c if k.size == 78]
    return [k for k in c if ((k[:, 2] > 0.1) & ~np.isnan(k[:, 0])).any()]


def depends_on_state(ref, selections):
    """Frames whose choice changes when the previous choice is swapped for another candidate of the previous selecting frame."""
    n, before = 0, None
    for people, prev, chosen in selections:
        if prev is None:
            before = None
        if chosen is None:
            continue
        if before is not None and prev is not None and len(candidates_of(people)) >= 2:
            for other in before:
                if not np.array_equal(other, prev, equal_nan=True) and not np.array_equal(ref._select_person(people, other), chosen, equal_nan=True):
                    n += 1
                    break
        before = candidates_of(people)
    return n


def time_reference(ref):
    work = os.path.join(WORK, 'timing')
    lay_out({'folders': ['cam', 'out'], 'files': {f'cam/{fn}': t for fn, t in camera_files(1000, 77, n_persons=3).items()}}, work)
    t0 = time.perf_counter()
    with contextlib.redirect_stdout(io.StringIO()), contextlib.redirect_stderr(io.StringIO()):
        ref.process(os.path.join(work, 'cam'), os.path.join(work, 'out'))
    print(f'reference process(), one core, 1 000 frames x 3 persons: {time.perf_counter() - t0:.3f} s')


def gen(timing=True):
    ref = load_reference()
    out = {'work_root': np.array(WORK)}
    names, selections = [], []
    for case in cases():
        n = case['name']
        names.append(n)
        first = len(selections)
        found, printed, lines, error = run_reference(ref, case, selections)
        out[f'{n}__files'] = np.array(json.dumps(case['files'], sort_keys=True))
        out[f'{n}__folders'] = np.array(json.dumps(case['folders']))
        out[f'{n}__call'] = np.array(json.dumps({'mode': case['mode'], 'input': case['input'], 'output': case['output'], 'argv': case['argv']}))
        out[f'{n}__found'] = np.array(json.dumps(found, sort_keys=True))
        out[f'{n}__printed'] = np.array(re.sub(r'processed in \d+\.\ds\.', 'processed in 0.0s.', printed))   # the one field that varies
        out[f'{n}__stderr'] = np.array(json.dumps(lines))
        out[f'{n}__error'] = np.array(json.dumps(error))
        shutil.rmtree(os.path.join(WORK, n))
        print(f'{n}: {len(found)} files found, {len(selections) - first} selections, {len(lines)} stderr lines, error {error}')
    disagree = sum(rules_disagree(*s) for s in selections)
    stateful = depends_on_state(ref, selections)
    assert disagree >= 1, 'no frame where the proximity rule and the most-valid rule disagree'
    assert stateful >= 1, 'no frame whose choice depends on the previous choice'
    out['cases'] = np.array(json.dumps(names))
    path = os.path.join(HERE, 'extract_units.npz')
    save_npz(path, out)
    print(f'{len(names)} cases, {disagree} frames where the two rules disagree, {stateful} whose choice depends on the previous one; '
          f'{os.path.getsize(path)} bytes -> {path}')
    if timing:
        time_reference(ref)
    shutil.rmtree(WORK, ignore_errors=True)


if __name__ == '__main__':
    gen(timing='--no-timing' not in sys.argv)
