"""Goldens of the reprojection utility, recorded through the reference's own code -> reproj_units.npz

Every case runs Pose2Sim/Utilities/reproj_from_trc_calib.py:reproj_from_trc_calib_func (imported through ref_shim: toml ->
tomli, cv2.Rodrigues / getOptimalNewCameraMatrix / projectPoints -> pose2sim_amd.cvmath, so the distorted cases are pinned
to that restatement, not to OpenCV itself) on a .trc and a calibration TOML written here, and stores

* the inputs as text and the arguments;
* the unrounded projections [C][F][K][2], from the reference's computeP + reprojection (or the shimmed cv2.projectPoints)
  called per (frame, marker, camera) as the utility calls them;
* the rounded and masked table [C][F][K][2]: the frames the utility hands to DataFrame.to_hdf, captured there (to_hdf is
  replaced by that recorder: pytables is absent, and with the real method no csv would be written);
* the list of files written and the text of every file, the directory the case ran in, what it printed;
* for the error cases the exception's type and message.

Cases: 2, 4 and 8 static cameras without and with distortion; a marker missing for some frames, one that leaves every
image, one behind a camera, markers planted within a tenth of a pixel of the four borders of camera 1 (both sides); a
zooming, a moving and a zooming + moving rig (8 rows, 6 camera frames); a .trc whose first frame is not 0; 1-frame and
1-marker files; calibrations with and without a metadata table; every output format alone and all together; an explicit
output root and a free-text markerset; no format (ValueError), cameras with different frame counts (ValueError), a camera
folder that already exists (the later folders are never made: FileNotFoundError after the first cameras' files, with the MMPose and with the OpenPose writer).

Tie condition: a value whose tenfold lies within 1e-6 of a half-integer could round either way under a reordered sum;
gen() refuses to write a fixture that holds one.  The file is written with fixed zip time stamps: running this script
again reproduces it byte for byte.  It also prints the reference's run time on 120 frames x 26 markers x 4 cameras.
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
import pandas as pd

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import ref_shim  # noqa: E402

from pose2sim_amd import synth, trc  # noqa: E402

WORK = os.path.join(os.path.realpath(tempfile.gettempdir()), 'reproj_golden_work')      # fixed: the MMPose files hold absolute paths


def load_reference():
    ref_shim.install()
    return importlib.import_module('Pose2Sim.Utilities.reproj_from_trc_calib')


def save_npz(path, arrays):
    """np.savez_compressed with fixed time stamps, so that the same arrays give the same bytes."""
    with zipfile.ZipFile(path, 'w', zipfile.ZIP_DEFLATED) as zf:
        for key, val in arrays.items():
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.asanyarray(val), allow_pickle=False)
            info = zipfile.ZipInfo(key + '.npy', date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            zf.writestr(info, buf.getvalue())


def trc_text(file_name, markers, frames, Q, rate=60):
    """Q [F][K][3] Z-up -> the text of a .trc file (rows as DataFrame.to_csv writes them: repr floats, NaN empty)."""
    rows = Q.reshape(len(Q), -1)[:, trc.yup_columns(len(markers))]
    lines = trc.header_lines(file_name, markers, rate, frames[0], len(frames))
    for fr, row in zip(frames, rows):
        lines.append('\t'.join([str(int(fr)), repr(float(fr / rate))] + ['' if np.isnan(v) else repr(float(v)) for v in row]))
    return '\n'.join(lines) + '\n'


def toml_value(v):
    if isinstance(v, (list, tuple, np.ndarray)):
        return '[ ' + ', '.join(toml_value(x) for x in v) + ']'
    return repr(float(v))


def toml_text(cams, per_frame=None, metadata=True, names=None):
    """per_frame: {'K': [C][Fp][3][3]} and / or {'R': [C][Fp][3], 'T': [C][Fp][3]} replace the static entries."""
    per_frame = per_frame or {}
    out = []
    for c in range(len(cams['K'])):
        name = names[c] if names else f'cam_{c + 1:02d}'
        out += [f'[{name}]', f'name = "{name}"', f'size = {toml_value(cams["S"][c])}',
                f'matrix = {toml_value(per_frame["K"][c] if "K" in per_frame else cams["K"][c])}',
                f'distortions = {toml_value(cams["dist"][c])}',
                f'rotation = {toml_value(per_frame["R"][c] if "R" in per_frame else cams["R"][c])}',
                f'translation = {toml_value(per_frame["T"][c] if "T" in per_frame else cams["T"][c])}', 'fisheye = false', '']
    if metadata:
        out += ['[metadata]', 'adjusted = false', 'error = 0.0']
    return '\n'.join(out) + '\n'


def world_point(cams, c, u, v, depth):
    """The point at `depth` m in front of camera c that the pinhole model puts on pixel (u, v)."""
    ray = np.linalg.inv(cams['K'][c]) @ np.array([u, v, 1.0])
    return cams['R_mat'][c].T @ (depth * ray - cams['T'][c])


def scene(C, F, K, seed, distort=False, special=False):
    """-> (cams, markers, Q [F][K'][3]).  special: a marker missing for some frames, one far outside every image, one behind
    camera 1, and eight planted a few hundredths of a pixel either side of the borders of camera 1."""
    cams = synth.make_cameras(C, seed=seed, distort=distort)
    Q = synth.make_points3d(F, 1, K, seed=seed)[:, 0]
    markers = [f'M{k:02d}' for k in range(K)]
    if special:
        Q[2:5, 3] = np.nan
        Q[F - 1, 0, 1] = np.nan                              # one coordinate only
        extra = {'Far': np.array([400.0, -250.0, 30.0]),
                 'Behind': -cams['R_mat'][0].T @ cams['T'][0] - 3.0 * cams['R_mat'][0][2]}
        w, h = cams['S'][0]
        for tag, (u, v) in {'L_in': (-0.04, 500.0), 'L_out': (-0.06, 500.0), 'R_out': (w - 0.04, 500.0), 'R_in': (w - 0.06, 500.0),
                            'T_in': (800.0, -0.04), 'T_out': (800.0, -0.06), 'B_out': (800.0, h - 0.04), 'B_in': (800.0, h - 0.06)}.items():
            extra[tag] = world_point(cams, 0, u, v, 4.5)
        Q = np.concatenate([Q, np.broadcast_to(np.array(list(extra.values()))[None], (F, len(extra), 3))], axis=1)
        markers += list(extra)
    return cams, markers, np.ascontiguousarray(Q)


def moving_rig(cams, n, seed, zoom, move):
    rng = np.random.default_rng(seed)
    per = {}
    C = len(cams['K'])
    if zoom:
        per['K'] = [[cams['K'][c] * np.array([[1 + 0.02 * f, 1, 1], [1, 1 + 0.02 * f, 1], [1, 1, 1]]) for f in range(n)] for c in range(C)]
    if move:
        per['R'] = [[cams['R'][c] + rng.normal(0, 0.004, 3) * f for f in range(n)] for c in range(C)]
        per['T'] = [[cams['T'][c] + rng.normal(0, 0.01, 3) * f for f in range(n)] for c in range(C)]
    return per


def cases():
    """-> list of dicts: name, trc file name, trc text, toml text, args (without the paths), prepare (folders to make first)."""
    out = []

    def add(name, cams, markers, Q, args, first_frame=0, per_frame=None, metadata=True, trc_name='trial.trc', premade=(), names=None):
        frames = np.arange(first_frame, first_frame + len(Q))
        out.append({'name': name, 'trc_name': trc_name, 'trc': trc_text(trc_name, markers, frames, Q),
                    'toml': toml_text(cams, per_frame, metadata, names), 'args': args, 'premade': list(premade)})

    o, d, m, u = {'openpose': True}, {'deeplabcut': True}, {'mmpose': True}, {'undistort_points': True}
    everything = {**o, **d, **m}
    for C, fmt, F, K, seed in ((2, o, 8, 26, 11), (4, everything, 12, 26, 12), (8, m, 6, 12, 13)):
        cams, markers, Q = scene(C, F, K, seed, special=(C == 4))
        add(f'static{C}', cams, markers, Q, fmt)
    for C, fmt, F, K, seed in ((2, {**d, **u}, 8, 26, 21), (4, {**everything, **u}, 12, 26, 22), (8, {**o, **u}, 6, 12, 23)):
        cams, markers, Q = scene(C, F, K, seed, distort=True, special=(C == 4))
        add(f'distorted{C}', cams, markers, Q, fmt)
    for name, zoom, move, seed in (('zooming', True, False, 31), ('moving', False, True, 32), ('zooming_moving', True, True, 33)):
        cams, markers, Q = scene(3, 8, 10, seed)
        add(name, cams, markers, Q, everything, per_frame=moving_rig(cams, 6, seed, zoom, move))
    cams, markers, Q = scene(3, 5, 10, 34)
    add('more_camera_frames_than_rows', cams, markers, Q, o, per_frame=moving_rig(cams, 7, 34, True, True))
    cams, markers, Q = scene(3, 7, 8, 41)
    add('first_frame_37', cams, markers, Q, everything, first_frame=37, trc_name='walk_37-43.trc')
    cams, markers, Q = scene(2, 1, 9, 42)
    add('one_frame', cams, markers, Q, everything)
    cams, markers, Q = scene(2, 6, 1, 43)
    add('one_marker', cams, markers, Q, everything)
    cams, markers, Q = scene(2, 6, 1, 43, distort=True)
    add('one_marker_distorted', cams, markers, Q, {**everything, **u})
    cams, markers, Q = scene(3, 5, 7, 44)
    add('no_metadata_named_cameras', cams, markers, Q, everything, metadata=False, names=['left', 'int_cam7', 'capture_volume'])
    add('output_root_and_markerset', cams, markers, Q, {**m, **o, 'markerset': 'custom', 'output_file_root': 'elsewhere/out'})
    add('dotted_name', cams, markers, Q, o, trc_name='s01.t02.filt.trc')
    add('error_no_format', cams, markers, Q, {})
    add('error_no_format_markerset', cams, markers, Q, {'markerset': 'halpe26', 'undistort_points': True})
    per = moving_rig(cams, 6, 45, True, False)
    per['K'][1] = per['K'][1][:4]
    add('error_ragged_frames', cams, markers, Q, o, per_frame=per)
    add('error_premade_folder', cams, markers, Q, m, premade=['trial_reproj', 'trial_reproj/cam02_json'])
    add('error_premade_folder_openpose', cams, markers, Q, o, premade=['trial_reproj', 'trial_reproj/cam02_json'])
    return out


def run_reference(ref, case, capture):
    """Runs the utility in WORK/<name>; -> (dir, files {relative path: text}, printed text, (error type, message) or None)."""
    work = os.path.join(WORK, case['name'])
    shutil.rmtree(work, ignore_errors=True)
    os.makedirs(work)
    for rel in case['premade']:
        os.makedirs(os.path.join(work, rel))
    trc_path, toml_path = os.path.join(work, case['trc_name']), os.path.join(work, 'Calib.toml')
    with open(trc_path, 'w') as fh:
        fh.write(case['trc'])
    with open(toml_path, 'w') as fh:
        fh.write(case['toml'])
    args = dict(case['args'])
    if args.get('output_file_root'):
        args['output_file_root'] = os.path.join(work, args['output_file_root'])
        os.makedirs(os.path.dirname(args['output_file_root']))
    full = {'input_trc_file': trc_path, 'input_calib_file': toml_path, 'openpose': False, 'deeplabcut': False, 'mmpose': False,
            'markerset': None, 'undistort_points': False, 'output_file_root': None, **args}
    before = {os.path.join(r, f) for r, _, fs in os.walk(work) for f in fs}
    error, printed = None, io.StringIO()
    real_to_hdf = pd.DataFrame.to_hdf
    pd.DataFrame.to_hdf = lambda self, *a, **k: capture.append(self.to_numpy(dtype=np.float64).copy())
    try:
        with contextlib.redirect_stdout(printed), warnings.catch_warnings():
            warnings.simplefilter('ignore')
            ref.reproj_from_trc_calib_func(**full)
    except Exception as e:
        error = (type(e).__name__, str(e))
    finally:
        pd.DataFrame.to_hdf = real_to_hdf
    files, folders = {}, []
    for r, ds, fs in os.walk(work):
        folders += [os.path.relpath(os.path.join(r, x), work) for x in ds]
        for f in fs:
            p = os.path.join(r, f)
            if p not in before:
                with open(p) as fh:
                    files[os.path.relpath(p, work)] = fh.read()
    return work, files, sorted(folders), printed.getvalue(), error


def reference_arrays(ref, case, work):
    """The unrounded projections, per (frame, marker, camera) through the reference's own functions, and the table
    captured from a deeplabcut run of the same inputs."""
    import cv2
    trc_path, toml_path = os.path.join(work, case['trc_name']), os.path.join(work, 'Calib.toml')
    undistort = bool(case['args'].get('undistort_points'))
    _, data = ref.df_from_trc(trc_path)
    Qz = ref.yup2zup(data.iloc[:, 2:]).to_numpy(dtype=np.float64)
    P = ref.computeP(toml_path, undistort=undistort)
    prm = ref.retrieve_calib_params(toml_path)
    C = len(P)
    F = len(Qz) if P.shape[1] == 1 else min(P.shape[1], len(Qz))
    K = Qz.shape[1] // 3
    raw = np.empty((C, F, K, 2))
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        for f in range(F):
            Pf = [P[c][0] if P.shape[1] == 1 else P[c][f] for c in range(C)]
            for k in range(K):
                q = np.append(Qz[f, 3 * k:3 * k + 3], 1)
                if undistort:
                    for c in range(C):
                        raw[c, f, k] = cv2.projectPoints(np.array(q[:-1]), prm['R'][c], prm['T'][c], prm['K'][c], prm['dist'][c])[0][0, 0]
                else:
                    x, y = ref.reprojection(Pf, q)
                    raw[:, f, k, 0], raw[:, f, k, 1] = x, y
    captured = []
    probe = dict(case, name=case['name'] + '__table', premade=[],
                 args={'deeplabcut': True, 'undistort_points': undistort})
    _, _, _, _, err = run_reference(ref, probe, captured)
    assert err is None and len(captured) == C, (case['name'], err)
    shutil.rmtree(os.path.join(WORK, probe['name']))
    return raw, np.stack(captured).reshape(C, F, K, 2)


def time_reference(ref):
    cams, markers, Q = scene(4, 120, 26, 5)
    case = {'name': 'timing', 'trc_name': 'trial.trc', 'trc': trc_text('trial.trc', markers, np.arange(120), Q),
            'toml': toml_text(cams), 'premade': []}
    for label, args in (('OpenPose only', {'openpose': True}), ('all three formats', {'openpose': True, 'deeplabcut': True, 'mmpose': True})):
        t0 = time.perf_counter()
        run_reference(ref, dict(case, args=args), [])
        print(f'reference, one core, 120 frames x 26 markers x 4 cameras, {label}: {time.perf_counter() - t0:.1f} s')
    shutil.rmtree(os.path.join(WORK, 'timing'))


def gen(timing=True):
    ref = load_reference()
    out = {'work_root': np.array(WORK)}
    names = []
    n_values = worst_tie = 0
    for case in cases():
        n = case['name']
        names.append(n)
        work, files, folders, printed, error = run_reference(ref, case, [])
        out[f'{n}__trc_name'] = np.array(case['trc_name'])
        out[f'{n}__trc'] = np.array(case['trc'])
        out[f'{n}__toml'] = np.array(case['toml'])
        out[f'{n}__args'] = np.array(json.dumps(case['args'], sort_keys=True))
        out[f'{n}__premade'] = np.array(json.dumps(case['premade']))
        out[f'{n}__files'] = np.array(json.dumps(files, sort_keys=True))
        out[f'{n}__folders'] = np.array(json.dumps(folders))
        out[f'{n}__printed'] = np.array(printed)
        out[f'{n}__error'] = np.array(json.dumps(error))
        if not n.startswith('error_no_format') and n != 'error_ragged_frames':
            raw, table = reference_arrays(ref, case, work)
            with np.errstate(invalid='ignore'):
                frac = np.abs(np.abs(raw * 10 - np.floor(raw * 10)) - 0.5)
            frac = frac[np.isfinite(frac)]
            if frac.size and frac.min() <= 1e-6:
                raise SystemExit(f'{n}: a value lies {frac.min():.2e} from a rounding tie: change the seed')
            n_values += frac.size
            worst_tie = min(worst_tie or 1.0, frac.min()) if frac.size else worst_tie
            out[f'{n}__raw'] = raw
            out[f'{n}__table'] = table
        shutil.rmtree(work)
    out['cases'] = np.array(json.dumps(names))
    path = os.path.join(HERE, 'reproj_units.npz')
    save_npz(path, out)
    print(f'{len(names)} cases, {n_values} projected values, nearest rounding tie {worst_tie:.2e} tenths of a pixel away; '
          f'{os.path.getsize(path)} bytes -> {path}')
    if timing:
        time_reference(ref)
    shutil.rmtree(WORK, ignore_errors=True)


if __name__ == '__main__':
    gen(timing='--no-timing' not in sys.argv)
