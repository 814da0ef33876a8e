"""Record tests/golden/measure_units.npz from the reference's own Pose2Sim.common functions (through ref_shim):
best_coords_for_measurements, mean_angles, compute_height, compute_leg_length, trimmed_mean, and euclidean_distance +
trimmed_mean for the segment lengths of kinematics.dict_segment_ratio.  Build container only.

    python tests/golden/make_golden_measure.py
    taskset -c 0 python tests/golden/make_golden_measure.py --time 36000    # the reference's time on one file, one core

What is recorded
  trials   synthetic .trc files of a HALPE_26-like person written here (their text, as bytes): walking, standing, crouching,
           in m and in px, with markers left out, with NaN gaps, from 1 to 1 500 frames
  cases    per case: the trial, the function, its arguments, and from the reference the return value, the log records, the
           exception type; for a returned frame its columns, index, a digest of its bytes and, for short ones, its values;
           the mean angles and the row heights the reference computed on the way (its mean_angles and trimmed_mean calls are
           intercepted), and the summed speeds from the reference's expression

The kernels agree with the reference to a tolerance on the angles while the selection is discrete, so every case keeps its
mean angles 1e-6 degrees away from large_hip_knee_angles and, where the 50-smallest branch runs, the 51 smallest angles 1e-6
apart: conditions on the INPUTS, asserted here on what the reference computed; a trial that fails is generated again with
another seed.
"""
import json
import logging
import os
import sys
import tempfile
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import ref_shim  # noqa: E402
import measure_numpy  # noqa: E402

MARGIN = 1e-6
HALPE_26 = ['Nose', 'LEye', 'REye', 'LEar', 'REar', 'LShoulder', 'RShoulder', 'LElbow', 'RElbow', 'LWrist', 'RWrist', 'LHip', 'RHip',
            'LKnee', 'RKnee', 'LAnkle', 'RAnkle', 'Head', 'Neck', 'Hip', 'LBigToe', 'RBigToe', 'LSmallToe', 'RSmallToe', 'LHeel', 'RHeel']
BODY_9 = ['Nose', 'LShoulder', 'RShoulder', 'LHip', 'RHip', 'LKnee', 'RKnee', 'LAnkle', 'RAnkle']
SEGMENTS = [['RKnee', 'RAnkle'], ['LHip', 'LKnee'], ['RShoulder', 'LHip'], ['Nose', 'RHip']]


def without(*names):
    return [m for m in HALPE_26 if m not in names]


def make_trial(kind, n, unit, markers, seed, gaps=0.0, all_nan=(), flex=1.0):
    """-> the text of a .trc: a person walking along X (Y up), standing or crouching; metres, or pixels at 400 per metre."""
    rng = np.random.default_rng(seed)
    fps, period = 60, 1.1
    t = np.arange(n) / fps
    speed, hip_amp, knee_amp, knee_0, hip_0, noise = {'walk': (1.3, 25.0, 50.0, 5.0, 0.0, 0.002), 'stand': (0.0, 0.0, 0.0, 3.0, 0.0, 0.0004),
                                                      'crouch': (0.6, 10.0, 15.0, 100.0, 75.0, 0.002)}[kind]
    pos = {}
    pelvis = np.stack([0.3 + speed * t, 0.92 - 0.25 * (kind == 'crouch') + 0.02 * np.sin(4 * np.pi * t / period), np.zeros(n)], axis=1)
    up = np.array([0.0, 1.0, 0.0])
    pos['Hip'] = pelvis
    pos['Neck'] = pelvis + 0.52 * up + [0.02, 0, 0]
    pos['Head'] = pos['Neck'] + 0.26 * up
    pos['Nose'] = pos['Neck'] + 0.15 * up + [0.1, 0, 0]
    for side, z, phase0 in (('R', 0.1, 0.0), ('L', -0.1, 0.5)):
        ph = 2 * np.pi * (t / period + phase0)
        a = np.radians(flex * (hip_0 + hip_amp * np.sin(ph)))
        k = np.radians(flex * (knee_0 + knee_amp * (1 - np.cos(ph + 0.6)) / 2))
        hip = pelvis + [0, 0, z]
        knee = hip + 0.42 * np.stack([np.sin(a), -np.cos(a), np.zeros(n)], axis=1)
        ankle = knee + 0.43 * np.stack([np.sin(a - k), -np.cos(a - k), np.zeros(n)], axis=1)
        pos[side + 'Hip'], pos[side + 'Knee'], pos[side + 'Ankle'] = hip, knee, ankle
        pos[side + 'Heel'] = ankle + [-0.05, -0.06, 0]
        pos[side + 'BigToe'] = ankle + [0.16, -0.07, 0]
        pos[side + 'SmallToe'] = ankle + [0.13, -0.07, 0.4 * z]
        shoulder = pos['Neck'] + [0, -0.02, 1.8 * z]
        swing = np.radians(20 * np.sin(ph + np.pi))
        elbow = shoulder + 0.3 * np.stack([np.sin(swing), -np.cos(swing), np.zeros(n)], axis=1)
        pos[side + 'Shoulder'], pos[side + 'Elbow'] = shoulder, elbow
        pos[side + 'Wrist'] = elbow + 0.26 * np.stack([np.sin(swing + 0.3), -np.cos(swing + 0.3), np.zeros(n)], axis=1)
        pos[side + 'Eye'] = pos['Nose'] + [-0.02, 0.04, 0.3 * z]
        pos[side + 'Ear'] = pos['Nose'] + [-0.09, 0.02, 0.7 * z]
    scale, digits = (1.0, 4) if unit == 'm' else (400.0, 1)
    table = np.concatenate([pos[m] for m in markers], axis=1)
    table = (table + rng.normal(0, noise, table.shape)) * scale
    hole = rng.random((n, len(markers))) < gaps
    for name in all_nan:
        hole[:, markers.index(name)] = True
    lines = ['PathFileType\t4\t(X/Y/Z)\ttrial.trc\n',
             'DataRate\tCameraRate\tNumFrames\tNumMarkers\tUnits\tOrigDataRate\tOrigDataStartFrame\tOrigNumFrames\n',
             f'{fps}\t{fps}\t{n}\t{len(markers)}\t{unit}\t{fps}\t0\t{n}\n',
             'Frame#\tTime\t' + '\t\t\t'.join(markers) + '\t\t\n',
             '\t\t' + '\t'.join(f'{a}{k + 1}' for k in range(len(markers)) for a in 'XYZ') + '\n']
    for i in range(n):
        cells = ['' if hole[i, j // 3] else f'{table[i, j]:.{digits}f}' for j in range(table.shape[1])]
        lines.append(f'{i + 1}\t{t[i]:.4f}\t' + '\t'.join(cells) + '\n')
    return ''.join(lines)


# name: (kind, frames, unit, markers, options)
TRIALS = {
    'walk_m': ('walk', 300, 'm', HALPE_26, {}),
    'walk_px': ('walk', 150, 'px', HALPE_26, {}),
    'deep_m': ('walk', 70, 'm', HALPE_26, {'flex': 1.9}),
    'deep_px': ('walk', 70, 'px', without('Hip', 'Neck'), {'flex': 1.9}),
    'no_hip': ('walk', 70, 'm', without('Hip'), {}),
    'no_neck': ('walk', 70, 'm', without('Neck'), {}),
    'no_head': ('walk', 70, 'm', without('Head'), {}),
    'no_heels': ('walk', 70, 'm', without('LHeel', 'RHeel'), {}),
    'no_rheel': ('walk', 70, 'px', without('RHeel'), {}),
    'body_1500': ('walk', 1500, 'm', BODY_9, {'flex': 1.7}),
    'no_rknee': ('walk', 70, 'm', without('RKnee'), {}),
    'no_lankle': ('walk', 70, 'px', without('LAnkle'), {}),
    'no_rshoulder': ('walk', 70, 'm', without('RShoulder'), {}),
    'no_lhip_no_hip': ('walk', 70, 'm', without('LHip', 'Hip'), {}),
    'no_lhip': ('walk', 70, 'm', without('LHip'), {}),
    'no_head_no_nose': ('walk', 70, 'm', without('Head', 'Nose'), {}),
    'stand_m': ('stand', 70, 'm', HALPE_26, {}),
    'stand_px': ('stand', 70, 'px', without('Hip', 'Neck', 'Head'), {}),
    'crouch': ('crouch', 70, 'm', HALPE_26, {}),
    'crouch_40': ('crouch', 40, 'm', HALPE_26, {}),
    'crouch_nan_knees': ('crouch', 70, 'm', HALPE_26, {'all_nan': ('RKnee', 'LKnee')}),
    'walk_nan_head': ('walk', 70, 'm', HALPE_26, {'all_nan': ('Head',)}),
    'gaps_m': ('walk', 70, 'm', HALPE_26, {'gaps': 0.04}),
    'gaps_px': ('walk', 70, 'px', without('Hip', 'Neck'), {'gaps': 0.15}),
    'len_1': ('walk', 1, 'm', HALPE_26, {}),
    'len_2': ('walk', 2, 'm', HALPE_26, {}),
    'len_49': ('walk', 49, 'm', HALPE_26, {}),
    'len_50': ('walk', 50, 'm', HALPE_26, {}),
    'len_51': ('walk', 51, 'px', HALPE_26, {}),
}


def case_list():
    cases = []

    def add(trial, func, **kwargs):
        cases.append({'name': f'{trial}-{func}' + ''.join(f'-{k}={v}' for k, v in sorted(kwargs.items()) if k != 'pairs'),
                      'trial': trial, 'func': func, 'kwargs': kwargs})
    for trial, (_, _, unit, markers, _) in TRIALS.items():
        speed = 0.2 if unit == 'm' else 50
        add(trial, 'best_coords_for_measurements', close_to_zero_speed=speed)
        add(trial, 'compute_height', close_to_zero_speed=speed)
        add(trial, 'compute_leg_length', close_to_zero_speed=speed)
        add(trial, 'mean_angles')
        add(trial, 'segment_lengths', pairs=SEGMENTS)
    for trial in ('walk_m', 'deep_px', 'gaps_m', 'len_51', 'len_2'):
        speed = 0.2 if TRIALS[trial][2] == 'm' else 50
        for pct in (0, 0.1, 0.5, 1.0):
            add(trial, 'best_coords_for_measurements', close_to_zero_speed=speed, fastest_frames_to_remove_percent=pct)
            add(trial, 'compute_height', close_to_zero_speed=speed, fastest_frames_to_remove_percent=pct, trimmed_extrema_percent=pct)
            add(trial, 'compute_leg_length', close_to_zero_speed=speed, fastest_frames_to_remove_percent=pct, trimmed_extrema_percent=pct)
            add(trial, 'segment_lengths', pairs=SEGMENTS, trimmed_extrema_percent=pct)
    add('walk_m', 'compute_height')                                   # the defaults: 50 on a file in metres, nothing moves enough
    add('walk_px', 'best_coords_for_measurements')                    # and 0.2 on a file in pixels
    add('deep_m', 'compute_height', close_to_zero_speed=0.2, large_hip_knee_angles=30)
    add('deep_m', 'best_coords_for_measurements', close_to_zero_speed=0.2, large_hip_knee_angles=20)
    add('body_1500', 'best_coords_for_measurements', close_to_zero_speed=0.1, large_hip_knee_angles=40)
    add('walk_m', 'segment_lengths', pairs=[['RKnee', 'Tail']])
    return cases


class Capture(logging.Handler):
    def __init__(self):
        super().__init__(level=logging.DEBUG)
        self.records = []

    def emit(self, record):
        self.records.append([record.levelname, record.getMessage()])


def run_case(common, case, text, path):
    """-> the record of one case from the reference."""
    Q_coords, markers = measure_numpy.read_trc_text(text)
    kw = dict(case['kwargs'])
    seen = {'ang_mean': [], 'heights': []}
    real_angles, real_trim = common.mean_angles, common.trimmed_mean

    def spy_angles(*a, **k):
        out = real_angles(*a, **k)
        seen['ang_mean'].append(np.array(out, dtype=np.float64))
        return out

    def spy_trim(arr, *a, **k):
        seen['heights'].append(np.array(arr, dtype=np.float64))
        return real_trim(arr, *a, **k)
    cap = Capture()
    root = logging.getLogger()
    root.addHandler(cap)
    old_level = root.level
    root.setLevel(logging.DEBUG)
    rec = {'exc': '', 'arrays': {}}
    func = case['func']
    try:
        if func != 'mean_angles':
            common.mean_angles = spy_angles
        if func in ('compute_height', 'compute_leg_length'):
            common.trimmed_mean = spy_trim
        with np.errstate(all='ignore'):
            if func == 'best_coords_for_measurements':
                frame = common.best_coords_for_measurements(Q_coords, markers, **kw)
                rec['columns'] = [str(c) for c in frame.columns]
                rec['digest'] = measure_numpy.frame_digest(frame)
                rec['arrays']['index'] = np.asarray(frame.index, dtype=np.int64)
                if len(frame) <= 51 and 'fastest_frames_to_remove_percent' not in kw:
                    rec['arrays']['values'] = frame.to_numpy(dtype=np.float64)
                if 'fastest_frames_to_remove_percent' not in kw:
                    rec['arrays']['sum_speeds'] = measure_numpy.pandas_sum_speeds(Q_coords, markers)
            elif func == 'compute_height':
                rec['arrays']['ret'] = np.float64(common.compute_height(Q_coords, markers, **kw))
            elif func == 'compute_leg_length':
                rec['arrays']['ret'] = np.float64(common.compute_leg_length(path, **kw))
            elif func == 'mean_angles':
                rec['arrays']['ret'] = np.array(common.mean_angles(Q_coords), dtype=np.float64)
            elif func == 'segment_lengths':
                p = kw.get('trimmed_extrema_percent', 0.5)
                lengths = np.array([common.euclidean_distance(Q_coords.iloc[:, markers.index(a) * 3:markers.index(a) * 3 + 3],
                                                              Q_coords.iloc[:, markers.index(b) * 3:markers.index(b) * 3 + 3]) for a, b in kw['pairs']])
                rec['arrays']['ret'] = np.array([common.trimmed_mean(arr, trimmed_extrema_percent=p) for arr in lengths])
    except Exception as e:                                    # noqa: BLE001  the type is what is recorded
        rec['exc'] = type(e).__name__
    finally:
        common.mean_angles, common.trimmed_mean = real_angles, real_trim
        root.removeHandler(cap)
        root.setLevel(old_level)
    rec['logs'] = cap.records
    if seen['ang_mean']:
        rec['ang_mean'] = seen['ang_mean'][0]                 # for the margins; kept with the frame cases only
        if func == 'best_coords_for_measurements':
            rec['arrays']['ang_mean'] = rec['ang_mean']
    if seen['heights'] and func == 'compute_height':
        rec['arrays']['rows'] = seen['heights'][0]
    return rec


def margins_hold(case, rec):
    ang = rec.pop('ang_mean', None)
    if ang is None:
        return True
    limit = case['kwargs'].get('large_hip_knee_angles', 45)
    ok = ang[~np.isnan(ang)]
    if len(ok) and np.abs(ok - limit).min() <= MARGIN:
        return False
    if (ok < limit).sum() < 50 and len(ok) > 1:
        first = np.sort(ok)[:51]
        if np.diff(first).min() <= MARGIN:
            return False
    return True


def record():
    common = ref_shim.load()[0]
    cases = case_list()
    out, trial_text, meta = {}, {}, []
    with tempfile.TemporaryDirectory() as tmp:
        for name, (kind, n, unit, markers, opts) in TRIALS.items():
            mine = [c for c in cases if c['trial'] == name]
            for attempt in range(20):
                text = make_trial(kind, n, unit, markers, seed=1000 * attempt + sum(map(ord, name)), **opts)
                path = os.path.join(tmp, f'{name}.trc')
                with open(path, 'w') as fh:
                    fh.write(text)
                recs = [run_case(common, c, text, path) for c in mine]
                if all(margins_hold(c, r) for c, r in zip(mine, recs)):
                    break
            else:
                raise SystemExit(f'{name}: no seed keeps the margins')
            trial_text[name] = text
            for c, r in zip(mine, recs):
                c['rec'] = r
    for i, c in enumerate(cases):
        r = c.pop('rec')
        for key, arr in r.pop('arrays').items():
            out[f'c{i}_{key}'] = arr
        meta.append({**c, **r})
    for name, text in trial_text.items():
        out['trial_' + name] = np.frombuffer(text.encode(), dtype=np.uint8)
    rng = np.random.default_rng(5)
    tm = []
    for n in (1, 2, 3, 7, 50, 51, 1000):
        x = np.round(rng.normal(1.7, 0.05, n), 3)
        for p in (0, 0.1, 0.5, 1.0):
            tm.append({'n': n, 'p': p})
            out[f't{len(tm) - 1}_x'] = x
            out[f't{len(tm) - 1}_ret'] = np.float64(common.trimmed_mean(x, trimmed_extrema_percent=p))
    out['meta'] = np.frombuffer(json.dumps({'cases': meta, 'trimmed': tm}).encode(), dtype=np.uint8)
    target = os.path.join(HERE, 'measure_units.npz')
    np.savez_compressed(target, **out)
    kinds = {}
    for m in meta:
        kinds[m['exc'] or 'ok'] = kinds.get(m['exc'] or 'ok', 0) + 1
    print(f'{target}: {os.path.getsize(target)} bytes, {len(meta)} cases {kinds}, {len(tm)} trimmed means')


def time_reference(n):
    common = ref_shim.load()[0]
    text = make_trial('walk', n, 'm', HALPE_26, seed=3)
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, 'long.trc')
        with open(path, 'w') as fh:
            fh.write(text)
        best = None
        for _ in range(3):
            t0 = time.perf_counter()
            Q_coords, _, _, markers, _ = common.read_trc(path)
            t1 = time.perf_counter()
            common.compute_height(Q_coords, markers, close_to_zero_speed=0.2)
            common.compute_leg_length(path, close_to_zero_speed=0.2)
            kept = common.best_coords_for_measurements(Q_coords, markers, close_to_zero_speed=0.2)
            for a, b in SEGMENTS:
                common.trimmed_mean(common.euclidean_distance(kept[a], kept[b]))
            t2 = time.perf_counter()
            best = (t1 - t0, t2 - t1) if best is None or t2 - t1 < best[1] else best
    print(f'{n} frames x {len(HALPE_26)} markers: read_trc {best[0] * 1e3:.1f} ms; compute_height + compute_leg_length (reads the file again) '
          f'+ best_coords + {len(SEGMENTS)} segment lengths {best[1] * 1e3:.1f} ms')


if __name__ == '__main__':
    if len(sys.argv) > 2 and sys.argv[1] == '--time':
        time_reference(int(sys.argv[2]))
    else:
        record()
