"""Record tests/golden/gait_units.npz from the reference's own Utilities/trc_gaitevents.py (through ref_shim, plot=False)
and from scipy.signal.find_peaks.  Build container only: the reference does not exist anywhere else.

    python tests/golden/make_golden_gait.py
    taskset -c 0 python tests/golden/make_golden_gait.py --time 36000    # the reference's time on one file, one core

What is recorded
  trials   synthetic walking / running / standing .trc files written here (their text, as bytes)
  cases    per case: the trial, the arguments, and from trc_gaitevents_func the returned tuples, the console text, the
           text appended to the output file, the exception type when it raises, and the event frames as they were before
           clean_gait_events (the first call of it is intercepted), for the host test of the list logic
  fp_*     tables with scipy.signal.find_peaks(x, prominence=p) per column for p in None, 0, a mid value, inf

The kernels agree with scipy to a tolerance on the filtered signals while events are discrete, so every case that does
not raise must keep its filtered samples away from its threshold by 1e-6 * max(1, |threshold|), and its prominences away
from the bound by 1e-6: conditions on the INPUTS, asserted here on what the reference computed (its filtfilt /
gaussian_filter1d / find_peaks calls are intercepted); a trial that fails is generated again with another seed.
"""
import contextlib
import importlib
import io
import json
import os
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import ref_shim  # noqa: E402

MARKERS = ['Hip', 'RHeel', 'RBigToe', 'LHeel', 'LBigToe', 'Neck']
UNIT_PER_M = {'m': 1.0, 'dm': 10.0, 'cm': 100.0, 'mm': 1000.0, 'in': 39.37}
MARGIN = 1e-6


def _axis(d):
    d = d if len(d) == 2 else '+' + d
    return (1.0 if d[0] == '+' else -1.0), 'XYZ'.index(d[1])


def make_trial(kind, n, fps, unit, fwd, up, seed, noise=0.002, wobble=0.0):
    """-> the text of a .trc: a person moving along `fwd` with `up` as the vertical, metres scaled to `unit`."""
    rng = np.random.default_rng(seed)
    t = np.arange(n) / fps
    speed, period, stance = {'walk': (1.3, 1.1, 0.62), 'run': (3.4, 0.7, 0.36), 'stand': (0.0, 1.0, 1.0)}[kind]
    reach = speed * period * stance / 2                       # the foot travels 2 * reach under the hip during stance
    pos = {}
    hip_f = 0.3 + speed * t
    pos['Hip'] = (hip_f, np.full(n, 0.95) + 0.02 * np.sin(4 * np.pi * t / period), np.zeros(n))
    pos['Neck'] = (hip_f + 0.02, np.full(n, 1.45), np.zeros(n))
    for side, phase0, lat in (('R', 0.0, 0.1), ('L', 0.5, -0.1)):
        ph = (t / period + phase0) % 1.0
        in_stance = ph < stance
        swing = np.clip((ph - stance) / max(1.0 - stance, 1e-9), 0.0, 1.0)
        rel = np.where(in_stance, reach * (1 - 2 * ph / stance), -reach * np.cos(np.pi * swing))
        lift = np.where(in_stance, 0.0, np.sin(np.pi * swing) ** 2)
        if wobble:                                            # a stumble: extra dips of the swinging foot and jitter
            lift = lift * (1 - wobble * np.sin(6 * np.pi * swing) ** 2)
            rel = rel + 0.4 * wobble * reach * np.sin(2 * np.pi * 3.1 * t + phase0)
        foot_f = hip_f + rel
        pos[side + 'Heel'] = (foot_f - 0.05, 0.04 + 0.16 * lift, np.full(n, lat))
        pos[side + 'BigToe'] = (foot_f + 0.17, 0.025 + 0.12 * lift, np.full(n, lat))
    (sf, af), (su, au) = _axis(fwd), _axis(up)
    al = 3 - af - au
    scale = UNIT_PER_M[unit]
    table = np.zeros((n, 3 * len(MARKERS)))
    for k, m in enumerate(MARKERS):
        f, u, lateral = pos[m]
        table[:, 3 * k + af] = sf * f
        table[:, 3 * k + au] = su * u
        table[:, 3 * k + al] = lateral
    table = (table + rng.normal(0, noise, table.shape)) * scale
    lines = ['PathFileType\t4\t(X/Y/Z)\ttrial.trc\n',
             'DataRate\tCameraRate\tNumFrames\tNumMarkers\tUnits\tOrigDataRate\tOrigDataStartFrame\tOrigNumFrames\n',
             f'{fps}\t{fps}\t{n}\t{len(MARKERS)}\t{unit}\t{fps}\t0\t{n}\n',
             'Frame#\tTime\t' + '\t\t\t'.join(MARKERS) + '\t\t\n',
             '\t\t' + '\t'.join(f'{a}{k + 1}' for k in range(len(MARKERS)) for a in 'XYZ') + '\n']
    for i in range(n):
        lines.append(f'{i + 1}\t{t[i]:.4f}\t' + '\t'.join(f'{v:.6f}' for v in table[i]) + '\n')
    return ''.join(lines)


# name: (kind, frames, fps, unit, forward, up, noise, wobble)
TRIALS = {
    'walk_m': ('walk', 300, 60, 'm', 'X', 'Y', 0.002, 0.0),
    'walk_cm': ('walk', 280, 60, 'cm', '-Z', 'Y', 0.002, 0.0),
    'walk_mm': ('walk', 320, 50, 'mm', 'Y', 'Z', 0.002, 0.0),
    'walk_dm': ('walk', 260, 60, 'dm', '-X', 'Z', 0.002, 0.0),
    'walk_down': ('walk', 300, 60, 'm', '-X', '-Y', 0.002, 0.0),
    'run_m': ('run', 300, 100, 'm', 'Z', 'X', 0.002, 0.0),
    'run_cm': ('run', 260, 100, 'cm', '-Y', '-Z', 0.002, 0.0),
    'run_mm': ('run', 280, 120, 'mm', 'Z', '-X', 0.002, 0.0),
    'walk_noisy': ('walk', 400, 60, 'm', 'X', 'Y', 0.012, 0.9),
    'run_noisy': ('run', 360, 100, 'cm', '-X', 'Y', 0.010, 0.8),
    'walk_inch': ('walk', 300, 60, 'in', 'X', 'Y', 0.002, 0.0),
    'stand': ('stand', 200, 60, 'm', 'X', 'Y', 0.0005, 0.0),
    'short': ('walk', 10, 60, 'm', 'X', 'Y', 0.002, 0.0),
    'eleven': ('walk', 11, 60, 'm', 'X', 'Y', 0.002, 0.0),
}
METHODS = ('forward_coordinates', 'height_coordinates', 'forward_velocity')
MOTIONS = ('gait', 'sprint', '')


def case_list():
    cases = []

    def add(trial, method, motion, **extra):
        _, _, _, _, fwd, up, _, _ = TRIALS[trial]
        args = {'method': method, 'motion_type': motion, 'gait_direction': fwd, 'up_direction': up}
        args.update(extra)
        cases.append({'name': f'{trial}-{method}-{motion or "none"}' + ''.join(f'-{k}={v}' for k, v in sorted(extra.items())),
                      'trial': trial, 'args': args})
    for trial in ('walk_m', 'run_m', 'walk_noisy', 'run_noisy'):          # every method x motion type
        for method in METHODS:
            for motion in MOTIONS:
                add(trial, method, motion)
    k = 0
    for trial in ('walk_cm', 'walk_mm', 'walk_dm', 'walk_down', 'run_cm', 'run_mm', 'walk_inch', 'stand', 'short', 'eleven'):
        for method in METHODS:
            add(trial, method, MOTIONS[k % 3])
            k += 1
    add('walk_m', 'height_coordinates', 'gait', height_threshold=9.5)
    add('run_m', 'forward_velocity', 'sprint', forward_velocity_threshold=2.25)
    add('walk_m', 'height_coordinates', 'gait', cut_off_frequency=40)       # 40 * dt * 2 >= 1
    add('walk_m', 'forward_velocity', 'gait', cut_off_frequency=40)      # its unused butter call raises too
    add('walk_m', 'forward_coordinates', 'gait', sacrum_marker='Pelvis')    # not in the file
    add('walk_m', 'height_coordinates', 'gait', left_toe_marker='LToe')
    add('walk_m', 'forward_velocity', 'gait', right_toe_marker='RToe')
    add('walk_m', 'forward_coordinates', 'gait', save_output='False')       # a string from the command line: truthy
    cases.append({'name': 'walk_m-defaults', 'trial': 'walk_m', 'args': {}})  # called as a function with the path alone
    return cases


class Recorder:
    """Stands where the reference module has `signal` and `gaussian_filter1d`: the same scipy calls, their results kept."""

    def __init__(self, scipy_signal, gaussian):
        self._signal, self._gaussian = scipy_signal, gaussian
        self.reset()

    def reset(self):
        self.filtered, self.prominences, self.raw_frames = [], [], None

    def butter(self, *a, **k):
        return self._signal.butter(*a, **k)

    def filtfilt(self, *a, **k):
        out = self._signal.filtfilt(*a, **k)
        self.filtered.append(np.array(out))
        return out

    def gaussian_filter1d(self, *a, **k):
        out = self._gaussian(*a, **k)
        self.filtered.append(np.array(out))
        return out

    def find_peaks(self, x, prominence=None):
        peaks = self._signal.find_peaks(x)[0]
        self.prominences.append(self._signal.peak_prominences(x, peaks)[0])
        return self._signal.find_peaks(x, prominence=prominence)


def run_case(ref, rec, case, trc_text, folder):
    """-> the record of one case; raises AssertionError when the trial lies too close to a threshold."""
    path = os.path.join(folder, case['trial'] + '.trc')
    with open(path, 'w') as fh:
        fh.write(trc_text)
    out_file = os.path.join(folder, case['args'].get('output_file', 'gaitevents.txt'))
    if os.path.exists(out_file):
        os.remove(out_file)
    rec.reset()
    clean = ref.clean_gait_events

    def spy(gait_events, motion_type='gait'):
        if rec.raw_frames is None:
            rec.raw_frames = [list(v) for v in gait_events]
        return clean(gait_events, motion_type=motion_type)
    ref.clean_gait_events = spy
    buf = io.StringIO()
    record = {'name': case['name'], 'trial': case['trial'], 'args': case['args'], 'error': '', 'result': None}
    try:
        with contextlib.redirect_stdout(buf):
            res = ref.trc_gaitevents_func(trc_path=path, plot=False, **case['args'])
        record['result'] = [[list(v) for v in res[0]], [list(v) for v in res[1]]]
    except Exception as e:                                    # recorded: the mirror must raise the same type
        record['error'] = type(e).__name__
    finally:
        ref.clean_gait_events = clean
    record['console'] = buf.getvalue()
    record['file'] = open(out_file).read() if os.path.exists(out_file) else ''
    record['raw_frames'] = None if rec.raw_frames is None else [[int(i) for i in v] for v in rec.raw_frames]
    if not record['error']:
        args = case['args']
        method = args.get('method', 'height_coordinates')
        unit = TRIALS[case['trial']][3]
        if method == 'forward_coordinates':
            bound = {'m': .1, 'dm': 1, 'cm': 10, 'mm': 100}.get(unit, np.inf)
            for prom in rec.prominences:
                assert not np.any(np.abs(prom - bound) <= MARGIN), (case['name'], 'a prominence too close to the bound')
        else:
            if method == 'height_coordinates':
                thr = args.get('height_threshold', 6)
            else:
                thr = args.get('forward_velocity_threshold', 1) * {'m': 1, 'dm': 10, 'cm': 100, 'mm': 1000}.get(unit, np.inf)
            assert len(rec.filtered) == 2, case['name']
            for sig in rec.filtered:
                assert not np.any(np.abs(sig - thr) <= MARGIN * max(1.0, abs(thr))), (case['name'], 'a sample too close to the threshold')
    return record


def find_peaks_tables():
    rng = np.random.default_rng(2025)
    nan, inf = np.nan, np.inf
    t = {}
    t['len1'] = np.array([[1.0, nan, inf]])
    t['len2'] = np.array([[1.0, 2.0, nan], [2.0, 1.0, 3.0]])
    t['len3'] = np.array([[1.0, 1.0, 3.0, nan, 0.0, 0.0, -inf], [3.0, 1.0, 2.0, 1.0, inf, nan, 0.0], [2.0, 1.0, 1.0, 0.0, 0.0, 0.0, -inf]])
    t['equal'] = np.full((50, 2), 3.25)
    plateaus = [[0, 1, 1, 0, 0, 2, 2, 2, 0, 1, 0, 0],           # even and odd plateaus in the middle
                [4, 4, 4, 1, 2, 2, 2, 2, 1, 3, 3, 3],           # plateaus touching either end are no peaks
                [0, 5, 5, 5, 5, 5, 5, 5, 5, 5, 5, 0],           # one plateau of even length end to end
                [0, 5, 5, 5, 5, 5, 5, 5, 5, 5, 0, 0],           # and of odd length
                [1, 2, 2, 3, 3, 2, 2, 1, 1, 4, 4, 0],           # steps up and down
                [0, 1, 0, 1, 0, 1, 0, 2, 0, 1, 0, 0]]           # equal peaks: bases nearest to the peak
    t['plateaus'] = np.array(plateaus, dtype=np.float64).T
    nans = [[0, 1, nan, 0, 2, 0, nan, 3, 0, 1, 0, 0],           # a NaN next to a maximum on either side
            [0, 2, 2, nan, 2, 2, 0, 1, 0, 0, 0, 0],             # a NaN inside a would-be plateau
            [nan, 1, 0, 3, 1, 2, nan, 2, 1, 5, 0, nan],         # NaN at the ends; a NaN ends the scan for the bases
            [0, 3, 1, 2, 1, 4, 1, nan, 1, 2, 1, 0],
            [nan] * 12]
    t['nans'] = np.array(nans, dtype=np.float64).T
    infs = [[0, inf, 0, 1, 0, inf, inf, 0, -inf, 1, -inf, 0],
            [-inf, 0, -inf, -inf, 1, -inf, 2, 1, 3, -inf, 0, -inf],
            [inf, 0, 1, 0, inf, 0, 2, 0, inf, 1, 0, inf],
            [-inf, -inf, -inf, 0, -inf, -inf, inf, -inf, 1, 2, 1, -inf]]
    t['infs'] = np.array(infs, dtype=np.float64).T
    for n in (257, 513):
        i = np.arange(n, dtype=np.float64)
        rise = i + 10.0 * (np.arange(n) % 2)                   # every peak higher than all before it: the left scan runs to the start
        t[f'saw{n}'] = np.stack([rise, rise[::-1], -rise, np.where(np.arange(n) % 2 == 1, 1.0, 0.0)], axis=1)
    walk = np.cumsum(rng.normal(0, 1, (1000, 1)), axis=0)
    t['one_column'] = np.round(walk, 1)
    wide = np.cumsum(rng.normal(0, 1, (700, 65)), axis=0)
    wide[:, ::2] = np.round(wide[:, ::2], 0)                   # plateaus in every other column
    wide[:, 5] = np.round(wide[:, 5] / 4, 0) * 4               # long plateaus: whole blocks of equal samples
    wide[:, 7] = 2.0
    wide[100:612, 7] = 5.0                                     # a plateau over two whole blocks
    wide[:, 9] = np.sin(np.arange(700) / 40.0) * 20            # slow: scans cross several blocks
    for c in (3, 10, 20):
        wide[rng.random(700) < 0.02, c] = nan
    wide[:, 11] = nan
    t['wide'] = wide
    return t


def record_find_peaks(out):
    from scipy import signal
    names = []
    for name, x in find_peaks_tables().items():
        names.append(name)
        out[f'fp_{name}_x'] = x
        all_prom = np.concatenate([signal.peak_prominences(x[:, c], signal.find_peaks(x[:, c])[0])[0] for c in range(x.shape[1])])
        finite = all_prom[np.isfinite(all_prom)]
        mid = float(np.median(finite)) if len(finite) else 1.0
        out[f'fp_{name}_mid'] = np.float64(mid)
        for key, p in (('none', None), ('zero', 0), ('mid', mid), ('inf', np.inf)):
            cols = []
            for c in range(x.shape[1]):
                if p is None:
                    peaks = signal.find_peaks(x[:, c])[0]
                    prom, lb, rb = signal.peak_prominences(x[:, c], peaks)
                else:
                    peaks, props = signal.find_peaks(x[:, c], prominence=p)
                    prom, lb, rb = props['prominences'], props['left_bases'], props['right_bases']
                cols.append((peaks, prom, lb, rb))
            out[f'fp_{name}_{key}_counts'] = np.array([len(c[0]) for c in cols], dtype=np.int64)
            out[f'fp_{name}_{key}_peaks'] = np.concatenate([c[0] for c in cols]).astype(np.int64)
            out[f'fp_{name}_{key}_prom'] = np.concatenate([c[1] for c in cols]).astype(np.float64)
            out[f'fp_{name}_{key}_lb'] = np.concatenate([c[2] for c in cols]).astype(np.int64)
            out[f'fp_{name}_{key}_rb'] = np.concatenate([c[3] for c in cols]).astype(np.int64)
    out['fp_names'] = np.array(names)


def time_reference(ref, frames, repeats=3):
    """Seconds trc_gaitevents_func of the reference takes on one walking trial of `frames` frames, plot=False."""
    import time
    with tempfile.TemporaryDirectory() as folder:
        path = os.path.join(folder, 'trial.trc')
        with open(path, 'w') as fh:
            fh.write(make_trial('walk', frames, 60, 'm', 'X', 'Y', 1, 0.002, 0.0))
        for method in METHODS:
            times = []
            for _ in range(repeats + 1):
                t0 = time.perf_counter()
                with contextlib.redirect_stdout(io.StringIO()):
                    ref.trc_gaitevents_func(trc_path=path, method=method, plot=False)
                times.append(time.perf_counter() - t0)
            print(f'{method}: {frames} frames, after one warm-up run: ' + ', '.join(f'{t:.3f}' for t in times[1:]) + ' s')


def main():
    ref_shim.install()
    ref = importlib.import_module('Pose2Sim.Utilities.trc_gaitevents')
    if len(sys.argv) == 3 and sys.argv[1] == '--time':
        return time_reference(ref, int(sys.argv[2]))
    rec = Recorder(ref.signal, ref.gaussian_filter1d)
    ref.signal, ref.gaussian_filter1d = rec, rec.gaussian_filter1d
    cases = case_list()
    out, records, seeds = {}, {}, {}
    with tempfile.TemporaryDirectory() as folder:
        for trial, (kind, n, fps, unit, fwd, up, noise, wobble) in TRIALS.items():
            mine = [c for c in cases if c['trial'] == trial]
            for seed in range(100, 140):
                text = make_trial(kind, n, fps, unit, fwd, up, seed, noise, wobble)
                try:
                    got = [run_case(ref, rec, c, text, folder) for c in mine]
                except AssertionError as e:
                    print(f'{trial}: seed {seed} refused ({e.args[0][1]}), next seed')
                    continue
                out['trial_' + trial] = np.frombuffer(text.encode(), dtype=np.uint8)
                seeds[trial] = seed
                for r in got:
                    records[r['name']] = r
                break
            else:
                raise SystemExit(f'{trial}: no seed keeps its signals away from the thresholds')
    ordered = [records[c['name']] for c in cases]
    changed = 0
    for r in ordered:                                         # does the cleaning do real work somewhere?
        if not r['error'] and r['raw_frames'] is not None:
            raw, res = r['raw_frames'], r['result'][1]
            changed += sum(len(a) - len(b) for a, b in zip(raw, res)) > 4     # the ends account for 4 at most
    n_err = sum(bool(r['error']) for r in ordered)
    print(f'{len(ordered)} cases, {n_err} raise ({sorted({r["error"] for r in ordered if r["error"]})}); '
          f'the cleaning drops more than the ends in {changed}; seeds {seeds}')
    assert changed >= 3, 'the noisy trials do not make alternate_lists work'
    assert {'IndexError', 'ValueError', 'KeyError'} <= {r['error'] for r in ordered}
    out['cases_json'] = np.array(json.dumps(ordered))
    record_find_peaks(out)
    np.savez_compressed(os.path.join(HERE, 'gait_units.npz'), **out)
    print('wrote gait_units.npz,', os.path.getsize(os.path.join(HERE, 'gait_units.npz')), 'bytes')


if __name__ == '__main__':
    main()
