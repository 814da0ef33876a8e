#!/usr/bin/env python
# -*- coding: utf-8 -*-
"""Gait events (heel strikes and toe-offs) from a .trc file, on the GPU: the drop-in for the reference's
Utilities/trc_gaitevents.py.

    from pose2sim_amd import trc_gaitevents
    trc_gaitevents.trc_gaitevents_func(trc_path='trial.trc')
    trc_gaitevents.trc_gaitevents_func(trc_path='trial.trc', method='forward_coordinates', gait_direction='-X')
    trc_gaitevents.trc_gaitevents_batch(['trial_P1.trc', 'trial_P2.trc'], method='forward_velocity', gait_direction='Z')
    python -m pose2sim_amd.trc_gaitevents -i trial.trc --method height_coordinates --height_threshold 6

Three methods, as in the reference:
  forward_coordinates  on = peaks of sign * (heel - sacrum), off = peaks of sign * (sacrum - toe) along the gait direction:
                       scipy.signal.find_peaks with a prominence bound (Engine.find_peaks, bit for bit)
  height_coordinates   toe height, zero-phase Butterworth, contact while below height_threshold (cm)
  forward_velocity     forward toe speed, Gaussian smoothing, contact while below forward_velocity_threshold (m/s)
The signals and their peaks / runs are computed by the kernels of csrc/p2s_gait.hip (Engine.gait_contacts); the list
logic over the few dozen events they give (clean_gait_events, alternate_lists) is Python.  Without the library or a GPU
the module raises, like the rest of the package: there is no CPU fallback.

It returns the reference's two tuples, (t_Ron, t_Lon, t_Roff, t_Loff), (frame_Ron, frame_Lon, frame_Roff, frame_Loff),
prints its console report and appends its block to <trc dir>/<output_file>, byte for byte.  `plot` is accepted and
ignored: the figure is not drawn (Engine.gait_contacts returns the filtered signals for whoever wants to draw it).

Quirks of the reference that are kept, not fixed:
  * For the two threshold methods the frame indices count from the SECOND sample (the [1:] series is re-indexed from 0),
    while the times are looked up as time_col[frame]: a reported time is one sample early for its frame.
  * The events are cleaned twice, once as frames and once as times, and nothing ties the two results together.
  * Strings from the command line are truthy: `--save_output False` saves, `--plot False` would plot.
  * An unknown unit gives a prominence bound (forward_coordinates) or a unit factor (the other two) of inf: no peak is
    kept, or the signal is inf / NaN, and the cleaning then raises IndexError.
  * height_coordinates reads the axis of up_direction and ignores its sign; forward_velocity builds Butterworth
    coefficients it does not use, so a cut_off_frequency at or above Nyquist raises there too.
  * forward_velocity multiplies the coordinates AND the threshold by 100 for cm and by 1000 for mm (height_coordinates
    converts to cm correctly): on real data in cm or mm the noise alone stays above the threshold and no event is found.
  * The output block says "Forward velovity threshold".
  * A marker that is not in the file raises ValueError with forward_coordinates (list.index) and KeyError with the
    other two (a column lookup).
  * alternate_lists with strategy 'last' on a first value below 0 raises UnboundLocalError.
Inputs on which the reference raises raise the same exception type here, before anything is written for that file: no
event on a side (IndexError), a column too short for filtfilt's padding (ValueError), cut_off_frequency * dt * 2 >= 1
(ValueError), a marker that is not in the file.
"""
import argparse
import os

import numpy as np

from . import trc as _trc

METHODS = ('forward_coordinates', 'height_coordinates', 'forward_velocity')
DEFAULTS = (('method', 'height_coordinates'), ('gait_direction', '+X'), ('up_direction', '+Y'),
            ('forward_velocity_threshold', 1), ('height_threshold', 6), ('motion_type', 'gait'), ('sacrum_marker', 'Hip'),
            ('right_heel_marker', 'RHeel'), ('right_toe_marker', 'RBigToe'), ('left_heel_marker', 'LHeel'),
            ('left_toe_marker', 'LBigToe'), ('cut_off_frequency', 10), ('plot', True), ('save_output', True),
            ('output_file', 'gaitevents.txt'))
GAUSS_SIGMA = 5                                       # gaussian_filter1d(speed, 5)


def main():
    p = argparse.ArgumentParser(description='Gait on and off events from a .trc file with the "forward_coordinates", '
                                            '"height_coordinates" or "forward_velocity" method, computed on the GPU.')
    p.add_argument('-i', '--trc_path', required=True, help='input .trc file')
    p.add_argument('-g', '--gait_direction', default='X', required=False, help='"X", "Y", "Z", "-X", "-Y" or "-Z" (write -g=-X). Default "X"')
    p.add_argument('-u', '--up_direction', default='Y', required=False, help='"X", "Y", "Z", "-X", "-Y" or "-Z". Default "Y"')
    p.add_argument('-m', '--method', default='height_coordinates', required=False, help='one of ' + ', '.join(METHODS) + '. Default height_coordinates')
    p.add_argument('-V', '--forward_velocity_threshold', default=1, type=float, required=False, help='forward speed below which the foot is on the ground, m/s (forward_velocity). Default 1')
    p.add_argument('-H', '--height_threshold', default=6, type=float, required=False, help='height below which the foot is on the ground, cm (height_coordinates). Default 6')
    p.add_argument('-t', '--motion_type', default='gait', required=False, help='"gait" (right and left alternate), "sprint" (with a flight phase in between) or "" (no constraint). Default "gait"')
    p.add_argument('--sacrum_marker', default='Hip', required=False, help='Default "Hip"')
    p.add_argument('--right_heel_marker', default='RHeel', required=False, help='Default "RHeel"')
    p.add_argument('--right_toe_marker', default='RBigToe', required=False, help='Default "RBigToe"')
    p.add_argument('--left_heel_marker', default='LHeel', required=False, help='Default "LHeel"')
    p.add_argument('--left_toe_marker', default='LBigToe', required=False, help='Default "LBigToe"')
    p.add_argument('-f', '--cut_off_frequency', default=10, type=float, required=False, help='Butterworth cut-off frequency, Hz. Default 10')
    p.add_argument('-p', '--plot', default=True, required=False, help='accepted and ignored: the figure is not drawn')
    p.add_argument('-s', '--save_output', default=True, required=False, help='append the events to the output file (any string is truthy). Default True')
    p.add_argument('-o', '--output_file', default='gaitevents.txt', required=False, help='Default "gaitevents.txt"')
    trc_gaitevents_func(**vars(p.parse_args()))


# ---- list logic (Python, as in the reference) --------------------------------------------------------------------------
def first_step_side(Ron, Lon):
    return 'R' if Ron[0] < Lon[0] else 'L'


def alternate_lists(*lists, strategy='last'):
    """Make the values of several sorted lists take turns: list 0, list 1, ..., list 0, ...  Walking all values in
    ascending order (ties in list order) from the first value of list 0, a value is taken when it belongs to the list whose
    turn it is and is not below the value before it; with strategy 'last' a later value of the list that was served last
    replaces the one taken ('first' keeps the first)."""
    merged = [(k, v) for k, lst in enumerate(lists) for v in lst]
    merged.sort(key=lambda kv: kv[1])
    start = next((i for i, kv in enumerate(merged) if kv[0] == 0), len(merged))
    out = [[] for _ in lists]
    turn, before, served = 0, 0, None
    for k, v in merged[start:]:
        if k == turn and v >= before:
            out[k].append(v)
            served = turn
            turn += 1
        if strategy == 'last':
            if served is None:                            # the reference reads a name it has not bound yet
                raise UnboundLocalError("cannot access local variable 'last_index' where it is not associated with a value")
            if k == served and v > before:
                out[served][-1] = v
        before = v
        if turn >= len(lists):
            turn = 0
    return out


def clean_gait_events(gait_events, motion_type='gait'):
    """Right and left alternate ('gait': first strike, last take-off), or on / off / on / off of the two sides alternate
    ('sprint'); then an off before the first on and an on after the last off are dropped, per side."""
    Ron, Lon, Roff, Loff = gait_events
    if motion_type == 'gait':
        if first_step_side(Ron, Lon) == 'R':
            Ron, Lon = alternate_lists(Ron, Lon, strategy='first')
            Roff, Loff = alternate_lists(Roff, Loff, strategy='last')
        else:
            Lon, Ron = alternate_lists(Lon, Ron, strategy='first')
            Loff, Roff = alternate_lists(Loff, Roff, strategy='last')
    if motion_type == 'sprint':
        if first_step_side(Ron, Lon) == 'R':
            Ron, Roff, Lon, Loff = alternate_lists(Ron, Roff, Lon, Loff, strategy='last')
        else:
            Lon, Loff, Ron, Roff = alternate_lists(Lon, Loff, Ron, Roff, strategy='last')
    if Ron[0] > Roff[0]:
        Roff.pop(0)
    if Lon[0] > Loff[0]:
        Loff.pop(0)
    if Ron[-1] > Roff[-1]:
        Ron.pop(-1)
    if Lon[-1] > Loff[-1]:
        Lon.pop(-1)
    return Ron, Lon, Roff, Loff


def start_end_true_seq(on, off, first_low):
    """The reference's start_end_true_seq and the `if 0 in on: on.remove(0)` of its callers, from what Engine.gait_contacts
    returns: the reference indexes its list of run ends, which is empty when the whole signal is below the threshold."""
    if first_low and len(off) == 0:
        raise IndexError('list index out of range')
    return [int(i) for i in on], [int(i) for i in off]


# ---- arguments -----------------------------------------------------------------------------------------------------------
def _direction(d):
    if len(d) == 1:
        return +1, d
    if len(d) == 2:
        return int(d[0] + '1'), d[1]
    return d


def resolve_args(args):
    """The reference's argument handling: defaults for what is None, (sign, axis) directions, the method check."""
    cfg = {'trc_path': args.get('trc_path')}
    for key, default in DEFAULTS:
        value = args.get(key)
        cfg[key] = default if value is None else value
    cfg['gait_direction'] = _direction(cfg['gait_direction'])
    cfg['up_direction'] = _direction(cfg['up_direction'])
    if cfg['method'] not in METHODS:
        raise ValueError('Method must be "forward_coordinates", "height_coordinates", or "forward_velocity"')
    return cfg


def _head_lines(cfg):
    m = cfg['method']
    if m == 'forward_coordinates':
        first = 'Method: forward_coordinates'
    elif m == 'height_coordinates':
        first = f'Method: height_coordinates. Height threshold: {cfg["height_threshold"]} cm'
    else:
        first = f'Method: forward_velocity. Forward velocity threshold: {cfg["forward_velocity_threshold"]} m/s'
    return [first, f'Motion type: {cfg["motion_type"]}']


# ---- one file: what the host does before and after the device call ------------------------------------------------------
def _prepare(cfg, trc_path):
    """Read the file and lay out the columns the device call needs -> dict; raises what the reference raises there."""
    from scipy import signal
    method = cfg['method']
    sign, direction = cfg['up_direction'] if method == 'height_coordinates' else cfg['gait_direction']
    axis = ['X', 'Y', 'Z'].index(direction)
    Q_coords, _, time_col, trc_markers, header = _trc.read_trc(trc_path)
    unit = header[2].split('\t')[4]
    coords = Q_coords.to_numpy()
    prep = {'time_col': time_col, 'method': method, 'sign': sign}
    if method == 'forward_coordinates':
        prep['bound'] = .1 if unit == 'm' else 1 if unit == 'dm' else 10 if unit == 'cm' else 100 if unit == 'mm' else np.inf
        markers = [cfg[k] for k in ('right_heel_marker', 'right_toe_marker', 'left_heel_marker', 'left_toe_marker', 'sacrum_marker')]
        rheel, rtoe, lheel, ltoe, hip = (coords[:, axis + trc_markers.index(m) * 3] for m in markers)
        # Ron, Lon, Roff, Loff
        prep['columns'] = [sign * (rheel - hip), sign * (lheel - hip), sign * (hip - rtoe), sign * (hip - ltoe)]
        return prep
    markers = [cfg['right_toe_marker'], cfg['left_toe_marker']]
    by_name = {m: i for i, m in reversed(list(enumerate(trc_markers)))}

    def column(m):
        if m not in by_name:
            raise KeyError(m)
        return coords[:, axis + by_name[m] * 3]
    if method == 'height_coordinates':
        prep['factor'] = 100 if unit == 'm' else 10 if unit == 'dm' else 1 if unit == 'cm' else .1 if unit == 'mm' else np.inf
        prep['threshold'] = cfg['height_threshold']
        prep['columns'] = [column(m) for m in markers]
        prep['dt'] = time_col.diff().mean()
        b, a = signal.butter(4 / 2, cfg['cut_off_frequency'] * prep['dt'] * 2, 'low', analog=False)
        prep['filter'] = (b, a, signal.lfilter_zi(b, a))
        padlen = 3 * max(len(a), len(b))
        if len(time_col) - 1 <= padlen:                   # scipy.signal.filtfilt's refusal
            raise ValueError(f'The length of the input vector x must be greater than padlen, which is {padlen}.')
    else:
        prep['factor'] = 1 if unit == 'm' else 10 if unit == 'dm' else 100 if unit == 'cm' else 1000 if unit == 'mm' else np.inf
        prep['threshold'] = cfg['forward_velocity_threshold'] * prep['factor']
        prep['dt'] = time_col.diff().mean()
        signal.butter(4 / 2, cfg['cut_off_frequency'] * prep['dt'] * 2, 'low', analog=False)   # unused there too; it can raise
        prep['columns'] = [column(m) for m in markers]
    return prep


def gaussian_weights(sigma=GAUSS_SIGMA):
    """The weights scipy.ndimage.gaussian_filter1d(., sigma) correlates with (truncate 4), from scipy's own function."""
    from scipy.ndimage import _filters
    radius = int(4.0 * float(sigma) + 0.5)
    return np.asarray(_filters._gaussian_kernel1d(float(sigma), 0, radius)[::-1], dtype=np.float64)


def _detect(engine, preps):
    """One device call for all prepared files -> per file the raw event lists (frame_Ron, frame_Lon, frame_Roff,
    frame_Loff) or the exception start_end_true_seq raises on it."""
    if not preps:
        return []
    method = preps[0]['method']
    if method == 'forward_coordinates':
        rows = max(len(c) for p in preps for c in p['columns'])
        table = np.full((rows, 4 * len(preps)), np.nan)       # a NaN tail ends every scan where the column ends
        for i, p in enumerate(preps):
            for j, c in enumerate(p['columns']):
                table[:len(c), 4 * i + j] = c
        found = engine.find_peaks(table, prominence=np.repeat([float(p['bound']) for p in preps], 4))
        return [tuple(found[4 * i + j][0].tolist() for j in range(4)) for i in range(len(preps))]
    columns = [c for p in preps for c in p['columns']]
    rep = lambda key: np.repeat([float(p[key]) for p in preps], 2)    # noqa: E731
    if method == 'height_coordinates':
        # the coefficients depend on the file's dt: files that share them share a call
        out = [None] * len(preps)
        groups = {}
        for i, p in enumerate(preps):
            groups.setdefault(np.concatenate(p['filter']).tobytes(), []).append(i)
        for idx in groups.values():
            b, a, zi = preps[idx[0]]['filter']
            sel = [preps[i] for i in idx]
            _, on, off, first = engine.gait_contacts([c for p in sel for c in p['columns']], method, dt=np.repeat([float(p['dt']) for p in sel], 2),
                                                     threshold=np.repeat([float(p['threshold']) for p in sel], 2),
                                                     factor=np.repeat([float(p['factor']) for p in sel], 2), b=b, a=a, zi=zi)
            for k, i in enumerate(idx):
                out[i] = (on[2 * k:2 * k + 2], off[2 * k:2 * k + 2], first[2 * k:2 * k + 2])
    else:
        _, on, off, first = engine.gait_contacts(columns, method, dt=rep('dt'), threshold=rep('threshold'), factor=rep('factor'),
                                                 sign=preps[0]['sign'], weights=gaussian_weights())
        out = [(on[2 * i:2 * i + 2], off[2 * i:2 * i + 2], first[2 * i:2 * i + 2]) for i in range(len(preps))]
    raw = []
    for on, off, first in out:
        try:
            Ron, Roff = start_end_true_seq(on[0], off[0], first[0])
            Lon, Loff = start_end_true_seq(on[1], off[1], first[1])
            raw.append((Ron, Lon, Roff, Loff))
        except IndexError as e:
            raw.append(e)
    return raw


def events_from_frames(cfg, trc_path, time_col, raw_frames):
    """From the detected frames on: times, the two cleanings, the console report, the appended block, the result."""
    frame_Ron, frame_Lon, frame_Roff, frame_Loff = (list(f) for f in raw_frames)
    t_Ron, t_Lon, t_Roff, t_Loff = (time_col[f].tolist() for f in (frame_Ron, frame_Lon, frame_Roff, frame_Loff))
    motion_type = cfg['motion_type']
    frame_Ron, frame_Lon, frame_Roff, frame_Loff = clean_gait_events((frame_Ron, frame_Lon, frame_Roff, frame_Loff), motion_type=motion_type)
    t_Ron, t_Lon, t_Roff, t_Loff = clean_gait_events((t_Ron, t_Lon, t_Roff, t_Loff), motion_type=motion_type)
    print('Times:')
    print('Right on:', t_Ron)
    print('Right off:', t_Roff)
    print('Left on:', t_Lon)
    print('Left off:', t_Loff)
    print('\nFrames:')
    print('Right on:', frame_Ron)
    print('Right off:', frame_Roff)
    print('Left on:', frame_Lon)
    print('Left off:', frame_Loff)
    if cfg['save_output'] or cfg['save_output'] is None:
        method = cfg['method']
        L = os.path.basename(trc_path) + '\n'
        L += f'Method: {method}. '
        L += (f'Height threshold: {cfg["height_threshold"]}\n' if method == 'height_coordinates'
              else f'Forward velovity threshold: {cfg["forward_velocity_threshold"]}\n' if method == 'forward_velocity' else '\n')
        L += f'Motion type: {motion_type}\n'
        L += 'Times:\n'
        for label, values in (('Right on', t_Ron), ('Left on', t_Lon), ('Right off', t_Roff), ('Left off', t_Loff)):
            L += f'\t{label}: {values}\n'
        L += 'Frames:\n'
        for label, values in (('Right on', frame_Ron), ('Left on', frame_Lon), ('Right off', frame_Roff), ('Left off', frame_Loff)):
            L += f'\t{label}: {values}\n'
        L += '\n'
        with open(os.path.join(os.path.dirname(trc_path), cfg['output_file']), 'a') as fh:
            fh.write(L)
    return (t_Ron, t_Lon, t_Roff, t_Loff), (frame_Ron, frame_Lon, frame_Roff, frame_Loff)


def _make_engine():
    from .engine import Engine
    return Engine(0)


def trc_gaitevents_batch(trc_paths, **args):
    """trc_gaitevents_func on every file of trc_paths with the same arguments: the files' columns go to the device in one
    call (forward_coordinates, forward_velocity; height_coordinates: one call per distinct frame interval, since the
    filter coefficients depend on it), and the reports are printed and appended in order.  -> the list of per-file
    results.  A file on which the reference raises does so after the files before it have been reported; the files after
    it are not."""
    engine = args.pop('engine', None)
    args.pop('trc_path', None)
    cfg = resolve_args(args)
    trc_paths = list(trc_paths)
    preps = []
    for path in trc_paths:
        try:
            preps.append(_prepare(cfg, path))
        except Exception as e:                            # raised when the file's turn comes
            preps.append(e)
            break
    good = [p for p in preps if not isinstance(p, Exception)]
    if good:
        engine = engine or _make_engine()
    raw = iter(_detect(engine, good))
    results = []
    for path, prep in zip(trc_paths, preps):
        for line in _head_lines(cfg):
            print(line)
        if isinstance(prep, Exception):
            raise prep
        frames = next(raw)
        if isinstance(frames, Exception):
            raise frames
        results.append(events_from_frames(cfg, path, prep['time_col'], frames))
    return results


def trc_gaitevents_func(**args):
    """Gait events of one .trc file; arguments, defaults, console report, appended block and the returned
    (t_Ron, t_Lon, t_Roff, t_Loff), (frame_Ron, frame_Lon, frame_Roff, frame_Loff) are the reference's (see the module's
    docstring for the methods and the quirks that are kept)."""
    args = dict(args)
    return trc_gaitevents_batch([args.get('trc_path')], **args)[0]


if __name__ == '__main__':
    main()
