#!/usr/bin/env python
# -*- coding: utf-8 -*-
"""Body measurements from a filtered .trc, on the GPU: the reference's best_coords_for_measurements, mean_angles,
compute_height, compute_leg_length and trimmed_mean (common.py:427-455, :797-1034) and the .trc half of
kinematics.dict_segment_ratio (:299-304), which is what `participant_height = 'auto'` and the OpenSim scale factors are
made from.

    from pose2sim_amd import measurements, trc
    Q_coords, _, _, markers, _ = trc.read_trc('trial.trc')
    measurements.compute_height(Q_coords, markers, close_to_zero_speed=0.2)
    measurements.compute_leg_length('trial.trc')
    measurements.measure_batch(['trial_P1.trc', 'trial_P2.trc'], pairs=[('RKnee', 'RAnkle')], close_to_zero_speed=0.2)
    python -m pose2sim_amd.measurements -i trial.trc

Signatures, defaults, return values, exception types and `logging` texts are the reference's; DataFrames have its layout
(every marker's name on its three columns, as trc.read_trc returns them).  The numbers come from csrc/p2s_measure.hip
(Engine.body_measure, Engine.trimmed_means): summed speeds, a stable order of the frames by speed and by angle, the mean
knee and hip angles, lengths, heights and trimmed means, for a whole batch of files in one device call.  Without the
library or a GPU the module raises, like the rest of the package: there is no CPU fallback.

Quirks of the reference that are kept, not fixed:
  * best_coords_for_measurements returns the frame WITH the MidShoulder (and Hip) columns it appended: the slice that
    would drop them compares two equal counts and never runs.
  * The returned rows are in ascending-speed order (or ascending-angle order in the 50-smallest branch), and their index
    labels are places among the speed-selected rows, not frame numbers.
  * Fewer than 50 rows below the angle limit means "the 50 smallest angles", also when every row was below it: a file of
    40 good rows comes back reordered by angle.  Series.nsmallest does not drop NaN angles: they come last and fill up
    when fewer than 50 rows have an angle.
  * Row 0 has speed 0, so it is never among the rows kept by speed.
  * A missing heel marker makes BOTH feet 10 cm; a missing ankle is first reported as a missing heel, then raises.
  * euclidean_distance of a pair whose differences are NaN in every kept row is inf, not 0, and so is the height.
  * trimmed_mean with an empty slice (a percentage of 1, or one row) is the plain mean of the unsorted array.
  * mean_angles ignores its ang_to_consider.
What differs: marker names must be unique (ValueError otherwise; pandas' behaviour on duplicate names is not reproduced).
keypoints_names may name a part of the frame's markers, in any order: the speeds then sum over those, as in the reference.
"""
import argparse
import logging

import numpy as np
import pandas as pd

from . import _lib
from . import trc as _trc

HEIGHT_PAIRS = (('RHeel', 'RAnkle'), ('LHeel', 'LAnkle'), ('RAnkle', 'RKnee'), ('LAnkle', 'LKnee'), ('RKnee', 'RHip'),
                ('LKnee', 'LHip'), ('RHip', 'RShoulder'), ('LHip', 'LShoulder'))     # then mid-shoulder to Head or Nose
ANGLE_MARKERS = ('RAnkle', 'RKnee', 'RHip', 'LAnkle', 'LKnee', 'LHip')
_PAD = ' ' * 28                                        # the reference's messages continue their lines with a backslash
MSG_ALL_SLOW = ('All frames have speed close to zero. Make sure the person is moving and correctly detected, or change '
                'close_to_zero_speed to a lower value. Not restricting the speeds to be above any threshold.')
MSG_NO_ANGLES = ('At least one among the RAnkle, RKnee, RHip, RShoulder, LAnkle, LKnee, LHip, LShoulder markers is missing for '
                 'computing the knee and hip angles. Not restricting these angles to be below {}°.')
MSG_ALL_DATA = ('The selected person might not move, or is crouching for the whole sequence, or is not well detected. Taking all '
                'available data instead of filtering them.')
MSG_NO_HEEL = 'The Heel marker is missing from your model. Considering Foot to Heel size as 10 cm.'
MSG_NO_HEAD = 'The Head marker is missing from your model. Considering Neck to Head size as 1.33 times Neck to MidShoulder size.'
MSG_HEIGHT_LOG = ('At least one of the following markers is missing for computing the height of the person:' + _PAD
                  + 'RAnkle, RKnee, RHip, RShoulder, LAnkle, LKnee, LHip, LShoulder.\n' + _PAD
                  + 'Make sure that the person is entirely visible, or use a calibration file instead, or set "to_meters=false".')
MSG_HEIGHT_RAISE = ('At least one of the following markers is missing for computing the height of the person:' + ' ' * 25
                    + 'RAnkle, RKnee, RHip, RShoulder, LAnkle, LKnee, LHip, LShoulder.' + ' ' * 25
                    + 'Make sure that the person is entirely visible, or use a calibration file instead, or set "to_meters=false".')
MSG_LEG_LOG = ('At least one of the following markers is missing for computing the leg length of the person:' + ' ' * 36
               + 'RAnkle, RKnee, RHip, LAnkle, LKnee, LHip.')
MSG_LEG_RAISE = ('At least one of the following markers is missing for computing the leg length of the person:' + ' ' * 33
                 + 'RAnkle, RKnee, RHip, LAnkle, LKnee, LHip.')


def _make_engine():
    from .engine import Engine
    return Engine(0)


def frame_markers(Q_coords):
    """The marker names of a DataFrame in the reference's layout: every name on three neighbouring columns, no name twice."""
    cols = list(Q_coords.columns)
    names = cols[::3]
    if len(cols) % 3 or any(cols[3 * i + j] != n for i, n in enumerate(names) for j in range(3)):
        raise ValueError('Q_coords must have three columns per marker, each named after it')
    if len(set(names)) != len(names):
        raise ValueError('marker names must be unique')
    return names


class _Plan:
    """What one file asks of Engine.body_measure, and what the reference would log or raise around it."""

    def __init__(self, Q_coords, keypoints_names, restrict=True, height=False, leg=False, pairs=None):
        self.Q = Q_coords
        self.error = None                                 # raised by best_coords_for_measurements before any number
        names = frame_markers(Q_coords)
        keypoints_names = list(keypoints_names)
        if len(set(keypoints_names)) != len(keypoints_names):
            raise ValueError('marker names must be unique')
        has = set(names)
        # the device table: the markers of keypoints_names first, in that order -- the speeds sum over them alone, left to
        # right --, then the frame's other markers, which the lengths and angles may still use
        order = [n for n in keypoints_names if n in has] + [n for n in names if n not in set(keypoints_names)]
        self.names = order
        self.n_speed = len(keypoints_names)
        at = {n: i for i, n in enumerate(names)}
        values = Q_coords.to_numpy(dtype=np.float64)
        self.table = values if order == names else values[:, [3 * at[n] + j for n in order for j in range(3)]]
        K = len(names)
        index = {n: i for i, n in enumerate(order)}
        index['MidShoulder'] = K
        self.add_hip = 'Hip' not in keypoints_names
        if 'MidShoulder' in has or (self.add_hip and 'Hip' in has):   # the reference would append a second marker of that name
            raise ValueError('marker names must be unique: the frame already has a column the reference appends')
        missing = [n for n in ('RShoulder', 'LShoulder') + (('RHip', 'LHip') if self.add_hip else ()) if n not in has]
        missing += [n for n in keypoints_names if n not in has]
        if missing:
            self.error = KeyError(missing[0])
            return
        if self.add_hip:
            index['Hip'] = K + 1
        self.roles = [index.get(n, -1) if n in has else -1 for n in _lib.P2S_MEASURE_ROLES]
        self.angles_ok = all(n in has for n in ANGLE_MARKERS)      # Hip and Neck (or the shoulders) are there by now
        self.flags = _lib.P2S_MEASURE_SPEED
        if restrict and self.angles_ok:
            self.flags |= _lib.P2S_MEASURE_ANGLES | _lib.P2S_MEASURE_RESTRICT
        known = lambda pair: all(n in index for n in pair)    # noqa: E731
        self.heel_ok = known(HEIGHT_PAIRS[0]) and known(HEIGHT_PAIRS[1])
        self.body_ok = all(known(p) for p in HEIGHT_PAIRS[2:])
        self.leg_ok = all(known(p) for p in HEIGHT_PAIRS[2:6])
        self.head = 'Head' if 'Head' in index else 'Nose' if 'Nose' in index else None
        self.head_factor = 1.008 if self.head == 'Head' else 1.5
        self.want_height, self.want_leg = height, leg
        fixed = [tuple(index[n] for n in p) if known(p) else (-1, -1) for p in HEIGHT_PAIRS]
        fixed.append((K, index[self.head]) if self.head else (-1, -1))
        if height and self.body_ok and self.head:
            self.flags |= _lib.P2S_MEASURE_HEIGHT | (0 if self.heel_ok else _lib.P2S_MEASURE_FEET_CONST)
        if leg and self.leg_ok:
            self.flags |= _lib.P2S_MEASURE_LEG
        self.pair_error = None
        extra = []
        for a, b in (pairs or ()):
            # dict_segment_ratio looks the names up with list.index on the marker list: ValueError for an unknown one
            if a not in has or b not in has:
                self.pair_error = ValueError(f'{a if a not in has else b!r} is not in list')
                extra = [(-1, -1)] * len(pairs)
                break
            extra.append((index[a], index[b]))
        self.pairs = fixed + extra

    def extended(self):
        """Q_coords with the MidShoulder (and Hip) columns best_coords_for_measurements appends."""
        Q = self.Q
        mid = pd.DataFrame((Q['RShoulder'].values + Q['LShoulder'].values) / 2)
        mid.columns = ['MidShoulder'] * 3
        Q = pd.concat((Q.reset_index(drop=True), mid), axis=1)
        if self.add_hip:
            hip = pd.DataFrame((Q['RHip'].values + Q['LHip'].values) / 2)
            hip.columns = ['Hip'] * 3
            Q = pd.concat((Q.reset_index(drop=True), hip), axis=1)
        return Q

    # what the reference logs and raises, in its order, given the device's result `res`
    def log_selection(self, res, large_hip_knee_angles):
        if res['all_slow']:
            logging.warning(MSG_ALL_SLOW)
        if not self.angles_ok:
            logging.warning(MSG_NO_ANGLES.format(large_hip_knee_angles))
        if res['all_data']:
            logging.warning(MSG_ALL_DATA)

    def finish_height(self, res):
        if not self.heel_ok:
            logging.warning(MSG_NO_HEEL)
        if not self.body_ok:
            logging.error(MSG_HEIGHT_LOG)
            raise ValueError(MSG_HEIGHT_RAISE)
        if self.head is None:
            raise KeyError('Nose')
        if self.head != 'Head':
            logging.warning(MSG_NO_HEAD)
        return np.float64(res['height'])

    def finish_leg(self, res):
        if not self.leg_ok:
            logging.error(MSG_LEG_LOG)
            raise ValueError(MSG_LEG_RAISE)
        return np.float64(res['leg_length'])


def _run(engine, plans, fastest_frames_to_remove_percent, close_to_zero_speed, large_hip_knee_angles, trimmed_extrema_percent=0.5):
    """Engine.body_measure for the plans without an early error -> one result (or None) per plan."""
    good = [p for p in plans if p.error is None]
    if not good:
        return [None] * len(plans)
    engine = engine or _make_engine()
    speed = np.broadcast_to(np.asarray(close_to_zero_speed, dtype=np.float64), (len(plans),))
    out = iter(engine.body_measure([p.table for p in good], [p.roles for p in good], [p.pairs for p in good], [p.flags for p in good],
                                   close_to_zero_speed=[s for s, p in zip(speed, plans) if p.error is None],
                                   fastest_frames_to_remove_percent=fastest_frames_to_remove_percent,
                                   large_hip_knee_angles=large_hip_knee_angles, trimmed_extrema_percent=trimmed_extrema_percent,
                                   head_factor=[p.head_factor for p in good], n_speed_markers=[p.n_speed for p in good]))
    return [next(out) if p.error is None else None for p in plans]


def _kept_frame(plan, res):
    Q = plan.extended()
    if res['all_data']:
        return Q.copy()
    kept = Q.iloc[res['kept_frame']]
    kept.index = pd.Index(res['kept_pos'], dtype=np.int64)
    return kept


def best_coords_for_measurements(Q_coords, keypoints_names, fastest_frames_to_remove_percent=0.2, close_to_zero_speed=0.2,
                                 large_hip_knee_angles=45, engine=None):
    """The rows of Q_coords fit for measuring (common.py:872-932): the frames whose summed marker speed is above
    close_to_zero_speed, the slowest 1 - fastest_frames_to_remove_percent of them, then those with a mean knee and hip
    angle below large_hip_knee_angles (the 50 smallest angles when fewer than 50 are; everything when none is left).
    -> DataFrame with the MidShoulder (and Hip) columns appended, rows and index as the reference returns them."""
    plan = _Plan(Q_coords, keypoints_names)
    if plan.error:
        raise plan.error
    res = _run(engine, [plan], fastest_frames_to_remove_percent, close_to_zero_speed, large_hip_knee_angles)[0]
    plan.log_selection(res, large_hip_knee_angles)
    return _kept_frame(plan, res)


def compute_height(Q_coords, keypoints_names, fastest_frames_to_remove_percent=0.1, close_to_zero_speed=50, large_hip_knee_angles=45,
                   trimmed_extrema_percent=0.5, engine=None):
    """The person's height from the trc data (common.py:935-990): per kept row the mean foot, shank, thigh and back
    lengths of both sides plus the head, then trimmed_mean.  Units of Q_coords."""
    plan = _Plan(Q_coords, keypoints_names, height=True)
    if plan.error:
        raise plan.error
    res = _run(engine, [plan], fastest_frames_to_remove_percent, close_to_zero_speed, large_hip_knee_angles, trimmed_extrema_percent)[0]
    plan.log_selection(res, large_hip_knee_angles)
    return plan.finish_height(res)


def compute_leg_length(trc_path, fastest_frames_to_remove_percent=0.1, close_to_zero_speed=50, large_hip_knee_angles=45,
                       trimmed_extrema_percent=0.5, engine=None):
    """The person's leg length, hip joint centre to ankle joint centre, from a .trc file (common.py:993-1034)."""
    Q_coords, _, _, markers, _ = _trc.read_trc(trc_path)
    plan = _Plan(Q_coords, markers, leg=True)
    if plan.error:
        raise plan.error
    res = _run(engine, [plan], fastest_frames_to_remove_percent, close_to_zero_speed, large_hip_knee_angles, trimmed_extrema_percent)[0]
    plan.log_selection(res, large_hip_knee_angles)
    return plan.finish_leg(res)


def trimmed_mean(arr, trimmed_extrema_percent=0.5, engine=None):
    """Mean of arr without its trimmed_extrema_percent most extreme values, half at either end (common.py:427-455)."""
    arr = np.asarray(arr, dtype=np.float64)
    if arr.ndim != 1:
        raise ValueError('trimmed_mean takes a 1-D array')
    if arr.size == 0:
        return np.float64(np.nan)
    return np.float64((engine or _make_engine()).trimmed_means([arr], trimmed_extrema_percent)[0])


def mean_angles(Q_coords, ang_to_consider=['right knee', 'left knee', 'right hip', 'left hip'], engine=None):
    """The mean of |right knee|, |left knee|, |right hip|, |left hip| flexion for every row (common.py:797-831).  Like the
    reference it needs a Hip column, takes the mid-shoulder for a missing Neck, and ignores ang_to_consider."""
    names = frame_markers(Q_coords)
    for n in (() if 'Neck' in names else ('RShoulder', 'LShoulder')) + ANGLE_MARKERS + ('Hip',):
        if n not in names:
            raise KeyError(n)
    roles = [names.index(n) if n in names else -1 for n in _lib.P2S_MEASURE_ROLES]
    res = (engine or _make_engine()).body_measure([Q_coords.to_numpy(dtype=np.float64)], [roles], np.zeros((1, 0, 2), dtype=np.int32),
                                                  [_lib.P2S_MEASURE_ANGLES])[0]
    return np.array(res['angles'])


def segment_lengths(Q_coords, markers, pairs, trimmed_extrema_percent=0.5, engine=None):
    """trimmed_mean(euclidean_distance(Q[a], Q[b])) for every (a, b) of pairs over all rows of Q_coords: the segment lengths
    dict_segment_ratio (kinematics.py:299-304) scales the model with.  As there, a marker's columns are found by its place
    in `markers`, and a name that is not in it raises ValueError.  -> float64 [len(pairs)]."""
    markers = list(markers)
    if len(set(markers)) != len(markers):
        raise ValueError('marker names must be unique')
    idx = np.array([(markers.index(a), markers.index(b)) for a, b in pairs], dtype=np.int32).reshape(-1, 2)
    table = Q_coords.to_numpy(dtype=np.float64)
    if table.shape[1] < 3 * len(markers):
        raise ValueError(f'{len(markers)} markers need {3 * len(markers)} columns, Q_coords has {table.shape[1]}')
    if len(idx) == 0 or len(table) == 0:
        return np.empty(0) if len(idx) == 0 else np.full(len(idx), np.nan)
    table = table[:, :table.shape[1] // 3 * 3]
    res = (engine or _make_engine()).body_measure([table], [[-1] * len(_lib.P2S_MEASURE_ROLES)], [idx], [0],
                                                  trimmed_extrema_percent=trimmed_extrema_percent)[0]
    return np.array(res['lengths'])


def _branch(res):
    return 'all_data' if res['all_data'] else 'few_small_angles' if res['few_small_angles'] else 'all_slow' if res['all_slow'] else 'selected'


def measure_batch(trc_paths, pairs=None, engine=None, fastest_frames_to_remove_percent=0.1, close_to_zero_speed=50,
                  large_hip_knee_angles=45, trimmed_extrema_percent=0.5):
    """compute_height, compute_leg_length and the segment lengths of `pairs` (marker-name pairs, measured on the rows
    best_coords_for_measurements keeps) for every file of trc_paths, all files in one device call.  close_to_zero_speed:
    one value or one per file (files in m and in px may share a call).  -> one dict per file: 'height', 'leg_length',
    'segment_lengths' -- each the value, or the exception the single-file function raises on that file --, 'frames_kept'
    (frame indices in the reference's order), 'branch' ('selected', 'all_slow', 'few_small_angles', 'all_data'), 'units'.
    The reference's warnings are logged once per file, in file order."""
    trc_paths = list(trc_paths)
    pairs = [tuple(p) for p in (pairs or ())]
    plans, units = [], []
    for path in trc_paths:
        Q_coords, _, _, markers, header = _trc.read_trc(path)
        plans.append(_Plan(Q_coords, markers, height=True, leg=True, pairs=pairs))
        fields = header[2].rstrip('\n').split('\t')
        units.append(fields[4] if len(fields) > 4 else '')
    results = _run(engine, plans, fastest_frames_to_remove_percent, close_to_zero_speed, large_hip_knee_angles, trimmed_extrema_percent)
    out = []
    for plan, res, unit in zip(plans, results, units):
        if plan.error:
            out.append({'height': plan.error, 'leg_length': plan.error, 'segment_lengths': plan.error, 'frames_kept': None,
                        'branch': None, 'units': unit})
            continue
        plan.log_selection(res, large_hip_knee_angles)
        one = {'frames_kept': res['kept_frame'], 'branch': _branch(res), 'units': unit}
        for key, finish in (('height', plan.finish_height), ('leg_length', plan.finish_leg)):
            try:
                one[key] = finish(res)
            except (ValueError, KeyError) as e:
                one[key] = e
        one['segment_lengths'] = plan.pair_error or np.array(res['lengths'][len(HEIGHT_PAIRS) + 1:])
        out.append(one)
    return out


def main():
    p = argparse.ArgumentParser(description='Height and leg length of the person of one or more .trc files, computed on the GPU.')
    p.add_argument('-i', '--trc_paths', required=True, nargs='+', help='input .trc files')
    p.add_argument('-f', '--fastest_frames_to_remove_percent', default=0.1, type=float, help='share of the fastest frames left out. Default 0.1')
    p.add_argument('-s', '--close_to_zero_speed', default=None, type=float,
                   help='summed marker speed per frame at or below which a frame is left out. Default 0.2 for a file in m, 50 otherwise (px)')
    p.add_argument('-a', '--large_hip_knee_angles', default=45, type=float, help='mean knee and hip angle from which a frame is left out. Default 45')
    p.add_argument('-t', '--trimmed_extrema_percent', default=0.5, type=float, help='share of extreme values trimmed before the mean. Default 0.5')
    args = p.parse_args()
    speeds = args.close_to_zero_speed
    if speeds is None:
        speeds = []
        for path in args.trc_paths:
            with open(path, 'r') as fh:
                fields = [next(fh) for _ in range(3)][2].rstrip('\n').split('\t')
            speeds.append(0.2 if len(fields) > 4 and fields[4] == 'm' else 50)
    results = measure_batch(args.trc_paths, None, None, args.fastest_frames_to_remove_percent, speeds, args.large_hip_knee_angles,
                            args.trimmed_extrema_percent)
    for path, res in zip(args.trc_paths, results):
        print(path)
        for key, label in (('height', 'Height'), ('leg_length', 'Leg length')):
            value = res[key]
            print(f'  {label}: ' + (f'{type(value).__name__}: {value}' if isinstance(value, Exception) else f'{value:.4f} {res["units"]}'))
        print(f'  Frames used: {len(res["frames_kept"]) if res["frames_kept"] is not None else 0} ({res["branch"]})')


if __name__ == '__main__':
    main()
