"""scipy / pandas restatement of Engine.find_peaks and Engine.gait_contacts: the live reference of tests/test_gait_gpu.py
and the engine that lets tests/test_gait_host.py run the whole utility without a GPU.  Test infrastructure, not a
fallback: the package never imports it."""
import itertools
import json
import os

import numpy as np
import pandas as pd
from scipy import signal
from scipy.ndimage import gaussian_filter1d

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'gait_units.npz')


def load_golden():
    g = np.load(GOLDEN)
    return g, json.loads(str(g['cases_json']))


def write_trial(g, trial, folder, name=None):
    path = os.path.join(str(folder), (name or trial) + '.trc')
    with open(path, 'wb') as fh:
        fh.write(bytes(g['trial_' + trial]))
    return path


def peaks_of_column(x, prominence):
    if prominence is None:
        peaks = signal.find_peaks(x)[0]
        return (peaks,) + tuple(signal.peak_prominences(x, peaks))
    peaks, props = signal.find_peaks(x, prominence=prominence)
    return peaks, props['prominences'], props['left_bases'], props['right_bases']


def contact_signal(column, method, dt, factor, sign=1, b=None, a=None):
    """What gait_events_height_coords / gait_events_fwd_vel do to one column, with pandas and scipy."""
    s = pd.Series(np.asarray(column, dtype=np.float64)) * factor
    if method == 'height_coordinates':
        return signal.filtfilt(b, a, s[1:])
    v = s.diff() / dt
    v = v.where(v < 0, other=0) if sign == -1 else v.where(v > 0, other=0)
    return gaussian_filter1d(v.abs()[1:], 5)


def runs_of(sig, threshold):
    """The runs of signal < threshold as the reference's start_end_true_seq and its callers list them -> (on, off): the
    first sample of every run but one that starts at sample 0, and the last sample of every run that ends before the
    signal does.  Stated over the runs themselves, not over edges as the kernel and the stand-in engine find them.  Raises
    IndexError, as the reference does, when no sample lies at or above the threshold."""
    low = (np.asarray(sig) < threshold).tolist()
    on, off, start = [], [], 0
    for is_low, run in itertools.groupby(low):
        stop = start + len(list(run))
        if is_low:
            if start > 0:
                on.append(start)
            if stop < len(low):
                off.append(stop - 1)
        start = stop
    if False not in low:
        raise IndexError('list index out of range')
    return on, off


class ScipyGaitEngine:
    def find_peaks(self, data, prominence=None):
        data = np.asarray(data, dtype=np.float64)
        bound = None if prominence is None else np.broadcast_to(np.asarray(prominence, dtype=np.float64), (data.shape[1],))
        return [peaks_of_column(data[:, c], None if bound is None else bound[c]) for c in range(data.shape[1])]

    def gait_contacts(self, columns, method, dt, threshold, factor=1.0, sign=1, b=None, a=None, zi=None, weights=None):
        n = len(columns)
        dt, threshold, factor = (np.broadcast_to(np.asarray(v, dtype=np.float64), (n,)) for v in (dt, threshold, factor))
        sigs, ons, offs, first = [], [], [], []
        for c, col in enumerate(columns):
            with np.errstate(invalid='ignore'):
                sig = contact_signal(col, method, dt[c], factor[c], sign, b, a)
            low = sig < threshold[c]
            edges = np.flatnonzero(low[1:] != low[:-1]) + 1
            sigs.append(sig)
            ons.append(np.array([i for i in edges if low[i]], dtype=np.int64))
            offs.append(np.array([i - 1 for i in edges if not low[i]], dtype=np.int64))
            first.append(bool(len(low) and low[0]))
        return sigs, ons, offs, np.array(first)
