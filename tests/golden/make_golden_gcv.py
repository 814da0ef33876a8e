"""Goldens of the GCV smoothing-spline filter, recorded from the reference -> gcv_units.npz

* gcv_spline_filter_1d (filtering.py:163-313) on 60 columns of 5 to 1 500 samples (two of 1 500, the rest up to 400) with NaN / zero gaps, spikes, a flat
  stretch, a constant run (zero MAD) and a linear ramp: cut_off_frequency 'auto' with smoothing_factor 1, 0.5, 2 and 10,
  and integer cut-offs 3, 6, 10 Hz at 30 to 120 fps.  With each column the lambda of every filtered run (captured by
  wrapping the reference's _compute_optimal_gcv_parameter_numstable), and for 'auto' whether the run lies on a straight
  line (a constant run or a ramp: the penalty's null space, where the fit is exact whatever lambda, GCV is rounding noise
  and the lambda the search returns is arbitrary);
* filter_all (:728-830) with type = 'gcv_spline' on written .trc files ('auto'; a numeric cut-off; reject_outliers;
  a frame range), 40 to 50 frames each: the text it produces and the recap line it logs (texts stored as UTF-8 bytes);
* the exception the reference raises for a column holding a run of 3 samples.

Runs of 2 to 4 samples make the reference raise, so the generated columns and files have none (they are blanked).
"""
import io
import logging
import os
import sys
import tempfile

import numpy as np
import pandas as pd

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden_filter as g1  # noqa: E402


def blank_short_runs(col):
    """Set every run of 2 to 4 valid samples (not NaN, not 0) to NaN."""
    col = np.array(col, dtype=np.float64)
    good = np.flatnonzero(~(np.isnan(col) | (col == 0)))
    if len(good):
        for seq in np.split(good, np.flatnonzero(np.diff(good) > 1) + 1):
            if 2 <= len(seq) <= 4:
                col[seq] = np.nan
    return col


def column(rng, L, frame_rate, mode):
    t = np.arange(L) / frame_rate
    col = 1.2 + 0.4 * np.sin(2 * np.pi * 1.1 * t) + 0.05 * np.sin(2 * np.pi * 17 * t) + rng.normal(0, 0.01, L)
    if L > 20:
        spikes = rng.random(L) < 0.03
        col[spikes] += rng.normal(0, 0.3, int(spikes.sum()))
    if mode == 1 and L > 20:
        col[rng.random(L) < 0.03] = np.nan
    elif mode == 2 and L > 40:
        g = int(rng.integers(5, L - 30)); col[g:g + int(rng.integers(1, 25))] = np.nan
        col[rng.random(L) < 0.02] = 0.0
    elif mode == 3:
        col[:int(rng.integers(1, max(2, L // 3)))] = np.nan
    elif mode == 4 and L > 30:
        col[10:20] = col[9]                                                   # a flat stretch
    elif mode == 5:
        col[:] = 0.731                                                        # a constant run: MAD 0
    elif mode == 6:
        col = -0.4 + 0.002 * np.arange(L)                                     # a linear ramp: no roughness at all
    return blank_short_runs(col)


def with_lambdas(filt, fn):
    """Run fn() with the reference's GCV search wrapped; -> (result, the lambdas it returned, in call order)."""
    found = []
    orig = filt._compute_optimal_gcv_parameter_numstable

    def wrapped(x, y):
        lam = orig(x, y)
        found.append(float(lam))
        return lam
    filt._compute_optimal_gcv_parameter_numstable = wrapped
    try:
        return fn(), found
    finally:
        filt._compute_optimal_gcv_parameter_numstable = orig


def run_starts(col):
    good = np.flatnonzero(~(np.isnan(col) | (col == 0)))
    if not len(good):
        return []
    return [int(s[0]) for s in np.split(good, np.flatnonzero(np.diff(good) > 1) + 1) if len(s) >= 5]


def run_lengths(col):
    good = np.flatnonzero(~(np.isnan(col) | (col == 0)))
    if not len(good):
        return []
    return [len(s) for s in np.split(good, np.flatnonzero(np.diff(good) > 1) + 1) if len(s) >= 5]


def on_a_line(run):
    """The run lies on a straight line (to rounding): it is in the penalty's null space, every lambda fits it exactly
    and GCV is rounding noise -- the lambda the search returns is arbitrary (moving every sample one ulp up or down at
    random moves the reference's own from 36 to 45-74 on a ramp of 12 samples)."""
    x = np.arange(len(run))
    fit = np.polyval(np.polyfit(x, run, 1), x)
    return bool(np.max(np.abs(run - fit)) <= 1e-9 * max(1.0, float(np.max(np.abs(run)))))


def gcv_config(project_dir, cutoff, sf, frame_rate):
    cfg = g1.filter_config(project_dir, 4, 6, frame_rate)
    cfg['filtering']['type'] = 'gcv_spline'
    cfg['filtering']['gcv_spline'] = {'cut_off_frequency': cutoff, 'smoothing_factor': sf}
    return cfg


def trc_without_short_runs(n_frames, rate, seed, first_frame, frame_range=None):
    """make_golden_filter.synthetic_trc_text with the runs of 2 to 4 samples blanked, in the whole file and inside
    frame_range (blanking whole runs never shortens another run)."""
    name, text = g1.synthetic_trc_text(n_frames, rate, seed=seed, first_frame=first_frame)
    lines = text.split('\n')
    rows = pd.DataFrame([[float(v) if v else np.nan for v in r.split('\t')] for r in lines[5:] if r])
    frames = rows[0].to_numpy()
    inside = np.ones(len(rows), dtype=bool) if frame_range is None else (frames >= frame_range[0]) & (frames < frame_range[1])
    for c in range(2, rows.shape[1]):
        v = rows[c].to_numpy().copy()
        v[inside] = blank_short_runs(v[inside])
        rows[c] = blank_short_runs(v)
    rows[0] = rows[0].astype(int)
    buf = io.StringIO()
    rows.to_csv(buf, sep='\t', index=False, header=None, lineterminator='\n')
    return name, '\n'.join(lines[:5]) + '\n' + buf.getvalue()


def utf8(text):
    """A text as its UTF-8 bytes (uint8; a quarter of a NumPy unicode array): the tests decode gold[key].tobytes()."""
    return np.frombuffer(text.encode('utf-8'), dtype=np.uint8)


class _Lines(logging.Handler):
    def __init__(self):
        super().__init__()
        self.lines = []

    def emit(self, record):
        self.lines.append(record.getMessage())


def gen():
    filt, _ = g1.load_filtering()
    rng = np.random.default_rng(4242)
    out = {}

    # ---- columns through gcv_spline_filter_1d -----------------------------------------------------------------------------
    logging.disable(logging.CRITICAL)
    n = 0
    for case in range(60):
        L = int(rng.choice([5, 6, 9, 12, 31, 64, 120, 400])) if case >= 4 else [5, 5, 6, 1500][case]
        L = 1500 if case == 40 else L
        frame_rate = int(rng.choice([30, 60, 100, 120]))
        mode = case % 7
        col = column(rng, L, frame_rate, mode)
        auto = case % 3 != 2
        cutoff = 'auto' if auto else int(rng.choice([3, 6, 10]))
        sf = float(rng.choice([1.0, 0.5, 2.0, 10.0])) if auto else 1.0
        cfg = gcv_config('.', cutoff, sf, frame_rate)
        res, lams = with_lambdas(filt, lambda: filt.gcv_spline_filter_1d(cfg, frame_rate, pd.Series(col.copy())))
        starts = run_starts(col)
        lam = np.full(L, np.nan)
        if auto:
            assert len(lams) == len(starts)
            lam[starts] = np.array(lams) * sf
            free = np.full(L, np.nan)
            for s0, ln in zip(starts, run_lengths(col)):
                free[s0] = 1.0 if on_a_line(col[s0:s0 + ln]) else 0.0
            out[f'col{n}_lam_free'] = free
        else:
            lam[starts] = (frame_rate / (2 * np.pi * float(cutoff))) ** 4 * sf
        out[f'col{n}_in'] = col
        out[f'col{n}_prm'] = np.array([1.0 if auto else 0.0, sf, 0.0 if auto else float(cutoff), float(frame_rate)])
        out[f'col{n}_out'] = np.asarray(res, dtype=np.float64)
        out[f'col{n}_lam'] = lam
        n += 1
    out['n_cols'] = np.array(n)

    # ---- the refusal of a short run ---------------------------------------------------------------------------------------
    short = np.r_[1.0 + 0.01 * np.arange(8), np.nan, 2.0, 2.1, 2.2, np.nan, 1.0 + 0.01 * np.arange(8)]
    for key, cutoff in (('short_auto', 'auto'), ('short_fixed', 6)):
        try:
            filt.gcv_spline_filter_1d(gcv_config('.', cutoff, 1.0, 60), 60, pd.Series(short.copy()))
            raise AssertionError('the reference accepted a run of 3 samples')
        except ValueError as e:
            out[f'{key}_type'] = np.array(type(e).__name__)
            out[f'{key}_msg'] = np.array(str(e))
    out['short_in'] = short

    # ---- filter_all on files ----------------------------------------------------------------------------------------------
    logging.disable(logging.NOTSET)
    root = logging.getLogger()
    root.setLevel(logging.INFO)
    n = 0
    for (frames, rate, first, cutoff, sf, reject, frame_range) in ((48, 60, 0, 'auto', 1.0, False, 'auto'),
                                                                  (40, 30, 17, 6, 1.0, False, 'auto'),
                                                                  (44, 100, 0, 'auto', 2.0, True, 'auto'),
                                                                  (50, 60, 10, 'auto', 0.5, False, [25, 45])):
        with tempfile.TemporaryDirectory(prefix='gcv_') as tmp:
            trial = os.path.join(tmp, 'trial')
            os.makedirs(os.path.join(trial, 'pose-3d'))
            name, text = trc_without_short_runs(frames, rate, 1300 + n, first, None if frame_range == 'auto' else frame_range)
            with open(os.path.join(trial, 'pose-3d', name), 'w') as fh:
                fh.write(text)
            cfg = gcv_config(trial, cutoff, sf, rate)
            cfg['filtering']['reject_outliers'] = reject
            cfg['project']['frame_range'] = frame_range
            h = _Lines()
            root.addHandler(h)
            try:
                filt.filter_all(cfg)
            finally:
                root.removeHandler(h)
            produced = sorted(f for f in os.listdir(os.path.join(trial, 'pose-3d')) if 'filt' in f)
            assert len(produced) == 1, produced
            out[f'file{n}_name'] = np.array(name); out[f'file{n}_text'] = utf8(text)
            out[f'file{n}_prm'] = np.array([str(cutoff), repr(sf), str(reject), str(rate), str(frame_range)])
            out[f'file{n}_out_name'] = np.array(produced[0])
            out[f'file{n}_out_text'] = utf8(open(os.path.join(trial, 'pose-3d', produced[0])).read())
            out[f'file{n}_recap'] = np.array([m for m in h.lines if m.startswith('--> Filter type')][0])
        n += 1
    out['n_files'] = np.array(n)
    np.savez_compressed(os.path.join(HERE, 'gcv_units.npz'), **out)
    print('gcv_units.npz:', len(out), 'arrays')


if __name__ == '__main__':
    gen()
