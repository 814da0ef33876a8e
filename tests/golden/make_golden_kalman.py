"""Goldens of the Kalman filter of the filtering stage, recorded through the reference's own code -> kalman_units.npz

filterpy, from which the reference takes KalmanFilter and Q_discrete_white_noise, is not importable here.  What is
recorded is therefore the reference's kalman_filter_1d / kalman_filter (filtering.py:316-434: initial state, F, H, P, R,
Q, the `smooth == True` test on int(smooth), the splitting into runs) and filter_all (:728-830), executed unchanged,
with filterpy's recursion replaced by filterpy_standin.py; filterpy itself has never run.  Next to every reference
output the fixture stores the exact posterior means of the same model (tests/kalman_exact.py: one dense solve at 60
digits, no recursion), rounded to float64.

* columns through kalman_filter_1d(config, frame_rate, pd.Series(col)): every frame rate of 25 / 30 / 60 / 120 / 240 with
  every trust ratio of 1 / 20 / 500 / 5000, `smooth` in {True, False, 1, 0, 2}, signal scales 1, 1000, -1 and -1000, as
  single runs that start at frame 0 and end at the last one; then constant columns, runs of 1, 2, 3 (left alone), 4, 5,
  6 and more samples split by NaN, by exact zeros and by both, a column that starts late, one that ends early, all-NaN
  and all-zero columns, columns of 1, 2, 3 and 4 frames, and two columns of a few hundred frames.  No run is longer
  than 100 samples (48 where only the filter runs, which costs one solve per sample), so every column has its exact
  values;
* the text filter_all writes with type = 'kalman' on the synthetic .trc of the other filter goldens: trust 500 with the
  smoother, and trust 20 with the filter alone.

Distance of the reference's outputs (stand-in recursion, float64) from the exact values over all columns of this
fixture, relative to max(1, |value|): worst 2.6e-15 (column 5: 100 samples at 30 fps, trust 20, smoother, scale -1).  gen()
refuses to write a fixture in which any column is further than 1e-10.

The file is written with fixed zip time stamps: running this script again reproduces it byte for byte.
"""
import importlib
import io
import itertools
import logging
import os
import sys
import tempfile
import types
import zipfile

import numpy as np
import pandas as pd

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import ref_shim  # noqa: E402
import filterpy_standin  # noqa: E402
import kalman_exact  # noqa: E402

SMOOTH_VALUES = {'True': True, 'False': False, '1': 1, '0': 0, '2': 2}     # stored by name: True and 1 are different cases
NAN, ZERO = 'nan', 'zero'


def load_filtering():
    ref_shim.install()
    for name in ('statsmodels', 'statsmodels.nonparametric', 'statsmodels.nonparametric.smoothers_lowess', 'filterpy'):
        sys.modules.setdefault(name, types.ModuleType(name))
    sys.modules['statsmodels.nonparametric.smoothers_lowess'].lowess = None
    sys.modules['filterpy.kalman'] = filterpy_standin
    sys.modules['filterpy.common'] = filterpy_standin
    import make_golden_filter as g1
    return importlib.import_module('Pose2Sim.filtering'), g1


def column(rng, layout, frame_rate, scale, constant=False):
    """layout: run lengths (int) and gaps ((NAN | ZERO, length)) in order."""
    L = sum(p if isinstance(p, int) else p[1] for p in layout)
    t = np.arange(L) / frame_rate
    col = scale * (1.2 + 0.4 * np.sin(2 * np.pi * 1.1 * t + rng.uniform(0, 6)) + 0.05 * np.sin(2 * np.pi * 7 * t) + rng.normal(0, 0.005, L))
    if constant:
        col[:] = scale * 1.5
    at = 0
    for p in layout:
        if isinstance(p, int):
            at += p
        else:
            col[at:at + p[1]] = np.nan if p[0] == NAN else 0.0
            at += p[1]
    return col


def cases():
    """(layout, frame_rate, trust_ratio, name of the smooth value, scale, constant)."""
    out = []
    names = list(SMOOTH_VALUES)
    scales = (1, 1000, -1, -1000)
    for i, (rate, trust) in enumerate(itertools.product((25, 30, 60, 120, 240), (1, 20, 500, 5000))):
        smooth = names[i % 5]
        L = (60, 100, 80, 37)[i % 4] if kalman_exact.smoothing_is_on(SMOOTH_VALUES[smooth]) else (48, 33, 20, 41)[i % 4]
        out.append(([L], rate, trust, smooth, scales[(i + i // 4) % 4], False))
    out += [
        ([30], 60, 500, 'True', 1, True),                                              # constant columns
        ([20], 100, 20, 'False', -1000, True),
        ([1, (NAN, 1), 2, (NAN, 2), 3, (NAN, 1), 4, (NAN, 3), 5, (NAN, 1), 6, (NAN, 2), 40], 30, 500, 'True', 1, False),
        ([1, (ZERO, 1), 2, (ZERO, 2), 3, (ZERO, 1), 4, (ZERO, 3), 5, (ZERO, 1), 6, (ZERO, 2), 40], 120, 500, 'False', 1, False),
        ([(NAN, 2), 7, (NAN, 1), (ZERO, 1), 30, (ZERO, 2), 3, (NAN, 1), 48, (ZERO, 1)], 240, 20, '2', 1000, False),
        ([(NAN, 5), 100], 60, 500, '1', 1, False),                                     # starts late, ends at the last frame
        ([64, (ZERO, 3)], 60, 500, 'True', -1000, False),                              # starts at frame 0, ends early
        ([(NAN, 25)], 60, 500, 'True', 1, False),                                      # all NaN
        ([(ZERO, 12)], 60, 500, 'False', 1, False),                                    # all zero
        ([1], 60, 500, 'True', 1, False), ([2], 60, 500, 'True', 1, False), ([3], 60, 500, 'True', 1, False),
        ([1, (NAN, 1), 1], 60, 500, 'False', 1, False),
        ([4], 25, 500, 'True', 1, False), ([4], 240, 20, 'False', 1000, False),        # the shortest run that is filtered
        ([5], 60, 1, '1', -1, False), ([6], 60, 5000, '0', 1, False),
        ([90, (NAN, 4), 100, (ZERO, 1), 75, (NAN, 1), 3, (NAN, 2), 60], 60, 500, 'True', 1, False),
        ([48, (NAN, 2), 40, (ZERO, 1), 48, (NAN, 1), 2, (ZERO, 2), 44, (NAN, 1), (ZERO, 1), 4, (NAN, 3), 45], 120, 20, '0', 1000, False),
    ]
    return out


def save_npz(path, arrays):
    """np.savez_compressed with fixed time stamps, so that the same arrays give the same bytes."""
    with zipfile.ZipFile(path, 'w', zipfile.ZIP_DEFLATED) as zf:
        for key, val in arrays.items():
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.asanyarray(val), allow_pickle=False)
            info = zipfile.ZipInfo(key + '.npy', date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            zf.writestr(info, buf.getvalue())


def gen():
    filt, g1 = load_filtering()
    logging.disable(logging.CRITICAL)
    rng = np.random.default_rng(4242)
    out = {}
    worst = (0.0, -1)
    for n, (layout, rate, trust, smooth, scale, constant) in enumerate(cases()):
        col = column(rng, layout, rate, scale, constant)
        cfg = g1.filter_config('.', 4, 6, rate)
        cfg['filtering']['kalman'] = {'trust_ratio': trust, 'smooth': SMOOTH_VALUES[smooth]}
        ref = np.asarray(filt.kalman_filter_1d(cfg, rate, pd.Series(col.copy())), dtype=np.float64)
        exact = kalman_exact.column(col, rate, trust, SMOOTH_VALUES[smooth])
        assert np.array_equal(np.isnan(ref), np.isnan(exact)), n
        ok = ~np.isnan(exact)
        d = float((np.abs(ref[ok] - exact[ok]) / np.maximum(1.0, np.abs(exact[ok]))).max()) if ok.any() else 0.0
        print(f'column {n}: {len(col)} frames, {rate} fps, trust {trust}, smooth {smooth}, scale {scale}: |reference - exact| {d:.2e}', flush=True)
        assert d <= 1e-10, (n, d)
        worst = max(worst, (d, n))
        out[f'col{n}_in'] = col
        out[f'col{n}_prm'] = np.array([rate, trust], dtype=np.int64)
        out[f'col{n}_smooth'] = np.array(smooth)
        out[f'col{n}_out'] = ref
        out[f'col{n}_exact'] = exact
    out['n_cols'] = np.array(n + 1)
    print(f'worst |reference - exact| relative to max(1, |value|): {worst[0]:.2e} (column {worst[1]})')

    # ---- filter_all with type = 'kalman' on files --------------------------------------------------------------------------
    for n, (frames, rate, first, trust, smooth) in enumerate(((160, 60, 0, 500, True), (90, 30, 17, 20, False))):
        with tempfile.TemporaryDirectory() as tmp:
            trial = os.path.join(tmp, 'trial')
            os.makedirs(os.path.join(trial, 'pose-3d'))
            name, text = g1.synthetic_trc_text(frames, rate, seed=1300 + n, first_frame=first)
            with open(os.path.join(trial, 'pose-3d', name), 'w') as fh:
                fh.write(text)
            cfg = g1.filter_config(trial, 4, 6, rate)
            cfg['filtering']['type'] = 'kalman'
            cfg['filtering']['kalman'] = {'trust_ratio': trust, 'smooth': smooth}
            filt.filter_all(cfg)
            produced = sorted(f for f in os.listdir(os.path.join(trial, 'pose-3d')) if 'filt' in f)
            assert len(produced) == 1, produced
            out[f'file{n}_name'] = np.array(name); out[f'file{n}_text'] = np.array(text)
            out[f'file{n}_rate'] = np.array(rate); out[f'file{n}_trust'] = np.array(trust); out[f'file{n}_smooth'] = np.array(smooth)
            out[f'file{n}_out_name'] = np.array(produced[0])
            out[f'file{n}_out_text'] = np.array(open(os.path.join(trial, 'pose-3d', produced[0])).read())
    out['n_files'] = np.array(n + 1)
    path = os.path.join(HERE, 'kalman_units.npz')
    save_npz(path, out)
    print('kalman_units.npz:', len(out), 'arrays,', os.path.getsize(path), 'bytes')


if __name__ == '__main__':
    gen()
