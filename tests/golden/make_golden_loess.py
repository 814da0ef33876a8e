"""Goldens of the LOESS filter of the filtering stage, recorded through the reference's own code -> loess_units.npz

statsmodels, from which the reference takes lowess, is not importable here.  What is recorded is therefore the
reference's loess_filter_1d (filtering.py:532-558: the NaN mask, the splitting into runs, the `len(seq) > kernel` test,
frac = kernel / len(seq), the absolute frame indices as abscissae) and filter_all (:728-830), executed unchanged, with
lowess replaced by statsmodels_standin.py; statsmodels itself has never run, and everything here is parity-unpinned
against it.  Next to every reference output the fixture stores the exact values of the definition (tests/loess_exact.py:
the weighted least-squares line of every sample at 60 digits), rounded to float64.

* columns through loess_filter_1d(config, frame_rate, pd.Series(col)) with nb_values_used in 2, 3, 4, 5, 5.5, 6, 30, 31
  and 257, at scales 1 and -1000: runs of exactly nb samples (left alone) and nb + 1 samples (the shortest that is
  filtered), runs split by one NaN, runs at the first and at the last frame, zeros inside a run (they stay data),
  constant and exactly linear columns, columns of 1 and of nb + 1 frames, an all-NaN column, and two runs that start
  near frame 99 000.  No run is longer than 400 samples and no frame index exceeds 100 000;
* the text filter_all writes with type = 'loess' on the synthetic .trc of the other filter goldens: nb_values_used 5
  under the key `loess`, and 30 under the key `LOESS` (the reference reads either) with the first frame at 17.

For every run gen() asserts that the reference's k = int(nb / L * L + 1e-10) is the k of pose2sim_amd.engine.loess_window.
Distance of the reference's outputs (stand-in, float64, sums over the absolute frame indices) from the exact values over
all columns and files of this fixture, relative to max(1, |value|): worst 9.7e-12 (column 56, a run at frame 98 765;
3.5e-14 over the columns whose frame indices stay below 1 000).  gen() refuses to write a fixture in which any column
is further than 1e-10.

The file is written with fixed zip time stamps: running this script again reproduces it byte for byte.
"""
import importlib
import logging
import os
import sys
import tempfile
import types

import numpy as np
import pandas as pd

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import ref_shim  # noqa: E402
import statsmodels_standin  # noqa: E402
import loess_exact  # noqa: E402
from make_golden_kalman import save_npz  # noqa: E402

NB_VALUES = (2, 3, 4, 5, 5.5, 6, 30, 31, 257)
NAN = 'nan'


def load_filtering():
    ref_shim.install()
    for name in ('statsmodels', 'statsmodels.nonparametric', 'filterpy', 'filterpy.kalman', 'filterpy.common'):
        sys.modules.setdefault(name, types.ModuleType(name))
    sys.modules['statsmodels.nonparametric.smoothers_lowess'] = statsmodels_standin
    sys.modules['filterpy.kalman'].KalmanFilter = None
    sys.modules['filterpy.common'].Q_discrete_white_noise = None
    import make_golden_filter as g1
    filt = importlib.import_module('Pose2Sim.filtering')
    assert filt.lowess is statsmodels_standin.lowess
    return filt, g1


def column(rng, layout, scale, kind='signal', zeros=()):
    """layout: run lengths (int) and NaN gaps ((NAN, length)) in order; zeros: positions set to exactly 0 afterwards."""
    L = sum(p if isinstance(p, int) else p[1] for p in layout)
    t = np.arange(L) / 60.0
    if kind == 'constant':
        col = np.full(L, scale * 1.5)
    elif kind == 'linear':
        col = scale * (0.25 + 0.125 * np.arange(L))              # exact in float64
    else:
        col = scale * (1.2 + 0.4 * np.sin(2 * np.pi * 1.1 * t + rng.uniform(0, 6)) + 0.05 * np.sin(2 * np.pi * 7 * t) + rng.normal(0, 0.005, L))
    at = 0
    for p in layout:
        if isinstance(p, int):
            at += p
        else:
            col[at:at + p[1]] = np.nan
            at += p[1]
    for z in zeros:
        assert not np.isnan(col[z])
        col[z] = 0.0
    return col


def cases():
    """(layout, nb_values_used, scale, kind, zeros)."""
    out = []
    for n, nb in enumerate(NB_VALUES):
        n0 = int(np.floor(nb))
        long_run = min(3 * n0 + 7, 400)
        s1, s2 = (1, -1000) if n % 2 == 0 else (-1000, 1)
        # a run of exactly nb samples at the first frame, the shortest filtered run, a long run up to the last frame
        out.append(([n0, (NAN, 1), n0 + 1, (NAN, 2), long_run], nb, s1, 'signal', ()))
        # starts late, zeros inside the filtered runs, one NaN splitting two filtered runs, ends early
        mid = min(2 * n0 + 5, 400)
        out.append(([(NAN, 3), mid, (NAN, 1), n0 + 2, (NAN, 4)], nb, s2, 'signal', (3 + mid // 2, 3 + mid // 2 + 1, 3 + mid + 1 + 1)))
        out.append(([min(n0 + 9, 400)], nb, s2, 'constant', ()))
        out.append(([(NAN, 1), min(2 * n0 + 3, 400)], nb, s1, 'linear', ()))
        out.append(([n0 + 1], nb, s1, 'signal', ()))                      # a column of nb + 1 frames
        out.append(([1], nb, s2, 'signal', ()))                           # a column of 1 frame
    out += [
        ([(NAN, 25)], 5, 1, 'signal', ()),                                # all NaN
        ([(NAN, 99000), 100], 5, 1, 'signal', ()),                        # large frame indices
        ([(NAN, 98765), 120, (NAN, 1), 31, (NAN, 2), 30], 30, -1000, 'signal', (98800,)),
    ]
    return out


def distance(got, want):
    assert got.shape == want.shape and np.array_equal(np.isnan(got), np.isnan(want))
    ok = ~np.isnan(want)
    return float((np.abs(got[ok] - want[ok]) / np.maximum(1.0, np.abs(want[ok]))).max()) if ok.any() else 0.0


def check_windows(col, nb):
    """The reference's k for every run it filters is the k the engine derives from nb alone."""
    from pose2sim_amd.engine import loess_window
    k, min_run = loess_window(nb)
    for seq in loess_exact.runs(col, nb):
        assert loess_exact.window(nb, len(seq)) == k and len(seq) >= min_run and len(seq) <= 400, (nb, len(seq))
        assert seq[-1] <= 100000
    good = np.where(~np.isnan(col))[0]
    if good.size:
        for seq in np.split(good, np.where(np.diff(good) > 1)[0] + 1):
            assert (len(seq) > nb) == (len(seq) >= min_run), (nb, len(seq))


def gen():
    filt, g1 = load_filtering()
    logging.disable(logging.CRITICAL)
    rng = np.random.default_rng(5757)
    out = {}
    worst = (0.0, 'none')
    for n, (layout, nb, scale, kind, zeros) in enumerate(cases()):
        col = column(rng, layout, scale, kind, zeros)
        cfg = g1.filter_config('.', 4, 6, 60)
        cfg['filtering']['loess'] = {'nb_values_used': nb}
        check_windows(col, nb)
        ref = np.asarray(filt.loess_filter_1d(cfg, 60, pd.Series(col.copy())), dtype=np.float64)
        exact = loess_exact.column(col, nb)
        d = distance(ref, exact)
        print(f'column {n}: {len(col)} frames, nb_values_used {nb}, scale {scale}, {kind}: |reference - exact| {d:.2e}', flush=True)
        assert d <= 1e-10, (n, d)
        worst = max(worst, (d, f'column {n}'), key=lambda v: v[0])
        out[f'col{n}_in'] = col
        out[f'col{n}_nb'] = np.array(float(nb))
        out[f'col{n}_out'] = ref
        out[f'col{n}_exact'] = exact
    out['n_cols'] = np.array(n + 1)

    # ---- filter_all with type = 'loess' on files ---------------------------------------------------------------------------
    from pose2sim_amd import trc
    for n, (frames, rate, first, nb, key) in enumerate(((160, 60, 0, 5, 'loess'), (90, 30, 17, 30, 'LOESS'))):
        with tempfile.TemporaryDirectory() as tmp:
            trial = os.path.join(tmp, 'trial')
            os.makedirs(os.path.join(trial, 'pose-3d'))
            name, text = g1.synthetic_trc_text(frames, rate, seed=1400 + n, first_frame=first)
            with open(os.path.join(trial, 'pose-3d', name), 'w') as fh:
                fh.write(text)
            cfg = g1.filter_config(trial, 4, 6, rate)
            cfg['filtering']['type'] = 'loess'
            del cfg['filtering']['loess']
            cfg['filtering'][key] = {'nb_values_used': nb}
            filt.filter_all(cfg)
            produced = sorted(f for f in os.listdir(os.path.join(trial, 'pose-3d')) if 'filt' in f)
            assert len(produced) == 1, produced
            raw = trc.load_trc(os.path.join(trial, 'pose-3d', name))[2]
            got = trc.load_trc(os.path.join(trial, 'pose-3d', produced[0]))[2]
            d = 0.0
            for c in range(raw.shape[1]):
                check_windows(raw[:, c], nb)
                d = max(d, distance(got[:, c], loess_exact.column(raw[:, c], nb)))
            print(f'file {n}: {frames} frames from {first}, nb_values_used {nb} under {key!r}: |reference - exact| {d:.2e}', flush=True)
            assert d <= 1e-10, (n, d)
            worst = max(worst, (d, f'file {n}'), key=lambda v: v[0])
            out[f'file{n}_name'] = np.array(name); out[f'file{n}_text'] = np.array(text)
            out[f'file{n}_rate'] = np.array(rate); out[f'file{n}_nb'] = np.array(nb); out[f'file{n}_key'] = np.array(key)
            out[f'file{n}_out_name'] = np.array(produced[0])
            out[f'file{n}_out_text'] = np.array(open(os.path.join(trial, 'pose-3d', produced[0])).read())
    out['n_files'] = np.array(n + 1)
    print(f'worst |reference - exact| relative to max(1, |value|): {worst[0]:.2e} ({worst[1]})')
    path = os.path.join(HERE, 'loess_units.npz')
    save_npz(path, out)
    print('loess_units.npz:', len(out), 'arrays,', os.path.getsize(path), 'bytes')


if __name__ == '__main__':
    gen()
