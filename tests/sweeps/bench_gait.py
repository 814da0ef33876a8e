"""Times of the gait kernels and of trc_gaitevents_batch on the GPU.

    python tests/sweeps/bench_gait.py [--files 64] [--frames 36000] [--repeats 7] [--out gait_bench.json]

Kernel times are Engine.gait_kernel_ms() (HIP events around the kernels of one call): one warm-up call, then `repeats`
calls, median and extremes reported.  The end-to-end time of trc_gaitevents_batch includes reading the .trc files with
pandas, which dominates it; it is taken once per method after a warm-up on two files, and the reading is timed apart.
"""
import argparse
import contextlib
import io
import json
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), '..', '..'))
sys.path[:0] = [ROOT, os.path.join(ROOT, 'tests', 'golden')]
from make_golden_gait import make_trial  # noqa: E402

from pose2sim_amd import trc as p2s_trc  # noqa: E402
from pose2sim_amd import trc_gaitevents as tg  # noqa: E402
from pose2sim_amd.engine import Engine  # noqa: E402


def spread(values):
    v = sorted(values)
    return {'median': v[len(v) // 2], 'min': v[0], 'max': v[-1], 'n': len(v)}


def kernel_times(call, engine, repeats):
    call()
    ms = []
    for _ in range(repeats):
        call()
        ms.append(engine.gait_kernel_ms())
    return spread(ms)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--files', type=int, default=64)
    ap.add_argument('--frames', type=int, default=36000)
    ap.add_argument('--repeats', type=int, default=7)
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    engine = Engine(0)
    res = {'files': a.files, 'frames': a.frames}
    with tempfile.TemporaryDirectory() as folder:
        text = make_trial('walk', a.frames, 60, 'm', 'X', 'Y', 1, 0.002, 0.0)
        paths = []
        for i in range(a.files):
            paths.append(os.path.join(folder, f'trial_P{i}.trc'))
            with open(paths[-1], 'w') as fh:
                fh.write(text)
        t0 = time.perf_counter()
        p2s_trc.read_trc(paths[0])
        res['read_one_file_s'] = time.perf_counter() - t0
        for method in tg.METHODS:
            cfg = tg.resolve_args({'method': method})
            prep = tg._prepare(cfg, paths[0])
            preps = [prep] * a.files
            res[method] = {'kernel_ms': kernel_times(lambda: tg._detect(engine, preps), engine, a.repeats)}
            with contextlib.redirect_stdout(io.StringIO()):
                tg.trc_gaitevents_batch(paths[:2], method=method, engine=engine, output_file='warm.txt')
                t0 = time.perf_counter()
                out = tg.trc_gaitevents_batch(paths, method=method, engine=engine)
                res[method]['batch_s'] = time.perf_counter() - t0
            res[method]['events_first_file'] = [len(v) for v in out[0][1]]
            print(method, res[method], flush=True)
    rng = np.random.default_rng(3)
    table = np.round(np.cumsum(rng.normal(0, 1, (a.frames, 78)), axis=0), 2)
    for name, p in (('none', None), ('0.5', 0.5)):
        res[f'find_peaks_{a.frames}x78_prominence_{name}'] = dict(
            kernel_ms=kernel_times(lambda: engine.find_peaks(table, prominence=p), engine, a.repeats),
            peaks=int(sum(len(c[0]) for c in engine.find_peaks(table, prominence=p))))
    saw = np.repeat((np.arange(a.frames) + 10.0 * (np.arange(a.frames) % 2))[:, None], 78, axis=1)
    res[f'find_peaks_{a.frames}x78_rising_sawtooth'] = dict(kernel_ms=kernel_times(lambda: engine.find_peaks(saw, prominence=0.5), engine, a.repeats))
    print(json.dumps(res))
    if a.out:
        with open(a.out, 'w') as fh:
            json.dump(res, fh, indent=1)


if __name__ == '__main__':
    main()
