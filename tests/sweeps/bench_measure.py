"""Times of the measurement kernels and of measure_batch on the GPU.

    python tests/sweeps/bench_measure.py [--files 64] [--frames 36000] [--repeats 7] [--out measure_bench.json]

Kernel times are Engine.measure_kernel_ms() (HIP events around the kernels of one call): one warm-up call, then `repeats`
calls, median and extremes reported.  The end-to-end time of measure_batch includes reading the .trc files with pandas,
which dominates it; it is taken after a warm-up on two files, and the reading is timed apart.
"""
import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), '..', '..'))
sys.path[:0] = [ROOT, os.path.join(ROOT, 'tests', 'golden')]
from make_golden_measure import HALPE_26, SEGMENTS, make_trial  # noqa: E402

from pose2sim_amd import measurements  # noqa: E402
from pose2sim_amd import trc as p2s_trc  # noqa: E402
from pose2sim_amd.engine import Engine  # noqa: E402


def spread(values):
    v = sorted(values)
    return {'median': v[len(v) // 2], 'min': v[0], 'max': v[-1], 'n': len(v)}


def kernel_times(call, engine, repeats):
    call()
    ms = []
    for _ in range(repeats):
        call()
        ms.append(engine.measure_kernel_ms())
    return spread(ms)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--files', type=int, default=64)
    ap.add_argument('--frames', type=int, default=36000)
    ap.add_argument('--repeats', type=int, default=7)
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    engine = Engine(0)
    res = {'files': a.files, 'frames': a.frames, 'markers': len(HALPE_26), 'segment_pairs': len(SEGMENTS)}
    with tempfile.TemporaryDirectory() as folder:
        text = make_trial('walk', a.frames, 'm', HALPE_26, seed=3)
        paths = []
        for i in range(a.files):
            paths.append(os.path.join(folder, f'trial_P{i}.trc'))
            with open(paths[-1], 'w') as fh:
                fh.write(text)
        t0 = time.perf_counter()
        Q_coords, _, _, markers, _ = p2s_trc.read_trc(paths[0])
        res['read_one_file_s'] = time.perf_counter() - t0
        plan = measurements._Plan(Q_coords, markers, height=True, leg=True, pairs=SEGMENTS)
        for count in sorted({1, a.files}):
            plans = [plan] * count
            res[f'body_measure_{count}_files'] = {'kernel_ms': kernel_times(lambda: measurements._run(engine, plans, 0.1, 0.2, 45, 0.5), engine, a.repeats)}
            print(count, res[f'body_measure_{count}_files'], flush=True)
        measurements.measure_batch(paths[:2], pairs=SEGMENTS, engine=engine, close_to_zero_speed=0.2)
        t0 = time.perf_counter()
        out = measurements.measure_batch(paths, pairs=SEGMENTS, engine=engine, close_to_zero_speed=0.2)
        res['measure_batch_s'] = time.perf_counter() - t0
        res['first_file'] = {'height': float(out[0]['height']), 'leg_length': float(out[0]['leg_length']), 'frames_kept': len(out[0]['frames_kept'])}
    rng = np.random.default_rng(3)
    columns = [np.round(np.cumsum(rng.normal(0, 1, a.frames)), 2) for _ in range(78)]
    res[f'stable_argsort_78x{a.frames}'] = {'kernel_ms': kernel_times(lambda: engine.stable_argsort(columns), engine, a.repeats)}
    res[f'trimmed_means_78x{a.frames}'] = {'kernel_ms': kernel_times(lambda: engine.trimmed_means(columns, 0.5), engine, a.repeats)}
    print(json.dumps(res))
    if a.out:
        with open(a.out, 'w') as fh:
            json.dump(res, fh, indent=1)


if __name__ == '__main__':
    main()
