"""Timing of the confidence kernels on the MI355X.

    python tests/sweeps/sweep_confidence.py [--out FILE] [--reps N]

Engine.confidence_stats on the two seeded workloads of tests/test_confidence_gpu.py (3 cameras x 108 000 frames, 8 x
36 000, 26 keypoints, thresholds 0.4 / 0.5 / 0.6): the kernels' time from HIP events around all of them (median and least
of N after one warm-up) and the call's own time (host clock, ends in a synchronise: holds the copies to and from the
device).  Bytes: with T the bytes of the tables, the transposition reads and writes T, the compaction reads T and writes
what is not NaN, the mean and the deviations read it once each (6 T together), and the selection reads it once for the
first histogram and eight or nine times per percentile pair (about 46 T, from L2 where the column fits).
Engine.column_mean_std alone: 81 columns of 108 000 rows."""
import argparse
import json
import os
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
sys.path.insert(0, os.path.dirname(HERE))

PEAK_BPS = 8.0e12
STREAM_PASSES, SELECT_PASSES = 6, 46


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=None)
    ap.add_argument('--reps', type=int, default=10)
    args = ap.parse_args()
    import confidence_numpy as cn
    from pose2sim_amd.engine import Engine
    eng = Engine(0)
    rows = []
    for C, F, seed in ((3, 108000, 2024), (8, 36000, 2025)):
        tables = cn.seeded_tables(C, F, seed)
        kernel, call = [], []
        for rep in range(args.reps + 1):
            t0 = time.perf_counter()
            res = eng.confidence_stats(tables, (0.4, 0.5, 0.6))
            call.append(time.perf_counter() - t0)
            kernel.append(eng.confidence_kernel_ms())
        T = C * F * 26 * 8
        rows.append({'shape': [C, F], 'entries': int(res['counts'].sum()), 'table_bytes': T,
                     'kernels_ms_median': float(np.median(kernel[1:])), 'kernels_ms_min': float(np.min(kernel[1:])),
                     'call_ms_median': float(np.median(call[1:]) * 1e3),
                     'stream_bytes': STREAM_PASSES * T, 'select_bytes': SELECT_PASSES * T,
                     'floor_us_all_passes': (STREAM_PASSES + SELECT_PASSES) * T / PEAK_BPS * 1e6,
                     'floor_us_one_read': T / PEAK_BPS * 1e6})
    cols = np.random.default_rng(1).uniform(0, 1, (108000, 81))
    times = []
    for rep in range(args.reps + 1):
        t0 = time.perf_counter()
        eng.column_mean_std(cols)
        times.append(time.perf_counter() - t0)
    res = {'confidence': rows, 'mean_std_81x108000_call_ms_median': float(np.median(times[1:]) * 1e3)}
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, 'w') as fh:
            fh.write(line + '\n')


if __name__ == '__main__':
    main()
