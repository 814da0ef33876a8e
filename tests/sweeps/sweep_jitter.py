"""Timing of the jitter kernels on the MI355X.

    python tests/sweeps/sweep_jitter.py [--out FILE] [--reps N]

Engine.jitter on the two seeded workloads of tests/test_jitter_gpu.py (3 cameras x 108 000 frames, 8 x 36 000): the
kernels' time from HIP events around all of them (median and least of N after one warm-up) and the call's own time
(host clock, ends in a synchronise: holds the copies to and from the device).  Under `rocprofv3 --kernel-trace --stats`
the per-kernel split comes from the profiler; the per-frame pass moves 624 B in and 216 B + 9 B out per frame, which
gives its share of the 8 TB/s roofline from the profiler's time for jitter_frames_kernel.
Engine.column_order_stats alone: 81 columns of 108 000 rows, both middle ranks."""
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
FRAME_BYTES = 624 + 216 + 9


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=None)
    ap.add_argument('--reps', type=int, default=10)
    args = ap.parse_args()
    import jitter_numpy as jn
    from pose2sim_amd.engine import Engine
    eng = Engine(0)
    rows = []
    for C, F, seed in ((3, 108000, 2024), (8, 36000, 2025)):
        series = [jn.seeded_series(F, seed * 100 + c) for c in range(C)]
        kernel, call = [], []
        for rep in range(args.reps + 1):
            t0 = time.perf_counter()
            res = eng.jitter(series)
            call.append(time.perf_counter() - t0)
            kernel.append(eng.jitter_kernel_ms())
        rows.append({'shape': [C, F], 'events': int(len(res['events'])), 'per_pattern': jn.pattern_counts(res['events']),
                     'kernels_ms_median': float(np.median(kernel[1:])), 'kernels_ms_min': float(np.min(kernel[1:])),
                     'call_ms_median': float(np.median(call[1:]) * 1e3), 'frame_pass_bytes': C * F * FRAME_BYTES,
                     'frame_pass_floor_us': C * F * FRAME_BYTES / PEAK_BPS * 1e6})
    cols = np.abs(np.random.default_rng(1).normal(3, 2, (108000, 81)))
    times = []
    for rep in range(args.reps + 1):
        t0 = time.perf_counter()
        eng.column_order_stats(cols, [(108000 - 1) // 2, 108000 // 2])
        times.append(time.perf_counter() - t0)
    res = {'jitter': rows, 'order_stats_81x108000_call_ms_median': float(np.median(times[1:]) * 1e3)}
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, 'w') as fh:
            fh.write(line + '\n')


if __name__ == '__main__':
    main()
