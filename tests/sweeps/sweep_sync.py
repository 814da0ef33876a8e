"""Timing of the synchronization stage and its kernels: C cameras x F frames, approx_time_maxspeed 'auto'.

    python tests/sweeps/sweep_sync.py [--cams 8] [--frames 36000] [--out FILE]        # on the GPU box
    python tests/sweeps/sweep_sync.py --reference --cams 8 --frames 6000              # the reference, on the build host

GPU mode: Engine.sync_speeds and Engine.lagged_pearson on the trial's own inputs (median of 5 after one warm-up), then
the whole stage (JSON parse, person choice, kernels, copies into pose-sync/) on the JSON files; checks that the planted
offsets are recovered.  Reference mode: the reference's synchronize_cams_all on the same trial (its CPU time).  Kernel
times per launch come from a separate `rocprofv3 --kernel-trace --stats` run of this script.
"""
import argparse
import json
import logging
import os
import shutil
import sys
import tempfile
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
import sync_trials as st  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--cams', type=int, default=8)
    ap.add_argument('--frames', type=int, default=36000)
    ap.add_argument('--reference', action='store_true')
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    shifts = [0, 7, -12, 25, -31, 44, 3, -18][:args.cams]
    logging.disable(logging.WARNING)
    tmp = tempfile.mkdtemp(prefix='sweep_sync_')
    res = {'cams': args.cams, 'frames': args.frames}
    try:
        t0 = time.perf_counter()
        trial = st.make_trial(31, [args.frames] * args.cams, shifts)
        trial_dir = os.path.join(tmp, 'trial')
        st.write_trial(trial, os.path.join(trial_dir, 'pose'))
        res['write_json_s'] = time.perf_counter() - t0
        cfg = st.sync_config(trial_dir)
        if args.reference:
            sys.path.insert(0, os.path.join(os.path.dirname(HERE), 'golden'))
            import importlib
            import ref_shim
            ref_shim.install()
            sync = importlib.import_module('Pose2Sim.synchronization')
            t0 = time.perf_counter()
            sync.synchronize_cams_all(cfg)
            res['reference_stage_s'] = time.perf_counter() - t0
        else:
            from scipy import signal
            from pose2sim_amd import synchronization
            from pose2sim_amd.engine import Engine
            eng = Engine(0)
            b, a = signal.butter(2, 6 / 15, 'low')
            zi = signal.lfilter_zi(b, a)
            coords = []
            for c in range(args.cams):
                xy = trial['xy'][c, :, 0].astype(np.float64) / 10
                lik = trial['lik'][c, :, 0].astype(np.float64) / 100
                xy[lik <= 0.4] = np.nan
                coords.append(np.ascontiguousarray(xy.reshape(args.frames, -1)))
            half = args.frames // 2

            def timed(fn, reps=5):
                fn()
                ts = []
                for _ in range(reps):
                    t = time.perf_counter()
                    out = fn()
                    ts.append(time.perf_counter() - t)
                return float(np.median(ts)), out
            res['sync_speeds_ms'], sp = timed(lambda: eng.sync_speeds(coords, b, a, zi))
            res['sync_speeds_ms'] *= 1e3
            res['lagged_pearson_ms'], (r, arg, mx) = timed(lambda: eng.lagged_pearson(sp[0], sp[1:], -half, half))
            res['lagged_pearson_ms'] *= 1e3
            res['pearson_offsets'] = [int(half - k) for k in arg]
            t0 = time.perf_counter()
            offsets = synchronization.synchronize_cams_all(cfg, engine=eng)
            res['stage_s'] = time.perf_counter() - t0
            res['offsets'] = offsets
            res['offsets_ok'] = offsets == [-s for s in shifts]
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, 'w') as fh:
            fh.write(line + '\n')


if __name__ == '__main__':
    main()
