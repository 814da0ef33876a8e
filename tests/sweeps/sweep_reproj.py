"""Timing of the reprojection kernel and of the reproj_from_trc_calib utility on the MI355X.

    python tests/sweeps/sweep_reproj.py [--out FILE] [--skip-files]

Kernel: Engine.reproject at 36 000 frames x 133 markers x 32 cameras, plain and distorted, with and without the unrounded
plane; the kernel's time from HIP events around it (median of 5 after one warm-up), achieved bytes/s from the shape
(24 B read per (frame, marker), 16 B written per camera, 32 B with the unrounded plane) and its share of the 6.3 TB/s a
streaming kernel achieves on this GPU.  The call's own time (host clock, ends in a synchronise) holds the copies too.
Utility, OpenPose only: 120 x 26 x 4 and 36 000 x 26 x 8 (288 000 files), split into reading the inputs, the kernel, the
copies around it and the file writing, and the whole call end to end."""
import argparse
import contextlib
import io
import json
import os
import shutil
import sys
import tempfile
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

ACHIEVABLE_BPS = 6.3e12


def kernel_rows(eng, F, K, Cn):
    from pose2sim_amd import synth
    rows = []
    for distort in (False, True):
        cams = synth.make_cameras(Cn, seed=9, distort=distort)
        Q = np.ascontiguousarray(synth.make_points3d(F, 1, K, seed=9)[:, 0])
        sizes = np.array(cams['S'])
        kw = {'cal': cams} if distort else {'P': np.array(synth.projection_matrices(cams))[:, None]}
        for raw in (True, False):
            kernel, call = [], []
            for rep in range(6):
                t0 = time.perf_counter()
                eng.reproject(Q, sizes=sizes, raw=raw, **kw)
                call.append(time.perf_counter() - t0)
                kernel.append(eng.reproject_kernel_ms())
            ms = float(np.median(kernel[1:]))
            nbytes = F * K * (24 + (32 if raw else 16) * Cn)
            rows.append({'shape': [F, K, Cn], 'distorted': distort, 'uv_raw': raw, 'kernel_ms': ms, 'bytes': nbytes,
                         'bytes_per_s': nbytes / (ms * 1e-3), 'share_of_achievable': nbytes / (ms * 1e-3) / ACHIEVABLE_BPS,
                         'call_s': float(np.median(call[1:]))})
    return rows


def utility_row(eng, tmp, F, K, Cn):
    from pose2sim_amd import calib, engine, synth, trc
    from pose2sim_amd import reproj_from_trc_calib as rp
    cams = synth.make_cameras(Cn, seed=5)
    Q = synth.make_points3d(F, 1, K, seed=5)[:, 0]
    work = os.path.join(tmp, f'u{F}')
    os.makedirs(work)
    trc_path = trc.write_trc(work, 'trial', np.arange(F), Q.reshape(F, -1), [f'M{k:02d}' for k in range(K)], 60)
    toml_path = os.path.join(work, 'Calib.toml')
    calib.write_calibration_toml(toml_path, cams)
    row = {'shape': [F, K, Cn], 'files': F * Cn}
    t0 = time.perf_counter()
    with contextlib.redirect_stdout(io.StringIO()):
        rp.reproj_from_trc_calib_func(engine=eng, input_trc_file=trc_path, input_calib_file=toml_path, openpose=True)
    row['end_to_end_s'] = time.perf_counter() - t0
    # the same steps under separate clocks, into a second folder
    t0 = time.perf_counter()
    _, _, Qz = rp.read_markers(trc_path)
    P, _ = rp.projection_matrices(rp.read_cameras(toml_path))
    row['read_s'] = time.perf_counter() - t0
    t0 = time.perf_counter()
    uv = eng.reproject(Qz, P=P, sizes=np.array(cams['S']))
    call = time.perf_counter() - t0
    row['kernel_s'] = eng.reproject_kernel_ms() * 1e-3
    row['copy_s'] = call - row['kernel_s']
    dirs = [os.path.join(work, 'again', f'cam{c + 1:02d}_json') for c in range(Cn)]
    for d in dirs:
        os.makedirs(d)
    t0 = time.perf_counter()
    n = engine.write_openpose_files(dirs, 'trial_0-0', uv)
    row['write_s'] = time.perf_counter() - t0
    assert n == F * Cn
    shutil.rmtree(work)
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=None)
    ap.add_argument('--skip-files', action='store_true', help='kernel rows only')
    args = ap.parse_args()
    from pose2sim_amd.engine import Engine
    eng = Engine(0)
    res = {'kernel': kernel_rows(eng, 36000, 133, 32), 'utility': []}
    if not args.skip_files:
        tmp = tempfile.mkdtemp(prefix='sweep_reproj_')
        try:
            res['utility'] = [utility_row(eng, tmp, 120, 26, 4), utility_row(eng, tmp, 36000, 26, 8)]
        finally:
            shutil.rmtree(tmp, ignore_errors=True)
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, 'w') as fh:
            fh.write(line + '\n')


if __name__ == '__main__':
    main()
