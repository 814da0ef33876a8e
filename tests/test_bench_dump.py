"""bench.py --dump-outputs: what the last timed step computed, written as finite float32 / float64 .npy files of at most
64 MB in all (which items are valid in an array of its own), the same from run to run for the same arguments (so that two
builds can be compared output for output)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import bench

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_dump_sample_is_fixed_and_fits_the_budget():
    assert np.array_equal(bench.dump_sample(1000, 40), np.arange(1000))
    n = 2_600_000                                          # cfg2's units, 40 B of results each
    a, b = bench.dump_sample(n, 40), bench.dump_sample(n, 40)
    assert np.array_equal(a, b)
    assert len(a) < n and (np.diff(a) > 0).all() and 0 <= a[0] and a[-1] < n
    assert len(a) * (40 + 8) <= bench.DUMP_BUDGET


def test_write_dump_takes_finite_floats_only(tmp_path):
    bench.write_dump(str(tmp_path / 'd'), {'x': np.zeros(3, np.float32), 'y': np.ones((2, 2))})
    assert np.array_equal(np.load(tmp_path / 'd' / 'y.npy'), np.ones((2, 2)))
    with pytest.raises(AssertionError):
        bench.write_dump(str(tmp_path / 'e'), {'i': np.zeros(3, np.int32)})
    for bad in (np.nan, np.inf):
        with pytest.raises(AssertionError):
            bench.write_dump(str(tmp_path / 'f'), {'x': np.array([1.0, bad])})


def test_invalid_items_are_zero_and_flagged_apart():
    Q = np.array([[1.0, 2.0, 3.0], [np.nan] * 3, [4.0, 5.0, 6.0]])
    err = np.array([0.5, np.nan, 1.5], np.float32)
    ok = np.isfinite(err)
    assert np.array_equal(bench.where_valid(ok, Q), [[1, 2, 3], [0, 0, 0], [4, 5, 6]])
    got = bench.where_valid(ok, err)
    assert got.dtype == np.float32 and np.array_equal(got, [0.5, 0, 1.5])


def test_steps_below_one_are_refused():
    env = {k: v for k, v in os.environ.items() if k not in ('WORLD_SIZE', 'RANK', 'LOCAL_RANK', 'MASTER_ADDR', 'MASTER_PORT')}
    env['P2S_BENCH_DRY'] = '1'
    r = subprocess.run([sys.executable, os.path.join(ROOT, 'bench.py'), '--steps', '0'], env=env, capture_output=True, text=True,
                       timeout=300)
    assert r.returncode != 0 and '--steps' in r.stderr


@pytest.mark.gpu
@pytest.mark.parametrize('config,steps,names', [
    ('cfg2', 7, {'unit_index', 'accepted', 'Q', 'err', 'n_excluded', 'camera_mask'}),
    ('single', 7, {'frame_index', 'found', 'combination', 'error', 'Q'}),
    ('cfg3', 2, {'frame_index', 'n_detections', 'affinity'})])
def test_dump_is_the_same_from_run_to_run(tmp_path, config, steps, names):
    """Two runs whose pre-rolls differ in length write identical, finite outputs of the last timed step."""
    dumps = []
    for preroll in ('0', '100'):
        d = tmp_path / f'dump_{preroll}'
        cmd = [sys.executable, os.path.join(ROOT, 'bench.py'), '--config', config, '--steps', str(steps), '--warmup', '2',
               '--no-cpu-baseline', '--preroll-ms', preroll, '--dump-outputs', str(d)]
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=900, cwd=ROOT)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
        assert json.loads([ln for ln in r.stdout.splitlines() if ln.startswith('{')][-1])['steps'] == steps
        files = sorted(os.listdir(d))
        assert {f[:-4] for f in files} == names
        assert sum(os.path.getsize(d / f) for f in files) <= 64_000_000
        dumps.append({f: np.load(d / f) for f in files})
    for f, a in dumps[0].items():
        assert a.dtype in (np.float32, np.float64), f
        assert np.isfinite(a).all(), f
        assert np.array_equal(a, dumps[1][f]), f
    if config == 'cfg2':
        assert dumps[0]['accepted.npy'].mean() > 0.99              # the accepted fraction of cfg2 is ~1
    if config == 'cfg3':
        assert (dumps[0]['n_detections.npy'] > 0).all() and np.abs(dumps[0]['affinity.npy']).max() > 0
