"""The host code the primary-person extraction adds -- the parser's per-person flags, their gather and the writer of the
single-person documents -- under AddressSanitizer + UBSan (host build, g++, a stand-alone program): the acceptance corpus
of test_ingest.py, lists of every flag, and documents of the three kinds with extreme floats and the ends of int64.  Any
out-of-bounds access, leak or undefined behaviour fails."""
import os
import subprocess

import pytest

from test_ingest import DOCS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LISTS = ['1', '1.0', '-0', '10000000000', '99999999999999999999', '-99999999999999999999999999999999', '1, null', 'true, false', '"a"', '[[1]]', '',
         '1e999, -1e999, NaN, Infinity, -Infinity', ', '.join(['7'] * 78), ', '.join(['7.5'] * 399)]


@pytest.fixture(scope='module')
def driver(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp('asan') / 'extract_driver')
    src = os.path.join(ROOT, 'pose2sim_amd', 'csrc')
    cmd = ['g++', '-std=c++17', '-O1', '-g', '-fsanitize=address,undefined', '-fno-omit-frame-pointer', '-pthread', '-I', os.path.join(ROOT, 'include'),
           os.path.join(ROOT, 'tests', 'native', 'extract_driver.cpp')] + [os.path.join(src, f) for f in ('p2s_ingest.cpp', 'p2s_rewrite.cpp', 'p2s_trc.cpp')] + ['-o', exe]
    subprocess.run(cmd, check=True, capture_output=True)
    return exe


def test_flags_and_writer_under_asan_and_ubsan(driver, tmp_path):
    docs = [d.encode() if isinstance(d, str) else d for d in DOCS]
    docs += [('{"people": [7, {"pose_keypoints_2d": 3}, {"pose_keypoints_2d": [' + text + ']}]}').encode() for text in LISTS]
    docs.append(b'{"people": [{"pose_keypoints_2d": [1, 2], "pose_keypoints_2d": "x"}, {"pose_keypoints_2d": "x", "pose_keypoints_2d": [1.5]}]}')
    paths = []
    for i, d in enumerate(docs):
        p = tmp_path / f'd_{i:04d}.json'
        p.write_bytes(d)
        paths.append(str(p))
    paths += [str(tmp_path / 'missing.json'), '']
    env = dict(os.environ, ASAN_OPTIONS='detect_leaks=1:abort_on_error=0', UBSAN_OPTIONS='halt_on_error=1:print_stacktrace=1')
    for threads in ('1', '8'):
        out = tmp_path / f'out_{threads}'
        out.mkdir()
        r = subprocess.run([driver, threads, str(out)], input='\n'.join(paths) + '\n', capture_output=True, text=True, env=env, timeout=600)
        assert r.returncode == 0, r.stdout[-1000:] + r.stderr[-4000:]
        assert 'runtime error' not in r.stderr and 'AddressSanitizer' not in r.stderr, r.stderr[-4000:]
        assert r.stdout.startswith(f'files {len(paths)} ')
        assert len(os.listdir(out)) == 3 * 294
