"""csrc/p2s_host.h -- the thread pool, the thread-count rule and the UTF-8 check that the host-only translation units
share -- in a stand-alone program (tests/native/host_pool_driver.cpp) under AddressSanitizer + UBSan: every index is
visited exactly once at every (n, grain, thread count), a body that throws std::bad_alloc makes the call return false and
the process goes on."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_host_pool_under_asan_and_ubsan(tmp_path):
    exe = str(tmp_path / 'host_pool_driver')
    cmd = ['g++', '-std=c++17', '-O1', '-g', '-pthread', '-fsanitize=address,undefined', '-fno-omit-frame-pointer',
           '-I', os.path.join(ROOT, 'pose2sim_amd', 'csrc'), os.path.join(ROOT, 'tests', 'native', 'host_pool_driver.cpp'), '-o', exe]
    subprocess.run(cmd, check=True, capture_output=True)
    env = dict(os.environ, ASAN_OPTIONS='detect_leaks=1:abort_on_error=0', UBSAN_OPTIONS='halt_on_error=1:print_stacktrace=1')
    r = subprocess.run([exe], capture_output=True, text=True, env=env, timeout=300)
    assert r.returncode == 0, r.stdout[-1000:] + r.stderr[-4000:]
    assert 'runtime error' not in r.stderr and 'AddressSanitizer' not in r.stderr, r.stderr[-4000:]
    assert r.stdout.strip() == 'host pool ok'
