"""The primary-person selection on the MI355X, through the C-ABI: the whole utility against the goldens recorded from the
reference (tests/golden/extract_units.npz), and Engine.track_select against the NumPy restatement (tests/extract_numpy.py,
pinned to the reference's rule by tests/test_extract_host.py) on seeded cameras placed around the tile of the map scan.
There is no tolerance: chosen, n_candidates and prev must be equal.  Every test prints its figures before it asserts."""
import ctypes as C
import time

import numpy as np
import pytest

import extract_numpy as en
from pose2sim_amd import _lib
from test_extract_host import ALL, gold, run_case  # noqa: F401

pytestmark = pytest.mark.gpu

T = _lib.P2S_TRACK_TILE
LARGE = (8, 36000, 3)                                     # cameras, frames, persons: the workload's own shape


@pytest.fixture(scope='module')
def engine():
    from pose2sim_amd.engine import Engine
    return Engine(0)


def check(engine, cameras, n_kpts=26, thr=0.1):
    got = engine.track_select(cameras, n_kpts, thr)
    want = en.NumpyExtractEngine().track_select(cameras, n_kpts, thr)
    for key in ('n_candidates', 'prev', 'chosen'):
        for c in range(len(cameras)):
            assert np.array_equal(got[key][c], want[key][c]), (key, c, np.flatnonzero(got[key][c] != want[key][c])[:8])
    return got


@pytest.mark.parametrize('name', ALL)
def test_utility_on_the_gpu_reproduces_the_recorded_case(gold, engine, tmp_path, name, capsys, monkeypatch):   # noqa: F811
    run_case(gold, name, str(tmp_path), engine, capsys, monkeypatch)


@pytest.mark.parametrize('F', [1, 2, T - 1, T, T + 1, 2 * T + 1, 5 * T + 3])
def test_chain_lengths_around_the_tile(engine, F):
    cam = en.crowd_camera(F, 100 + F, 4)
    stats = en.chain_stats([cam])
    print(f'{F} frames: {stats[0][0]} depend on the previous choice, longest run {stats[0][1]}')
    check(engine, [cam])


@pytest.mark.parametrize('F', [255, 256, 257, 513])
def test_prev_across_the_edge_of_the_frame_tile(engine, F):
    """The previous selecting frame comes from a scan in tiles of 256 frames (p2s_scan.h; id_switch runs the same kernels):
    cameras that end before, on and one frame after a tile's edge and in a third tile.  Nobody is listed in frames 200 ..
    249 nor from frame 253 to the last but one (at most to 511), so the answers lie in a frame's own tile, in the tile before
    and, for 513 frames, two tiles back, past a tile without anybody.  A second, shorter camera goes in the same call: its
    last tile is not the grid's."""
    empty = [f for f in list(range(200, 250)) + list(range(253, min(F - 1, 512))) if f < F]
    cams = [en.crowd_camera(F, 200 + F, 3, empty=empty), en.crowd_camera(F - 130, 201 + F, 2, empty=range(100, F - 131))]
    got = check(engine, cams)
    prev, n = got['prev'], got['n_candidates']
    print(f'{F} and {F - 130} frames: prev[250] = {prev[0][250]}, prev of the last frames {prev[0][-1]} and {prev[1][-1]}, '
          f'frames with a candidate {int((n[0] > 0).sum())} and {int((n[1] > 0).sum())}')
    assert prev[0][250] == 199 and prev[0][-1] == 252 and n[0][-1] > 0
    assert prev[1][-1] == 99 and n[1][-1] > 0


def test_cameras_without_frames_and_without_candidates(engine):
    nobody = (np.zeros((0, 26, 3)), np.zeros(1, dtype=np.int64))
    weak = en.crowd_camera(2 * T + 5, 7, 3)
    weak[0][:, :, 2] = 0.05                                          # listed, never a candidate
    nan_x = en.crowd_camera(T + 1, 8, 2)
    nan_x[0][:, :, 0] = np.nan                                       # confident, but no x at all
    late = en.crowd_camera(6 * T + 9, 9, 3, empty=range(0, 4 * T + 3))   # the only candidates come after a long empty stretch
    unlisted = en.crowd_camera(3 * T, 10, 3, empty=range(3 * T))     # frames, nobody listed
    cams = [nobody, weak, en.crowd_camera(3 * T + 2, 11, 3), nan_x, late, nobody, unlisted]
    got = check(engine, cams)
    assert len(got['chosen'][0]) == 0 and (got['chosen'][1] == -1).all() and (got['chosen'][3] == -1).all() and (got['chosen'][6] == -1).all()
    assert (got['chosen'][4][:4 * T + 3] == -1).all() and (got['chosen'][4][4 * T + 3:] >= 0).all()
    assert got['prev'][4][4 * T + 3] == -1 and got['prev'][4][4 * T + 4] == 4 * T + 3
    check(engine, [nobody])


def test_four_unequal_cameras_in_one_call_and_one_call_each(engine):
    cams = [en.crowd_camera(F, 20 + i, n, empty=range(5, 5 + i * 7)) for i, (F, n) in enumerate(((7 * T + 3, 3), (T - 2, 5), (2 * T, 2), (260, 4)))]
    together = check(engine, cams)
    for c, cam in enumerate(cams):
        alone = engine.track_select([cam])
        for key in together:
            assert np.array_equal(alone[key][0], together[key][c]), (key, c)


def crowded(F, seed, counts):
    """Frame f keeps the first counts[f] of 33 listed persons."""
    persons, offsets = en.crowd_camera(F, seed, 33, p_dup=0.0)
    keep = (np.arange(33)[None, :] < np.asarray(counts)[:, None]).ravel()
    return persons[keep], np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)


def test_one_to_thirty_two_candidates(engine):
    counts = np.concatenate([np.arange(1, 33), np.arange(32, 0, -1), [32, 32, 1, 32, 2, 31]])
    cam = crowded(len(counts), 31, counts)
    stats = en.chain_stats([cam])
    print(f'{len(counts)} frames of 1 to 32 candidates: {stats[0][0]} depend on the previous choice')
    got = check(engine, [cam])
    assert np.array_equal(got['n_candidates'][0], counts)


def test_thirty_three_candidates_are_refused(engine):
    counts = np.full(5, 3)
    counts[2] = 33
    with pytest.raises(_lib.P2sError, match='camera 1, frame 2 has 33 candidates'):
        engine.track_select([en.crowd_camera(4, 1, 3), crowded(5, 32, counts)])
    weak = crowded(5, 32, counts)
    weak[0][weak[1][2], :, 2] = 0.05                                 # 33 listed, 32 of them candidates: taken
    check(engine, [weak])


@pytest.mark.parametrize('single', ['none', 'first slot', 'last slot', 'both'])
def test_the_scan_over_many_tiles(engine, single):
    """A crowd that never drops to one candidate by itself: the choice of nearly every frame depends on the one before, so
    the tiles' composed maps are not constant and the scan of the aggregates decides the answer."""
    F = 20 * T
    at = {'none': (), 'first slot': (7 * T,), 'last slot': (12 * T - 1,), 'both': (7 * T, 12 * T - 1, 15 * T - 1, 15 * T)}[single]
    cams = [en.crowd_camera(F, 40 + n, n, single_at=at) for n in (3, 4, 5, 6)]
    stats = en.chain_stats(cams)
    print(f'{single}: (frames that depend on the previous choice, longest run) per camera {stats} of {F} frames, tile {T}')
    for varies, longest in stats:
        assert varies >= F // 4
        assert longest >= 3 * T
    got = check(engine, cams)
    for c in range(len(cams)):
        for f in at:
            assert got['n_candidates'][c][f] == 1


@pytest.mark.parametrize('n_kpts', [1, 7, 8, 9, 16, 17, 26, 127])
def test_keypoint_counts_where_numpy_changes_branch(engine, n_kpts):
    persons, offsets, built = en.shared_camera(n_kpts, 50 + n_kpts)
    seen = en.camera_maps(persons, offsets)['shared']
    print(f'n_kpts {n_kpts}: shared-keypoint counts built in {sorted(built)}, met {sorted(seen)}')
    assert built <= seen and built == {m for m in (0, 1, 7, 8, n_kpts) if m <= n_kpts and not (m == 0 and n_kpts < 2)}
    check(engine, [(persons, offsets), en.crowd_camera(2 * T + 3, 60 + n_kpts, 4, n_kpts=n_kpts)], n_kpts=n_kpts)


def test_nan_values(engine):
    persons, offsets = en.crowd_camera(4 * T, 70, 3)
    rng = np.random.default_rng(71)
    n = len(persons)
    persons[rng.integers(0, n, n // 5), rng.integers(0, 26, n // 5), 0] = np.nan     # NaN x, often on a confident keypoint
    persons[rng.integers(0, n, n // 5), rng.integers(0, 26, n // 5), 2] = np.nan     # NaN confidence
    some = rng.integers(0, n, n // 8)
    persons[some, rng.integers(0, 26, len(some)), 1] = np.nan                        # NaN y: that person's mean is NaN
    maps = en.camera_maps(persons, offsets)
    print(f'{int(np.isnan(persons[:, :, 1]).any(axis=1).sum())} of {n} persons with a NaN y, {en.chain_stats([(persons, offsets)])}')
    check(engine, [(persons, offsets)])
    everybody = persons.copy()
    everybody[:, 3, 1] = np.nan                                      # every mean NaN: the fallback throughout
    everybody[:, 3, 2] = 0.9
    everybody[:, 3, 0] = 5.0
    got = check(engine, [(everybody, offsets)])
    assert maps['counts'].min() >= 2 and (got['chosen'][0] >= 0).all()


def test_refusals(engine):
    fn = engine._lib.p2s_track_select_host
    persons, offsets = en.crowd_camera(4, 80, 2, p_dup=0.0)
    n_frames = np.array([4], dtype=np.int64)
    out = np.zeros(4, dtype=np.int32)
    p = lambda a: a.ctypes.data_as(C.c_void_p)                       # noqa: E731

    def call(ctx=engine._h, cams=1, frames=n_frames, off=offsets, pers=persons, kpts=26):
        return fn(ctx, cams, None if frames is None else p(frames), None if off is None else p(off), None if pers is None else p(pers), kpts,
                  0.1, p(out), None, None)
    assert call() == 0                                               # two of the outputs may be NULL
    for kwargs in ({'ctx': None}, {'frames': None}, {'off': None}, {'pers': None}, {'kpts': 0}, {'kpts': 128}, {'cams': 0},
                   {'off': np.array([0, 2, 1, 6, 8], dtype=np.int64)}, {'off': np.array([1, 2, 4, 6, 8], dtype=np.int64)},
                   {'frames': np.array([-1], dtype=np.int64)}):
        assert call(**kwargs) == _lib.P2S_ERR_INVALID_ARG, kwargs
    from pose2sim_amd.engine import Engine
    fresh = Engine(0)
    with pytest.raises(_lib.P2sError, match='has not run'):
        fresh.track_select_kernel_ms()


def test_large_session(engine):
    Cn, F, n = LARGE
    t0 = time.perf_counter()
    cams = [en.crowd_camera(F, 900 + c, n, p_dup=0.0) for c in range(Cn)]
    t1 = time.perf_counter()
    want = en.NumpyExtractEngine().track_select(cams)
    t2 = time.perf_counter()
    engine.track_select(cams[:1])                                    # warm the staging buffers
    t3 = time.perf_counter()
    got = engine.track_select(cams)
    t4 = time.perf_counter()
    stats = en.chain_stats(cams[:1])
    print(f'{Cn} x {F} x {n}: kernels {engine.track_select_kernel_ms():.3f} ms, call {t4 - t3:.3f} s, restatement {t2 - t1:.2f} s, '
          f'generation {t1 - t0:.2f} s; camera 0: {stats[0]}')
    for key in ('n_candidates', 'prev', 'chosen'):
        for c in range(Cn):
            assert np.array_equal(got[key][c], want[key][c]), (key, c)
