"""The ID switch kernels, the assignment solver and the whole utility on the MI355X, through the C-ABI: against the goldens
recorded from the reference (tests/golden/idswitch_units.npz), against NumPy and scipy themselves on single pairs and on
seeded matrices, and against the NumPy / scipy stand-in on scans of every length around the tile sizes and on large seeded
tables.  There is no tolerance: every array must be equal.  Every test prints its figures before it asserts."""
import json
import os
import time

import numpy as np
import pytest

import idswitch_numpy as isn
from pose2sim_amd import id_switch_analyze as ids
from test_idswitch_host import (ALL, ERROR_CASES, KINDS, SHAPES, check_engine_on_case, check_lsap, gold, run_case)  # noqa: F401
from test_jitter_host import same

pytestmark = pytest.mark.gpu

LARGE = ((3, 108000, 2024), (8, 36000, 2025))            # (cameras, frames, seed): the sizes of tests/test_jitter_gpu.py
# frames per camera: around a wave (64), a tile of the per-frame passes (256) and four of them, a length that spans three
# tiles, and one that takes the scan of the tiles (1024 tiles a round) into its third round
SCAN_LENGTHS = (1, 2, 63, 64, 65, 255, 256, 257, 600, 1023, 1024, 1025, 2 * 1024 * 256 + 300)
COST_KINDS = ('three decimals', 'full precision', 'cancellation')


@pytest.fixture(scope='module')
def engine():
    from pose2sim_amd.engine import Engine
    return Engine(0)


def same_tables(res, ref):
    for key in ref:
        if key == 'stats':
            assert same(res[key], ref[key]), key
            continue
        assert len(res[key]) == len(ref[key]), key
        for c, (a, b) in enumerate(zip(res[key], ref[key])):
            assert a.dtype == b.dtype and same(a, b), (key, c)


@pytest.mark.parametrize('name', [n for n in ALL if n not in ERROR_CASES])
def test_kernels_reproduce_the_reference(gold, engine, tmp_path, name, capsys):   # noqa: F811
    with capsys.disabled():
        check_engine_on_case(gold, name, str(tmp_path), engine)


@pytest.mark.parametrize('name', ALL)
def test_utility_on_the_gpu_writes_the_recorded_files(gold, engine, tmp_path, name, capsys, monkeypatch):   # noqa: F811
    run_case(gold, name, str(tmp_path), engine, capsys, monkeypatch)


def pair(n_shared, kind, rng):
    """Two persons with exactly n_shared keypoints above 0.1 in both, at scattered places."""
    if kind == 'three decimals':
        a, b = np.round(rng.uniform(0, 1920, (26, 3)), 3), np.round(rng.uniform(0, 1920, (26, 3)), 3)
    elif kind == 'full precision':
        a, b = rng.uniform(0, 1920, (26, 3)), rng.uniform(0, 1920, (26, 3))
    else:                                                             # near 1e8 a double's last digit is 2^-26
        a, b = 1e8 + rng.integers(0, 64, (26, 3)) * 2.0 ** -26, 1e8 + rng.integers(0, 64, (26, 3)) * 2.0 ** -26
    shared = np.zeros(26, dtype=bool)
    shared[rng.choice(26, n_shared, replace=False)] = True
    a[:, 2] = np.where(shared | (rng.random(26) < 0.5), 0.8, 0.1)     # 0.1 itself is not above the threshold
    b[:, 2] = np.where(shared, 0.3, np.where(a[:, 2] > 0.1, 0.05, 0.9))
    return a, b


@pytest.mark.parametrize('kind', COST_KINDS)
def test_cost_of_one_pair_against_numpy(engine, kind, capsys):
    rng = np.random.default_rng(COST_KINDS.index(kind))
    pairs = [pair(n, kind, rng) for n in range(27) for _ in range(4)]
    res = engine.id_switch([(np.stack(p), [0, 1, 2]) for p in pairs])     # one camera a pair: two frames of one person
    want = [isn.pair_cost(a, b) for a, b in pairs]
    with capsys.disabled():
        print(f'pair costs, {kind}: {[float(d[0]) if len(d) else None for d in res["distances"]][::9]} (NumPy {want[::9]})')
    for c, (a, b) in enumerate(pairs):
        n = int(((a[:, 2] > 0.1) & (b[:, 2] > 0.1)).sum())
        assert n == c // 4
        if n < 3:
            assert want[c] == 1e9 and len(res['distances'][c]) == 0 and res['n_lost'][c][1] == 1 and res['n_appeared'][c][1] == 1
        else:
            assert same(res['distances'][c], [want[c]]), (kind, n)
            assert res['n_matched'][c][1] == 1 and same(res['stats'][c], [want[c]] * 6)


@pytest.mark.parametrize('kind', KINDS)
def test_lsap_on_the_gpu_equals_scipy(engine, kind):
    for shape in SHAPES:
        check_lsap(engine.lsap, shape, kind)


def test_lsap_refuses_what_scipy_refuses(engine):
    from scipy.optimize import linear_sum_assignment
    rows, cols = engine.lsap(np.array([[4.0, 1.0], [2.0, 8.0], [3.0, 3.0]]))      # one matrix, more rows than columns
    assert (list(rows), list(cols)) == tuple(map(list, linear_sum_assignment(np.array([[4.0, 1.0], [2.0, 8.0], [3.0, 3.0]]))))
    for bad in (np.nan, -np.inf, np.inf):
        cost = np.ones((2, 3, 3))
        cost[1, 1] = bad
        with pytest.raises(ValueError) as want:
            linear_sum_assignment(cost[1])
        with pytest.raises(ValueError) as caught:
            engine.lsap(cost)
        assert str(caught.value) == str(want.value)


def scan_camera(F, seed):
    """One person at most a frame, present in runs whose ends fall around every multiple of 64 frames: the empty runs
    start before a boundary and end on it, after it, or run across several."""
    rng = np.random.default_rng(seed)
    present = np.zeros(F, dtype=bool)
    f = int(rng.integers(0, 3))
    while f < F:
        run = int(rng.integers(1, 5)) if F < 5000 else int(rng.integers(1, 40))
        present[f:f + run] = True
        nxt = f + run + int(rng.integers(1, 6))
        edge = (nxt // 64 + 1) * 64 + int(rng.integers(-2, 3)) + 64 * int(rng.integers(0, 2 if F < 5000 else 40))
        f = edge if rng.random() < 0.7 else nxt
    n = int(present.sum())
    base = np.stack([100.0 + 7.0 * np.arange(26), 300.0 + 11.0 * (np.arange(26) % 6), np.full(26, 0.9)], axis=1)
    persons = np.repeat(base[None], n, axis=0)
    persons[:, :, 0] += np.arange(n)[:, None]
    return persons, np.concatenate([[0], np.cumsum(present)]).astype(np.int64)


def test_previous_frame_scan_on_every_length(engine, capsys):
    cams = [scan_camera(F, 10 + i) for i, F in enumerate(SCAN_LENGTHS)]
    ref = isn.NumpyIdSwitchEngine().id_switch(cams)
    res = engine.id_switch(cams)
    with capsys.disabled():
        print(f'scan lengths {SCAN_LENGTHS}: frames with a person {[int((c > 0).sum()) for c in res["counts"]]}, longest empty run '
              f'{[int(z.max()) for z in res["zero_run"]]}')
    for c, F in enumerate(SCAN_LENGTHS):                              # the fixture covers what it claims
        empty = ref['counts'][c] == 0
        for b in range(64, F, 64):
            if F < 5000:
                assert empty[max(b - 8, 0):b + 8].any(), (F, b)
        assert F < 3 or (ref['zero_run'][c].max() > 0 and (ref['prev'][c] >= 0).any())
    same_tables(res, ref)


def test_empty_cameras_and_single_frames(engine):
    ghost = np.zeros((5, 26, 3))
    ghost[:, :, 2] = [[0.0], [np.nan], [-1.0], [0.0], [np.nan]]
    one = (np.full((2, 26, 3), 0.5), [0, 2])
    cams = [(ghost, [0, 2, 2, 5]),                                    # persons listed, none kept
            (np.zeros((0, 26, 3)), [0, 0, 0]),                        # nobody listed
            one,                                                      # a single frame
            (np.zeros((0, 26, 3)), [0])]                              # no frame at all
    res, ref = engine.id_switch(cams), isn.NumpyIdSwitchEngine().id_switch(cams)
    same_tables(res, ref)
    assert [len(c) for c in res['counts']] == [3, 2, 1, 0] and not any(c.any() for c in res['counts'][:2]) and res['counts'][2][0] == 2
    assert np.isnan(res['stats']).all() and list(res['prev'][0]) == [-1, -1, -1] and list(res['zero_run'][0]) == [0, 1, 2]


def test_refusals(engine, tmp_path):
    from pose2sim_amd._lib import P2sError
    from pose2sim_amd.engine import Engine
    with pytest.raises(P2sError, match='p2s_id_switch_host has not run on this context'):
        Engine(0).id_switch_kernel_ms()
    with pytest.raises(P2sError, match='offsets must rise'):
        engine.id_switch([(np.zeros((2, 26, 3)), [0, 3])])
    crowd = np.full((33 + 32, 26, 3), 0.5)
    res = engine.id_switch([(crowd, [0, 32, 65])])
    assert list(res['counts'][0]) == [32, 33] and list(res['flags'][0]) == [0, 4] and len(res['distances'][0]) == 0
    cam = os.path.join(str(tmp_path), 'pose', 'cam01_json')
    os.makedirs(cam)
    for i, n in enumerate((32, 33)):
        with open(os.path.join(cam, f'{i}.json'), 'w') as fh:
            json.dump({'people': [{'pose_keypoints_2d': [0.5] * 78}] * n}, fh)
    with pytest.raises(ValueError, match='1.json holds 33 valid persons'):
        ids.analyze_id_switches(os.path.join(str(tmp_path), 'pose'), output_dir=os.path.join(str(tmp_path), 'out'), engine=engine)
    assert not os.path.exists(os.path.join(str(tmp_path), 'out'))


@pytest.mark.parametrize('C,F,seed', LARGE)
def test_large_seeded_tables_equal_the_stand_in(engine, C, F, seed, capsys):
    cams = isn.seeded_cameras(C, F, seed)
    ref = isn.NumpyIdSwitchEngine().id_switch(cams)
    first = engine.id_switch(cams)                                    # warm-up: code objects, allocations
    t0 = time.perf_counter()
    res = engine.id_switch(cams)
    call = time.perf_counter() - t0
    ms = engine.id_switch_kernel_ms()
    with capsys.disabled():
        print(f'id_switch {C} x {F}: {sum(len(p) for p, _ in cams)} persons, {sum(len(d) for d in res["distances"])} distances; '
              f'kernels {ms:.3f} ms, call with the copies {call * 1e3:.1f} ms')
    assert all((c == 0).any() and (c >= 3).any() for c in ref['counts']) and all(n.sum() > 0 for n in ref['n_lost'])
    same_tables(res, ref)
    for key in ref:
        for a, b in zip(first[key], res[key]):
            assert np.asarray(a).tobytes() == np.asarray(b).tobytes(), key     # two runs, the same bytes
