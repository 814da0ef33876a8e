"""The ID switch kernels, the assignment solver and the whole utility on the MI355X, through the C-ABI: against the goldens
recorded from the reference (tests/golden/idswitch_units.npz), against NumPy and scipy themselves on single pairs and on
seeded matrices, and against the NumPy / scipy stand-in on scans of every length around the tile sizes, on large seeded
tables and on crowded frames: up to 32 x 32 persons, pair counts around the 64 lanes of a round and up to sixteen rounds, pairs that cannot
match, matrices scipy refuses and exact ties.  There is no tolerance: every array must be equal.  Every test prints its
figures before it asserts."""
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


# ---- crowded frames: the match kernel beyond one round of 64 pairs, up to 32 x 32 persons ------------------------------------
CROWDS = (8, 9, 12, 20, 32)                                          # max_persons of the seeded crowd cameras
BOUNDARY_COUNTS = (7, 9, 0, 8, 8, 5, 13, 5, 0, 0, 16, 8, 1, 32, 1, 32, 32, 31, 32, 20, 32, 33, 32, 32)   # kept persons per frame
# P * Q of every matched frame of BOUNDARY_COUNTS, against the last non-empty frame; the two frames that touch the 33 are refused
BOUNDARY_PAIRS = (63, 72, 64, 40, 65, 65, 80, 128, 8, 32, 32, 32, 1024, 992, 992, 640, 640, 1024)


def pair_counts(tables, c=0):
    """P * Q of every frame of camera c that has persons and a previous frame, 0 elsewhere, from the stand-in's tables."""
    counts, prev = tables['counts'][c].astype(np.int64), tables['prev'][c]
    return np.where((counts > 0) & (prev >= 0), counts[np.maximum(prev, 0)] * counts, 0)


def ghost_frames(cam, tables, c=0):
    """Frames that list another number of persons than the filter keeps."""
    return int((np.diff(cam[1]) != tables['counts'][c]).sum())


@pytest.fixture(scope='module')
def crowds():
    """{max_persons: (camera, the stand-in's result on it alone)}; the fixture proves what the tests below lean on."""
    out = {}
    for m in CROWDS:
        cam = isn.seeded_camera(400, 7000 + m, max_persons=m)
        ref = isn.NumpyIdSwitchEngine().id_switch([cam])
        pq = pair_counts(ref)
        assert pq.max() == 64 and (pq == 64).any() if m == 8 else (pq > 64).any(), m     # exactly one full round, or more
        assert ghost_frames(cam, ref) > 0 and ref['n_lost'][0].sum() > 0 and ref['n_appeared'][0].sum() > 0 and not ref['flags'][0].any(), m
        out[m] = (cam, ref)
    return out


@pytest.mark.parametrize('max_persons', CROWDS)
def test_seeded_crowd_equals_the_stand_in(engine, crowds, max_persons, capsys):
    cam, ref = crowds[max_persons]
    pq = pair_counts(ref)
    with capsys.disabled():
        print(f'crowd of {max_persons}: {int((pq > 64).sum())} frames with P*Q > 64, max P*Q {int(pq.max())}, '
              f'{ghost_frames(cam, ref)} ghost frames, {len(ref["distances"][0])} distances')
    same_tables(engine.id_switch([cam]), ref)


def test_seeded_crowds_in_one_call_equal_the_stand_in(engine, crowds, capsys):
    """Cameras of very different person totals: n_rows is the largest one's, the smaller cameras' columns end in NaN."""
    cams = [crowds[m][0] for m in CROWDS]
    ref = {key: [crowds[m][1][key][0] for m in CROWDS] for key in isn.TABLES + ('distances', 'kept')}
    ref['stats'] = np.concatenate([crowds[m][1]['stats'] for m in CROWDS])
    persons = [len(p) for p, _ in cams]
    with capsys.disabled():
        print(f'crowds {CROWDS} in one call: {persons} persons, {[len(d) for d in ref["distances"]]} distances')
    assert max(persons) > 2 * min(persons) and all(len(d) < max(persons) for d in ref['distances'])
    same_tables(engine.id_switch(cams), ref)


def boundary_camera(digits):
    """BOUNDARY_COUNTS persons a frame out of a pool of 33: everyone has a home, drifts a little from frame to frame, has
    about one confidence in ten below 0.1 and stands at a seeded random place of the frame's list."""
    rng = np.random.default_rng(33)
    home = np.stack([150.0 + 210.0 * (np.arange(33) % 8), 150.0 + 190.0 * (np.arange(33) // 8)], axis=1)     # [33][2]
    shape = rng.uniform(-60, 60, (33, 26, 2))
    persons = []
    for f, n in enumerate(BOUNDARY_COUNTS):
        who = rng.permutation(33)[:n]                                  # who is there, in list order
        xy = home[who, None, :] + shape[who] + rng.normal(0, 2.0, (n, 26, 2))
        conf = rng.uniform(0.3, 0.98, (n, 26))
        conf[rng.random(conf.shape) < 0.1] = 0.05
        persons.append(np.concatenate([xy, conf[..., None]], axis=2))
    persons = np.concatenate(persons)
    return (persons if digits is None else np.round(persons, digits)), np.concatenate([[0], np.cumsum(BOUNDARY_COUNTS)]).astype(np.int64)


@pytest.mark.parametrize('digits', (3, None), ids=('three decimals', 'full precision'))
def test_pair_count_boundaries(engine, digits, capsys):
    """One pair short of a round, a round, one pair more, two rounds, sixteen, and back; across empty frames; next to a
    frame with too many persons."""
    cam = boundary_camera(digits)
    ref = isn.NumpyIdSwitchEngine().id_switch([cam])
    pq, flags = pair_counts(ref), ref['flags'][0]
    with capsys.disabled():
        print(f'pair counts per frame {pq.tolist()}, flags {flags.tolist()}, matched {ref["n_matched"][0].tolist()}')
    assert tuple(ref['counts'][0]) == BOUNDARY_COUNTS
    assert tuple(pq[(pq > 0) & (flags == 0)]) == BOUNDARY_PAIRS
    assert flags.tolist() == [4 if f in (21, 22) else 0 for f in range(len(BOUNDARY_COUNTS))]
    assert (ref['n_matched'][0][(pq > 0) & (flags == 0)] > 0).all()
    same_tables(engine.id_switch([cam]), ref)


def half_bodies(n, k, seed):
    """Two frames of n persons: k with keypoints 0..12 only, then k with keypoints 13..25 only, and n - k whole ones in
    both, everyone at a seeded place of the list.  Upper against lower body shares no keypoint: 1e9."""
    rng = np.random.default_rng(seed)
    home = rng.uniform([200, 200], [1700, 900], (n, 2))
    shape = rng.uniform(-60, 60, (26, 2))
    frames = []
    for keep in (np.arange(26) < 13, np.arange(26) >= 13):
        xy = home[:, None, :] + shape[None] + rng.normal(0, 2.0, (n, 26, 2))
        conf = rng.uniform(0.3, 0.98, (n, 26))
        conf[:k] = np.where(keep, conf[:k], 0.05)
        frames.append(np.round(np.concatenate([xy, conf[..., None]], axis=2), 3)[rng.permutation(n)])
    return np.concatenate(frames), [0, n, 2 * n]


def test_unmatchable_pairs_inside_a_crowd(engine, capsys):
    cams = [half_bodies(16, 12, 1), half_bodies(32, 28, 2)]
    ref = isn.NumpyIdSwitchEngine().id_switch(cams)
    figures = [tuple(int(ref[key][c][1]) for key in ('n_matched', 'n_lost', 'n_appeared')) for c in range(2)]
    with capsys.disabled():
        print(f'half bodies among 16 and 32 persons: (matched, lost, appeared) {figures}')
    assert all(min(f) > 0 for f in figures) and not any(fl.any() for fl in ref['flags'])
    same_tables(engine.id_switch(cams), ref)


def refused_camera():
    """Five frames of 12 persons: a NaN coordinate on a shared keypoint of the last person of frame 1 (a cost that is NaN
    at pair 64 and beyond), an infinite person at the end of frame 3."""
    rng = np.random.default_rng(12)
    home = rng.uniform([200, 200], [1700, 900], (12, 2))
    shape = rng.uniform(-60, 60, (26, 2))
    xy = home[None, :, None, :] + shape[None, None] + rng.normal(0, 2.0, (5, 12, 26, 2))
    conf = rng.uniform(0.3, 0.98, (5, 12, 26))
    conf[rng.random(conf.shape) < 0.1] = 0.05
    p = np.round(np.concatenate([xy, conf[..., None]], axis=3), 3)
    p[0, :, 25, 2] = 0.9
    p[1, 11, 25] = [np.nan, p[1, 11, 25, 1], 0.9]
    p[3, 11, :, 0], p[3, 11, :, 2] = np.inf, 0.9
    return p.reshape(60, 26, 3), 12 * np.arange(6)


def test_scipys_refusals_on_a_large_matrix(engine, capsys):
    cam = refused_camera()
    ref = isn.NumpyIdSwitchEngine().id_switch([cam])
    with capsys.disabled():
        print(f'refusals at 12 x 12: flags {ref["flags"][0].tolist()}, matched {ref["n_matched"][0].tolist()}')
    assert ref['flags'][0].tolist() == [0, 1, 1, 2, 2] and not ref['n_matched'][0].any() and len(ref['distances'][0]) == 0
    first = np.array([isn.pair_cost(a, cam[0][12 + 11]) for a in cam[0][:12]])       # the column of frame 1's last person
    assert np.isnan(first).all() and 5 * 12 + 11 >= 64
    res = engine.id_switch([cam])
    same_tables(res, ref)
    assert np.isnan(res['stats']).all()


def twins_camera(n, seed):
    """Three frames of n persons, three of them listed twice with the same 78 numbers: equal rows and equal columns in the
    cost matrix; the twins stand still from frame 0 to 1 (a block of exact zeros) and move together from 1 to 2."""
    rng = np.random.default_rng(seed)
    home = rng.uniform([200, 200], [1700, 900], (n - 3, 2))
    shape = rng.uniform(-60, 60, (26, 2))
    frames = []
    for f in range(3):
        xy = home[:, None, :] + shape[None] + rng.normal(0, 2.0, (n - 3, 26, 2))
        conf = rng.uniform(0.3, 0.98, (n - 3, 26))
        conf[rng.random(conf.shape) < 0.1] = 0.05
        p = np.round(np.concatenate([xy, conf[..., None]], axis=2), 3)
        if f == 1:
            p[:3] = frames[0][:3]                                     # list places 0..2 of frame 0 hold the first twins
        frames.append(np.concatenate([p, p[:3]]))
    order = [np.arange(n), rng.permutation(n), rng.permutation(n)]
    return np.concatenate([fr[o] for fr, o in zip(frames, order)]), [0, n, 2 * n, 3 * n]


def test_exact_ties_inside_a_crowd(engine, capsys):
    cams = [twins_camera(n, n) for n in (20, 32, 9)]
    ref = isn.NumpyIdSwitchEngine().id_switch(cams)
    with capsys.disabled():
        print(f'twins among 20, 32 and 9 persons: matched {[m.tolist() for m in ref["n_matched"]]}, '
              f'zero distances {[int((d == 0).sum()) for d in ref["distances"]]}')
    for c, (p, off) in enumerate(cams):
        for f in range(3):
            rows = p[off[f]:off[f + 1]].reshape(-1, 78)
            assert len(rows) - len(np.unique(rows, axis=0)) == 3, (c, f)              # three persons twice
        assert (ref['distances'][c] == 0).sum() == 6 and not ref['flags'][c].any()    # both twins of each, matched at cost 0
    same_tables(engine.id_switch(cams), ref)
