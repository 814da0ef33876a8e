"""The cases of person tracking across frames (a helper, not a test), shared by tests/test_track_host.py (the library's host
path) and tests/test_track_gpu.py (the kernel): every check takes `run`, a callable with the signature of
Engine.track_persons_3d, and compares exactly -- integers as integers, floats bit for bit with the NaNs in place."""
import functools
import os

import numpy as np

import track_numpy as tn
from pose2sim_amd import triangulation

NAMES = ('Q_rows', 'ids', 'matched_dist', 'n_slots', 'state')


def same(got, want):
    got, want = np.asarray(got), np.asarray(want)
    if got.shape != want.shape:
        return False
    if want.dtype.kind == 'f':
        return got.dtype == want.dtype and np.array_equal(np.isnan(got), np.isnan(want)) and \
            np.array_equal(got[~np.isnan(got)].view(np.int64), want[~np.isnan(want)].view(np.int64))
    return np.array_equal(got, want)


def assert_same_run(got, want, upto=None, what=''):
    """got: what `run` returned for one trial, want: track_numpy.replay's tuple; upto: compare the frames before it only
    (and not the state)."""
    for name, g, w in zip(NAMES, got, want):
        if upto is not None:
            if name == 'state':
                continue
            g, w = g[:upto], w[:upto]
        assert same(g, w), (what, name)


@functools.lru_cache(maxsize=None)
def generated(case, first):
    """(Q, max_dist, the mirror's replay) of TRIALS[case] (or of OVERFLOW for case -1) from frame `first`, checked against
    the stage's own host loop."""
    F, P, K, max_dist, p_jump = tn.OVERFLOW if case < 0 else tn.TRIALS[case]
    Q = tn.make_trial(F, P, K, p_jump, seed=1)
    want = tn.replay(Q, first, max_dist)
    rows, ids = triangulation.track_persons(Q, (first, first + F), True, max_dist)
    assert same(want[0], rows) and same(want[1], ids), (case, first)
    return Q, max_dist, want


def check_golden_steps(run, golden_dir):
    """The 60 recorded single steps of sort_people_sports2d: a one-frame trial from the recorded previous state."""
    z = np.load(os.path.join(golden_dir, 'host_units.npz'))
    n_cases, skipped, stateless = int(z['n_sort']), 0, 0
    assert n_cases == 60
    for i in range(n_cases):
        prev, curr = z[f'sort{i}_prev'], z[f'sort{i}_curr']
        max_dist = None if np.isnan(z[f'sort{i}_max']) else float(z[f'sort{i}_max'])
        P = len(curr)
        if P == 0:                                                   # no detection at all: n_persons = 0 is refused
            skipped += 1
            continue
        rows, ids, _, n_slots, state, status = run(curr[None], first_frame=1, max_dist=max_dist, state=prev)
        assert not status.any(), i
        assert same(rows[0], z[f'sort{i}_out1'][:P]), i
        if len(prev) == 0:                                           # the reference returns neither a state nor ids then
            stateless += 1
            assert same(ids[0], np.arange(P)) and n_slots[0] == P, i
            continue
        assert same(state, z[f'sort{i}_out0']), i
        assert same(ids[0], z[f'sort{i}_out2'][:P].astype(np.int32)), i
        assert n_slots[0] == len(z[f'sort{i}_out2']), i
    # of the 60 recorded cases 8 have no detection; the 12 without a previous state run with what the reference returns for them
    assert skipped == 8 and stateless == 12


def check_generated(run):
    """The generated trials one by one and all in one batched call, from frame 0 and from frame 5."""
    cases = [(c, first) for c in range(len(tn.TRIALS)) for first in (0, 5)]
    most_slots = 0
    for c, first in cases:
        Q, max_dist, want = generated(c, first)
        if Q.shape[1] >= 2:
            assert tn.reordered_share(want[1]) >= 0.5, (c, first)
        most_slots = max(most_slots, int(want[3].max()))
        got = run(Q, first_frame=first, max_dist=max_dist)
        assert not got[5].any()
        assert_same_run(got, want, what=(c, first))
    assert most_slots >= 12
    # one call per (P, K, max_dist): a batch shares them
    shapes = sorted({(tn.TRIALS[c][1], tn.TRIALS[c][2], tn.TRIALS[c][3]) for c, _ in cases}, key=str)
    for shape in shapes:
        batch = [(c, first) for c, first in cases if (tn.TRIALS[c][1], tn.TRIALS[c][2], tn.TRIALS[c][3]) == shape]
        got = run([generated(c, first)[0] for c, first in batch], first_frame=[first for _, first in batch], max_dist=shape[2])
        for b, (c, first) in enumerate(batch):
            assert not got[5][b].any()
            assert_same_run([g[b] for g in got[:5]], generated(c, first)[2], what=('batch', c, first))
    # trials of unequal lengths in one call: the K = 26, max_dist = 1.0 trial at three lengths
    Q, max_dist, _ = generated(1, 5)
    cuts = (40, 1, 17)
    got = run([Q[:n] for n in cuts], first_frame=5, max_dist=max_dist)
    for b, n in enumerate(cuts):
        assert_same_run([g[b] for g in got[:5]], tn.replay(Q[:n], 5, max_dist), what=('cut', n))


def check_overflow(run):
    """A trial that passes 32 slots: status names the frame, everything before it is the mirror's; cut one frame earlier
    it ends with exactly 32 slots and status 0."""
    Q, max_dist, want = generated(-1, 0)
    over = np.flatnonzero(want[3] > 32)
    assert len(over) and want[3].max() > 32
    first_over = int(over[0])
    got = run(Q, first_frame=0, max_dist=max_dist)
    assert list(got[5]) == [first_over + 1, 0]
    assert_same_run(got, want, upto=first_over, what='overflow')
    # from the frame that stopped the trial on the library writes nothing: the engine returns "nobody", not what came down
    assert np.isnan(got[0][first_over:]).all() and (got[1][first_over:] == -1).all() and np.isnan(got[2][first_over:]).all()
    assert not got[3][first_over:].any() and len(got[0]) == len(Q)
    short =tn.replay(Q[:first_over], 0, max_dist)
    assert short[3][-1] == 32
    got = run(Q[:first_over], first_frame=0, max_dist=max_dist)
    assert not got[5].any() and len(got[4]) == 32
    assert_same_run(got, short, what='exactly 32')
    # beside a trial that overflows, the others of a batch are whole
    got = run([Q, Q[:first_over]], first_frame=0, max_dist=max_dist)
    assert list(got[5][0]) == [first_over + 1, 0] and not got[5][1].any()
    assert_same_run([g[1] for g in got[:5]], short, what='batch beside an overflow')


def check_chunks(run):
    """One call equals two calls joined through the state, cut where there are more slots than persons."""
    for c, first in ((3, 0), (2, 5)):
        Q, max_dist, want = generated(c, first)
        P = Q.shape[1]
        cut = int(np.flatnonzero(want[3] > P)[0]) + 3
        assert 0 < cut < len(Q) and want[3][cut - 1] > P
        a = run(Q[:cut], first_frame=first, max_dist=max_dist)
        b = run(Q[cut:], first_frame=first + cut, max_dist=max_dist, state=a[4])
        joined = [np.concatenate([a[k], b[k]]) for k in range(4)] + [b[4]]
        assert not a[5].any() and not b[5].any()
        assert_same_run(joined, want, what=('chunks', c))


def check_degenerate(run):
    """Ties and degenerate frames: the assignment is whatever scipy gives."""
    rng = np.random.default_rng(5)
    trials = {}
    trials['all NaN'] = (np.full((6, 3, 26, 3), np.nan), 1.0)
    twins = tn.make_trial(8, 3, 26, 0.0, seed=3)
    twins[:, 1] = twins[:, 0]
    trials['two identical persons'] = (twins, None)
    trials['two identical persons, bounded'] = (twins, 0.5)
    inf = tn.make_trial(8, 3, 17, 0.0, seed=4)
    inf[2, 1, 5, 0] = np.inf
    inf[3, 0, 2, 1] = np.inf
    inf[5, 2, :, 2] = np.inf
    trials['+inf'] = (inf, 1.0)
    trials['+inf, unbounded'] = (inf, None)
    full = rng.uniform(-2, 2, (1, 32, 2, 3)) + rng.normal(0, 0.4, (5, 32, 2, 3))
    full = np.stack([f[rng.permutation(32)] for f in full])
    full[rng.random((5, 32, 2)) < 0.1] = np.nan
    trials['32 x 32'] = (full, None)
    trials['one keypoint'] = (tn.make_trial(12, 5, 1, 0.05, seed=6), 1.0)
    trials['7 keypoints'] = (tn.make_trial(12, 5, 7, 0.05, seed=7), 1.0)
    trials['128 keypoints'] = (tn.make_trial(6, 3, 128, 0.0, seed=8), None)
    trials['129 keypoints'] = (tn.make_trial(6, 3, 129, 0.0, seed=9), None)
    for what, (Q, max_dist) in trials.items():
        for first in (0, 3):
            want = tn.replay(Q, first, max_dist)
            rows, ids = triangulation.track_persons(Q, (first, first + len(Q)), True, max_dist)
            assert same(want[0], rows) and same(want[1], ids), what
            got = run(Q, first_frame=first, max_dist=max_dist)
            assert not got[5].any(), what
            assert_same_run(got, want, what=(what, first))
    got = run(np.empty((0, 3, 26, 3)))                               # a trial without frames: the state it started with
    assert got[0].shape == (0, 3, 26, 3) and got[4].shape == (3, 26, 3) and np.isnan(got[4]).all() and not got[5].any()
