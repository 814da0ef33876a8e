"""NumPy / scipy stand-in for Engine.id_switch and Engine.lsap: the person filter, the cost of a pair, scipy's own
linear_sum_assignment and np.mean / np.median / np.percentile / np.min / np.max, as Utilities/id_switch_analyze.py calls
them.  Test infrastructure: it stands in for the Engine in the host tests and for the reference at sizes too big to
record; tests/test_idswitch_host.py pins it to the recorded goldens.  Also the seeded tables of the large tests."""
import numpy as np
from scipy.optimize import linear_sum_assignment

TABLES = ('counts', 'prev', 'zero_run', 'n_matched', 'n_lost', 'n_appeared', 'flags')
STATS = ('mean', 'median', 'p95', 'p99', 'min', 'max')
LSAP_ERRORS = {'matrix contains invalid numeric entries': 1, 'cost matrix is infeasible': 2}


def pair_cost(a, b):
    shared = (a[:, 2] > 0.1) & (b[:, 2] > 0.1)
    if shared.sum() < 3:
        return 1e9
    return float(np.sqrt(((a[shared, :2] - b[shared, :2]) ** 2).sum(axis=1)).mean())


def distance_stats(d):
    if len(d) == 0:
        return [np.nan] * 6
    d = np.array(d)
    return [np.mean(d), np.median(d), np.percentile(d, 95), np.percentile(d, 99), np.min(d), np.max(d)]


class NumpyIdSwitchEngine:
    def lsap(self, cost):
        cost = np.asarray(cost, dtype=np.float64)
        if cost.ndim == 2:
            r, c = linear_sum_assignment(cost)
            return r.astype(np.int32), c.astype(np.int32)
        pairs = [linear_sum_assignment(m) for m in cost]
        return (np.array([r for r, _ in pairs], dtype=np.int32).reshape(len(cost), -1),
                np.array([c for _, c in pairs], dtype=np.int32).reshape(len(cost), -1))

    def id_switch(self, cameras):
        out = {name: [] for name in TABLES + ('distances', 'kept')}
        stats = []
        for persons, offsets in cameras:
            t, distances, kept = camera_tables(np.asarray(persons, dtype=np.float64).reshape(-1, 26, 3), np.asarray(offsets, dtype=np.int64))
            for name in TABLES:
                out[name].append(t[name])
            out['distances'].append(np.array(distances, dtype=np.float64))
            out['kept'].append(kept)
            stats.append(distance_stats(distances))
        out['stats'] = np.array(stats, dtype=np.float64).reshape(len(cameras), 6)
        return out


def pair_costs(A, B):
    """pair_cost of every row of A [n][26][3] against the same row of B, the pairs grouped by their number of shared
    keypoints so that every mean is NumPy's own over a contiguous run of that many distances."""
    shared = (A[:, :, 2] > 0.1) & (B[:, :, 2] > 0.1)
    m = shared.sum(axis=1)
    with np.errstate(invalid='ignore'):
        d = np.sqrt(((A[:, :, :2] - B[:, :, :2]) ** 2).sum(axis=2))
    cost = np.full(len(A), 1e9)
    for k in np.unique(m[m >= 3]):
        rows = np.flatnonzero(m == k)
        cost[rows] = np.ascontiguousarray(d[rows][shared[rows]].reshape(len(rows), k)).mean(axis=1)
    return cost


def camera_tables(persons, offsets, chunk=8192):
    F = len(offsets) - 1
    t = {name: np.zeros(F, dtype=np.int32) for name in TABLES}
    with np.errstate(invalid='ignore'):
        keep = (persons[:, :, 2] > 0).any(axis=1)
    kept = np.flatnonzero(keep)
    first = np.searchsorted(kept, offsets)                            # [F + 1] every frame's run in `kept`
    counts = np.diff(first)
    frames = np.arange(F)
    last = np.maximum.accumulate(np.where(counts > 0, frames, -1))    # inclusive
    prev = np.concatenate([[-1], last[:-1]])[:F]
    t['counts'][:], t['prev'][:], t['zero_run'][:] = counts, prev, frames - 1 - prev
    todo = np.flatnonzero((counts > 0) & (prev >= 0))
    distances = []
    for c0 in range(0, len(todo), chunk):
        fs = todo[c0:c0 + chunk]
        P, Q = counts[prev[fs]], counts[fs]
        crowded = (P > 32) | (Q > 32)
        t['flags'][fs[crowded]] = 4
        fs, P, Q = fs[~crowded], P[~crowded], Q[~crowded]
        n_pairs = P * Q
        start = np.cumsum(n_pairs) - n_pairs
        local = np.arange(int(n_pairs.sum())) - np.repeat(start, n_pairs)
        i, j = local // np.repeat(Q, n_pairs), local % np.repeat(Q, n_pairs)
        cost = pair_costs(persons[kept[np.repeat(first[prev[fs]], n_pairs) + i]], persons[kept[np.repeat(first[fs], n_pairs) + j]])
        for n, f in enumerate(fs.tolist()):
            matrix = cost[start[n]:start[n] + n_pairs[n]].reshape(P[n], Q[n])
            try:
                rows, cols = linear_sum_assignment(matrix)
            except ValueError as e:
                t['flags'][f] = LSAP_ERRORS[str(e)]
                continue
            found = matrix[rows, cols]
            found = found[found < 1e9]
            distances.append(found)
            t['n_matched'][f], t['n_lost'][f], t['n_appeared'][f] = len(found), P[n] - len(found), Q[n] - len(found)
    return t, (np.concatenate(distances) if distances else np.zeros(0)), kept


def seeded_camera(F, seed, max_persons=4):
    """-> (persons [N][26][3], offsets [F + 1]): up to max_persons people who drift by a few pixels a frame, enter and leave,
    sometimes swap their list order or go missing for a while; about one confidence in ten is below 0.1, a few persons are
    listed with zero confidence throughout, a few frames hold nobody.  Three-decimal values, as detectors write them."""
    rng = np.random.default_rng(seed)
    shape = rng.uniform(-60, 60, (max_persons, 26, 2))
    centre = rng.uniform([300, 300], [1600, 800], (max_persons, 2))
    step = rng.normal(0, 3.0, (F, max_persons, 2)).cumsum(axis=0)
    present = np.ones((F, max_persons), dtype=bool)
    for p in range(max_persons):                                   # person p is away in a few stretches
        for start in rng.integers(0, F, max(1, F // 400) * (p + 1)):
            present[start:start + int(rng.integers(1, 40)), p] = False
    nobody = rng.random(F) < 0.01
    present[nobody] = False
    xy = centre[None, :, None, :] + step[:, :, None, :] + shape[None] + rng.normal(0, 1.0, (F, max_persons, 26, 2))
    conf = rng.uniform(0.3, 0.98, (F, max_persons, 26))
    conf[rng.random(conf.shape) < 0.1] = 0.05
    ghost = rng.random((F, max_persons)) < 0.02                    # listed, but dropped by the filter
    conf[ghost] = 0.0
    order = np.tile(np.arange(max_persons), (F, 1))
    swap = rng.random(F) < 0.05
    order[swap] = order[swap][:, ::-1]
    table = np.round(np.concatenate([xy, conf[..., None]], axis=3), 3)
    listed = np.take_along_axis(present, order, axis=1)              # in list order
    persons = np.take_along_axis(table, order[:, :, None, None], axis=1)[listed]
    return persons.reshape(-1, 26, 3), np.concatenate([[0], np.cumsum(listed.sum(axis=1))]).astype(np.int64)


def seeded_cameras(C, F, seed):
    return [seeded_camera(F, seed * 100 + c) for c in range(C)]
