"""NumPy stand-in for Engine.track_select: the reference's _select_person (Utilities/pose_extract_person.py:37-87) along a
camera, one frame after the other.  What a frame would choose for every possible previous choice is computed first, with
np.mean itself over contiguous runs of the shared keypoints' distances (the pairs grouped by their number of shared
keypoints, as tests/idswitch_numpy.py does); the walk over the frames is then a plain sequential loop.  Test
infrastructure: it stands in for the Engine in the host tests and for the reference at sizes too big to record;
tests/test_extract_host.py pins it to the recorded goldens and to the native host selection.  Also chain_stats, which says
how much of a camera really depends on the previous choice, and the seeded cameras of the GPU tests."""
import numpy as np

MAX_CANDIDATES = 32


def pair_means(A, B, valid_a, valid_b):
    """Mean distance of every row of A [n][K][3] to the same row of B over the keypoints valid in both; inf without one."""
    shared = valid_a & valid_b
    m = shared.sum(axis=1)
    with np.errstate(invalid='ignore', over='ignore'):
        d = np.sqrt(((B[:, :, :2] - A[:, :, :2]) ** 2).sum(axis=2))
    cost = np.full(len(A), np.inf)
    for k in np.unique(m[m > 0]):
        rows = np.flatnonzero(m == k)
        with np.errstate(invalid='ignore', over='ignore'):
            cost[rows] = np.ascontiguousarray(d[rows][shared[rows]].reshape(len(rows), k)).mean(axis=1)
    return cost, m


def camera_maps(persons, offsets, conf_threshold=0.1, chunk=8192):
    """-> dict: 'counts' [F] candidates, 'prev' [F], 'first' [F + 1] every frame's run in 'cand' (the candidates as indices
    into persons), 'maps' [F][32] uint8: what frame f chooses (a position in its candidate list) if the previous selecting
    frame chose its j-th candidate, 'P' [F] how many of those entries can be entered, 'shared' the set of shared-keypoint
    counts met."""
    F = len(offsets) - 1
    with np.errstate(invalid='ignore'):
        above = persons[:, :, 2] > conf_threshold
    valid = above & ~np.isnan(persons[:, :, 0])
    cand = np.flatnonzero(valid.any(axis=1))
    n_conf = above.sum(axis=1)
    first = np.searchsorted(cand, offsets)
    counts = np.diff(first).astype(np.int64)
    if (counts > MAX_CANDIDATES).any():
        raise ValueError(f'frame {int(np.flatnonzero(counts > MAX_CANDIDATES)[0])} has more than {MAX_CANDIDATES} candidates')
    frames = np.arange(F)
    last = np.maximum.accumulate(np.where(counts > 0, frames, -1)) if F else np.zeros(0, dtype=np.int64)
    prev = np.concatenate([[-1], last[:-1]])[:F].astype(np.int64)
    # the fallback: the first candidate with the most confidences above the threshold
    frame_of = np.repeat(frames, counts)
    order = np.lexsort((np.arange(len(cand)), -n_conf[cand], frame_of))
    fallback = np.zeros(F, dtype=np.int64)
    has = counts > 0
    fallback[has] = order[first[:-1][has]] - first[:-1][has]
    maps = np.zeros((F, MAX_CANDIDATES), dtype=np.uint8)
    maps[:] = np.where(has & (counts > 1), fallback, 0)[:, None]          # one candidate: it; no earlier choice: the fallback
    maps[~has] = np.arange(MAX_CANDIDATES, dtype=np.uint8)                # nobody: the previous choice stays
    P = np.where(has & (prev >= 0), counts[np.maximum(prev, 0)], 0)
    todo = np.flatnonzero((counts > 1) & (prev >= 0))
    shared_seen = set()
    for c0 in range(0, len(todo), chunk):
        fs = todo[c0:c0 + chunk]
        Pn, Qn = counts[prev[fs]], counts[fs]
        n_pairs = Pn * Qn
        start = np.cumsum(n_pairs) - n_pairs
        local = np.arange(int(n_pairs.sum())) - np.repeat(start, n_pairs)
        j, i = local // np.repeat(Qn, n_pairs), local % np.repeat(Qn, n_pairs)
        ia, ib = cand[np.repeat(first[prev[fs]], n_pairs) + j], cand[np.repeat(first[fs], n_pairs) + i]
        cost, m = pair_means(persons[ia], persons[ib], valid[ia], valid[ib])
        shared_seen |= set(np.unique(m).tolist())
        cost = np.where(np.isnan(cost), np.inf, cost)                     # NaN and inf are not eligible
        for p, q in set(zip(Pn.tolist(), Qn.tolist())):
            rows = np.flatnonzero((Pn == p) & (Qn == q))
            block = cost[start[rows][:, None] + np.arange(p * q)[None, :]].reshape(len(rows), p, q)
            best = block.argmin(axis=2)                                   # the first of equal means
            eligible = block.min(axis=2) < np.inf
            maps[fs[rows], :p] = np.where(eligible, best, fallback[fs[rows]][:, None])
    return {'counts': counts, 'prev': prev, 'first': first, 'cand': cand, 'maps': maps, 'P': P, 'shared': shared_seen}


def camera_select(persons, offsets, conf_threshold=0.1):
    t = camera_maps(persons, offsets, conf_threshold)
    F = len(offsets) - 1
    chosen = np.full(F, -1, dtype=np.int32)
    table = t['maps'].tobytes()
    state = 0
    for f in np.flatnonzero(t['counts'] > 0).tolist():                    # one frame after the other
        state = table[f * MAX_CANDIDATES + state]
        chosen[f] = state
    sel = chosen >= 0
    chosen[sel] = t['cand'][t['first'][:-1][sel] + chosen[sel]] - offsets[:-1][sel]
    return chosen, t['counts'].astype(np.int32), t['prev'].astype(np.int32)


class NumpyExtractEngine:
    def track_select(self, cameras, n_kpts=26, conf_threshold=0.1):
        out = {'chosen': [], 'n_candidates': [], 'prev': []}
        for persons, offsets in cameras:
            persons = np.asarray(persons, dtype=np.float64).reshape(-1, n_kpts, 3)
            c, n, p = camera_select(persons, np.asarray(offsets, dtype=np.int64), conf_threshold)
            out['chosen'].append(c); out['n_candidates'].append(n); out['prev'].append(p)
        return out


def chain_stats(cameras, n_kpts=26, conf_threshold=0.1):
    """Per camera (frames whose map is not constant -- the choice depends on the previous one --, the longest run of
    consecutive selecting frames without a constant map)."""
    out = []
    for persons, offsets in cameras:
        t = camera_maps(np.asarray(persons, dtype=np.float64).reshape(-1, n_kpts, 3), np.asarray(offsets, dtype=np.int64), conf_threshold)
        sel = np.flatnonzero(t['counts'] > 0)
        m, P = t['maps'][sel].astype(np.int64), t['P'][sel]
        inside = np.arange(MAX_CANDIDATES)[None, :] < np.maximum(P, 1)[:, None]
        varies = np.where(inside, m, m[:, :1]).max(axis=1) != np.where(inside, m, m[:, :1]).min(axis=1)
        longest = run = 0
        for v in varies.tolist():
            run = run + 1 if v else 0
            longest = max(longest, run)
        out.append((int(varies.sum()), longest))
    return out


def crowd_camera(F, seed, n_persons=4, n_kpts=26, single_at=(), empty=(), p_dup=0.02):
    """-> (persons [N][n_kpts][3], offsets [F + 1]): n_persons people on slow crossing paths, every one listed in every frame
    in shuffled order, coordinates rounded to 2 decimals; now and then a person is listed twice (an exact tie); about one
    confidence in ten is below the threshold.  Frames in `single_at` hold one candidate only (the others' confidences are all
    low): a constant map.  Frames in `empty` list nobody."""
    rng = np.random.default_rng(seed)
    shape = rng.uniform(-40, 40, (n_persons, n_kpts, 2))
    a, b = rng.uniform([200, 200], [1700, 900], (n_persons, 2)), rng.uniform([200, 200], [1700, 900], (n_persons, 2))
    w = (np.arange(F) / max(F - 1, 1))[:, None, None]
    centre = a[None] * (1 - w) + b[None] * w                              # straight paths that cross
    xy = centre[:, :, None, :] + shape[None] + rng.normal(0, 0.8, (F, n_persons, n_kpts, 2))
    conf = rng.uniform(0.3, 0.98, (F, n_persons, n_kpts))
    conf[rng.random(conf.shape) < 0.1] = 0.05
    conf[:, :, 0] = np.maximum(conf[:, :, 0], 0.3)                        # everybody stays a candidate
    table = np.round(np.concatenate([xy, conf[..., None]], axis=3), 2)
    order = rng.permuted(np.tile(np.arange(n_persons), (F, 1)), axis=1)
    listed = np.take_along_axis(table, order[:, :, None, None], axis=1)   # in list order
    single = np.array(sorted(set(single_at)), dtype=np.int64)
    listed[single, :-1, :, 2] = 0.05                                      # the last listed person alone stays a candidate
    reps = 1 + (rng.random((F, n_persons)) < p_dup)                       # listed twice: next to itself
    reps[np.array(sorted(set(empty)), dtype=np.int64)] = 0
    persons = np.repeat(listed.reshape(F * n_persons, n_kpts, 3), reps.ravel(), axis=0)
    return persons, np.concatenate([[0], np.cumsum(reps.sum(axis=1))]).astype(np.int64)


def shared_camera(n_kpts, seed, targets=(0, 1, 7, 8, None)):
    """A camera of two candidates a frame in which the keypoints shared with the previous choice number each of `targets`
    (None = all n_kpts) where n_kpts allows it.  -> (persons, offsets, the counts built in)."""
    rng = np.random.default_rng(seed)
    wanted = sorted({n_kpts if t is None else t for t in targets if (n_kpts if t is None else t) <= n_kpts and not (t == 0 and n_kpts < 2)})
    frames = []

    def frame(valid):
        kp = np.concatenate([rng.uniform(100, 900, (2, n_kpts, 2)).round(2), np.full((2, n_kpts, 1), 0.05)], axis=2)
        kp[:, valid, 2] = 0.9
        return kp
    every = np.arange(n_kpts)
    for m in wanted * 3:
        frames.append(frame(every))                                       # shares all with whatever came before it
        if m == 0:
            frames[-1] = frame(every[:-1])
            frames.append(frame(every[-1:]))                              # nothing in common: the fallback inside a run
        else:
            frames.append(frame(every[:m]))
    persons = np.concatenate(frames)
    return persons, np.arange(0, len(persons) + 1, 2, dtype=np.int64), set(wanted)
