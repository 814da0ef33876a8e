"""Person tracking across frames with NumPy and scipy (a helper, not a test): the loop of triangulation.py:823-874 around
sort_people_sports2d (common.py:1037-1136), with the slot table kept whole and the matched distances kept -- what
csrc/p2s_track.hip computes -- and the generator of the trials the tracking tests run."""
import warnings

import numpy as np
from scipy.optimize import linear_sum_assignment


def replay(Q, first_frame=0, max_dist=None, state=None):
    """Q [F][P][K][3] -> (Q_rows [F][P][K][3], ids [F][P], matched_dist [F][P], n_slots [F], state [n][K][3]).  The state is
    the last non-NaN value of every coordinate of every slot; it starts as P slots of NaN or as `state`, and has no limit
    of 32 slots."""
    F, P, K, _ = Q.shape
    S = np.full((P, K, 3), np.nan) if state is None else np.array(state, dtype=np.float64).reshape(-1, K, 3)
    Q_rows, ids = np.full((F, P, K, 3), np.nan), np.full((F, P), -1, dtype=np.int64)
    matched, n_slots = np.full((F, P), np.nan), np.zeros(F, dtype=np.int64)
    for fi in range(F):
        C, n = Q[fi], len(S)
        slot_det = np.full(max(n, P), -1, dtype=np.int64)
        slot_dist = np.full(max(n, P), np.nan)
        if first_frame + fi == 0 or n == 0:
            slot_det[:P] = np.arange(P)
        else:
            with warnings.catch_warnings():
                warnings.simplefilter('ignore')
                diff = C[np.newaxis, :, :, :] - S[:, np.newaxis, :, :]
                dist = np.nanmean(np.sqrt(np.nansum(diff ** 2, axis=3)), axis=2)
            dist = np.nan_to_num(dist, nan=1e10, posinf=1e10)
            pairs = [(i, j) for i, j in zip(*linear_sum_assignment(dist)) if max_dist is None or dist[i, j] <= max_dist]
            for i, j in pairs:
                slot_det[i], slot_dist[i] = j, dist[i, j]
            new = [j for j in range(P) if j not in {j for _, j in pairs}]
            slot_det = np.concatenate([slot_det[:n], new]).astype(np.int64)
            slot_dist = np.concatenate([slot_dist[:n], np.full(len(new), np.nan)])
        placed = np.where((slot_det >= 0)[:, None, None], C[np.maximum(slot_det, 0)], np.nan)
        S = np.concatenate([S, np.full((len(slot_det) - n, K, 3), np.nan)])
        S = np.where(np.isnan(placed), S, placed)
        Q_rows[fi], ids[fi], matched[fi], n_slots[fi] = placed[:P], slot_det[:P], slot_dist[:P], len(S)
    return Q_rows, ids, matched, n_slots, S


def make_trial(F, P, K, p_jump=0.0, seed=1):
    """Q [F][P][K][3]: persons as clouds of K points (body scale 0.3 m) around centres in +-2 m that drift by a random
    walk of 1 cm a frame, 5 mm of noise, a keypoint NaN with probability 0.1, a whole person NaN with probability 0.1,
    with probability p_jump a frame a person's centre moves 3 m for good, the detection order shuffled in every frame."""
    rng = np.random.default_rng(seed)
    centre, body = rng.uniform(-2, 2, (P, 1, 3)), rng.normal(0, 0.3, (P, K, 3))
    Q = np.empty((F, P, K, 3))
    for f in range(F):
        centre += rng.normal(0, 0.01, (P, 1, 3))
        jump = rng.random(P) < p_jump
        step = rng.normal(0, 1, (P, 1, 3))
        centre[jump] += 3.0 * (step / np.linalg.norm(step, axis=2, keepdims=True))[jump]
        order = rng.permutation(P)
        pts = centre + body + rng.normal(0, 0.005, (P, K, 3))
        pts[rng.random((P, K)) < 0.1] = np.nan
        pts[rng.random(P) < 0.1] = np.nan
        Q[f] = pts[order]
    return Q


def reordered_share(ids):
    """The share of the frames whose slots do not take the detections in their own order."""
    return float(np.mean((ids != np.arange(ids.shape[1])).any(axis=1)))


# (F, P, K, max_dist, p_jump) of the generated trials, seed 1
TRIALS = ((40, 3, 26, None, 0.0), (40, 3, 26, 1.0, 0.02), (40, 4, 17, 0.5, 0.05), (40, 8, 26, 1.0, 0.02), (40, 1, 26, 1.0, 0.05),
          (40, 2, 133, 1.0, 0.02))
OVERFLOW = (60, 4, 26, 1.0, 0.15)
