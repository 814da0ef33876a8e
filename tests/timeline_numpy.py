"""NumPy mirror of the device contract of csrc/p2s_timeline.hip (Engine.timeline_rows), written from the loop of
Pose2Sim/Utilities/confidence_timeline.py:93-130: arrays in, arrays out, a Python loop over files, persons and slots as
there.  Checked against the goldens in tests/test_timeline_host.py; the host path and the kernels are checked against it."""
import csv
import io
import json

import numpy as np

N_KEYPOINTS = 26
OUTPUTS = ('row_off', 'frame', 'person', 'slot', 'confidence', 'n_people', 'series_off', 'series_frame', 'series_conf')


def timeline_rows(file_off, person_base, valid, conf):
    """What Engine.timeline_rows returns, by the reference's loops."""
    file_off, person_base = np.asarray(file_off, dtype=np.int64), np.asarray(person_base, dtype=np.int64)
    valid, conf = np.asarray(valid).astype(bool), np.asarray(conf, dtype=np.float64)
    C, K = len(file_off) - 1, conf.shape[1]
    rows, row_off, n_people, series_off, series_frame, series_conf = [], [0], [], [0], [], [[] for _ in range(K)]
    for c in range(C):
        grouped, most = {}, 0
        for frame_idx, f in enumerate(range(file_off[c], file_off[c + 1])):
            most = max(most, int(person_base[f + 1] - person_base[f]))
            for person_idx, i in enumerate(range(person_base[f], person_base[f + 1])):
                if not valid[i]:
                    continue
                for k in range(K):
                    rows.append((frame_idx, person_idx, k, conf[i, k]))
                    grouped.setdefault((k, person_idx), ([], []))
                    grouped[(k, person_idx)][0].append(frame_idx)
                    grouped[(k, person_idx)][1].append(conf[i, k])
        row_off.append(len(rows))
        n_people.append(most)
        for p in range(most):                                         # every slot of a person has the same frames
            frames = grouped.get((0, p), ([], []))[0]
            series_frame += frames
            for k in range(K):
                series_conf[k] += grouped.get((k, p), ([], []))[1]
            series_off.append(series_off[-1] + len(frames))
    return {'row_off': np.array(row_off, dtype=np.int64), 'frame': np.array([r[0] for r in rows], dtype=np.int32),
            'person': np.array([r[1] for r in rows], dtype=np.int32), 'slot': np.array([r[2] for r in rows], dtype=np.int32),
            'confidence': np.array([r[3] for r in rows], dtype=np.float64), 'n_people': np.array(n_people, dtype=np.int64),
            'series_off': np.array(series_off, dtype=np.int64), 'series_frame': np.array(series_frame, dtype=np.int32),
            'series_conf': np.array(series_conf, dtype=np.float64).reshape(K, len(series_frame))}


def same(a, b):
    """Equal dtype, shape and bytes but for the payload of NaN: every integer exact, every double the copied one."""
    a, b = np.asarray(a), np.asarray(b)
    if a.dtype != b.dtype or a.shape != b.shape:
        return False
    if a.dtype.kind == 'f':
        nan = np.isnan(a)
        return bool(np.array_equal(nan, np.isnan(b)) and np.array_equal(a[~nan].view(np.int64), b[~nan].view(np.int64)))
    return bool(np.array_equal(a, b))


def assert_same(got, want, what=''):
    assert list(got) == list(OUTPUTS), list(got)
    for key in OUTPUTS:
        assert same(got[key], want[key]), (what, key)


class HostTimelineEngine:
    """Stands where an Engine goes: the library's host path (ctx == NULL), no GPU."""

    @staticmethod
    def timeline_rows(file_off, person_base, valid, conf):
        from pose2sim_amd.engine import timeline_rows_host
        return timeline_rows_host(file_off, person_base, valid, conf)


def seeded_case(n_files, most, K, seed, p_valid=0.6, p_empty=0.1):
    """Cameras of n_files[c] files whose lists hold up to most[c] entries (most[c] = 0: nobody listed), each valid with
    probability p_valid[c] (one value, or one a camera), a file empty with probability p_empty; confidences of three
    decimals with a few NaN, zeros and values whose repr needs 17 digits.  -> (file_off, person_base, valid, conf)."""
    rng = np.random.default_rng(seed)
    p_valid = np.broadcast_to(np.asarray(p_valid, dtype=np.float64), (len(n_files),))
    counts, valid = [], []
    for F, m, pv in zip(n_files, most, p_valid):
        n = rng.integers(0, m + 1, F) if m else np.zeros(F, dtype=np.int64)
        n[rng.random(F) < p_empty] = 0
        if F and m:
            n[rng.integers(0, F)] = m                                 # the camera's longest list is `most`
        counts.append(n)
        valid.append(rng.random(int(n.sum())) < pv)
    person_base = np.concatenate([[0], np.cumsum(np.concatenate(counts))]).astype(np.int64)
    valid = np.concatenate(valid)
    conf = np.round(rng.uniform(0.0, 1.0, (len(valid), K)), 3)
    special = rng.random(conf.shape)
    conf[special < 0.02] = np.nan
    conf[(special >= 0.02) & (special < 0.04)] = 0.0
    conf[(special >= 0.04) & (special < 0.06)] = 0.1 + 0.2
    file_off = np.concatenate([[0], np.cumsum(n_files)]).astype(np.int64)
    return file_off, person_base, valid, conf


def arrays_from_documents(texts, index):
    """The device's inputs for one folder from its files' texts in sorted order, read as the reference reads them: a text
    that does not decode holds nobody.  index: the resolved keypoints' indices.  -> (person_base, valid, conf)."""
    counts, valid, conf = [], [], []
    for text in texts:
        try:
            people = json.loads(text).get('people', [])
        except json.JSONDecodeError:
            people = []
        counts.append(len(people))
        for person in people:
            kps = person.get('pose_keypoints_2d', [])
            ok = len(kps) >= 3 * N_KEYPOINTS
            valid.append(ok)
            conf.append([float(kps[3 * k + 2]) for k in index] if ok else [0.0] * len(index))
    person_base = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
    return person_base, np.array(valid, dtype=bool), np.array(conf, dtype=np.float64).reshape(len(valid), len(index))


def csv_bytes(res, names):
    """The reference's CSV of the rows of `res`, by csv.writer itself."""
    out = io.StringIO(newline='')
    writer = csv.writer(out)
    writer.writerow(['frame', 'person', 'keypoint', 'confidence'])
    writer.writerows((int(f), int(p), names[s], float(v)) for f, p, s, v in zip(res['frame'], res['person'], res['slot'], res['confidence']))
    return out.getvalue().encode()
