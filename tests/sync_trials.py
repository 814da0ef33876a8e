"""Synthetic trials of unsynchronised cameras for the synchronization stage: one person whose vertical position jumps at
random times (not periodic, so that the best lag is unambiguous), seen by every camera with a planted frame shift, as
OpenPose JSON files.  Shared by tests/golden/make_golden_sync.py (which records the reference on them) and the tests
(which write the recorded arrays back to files).

A trial is a dict of arrays:
  xy   int16 [C][F][P][K][2]  coordinates in tenths of a pixel        lik  uint8 [C][F][P][K]  likelihood in hundredths
  n_frames int [C]            files per camera (<= F)                 n_persons uint8 [C][F]
  kind int8 [C][F]            0 normal, 1 empty "people", 2 a first person without "pose_keypoints_2d",
                              3 the main person's list truncated to `trunc` values, 4 no "people" key
"""
import json
import os

import numpy as np

from pose2sim_amd import poseio

KIND_NORMAL, KIND_EMPTY, KIND_NO_LIST_PERSON, KIND_TRUNCATED, KIND_NO_PEOPLE = 0, 1, 2, 3, 4


def world_motion(rng, n_t):
    """(x, y) of the person's centre over n_t world frames: a slow horizontal drift and vertical jumps at random times."""
    t = np.arange(n_t, dtype=np.float64)
    y = np.full(n_t, 600.0)
    t0 = 10.0
    while t0 < n_t:
        w = rng.uniform(4, 12)
        y -= rng.uniform(40, 160) * np.exp(-0.5 * ((t - t0) / w) ** 2)
        t0 += rng.uniform(25, 90)
    x = 900.0 + np.cumsum(rng.normal(0, 1.5, n_t))
    return x, y


def make_trial(seed, n_frames, shifts, n_kpts=26, distractor=0.0, kinds=None, low_lik_kpts=(), lik_range=(0.5, 1.0)):
    """Camera c's file f shows world frame f + margin + shifts[c]; kinds: {kind: probability} of the special files;
    low_lik_kpts: JSON keypoint ids whose likelihood is 0.3 throughout."""
    rng = np.random.default_rng(seed)
    C, F = len(shifts), int(max(n_frames))
    margin = int(max(abs(s) for s in shifts)) + 5
    wx, wy = world_motion(rng, F + 2 * margin)
    body = np.stack([rng.uniform(-60, 60, n_kpts), rng.uniform(-180, 180, n_kpts)], axis=1)
    P = 2 if distractor else 1
    xy = np.zeros((C, F, P, n_kpts, 2))
    lik = np.zeros((C, F, P, n_kpts))
    for c, s in enumerate(shifts):
        gain, dx, dy = rng.uniform(0.7, 1.3), rng.uniform(-200, 200), rng.uniform(-100, 100)
        t = np.arange(F) + margin + s
        xy[c, :, 0, :, 0] = gain * (wx[t][:, None] + body[None, :, 0]) + dx
        xy[c, :, 0, :, 1] = gain * (wy[t][:, None] + body[None, :, 1]) + dy
        xy[c, :, 0] += rng.normal(0, 0.6, (F, n_kpts, 2))
        lik[c, :, 0] = rng.uniform(*lik_range, (F, n_kpts))
        low = rng.random((F, n_kpts)) < 0.03
        lik[c, :, 0][low] = 0.1
        undetected = rng.random((F, n_kpts)) < 0.01
        xy[c, :, 0][undetected] = 0.0
        lik[c, :, 0][undetected] = 0.0
        for k in low_lik_kpts:
            lik[c, :, 0, k] = 0.3
        if P == 2:                                   # a second person, larger than the main one in some files
            big = rng.random(F) < distractor
            xy[c, :, 1] = rng.uniform(100, 300, (F, 1, 2)) + rng.uniform(0, 150, (F, n_kpts, 2))
            xy[c, big, 1] = rng.uniform(0, 60, (int(big.sum()), 1, 2)) + rng.uniform(0, 900, (int(big.sum()), n_kpts, 2))
            lik[c, :, 1] = rng.uniform(0.5, 1.0, (F, n_kpts))
    n_persons = np.full((C, F), P, dtype=np.uint8)
    kind = np.zeros((C, F), dtype=np.int8)
    for k, p in (kinds or {}).items():
        kind[(rng.random((C, F)) < p) & (kind == 0)] = k
    return {'xy': np.round(xy * 10).astype(np.int16), 'lik': np.round(lik * 100).astype(np.uint8),
            'n_frames': np.asarray(n_frames, dtype=np.int64), 'n_persons': n_persons, 'kind': kind,
            'trunc': np.array(3 * n_kpts - 4)}


def person_arrays(trial, c, f):
    """The (x, y, likelihood) [K][3] arrays of the persons of camera c's file f, as written."""
    xy = trial['xy'][c, f].astype(np.float64) / 10
    lik = trial['lik'][c, f].astype(np.float64) / 100
    return [np.concatenate([xy[p], lik[p][:, None]], axis=1) for p in range(int(trial['n_persons'][c, f]))]


def write_trial(trial, pose_dir):
    """pose_dir/camXX_json/camXX_FFFFFF.json for every camera and file; -> the camera directory names."""
    dirs = []
    for c in range(len(trial['n_frames'])):
        name = f'cam{c + 1:02d}_json'
        os.makedirs(os.path.join(pose_dir, name), exist_ok=True)
        dirs.append(name)
        for f in range(int(trial['n_frames'][c])):
            path = os.path.join(pose_dir, name, f'cam{c + 1:02d}_{f:06d}.json')
            kind = int(trial['kind'][c, f])
            people = person_arrays(trial, c, f)
            if kind == KIND_EMPTY:
                poseio.write_openpose_json(path, [])
            elif kind == KIND_NO_PEOPLE:
                with open(path, 'w') as fh:
                    json.dump({'version': 1.3}, fh)
            else:
                if kind == KIND_TRUNCATED:
                    people[0] = people[0].ravel()[:int(trial['trunc'])]
                poseio.write_openpose_json(path, people)
                if kind == KIND_NO_LIST_PERSON:
                    with open(path) as fh:
                        doc = json.load(fh)
                    doc['people'].insert(0, {'person_id': [-1]})
                    with open(path, 'w') as fh:
                        json.dump(doc, fh)
    return dirs


def sync_config(project_dir, **sync):
    cfg = {'project': {'project_dir': project_dir, 'frame_rate': 30, 'frame_range': 'auto'},
           'pose': {'pose_model': 'HALPE_26', 'vid_img_extension': 'mp4'},
           'synchronization': {'synchronization_gui': False, 'display_sync_plots': False, 'save_sync_plots': False,
                               'keypoints_to_consider': 'all', 'approx_time_maxspeed': 'auto',
                               'time_range_around_maxspeed': 2.0, 'likelihood_threshold': 0.4, 'filter_cutoff': 6,
                               'filter_order': 4}}
    project = sync.pop('project', {})
    cfg['project'].update(project)
    cfg['synchronization'].update(sync)
    return cfg
