"""Goldens of the synchronization stage, recorded from the reference -> sync_units.npz

synchronize_cams_all (synchronization.py:1346-1612) on synthetic trials (tests/sync_trials.py: one person jumping at
random times, planted frame shifts per camera), with display_sync_plots = save_sync_plots = false and MPLBACKEND=Agg.
time_lagged_cross_corr (:1291-1343) is wrapped to capture the two speed series of every call and its r list.  Per case:
the config (JSON, project_dir left out), the trial it runs on, the speeds of every camera, the r curves, the offsets and
correlations of the log, the sorted pose-sync/ listing of every camera, the log lines, and for the error cases the
exception's type and message.  The trials are stored as the arrays the tests write back to JSON files.
"""
import json
import logging
import os
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
os.environ.setdefault('MPLBACKEND', 'Agg')
import ref_shim  # noqa: E402
import sync_trials as st  # noqa: E402


def trials():
    from pose2sim_amd import skeletons
    ids, names, _ = skeletons.keypoints('HALPE_26')
    right = [i for i, n in zip(ids, names) if n.startswith('R')]          # JSON keypoint ids of the model's R* keypoints
    return {
        'A': st.make_trial(11, [600] * 4, [0, 7, -12, 25]),
        'B': st.make_trial(12, [200] * 3, [0, 5, -9], distractor=0.05,
                           kinds={st.KIND_EMPTY: 0.03, st.KIND_NO_LIST_PERSON: 0.04, st.KIND_TRUNCATED: 0.02, st.KIND_NO_PEOPLE: 0.01}),
        'C': st.make_trial(13, [240, 200, 220], [0, -6, 10]),
        'E': st.make_trial(14, [120] * 3, [0, 4, -3], low_lik_kpts=right, lik_range=(0.8, 1.0)),
    }


CASES = [
    ('auto_all', 'A', {}),
    ('times_clipped', 'A', {'approx_time_maxspeed': [1.0, 19.5, 0.5, 10.0], 'time_range_around_maxspeed': 3.0}),
    ('one_time', 'A', {'approx_time_maxspeed': [10.0], 'time_range_around_maxspeed': 4.0}),
    ('right', 'A', {'keypoints_to_consider': 'right'}),
    ('left', 'A', {'keypoints_to_consider': 'left'}),
    ('names', 'A', {'keypoints_to_consider': ['RWrist', 'LWrist', 'Nose', 'NotAKeypoint']}),
    ('multi_person', 'B', {}),
    ('ref_not_first', 'C', {}),
    ('short_unfiltered', 'A', {'approx_time_maxspeed': [10.0] * 4, 'time_range_around_maxspeed': 0.1}),
    ('all_r_nan', 'E', {'keypoints_to_consider': 'right', 'likelihood_threshold': 0.5}),
    ('fps_auto', 'A', {'project': {'frame_rate': 'auto'}, 'filter_cutoff': 5}),
    ('err_all_nan', 'E', {'likelihood_threshold': 1.0}),
    ('err_bad_time_keyword', 'A', {'approx_time_maxspeed': 'sometimes'}),
    ('err_bad_keypoints_keyword', 'A', {'keypoints_to_consider': 'middle'}),
    ('err_padlen', 'A', {'approx_time_maxspeed': [10.0] * 4, 'time_range_around_maxspeed': 0.14}),
    ('err_unfiltered_subset', 'A', {'approx_time_maxspeed': [10.0] * 4, 'time_range_around_maxspeed': 0.1,
                                    'keypoints_to_consider': 'right'}),
]


class _Lines(logging.Handler):
    def __init__(self):
        super().__init__()
        self.lines = []

    def emit(self, record):
        self.lines.append(record.getMessage())


def gen():
    ref_shim.install()
    import importlib
    sync = importlib.import_module('Pose2Sim.synchronization')
    out = {}
    all_trials = trials()
    for name, t in all_trials.items():
        for key, value in t.items():
            out[f'trial{name}_{key}'] = value
    root = logging.getLogger()
    root.setLevel(logging.INFO)
    orig = sync.time_lagged_cross_corr
    for n, (case, trial_name, overrides) in enumerate(CASES):
        calls = []

        def wrapped(camx, camy, lag_range, show=True, ref_cam_name='0', cam_name='1'):
            res = orig(camx, camy, lag_range, show=show, ref_cam_name=ref_cam_name, cam_name=cam_name)
            lr = [-lag_range, lag_range] if isinstance(lag_range, int) else lag_range
            r = [camx.corr(camy.shift(lag)) for lag in range(lr[0], lr[1])]
            calls.append((np.asarray(camx, dtype=np.float64), np.asarray(camy, dtype=np.float64), np.asarray(r), res[0], res[1]))
            return res
        sync.time_lagged_cross_corr = wrapped
        with tempfile.TemporaryDirectory(prefix='sync_') as tmp:
            trial_dir = os.path.join(tmp, 'trial')
            dirs = st.write_trial(all_trials[trial_name], os.path.join(trial_dir, 'pose'))
            cfg = st.sync_config(trial_dir, **json.loads(json.dumps(overrides)))
            h = _Lines()
            root.addHandler(h)
            err = None
            try:
                sync.synchronize_cams_all(cfg)
            except Exception as e:                                                   # noqa: BLE001
                err = e
            finally:
                root.removeHandler(h)
                sync.time_lagged_cross_corr = orig
            stored = dict(overrides)
            out[f'case{n}_name'] = np.array(case)
            out[f'case{n}_trial'] = np.array(trial_name)
            out[f'case{n}_config'] = np.array(json.dumps(stored))
            out[f'case{n}_logs'] = np.array(json.dumps([line.replace(tmp, '<TMP>') for line in h.lines]))
            if err is not None:
                out[f'case{n}_error'] = np.array([type(err).__name__, str(err)])
                print(case, type(err).__name__, str(err)[:80])
                continue
            sync_dir = os.path.join(trial_dir, 'pose-sync')
            out[f'case{n}_listing'] = np.array(json.dumps({d: sorted(os.listdir(os.path.join(sync_dir, d))) for d in dirs}))
            out[f'case{n}_n_calls'] = np.array(len(calls))
            for k, (camx, camy, r, off, corr) in enumerate(calls):
                if k == 0:
                    out[f'case{n}_speed_ref'] = camx
                out[f'case{n}_speed{k}'] = camy
                out[f'case{n}_r{k}'] = r
                out[f'case{n}_section{k}'] = np.array([off, corr], dtype=np.float64)
            print(case, [line for line in h.lines if line.startswith('-->')])
    out['n_cases'] = np.array(len(CASES))
    np.savez_compressed(os.path.join(HERE, 'sync_units.npz'), **out)
    print('sync_units.npz:', len(out), 'arrays', os.path.getsize(os.path.join(HERE, 'sync_units.npz')), 'bytes')


if __name__ == '__main__':
    gen()
