"""The stage list of tests/test_engine_reuse_gpu.py (a helper, not a test): every host entry point of include/p2s.h as a call on
an Engine, at two sizes.  STAGE_ENTRY names the entry point behind every stage; tests/test_engine_reuse_host.py holds it
against the header, so an entry point that is added without a stage here fails there, without a GPU.

A stage is (name, call(engine) -> tuple of arrays).  Its inputs are seeded and depend on the size alone.  A call that needs
another calibration or a tuning key sets it, runs, and puts the engine back as new_engine() made it: the calls of one engine
see nothing of each other but the staging slots and the work-list triangulation's buffers, which is what the test is about.
The shapes are the smallest that still cross the stage's own tile: 256 samples or frames for the scans, the gait runs, the
peak finder and the passes of refine / relpose, 1024 records for the sort, 32 frames for the selection's map scan."""
import contextlib
import functools

import numpy as np
from scipy import signal

import extract_numpy as en
import gaps_numpy as gn
import idswitch_numpy as isn
import refine_scipy as rs
import relpose_numpy as rn
import timeline_numpy as tln
import track_numpy as tn
from pose2sim_amd import _lib, measurements, skeletons, synth

C, K = 4, 26                       # the smoke() rig: 4 cameras, HALPE_26
SMALL, LARGE = (6, 64), (19, 190)  # (frames of the triangulation stages, frames of the column stages): ~3x forces every slot to grow
GAUSSIAN, KALMAN, HAMPEL, ONE_EURO, MEDIAN = 2, 5, 1, 4, 3      # include/p2s.h P2S_FILTER_*
PAST_TILE = 200                    # added to the column stages' frames where a tile of 256 has to be crossed at both sizes
PAST_SORT_TILE = 1025              # one record more than a workgroup sorts in LDS (test_measure_gpu.py)
MARKERS = ['Nose', 'LEye', 'REye', 'LEar', 'REar', 'LShoulder', 'RShoulder', 'LElbow', 'RElbow', 'LWrist', 'RWrist', 'LHip', 'RHip',
           'LKnee', 'RKnee', 'LAnkle', 'RAnkle', 'Head', 'Neck', 'Hip', 'LBigToe', 'RBigToe', 'LSmallToe', 'RSmallToe', 'LHeel', 'RHeel']

# stage -> the entry point of include/p2s.h it drives
STAGE_ENTRY = {
    'triangulate': 'p2s_triangulate_host', 'triangulate_swap': 'p2s_triangulate_host', 'triangulate_f64': 'p2s_triangulate_host',
    'triangulate_noscreen': 'p2s_triangulate_host', 'triangulate_deep': 'p2s_triangulate_host',
    **{f'triangulate_{path}{v}': 'p2s_triangulate_host' for path in ('worklist', 'onetile', 'twotiles', 'pooled') for v in ('', '_swap_undistort')},
    'associate': 'p2s_associate_host', 'associate_general': 'p2s_associate_host', 'associate_single': 'p2s_associate_single_host',
    'butterworth': 'p2s_butterworth_host',
    **{f'filter_{k}': 'p2s_filter_columns_host' for k in ('gaussian', 'kalman', 'hampel', 'one_euro', 'median')},
    'gcv_spline': 'p2s_gcv_spline_host', 'loess': 'p2s_loess_host', 'trc_metrics': 'p2s_trc_metrics_host',
    'sync_speeds': 'p2s_sync_speeds_host', 'lagged_pearson': 'p2s_lagged_pearson_host',
    'reproject_pinhole': 'p2s_reproject_host', 'reproject_distorted': 'p2s_reproject_host',
    'column_order_stats': 'p2s_column_order_stats_host', 'jitter': 'p2s_jitter_host', 'confidence_stats': 'p2s_confidence_stats_host',
    'column_mean_std': 'p2s_column_mean_std_host', 'lsap': 'p2s_lsap_host', 'id_switch': 'p2s_id_switch_host',
    'find_peaks': 'p2s_find_peaks_host', 'find_peaks_bounds': 'p2s_find_peaks_host',
    'gait_height': 'p2s_gait_contacts_host', 'gait_velocity': 'p2s_gait_contacts_host',
    'stable_argsort': 'p2s_stable_argsort_host', 'trimmed_means': 'p2s_trimmed_means_host', 'body_measure': 'p2s_body_measure_host',
    'track_select': 'p2s_track_select_host',
    'track_persons_batch': 'p2s_track_persons_host', 'track_persons_continued': 'p2s_track_persons_host', 'track_persons_overflow': 'p2s_track_persons_host',
    **{f'interpolate_gaps_{k}': 'p2s_interpolate_gaps' for k in ('linear', 'slinear', 'quadratic', 'cubic')},
    **{f'interpolate_gaps_{k}_chunked': 'p2s_interpolate_gaps' for k in ('slinear', 'quadratic', 'cubic')},
    'fill_gaps_last_value': 'p2s_fill_gaps', 'fill_gaps_zeros': 'p2s_fill_gaps', 'gap_runs': 'p2s_gap_runs', 'gap_runs_overflow': 'p2s_gap_runs',
    'timeline_rows': 'p2s_timeline_rows_host', 'refine_extrinsics': 'p2s_refine_extrinsics_host', 'relative_poses': 'p2s_relative_poses_host',
}


def default_calibration(eng):
    cams = synth.make_cameras(C, seed=7)
    eng.set_calibration(synth.projection_matrices(cams), cams)


def new_engine():
    from pose2sim_amd.engine import Engine
    eng = Engine(0)
    default_calibration(eng)
    return eng


def _tuning_defaults():
    from pose2sim_amd.engine import Engine
    return {Engine.TUNE_TRI_PATH: Engine.TRI_PATH_AUTO, Engine.TUNE_SCREEN: 1, Engine.TUNE_DEEP_MIN_SUBSETS: 4096,
            Engine.TUNE_ASSOC_FORM: Engine.ASSOC_FORM_AUTO, Engine.TUNE_GAPS_WORKSPACE_KB: 256 * 1024}


@contextlib.contextmanager
def tuned(eng, tuning, calibration=None):
    """The engine with these tuning keys (and this (P, cams) calibration) set; as new_engine() made it afterwards."""
    defaults = _tuning_defaults()
    try:
        for key, value in tuning.items():
            eng.set_tuning(key, value)
        if calibration is not None:
            eng.set_calibration(*calibration)
        yield eng
    finally:
        for key in tuning:
            eng.set_tuning(key, defaults[key])
        if calibration is not None:
            default_calibration(eng)


def flat(out):
    """Whatever an Engine method returns -- arrays, scalars, lists, tuples and dicts of them -- as one tuple of arrays, dicts in
    key order."""
    if isinstance(out, dict):
        return tuple(a for key in sorted(out) for a in flat(out[key]))
    if isinstance(out, (list, tuple)):
        return tuple(a for item in out for a in flat(item))
    return (np.asarray(out),)


def _standing_table(n, rng):
    """[n][78]: a person who sways on the spot, frames below and above close_to_zero_speed, a few NaN markers
    (test_measure_gpu.py's long table)."""
    stand = {'Hip': (0, 0.92, 0), 'Hip_': (0, 0.92, 0.1), 'Knee_': (0.02, 0.5, 0.1), 'Ankle_': (0, 0.08, 0.1), 'Heel_': (-0.05, 0.02, 0.1),
             'BigToe_': (0.16, 0.01, 0.1), 'SmallToe_': (0.13, 0.01, 0.14), 'Neck': (0.02, 1.44, 0), 'Shoulder_': (0.02, 1.42, 0.18),
             'Elbow_': (0.02, 1.12, 0.2), 'Wrist_': (0.05, 0.86, 0.2), 'Head': (0.02, 1.7, 0), 'Nose': (0.12, 1.59, 0), 'Eye_': (0.1, 1.63, 0.03),
             'Ear_': (0.03, 1.61, 0.07)}
    rest = np.array([stand[m] if m in stand else np.array(stand[m[1:] + '_']) * (1, 1, 1 if m[0] == 'R' else -1) for m in MARKERS]).reshape(1, 78)
    sigma = 0.004 * (0.6 + 0.8 * rng.random((n, 1)))
    table = np.round(rest + 0.02 * np.cumsum(rng.normal(0, 1, (n, 78)), axis=0) / np.sqrt(np.arange(1, n + 1))[:, None]
                     + sigma * rng.normal(0, 1, (n, 78)), 3)
    table[rng.random((n, 26)).repeat(3, axis=1) < 0.01] = np.nan
    return table


@functools.lru_cache(maxsize=None)
def stages(size):
    """-> [(name, call(engine) -> tuple of arrays)] for one size; the inputs depend on the size alone, are built once and
    are never written to."""
    Ft, Fc = size
    rng = np.random.default_rng(Fc)
    ids, names, swap = skeletons.keypoints('HALPE_26')
    from pose2sim_amd.engine import Engine
    wl = synth.make_config(Ft, C, K, 2, seed=7, p_lowlik=0.1, p_outlier=0.08)
    xyl = wl['xyl']                                                    # [Ft][2][C][K][3]
    n_persons = np.full((Ft, C), 2, dtype=np.int32)
    n_persons[0, 1] = 1                                                # ragged: one detection fewer in one camera
    kpts = np.concatenate([xyl[f, :n_persons[f, c], c] for f in range(Ft) for c in range(C)])   # camera-major, then person
    col = synth.make_config(Fc, C, K, 1, seed=11, p_missing_cam=0.0)
    Q = col['Q3d'][:, 0]                                               # [Fc][K][3]
    clean = Q[:, :2].reshape(Fc, 6) + rng.normal(0, 0.01, (Fc, 6))
    gapped = clean.copy()
    gapped[10:13, 2] = np.nan                                          # runs of 10 and Fc - 13 samples in one column
    gapped[:7, 4] = 0.0                                                # zeros are missing samples too
    b, a = signal.butter(2, 6 / 30, 'low')                             # 4th order zero-phase at 60 fps, as filtering.py
    zi = signal.lfilter_zi(b, a)
    weights = np.exp(-0.5 * (np.arange(-4, 5) / 1.5) ** 2)
    weights /= weights.sum()
    coords = [col['xyl'][:Fc - 3 * c, 0, c, :3, :2].reshape(-1, 6).astype(np.float64) for c in range(3)]
    for c in coords:
        c[rng.random(c.shape) < 0.05] = np.nan
    speeds = [np.abs(rng.normal(0, 1, n)) for n in (Fc, Fc - 5, Fc + 4)]
    speeds[1][3] = np.nan
    sizes = np.array(col['cams']['S'])
    dcams = synth.make_cameras(C, seed=7, distort=True)
    Qn = Q.copy()
    Qn[2, 5] = np.nan
    stats_in = clean.copy()
    stats_in[rng.random(clean.shape) < 0.1] = np.nan
    series = [col['xyl'][:Fc - 2 * c, 0, c].astype(np.float64) for c in range(2)]     # [frames][26][3]
    conf_tables = [rng.uniform(0.0, 1.0, (n, K)) for n in (Fc, Fc - 7)]
    for t in conf_tables:
        t[rng.random(len(t)) < 0.1] = np.nan                           # frames without a person
    costs = rng.uniform(0.0, 100.0, (Fc, 7, 5))
    crowds = [isn.seeded_camera(Fc, 9000 + c, max_persons=9) for c in range(2)]
    prm = Engine.tri_params(15.0, 0.3, 2)
    prm_swap = Engine.tri_params(15.0, 0.3, 2, lr_swap=True)

    # -- triangulation on every path: plain, and with L/R swap and undistortion on a distorted rig --------------------------
    wlu = synth.make_config(Ft, C, K, 2, seed=7, undistort=True, lr_swap=True, swap_idx=swap, p_lowlik=0.1, p_outlier=0.08)
    prm_su = Engine.tri_params(15.0, 0.3, 2, undistort=True, lr_swap=True)
    x64 = xyl.astype(np.float64) + 1e-9                                # no longer float32 numbers: the float64 kernels
    wl8 = synth.make_config(Ft, 8, K, 2, seed=308, undistort=True, lr_swap=True, swap_idx=swap, p_outlier=0.25, p_lowlik=0.05, p_missing_cam=0.02)
    prm8 = Engine.tri_params(8.0, 0.3, 2, undistort=True, lr_swap=True)

    def tri(tuning, x=xyl, params=prm, swap_idx=None, calibration=None):
        def call(e):
            with tuned(e, tuning, calibration):
                return e.triangulate(x, params, swap_idx=swap_idx)
        return call

    def tri_deep(e):
        # 8 cameras, the deep threshold at 10 subsets: every level from the second on goes through deep_entries / ctl / sched /
        # partials (test_deep_levels_spread_over_the_gpu)
        with tuned(e, {Engine.TUNE_TRI_PATH: Engine.TRI_PATH_WORKLIST, Engine.TUNE_DEEP_MIN_SUBSETS: 10}, (wl8['P'], wl8['cams'])):
            out = e.triangulate(wl8['xyl'], prm8, swap_idx=swap)
        assert (out[2].reshape(-1) - np.isnan(wl8['xyl'][..., 2]).sum(axis=2).reshape(-1) >= 2).any()     # some unit went past level 1
        return out

    paths = {'worklist': Engine.TRI_PATH_WORKLIST, 'onetile': Engine.TRI_PATH_ONE_TILE, 'twotiles': Engine.TRI_PATH_TWO_TILES,
             'pooled': Engine.TRI_PATH_POOLED}
    tri_stages = []
    for name, path in paths.items():
        tri_stages.append((f'triangulate_{name}', tri({Engine.TUNE_TRI_PATH: path})))
        tri_stages.append((f'triangulate_{name}_swap_undistort', tri({Engine.TUNE_TRI_PATH: path}, wlu['xyl'], prm_su, swap, (wlu['P'], wlu['cams']))))

    def associate_general(e):
        with tuned(e, {Engine.TUNE_ASSOC_FORM: Engine.ASSOC_FORM_GENERAL}):
            return (e.associate(n_persons, kpts, e.assoc_params(0.1, 0.2, 2)),)

    # -- the stages merged since the list was first written ----------------------------------------------------------------
    noisy = np.round(np.cumsum(rng.normal(0, 1, (Fc, 6)), axis=0), 1)  # a peak about every third sample: more than find_peaks' first capacity
    noisy[5:9, 1] = noisy[5, 1]                                        # a plateau
    bounds = np.where(np.arange(6) % 2 == 0, 0.0, 1.5)
    gait_lens = (Fc, Fc - 7, 2 * Fc + 141)                             # unequal, the longest past one round of 256 samples
    toes = [0.03 + 0.1 * np.sin(2 * np.pi * np.arange(n) / 66.0 + s) ** 2 + rng.normal(0, 0.003, n) for s, n in enumerate(gait_lens)]
    walks = [np.cumsum(np.abs(t)) * (1 + s) for s, t in enumerate(toes)]
    walks[1][::7] -= 0.3                                               # steps against the direction: zeroed
    walks[2][20] = np.nan
    sort_columns = [np.where(rng.random(n) < 0.2, np.nan, np.round(rng.normal(0, 1, n), 1)) for n in (Fc, 1, PAST_SORT_TILE + Fc)]
    trim_columns = [np.round(rng.normal(1.7, 0.05, n), 3) for n in (Fc, 1, PAST_SORT_TILE + Fc)]
    tables = [_standing_table(n, rng) for n in (PAST_SORT_TILE + Fc, Fc)]
    roles = [MARKERS.index(m) for m in _lib.P2S_MEASURE_ROLES]
    pairs = [(MARKERS.index(p), MARKERS.index(q)) for p, q in measurements.HEIGHT_PAIRS] + [(K, MARKERS.index('Head')), (K + 1, MARKERS.index('Nose'))]
    every = _lib.P2S_MEASURE_SPEED | _lib.P2S_MEASURE_ANGLES | _lib.P2S_MEASURE_RESTRICT | _lib.P2S_MEASURE_HEIGHT | _lib.P2S_MEASURE_LEG
    measure_flags = [every, every & ~_lib.P2S_MEASURE_RESTRICT]
    select_cams = [en.crowd_camera(Fc + PAST_TILE, 40, single_at=(3, 40), empty=(0, 17, 18)), en.crowd_camera(Fc - 9, 41, n_persons=3)]
    trial = tn.make_trial(Fc, 3, 26, 0.02, seed=Fc)
    batch = [trial, trial[:1], trial[:Fc // 3]]                        # unequal lengths, one of a single frame
    over = tn.make_trial(*tn.OVERFLOW[:3], tn.OVERFLOW[4], seed=1)     # passes 32 slots (track_cases.check_overflow)
    gaps_F = Fc + PAST_TILE
    gapped_cols, labels = gn.make_case(gaps_F, 6)                      # with the column of 4 good samples, the all-NaN one, the one with +inf
    filled = gapped_cols.copy()
    filled[gaps_F // 2, 0], filled[gaps_F - 1, 5] = np.inf, -np.inf
    timeline = tln.seeded_case((Fc + PAST_TILE, 5, Fc), (3, 0, 2), K, seed=Fc)
    refine = rs.make_case('ring', C=3, F=17 * Fc // 64, Kp=16, seed=Fc)                 # 17 frames of 16: one frame more than P2S_REFINE_TILE points
    walk = rn.walk_case('ring', C=3, F=65 if size == SMALL else 257, Kp=1, seed=Fc)     # one point past a wave, one past P2S_RELPOSE_TILE
    relpose = rn.inputs(walk, H=65, m=8, seed=Fc)

    def gait_height(e):
        return flat(e.gait_contacts(toes, 'height_coordinates', dt=1 / 60, threshold=[6.0, 4.0, 8.0], factor=100.0, b=b, a=a, zi=zi))

    def gait_velocity(e):
        return flat(e.gait_contacts(walks, 'forward_velocity', dt=[1 / 60, 1 / 50, 1 / 100], threshold=[1.0, 5.0, 20.0], sign=1, weights=weights))

    def track_continued(e):
        cut = Fc // 2
        first = e.track_persons_3d(trial[:cut], first_frame=0, max_dist=1.0)
        return flat(first) + flat(e.track_persons_3d(trial[cut:], first_frame=cut, max_dist=1.0, state=first[4]))

    def track_overflow(e):
        out = e.track_persons_3d([over, over[:10]], first_frame=0, max_dist=tn.OVERFLOW[3])
        assert out[5][0][0] > 0 and not out[5][1].any()               # the first trial stops, the one beside it is whole
        return flat(out)

    def gaps(kind, workspace_kb=None):
        def call(e):
            with tuned(e, {} if workspace_kb is None else {Engine.TUNE_GAPS_WORKSPACE_KB: workspace_kb}):
                return e.interpolate_gaps(gapped_cols, labels, 20, kind)
        return call

    def gap_runs(capacity):
        def call(e):
            table, count, overflow = e.gap_runs(filled, 1, gaps_F - 2, 20, capacity=capacity, raw=True)
            assert overflow == (capacity is not None)
            return flat((table, count, overflow))
        return call

    return [
        ('triangulate', lambda e: e.triangulate(xyl, prm)),
        ('triangulate_swap', lambda e: e.triangulate(xyl, prm_swap, swap_idx=swap)),
        *tri_stages,
        ('triangulate_noscreen', tri({Engine.TUNE_SCREEN: 0})),
        ('triangulate_f64', lambda e: e.triangulate(x64, prm)),
        ('triangulate_deep', tri_deep),
        ('associate', lambda e: (e.associate(n_persons, kpts, e.assoc_params(0.1, 0.2, 2)),)),
        ('associate_general', associate_general),
        ('associate_single', lambda e: e.associate_single(n_persons, kpts[:, 0], 15.0, 0.3, 2)),
        ('butterworth', lambda e: (e.butterworth(gapped, b, a, zi),)),
        ('filter_gaussian', lambda e: (e.filter_columns(GAUSSIAN, clean, weights),)),
        ('filter_kalman', lambda e: (e.filter_columns(KALMAN, clean, [1 / 60, 0.01, 5.0, 1.0]),)),
        ('filter_hampel', lambda e: (e.filter_columns(HAMPEL, clean, [2.0]),)),
        ('filter_one_euro', lambda e: (e.filter_columns(ONE_EURO, clean, [1 / 60, 1.0, 0.007, 1.0]),)),
        ('filter_median', lambda e: (e.filter_columns(MEDIAN, clean, [5]),)),
        ('gcv_spline', lambda e: e.gcv_spline(gapped, 'auto', 1.0, 60)),
        ('loess', lambda e: (e.loess(gapped, 9),)),
        ('trc_metrics', lambda e: e.trc_metrics(Qn, [[0, 1], [1, 2], [5, 20]])),
        ('sync_speeds', lambda e: tuple(e.sync_speeds(coords, b, a, zi))),
        ('lagged_pearson', lambda e: e.lagged_pearson(speeds[0], speeds[1:], -10, 11)),
        ('reproject_pinhole', lambda e: e.reproject(Qn, P=np.array(col['P']), sizes=sizes, raw=True)),
        ('reproject_distorted', lambda e: e.reproject(Qn, cal=dcams, sizes=sizes, raw=True)),
        ('column_order_stats', lambda e: e.column_order_stats(stats_in, [0, -1, Fc // 2, Fc])),
        ('jitter', lambda e: flat(e.jitter(series, multiplier=2.0))),
        ('confidence_stats', lambda e: flat(e.confidence_stats(conf_tables, (0.4, 0.6)))),
        ('column_mean_std', lambda e: e.column_mean_std(stats_in)),
        ('lsap', lambda e: e.lsap(costs)),
        ('id_switch', lambda e: flat(e.id_switch(crowds))),
        ('find_peaks', lambda e: flat(e.find_peaks(noisy))),
        ('find_peaks_bounds', lambda e: flat(e.find_peaks(noisy, prominence=bounds))),
        ('gait_height', gait_height),
        ('gait_velocity', gait_velocity),
        ('stable_argsort', lambda e: flat(e.stable_argsort(sort_columns))),
        ('trimmed_means', lambda e: (e.trimmed_means(trim_columns, 0.5),)),
        ('body_measure', lambda e: flat(e.body_measure(tables, [roles, roles], [pairs, pairs], measure_flags, fastest_frames_to_remove_percent=0.1,
                                                       large_hip_knee_angles=20, row_values=True))),
        ('track_select', lambda e: flat(e.track_select(select_cams))),
        ('track_persons_batch', lambda e: flat(e.track_persons_3d(batch, first_frame=[0, 5, 0], max_dist=1.0))),
        ('track_persons_continued', track_continued),
        ('track_persons_overflow', track_overflow),
        *[(f'interpolate_gaps_{kind}', gaps(kind)) for kind in ('linear', 'slinear', 'quadratic', 'cubic')],
        *[(f'interpolate_gaps_{kind}_chunked', gaps(kind, 32)) for kind in ('slinear', 'quadratic', 'cubic')],   # 32 KiB: two columns at a time, or one
        ('fill_gaps_last_value', lambda e: (e.fill_gaps(filled, 'last_value'),)),
        ('fill_gaps_zeros', lambda e: (e.fill_gaps(filled, 'zeros'),)),
        ('gap_runs', gap_runs(None)),
        ('gap_runs_overflow', gap_runs(3)),
        ('timeline_rows', lambda e: flat(e.timeline_rows(*timeline))),
        ('refine_extrinsics', lambda e: flat(e.refine_extrinsics(refine['xyl'], refine['K'], refine['R0'], refine['t0'], refine['X0'], lik_thr=refine['lik_thr']))),
        ('relative_poses', lambda e: flat(e.relative_poses(*relpose, all_hypotheses=True))),
    ]
