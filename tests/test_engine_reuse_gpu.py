"""One Engine driven through every host entry point, at changing sizes and in changing order.

The host calls take their device buffers from the context's staging slots: the i-th buffer a call asks for is slot i,
whatever stage asked for it last and however large it was then.  What can go wrong there -- two operands of one call in
one slot, a slot that did not grow, a result read from the stale tail of a larger earlier call -- shows only when
different stages and sizes share a context.  So every result of the shared engine must equal, bit for bit and NaN for NaN,
the result of the identical call on a fresh Engine that has run nothing else.
"""
import numpy as np
import pytest
from scipy import signal

import idswitch_numpy as isn
from pose2sim_amd import skeletons, synth

pytestmark = pytest.mark.gpu

C, K = 4, 26                       # the smoke() rig: 4 cameras, HALPE_26
SMALL, LARGE = (6, 64), (19, 190)  # (frames of the triangulation stages, frames of the column stages): ~3x forces every slot to grow
GAUSSIAN, KALMAN, HAMPEL, ONE_EURO = 2, 5, 1, 4      # include/p2s.h P2S_FILTER_*


def new_engine():
    from pose2sim_amd.engine import Engine
    eng = Engine(0)
    cams = synth.make_cameras(C, seed=7)
    eng.set_calibration(synth.projection_matrices(cams), cams)
    return eng


def stages(size):
    """-> [(name, call(engine) -> tuple of arrays)] for one size; the inputs depend on the size alone."""
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

    def jitter(e):
        out = e.jitter(series, multiplier=2.0)
        return tuple(np.asarray(v) for k in sorted(out) for v in (out[k] if isinstance(out[k], list) else [out[k]]))

    def confidence_stats(e):
        out = e.confidence_stats(conf_tables, (0.4, 0.6))
        return tuple(out[k] for k in ('stats', 'counts', 'below', 'below_rate', 'bands', 'band_rate'))

    def id_switch(e):
        out = e.id_switch(crowds)
        return tuple(np.asarray(v) for k in isn.TABLES + ('distances', 'kept') for v in out[k]) + (out['stats'],)

    return [
        ('triangulate', lambda e: e.triangulate(xyl, prm)),
        ('triangulate_swap', lambda e: e.triangulate(xyl, prm_swap, swap_idx=swap)),
        ('associate', lambda e: (e.associate(n_persons, kpts, e.assoc_params(0.1, 0.2, 2)),)),
        ('associate_single', lambda e: e.associate_single(n_persons, kpts[:, 0], 15.0, 0.3, 2)),
        ('butterworth', lambda e: (e.butterworth(gapped, b, a, zi),)),
        ('filter_gaussian', lambda e: (e.filter_columns(GAUSSIAN, clean, weights),)),
        ('filter_kalman', lambda e: (e.filter_columns(KALMAN, clean, [1 / 60, 0.01, 5.0, 1.0]),)),
        ('filter_hampel', lambda e: (e.filter_columns(HAMPEL, clean, [2.0]),)),
        ('filter_one_euro', lambda e: (e.filter_columns(ONE_EURO, clean, [1 / 60, 1.0, 0.007, 1.0]),)),
        ('gcv_spline', lambda e: e.gcv_spline(gapped, 'auto', 1.0, 60)),
        ('trc_metrics', lambda e: e.trc_metrics(Qn, [[0, 1], [1, 2], [5, 20]])),
        ('sync_speeds', lambda e: tuple(e.sync_speeds(coords, b, a, zi))),
        ('lagged_pearson', lambda e: e.lagged_pearson(speeds[0], speeds[1:], -10, 11)),
        ('reproject_pinhole', lambda e: e.reproject(Qn, P=np.array(col['P']), sizes=sizes, raw=True)),
        ('reproject_distorted', lambda e: e.reproject(Qn, cal=dcams, sizes=sizes, raw=True)),
        ('column_order_stats', lambda e: e.column_order_stats(stats_in, [0, -1, Fc // 2, Fc])),
        ('jitter', jitter),
        ('confidence_stats', confidence_stats),
        ('column_mean_std', lambda e: e.column_mean_std(stats_in)),
        ('lsap', lambda e: e.lsap(costs)),
        ('id_switch', id_switch),
    ]


def same(got, want):
    return len(got) == len(want) and all(g.dtype == w.dtype and g.shape == w.shape and np.array_equal(g, w, equal_nan=g.dtype.kind == 'f')
                                         for g, w in zip(got, want))


@pytest.fixture(scope='module')
def fresh():
    """{(size, name): (first, second)}: every call on an Engine of its own that has run nothing else, and once more on it."""
    out = {}
    for size in (SMALL, LARGE):
        for name, call in stages(size):
            eng = new_engine()
            out[size, name] = (tuple(call(eng)), tuple(call(eng)))
            eng.close()
    return out


def test_every_stage_repeats_itself_on_a_fresh_engine(fresh):
    """The premise of the comparison below: the same call twice on a fresh engine gives the same bits."""
    differing = [key for key, (first, second) in fresh.items() if not same(first, second)]
    assert differing == []


def test_one_engine_through_every_stage_and_size(fresh):
    """Small shapes, the same calls at three times the frames (every slot grows), the small shapes again in reverse
    order (every slot now holds the stale tail of a larger call of another stage)."""
    eng = new_engine()
    differing = []
    for rnd, (size, order) in enumerate(((SMALL, 1), (LARGE, 1), (SMALL, -1))):
        for name, call in stages(size)[::order]:
            if not same(tuple(call(eng)), fresh[size, name][0]):
                differing.append((rnd, name))
    eng.close()
    assert differing == []
