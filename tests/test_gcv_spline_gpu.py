"""p2s_gcv_spline_kernel on the MI355X, through the C-ABI (Engine.gcv_spline): against the reference's goldens
(tests/golden/gcv_units.npz) and against SciPy's make_smoothing_spline on seeded inputs (tests/gcv_scipy.py).

Parity bars, from the reference's own sensitivity (perturbing every input sample by one ulp moves its output by up to
7.9e-8 with cut-off 'auto' and 2.4e-15 with a fixed cut-off):
  fixed cut-off  |out - ref| <= 1e-9 max(1, |ref|)
  'auto'         |out - ref| <= 1e-6 max(1, |ref|); |lam - lam_ref| <= 1e-4 max(1, lam_ref), except on a run that lies
                 on a straight line (a constant run or a ramp: the penalty's null space, where every lambda fits
                 exactly and GCV is rounding noise -- moving every sample one ulp at random moves the reference's own
                 lambda from 36 to 45-74 on a ramp); there lambda must lie in the search interval (0, n] x
                 smoothing_factor and the output within the bar like any other
and everywhere the same NaN pattern, and the samples outside the filtered runs bit for bit."""
import os

import numpy as np
import pytest

from gcv_scipy import gcv_spline_columns, runs

pytestmark = pytest.mark.gpu

BAR_FIXED, BAR_AUTO, BAR_LAM = 1e-9, 1e-6, 1e-4


@pytest.fixture(scope='module')
def engine():
    from pose2sim_amd.engine import Engine
    return Engine(0)


@pytest.fixture(scope='module')
def gold(golden_dir):
    return np.load(os.path.join(golden_dir, 'gcv_units.npz'))


def _text(gold, key):
    """A .trc text of the goldens (stored as its UTF-8 bytes)."""
    return gold[key].tobytes().decode('utf-8')


def _filtered_mask(data):
    m = np.zeros(data.shape, dtype=bool)
    for c in range(data.shape[1]):
        for seq in runs(data[:, c]):
            if len(seq) >= 5:
                m[seq, c] = True
    return m


def _check(data, got, ref, bar, what):
    """NaN pattern, untouched samples bit for bit, filtered ones within bar; returns the worst relative deviation."""
    assert np.array_equal(np.isnan(got), np.isnan(ref)), what
    f = _filtered_mask(data)
    assert np.array_equal(got[~f], data[~f], equal_nan=True), what
    if not f.any():
        return 0.0
    dev = np.abs(got[f] - ref[f]) / np.maximum(1.0, np.abs(ref[f]))
    assert dev.max() <= bar, f'{what}: {dev.max():.3e} > {bar:.0e}'
    return float(dev.max())


def test_golden_columns(engine, gold):
    """All 60 golden columns: each mode and smoothing factor in one launch (columns NaN-padded to a common length)."""
    n = int(gold['n_cols'])
    prm = np.stack([gold[f'col{i}_prm'] for i in range(n)])
    worst = {'auto': 0.0, 'fixed': 0.0, 'lam': 0.0}
    groups = {}
    for i in range(n):
        auto, sf, cutoff, rate = prm[i]
        groups.setdefault((bool(auto), float(sf), float(cutoff), float(rate)), []).append(i)
    for (auto, sf, cutoff, rate), cols in groups.items():
        F = max(len(gold[f'col{i}_in']) for i in cols)
        pad = lambda key: np.stack([np.r_[gold[f'col{i}_{key}'], np.full(F - len(gold[f'col{i}_{key}']), np.nan)] for i in cols], axis=1)  # noqa: E731
        data, ref, lam_ref = pad('in'), pad('out'), pad('lam')
        out, lam = engine.gcv_spline(data, 'auto' if auto else int(cutoff), sf, rate)
        worst['auto' if auto else 'fixed'] = max(worst['auto' if auto else 'fixed'],
                                                 _check(data, out, ref, BAR_AUTO if auto else BAR_FIXED, f'columns {cols}'))
        assert np.array_equal(np.isnan(lam), np.isnan(lam_ref)), cols
        ok = ~np.isnan(lam_ref)
        rel = np.abs(lam[ok] - lam_ref[ok]) / np.maximum(1.0, lam_ref[ok])
        if auto:
            free = pad('lam_free')[ok] == 1.0                                  # runs on a line: lambda arbitrary
            n_run = np.array([len(seq) for c in range(data.shape[1]) for seq in runs(data[:, c]) if len(seq) >= 5])
            starts = np.array([(seq[0], c) for c in range(data.shape[1]) for seq in runs(data[:, c]) if len(seq) >= 5])
            order = np.lexsort((starts[:, 1], starts[:, 0]))                   # row-major, as lam[ok] is
            n_run = n_run[order]
            assert ((lam[ok][free] > 0) & (lam[ok][free] <= n_run[free] * sf)).all(), cols
            assert (rel[~free] <= BAR_LAM).all(), (cols, rel[~free].max())
            rel = rel[~free]
        else:
            assert (rel <= BAR_FIXED).all(), (cols, rel.max())
        if rel.size:
            worst['lam'] = max(worst['lam'], float(rel.max()))
    print(f"\ngolden columns: worst |d out| auto {worst['auto']:.3e}, fixed {worst['fixed']:.3e}; worst |d lam| {worst['lam']:.3e}")


def test_short_run_and_failures_raise_the_reference_error(engine, gold):
    data = gold['short_in'][:, None]
    for mode, cutoff in (('short_auto', 'auto'), ('short_fixed', 6)):
        with pytest.raises(ValueError) as e:
            engine.gcv_spline(data, cutoff, 1.0, 60)
        assert type(e.value).__name__ == str(gold[f'{mode}_type']) and str(e.value) == str(gold[f'{mode}_msg'])


@pytest.fixture
def work_dir():
    """A scratch directory whose path does not contain 'filt' (the reference skips every .trc whose path does)."""
    import shutil
    import tempfile
    from pathlib import Path
    d = tempfile.mkdtemp(prefix='p2s_gcv_')
    yield Path(d)
    shutil.rmtree(d, ignore_errors=True)


def test_filter_all_on_the_gpu(gold, work_dir):
    """The stage with the real engine: file name and header byte for byte, values within the bars."""
    from pose2sim_amd import filtering
    from pose2sim_amd.engine import Engine
    eng = Engine(0)
    base = work_dir
    for i in range(int(gold['n_files'])):
        cutoff, sf, reject, rate, frame_range = (str(v) for v in gold[f'file{i}_prm'])
        trial = base / f'trial{i}'
        (trial / 'pose-3d').mkdir(parents=True)
        (trial / 'pose-3d' / str(gold[f'file{i}_name'])).write_text(_text(gold, f'file{i}_text'))
        cfg = {'project': {'project_dir': str(trial), 'frame_rate': int(rate),
                           'frame_range': 'auto' if frame_range == 'auto' else [int(v) for v in frame_range.strip('[]').split(',')]},
               'pose': {'vid_img_extension': 'mp4'},
               'filtering': {'type': 'gcv_spline', 'filter': True, 'reject_outliers': reject == 'True', 'make_c3d': False,
                             'gcv_spline': {'cut_off_frequency': cutoff if cutoff == 'auto' else int(cutoff), 'smoothing_factor': float(sf)}}}
        paths = filtering.filter_all(cfg, engine=eng)
        assert [os.path.basename(p) for p in paths] == [str(gold[f'file{i}_out_name'])]
        got, ref = open(paths[0]).read().split('\n'), _text(gold, f'file{i}_out_text').split('\n')
        assert got[:5] == ref[:5] and len(got) == len(ref)
        parse = lambda lines: np.array([[float(v) if v else np.nan for v in r.split('\t')] for r in lines[5:] if r])  # noqa: E731
        g, r = parse(got), parse(ref)
        assert np.array_equal(g[:, :2], r[:, :2])
        assert np.array_equal(np.isnan(g), np.isnan(r))
        ok = ~np.isnan(r)
        dev = np.abs(g[ok] - r[ok]) / np.maximum(1.0, np.abs(r[ok]))
        bar = BAR_AUTO if cutoff == 'auto' else BAR_FIXED
        print(f'\nfile {i} ({cutoff}): worst |d| {dev.max():.3e}')
        assert dev.max() <= bar


def _seeded(F, C, seed):
    rng = np.random.default_rng(seed)
    t = np.arange(F)[:, None] / 60.0
    data = 0.8 + 0.3 * np.sin(2 * np.pi * rng.uniform(0.3, 2.0, C) * t + rng.uniform(0, 6, C)) + rng.normal(0, 0.01, (F, C))
    for c in range(C):                                                 # gaps: NaN and zero stretches, isolated misses
        for _ in range(int(rng.integers(0, 4))):
            g = int(rng.integers(0, F - 40)); data[g:g + int(rng.integers(5, 40)), c] = np.nan if rng.random() < 0.7 else 0.0
        data[rng.random(F) < 0.0005, c] = np.nan
    # no runs of 2 to 4 samples (the reference refuses them)
    for c in range(C):
        for seq in runs(data[:, c]):
            if 2 <= len(seq) <= 4:
                data[seq, c] = np.nan
    return data


def test_large_matrix_against_scipy(engine):
    """78 columns x 10 000 frames with gaps.  Fixed cut-off: every column against SciPy.  'auto': the search of six
    columns against SciPy's (its Python-loop search costs ~3 s per 10 000 samples), and the fit of every column with
    the GPU's lambda against make_smoothing_spline's fit with that lambda."""
    data = _seeded(10000, 78, 11)
    out, lam = engine.gcv_spline(data, 6, 1.0, 60)
    ref, lam_ref = gcv_spline_columns(data, 6, 1.0, 60)
    d_fixed = _check(data, out, ref, BAR_FIXED, 'fixed 78 x 10000')
    assert np.array_equal(lam, lam_ref, equal_nan=True)

    out, lam = engine.gcv_spline(data, 'auto', 1.0, 60)
    ref, _ = gcv_spline_columns(data, 'auto', 1.0, 60, lam_override=lam)
    d_fit = _check(data, out, ref, BAR_FIXED * 10, "'auto' fit with the GPU's lambda")
    sub = [0, 13, 29, 41, 60, 77]
    ref, lam_ref = gcv_spline_columns(data[:, sub], 'auto', 1.0, 60)
    d_auto = _check(data[:, sub], out[:, sub], ref, BAR_AUTO, "'auto' 6 x 10000")
    ok = ~np.isnan(lam_ref)
    assert np.array_equal(ok, ~np.isnan(lam[:, sub]))
    d_lam = float((np.abs(lam[:, sub][ok] - lam_ref[ok]) / np.maximum(1.0, lam_ref[ok])).max())
    assert d_lam <= BAR_LAM
    print(f'\n78 x 10000: fixed {d_fixed:.3e}; auto fit {d_fit:.3e}; auto (6 columns) {d_auto:.3e}, lam {d_lam:.3e}')


def test_edge_shapes(engine):
    F = 40
    assert engine.gcv_spline(np.zeros((F, 0)), 'auto', 1.0, 60)[0].shape == (F, 0)
    assert engine.gcv_spline(np.zeros((0, 3)), 6, 1.0, 60)[0].shape == (0, 3)
    rng = np.random.default_rng(3)
    data = 1.0 + 0.1 * rng.normal(size=(F, 4))
    data[:, 0] = np.nan                                                # all NaN
    data[5:, 1] = np.nan                                               # a run of exactly 5
    data[:, 2] = np.nan; data[7, 2] = 0.9; data[20:30, 2] = 1.1 + 0.01 * rng.normal(size=10)   # a single-sample run, and 10
    data[::2, 3] = 0.0                                                 # single samples between zeros only
    for cutoff in ('auto', 3):
        out, lam = engine.gcv_spline(data, cutoff, 2.0, 60)
        ref, lam_ref = gcv_spline_columns(data, cutoff, 2.0, 60)
        _check(data, out, ref, BAR_AUTO if cutoff == 'auto' else BAR_FIXED, f'edge shapes {cutoff}')
        assert np.array_equal(np.isnan(lam), np.isnan(lam_ref))
        assert np.isnan(lam[:, [0, 3]]).all() and not np.isnan(lam[0, 1]) and not np.isnan(lam[20, 2])


def test_pose2sim_filtering_with_a_gcv_spline_config(gold, work_dir, monkeypatch):
    """Pose2Sim.filtering() on a trial whose Config.toml says type = 'gcv_spline': the reference's file name and header,
    values within the 'auto' bar."""
    from pose2sim_amd import Pose2Sim
    trial = work_dir / 'trial'
    (trial / 'pose-3d').mkdir(parents=True)
    (trial / 'pose-3d' / str(gold['file0_name'])).write_text(_text(gold, 'file0_text'))
    (trial / 'Config.toml').write_text('[project]\nframe_rate = 60\nframe_range = []\n\n[pose]\nvid_img_extension = "mp4"\n\n'
                                       '[logging]\nuse_custom_logging = true\n\n'
                                       '[filtering]\ntype = "gcv_spline"\nfilter = true\nreject_outliers = false\nmake_c3d = false\n'
                                       '[filtering.gcv_spline]\ncut_off_frequency = "auto"\nsmoothing_factor = 1.0\n')
    monkeypatch.chdir(trial)
    Pose2Sim.filtering()
    got = (trial / 'pose-3d' / str(gold['file0_out_name'])).read_text().split('\n')
    ref = _text(gold, 'file0_out_text').split('\n')
    assert got[:5] == ref[:5] and len(got) == len(ref)
    parse = lambda lines: np.array([[float(v) if v else np.nan for v in r.split('\t')] for r in lines[5:] if r])  # noqa: E731
    g, r = parse(got), parse(ref)
    assert np.array_equal(np.isnan(g), np.isnan(r))
    ok = ~np.isnan(r)
    assert (np.abs(g[ok] - r[ok]) / np.maximum(1.0, np.abs(r[ok]))).max() <= BAR_AUTO
