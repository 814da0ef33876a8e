"""What bench.py computes, checked against the CPU oracles at the benchmarked shapes.

For each config: bench.py runs one timed step in a child process and dumps its outputs (--dump-outputs); this process
rebuilds the input that step read, re-runs the entry the bench times on a fresh Engine and requires the dumped items bit
for bit; then the re-run is compared with the oracles on samples chosen to include the places where kernels go wrong
(chunk bounds of the one-launch kernels, the deepest searches, rejected units, frames of every search class).  The
association configs also run every frame through the float64 instantiation of their kernel, which must equal the
float32 run bit for bit: both widen to double as they load and share every operation after the load.
cfg5 at full length (12.5 GB per GPU) is left out: it runs cfg5_tenth's kernels.
"""
import os
import subprocess
import sys
import time

import numpy as np
import pytest

import bench
from test_tri_gpu import TOL_E, _compare, oracle_threads

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _run_bench(config, out_dir):
    """One timed step of `config` in a fresh child process; -> {name: dumped array}.  With no pre-roll and no warm-up
    the one timed step is the first step of the run, so it reads input buffer 0 (seed = cfg['seed'] on rank 0)."""
    env = {k: v for k, v in os.environ.items() if k not in ('WORLD_SIZE', 'RANK', 'LOCAL_RANK', 'MASTER_ADDR', 'MASTER_PORT')}
    cmd = [sys.executable, os.path.join(ROOT, 'bench.py'), '--config', config, '--steps', '1', '--warmup', '0',
           '--preroll-ms', '0', '--no-cpu-baseline', '--dump-outputs', str(out_dir)]
    r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    return {f[:-4]: np.load(os.path.join(out_dir, f)) for f in sorted(os.listdir(out_dir))}


def _engine():
    import torch
    import __graft_entry__ as entry
    entry.build_hip()
    from pose2sim_amd.engine import Engine
    eng = Engine(0)
    eng.set_stream(torch.cuda.current_stream().cuda_stream)
    return eng


def _same_as_dump(dump, mine):
    assert set(dump) == set(mine), (sorted(dump), sorted(mine))
    for k, a in mine.items():
        assert a.dtype == dump[k].dtype and np.array_equal(a, dump[k]), f'{k}: the re-run differs from what the bench dumped'


def _bits_equal(a, b):
    """Two device tensors hold the same bytes (NaN payloads included)."""
    import torch
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(a.contiguous().view(torch.uint8), b.contiguous().view(torch.uint8))


# ---- triangulation ---------------------------------------------------------------------------------------------------
def chunk_bounds(n_blocks, C, K, fused, blocks_per_tile):
    """[(first block, end)] of the launches p2s_triangulate_device makes for float32 observations: the one-launch kernels
    keep 32-bit byte offsets below 2^31 from a.block0 in chunks of whole 16-block groups; the work-list pair takes chunks of
    whole tiles of at most 2^22 units."""
    if fused:
        chunk = max(16, ((1 << 31) // (C * K * 12)) // 16 * 16)
    else:
        fb = blocks_per_tile
        chunk = max(fb, ((1 << 22) // K) // fb * fb)
        chunk = min(chunk, -(-n_blocks // fb) * fb)
    return [(b0, min(b0 + chunk, n_blocks)) for b0 in range(0, n_blocks, chunk)]


# blocks drawn at random per config (the C oracle: ~300 blocks/s/core at 8 cameras, ~8 at 32 with undistortion and swap)
TRI_SAMPLE = {'cfg2': 20_000, 'cfg2_clean': 20_000, 'cfg4': 8_000, 'cfg5_tenth': 1_000}


@pytest.mark.parametrize('config', ['cfg2', 'cfg2_clean', 'cfg4', 'cfg5_tenth'])
def test_triangulation_config_against_the_oracle(tmp_path, config):
    import torch
    from oracle import tri_oracle
    from pose2sim_amd import skeletons, synth, synth_device
    from pose2sim_amd.engine import P2S_F32
    dump = _run_bench(config, tmp_path / 'dump')
    cfg = bench.CONFIGS[config]
    ids, names, swap_list = skeletons.keypoints(cfg['model'])
    K, C, Pn, F = len(ids), cfg['C'], cfg['Pn'], cfg['F']
    n_blocks, n_units = F * Pn, F * Pn * K
    cams = synth.make_cameras(C, seed=cfg['seed'], distort=cfg['undistort'])
    P = synth.projection_matrices(cams, cfg['undistort'])
    dev = torch.device('cuda', 0)
    # input buffer 0 of rank 0, with bench.py's arguments
    d_xyl = synth_device.make_observations_device(cams, F, Pn, K, seed=cfg['seed'], device=dev, distort=cfg['undistort'],
                                                  p_lr_swap=0.02 if cfg['lr_swap'] else 0.0, swap_idx=swap_list,
                                                  **dict(cfg.get('gen', {})))
    d_swap = torch.from_numpy(np.asarray(swap_list, dtype=np.int32)).to(dev)
    d_Q = torch.empty((n_units, 3), dtype=torch.float64, device=dev)
    d_e = torch.empty(n_units, dtype=torch.float32, device=dev)
    d_m = torch.empty(n_units, dtype=torch.int32, device=dev)
    d_x = torch.empty(n_units, dtype=torch.uint8, device=dev)
    eng = _engine()
    try:
        eng.set_calibration(P, cams)
        prm = eng.tri_params(cfg['thr'], cfg['lik'], cfg['min_cams'], cfg['undistort'], cfg['lr_swap'])
        eng.triangulate_device(n_blocks, K, P2S_F32, d_xyl, d_swap, prm, d_Q.data_ptr(), d_e.data_ptr(), d_x.data_ptr(), d_m.data_ptr())
        torch.cuda.synchronize()
        fb = eng.tri_geometry(K, P2S_F32)['blocks_per_tile']
    finally:
        eng.close()
    Q, err = d_Q.cpu().numpy(), d_e.cpu().numpy()
    nex, mask = d_x.cpu().numpy(), d_m.cpu().numpy().view(np.uint32)

    # the dumped items, as bench.py writes them
    idx = dump['unit_index'].astype(np.int64)
    acc = np.isfinite(err[idx])
    _same_as_dump(dump, {'unit_index': idx.astype(np.float64), 'accepted': acc.astype(np.float32),
                         'Q': bench.where_valid(acc, Q[idx]), 'err': bench.where_valid(acc, err[idx]),
                         'n_excluded': nex[idx].astype(np.float32), 'camera_mask': mask[idx].astype(np.float64)})

    # the oracle's blocks: a seeded sample, the first and last 64 blocks of every launch, the last block, the blocks of
    # the 200 units with the most excluded cameras and (a sample of) the blocks holding rejected units
    rng = np.random.default_rng(cfg['seed'] + 31)
    fused = not cfg['undistort'] and not cfg['lr_swap'] and C <= 16
    bounds = chunk_bounds(n_blocks, C, K, fused, fb)
    edge = np.concatenate([np.r_[b0:min(b0 + 64, b1)] for b0, b1 in bounds] + [np.r_[max(b0, b1 - 64):b1] for b0, b1 in bounds])
    deepest = np.argsort(-nex.astype(np.int64), kind='stable')[:200] // K
    rejected = np.unique(np.flatnonzero(np.isnan(err)) // K)
    if len(rejected) > 300:
        rejected = rng.choice(rejected, 300, replace=False)
    blocks = np.unique(np.concatenate([rng.choice(n_blocks, TRI_SAMPLE[config], replace=False), edge, [n_blocks - 1],
                                       deepest, rejected]).astype(np.int64))
    xyl = d_xyl.view(n_blocks, C, K, 3)[torch.from_numpy(blocks).to(dev)].cpu().numpy().astype(np.float64)
    del d_xyl, d_Q, d_e, d_m, d_x
    torch.cuda.empty_cache()
    t0 = time.perf_counter()
    Qr, er, nr, mr = tri_oracle.triangulate_batch(xyl, P, cams if cfg['undistort'] else None, swap_list, cfg['lik'], cfg['thr'],
                                                  cfg['min_cams'], cfg['lr_swap'], cfg['undistort'], threads=oracle_threads())
    t_oracle = time.perf_counter() - t0
    units = (blocks[:, None] * K + np.arange(K)).ravel()
    dq = _compare(Q[units], err[units], nex[units], mask[units], Qr, er, nr, mr, config)
    er = er.reshape(-1)
    ok = ~np.isnan(er)
    de = float((np.abs(err[units][ok].astype(np.float64) - er[ok]) / np.maximum(1.0, np.abs(er[ok]))).max())
    assert de <= TOL_E
    sides = '; '.join(f'[{b0}, {b1})' for b0, b1 in bounds)
    print(f'{config}: {len(blocks)} blocks = {len(units)} units against the oracle ({len(edge)} at the launch bounds {sides}, '
          f'{len(rejected)} with rejected units, max n_excl {int(nex.max())}), worst |dQ| = {dq:.3e} m, worst error deviation '
          f'{de:.3e}, oracle {t_oracle:.1f} s on {oracle_threads()} threads')


# ---- association ---------------------------------------------------------------------------------------------------
def _frame_lists(n_persons, rows, f, offsets):
    """Frame f as the oracles take it: per camera, the flat float64 keypoint lists of its detections."""
    per_cam, r = [], int(offsets[f])
    for c in range(n_persons.shape[1]):
        per_cam.append([rows[r + i].astype(np.float64).ravel() for i in range(n_persons[f, c])])
        r += int(n_persons[f, c])
    return per_cam


def test_cfg3_against_the_oracle(tmp_path):
    import torch
    from oracle import association_ref as ar
    from pose2sim_amd.engine import P2S_F32, P2S_F64
    dump = _run_bench('cfg3', tmp_path / 'dump')
    cfg = bench.CONFIGS['cfg3']
    xyl, cams, P, swap, K = bench.make_workload(cfg, 0)
    n_persons, kpts = bench.make_association_inputs(xyl, cfg['seed'])
    del xyl
    F, C = n_persons.shape
    per_frame = n_persons.sum(axis=1, dtype=np.int64)
    offsets = np.zeros(F + 1, dtype=np.int64)
    np.cumsum(per_frame, out=offsets[1:])
    n_max = max(2, (int(per_frame.max()) + 1) & ~1)
    dev = torch.device('cuda', 0)
    d_np, d_off = torch.from_numpy(n_persons).to(dev), torch.from_numpy(offsets).to(dev)
    d_kp = torch.from_numpy(kpts).to(dev)
    eng = _engine()
    try:
        eng.set_calibration(P, cams)
        prm = eng.assoc_params(0.1, 0.2, cfg['min_cams'])
        d_aff = torch.empty((F, n_max, n_max), dtype=torch.float64, device=dev)
        eng.associate_device(F, K, n_max, P2S_F32, d_np, d_off, d_kp, prm, d_aff)
        # every frame again through the float64 instantiation, on the same numbers widened
        d_kp64 = d_kp.to(torch.float64)
        d_aff64 = torch.empty_like(d_aff)
        eng.associate_device(F, K, n_max, P2S_F64, d_np, d_off, d_kp64, prm, d_aff64)
        torch.cuda.synchronize()
        r = np.arange(n_max)
        valid = (r[None, :, None] < per_frame[:, None, None]) & (r[None, None, :] < per_frame[:, None, None])
        d_valid = torch.from_numpy(valid).to(dev)
        d_aff.masked_fill_(~d_valid, 0.0)
        d_aff64.masked_fill_(~d_valid, 0.0)
        assert _bits_equal(d_aff, d_aff64), 'float32 and float64 association runs differ'
        del d_aff64, d_kp64, d_valid
        aff = d_aff.cpu().numpy()
        idx = dump['frame_index'].astype(np.int64)
        _same_as_dump(dump, {'frame_index': idx.astype(np.float64), 'n_detections': per_frame[idx].astype(np.float64),
                             'affinity': aff[idx]})

        # the oracle on a seeded sample of the dumped frames and on the frames with the most detections; a frame holding an
        # all-zero detection (a person some camera misses) converges to a rounding-decided tie: its continuous iterates
        # after 1 and 3 passes are compared instead
        rng = np.random.default_rng(cfg['seed'] + 41)
        fullest = np.flatnonzero(per_frame == per_frame.max())[:24]
        frames = np.unique(np.concatenate([rng.choice(idx, 320, replace=False), fullest]))
        zero_row = (kpts == 0).all(axis=(1, 2))
        has_zero = np.add.reduceat(zero_row, offsets[:-1]) > 0
        tie = frames[has_zero[frames]]
        cal = {'inv_K': cams['inv_K'], 'R_mat': cams['R_mat'], 'T': cams['T']}
        t0 = time.perf_counter()
        worst = 0.0
        for f in frames[~has_zero[frames]]:
            per_cam = _frame_lists(n_persons, kpts, f, offsets)
            cum = np.cumsum([0] + [len(p) for p in per_cam])
            ref = ar.match_svt(ar.affinity_matrix(per_cam, cal, cum, 0.1), cum, max_iter=20)
            ref = np.where(ref < 0.2, 0.0, ref)
            N = int(per_frame[f])
            d = float(np.abs(aff[f, :N, :N] - ref).max())
            worst = max(worst, d)
            assert d <= 1e-9, (f, N, d)
        worst_it = 0.0
        if len(tie):
            t_np = n_persons[tie]
            t_rows = np.concatenate([kpts[offsets[f]:offsets[f + 1]] for f in tie])
            for it in (1, 3):
                got = eng.associate(t_np, t_rows, eng.assoc_params(0.1, -1.0, cfg['min_cams'], max_iter=it))
                for j, f in enumerate(tie):
                    per_cam = _frame_lists(n_persons, kpts, f, offsets)
                    cum = np.cumsum([0] + [len(p) for p in per_cam])
                    ref = ar.match_svt(ar.affinity_matrix(per_cam, cal, cum, 0.1), cum, max_iter=it)
                    N = int(per_frame[f])
                    d = float(np.abs(got[j, :N, :N] - ref).max())
                    worst_it = max(worst_it, d)
                    assert d <= 1e-9, (f, it, N, d)
    finally:
        eng.close()
    print(f'cfg3: {len(frames) - len(tie)} converged frames (detections up to {int(per_frame[frames].max())}) within '
          f'{worst:.3e}; {len(tie)} frames with an all-zero detection compared after 1 and 3 passes within {worst_it:.3e}; '
          f'oracle {time.perf_counter() - t0:.1f} s; float64 run equal to the float32 run on all {F} frames')


def test_single_against_the_oracle(tmp_path):
    import multiprocessing
    import torch
    from oracle import association_single_ref as sr
    from pose2sim_amd import skeletons
    from pose2sim_amd.engine import P2S_F32, P2S_F64
    from test_assoc_gpu import _check_single
    dump = _run_bench('single', tmp_path / 'dump')
    cfg = bench.CONFIGS['single']
    xyl, cams, P, swap, K = bench.make_workload(cfg, 0)
    n_persons, kpts = bench.make_association_inputs(xyl, cfg['seed'])
    del xyl
    ids, names, _ = skeletons.keypoints(cfg['model'])
    tracked = np.ascontiguousarray(kpts[:, names.index('Neck'), :])
    del kpts
    F, C = n_persons.shape
    offsets = np.zeros(F + 1, dtype=np.int64)
    np.cumsum(n_persons.sum(axis=1, dtype=np.int64), out=offsets[1:])
    dev = torch.device('cuda', 0)
    d_np, d_off = torch.from_numpy(n_persons).to(dev), torch.from_numpy(offsets).to(dev)
    outs = {}
    eng = _engine()
    try:
        eng.set_calibration(P, cams)
        for dtype, host in ((P2S_F32, tracked), (P2S_F64, tracked.astype(np.float64))):
            d_tk = torch.from_numpy(host).to(dev)
            o = (torch.empty((F, C), dtype=torch.int32, device=dev), torch.empty(F, dtype=torch.float64, device=dev),
                 torch.empty((F, 3), dtype=torch.float64, device=dev))
            eng.associate_single_device(F, dtype, d_np, d_off, d_tk, cfg['thr'], cfg['lik'], cfg['min_cams'], *o)
            torch.cuda.synchronize()
            outs[dtype] = o
    finally:
        eng.close()
    for a, b, what in zip(outs[P2S_F32], outs[P2S_F64], ('combination', 'error', 'Q')):
        assert _bits_equal(a, b), f'{what}: float32 and float64 single-person runs differ'
    comb, err, Q = (t.cpu().numpy() for t in outs[P2S_F32])
    idx = dump['frame_index'].astype(np.int64)
    solved = np.isfinite(err[idx])
    _same_as_dump(dump, {'frame_index': idx.astype(np.float64), 'found': solved.astype(np.float32),
                         'combination': comb[idx].astype(np.float32), 'error': bench.where_valid(solved, err[idx]),
                         'Q': bench.where_valid(solved, Q[idx])})

    # a seeded sample and frames of every class of the search
    rng = np.random.default_rng(cfg['seed'] + 51)
    lik = tracked[:, 2]
    unusable = (lik < cfg['lik']) | (lik == 0)                    # a detection whose camera the search switches off
    low = np.add.reduceat(unusable, offsets[:-1]) > 0
    # solved with a camera off whose detections are all usable: an extra camera was switched off
    cam_of_row = np.repeat(np.tile(np.arange(C), F), n_persons.ravel())
    frame_of_row = np.repeat(np.arange(F), n_persons.sum(axis=1))
    bad_cam = np.zeros((F, C), bool)
    bad_cam[frame_of_row[unusable], cam_of_row[unusable]] = True
    extra = np.isfinite(err) & ((comb == -1) & (n_persons > 0) & ~bad_cam).any(axis=1)
    n_comb = np.prod(np.maximum(n_persons, 1).astype(np.float64), axis=1)
    classes = {'no solution': np.flatnonzero(~np.isfinite(err)), 'extra cameras off': np.flatnonzero(extra),
               'low likelihood': np.flatnonzero(low), '6561 combinations': np.flatnonzero(n_comb == 6561)}
    picked = [rng.choice(idx, 160, replace=False)]
    for name, fr in classes.items():
        # with 3 detections on each of 8 cameras every frame of the workload has had a solution so far; frames without one
        # are in tests/test_assoc_gpu.py (test_single_person_edge_cases)
        assert len(fr) or name == 'no solution', f'the single workload has no frame of class {name!r}'
        if len(fr):
            picked.append(rng.choice(fr, min(len(fr), 24), replace=False))
    frames = np.unique(np.concatenate(picked))
    Pl = [np.asarray(p) for p in P]
    jobs = []
    for f in frames:
        per_cam = [[list(r) for r in p] for p in _frame_lists(n_persons, tracked, f, offsets)]
        jobs.append((per_cam, sr.persons_combinations(n_persons[f]), Pl, 0, cfg['thr'], cfg['min_cams'], cfg['lik']))
    t0 = time.perf_counter()
    n_workers = min(16, oracle_threads())
    # the oracle is NumPy at ~0.3 s per frame: spawned workers, which import numpy and the oracle only
    with multiprocessing.get_context('spawn').Pool(n_workers) as pool:
        res = pool.starmap(sr.best_persons_and_cameras, jobs, chunksize=1)
    t_oracle = time.perf_counter() - t0
    want_e = np.array([r[0] for r in res])
    want_c = np.array([r[1] for r in res])
    want_q = np.array([r[2] for r in res])
    _check_single(comb[frames], err[frames], Q[frames], want_c, want_e, want_q, 'single')
    ok = np.isfinite(want_e)
    dq = float(np.abs(Q[frames][ok] - want_q[ok]).max()) if ok.any() else 0.0
    de = float(np.abs(err[frames][ok] - want_e[ok]).max()) if ok.any() else 0.0
    counts = ', '.join(f'{name} {int(np.isin(frames, fr).sum())}' for name, fr in classes.items())
    print(f'single: {len(frames)} frames against the oracle ({counts}), worst |dQ| = {dq:.3e} m, worst |d error| = {de:.3e} px, '
          f'oracle {t_oracle:.1f} s on {n_workers} workers; float64 run equal to the float32 run on all {F} frames')
