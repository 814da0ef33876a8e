"""Python face of the HIP engine: one ``Engine`` per GPU, thin wrappers over the C-ABI.

Host arrays are NumPy (the library copies them in and out); device-resident operands are passed
as raw pointers (``tensor.data_ptr()``), with torch used only as the allocator / stream owner.
"""
import ctypes as C

import numpy as np

from . import _lib
from ._lib import P2S_F32, P2S_F64, AssocParams, P2sError, SingleParams, TriParams  # noqa: F401


def _ptr(a):
    if a is None:
        return None
    if isinstance(a, np.ndarray):
        return a.ctypes.data_as(C.c_void_p)
    if hasattr(a, 'data_ptr'):
        return C.c_void_p(a.data_ptr())
    return C.c_void_p(int(a))


def _optr(a):
    """_ptr of an array, None for an empty one (the library takes NULL for "no data")."""
    return _ptr(a) if a.size else None


def _entry(lib, name):
    """The entry point `name` of the loaded library; a library built before it existed is refused."""
    fn = getattr(lib, name, None)
    if fn is None:
        raise NotImplementedError(f'{_lib.LIB_PATH} has no {name}: rebuild it')
    return fn


def _kernel_ms(self, name):
    """What p2s_<name>_kernel_ms answers for the engine `self`: the kernel time of that stage's last call, from the HIP
    events around its kernels."""
    ms = C.c_float(0)
    _lib.check(_entry(self._lib, f'p2s_{name}_kernel_ms')(self._h, C.byref(ms)))
    return ms.value


def _matrix(data):
    """data as a contiguous float64 [n_frames][n_cols] matrix."""
    data = np.ascontiguousarray(data, dtype=np.float64)
    if data.ndim != 2:
        raise P2sError(f'data has shape {data.shape}; expected [n_frames][n_cols]')
    return data


def _coeffs(b, a, zi):
    """Filter coefficients b, a and the start state zi (scipy.signal.lfilter_zi) as contiguous float64 vectors."""
    b, a, zi = (np.ascontiguousarray(v, dtype=np.float64).reshape(-1) for v in (b, a, zi))
    if len(a) != len(b) or len(zi) != len(b) - 1:
        raise P2sError('b, a and zi must have n, n and n - 1 coefficients')
    return b, a, zi


def _offsets(lengths):
    """[0, lengths[0], lengths[0] + lengths[1], ...] as int64: where every run of `lengths` starts, and the total."""
    return np.concatenate([[0], np.cumsum(lengths, dtype=np.int64)])


def _per(values, n, dtype=np.float64):
    """One value, or one per item, as a contiguous vector of n."""
    return np.ascontiguousarray(np.broadcast_to(np.asarray(values, dtype=dtype), (n,)))


def _pack_persons(cameras, n_kpts):
    """cameras: per camera (persons [N][n_kpts][3], offsets [n_frames + 1]) -> (persons, offsets) per camera as checked
    arrays, n_frames [C], base [C + 1] the cameras' first persons, off [frames + 1] the first person of every frame among
    all persons, flat: the persons of all cameras back to back."""
    persons, offsets = [], []
    for p, o in cameras:
        p = np.ascontiguousarray(p, dtype=np.float64).reshape(-1, n_kpts, 3)
        o = np.ascontiguousarray(o, dtype=np.int64).reshape(-1)
        if len(o) < 1 or o[0] != 0 or o[-1] != len(p) or (np.diff(o) < 0).any():
            raise P2sError('offsets must rise from 0 to the number of persons')
        persons.append(p)
        offsets.append(o)
    if len(persons) < 1:
        raise P2sError('at least one camera is required')
    n_frames = np.array([len(o) - 1 for o in offsets], dtype=np.int64)
    base = _offsets([len(p) for p in persons])
    off = np.concatenate([o[:-1] + b for o, b in zip(offsets, base[:-1])] + [base[-1:]]).astype(np.int64)
    flat = persons[0] if len(persons) == 1 else np.concatenate(persons)
    return persons, offsets, n_frames, base, off, flat


def loess_window(nb_values_used):
    """(k, min_run) of the reference's loess filter for its nb_values_used: statsmodels' lowess takes
    k = int(frac * n + 1e-10) neighbours with frac = nb / n, and the reference filters the runs with len > nb
    (filtering.py:552-556)."""
    nb = float(nb_values_used)
    if not nb >= 2:
        raise ValueError(f'loess: nb_values_used = {nb_values_used} gives a window of fewer than 2 samples, whose radius is 0')
    return int(nb + 1e-10), int(np.floor(nb)) + 1


def _cal_arrays(cal, n):
    """K [n][9], dist [n][5] (k1, k2, p1, p2[, k3]), R [n][9], T [n][3] of a calibration dict, contiguous float64."""
    d = np.zeros((n, 5))
    for c in range(n):
        dc = np.asarray(cal['dist'][c], dtype=np.float64).ravel()
        if len(dc) > 5 and np.any(dc[5:] != 0):
            raise P2sError('only k1,k2,p1,p2[,k3] distortion terms are supported')
        d[c, :min(5, len(dc))] = dc[:5]
    K, R, T = (np.ascontiguousarray(np.asarray(cal[k], dtype=np.float64).reshape(n, w)) for k, w in (('K', 9), ('R_mat', 9), ('T', 3)))
    return K, d, R, T


def as_packed(xyl):
    """Pick the narrowest exact dtype for an observation tensor: float32 when every value is
    float32-representable (RTMLib output is, poseEstimation.py:259), else float64, so that the
    kernel sees exactly the numbers the reference would read from the JSON files."""
    xyl = np.asarray(xyl)
    if xyl.dtype == np.float32:
        return np.ascontiguousarray(xyl), P2S_F32
    x64 = np.ascontiguousarray(xyl, dtype=np.float64)
    x32 = x64.astype(np.float32)
    same = (x32.astype(np.float64) == x64) | np.isnan(x64)
    if same.all():
        return x32, P2S_F32
    return x64, P2S_F64


def write_openpose_files(cam_dirs, name_root, uv, marker_index=None, n_threads=0):
    """dataset_to_openpose (Utilities/reproj_from_trc_calib.py:245-286) for every camera and frame: the files
    `<cam_dirs[c]>/<name_root>_cam<c+1>_openpose_<frame>.json` from uv [C][F][K][2], written by the native writer on at
    most 16 host threads (no GPU involved).  marker_index: the marker of every output position (default: all, in order).
    -> number of files written."""
    import os
    lib = _lib.load()
    fn = _entry(lib, 'p2s_write_openpose_files')
    uv = np.ascontiguousarray(uv, dtype=np.float64)
    if uv.ndim != 4 or uv.shape[3] != 2 or uv.shape[0] != len(cam_dirs):
        raise P2sError(f'uv has shape {uv.shape}; expected [{len(cam_dirs)}][F][K][2]')
    Cn, F, K = uv.shape[:3]
    idx = np.arange(K, dtype=np.int32) if marker_index is None else np.ascontiguousarray(marker_index, dtype=np.int32).reshape(-1)
    names = [os.fsencode(d) for d in cam_dirs]
    offsets = _offsets([len(n) for n in names])
    done = C.c_int64(0)
    _lib.check(fn(b''.join(names), _ptr(offsets), os.fsencode(name_root), Cn, F, K, len(idx), _optr(idx), _optr(uv),
                  int(n_threads), C.byref(done)))
    return done.value


class TrackShapeError(P2sError):
    """p2s_track_persons_* refused the shape: persons outside 1 .. 32, or keypoints beyond what the device's LDS holds."""


def _track_persons(lib, handle, Q, first_frame, max_dist, state):
    """p2s_track_persons_host on `handle` (None: the library's host path) for one trial Q [F][P][K][3] or a list of
    trials of one P and K; what Engine.track_persons_3d returns."""
    fn = _entry(lib, 'p2s_track_persons_host')
    single = not isinstance(Q, (list, tuple))
    trials = [np.ascontiguousarray(q, dtype=np.float64) for q in ([Q] if single else Q)]
    if not trials or any(q.ndim != 4 or q.shape[1:] != trials[0].shape[1:] or q.shape[3] != 3 for q in trials):
        raise P2sError('every trial needs a [n_frames][n_persons][n_kpts][3] array with the same n_persons and n_kpts')
    T, (P, K) = len(trials), trials[0].shape[1:3]
    off = _offsets([len(q) for q in trials])
    N = int(off[-1])
    first = _per(first_frame, T, np.int64)
    flat = trials[0] if T == 1 else np.concatenate(trials)
    S = _lib.P2S_TRACK_MAX_SLOTS
    state_in = n_in = None
    if state is not None:
        states = [np.asarray(s, dtype=np.float64).reshape(-1, K, 3) for s in ([state] if single else state)]
        if len(states) != T or max(len(s) for s in states) > S:
            raise P2sError(f'state: one [n <= {S}][n_kpts][3] array per trial')
        n_in = np.array([len(s) for s in states], dtype=np.int32)
        state_in = np.full((T, S, K, 3), np.nan)
        for t, s in enumerate(states):
            state_in[t, :len(s)] = s
    ids, n_slots = np.empty((N, P), dtype=np.int32), np.empty(N, dtype=np.int32)
    rows, dist = np.empty((N, P, K, 3)), np.empty((N, P))
    state_out, n_out, status = np.empty((T, S, K, 3)), np.zeros(T, dtype=np.int32), np.zeros((T, 2), dtype=np.int32)
    rc = fn(handle, T, _ptr(off), _ptr(first), P, K, _optr(flat), 0 if max_dist is None else 1, 0.0 if max_dist is None else float(max_dist),
            _ptr(state_in), _ptr(n_in), _optr(ids), _optr(rows), _optr(dist), _optr(n_slots), _ptr(state_out), _ptr(n_out), _ptr(status))
    if rc == _lib.P2S_ERR_INVALID_ARG:
        raise TrackShapeError(f'p2s error {rc}: {lib.p2s_last_error().decode()}')
    _lib.check(rc)
    for t in np.flatnonzero(status[:, 0] > 0):                        # a stopped trial: the library writes nothing from that frame on
        stop = slice(off[t] + status[t, 0] - 1, off[t + 1])
        rows[stop], ids[stop], dist[stop], n_slots[stop] = np.nan, -1, np.nan, 0
    cut = lambda a: [a[off[t]:off[t + 1]] for t in range(T)]         # noqa: E731
    out = (cut(rows), cut(ids), cut(dist), cut(n_slots), [state_out[t, :n_out[t]] for t in range(T)], list(status))
    return tuple(o[0] for o in out) if single else out


def track_persons_3d_host(Q, first_frame=0, max_dist=None, state=None):
    """Engine.track_persons_3d by the library's host path (no context, no GPU): the same code, for checking it."""
    return _track_persons(_lib.load(), None, Q, first_frame, max_dist, state)


def _interpolate_gaps(lib, handle, coords, labels, max_gap, kind):
    """p2s_interpolate_gaps on `handle` (None: the library's host path); what Engine.interpolate_gaps returns."""
    fn = _entry(lib, 'p2s_interpolate_gaps')
    coords = _matrix(coords)
    labels = np.ascontiguousarray(labels, dtype=np.int64).reshape(-1)
    if len(labels) != len(coords):
        raise P2sError(f'{len(labels)} labels for {len(coords)} frames')
    out, status = np.empty_like(coords), np.zeros(coords.shape[1], dtype=np.int32)
    code = _lib.P2S_GAPS_KINDS.get(kind, -1) if kind is None or isinstance(kind, str) else -1
    _lib.check(fn(handle, coords.shape[0], coords.shape[1], _optr(coords), _optr(labels), float(max_gap), code, _optr(out), _optr(status)))
    return out, status


def _fill_gaps(lib, handle, coords, how):
    fn = _entry(lib, 'p2s_fill_gaps')
    coords = _matrix(coords)
    out = np.empty_like(coords)
    code = _lib.P2S_GAPS_FILLS.get(how, 0) if isinstance(how, str) else 0
    _lib.check(fn(handle, coords.shape[0], coords.shape[1], _optr(coords), code, _optr(out)))
    return out


def _gap_runs(lib, handle, x, first, last, max_gap, capacity, raw):
    fn = _entry(lib, 'p2s_gap_runs')
    x = _matrix(x)
    F, K = x.shape
    cap = K * ((F + 1) // 2) if capacity is None else int(capacity)      # a run and the sample that ends it: no column holds more
    table = np.empty((max(cap, 0), 4), dtype=np.int32)
    count, over = C.c_int64(0), C.c_int32(0)
    _lib.check(fn(handle, F, K, _optr(x), int(first), int(last), float(max_gap), cap, _ptr(table), C.byref(count), C.byref(over)))
    table = table[:min(count.value, cap)]
    if raw:
        return table, count.value, bool(over.value)
    if over.value:
        raise P2sError(f'{count.value} runs do not fit a table of {cap}')
    done, left = [[] for _ in range(K)], [[] for _ in range(K)]
    for c, a, b, is_long in table.tolist():
        (left if is_long else done)[c].append(f'{a}:{b}')
    return done, left


def interpolate_gaps_host(coords, labels, max_gap, kind):
    """Engine.interpolate_gaps by the library's host path (no context, no GPU): the same code, for checking it."""
    return _interpolate_gaps(_lib.load(), None, coords, labels, max_gap, kind)


def fill_gaps_host(coords, how):
    return _fill_gaps(_lib.load(), None, coords, how)


def gap_runs_host(x, first, last, max_gap, capacity=None, raw=False):
    return _gap_runs(_lib.load(), None, x, first, last, max_gap, capacity, raw)


TIMELINE_MAX_KPTS = 26


def _timeline_rows(lib, handle, file_off, person_base, valid, conf):
    """p2s_timeline_rows_host on `handle` (None: the library's host path); what Engine.timeline_rows returns."""
    fn = _entry(lib, 'p2s_timeline_rows_host')
    file_off = np.ascontiguousarray(file_off, dtype=np.int64).reshape(-1)
    person_base = np.ascontiguousarray(person_base, dtype=np.int64).reshape(-1)
    valid = np.ascontiguousarray(np.asarray(valid).reshape(-1) != 0, dtype=np.uint8)
    conf = np.ascontiguousarray(conf, dtype=np.float64)
    if len(file_off) < 2 or file_off[0] != 0 or (np.diff(file_off) < 0).any():
        raise ValueError('file_off must rise from 0, one entry a camera and one more')
    if len(person_base) != file_off[-1] + 1 or person_base[0] != 0 or (np.diff(person_base) < 0).any():
        raise ValueError(f'person_base must rise from 0 and have {int(file_off[-1]) + 1} entries, one a file and one more')
    N = int(person_base[-1])
    if len(valid) != N or conf.ndim != 2 or len(conf) != N:
        raise ValueError(f'valid [{N}] and conf [{N}][K] are required: one entry a listed person')
    K = conf.shape[1]
    if not 1 <= K <= TIMELINE_MAX_KPTS:
        raise ValueError(f'conf has {K} keypoints; expected 1 .. {TIMELINE_MAX_KPTS}')
    Cn, nv = len(file_off) - 1, int(valid.sum())
    counts = np.diff(person_base)
    S = sum(int(counts[a:b].max(initial=0)) for a, b in zip(file_off[:-1], file_off[1:]))
    out = {'row_off': np.zeros(Cn + 1, dtype=np.int64), 'frame': np.empty(K * nv, dtype=np.int32), 'person': np.empty(K * nv, dtype=np.int32),
           'slot': np.empty(K * nv, dtype=np.int32), 'confidence': np.empty(K * nv), 'n_people': np.zeros(Cn, dtype=np.int64),
           'series_off': np.zeros(S + 1, dtype=np.int64), 'series_frame': np.empty(nv, dtype=np.int32), 'series_conf': np.empty((K, nv))}
    _lib.check(fn(handle, Cn, _ptr(file_off), _ptr(person_base), _optr(valid), K, _optr(conf), K * nv, S, _ptr(out['row_off']),
                  _optr(out['frame']), _optr(out['person']), _optr(out['slot']), _optr(out['confidence']), _ptr(out['n_people']),
                  _ptr(out['series_off']), _optr(out['series_frame']), _optr(out['series_conf'])))
    return out


def timeline_rows_host(file_off, person_base, valid, conf):
    """Engine.timeline_rows by the library's host path (no context, no GPU): the same code, for checking it."""
    return _timeline_rows(_lib.load(), None, file_off, person_base, valid, conf)


def write_timeline_csv(path, frame, person, slot, confidence, names, n_threads=0):
    """The reference's confidence_timeline.csv (csv.writer with newline='') by the native writer on host threads
    (p2s_timeline_write_csv): header, then `frame,person,names[slot],repr(confidence)` and \\r\\n for every row."""
    import os
    lib = _lib.load()
    fn = _entry(lib, 'p2s_timeline_write_csv')
    frame, person, slot = (np.ascontiguousarray(v, dtype=np.int32).reshape(-1) for v in (frame, person, slot))
    confidence = np.ascontiguousarray(confidence, dtype=np.float64).reshape(-1)
    if not len(frame) == len(person) == len(slot) == len(confidence):
        raise ValueError('frame, person, slot and confidence must have one entry a row')
    enc = [n.encode() for n in names]
    off = _offsets([len(e) for e in enc])
    _lib.check(fn(os.fsencode(path), len(frame), _optr(frame), _optr(person), _optr(slot), _optr(confidence), len(enc), b''.join(enc),
                  _ptr(off), int(n_threads)))


def _refine_extrinsics(lib, handle, xyl, K, R, t, X0, lik_thr, huber_px, min_cams, max_iter, ftol):
    fn = _entry(lib, 'p2s_refine_extrinsics_host')
    xyl = np.asarray(xyl)
    if xyl.ndim < 3 or xyl.shape[-1] != 3:
        raise P2sError(f'xyl has shape {xyl.shape}; expected [..., C, K, 3]')
    Cn, Kn = xyl.shape[-3], xyl.shape[-2]
    dtype = P2S_F32 if xyl.dtype == np.float32 else P2S_F64
    # [..., C, K, 3] -> [points = (..., K)][C][3], the library's layout
    pts = np.ascontiguousarray(np.moveaxis(xyl.reshape((-1, Cn, Kn, 3)), 1, 2).reshape(-1, Cn, 3),
                               dtype=np.float32 if dtype == P2S_F32 else np.float64)
    N = pts.shape[0]
    K, R = (np.ascontiguousarray(np.asarray(v, dtype=np.float64).reshape(-1, 9)) for v in (K, R))
    t = np.ascontiguousarray(np.asarray(t, dtype=np.float64).reshape(-1, 3))
    X0 = np.ascontiguousarray(np.asarray(X0, dtype=np.float64).reshape(-1, 3))
    if not (len(K) == len(R) == len(t) == Cn):
        raise P2sError(f'K, R and t hold {len(K)}, {len(R)} and {len(t)} cameras; xyl has {Cn}')
    if len(X0) != N:
        raise P2sError(f'X0 holds {len(X0)} points; xyl has {N}')
    prm = _lib.RefineParams(float(lik_thr), float(huber_px), float(ftol), int(min_cams), int(max_iter))
    rep = _lib.RefineReport()
    R_out, t_out, X_out = np.empty((Cn, 3, 3)), np.empty((Cn, 3)), np.empty((N, 3))
    _lib.check(fn(handle, N, Cn, dtype, _ptr(pts), _ptr(K), _ptr(R), _ptr(t), _ptr(X0), C.byref(prm), _ptr(R_out), _ptr(t_out),
                  _ptr(X_out), C.byref(rep)))
    report = {'cost_before': rep.cost_before, 'cost_after': rep.cost_after, 'iterations': rep.iterations, 'accepted': rep.accepted,
              'lambda': rep.lambda_final, 'kept_points': rep.kept_points, 'held_coord': rep.held_coord,
              'rms_before': np.array(rep.rms_before[:Cn]), 'rms_after': np.array(rep.rms_after[:Cn])}
    return R_out, t_out, X_out.reshape(xyl.shape[:-3] + (Kn, 3)), report


def refine_extrinsics_host(xyl, K, R, t, X0, lik_thr=0.3, huber_px=3.0, min_cams=2, max_iter=100, ftol=1e-12):
    """Engine.refine_extrinsics with the library's host path (no GPU): the same per-point functions, pass after pass."""
    return _refine_extrinsics(_lib.load(), None, xyl, K, R, t, X0, lik_thr, huber_px, min_cams, max_iter, ftol)


def refine_held_coord(R, t):
    """The coordinate of camera 1's translation that refine_extrinsics holds: argmax_j |(t1 - R1 R0^T t0)_j|, the first
    index on ties (host arithmetic of the library)."""
    R = np.ascontiguousarray(np.asarray(R, dtype=np.float64).reshape(-1, 9)[:2])
    t = np.ascontiguousarray(np.asarray(t, dtype=np.float64).reshape(-1, 3)[:2])
    if len(R) < 2 or len(t) < 2:
        raise P2sError('the gauge needs two cameras')
    j = C.c_int32(-1)
    _lib.check(_entry(_lib.load(), 'p2s_refine_held_coord')(_ptr(R), _ptr(t), C.byref(j)))
    return j.value


def _relative_poses(lib, handle, xn, usable, pairs, samples, thr2, rounds, all_hypotheses, score_points):
    fn = _entry(lib, 'p2s_relative_poses_host')
    xn = np.ascontiguousarray(xn, dtype=np.float64)
    if xn.ndim != 3 or xn.shape[-1] != 2:
        raise P2sError(f'xn has shape {xn.shape}; expected [C][N][2]')
    Cn, N = xn.shape[:2]
    usable = np.ascontiguousarray(np.asarray(usable) != 0, dtype=np.uint8)
    pairs = np.ascontiguousarray(pairs, dtype=np.int32).reshape(-1, 2)
    samples = np.ascontiguousarray(samples, dtype=np.int32)
    P = len(pairs)
    thr2 = _per(thr2, P)
    if usable.shape != (Cn, N):
        raise P2sError(f'usable has shape {usable.shape}; expected {(Cn, N)}')
    if samples.ndim != 3 or samples.shape[0] != P:
        raise P2sError(f'samples has shape {samples.shape}; expected [{P}][H][m]')
    H, m = samples.shape[1:]
    out = {'E': np.empty((P, 3, 3)), 'R': np.empty((P, 3, 3)), 't': np.empty((P, 3)), 'cost': np.empty(P), 'inliers': np.empty(P, dtype=np.int32),
           'front': np.empty(P, dtype=np.int32), 'winner': np.empty(P, dtype=np.int32), 'refits': np.empty(P, dtype=np.int32),
           'mask': np.empty((P, N), dtype=np.uint8)}
    if all_hypotheses:
        out.update(hyp_E=np.empty((P, H, 3, 3)), hyp_cost=np.empty((P, H)), hyp_inliers=np.empty((P, H), dtype=np.int32))
    _lib.check(fn(handle, Cn, N, _ptr(xn), _ptr(usable), P, _ptr(pairs), H, m, _ptr(samples), _ptr(thr2), int(rounds), int(score_points),
                  *[_ptr(out[k]) for k in ('E', 'R', 't', 'cost', 'inliers', 'front', 'winner', 'refits', 'mask')],
                  *[_ptr(out.get(k)) for k in ('hyp_E', 'hyp_cost', 'hyp_inliers')]))
    out['mask'] = out['mask'].view(bool)
    return out


def relative_poses_host(xn, usable, pairs, samples, thr2, rounds=3, all_hypotheses=False, score_points=0):
    """Engine.relative_poses with the library's host path (no GPU): the same per-hypothesis and per-point functions."""
    return _relative_poses(_lib.load(), None, xn, usable, pairs, samples, thr2, rounds, all_hypotheses, score_points)


def _fit_planes(lib, handle, points, usable, ref, samples, thr, rounds, all_hypotheses):
    fn = _entry(lib, 'p2s_fit_planes_host')
    points = np.ascontiguousarray(points, dtype=np.float64)
    if points.ndim != 3 or points.shape[-1] != 3:
        raise P2sError(f'points has shape {points.shape}; expected [B][N][3]')
    B, N = points.shape[:2]
    usable = np.ascontiguousarray(np.asarray(usable) != 0, dtype=np.uint8)
    ref = np.ascontiguousarray(ref, dtype=np.float64)
    samples = np.ascontiguousarray(samples, dtype=np.int32)
    thr = _per(thr, B)
    if usable.shape != (B, N):
        raise P2sError(f'usable has shape {usable.shape}; expected {(B, N)}')
    if ref.shape != (B, 3):
        raise P2sError(f'ref has shape {ref.shape}; expected {(B, 3)}')
    if samples.ndim != 3 or samples.shape[0] != B or samples.shape[2] != 3:
        raise P2sError(f'samples has shape {samples.shape}; expected [{B}][H][3]')
    H = samples.shape[1]
    out = {'plane': np.empty((B, 4)), 'cost': np.empty(B), 'inliers': np.empty(B, dtype=np.int32), 'below': np.empty(B, dtype=np.int32),
           'winner': np.empty(B, dtype=np.int32), 'refits': np.empty(B, dtype=np.int32), 'centroid': np.empty((B, 3)), 'evals': np.empty((B, 3)),
           'mask': np.empty((B, N), dtype=np.uint8)}
    if all_hypotheses:
        out.update(hyp_plane=np.empty((B, H, 4)), hyp_cost=np.empty((B, H)), hyp_inliers=np.empty((B, H), dtype=np.int32))
    _lib.check(fn(handle, B, N, _ptr(points), _ptr(usable), _ptr(ref), H, _ptr(samples), _ptr(thr), int(rounds),
                  *[_ptr(out[k]) for k in ('plane', 'cost', 'inliers', 'below', 'winner', 'refits', 'centroid', 'evals', 'mask')],
                  *[_ptr(out.get(k)) for k in ('hyp_plane', 'hyp_cost', 'hyp_inliers')]))
    out['mask'] = out['mask'].view(bool)
    return out


def fit_planes_host(points, usable, ref, samples, thr, rounds=3, all_hypotheses=False):
    """Engine.fit_planes with the library's host path (no GPU): the same per-hypothesis and per-point functions."""
    return _fit_planes(_lib.load(), None, points, usable, ref, samples, thr, rounds, all_hypotheses)


class Engine:
    def __init__(self, device=0):
        self._lib = _lib.load()
        h = C.c_void_p()
        _lib.check(self._lib.p2s_create(int(device), C.byref(h)))
        self._h = h
        self.device = int(device)
        self.n_cams = 0

    def close(self):
        if getattr(self, '_h', None):
            self._lib.p2s_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # -- calibration -----------------------------------------------------------------------
    def set_calibration(self, P, cal=None):
        """P: C projection matrices (3x4).  cal: dict with 'K', 'dist', 'R_mat', 'T', 'optim_K'
        lists (retrieve_calib_params, common.py:254-288) -- needed for undistortion / association."""
        P = np.ascontiguousarray(np.asarray(P, dtype=np.float64).reshape(-1, 12))
        n = P.shape[0]
        args = [None] * 5
        keep = [P]
        if cal is not None:
            K, d, R, T = _cal_arrays(cal, n)
            nk = np.ascontiguousarray(np.asarray(cal['optim_K'], dtype=np.float64).reshape(n, 9))
            keep += [K, d, R, T, nk]
            args = [_ptr(K), _ptr(d), _ptr(R), _ptr(T), _ptr(nk)]
        _lib.check(self._lib.p2s_set_calibration(self._h, n, _ptr(P), *args))
        self.n_cams = n

    def set_stream(self, stream_handle):
        """Enqueue on this HIP stream (0 / None = HIP's default stream, which is torch's default)."""
        _lib.check(self._lib.p2s_set_stream(self._h, C.c_void_p(int(stream_handle or 0))))

    def synchronize(self):
        _lib.check(self._lib.p2s_synchronize(self._h))

    # p2s_set_tuning keys (include/p2s.h): experiments and tests only, results never depend on them
    TUNE_TRI_PATH, TUNE_FORCE_TILED, TUNE_NO_OVERLAP, TUNE_SEARCH_JOB, TUNE_DIAG_MODE, TUNE_MAX_SUBSETS, TUNE_DEEP_MIN_SUBSETS = 1, 2, 3, 4, 5, 6, 7
    TUNE_ASSOC_FORM, TUNE_POOL_SINGLES_PCT, TUNE_DEEP_PRUNE, TUNE_SCREEN, TUNE_POOL_TILES, TUNE_GAPS_WORKSPACE_KB = 8, 9, 10, 11, 12, 13
    TUNE_POISON_STAGING = 14
    TRI_PATH_AUTO, TRI_PATH_WORKLIST, TRI_PATH_ONE_TILE, TRI_PATH_POOLED, TRI_PATH_TWO_TILES = 0, 1, 2, 3, 4
    ASSOC_FORM_AUTO, ASSOC_FORM_GENERAL = 0, 1

    def tri_stats(self, reset=False):
        """Counters of this engine's triangulation calls: units that entered the camera-subset search, subsets
        evaluated (fp64), 64-lane evaluation passes, units stopped by the 2^26-subsets-per-level safety valve, the pruned
        passes' per-camera errors and candidates, subsets looked at by the pooled kernel's fp32 screen and its passes."""
        out = np.zeros(8, dtype=np.uint64)
        _lib.check(self._lib.p2s_get_tri_stats(self._h, _ptr(out), 1 if reset else 0))
        return {'search_units': int(out[0]), 'subsets_evaluated': int(out[1]), 'passes': int(out[2]), 'capped_units': int(out[3]),
                'pruned_camera_errors': int(out[4]), 'pruned_subsets': int(out[5]),
                'screened_subsets': int(out[6]), 'screen_passes': int(out[7])}

    def assoc_stats(self, reset=False):
        """Counters of this engine's multi-person association calls: frames with detections, ADMM passes, Jacobi sweeps,
        fp64 operations (the kernels' own count)."""
        out = np.zeros(4, dtype=np.uint64)
        _lib.check(self._lib.p2s_get_assoc_stats(self._h, _ptr(out), 1 if reset else 0))
        return {'frames': int(out[0]), 'admm_passes': int(out[1]), 'jacobi_sweeps': int(out[2]), 'fp64_flops': int(out[3])}

    def set_tuning(self, key, value):
        _lib.check(self._lib.p2s_set_tuning(self._h, int(key), int(value)))

    # -- triangulation ---------------------------------------------------------------------
    @staticmethod
    def tri_params(thr, lik_thr, min_cams, undistort=False, lr_swap=False):
        return TriParams(float(thr), float(lik_thr), int(min_cams), int(bool(undistort)), int(bool(lr_swap)), 0)

    def triangulate(self, xyl, params, swap_idx=None):
        """xyl: [..., C, K, 3] float32/float64 host array (leading dims = frames x persons).
        Returns Q [..., K, 3] f64, err [..., K] f32, n_excl [..., K] u8, mask [..., K] u32."""
        xyl, dtype = as_packed(xyl)
        Cn, K = xyl.shape[-3], xyl.shape[-2]
        if Cn != self.n_cams or xyl.shape[-1] != 3:
            raise P2sError(f'xyl has shape {xyl.shape}; expected [..., {self.n_cams}, K, 3]')
        lead = xyl.shape[:-3]
        nb = int(np.prod(lead)) if lead else 1
        Q = np.empty((nb, K, 3), dtype=np.float64)
        err = np.empty((nb, K), dtype=np.float32)
        nex = np.empty((nb, K), dtype=np.uint8)
        mask = np.empty((nb, K), dtype=np.uint32)
        sw = None
        if swap_idx is not None:
            sw = np.ascontiguousarray(np.asarray(swap_idx, dtype=np.int32))
            if sw.shape != (K,) or sw.min() < 0 or sw.max() >= K:
                raise P2sError('swap_idx must be K indices in [0, K)')
        _lib.check(self._lib.p2s_triangulate_host(self._h, nb, K, dtype, _ptr(xyl), _ptr(sw), C.byref(params),
                                                  _ptr(Q), _ptr(err), _ptr(nex), _ptr(mask)))
        return (Q.reshape(lead + (K, 3)), err.reshape(lead + (K,)), nex.reshape(lead + (K,)),
                mask.reshape(lead + (K,)))

    def triangulate_packed(self, xyl, params, swap_idx=None, pad_blocks=None):
        """Multi-GPU form of triangulate(): the observations go up, the kernels run, and the results STAY on this GPU
        in one packed uint8 torch tensor (parallel.section_offsets layout, sections sized for pad_blocks >= n_blocks
        blocks, zero beyond this call's blocks) -- the operand of the path's single all-gather.  Returns a
        parallel.PackedDeviceResults."""
        import torch
        from . import parallel
        xyl, dtype = as_packed(xyl)
        Cn, K = xyl.shape[-3], xyl.shape[-2]
        if Cn != self.n_cams or xyl.shape[-1] != 3:
            raise P2sError(f'xyl has shape {xyl.shape}; expected [..., {self.n_cams}, K, 3]')
        nb = int(np.prod(xyl.shape[:-3])) if xyl.ndim > 3 else 1
        pad = nb if pad_blocks is None else int(pad_blocks)
        if pad < nb:
            raise P2sError(f'pad_blocks={pad} < {nb} blocks')
        dev = torch.device('cuda', self.device)
        off_e, off_m, off_n, total = parallel.section_offsets(pad * K)
        with torch.cuda.device(dev):
            stream = torch.cuda.current_stream(dev)
            buf = torch.zeros(max(total, 16), dtype=torch.uint8, device=dev)
            if nb:
                d_x = torch.from_numpy(xyl.reshape(-1)).to(dev)
                d_sw = None
                if swap_idx is not None:
                    d_sw = torch.from_numpy(np.ascontiguousarray(np.asarray(swap_idx, dtype=np.int32))).to(dev)
                self.set_stream(stream.cuda_stream)
                b = buf.data_ptr()
                self.triangulate_device(nb, K, dtype, d_x, d_sw, params, b, b + off_e, b + off_n, b + off_m)
                stream.synchronize()                   # d_x / d_sw may be freed when this returns
        return parallel.PackedDeviceResults(buf, nb, pad, K)

    def triangulate_device(self, n_blocks, K, dtype, d_xyl, d_swap, params, d_Q, d_err, d_nexcl, d_mask):
        """Device-resident operands (tensors or raw pointers); enqueues on the engine's stream."""
        _lib.check(self._lib.p2s_triangulate_device(self._h, int(n_blocks), int(K), int(dtype), _ptr(d_xyl),
                                                    _ptr(d_swap), C.byref(params), _ptr(d_Q), _ptr(d_err),
                                                    _ptr(d_nexcl), _ptr(d_mask)))

    def triangulate_frames(self, xyl, P_frames, params, block_frame=None):
        """Triangulation with per-frame cameras (a moving and / or zooming rig).  xyl: [F, C, K, 3] or [F, persons, C, K, 3]
        float32/float64 host array; P_frames: [Fc, C, 3, 4].  Row f of the leading dimension uses calibration frame f, its
        persons alike; block_frame ([blocks] int64, never decreasing) names the calibration frame of every block instead.
        Needs no set_calibration and leaves it alone.  Returns what triangulate returns."""
        xyl, dtype = as_packed(xyl)
        P = np.ascontiguousarray(P_frames, dtype=np.float64)
        if P.ndim != 4 or P.shape[2:] != (3, 4):
            raise P2sError(f'P_frames has shape {P.shape}; expected [Fc, C, 3, 4]')
        Fc, Cn = P.shape[:2]
        if xyl.ndim not in (4, 5) or xyl.shape[-3] != Cn or xyl.shape[-1] != 3:
            raise P2sError(f'xyl has shape {xyl.shape}; expected [F, {Cn}, K, 3] or [F, persons, {Cn}, K, 3]')
        K = xyl.shape[-2]
        lead = xyl.shape[:-3]
        nb = int(np.prod(lead))
        if block_frame is None:
            block_frame = np.repeat(np.arange(lead[0], dtype=np.int64), nb // lead[0] if lead[0] else 0)
        bf = np.ascontiguousarray(np.asarray(block_frame).reshape(-1), dtype=np.int64)
        if bf.shape != (nb,):
            raise P2sError(f'block_frame has {bf.size} entries; expected one per block, {nb}')
        Q = np.empty((nb, K, 3), dtype=np.float64)
        err = np.empty((nb, K), dtype=np.float32)
        nex = np.empty((nb, K), dtype=np.uint8)
        mask = np.empty((nb, K), dtype=np.uint32)
        _lib.check(_entry(self._lib, 'p2s_triangulate_frames_host')(self._h, Fc, Cn, _ptr(P), nb, K, dtype, _ptr(xyl), _ptr(bf),
                                                                    C.byref(params), _ptr(Q), _ptr(err), _ptr(nex), _ptr(mask)))
        return (Q.reshape(lead + (K, 3)), err.reshape(lead + (K,)), nex.reshape(lead + (K,)), mask.reshape(lead + (K,)))

    def triangulate_frames_device(self, n_cal_frames, n_cams, d_P, n_blocks, K, dtype, d_xyl, d_block_frame, params, d_Q, d_err,
                                  d_nexcl, d_mask):
        """Device-resident operands (tensors or raw pointers); enqueues on the engine's stream after reading
        d_block_frame back once."""
        _lib.check(_entry(self._lib, 'p2s_triangulate_frames_device')(self._h, int(n_cal_frames), int(n_cams), _ptr(d_P), int(n_blocks),
                                                                      int(K), int(dtype), _ptr(d_xyl), _ptr(d_block_frame),
                                                                      C.byref(params), _ptr(d_Q), _ptr(d_err), _ptr(d_nexcl),
                                                                      _ptr(d_mask)))

    def timing_begin(self):
        _lib.check(self._lib.p2s_timing_begin(self._h))

    def timing_end(self):
        ms = C.c_float(0)
        _lib.check(self._lib.p2s_timing_end(self._h, C.byref(ms)))
        return ms.value

    def tri_geometry(self, K, dtype=P2S_F32):
        fb, th, lds = C.c_int32(), C.c_int32(), C.c_int32()
        _lib.check(self._lib.p2s_tri_geometry(self.n_cams, int(K), int(dtype), C.byref(fb), C.byref(th), C.byref(lds)))
        return {'blocks_per_tile': fb.value, 'threads': th.value, 'lds_bytes': lds.value}

    # -- downstream of the .trc -----------------------------------------
    def butterworth(self, data, b, a, zi):
        """Zero-phase Butterworth filter of every column of data [n_frames][n_cols] (filtering.py:437-471)."""
        data = _matrix(data)
        b, a, zi = _coeffs(b, a, zi)
        out = np.empty_like(data)
        _lib.check(self._lib.p2s_butterworth_host(self._h, data.shape[0], data.shape[1], _optr(data), len(b), _ptr(b), _ptr(a),
                                                  _ptr(zi), _optr(out)))
        return out

    def filter_columns(self, kind, data, params):
        """One of the window / recurrence filters of filtering.py on every column of data [n_frames][n_cols]
        (include/p2s.h: P2S_FILTER_HAMPEL = 1, _GAUSSIAN = 2, _MEDIAN = 3, _ONE_EURO = 4, _KALMAN = 5, with their
        parameters)."""
        data = _matrix(data)
        params = np.ascontiguousarray(params, dtype=np.float64).reshape(-1)
        out = np.empty_like(data)
        _lib.check(self._lib.p2s_filter_columns_host(self._h, int(kind), data.shape[0], data.shape[1], _optr(data), _optr(params),
                                                     params.size, _optr(out)))
        return out

    _GCV_ERRORS = {_lib.P2S_ERR_GCV_SHORT_RUN: ValueError, _lib.P2S_ERR_GCV_ILL_POSED: ValueError,
                   _lib.P2S_ERR_GCV_NO_MINIMUM: ValueError, _lib.P2S_ERR_GCV_SINGULAR: np.linalg.LinAlgError}

    def gcv_spline(self, data, cutoff='auto', smoothing_factor=1.0, frame_rate=None):
        """gcv_spline_filter_1d (filtering.py:163-313) on every column of data [n_frames][n_cols]: a natural cubic
        smoothing spline through every run of >= 5 valid samples, lambda chosen by GCV (cutoff 'auto') or
        (frame_rate / (2 pi cutoff))^4, times smoothing_factor either way.  Returns (out, lam): the filtered matrix and
        [n_frames][n_cols] the lambda of the fit at the first sample of every filtered run, NaN elsewhere.  Failures
        raise what the reference raises: ValueError (a run of 2 to 4 samples, an ill-posed problem, a search without a
        minimum, a negative lambda), numpy.linalg.LinAlgError (a singular system)."""
        fn = _entry(self._lib, 'p2s_gcv_spline_host')
        data = _matrix(data)
        auto = cutoff == 'auto'
        lam = 0.0 if auto else float((frame_rate / (2 * np.pi * float(cutoff))) ** 4)     # filtering.py:301
        out = np.empty_like(data)
        lam_out = np.full(data.shape, np.nan)
        rc = fn(self._h, data.shape[0], data.shape[1], _optr(data), 1 if auto else 0, lam, float(smoothing_factor), _optr(out),
                _optr(lam_out))
        if rc in self._GCV_ERRORS:
            raise self._GCV_ERRORS[rc](self._lib.p2s_last_error().decode())
        if rc == _lib.P2S_ERR_INVALID_ARG and self._lib.p2s_last_error().decode() == 'Regularization parameter should be non-negative':
            raise ValueError('Regularization parameter should be non-negative')
        _lib.check(rc)
        return out, lam_out

    def loess(self, data, nb_values_used):
        """loess_filter_1d (filtering.py:532-558) on every column of data [n_frames][n_cols]: every run of more than
        nb_values_used consecutive non-NaN samples (zeros are data) is replaced by its local linear regression over the
        k = int(nb_values_used + 1e-10) nearest samples with tricube weights -- statsmodels' lowess with
        frac = nb_values_used / len(run), it = 0 -- and every other sample is copied.  nb_values_used < 2 raises
        ValueError: a window of one sample has radius 0."""
        fn = _entry(self._lib, 'p2s_loess_host')
        data = _matrix(data)
        k, min_run = loess_window(nb_values_used)
        out = np.empty_like(data)
        _lib.check(fn(self._h, data.shape[0], data.shape[1], _optr(data), k, min_run, _optr(out)))
        return out

    def trc_metrics(self, xyz, bones):
        """trc_evaluate's per-frame quantities for xyz [F][K][3] and bones [n][2] (parent, child marker indices):
        bone_len [n][F], bone_stats [n][3] (mean, population sd, n_valid), accel [K][F-2], missing [K]."""
        xyz = np.ascontiguousarray(xyz, dtype=np.float64)
        if xyz.ndim != 3 or xyz.shape[2] != 3:
            raise P2sError(f'xyz has shape {xyz.shape}; expected [F][K][3]')
        bones = np.ascontiguousarray(np.asarray(bones, dtype=np.int32).reshape(-1, 2))
        F, K = xyz.shape[:2]
        nb = bones.shape[0]
        bone_len = np.full((nb, F), np.nan)
        bone_stats = np.full((nb, 3), np.nan)
        accel = np.full((K, max(F - 2, 0)), np.nan)
        missing = np.zeros(K, dtype=np.int64)
        _lib.check(self._lib.p2s_trc_metrics_host(self._h, F, K, _optr(xyz), nb, _optr(bones), _optr(bone_len), _optr(bone_stats),
                                                  _optr(accel), _optr(missing)))
        return bone_len, bone_stats, accel, missing

    # -- a .trc back onto the image planes (Utilities/reproj_from_trc_calib.py:446-475) --------------------------------
    def reproject(self, Q, P=None, cal=None, sizes=None, raw=False):
        """Q [F][K][3] (Z-up X, Y, Z; NaN = missing) onto C cameras.  Either P [C][Fp][3][4] (or [C][3][4]) with Fp = 1
        or F -- the pinhole projection, one matrix per frame for moving / zooming cameras -- or cal, a dict with 'K',
        'dist' (k1, k2, p1, p2[, k3]), 'R_mat' and 'T' per camera: cv2.projectPoints with distortion, static cameras.
        sizes [C][2] (width, height).  -> uv [C][F][K][2] rounded to one decimal with NaN outside the image, as the
        reference stores it; with raw=True (uv, uv_raw), uv_raw being the pixels as computed."""
        fn = _entry(self._lib, 'p2s_reproject_host')
        Q = np.ascontiguousarray(Q, dtype=np.float64)
        if Q.ndim != 3 or Q.shape[2] != 3:
            raise P2sError(f'Q has shape {Q.shape}; expected [F][K][3]')
        if (P is None) == (cal is None):
            raise P2sError('give either P (pinhole) or cal (distorted), not both')
        F, K = Q.shape[:2]
        args = [None] * 5
        if cal is None:
            P = np.asarray(P, dtype=np.float64)
            if P.ndim == 3:
                P = P[:, None]
            if P.ndim != 4 or P.shape[2:] != (3, 4):
                raise P2sError(f'P has shape {P.shape}; expected [C][Fp][3][4]')
            P = np.ascontiguousarray(P)
            Cn, Fp = P.shape[:2]
            args[0] = _ptr(P)
            flags = 0
        else:
            Cn, Fp = len(cal['K']), 1
            keep = _cal_arrays(cal, Cn)
            args[1:] = [_ptr(x) for x in keep]
            flags = _lib.P2S_REPROJ_DISTORTED
        sizes = np.ascontiguousarray(sizes, dtype=np.float64)
        if sizes.shape != (Cn, 2):
            raise P2sError(f'sizes has shape {sizes.shape}; expected [{Cn}][2]')
        uv = np.empty((Cn, F, K, 2))
        uv_raw = np.empty((Cn, F, K, 2)) if raw else None
        _lib.check(fn(self._h, F, K, _optr(Q), Cn, Fp, *args, _ptr(sizes), flags, _ptr(uv_raw) if raw else None, _ptr(uv)))
        return (uv, uv_raw) if raw else uv

    def reproject_kernel_ms(self):
        """Kernel time of the last reproject() call, from HIP events around it."""
        return _kernel_ms(self, 'reproject')

    def write_openpose_files(self, cam_dirs, name_root, uv, marker_index=None, n_threads=0):
        return write_openpose_files(cam_dirs, name_root, uv, marker_index, n_threads)

    # -- exact order statistics; 2D keypoint jitter (Utilities/keypoint_jitter_analyze.py:143-325) -------------------------
    def column_order_stats(self, data, ranks):
        """data [n_rows][n_cols] float64 (any strides; NaN entries are skipped), ranks: 0-based positions among each
        column's sorted non-NaN entries, negative = from the top.  -> (values [n_cols][n_ranks], NaN where the rank is
        outside the column's count; counts [n_cols] of non-NaN entries).  Exact: a radix select on the bit patterns."""
        fn = _entry(self._lib, 'p2s_column_order_stats_host')
        data = np.asarray(data, dtype=np.float64)
        if data.ndim != 2:
            raise P2sError(f'data has shape {data.shape}; expected [n_rows][n_cols]')
        cols = np.ascontiguousarray(data.T)                       # the library takes the columns contiguous
        ranks = np.ascontiguousarray(ranks, dtype=np.int64).reshape(-1)
        n_cols, n_rows = cols.shape
        out = np.empty((n_cols, len(ranks)))
        counts = np.zeros(n_cols, dtype=np.int64)
        _lib.check(fn(self._h, n_rows, n_cols, _optr(cols), len(ranks), _optr(ranks), _optr(out), _optr(counts)))
        return out, counts

    def jitter(self, series, multiplier=5.0, image_size=(1920, 1080)):
        """series: one [n_frames][26][3] (x, y, confidence) float64 array per camera (lengths may differ, each >= 1).
        -> dict: per camera (lists) 'displacements' [F-1][26] (a transposed view of the keypoint-major table the kernels
        keep), 'bb_areas' [F], 'jitter_mask' [F-1][26] bool, 'medians', 'thresholds' [26], 'median_bb_area', 'counts' [26];
        and 'events' [n][4] int32 (camera, frame, keypoint, pattern 0 A / 1 C / 2 D / 3 E) for all cameras, in the
        reference's order."""
        fn = _entry(self._lib, 'p2s_jitter_host')
        series = [np.ascontiguousarray(s, dtype=np.float64) for s in series]
        for s in series:
            if s.ndim != 3 or s.shape[1:] != (26, 3) or len(s) < 1:
                raise P2sError(f'a series has shape {s.shape}; expected [n_frames >= 1][26][3]')
        Cn = len(series)
        n_frames = np.array([len(s) for s in series], dtype=np.int64)
        flat = series[0] if Cn == 1 else np.concatenate(series)
        frames, rows = int(n_frames.sum()), int(n_frames.sum()) - Cn
        disp, areas = np.empty(rows * 26), np.empty(frames)
        med, thr, med_area = np.empty((Cn, 26)), np.empty((Cn, 26)), np.empty(Cn)
        mask, counts = np.empty((rows, 26), dtype=np.uint8), np.zeros((Cn, 26), dtype=np.int32)
        capacity = min(max(rows, 1) * 26, 1 << 18)
        while True:
            events, found = np.empty((capacity, 4), dtype=np.int32), C.c_int64(0)
            _lib.check(fn(self._h, Cn, _ptr(n_frames), _ptr(flat), float(multiplier), float(image_size[0]), float(image_size[1]),
                          _optr(disp), _ptr(areas), _ptr(med), _ptr(thr), _ptr(med_area), _optr(mask), _ptr(counts), capacity,
                          _ptr(events), C.byref(found)))
            if found.value <= capacity:
                break
            capacity = found.value                                # a second call with room for every event
        f_off = _offsets(n_frames)
        r_off = f_off - np.arange(Cn + 1)
        out = {'displacements': [], 'bb_areas': [], 'jitter_mask': [], 'medians': list(med), 'thresholds': list(thr),
               'median_bb_area': [float(v) for v in med_area], 'counts': list(counts), 'events': events[:found.value]}
        for c in range(Cn):
            R = int(n_frames[c]) - 1
            out['displacements'].append(disp[26 * r_off[c]:26 * r_off[c + 1]].reshape(26, R).T)
            out['bb_areas'].append(areas[f_off[c]:f_off[c + 1]])
            out['jitter_mask'].append(mask[r_off[c]:r_off[c + 1]].view(np.bool_))
        return out

    def jitter_kernel_ms(self):
        """Kernel time of the last jitter() call, from HIP events around its kernels."""
        return _kernel_ms(self, 'jitter')

    # -- scipy.signal.find_peaks; gait contact signals (Utilities/trc_gaitevents.py) ---------------------------------------
    def find_peaks(self, data, prominence=None):
        """scipy.signal.find_peaks(column, prominence=prominence) for every column of data [n_rows][n_cols] float64 (any
        strides), bit for bit; prominence: one bound, or one per column.  -> one (peaks int64, prominences, left_bases
        int64, right_bases int64) per column.  With prominence None every local maximum is returned, with its prominence
        and bases."""
        fn = _entry(self._lib, 'p2s_find_peaks_host')
        data = np.asarray(data, dtype=np.float64)
        if data.ndim != 2 or data.shape[0] < 1 or data.shape[1] < 1:
            raise P2sError(f'data has shape {data.shape}; expected [n_rows >= 1][n_cols >= 1]')
        cols = np.ascontiguousarray(data.T)                       # the library takes the columns contiguous
        n_cols, n_rows = cols.shape
        bound = None if prominence is None else _per(prominence, n_cols)
        capacity = min(max(cols.size // 16, 64), 1 << 22)
        counts, found = np.zeros(n_cols, dtype=np.int32), C.c_int64(0)
        while True:
            peaks, lb, rb = (np.empty(capacity, dtype=np.int64) for _ in range(3))
            prom = np.empty(capacity)
            _lib.check(fn(self._h, n_rows, n_cols, _ptr(cols), _ptr(bound), capacity, _ptr(peaks), _ptr(prom), _ptr(lb), _ptr(rb),
                          _ptr(counts), C.byref(found)))
            if found.value <= capacity:
                break
            capacity = found.value                                # a second call with room for every peak
        off = _offsets(counts)
        return [(peaks[off[c]:off[c + 1]], prom[off[c]:off[c + 1]], lb[off[c]:off[c + 1]], rb[off[c]:off[c + 1]]) for c in range(n_cols)]

    GAIT_METHODS = {'height_coordinates': 0, 'forward_velocity': 1}

    def gait_contacts(self, columns, method, dt, threshold, factor=1.0, sign=1, b=None, a=None, zi=None, weights=None):
        """The contact signal of trc_gaitevents' two threshold methods and its runs, for a batch of toe columns at once.
        columns: 1-D float64 arrays, lengths may differ; dt, threshold, factor: one value or one per column.
        'height_coordinates': scipy.signal.filtfilt(b, a, (factor * column)[1:]) over the whole column, zi =
        lfilter_zi(b, a); a column too short for its padding raises scipy's ValueError.  'forward_velocity': diff / dt,
        the samples whose sign is not `sign` zeroed, abs, [1:], correlate1d with `weights` (gaussian_filter1d's, from the
        host), mode 'reflect'.  -> (signals, on, off, first_low): per column the filtered signal (one sample fewer than
        the column), the run starts of signal < threshold with index 0 taken off, the run ends, and whether the first
        sample is below the threshold (with no run end: start_end_true_seq raises on such a column)."""
        fn = _entry(self._lib, 'p2s_gait_contacts_host')
        if method not in self.GAIT_METHODS:
            raise P2sError(f'method {method!r}; expected one of {sorted(self.GAIT_METHODS)}')
        m = self.GAIT_METHODS[method]
        columns = [np.asarray(c, dtype=np.float64).reshape(-1) for c in columns]
        n = len(columns)
        if n < 1 or min(len(c) for c in columns) < 1:
            raise P2sError('gait_contacts: at least one column, every column with at least one sample')
        lens = np.array([len(c) for c in columns], dtype=np.int64)
        max_rows = int(lens.max())
        dt, threshold, factor = _per(dt, n), _per(threshold, n), _per(factor, n)
        n_coef = n_w = 0
        if m == 0:
            b, a, zi = _coeffs(b, a, zi)
            n_coef = len(b)
            if int(lens.min()) - 1 <= 3 * n_coef:                 # scipy.signal.filtfilt's own refusal (_validate_pad)
                raise ValueError(f'The length of the input vector x must be greater than padlen, which is {3 * n_coef}.')
        else:
            weights = np.ascontiguousarray(weights, dtype=np.float64).reshape(-1)
            n_w = len(weights)
        table = np.full((max_rows, n), np.nan)
        for c, col in enumerate(columns):
            table[:len(col), c] = col
        signal = np.empty((max_rows - 1, n))
        n_on, n_off, first = np.zeros(n, dtype=np.int32), np.zeros(n, dtype=np.int32), np.zeros(n, dtype=np.uint8)
        capacity = 256
        while True:
            on, off = np.empty((n, capacity), dtype=np.int32), np.empty((n, capacity), dtype=np.int32)
            _lib.check(fn(self._h, m, n, max_rows, _ptr(lens), _ptr(table), _ptr(dt), _ptr(threshold), _ptr(factor), int(sign),
                          n_coef, _ptr(b) if m == 0 else None, _ptr(a) if m == 0 else None, _ptr(zi) if m == 0 else None,
                          n_w, _ptr(weights) if m == 1 else None, _optr(signal), capacity, _ptr(on), _ptr(off), _ptr(n_on),
                          _ptr(n_off), _ptr(first)))
            need = int(max(n_on.max(), n_off.max()))
            if need <= capacity:
                break
            capacity = need                                       # a second call with room for every event
        return ([signal[:lens[c] - 1, c] for c in range(n)], [on[c, :n_on[c]].astype(np.int64) for c in range(n)],
                [off[c, :n_off[c]].astype(np.int64) for c in range(n)], first.astype(bool))

    def gait_kernel_ms(self):
        """Kernel time of the last find_peaks() or gait_contacts() call, from HIP events around its kernels."""
        return _kernel_ms(self, 'gait')

    # -- stable sort, trimmed means, body measurements (common.py:378-455, :715-1034) ---------------------------------------
    @staticmethod
    def _segments(columns, what):
        columns = [np.asarray(c, dtype=np.float64).reshape(-1) for c in columns]
        if not columns or min(len(c) for c in columns) < 1:
            raise P2sError(f'{what}: at least one column, every column with at least one entry')
        return columns, np.array([len(c) for c in columns], dtype=np.int64), np.ascontiguousarray(np.concatenate(columns))

    def stable_argsort(self, columns):
        """columns: 1-D float64 arrays, lengths may differ.  -> one int64 order per column, np.argsort(column, kind='stable'):
        -inf < ... < -0.0 = +0.0 < ... < inf < NaN, equal keys in input order.  One device call for the batch."""
        fn = _entry(self._lib, 'p2s_stable_argsort_host')
        columns, lens, data = self._segments(columns, 'stable_argsort')
        order = np.empty(len(data), dtype=np.int32)
        _lib.check(fn(self._h, len(columns), _ptr(lens), _ptr(data), _ptr(order)))
        off = _offsets(lens)
        return [order[off[c]:off[c + 1]].astype(np.int64) for c in range(len(columns))]

    def trimmed_means(self, columns, trimmed_extrema_percent=0.5):
        """The reference's trimmed_mean (common.py:427-455) of every column, bit for bit: np.mean(np.sort(x)[int(n * p / 2) :
        int(n * (1 - p / 2))]), np.mean(x) when the slice is empty.  columns: 1-D float64 arrays, lengths may differ.
        -> float64 [n_columns]."""
        fn = _entry(self._lib, 'p2s_trimmed_means_host')
        columns, lens, data = self._segments(columns, 'trimmed_means')
        means = np.empty(len(columns))
        _lib.check(fn(self._h, len(columns), _ptr(lens), _ptr(data), float(trimmed_extrema_percent) / 2, _ptr(means)))
        return means

    def body_measure(self, tables, marker_index, pairs, flags, close_to_zero_speed=0.2, fastest_frames_to_remove_percent=0.2,
                     large_hip_knee_angles=45, trimmed_extrema_percent=0.5, head_factor=1.008, row_values=False, n_speed_markers=None):
        """best_coords_for_measurements, mean_angles, compute_height, compute_leg_length and trimmed segment lengths
        (common.py:797-1034, kinematics.py:299-304) for a batch of tables in one device call.
        tables: [n_rows][3 n_markers] float64 per file, shapes may differ.  marker_index: per file the 10 marker indices
        of _lib.P2S_MEASURE_ROLES, -1 = absent.  pairs: per file [n_pairs][2] marker indices (n_markers = mid-shoulder,
        n_markers + 1 = mid-hip, -1 = skip the pair), n_pairs the same for every file; pairs 0 .. 8 are compute_height's
        (include/p2s.h).  flags: per file, P2S_MEASURE_* of _lib.  close_to_zero_speed, head_factor: one value or one per
        file.  n_speed_markers: per file, the summed speed runs over the table's first so many markers (None: all).  -> one dict per file:
          sum_speeds [n_rows]; n_selected and angles [n_selected]: the mean angles of the speed-selected rows (NaN-filled
          without P2S_MEASURE_ANGLES); kept_pos, kept_frame [n_kept]: the kept rows' places among the selected rows and
          their frames, in the reference's order; all_slow, few_small_angles, all_data: the fallback branch that ran;
          row_heights [n_kept]; height, leg_length; lengths [n_pairs]: the trimmed means; row_values [n_pairs + 2][n_kept]
          when asked for (per-row lengths, heights, leg lengths)."""
        fn = _entry(self._lib, 'p2s_body_measure_host')
        tables = [np.ascontiguousarray(t, dtype=np.float64) for t in tables]
        nf = len(tables)
        if nf < 1 or any(t.ndim != 2 or t.shape[0] < 1 or t.shape[1] < 3 or t.shape[1] % 3 for t in tables):
            raise P2sError('body_measure: at least one table, every table [n_rows >= 1][3 n_markers]')
        n_rows = np.array([t.shape[0] for t in tables], dtype=np.int64)
        n_mk = np.array([t.shape[1] // 3 for t in tables], dtype=np.int32)
        roles = np.ascontiguousarray(marker_index, dtype=np.int32).reshape(nf, len(_lib.P2S_MEASURE_ROLES))
        pairs = np.ascontiguousarray(pairs, dtype=np.int32).reshape(nf, -1, 2)
        n_pairs = pairs.shape[1]
        flags = _per(flags, nf, np.int32)
        thr, head = _per(close_to_zero_speed, nf), _per(head_factor, nf)
        n_speed = None if n_speed_markers is None else _per(n_speed_markers, nf, np.int32)
        data = np.concatenate([t.reshape(-1) for t in tables])
        N, ncol = int(n_rows.sum()), n_pairs + 2
        speeds, angles, heights = np.empty(N), np.empty(N), np.empty(N)
        pos, frame = np.empty(N, dtype=np.int32), np.empty(N, dtype=np.int32)
        n_sel, n_kept, branch = (np.zeros(nf, dtype=np.int32) for _ in range(3))
        values = np.empty((ncol, N)) if row_values else None
        means = np.empty((nf, ncol))
        _lib.check(fn(self._h, nf, _ptr(n_rows), _ptr(n_mk), _ptr(data), _ptr(flags), _ptr(roles), n_pairs, _optr(pairs), _ptr(head),
                      _ptr(thr), _ptr(n_speed), 1 - float(fastest_frames_to_remove_percent), float(large_hip_knee_angles),
                      float(trimmed_extrema_percent) / 2, _ptr(speeds), _ptr(angles), _ptr(n_sel), _ptr(pos), _ptr(frame),
                      _ptr(n_kept), _ptr(branch), _ptr(heights), _ptr(values), _ptr(means)))
        off = _offsets(n_rows)
        out = []
        for f in range(nf):
            o, k = off[f], int(n_kept[f])
            res = {'sum_speeds': speeds[o:off[f + 1]], 'n_selected': int(n_sel[f]),
                   'angles': angles[o:o + n_sel[f]],
                   'kept_pos': pos[o:o + k].astype(np.int64), 'kept_frame': frame[o:o + k].astype(np.int64),
                   'all_slow': bool(branch[f] & _lib.P2S_MEASURE_ALL_SLOW),
                   'few_small_angles': bool(branch[f] & _lib.P2S_MEASURE_FEW_SMALL_ANGLES),
                   'all_data': bool(branch[f] & _lib.P2S_MEASURE_ALL_DATA),
                   'row_heights': heights[o:o + k], 'height': means[f, n_pairs], 'leg_length': means[f, n_pairs + 1],
                   'lengths': means[f, :n_pairs]}
            if row_values:
                res['row_values'] = values[:, o:o + k]
            out.append(res)
        return out

    def measure_kernel_ms(self):
        """Kernel time of the last stable_argsort(), trimmed_means() or body_measure() call, from HIP events around its
        kernels."""
        return _kernel_ms(self, 'measure')

    # -- np.mean / np.std of columns; 2D confidence statistics (Utilities/pose_confidence_analyze.py:118-219) ------------
    def column_mean_std(self, data):
        """data [n_rows][n_cols] float64 (any strides; NaN entries are skipped).  -> (mean [n_cols], std [n_cols], counts
        [n_cols]): np.mean and np.std of every column's non-NaN entries in row order, bit for bit (NumPy's own summation
        order), NaN for a column without entries."""
        fn = _entry(self._lib, 'p2s_column_mean_std_host')
        data = np.asarray(data, dtype=np.float64)
        if data.ndim != 2:
            raise P2sError(f'data has shape {data.shape}; expected [n_rows][n_cols]')
        cols = np.ascontiguousarray(data.T)                       # the library takes the columns contiguous
        n_cols, n_rows = cols.shape
        mean, std = np.empty(n_cols), np.empty(n_cols)
        counts = np.zeros(n_cols, dtype=np.int64)
        _lib.check(fn(self._h, n_rows, n_cols, _optr(cols), _optr(mean), _optr(std), _optr(counts)))
        return mean, std, counts

    CONFIDENCE_STATS = ('mean', 'median', 'std', 'min', 'max', 'p5', 'p25', 'p75', 'p95')
    CONFIDENCE_BANDS = ('low', 'danger', 'medium', 'high', 'very_high')

    def confidence_stats(self, tables, thresholds=(0.4,)):
        """tables: one [n_frames][K] float64 confidence table per camera (NaN rows = no person; lengths may differ, each
        >= 1; K <= 64), thresholds: up to 8.  Per (camera, keypoint) over the non-NaN entries in frame order -> dict:
        'stats' [C][K][9] (CONFIDENCE_STATS: np.mean, np.median, np.std, min, max, np.percentile 5 / 25 / 75 / 95; NaN
        without entries), 'counts' [C][K] int64, 'below' [T][C][K] int64 entries < threshold, 'below_rate' [T][C][K]
        (NaN without entries), 'bands' [C][K][5] int64 (CONFIDENCE_BANDS: [0, 0.4), [0.4, 0.6), [0.6, 0.8), [0.8, 1.0]
        closed, [1.0, inf)), 'band_rate' [C][K][5] (0.0 without entries)."""
        fn = _entry(self._lib, 'p2s_confidence_stats_host')
        tables = [np.ascontiguousarray(t, dtype=np.float64) for t in tables]
        if not tables or any(t.ndim != 2 or t.shape[1] != tables[0].shape[1] or len(t) < 1 for t in tables):
            raise P2sError('every camera needs an [n_frames >= 1][K] table with the same K')
        Cn, K = len(tables), tables[0].shape[1]
        n_frames = np.array([len(t) for t in tables], dtype=np.int64)
        flat = tables[0] if Cn == 1 else np.concatenate(tables)
        thr = np.ascontiguousarray(thresholds, dtype=np.float64).reshape(-1)
        stats = np.empty((Cn, K, 9))
        counts = np.zeros((Cn, K), dtype=np.int64)
        below = np.zeros((len(thr), Cn, K), dtype=np.int64)
        bands = np.zeros((Cn, K, 5), dtype=np.int64)
        _lib.check(fn(self._h, Cn, _ptr(n_frames), K, _optr(flat), len(thr), _optr(thr), _optr(stats), _optr(counts), _optr(below),
                      _optr(bands)))
        with np.errstate(invalid='ignore', divide='ignore'):
            below_rate = below / counts                           # int64 / int64: the correctly rounded quotient, 0 / 0 = NaN
            band_rate = np.where(counts[:, :, None] > 0, bands / counts[:, :, None], 0.0)
        return {'stats': stats, 'counts': counts, 'below': below, 'below_rate': below_rate, 'bands': bands, 'band_rate': band_rate}

    def confidence_kernel_ms(self):
        """Kernel time of the last confidence_stats() call, from HIP events around its kernels."""
        return _kernel_ms(self, 'confidence')

    # -- linear_sum_assignment; frame-to-frame person matching (Utilities/id_switch_analyze.py:47-145, 148-291, 364-388) --
    def lsap(self, cost):
        """cost: [n][n_rows][n_cols] (or one [n_rows][n_cols]) float64 matrices of one shape, up to 32 x 32.  ->
        (row_ind, col_ind) [n][min(n_rows, n_cols)] int32 (or one pair of vectors): scipy.optimize.linear_sum_assignment of
        every matrix, solved on the GPU, exactly scipy's answer with its ties.  A matrix scipy refuses raises scipy's
        ValueError."""
        fn = _entry(self._lib, 'p2s_lsap_host')
        cost = np.ascontiguousarray(cost, dtype=np.float64)
        single = cost.ndim == 2
        if single:
            cost = cost[None]
        if cost.ndim != 3 or not (1 <= cost.shape[1] <= _lib.P2S_LSAP_MAX and 1 <= cost.shape[2] <= _lib.P2S_LSAP_MAX):
            raise P2sError(f'cost has shape {cost.shape}; expected [n][1..{_lib.P2S_LSAP_MAX}][1..{_lib.P2S_LSAP_MAX}]')
        n, k = len(cost), min(cost.shape[1:])
        rows, cols = np.empty((n, k), dtype=np.int32), np.empty((n, k), dtype=np.int32)
        status = np.zeros(n, dtype=np.int32)
        _lib.check(fn(self._h, n, cost.shape[1], cost.shape[2], _optr(cost), _optr(rows), _optr(cols), _optr(status)))
        if status.any():
            raise ValueError(_lib.P2S_LSAP_ERRORS[int(status[np.flatnonzero(status)[0]])])
        return (rows[0], cols[0]) if single else (rows, cols)

    ID_SWITCH_TABLES = ('counts', 'prev', 'zero_run', 'n_matched', 'n_lost', 'n_appeared', 'flags')
    ID_SWITCH_STATS = ('mean', 'median', 'p95', 'p99', 'min', 'max')

    def id_switch(self, cameras):
        """cameras: per camera (persons [N][26][3] float64, every listed person of every readable frame in order; offsets
        [n_frames + 1], the first person of every frame).  -> dict of per-camera lists: the per-frame int32 tables
        ID_SWITCH_TABLES ('counts' kept persons, 'prev' the last earlier frame with one or -1, 'zero_run' the empty frames
        between, 'n_matched' / 'n_lost' / 'n_appeared' of the assignment against that frame, 'flags' 0 or why the frame was
        not matched: 1 / 2 scipy's refusals (_lib.P2S_LSAP_ERRORS), 4 more than 32 kept persons), 'distances' the matched
        costs in frame and previous-person order, 'kept' the indices of the kept persons in order; and 'stats' [C][6] (ID_SWITCH_STATS; NaN without distances)."""
        fn = _entry(self._lib, 'p2s_id_switch_host')
        persons, offsets, n_frames, base, off, flat = _pack_persons(cameras, 26)
        Cn, frames, N = len(persons), int(n_frames.sum()), int(base[-1])
        tables = np.zeros((len(self.ID_SWITCH_TABLES), frames), dtype=np.int32)
        dist, n_dist, stats = np.empty(N), np.zeros(Cn, dtype=np.int64), np.empty((Cn, len(self.ID_SWITCH_STATS)))
        slots = np.zeros(N, dtype=np.int32)
        _lib.check(fn(self._h, Cn, _ptr(n_frames), _ptr(off), _optr(flat), _optr(tables), _optr(slots), _optr(dist), _ptr(n_dist),
                      _ptr(stats)))
        f_off = _offsets(n_frames)
        d_off = _offsets(n_dist)
        out = {name: [tables[i, f_off[c]:f_off[c + 1]] for c in range(Cn)] for i, name in enumerate(self.ID_SWITCH_TABLES)}
        out['kept'] = []
        for c in range(Cn):                                       # the frames' runs of kept persons -> one rising index list
            counts, first = out['counts'][c].astype(np.int64), offsets[c][:-1]
            run = np.repeat(first, counts)                        # every kept person's frame's first person
            nth = np.arange(int(counts.sum())) - np.repeat(np.cumsum(counts) - counts, counts)
            out['kept'].append(run + slots[base[c] + run + nth])
        out['distances'] = [dist[d_off[c]:d_off[c + 1]] for c in range(Cn)]
        out['stats'] = stats
        return out

    def id_switch_kernel_ms(self):
        """Kernel time of the last id_switch() call, from HIP events around its kernels."""
        return _kernel_ms(self, 'id_switch')

    # -- primary-person selection (Utilities/pose_extract_person.py:37-87) --------------------------------------------------
    def track_select(self, cameras, n_kpts=26, conf_threshold=0.1):
        """cameras: per camera (persons [N][n_kpts][3] float64, the persons whose list has exactly 3 * n_kpts numbers, of every
        frame in list order; offsets [n_frames + 1], the first person of every frame), as for id_switch.  The reference's
        _select_person along every camera, all cameras in one call and without a loop over the frames (csrc/p2s_extract.hip).
        -> dict of per-camera int32 lists: 'chosen' the selected person as an index into the frame's own run (-1: the frame
        has no candidate), 'n_candidates', 'prev' the last earlier frame with a candidate (-1: none).  More than 32
        candidates in a frame are refused."""
        fn = _entry(self._lib, 'p2s_track_select_host')
        n_kpts = int(n_kpts)
        persons, _, n_frames, _, off, flat = _pack_persons(cameras, max(n_kpts, 1))
        Cn, frames = len(persons), int(n_frames.sum())
        tables = np.zeros((3, frames), dtype=np.int32)
        _lib.check(fn(self._h, Cn, _ptr(n_frames), _ptr(off), _optr(flat), n_kpts, float(conf_threshold), _optr(tables[0]),
                      _optr(tables[1]), _optr(tables[2])))
        f_off = _offsets(n_frames)
        return {name: [tables[i, f_off[c]:f_off[c + 1]] for c in range(Cn)] for i, name in enumerate(('chosen', 'n_candidates', 'prev'))}

    def track_select_kernel_ms(self):
        """Kernel time of the last track_select() call, from HIP events around its kernels."""
        return _kernel_ms(self, 'track_select')

    # -- person tracking across frames (triangulation.py:823-874, common.py:1037-1136) ---------------------------------------
    def track_persons_3d(self, Q, first_frame=0, max_dist=None, state=None):
        """Q: one trial [F][P][K][3] float64 of triangulated points (NaN = none), or a list of trials of one P <= 32 and K
        (lengths may differ); first_frame: the absolute number of the trial's first frame (one, or one per trial: frame 0 is
        not matched); max_dist: the reference's max_distance_m; state: the `state` of an earlier call ([n][K][3], n <= 32,
        per trial), to continue a trial in chunks.  The reference's frame-by-frame sort_people_sports2d, every trial a
        workgroup of one launch (csrc/p2s_track.hip).  -> (Q_rows [F][P][K][3] the points in tracked order, ids [F][P] int32
        the detection every slot took or -1, matched_dist [F][P] the mean keypoint distance of every kept pair or NaN,
        n_slots [F] int32, state [n][K][3], status [2] int32: zeros, or (the first frame, plus 1, that would have passed 32
        slots, the assignment's refusal if that stopped it) -- from that frame on the library writes nothing, and the rows are NaN, the
        ids -1, matched_dist NaN and n_slots 0), each a list for a list of trials.  A shape the kernel does not take raises TrackShapeError."""
        return _track_persons(self._lib, self._h, Q, first_frame, max_dist, state)

    def track_persons_3d_device(self, frame_off, first_frame, P, K, d_Q, max_dist=None, d_state_in=None, d_n_state_in=None, d_ids=None,
                                d_Q_rows=None, d_matched_dist=None, d_n_slots=None, d_state_out=None, d_n_state_out=None, d_status=None):
        """Device-resident form (tensors or raw pointers; frame_off [T + 1] and first_frame [T] are host int64 arrays):
        enqueues on the engine's stream and reads nothing back -- d_Q may be what triangulate_device just filled.
        d_status [T][2] int32 is required, every other output may be None."""
        fn = _entry(self._lib, 'p2s_track_persons_device')
        off = np.ascontiguousarray(frame_off, dtype=np.int64).reshape(-1)
        first = _per(first_frame, max(len(off) - 1, 0), np.int64)
        rc = fn(self._h, len(off) - 1, _ptr(off), _ptr(first), int(P), int(K), _ptr(d_Q), 0 if max_dist is None else 1,
                0.0 if max_dist is None else float(max_dist), _ptr(d_state_in), _ptr(d_n_state_in), _ptr(d_ids), _ptr(d_Q_rows),
                _ptr(d_matched_dist), _ptr(d_n_slots), _ptr(d_state_out), _ptr(d_n_state_out), _ptr(d_status))
        if rc == _lib.P2S_ERR_INVALID_ARG:
            raise TrackShapeError(f'p2s error {rc}: {self._lib.p2s_last_error().decode()}')
        _lib.check(rc)

    def track_persons_kernel_ms(self):
        """Kernel time of the last track_persons_3d() call, from HIP events around its kernel."""
        return _kernel_ms(self, 'track_persons')

    # -- trajectory gaps after triangulation (triangulation.py:888-953) -------------------------------------------------------
    def interpolate_gaps(self, coords, labels, max_gap, kind):
        """postproc.interpolate_gaps for coords [F][C] float64 -- all persons of a trial as columns side by side -- with the
        frame numbers labels [F] (increasing): bad samples (NaN or 0) in runs of at most max_gap (a count or inf) take
        interp1d's value through the column's good samples, longer runs become NaN, columns with 4 or fewer good samples stay.
        kind: None (linear, no extrapolation), 'linear', 'slinear', 'quadratic', 'cubic' (csrc/p2s_gaps.hip).
        -> (out [F][C], status [C] int32: nonzero for a column the kernels left untouched -- a spline kind with +-inf among
        its good samples).  The input is not modified."""
        return _interpolate_gaps(self._lib, self._h, coords, labels, max_gap, kind)

    def fill_gaps(self, coords, how):
        """postproc.fill_gaps on a copy: 'last_value', 'zeros'; anything else returns the table as it is."""
        return _fill_gaps(self._lib, self._h, coords, how)

    def gap_runs(self, x, first, last, max_gap, capacity=None, raw=False):
        """postproc.gap_spans for x [F][K]: (done, left), per column the 'a:b' runs of positions strictly between first and
        last that are 0 or not finite -- those of at most max_gap positions, and the longer ones.  capacity: rows of the
        device table (default: what F frames can hold at most); raw=True -> (table [n][4] int32 of (column, start, end,
        long), count, overflow) instead, without raising when the table was too small."""
        return _gap_runs(self._lib, self._h, x, first, last, max_gap, capacity, raw)

    def gaps_kernel_ms(self):
        """Kernel time of the last interpolate_gaps(), fill_gaps() or gap_runs() call, from HIP events around its kernels."""
        return _kernel_ms(self, 'gaps')

    # -- confidence timeline (Utilities/confidence_timeline.py:89-130) ---------------------------------------------------------
    def timeline_rows(self, file_off, person_base, valid, conf):
        """The rows and series of confidence_timeline for every camera folder in one call (csrc/p2s_timeline.hip).
        file_off [C + 1]: the files of every camera; person_base [n_files + 1]: the listed persons of every file; valid
        [N]: the person's list held at least 78 numbers; conf [N][K] float64, 1 <= K <= 26: the confidences of the resolved
        keypoints.  -> dict: 'row_off' [C + 1] int64 and, a row for every (file, valid person, slot) in that order,
        'frame', 'person', 'slot' int32 (camera-local file, position in the file's list, index into the K keypoints) and
        'confidence'; 'n_people' [C] the longest list of every camera; 'series_off' [sum(n_people) + 1] int64, one series
        per camera and person index below n_people: 'series_frame' the files whose entry is valid, in order, and
        'series_conf' [K][valid persons] their confidences, slot-major.  Bad offsets, lengths or K raise ValueError."""
        return _timeline_rows(self._lib, self._h, file_off, person_base, valid, conf)

    def timeline_kernel_ms(self):
        """Kernel time of the last timeline_rows() call, from HIP events around its kernels."""
        return _kernel_ms(self, 'timeline')

    # -- extrinsics refinement from keypoints (csrc/p2s_refine.hip) ---------------------------------------------
    def refine_extrinsics(self, xyl, K, R, t, X0, lik_thr=0.3, huber_px=3.0, min_cams=2, max_iter=100, ftol=1e-12):
        """Bundle adjustment of the cameras' R [C][3][3] and t [C][3] on xyl [F..., C, K, 3] (pinhole pixels and likelihood,
        float32 or float64) from the start points X0 [prod(F...) * K][3], K [C][3][3] held: the Huber cost of the weighted
        reprojection residuals over all cameras and points, camera 0 and one coordinate of camera 1's translation held
        (include/p2s.h).  -> (R, t, X [F..., K, 3], report): X is NaN where a point was dropped; report holds
        cost_before, cost_after, iterations, accepted, lambda, kept_points, held_coord, rms_before and rms_after [C] px."""
        return _refine_extrinsics(self._lib, self._h, xyl, K, R, t, X0, lik_thr, huber_px, min_cams, max_iter, ftol)

    def refine_kernel_ms(self):
        """Time of the last refine_extrinsics() call between the HIP events around its kernels (the host's reduced solves
        between the launches included)."""
        return _kernel_ms(self, 'refine')

    # -- relative poses of camera pairs (csrc/p2s_relpose.hip) ---------------------------------------------------
    def relative_poses(self, xn, usable, pairs, samples, thr2, rounds=3, all_hypotheses=False, score_points=0):
        """The essential matrix and (R, t), X_b = R X_a + t with |t| = 1, of every camera pair by hypothesise and score.
        xn [C][N][2] normalised pinhole coordinates, usable [C][N], pairs [P][2], samples [P][H][m] point indices (8 <= m <=
        16), thr2 the squared Sampson threshold in normalised units (one, or one a pair); the hypotheses are scored on at
        most score_points evenly spaced points of a pair (0: all), the refits (at most `rounds`) use all.
        -> dict: E [P][3][3], R, t [P][3], cost, inliers, front, winner, refits [P], mask [P][N]; with all_hypotheses also
        hyp_E [P][H][3][3], hyp_cost, hyp_inliers [P][H].  A pair without a result has NaN, counts 0 and winner -1."""
        return _relative_poses(self._lib, self._h, xn, usable, pairs, samples, thr2, rounds, all_hypotheses, score_points)

    def relpose_kernel_ms(self):
        """Time of the last relative_poses() call between the HIP events around its kernels (the refits' eigen-solves on the
        host between them included)."""
        return _kernel_ms(self, 'relpose')

    # -- the dominant plane of point sets: the floor under a walk (csrc/p2s_floor.hip) -----------------------------
    def fit_planes(self, points, usable, ref, samples, thr, rounds=3, all_hypotheses=False):
        """The plane n . x = d that most points of every problem lie on, by hypothesise and score.  points [B][N][3], usable
        [B][N], ref [B][3] a point above the plane (it orients n), samples [B][H][3] point indices, thr the inlier distance in
        the points' unit (one, or one a problem); at most `rounds` refits on the inliers, kept while the cost falls.
        -> dict: plane [B][4] (n, d), cost, inliers, below, winner, refits [B], centroid [B][3] and evals [B][3] of the
        inliers (ascending eigenvalues of their scatter over their count), mask [B][N]; with all_hypotheses also hyp_plane
        [B][H][4], hyp_cost, hyp_inliers [B][H].  A problem without a result has NaN, counts 0 and winner -1."""
        return _fit_planes(self._lib, self._h, points, usable, ref, samples, thr, rounds, all_hypotheses)

    def floor_kernel_ms(self):
        """Time of the last fit_planes() call between the HIP events around its kernels (the refits' eigen-solves on the host
        between them included)."""
        return _kernel_ms(self, 'floor')

    # -- synchronization (synchronization.py:1271-1343, 1541-1585) -------------------------------------------------------
    def sync_speeds(self, coords, b, a, zi):
        """coords: one [n_frames][n_cols] array per camera, the (x, y) columns of the keypoints to consider with the
        low-likelihood points NaN.  Interpolation, bfill / ffill, zero-phase Butterworth filter of every column (cameras
        with more than 3 (len(b) - 1) frames), sum of |vertical speed|, filter of that sum.  -> one speed array per
        camera.  A camera whose length lies between the reference's threshold and scipy's padlen raises scipy's
        ValueError."""
        fn = _entry(self._lib, 'p2s_sync_speeds_host')
        cols = [np.ascontiguousarray(c, dtype=np.float64) for c in coords]
        if any(c.ndim != 2 for c in cols) or len({c.shape[1] for c in cols}) > 1:
            raise P2sError('every camera needs an [n_frames][n_cols] array with the same n_cols')
        n_cols = cols[0].shape[1] if cols else 0
        lens = np.array([c.shape[0] for c in cols], dtype=np.int64)
        flat = np.ascontiguousarray(np.concatenate([c.reshape(-1) for c in cols])) if cols else np.zeros(0)
        b, a, zi = _coeffs(b, a, zi)
        out = np.empty(int(lens.sum()), dtype=np.float64)
        rc = fn(self._h, len(cols), _optr(lens), n_cols, _optr(flat), len(b), _ptr(b), _ptr(a), _ptr(zi), _optr(out))
        if rc == _lib.P2S_ERR_SYNC_PADLEN:
            raise ValueError(self._lib.p2s_last_error().decode())
        _lib.check(rc)
        return np.split(out, np.cumsum(lens)[:-1]) if cols else []

    def lagged_pearson(self, ref, signals, lag_lo, lag_hi):
        """Series(ref).corr(Series(s).shift(lag)) for every signal s and lag in [lag_lo, lag_hi).
        -> (r [n_sig][n_lags], argmax [n_sig] as np.argmax of each r row, max_corr [n_sig] as np.nanmax)."""
        fn = _entry(self._lib, 'p2s_lagged_pearson_host')
        ref = np.ascontiguousarray(ref, dtype=np.float64).reshape(-1)
        sigs = [np.ascontiguousarray(s, dtype=np.float64).reshape(-1) for s in signals]
        lens = np.array([len(s) for s in sigs], dtype=np.int64)
        flat = np.ascontiguousarray(np.concatenate(sigs)) if sigs else np.zeros(0)
        n_lags = int(lag_hi) - int(lag_lo)
        r = np.empty((len(sigs), max(n_lags, 0)), dtype=np.float64)
        arg = np.zeros(len(sigs), dtype=np.int64)
        mx = np.full(len(sigs), np.nan)
        _lib.check(fn(self._h, _optr(ref), len(ref), len(sigs), _optr(flat), _optr(lens), int(lag_lo), int(lag_hi), _optr(r),
                      _optr(arg), _optr(mx)))
        return r, arg, mx

    # -- association -----------------------------------------------------------------------
    @staticmethod
    def assoc_params(recon_thr, min_affinity, min_cams, max_iter=20, w_rank=50.0, tol=1e-4, w_sparse=0.1):
        """matchSVT constants are the reference's call-site values (personAssociation.py:799)."""
        return AssocParams(float(recon_thr), float(min_affinity), int(min_cams), int(max_iter), float(w_rank),
                           float(tol), float(w_sparse))

    def associate(self, n_persons, kpts, params):
        """n_persons [F][C] int, kpts [rows][Kj][3] (camera-major then person, JSON keypoint order).
        Returns the thresholded matchSVT matrices [F][n_max][n_max] (top-left N_f x N_f valid)."""
        n_persons = np.ascontiguousarray(np.asarray(n_persons, dtype=np.int32))
        F, Cn = n_persons.shape
        if Cn != self.n_cams:
            raise P2sError(f'n_persons has {Cn} cameras; calibration has {self.n_cams}')
        kpts, dtype = as_packed(kpts)
        per_frame = n_persons.sum(axis=1, dtype=np.int64)
        offsets = _offsets(per_frame)
        if kpts.ndim != 3 or kpts.shape[0] != offsets[-1] or kpts.shape[2] != 3:
            raise P2sError(f'kpts has shape {kpts.shape}; expected [{offsets[-1]}, Kj, 3]')
        n_max = int(per_frame.max()) if F else 0
        n_max = max(2, (n_max + 1) & ~1)
        aff = np.zeros((F, n_max, n_max), dtype=np.float64)
        _lib.check(self._lib.p2s_associate_host(self._h, F, kpts.shape[1], n_max, dtype, _ptr(n_persons), _ptr(offsets),
                                                _optr(kpts), C.byref(params), _ptr(aff)))
        return aff

    def associate_single(self, n_persons, tracked, reproj_thr, lik_thr, min_cams):
        """Single-person association (personAssociation.py:154-257).  n_persons [F][C] int, tracked [rows][3]
        = (x, y, likelihood) of the tracked keypoint of every detected person, camera-major per frame.
        Returns comb int32 [F][C] (chosen person per camera, -1 = camera off), err [F] (inf: none), Q [F][3]."""
        n_persons = np.ascontiguousarray(np.asarray(n_persons, dtype=np.int32))
        F, Cn = n_persons.shape
        if Cn != self.n_cams:
            raise P2sError(f'n_persons has {Cn} cameras; calibration has {self.n_cams}')
        tracked, dtype = as_packed(np.asarray(tracked).reshape(-1, 3))
        offsets = _offsets(n_persons.sum(axis=1, dtype=np.int64))
        if tracked.shape[0] != offsets[-1]:
            raise P2sError(f'tracked has {tracked.shape[0]} rows; n_persons sums to {offsets[-1]}')
        comb = np.full((F, Cn), -1, dtype=np.int32)
        err = np.full(F, np.inf)
        Q = np.full((F, 3), np.nan)
        prm = SingleParams(float(reproj_thr), float(lik_thr), int(min_cams), 0)
        _lib.check(self._lib.p2s_associate_single_host(self._h, F, dtype, _ptr(n_persons), _ptr(offsets), _optr(tracked),
                                                       C.byref(prm), _ptr(comb), _ptr(err), _ptr(Q)))
        return comb, err, Q

    def associate_single_device(self, F, dtype, d_n_persons, d_offsets, d_tracked, reproj_thr, lik_thr, min_cams,
                                d_comb, d_err, d_Q):
        """Device-pointer form of associate_single; the caller has checked persons per camera <= 16 and the
        number of combinations per frame (the host entry point does both)."""
        prm = SingleParams(float(reproj_thr), float(lik_thr), int(min_cams), 0)
        _lib.check(self._lib.p2s_associate_single_device(self._h, int(F), int(dtype), _ptr(d_n_persons), _ptr(d_offsets),
                                                         _ptr(d_tracked), C.byref(prm), _ptr(d_comb), _ptr(d_err),
                                                         _ptr(d_Q)))

    def associate_device(self, F, Kj, n_max, dtype, d_n_persons, d_offsets, d_kpts, params, d_aff):
        _lib.check(self._lib.p2s_associate_device(self._h, int(F), int(Kj), int(n_max), int(dtype),
                                                  _ptr(d_n_persons), _ptr(d_offsets), _ptr(d_kpts),
                                                  C.byref(params), _ptr(d_aff)))
