"""NumPy / pandas restatement of what csrc/p2s_measure.hip computes, for shapes the golden file does not hold, and as a
stand-in for the device in the host tests: NumpyEngine has Engine's stable_argsort, trimmed_means and body_measure.
A helper, not a test."""
import numpy as np
import pandas as pd

SPEED, ANGLES, RESTRICT, FEET_CONST, HEIGHT, LEG = 1, 2, 4, 8, 16, 32


def trimmed_mean(x, p):
    x = np.asarray(x, dtype=np.float64)
    s = np.sort(x)
    part = s[int(len(s) * (p / 2)):int(len(s) * (1 - p / 2))]
    return np.mean(x) if len(part) == 0 else np.mean(part)


def sum_speeds(table, n_speed=None):
    """nansum over the markers of the norm of the frame-to-frame difference; row 0 is 0."""
    table = np.asarray(table, dtype=np.float64)
    out = np.zeros(len(table))
    d = np.diff(table, axis=0)
    for m in range(table.shape[1] // 3 if n_speed is None else n_speed):
        dx, dy, dz = d[:, 3 * m], d[:, 3 * m + 1], d[:, 3 * m + 2]
        norm = np.sqrt((dx * dx + dy * dy) + dz * dz)
        out[1:] = out[1:] + np.where(np.isnan(norm), 0.0, norm)
    return out


def point(table, roles, m):
    K = table.shape[1] // 3
    if m < K:
        return table[:, 3 * m:3 * m + 3]
    r, l = (roles[0], roles[1]) if m == K else (roles[2], roles[3])
    return (table[:, 3 * r:3 * r + 3] + table[:, 3 * l:3 * l + 3]) / 2


def angle(u, v, offset, factor):
    cross = np.stack([u[:, 1] * v[:, 2] - u[:, 2] * v[:, 1], u[:, 2] * v[:, 0] - u[:, 0] * v[:, 2], u[:, 0] * v[:, 1] - u[:, 1] * v[:, 0]], axis=1)
    norm = np.sqrt((cross[:, 0] * cross[:, 0] + cross[:, 1] * cross[:, 1]) + cross[:, 2] * cross[:, 2])
    ang = (np.degrees(np.arctan2(norm, np.einsum('ij,ij->i', u, v))) + offset) * factor
    ang = np.where(ang > 180, ang - 360, ang)
    ang = np.where(ang < -180, ang + 360, ang)
    return np.abs(ang)


def mean_angles(rows, roles):
    K = rows.shape[1] // 3
    P = lambda m: point(rows, roles, m)                       # noqa: E731
    hip, neck = P(roles[4] if roles[4] >= 0 else K + 1), P(roles[5] if roles[5] >= 0 else K)
    total = np.zeros(len(rows))
    for side in range(2):
        total = total + angle(P(roles[8 + side]) - P(roles[6 + side]), P(roles[2 + side]) - P(roles[6 + side]), -180.0, 1.0)
    for side in range(2):
        total = total + angle(P(roles[2 + side]) - P(roles[6 + side]), neck - hip, 0.0, -1.0)
    return total / 4


def distance(rows, roles, pair):
    if pair[0] < 0 or pair[1] < 0:
        return np.zeros(len(rows))
    d = point(rows, roles, pair[1]) - point(rows, roles, pair[0])
    if np.isnan(d).all():
        return np.full(len(rows), np.inf)
    sq = np.where(np.isnan(d), 0.0, d * d)
    return np.sqrt((sq[:, 0] + sq[:, 1]) + sq[:, 2])


def measure(table, roles, pairs, flags, close_to_zero_speed, keep_fraction, angle_limit, trimmed_extrema_percent, head_factor, n_speed=None):
    table = np.asarray(table, dtype=np.float64)
    n = len(table)
    res = {'sum_speeds': sum_speeds(table, n_speed), 'all_slow': False, 'few_small_angles': False, 'all_data': False}
    frames = np.arange(n)
    if flags & SPEED:
        above = np.flatnonzero(res['sum_speeds'] > close_to_zero_speed)
        if len(above) == 0:
            res['all_slow'] = True
        else:
            order = above[np.argsort(res['sum_speeds'][above], kind='stable')]
            frames = order[:int(len(above) * keep_fraction)]
    res['n_selected'] = len(frames)
    res['angles'] = mean_angles(table[frames], roles) if flags & ANGLES else np.full(len(frames), np.nan)
    pos = np.arange(len(frames))
    if flags & RESTRICT:
        pos = np.flatnonzero(res['angles'] < angle_limit)
        if len(pos) < 50:
            res['few_small_angles'] = True
            order = np.argsort(res['angles'], kind='stable')
            pos = order[:50]                                  # Series.nsmallest: NaN angles come last and are kept
    if len(pos) == 0:
        res['all_data'] = True
        pos, frames = np.arange(n), np.arange(n)
    res['kept_pos'], res['kept_frame'] = pos.astype(np.int64), frames[pos].astype(np.int64)
    rows = table[res['kept_frame']]
    L = [distance(rows, roles, p) for p in pairs]
    nan = np.full(len(rows), np.nan)
    heights = legs = nan
    if flags & HEIGHT:
        feet = (0.10 + 0.10) / 2 if flags & FEET_CONST else (L[0] + L[1]) / 2
        heights = feet + (L[2] + L[3]) / 2 + (L[4] + L[5]) / 2 + (L[6] + L[7]) / 2 + L[8] * head_factor
    if flags & LEG:
        legs = (L[2] + L[3]) / 2 + (L[4] + L[5]) / 2
    res['row_values'] = np.array(L + [heights, legs]).reshape(len(pairs) + 2, len(rows))
    res['row_heights'] = np.asarray(heights)
    res['lengths'] = np.array([trimmed_mean(v, trimmed_extrema_percent) for v in L])
    res['height'] = trimmed_mean(heights, trimmed_extrema_percent)
    res['leg_length'] = trimmed_mean(legs, trimmed_extrema_percent)
    return res


class NumpyEngine:
    """Engine's three measurement calls in NumPy."""

    def stable_argsort(self, columns):
        return [np.argsort(np.asarray(c, dtype=np.float64), kind='stable').astype(np.int64) for c in columns]

    def trimmed_means(self, columns, trimmed_extrema_percent=0.5):
        return np.array([trimmed_mean(c, trimmed_extrema_percent) for c in columns])

    def body_measure(self, tables, marker_index, pairs, flags, close_to_zero_speed=0.2, fastest_frames_to_remove_percent=0.2,
                     large_hip_knee_angles=45, trimmed_extrema_percent=0.5, head_factor=1.008, row_values=False, n_speed_markers=None):
        nf = len(tables)
        n_speed = [None] * nf if n_speed_markers is None else np.broadcast_to(np.asarray(n_speed_markers), (nf,))
        flags = np.broadcast_to(np.asarray(flags), (nf,))
        speed = np.broadcast_to(np.asarray(close_to_zero_speed, dtype=np.float64), (nf,))
        head = np.broadcast_to(np.asarray(head_factor, dtype=np.float64), (nf,))
        with np.errstate(all='ignore'):
            return [measure(tables[f], list(marker_index[f]), [tuple(p) for p in np.asarray(pairs[f]).reshape(-1, 2)], int(flags[f]),
                            speed[f], 1 - fastest_frames_to_remove_percent, float(large_hip_knee_angles), trimmed_extrema_percent,
                            head[f], None if n_speed[f] is None else int(n_speed[f])) for f in range(nf)]


def pandas_sum_speeds(Q_coords, keypoints_names):
    """The reference's expression for the summed speeds, on a DataFrame in its layout."""
    return np.nansum([np.linalg.norm(Q_coords[kpt].diff(), axis=1) for kpt in keypoints_names], axis=0)


def frame_digest(frame):
    """sha256 over the bytes of a frame's values, its index and its column names."""
    import hashlib
    h = hashlib.sha256()
    h.update(np.ascontiguousarray(frame.to_numpy(dtype=np.float64)).tobytes())
    h.update(np.asarray(frame.index, dtype=np.int64).tobytes())
    h.update('\t'.join(map(str, frame.columns)).encode())
    return h.hexdigest()


def read_trc_text(text):
    """A trial's text -> (Q_coords, markers) as pose2sim_amd.trc.read_trc gives them, without a file."""
    import io
    lines = text.split('\n')
    markers = [m.strip() for m in lines[3].split('\t')[2::3] if m.strip()]
    block = pd.read_csv(io.StringIO(text), sep='\t', skiprows=5, header=None)
    coords = block.iloc[:, 2:2 + 3 * len(markers)].to_numpy(dtype=np.float64)
    return pd.DataFrame(coords, columns=[m for m in markers for _ in range(3)]), markers
