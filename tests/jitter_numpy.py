"""Vectorised NumPy restatement of the arithmetic of Utilities/keypoint_jitter_analyze.py (displacements, box areas,
medians, thresholds, event mask, ordered events, patterns), with Engine.jitter's interface.  Test infrastructure: it
stands in for the Engine in the host tests and for the reference at sizes too big to record; tests/test_jitter_host.py
pins it to the recorded goldens bit for bit."""
import warnings

import numpy as np

CONF, MARGIN, LOW_CONF = 0.1, 10, 0.3


def displacements(series):
    x, y, ok = series[:, :, 0], series[:, :, 1], series[:, :, 2] > CONF
    dx, dy = x[1:] - x[:-1], y[1:] - y[:-1]
    with np.errstate(invalid='ignore', over='ignore'):
        d = np.sqrt(dx * dx + dy * dy)
    d[~(ok[1:] & ok[:-1])] = np.nan
    return d


def boxes(series):
    """-> (x_lo, y_lo, x_hi, y_hi, n_valid) per frame; min / max propagate a NaN coordinate of a valid keypoint."""
    ok = series[:, :, 2] > CONF
    x, y = series[:, :, 0], series[:, :, 1]
    lo = [np.where(ok, v, np.inf).min(axis=1) for v in (x, y)]
    hi = [np.where(ok, v, -np.inf).max(axis=1) for v in (x, y)]
    return lo[0], lo[1], hi[0], hi[1], ok.sum(axis=1)


def nanmedian(a, axis=None):
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')              # all-NaN and empty columns give NaN
        return np.nanmedian(a, axis=axis)


def camera(series, multiplier, image_size):
    F = len(series)
    d = displacements(series)
    x_lo, y_lo, x_hi, y_hi, n = boxes(series)
    with np.errstate(invalid='ignore', over='ignore'):
        area = np.where(n >= 2, (x_hi - x_lo) * (y_hi - y_lo), np.nan)
    w, h = image_size
    edge = (n >= 2) & ((x_lo < MARGIN) | (y_lo < MARGIN) | (x_hi > w - MARGIN) | (y_hi > h - MARGIN))
    med_area = float(nanmedian(area))
    med = nanmedian(d, axis=0) if F > 1 else np.full(series.shape[1], np.nan)
    thr = med * multiplier
    thr[med == 0] = 10.0
    with np.errstate(invalid='ignore'):
        mask = d > thr[None, :]
    rows, kpts = np.nonzero(mask)                    # row-major: np.argwhere's order
    f = rows + 1
    small = ~np.isnan(area[f]) & (not np.isnan(med_area))
    with np.errstate(invalid='ignore'):
        small &= area[f] < med_area * 0.5
        pattern = np.where(edge[f], 0, np.where(small, 1, np.where(series[f, kpts, 2] < LOW_CONF, 2, 3)))
    events = np.stack([np.zeros_like(f), f, kpts, pattern], axis=1).astype(np.int32).reshape(-1, 4)
    return {'displacements': d, 'bb_areas': area, 'jitter_mask': mask, 'medians': med, 'thresholds': thr, 'median_bb_area': med_area,
            'counts': mask.sum(axis=0).astype(np.int32), 'events': events, 'edge': edge}


class NumpyJitterEngine:
    def jitter(self, series, multiplier=5.0, image_size=(1920, 1080)):
        per = [camera(np.asarray(s, dtype=np.float64), multiplier, image_size) for s in series]
        out = {k: [p[k] for p in per] for k in per[0] if k != 'events'}
        for c, p in enumerate(per):
            p['events'][:, 0] = c
        out['events'] = np.concatenate([p['events'] for p in per])
        return out


def seeded_series(F, seed, image_size=(1920, 1080), period=None, p_low=0.05, p_outlier=0.01, p_missing=0.01, decimals=None):
    """One camera's [F][26][3] synthetic person: a root sweeping across the image and past its left and right borders, a
    scale of 1 +- 0.6, 1.5 px noise, low confidences (outliers are four times as likely there), a few confidences below
    the validity threshold, 80 px gross outliers, missing frames (all NaN).  Values are rounded to float32 (or to
    `decimals` places: short JSON text), so that all four patterns A, C, D and E occur."""
    rng = np.random.default_rng(seed)
    w, h = image_size
    t = np.arange(F, dtype=np.float64)
    period = period or rng.uniform(900.0, 1800.0)
    body = np.stack([rng.uniform(-0.08, 0.08, 26), rng.uniform(-0.22, 0.22, 26)], axis=1) * h
    cx = w / 2 + 0.5 * w * np.sin(2 * np.pi * t / period + rng.uniform(0, 6.28))
    cy = h / 2 + 0.1 * h * np.sin(2 * np.pi * t / (0.61 * period) + rng.uniform(0, 6.28))
    scale = 1 + 0.6 * np.sin(2 * np.pi * t / (0.37 * period) + rng.uniform(0, 6.28))
    xy = np.stack([cx, cy], axis=1)[:, None, :] + body[None] * scale[:, None, None] + rng.normal(0, 1.5, (F, 26, 2))
    conf = rng.uniform(0.5, 0.95, (F, 26))
    low = rng.random((F, 26)) < p_low
    conf[low] = rng.uniform(0.12, 0.29, int(low.sum()))
    gone = rng.random((F, 26)) < 0.01
    conf[gone] = rng.uniform(0.0, 0.09, int(gone.sum()))
    out = rng.random((F, 26)) < np.where(low, 4 * p_outlier, p_outlier)
    angle = rng.uniform(0, 2 * np.pi, int(out.sum()))
    xy[out] += 80.0 * np.stack([np.cos(angle), np.sin(angle)], axis=1)
    s = np.concatenate([xy, conf[:, :, None]], axis=2)
    if decimals is None:
        s = s.astype(np.float32).astype(np.float64)
    else:
        s = np.round(s, decimals)
    s[rng.random(F) < p_missing] = np.nan
    return s


def pattern_counts(events):
    return {p: int(n) for p, n in zip('ACDE', np.bincount(events[:, 3], minlength=4))}
