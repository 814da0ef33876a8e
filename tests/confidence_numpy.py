"""NumPy stand-in for Engine.confidence_stats and Engine.column_mean_std: np.mean, np.std, np.median, np.percentile, np.min and
np.max themselves on every column's non-NaN entries, as Utilities/pose_confidence_analyze.py calls them.  Test
infrastructure: it stands in for the Engine in the host tests and for the reference at sizes too big to record;
tests/test_confidence_host.py pins it to the recorded goldens bit for bit."""
import numpy as np

STATS = ('mean', 'median', 'std', 'min', 'max', 'p5', 'p25', 'p75', 'p95')
BANDS = ((0.0, 0.4), (0.4, 0.6), (0.6, 0.8), (0.8, 1.0), (1.0, np.inf))      # the fourth is closed above


def column_stats(valid):
    if len(valid) == 0:
        return [np.nan] * 9
    with np.errstate(all='ignore'):
        return [np.mean(valid), np.median(valid), np.std(valid), np.min(valid), np.max(valid)] + [np.percentile(valid, q) for q in (5, 25, 75, 95)]


class NumpyConfidenceEngine:
    def column_mean_std(self, data):
        data = np.asarray(data, dtype=np.float64)
        cols = [data[:, c][~np.isnan(data[:, c])] for c in range(data.shape[1])]
        with np.errstate(all='ignore'):
            mean = np.array([np.mean(v) if len(v) else np.nan for v in cols])
            std = np.array([np.std(v) if len(v) else np.nan for v in cols])
        return mean, std, np.array([len(v) for v in cols], dtype=np.int64)

    def confidence_stats(self, tables, thresholds=(0.4,)):
        tables = [np.asarray(t, dtype=np.float64) for t in tables]
        Cn, K, T = len(tables), tables[0].shape[1], len(thresholds)
        stats = np.empty((Cn, K, 9))
        counts = np.zeros((Cn, K), dtype=np.int64)
        below = np.zeros((T, Cn, K), dtype=np.int64)
        bands = np.zeros((Cn, K, 5), dtype=np.int64)
        for c, t in enumerate(tables):
            for k in range(K):
                col = t[:, k]
                valid = col[~np.isnan(col)]
                stats[c, k] = column_stats(valid)
                counts[c, k] = len(valid)
                below[:, c, k] = [np.sum(valid < th) for th in thresholds]
                bands[c, k] = [np.sum((valid >= lo) & ((valid <= hi) if i == 3 else (valid < hi))) for i, (lo, hi) in enumerate(BANDS)]
        with np.errstate(invalid='ignore', divide='ignore'):
            below_rate = below / counts
            band_rate = np.where(counts[:, :, None] > 0, bands / counts[:, :, None], 0.0)
        return {'stats': stats, 'counts': counts, 'below': below, 'below_rate': below_rate, 'bands': bands, 'band_rate': band_rate}


def seeded_tables(C, F, seed):
    """The confidence columns of jitter_numpy.seeded_series: one [F][26] table per camera (about 1 % all-NaN frames)."""
    import jitter_numpy as jn
    return [np.ascontiguousarray(jn.seeded_series(F, seed * 100 + c)[:, :, 2]) for c in range(C)]
