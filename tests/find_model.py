"""The numpy model of the search (FlacArray.find, find_flac_device): np.nonzero of the predicate on the known samples,
and a brute-force boolean-mask model of StreamHits.ranges(pad).  Nothing here calls the library."""
import numpy as np

I64_MIN, I64_MAX = -(2**63), 2**63 - 1


def _per_row(v, rows, missing, dtype):
    if v is None:
        v = missing
    a = np.asarray(v, dtype=dtype)
    return np.broadcast_to(a, (rows,)) if a.ndim == 0 else a.reshape(rows)


def hit_mask(x, lo=None, hi=None, inside=False, dtype=np.int64):
    """x [rows, n] -> bool [rows, n]: (x < lo[row] or x > hi[row]) != inside.  Integer data are compared as int64, float
    data (dtype=np.float64) exactly, in float64; None is no limit on that side."""
    x = np.asarray(x)
    rows = x.shape[0]
    if dtype == np.float64:
        lo_r, hi_r = _per_row(lo, rows, -np.inf, np.float64), _per_row(hi, rows, np.inf, np.float64)
        xx = x.astype(np.float64)
    else:
        lo_r, hi_r = _per_row(lo, rows, I64_MIN, np.int64), _per_row(hi, rows, I64_MAX, np.int64)
        xx = x.astype(np.int64)
    return ((xx < lo_r[:, None]) | (xx > hi_r[:, None])) != bool(inside)


def hits(x, lo=None, hi=None, inside=False, first=0, last=None, dtype=np.int64):
    """(counts [rows], rows [total], positions [total], values [total]) of the hits in x[:, first:last], sorted by (row,
    position); positions are stream coordinates, values are taken from x as it is."""
    x = np.asarray(x)
    last = x.shape[1] if last is None else last
    m = hit_mask(x[:, first:last], lo, hi, inside, dtype)
    r, p = np.nonzero(m)
    p = p + first
    return m.sum(axis=1).astype(np.int64), r.astype(np.int64), p.astype(np.int64), x[r, p]


def ranges(n_rows, rows, positions, first, last, pad, streams=None):
    """The mask model of StreamHits.ranges: every hit sets mask[row, p - pad : p + pad + 1] inside [first, last); the
    runs of set samples are the ranges -- int64 [k, 3], rows (stream or row, first, last exclusive), sorted."""
    out = []
    for r in range(n_rows):
        m = np.zeros(last - first + 2, dtype=bool)  # (a clear sample at either end closes every run)
        for p in np.asarray(positions)[np.asarray(rows) == r]:
            a, b = max(int(p) - pad, first), min(int(p) + pad + 1, last)
            m[a - first + 1 : b - first + 1] = True
        d = np.diff(m.astype(np.int8))
        for a, b in zip(np.flatnonzero(d == 1), np.flatnonzero(d == -1)):
            out.append((r if streams is None else int(streams[r]), int(a) + first, int(b) + first))
    return np.asarray(out, dtype=np.int64).reshape(-1, 3)
