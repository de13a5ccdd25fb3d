"""Host model of FlacArray.histogram / order_statistic, independent of flacarray_amd: the bin rule with its unsigned
subtraction, the automatic choice of lo / shift, and the rank-refinement loop that narrows a value range by 11 bits per
histogram pass.  Everything works on known integers x [rows, n] (int32 or int64) in numpy; values that can leave int64
(edges, spans) are Python integers."""
import numpy as np

REFINE_BINS = 2048
REFINE_BITS = 11


def _per_row(v, rows, dtype):
    return np.broadcast_to(np.asarray(v, dtype=dtype), (rows,))


def bin_counts(x, lo, shift, nbins):
    """(counts [rows, nbins], below [rows], above [rows]) of x [rows, n]: a sample under lo[r] counts in below; otherwise
    its bin is ((uint64)x - (uint64)lo) >> shift -- exact for every x >= lo, INT64_MAX - INT64_MIN included -- counted in
    counts or, from nbins on, in above.  lo / shift: scalars or one per row."""
    x = np.asarray(x).astype(np.int64)
    rows = x.shape[0]
    lo = _per_row(lo, rows, np.int64)
    shift = _per_row(shift, rows, np.int64)
    counts = np.zeros((rows, nbins), dtype=np.int64)
    below = np.zeros(rows, dtype=np.int64)
    above = np.zeros(rows, dtype=np.int64)
    for r in range(rows):
        under = x[r] < lo[r]
        d = x[r][~under].view(np.uint64) - lo[r : r + 1].view(np.uint64)  # modulo 2^64: the true difference
        b = d >> np.uint64(shift[r])
        over = b >= np.uint64(nbins)
        below[r] = int(under.sum())
        above[r] = int(over.sum())
        counts[r] = np.bincount(b[~over].astype(np.int64), minlength=nbins)
    return counts, below, above


def auto_range(x, nbins):
    """(lo [rows] int64, shift [rows] int64): lo is the row's minimum and shift the smallest value with
    (max - min) >> shift < nbins, the span taken in Python integers."""
    x = np.asarray(x)
    lo = x.min(axis=1).astype(np.int64)
    shift = np.zeros(x.shape[0], dtype=np.int64)
    for r in range(x.shape[0]):
        span = int(x[r].max()) - int(x[r].min())
        s = 0
        while (span >> s) >= nbins:
            s += 1
        shift[r] = s
    return lo, shift


def edges(lo, shift, nbins):
    """The nbins + 1 edges of one row as Python integers."""
    return [int(lo) + (j << int(shift)) for j in range(nbins + 1)]


def order_statistic(x, ranks, count=None):
    """The refinement loop on x [rows, n] for ranks [rows] (one rank per row): (values [rows] int64, passes).  Each pass
    is one bin_counts call over ALL samples (as the device pass is); `count`, if given, is called with (lo, shift) per pass."""
    x = np.asarray(x)
    k = np.asarray(ranks, dtype=np.int64)
    lo, shift = auto_range(x, REFINE_BINS)
    passes = 0
    while True:
        if count is not None:
            count(lo.copy(), shift.copy())
        counts, below, _ = bin_counts(x, lo, shift, REFINE_BINS)
        passes += 1
        kk = k - below  # the rank among the samples at or over lo
        cum = np.cumsum(counts, axis=1)
        b = (cum <= kk[:, None]).sum(axis=1)  # the first bin whose cumulative count exceeds it
        assert np.all(b < REFINE_BINS)
        lo = lo + (b.astype(np.int64) << shift)
        if not shift.any():
            return lo, passes
        shift = np.maximum(shift - REFINE_BITS, 0)


def quantile_rank(q, n, method):
    """numpy's rank for method 'lower' / 'higher': floor / ceil of the float64 product q * (n - 1)."""
    pos = np.float64(q) * np.float64(n - 1)
    return int(np.floor(pos) if method == "lower" else np.ceil(pos))
