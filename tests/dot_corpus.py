"""Stores, templates and the oracle for the projections (FlacArray.dot, K7D).

Builders only: nothing here calls the library's device side or the GPU.  tests/test_dot_corpus.py asserts on the CPU that
the stores and templates have what they are for; tests/test_gpu_dot.py sends them through the device paths.

The stores are those of tests/xsum_corpus.py -- K7D runs in K7X's task layout, so what makes a wave hard is the same: A and
B (131 writer streams: three plan rows of 64 + 64 + 3 lanes, LPC orders 1-32 and wasted bits mixed inside one wave, a short
last frame), C (70 library streams of full-range noise), D (5 two-channel streams) -- plus the samples of one small store
the library writes, whose first two rows hold INT32_MIN and INT32_MAX at sample 0 and on both sides of a frame boundary.

Templates are drawn from {0, +1, -1, INT32_MIN, INT32_MAX, noise}; K in KS covers less than a pass, exactly one pass of 8,
the seam (9) and three passes (17).  The wide set leaves int32 up to both ends of int64.

The oracle is Python integers and nothing else.
"""
import functools

import numpy as np

from tests import xsum_corpus as X

store_a, store_b, store_d, samples_c = X.store_a, X.store_b, X.store_d, X.samples_c

INT32_MIN, INT32_MAX = -(2**31), 2**31 - 1
INT64_MIN, INT64_MAX = -(2**63), 2**63 - 1
KS = (1, 3, 8, 9, 17)
EXT_BLOCK = 4096  # the library's frame length
N_EXT, LEN_EXT = 6, EXT_BLOCK + 50


@functools.lru_cache(maxsize=None)
def samples_extremes():
    """int32 [6, 4146]: small noise; rows 0 and 1 hold the two int32 extremes at sample 0 and at the last sample of frame
    0 and the first of frame 1, each row the other's mirror."""
    rng = np.random.default_rng(4242)
    x = rng.integers(-1000, 1000, (N_EXT, LEN_EXT)).astype(np.int32)
    for row, (a, b) in enumerate(((INT32_MIN, INT32_MAX), (INT32_MAX, INT32_MIN))):
        x[row, 0] = a
        x[row, EXT_BLOCK - 1] = b
        x[row, EXT_BLOCK] = a
    return x


def templates(K, n, seed=0):
    """int64 [K, n] inside int32: every sample of every template drawn from {0, 1, -1, INT32_MIN, INT32_MAX, noise}."""
    rng = np.random.default_rng(1000 * K + n + seed)
    kind = rng.integers(0, 6, (K, n))
    noise = rng.integers(INT32_MIN, INT32_MAX, (K, n), endpoint=True)
    table = np.array([0, 1, -1, INT32_MIN, INT32_MAX, 0], dtype=np.int64)
    return np.where(kind == 5, noise, table[kind]).astype(np.int64)


def constant_templates(n):
    """int64 [2, n]: all INT32_MIN, all INT32_MAX -- with full-range samples every product has the largest magnitude
    there is, of either sign."""
    return np.stack([np.full(n, INT32_MIN, dtype=np.int64), np.full(n, INT32_MAX, dtype=np.int64)])


def wide_templates(n, seed=0):
    """int64 [5, n] that leave int32: row 0 holds INT64_MIN, INT64_MAX, 2^31 and -2^31 - 1 among noise of all 64 bits, row 1
    only 2^31 and -2^31 - 1 among zeros (just outside int32 on either side; the negative value sets all three planes),
    row 2 multiples of 2^31
    below 2^62 (its lowest and highest planes are zero and are dropped), row 3 fits int32 (it stays one plane), row 4 is
    all zeros (no plane at all)."""
    rng = np.random.default_rng(77 + n + seed)
    T = np.zeros((5, n), dtype=np.int64)
    T[0] = rng.integers(INT64_MIN, INT64_MAX, n, endpoint=True)
    marks = np.array([INT64_MIN, INT64_MAX, 2**31, -(2**31) - 1], dtype=np.int64)
    T[0, : min(4, n)] = marks[: min(4, n)]
    T[1, ::2] = 2**31
    T[1, 1::3] = -(2**31) - 1
    T[2] = rng.integers(0, 2**31, n) << 31
    T[3] = templates(1, n, seed)[0]
    return T


def ranges(n, block):
    """(first, last): everything; [1, n); [0, n - 1); inside one frame; one that starts among a frame's warm-up samples
    (frame sample 5: the orders above 5 have not predicted anything yet) and ends inside that frame; one that starts and
    ends off every 32-sample tile boundary and lies across two frames."""
    return ((0, n), (1, n), (0, n - 1), (block + 33, block + 50), (block + 5, block + 60), (block - 13, block + 45))


def subset(n_stream=131, count=67, seed=3):
    """A permuted subset of `count` streams."""
    return np.random.default_rng(seed).permutation(n_stream)[:count].astype(np.int64)


def oracle(x, T, first, last, streams=None):
    """Object array [rows, K] of Python integers: x[streams, first:last] @ T.T on the known samples."""
    sel = np.arange(x.shape[0]) if streams is None else np.asarray(streams)
    T = np.asarray(T)
    assert T.shape[1] == last - first
    return x[sel, first:last].astype(object) @ T.astype(object).T


def kernel_model(x, t):
    """What K7D keeps per template for the samples x and template values t (int32 each, at most 65535 of them): the two
    accumulators lo += (uint32)p as uint64 and hi += p >> 32 (arithmetic) as int64, p = (int64)x * t, in numpy's wrapping
    integer arithmetic.  Returns (hi, lo) as Python integers, hi signed and lo unsigned."""
    p = np.asarray(x, dtype=np.int64) * np.asarray(t, dtype=np.int64)
    lo = np.sum((p & 0xFFFFFFFF).astype(np.uint64), dtype=np.uint64)
    hi = np.sum(p >> 32, dtype=np.int64)
    return int(hi), int(lo)
