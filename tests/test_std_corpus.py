"""CPU checks of the np.std corpus (tests/std_corpus.py): the reference holds on every case -- npsum.std_model, the
recipe the kernel implements, equals np.std under the case's buffer size bit for bit -- and the corpus reaches the paths
it was built for, asserted from the plan (flacarray_amd.npsum.pairwise_plan), never from a kernel's output."""
import numpy as np
import pytest

from flacarray_amd import npsum
from tests import std_corpus as C

PLAN_BATCH = 2048  # kStdPlanLeaves of csrc/std_kernels.hpp: leaf sums the plan path holds at a time
FOLD_BLOCK = 256  # threads per block of stream_fold_kernel


@pytest.fixture(scope="module")
def corpus():
    return C.build()


def _bits(a):
    a = np.atleast_1d(np.asarray(a))
    return a.view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


def _same(got, want):
    """Bit patterns equal, any NaN equal to any NaN."""
    if got.dtype != want.dtype or got.shape != want.shape:
        return False
    nan = np.isnan(want)
    return np.array_equal(np.isnan(got), nan) and np.array_equal(_bits(got)[~nan], _bits(want)[~nan])


@pytest.mark.parametrize("name", C.NAMES)
def test_model_is_np_std_on_the_corpus(corpus, name):
    case = corpus[name]
    _, dtype, x, b = case
    want = C.reference(case)
    old = np.getbufsize()
    try:
        with np.errstate(all="ignore"):
            got = npsum.std_model(x, b)
    finally:
        np.setbufsize(old)
    assert want.dtype == np.dtype(dtype)
    assert _same(got, want), (name, int((_bits(got) != _bits(want)).sum()))


def test_names_are_unique_and_both_dtypes_have_every_case():
    assert len(set(C.NAMES)) == len(C.NAMES)
    f32 = sorted(n.replace("_f32", "") for n in C.NAMES if "_f32" in n)
    f64 = sorted(n.replace("_f64", "") for n in C.NAMES if "_f64" in n)
    assert f32 == f64 and len(f32) * 2 == len(C.NAMES)


def test_geometries_reach_their_paths(corpus):
    for b in C.BUFSIZES:
        lengths = C.geometry_lengths(b)
        assert {"b-1", "b", "b+1", "3b+5", "8192"} <= set(lengths)
        assert ("2b+8192" in lengths) == (b not in (16, 1024))
        for dtype in C.DTYPES:
            t = C.tag(dtype)
            # the second row starts off a 16-byte boundary in at least one case of this buffer size and dtype
            odd = [n for n in lengths.values() if (n * np.dtype(dtype).itemsize) % 16]
            assert odd, (b, t)
            for label, n in lengths.items():
                _, _, x, bb = corpus[f"geom_{t}_buf{b}_{label}"]
                assert x.shape[1] == n and x.shape[0] >= 2 and bb == b
        # which plans the lengths ask for
        full, tail = C.chunk_lengths(3 * b + 5, b)
        assert (full, tail) == (b, 5)  # several full chunks, then a tail that starts from -0.0 (fewer than 8 elements)
        assert C.chunk_lengths(b + 1, b) == (b, 1) and C.chunk_lengths(b - 1, b) == (None, b - 1)
        if "2b+8192" in lengths:
            assert C.chunk_lengths(lengths["2b+8192"], b) == (b, npsum.FAST_CHUNK)  # the fast path as the tail
        assert C.chunk_lengths(8192, b) == ((None, 8192) if b > 8192 else (b, None))
    # more leaves than one batch of the plan path: 262160 ends in a batch of 2, 2**20 fills four batches exactly
    assert C.plan_leaves(262160) == PLAN_BATCH + 2
    assert C.plan_leaves(2**20) == 4 * PLAN_BATCH
    assert C.plan_leaves(262159) > PLAN_BATCH and C.plan_leaves(2**20 - 1) > PLAN_BATCH
    # both plans non-empty and different: a full chunk of b and a tail that is neither b nor 8192
    for b in C.BUFSIZES:
        full, tail = C.chunk_lengths(b + 1, b)
        assert full != npsum.FAST_CHUNK and tail not in (full, npsum.FAST_CHUNK)
    # the stack of the postfix program goes deeper than the two or three levels of the parent's tests
    _, ops = npsum.pairwise_plan(2**20)
    assert np.cumsum(np.where(ops == 1, 1, -1)).max() >= 14


def test_sweep_is_wide_and_ragged(corpus):
    for dtype in C.DTYPES:
        for n in C.SWEEP_LENGTHS:
            _, _, x, b = corpus[f"sweep_{C.tag(dtype)}_n{n}"]
            assert x.shape == (C.SWEEP_ROWS, n) and b == C.DEFAULT_BUFSIZE
            assert x.shape[0] > FOLD_BLOCK and x.shape[0] % FOLD_BLOCK  # S2's last block is ragged
            assert np.isfinite(x).all()
            with np.errstate(all="ignore"):
                ex = np.frexp(np.abs(x).max(axis=1))[1]
            fi = np.finfo(dtype)
            assert ex.min() < fi.minexp and ex.max() > fi.maxexp - 12  # from subnormal rows to rows near overflow
            want = C.reference(corpus[f"sweep_{C.tag(dtype)}_n{n}"])
            ok = np.isfinite(want) & (want > 0)
            assert ok.sum() > C.SWEEP_ROWS // 3  # and a third of the rows at least has a std that is neither 0 nor inf
    assert {n for n in C.SWEEP_LENGTHS if n < 8} and {n % 8 for n in C.SWEEP_LENGTHS if n > 8} - {0}


def test_hard_square_roots_sit_on_rounding_boundaries(corpus):
    for dtype in C.DTYPES:
        t = C.tag(dtype)
        rows, dist = C.sqrt_rows(t)
        assert rows.shape == (C.SQRT_KEPT, 4) and rows.dtype == np.dtype(dtype)
        assert np.array_equal(rows[:, 0], -rows[:, 1]) and np.array_equal(rows[:, 2], -rows[:, 3])
        close = np.abs(dist) < 2.0**-10
        assert close.sum() >= 1000, (t, int(close.sum()))
        assert (dist[close] < 0).sum() > 100 and (dist[close] > 0).sum() > 100, t
        # the measure is of the variance numpy really forms: recompute it from np.var's bits, with integers
        with np.errstate(all="ignore"):
            v = np.var(rows, axis=-1)
        again = np.array([C.sqrt_boundary_distance(x, dtype) for x in v[:64].tolist()])
        assert np.array_equal(again, dist[:64])
        # and it means what it says: the correctly rounded root is the lower neighbour exactly when dist < 0
        for x, d in zip(v[:64].tolist(), dist[:64].tolist()):
            s = float(np.sqrt(dtype(x)))  # numpy's sqrt is correctly rounded
            below = s * s <= x if d < 0 else s * s >= x
            assert below, (t, x, d)


def test_sqrt_boundary_distance_on_known_values():
    # sqrt(1 + 2**-23) = 1 + 2**-24 - 2**-49...: a hair below the midpoint of float32's 1 and 1 + 2**-23
    d = C.sqrt_boundary_distance(float(np.float32(1) + np.float32(2.0**-23)), np.float32)
    assert -(2.0**-20) < d < 0
    assert C.sqrt_boundary_distance(4.0, np.float64) == -0.5 and C.sqrt_boundary_distance(2.25, np.float32) == -0.5


def test_hard_values_are_what_they_claim(corpus):
    for dtype in C.DTYPES:
        t = C.tag(dtype)
        fi = np.finfo(dtype)
        want = {k: C.reference(corpus[f"hard_{t}_{k}"]) for k in C.HARD_KINDS}
        for k in C.HARD_KINDS:
            x = corpus[f"hard_{t}_{k}"][2]
            assert x.shape == (3, C.HARD_N)
            assert np.isfinite(want[k][[0, 2]]).all() and (want[k][[0, 2]] > 0).all()  # ordinary neighbours
        for k in ("pinf", "ninf_last", "both_inf"):
            assert np.isnan(want[k][1])  # inf - inf
        assert np.isinf(corpus[f"hard_{t}_ninf_last"][2][1, -1])
        with np.errstate(all="ignore"):
            x = corpus[f"hard_{t}_sum_overflow"][2][1]
            assert np.isfinite(x).all() and np.isinf(np.sum(x))
            x = corpus[f"hard_{t}_square_overflow"][2][1]
            assert np.isfinite(x).all() and np.isfinite(np.sum(x)) and np.isinf(x * x).any()
            assert np.isinf(want["square_overflow"][1])
            x = corpus[f"hard_{t}_subnormal_var"][2][1]
            sq = x * x
            assert (sq[sq > 0] < fi.smallest_normal).all() and (sq > 0).sum() > C.HARD_N // 2
            var = np.var(x)
            assert 0 < var < fi.smallest_normal
            scale = 1e-21 if t == "f32" else 1e-158
            assert 0.5 * scale < want["subnormal_var"][1] < 2 * scale  # a flushed denormal would give 0
            x = corpus[f"hard_{t}_subnormals"][2][1]
            assert (np.abs(x) < fi.smallest_normal).all() and (x != 0).sum() > C.HARD_N // 2
            x = corpus[f"hard_{t}_negzero"][2][1]
            assert (x == 0).all() and np.signbit(x).all() and want["negzero"][1] == 0
            x = corpus[f"hard_{t}_cancel"][2][1]
            assert x[:4].tolist() == [1e8, 1.0, -1e8, 3.0]


def test_nan_positions_are_the_edges(corpus):
    for dtype in C.DTYPES:
        t = C.tag(dtype)
        for name, n, big in ((f"nan_{t}_default", C.HARD_N, False), (f"nan_{t}_batches", C.NAN_BIG_N, True)):
            case = corpus[name]
            x = case[2]
            pos = C.nan_positions(n, big)
            assert {0, 7, 8, 127, 128, 8191, 8192, n - 1} <= set(pos)
            assert x.shape == (len(pos) + 1, n)
            for r, p in enumerate(pos):
                assert np.flatnonzero(np.isnan(x[r])).tolist() == [p]
            assert not np.isnan(x[-1]).any()
            want = C.reference(case)
            assert np.isnan(want[:-1]).all() and np.isfinite(want[-1])
        # batch and chunk edges of the 262160 plan: leaf 2047 is the first batch's last, leaf 2048 opens the second
        leaves, _ = npsum.pairwise_plan(C.NAN_BIG_BUF)
        assert case[3] == C.NAN_BIG_BUF
        assert leaves[PLAN_BATCH - 1, 0] <= 262016 and leaves[PLAN_BATCH, 0] == 262024
        assert {262016, 262023, 262024, 262159, 262160} <= set(C.nan_positions(C.NAN_BIG_N, True))
        assert leaves[-1, 0] + leaves[-1, 1] == 262160
