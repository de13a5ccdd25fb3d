"""CPU tests of flacarray_amd.npsum: the plan of numpy's pairwise sum and the vectorised model of np.std, which must be
bitwise equal to np.std itself -- the device kernel (csrc/std_kernels.hpp) is checked against both."""
import numpy as np
import pytest

from flacarray_amd import npsum

LENGTHS = [1, 7, 8, 9, 127, 128, 129, 136, 1000, 8191, 8192, 8193, 10000, 12345, 100000, 2**20 - 3]


def _inputs(kind, shape, dtype, rng):
    if kind == "normal":
        x = rng.normal(size=shape)
    elif kind == "dc":
        x = 1e6 + rng.normal(size=shape)
    elif kind == "constant":
        x = np.full(shape, 0.1)
    else:  # mixed signs over six decades
        x = rng.normal(size=shape) * 10 ** rng.uniform(-3, 3, size=shape)
    return x.astype(dtype)


def _bits(a):
    return a.view(np.uint32 if a.dtype == np.float32 else np.uint64)


def _shapes(n):
    if n >= 100000:
        return [(n,), (2, n)]
    return [(n,), (3, n), (2, 3, n)]


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("n", LENGTHS)
def test_std_model_is_np_std(dtype, n):
    rng = np.random.default_rng(n)
    for shape in _shapes(n):
        for kind in ("normal", "dc", "constant", "mixed"):
            x = _inputs(kind, shape, dtype, rng)
            got, want = npsum.std_model(x), np.std(x, axis=-1)
            assert got.dtype == want.dtype and got.shape == want.shape
            assert np.array_equal(_bits(np.atleast_1d(got)), _bits(np.atleast_1d(want))), (shape, kind)


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_std_model_follows_the_buffer_size(dtype):
    """numpy's chunk is np.getbufsize(): after setbufsize(4096) the model (chunk read at call time) still matches."""
    rng = np.random.default_rng(7)
    old = np.getbufsize()
    try:
        np.setbufsize(4096)
        for n in (4095, 4096, 4097, 8192, 10000, 12345, 100000):
            x = _inputs("dc", (3, n), dtype, rng)
            assert np.array_equal(_bits(npsum.std_model(x)), _bits(np.std(x, axis=-1))), n
    finally:
        np.setbufsize(old)
    # the chunk is a parameter of the model, not a constant: an explicit one overrides np.getbufsize()
    x = _inputs("dc", (3, 12345), dtype, rng)
    try:
        np.setbufsize(4096)
        want = np.std(x, axis=-1)
    finally:
        np.setbufsize(old)
    assert np.array_equal(_bits(npsum.std_model(x, bufsize=4096)), _bits(want))


def test_plan_of_a_full_chunk_is_the_perfect_tree():
    leaves, ops = npsum.pairwise_plan(8192)
    assert np.array_equal(leaves, np.stack([np.arange(64) * 128, np.full(64, 128)], axis=1))
    # post-order of a perfect binary tree: every push of an odd leaf closes as many adds as its index has trailing ones
    want = []
    for i in range(64):
        want.append(1)
        j = i
        while j & 1:
            want.append(0)
            j >>= 1
    assert ops.tolist() == want


@pytest.mark.parametrize("n", [1, 7, 8, 129, 1000, 8191, 8193, 12345, 100000])
def test_plan_covers_the_chunk(n):
    leaves, ops = npsum.pairwise_plan(n)
    assert leaves[0, 0] == 0 and np.array_equal(leaves[1:, 0], np.cumsum(leaves[:-1, 1]))
    assert leaves[:, 1].sum() == n and leaves[:, 1].max() <= 128
    assert n <= 128 or leaves[:, 1].min() >= 64  # (the kernel's bound on the number of leaves per chunk)
    assert ops.sum() == len(leaves) and len(ops) == 2 * len(leaves) - 1
    depth = np.cumsum(np.where(ops == 1, 1, -1))
    assert depth.min() >= 1 and depth[-1] == 1


def test_pairwise_sum_matches_numpy_below_the_buffer_size():
    rng = np.random.default_rng(3)
    for n in (5, 100, 129, 1000, 8192):
        x = rng.normal(size=(4, n)).astype(np.float32)
        assert np.array_equal(npsum.pairwise_sum(x), np.add.reduce(x, axis=-1))
