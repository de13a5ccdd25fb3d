"""Host-side checks of the binned reduction: the new entry points exist and the ABI revision did not move, every
argument error is a ValueError raised before anything touches a device (CPU tensors, host arrays), and the arithmetic
of StreamStats on hand-made fields: sumsq from the limbs, mean() and std() against exact rational arithmetic."""
import math
import os
import re
import subprocess
from fractions import Fraction

import numpy as np
import pytest
import torch

import flacarray_amd as fa
from flacarray_amd import _lib
from tests.conftest import ROOT

HEADER = os.path.join(ROOT, "include", "flacarray_hip.h")
NEW_SYMBOLS = ("fa_reduce_i32_device", "fa_reduce_i64_device", "fa_reduce_indexed")


def test_new_symbols_and_abi_revision():
    with open(HEADER) as f:
        text = f.read()
    assert re.search(r"^#define FA_ABI_VERSION 4\b", text, re.M)
    assert _lib.ABI_VERSION == 4 and _lib.lib().fa_abi_version() == 4
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = {line.split()[-1] for line in out.splitlines() if line.strip()}
    for name in NEW_SYMBOLS:
        assert name in _lib.SYMBOLS
        getattr(_lib.lib(), name)
        assert re.search(r"^int %s\(" % name, text, re.M), name
        assert name in exported, name
    for name in ("reduce_flac_device", "StreamStats"):
        assert name in fa.__all__ and hasattr(fa, name)
    assert callable(fa.FlacArray.reduce) and callable(fa.DeviceDecodeIndex.reduce)


def _cpu_store(n_stream=6):
    return torch.zeros(4096, dtype=torch.uint8), torch.arange(n_stream, dtype=torch.int64) * 100, torch.full((n_stream,), 100, dtype=torch.int64)


BAD_ARGS = [
    ("width0", dict(width=0)),
    ("width_negative", dict(width=-5)),
    ("empty_range", dict(first_sample=10, last_sample=10)),
    ("reversed_range", dict(first_sample=11, last_sample=10)),
    ("first_negative", dict(first_sample=-1, last_sample=10)),
    ("last_beyond", dict(last_sample=1001)),
    ("first_beyond", dict(first_sample=1000)),
    ("streams_2d", dict(streams=np.zeros((2, 2), np.int64))),
    ("streams_float", dict(streams=np.array([0.0, 1.0]))),
    ("streams_negative", dict(streams=[-1])),
    ("streams_beyond", dict(streams=[0, 6])),
    ("streams_twice", dict(streams=[3, 1, 3])),
]


@pytest.mark.parametrize("name,kw", BAD_ARGS, ids=[b[0] for b in BAD_ARGS])
def test_reduce_flac_device_argument_errors_need_no_device(name, kw):
    comp, st, nb = _cpu_store()
    with pytest.raises(ValueError):
        fa.reduce_flac_device(comp, st, nb, 1000, **kw)


def _host_array(dtype=np.int32):
    """A FlacArray assembled by hand (nothing is encoded: its reduce must fail on the arguments before it reads a byte)."""
    return fa.FlacArray(None, shape=(2, 3, 1000), global_shape=None, compressed=np.zeros(64, np.uint8), dtype=np.dtype(dtype),
                        stream_starts=np.zeros((2, 3), np.int64), stream_nbytes=np.zeros((2, 3), np.int64))


@pytest.mark.parametrize("name,kw", BAD_ARGS, ids=[b[0] for b in BAD_ARGS])
def test_flacarray_reduce_argument_errors_need_no_device(name, kw):
    kw = {{"first_sample": "first", "last_sample": "last"}.get(k, k): v for k, v in kw.items()}
    with pytest.raises(ValueError):
        _host_array().reduce(**kw)


def test_empty_streams_returns_empty_arrays_without_a_device():
    for dt, limbs in ((np.int32, True), (np.int64, False)):
        s = _host_array(dt).reduce(width=300, streams=np.zeros(0, np.int64))
        assert isinstance(s, fa.StreamStats)
        for f in (s.count, s.min, s.max, s.sum, s.min_int, s.max_int):
            assert f.shape == (0, 4)
        assert s.min.dtype == dt and s.sum.dtype == np.int64
        assert (s.sumsq_hi is not None) == limbs and (s.sumsq is not None) == limbs
        if limbs:
            assert s.sumsq_lo.shape == (0, 4) and s.sumsq.shape == (0, 4)


def _stats(rows):
    """StreamStats of hand-made integer rows (one bin per row), limbs computed with Python integers."""
    cnt = np.array([[len(r)] for r in rows], np.int64)
    sm = np.array([[sum(int(v) for v in r)] for r in rows], np.int64)
    hi = np.array([[sum((int(v) * int(v)) >> 32 for v in r)] for r in rows], np.uint64)
    lo = np.array([[sum((int(v) * int(v)) & 0xFFFFFFFF for v in r)] for r in rows], np.uint64)
    mn = np.array([[min(r)] for r in rows], np.int64)
    mx = np.array([[max(r)] for r in rows], np.int64)
    return fa.StreamStats(cnt, mn, mx, sm, hi, lo, mn, mx)


def test_sumsq_from_limbs_is_correctly_rounded_up_to_2_21_samples():
    """n <= 2^21 samples at the +-2^31 extremes: hi < 2^51 and lo < 2^53, both convert exactly, one rounding."""
    rng = np.random.default_rng(7)
    for n in (1, 2, 3, 1000, 2**20 + 1, 2**21):
        for kind in ("min", "max", "mixed", "random"):
            if kind == "min":
                x = np.full(n, -(2**31), np.int64)
            elif kind == "max":
                x = np.full(n, 2**31 - 1, np.int64)
            elif kind == "mixed":
                x = np.where(np.arange(n) % 3 == 0, -(2**31), 2**31 - 1 - (np.arange(n) % 5)).astype(np.int64)
            else:
                x = rng.integers(-(2**31), 2**31, n)
            q = (x * x).astype(np.uint64)  # <= 2^62
            hi, lo = int((q >> np.uint64(32)).sum(dtype=np.uint64)), int((q & np.uint64(0xFFFFFFFF)).sum(dtype=np.uint64))
            exact = (hi << 32) + lo
            assert exact == int((q >> np.uint64(31)).sum(dtype=np.uint64)) * 2**31 + int((q & np.uint64(2**31 - 1)).sum(dtype=np.uint64))
            s = fa.StreamStats(np.array([n]), None, None, None, np.array([hi], np.uint64), np.array([lo], np.uint64), None, None)
            assert s.sumsq.dtype == np.float64 and s.sumsq[0] == float(exact), (n, kind)


def test_mean_is_true_division():
    rows = [[1, 2, 4], [2**31 - 1] * 7 + [-5], [-(2**31)] * 3, [3, -3], [2**31 - 1, 2**31 - 2, 2**31 - 4]]
    s = _stats(rows)
    got = s.mean()
    assert got.dtype == np.float64 and got.shape == (len(rows), 1)
    for i, r in enumerate(rows):
        assert got[i, 0] == sum(r) / len(r)
    # a sum beyond 2^53: converting it to float64 before dividing rounds twice
    big = fa.StreamStats(np.array([3]), None, None, np.array([2**62 + 1]), None, None, None, None)
    assert big.mean()[0] == (2**62 + 1) / 3


def test_std_does_not_cancel():
    """A bin of mean 2^30 and spread 1: sum of squares ~ n 2^60, the variance 0.25 -- E[x^2] - E[x]^2 in float64 has lost
    every digit of it; the exact form has not."""
    rows = [[2**30, 2**30 + 1] * 500, [2**30 - 1, 2**30, 2**30 + 1] * 333, [2**31 - 1, 2**31 - 2] * 4096, [5] * 10, [-(2**31), 2**31 - 1]]
    s = _stats(rows)
    got = s.std()
    assert got.dtype == np.float64
    for i, r in enumerate(rows):
        n = len(r)
        var = Fraction(n * sum(v * v for v in r) - sum(r) ** 2, n * n)
        assert got[i, 0] == math.sqrt(float(var)), i
    assert got[0, 0] == 0.5 and got[3, 0] == 0.0
    naive = np.sqrt(s.sumsq / s.count - (s.sum / s.count) ** 2)
    assert not naive[0, 0] == 0.5  # (what the test is for: the naive formula fails this bin)


def test_float_store_statistics_map_through_offset_and_gain():
    s0 = _stats([[10, 20, 30], [-4, 4]])
    s = fa.StreamStats(s0.count, None, None, s0.sum, s0.sumsq_hi, s0.sumsq_lo, s0.min_int, s0.max_int,
                       offsets=np.array([[1.5], [-2.0]]), gains=np.array([[4.0], [0.5]]))
    assert np.array_equal(s.mean(), [[1.5 + 20 / 4.0], [-2.0]])
    assert np.array_equal(s.std(), s0.std() / np.array([[4.0], [0.5]]))


def test_std_of_a_64_bit_store_is_an_error():
    s = fa.StreamStats(np.array([2]), None, None, np.array([3]), None, None, None, None)
    assert s.sumsq is None
    with pytest.raises(ValueError):
        s.std()
