"""Host-side checks of the value histogram and the order statistics built on it: the numpy model (tests/histogram_model.py)
against np.sort at the extremes of int32 and int64 with its bound on the number of passes, every argument error as a
ValueError raised before anything touches a device (the library handle raises if it is reached), and the arithmetic of
StreamHistogram on hand-made fields."""
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import flacarray_amd as fa
from flacarray_amd import _lib, libflacarray
from flacarray_amd.array import _auto_shift
from tests import histogram_model as M
from tests.conftest import ROOT

HEADER = os.path.join(ROOT, "include", "flacarray_hip.h")
NEW_SYMBOLS = ("fa_histogram_i32_device", "fa_histogram_i64_device", "fa_histogram_indexed")
I32 = (-(2**31), 2**31 - 1)
I64 = (-(2**63), 2**63 - 1)


def test_new_symbols_and_abi_revision():
    with open(HEADER) as f:
        text = f.read()
    assert re.search(r"^#define FA_ABI_VERSION 4\b", text, re.M)
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = {line.split()[-1] for line in out.splitlines() if line.strip()}
    for name in NEW_SYMBOLS:
        assert name in _lib.SYMBOLS
        getattr(_lib.lib(), name)
        assert re.search(r"^int %s\(" % name, text, re.M), name
        assert name in exported, name
    for name in ("histogram_flac_device", "StreamHistogram"):
        assert name in fa.__all__ and hasattr(fa, name)
    for name in ("histogram", "order_statistic", "quantile", "median"):
        assert callable(getattr(fa.FlacArray, name))
    assert callable(fa.DeviceDecodeIndex.histogram)


# ---- the model --------------------------------------------------------------------------------------------------------

def _extreme_rows(dtype, n, rng):
    lo, hi = I32 if dtype == np.int32 else I64
    rows = [
        rng.integers(lo, hi, n, dtype=dtype, endpoint=True),                    # the full range
        np.where(np.arange(n) % 2 == 0, lo, hi).astype(dtype),                  # only the two extremes
        np.full(n, hi, dtype),                                                  # constant at the top
        np.full(n, lo, dtype),                                                  # constant at the bottom
        (hi - rng.integers(0, 5, n)).astype(dtype),                             # a narrow band under the top
        (lo + rng.integers(0, 3000, n)).astype(dtype),                          # a band over the bottom, wider than 2048
        rng.integers(-1000, 1000, n).astype(dtype),
    ]
    x = np.stack(rows)
    x[0, 0], x[0, -1] = lo, hi
    return x


@pytest.mark.parametrize("dtype,bound", [(np.int32, 3), (np.int64, 6)], ids=["int32", "int64"])
@pytest.mark.parametrize("n", [1, 2, 5, 1000])
def test_model_order_statistics_are_exact_within_the_pass_bound(dtype, bound, n):
    rng = np.random.default_rng(100 + n)
    x = _extreme_rows(dtype, n, rng)
    want = np.sort(x, axis=1)
    most = 0
    for k in sorted({0, n // 2, n - 1, (n - 1) // 3}):
        got, passes = M.order_statistic(x, np.full(x.shape[0], k))
        assert np.array_equal(got, want[:, k].astype(np.int64)), (n, k)
        most = max(most, passes)
    assert most <= bound
    if n >= 2:
        assert most == bound  # (row 0 spans the full range: shift0 is 21 / 53)
    per_row = rng.integers(0, n, x.shape[0])
    got, _ = M.order_statistic(x, per_row)
    assert np.array_equal(got, want[np.arange(x.shape[0]), per_row].astype(np.int64))


def test_model_pass_schedule():
    """The first pass at the automatic shift with 2048 bins, every further one 11 bits finer, the last at shift 0."""
    x = np.array([[I32[0], 0, I32[1]], [5, 5, 5], [0, 1 << 20, 3]], dtype=np.int32)
    seen = []
    M.order_statistic(x, np.array([1, 1, 1]), count=lambda lo, sh: seen.append(sh))
    assert [s.tolist() for s in seen] == [[21, 0, 10], [10, 0, 0], [0, 0, 0]]


def test_model_bin_rule_unsigned_subtraction():
    x = np.array([[I64[0], -1, 0, I64[1], I64[1] - 1]], dtype=np.int64)
    c, b, a = M.bin_counts(x, I64[0], 63, 2)
    assert c.tolist() == [[2, 3]] and b.tolist() == [0] and a.tolist() == [0]
    c, b, a = M.bin_counts(x, I64[0] + 1, 62, 3)  # x - lo reaches 2^64 - 2: no signed difference holds it
    assert c.tolist() == [[0, 2, 0]] and b.tolist() == [1] and a.tolist() == [2]  # (-1 and 0 in bin 1, the top two beyond bin 2)
    c, b, a = M.bin_counts(x, 0, 0, 1)
    assert c.tolist() == [[1]] and b.tolist() == [2] and a.tolist() == [2]
    for arr in (c, b, a):
        assert arr.dtype == np.int64


@pytest.mark.parametrize("bins", [1, 2, 255, 256, 2047, 2048])
def test_auto_shift_matches_the_model(bins):
    rng = np.random.default_rng(bins)
    for dtype in (np.int32, np.int64):
        x = _extreme_rows(dtype, 50, rng)
        if bins == 1 and dtype == np.int64:
            x = x[2:]  # (one bin over a span of 2^63 and more would need shift 64)
        lo, sh = M.auto_range(x, bins)
        got = _auto_shift(x.min(axis=1).astype(np.int64), x.max(axis=1).astype(np.int64), bins)
        assert np.array_equal(got, sh) and got.dtype == np.int32
        c, b, a = M.bin_counts(x, lo, sh, bins)
        assert not b.any() and not a.any() and np.all(c.sum(axis=1) == 50)


def test_quantile_rank_is_numpys():
    rng = np.random.default_rng(5)
    for n in (1, 2, 7, 1001, 4099):
        x = np.sort(rng.integers(-1000, 1000, n))
        for q in (0.0, 0.25, 0.5, 0.75, 1.0, 0.1, 0.3333, 0.999, 1e-9):
            for method in ("lower", "higher"):
                assert x[M.quantile_rank(q, n, method)] == np.quantile(x, q, method=method), (n, q, method)


# ---- argument errors --------------------------------------------------------------------------------------------------

@pytest.fixture
def no_library(monkeypatch):
    def reached():
        raise AssertionError("the library was reached before the arguments were checked")

    monkeypatch.setattr(_lib, "lib", reached)
    monkeypatch.setattr(libflacarray, "_stream_ptr", reached)


def _cpu_store(n_stream=6):
    return torch.zeros(4096, dtype=torch.uint8), torch.arange(n_stream, dtype=torch.int64) * 100, torch.full((n_stream,), 100, dtype=torch.int64)


RANGE_ARGS = [
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
BIN_ARGS = [
    ("nbins0", dict(nbins=0)),
    ("nbins_negative", dict(nbins=-1)),
    ("nbins_2049", dict(nbins=2049)),
    ("nbins_float", dict(nbins=16.0)),
    ("shift_negative", dict(shift=-1)),
    ("shift_64", dict(shift=64)),
    ("shift_array_64", dict(shift=np.array([0, 1, 2, 3, 4, 64]))),
    ("shift_float", dict(shift=1.0)),
    ("shift_length", dict(shift=np.zeros(5, np.int32))),
    ("shift_2d", dict(shift=np.zeros((6, 1), np.int32))),
    ("lo_over_int64", dict(lo=2**63)),
    ("lo_under_int64", dict(lo=-(2**63) - 1)),
    ("lo_uint64_over", dict(lo=np.full(6, 2**63, np.uint64))),
    ("lo_float", dict(lo=0.5)),
    ("lo_length", dict(lo=np.zeros(7, np.int64))),
    ("lo_tensor_length", dict(lo=torch.zeros(2, dtype=torch.int64))),
    ("lo_length_of_subset", dict(lo=np.zeros(6, np.int64), streams=[1, 2])),
]


@pytest.mark.parametrize("name,kw", RANGE_ARGS + BIN_ARGS, ids=[b[0] for b in RANGE_ARGS + BIN_ARGS])
def test_histogram_flac_device_argument_errors_need_no_device(no_library, name, kw):
    comp, st, nb = _cpu_store()
    args = dict(lo=0, shift=0, nbins=16)
    args.update(kw)
    with pytest.raises(ValueError):
        fa.histogram_flac_device(comp, st, nb, 1000, **args)


def _host_array(dtype=np.int32):
    """A FlacArray assembled by hand (nothing is encoded: the calls must fail on the arguments before they read a byte)."""
    return fa.FlacArray(None, shape=(2, 3, 1000), global_shape=None, compressed=np.zeros(64, np.uint8), dtype=np.dtype(dtype),
                        stream_starts=np.zeros((2, 3), np.int64), stream_nbytes=np.zeros((2, 3), np.int64))


@pytest.mark.parametrize("name,kw", RANGE_ARGS + BIN_ARGS, ids=[b[0] for b in RANGE_ARGS + BIN_ARGS])
def test_flacarray_histogram_argument_errors_need_no_device(no_library, name, kw):
    kw = {{"first_sample": "first", "last_sample": "last", "nbins": "bins"}.get(k, k): v for k, v in kw.items()}
    with pytest.raises(ValueError):
        _host_array().histogram(**kw)


RANK_ARGS = [
    ("rank_negative", dict(ranks=[-1])),
    ("rank_n", dict(ranks=[1000])),
    ("rank_beyond_range", dict(ranks=[10], first=5, last=15)),
    ("rank_float", dict(ranks=[0.5])),
    ("rank_rows_mismatch", dict(ranks=np.zeros((5, 2), np.int64))),
    ("rank_3d", dict(ranks=np.zeros((6, 1, 1), np.int64))),
    ("rank_scalar", dict(ranks=3)),
]


@pytest.mark.parametrize("name,kw", RANK_ARGS + [(n, dict(kw, ranks=[0])) for n, kw in RANGE_ARGS], ids=[b[0] for b in RANK_ARGS + RANGE_ARGS])
def test_order_statistic_argument_errors_need_no_device(no_library, name, kw):
    kw = {{"first_sample": "first", "last_sample": "last"}.get(k, k): v for k, v in kw.items()}
    with pytest.raises(ValueError):
        _host_array().order_statistic(**kw)


@pytest.mark.parametrize("kw", [dict(q=0.5, method="linear"), dict(q=0.5, method="nearest"), dict(q=-0.1), dict(q=1.5), dict(q=[[0.5]]),
                                dict(q=0.5, first=10, last=10), dict(q=0.5, streams=[9])])
def test_quantile_argument_errors_need_no_device(no_library, kw):
    with pytest.raises(ValueError):
        _host_array().quantile(**kw)


def test_median_argument_errors_need_no_device(no_library):
    for kw in (dict(first=10, last=10), dict(last=1001), dict(streams=[0, 0])):
        with pytest.raises(ValueError):
            _host_array().median(**kw)


def test_empty_streams_return_empty_arrays_without_a_device(no_library):
    comp, st, nb = _cpu_store()
    none = np.zeros(0, np.int64)
    for dt in (np.int32, np.int64):
        h = _host_array(dt).histogram(bins=7, streams=none)
        assert isinstance(h, fa.StreamHistogram)
        assert h.counts.shape == (0, 7) and h.below.shape == (0,) and h.above.shape == (0,) and h.lo.shape == (0,) and h.shift.shape == (0,)
        assert h.counts.dtype == np.int64
        assert h.edges().shape == (0, 8)
        v = _host_array(dt).order_statistic([0, 5], streams=none)
        assert v.shape == (0, 2) and v.dtype == dt
        assert _host_array(dt).median(streams=none).shape == (0,)


# ---- StreamHistogram --------------------------------------------------------------------------------------------------

def test_edges_in_int64_and_beyond():
    z = np.zeros((2,), np.int64)
    h = fa.StreamHistogram(np.zeros((2, 4), np.int64), z, z, np.array([-8, I64[0]], np.int64), np.array([0, 61], np.int32))
    e = h.edges()
    assert e.dtype == np.int64 and e.shape == (2, 5)
    assert e.tolist() == [M.edges(-8, 0, 4), M.edges(I64[0], 61, 4)]
    assert e[1, 4] == 0
    # the last edge of a row that ends at INT64_MAX is 2^63: Python integers
    h = fa.StreamHistogram(np.zeros((2, 4), np.int64), z, z, np.array([-8, I64[0]], np.int64), np.array([0, 62], np.int32))
    e = h.edges()
    assert e.dtype == object and e.shape == (2, 5)
    assert e[1, 4] == 2**63 and isinstance(e[1, 4], int) and e[1].tolist() == M.edges(I64[0], 62, 4)
    assert e[0].tolist() == [-8, -7, -6, -5, -4]
    h = fa.StreamHistogram(np.zeros((1, 2048), np.int64), z[:1], z[:1], np.array([I64[1] - 5], np.int64), np.array([63], np.int32))
    assert h.edges()[0, 2048] == I64[1] - 5 + (2048 << 63)


def test_edges_keep_the_leading_shape():
    lo = np.arange(6, dtype=np.int64).reshape(2, 3) * 100
    h = fa.StreamHistogram(np.zeros((2, 3, 3), np.int64), np.zeros((2, 3), np.int64), np.zeros((2, 3), np.int64), lo, np.full((2, 3), 4, np.int32))
    e = h.edges()
    assert e.shape == (2, 3, 4) and e[1, 2].tolist() == [500, 516, 532, 548]


def test_float_edges_map_through_offset_and_gain():
    z = np.zeros(2, np.int64)
    h = fa.StreamHistogram(np.zeros((2, 2), np.int64), z, z, np.array([-4, 10], np.int64), np.array([1, 0], np.int32),
                           offsets=np.array([1.5, -2.0]), gains=np.array([4.0, 0.5]))
    assert np.array_equal(h.float_edges(), [[1.5 - 1.0, 1.5 - 0.5, 1.5], [-2.0 + 20.0, -2.0 + 22.0, -2.0 + 24.0]])
    assert h.float_edges().dtype == np.float64
    with pytest.raises(ValueError):
        fa.StreamHistogram(np.zeros((2, 2), np.int64), z, z, z, z.astype(np.int32)).float_edges()


def test_stream_histogram_is_frozen():
    z = np.zeros(1, np.int64)
    h = fa.StreamHistogram(np.zeros((1, 2), np.int64), z, z, z, z.astype(np.int32))
    with pytest.raises(Exception):
        h.counts = None
