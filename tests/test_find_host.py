"""Host-side checks of the search (FlacArray.find): the symbols of the C ABI, every argument error as a ValueError raised
before anything touches a device (the library handle raises if it is reached), the bisection that maps float limits to
their exact integer images against brute force with the restore model (tests/quant_model.py) as the callable, and
StreamHits.ranges against the boolean-mask model (tests/find_model.py)."""
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import flacarray_amd as fa
from flacarray_amd import _lib, libflacarray
from flacarray_amd.libflacarray import float_limit_images, float_limits_to_int
from tests import find_model as M
from tests import quant_model as Q
from tests.conftest import ROOT

HEADER = os.path.join(ROOT, "include", "flacarray_hip.h")
NEW_SYMBOLS = ("fa_find_plan_device", "fa_find_plan_indexed", "fa_find_count_i32_device", "fa_find_count_i64_device", "fa_find_count_indexed",
               "fa_find_fill_i32_device", "fa_find_fill_i64_device", "fa_find_fill_indexed")


def test_new_symbols_and_abi_revision():
    with open(HEADER) as f:
        text = f.read()
    assert re.search(r"^#define FA_ABI_VERSION 4\b", text, re.M)
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = {line.split()[-1] for line in out.splitlines() if line.strip()}
    for name in NEW_SYMBOLS:
        assert name in _lib.SYMBOLS
        f = getattr(_lib.lib(), name)
        assert f.argtypes is not None and len(f.argtypes) == len(re.search(r"^int %s\(([^;]*)\);" % name, text, re.M | re.S).group(1).split(",")), name
        assert name in exported, name
    for name in ("find_flac_device", "find_counts_flac_device", "StreamHits"):
        assert name in fa.__all__ and hasattr(fa, name)
    for name in ("find", "find_counts"):
        assert callable(getattr(fa.FlacArray, name)) and callable(getattr(fa.DeviceDecodeIndex, name))


# ---- argument errors --------------------------------------------------------------------------------------------------

@pytest.fixture
def no_library(monkeypatch):
    def reached(*a, **kw):
        raise AssertionError("the library was reached before the arguments were checked")

    monkeypatch.setattr(_lib, "lib", reached)
    monkeypatch.setattr(_lib, "require_device", reached)
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
LIMIT_ARGS = [
    ("lo_length", dict(lo=np.zeros(7, np.int64))),
    ("hi_length", dict(hi=np.zeros(5, np.int64))),
    ("hi_tensor_length", dict(hi=torch.zeros(2, dtype=torch.int64))),
    ("lo_length_of_subset", dict(lo=np.zeros(6, np.int64), streams=[1, 2])),
    ("lo_2d", dict(lo=np.zeros((6, 1), np.int64))),
    ("lo_bool", dict(lo=True)),
    ("hi_bool_array", dict(hi=np.zeros(6, bool))),
    ("lo_bool_in_list", dict(lo=np.array([0, 1, 2, 3, 4, True], dtype=object))),
    ("lo_over_int64", dict(lo=2**63)),
    ("hi_under_int64", dict(hi=-(2**63) - 1)),
    ("lo_string", dict(lo="3")),
    ("inside_int", dict(inside=1)),
    ("max_hits_negative", dict(max_hits=-1)),
    ("max_hits_float", dict(max_hits=10.0)),
    ("max_hits_bool", dict(max_hits=True)),
]
INT_ONLY = [
    ("lo_float", dict(lo=0.5)),
    ("hi_float_array", dict(hi=np.zeros(6, np.float64))),
    ("lo_nan", dict(lo=float("nan"))),
    ("hi_inf", dict(hi=float("inf"))),
]


@pytest.mark.parametrize("name,kw", RANGE_ARGS + LIMIT_ARGS + INT_ONLY, ids=[b[0] for b in RANGE_ARGS + LIMIT_ARGS + INT_ONLY])
def test_find_flac_device_argument_errors_need_no_device(no_library, name, kw):
    comp, st, nb = _cpu_store()
    with pytest.raises(ValueError):
        fa.find_flac_device(comp, st, nb, 1000, **kw)
    kw = {k: v for k, v in kw.items() if k != "max_hits"}
    if kw:
        with pytest.raises(ValueError):
            fa.find_counts_flac_device(comp, st, nb, 1000, **kw)


def _host_array(dtype=np.int32, gains=None):
    """A FlacArray assembled by hand (nothing is encoded: the calls must fail on the arguments before they read a byte)."""
    kw = {}
    if np.dtype(dtype).kind == "f":
        kw = dict(stream_offsets=np.zeros((2, 3), dtype), stream_gains=np.ones((2, 3), dtype) if gains is None else np.asarray(gains, dtype).reshape(2, 3))
    return fa.FlacArray(None, shape=(2, 3, 1000), global_shape=None, compressed=np.zeros(64, np.uint8), dtype=np.dtype(dtype),
                        stream_starts=np.zeros((2, 3), np.int64), stream_nbytes=np.zeros((2, 3), np.int64), **kw)


def _array_kw(kw):
    return {{"first_sample": "first", "last_sample": "last"}.get(k, k): v for k, v in kw.items()}


@pytest.mark.parametrize("dtype", [np.int32, np.int64], ids=["int32", "int64"])
@pytest.mark.parametrize("name,kw", RANGE_ARGS + LIMIT_ARGS + INT_ONLY, ids=[b[0] for b in RANGE_ARGS + LIMIT_ARGS + INT_ONLY])
def test_flacarray_find_argument_errors_need_no_device(no_library, name, kw, dtype):
    with pytest.raises(ValueError):
        _host_array(dtype).find(**_array_kw(kw))
    kw = {k: v for k, v in kw.items() if k != "max_hits"}
    if kw:
        with pytest.raises(ValueError):
            _host_array(dtype).find_counts(**_array_kw(kw))


FLOAT_ARGS = [
    ("lo_nan", dict(lo=float("nan"))),
    ("hi_nan_in_array", dict(hi=np.array([0, 1, 2, np.nan, 4, 5.0]))),
    ("lo_bool", dict(lo=False)),
    ("lo_length", dict(lo=np.zeros(5))),
    ("lo_complex", dict(lo=1j)),
    ("quantised_float", dict(lo=0.5, quantised=True)),
    ("quantised_not_bool", dict(lo=0, quantised=1)),
]


@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["float32", "float64"])
@pytest.mark.parametrize("name,kw", RANGE_ARGS + FLOAT_ARGS, ids=[b[0] for b in RANGE_ARGS + FLOAT_ARGS])
def test_flacarray_find_float_argument_errors_need_no_device(no_library, name, kw, dtype):
    with pytest.raises(ValueError):
        _host_array(dtype).find(**_array_kw(kw))
    with pytest.raises(ValueError):
        _host_array(dtype).find_counts(**_array_kw(kw))


@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["float32", "float64"])
@pytest.mark.parametrize("gain", [0.0, -2.0, np.inf, np.nan])
def test_float_limits_need_finite_positive_gains(no_library, dtype, gain):
    arr = _host_array(dtype, gains=[1.0, 1.0, gain, 1.0, 1.0, 1.0])
    with pytest.raises(ValueError, match="gain"):
        arr.find(lo=-1.0, hi=1.0)
    with pytest.raises(ValueError, match="gain"):
        arr.find_counts(lo=-1.0, hi=1.0, streams=[2])


def test_empty_streams_return_empty_results_without_a_device(no_library):
    none = np.zeros(0, np.int64)
    for dt in (np.int32, np.int64, np.float32, np.float64):
        h = _host_array(dt).find(lo=0, hi=1, streams=none)
        assert isinstance(h, fa.StreamHits)
        assert h.counts.shape == (0,) and h.offsets.tolist() == [0] and h.positions.shape == (0,) and h.rows.shape == (0,)
        assert h.values.dtype == np.dtype(dt) and h.values.shape == (0,) and h.int_values.dtype == np.int64
        assert h.ranges(3).shape == (0, 3)
        c = _host_array(dt).find_counts(lo=0, hi=1, streams=[])
        assert c.shape == (0,) and c.dtype == np.int64


# ---- float limits -> integer images -------------------------------------------------------------------------------------

def _monotone_rows(case, dtype):
    """The rows of a restore case on which offset + coeff * float(q) is non-decreasing in q and never NaN: a finite
    positive gain whose reciprocal (as the restore forms it) is finite, and a finite offset."""
    g = np.asarray(case.gains, dtype=dtype).astype(np.float64)
    with np.errstate(all="ignore"):
        coeff = (1.0 / g).astype(dtype)
    return np.flatnonzero(np.isfinite(g) & (g > 0) & np.isfinite(coeff) & np.isfinite(np.asarray(case.offsets, dtype=np.float64)))


def _restore_for(dtype, off, gain):
    it = np.int32 if dtype == np.float32 else np.int64

    def restore(q):
        return Q.restore(np.asarray(q).astype(it).reshape(-1, 1), off, gain).reshape(-1)

    return restore


@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["float32", "float64"])
def test_limit_images_against_brute_force_in_a_small_range(dtype):
    """Every q of [-300, 300] is enumerated: the images are the first q at or above lo and the last at or below hi."""
    case = Q.restore_cases(dtype)[0]
    keep = _monotone_rows(case, dtype)
    assert keep.size >= 3
    off, gain = np.asarray(case.offsets)[keep], np.asarray(case.gains)[keep]
    restore = _restore_for(dtype, off, gain)
    qmin, qmax = -300, 300
    qs = np.arange(qmin, qmax + 1)
    table = np.stack([restore(np.full(keep.size, q)) for q in qs], axis=1).astype(np.float64)  # [rows, q]
    assert np.all(table[:, 1:] >= table[:, :-1])
    mid = table[:, 310]
    limits = []
    for v in (mid, np.nextafter(mid, -np.inf), np.nextafter(mid, np.inf),
              np.nextafter(mid.astype(dtype), dtype(-np.inf)).astype(np.float64), np.nextafter(mid.astype(dtype), dtype(np.inf)).astype(np.float64),
              (table[:, 310] + table[:, 311]) / 2, table[:, 0], table[:, -1], table[:, 0] - np.abs(table[:, 0]) - 1, table[:, -1] + np.abs(table[:, -1]) + 1,
              np.full(keep.size, -np.inf), np.full(keep.size, np.inf)):
        limits.append(np.asarray(v, dtype=np.float64))
    for lo in limits:
        for hi in limits:
            lo_q, hi_q = float_limit_images(restore, lo, hi, qmin, qmax)
            for r in range(keep.size):
                ge = np.flatnonzero(table[r] >= lo[r])
                le = np.flatnonzero(table[r] <= hi[r])
                assert lo_q[r] == (qs[ge[0]] if ge.size else qmax + 1), (r, lo[r])
                assert hi_q[r] == (qs[le[-1]] if le.size else qmin - 1), (r, hi[r])


@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["float32", "float64"])
def test_limit_images_over_the_restore_corpus(dtype):
    """The full integer range: limits exactly on a restored value, one ulp either side (of the store's type and of
    float64), between two neighbours, beyond both ends and +-inf.  The images split every probed q -- the case's own
    integers, the range's ends, the images and their neighbours -- exactly as the float comparison does."""
    it = np.int32 if dtype == np.float32 else np.int64
    ii = np.iinfo(it)
    qmin, qmax = int(ii.min), int(ii.max)
    calls = []
    for case in Q.restore_cases(dtype)[:3]:
        keep = _monotone_rows(case, dtype)
        off, gain = np.asarray(case.offsets)[keep], np.asarray(case.gains)[keep]
        inner = _restore_for(dtype, off, gain)

        def restore(q):
            calls[-1] += 1
            return inner(q)

        ints = np.asarray(case.ints)[keep]
        for col in (0, 1, 3, 6, ints.shape[1] - 1):
            q0 = ints[:, col].astype(np.int64)
            v = inner(q0).astype(np.float64)
            nxt = inner(np.minimum(q0, qmax - 1) + 1).astype(np.float64)
            one_ulp = lambda x, d: np.nextafter(x.astype(dtype), dtype(d)).astype(np.float64)  # noqa: E731
            for lo, hi in ((v, v), (one_ulp(v, -np.inf), one_ulp(v, np.inf)), (one_ulp(v, np.inf), one_ulp(v, -np.inf)),
                           (np.nextafter(v, np.inf), np.nextafter(v, -np.inf)), ((v + nxt) / 2, (v + nxt) / 2),
                           (np.full(v.size, -np.inf), np.full(v.size, np.inf)), (np.full(v.size, np.inf), np.full(v.size, -np.inf)),
                           (inner(np.full(v.size, qmin)).astype(np.float64) - 1e300, inner(np.full(v.size, qmax)).astype(np.float64) + 1e300)):
                calls.append(0)
                lo_q, hi_q = float_limit_images(restore, lo, hi, qmin, qmax)
                assert calls[-1] <= 2 * 65, calls[-1]
                lo_i, hi_i = float_limits_to_int(inner, lo, hi, qmin, qmax)
                probes = [q0, np.full(v.size, qmin), np.full(v.size, qmax), np.zeros(v.size, np.int64)]
                for img in (lo_q, hi_q):
                    for d in (-1, 0, 1):
                        probes.append(np.array([min(max(int(e) + d, qmin), qmax) for e in img], dtype=np.int64))
                for q in probes:
                    x = inner(q).astype(np.float64)
                    qo = q.astype(object)
                    assert np.array_equal(x < lo, qo < lo_q), (case.name, col)
                    assert np.array_equal(x > hi, qo > hi_q), (case.name, col)
                    assert np.array_equal((x < lo) | (x > hi), (q < lo_i) | (q > hi_i)), (case.name, col)
                assert lo_i.dtype == np.int64 and hi_i.dtype == np.int64


# ---- StreamHits.ranges ---------------------------------------------------------------------------------------------------

def _hits(counts, positions, first, last, streams=None):
    counts = np.asarray(counts, dtype=np.int64)
    offsets = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
    rows = np.repeat(np.arange(counts.size), counts).astype(np.int64)
    pos = np.asarray(positions, dtype=np.int64)
    return fa.StreamHits(counts, offsets, rows, pos, pos.astype(np.int32), pos.copy(), first, last, None if streams is None else np.asarray(streams))


@pytest.mark.parametrize("pad", [0, 1, 2, 7, 1000])
def test_ranges_against_the_mask_model(pad):
    first, last = 10, 60
    per_row = [[10, 11, 13, 20, 59], [], [12, 14, 17, 30, 31, 32, 58], [59], [10], [35]]  # hits at first and last - 1, an empty row
    counts = [len(p) for p in per_row]
    pos = [p for row in per_row for p in row]
    for streams in (None, [7, 3, 5, 0, 9, 2]):
        h = _hits(counts, pos, first, last, streams)
        got = h.ranges(pad)
        want = M.ranges(len(per_row), h.rows, h.positions, first, last, pad, streams)
        assert got.dtype == np.int64 and got.shape == want.shape and np.array_equal(got, want), (pad, got.tolist(), want.tolist())
        assert np.all(got[:, 1] >= first) and np.all(got[:, 2] <= last) and np.all(got[:, 1] < got[:, 2])
    if pad == 0:
        assert got.tolist()[:4] == [[7, 10, 12], [7, 13, 14], [7, 20, 21], [7, 59, 60]]
    if pad == 1000:
        assert got.tolist() == [[7, 10, 60], [5, 10, 60], [0, 10, 60], [9, 10, 60], [2, 10, 60]]


def test_ranges_random_against_the_mask_model():
    rng = np.random.default_rng(3)
    for trial in range(20):
        first = int(rng.integers(0, 50))
        last = first + int(rng.integers(1, 200))
        per_row = [np.sort(rng.choice(np.arange(first, last), size=int(rng.integers(0, min(last - first, 30) + 1)), replace=False)) for _ in range(4)]
        h = _hits([p.size for p in per_row], np.concatenate(per_row), first, last)
        for pad in (0, 1, 3, 50):
            assert np.array_equal(h.ranges(pad), M.ranges(4, h.rows, h.positions, first, last, pad)), (trial, pad)


def test_ranges_argument_errors():
    h = _hits([1], [3], 0, 10)
    for pad in (-1, 1.5, True, None):
        with pytest.raises(ValueError):
            h.ranges(pad)
