"""Host-side checks of the projections (FlacArray.dot): the limb split of wide templates and its inverse on the extreme
values, a numpy model of the kernel's two accumulators against the exact product sum, StreamDots.value() on hand-made
fields, every argument error raised before anything touches a device (the library handle raises if it is reached), and the
three entry points declared, listed and exported."""
import math
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import flacarray_amd as fa
from flacarray_amd import _lib, libflacarray
from flacarray_amd.libflacarray import dot_exact, dot_template_limbs, dot_template_unlimbs
from tests import dot_corpus as C
from tests.conftest import ROOT

HEADER = os.path.join(ROOT, "include", "flacarray_hip.h")
NEW_SYMBOLS = ("fa_dot_i32_device", "fa_dot_i64_device", "fa_dot_indexed")


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
    for name in ("dot_flac_device", "StreamDots", "dot_template_limbs", "dot_template_unlimbs", "dot_exact"):
        assert name in fa.__all__ and hasattr(fa, name)
    assert callable(fa.FlacArray.dot) and callable(fa.DeviceDecodeIndex.dot)


# ---- the limb split -----------------------------------------------------------------------------------------------------

EXTREMES = [C.INT64_MIN, C.INT64_MIN + 1, -(2**62) - 1, -(2**62), -(2**31) - 1, C.INT32_MIN, -1, 0, 1, C.INT32_MAX, 2**31, 2**62 - 1, 2**62,
            C.INT64_MAX - 1, C.INT64_MAX]


def test_limb_split_of_the_extreme_values():
    # one template per value among zeros: never fits int32 by accident of its neighbours
    T = np.zeros((len(EXTREMES), 3), dtype=np.int64)
    T[:, 1] = EXTREMES
    planes, index = dot_template_limbs(T)
    assert planes.dtype == np.int32 and index.dtype == np.int64 and planes.shape == (index.shape[0], 3)
    for k, v in enumerate(EXTREMES):
        mine = [(int(j), planes[m]) for m, (kk, j) in enumerate(index) if kk == k]
        if C.INT32_MIN <= v <= C.INT32_MAX:
            assert (len(mine) == 1 and mine[0][0] == 0 and int(mine[0][1][1]) == v) or (v == 0 and not mine), v
            continue
        assert sum(int(p[1]) << (31 * j) for j, p in mine) == v, v
        for j, p in mine:
            assert np.any(p != 0), (v, j)  # planes that are all zero are dropped
            assert (0 <= int(p[1]) < 2**31) if j < 2 else (-2 <= int(p[1]) <= 1), (v, j)
    # the inverse on products: x * T for a few x, through the planes
    xs = [C.INT32_MIN, -3, 0, 7, C.INT32_MAX]
    products = np.array([[x * sum(int(v) for v in planes[m]) for m in range(planes.shape[0])] for x in xs], dtype=object)
    back = dot_template_unlimbs(products, index, len(EXTREMES))
    assert back.shape == (len(xs), len(EXTREMES))
    for r, x in enumerate(xs):
        assert [back[r, k] for k in range(len(EXTREMES))] == [x * v for v in EXTREMES]


def test_limb_split_of_the_corpus_templates():
    n = 213
    T = C.wide_templates(n)
    planes, index = dot_template_limbs(T)
    per = {k: sorted(int(j) for kk, j in index if kk == k) for k in range(5)}
    assert per == {0: [0, 1, 2], 1: [0, 1, 2], 2: [1], 3: [0], 4: []}
    rebuilt = dot_template_unlimbs(planes.astype(object).T, index, 5)  # (the planes themselves as "products" of 1)
    assert np.array_equal(rebuilt, T.astype(object).T)
    # narrow templates are left alone, negative values included
    N = C.templates(9, n)
    planes, index = dot_template_limbs(N)
    assert np.array_equal(planes, N.astype(np.int32)) and index.tolist() == [[k, 0] for k in range(9)]
    with pytest.raises(TypeError):
        dot_template_limbs(np.zeros((1, 4)))
    with pytest.raises(ValueError):
        dot_template_limbs(np.array([[2**63]], dtype=np.uint64))
    with pytest.raises(ValueError):
        dot_template_limbs(np.zeros(4, np.int64))


# ---- the kernel's accumulators ------------------------------------------------------------------------------------------

def test_accumulator_model_equals_the_exact_sum_on_the_corner_values():
    corner = [C.INT32_MIN, -1, 0, 1, C.INT32_MAX]
    for x in corner:
        for t in corner:
            for reps in (1, 2, 65535):  # a frame has at most 65535 samples: neither accumulator may wrap inside it
                hi, lo = C.kernel_model(np.full(reps, x), np.full(reps, t))
                assert hi * 2**32 + lo == reps * x * t, (x, t, reps)
                assert -(2**63) <= hi < 2**63 and 0 <= lo < 2**64
    # mixed signs in one sum, and the combination the device calls' results go through
    rng = np.random.default_rng(5)
    x = rng.choice(corner, 4096)
    t = rng.choice(corner, 4096)
    hi, lo = C.kernel_model(x, t)
    exact = sum(int(a) * int(b) for a, b in zip(x, t))
    assert hi * 2**32 + lo == exact
    got = dot_exact(torch.tensor([[hi]], dtype=torch.int64), torch.from_numpy(np.array([[lo]], dtype=np.uint64).view(np.int64)))
    assert got.dtype == object and got[0, 0] == exact
    # a logical shift of the upper limb, the mistake the signed limb invites, is caught by any negative product
    p = np.int64(-1) * np.int64(1)
    assert (int(np.uint64(p) >> np.uint64(32)) << 32) + int(np.uint64(p) & np.uint64(0xFFFFFFFF)) != -1


def test_two_channel_combination():
    # x = xh * 2^32 + xl against t: (hi, lo) of xl * t and of xh * t
    for x in (C.INT64_MIN, -(2**40) - 3, -1, 0, 5, 2**32, C.INT64_MAX):
        for t in (C.INT32_MIN, -1, 0, 1, C.INT32_MAX):
            xl, xh = x & 0xFFFFFFFF, x >> 32
            pl, ph = xl * t, xh * t
            assert -(2**63) <= pl < 2**63 and -(2**63) <= ph < 2**63
            cell = np.array([[[pl >> 32, pl & 0xFFFFFFFF, ph >> 32, ph & 0xFFFFFFFF]]], dtype=np.int64)
            assert dot_exact(cell)[0, 0] == x * t, (x, t)


# ---- StreamDots ---------------------------------------------------------------------------------------------------------

def test_stream_dots_value_on_hand_made_fields():
    exact = np.array([[3, -(2**70)], [2**53 + 1, 0]], dtype=object)
    d = fa.StreamDots(exact, np.array([10, -4], dtype=object), 7)
    v = d.value()
    assert v.dtype == np.float64 and v.shape == (2, 2)
    assert v.tolist() == [[3.0, -float(2**70)], [float(2**53 + 1), 0.0]]
    # a float store: offset[r] * template_sum[k] + exact[r, k] / gain[r], every row with its own gain
    off = np.array([[0.5], [-2.0]])
    gain = np.array([[4.0], [1024.0]])
    f = fa.StreamDots(exact, np.array([10, -4], dtype=object), 7, off, gain).value()
    want = [[0.5 * 10 + 3 / 4.0, 0.5 * -4 + float(-(2**70)) / 4.0], [-2.0 * 10 + float(2**53 + 1) / 1024.0, -2.0 * -4 + 0.0]]
    assert f.tolist() == want
    # one 1-D template: no K axis anywhere
    one = fa.StreamDots(np.array([6, -9], dtype=object), 5, 7, np.array([1.0, 2.0]), np.array([3.0, 3.0])).value()
    assert one.tolist() == [1.0 * 5 + 6 / 3.0, 2.0 * 5 + -9 / 3.0]
    assert math.isfinite(fa.StreamDots(np.array([[2**32 * 2**63 * 2**31]], dtype=object), np.array([0], dtype=object), 1).value()[0, 0])


# ---- refusals, before the device ----------------------------------------------------------------------------------------

@pytest.fixture
def no_library(monkeypatch):
    def reached():
        raise AssertionError("the library was reached before the arguments were checked")

    monkeypatch.setattr(_lib, "lib", reached)
    monkeypatch.setattr(libflacarray, "_stream_ptr", reached)


def _cpu_store(n_stream=6):
    return torch.zeros(4096, dtype=torch.uint8), torch.arange(n_stream, dtype=torch.int64) * 100, torch.full((n_stream,), 100, dtype=torch.int64)


def _host_array(dtype=np.int32, **kw):
    """A FlacArray assembled by hand (nothing is encoded: the calls must fail on the arguments before they read a byte)."""
    return fa.FlacArray(None, shape=(2, 3, 1000), global_shape=None, compressed=np.zeros(64, np.uint8), dtype=np.dtype(dtype),
                        stream_starts=np.zeros((2, 3), np.int64), stream_nbytes=np.zeros((2, 3), np.int64), **kw)


I32 = lambda *shape: np.ones(shape, dtype=np.int32)  # noqa: E731

REFUSALS = [
    ("length_short", ValueError, dict(templates=I32(2, 999))),
    ("length_long", ValueError, dict(templates=I32(1001))),
    ("length_of_the_range", ValueError, dict(templates=I32(2, 1000), first_sample=10, last_sample=20)),
    ("no_template", ValueError, dict(templates=I32(0, 1000))),
    ("three_axes", ValueError, dict(templates=I32(1, 1, 1000))),
    ("float32", TypeError, dict(templates=np.ones((2, 1000), np.float32))),
    ("float64_1d", TypeError, dict(templates=np.ones(1000))),
    ("bool", TypeError, dict(templates=np.ones((2, 1000), bool))),
    ("complex", TypeError, dict(templates=np.ones((2, 1000), complex))),
    ("strings", TypeError, dict(templates=np.array([["a"] * 1000]))),
    ("float_tensor", TypeError, dict(templates=torch.ones((2, 1000)))),
    ("beyond_int64", ValueError, dict(templates=np.full((1, 1000), 2**63, dtype=np.uint64))),
    ("empty_range", ValueError, dict(templates=I32(1, 0), first_sample=10, last_sample=10)),
    ("first_after_last", ValueError, dict(templates=I32(1, 1), first_sample=11, last_sample=10)),
    ("first_negative", ValueError, dict(templates=I32(1, 11), first_sample=-1, last_sample=10)),
    ("last_beyond", ValueError, dict(templates=I32(1, 1001), last_sample=1001)),
    ("streams_twice", ValueError, dict(templates=I32(1, 1000), streams=[3, 1, 3])),
    ("streams_beyond", ValueError, dict(templates=I32(1, 1000), streams=[0, 6])),
    ("streams_negative", ValueError, dict(templates=I32(1, 1000), streams=[-1])),
    ("streams_2d", ValueError, dict(templates=I32(1, 1000), streams=np.zeros((2, 2), np.int64))),
]


@pytest.mark.parametrize("name,exc,kw", REFUSALS, ids=[r[0] for r in REFUSALS])
def test_flacarray_dot_argument_errors_need_no_device(no_library, name, exc, kw):
    kw = {{"first_sample": "first", "last_sample": "last"}.get(k, k): v for k, v in kw.items()}
    with pytest.raises(exc) as e:
        _host_array().dot(**kw)
    if name.startswith("float"):
        assert "np.rint(T * 2**k)" in str(e.value)


@pytest.mark.parametrize("name,exc,kw", REFUSALS, ids=[r[0] for r in REFUSALS])
def test_dot_flac_device_argument_errors_need_no_device(no_library, name, exc, kw):
    comp, st, nb = _cpu_store()
    kw = dict(kw)
    t = kw.pop("templates")
    if name == "beyond_int64":
        exc = TypeError  # (and int32 only: wider templates are split by FlacArray.dot)
    with pytest.raises(exc):
        fa.dot_flac_device(comp, st, nb, 1000, t, **kw)


def test_device_calls_take_int32_templates_only(no_library):
    comp, st, nb = _cpu_store()
    with pytest.raises(TypeError) as e:
        fa.dot_flac_device(comp, st, nb, 1000, np.ones((2, 1000), np.int64))
    assert "dot_template_limbs" in str(e.value)
    # accepted arguments go on towards the device, which is not there
    with pytest.raises(Exception) as e:
        fa.dot_flac_device(comp, st, nb, 1000, I32(2, 1000))
    assert not isinstance(e.value, (ValueError, TypeError))
    with pytest.raises(Exception) as e:
        _host_array().dot(np.full((3, 1000), 2**40, dtype=np.int64))
    assert not isinstance(e.value, (ValueError, TypeError))
    # a range of 2^32 samples is refused on the host as the library refuses it
    with pytest.raises(ValueError):
        libflacarray._dot_args(4, 2**32 + 5, 0, 2**32, None)
    first, last, order, rows = libflacarray._dot_args(131, 300, 0, None, None)
    assert (first, last) == (0, 300) and rows.tolist() == [[0, 0, 64], [0, 64, 64], [0, 128, 3]] and order.tolist() == list(range(131))
