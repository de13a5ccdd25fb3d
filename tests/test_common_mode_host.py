"""Host-side checks of the fold across streams (FlacArray.common_mode): the plan against brute force, the arithmetic of
CrossStreamStats against Python integers, the rules for float stores, every argument error as a ValueError raised before
anything touches a device (the library handle raises if it is reached), and the three entry points declared, listed and
exported."""
import math
import os
import re
import subprocess
from fractions import Fraction

import numpy as np
import pytest
import torch

import flacarray_amd as fa
from flacarray_amd import _lib, libflacarray
from flacarray_amd.libflacarray import xsum_plan
from tests import xsum_corpus as C
from tests.conftest import ROOT

HEADER = os.path.join(ROOT, "include", "flacarray_hip.h")
NEW_SYMBOLS = ("fa_xsum_i32_device", "fa_xsum_i64_device", "fa_xsum_indexed")


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
    for name in ("common_mode_flac_device", "CrossStreamStats"):
        assert name in fa.__all__ and hasattr(fa, name)
    assert callable(fa.FlacArray.common_mode) and callable(fa.DeviceDecodeIndex.common_mode)


# ---- the plan ---------------------------------------------------------------------------------------------------------

def check_plan(lab, G):
    perm, rows, count = xsum_plan(lab, G)
    lab = np.asarray(lab)
    assert perm.dtype == np.int64 and rows.dtype == np.int64 and rows.shape[1:] == (3,) and count.shape == (G,)
    assert sorted(perm.tolist()) == list(range(lab.size))
    seen = np.zeros(lab.size, dtype=np.int64)  # how many real lanes hold each selected stream
    lanes = np.zeros(G, dtype=np.int64)        # lanes (real and padding) of each group
    for g, pos0, real in rows.tolist():
        assert 0 <= g < G and 1 <= real <= 64 and 0 <= pos0 and pos0 + real <= lab.size
        for p in perm[pos0 : pos0 + real]:
            assert lab[p] == g  # a row holds streams of its group only
            seen[p] += 1
        lanes[g] += 64
    assert np.all(seen == 1)  # every selected stream in exactly one real lane
    for g in range(G):
        members = np.flatnonzero(lab == g)
        assert count[g] == members.size
        assert lanes[g] == -(-members.size // 64) * 64  # padded to the next multiple of 64, no further
        # stable: a group's streams keep the caller's order
        mine = [p for r in rows.tolist() if r[0] == g for p in perm[r[1] : r[1] + r[2]].tolist()]
        assert mine == members.tolist()
    # the rows of a group are adjacent and only its last one is short
    gs = rows[:, 0].tolist()
    assert gs == sorted(gs)
    for i in range(len(gs) - 1):
        if gs[i] == gs[i + 1]:
            assert rows[i, 2] == 64 and rows[i + 1, 1] == rows[i, 1] + 64
    return rows


def test_plan_six_sizes_interleaved_against_brute_force():
    lab, _ = C.interleaved(C.SIX_SIZES, seed=3)
    assert lab.size == 323 and np.any(np.diff(lab) < 0)
    rows = check_plan(lab, len(C.SIX_SIZES))
    per_group = np.bincount(rows[:, 0], minlength=6).tolist()
    assert per_group == [0, 1, 1, 1, 2, 3]
    assert sorted(rows[:, 2].tolist()) == sorted([1, 63, 64, 64, 1, 64, 64, 2])


@pytest.mark.parametrize("lab,G", [([], 1), ([], 3), ([0], 1), ([2, 2, 2], 4), (list(range(5)) * 30, 5), ([0] * 64, 1), ([0] * 128, 2)])
def test_plan_small_cases(lab, G):
    check_plan(np.asarray(lab, dtype=np.int64), G)


def test_plan_refuses_labels_outside_the_groups():
    for lab, G in (([0, 3], 3), ([-1, 0], 2), ([0], 0)):
        with pytest.raises(ValueError):
            xsum_plan(np.asarray(lab), G)


# ---- CrossStreamStats ---------------------------------------------------------------------------------------------------

def _stats_of(x, lab, G, off_mean=None, gain=None):
    count, sm, sq = C.expected(x, 0, x.shape[1], None, lab, G)
    hi = np.array([[int(v) >> 32 for v in r] for r in sq], dtype=np.uint64)
    lo = np.array([[int(v) & 0xFFFFFFFF for v in r] for r in sq], dtype=np.uint64)
    # (the limbs of the SUM are not the sums of the limbs; mean / std only use hi * 2^32 + lo, which is the same)
    return fa.CrossStreamStats(count, sm, hi, lo, off_mean, gain), count, sm, sq


def test_mean_and_std_against_python_integers():
    rng = np.random.default_rng(2)
    x = rng.integers(-(2**31), 2**31, (40, 17), dtype=np.int64).astype(np.int32)
    x[:, 3] = 2**31 - 1  # no scatter at all: std exactly 0
    x[:, 4] = np.where(np.arange(40) % 2 == 0, 2**31 - 1, 2**31 - 2)  # tiny scatter on a huge level: cancellation
    lab = rng.integers(0, 3, 40)
    lab[lab == 1] = 2  # group 1 is empty
    s, count, sm, sq = _stats_of(x, lab, 4)
    mean, std = s.mean(), s.std()
    assert mean.shape == std.shape == (4, 17) and mean.dtype == std.dtype == np.float64
    for g in range(4):
        if count[g] == 0:
            assert np.all(np.isnan(mean[g])) and np.all(np.isnan(std[g]))
            continue
        c = int(count[g])
        for j in range(17):
            assert mean[g, j] == int(sm[g, j]) / c  # Python's integer division: correctly rounded
            var = Fraction(c * int(sq[g, j]) - int(sm[g, j]) ** 2, c * c)
            assert var >= 0
            assert std[g, j] == math.sqrt(var.numerator / var.denominator)
    assert np.all(std[[0, 2, 3], 3][count[[0, 2, 3]] > 0] == 0.0)
    assert np.all(std[0, 4] <= 0.5) and std[0, 4] > 0.0
    assert np.array_equal(s.sumsq, s.sumsq_hi.astype(np.float64) * 2.0**32 + s.sumsq_lo.astype(np.float64))


def test_float_fields_scale_mean_and_std():
    rng = np.random.default_rng(5)
    x = rng.integers(-(2**20), 2**20, (10, 9)).astype(np.int32)
    lab = np.array([0, 0, 0, 1, 1, 1, 1, 0, 0, 0])
    plain, count, sm, sq = _stats_of(x, lab, 3)
    off_mean = np.array([0.25, -3.0, np.nan])
    gain = np.array([-1024.0, 8.0, np.nan])
    s = fa.CrossStreamStats(plain.count, plain.sum, plain.sumsq_hi, plain.sumsq_lo, off_mean, gain)
    m, sd = s.mean(), s.std()
    for g in (0, 1):
        assert np.array_equal(m[g], off_mean[g] + plain.mean()[g] / gain[g])
        assert np.array_equal(sd[g], plain.std()[g] / abs(gain[g]))
    assert np.all(np.isnan(m[2])) and np.all(np.isnan(sd[2]))
    with pytest.raises(ValueError):
        fa.CrossStreamStats(plain.count, plain.sum, None, None).std()
    assert fa.CrossStreamStats(plain.count, plain.sum, None, None).sumsq is None


# ---- argument errors need no device -------------------------------------------------------------------------------------

@pytest.fixture
def no_library(monkeypatch):
    def reached():
        raise AssertionError("the library was reached before the arguments were checked")

    monkeypatch.setattr(_lib, "lib", reached)
    monkeypatch.setattr(libflacarray, "_stream_ptr", reached)


def _cpu_store(n_stream=6):
    return torch.zeros(4096, dtype=torch.uint8), torch.arange(n_stream, dtype=torch.int64) * 100, torch.full((n_stream,), 100, dtype=torch.int64)


REFUSALS = [
    ("streams_twice", dict(streams=[3, 1, 3])),
    ("streams_beyond", dict(streams=[0, 6])),
    ("streams_negative", dict(streams=[-1])),
    ("streams_2d", dict(streams=np.zeros((2, 2), np.int64))),
    ("label_beyond", dict(groups=[0, 1, 2, 0, 1, 3], n_groups=3)),
    ("label_negative", dict(groups=[0, 1, 2, 0, 1, -1], n_groups=3)),
    ("label_negative_auto", dict(groups=[0, 1, 2, 0, 1, -1])),
    ("labels_length", dict(groups=[0, 1, 2])),
    ("labels_length_of_subset", dict(groups=[0, 1, 0, 1, 0, 1], streams=[1, 2])),
    ("labels_float", dict(groups=np.zeros(6))),
    ("labels_2d", dict(groups=np.zeros((6, 1), np.int64))),
    ("n_groups_0", dict(n_groups=0)),
    ("squares_with_int64", dict(squares=True, is_int64=True)),
    ("first_after_last", dict(first_sample=11, last_sample=10)),
    ("first_negative", dict(first_sample=-1, last_sample=10)),
    ("last_beyond", dict(last_sample=1001)),
]


@pytest.mark.parametrize("name,kw", REFUSALS, ids=[r[0] for r in REFUSALS])
def test_common_mode_flac_device_argument_errors_need_no_device(no_library, name, kw):
    comp, st, nb = _cpu_store()
    with pytest.raises(ValueError):
        fa.common_mode_flac_device(comp, st, nb, 1000, **kw)


def _host_array(dtype=np.int32, **kw):
    """A FlacArray assembled by hand (nothing is encoded: the calls must fail on the arguments before they read a byte)."""
    return fa.FlacArray(None, shape=(2, 3, 1000), global_shape=None, compressed=np.zeros(64, np.uint8), dtype=np.dtype(dtype),
                        stream_starts=np.zeros((2, 3), np.int64), stream_nbytes=np.zeros((2, 3), np.int64), **kw)


@pytest.mark.parametrize("name,kw", [r for r in REFUSALS if not ({"n_groups", "squares"} & set(r[1]))],
                         ids=[r[0] for r in REFUSALS if not ({"n_groups", "squares"} & set(r[1]))])
def test_flacarray_common_mode_argument_errors_need_no_device(no_library, name, kw):
    kw = {{"first_sample": "first", "last_sample": "last"}.get(k, k): v for k, v in kw.items()}
    with pytest.raises(ValueError):
        _host_array().common_mode(**kw)


def test_mixed_gains_are_refused_before_the_device_and_name_the_ways_out(no_library):
    gains = np.full((2, 3), 1024.0, np.float32)
    gains[1, 1] = np.nextafter(np.float32(1024.0), np.float32(2048.0))  # one ulp: not "shared bit for bit"
    arr = _host_array(np.float32, stream_offsets=np.zeros((2, 3), np.float32), stream_gains=gains)
    with pytest.raises(ValueError) as e:
        arr.common_mode()
    assert "quanta=" in str(e.value) and "quantised=True" in str(e.value)
    # a grouping that keeps the odd stream to itself shares a gain within every group, and so do quantised=True and a
    # subset without it: not refused (the call goes on towards the device, which is not there)
    for kw in (dict(groups=[0, 0, 0, 0, 1, 0]), dict(quantised=True), dict(streams=[5, 0])):
        with pytest.raises(Exception) as e:
            arr.common_mode(**kw)
        assert not isinstance(e.value, ValueError), kw
    with pytest.raises(ValueError):
        arr.common_mode(streams=[4, 0])
