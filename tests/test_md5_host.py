"""Host-side checks of the STREAMINFO MD5 work: the new entry points exist and the ABI revision did not move, stream_md5
reads the signatures libFLAC-shaped fixtures carry (expected values from hashlib over the fixtures' own samples), the
encode-md5 default round trips, and the argument checks of md5_device / check_md5_device that need no device."""
import hashlib
import os
import re
import struct
import subprocess

import numpy as np
import pytest
import torch

import flacarray_amd as fa
from flacarray_amd import _lib, libflacarray
from tests.conftest import ROOT
from tests.golden import flac_writer as W
from tests.golden import pyflac, rfc9639

HEADER = os.path.join(ROOT, "include", "flacarray_hip.h")
NEW_SYMBOLS = ("fa_md5_i32_device", "fa_md5_i64_device", "fa_sign_streams_device", "fa_check_md5_device", "fa_set_encode_md5")


def test_new_symbols_and_abi_revision():
    for name in NEW_SYMBOLS:
        assert name in _lib.SYMBOLS
        getattr(_lib.lib(), name)
    with open(HEADER) as f:
        text = f.read()
    assert re.search(r"^#define FA_ABI_VERSION 4\b", text, re.M)
    assert _lib.ABI_VERSION == 4 and _lib.lib().fa_abi_version() == 4
    for name in NEW_SYMBOLS:
        assert re.search(r"\b%s\(" % name, text), name


def test_new_symbols_exported_by_the_library():
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = {line.split()[-1] for line in out.splitlines() if line.strip()}
    for name in NEW_SYMBOLS:
        assert name in exported, name


def test_stream_md5_of_generated_streams():
    """Every stream of flac_writer.all_batches() carries the MD5 of its own samples: int32 rows as '<i4', two-channel
    rows as '<i8' (channel 0 = low word)."""
    batches = W.all_batches()
    count = 0
    for b in batches:
        blob, st, _ = W.pack(b["streams"])
        got = fa.stream_md5(blob, st)
        assert got.shape == (len(b["streams"]), 16) and got.dtype == np.uint8
        fmt = "<i4" if b["channels"] == 1 else "<i8"
        for i, x in enumerate(b["samples"]):
            assert got[i].tobytes() == hashlib.md5(np.asarray(x).astype(fmt).tobytes()).digest(), (b["name"], i)
            count += 1
    assert (len(batches), count) == (50, 114)


@pytest.mark.parametrize("name", ["example1", "example2", "example3"])
def test_stream_md5_of_rfc9639_examples(name):
    data, _, bps, _, _ = rfc9639.EXAMPLES[name]
    samples, info = pyflac.decode_stream(data)
    assert info["bps"] == bps
    want = hashlib.md5(struct.pack(f"<{len(samples)}{ {8: 'b', 16: 'h'}[bps] }", *samples)).digest()
    blob = np.frombuffer(data, dtype=np.uint8)
    got = fa.stream_md5(blob, np.array([0], dtype=np.int64))
    assert got.shape == (1, 16) and got[0].tobytes() == want


def test_stream_md5_shapes_unsigned_and_errors(oracle):
    x = (np.arange(6 * 300, dtype=np.int32).reshape(2, 3, 300) * 7919) % 1000
    blob, st, nb = oracle.encode_i32(x.reshape(6, 300), 5)
    got = fa.stream_md5(blob, st.reshape(2, 3))
    assert got.shape == (2, 3, 16) and not got.any()  # the oracle writes "not computed"
    with pytest.raises(ValueError, match="fLaC"):
        fa.stream_md5(np.zeros(100, dtype=np.uint8), np.array([0], dtype=np.int64))
    bad = blob.copy()
    bad[st[1] + 7] = 35  # STREAMINFO length
    with pytest.raises(ValueError, match="Stream 1"):
        fa.stream_md5(bad, st)
    with pytest.raises(ValueError, match="outside"):
        fa.stream_md5(blob[:30], np.array([0], dtype=np.int64))
    with pytest.raises(ValueError, match="uint8"):
        fa.stream_md5(blob.astype(np.int8), st)


def test_encode_md5_default_round_trip():
    assert fa.set_encode_md5(True) is False  # initially off
    try:
        assert libflacarray._encode_md5_default() is True
        with libflacarray._EncodeMd5(False):
            assert libflacarray._encode_md5_default() is False
        assert libflacarray._encode_md5_default() is True
        with libflacarray._EncodeMd5(None):
            assert libflacarray._encode_md5_default() is True
    finally:
        assert fa.set_encode_md5(False) is True
    assert libflacarray._encode_md5_default() is False
    assert _lib.lib().fa_set_encode_md5(-1) == 0  # a negative argument only reads


I32 = torch.zeros((3, 32), dtype=torch.int32)
F32 = torch.zeros((3, 32), dtype=torch.float32)
ONE = torch.ones(3)


@pytest.mark.parametrize(
    "args, kw, match",
    [
        ((I32.to(torch.int16),), {}, "Unsupported data type"),
        ((torch.zeros((), dtype=torch.int32),), {}, "stream axis"),
        ((torch.zeros((3, 64), dtype=torch.int32)[:, ::2],), {}, "C-contiguous"),
        ((torch.zeros((32, 3), dtype=torch.int32).t(),), {}, "C-contiguous"),
        ((torch.zeros((2, 3, 64), dtype=torch.int32)[:, :, :32],), {}, "C-contiguous"),
        ((F32,), {"offsets": ONE}, "also provide the gains"),
        ((F32,), {}, "needs the offsets and gains"),
        ((I32,), {"offsets": ONE, "gains": ONE}, "float data only"),
        ((F32,), {"offsets": torch.ones(2), "gains": torch.ones(2)}, "one value per stream"),
        ((torch.zeros((3, 17), dtype=torch.int32),), {"final": False}, "whole number of 64-byte blocks"),
        ((torch.zeros((3, 12), dtype=torch.int64),), {"final": False}, "whole number of 64-byte blocks"),
        ((I32,), {"n_before": 8, "state": torch.zeros((3, 4), dtype=torch.int32)}, "whole number of 64-byte blocks"),
        ((I32,), {"n_before": 16}, "go together"),
        ((I32,), {"n_before": 16, "state": torch.zeros((3, 4), dtype=torch.int64)}, "int32 tensor of shape"),
    ],
)
def test_md5_device_argument_checks(args, kw, match):
    with pytest.raises(ValueError, match=match):
        fa.md5_device(*args, **kw)


def test_md5_device_needs_the_gpu():
    with pytest.raises(RuntimeError, match="on the GPU"):
        fa.md5_device(I32)
    with pytest.raises(RuntimeError, match="on the GPU"):
        fa.md5_device(torch.zeros((3, 64), dtype=torch.int32)[:, 16:48])  # (a column range passes the layout check)


def _store():
    return torch.zeros(64, dtype=torch.uint8), torch.zeros(3, dtype=torch.int64), torch.full((3,), 20, dtype=torch.int64)


def test_check_md5_device_argument_checks():
    comp, st, nb = _store()
    with pytest.raises(ValueError, match="uint8"):
        fa.check_md5_device(comp.to(torch.int8), st, nb, 10)
    with pytest.raises(ValueError, match="int64"):
        fa.check_md5_device(comp, st.to(torch.int32), nb, 10)
    with pytest.raises(ValueError, match="same shape"):
        fa.check_md5_device(comp, st, nb[:2], 10)
    with pytest.raises(ValueError, match="C-contiguous"):
        fa.check_md5_device(comp, torch.zeros((3, 2), dtype=torch.int64)[:, 0], nb, 10)
    with pytest.raises(ValueError, match="stream size"):
        fa.check_md5_device(comp, st, nb, 0)
    with pytest.raises(RuntimeError, match="same GPU"):
        fa.check_md5_device(comp, st, nb, 10)


def test_sign_streams_device_argument_checks():
    comp, st, _ = _store()
    with pytest.raises(ValueError, match="uint8"):
        fa.sign_streams_device(comp, st, torch.zeros((3, 16), dtype=torch.int8))
    with pytest.raises(ValueError, match="sixteen bytes per stream"):
        fa.sign_streams_device(comp, st, torch.zeros((2, 16), dtype=torch.uint8))
    with pytest.raises(RuntimeError, match="same GPU"):
        fa.sign_streams_device(comp, st, torch.zeros((3, 16), dtype=torch.uint8))


def test_md5_property_reads_the_host_mirror():
    b = W.all_batches()[0]
    blob, st, nb = W.pack(b["streams"])
    k = len(b["streams"])
    dt = np.int32 if b["channels"] == 1 else np.int64
    arr = fa.FlacArray._assemble((k, b["n"]), None, dt, blob, st, nb, None, None)
    assert np.array_equal(arr.md5, fa.stream_md5(blob, st)) and arr.md5.shape == (k, 16)
