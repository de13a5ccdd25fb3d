"""Host-side checks of the compare sink and encode verification: ABI revision, the new error bit, the encode-verify
default, and the argument checks of compare_flac_device / FlacArray.first_mismatch that need no device."""
import os
import re

import numpy as np
import pytest
import torch

import flacarray_amd as fa
from flacarray_amd import _lib, libflacarray
from tests.conftest import ROOT

HEADER = os.path.join(ROOT, "include", "flacarray_hip.h")
# error bits the reference defines (flacarray.h:20-40): bits 0 to 19
REFERENCE_BITS = set(range(20))


def _header_defines():
    out = {}
    with open(HEADER) as f:
        for m in re.finditer(r"#define (FA_\w+) \(?([^/\n]*?)\)?\s*(?:/\*.*)?$", f.read(), re.M):
            out[m.group(1)] = m.group(2).strip()
    return out


def _bit(expr):
    m = re.fullmatch(r"1 << (\d+)", expr)
    return int(m.group(1)) if m else None


def test_abi_revision_is_4():
    d = _header_defines()
    assert int(d["FA_ABI_VERSION"]) == _lib.ABI_VERSION == 4
    assert _lib.lib().fa_abi_version() == 4


def test_encode_verify_error_bit():
    d = _header_defines()
    bit = _bit(d["FA_ERROR_ENCODE_VERIFY"])
    assert bit == 26 and _lib.ERROR_ENCODE_VERIFY == 1 << bit
    assert bit not in REFERENCE_BITS
    others = {k: _bit(v) for k, v in d.items() if k.startswith("FA_ERROR_") and k not in ("FA_ERROR_NONE", "FA_ERROR_ENCODE_VERIFY")}
    assert None not in others.values() and bit not in others.values()


def test_new_symbols_registered():
    for name in ("fa_compare_i32_device", "fa_compare_i64_device", "fa_set_encode_verify"):
        assert name in _lib.SYMBOLS
        getattr(_lib.lib(), name)


def test_encode_verify_default_round_trip():
    assert fa.set_encode_verify(True) is False  # initially off
    try:
        assert libflacarray._encode_verify_default() is True
        with libflacarray._EncodeVerify(False):
            assert libflacarray._encode_verify_default() is False
        assert libflacarray._encode_verify_default() is True
    finally:
        assert fa.set_encode_verify(False) is True
    assert libflacarray._encode_verify_default() is False


def _store(n_stream=3, n=10):
    comp = torch.zeros(64, dtype=torch.uint8)
    st = torch.zeros(n_stream, dtype=torch.int64)
    nb = torch.zeros(n_stream, dtype=torch.int64)
    return comp, st, nb


@pytest.mark.parametrize(
    "kw, match",
    [
        (dict(data=torch.zeros((3, 10), dtype=torch.int16)), "Unsupported data type"),
        (dict(data=torch.zeros((4, 10), dtype=torch.int32)), "does not match"),
        (dict(data=torch.zeros((3, 2, 10), dtype=torch.int32)), "does not match"),
        (dict(data=torch.zeros((3, 0), dtype=torch.int32)), "non-empty"),
        (dict(data=torch.zeros((10, 3), dtype=torch.int32).t()), "C-contiguous"),
        (dict(data=torch.zeros((3, 10), dtype=torch.float32)), "offsets and gains"),
        (dict(data=torch.zeros((3, 10), dtype=torch.float64), offsets=torch.zeros(3, dtype=torch.float64)), "gains"),
        (dict(data=torch.zeros((3, 10), dtype=torch.int64), offsets=torch.zeros(3), gains=torch.ones(3)), "float data only"),
        (dict(data=torch.zeros((3, 10), dtype=torch.float32), offsets=torch.zeros(2), gains=torch.ones(2)), "one value per stream"),
    ],
)
def test_compare_flac_device_argument_checks(kw, match):
    comp, st, nb = _store()
    with pytest.raises(ValueError, match=match):
        fa.compare_flac_device(comp, st, nb, **kw)


def test_compare_flac_device_index_checks():
    comp, st, nb = _store()
    with pytest.raises(ValueError, match="uint8"):
        fa.compare_flac_device(comp.to(torch.int8), st, nb, torch.zeros((3, 10), dtype=torch.int32))
    with pytest.raises(ValueError, match="int64"):
        fa.compare_flac_device(comp, st.to(torch.int32), nb, torch.zeros((3, 10), dtype=torch.int32))


def test_first_mismatch_argument_checks():
    blob = np.zeros(16, dtype=np.uint8)
    arr = fa.FlacArray._assemble((2, 3, 50), None, np.int32, blob, np.zeros((2, 3), np.int64), np.zeros((2, 3), np.int64), None, None)
    with pytest.raises(ValueError, match="shape"):
        arr.first_mismatch(np.zeros((6, 50), dtype=np.int32))
    with pytest.raises(ValueError, match="dtype"):
        arr.first_mismatch(np.zeros((2, 3, 50), dtype=np.int64))
    with pytest.raises(ValueError, match="dtype"):
        arr.first_mismatch(torch.zeros((2, 3, 50), dtype=torch.float32))
