"""CPU tests of FlacArray.append's splice model (tests/append_model.py) against the oracle's one-shot encode, of the
CRC-16 combine identity the splice kernel relies on, and of the host-side argument checks of FlacArray.append (they
raise before any device call)."""
import numpy as np
import pytest

import flacarray_amd as fa
from tests import append_model as M
from tests.conftest import sinusoid_noise_i32, strip_seektable


def _block(level):
    return 1152 if level <= 2 else 4096


def _check_split(oracle, x, n_old, level, encode):
    r = n_old % _block(level)
    got = M.splice(encode(x[:, :n_old], level), encode(x[:, n_old - r :], level))
    want = encode(x, level)
    for g, w in zip(got, want):
        assert np.array_equal(g, w)


@pytest.mark.parametrize("level", [1, 5])
@pytest.mark.parametrize("where", ["boundary", "inside", "short"])
def test_splice_i32_equals_one_shot_encode(oracle, level, where):
    B = _block(level)
    x = sinusoid_noise_i32(3, 5 * B + 333, seed=level)
    n_old = {"boundary": 2 * B, "inside": 2 * B + 517, "short": 37}[where]
    _check_split(oracle, x, n_old, level, oracle.encode_i32)


@pytest.mark.parametrize("level", [1, 5])
@pytest.mark.parametrize("n_old_frac", [1.0, 1.5])
def test_splice_i64_equals_one_shot_encode(oracle, level, n_old_frac):
    B = _block(level)
    rng = np.random.default_rng(7)
    x = (sinusoid_noise_i32(2, 4 * B + 11).astype(np.int64) << 20) + rng.integers(0, 1 << 20, (2, 4 * B + 11))
    _check_split(oracle, x, int(n_old_frac * B), level, oracle.encode_i64)


def test_splice_chain_of_chunks(oracle):
    """Several appends in a row, chunks of one sample and chunks that end inside a frame."""
    level, B = 1, 1152
    x = sinusoid_noise_i32(2, 3 * B + 5, seed=3)
    cuts = [1, 2, 700, B + 3, 2 * B, 2 * B + 1, 3 * B + 5]
    store = oracle.encode_i32(x[:, : cuts[0]], level)
    for a, b in zip(cuts, cuts[1:]):
        r = a % B
        store = M.splice(store, oracle.encode_i32(x[:, a - r : b], level))
    for g, w in zip(store, oracle.encode_i32(x, level)):
        assert np.array_equal(g, w)


@pytest.mark.parametrize("n_old", [127 * 1152 + 100, 2047 * 1152 + 1, 2048 * 1152])
def test_splice_across_utf8_length_change(oracle, n_old):
    """Frame numbers crossing 128 and 2048, where the UTF-8 field grows by a byte (level 1: ~2.4 M samples)."""
    level, B = 1, 1152
    total = 2050 * 1152 + 17
    rng = np.random.default_rng(11)
    x = np.cumsum(rng.integers(-40, 41, (1, total)), axis=1).astype(np.int32)
    if n_old < 1000 * B:  # (the 128 crossing needs no 2.4 M samples)
        x = x[:, : 130 * B + 9]
    _check_split(oracle, x, n_old, level, oracle.encode_i32)


def test_crc16_combine_identity():
    rng = np.random.default_rng(5)
    for _ in range(40):
        h = rng.integers(0, 256, int(rng.integers(1, 24)), dtype=np.uint8).tobytes()
        p = rng.integers(0, 256, int(rng.integers(0, 5000)), dtype=np.uint8).tobytes()
        assert M.crc16(h + p) == M.crc16_combine(M.crc16(h), M.crc16(p), len(p))
    for nbytes in (0, 1, 2, 3, 100, 4095, 16640):
        # crc16 of the polynomial 1 followed by n zero bytes is x^(8n) * x^16 mod G
        assert M.crc16_mulmod(M.crc16_xpow8(nbytes), M.crc16_xpow8(2)) == M.crc16(b"\x01" + bytes(nbytes))


def test_utf8_growth_closed_form():
    for m in (0, 1, 127, 128, 129, 2047, 2048, 2049, 70000):
        assert M.utf8_len_sum(m) == sum(M.utf8_len(v) for v in range(m))
    for v in (0, 127, 128, 2047, 2048, 65535, 65536, 2**21 - 1, 2**21, 2**26, 2**31 - 1, 2**31):
        assert len(M.utf8_number(v)) == M.utf8_len(v)


# ---- host-side argument checks: none of these reaches the device ----
def _host_array(oracle, x, level=5):
    blob, st, nb = oracle.encode_i32(x, level)
    shape = x.shape if x.shape[0] > 1 else (x.shape[1],)
    return fa.FlacArray._assemble(shape, None, np.int32, blob, st.reshape(x.shape[:-1]), nb.reshape(x.shape[:-1]), None, None)


def test_append_rejects_wrong_dtype_and_shape(oracle):
    arr = _host_array(oracle, sinusoid_noise_i32(3, 5000))
    with pytest.raises(ValueError, match="dtype"):
        arr.append(np.zeros((3, 10), dtype=np.int64))
    with pytest.raises(ValueError, match="shape"):
        arr.append(np.zeros((2, 10), dtype=np.int32))
    with pytest.raises(ValueError, match="shape"):
        arr.append(np.zeros(10, dtype=np.int32))
    with pytest.raises(ValueError):
        arr.append(np.zeros((3, 10), dtype=np.int32), level=9)


def test_append_rejects_level_of_other_block_size(oracle):
    arr = _host_array(oracle, sinusoid_noise_i32(2, 5000), level=5)
    with pytest.raises(ValueError, match="block size"):
        arr.append(np.zeros((2, 10), dtype=np.int32), level=1)


def test_append_rejects_streams_without_seektable(oracle):
    x = sinusoid_noise_i32(2, 5000)
    blob, st, nb = strip_seektable(*oracle.encode_i32(x, 5))
    arr = fa.FlacArray._assemble(x.shape, None, np.int32, blob, st, nb, None, None)
    with pytest.raises(ValueError, match="SEEKTABLE"):
        arr.append(np.zeros((2, 10), dtype=np.int32))


def test_append_rejects_distributed_store(oracle):
    x = sinusoid_noise_i32(2, 5000)
    blob, st, nb = oracle.encode_i32(x, 5)
    arr = fa.FlacArray._assemble(x.shape, (4, 5000), np.int32, blob, st, nb, None, None)
    with pytest.raises(NotImplementedError):
        arr.append(np.zeros((2, 10), dtype=np.int32))


def test_append_of_nothing_is_a_no_op(oracle):
    arr = _host_array(oracle, sinusoid_noise_i32(2, 5000))
    blob = arr.compressed.copy()
    assert arr.append(np.zeros((2, 0), dtype=np.int32)) is arr
    assert np.array_equal(arr.compressed, blob) and arr.shape == (2, 5000)


def test_append_flac_device_is_exported():
    assert "append_flac_device" in fa.__all__ and callable(fa.append_flac_device)
    assert callable(fa.FlacArray.append)
