"""CPU tests of FlacArray.overwrite's splice model (tests/overwrite_model.py) against the oracle's one-shot encode of the
patched array, of the seek-point rewrite alone, and of the host-side argument checks of FlacArray.overwrite (they raise
before any device call)."""
import numpy as np
import pytest

import flacarray_amd as fa
from tests import append_model as A
from tests import overwrite_model as M
from tests.conftest import sinusoid_noise_i32, strip_seektable


def _block(level):
    return 1152 if level <= 2 else 4096


def _same(got, want):
    for g, w in zip(got, want):
        assert np.array_equal(np.ravel(g), np.ravel(w))


def _check(x, first, data, streams, level, encode):
    got = M.overwrite(encode(x, level), x, first, data, streams, level, encode)
    _same(got, encode(M.patched(x, first, data, streams), level))
    return got


CASES = sorted(M.geometry_cases(4096, 5 * 4096 + 37))


@pytest.mark.parametrize("level", [1, 5])
@pytest.mark.parametrize("case", CASES)
def test_splice_i32_equals_one_shot_encode(oracle, level, case):
    B = _block(level)
    N = 5 * B + 37
    first, n = M.geometry_cases(B, N)[case]
    x = sinusoid_noise_i32(3, N, seed=level)
    data = sinusoid_noise_i32(3, n, seed=level + 40) // 3
    _check(x, first, data, None, level, oracle.encode_i32)


@pytest.mark.parametrize("level", [1, 5])
@pytest.mark.parametrize("case", ["inside_last_frame", "ends_at_stream_end", "whole_stream", "across_one_boundary"])
def test_splice_without_a_short_last_frame(oracle, level, case):
    B = _block(level)
    N = 4 * B
    first, n = M.geometry_cases(B, N)[case]
    x = sinusoid_noise_i32(2, N, seed=level + 2)
    _check(x, first, sinusoid_noise_i32(2, n, seed=9), None, level, oracle.encode_i32)


@pytest.mark.parametrize("level", [1, 5])
def test_splice_i64_equals_one_shot_encode(oracle, level):
    B = _block(level)
    N = 4 * B + 11
    rng = np.random.default_rng(7)
    x = (sinusoid_noise_i32(2, N).astype(np.int64) << 20) + rng.integers(0, 1 << 20, (2, N))
    data = rng.integers(-300, 300, (2, B + 500)).astype(np.int64)  # (small values of both signs)
    _check(x, B + 70, data, None, level, oracle.encode_i64)


@pytest.mark.parametrize("level", [1, 5])
def test_suffix_moves_both_ways(oracle, level):
    """Noise -> zeros shrinks the middle frames (CONSTANT), quiet -> full-range noise grows them (VERBATIM)."""
    B = _block(level)
    N = 5 * B + 37
    rng = np.random.default_rng(3)
    x = sinusoid_noise_i32(2, N, seed=5)
    old = oracle.encode_i32(x, level)
    got = _check(x, B + 10, np.zeros((2, 2 * B), dtype=np.int32), None, level, oracle.encode_i32)
    assert np.all(got[2] < old[2])
    noise = rng.integers(-(2**31), 2**31, (2, 2 * B), dtype=np.int64).astype(np.int32)
    got = _check(x, B + 10, noise, None, level, oracle.encode_i32)
    assert np.all(got[2] > old[2])


def test_splice_across_utf8_length_change(oracle):
    """Level 1, the new frames' numbers cross 128: the encode's frames 0..3 become 126..129."""
    B = 1152
    N = 131 * B + 37
    rng = np.random.default_rng(11)
    x = np.cumsum(rng.integers(-40, 41, (2, N)), axis=1).astype(np.int32)
    first, end = 126 * B + 5, 129 * B + 105
    assert M.span_frames(N, B, first, end - first) == (126, 130)
    _check(x, first, sinusoid_noise_i32(2, end - first, seed=2), None, 1, oracle.encode_i32)


def test_stream_subset_and_untouched_signature(oracle):
    """6 streams, streams=[4, 1]: rows in that order; the other four come back as they are, a signature included."""
    level, B = 5, 4096
    N = 3 * B + 100
    x = sinusoid_noise_i32(6, N, seed=8)
    blob, st, nb = oracle.encode_i32(x, level)
    blob = blob.copy()
    for s in range(6):  # (any non-zero MD5 field stands for a signature here)
        blob[st[s] + 26 : st[s] + 42] = np.arange(16, dtype=np.uint8) + 1 + s
    data = sinusoid_noise_i32(2, B + 9, seed=12) // 7
    got = M.overwrite((blob, st, nb), x, B - 4, data, [4, 1], level, oracle.encode_i32)
    want = oracle.encode_i32(M.patched(x, B - 4, data, [4, 1]), level)
    _same(got[1:], want[1:])
    for s in range(6):
        g = got[0][got[1][s] : got[1][s] + got[2][s]]
        w = want[0][want[1][s] : want[1][s] + want[2][s]].copy()
        if s in (4, 1):
            assert not g[26:42].any()
        else:
            assert np.array_equal(g, blob[st[s] : st[s] + nb[s]])
            w[26:42] = np.arange(16, dtype=np.uint8) + 1 + s
        assert np.array_equal(g, w)


def test_seek_point_rewrite():
    pts = b"".join(sn.to_bytes(8, "big") + off.to_bytes(8, "big") + ns.to_bytes(2, "big") for sn, off, ns in [(8192, 1000, 4096), (12288, 70000, 37)])
    for delta in (-999, 0, 5, 1 << 33):
        out = M.move_seek_points(pts, delta)
        assert len(out) == 36
        for k, (sn, off, ns) in enumerate([(8192, 1000, 4096), (12288, 70000, 37)]):
            pt = out[18 * k : 18 * k + 18]
            assert (int.from_bytes(pt[:8], "big"), int.from_bytes(pt[8:16], "big"), int.from_bytes(pt[16:], "big")) == (sn, off + delta, ns)
    assert M.move_seek_points(b"", 7) == b""


def test_growth_closed_form():
    for base, k in [(0, 5), (126, 4), (127, 1), (128, 3), (2040, 20), (5, 0)]:
        assert M.growth(base, k) == sum(A.utf8_len(base + i) - A.utf8_len(i) for i in range(k))


def test_model_refuses_bad_arguments(oracle):
    x = sinusoid_noise_i32(2, 5000)
    old = oracle.encode_i32(x, 5)
    new = oracle.encode_i32(x[:, :4096], 5)
    with pytest.raises(ValueError):
        M.splice(old, new, 10, 20, streams=[0, 0])
    with pytest.raises(ValueError):
        M.splice(old, new, 10, 20, streams=[0, 2])
    with pytest.raises(ValueError):
        M.splice(old, new, 4990, 20)
    with pytest.raises(ValueError):
        M.splice(strip_seektable(*old), new, 10, 20)


# ---- host-side argument checks: none of these reaches the device ----
def _host_array(oracle, x, level=5):
    blob, st, nb = oracle.encode_i32(x, level)
    shape = x.shape if x.shape[0] > 1 else (x.shape[1],)
    return fa.FlacArray._assemble(shape, None, np.int32, blob, st.reshape(x.shape[:-1]), nb.reshape(x.shape[:-1]), None, None)


def test_overwrite_rejects_range_dtype_shape_level_and_streams(oracle):
    arr = _host_array(oracle, sinusoid_noise_i32(3, 5000))
    blob = arr.compressed.copy()
    z = np.zeros((3, 10), dtype=np.int32)
    for first, data in [(-1, z), (4991, z), (5000, z[:, :1]), (0, np.zeros((3, 5001), dtype=np.int32))]:
        with pytest.raises(ValueError, match="samples"):
            arr.overwrite(first, data)
    with pytest.raises(ValueError, match="dtype"):
        arr.overwrite(0, z.astype(np.int64))
    with pytest.raises(ValueError, match="shape"):
        arr.overwrite(0, z[:2])
    with pytest.raises(ValueError, match="shape"):
        arr.overwrite(0, z[0])
    with pytest.raises(ValueError, match="shape"):
        arr.overwrite(0, z, streams=[0, 1])
    with pytest.raises(ValueError):
        arr.overwrite(0, z, level=9)
    with pytest.raises(ValueError, match="block size"):
        arr.overwrite(0, z, level=1)
    with pytest.raises(ValueError, match="twice"):
        arr.overwrite(0, z[:2], streams=[1, 1])
    with pytest.raises(ValueError, match="outside"):
        arr.overwrite(0, z[:2], streams=[1, 3])
    with pytest.raises(ValueError, match="outside"):
        arr.overwrite(0, z[:1], streams=[-1])
    with pytest.raises(ValueError, match="1-D"):
        arr.overwrite(0, z[:2], streams=[[0, 1]])
    assert np.array_equal(arr.compressed, blob)


def test_overwrite_rejects_streams_without_seektable_and_distributed_stores(oracle):
    x = sinusoid_noise_i32(2, 5000)
    blob, st, nb = strip_seektable(*oracle.encode_i32(x, 5))
    arr = fa.FlacArray._assemble(x.shape, None, np.int32, blob, st, nb, None, None)
    with pytest.raises(ValueError, match="SEEKTABLE"):
        arr.overwrite(0, np.zeros((2, 10), dtype=np.int32))
    blob, st, nb = oracle.encode_i32(x, 5)
    arr = fa.FlacArray._assemble(x.shape, (4, 5000), np.int32, blob, st, nb, None, None)
    with pytest.raises(NotImplementedError):
        arr.overwrite(0, np.zeros((2, 10), dtype=np.int32))


def test_overwrite_of_nothing_is_a_no_op_and_setitem_still_raises(oracle):
    arr = _host_array(oracle, sinusoid_noise_i32(2, 5000))
    blob = arr.compressed.copy()
    assert arr.overwrite(100, np.zeros((2, 0), dtype=np.int32)) is arr
    assert arr.overwrite(100, np.zeros((0, 7), dtype=np.int32), streams=np.zeros(0, dtype=np.int64)) is arr
    assert np.array_equal(arr.compressed, blob) and arr.shape == (2, 5000)
    with pytest.raises(RuntimeError):
        arr[0, 5] = 1


def test_overwrite_flac_device_is_exported():
    assert "overwrite_flac_device" in fa.__all__ and callable(fa.overwrite_flac_device)
    assert callable(fa.FlacArray.overwrite)
