"""GPU tests of FlacArray.overwrite / overwrite_flac_device: after replacing samples [first, first + n) of some or all
streams the store is byte for byte the one-shot encode of the patched array (the library's, the oracle's) and the output
of the plain-Python splice model (tests/overwrite_model.py), for every geometry of the range against the frame grid, a
suffix that moves either way, frame numbers whose UTF-8 field grows, a stream subset, int64 and float stores, and
compositions with append."""
import numpy as np
import pytest
import torch

import flacarray_amd as fa
from tests import overwrite_model as M
from tests import quant_model as Q
from tests.conftest import sinusoid_noise_f32, sinusoid_noise_i32
from tests.golden import flac_writer as W

pytestmark = pytest.mark.gpu


@pytest.fixture(params=["auto", "k7"])
def decoder_dispatch(request, monkeypatch):
    """As in test_gpu_append.py: the library's own dispatch, and K7 + K3F for every array of their geometry -- so the
    span decode and the span encode take both kernel families."""
    if request.param == "k7":
        monkeypatch.setenv("FLACARRAY_HIP_LATENCY", "0")
        monkeypatch.setenv("FLACARRAY_HIP_PLACED_BELOW", "0")
    else:
        monkeypatch.delenv("FLACARRAY_HIP_LATENCY", raising=False)
        monkeypatch.delenv("FLACARRAY_HIP_PLACED_BELOW", raising=False)
    return request.param


def quantise_given(x, offsets, gains):
    """utils.c:229-240 (float32) / :316-323 (float64) with given per-stream offsets and gains."""
    x = np.asarray(x)
    with np.errstate(all="ignore"):
        if x.dtype == np.float32:
            st = (x - np.asarray(offsets, np.float32).reshape(-1, 1)).astype(np.float32)
            pr = (np.asarray(gains, np.float32).reshape(-1, 1) * st).astype(np.float32).astype(np.float64)
            return Q.cvtt(np.where(st >= 0, pr + 0.5, pr - 0.5), 32)
        t = x - np.asarray(offsets, np.float64).reshape(-1, 1)
        g = np.asarray(gains, np.float64).reshape(-1, 1)
        return Q.cvtt(np.where(t >= 0, g * t + 0.5, g * t - 0.5), 64)


def _data(kind, n_stream, n, seed=1):
    x = sinusoid_noise_i32(n_stream, n, seed=seed)
    if kind == "int64":
        rng = np.random.default_rng(seed)
        return (x.astype(np.int64) << 18) + rng.integers(0, 1 << 18, x.shape)
    return x


def _block(level):
    return 1152 if level <= 2 else 4096


def _same_store(arr, want):
    blob, st, nb = want
    assert np.array_equal(np.asarray(arr.compressed), blob)
    assert np.array_equal(np.asarray(arr.stream_starts).reshape(-1), np.asarray(st).reshape(-1))
    assert np.array_equal(np.asarray(arr.stream_nbytes).reshape(-1), np.asarray(nb).reshape(-1))


def _triple(arr):
    return np.array(arr.compressed), np.array(arr.stream_starts).reshape(-1), np.array(arr.stream_nbytes).reshape(-1)


def _overwrite_and_check(oracle, x, first, data, streams, level, resident=False, **kw):
    """from_array(x).overwrite(first, data, streams): the store equals from_array(y), the oracle's encode of y and the
    model's output, and decodes to y.  Returns (array, y, the old store's triple)."""
    wide = x.dtype == np.int64
    enc = oracle.encode_i64 if wide else oracle.encode_i32
    arr = fa.FlacArray.from_array(x, level=level)
    if resident:
        arr.to_device()
    old = _triple(arr)
    assert arr.overwrite(first, data, streams=streams, level=level, **kw) is arr
    y = M.patched(x, first, data, streams)
    one = fa.FlacArray.from_array(y, level=level)
    _same_store(arr, (one.compressed, one.stream_starts, one.stream_nbytes))
    _same_store(arr, enc(y, level))
    _same_store(arr, M.overwrite(old, x, first, data, streams, level, enc))
    assert arr.shape == x.shape and np.array_equal(arr.to_array(), y)
    return arr, y, old


GEOMETRY = sorted(M.geometry_cases(4096, 5 * 4096 + 37))


@pytest.mark.parametrize("level", [1, 5])
@pytest.mark.parametrize("case", GEOMETRY)
def test_overwrite_geometry(oracle, decoder_dispatch, level, case):
    B = _block(level)
    N = 5 * B + 37
    first, n = M.geometry_cases(B, N)[case]
    x = _data("int32", 3, N, seed=level + 1)
    data = sinusoid_noise_i32(3, n, seed=level + 50) // 3
    _overwrite_and_check(oracle, x, first, data, None, level)


@pytest.mark.parametrize("level", [1, 5])
@pytest.mark.parametrize("case", ["inside_last_frame", "ends_at_stream_end", "whole_stream", "ends_on_boundary"])
def test_overwrite_geometry_without_a_short_last_frame(oracle, decoder_dispatch, level, case):
    B = _block(level)
    N = 4 * B
    first, n = M.geometry_cases(B, N)[case]
    x = _data("int32", 2, N, seed=level + 3)
    _overwrite_and_check(oracle, x, first, sinusoid_noise_i32(2, n, seed=77), None, level)


@pytest.mark.parametrize("level", [1, 5])
@pytest.mark.parametrize("way", ["shrinks", "grows"])
def test_overwrite_moves_the_suffix_both_ways(oracle, decoder_dispatch, level, way):
    """Noise -> zeros: the frames become CONSTANT, delta < 0.  Quiet -> full-range noise: VERBATIM, delta > 0.  The
    overwritten length differs per stream, so every stream has its own delta and suffix misalignment; a slice inside
    the suffix read through the rebuilt decode index proves the rewritten seek offsets."""
    B = _block(level)
    N = 6 * B + 37
    rng = np.random.default_rng(level)
    if way == "shrinks":
        x = _data("int32", 3, N, seed=level + 5)
        data = np.zeros((3, 3 * B), dtype=np.int32)
        for s in range(3):  # (stream s keeps its noise behind B + s B + 11 s zeros)
            data[s, B + s * B + 11 * s :] = x[s, B + 3 + B + s * B + 11 * s : B + 3 + 3 * B]
    else:
        x = (sinusoid_noise_i32(3, N, seed=level + 6) >> 12).astype(np.int32)
        data = rng.integers(-(2**31), 2**31, (3, 3 * B), dtype=np.int64).astype(np.int32)
        for s in range(3):
            data[s, B + s * B + 11 * s :] = x[s, B + 3 + B + s * B + 11 * s : B + 3 + 3 * B]
    arr, y, old = _overwrite_and_check(oracle, x, B + 3, data, None, level, resident=True)
    delta = np.asarray(arr.stream_nbytes).reshape(-1) - old[2]
    assert np.all(delta < 0) if way == "shrinks" else np.all(delta > 0)
    assert len(set(delta.tolist())) == 3
    assert arr.is_resident  # (the old decode index was closed; to_array above has built the new store's)
    lo, hi = 5 * B + 100, 6 * B + 30  # (frame 5 and the short last one: behind the span, frames 1-4)
    assert np.array_equal(arr[:, lo:hi], y[:, lo:hi])
    got = arr.read_slices([2, 0], [5 * B + 1, 5 * B + 7], [B, 50])
    assert np.array_equal(got[0], y[2, 5 * B + 1 : 6 * B + 1]) and np.array_equal(got[1], y[0, 5 * B + 7 : 5 * B + 57])
    ix = fa.DeviceDecodeIndex(arr._resident["compressed"], arr._resident["starts"], arr._resident["nbytes"], N)
    assert np.array_equal(ix.decode(lo, hi).cpu().numpy(), y[:, lo:hi])
    ix.close()


def test_overwrite_across_frame_128_utf8_growth(oracle, decoder_dispatch):
    """Level 1, two streams of 131 x 1152 + 37 samples: the encode's frames 0..3 become 126..129, whose UTF-8 number
    grows from one to two bytes at 128."""
    B = 1152
    N = 131 * B + 37
    first, end = 126 * B + 5, 129 * B + 105
    assert M.span_frames(N, B, first, end - first) == (126, 130)
    x = _data("int32", 2, N, seed=9)
    _overwrite_and_check(oracle, x, first, sinusoid_noise_i32(2, end - first, seed=10), None, 1)


def test_overwrite_stream_subset_and_signatures(oracle, decoder_dispatch):
    """6 streams (a 2 x 3 array), streams=[4, 1]: the rows of `data` in that order, the other four streams verbatim --
    their signatures too."""
    level, B = 5, 4096
    N = 3 * B + 100
    x = _data("int32", 6, N, seed=12).reshape(2, 3, N)
    data = sinusoid_noise_i32(2, B + 9, seed=13) // 5
    first = B - 4
    arr = fa.FlacArray.from_array(x, level=level, md5=True)
    assert np.all(arr.check_md5() == 1)
    old = _triple(arr)
    arr.overwrite(first, data, streams=[4, 1], level=level)
    y = M.patched(x.reshape(6, N), first, data, [4, 1])
    assert np.array_equal(y[4, first : first + B + 9], data[0]) and np.array_equal(y[1, first : first + B + 9], data[1])
    assert np.array_equal(arr.check_md5().reshape(-1), [1, -1, 1, 1, -1, 1])
    _same_store(arr, M.overwrite(old, x.reshape(6, N), first, data, [4, 1], level, oracle.encode_i32))
    assert arr.shape == x.shape and np.array_equal(arr.to_array().reshape(6, N), y)
    # the unsigned encode of y: the same sizes, and the same bytes outside the four kept signatures
    blob, st, nb = oracle.encode_i32(y, level)
    one = fa.FlacArray.from_array(y, level=level, md5=False)
    assert np.array_equal(one.compressed, blob)
    signed = blob.copy()
    for s in (0, 2, 3, 5):
        signed[st[s] + 26 : st[s] + 42] = old[0][old[1][s] + 26 : old[1][s] + 42]
        assert signed[st[s] + 26 : st[s] + 42].any()
    _same_store(arr, (signed, st, nb))
    # md5=True: overwrite followed by sign()
    data2 = sinusoid_noise_i32(1, 50, seed=14)
    arr.overwrite(2 * B + 1, data2, streams=np.array([5]), level=level, md5=True)
    assert np.all(arr.check_md5() == 1)
    y[5, 2 * B + 1 : 2 * B + 51] = data2[0]
    assert np.array_equal(arr.to_array().reshape(6, N), y)
    full = fa.FlacArray.from_array(y.reshape(2, 3, N), level=level, md5=True)
    _same_store(arr, (full.compressed, full.stream_starts, full.stream_nbytes))


@pytest.mark.parametrize("level", [1, 5])
def test_overwrite_int64(oracle, decoder_dispatch, level):
    """Two-channel streams; the new samples hold a stretch of small values of both signs, so a patched frame takes the
    side / right decision anew."""
    B = _block(level)
    N = 4 * B + 11
    x = _data("int64", 2, N, seed=level + 15)
    rng = np.random.default_rng(level)
    data = _data("int64", 2, B + 700, seed=level + 16)
    data[:, 200 : B + 300] = rng.integers(-300, 300, (2, B + 100))
    _overwrite_and_check(oracle, x, B - 150, data, None, level)
    _overwrite_and_check(oracle, x, 0, _data("int64", 1, N, seed=3), [1], level)


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("resident", [False, True])
def test_overwrite_float_quantises_with_store_parameters(oracle, dtype, resident):
    level, N, first, n = 5, 3 * 4096 + 200, 4000, 4300
    x = sinusoid_noise_f32(3, N, seed=4).astype(dtype)
    data = sinusoid_noise_f32(2, n, seed=5).astype(dtype)
    # out-of-range values: far outside the store's range (INT_MIN), and the infinities
    data[0, 3] = 1e30
    data[1, 7] = -1e30
    data[1, 11] = np.inf
    data[1, 12] = -np.inf
    arr = fa.FlacArray.from_array(x, level=level, quanta=1e-3)
    if resident:
        arr.to_device()
    off, gain = np.array(arr.stream_offsets), np.array(arr.stream_gains)
    wide = dtype == np.float64
    dec = oracle.decode_i64 if wide else oracle.decode_i32
    ints = dec(arr.compressed, arr.stream_starts, arr.stream_nbytes, N)
    old = _triple(arr)
    arr.overwrite(first, data, streams=[2, 0], level=level)
    new = quantise_given(data, off[[2, 0]], gain[[2, 0]])
    assert new.min() == np.iinfo(new.dtype).min
    y = M.patched(ints, first, new, [2, 0])
    enc = oracle.encode_i64 if wide else oracle.encode_i32
    _same_store(arr, enc(y, level))
    _same_store(arr, M.overwrite(old, ints, first, new, [2, 0], level, enc))
    assert np.array_equal(arr.stream_offsets, off) and np.array_equal(arr.stream_gains, gain)
    restore = Q.int64_to_float64 if wide else Q.int32_to_float32
    assert Q.bits_equal(arr.to_array(), restore(y, off, gain))
    assert arr.is_resident == resident


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_overwrite_nan_raises_and_leaves_the_store(dtype):
    x = sinusoid_noise_f32(2, 6000, seed=5).astype(dtype)
    arr = fa.FlacArray.from_array(x, level=5, quanta=1e-3)
    before = (arr.compressed.copy(), np.array(arr.stream_starts), arr.shape)
    y = np.ascontiguousarray(x[:, 4000:5000])
    y[1, 17] = np.nan
    with pytest.raises(RuntimeError, match="NaN"):
        arr.overwrite(100, y)
    assert np.array_equal(arr.compressed, before[0]) and np.array_equal(arr.stream_starts, before[1]) and arr.shape == before[2]


@pytest.mark.parametrize("kind", ["int32", "int64"])
def test_overwrite_composes_with_append(oracle, decoder_dispatch, kind):
    """Append, overwrite across the old / new seam, append again: the one-shot encode of the final samples."""
    level, B = 5, 4096
    n0, n1, n2 = B + 900, 2 * B + 5, B + 70
    x = _data(kind, 3, n0 + n1 + n2, seed=21)
    arr = fa.FlacArray.from_array(np.ascontiguousarray(x[:, :n0]), level=level)
    arr.append(np.ascontiguousarray(x[:, n0 : n0 + n1]), level=level)
    data = _data(kind, 3, 1500, seed=22)
    arr.overwrite(n0 - 700, data, level=level)
    arr.append(np.ascontiguousarray(x[:, n0 + n1 :]), level=level)
    y = M.patched(x, n0 - 700, data)
    _same_store(arr, (oracle.encode_i64 if kind == "int64" else oracle.encode_i32)(y, level))
    one = fa.FlacArray.from_array(y, level=level)
    _same_store(arr, (one.compressed, one.stream_starts, one.stream_nbytes))
    assert np.array_equal(arr.to_array(), y)
    # and an overwrite of a 1-D array with a device tensor, twice in a row
    z = _data(kind, 1, 3 * B + 9, seed=23).reshape(-1)
    one = fa.FlacArray.from_array(z, level=level)
    d1, d2 = _data(kind, 1, 600, seed=24).reshape(-1), _data(kind, 1, B, seed=25).reshape(-1)
    one.overwrite(B - 300, torch.from_numpy(d1).cuda(), level=level).overwrite(2 * B, d2, level=level)
    z[B - 300 : B + 300] = d1
    z[2 * B : 3 * B] = d2
    assert one.shape == z.shape
    _same_store(one, (oracle.encode_i64 if kind == "int64" else oracle.encode_i32)(z.reshape(1, -1), level))


@pytest.mark.parametrize("kind", ["int32", "int64"])
def test_overwrite_resident_and_host_agree(oracle, kind):
    x = _data(kind, 4, 14000, seed=6)
    data = _data(kind, 4, 5000, seed=7)
    host = fa.FlacArray.from_array(x, level=5)
    res = fa.FlacArray.from_device_array(torch.from_numpy(x).cuda(), level=5)
    res.to_array()  # (builds the decode index, which the overwrite must close and rebuild)
    copy = fa.FlacArray(host)
    host.overwrite(3000, data, verify=True)
    res.overwrite(3000, torch.from_numpy(data).cuda(), verify=True)
    assert res.is_resident and not host.is_resident
    assert host == res and np.array_equal(host.compressed, res.compressed)
    comp = res._resident["compressed"]
    assert comp.untyped_storage().nbytes() == comp.numel() == res.compressed.size
    y = M.patched(x, 3000, data)
    _same_store(host, (oracle.encode_i64 if kind == "int64" else oracle.encode_i32)(y, 5))
    for arr in (host, res):
        assert np.array_equal(arr[1:3, 2000:10000], y[1:3, 2000:10000])
        assert np.all(arr.first_mismatch(y) == -1)
    assert np.array_equal(copy.to_array(), x)
    with pytest.raises(RuntimeError):
        host[0, 5] = 1
    with pytest.raises(RuntimeError):
        res[0, 5] = 1


def test_overwrite_device_twin_and_verify(oracle):
    """overwrite_flac_device on an oracle-written store, all streams and a subset, with verify=True."""
    level, N = 1, 7000
    x = sinusoid_noise_i32(3, N, seed=8)
    blob, st, nb = oracle.encode_i32(x, level)
    dev = torch.device("cuda")
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)  # noqa: E731
    comp = up(blob)
    data = sinusoid_noise_i32(3, 2000, seed=9)
    out = fa.overwrite_flac_device(comp, up(st), up(nb), N, 1000, up(data), level=level, verify=True, compact=True)
    y = M.patched(x, 1000, data)
    for g, w in zip(out, oracle.encode_i32(y, level)):
        assert np.array_equal(g.cpu().numpy().reshape(-1), w.reshape(-1))
    out2 = fa.overwrite_flac_device(out[0], out[1], out[2], N, 6990, up(data[1:, :10]), streams=torch.tensor([2, 0]), level=level, verify=True)
    y2 = M.patched(y, 6990, data[1:, :10], [2, 0])
    for g, w in zip(out2, oracle.encode_i32(y2, level)):
        assert np.array_equal(g.cpu().numpy().reshape(-1), w.reshape(-1))
    assert np.array_equal(comp.cpu().numpy(), blob)
    with pytest.raises(ValueError, match="twice"):
        fa.overwrite_flac_device(comp, up(st), up(nb), N, 0, up(data[:2]), streams=[1, 1], level=level)
    with pytest.raises(ValueError, match="samples"):
        fa.overwrite_flac_device(comp, up(st), up(nb), N + 1, 0, up(data), level=level)
    with pytest.raises(ValueError, match="channel"):
        fa.overwrite_flac_device(comp, up(st), up(nb), N, 0, up(data.astype(np.int64)), level=level)


def test_overwrite_mid_size_splits_streams_over_workgroups(oracle, decoder_dispatch):
    """Streams of several hundred KB: the splice gives every stream several workgroups (one per ~64 KB of output), which
    share the prefix and suffix copies, the suffix seek points and the renumbered frames."""
    level, N = 5, 323_461
    x = _data("int32", 2, N, seed=30)
    data = (sinusoid_noise_i32(2, 40_000, seed=31) >> 9).astype(np.int32)
    arr, _, _ = _overwrite_and_check(oracle, x, 100_003, data, None, level)
    assert np.asarray(arr.stream_nbytes).min() > 4 * 65536


def test_overwrite_errors_leave_the_store(oracle):
    """Refused before any device copy: range, dtype, shape, level, a stream named twice, a libFLAC-style store."""
    x = _data("int32", 3, 9000, seed=2)
    arr = fa.FlacArray.from_device_array(torch.from_numpy(x).cuda(), level=5)
    before = _triple(arr)
    comp = arr._resident["compressed"]
    z = np.zeros((3, 10), dtype=np.int32)
    bad = [
        (dict(first=-1, data=z), "samples"),
        (dict(first=8991, data=z), "samples"),
        (dict(first=0, data=np.zeros((3, 9001), dtype=np.int32)), "samples"),
        (dict(first=0, data=z.astype(np.int64)), "dtype"),
        (dict(first=0, data=z.astype(np.float32)), "dtype"),
        (dict(first=0, data=z[:2]), "shape"),
        (dict(first=0, data=z[0]), "shape"),
        (dict(first=0, data=z, streams=[0, 2]), "shape"),
        (dict(first=0, data=z, level=1), "block size"),
        (dict(first=0, data=z[:2], streams=[2, 2]), "twice"),
        (dict(first=0, data=z[:2], streams=[0, 3]), "outside"),
    ]
    for kw, match in bad:
        with pytest.raises(ValueError, match=match):
            arr.overwrite(**kw)
        assert arr._resident["compressed"] is comp
    for g, w in zip(_triple(arr), before):
        assert np.array_equal(g, w)
    assert np.array_equal(arr.to_array(), x)
    # streams written without this library's SEEKTABLE (libFLAC's layout: a VORBIS_COMMENT block, no seek points)
    rng = np.random.default_rng(5)
    made = [W.write_stream(rng, 9000, 4096, layout="libflac", cheap=True) for _ in range(2)]
    blob, st, nb = W.pack([m[1] for m in made])
    foreign = fa.FlacArray._assemble((2, 9000), None, np.int32, blob, st, nb, None, None)
    assert np.array_equal(foreign.to_array(), np.stack([m[0] for m in made]))
    with pytest.raises(ValueError, match="SEEKTABLE"):
        foreign.overwrite(0, np.zeros((2, 10), dtype=np.int32))
    assert np.array_equal(foreign.compressed, blob)
    # the device twin refuses them too, on the device, before anything is decoded
    dev = torch.device("cuda")
    with pytest.raises(ValueError, match="SEEKTABLE"):
        fa.overwrite_flac_device(torch.from_numpy(blob).to(dev), torch.from_numpy(st).to(dev), torch.from_numpy(nb).to(dev), 9000, 0,
                                 torch.zeros((2, 10), dtype=torch.int32, device=dev), level=5)
