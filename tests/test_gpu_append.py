"""GPU tests of FlacArray.append / append_flac_device: the appended store is byte for byte the one-shot encode of the
concatenation (and the oracle's), for int32 / int64 at levels 0-8 and any chunking; float stores quantise the new
samples with their own offsets and gains (a given-parameter model of utils.c:229-240 / :316-323 below)."""
import numpy as np
import pytest
import torch

import flacarray_amd as fa
from tests import quant_model as Q
from tests.conftest import sinusoid_noise_f32, sinusoid_noise_i32

pytestmark = pytest.mark.gpu


@pytest.fixture(params=["auto", "k7"])
def decoder_dispatch(request, monkeypatch):
    """As in test_gpu_parity.py: the library's own dispatch, and K7 + K3F for every array of their geometry -- so the
    tail decode and the chunk encode take both kernel families."""
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


def _same_store(arr, want):
    blob, st, nb = want
    assert np.array_equal(np.asarray(arr.compressed), blob)
    assert np.array_equal(np.asarray(arr.stream_starts).reshape(-1), np.asarray(st).reshape(-1))
    assert np.array_equal(np.asarray(arr.stream_nbytes).reshape(-1), np.asarray(nb).reshape(-1))


CHUNKINGS = {
    "frame_boundary": lambda B: [2 * B, B, 2 * B + 7],
    "inside_frame": lambda B: [B + 100, 1, 517, 3 * B - 1, 25],
    "short_start": lambda B: [5, B - 5, 3, 2 * B],
}


@pytest.mark.parametrize("kind", ["int32", "int64"])
@pytest.mark.parametrize("level", [0, 1, 3, 5, 8])
@pytest.mark.parametrize("chunking", sorted(CHUNKINGS))
def test_append_equals_one_shot_encode(oracle, decoder_dispatch, kind, level, chunking):
    B = 1152 if level <= 2 else 4096
    sizes = CHUNKINGS[chunking](B)
    x = _data(kind, 3, sum(sizes), seed=level + 1)
    arr = fa.FlacArray.from_array(np.ascontiguousarray(x[:, : sizes[0]]), level=level)
    pos = sizes[0]
    for k in sizes[1:]:
        arr.append(np.ascontiguousarray(x[:, pos : pos + k]), level=level)
        pos += k
    assert arr.shape == x.shape
    one = fa.FlacArray.from_array(x, level=level)
    _same_store(arr, (one.compressed, one.stream_starts, one.stream_nbytes))
    enc = oracle.encode_i64 if kind == "int64" else oracle.encode_i32
    _same_store(arr, enc(x, level))
    assert np.array_equal(arr.to_array(), x)


def test_append_across_frame_2048_utf8_growth():
    """Level 5, streams of 2048 x 4096 + 3 samples grown by a chunk: the new frames' numbers cross 2048, where their
    UTF-8 field grows from two to three bytes."""
    B = 4096
    n_old, n_new = 2047 * B + 3, B + 2 * B
    x = _data("int32", 3, n_old + n_new, seed=9)
    xt = torch.from_numpy(x).cuda()
    arr = fa.FlacArray.from_device_array(xt[:, :n_old].contiguous(), level=5)
    arr.append(xt[:, n_old:].contiguous(), level=5)
    comp, st, nb = fa.encode_flac_device(xt, level=5, compact=True)
    _same_store(arr, (comp.cpu().numpy(), st.cpu().numpy(), nb.cpu().numpy()))
    assert arr.is_resident
    assert np.array_equal(arr[:, n_old - 10 : n_old + 10], x[:, n_old - 10 : n_old + 10])


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("resident", [False, True])
def test_append_float_quantises_with_store_parameters(oracle, dtype, resident):
    level, n_old, n_new = 5, 5000, 4200
    x = sinusoid_noise_f32(3, n_old + n_new, seed=4).astype(dtype)
    # out-of-range values: far outside the old range (INT_MIN), and the infinities
    x[0, n_old + 3] = 1e30
    x[1, n_old + 7] = -1e30
    x[2, n_old + 11] = np.inf
    x[2, n_old + 12] = -np.inf
    arr = fa.FlacArray.from_array(np.ascontiguousarray(x[:, :n_old]), level=level, quanta=1e-3)
    if resident:
        arr.to_device()
    off, gain = np.array(arr.stream_offsets), np.array(arr.stream_gains)
    wide = dtype == np.float64
    dec = oracle.decode_i64 if wide else oracle.decode_i32
    old_ints = dec(arr.compressed, arr.stream_starts, arr.stream_nbytes, n_old)
    arr.append(np.ascontiguousarray(x[:, n_old:]), level=level)
    ints = np.concatenate([old_ints, quantise_given(x[:, n_old:], off, gain)], axis=1)
    assert ints.min() == np.iinfo(ints.dtype).min
    _same_store(arr, (oracle.encode_i64 if wide else oracle.encode_i32)(ints, level))
    assert np.array_equal(arr.stream_offsets, off) and np.array_equal(arr.stream_gains, gain)
    restore = Q.int64_to_float64 if wide else Q.int32_to_float32
    assert Q.bits_equal(arr.to_array(), restore(ints, off, gain))
    assert arr.is_resident == resident


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_append_nan_raises_and_leaves_the_store(dtype):
    x = sinusoid_noise_f32(2, 6000, seed=5).astype(dtype)
    arr = fa.FlacArray.from_array(np.ascontiguousarray(x[:, :4000]), level=5, quanta=1e-3)
    before = (arr.compressed.copy(), np.array(arr.stream_starts), arr.shape)
    y = np.ascontiguousarray(x[:, 4000:])
    y[1, 17] = np.nan
    with pytest.raises(RuntimeError, match="NaN"):
        arr.append(y)
    assert np.array_equal(arr.compressed, before[0]) and np.array_equal(arr.stream_starts, before[1]) and arr.shape == before[2]


@pytest.mark.parametrize("kind", ["int32", "int64"])
def test_append_resident_and_host_agree_and_read_across(kind):
    x = _data(kind, 4, 9000 + 5000, seed=6)
    host = fa.FlacArray.from_array(np.ascontiguousarray(x[:, :9000]), level=5)
    res = fa.FlacArray.from_device_array(torch.from_numpy(np.ascontiguousarray(x[:, :9000])).cuda(), level=5)
    res.to_array()  # (builds the decode index, which the append must close and rebuild)
    copy = fa.FlacArray(host)
    host.append(np.ascontiguousarray(x[:, 9000:]), verify=True)
    res.append(torch.from_numpy(np.ascontiguousarray(x[:, 9000:])).cuda(), verify=True)
    assert res.is_resident and not host.is_resident
    assert host == res and np.array_equal(host.compressed, res.compressed)
    for arr in (host, res):
        assert np.array_equal(arr[1:3, 8000:10000], x[1:3, 8000:10000])
        got = arr.read_slices([0, 3, 2], [8190, 0, 12000], [20, 14000, 2000])
        assert np.array_equal(got[0], x[0, 8190:8210]) and np.array_equal(got[1], x[3]) and np.array_equal(got[2], x[2, 12000:])
        assert np.all(arr.first_mismatch(x) == -1)
    assert copy.shape == (4, 9000) and np.array_equal(copy.to_array(), x[:, :9000])


def test_append_single_stream_and_device_twin(oracle):
    x = sinusoid_noise_i32(1, 7000, seed=8).reshape(-1)
    arr = fa.FlacArray.from_array(np.ascontiguousarray(x[:3000]), level=1)
    arr.append(np.ascontiguousarray(x[3000:]), level=1)
    assert arr.shape == (7000,)
    _same_store(arr, oracle.encode_i32(x.reshape(1, -1), 1))
    blob, st, nb = oracle.encode_i32(x[:3000].reshape(1, -1), 1)
    dev = torch.device("cuda")
    out = fa.append_flac_device(torch.from_numpy(blob).to(dev), torch.from_numpy(st).to(dev), torch.from_numpy(nb).to(dev), 3000,
                                torch.from_numpy(np.ascontiguousarray(x[3000:])).to(dev), level=1, verify=True)
    _same_store(arr, tuple(t.cpu().numpy() for t in out))


@pytest.mark.parametrize("level", [1, 5])
@pytest.mark.parametrize("kind", ["int32", "int64"])
def test_append_mid_size_splits_streams_over_workgroups(oracle, decoder_dispatch, kind, level):
    """Streams of several hundred KB: the splice gives every stream several workgroups (one per ~64 KB of output), so the
    copy of the kept frames and the renumbered frames are shared out over them."""
    n_old, n_new = 200_003, 123_457
    x = _data(kind, 2, n_old + n_new, seed=level + 20)
    arr = fa.FlacArray.from_array(np.ascontiguousarray(x[:, :n_old]), level=level)
    arr.append(np.ascontiguousarray(x[:, n_old:]), level=level)
    assert np.asarray(arr.stream_nbytes).min() > 4 * 65536
    _same_store(arr, (oracle.encode_i64 if kind == "int64" else oracle.encode_i32)(x, level))


@pytest.mark.parametrize("n_old", [2 * 4096, 2 * 4096 + 5])
@pytest.mark.parametrize("kind", ["int32", "int64"])
def test_append_device_twin_refuses_data_of_the_other_width(oracle, kind, n_old):
    """int32 data against two-channel streams (and int64 against one-channel streams) raise before anything is written,
    with and without an old short tail."""
    x = _data(kind, 2, n_old)
    blob, st, nb = (oracle.encode_i64 if kind == "int64" else oracle.encode_i32)(x, 5)
    dev = torch.device("cuda")
    other = torch.from_numpy(np.zeros((2, 100), dtype=np.int32 if kind == "int64" else np.int64)).to(dev)
    comp = torch.from_numpy(blob).to(dev)
    with pytest.raises(ValueError, match="channel"):
        fa.append_flac_device(comp, torch.from_numpy(st).to(dev), torch.from_numpy(nb).to(dev), n_old, other, level=5)
    assert np.array_equal(comp.cpu().numpy(), blob)


@pytest.mark.parametrize("delta", [-1, 1])
def test_append_device_twin_refuses_a_wrong_stream_size(oracle, delta):
    """A stream_size other than the one in STREAMINFO -- here one that keeps the frame count -- raises ValueError instead of
    dropping or inventing tail samples."""
    n_old = 3 * 4096 + 100
    x = _data("int32", 2, n_old)
    blob, st, nb = oracle.encode_i32(x, 5)
    dev = torch.device("cuda")
    new = torch.from_numpy(np.zeros((2, 100), dtype=np.int32)).to(dev)
    with pytest.raises(ValueError, match="samples"):
        fa.append_flac_device(torch.from_numpy(blob).to(dev), torch.from_numpy(st).to(dev), torch.from_numpy(nb).to(dev), n_old + delta,
                              new, level=5)


def test_append_keeps_a_resident_blob_of_exact_size():
    x = _data("int32", 2, 9000)
    arr = fa.FlacArray.from_device_array(torch.from_numpy(np.ascontiguousarray(x[:, :5000])).cuda(), level=5)
    arr.append(torch.from_numpy(np.ascontiguousarray(x[:, 5000:])).cuda())
    comp = arr._resident["compressed"]
    assert comp.untyped_storage().nbytes() == comp.numel() == arr.compressed.size
    assert np.array_equal(arr.to_array(), x)
