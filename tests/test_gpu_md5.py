"""STREAMINFO MD5 on the GPU: the lane-per-stream hash kernel, signing at encode time through every encode entry point,
the chunked decode-and-hash check, sign() and append.  Every expected value comes from hashlib over the integers: int32
rows as '<i4', int64 rows as '<i8' (two 32-bit channels interleaved, channel 0 = low word)."""
import hashlib

import numpy as np
import pytest

from flacarray_amd import libflacarray
from tests.conftest import full_range_i32, sinusoid_noise_f32, sinusoid_noise_i32
from tests.golden import flac_writer as W
from tests.golden import rfc9639
from tests.test_gpu_compare import GEOMS, _frame_offsets, _header_bytes

pytestmark = pytest.mark.gpu

LENGTHS = [0, 1, 13, 14, 15, 16, 17, 4095, 4096, 4097, 100_000]
STREAMS = [1, 63, 64, 65, 300]
SHAPES = sorted({shape for _, shape in GEOMS})
LEVELS = [0, 3, 5, 8]


@pytest.fixture(scope="module")
def torch():
    import torch

    return torch


@pytest.fixture(scope="module")
def fa():
    import flacarray_amd

    return flacarray_amd


@pytest.fixture(params=["auto", "k7"])
def decoder_dispatch(request, monkeypatch):
    """The decoder dispatches the neighbouring GPU test files run under (the variable is read per call); requested by
    every test that decodes."""
    monkeypatch.delenv("FLACARRAY_HIP_LATENCY", raising=False)
    if request.param == "k7":
        monkeypatch.setenv("FLACARRAY_HIP_LATENCY", "0")
    return request.param


def _md5(x):
    """hashlib's digest of every row of an integer array, (rows, 16) uint8."""
    x = np.asarray(x)
    fmt = {4: "<i4", 8: "<i8"}[x.dtype.itemsize]
    x2 = x.reshape(int(np.prod(x.shape[:-1], dtype=np.int64)), x.shape[-1]).astype(fmt)
    return np.stack([np.frombuffer(hashlib.md5(r.tobytes()).digest(), dtype=np.uint8) for r in x2])


def _full_range(dtype, shape, seed):
    rng = np.random.default_rng(seed)
    info = np.iinfo(dtype)
    x = rng.integers(info.min, info.max, size=shape, dtype=dtype, endpoint=True)
    flat = x.reshape(-1)
    if flat.size > 0:
        flat[0] = info.min
    if flat.size > 1:
        flat[-1] = info.max
    if flat.size > 2:
        flat[flat.size // 2] = info.min
    return x


def _dev(torch, *arrays):
    return tuple(torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in arrays)



# ---------------------------------------------------------------------------------------------------------------------
# md5_device
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [np.int32, np.int64])
@pytest.mark.parametrize("n", LENGTHS)
def test_md5_device_lengths_and_stream_counts(fa, torch, dtype, n):
    for ns in STREAMS:
        x = _full_range(dtype, (ns, n), seed=n + ns)
        got = fa.md5_device(torch.from_numpy(x).cuda())
        assert got.dtype == torch.uint8 and tuple(got.shape) == (ns, 16)
        assert np.array_equal(got.cpu().numpy(), _md5(x)), (dtype, n, ns)
    if n == 0:
        assert got.cpu().numpy()[0].tobytes() == hashlib.md5(b"").digest()


def test_md5_device_leading_shape_and_1d(fa, torch):
    x = _full_range(np.int32, (3, 5, 777), seed=1)
    assert np.array_equal(fa.md5_device(torch.from_numpy(x).cuda()).cpu().numpy(), _md5(x))
    y = _full_range(np.int64, (1001,), seed=2)
    assert np.array_equal(fa.md5_device(torch.from_numpy(y).cuda()).cpu().numpy(), _md5(y[None]))


@pytest.mark.parametrize("dtype", [np.int32, np.int64])
@pytest.mark.parametrize("width, lo, hi", [(1000, 16, 349), (1000, 3, 500), (1001, 0, 1001 - 8), (4096 + 64, 64, 64 + 4096), (999, 998, 999)])
def test_md5_device_column_range_of_a_wider_image(fa, torch, dtype, width, lo, hi):
    img = _full_range(dtype, (70, width), seed=width + lo)
    d = torch.from_numpy(img).cuda()
    got = fa.md5_device(d[:, lo:hi])
    assert np.array_equal(got.cpu().numpy(), _md5(img[:, lo:hi]))


@pytest.mark.parametrize("dtype", [np.int32, np.int64])
@pytest.mark.parametrize("cuts", [(1024,), (16,), (4096, 4096 + 16), (16, 32, 48, 1024, 4096, 8192 + 64), (8192 + 96,)])
def test_md5_device_resumed_equals_one_call(fa, torch, dtype, cuts):
    n = 8192 + 96 + (0 if cuts[-1] == 8192 + 96 else 37)
    x = _full_range(dtype, (65, n), seed=len(cuts))
    d = torch.from_numpy(x).cuda()
    whole = fa.md5_device(d)
    state, at = None, 0
    for c in cuts:
        state = fa.md5_device(d[:, at:c], state=state, n_before=at, final=False)
        assert state.dtype == torch.int32 and tuple(state.shape) == (65, 4)
        at = c
    got = fa.md5_device(d[:, at:], state=state, n_before=at, final=True)  # (possibly empty: only the padding is left)
    assert np.array_equal(got.cpu().numpy(), whole.cpu().numpy())
    assert np.array_equal(got.cpu().numpy(), _md5(x))


@pytest.mark.parametrize("ft", [np.float32, np.float64])
@pytest.mark.parametrize("shape", [(65, 5000), (3, 4096), (2, 7), (70, 1003)])
def test_md5_device_float_is_the_hash_of_the_quantised_integers(fa, torch, ft, shape):
    x = sinusoid_noise_f32(*shape, seed=shape[1]).astype(ft)
    x[0, 0] *= 1e3  # (a larger range in one stream: its own offset and gain)
    quanta = np.linspace(1e-4, 3e-3, shape[0]).astype(ft)
    wrap = libflacarray.wrap_float32_to_int32 if ft == np.float32 else libflacarray.wrap_float64_to_int64
    ints, off, gain = wrap(x.reshape(-1), shape[0], shape[1], quanta)
    want = _md5(ints.reshape(shape))
    dx, doff, dgain = _dev(torch, x, off, gain)
    assert np.array_equal(fa.md5_device(dx, doff, dgain).cpu().numpy(), want)
    # a column range, and resumed
    wide = np.concatenate([x, x[:, ::-1]], axis=1)
    dw = torch.from_numpy(wide).cuda()
    assert np.array_equal(fa.md5_device(dw[:, : shape[1]], doff, dgain).cpu().numpy(), want)
    if shape[1] > 64:
        state = fa.md5_device(dx[:, :64], doff, dgain, final=False)
        got = fa.md5_device(dx[:, 64:], doff, dgain, state=state, n_before=64)
        assert np.array_equal(got.cpu().numpy(), want)


@pytest.mark.parametrize("ft", [np.float32, np.float64])
def test_md5_device_nan_raises(fa, torch, ft):
    x = sinusoid_noise_f32(5, 3000, seed=4).astype(ft)
    x[3, 2999] = np.nan
    one = torch.ones(5, dtype=torch.float32 if ft == np.float32 else torch.float64).cuda()
    with pytest.raises(RuntimeError, match="NaN"):
        fa.md5_device(torch.from_numpy(x).cuda(), one, one)


# ---------------------------------------------------------------------------------------------------------------------
# signing at encode time
# ---------------------------------------------------------------------------------------------------------------------
def _check_signed_pair(fa, plain, signed, want):
    """`signed` equals `plain` in starts, nbytes and every byte but [26, 42) of each stream; those are `want`; the plain
    ones are zero."""
    (c0, s0, n0), (c1, s1, n1) = [tuple(np.asarray(a.cpu().numpy() if hasattr(a, "cpu") else a) for a in t[:3]) for t in (plain, signed)]
    assert np.array_equal(s0, s1) and np.array_equal(n0, n1) and c0.shape == c1.shape
    field = (s0.reshape(-1)[:, None] + 26 + np.arange(16)[None, :]).reshape(-1)
    mask = np.ones(c0.size, dtype=bool)
    mask[field] = False
    assert np.array_equal(c0[mask], c1[mask])
    assert not fa.stream_md5(c0, s0.reshape(-1)).any()
    assert np.array_equal(fa.stream_md5(c1, s1.reshape(-1)), want)


@pytest.mark.parametrize("level", LEVELS)
@pytest.mark.parametrize("shape", SHAPES)
def test_encode_device_md5_int32(fa, torch, level, shape):
    x = sinusoid_noise_i32(*shape, seed=level + shape[0])
    x[0, :3] = [np.iinfo(np.int32).min, np.iinfo(np.int32).max, -1]
    d = torch.from_numpy(x).cuda()
    plain = fa.encode_flac_device(d, level=level, md5=False)
    default = fa.encode_flac_device(d, level=level)
    signed = fa.encode_flac_device(d, level=level, md5=True)
    assert np.array_equal(plain[0].cpu().numpy(), default[0].cpu().numpy())
    _check_signed_pair(fa, plain, signed, _md5(x))


@pytest.mark.parametrize("level", LEVELS)
def test_encode_device_md5_int64_and_floats(fa, torch, level):
    shape = (12, 20_000)
    x64 = sinusoid_noise_i32(*shape, seed=level).astype(np.int64) * 3_000_001 + 12345
    x64[0, :2] = [np.iinfo(np.int64).min, np.iinfo(np.int64).max]
    d = torch.from_numpy(x64).cuda()
    _check_signed_pair(fa, fa.encode_flac_device(d, level=level), fa.encode_flac_device(d, level=level, md5=True), _md5(x64))
    for ft, enc, shp in ((np.float32, fa.encode_flac_device_f32, (8, 16_384)), (np.float32, fa.encode_flac_device_f32, shape),
                         (np.float64, fa.encode_flac_device_f64, shape)):
        x = sinusoid_noise_f32(*shp, seed=level + 1).astype(ft)
        q = torch.full((shp[0],), 1e-3, dtype=torch.float32 if ft == np.float32 else torch.float64).cuda()
        dx = torch.from_numpy(x).cuda()
        plain = enc(dx, q, level=level)
        signed = enc(dx, q, level=level, md5=True)
        ints = fa.decode_flac_device(plain[0], plain[1], plain[2], shp[1], is_int64=ft == np.float64).cpu().numpy()
        wrap = libflacarray.wrap_float32_to_int32 if ft == np.float32 else libflacarray.wrap_float64_to_int64
        model, _, _ = wrap(x.reshape(-1), shp[0], shp[1], np.full(shp[0], 1e-3, dtype=ft))
        assert np.array_equal(ints, model.reshape(shp))
        _check_signed_pair(fa, plain, signed, _md5(ints))


@pytest.mark.parametrize("level", [0, 5])
def test_host_encoders_sign(fa, torch, level, monkeypatch):
    """encode_flac, array_compress, FlacArray.from_array / from_device_array with md5=True, and the reference's C entry
    points under set_encode_md5(True); several chunks of streams through the host pipeline."""
    monkeypatch.setenv("FLACARRAY_HIP_HOST_CHUNK_BYTES", str(5 * 9000 * 4))
    shape = (12, 9000)
    x = sinusoid_noise_i32(*shape, seed=level + 5)
    x64 = x.astype(np.int64) * 3_000_001 - 7
    xf = sinusoid_noise_f32(*shape, seed=level + 6)
    xd = xf.astype(np.float64)
    for arr in (x, x64):
        plain = fa.encode_flac(arr, level)
        _check_signed_pair(fa, plain, fa.encode_flac(arr, level, md5=True), _md5(arr))
        _check_signed_pair(fa, plain, fa.array_compress(arr, level=level, md5=True), _md5(arr))
        _check_signed_pair(fa, fa.array_compress(arr, level=level, md5=False), fa.array_compress(arr, level=level, md5=True), _md5(arr))
        a = fa.FlacArray.from_array(arr, level=level, md5=True)
        assert np.array_equal(a.md5, _md5(arr)) and not fa.FlacArray.from_array(arr, level=level).md5.any()
        r = fa.FlacArray.from_device_array(torch.from_numpy(arr).cuda(), level=level, md5=True)
        assert np.array_equal(r.md5, _md5(arr)) and a == r
        assert np.array_equal(r._resident["compressed"].cpu().numpy(), r.compressed)
        wrap = libflacarray.wrap_encode_i32 if arr.dtype == np.int32 else libflacarray.wrap_encode_i64
        assert fa.set_encode_md5(True) is False
        try:
            by_default = wrap(arr.reshape(-1), shape[0], shape[1], level)
            assert np.array_equal(fa.FlacArray.from_array(arr, level=level).md5, _md5(arr))  # (md5=None follows the default)
            assert not fa.FlacArray.from_array(arr, level=level, md5=False).md5.any()
            assert np.array_equal(fa.encode_flac_device(torch.from_numpy(arr).cuda(), level=level)[0].cpu().numpy(), by_default[0])
        finally:
            assert fa.set_encode_md5(False) is True
        _check_signed_pair(fa, plain, by_default, _md5(arr))
    for arr in (xf, xd):
        plain = fa.array_compress(arr, level=level, quanta=1e-3)
        signed = fa.array_compress(arr, level=level, quanta=1e-3, md5=True)
        ints = fa.decode_flac(plain[0], plain[1], plain[2], shape[1], is_int64=arr.dtype == np.float64)
        _check_signed_pair(fa, plain, signed, _md5(ints))
        a = fa.FlacArray.from_array(arr, level=level, quanta=1e-3, md5=True)
        r = fa.FlacArray.from_device_array(torch.from_numpy(arr).cuda(), level=level, quanta=1e-3, md5=True)
        assert np.array_equal(a.md5, _md5(ints)) and a == r


# ---------------------------------------------------------------------------------------------------------------------
# check
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [np.int32, np.int64])
def test_check_signed_unsigned_and_a_flipped_digest_byte(fa, torch, decoder_dispatch, dtype):
    shape = (6, 20_000)
    x = sinusoid_noise_i32(*shape, seed=31).astype(dtype)
    d = torch.from_numpy(x).cuda()
    i64 = dtype == np.int64
    comp, st, nb = fa.encode_flac_device(d, level=5, md5=True)
    status, dig = fa.check_md5_device(comp, st, nb, shape[1], is_int64=i64, return_digests=True)
    assert status.dtype == torch.int8 and (status.cpu().numpy() == 1).all()
    assert np.array_equal(dig.cpu().numpy(), _md5(x))
    plain = fa.encode_flac_device(d, level=5)
    assert (fa.check_md5_device(*plain, shape[1], is_int64=i64).cpu().numpy() == -1).all()
    status, dig = fa.check_md5_device(*plain, shape[1], is_int64=i64, return_digests=True)
    assert (status.cpu().numpy() == -1).all() and np.array_equal(dig.cpu().numpy(), _md5(x))
    bad = comp.clone()
    bad[int(st[2]) + 26 + 9] ^= 0x40
    e = np.ones(shape[0], dtype=np.int8)
    e[2] = 0
    assert np.array_equal(fa.check_md5_device(bad, st, nb, shape[1], is_int64=i64).cpu().numpy(), e)
    # the same through FlacArray, host store and resident store
    a = fa.FlacArray.from_array(x.reshape(2, 3, -1), level=5, md5=True)
    assert a.check_md5().shape == (2, 3) and a.check_md5().dtype == np.int8 and (a.check_md5() == 1).all()
    assert (a.to_device().check_md5() == 1).all()
    assert (fa.FlacArray.from_array(x, level=5).check_md5() == -1).all()


def test_check_catches_a_payload_bit_the_frame_crc_is_not_asked_about(fa, torch, decoder_dispatch):
    """full_range_i32 data are VERBATIM frames: a flipped bit inside sample i's bytes changes sample i and nothing else.
    Frame CRC checking is off, so the decode itself succeeds and the MD5 is what notices."""
    shape = (6, 20_000)
    x = full_range_i32(shape)
    comp, st, nb = fa.encode_flac_device(torch.from_numpy(x).cuda(), level=5, md5=True)
    blob = comp.cpu().numpy().copy()
    starts, nbytes = st.cpu().numpy(), nb.cpu().numpy()
    s, i = 4, 5000
    seg = blob[starts[s] : starts[s] + nbytes[s]]
    at = _frame_offsets(seg)[1]
    sub = at + _header_bytes(seg, at)
    assert seg[sub] == 0x02
    blob[starts[s] + sub + 1 + 4 * (i - 4096) + 2] ^= 0x10
    dblob = torch.from_numpy(blob).cuda()
    y = fa.decode_flac_device(dblob, st, nb, shape[1], verify=False).cpu().numpy()
    assert np.array_equal(np.argwhere(y != x), [[s, i]])
    e = np.ones(shape[0], dtype=np.int8)
    e[s] = 0
    assert np.array_equal(fa.check_md5_device(dblob, st, nb, shape[1], verify=False).cpu().numpy(), e)
    assert (fa.check_md5_device(comp, st, nb, shape[1], verify=False).cpu().numpy() == 1).all()


@pytest.mark.parametrize("dtype", [np.int32, np.int64])
def test_check_in_several_column_chunks_with_a_ragged_last_one(fa, torch, decoder_dispatch, dtype):
    shape = (5, 20_000 + 13)
    x = sinusoid_noise_i32(*shape, seed=41).astype(dtype)
    i64 = dtype == np.int64
    comp, st, nb = fa.encode_flac_device(torch.from_numpy(x).cuda(), level=5, md5=True)
    item = 8 if i64 else 4
    for width in (4096, 10_000 - 10_000 % 16, 16):  # frame-aligned chunks, chunks that cut frames, one 64-byte block per chunk
        if width == 16 and decoder_dispatch == "k7":
            continue  # (1251 ranged decodes; once is enough)
        cap = shape[0] * width * item
        status, dig = fa.check_md5_device(comp, st, nb, shape[1], is_int64=i64, return_digests=True, max_temp_bytes=cap)
        assert (status.cpu().numpy() == 1).all(), width
        assert np.array_equal(dig.cpu().numpy(), _md5(x)), width
    assert shape[1] % 4096 % 16 != 0  # the last chunk is ragged in every case


def _single_block(batches):
    return [b for b in batches if b["block"] is not None]


def test_check_foreign_signatures(fa, torch, decoder_dispatch):
    """The 114 streams of flac_writer.all_batches() carry signatures this code did not compute (tests/test_md5_host.py
    checks all of them against hashlib on the CPU).  Default cap: every stream in one chunk, all must match.  Small cap:
    several chunks, for the batches of one block size (ranged decodes need one)."""
    batches = W.all_batches()
    checked = failed = 0
    for b in batches:
        blob, st, nb = W.pack(b["streams"])
        d = _dev(torch, blob, st, nb)
        status = fa.check_md5_device(*d, b["n"], is_int64=b["channels"] == 2).cpu().numpy()
        checked += status.size
        failed += int((status != 1).sum())
        assert (status == 1).all(), (b["name"], status)
    assert (len(batches), checked, failed) == (50, 114, 0)
    single = _single_block(batches)
    checked = 0
    for b in single:
        blob, st, nb = W.pack(b["streams"])
        d = _dev(torch, blob, st, nb)
        k, item = len(b["streams"]), 4 * b["channels"]
        per_block = 64 // item
        width = max(per_block, (b["n"] // 3) // per_block * per_block)
        assert -(-b["n"] // width) >= 3, b["name"]  # several chunks
        status = fa.check_md5_device(*d, b["n"], is_int64=b["channels"] == 2, max_temp_bytes=k * width * item).cpu().numpy()
        checked += status.size
        assert (status == 1).all(), (b["name"], width, status)
    assert (len(single), checked) == (49, 110)


@pytest.mark.parametrize("name", ["example1", "example2", "example3"])
def test_check_narrow_samples_are_not_checkable(fa, torch, name):
    data, channels, bps, n, _ = rfc9639.EXAMPLES[name]
    blob = np.frombuffer(data, dtype=np.uint8).copy()
    d = _dev(torch, blob, np.array([0], np.int64), np.array([blob.size], np.int64))
    assert bps in (8, 16)
    status, dig = fa.check_md5_device(*d, n, is_int64=channels == 2, return_digests=True)
    assert status.cpu().numpy().tolist() == [-2] and not dig.cpu().numpy().any()


# ---------------------------------------------------------------------------------------------------------------------
# sign
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("resident", [False, True])
@pytest.mark.parametrize("dtype", [np.int32, np.int64])
def test_sign_an_unsigned_store(fa, torch, decoder_dispatch, dtype, resident):
    x = sinusoid_noise_i32(6, 20_000, seed=51).astype(dtype).reshape(2, 3, -1)
    a = fa.FlacArray.from_device_array(torch.from_numpy(x).cuda(), level=5) if resident else fa.FlacArray.from_array(x, level=5)
    before = fa.FlacArray(a)
    unsigned = a.compressed.copy()
    assert a.sign() is a
    assert (a.check_md5() == 1).all()
    assert a.md5.shape == (2, 3, 16) and np.array_equal(a.md5.reshape(-1, 16), _md5(x))
    assert not before.md5.any() and np.array_equal(before.compressed, unsigned) and before != a
    assert np.array_equal(a.stream_starts, before.stream_starts) and np.array_equal(a.stream_nbytes, before.stream_nbytes)
    assert a == fa.FlacArray.from_array(x, level=5, md5=True)
    assert a.is_resident == resident
    if resident:
        assert np.array_equal(a._resident["compressed"].cpu().numpy(), a.compressed)
    assert np.array_equal(a.to_array(), x)


def test_sign_a_float_store(fa, torch, decoder_dispatch):
    x = sinusoid_noise_f32(6, 20_000, seed=53)
    a = fa.FlacArray.from_array(x, level=5, quanta=1e-3).sign()
    ints = fa.decode_flac(a.compressed, a.stream_starts, a.stream_nbytes, 20_000)
    assert np.array_equal(a.md5, _md5(ints)) and (a.check_md5() == 1).all()
    assert a == fa.FlacArray.from_array(x, level=5, quanta=1e-3, md5=True)


def test_sign_a_foreign_store_with_its_digest_zeroed(fa, torch, decoder_dispatch):
    for b in [bb for bb in _single_block(W.all_batches())][:6]:
        blob, st, nb = W.pack(b["streams"])
        want = fa.stream_md5(blob, st)
        blob[(st[:, None] + 26 + np.arange(16)[None, :]).reshape(-1)] = 0
        dt = np.int32 if b["channels"] == 1 else np.int64
        a = fa.FlacArray._assemble((len(b["streams"]), b["n"]), None, dt, blob, st, nb, None, None)
        assert (a.check_md5() == -1).all()
        a.sign()
        assert np.array_equal(a.md5, want) and np.array_equal(a.md5, _md5(b["samples"])) and (a.check_md5() == 1).all(), b["name"]


def test_sign_refuses_narrow_samples(fa, torch):
    data, channels, bps, n, _ = rfc9639.EXAMPLES["example3"]
    blob = np.frombuffer(data, dtype=np.uint8).copy()
    a = fa.FlacArray._assemble((1, n), None, np.int32, blob, np.array([0], np.int64), np.array([blob.size], np.int64), None, None)
    assert a.check_md5().tolist() == [-2]
    with pytest.raises(ValueError, match="32 bits per sample"):
        a.sign()


def test_sign_streams_device_rejects_a_blob_without_streaminfo(fa, torch):
    comp = torch.zeros(200, dtype=torch.uint8).cuda()
    st = torch.tensor([0, 100], dtype=torch.int64).cuda()
    with pytest.raises(ValueError, match="fLaC"):
        fa.sign_streams_device(comp, st, torch.full((2, 16), 7, dtype=torch.uint8).cuda())
    assert not comp.cpu().numpy().any()  # nothing written


# ---------------------------------------------------------------------------------------------------------------------
# append
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("resident", [False, True])
@pytest.mark.parametrize("kind", ["int32", "int64", "float32"])
def test_append_md5(fa, torch, decoder_dispatch, kind, resident):
    n0, n1 = 10_000, 7001
    base = sinusoid_noise_i32(5, n0 + n1, seed=61)
    if kind == "int64":
        base = base.astype(np.int64) * 3_000_001 + 5
    if kind == "float32":
        base = sinusoid_noise_f32(5, n0 + n1, seed=61)
    kw = {"quanta": 1e-3} if kind == "float32" else {}

    def make(md5):
        x0 = np.ascontiguousarray(base[:, :n0])
        if resident:
            return fa.FlacArray.from_device_array(torch.from_numpy(x0).cuda(), level=5, md5=md5, **kw)
        return fa.FlacArray.from_array(x0, level=5, md5=md5, **kw)

    tail = np.ascontiguousarray(base[:, n0:])
    # by default: unsigned (also when the old store was signed), and byte for byte what an append gave before
    plain = make(False).append(tail)
    from_signed = make(True).append(tail)
    assert not plain.md5.any() and plain == from_signed
    if kind != "float32":
        assert plain == fa.FlacArray.from_array(base, level=5)
    # md5=True: the digest of the concatenated integers
    signed = make(False).append(tail, md5=True)
    ints = fa.decode_flac(plain.compressed, plain.stream_starts, plain.stream_nbytes, n0 + n1, is_int64=kind == "int64")
    if kind != "float32":
        assert np.array_equal(ints, base)
    assert np.array_equal(signed.md5, _md5(ints)) and (signed.check_md5() == 1).all()
    _check_signed_pair(fa, (plain.compressed, plain.stream_starts, plain.stream_nbytes),
                       (signed.compressed, signed.stream_starts, signed.stream_nbytes), _md5(ints))
    if resident:
        assert np.array_equal(signed._resident["compressed"].cpu().numpy(), signed.compressed)
    # the device call
    d = _dev(torch, make(False).compressed, make(False).stream_starts, make(False).stream_nbytes)
    if kind != "float32":
        out = fa.append_flac_device(*d, n0, torch.from_numpy(tail).cuda(), level=5, md5=True)
        assert np.array_equal(out[0].cpu().numpy(), signed.compressed)
