"""The compare sink (compare_flac_device, FlacArray.first_mismatch) and verification after encode (verify=, set_encode_verify)
on the GPU.

Geometries reach both single-pass encoders: (64, 300_000) at levels 5 and 8 has 4736 frames and goes to K3F; (8, 300_000)
and (12, 1000) go to K3G, as every level-0 array does.  Every stream ends in a short frame.  Mutated copies must give
exactly the first changed sample of each stream and -1 for the others; what is compared is integers, so a float change
that leaves its quantised integer the same is not a mismatch."""
import numpy as np
import pytest

from tests import quant_model as M
from tests.compare_corpus import _frame_offsets, _header_bytes
from tests.conftest import full_range_i32, sinusoid_noise_f32, sinusoid_noise_i32, strip_seektable

pytestmark = pytest.mark.gpu

GEOMS = [(0, (8, 300_000)), (0, (12, 1000)), (5, (64, 300_000)), (5, (8, 300_000)), (5, (12, 1000)), (8, (64, 300_000)),
         (8, (8, 300_000)), (8, (12, 1000)), (5, (8, 300_001))]  # (an odd length: rows not 16-byte aligned)


@pytest.fixture(scope="module")
def torch():
    import torch

    assert torch.cuda.is_available()
    return torch


@pytest.fixture(scope="module")
def fa():
    import flacarray_amd

    return flacarray_amd


def _block(level):
    return 1152 if level <= 2 else 4096


def _positions(shape, level):
    """{stream: [changed samples]}: a stream's first sample, both sides of the first frame boundary, the last sample, two
    far apart, and one inside the short last frame."""
    n_stream, n = shape
    B = _block(level)
    short0 = (n // B) * B
    short = short0 + (n - short0) // 2 if n % B else n - 1
    pos = {0: [0], 1: [min(B - 1, n - 1)], 2: [n - 1], 3: [min(12345, n // 3), min(200_000, n - 2)], 5: [short]}
    return pos


def _mutate(x, pos, delta):
    y = x.copy()
    for s, idx in pos.items():
        for i in idx:
            y[s, i] = delta(y[s, i])
    return y


def _expect(n_stream, pos):
    e = np.full(n_stream, -1, dtype=np.int64)
    for s, idx in pos.items():
        e[s] = min(idx)
    return e


def _compare(fa, torch, comp, st, nb, x, offsets=None, gains=None):
    return fa.compare_flac_device(comp, st, nb, torch.from_numpy(np.ascontiguousarray(x)).cuda(), offsets, gains).cpu().numpy()


@pytest.mark.parametrize("level, shape", GEOMS)
def test_compare_int32(fa, torch, level, shape):
    x = sinusoid_noise_i32(*shape, seed=level + shape[0])
    comp, st, nb = fa.encode_flac_device(torch.from_numpy(x).cuda(), level=level)
    assert (_compare(fa, torch, comp, st, nb, x) == -1).all()
    pos = _positions(shape, level)
    y = _mutate(x, pos, lambda v: v ^ 1)
    assert np.array_equal(_compare(fa, torch, comp, st, nb, y), _expect(shape[0], pos))
    # the other side of the first frame boundary, alone
    B = _block(level)
    if shape[1] > B:
        pos2 = {1: [B], 4: [B], 6: [shape[1] - 1]}
        assert np.array_equal(_compare(fa, torch, comp, st, nb, _mutate(x, pos2, lambda v: v + 7)), _expect(shape[0], pos2))
    # streams without their SEEKTABLE (found by the sync scan) compare the same
    blob2, st2, nb2 = strip_seektable(comp.cpu().numpy(), st.cpu().numpy(), nb.cpu().numpy())
    c2, s2, n2 = (torch.from_numpy(a).cuda() for a in (blob2, st2, nb2))
    assert np.array_equal(_compare(fa, torch, c2, s2, n2, y), _expect(shape[0], pos))
    assert (_compare(fa, torch, c2, s2, n2, x) == -1).all()


@pytest.mark.parametrize("level, shape", [(0, (8, 300_000)), (5, (8, 300_000)), (5, (12, 1000))])
def test_compare_int64_high_and_low_words(fa, torch, level, shape):
    x = sinusoid_noise_i32(*shape, seed=7).astype(np.int64) * 3_000_001 + 12345
    comp, st, nb = fa.encode_flac_device(torch.from_numpy(x).cuda(), level=level)
    assert (_compare(fa, torch, comp, st, nb, x) == -1).all()
    pos = _positions(shape, level)
    for delta in (lambda v: v ^ (1 << 40), lambda v: v ^ 1):
        y = _mutate(x, pos, delta)
        assert np.array_equal(_compare(fa, torch, comp, st, nb, y), _expect(shape[0], pos))
    blob2, st2, nb2 = strip_seektable(comp.cpu().numpy(), st.cpu().numpy(), nb.cpu().numpy())
    c2, s2, n2 = (torch.from_numpy(a).cuda() for a in (blob2, st2, nb2))
    assert np.array_equal(_compare(fa, torch, c2, s2, n2, _mutate(x, pos, lambda v: v ^ (1 << 40))), _expect(shape[0], pos))


def _float_case(dtype, shape, seed=3):
    x = sinusoid_noise_f32(*shape, seed=seed).astype(dtype)
    q = np.full(shape[0], 1e-3, dtype=dtype)
    return x, q


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("level, shape", [(5, (64, 65_536)), (5, (8, 300_000)), (0, (12, 1000)), (5, (8, 300_001))])
def test_compare_float_quanta(fa, torch, dtype, level, shape):
    x, q = _float_case(dtype, shape)
    enc = fa.encode_flac_device_f32 if dtype == np.float32 else fa.encode_flac_device_f64
    comp, st, nb, off, gain = enc(torch.from_numpy(x).cuda(), torch.from_numpy(q).cuda(), level=level)
    assert (_compare(fa, torch, comp, st, nb, x, off, gain) == -1).all()
    ints = M.quantise(x, q)[0]
    pos = _positions(shape, level)
    # one and a half quanta: the quantised integer moves
    y = _mutate(x, pos, lambda v: v + dtype(1.5e-3))
    assert np.array_equal(_compare(fa, torch, comp, st, nb, y, off, gain), _expect(shape[0], pos))
    # the next float up: the quantised integer stays (checked with the model) -- not a mismatch
    z = _mutate(x, pos, lambda v: np.nextafter(v, dtype(np.inf)))
    zi = M.quantise(z, q)[0]
    same = {s: [i for i in idx if zi[s, i] == ints[s, i]] for s, idx in pos.items()}
    assert sum(len(v) for v in same.values()) >= 4
    z2 = _mutate(x, same, lambda v: np.nextafter(v, dtype(np.inf)))
    assert (_compare(fa, torch, comp, st, nb, z2, off, gain) == -1).all()


def test_compare_corrupt_verbatim_sample(fa, torch):
    """full_range_i32 data are VERBATIM frames: a flipped bit inside sample i's bytes changes sample i and nothing else."""
    shape = (6, 20_000)
    x = full_range_i32(shape)
    comp, st, nb = fa.encode_flac_device(torch.from_numpy(x).cuda(), level=5)
    blob = comp.cpu().numpy().copy()
    starts, nbytes = st.cpu().numpy(), nb.cpu().numpy()
    s, i = 4, 5000  # frame 1, sample 904 of the frame
    seg = blob[starts[s] : starts[s] + nbytes[s]]
    at = _frame_offsets(seg)[1]
    sub = at + _header_bytes(seg, at)
    assert seg[sub] == 0x02  # VERBATIM subframe, no wasted bits, 32-bit samples from the next byte on
    blob[starts[s] + sub + 1 + 4 * (i - 4096) + 2] ^= 0x10
    got = _compare(fa, torch, torch.from_numpy(blob).cuda(), st, nb, x)
    e = np.full(shape[0], -1)
    e[s] = i
    assert np.array_equal(got, e)


def test_compare_damaged_frame_header(fa, torch):
    shape = (6, 20_000)
    x = sinusoid_noise_i32(*shape, seed=11)
    comp, st, nb = fa.encode_flac_device(torch.from_numpy(x).cuda(), level=5)
    blob = comp.cpu().numpy().copy()
    starts, nbytes = st.cpu().numpy(), nb.cpu().numpy()
    s = 2
    at = _frame_offsets(blob[starts[s] : starts[s] + nbytes[s]])[2]
    blob[starts[s] + at + 3] ^= 0x10  # frame 2's channel assignment (its CRC-8 no longer matches)
    got = _compare(fa, torch, torch.from_numpy(blob).cuda(), st, nb, x)
    assert 0 <= got[s] <= 2 * 4096
    assert (np.delete(got, s) == -1).all()


def test_compare_int64_damaged_frames(fa, torch):
    """Two-channel streams: a damaged frame header (the frame is rejected before it is decoded) and a flipped bit inside a
    frame's residuals, each in a stream of its own; the other streams still compare clean."""
    shape = (6, 20_000)
    x = sinusoid_noise_i32(*shape, seed=19).astype(np.int64) * 3_000_001 + 12345
    comp, st, nb = fa.encode_flac_device(torch.from_numpy(x).cuda(), level=5)
    blob = comp.cpu().numpy().copy()
    starts, nbytes = st.cpu().numpy(), nb.cpu().numpy()
    fo2 = _frame_offsets(blob[starts[2] : starts[2] + nbytes[2]])
    blob[starts[2] + fo2[2] + 3] ^= 0x10  # frame 2's channel assignment (its CRC-8 no longer matches)
    fo4 = _frame_offsets(blob[starts[4] : starts[4] + nbytes[4]])
    blob[starts[4] + (fo4[1] + fo4[2]) // 2] ^= 0x08  # inside frame 1
    got = _compare(fa, torch, torch.from_numpy(blob).cuda(), st, nb, x)
    assert 0 <= got[2] <= 2 * 4096
    assert 4096 <= got[4] < 2 * 4096
    assert (np.delete(got, [2, 4]) == -1).all()


@pytest.mark.parametrize("dtype", [np.int32, np.int64])
def test_compare_truncated_last_stream(fa, torch, dtype):
    """The last stream loses its tail inside a run of zero residuals (the data end in zeros): the decoder runs out of bits
    and rejects the frame, whose remaining samples would otherwise decode to the very zeros the input holds."""
    n = 20_000
    x = sinusoid_noise_i32(4, n, seed=21).astype(dtype)
    if dtype == np.int64:
        x = x * 3_000_001 + 12345
    x[3, 16_384 + 100 :] = 0
    comp, st, nb = fa.encode_flac_device(torch.from_numpy(x).cuda(), level=5)
    cut = 20  # the stream's last 20 bytes are gone; what the decoder reads past the end is zeros
    blob = comp.cpu().numpy().copy()
    blob[-cut:] = 0
    nb2 = nb.clone()
    nb2[3] -= cut
    got = _compare(fa, torch, torch.from_numpy(blob).cuda(), st, nb2, x)
    assert 0 <= got[3] <= 16_384
    assert (got[:3] == -1).all()


def _same(a, b):
    for u, v in zip(a, b):
        if u is None or v is None:
            assert u is None and v is None
            continue
        u = u.cpu().numpy() if hasattr(u, "cpu") else np.asarray(u)
        v = v.cpu().numpy() if hasattr(v, "cpu") else np.asarray(v)
        assert u.dtype == v.dtype and np.array_equal(u.view(np.uint8), v.view(np.uint8))


@pytest.mark.parametrize("shape", [(64, 300_000), (12, 1000)])
def test_device_encode_verify_same_result(fa, torch, shape):
    x = sinusoid_noise_i32(*shape, seed=5)
    t = torch.from_numpy(x).cuda()
    _same(fa.encode_flac_device(t, level=5, verify=True), fa.encode_flac_device(t, level=5))
    t64 = torch.from_numpy(x.astype(np.int64) << 20).cuda()
    _same(fa.encode_flac_device(t64, level=5, verify=True), fa.encode_flac_device(t64, level=5))
    xf, q = _float_case(np.float32, shape)
    tf, tq = torch.from_numpy(xf).cuda(), torch.from_numpy(q).cuda()
    _same(fa.encode_flac_device_f32(tf, tq, level=5, verify=True), fa.encode_flac_device_f32(tf, tq, level=5))
    xd, qd = _float_case(np.float64, shape)
    td, tqd = torch.from_numpy(xd).cuda(), torch.from_numpy(qd).cuda()
    _same(fa.encode_flac_device_f64(td, tqd, level=5, verify=True), fa.encode_flac_device_f64(td, tqd, level=5))


@pytest.mark.parametrize("dtype", ["int32", "int64", "float32", "float64"])
def test_array_compress_verify_same_result(fa, torch, dtype, monkeypatch):
    monkeypatch.setenv("FLACARRAY_HIP_HOST_CHUNK_BYTES", str(1 << 20))  # several chunks through the pipeline
    x = sinusoid_noise_i32(16, 70_000, seed=9)
    if dtype == "int64":
        x = x.astype(np.int64) * 5_000_011
    elif dtype.startswith("float"):
        x = sinusoid_noise_f32(16, 70_000, seed=9).astype(dtype)
    kw = {} if dtype.startswith("int") else {"quanta": 1e-3}
    _same(fa.array_compress(x, level=5, verify=True, **kw), fa.array_compress(x, level=5, verify=False, **kw))
    # the process default
    assert fa.set_encode_verify(True) is False
    try:
        _same(fa.array_compress(x, level=5, **kw), fa.array_compress(x, level=5, verify=False, **kw))
    finally:
        fa.set_encode_verify(False)


def test_flacarray_verify_and_first_mismatch(fa, torch):
    x = sinusoid_noise_i32(8, 50_000, seed=13).reshape(2, 4, 50_000)
    a = fa.FlacArray.from_array(x, level=5, verify=True)
    assert a == fa.FlacArray.from_array(x, level=5)
    b = fa.FlacArray.from_device_array(torch.from_numpy(x).cuda(), level=5, verify=True)
    assert b == a
    y = x.copy()
    y[1, 2, 30_000] += 1
    y[0, 0, 0] -= 1
    e = np.full((2, 4), -1)
    e[1, 2], e[0, 0] = 30_000, 0
    assert a.first_mismatch(x).tolist() == np.full((2, 4), -1).tolist()
    assert np.array_equal(a.first_mismatch(y), e)  # not resident, numpy argument
    assert np.array_equal(a.first_mismatch(torch.from_numpy(y).cuda()), e)  # tensor argument
    assert np.array_equal(b.first_mismatch(y), e)  # resident
    a.to_device()
    assert np.array_equal(a.first_mismatch(torch.from_numpy(y)), e)
    a.release_device()


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_flacarray_first_mismatch_float(fa, torch, dtype):
    x = sinusoid_noise_f32(4, 30_000, seed=17).astype(dtype)
    a = fa.FlacArray.from_array(x, level=5, quanta=1e-3, verify=True)
    assert (a.first_mismatch(x) == -1).all()
    y = x.copy()
    y[3, 29_999] += dtype(0.01)
    assert a.first_mismatch(y).tolist() == [-1, -1, -1, 29_999]
    a.to_device()
    assert a.first_mismatch(torch.from_numpy(y).cuda()).tolist() == [-1, -1, -1, 29_999]
