"""GPU tests of FlacArray.concatenate / extend / join_flac_device: the joined store is byte for byte from_array of the
concatenated array (compressed, stream_starts, stream_nbytes compared whole), over the corpus whose preconditions
tests/test_join_model.py asserts on the CPU (every payload misalignment, payloads under 16 bytes, VERBATIM frames,
headers that grow by 0, 1 and 2 bytes); decoded values are checked under both decoder dispatches where a decode or an
encode runs, as tests/test_gpu_window.py does."""
import ctypes

import numpy as np
import pytest
import torch

import flacarray_amd as fa
from flacarray_amd import _lib
from tests import join_model as J
from tests import reindex_model as R
from tests import window_model as W
from tests.conftest import sinusoid_noise_f32, sinusoid_noise_i32, strip_seektable

pytestmark = pytest.mark.gpu

FA_ERROR_ALLOC, FA_ERROR_ZERO_STREAMSIZE, FA_ERROR_ENCODE_INIT = 1 << 0, 1 << 3, 1 << 8
FA_ERROR_DECODE_INIT, FA_ERROR_DECODE_SAMPLE_RANGE, FA_ERROR_DECODE_SEEK = 1 << 13, 1 << 17, 1 << 18


@pytest.fixture(params=["auto", "k7"])
def decoder_dispatch(request, monkeypatch):
    """As in test_gpu_parity.py: the library's own dispatch, and K7 + K3F for every array of their geometry."""
    if request.param == "k7":
        monkeypatch.setenv("FLACARRAY_HIP_LATENCY", "0")
        monkeypatch.setenv("FLACARRAY_HIP_PLACED_BELOW", "0")
    else:
        monkeypatch.delenv("FLACARRAY_HIP_LATENCY", raising=False)
        monkeypatch.delenv("FLACARRAY_HIP_PLACED_BELOW", raising=False)
    return request.param


def _same_store(arr, want):
    assert arr.shape == want.shape and arr.dtype == want.dtype
    assert np.array_equal(np.asarray(arr.stream_nbytes), np.asarray(want.stream_nbytes))
    assert np.array_equal(np.asarray(arr.stream_starts), np.asarray(want.stream_starts))
    assert np.array_equal(np.asarray(arr.compressed), np.asarray(want.compressed))


def _snapshot(arr):
    return np.array(arr.compressed, copy=True), np.array(arr.stream_starts, copy=True), arr.shape


def _unchanged(arr, before):
    assert np.array_equal(arr.compressed, before[0]) and np.array_equal(arr.stream_starts, before[1]) and arr.shape == before[2]


def _parts(x, cuts, level, resident):
    """from_array of every piece; resident: "all", "none", or "mixed" (every other part, the first one resident)."""
    out = []
    for i, p in enumerate(J.pieces(x, cuts)):
        arr = fa.FlacArray.from_array(p, level=level)
        if resident == "all" or (resident == "mixed" and i % 2 == 0):
            arr.to_device()
        out.append(arr)
    return out


# ------------------------------------------------------------------------------------------------------ whole corpus
@pytest.mark.parametrize("kind", ["int32", "int64"])
@pytest.mark.parametrize("level", J.LEVELS)
def test_aligned_corpus(level, kind):
    """No sample decoded, nothing encoded: parts of B, 4 B and 5 B samples, a last part that is only the 7-sample tail,
    three and six parts; a constant row (13-byte frames) beside a full-scale one (VERBATIM frames)."""
    x = W.edge_rows(level, kind == "int64")
    want = fa.FlacArray.from_array(x, level=level)
    for i, cuts in enumerate(J.aligned_cuts(level)):
        parts = _parts(x, cuts, level, ("all", "none", "mixed")[i % 3])
        before = [_snapshot(p) for p in parts]
        out = fa.FlacArray.concatenate(parts, level=level, verify=True)
        _same_store(out, want)
        assert out.is_resident == parts[0].is_resident and not out.md5.any(), cuts
        assert np.array_equal(out.to_array(), x), cuts
        for p, b in zip(parts, before):
            _unchanged(p, b)


@pytest.mark.parametrize("kind", ["int32", "int64"])
@pytest.mark.parametrize("level", J.LEVELS)
def test_unaligned_corpus(decoder_dispatch, level, kind):
    """A part, other than the last, that ends inside a frame: the parts behind it are decoded and appended."""
    x = W.edge_rows(level, kind == "int64")
    want = fa.FlacArray.from_array(x, level=level)
    for i, cuts in enumerate(J.unaligned_cuts(level)):
        parts = _parts(x, cuts, level, ("mixed", "all", "none")[i % 3])
        before = [_snapshot(p) for p in parts]
        out = fa.FlacArray.concatenate(parts, level=level, verify=True)
        _same_store(out, want)
        assert out.is_resident == parts[0].is_resident, cuts
        assert np.array_equal(out.to_array(), x), cuts
        for p, b in zip(parts, before):
            _unchanged(p, b)


def test_unaligned_row_chunks():
    """max_temp_bytes of two rows over five rows: chunks of 2, 2 and 1 rows, each appended to its rows of the prefix."""
    level, B = 1, 1152
    x = torch.from_numpy(sinusoid_noise_i32(5, 4 * B + 11, seed=4)).cuda()
    want = fa.encode_flac_device(x, level=level, compact=True)
    cuts = (B, 2 * B + 3, 3 * B)
    bounds = (0,) + cuts + (x.shape[1],)
    stores = [fa.encode_flac_device(x[:, a:b].contiguous(), level=level, compact=True) + (b - a,) for a, b in zip(bounds, bounds[1:])]
    n_rest = x.shape[1] - cuts[1]
    for cap in (2 * n_rest * 4, 2 * n_rest * 4 + 3, 1, None):
        got = fa.join_flac_device(stores, level=level, verify=True, max_temp_bytes=cap)
        for g, w in zip(got, want):
            assert torch.equal(g, w), cap


# ------------------------------------------------------------------------------------------------------ inverse of window
@pytest.mark.parametrize("level", J.LEVELS)
def test_inverse_of_window(level):
    B = W.block_size(level)
    x = W.edge_rows(level)
    arr = fa.FlacArray.from_array(x, level=level).to_device()
    for c in (B, 2 * B, 4 * B, 5 * B):
        out = fa.FlacArray.concatenate([arr.window(0, c, level=level), arr.window(c, None, level=level)], level=level, verify=True)
        _same_store(out, arr)
    three = [arr.window(0, 2 * B, level=level), arr.window(2 * B, 3 * B, level=level), arr.window(3 * B, None, level=level)]
    _same_store(fa.FlacArray.concatenate(three, level=level, verify=True), arr)


# ------------------------------------------------------------------------------------------------------ number field
@pytest.fixture(scope="module")
def number_store():
    x = W.number_rows()
    return x, fa.FlacArray.from_array(x, level=W.NUMBER_LEVEL).to_device()


@pytest.mark.parametrize("cuts", J.NUMBER_CUTS, ids=lambda c: "-".join(str(v // J.NUMBER_B) for v in c))
def test_number_field(number_store, cuts):
    """Parts on bases on both sides of 128 and 2048, and parts whose own frames cross a threshold while being raised:
    headers grow by 0, 1 and 2 bytes.  The parts are cut out with window (tests/test_gpu_window.py pins those bytes)."""
    x, arr = number_store
    bounds = (0,) + tuple(cuts) + (x.shape[1],)
    parts = [arr.window(a, b, level=W.NUMBER_LEVEL) for a, b in zip(bounds, bounds[1:])]
    out = fa.FlacArray.concatenate(parts, level=W.NUMBER_LEVEL, verify=True)
    _same_store(out, arr)


# ------------------------------------------------------------------------------------------------------ extend
@pytest.mark.parametrize("resident", [True, False], ids=["resident", "host"])
def test_extend(decoder_dispatch, resident):
    level, B = 5, 4096
    cur = sinusoid_noise_i32(3, 2 * B, seed=30)
    arr = fa.FlacArray.from_array(cur, level=level)
    if resident:
        arr.to_device()
    kept = fa.FlacArray(arr)  # a copy made before keeps the old store
    before = _snapshot(kept)
    assert np.array_equal(arr[:, 3:40], cur[:, 3:40])  # (builds the decode index that extend has to close)
    more = sinusoid_noise_i32(3, B + 70, seed=31)
    other = fa.FlacArray.from_array(more, level=level)
    keep_other = _snapshot(other)
    assert arr.extend(other, level=level, verify=True) is arr and arr.is_resident == resident
    cur = np.concatenate([cur, more], axis=1)
    _same_store(arr, fa.FlacArray.from_array(cur, level=level))
    assert np.array_equal(arr[:, B - 5 : 3 * B + 9], cur[:, B - 5 : 3 * B + 9])
    _unchanged(other, keep_other)
    # from_array -> extend -> trim -> append -> overwrite -> extend
    arr.trim(B, level=level, verify=True)
    cur = cur[:, B:]
    chunk = sinusoid_noise_i32(3, 1000, seed=32)
    arr.append(chunk, level=level, verify=True)
    cur = np.concatenate([cur, chunk], axis=1)
    patch = sinusoid_noise_i32(2, 700, seed=33)
    arr.overwrite(B - 100, patch, streams=[2, 0], level=level, verify=True)
    cur[[2, 0], B - 100 : B + 600] = patch
    last = sinusoid_noise_i32(3, 2 * B + 1, seed=34)
    arr.extend(fa.FlacArray.from_array(last, level=level).to_device(), level=level, verify=True)  # (an unaligned join)
    cur = np.concatenate([cur, last], axis=1)
    _same_store(arr, fa.FlacArray.from_array(cur, level=level))
    assert arr.is_resident == resident and np.array_equal(arr.to_array(), cur) and not arr.frame_status().any()
    if resident:
        assert arr._resident["compressed"].untyped_storage().nbytes() == arr.compressed.size  # an exact-size blob
    _unchanged(kept, before)
    one = fa.FlacArray.from_array(cur[0, :B], level=level)  # a 1-D array stays 1-D
    one.extend(fa.FlacArray.from_array(cur[0, B:], level=level), level=level, verify=True)
    assert one.shape == (cur.shape[1],)
    _same_store(one, fa.FlacArray.from_array(cur[0], level=level))


# ------------------------------------------------------------------------------------------------------ float stores
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_float_stores(decoder_dispatch, dtype):
    level, B = 5, 4096
    x = sinusoid_noise_f32(4, 3 * B + 77, seed=9).astype(dtype)
    arr = fa.FlacArray.from_array(x, level=level, quanta=np.array([1e-3, 2e-3, 5e-4, 1e-2], dtype=dtype)).to_device()
    full = arr.to_array()
    for cuts in ((B,), (B, 2 * B), (B + 5,)):
        bounds = (0,) + cuts + (x.shape[1],)
        parts = [arr.window(a, b, level=level) for a, b in zip(bounds, bounds[1:])]
        out = fa.FlacArray.concatenate(parts, level=level, verify=True)
        _same_store(out, arr)
        got = out.to_array()
        assert got.dtype == dtype and np.array_equal(got.view(np.uint8), full.view(np.uint8))
        assert np.array_equal(out.stream_offsets, arr.stream_offsets) and np.array_equal(out.stream_gains, arr.stream_gains)
    a, b = arr.window(0, B, level=level), fa.FlacArray(arr.window(B, None, level=level))  # (a copy: its gains are its own)
    b._st.gains[2] = np.nextafter(b._st.gains[2], dtype(1))
    with pytest.raises(ValueError, match="quantised differently"):
        fa.FlacArray.concatenate([a, b], level=level)
    with pytest.raises(ValueError, match="quantised differently"):
        a.extend(b, level=level)
    assert a.shape == (4, B)


# ------------------------------------------------------------------------------------------------------ signatures
def test_signatures():
    level, B = 5, 4096
    x = W.edge_rows(level)
    arr = fa.FlacArray.from_array(x, level=level, md5=True)
    assert (arr.check_md5() == 1).all()
    one = fa.FlacArray.concatenate([arr], level=level, verify=True)  # a single part: a verbatim copy, signature included
    _same_store(one, arr)
    assert np.array_equal(one.md5, arr.md5) and (one.check_md5() == 1).all()
    a, b = fa.FlacArray.from_array(x[:, :B], level=level, md5=True), fa.FlacArray.from_array(x[:, B:], level=level, md5=True)
    two = fa.FlacArray.concatenate([a, b], level=level)
    assert not two.md5.any() and (two.check_md5() == -1).all()
    signed = fa.FlacArray.concatenate([a, b], level=level, md5=True)
    assert (signed.check_md5() == 1).all() and np.array_equal(signed.md5, arr.md5)
    assert (fa.FlacArray(a).extend(b, level=level, md5=True).check_md5() == 1).all()
    stack = fa.FlacArray.concatenate([a, a.window(streams=[3, 1], level=level)], axis=0)  # every stream keeps its bytes
    assert stack.shape == (6, B) and (stack.check_md5() == 1).all()
    assert np.array_equal(stack.md5, np.concatenate([a.md5, a.md5[[3, 1]]]))


# ------------------------------------------------------------------------------------------------------ axis 0
@pytest.mark.parametrize("resident", [True, False], ids=["resident", "host"])
def test_axis0(resident):
    level = 5
    x = sinusoid_noise_i32(7, 5000, seed=40)
    cube = sinusoid_noise_i32(12, 4100, seed=41).reshape(4, 3, 4100)
    for full, cuts in ((x, (2, 3)), (cube, (1,))):
        parts = [fa.FlacArray.from_array(np.ascontiguousarray(p), level=level) for p in np.split(full, list(cuts), axis=0)]
        if resident:
            parts[0].to_device()
        out = fa.FlacArray.concatenate(parts, axis=0)
        _same_store(out, fa.FlacArray.from_array(full, level=level))
        assert out.is_resident == resident and np.array_equal(out.to_array(), full)
        key = (slice(1, None),) + (slice(None),) * (full.ndim - 2) + (slice(7, 99),)
        assert np.array_equal(out[key], full[key])
        if resident:
            assert torch.equal(out._resident["compressed"].cpu(), torch.from_numpy(np.asarray(out.compressed)))
            assert torch.equal(out._resident["starts"].cpu(), torch.from_numpy(np.asarray(out.stream_starts).reshape(-1)))
    # float offsets and gains are concatenated; the layouts may differ: a libFLAC-layout part beside one of this library's
    f = sinusoid_noise_f32(5, 4200, seed=42)
    quanta = np.array([1e-3, 2e-3, 5e-4, 1e-2, 3e-3], dtype=np.float32)
    whole = fa.FlacArray.from_array(f, level=level, quanta=quanta)
    a, b = fa.FlacArray.from_array(f[:2], level=level, quanta=quanta[:2]), fa.FlacArray.from_array(f[2:], level=level, quanta=quanta[2:])
    if resident:
        a.to_device()
    out = fa.FlacArray.concatenate([a, b], axis=0)
    _same_store(out, whole)
    assert np.array_equal(out.stream_offsets, whole.stream_offsets) and np.array_equal(out.stream_gains, whole.stream_gains)
    assert np.array_equal(out.to_array().view(np.uint8), whole.to_array().view(np.uint8))
    good = fa.FlacArray.from_array(x[:3], level=level)
    fb, fst, fnb = R.to_foreign(good.compressed, good.stream_starts, good.stream_nbytes)
    foreign = fa.FlacArray(None, shape=(3, 5000), compressed=fb, dtype=x.dtype, stream_starts=fst, stream_nbytes=fnb)
    mixed = fa.FlacArray.concatenate([fa.FlacArray.from_array(x[3:], level=level), foreign], axis=0)
    assert mixed.shape == (7, 5000) and not mixed.has_frame_index
    assert np.array_equal(mixed.compressed, np.concatenate([fa.FlacArray.from_array(x[3:], level=level).compressed, fb]))
    assert np.array_equal(mixed.stream_nbytes, np.concatenate([fa.FlacArray.from_array(x[3:], level=level).stream_nbytes, fnb]))


# ------------------------------------------------------------------------------------------------------ refusals
def test_verify_sees_a_damaged_part_and_extend_leaves_its_target():
    level, B = 5, 4096
    x = W.edge_rows(level)
    a = fa.FlacArray.from_array(x[:, : 2 * B], level=level).to_device()
    good = fa.FlacArray.from_array(x[:, 2 * B :], level=level)
    blob = np.array(good.compressed, copy=True)
    s = int(good.stream_starts[1])
    off1 = int.from_bytes(bytes(blob[s + 46 + 18 + 8 : s + 46 + 18 + 16]), "big")
    blob[s + 46 + 18 * 4 + off1 + 9] ^= 0x10  # a payload byte of frame 1 of stream 1
    bad = fa.FlacArray(None, shape=good.shape, compressed=blob, dtype=x.dtype, stream_starts=good.stream_starts, stream_nbytes=good.stream_nbytes)
    before = _snapshot(a)
    assert np.array_equal(a[:, 3:40], x[:, 3:40])
    with pytest.raises(RuntimeError, match=r"stream 1, frame 3"):
        fa.FlacArray.concatenate([a, bad], level=level, verify=True)
    with pytest.raises(RuntimeError, match="do not check"):
        a.extend(bad, level=level, verify=True)
    _unchanged(a, before)
    assert a.is_resident and np.array_equal(a[:, 7:99], x[:, 7:99])
    prev = fa.set_encode_verify(True)  # verify=None follows set_encode_verify
    try:
        with pytest.raises(RuntimeError, match="do not check"):
            a.extend(bad, level=level)
    finally:
        fa.set_encode_verify(prev)
    assert fa.FlacArray.concatenate([a, bad], level=level, verify=False).shape == x.shape  # (the copy itself does not look)


@pytest.mark.parametrize("damage", ["past_body", "swapped"])
def test_damaged_seek_table_is_refused_by_the_check_kernel(damage):
    """One seek offset past the body, two offsets swapped, in the second part: K15a's error word, before anything is
    read through them."""
    level, B = 5, 4096
    x = W.edge_rows(level)
    a = fa.FlacArray.from_array(x[:, :B], level=level)
    good = fa.FlacArray.from_array(x[:, B:], level=level)
    blob = np.array(good.compressed, copy=True)
    s = int(good.stream_starts[2])
    at = lambda f: slice(s + 46 + 18 * f + 8, s + 46 + 18 * f + 16)  # noqa: E731
    if damage == "past_body":
        blob[at(2)] = np.frombuffer(int(good.stream_nbytes[2]).to_bytes(8, "big"), dtype=np.uint8)
    else:
        p, q = blob[at(2)].copy(), blob[at(3)].copy()
        blob[at(2)], blob[at(3)] = q, p
    bad = fa.FlacArray(None, shape=good.shape, compressed=blob, dtype=x.dtype, stream_starts=good.stream_starts, stream_nbytes=good.stream_nbytes)
    keep = _snapshot(a)
    for parts in ([a, bad], [bad]):
        if len(parts) == 1:  # (a single part is copied as it is: no offset of its table is followed)
            _same_store(fa.FlacArray.concatenate(parts, level=level), bad)
            continue
        with pytest.raises(RuntimeError, match="seek table"):
            fa.FlacArray.concatenate(parts, level=level)
    with pytest.raises(RuntimeError, match="seek table"):
        a.extend(bad, level=level)
    _unchanged(a, keep)


def test_device_layout_test_refuses_foreign_streams():
    level, B = 5, 4096
    x = torch.from_numpy(W.edge_rows(level)).cuda()
    a = fa.encode_flac_device(x[:, :B].contiguous(), level=level, compact=True) + (B,)
    b = fa.encode_flac_device(x[:, B:].contiguous(), level=level, compact=True) + (x.shape[1] - B,)
    fb, fst, fnb = (torch.from_numpy(v).cuda() for v in strip_seektable(*(t.cpu().numpy() for t in b[:3])))
    for stores in ([a, (fb, fst, fnb, b[3])], [(fb, fst, fnb, b[3]), a]):
        with pytest.raises(ValueError, match=r"reindex\(\)"):
            fa.join_flac_device(stores, level=level)
    with pytest.raises(ValueError, match=r"reindex\(\)"):  # (the store is not level 1's, nor a two-channel one, nor of that size)
        fa.join_flac_device([a[:3] + (1152,), b], level=1)
    with pytest.raises(ValueError, match=r"reindex\(\)"):
        fa.join_flac_device([a, b], level=level, is_int64=True)
    with pytest.raises(ValueError, match=r"reindex\(\)"):
        fa.join_flac_device([a[:3] + (2 * B,), b], level=level)


# ------------------------------------------------------------------------------------------------------ fa_join_device
def _raw_join(stores, level, nch=1, n_stream=None, slack=64, short=0, shift=0):
    """fa_join_device through ctypes into a sentinel-filled buffer of capacity + slack bytes.  short: bytes taken off the
    capacity the call is told; shift: bytes the first part's blob is moved off its 16-byte alignment."""
    L = _lib.lib()
    P = len(stores)
    n_stream = stores[0][1].numel() if n_stream is None else n_stream
    i64s, ptrs = ctypes.c_int64 * P, ctypes.c_void_p * P
    sizes = i64s(*[s[3] for s in stores])
    nbytes = i64s(*[s[0].numel() for s in stores])
    ws_bytes = L.fa_join_workspace_bytes(P, n_stream, sizes, nch, level)
    cap = L.fa_join_capacity_bytes(P, nbytes, n_stream, sizes, nch, level)
    ws = torch.empty(max(ws_bytes, 16), dtype=torch.uint8, device="cuda")
    buf = torch.full((max(cap, 0) + slack,), 0xA5, dtype=torch.uint8, device="cuda")
    index = torch.full((2 * max(n_stream, 1),), -7, dtype=torch.int64, device="cuda")
    total = ctypes.c_int64(-1)
    blobs = [s[0] for s in stores]
    if shift:
        moved = torch.empty(blobs[0].numel() + 16, dtype=torch.uint8, device="cuda")
        moved[shift : shift + blobs[0].numel()] = blobs[0]
        blobs[0] = moved[shift : shift + blobs[0].numel()]
    torch.cuda.synchronize()
    rc = L.fa_join_device(P, ptrs(*[b.data_ptr() for b in blobs]), nbytes, ptrs(*[s[1].data_ptr() for s in stores]),
                          ptrs(*[s[2].data_ptr() for s in stores]), sizes, n_stream, nch, level, ws.data_ptr(), ws.numel(), buf.data_ptr(),
                          max(cap, 1) - short, index[:n_stream].data_ptr(), index[n_stream:].data_ptr(), ctypes.byref(total), None)
    torch.cuda.synchronize()
    return rc, total.value, buf, index[:n_stream], index[n_stream : 2 * n_stream], ws_bytes, cap


def test_entry_point_footprint_and_error_codes():
    level, B = 5, 4096
    x = torch.from_numpy(W.edge_rows(level)).cuda()
    size = x.shape[1]
    enc = lambda a, b: fa.encode_flac_device(x[:, a:b].contiguous(), level=level, compact=True) + (b - a,)  # noqa: E731
    want = fa.encode_flac_device(x, level=level, compact=True)
    for cuts in ((B,), (2 * B, 5 * B), (B, 2 * B, 3 * B, 4 * B, 5 * B)):
        bounds = (0,) + cuts + (size,)
        stores = [enc(a, b) for a, b in zip(bounds, bounds[1:])]
        rc, total, buf, starts, nbytes, ws_bytes, cap = _raw_join(stores, level)
        assert rc == 0 and ws_bytes > 0 and 0 < total <= cap
        assert total == int(nbytes.sum()) and torch.equal(starts, torch.cumsum(nbytes, 0) - nbytes)
        assert bool((buf[total:] == 0xA5).all())
        assert torch.equal(buf[:total], want[0]) and torch.equal(nbytes, want[2].reshape(-1))
        # the capacity is a bound, not the size: a buffer one byte short of the result is refused, and nothing is written
        rc, total2, buf, _, _, _, _ = _raw_join(stores, level, short=cap - total + 1)
        assert rc == FA_ERROR_ALLOC and total2 == 0 and bool((buf == 0xA5).all())
    # a single part: every stream verbatim
    rc, total, buf, _, nbytes, _, _ = _raw_join([enc(0, size)], level)
    assert rc == 0 and torch.equal(buf[:total], want[0]) and bool((buf[total:] == 0xA5).all())
    a, b, short_a = enc(0, B), enc(B, size), enc(0, B + 1)
    tail = enc(B + 1, size)
    hurt = b[0].clone()  # two seek offsets of stream 2 swapped
    s = int(b[1][2])
    at = lambda f: slice(s + 46 + 18 * f + 8, s + 46 + 18 * f + 16)  # noqa: E731
    p2, p3 = hurt[at(2)].clone(), hurt[at(3)].clone()
    hurt[at(2)], hurt[at(3)] = p3, p2
    refusals = (
        ([a, (hurt,) + b[1:]], {}, FA_ERROR_DECODE_SEEK),
        ([short_a, tail], {}, FA_ERROR_DECODE_SAMPLE_RANGE),  # the unaligned route is the caller's
        ([a[:3] + (1 << 36,), b], {}, FA_ERROR_DECODE_SAMPLE_RANGE),  # (refused on the sizes alone)
        ([a, b[:3] + (0,)], {}, FA_ERROR_ZERO_STREAMSIZE),
        ([a, b], {"shift": 4}, FA_ERROR_ENCODE_INIT),
        ([a, b], {"nch": 2}, FA_ERROR_DECODE_INIT),
        ([a, b[:3] + (b[3] + 1,)], {}, FA_ERROR_DECODE_INIT),  # not the size the streams were written for
        ([b, a], {}, FA_ERROR_DECODE_SAMPLE_RANGE),
    )
    for stores, kw, code in refusals:
        rc, total, buf, _, _, _, _ = _raw_join(stores, level, **kw)
        assert rc == code and total == 0 and bool((buf == 0xA5).all()), (code, kw)
    L = _lib.lib()
    assert L.fa_join_workspace_bytes((1 << 16) + 1, 4, (ctypes.c_int64 * ((1 << 16) + 1))(*([B] * ((1 << 16) + 1))), 1, level) == -1
