"""GPU tests of FlacArray.window / trim / window_flac_device: the windowed store is byte for byte from_array of the slice
(compressed, stream_starts, stream_nbytes compared whole), over the corpus whose preconditions tests/test_window_model.py
asserts on the CPU (every payload misalignment, payloads under 16 bytes, VERBATIM frames, headers that shrink by 0, 1
and 2 bytes); decoded values are checked under both decoder dispatches, as tests/test_gpu_parity.py does."""
import ctypes

import numpy as np
import pytest
import torch

import flacarray_amd as fa
from flacarray_amd import _lib
from tests import reindex_model as R
from tests import window_model as W
from tests.conftest import sinusoid_noise_f32, sinusoid_noise_i32

pytestmark = pytest.mark.gpu

FA_ERROR_ZERO_NSTREAM, FA_ERROR_DECODE_INIT, FA_ERROR_DECODE_SAMPLE_RANGE, FA_ERROR_DECODE_SEEK = 1 << 2, 1 << 13, 1 << 17, 1 << 18


@pytest.fixture(params=["auto", "k7"])
def decoder_dispatch(request, monkeypatch):
    """As in test_gpu_parity.py: the library's own dispatch, and K7 + K3F for every array of their geometry -- so the
    tail decode, the tail encode and the read-back take both kernel families."""
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


def _unchanged(arr, before):
    assert np.array_equal(arr.compressed, before[0]) and np.array_equal(arr.stream_starts, before[1]) and arr.shape == before[2]


def _snapshot(arr):
    return np.array(arr.compressed, copy=True), np.array(arr.stream_starts, copy=True), arr.shape


# ------------------------------------------------------------------------------------------------------ edges
@pytest.mark.parametrize("kind", ["int32", "int64"])
@pytest.mark.parametrize("level", [1, 5])
def test_edges(decoder_dispatch, level, kind):
    """One-sample windows, a window that is only the old short tail, truncate-only, drop-front-only, cuts one sample
    around a frame boundary; a constant row (13-byte frames) beside a full-scale one (VERBATIM frames)."""
    x = W.edge_rows(level, kind == "int64")
    arr = fa.FlacArray.from_array(x, level=level).to_device()
    before = _snapshot(arr)
    for first, last in W.edge_windows(level):
        out = arr.window(first, last, level=level, verify=True)
        _same_store(out, fa.FlacArray.from_array(x[:, first:last], level=level))
        assert out.is_resident and np.array_equal(out.to_array(), x[:, first:last]), (first, last)
    _unchanged(arr, before)
    # the same from a host store, in place
    B = W.block_size(level)
    host = fa.FlacArray.from_array(x, level=level)
    assert host.trim(B, 4 * B + 1, level=level, verify=True) is host and not host.is_resident
    _same_store(host, fa.FlacArray.from_array(x[:, B : 4 * B + 1], level=level))


# ------------------------------------------------------------------------------------------------------ number field
@pytest.fixture(scope="module")
def number_store():
    x = W.number_rows()
    return x, fa.FlacArray.from_array(x, level=W.NUMBER_LEVEL).to_device()


@pytest.mark.parametrize("f0", W.NUMBER_F0)
def test_number_field(number_store, f0):
    """Frame numbers of 1, 2 and 3 UTF-8 bytes renumbered downwards across 128 and 2048: headers shrink by 0, 1 and 2."""
    x, arr = number_store
    for first, last in W.number_windows(f0):
        out = arr.window(first, last, level=W.NUMBER_LEVEL, verify=True)
        _same_store(out, fa.FlacArray.from_array(x[:, first:last], level=W.NUMBER_LEVEL))


# ------------------------------------------------------------------------------------------------------ streams
def test_stream_selection(decoder_dispatch):
    level, B = 5, 4096
    x = W.edge_rows(level)
    arr = fa.FlacArray.from_array(x, level=level).to_device()
    for idx in W.STREAM_PICKS:  # a subset, a permutation, the reversed order
        out = arr.window(B, 3 * B + 5, streams=idx, level=level, verify=True)
        _same_store(out, fa.FlacArray.from_array(x[idx, B : 3 * B + 5], level=level))
        assert np.array_equal(out.to_array(), x[idx, B : 3 * B + 5])
        out = arr.window(0, 2 * B, streams=np.asarray(idx), level=level, verify=True)  # truncate only
        _same_store(out, fa.FlacArray.from_array(x[idx, : 2 * B], level=level))
    with pytest.raises(ValueError, match="twice"):
        arr.window(streams=[1, 1])
    with pytest.raises(ValueError, match="outside"):
        arr.window(streams=[0, 4])
    none = arr.window(B, 2 * B, streams=[])
    assert none.shape == (0, B) and none.compressed.size == 0
    dev = arr._resident
    e = fa.window_flac_device(dev["compressed"], dev["starts"], dev["nbytes"], x.shape[1], B, 2 * B, streams=np.zeros(0, np.int64))
    assert e[0].numel() == 0 and tuple(e[1].shape) == (0,) and tuple(e[2].shape) == (0,)


def test_whole_range_selection_keeps_signatures():
    level = 5
    x = W.edge_rows(level)
    arr = fa.FlacArray.from_array(x, level=level, md5=True)
    assert (arr.check_md5() == 1).all()
    for idx in W.STREAM_PICKS:
        out = arr.window(streams=idx, level=level, verify=True)
        assert out.shape == (len(idx), x.shape[1]) and out.has_frame_index
        for j, s in enumerate(idx):
            got = out.compressed[out.stream_starts[j] : out.stream_starts[j] + out.stream_nbytes[j]]
            assert np.array_equal(got, arr.compressed[arr.stream_starts[s] : arr.stream_starts[s] + arr.stream_nbytes[s]])
        assert (out.check_md5() == 1).all()
    # any other window comes out unsigned; md5=True signs it
    cut = arr.window(0, 4096, level=level)
    assert not cut.md5.any() and (cut.check_md5() == -1).all()
    assert (arr.window(4096, 3 * 4096 + 9, level=level, md5=True).check_md5() == 1).all()


# ------------------------------------------------------------------------------------------------------ unaligned
@pytest.mark.parametrize("kind", ["int32", "int64"])
def test_unaligned(decoder_dispatch, kind):
    level, B = 5, 4096
    x = W.edge_rows(level, kind == "int64")
    arr = fa.FlacArray.from_array(x, level=level).to_device()
    for first in (1, B - 1, B + 1):
        for last in (first + 1, 3 * B + 5, x.shape[1]):
            out = arr.window(first, last, level=level, verify=True)
            _same_store(out, fa.FlacArray.from_array(x[:, first:last], level=level))


def test_unaligned_row_chunks():
    """max_temp_bytes of two rows over five rows: chunks of 2, 2 and 1 rows, put back to back."""
    level, B = 1, 1152
    x = torch.from_numpy(sinusoid_noise_i32(5, 3 * B + 11, seed=4)).cuda()
    comp, st, nb = fa.encode_flac_device(x, level=level)
    first, last = B + 1, 3 * B + 2
    n = last - first
    want = fa.encode_flac_device(x[:, first:last].contiguous(), level=level, compact=True)
    for cap, idx in ((2 * n * 4, None), (2 * n * 4 + 3, [4, 0, 3, 1, 2]), (1, [1, 3]), (None, None)):
        got = fa.window_flac_device(comp, st, nb, x.shape[1], first, last, streams=idx, level=level, verify=True, max_temp_bytes=cap)
        if idx is not None:
            want_i = fa.encode_flac_device(x[idx, first:last].contiguous(), level=level, compact=True)
        else:
            want_i = want
        for g, w in zip(got, want_i):
            assert torch.equal(g, w)


# ------------------------------------------------------------------------------------------------------ float stores
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_float_stores(decoder_dispatch, dtype):
    level, B = 5, 4096
    wide = dtype == np.float64
    x = sinusoid_noise_f32(4, 3 * B + 77, seed=9).astype(dtype)
    arr = fa.FlacArray.from_array(x, level=level, quanta=np.array([1e-3, 2e-3, 5e-4, 1e-2], dtype=dtype)).to_device()
    full = arr.to_array()
    dev = arr._resident
    ints = fa.decode_flac_device(dev["compressed"], dev["starts"], dev["nbytes"], x.shape[1], is_int64=wide)
    for first, last, idx in ((B, 2 * B + 100, None), (0, B + 1, [3, 1]), (B, x.shape[1], [2, 0, 1]), (5, 2 * B, [1, 2]), (0, x.shape[1], [3, 0])):
        rows = slice(None) if idx is None else idx
        out = arr.window(first, last, streams=idx, level=level, verify=True)
        want = fa.encode_flac_device(ints[rows][:, first:last].contiguous(), level=level, compact=True)
        assert np.array_equal(out.compressed, want[0].cpu().numpy())
        assert np.array_equal(out.stream_starts.reshape(-1), want[1].cpu().numpy().reshape(-1))
        assert np.array_equal(out.stream_nbytes.reshape(-1), want[2].cpu().numpy().reshape(-1))
        got = out.to_array()
        assert got.dtype == dtype and np.array_equal(got.view(np.uint8), np.ascontiguousarray(full[rows, first:last]).view(np.uint8))
        assert np.array_equal(out.stream_offsets, np.asarray(arr.stream_offsets)[rows])
        assert np.array_equal(out.stream_gains, np.asarray(arr.stream_gains)[rows])


# ------------------------------------------------------------------------------------------------------ first-class result
def test_result_is_a_first_class_store(decoder_dispatch):
    level, B = 5, 4096
    x = sinusoid_noise_i32(3, 4 * B + 321, seed=2)
    arr = fa.FlacArray.from_array(x, level=level).to_device()
    arr.trim(B, 3 * B + 50, level=level, verify=True, md5=True)
    cur = x[:, B : 3 * B + 50]
    assert arr.shape == cur.shape and not arr.frame_status().any()
    assert (arr.check_md5() == 1).all()
    more = sinusoid_noise_i32(3, B + 3, seed=3)
    arr.append(more, level=level, verify=True)
    cur = np.concatenate([cur, more], axis=1)
    _same_store(arr, fa.FlacArray.from_array(cur, level=level))
    patch = sinusoid_noise_i32(2, 700, seed=5)
    arr.overwrite(B - 100, patch, streams=[2, 0], level=level, verify=True)
    cur[[2, 0], B - 100 : B + 600] = patch
    _same_store(arr, fa.FlacArray.from_array(cur, level=level))
    assert np.array_equal(arr.to_array(), cur) and not arr.frame_status().any()
    # a window of a window, and a 1-D array stays 1-D
    again = arr.window(B, 2 * B + 9, level=level).window(0, B + 1, streams=[1], level=level, verify=True)
    _same_store(again, fa.FlacArray.from_array(cur[[1], B : 2 * B + 1], level=level))
    one = fa.FlacArray.from_array(x[0], level=level)
    cut = one.window(B, 2 * B + 7, level=level, verify=True)
    assert cut.shape == (B + 7,)
    _same_store(cut, fa.FlacArray.from_array(x[0, B : 2 * B + 7], level=level))
    assert np.array_equal(cut.to_array(), x[0, B : 2 * B + 7])


# ------------------------------------------------------------------------------------------------------ rolling buffer
@pytest.mark.parametrize("resident", [True, False], ids=["resident", "host"])
def test_rolling_buffer(resident):
    level, B = 5, 4096
    cur = sinusoid_noise_i32(3, 2 * B + 100, seed=20)
    arr = fa.FlacArray.from_array(cur, level=level)
    if resident:
        arr.to_device()
    kept = fa.FlacArray(arr)  # a copy made before keeps the old store
    before = _snapshot(kept)
    for k in range(1, 6):
        chunk = sinusoid_noise_i32(3, k * B + 2 * k + 1, seed=20 + k)
        arr.append(chunk, level=level)
        cur = np.concatenate([cur, chunk], axis=1)
        if resident:
            arr[:, 3:40]  # (builds the decode index that trim has to close)
        assert arr.trim(first=k * B, level=level, verify=True) is arr
        cur = cur[:, k * B :]
    _same_store(arr, fa.FlacArray.from_array(cur, level=level))
    assert arr.is_resident == resident
    assert np.array_equal(arr[:, 5 : B + 9], cur[:, 5 : B + 9]) and np.array_equal(arr.to_array(), cur)
    if resident:
        assert arr._resident["compressed"].untyped_storage().nbytes() == arr.compressed.size  # an exact-size blob
    _unchanged(kept, before)


# ------------------------------------------------------------------------------------------------------ footprint
def _raw_window(comp, st, nb, size, idx, first, last, level, nch=1, slack=64):
    """fa_window_device through ctypes into a sentinel-filled buffer of capacity + slack bytes."""
    L = _lib.lib()
    n_stream = st.numel()
    m = n_stream if idx is None else len(idx)
    d_idx = None if idx is None else torch.tensor(idx, dtype=torch.int64, device="cuda")
    sizes = nb.cpu().numpy()  # (summed on the host: the refusal cases pass indices no tensor may be indexed with)
    picked = int(sizes.sum()) if idx is None else int(sum(sizes[i] for i in idx if 0 <= i < n_stream))
    ws_bytes = L.fa_window_workspace_bytes(n_stream, size, m, first, last, nch, level)
    cap = L.fa_window_capacity_bytes(picked, n_stream, size, m, first, last, nch, level)
    ws = torch.empty(max(ws_bytes, 16), dtype=torch.uint8, device="cuda")
    buf = torch.full((max(cap, 0) + slack,), 0xA5, dtype=torch.uint8, device="cuda")
    index = torch.full((2 * max(m, 1),), -7, dtype=torch.int64, device="cuda")
    total = ctypes.c_int64(-1)
    torch.cuda.synchronize()
    rc = L.fa_window_device(comp.data_ptr(), comp.numel(), st.data_ptr(), nb.data_ptr(), n_stream, size, None if d_idx is None else d_idx.data_ptr(),
                            m, first, last, nch, level, ws.data_ptr(), ws.numel(), buf.data_ptr(), max(cap, 1), index[:m].data_ptr(),
                            index[m:].data_ptr(), ctypes.byref(total), None)
    torch.cuda.synchronize()
    return rc, total.value, buf, index[:m], index[m : 2 * m], ws_bytes, cap


def test_footprint():
    level, B = 5, 4096
    x = torch.from_numpy(W.edge_rows(level)).cuda()
    size = x.shape[1]
    comp, st, nb = fa.encode_flac_device(x, level=level, compact=True)
    for idx, first, last in ((None, B, 3 * B + 5), ([2, 0, 3], B, 3 * B + 5), ([3, 1], 0, 2 * B + 9), ([1, 3, 0], 0, size), (None, 4 * B, size),
                             ([0], 5 * B, size)):
        rc, total, buf, starts, nbytes, ws_bytes, cap = _raw_window(comp, st, nb, size, idx, first, last, level)
        assert rc == 0 and ws_bytes >= 0 and 0 < total <= cap
        assert total == int(nbytes.sum())
        assert torch.equal(starts, torch.cumsum(nbytes, 0) - nbytes)
        assert bool((buf[total:] == 0xA5).all())
        rows = slice(None) if idx is None else idx
        want = fa.encode_flac_device(x[rows][:, first:last].contiguous(), level=level, compact=True)
        assert torch.equal(buf[:total], want[0]) and torch.equal(nbytes, want[2].reshape(-1))
    # the refusals of the C entry point write nothing: an unaligned first, an index named twice, an index out of range
    for idx, first, last, code in ((None, 1, B, FA_ERROR_DECODE_SAMPLE_RANGE), ([1, 1], B, 2 * B, FA_ERROR_ZERO_NSTREAM),
                                   ([0, 4], B, 2 * B, FA_ERROR_ZERO_NSTREAM), (None, B, B, FA_ERROR_DECODE_SAMPLE_RANGE)):
        rc, total, buf, _, _, _, _ = _raw_window(comp, st, nb, size, idx, first, last, level)
        assert rc == code and total == 0 and bool((buf == 0xA5).all())
    rc, total, buf, _, _, _, _ = _raw_window(comp, st, nb, size, [], B, 2 * B, level)
    assert rc == 0 and total == 0 and bool((buf == 0xA5).all())


# ------------------------------------------------------------------------------------------------------ refusals
def test_refusals_leave_the_store_unchanged():
    level, B = 5, 4096
    x = W.edge_rows(level)
    arr = fa.FlacArray.from_array(x, level=level).to_device()
    before = _snapshot(arr)
    for call in (arr.window, arr.trim):
        for first, last in ((-1, 10), (0, x.shape[1] + 1), (B, B), (B + 1, B)):
            with pytest.raises(ValueError, match="range"):
                call(first, last)
        with pytest.raises(ValueError, match="levels"):
            call(0, B, level=9)
        with pytest.raises(ValueError, match="block size"):
            call(0, B, level=1)
    dev = arr._resident
    with pytest.raises(ValueError, match="block size"):  # (the device's own layout test: the store is not level 1's)
        fa.window_flac_device(dev["compressed"], dev["starts"], dev["nbytes"], x.shape[1], 0, 1152, level=1)
    with pytest.raises(ValueError, match="block size"):  # (nor a two-channel one)
        fa.window_flac_device(dev["compressed"], dev["starts"], dev["nbytes"], x.shape[1], 0, B, level=level, is_int64=True)
    _unchanged(arr, before)
    assert arr.is_resident and np.array_equal(arr[:, 7:99], x[:, 7:99])
    dist = fa.FlacArray._assemble(x.shape, (8, x.shape[1]), x.dtype, arr.compressed, arr.stream_starts, arr.stream_nbytes, None, None)
    with pytest.raises(NotImplementedError):
        dist.window(0, B)
    with pytest.raises(NotImplementedError):
        dist.trim(0, B)
    # a libFLAC-layout store: on the host copy, and by the device's layout test
    fb, fst, fnb = R.to_foreign(arr.compressed, arr.stream_starts, arr.stream_nbytes)
    foreign = fa.FlacArray(None, shape=x.shape, compressed=fb, dtype=x.dtype, stream_starts=fst, stream_nbytes=fnb)
    keep = _snapshot(foreign)
    for call in (foreign.window, foreign.trim):
        with pytest.raises(ValueError, match=r"reindex\(\)"):
            call(B, 2 * B)
    _unchanged(foreign, keep)
    with pytest.raises(ValueError, match=r"reindex\(\)"):
        fa.window_flac_device(torch.from_numpy(fb).cuda(), torch.from_numpy(fst).cuda(), torch.from_numpy(fnb).cuda(), x.shape[1], B, 2 * B)


@pytest.mark.parametrize("damage", ["past_body", "swapped"])
def test_damaged_seek_table_is_refused_by_the_check_kernel(damage):
    """One seek offset past the body, two offsets swapped: K14a's error word, before anything is read through them."""
    level, B = 5, 4096
    x = W.edge_rows(level)
    good = fa.FlacArray.from_array(x, level=level)
    blob = np.array(good.compressed, copy=True)
    s = int(good.stream_starts[2])
    at = lambda f: slice(s + 46 + 18 * f + 8, s + 46 + 18 * f + 16)  # noqa: E731
    if damage == "past_body":
        blob[at(2)] = np.frombuffer(int(good.stream_nbytes[2]).to_bytes(8, "big"), dtype=np.uint8)
    else:
        a, b = blob[at(2)].copy(), blob[at(3)].copy()
        blob[at(2)], blob[at(3)] = b, a
    bad = fa.FlacArray(None, shape=x.shape, compressed=blob, dtype=x.dtype, stream_starts=good.stream_starts, stream_nbytes=good.stream_nbytes)
    keep = _snapshot(bad)
    with pytest.raises(RuntimeError, match="seek table"):
        bad.window(B, 4 * B + 9, level=level)
    with pytest.raises(RuntimeError, match="seek table"):
        bad.trim(B, 4 * B, level=level)
    _unchanged(bad, keep)
    # the frames a window does not touch are not its business: frame 0 alone is still cut out
    _same_store(bad.window(0, B, streams=[2, 1], level=level), good.window(0, B, streams=[2, 1], level=level))


# ------------------------------------------------------------------------------------------------------ verify
def test_the_verify_check_sees_a_wrong_number():
    """verify=True passes throughout this file; here the check it runs (frame_status_device over the result) is shown to
    see a header byte flipped after the fact: the number field of frame 1 of stream 0."""
    level, B = 5, 4096
    x = torch.from_numpy(W.edge_rows(level)).cuda()
    comp, st, nb = fa.encode_flac_device(x, level=level)
    out = fa.window_flac_device(comp, st, nb, x.shape[1], 2 * B, 5 * B, level=level, verify=True, compact=True)
    n = 3 * B
    assert not fa.frame_status_device(out[0], out[1], out[2], n, block_size=B).any()
    hurt = out[0].clone()
    s0 = int(out[1][0])
    off1 = int.from_bytes(bytes(out[0][s0 + 46 + 18 + 8 : s0 + 46 + 18 + 16].cpu().numpy()), "big")
    hurt[s0 + 46 + 18 * 3 + off1 + 4] ^= 0x02  # frame 1 now says 3
    status = fa.frame_status_device(hurt, out[1], out[2], n, block_size=B).reshape(4, 3)
    assert int(status[0, 1]) & fa.FRAME_HEADER and not status[1:].any() and not status[0, 0] and not status[0, 2]
    prev = fa.set_encode_verify(True)  # verify=None follows set_encode_verify
    try:
        arr = fa.FlacArray.from_array(x.cpu().numpy(), level=level)
        _same_store(arr.window(B, 2 * B + 1, level=level), fa.FlacArray.from_array(x.cpu().numpy()[:, B : 2 * B + 1], level=level))
    finally:
        fa.set_encode_verify(prev)
