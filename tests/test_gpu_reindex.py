"""FlacArray.reindex on the GPU against tests/reindex_model.py (whose preconditions tests/test_reindex_model.py checks on the
CPU): the bytes of every writer batch under both frame-location routes, stores of this library through a libFLAC layout
and back, a damaged source frame, signatures, the footprint of the copy at every source / destination misalignment, the
refusals (nothing written), the stream contract and residency."""
import ctypes

import numpy as np
import pytest

from tests import reindex_model as R
from tests import scrub_model as SM
from tests import stream_tools as T
from tests.golden import flac_writer as W

pytestmark = pytest.mark.gpu

GUARD = 4096  # sentinel bytes on each side of a guarded output
FA_ERROR_ALLOC, FA_ERROR_DECODE_INIT, FA_ERROR_DECODE_STREAMSIZE, FA_ERROR_DECODE_SEEK = 1, 1 << 13, 1 << 16, 1 << 18


@pytest.fixture(scope="module")
def torch():
    import torch

    assert torch.cuda.is_available()
    return torch


@pytest.fixture(scope="module")
def fa():
    import flacarray_amd

    return flacarray_amd


@pytest.fixture(scope="module")
def batches():
    return W.all_batches()


@pytest.fixture(scope="module")
def models():
    """The model's result per batch name, computed once."""
    made = {}

    def get(b):
        if b["name"] not in made:
            blob, st, nb = W.pack(b["streams"])
            made[b["name"]] = R.reindex_store(blob, st, nb, b["n"], b["block"], b["channels"])
        return made[b["name"]]

    yield get
    made.clear()


def _up(torch, a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _same_store(got, want):
    return all(np.array_equal(g.cpu().numpy() if hasattr(g, "cpu") else g, w) for g, w in zip(got, want))


def _small_batch(count=4, n=5 * 64 + 9, block=64, channels=1, seed=77, **kw):
    return W._batch("small", np.random.default_rng(seed), count, n, block, channels, **kw)


# ------------------------------------------------------------------------------------------------------ 1. bytes

@pytest.mark.parametrize("route", ["scan", "serial_walk"])
def test_bytes_equal_the_model(torch, fa, batches, models, monkeypatch, route):
    """Every writer batch: both channel counts, block sizes 16 to 65535, 2100-frame streams, the 65 600-frame stream (its
    seek points shared over several workgroups), all five layouts in one call; frames located by the sync scan, and with
    the scan switched off by the serial walk."""
    monkeypatch.delenv("FLACARRAY_HIP_NO_SYNC_SCAN", raising=False)
    if route == "serial_walk":
        monkeypatch.setenv("FLACARRAY_HIP_NO_SYNC_SCAN", "1")
    failed, layouts = [], set()
    for b in batches:
        d = tuple(_up(torch, a) for a in W.pack(b["streams"]))
        if b["block"] is None:
            with pytest.raises(ValueError, match="differ in block size"):
                fa.reindex_flac_device(*d, b["n"], is_int64=b["channels"] == 2)
            continue
        layouts |= {r["layout"] for r in b["records"]}
        try:
            got = fa.reindex_flac_device(*d, b["n"], is_int64=b["channels"] == 2)
            assert got[0].dtype == torch.uint8 and got[1].dtype == torch.int64 and got[2].dtype == torch.int64
            assert _same_store(got, models(b)), "bytes differ"
        except (AssertionError, RuntimeError) as e:
            failed.append((b["name"], type(e).__name__, str(e).splitlines()[0][:160] if str(e) else ""))
    assert not failed, "%d of %d batches fail: %s" % (len(failed), len(batches), failed)
    assert layouts == set(W.LAYOUTS)
    big = next(b for b in batches if b["name"] == "utf8_4byte")
    assert models(big)[0].size // 65536 > 1 and big["records"][0]["frames"] == 65600  # more than one workgroup for the stream


def test_compact_and_leading_shape(torch, fa):
    b = _small_batch(count=6)
    blob, st, nb = (_up(torch, a) for a in W.pack(b["streams"]))
    want = R.reindex_store(*W.pack(b["streams"]), b["n"], 64, 1)
    got = fa.reindex_flac_device(blob, st.reshape(2, 3), nb.reshape(2, 3), b["n"], compact=True)
    assert tuple(got[1].shape) == (2, 3) and tuple(got[2].shape) == (2, 3)
    assert got[0].untyped_storage().nbytes() == want[0].size  # an exact-size blob
    assert _same_store((got[0], got[1].reshape(-1), got[2].reshape(-1)), want)
    # its own output comes out byte-identical
    again = fa.reindex_flac_device(got[0], got[1], got[2], b["n"])
    assert _same_store((again[0], again[1].reshape(-1), again[2].reshape(-1)), want)


# ------------------------------------------------------------------------------------------------------ 2. own stores

def _foreign_twin(fa, a):
    """`a` with its store rewritten into libFLAC's layout."""
    fb, fst, fnb = R.to_foreign(a.compressed, a.stream_starts, a.stream_nbytes)
    ishape = np.shape(a.stream_starts)
    return fa.FlacArray(None, shape=a.shape, compressed=fb, dtype=a.dtype, stream_starts=fst.reshape(ishape), stream_nbytes=fnb.reshape(ishape),
                        stream_offsets=a.stream_offsets, stream_gains=a.stream_gains)


def _same_array(a, b):
    return (np.array_equal(a.compressed, b.compressed) and np.array_equal(a.stream_starts, b.stream_starts)
            and np.array_equal(a.stream_nbytes, b.stream_nbytes) and a.shape == b.shape and a.dtype == b.dtype)


OWN = {
    "int32 level 5": dict(shape=(3, 2 * 4096 + 100), dtype=np.int32, level=5),
    "int32 level 1": dict(shape=(2, 2, 3 * 1152 + 7), dtype=np.int32, level=1),
    "int64": dict(shape=(2, 2 * 4096 + 33), dtype=np.int64, level=5),
    "float32 quanta": dict(shape=(3, 4096 + 500), dtype=np.float32, level=5),
    "1-D": dict(shape=(2 * 4096 + 1,), dtype=np.int32, level=5),
}


def _data(spec, seed):
    rng = np.random.default_rng(seed)
    shape, dt = spec["shape"], spec["dtype"]
    t = np.arange(shape[-1])
    wave = np.sin(2 * np.pi * t / 700.0) * rng.random(shape[:-1] + (1,)) + rng.normal(0, 0.05, shape)
    if dt == np.float32:
        return wave.astype(np.float32)
    return np.rint(wave * (2.0**40 if dt == np.int64 else 2.0**20)).astype(dt)


@pytest.mark.parametrize("name", list(OWN))
def test_own_stores_come_back_and_can_be_spliced(torch, fa, name):
    """from_array -> libFLAC layout -> reindex() is the original store in every byte; append and overwrite, refused on
    the foreign array, then give the store from_array writes for the patched array.  (The float store: append and
    overwrite quantise with the store's own offsets and gains, so their result is compared with the same calls on the
    store that never left this library's layout -- from_array of patched floats would choose other offsets.)"""
    spec = OWN[name]
    x = _data(spec, seed=len(name))
    kw = dict(level=spec["level"])
    if spec["dtype"] == np.float32:
        kw["quanta"] = 1e-4
    a = fa.FlacArray.from_array(x, **kw)
    f = _foreign_twin(fa, a)
    assert a.has_frame_index and not f.has_frame_index and not _same_array(a, f)
    assert np.array_equal(f.to_array(), a.to_array())
    extra = _data(dict(spec, shape=spec["shape"][:-1] + (777,)), seed=5)
    patch = _data(dict(spec, shape=spec["shape"][:-1] + (300,)), seed=6)
    with pytest.raises(ValueError, match="libFLAC-written streams are not supported"):
        f.append(extra, level=spec["level"])
    with pytest.raises(ValueError, match="libFLAC-written streams are not supported"):
        f.overwrite(50, patch, level=spec["level"])
    assert f.reindex() is f
    assert f.has_frame_index and _same_array(f, a)
    assert (f.stream_offsets is None) == (a.stream_offsets is None)
    if a.stream_offsets is not None:
        assert np.array_equal(f.stream_offsets, a.stream_offsets) and np.array_equal(f.stream_gains, a.stream_gains)
    f.append(extra, level=spec["level"])
    f.overwrite(50, patch, level=spec["level"])
    if spec["dtype"] == np.float32:
        a.append(extra, level=spec["level"])
        a.overwrite(50, patch, level=spec["level"])
        want = a
    else:
        y = np.concatenate([x, extra], axis=-1)
        y[..., 50:350] = patch
        want = fa.FlacArray.from_array(y, **kw)
    assert _same_array(f, want)


# ------------------------------------------------------------------------------------------------------ 3. damage

def test_a_damaged_source_frame_is_caught_or_adopted(torch, fa):
    x = _data(dict(shape=(3, 4 * 1152 + 200), dtype=np.int32), seed=3)
    n, block = x.shape[1], 1152
    a = fa.FlacArray.from_array(x, level=1)
    f = _foreign_twin(fa, a)
    blob = np.array(f.compressed, copy=True)
    offs = R.store_offsets(blob, f.stream_starts, f.stream_nbytes, n, block, 1)
    s_bad, f_bad = 1, 2
    at = int(f.stream_starts[s_bad]) + offs[s_bad][f_bad + 1] - 2  # the CRC-16 of frame (1, 2)
    before = bytes(blob).count(b"\xff\xf8")
    blob[at : at + 2] ^= np.array([0x5A, 0x3C], dtype=np.uint8)
    assert bytes(blob).count(b"\xff\xf8") == before  # no sync candidate made or lost: the same frames are found
    bad = fa.FlacArray(None, shape=x.shape, compressed=blob, dtype=np.int32, stream_starts=f.stream_starts, stream_nbytes=f.stream_nbytes)
    with pytest.raises(RuntimeError, match="stream 1, frame 2, status 4"):
        bad.reindex()
    assert np.array_equal(bad.compressed, blob) and np.array_equal(bad.stream_starts, f.stream_starts) and not bad.has_frame_index
    assert (bad.frame_status() == SM.UNLOCATED).all()
    assert bad.reindex(verify=False) is bad and bad.has_frame_index
    model = R.reindex_store(blob, f.stream_starts, f.stream_nbytes, n, block, 1, offsets=offs)
    assert np.array_equal(bad.compressed, model[0]) and np.array_equal(bad.stream_starts, model[1]) and np.array_equal(bad.stream_nbytes, model[2])
    want_status = SM.frame_status(*model, n, 1, block)
    only = np.zeros((3, 5), dtype=np.uint8)
    only[s_bad, f_bad] = SM.CRC16
    assert np.array_equal(want_status, only)
    assert np.array_equal(bad.frame_status(), want_status)
    out, status = bad.salvage()
    assert np.array_equal(status, want_status)
    assert np.array_equal(out, SM.salvage_model(x, want_status, 0, n, 0, block))
    assert np.array_equal(bad.damaged_ranges(), [[s_bad, f_bad * block, (f_bad + 1) * block]])


# ------------------------------------------------------------------------------------------------------ 4. signatures

@pytest.mark.parametrize("channels", (1, 2))
def test_signatures_survive(torch, fa, channels):
    b = _small_batch(count=5, channels=channels, seed=78 + channels)
    blob, st, nb = W.pack(b["streams"])
    dt = np.int32 if channels == 1 else np.int64
    a = fa.FlacArray(None, shape=(5, b["n"]), compressed=blob, dtype=dt, stream_starts=st, stream_nbytes=nb)
    md5 = a.md5.copy()
    assert md5.any(axis=1).all() and (a.check_md5() == 1).all()
    a.reindex()
    assert np.array_equal(a.md5, md5) and (a.check_md5() == 1).all()
    assert np.array_equal(a.to_array(), b["samples"])


# ------------------------------------------------------------------------------------------------------ the C entry point

class CCall:
    """fa_reindex_device on a source blob at `src_off` bytes past a 256-byte boundary, into a buffer of `fill` bytes whose
    output pointer lies `out_off` bytes past GUARD; everything comes back as numpy."""

    def __init__(self, torch, blob, st, nb, n, nch, cap=None, fill=0xA5, src_off=0, out_off=0, block=None):
        from flacarray_amd import _lib

        L = _lib.lib()
        blob = np.ascontiguousarray(blob, dtype=np.uint8)
        k = len(st)
        src = torch.zeros(blob.size + 32, dtype=torch.uint8, device="cuda")
        if blob.size:
            src[src_off : src_off + blob.size] = _up(torch, blob)
        assert src.data_ptr() % 256 == 0
        d_st, d_nb = _up(torch, np.asarray(st, dtype=np.int64)), _up(torch, np.asarray(nb, dtype=np.int64))
        if cap is None:
            cap = L.fa_reindex_capacity_bytes(blob.size, k, n, block)
            assert cap >= 0
        self.cap = cap
        buf = torch.full((GUARD + out_off + max(cap, 0) + GUARD,), fill, dtype=torch.uint8, device="cuda")
        idx = torch.full((2 * max(k, 1),), -7, dtype=torch.int64, device="cuda")
        total = ctypes.c_int64(-1)
        vp = ctypes.c_void_p
        self.rc = L.fa_reindex_device(vp(src.data_ptr() + src_off), blob.size, vp(d_st.data_ptr()), vp(d_nb.data_ptr()), k, n, nch,
                                      vp(buf.data_ptr() + GUARD + out_off), cap, vp(idx.data_ptr()), vp(idx.data_ptr() + 8 * max(k, 1)),
                                      ctypes.byref(total), vp(torch.cuda.current_stream().cuda_stream))
        torch.cuda.synchronize()
        self.total = total.value
        self.buf = buf.cpu().numpy()
        self.lo = GUARD + out_off
        self.fill = fill
        self.starts, self.nbytes = idx[:k].cpu().numpy(), idx[max(k, 1) : max(k, 1) + k].cpu().numpy()

    def untouched(self, used=0):
        return bool((self.buf[: self.lo] == self.fill).all() and (self.buf[self.lo + used :] == self.fill).all())

    def out(self):
        return self.buf[self.lo : self.lo + self.total]


# ------------------------------------------------------------------------------------------------------ 5. footprint

def _staggered(b):
    """The batch's streams in one blob, the junk in front of each chosen so that (source - destination) mod 16 of the body
    copy is s mod 16 for stream s, for an output that starts on a 16-byte boundary."""
    n, block, nch = b["n"], b["block"], b["channels"]
    nf = -(-n // block)
    parts, st, nb, q = [], [], [], []
    src_at = dst_at = 0
    for s, seg in enumerate(b["streams"]):
        first = R.first_frame(seg)
        junk = (s - (src_at + first - (dst_at + 46 + 18 * nf))) % 16
        parts.append(bytes([0xC3]) * junk + seg)
        st.append(src_at + junk)
        nb.append(len(seg))
        q.append((src_at + junk + first - (dst_at + 46 + 18 * nf)) % 16)
        src_at += junk + len(seg)
        dst_at += 46 + 18 * nf + len(seg) - first
    assert sorted(set(q)) == list(range(16))
    return np.frombuffer(b"".join(parts), dtype=np.uint8), np.array(st, dtype=np.int64), np.array(nb, dtype=np.int64)


@pytest.mark.parametrize("fill", (0xA5, 0x00, 0xFF))
def test_footprint_at_every_misalignment(torch, fill):
    b = _small_batch(count=16, n=3 * 64 + 5, seed=79)
    blob, st, nb = _staggered(b)
    want = R.reindex_store(blob, st, nb, b["n"], 64, 1)
    for src_off in (0, 1, 7, 8):
        for out_off in (0, 3, 13):
            c = CCall(torch, blob, st, nb, b["n"], 1, fill=fill, src_off=src_off, out_off=out_off, block=64)
            assert c.rc == 0 and c.total == want[0].size <= c.cap, (src_off, out_off, c.rc)
            assert c.untouched(c.total), (src_off, out_off)
            assert np.array_equal(c.out(), want[0]) and np.array_equal(c.starts, want[1]) and np.array_equal(c.nbytes, want[2]), (src_off, out_off)


# ------------------------------------------------------------------------------------------------------ 6. refusals

def _own_store():
    b = _small_batch(count=3, layout="own", seed=80)
    return b, W.pack(b["streams"])


def _set_offset(blob, start, k, value):
    out = blob.copy()
    out[start + 46 + 18 * k + 8 : start + 46 + 18 * k + 16] = np.frombuffer(int(value).to_bytes(8, "big"), dtype=np.uint8)
    return out


def test_bad_seek_tables_are_refused(torch, fa):
    b, (blob, st, nb) = _own_store()
    n = b["n"]
    nf = -(-n // 64)
    good = CCall(torch, blob, st, nb, n, 1, block=64)
    assert good.rc == 0 and np.array_equal(good.out(), blob)  # own layout: the identity
    s = 1
    offs = R.own_offsets(bytes(blob[st[s] : st[s] + nb[s]]))
    rel = [o - offs[0] for o in offs]
    cases = {
        "point 2 past the stream end": _set_offset(blob, st[s], 2, int(nb[s]) + 100),
        "point 2 far past the blob": _set_offset(blob, st[s], 2, 1 << 40),
        "point 2 negative": _set_offset(blob, st[s], 2, (1 << 64) - 16),
        "last point inside the last 8 bytes": _set_offset(blob, st[s], nf - 1, int(nb[s]) - (46 + 18 * nf) - 7),
        "first point not the first frame": _set_offset(blob, st[s], 0, 1),
        "points 1 and 2 swapped": _set_offset(_set_offset(blob, st[s], 1, rel[2]), st[s], 2, rel[1]),
        "points 1 and 2 equal": _set_offset(blob, st[s], 2, rel[1]),
    }
    for name, bad in cases.items():
        c = CCall(torch, bad, st, nb, n, 1, block=64)
        assert c.rc == FA_ERROR_DECODE_SEEK and c.untouched(), (name, c.rc)
        with pytest.raises(RuntimeError, match="Reindexing failed, return code = %d" % FA_ERROR_DECODE_SEEK):
            fa.reindex_flac_device(_up(torch, bad), _up(torch, st), _up(torch, nb), n)
    # the first metadata block is not a STREAMINFO of 34 bytes: a PADDING block in front of it
    seg = bytes(blob[st[0] : st[0] + nb[0]])
    moved = seg[:4] + bytes([1, 0, 0, 2, 0, 0]) + seg[4:]
    c = CCall(torch, np.frombuffer(moved, dtype=np.uint8), [0], [len(moved)], n, 1, block=64)
    assert c.rc == FA_ERROR_DECODE_INIT and c.untouched()


@pytest.mark.parametrize("route", ["scan", "serial_walk"])
def test_what_the_decoders_refuse_is_refused(torch, fa, monkeypatch, route):
    """flac_writer.invalid_streams(): one frame each, CRCs intact.  The index step of the decoders rejects the
    variable-blocksize stream on both routes (no fixed-blocksize sync code to find, and the walk does not take the
    header); the walk, which parses subframes, also rejects the reserved subframe type and the partition shorter than
    its predictor order.  Whatever is rejected leaves the output untouched; whatever is indexed equals the model."""
    monkeypatch.delenv("FLACARRAY_HIP_NO_SYNC_SCAN", raising=False)
    if route == "serial_walk":
        monkeypatch.setenv("FLACARRAY_HIP_NO_SYNC_SCAN", "1")
    must = {"variable_blocksize"} | ({"reserved_type", "partition_shorter_than_order"} if route == "serial_walk" else set())
    seen = set()
    for name, data, n in W.invalid_streams():
        blob = np.frombuffer(data, dtype=np.uint8)
        c = CCall(torch, blob, [0], [blob.size], n, 1, block=64)
        if c.rc != 0:
            seen.add(name)
            assert c.untouched(), name
            with pytest.raises(RuntimeError, match="Reindexing failed"):
                fa.reindex_flac_device(_up(torch, blob), _up(torch, np.array([0])), _up(torch, np.array([blob.size])), n)
        else:
            assert n == 64, name  # (one frame: it begins behind the metadata)
            assert bytes(c.out()) == R.reindex_stream(data, [R.first_frame(data)], n, 64), name
    assert must <= seen and "valid" not in seen, seen


def test_wrong_geometry_and_capacity_are_refused(torch, fa):
    b = _small_batch(count=4, seed=81)
    blob, st, nb = W.pack(b["streams"])
    n = b["n"]
    want = R.reindex_store(blob, st, nb, n, 64, 1)
    ok = CCall(torch, blob, st, nb, n, 1, block=64)
    assert ok.rc == 0 and np.array_equal(ok.out(), want[0])
    c = CCall(torch, blob, st, nb, n, 2, block=64)  # the other channel count
    assert c.rc == FA_ERROR_DECODE_INIT and c.untouched()
    with pytest.raises(RuntimeError, match="Reindexing failed"):
        fa.reindex_flac_device(_up(torch, blob), _up(torch, st), _up(torch, nb), n, is_int64=True)
    # another frame count (more: the walk leaves the stream; fewer: the walk finds that many frames, the last of them is
    # not the stream's last), and the same frame count with another last block size
    for wrong, rc in ((n + 2 * 64, None), (n - 2 * 64, FA_ERROR_DECODE_STREAMSIZE), (n + 1, FA_ERROR_DECODE_STREAMSIZE), (n - 1, FA_ERROR_DECODE_STREAMSIZE)):
        c = CCall(torch, blob, st, nb, wrong, 1, block=64)
        assert c.rc != 0 and c.rc == (rc or c.rc) and c.untouched(), (wrong, c.rc)
        with pytest.raises(RuntimeError, match="Reindexing failed"):
            fa.reindex_flac_device(_up(torch, blob), _up(torch, st), _up(torch, nb), wrong)
    c = CCall(torch, blob, st, nb, n, 1, cap=want[0].size - 1)
    assert c.rc == FA_ERROR_ALLOC and c.untouched()
    c = CCall(torch, blob, st, nb, n, 1, cap=want[0].size)
    assert c.rc == 0 and c.untouched(c.total) and np.array_equal(c.out(), want[0])
    # an index that leaves the blob
    c = CCall(torch, blob, st, nb + np.array([0, 0, 0, 1]), n, 1, block=64)
    assert c.rc == FA_ERROR_DECODE_INIT and c.untouched()


def test_zero_streams(torch, fa):
    c = CCall(torch, np.zeros(0, np.uint8), np.zeros(0, np.int64), np.zeros(0, np.int64), 100, 1, cap=64)
    assert c.rc == 0 and c.total == 0 and c.untouched()
    e8, e64 = torch.zeros(0, dtype=torch.uint8, device="cuda"), torch.zeros(0, dtype=torch.int64, device="cuda")
    got = fa.reindex_flac_device(e8, e64, e64, 100)
    assert [t.numel() for t in got] == [0, 0, 0] and got[0].dtype == torch.uint8 and got[1].dtype == torch.int64


# ------------------------------------------------------------------------------------------------------ 7. stream contract

def test_on_a_side_stream_behind_a_producer(torch, fa):
    """The decoy is the same store with one frame's CRC-16 changed: the same parse, other bytes in the result."""
    b = _small_batch(count=4, n=40 * 64 + 9, seed=82)
    blob, st, nb = W.pack(b["streams"])
    decoy = blob.copy()
    decoy[-2:] ^= 0x55
    want = R.reindex_store(blob, st, nb, b["n"], 64, 1)
    d_st, d_nb = _up(torch, st), _up(torch, nb)
    call = lambda src: fa.reindex_flac_device(src, d_st, d_nb, b["n"], verify=False)  # noqa: E731
    side = torch.cuda.Stream()
    got, _ = T.run_delayed("reindex", side, [_up(torch, blob)], [_up(torch, decoy)], call)
    assert all(np.array_equal(g, w) for g, w in zip(got, want))
    # the verified call, whose status pass follows the copy on the same stream
    with torch.cuda.stream(side):
        out = [t.clone() for t in fa.reindex_flac_device(_up(torch, blob), d_st, d_nb, b["n"], verify=True)]
    side.synchronize()
    assert _same_store(out, want)


# ------------------------------------------------------------------------------------------------------ 8. residency

def test_a_resident_array_stays_resident(torch, fa):
    x = _data(dict(shape=(4, 3 * 1152 + 70), dtype=np.int32), seed=9)
    a = fa.FlacArray.from_array(x, level=1)
    f = _foreign_twin(fa, a).to_device()
    streams, first, count = [3, 0, 2], [5, 1152, 2000], [100, 1153, 1]

    def reads():
        r = f.reduce(width=500)
        return f[1:3, 100:2500], f[:], f.read_slices(streams, first, count), (r.min, r.max, r.sum, r.sumsq_hi, r.sumsq_lo)

    before = reads()
    assert f.is_resident and not f.has_frame_index
    assert np.array_equal(before[1], x)
    f.reindex()
    assert f.is_resident and f.has_frame_index and _same_array(f, a)
    res = f._resident
    assert res["index"] is None and res["compressed"].untyped_storage().nbytes() == a.compressed.size
    assert np.array_equal(res["compressed"].cpu().numpy(), a.compressed)
    after = reads()
    assert T.same(T.to_host(list(before)), T.to_host(list(after)))
    assert f._resident["index"] is not None  # rebuilt on use
    assert not f.frame_status().any()
    f.release_device()
