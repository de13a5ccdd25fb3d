"""The damage map and the decode through errors on the GPU, against tests/scrub_model.py: every store, every damage site.
`frame_status_device` equals the model byte for byte; a salvage returns the model's status, every frame of status 0 bit for
bit and the fill everywhere else, whatever range is asked for; what it writes is its output and nothing else; and neither
earlier calls nor the stream it runs on change its result.  FLACARRAY_HIP_LATENCY=0 sends the salvage's decode through the
throughput decoder K7, =1 through the latency decoder K7L."""
import ctypes

import numpy as np
import pytest

from tests import scrub_model as M
from tests import stream_tools as T
from tests import verify_corpus as V

pytestmark = pytest.mark.gpu

GUARD = 4096  # sentinel elements on each side of a guarded output


@pytest.fixture(scope="module")
def torch():
    import torch

    assert torch.cuda.is_available()
    return torch


@pytest.fixture(scope="module")
def fa():
    import flacarray_amd

    return flacarray_amd


@pytest.fixture(params=["k7", "k7l"])
def decoder_dispatch(request, monkeypatch):
    monkeypatch.setenv("FLACARRAY_HIP_LATENCY", "0" if request.param == "k7" else "1")
    return request.param


def _up(torch, a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


class Dev:
    """A store on the device, with what the decoders return for it while it is intact (computed once)."""

    def __init__(self, torch, fa, store):
        self.torch, self.fa, self.store = torch, fa, store
        self.blob, self.st, self.nb = _up(torch, store.blob), _up(torch, store.starts), _up(torch, store.nbytes)
        self.wide = store.channels == 2
        off, gain = V.float_params(store)
        self.off, self.gain = _up(torch, off), _up(torch, gain)
        self.ints = fa.decode_flac_device(self.blob, self.st, self.nb, store.n, is_int64=self.wide).cpu().numpy()
        assert np.array_equal(self.ints, store.data)
        self.floats = fa.decode_flac_device(self.blob, self.st, self.nb, store.n, offsets=self.off, gains=self.gain, is_int64=self.wide).cpu().numpy()

    def case(self, case):
        return _up(self.torch, case.blob), _up(self.torch, case.starts), _up(self.torch, case.nbytes)

    def status(self, triple, block_size="store"):
        b = self.store.block if block_size == "store" else block_size
        return self.fa.frame_status_device(*triple, self.store.n, is_int64=self.wide, block_size=b).cpu().numpy()

    def salvage(self, triple, first=-1, last=-1, floats=False, fill=None, block_size="store"):
        b = self.store.block if block_size == "store" else block_size
        kw = dict(offsets=self.off, gains=self.gain) if floats else {}
        out, status = self.fa.decode_flac_salvage_device(*triple, self.store.n, first, last, is_int64=self.wide, fill=fill, block_size=b, **kw)
        return out.cpu().numpy(), status.cpu().numpy()


@pytest.fixture(scope="module")
def devs(torch, fa, oracle):
    made = {}

    def get(name):
        if name not in made:
            made[name] = Dev(torch, fa, M.build_store(name))
        return made[name]

    yield get
    made.clear()


def _bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


# ------------------------------------------------------------------------------------------------------ the status

@pytest.mark.parametrize("name", M.STORES)
def test_frame_status_equals_the_model(devs, name):
    d = devs(name)
    st = d.store
    intact = d.status((d.blob, d.st, d.nb))
    assert intact.shape == (3, 3) and intact.dtype == np.uint8 and not intact.any()
    assert not d.status((d.blob, d.st, d.nb), block_size=None).any()  # the block size read from the store
    assert (d.status((d.blob, d.st, d.nb), block_size=st.block + 1) == M.UNLOCATED).all()
    for case in M.cases(name):
        got = d.status(d.case(case))
        want = M.expected(st, case)
        assert np.array_equal(got, want), (case.name, got.tolist(), want.tolist())
    # a leading shape, and a blob that is not 16-byte aligned
    shaped = d.fa.frame_status_device(d.blob, d.st.reshape(3, 1), d.nb.reshape(3, 1), st.n, is_int64=d.wide, block_size=st.block)
    assert tuple(shaped.shape) == (3, 1, 3) and not bool(shaped.any())
    case = M.cases(name)[0]
    padded = d.torch.zeros(case.blob.size + 16, dtype=d.torch.uint8, device="cuda")
    for shift in (1, 7):
        padded[shift : shift + case.blob.size] = _up(d.torch, case.blob)
        view = padded[shift : shift + case.blob.size]
        assert view.data_ptr() % 16 == shift
        got = d.fa.frame_status_device(view, _up(d.torch, case.starts), _up(d.torch, case.nbytes), st.n, is_int64=d.wide, block_size=st.block)
        assert np.array_equal(got.cpu().numpy(), M.expected(st, case)), (case.name, shift)


def test_frame_status_of_every_length(torch, fa, oracle):
    """Frames of every length around the fold's stripe and trip edges, each damaged in its first, its last covered and its
    two footer bytes in turn; the last frame of the last stream ends with the blob."""
    calls = 0
    for st in M.length_stores():
        starts, nbytes = _up(torch, st.starts), _up(torch, st.nbytes)
        run = lambda blob: fa.frame_status_device(_up(torch, blob), starts, nbytes, st.n, block_size=st.block).cpu().numpy()  # noqa: E731
        assert not run(st.blob).any(), st.name
        for label, blob in M.length_cases(st):
            want = M.frame_status(blob, st.starts, st.nbytes, st.n, 1, st.block)
            assert want[:, -1].all() and not want[:, :-1].any()
            got = run(blob)
            assert np.array_equal(got, want), (st.name, label, [fr[-1].nbytes - 2 for fr in st.frames], got[:, -1].tolist(), want[:, -1].tolist())
            calls += 1
    print("length corpus: %d stores, %d damaged calls" % (len(M.length_stores()), calls))


def test_bad_arguments(torch, fa, devs):
    d = devs("foreign64")
    L = __import__("flacarray_amd._lib", fromlist=["lib"]).lib()
    status = torch.zeros(9, dtype=torch.uint8, device="cuda")
    vp = lambda t: ctypes.c_void_p(t.data_ptr())  # noqa: E731
    args = lambda **kw: [kw.get("blob", vp(d.blob)), d.blob.numel(), vp(d.st), vp(d.nb), kw.get("n_stream", 3), kw.get("n", d.store.n),  # noqa: E731
                         kw.get("ch", 1), kw.get("block", 64), vp(status), None]
    assert L.fa_frame_status_device(*args()) == 0
    for kw in (dict(n_stream=0), dict(n=0), dict(ch=3), dict(ch=0), dict(block=0), dict(block=65536)):
        assert L.fa_frame_status_device(*args(**kw)) != 0, kw
    with pytest.raises(RuntimeError, match="first_sample is larger than last_sample"):
        fa.decode_flac_salvage_device(d.blob, d.st, d.nb, d.store.n, 5, 5)
    with pytest.raises(RuntimeError, match="last_sample is beyond end of stream"):
        fa.decode_flac_salvage_device(d.blob, d.st, d.nb, d.store.n, 0, d.store.n + 1)
    with pytest.raises(RuntimeError, match="you must also provide the gains"):
        fa.decode_flac_salvage_device(d.blob, d.st, d.nb, d.store.n, offsets=d.off)
    with pytest.raises(RuntimeError, match="starts data should be of type int64"):
        fa.decode_flac_salvage_device(d.blob, d.st.int(), d.nb, d.store.n)


# ----------------------------------------------------------------------------------------------------- the salvage

@pytest.mark.parametrize("name", M.STORES)
def test_salvage_equals_the_model(devs, decoder_dispatch, name):
    d = devs(name)
    st = d.store
    calls = 0
    for k, case in enumerate(M.cases(name)):
        triple = d.case(case)
        want_status = M.expected(st, case)
        for first, last in M.windows(st, want_status):
            fill = None if (k + first) % 2 == 0 else -7
            out, status = d.salvage(triple, first, last, fill=fill)
            assert np.array_equal(status, want_status), (case.name, first, last)
            want = M.salvage_model(d.ints, want_status, first, last, 0 if fill is None else fill, st.block)
            assert _bits(out, want), (case.name, first, last, np.argwhere(out != want)[:3].tolist())
            fout, fstatus = d.salvage(triple, first, last, floats=True)
            assert np.array_equal(fstatus, want_status)
            fwant = M.salvage_model(d.floats, want_status, first, last, np.nan, st.block)
            assert _bits(fout, fwant), (case.name, first, last, "float")
            calls += 2
    print("salvage %s %s: %d calls" % (name, decoder_dispatch, calls))


@pytest.mark.parametrize("name", M.STORES)
def test_salvage_of_an_intact_store_is_the_decode(devs, decoder_dispatch, name):
    d = devs(name)
    st = d.store
    intact = (d.blob, d.st, d.nb)
    for first, last in ((-1, -1), (0, st.n), (st.block - 1, st.block + 1), (st.n - 7, st.n), (5, 6)):
        out, status = d.salvage(intact, first, last, block_size=None)
        assert not status.any()
        want = d.fa.decode_flac_device(*intact, st.n, first, last, is_int64=d.wide).cpu().numpy()
        assert _bits(out, want)
        fout, _ = d.salvage(intact, first, last, floats=True)
        fwant = d.fa.decode_flac_device(*intact, st.n, first, last, offsets=d.off, gains=d.gain, is_int64=d.wide).cpu().numpy()
        assert _bits(fout, fwant)


@pytest.mark.parametrize("name", ["own1152", "own1152x2"])
def test_seek_damage_stops_the_decode_and_not_the_salvage(devs, decoder_dispatch, name):
    d = devs(name)
    st = d.store
    case = next(c for c in M.cases(name) if c.name.startswith("seek sample number") and c.name.endswith("f1"))
    triple = d.case(case)
    with pytest.raises(RuntimeError, match="Decoding failed"):
        d.fa.decode_flac_device(*triple, st.n, is_int64=d.wide)
    with pytest.raises(RuntimeError):
        d.fa.DeviceDecodeIndex(*triple, st.n, is_int64=d.wide)
    out, status = d.salvage(triple)
    s = int(case.name.split(" @ s")[1].split()[0])
    want = np.zeros((3, 3), np.uint8)
    want[s, 0:2] = M.UNLOCATED
    assert np.array_equal(status, want)
    keep = np.ones(out.shape, bool)
    keep[s, : 2 * st.block] = False
    assert np.array_equal(out[keep], st.data[keep]) and not out[~keep].any()
    assert np.array_equal(d.fa.decode_flac_device(d.blob, d.st, d.nb, st.n, is_int64=d.wide).cpu().numpy(), st.data)  # (no stale error)


# --------------------------------------------------------------------------------------------------- the footprint

def _vp(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


@pytest.mark.parametrize("name", ["own1152", "own4096", "own1152x2"])
def test_salvage_footprint(torch, fa, devs, decoder_dispatch, name):
    """The salvage through the C ABI into a guarded buffer of sentinel, the output pointer 1 to 3 elements off a 16-byte
    boundary: the whole buffer is compared."""
    from flacarray_amd import _lib

    L = _lib.lib()
    d = devs(name)
    st = d.store
    tdt, ndt, item = (torch.int64, np.int64, 8) if d.wide else (torch.int32, np.int32, 4)
    fn = L.fa_decode_salvage_i64_device if d.wide else L.fa_decode_salvage_i32_device
    sentinel = -0x5A5A5A5B
    picks = [c for c in M.cases(name) if c.name.split(" @ ")[0] in ("footer", "sync", "seek offset beyond", "zeros across f0 / f1", "half nbytes")]
    for k, case in enumerate(picks):
        triple = d.case(case)
        want_status = M.expected(st, case)
        for j, (first, last) in enumerate(M.windows(st, want_status)):
            m = 1 + (k + j) % 3
            nd = last - first
            for floats in (False, True):
                buf = torch.full((2 * GUARD + 4 + 3 * nd,), sentinel, dtype=tdt, device="cuda")
                assert buf.data_ptr() % 16 == 0
                status = torch.full((9,), 0xEE, dtype=torch.uint8, device="cuda")
                out = ctypes.c_void_p(buf.data_ptr() + (GUARD + m) * item)
                fill = np.array([np.nan if floats else -7], dtype=(np.float64 if d.wide else np.float32) if floats else ndt)
                o = (None, out, _vp(d.off), _vp(d.gain)) if floats else (out, None, None, None)
                torch.cuda.synchronize()
                rc = fn(_vp(triple[0]), triple[0].numel(), _vp(triple[1]), _vp(triple[2]), 3, st.n, first, last, *o, st.block,
                        ctypes.c_void_p(fill.ctypes.data), _vp(status), None)
                torch.cuda.synchronize()
                assert rc == 0, (case.name, first, last, rc)
                assert np.array_equal(status.cpu().numpy().reshape(3, 3), want_status)
                image = np.full(buf.numel(), sentinel, dtype=ndt)
                model = M.salvage_model(d.floats if floats else d.ints, want_status, first, last, fill[0], st.block)
                image[GUARD + m : GUARD + m + 3 * nd] = model.reshape(-1).view(ndt)
                assert buf.cpu().numpy().tobytes() == image.tobytes(), (case.name, first, last, floats, m)


@pytest.mark.parametrize("elem", [4, 8])
def test_fill_ranges_footprint(torch, elem):
    """fa_fill_ranges_device at odd offsets from a misaligned pointer: lengths around the 16-element group and the
    2048-element piece, and longer ones; ranges touch, leave gaps of one element, and come out of order."""
    from flacarray_amd import _lib

    L = _lib.lib()
    tdt, ndt = (torch.int32, np.int32) if elem == 4 else (torch.int64, np.int64)
    sentinel = 0x3C3C3C3C
    for lengths in ((1, 15, 16, 17, 2047, 2048, 2049, 1152, 4096), (4096, 2049, 1, 8193, 17, 0, 16, 65535)):
        for m in (0, 1, 3):
            offs, at = [], 1
            for n in lengths:
                offs.append(at)
                at += n + n % 2  # every range starts at an odd offset: it touches the one in front of it, or leaves one sentinel element
            order = list(range(len(lengths)))[::-1] if m == 1 else list(range(len(lengths)))
            h_off = np.array([offs[i] for i in order], dtype=np.int64)
            h_cnt = np.array([lengths[i] for i in order], dtype=np.int64)
            buf = torch.full((2 * GUARD + 4 + at,), sentinel, dtype=tdt, device="cuda")
            assert buf.data_ptr() % 16 == 0
            fill = np.array([-123456789 - m], dtype=ndt)
            image = np.full(buf.numel(), sentinel, dtype=ndt)
            for o, n in zip(offs, lengths):
                image[GUARD + m + o : GUARD + m + o + n] = fill[0]
            d_off, d_cnt = _up(torch, h_off), _up(torch, h_cnt)
            torch.cuda.synchronize()
            rc = L.fa_fill_ranges_device(ctypes.c_void_p(buf.data_ptr() + (GUARD + m) * elem), elem, len(lengths), _vp(d_off), _vp(d_cnt),
                                         ctypes.c_void_p(fill.ctypes.data), None)
            torch.cuda.synchronize()
            assert rc == 0
            assert buf.cpu().numpy().tobytes() == image.tobytes(), (lengths, m)
    assert L.fa_fill_ranges_device(None, 2, 1, None, None, None, None) != 0
    assert L.fa_fill_ranges_device(None, 4, 0, None, None, ctypes.c_void_p(fill.ctypes.data), None) == 0


# --------------------------------------------------------------------------------------------------- call state

def test_salvage_after_other_calls_and_on_a_side_stream(torch, fa, devs, decoder_dispatch):
    d = devs("own1152")
    st = d.store
    case = next(c for c in M.cases("own1152") if c.name.startswith("zeros across"))
    triple = d.case(case)
    want_status = M.expected(st, case)
    want = M.salvage_model(d.ints, want_status, 0, st.n, 0, st.block)
    first_out, first_status = d.salvage(triple)
    assert _bits(first_out, want) and np.array_equal(first_status, want_status)
    # other shapes through the decoders, the reducer and the encoder: they grow and dirty the cached scratch
    other = devs("lpc4096")
    fa.decode_flac_device(other.blob, other.st, other.nb, other.store.n, 3, other.store.n - 2)
    fa.reduce_flac_device(other.blob, other.st, other.nb, other.store.n, width=1000)
    fa.encode_flac_device(_up(torch, V.full_range_i32((2, 5000), seed=9)), level=3)
    fa.frame_status_device(other.blob, other.st, other.nb, other.store.n)
    for _ in range(2):
        out, status = d.salvage(triple)
        assert _bits(out, want) and np.array_equal(status, want_status)
    fout, _ = d.salvage(triple, 100, st.n - 100, floats=True)
    assert _bits(fout, M.salvage_model(d.floats, want_status, 100, st.n - 100, np.nan, st.block))
    # behind a delayed producer on a non-blocking side stream: the decoy is the intact blob
    side = torch.cuda.Stream()
    call = lambda blob: fa.decode_flac_salvage_device(blob, triple[1], triple[2], st.n, block_size=st.block)  # noqa: E731
    got, expected = T.run_delayed("salvage", side, [triple[0]], [d.blob.clone()], call)
    assert _bits(got[0], want) and np.array_equal(got[1], want_status)
    call = lambda blob: fa.frame_status_device(blob, triple[1], triple[2], st.n, block_size=st.block)  # noqa: E731
    got, expected = T.run_delayed("frame_status", side, [triple[0]], [d.blob.clone()], call)
    assert np.array_equal(got, want_status)


# ---------------------------------------------------------------------------------------------------- FlacArray

@pytest.mark.parametrize("kind", ["int32", "float32", "int64"])
@pytest.mark.parametrize("resident", [False, True], ids=["host", "resident"])
def test_flacarray_damage_methods(torch, fa, decoder_dispatch, kind, resident):
    rng = np.random.default_rng(31)
    n, block = 2 * 4096 + 7, 4096
    if kind == "int32":
        data = rng.integers(-(2**31), 2**31 - 1, (2, 2, n), dtype=np.int64).astype(np.int32)
    elif kind == "int64":
        data = V.full_range_i64((2, 2, n), seed=42)
    else:
        data = rng.normal(0, 1, (2, 2, n)).astype(np.float32)
    good = fa.FlacArray.from_array(data, level=5) if kind != "float32" else fa.FlacArray.from_array(data, level=5, quanta=1e-4)
    intact = good.to_array()
    blob = np.array(good.compressed, dtype=np.uint8, copy=True)
    starts, nbytes = np.asarray(good.stream_starts), np.asarray(good.stream_nbytes)
    # flat stream 2: a footer byte of its last frame (the last two bytes of the stream); flat stream 1: its second seek point
    s2 = int(starts.reshape(-1)[2])
    blob[s2 + int(nbytes.reshape(-1)[2]) - 1] ^= 0x01
    s1 = int(starts.reshape(-1)[1])
    seg = bytes(blob[s1 : s1 + int(nbytes.reshape(-1)[1])])
    blob[s1 + M._chain(seg)[2][0] + 18 + 7] ^= 0x01
    bad = fa.FlacArray(None, shape=good.shape, global_shape=good.global_shape, compressed=blob, dtype=good.dtype, stream_starts=starts,
                       stream_nbytes=nbytes, stream_offsets=good.stream_offsets, stream_gains=good.stream_gains)
    if resident:
        bad.to_device()
        with pytest.raises(RuntimeError):
            bad[0, 1, :10]
    want_status = np.zeros((2, 2, 3), np.uint8)
    want_status[1, 0, 2] = M.CRC16
    want_status[0, 1, 0:2] = M.UNLOCATED
    assert np.array_equal(M.frame_status(blob, starts, nbytes, n, 2 if kind == "int64" else 1, block).reshape(2, 2, 3), want_status)
    status = bad.frame_status()
    assert status.dtype == np.uint8 and np.array_equal(status, want_status)
    ranges = bad.damaged_ranges()
    assert np.array_equal(ranges, [[1, 0, 2 * block], [2, 2 * block, n]]) and ranges.dtype == np.int64
    assert np.array_equal(bad.damaged_ranges(status), ranges)
    fill = np.nan if kind == "float32" else 0
    for sl in (None, slice(block - 3, 2 * block + 5), slice(0, 10)):
        arr, st2 = bad.salvage(stream_slice=sl)
        assert np.array_equal(st2, want_status)
        lo, hi = (0, n) if sl is None else (sl.start, sl.stop)
        want = M.salvage_model(intact.reshape(4, n), want_status, lo, hi, fill, block).reshape(2, 2, hi - lo)
        assert _bits(arr, want), (kind, sl)
    arr, _ = bad.salvage(fill=5)
    assert _bits(arr, M.salvage_model(intact.reshape(4, n), want_status, 0, n, 5, block).reshape(2, 2, n))
    assert not good.frame_status().any() and good.damaged_ranges().shape == (0, 3)
    if resident:
        bad.release_device()
