"""Wide stores on every device path: thousands to 3 x 10^5 streams of one short frame each (tests/wide_corpus.py; the
thresholds each geometry crosses are asserted on the CPU by tests/test_wide_corpus.py).

The reference of everything here is the CPU oracle (oracle.encode_i32 / _i64, decode_*, float*_to_int*, int*_to_float*),
hashlib.md5 and numpy: the library is never compared with itself.  The oracle's results are made once per geometry and
shared through the module's cache; nothing writes into them.
"""
import ctypes
import hashlib

import numpy as np
import pytest

from tests import wide_corpus as WC

pytestmark = pytest.mark.gpu

GUARD = 4096
DISPATCH_VARS = ("FLACARRAY_HIP_PLACED_BELOW", "FLACARRAY_HIP_LATENCY", "FLACARRAY_HIP_SLOTS", "FLACARRAY_HIP_VERIFY_AFTER",
                 "FLACARRAY_HIP_NO_SYNC_SCAN", "FLACARRAY_HIP_PLACED_GRID")
INFO_KEYS = ["type", "order", "porder", "wasted", "shift", "precision", "nbytes", "blocksize"]


@pytest.fixture(scope="module")
def fa():
    import flacarray_amd

    return flacarray_amd


@pytest.fixture(scope="module")
def torch():
    import torch

    assert torch.cuda.is_available()
    return torch


@pytest.fixture(autouse=True)
def _own_dispatch(monkeypatch):
    for v in DISPATCH_VARS:
        monkeypatch.delenv(v, raising=False)


class Geo:
    """One case of WC.GEOMETRIES with the oracle's view of it: x (the integers), f / q (the floats and quanta of a float
    case), off / gain (the oracle's), and the oracle's encode (blob, st, nb)."""

    def __init__(self, oracle, shape, dt, level, quanta="given"):
        self.ns, self.n = shape
        self.dt, self.level, self.wide = dt, level, dt in ("i64", "f64")
        self.B = WC.block_size(level)
        self.nf = -(-self.n // self.B)
        self.f = self.q = self.off = self.gain = None
        if dt in ("i32", "i64"):
            self.x = WC.wide_rows(self.ns, self.n, self.wide, 0)
        else:
            ndt = np.float32 if dt == "f32" else np.float64
            self.f = WC.wide_floats(self.ns, self.n, ndt, 0)
            self.q = WC.wide_quanta(self.ns, ndt) if quanta == "given" else None
            self.x, self.off, self.gain = (oracle.float64_to_int64 if self.wide else oracle.float32_to_int32)(self.f, self.q)
        self.blob, self.st, self.nb = _oracle_encode(oracle, self.x, level)


def _oracle_encode(oracle, x, level):
    return (oracle.encode_i64 if x.dtype == np.int64 else oracle.encode_i32)(x, level, use_threads=True)


@pytest.fixture(scope="module")
def geo(oracle):
    made = {}

    def get(shape, dt, level, quanta="given"):
        key = (tuple(shape), dt, level, quanta)
        if key not in made:  # (all of them together: about 3 GB of host memory)
            made[key] = Geo(oracle, shape, dt, level, quanta)
        return made[key]

    yield get
    made.clear()


def _dev(torch, a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _host(t):
    return t.cpu().numpy() if hasattr(t, "cpu") else np.asarray(t)


def _assert_store(got, want, what=""):
    """(compressed, starts, nbytes) from the device against the oracle's triple; the index first (a wrong start names its
    stream), then the bytes, with the first differing stream named."""
    blob, st, nb = (_host(t).reshape(-1) for t in got[:3])
    wb, wst, wnb = (np.asarray(t).reshape(-1) for t in want)
    bad = np.flatnonzero(nb != wnb)
    assert bad.size == 0, "%s: %d stream sizes differ, first stream %d: %d, oracle %d" % (what, bad.size, bad[0], nb[bad[0]], wnb[bad[0]])
    bad = np.flatnonzero(st != wst)
    assert bad.size == 0, "%s: %d starts differ, first stream %d: %d, oracle %d" % (what, bad.size, bad[0], st[bad[0]], wst[bad[0]])
    assert blob.size == wb.size, "%s: %d bytes, oracle %d" % (what, blob.size, wb.size)
    if not np.array_equal(blob, wb):
        at = int(np.flatnonzero(blob != wb)[0])
        s = int(np.searchsorted(wst, at, side="right") - 1)
        raise AssertionError("%s: %d bytes differ, first at byte %d = stream %d + %d" % (what, int((blob != wb).sum()), at, s, at - wst[s]))


def _info_rows(info, g, s):
    k = g.nf * (2 if g.wide else 1)
    return _host(info[s * k : (s + 1) * k])


def _info_want(oracle, g, s):
    fn = oracle.stream_info_i64 if g.wide else oracle.stream_info
    return np.array([[f[k] for k in INFO_KEYS] for f in fn(g.x[s], g.level)], dtype=np.int32)


def _up_store(torch, g):
    return _dev(torch, g.blob), _dev(torch, g.st), _dev(torch, g.nb)


# ------------------------------------------------------------------------------------------------------------ encode

INT_CASES = [(name, shape, dt, level) for name, v in WC.GEOMETRIES.items() if name != "k3f_tailcap"
             for shape, dt, level in v["cases"] if dt in ("i32", "i64")]
# K3F's geometry also with FLACARRAY_HIP_PLACED_BELOW=0 (`k3f`: the route it takes by its frame count already, the bytes must
# not move) and sent to K3G (`placed`: 16 389 tickets of one whole frame each)
ROUTES = ["default", "slots", "k3f", "placed", "c_entry"]
ENCODE_PARAMS = [c + (r,) for c in INT_CASES for r in ROUTES if r not in ("k3f", "placed") or c[0] == "k3f_wide"]
ENCODE_IDS = ["%s-%dx%d-%s-l%d-%s" % (c[0], c[1][0], c[1][1], c[2], c[3], c[4]) for c in ENCODE_PARAMS]


def _c_encode(torch, xd, level, dirty=0xA5):
    """fa_encode_i32_device / _i64_device called as a C caller does: a workspace and an output buffer full of 0xA5, a guard
    of GUARD bytes behind `capacity`.  Returns (buffer with its guard, capacity, total, starts, nbytes)."""
    from flacarray_amd import _lib
    from flacarray_amd.libflacarray import _dp, _stream_ptr

    L = _lib.lib()
    i64 = xd.dtype == torch.int64
    ns, n = xd.shape
    cap = (L.fa_encode_capacity_bytes_i64 if i64 else L.fa_encode_capacity_bytes)(ns, n, level)
    need = (L.fa_encode_single_pass_workspace_bytes_i64 if i64 else L.fa_encode_single_pass_workspace_bytes)(ns, n, level)
    assert cap > 0 and need > 0
    ws = torch.full((need,), dirty, dtype=torch.uint8, device=xd.device)
    buf = torch.full((cap + GUARD,), dirty, dtype=torch.uint8, device=xd.device)
    index = torch.full((2 * ns,), -1, dtype=torch.int64, device=xd.device)
    total = ctypes.c_int64(-1)
    rc = (L.fa_encode_i64_device if i64 else L.fa_encode_i32_device)(
        _dp(xd), ns, n, level, _dp(ws), ws.numel(), _dp(buf), cap, _dp(index[:ns]), _dp(index[ns:]), ctypes.byref(total), None, _stream_ptr())
    torch.cuda.synchronize()
    assert rc == 0, "fa_encode_*_device returned %d" % rc
    return buf, cap, total.value, index[:ns], index[ns:]


@pytest.mark.parametrize("name,shape,dt,level,route", ENCODE_PARAMS, ids=ENCODE_IDS)
def test_encode(fa, torch, oracle, geo, monkeypatch, name, shape, dt, level, route):
    """Every integer geometry through every encode route that takes it: the triple is the oracle's byte for byte, and the
    d_info words of the first, the last and the boundary streams are the oracle's decisions."""
    g = geo(shape, dt, level)
    xd = _dev(torch, g.x)
    if route == "slots":
        monkeypatch.setenv("FLACARRAY_HIP_SLOTS", "1")
    elif route == "k3f":
        monkeypatch.setenv("FLACARRAY_HIP_PLACED_BELOW", "0")
    elif route == "placed":
        monkeypatch.setenv("FLACARRAY_HIP_PLACED_BELOW", "1000000000")
    if route == "c_entry":
        buf, cap, total, st, nb = _c_encode(torch, xd, level)
        assert total == g.blob.size
        _assert_store((buf[:total], st, nb), (g.blob, g.st, g.nb), "c entry")
        assert bool((buf[cap:] == 0xA5).all()), "bytes behind `capacity` were written"
        return
    comp, st, nb, info = fa.encode_flac_device(xd, level=level, return_info=True)
    torch.cuda.synchronize()
    _assert_store((comp, st, nb), (g.blob, g.st, g.nb), route)
    for s in WC.boundary_streams(g.ns):
        assert np.array_equal(_info_rows(info, g, s), _info_want(oracle, g, s)), "d_info of stream %d" % s


@pytest.mark.parametrize("quanta", ["given", "range"])
def test_encode_f32_k3f_wide(fa, torch, oracle, geo, quanta):
    """float32 (16 389, 4096) through fa_encode_f32_device (quantised in K3F's staging load): float32_range_kernel with
    n_stream * 1 blocks, float32_params_kernel's ragged last block; quanta given, and derived from each stream's range."""
    shape, dt, level = WC.GEOMETRIES["k3f_wide"]["cases"][2]
    g = geo(shape, dt, level, quanta)
    q = None if g.q is None else _dev(torch, g.q)
    comp, st, nb, off, gain = fa.encode_flac_device_f32(_dev(torch, g.f), quanta=q, level=level)
    torch.cuda.synchronize()
    assert _host(off).tobytes() == g.off.tobytes() and _host(gain).tobytes() == g.gain.tobytes()
    _assert_store((comp, st, nb), (g.blob, g.st, g.nb), "f32 " + quanta)


# ------------------------------------------------------------------------------------------------------------ decode

DECODE_CASES = [c for c in INT_CASES if not (c[0] == "k3f_wide" and c[3] == 8)]  # (level 8 writes frames of level 5's kinds)
DECODE_IDS = ["%s-%dx%d-%s-l%d" % (name, shape[0], shape[1], dt, level) for name, shape, dt, level in DECODE_CASES]
# K7L takes launches of at most 4096 frames on its own; those also go through K7 (FLACARRAY_HIP_LATENCY=0)
DECODE_PARAMS = [c + (lat,) for c in DECODE_CASES for lat in ("auto", "k7")
                 if lat == "auto" or c[1][0] * -(-c[1][1] // WC.block_size(c[3])) <= WC.LATENCY_MAX_TASKS]
DECODE_PARAM_IDS = ["%s-%dx%d-%s-l%d-%s" % (c[0], c[1][0], c[1][1], c[2], c[3], c[4]) for c in DECODE_PARAMS]


def _scales(g):
    """Per-stream offsets and gains that differ from stream to stream (exact in float32)."""
    ft = np.float64 if g.wide else np.float32
    s = np.arange(g.ns)
    return (s % 17).astype(ft), (2.0 ** (s % 3)).astype(ft)


def _restore(oracle, g, x, off, gain):
    return (oracle.int64_to_float64 if g.wide else oracle.int32_to_float32)(x, off, gain)


def _inner_range(n):
    return (n // 3, n - n // 4) if n >= 3 else (0, n)


@pytest.mark.parametrize("name,shape,dt,level,latency", DECODE_PARAMS, ids=DECODE_PARAM_IDS)
def test_decode(fa, torch, oracle, geo, monkeypatch, name, shape, dt, level, latency):
    """decode_flac_device of the ORACLE's blob: whole, a range inside a frame, integers and restored floats.  Up to 4096
    frames the launch is K7L's by default and K7's under FLACARRAY_HIP_LATENCY=0; above, K7's either way."""
    g = geo(shape, dt, level)
    if latency == "k7":
        monkeypatch.setenv("FLACARRAY_HIP_LATENCY", "0")
    comp, st, nb = _up_store(torch, g)
    lo, hi = _inner_range(g.n)
    off, gain = _scales(g)
    y = fa.decode_flac_device(comp, st, nb, g.n, is_int64=g.wide)
    assert np.array_equal(_host(y), g.x)
    del y
    y = fa.decode_flac_device(comp, st, nb, g.n, lo, hi, is_int64=g.wide)
    assert np.array_equal(_host(y), g.x[:, lo:hi])
    del y
    y = fa.decode_flac_device(comp, st, nb, g.n, lo, hi, offsets=_dev(torch, off), gains=_dev(torch, gain), is_int64=g.wide)
    assert _host(y).tobytes() == np.ascontiguousarray(_restore(oracle, g, g.x, off, gain)[:, lo:hi]).tobytes()


def _slices(g, seed=7, extra=10000):
    """One slice per stream in shuffled order, then `extra` random ones; and what they decode to, by one fancy index."""
    rng = np.random.default_rng(seed)
    ss = np.concatenate([rng.permutation(g.ns), rng.integers(0, g.ns, extra)]).astype(np.int64)
    ff = rng.integers(0, g.n, ss.size).astype(np.int64)
    cc = (1 + rng.integers(0, g.n - ff)).astype(np.int64)
    out_off = np.concatenate([[0], np.cumsum(cc)[:-1]])
    flat = np.repeat(ss * g.n + ff - out_off, cc) + np.arange(int(cc.sum()))
    return ss, ff, cc, g.x.reshape(-1)[flat]


@pytest.mark.parametrize("name,shape,dt,level", DECODE_CASES, ids=DECODE_IDS)
def test_decode_slices(fa, torch, geo, name, shape, dt, level):
    """decode_slices_device and DeviceDecodeIndex.decode_slices: one slice per stream in shuffled order plus 10 000 random
    ones in a single call, to the device and to the host."""
    g = geo(shape, dt, level)
    comp, st, nb = _up_store(torch, g)
    ss, ff, cc, want = _slices(g)
    got, _ = fa.decode_slices_device(comp, st, nb, g.n, ss, ff, cc, is_int64=g.wide)
    assert np.array_equal(_host(got), want)
    del got
    index = fa.DeviceDecodeIndex(comp, st, nb, g.n, is_int64=g.wide)
    try:
        got, _ = index.decode_slices(ss, ff, cc)
        assert np.array_equal(_host(got), want)
        del got
        got, _ = index.decode_slices(ss, ff, cc, to_host=True)
        assert np.array_equal(got, want)
        assert np.array_equal(_host(index.decode()), g.x)
    finally:
        index.close()


@pytest.mark.parametrize("resident", [True, False], ids=["resident", "host"])
@pytest.mark.parametrize("name,shape,dt,level", DECODE_CASES, ids=DECODE_IDS)
def test_flacarray_reads(fa, torch, geo, name, shape, dt, level, resident):
    """FlacArray over the oracle's store: __getitem__ and to_array(keep=) with a mask of every third stream."""
    g = geo(shape, dt, level)
    arr = fa.FlacArray(None, shape=g.x.shape, compressed=g.blob, dtype=g.x.dtype, stream_starts=g.st, stream_nbytes=g.nb)
    if resident:
        arr.to_device()
    try:
        lo, hi = _inner_range(g.n)
        assert np.array_equal(arr[::3, lo:hi], g.x[::3, lo:hi])
        assert np.array_equal(arr[g.ns - 2], g.x[g.ns - 2])
        keep = np.zeros(g.ns, dtype=bool)
        keep[::3] = True
        got, idx = arr.to_array(keep=keep, keep_indices=True)
        assert np.array_equal(got, g.x[::3]) and [i[0] for i in idx] == list(range(0, g.ns, 3))
    finally:
        arr.release_device()


VERIFY_CASES = [("u16", (70001, 19), "i32", 5), ("k3f_wide", (16389, 4096), "i32", 5)]


@pytest.mark.parametrize("name,shape,dt,level", VERIFY_CASES, ids=[c[0] for c in VERIFY_CASES])
def test_verified_decode_both_sides_of_16384_tasks(fa, torch, geo, name, shape, dt, level):
    """verify=True with 16 383 tasks (the frame check behind the decoder) and with all of them (16 384 and more: beside
    K7): the intact store decodes to its input, one flipped payload bit in stream n - 2 (16 382 for the small launch)
    raises."""
    g = geo(shape, dt, level)
    comp, st, nb = _up_store(torch, g)
    below = WC.BESIDE_MIN_TASKS - 1
    assert g.nf == 1 and below < g.ns
    for k in (below, g.ns):
        y = fa.decode_flac_device(comp, st[:k].contiguous(), nb[:k].contiguous(), g.n, verify=True)
        assert np.array_equal(_host(y), g.x[:k])
        del y
        bad = comp.clone()
        bad[int(g.st[k - 2] + g.nb[k - 2]) - 3] ^= 0x04  # (the last payload byte in front of the frame's CRC-16)
        with pytest.raises(RuntimeError, match="Decoding failed"):
            fa.decode_flac_device(bad, st[:k].contiguous(), nb[:k].contiguous(), g.n, verify=True)
        torch.cuda.synchronize()


STRIP_CASES = [c for c in DECODE_CASES if c[0] in ("scan3", "u16")]


@pytest.mark.parametrize("scan", ["sync_scan", "serial_walk"])
@pytest.mark.parametrize("name,shape,dt,level", STRIP_CASES, ids=["%s-%dx%d-%s-l%d" % (c[0], c[1][0], c[1][1], c[2], c[3]) for c in STRIP_CASES])
def test_decode_without_seektable(fa, torch, geo, monkeypatch, name, shape, dt, level, scan):
    """The stores without their SEEKTABLEs (the layout libFLAC writes): frames located by the sync scan (scan_sync_kernel with
    n_stream in grid.x) and, with the scan switched off, by the serial walk; whole, and one slice per stream."""
    if scan == "serial_walk":
        monkeypatch.setenv("FLACARRAY_HIP_NO_SYNC_SCAN", "1")
    g = geo(shape, dt, level)
    comp, st, nb = (_dev(torch, a) for a in WC.strip_seektables(g.blob, g.st, g.nb, g.nf))
    y = fa.decode_flac_device(comp, st, nb, g.n, is_int64=g.wide, verify=True)
    assert np.array_equal(_host(y), g.x)
    ss, ff, cc, want = _slices(g, seed=8, extra=100)
    got, _ = fa.decode_slices_device(comp, st, nb, g.n, ss, ff, cc, is_int64=g.wide)
    assert np.array_equal(_host(got), want)


# --------------------------------------------------------------------------------------------------- store operations

OPS_CASES = [c for c in INT_CASES if c[0] == "scan3"] + [("u16", (70001, 19), "i32", 5)]
OPS_IDS = ["%s-%dx%d-%s-l%d" % (name, shape[0], shape[1], dt, level) for name, shape, dt, level in OPS_CASES]
ops = pytest.mark.parametrize("name,shape,dt,level", OPS_CASES, ids=OPS_IDS)


def _clean(fa, torch, store, n, wide, B):
    status = fa.frame_status_device(store[0], store[1], store[2], n, is_int64=wide, block_size=B)
    assert int(torch.count_nonzero(status)) == 0, "frame_status is not all zero"


def _other(g, seed, n=None):
    """Another corpus of the case's stream count and type (new samples for appends, overwrites and joins)."""
    return WC.wide_rows(g.ns, g.n if n is None else n, g.wide, seed)


def _split(g):
    """Where an append starts: inside the only frame of a short stream, behind one whole frame and 7 samples of a long one."""
    return 20 if g.nf == 1 else g.B + 7


@ops
def test_append(fa, torch, oracle, geo, name, shape, dt, level):
    g = geo(shape, dt, level)
    k = _split(g)
    old = tuple(_dev(torch, a) for a in _oracle_encode(oracle, g.x[:, :k], level))
    got = fa.append_flac_device(*old, k, _dev(torch, g.x[:, k:]), level=level, verify=True)
    _assert_store(got, (g.blob, g.st, g.nb), "append")
    _clean(fa, torch, got, g.n, g.wide, g.B)


@pytest.mark.parametrize("which", ["all", "subset"])
@ops
def test_overwrite(fa, torch, oracle, geo, name, shape, dt, level, which):
    """Over all streams, and over a shuffled subset of 1500 (rows in the subset's order)."""
    g = geo(shape, dt, level)
    first = 3 if g.nf == 1 else g.B - 5  # (a long stream: across a frame boundary)
    m = 11 if g.nf == 1 else g.B + 9
    new = _other(g, 21, m)
    streams = None if which == "all" else np.random.default_rng(3).permutation(g.ns)[:1500]
    rows = slice(None) if streams is None else streams
    patched = g.x.copy()
    patched[rows, first : first + m] = new[rows]
    got = fa.overwrite_flac_device(*_up_store(torch, g), g.n, first, _dev(torch, new[rows]), streams=streams, level=level, verify=True)
    _assert_store(got, _oracle_encode(oracle, patched, level), "overwrite " + which)
    _clean(fa, torch, got, g.n, g.wide, g.B)


def _windows(g):
    """(what, first, last, streams): aligned with `last` at a frame's end and inside a frame, unaligned, and stream picks."""
    picks = np.random.default_rng(4).permutation(g.ns)[:1500]
    if g.nf == 1:
        return [("aligned_inside", 0, g.n // 2 + 1, None), ("unaligned", 5, g.n, None), ("picks", 0, g.n, picks), ("picks_inside", 0, 9, picks)]
    return [("aligned", g.B, 3 * g.B, None), ("aligned_inside", g.B, 2 * g.B + 100, None), ("unaligned", 100, g.n - 3, None),
            ("picks", 0, g.n, picks), ("picks_inside", g.B, 2 * g.B + 100, picks)]


@ops
def test_window(fa, torch, oracle, geo, name, shape, dt, level):
    g = geo(shape, dt, level)
    store = _up_store(torch, g)
    for what, first, last, streams in _windows(g):
        got = fa.window_flac_device(*store, g.n, first, last, streams=streams, level=level, is_int64=g.wide, verify=True)
        rows = slice(None) if streams is None else streams
        _assert_store(got, _oracle_encode(oracle, g.x[rows, first:last], level), "window " + what)
        _clean(fa, torch, got, last - first, g.wide, g.B)


@pytest.mark.parametrize("how", ["aligned", "unaligned"])
@ops
def test_join(fa, torch, oracle, geo, name, shape, dt, level, how):
    """Two and three parts: `aligned`, a part of one whole block in front (nothing decoded); `unaligned`, the case's own
    array in front (a decode and an append behind the first boundary).  The whole block in front of 70 001 streams is
    one of level 1 (1152 samples: u16's level-1 case) and the case's own samples repeated, which keeps the oracle's share
    of the test at a second."""
    if name == "u16" and how == "aligned":
        level = 1
    g = geo(shape, dt, level)
    if how == "aligned":
        head = np.ascontiguousarray(np.tile(g.x, (1, -(-g.B // g.n)))[:, : g.B]) if name == "u16" else _other(g, 31, g.B)
        parts = [head, g.x]
    else:
        parts = [g.x, _other(g, 32, 23), g.x[:, : g.n // 2]]
    stores = []
    for p in parts:
        enc = (g.blob, g.st, g.nb) if p is g.x else _oracle_encode(oracle, p, level)
        stores.append(tuple(_dev(torch, a) for a in enc) + (p.shape[1],))
    got = fa.join_flac_device(stores, level=level, is_int64=g.wide, verify=True)
    whole = np.concatenate(parts, axis=1)
    _assert_store(got, _oracle_encode(oracle, whole, level), "join " + how)
    _clean(fa, torch, got, whole.shape[1], g.wide, g.B)


@ops
def test_reindex(fa, torch, geo, name, shape, dt, level):
    """The store in libFLAC's layout (no SEEKTABLE, STREAMINFO last) adopted: the oracle's store again, byte for byte."""
    g = geo(shape, dt, level)
    foreign = tuple(_dev(torch, a) for a in WC.strip_seektables(g.blob, g.st, g.nb, g.nf))
    got = fa.reindex_flac_device(*foreign, g.n, is_int64=g.wide, verify=True)
    _assert_store(got, (g.blob, g.st, g.nb), "reindex")


def _digests(x):
    return np.array([np.frombuffer(hashlib.md5(row.tobytes()).digest(), np.uint8) for row in x])


@ops
def test_md5_sign_and_check(fa, torch, geo, name, shape, dt, level):
    """md5_device, sign_streams_device and check_md5_device against hashlib over every stream; stream n - 2 then gets a
    wrong signature and is the only one that fails."""
    g = geo(shape, dt, level)
    want = _digests(g.x)
    comp, st, nb = _up_store(torch, g)
    dig = fa.md5_device(_dev(torch, g.x))
    assert np.array_equal(_host(dig), want)
    status = fa.check_md5_device(comp, st, nb, g.n, is_int64=g.wide)
    assert bool((status == -1).all())  # unsigned
    signed = fa.sign_streams_device(comp.clone(), st, dig)
    blob = g.blob.copy()
    blob[g.st[:, None] + 26 + np.arange(16)[None, :]] = want
    assert np.array_equal(_host(signed), blob)
    signed[int(g.st[g.ns - 2]) + 30] ^= 0x40
    status, got = fa.check_md5_device(signed, st, nb, g.n, is_int64=g.wide, return_digests=True)
    expect = np.ones(g.ns, dtype=np.int8)
    expect[g.ns - 2] = 0
    assert np.array_equal(_host(status).reshape(-1), expect) and np.array_equal(_host(got), want)


@ops
def test_compare(fa, torch, geo, name, shape, dt, level):
    """compare_flac_device and FlacArray.first_mismatch with one sample changed in stream n_stream - 2."""
    g = geo(shape, dt, level)
    comp, st, nb = _up_store(torch, g)
    data = g.x.copy()
    assert np.all(_host(fa.compare_flac_device(comp, st, nb, _dev(torch, data))) == -1)
    at = g.n - 2
    data[g.ns - 2, at] += 1
    want = np.full(g.ns, -1, dtype=np.int64)
    want[g.ns - 2] = at
    dd = _dev(torch, data)
    assert np.array_equal(_host(fa.compare_flac_device(comp, st, nb, dd)).reshape(-1), want)
    arr = fa.FlacArray(None, shape=g.x.shape, compressed=g.blob, dtype=g.x.dtype, stream_starts=g.st, stream_nbytes=g.nb)
    assert np.array_equal(np.asarray(_host(arr.first_mismatch(dd))).reshape(-1), want)


def _binned(x, width, op):
    return op.reduceat(x, np.arange(0, x.shape[1], width), axis=1)


@pytest.mark.parametrize("width", [None, 5])
@ops
def test_reduce(fa, torch, geo, name, shape, dt, level, width):
    """Binned min / max / sum (and, for one-channel streams, the two limbs of the sum of squares) against numpy on int64."""
    g = geo(shape, dt, level)
    mn, mx, sm, qh, ql = fa.reduce_flac_device(*_up_store(torch, g), g.n, width=width, is_int64=g.wide, verify=True)
    x = g.x.astype(np.int64)
    w = g.n if width is None else width
    assert np.array_equal(_host(mn), _binned(x, w, np.minimum)) and np.array_equal(_host(mx), _binned(x, w, np.maximum))
    with np.errstate(over="ignore"):
        assert np.array_equal(_host(sm), _binned(x, w, np.add))  # (two-channel streams: modulo 2^64, as numpy's int64 wraps)
    if not g.wide:
        sq = x * x
        assert np.array_equal(_host(ql), _binned(sq & 0xFFFFFFFF, w, np.add)) and np.array_equal(_host(qh), _binned(sq >> 32, w, np.add))


@ops
def test_salvage(fa, torch, geo, name, shape, dt, level):
    """The last frame of streams 0, 1023, 1024, 65 536 (where there is one) and the last stream damaged: the damage map is
    non-zero exactly there, those frames come back as the fill value and every other sample as the oracle's input."""
    g = geo(shape, dt, level)
    hit = sorted({s for s in (0, 1023, 1024, 65536) if s < g.ns} | {g.ns - 1})
    blob = g.blob.copy()
    for s in hit:
        blob[g.st[s] + g.nb[s] - 3] ^= 0x20  # (the last payload byte in front of the last frame's CRC-16)
    out, status = fa.decode_flac_salvage_device(_dev(torch, blob), _dev(torch, g.st), _dev(torch, g.nb), g.n, is_int64=g.wide, fill=-7,
                                                block_size=g.B)
    status = _host(status).reshape(g.ns, g.nf)
    want = np.zeros((g.ns, g.nf), dtype=bool)
    want[hit, g.nf - 1] = True
    assert np.array_equal(status != 0, want)
    x = g.x.copy()
    x[hit, (g.nf - 1) * g.B :] = -7
    assert np.array_equal(_host(out), x)
    arr = fa.FlacArray(None, shape=g.x.shape, compressed=blob, dtype=g.x.dtype, stream_starts=g.st, stream_nbytes=g.nb)
    assert np.array_equal(arr.frame_status() != 0, want)


# ------------------------------------------------------------------------------------------------------ float stores

QCAP = WC.GEOMETRIES["qcap"]["cases"]


@pytest.mark.parametrize("op", ["append", "overwrite"])
@pytest.mark.parametrize("shape,dt,level", QCAP, ids=[c[1] for c in QCAP])
def test_float_splice_on_qcap(fa, torch, oracle, geo, shape, dt, level, op):
    """float32 / float64 append and overwrite of 70 001 x 241 samples (quantise_rows_kernel's second trip).  The new floats
    are the store's own rows reversed: they lie inside each stream's range, so the oracle quantises old and new samples
    together with the very offsets and gains of the store -- asserted -- and its integers are the expected ones."""
    g = geo(shape, dt, level)
    quant = oracle.float64_to_int64 if g.wide else oracle.float32_to_int32
    new = np.ascontiguousarray(g.f[:, ::-1])
    both, off, gain = quant(np.concatenate([g.f, new], axis=1), g.q)
    assert off.tobytes() == g.off.tobytes() and gain.tobytes() == g.gain.tobytes() and np.array_equal(both[:, : g.n], g.x)
    store = _up_store(torch, g)
    scale = dict(offsets=_dev(torch, g.off), gains=_dev(torch, g.gain))
    if op == "append":
        got = fa.append_flac_device(*store, g.n, _dev(torch, new), level=level, verify=True, **scale)
        want, n_new = both, 2 * g.n
    else:
        got = fa.overwrite_flac_device(*store, g.n, 0, _dev(torch, new), level=level, verify=True, **scale)
        want, n_new = both[:, g.n :], g.n
    _assert_store(got, _oracle_encode(oracle, np.ascontiguousarray(want), level), "float " + op)
    _clean(fa, torch, got, n_new, g.wide, g.B)


@pytest.mark.parametrize("dt", ["f32", "f64"])
def test_std_and_precision_on_u16_floats(fa, torch, oracle, dt):
    """std_device (the stream_chunk_sum / fold pair over 70 001 streams of 19 samples) against np.std bit for bit, and
    from_device_array(precision=) against the oracle's quantisation and encode with the quanta numpy's std gives."""
    from flacarray_amd.utils import _quanta_for

    ns, n = WC.GEOMETRIES["u16"]["cases"][0][0]
    ndt = np.float32 if dt == "f32" else np.float64
    f = WC.wide_floats(ns, n, ndt, 0)
    f = f[np.std(f, axis=-1) > 0]  # (a constant row has no precision-derived quantum; 69 000 streams and more stay)
    assert f.shape[0] > 65536 + 256
    fd = _dev(torch, f)
    assert _host(fa.std_device(fd)).tobytes() == np.std(f, axis=-1).tobytes()
    arr = fa.FlacArray.from_device_array(fd, level=5, precision=3)
    q = _quanta_for(f, (f.shape[0],), None, 3)
    ints, off, gain = (oracle.float64_to_int64 if dt == "f64" else oracle.float32_to_int32)(f, q)
    assert np.asarray(arr.stream_offsets).tobytes() == off.tobytes() and np.asarray(arr.stream_gains).tobytes() == gain.tobytes()
    _assert_store((arr.compressed, arr.stream_starts, arr.stream_nbytes), _oracle_encode(oracle, ints, 5), "precision")


# ------------------------------------------------------------------------------------------------------- k3f_tailcap

def test_k3f_tailcap(fa, torch, oracle):
    """(131 075, 8196) int32, level 5: K3F with a short last frame per stream -- the tail encoder with grid = n_stream and the
    second trip of the tail compaction.  4.3 GB of input, too large for a full oracle pass: it is generated on the device
    (wide_rows against torch), and ALL streams must satisfy: starts are the exclusive scan of nbytes and end at the blob
    size; compare_flac_device against the input reports no mismatch; frame_status is all zero; a verified whole decode
    equals the input.  64 of the 131 075 streams -- 0, 1, 1023, 1024, 65 535, 65 536, 131 071, 131 072, 131 073, the last
    two, and seeded random ones -- are made again on the host and must equal the oracle's encode of that row alone byte for
    byte (a stream's bytes do not depend on its neighbours): that is all the oracle sees of this case."""
    (ns, n), _, level = WC.GEOMETRIES["k3f_tailcap"]["cases"][0]
    xd = torch.empty((ns, n), dtype=torch.int32, device="cuda")
    for lo in range(0, ns, 8192):
        rows = np.arange(lo, min(lo + 8192, ns))
        xd[lo : lo + rows.size] = WC.wide_rows(ns, n, False, 0, rows=rows, xp=torch, device="cuda")
    comp, st, nb = fa.encode_flac_device(xd, level=level)
    torch.cuda.synchronize()
    st_h, nb_h = _host(st).reshape(-1), _host(nb).reshape(-1)
    assert st_h[0] == 0 and np.array_equal(st_h[1:], np.cumsum(nb_h)[:-1]) and st_h[-1] + nb_h[-1] == comp.numel()
    assert int(torch.count_nonzero(fa.compare_flac_device(comp, st, nb, xd) + 1)) == 0
    assert int(torch.count_nonzero(fa.frame_status_device(comp, st, nb, n, block_size=4096))) == 0
    y = fa.decode_flac_device(comp, st, nb, n, verify=True)
    assert torch.equal(y, xd)
    del y
    fixed = [0, 1, 1023, 1024, 65535, 65536, 131071, 131072, 131073, ns - 2, ns - 1]
    rng = np.random.default_rng(5)
    rows = list(fixed)
    while len(rows) < 64:
        r = int(rng.integers(0, ns))
        if r not in rows:
            rows.append(r)
    rows = np.array(rows)
    x = WC.wide_rows(ns, n, False, 0, rows=rows)
    assert np.array_equal(_host(xd[torch.as_tensor(rows, device="cuda")]), x)
    for k, s in enumerate(rows):
        blob_o, _, nb_o = oracle.encode_i32(x[k : k + 1], level)
        assert nb_h[s] == nb_o[0], "stream %d: %d bytes, oracle %d" % (s, nb_h[s], nb_o[0])
        assert np.array_equal(_host(comp[int(st_h[s]) : int(st_h[s] + nb_h[s])]), blob_o), "stream %d" % s
