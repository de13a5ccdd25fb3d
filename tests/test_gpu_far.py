"""Far offsets on every device path (tests/far_corpus.py; the thresholds are asserted on the CPU by tests/test_far_corpus.py).

Part A: the streams of a kit lie in a sparse blob of 2^32 + 2^20 bytes, around byte 2^31 and 2^32, behind an index that
        is not sorted by address, with decoys where a start truncated to 32 bits would land.
Part B: packed stores of full-range noise whose blob passes 1.25 * 2^32 bytes: every writer's output side.
Part C: streams of more than 2^16 frames and of more than 2^31 samples: zeros with a few frames of noise.

References: the CPU oracle, hashlib.md5 and numpy.  Where a far store is compared with "the same call on the compact
packing", the compact result is itself compared with the oracle in the same test or is what the other GPU modules pin.
Everything is exact: bytes, starts, nbytes, samples as bits, status bytes, digests.
"""
import hashlib
import time

import numpy as np
import pytest

from tests import far_corpus as FC
from tests.golden import flac_writer as W

pytestmark = pytest.mark.gpu

DISPATCH_VARS = ("FLACARRAY_HIP_PLACED_BELOW", "FLACARRAY_HIP_LATENCY", "FLACARRAY_HIP_SLOTS", "FLACARRAY_HIP_VERIFY_AFTER",
                 "FLACARRAY_HIP_NO_SYNC_SCAN", "FLACARRAY_HIP_PLACED_GRID")
ROLE = {r: i for i, r in enumerate(FC.ROLES)}


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
def _own_dispatch(monkeypatch, request):
    """Every test starts from the default dispatch; its wall time and peak device memory are printed (profiles/far.md)."""
    import torch

    for v in DISPATCH_VARS:
        monkeypatch.delenv(v, raising=False)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    t0 = time.perf_counter()
    yield
    torch.cuda.synchronize()
    print("\nFAR %s: %.2f s, peak %.2f GB" % (request.node.name, time.perf_counter() - t0, torch.cuda.max_memory_allocated() / 1e9))


def _dev(torch, a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _host(t):
    return t.cpu().numpy() if hasattr(t, "cpu") else np.asarray(t)


def _bits(a):
    a = _host(a)
    return a.view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize]) if a.dtype.kind == "f" else a


def _same_store(torch, got, want, what):
    """Two device triples: sizes, starts, then bytes."""
    assert torch.equal(got[2].reshape(-1), want[2].reshape(-1)), what + ": nbytes differ"
    assert torch.equal(got[1].reshape(-1), want[1].reshape(-1)), what + ": starts differ"
    assert got[0].numel() == want[0].numel() and torch.equal(got[0], want[0]), what + ": bytes differ"


def _is_oracle_store(got, want, what):
    blob, st, nb = (_host(t).reshape(-1) for t in got[:3])
    wb, wst, wnb = (np.asarray(t).reshape(-1) for t in want)
    assert np.array_equal(nb, wnb), "%s: nbytes %s, oracle %s" % (what, nb[:8], wnb[:8])
    assert np.array_equal(st, wst), "%s: starts differ" % what
    assert blob.size == wb.size and np.array_equal(blob, wb), "%s: bytes differ, first at %s" % (
        what, np.flatnonzero(blob[: wb.size] != wb[: blob.size])[:1])


def _oracle_encode(oracle, x, level):
    return (oracle.encode_i64 if x.dtype == np.int64 else oracle.encode_i32)(np.ascontiguousarray(x), level)


# ===================================================================================================== Part A: far bytes

@pytest.fixture(scope="module")
def kits(oracle):
    made = {}

    def get(name):
        if name not in made:
            made[name] = FC.Kit(name, oracle, W, hashlib.md5)
        return made[name]

    yield get
    made.clear()


@pytest.fixture(scope="module")
def far_blob(torch):
    blob = torch.full((FC.BLOB_BYTES,), FC.FILL, dtype=torch.uint8, device="cuda")
    assert blob.data_ptr() % 16 == 0
    yield blob
    del blob
    torch.cuda.empty_cache()


class Placed:
    """A kit's streams written into the blob under one layout: `far` = (blob, starts, nbytes) of rows 0 .. ROWS - 1 in the
    blob, `near` = the compact packing of the same rows.  Leaving the context puts the filler back."""

    def __init__(self, torch, blob, kit, layout):
        self.torch, self.blob, self.kit = torch, blob, kit
        self.st = kit.starts(layout)
        assert blob.numel() == FC.BLOB_BYTES and self.st.min() >= 0 and (self.st + kit.nb).max() <= FC.BLOB_BYTES

    def __enter__(self):
        k = self.kit
        for s, p in zip(k.streams, self.st):
            self.blob[int(p) : int(p) + s.size] = _dev(self.torch, s)
        self.far = (self.blob, _dev(self.torch, self.st[: FC.ROWS]), _dev(self.torch, k.nb[: FC.ROWS]))
        self.near = tuple(_dev(self.torch, a) for a in k.compact)
        return self

    def __exit__(self, *exc):
        for s, p in zip(self.kit.streams, self.st):
            self.blob[int(p) : int(p) + s.size] = FC.FILL
        return False


ALL = [(name, layout) for name in FC.KITS for layout in FC.LAYOUTS]
OWN = [(name, layout) for name, layout in ALL if FC.KITS[name][3] in ("own", "signed")]
STRIPPED = [(name, layout) for name, layout in ALL if FC.KITS[name][3] == "stripped"]
_ids = lambda cases: ["%s-%s" % c for c in cases]  # noqa: E731
every_kit = pytest.mark.parametrize("name,layout", ALL, ids=_ids(ALL))
own_kits = pytest.mark.parametrize("name,layout", OWN, ids=_ids(OWN))
stripped_kits = pytest.mark.parametrize("name,layout", STRIPPED, ids=_ids(STRIPPED))


def _store_rows(k):
    return k.x[: FC.ROWS]


def _range(n):
    return n // 3, n - n // 4


@every_kit
def test_far_decode(fa, torch, oracle, kits, far_blob, monkeypatch, name, layout):
    """Whole and ranged decode, verify off and on, through K7 (FLACARRAY_HIP_LATENCY=0) and K7L (=1); a stripped kit also
    with the serial walk instead of the sync scan; the float kit also restored."""
    k = kits(name)
    x = _store_rows(k)
    lo, hi = _range(k.n)
    with Placed(torch, far_blob, k, layout) as p:
        locators = ("scan", "walk") if k.layout == "stripped" else ("scan",)
        for locator in locators:
            if locator == "walk":
                monkeypatch.setenv("FLACARRAY_HIP_NO_SYNC_SCAN", "1")
            for lat in ("0", "1"):
                monkeypatch.setenv("FLACARRAY_HIP_LATENCY", lat)
                for verify in (False, True):
                    what = (locator, lat, verify)
                    y = fa.decode_flac_device(*p.far, k.n, is_int64=k.wide, verify=verify)
                    assert np.array_equal(_host(y), x), what
                    y = fa.decode_flac_device(*p.far, k.n, lo, hi, is_int64=k.wide, verify=verify)
                    assert np.array_equal(_host(y), x[:, lo:hi]), what
                    if k.f is not None:
                        off, gain = _dev(torch, k.off[: FC.ROWS]), _dev(torch, k.gain[: FC.ROWS])
                        y = fa.decode_flac_device(*p.far, k.n, lo, hi, offsets=off, gains=gain, verify=verify)
                        want = oracle.int32_to_float32(x, k.off[: FC.ROWS], k.gain[: FC.ROWS])[:, lo:hi]
                        assert np.array_equal(_bits(y), _bits(np.ascontiguousarray(want))), what


def _slices(k):
    """For every row: a slice across the second frame's end (where the straddling rows meet their mark), a few samples of
    the last frame, the first sample, and the whole row; shuffled."""
    ss, ff, cc = [], [], []
    for s in range(FC.ROWS):
        for f, c in ((2 * k.B - 40, 100), (k.n - 9, 9), (0, 1), (0, k.n), (k.B + 5, 7)):
            ss.append(s), ff.append(f), cc.append(c)
    order = np.random.default_rng(5).permutation(len(ss))
    ss, ff, cc = (np.array(v, dtype=np.int64)[order] for v in (ss, ff, cc))
    want = np.concatenate([k.x[s, f : f + c] for s, f, c in zip(ss, ff, cc)])
    return ss, ff, cc, want


def _reduce_want(x, first, last, width):
    x = x[:, first:last].astype(np.int64)
    edges = np.arange(0, x.shape[1], width)
    with np.errstate(over="ignore"):
        out = [np.minimum.reduceat(x, edges, axis=1), np.maximum.reduceat(x, edges, axis=1), np.add.reduceat(x, edges, axis=1)]
        sq = x * x
    return out + [np.add.reduceat(sq >> 32, edges, axis=1), np.add.reduceat(sq & 0xFFFFFFFF, edges, axis=1)]


def _check_reduce(got, x, first, last, width, wide, what):
    want = _reduce_want(x, first, last, width)
    for i, key in enumerate(("min", "max", "sum")):
        assert np.array_equal(_host(got[i]), want[i]), "%s: %s" % (what, key)
    if not wide:
        assert np.array_equal(_host(got[3]), want[3]) and np.array_equal(_host(got[4]), want[4]), "%s: sum of squares" % what


@every_kit
def test_far_slices_and_index(fa, torch, kits, far_blob, name, layout):
    """decode_slices_device; DeviceDecodeIndex.decode, decode_slices (to the device and to the host) and reduce."""
    k = kits(name)
    x = _store_rows(k)
    ss, ff, cc, want = _slices(k)
    lo, hi = _range(k.n)
    with Placed(torch, far_blob, k, layout) as p:
        got, _ = fa.decode_slices_device(*p.far, k.n, ss, ff, cc, is_int64=k.wide)
        assert np.array_equal(_host(got), want)
        got, _ = fa.decode_slices_device(*p.far, k.n, ss, ff, cc, is_int64=k.wide, verify=True)
        assert np.array_equal(_host(got), want)
        index = fa.DeviceDecodeIndex(*p.far, k.n, is_int64=k.wide)
        try:
            assert np.array_equal(_host(index.decode()), x)
            assert np.array_equal(_host(index.decode(lo, hi, verify=True)), x[:, lo:hi])
            got, _ = index.decode_slices(ss, ff, cc)
            assert np.array_equal(_host(got), want)
            got, _ = index.decode_slices(ss, ff, cc, to_host=True, verify=True)
            assert np.array_equal(got, want)
            _check_reduce(index.reduce(width=1000), x, 0, k.n, 1000, k.wide, "index.reduce")
        finally:
            index.close()


@every_kit
def test_far_reduce(fa, torch, kits, far_blob, name, layout):
    k = kits(name)
    x = _store_rows(k)
    with Placed(torch, far_blob, k, layout) as p:
        for width in (1000, 33):
            got = fa.reduce_flac_device(*p.far, k.n, width=width, is_int64=k.wide, verify=True)
            _check_reduce(got, x, 0, k.n, width, k.wide, "width %d" % width)
        picks = np.array([ROLE["B"], ROLE["L"], ROLE["E"]])
        got = fa.reduce_flac_device(*p.far, k.n, width=33, first_sample=k.B - 3, last_sample=k.n - 1, streams=picks, is_int64=k.wide)
        _check_reduce(got, x[picks], k.B - 3, k.n - 1, 33, k.wide, "picked streams")


@every_kit
def test_far_compare(fa, torch, kits, far_blob, name, layout):
    """The compare sink: equal data gives -1 everywhere; one changed sample in each of the rows at the 2^32 mark and at the
    blob's end (behind the straddled mark in row B) is found at its position, every other row stays -1."""
    k = kits(name)
    with Placed(torch, far_blob, k, layout) as p:
        if k.f is not None:
            data, scale = k.f[: FC.ROWS].copy(), (_dev(torch, k.off[: FC.ROWS]), _dev(torch, k.gain[: FC.ROWS]))
            step = 16 * k.q[: FC.ROWS]
        else:
            data, scale, step = _store_rows(k).copy(), (), np.ones(FC.ROWS, dtype=k.x.dtype)
        assert np.all(_host(fa.compare_flac_device(*p.far, _dev(torch, data), *scale)) == -1)
        want = np.full(FC.ROWS, -1, dtype=np.int64)
        for row, at in ((ROLE["B"], 2 * k.B + 11), (ROLE["E"], k.n - 2)):
            data[row, at] += step[row]
            want[row] = at
        assert np.array_equal(_host(fa.compare_flac_device(*p.far, _dev(torch, data), *scale)).reshape(-1), want)


def _digests(x):
    return np.array([np.frombuffer(hashlib.md5(np.ascontiguousarray(row).tobytes()).digest(), np.uint8) for row in x])


@every_kit
def test_far_md5(fa, torch, kits, far_blob, name, layout):
    """check_md5_device (signed kits and the writer's streams: 1 and hashlib's digests; the others: -1), then
    sign_streams_device in place on a copy of the blob: the whole image equals the expected one, in which only the 16
    digest bytes of each indexed stream differ from the blob, and the signed store checks."""
    k = kits(name)
    x = _store_rows(k)
    want = _digests(x)
    signed_already = k.layout in ("signed", "writer")
    with Placed(torch, far_blob, k, layout) as p:
        status, dig = fa.check_md5_device(*p.far, k.n, is_int64=k.wide, return_digests=True)
        assert np.all(_host(status) == (1 if signed_already else -1))
        if signed_already:
            assert np.array_equal(_host(dig), want)
        new = _digests(x[::-1]) if signed_already else want  # (a signed kit is signed again with other digests)
        image = p.far[0].clone()
        at = torch.from_numpy(p.st[: FC.ROWS, None] + 26 + np.arange(16)[None, :]).cuda()
        image[at] = _dev(torch, new)
        mine = p.far[0].clone()
        assert fa.sign_streams_device(mine, p.far[1], _dev(torch, new)) is mine
        assert torch.equal(mine, image)
        status, dig = fa.check_md5_device(mine, p.far[1], p.far[2], k.n, is_int64=k.wide, return_digests=True, verify=True)
        assert np.all(_host(status) == (0 if signed_already else 1)) and np.array_equal(_host(dig), want)
        del image, mine


@own_kits
def test_far_damage(fa, torch, kits, far_blob, name, layout):
    """frame_status_device is all zero; with one byte of the stored CRC-16 of the second frame of row B (the frame the
    straddled mark lies in) and of the last frame of row E flipped, exactly those two frames show FRAME_CRC16, and
    decode_flac_salvage_device returns them as the fill value and every other sample intact."""
    k = kits(name)
    x = _store_rows(k)
    with Placed(torch, far_blob, k, layout) as p:
        status = fa.frame_status_device(*p.far, k.n, is_int64=k.wide, block_size=k.B)
        assert status.shape == (FC.ROWS, k.nf) and int(torch.count_nonzero(status)) == 0
        hits = [(ROLE["B"], 1, int(p.st[ROLE["B"]]) + k.second_end[ROLE["B"]] - 1), (ROLE["E"], k.nf - 1, FC.BLOB_BYTES - 2)]
        try:
            for _, _, byte in hits:
                far_blob[byte] ^= 0x10
            want = np.zeros((FC.ROWS, k.nf), dtype=np.uint8)
            for row, frame, _ in hits:
                want[row, frame] = fa.FRAME_CRC16
            assert np.array_equal(_host(fa.frame_status_device(*p.far, k.n, is_int64=k.wide, block_size=k.B)), want)
            out, status = fa.decode_flac_salvage_device(*p.far, k.n, is_int64=k.wide, fill=-7, block_size=k.B)
            assert np.array_equal(_host(status), want)
            patched = x.copy()
            for row, frame, _ in hits:
                patched[row, frame * k.B : (frame + 1) * k.B] = -7
            assert np.array_equal(_host(out), patched)
        finally:
            for _, _, byte in hits:
                far_blob[byte] ^= 0x10


@stripped_kits
def test_far_reindex(fa, torch, kits, far_blob, name, layout):
    """reindex_flac_device of the stripped kit read from the far blob: the own-layout kit, byte for byte."""
    k = kits(name)
    with Placed(torch, far_blob, k, layout) as p:
        got = fa.reindex_flac_device(*p.far, k.n, is_int64=k.wide, verify=True)
        _is_oracle_store(got, FC.pack(k.own[: FC.ROWS]), "reindex")


def _writer_scale(torch, k):
    return {} if k.f is None else dict(offsets=_dev(torch, k.off[: FC.ROWS]), gains=_dev(torch, k.gain[: FC.ROWS]))


@own_kits
def test_far_window(fa, torch, oracle, kits, far_blob, name, layout):
    """window_flac_device reading the far store: aligned, aligned with a re-encoded tail, a stream subset over the whole
    range (pure selection), the whole range, and an unaligned cut.  Each equals the same call on the compact packing; for
    the integer kits also the oracle's encode of the cut array (unsigned: the signed kit keeps its MD5 where streams are
    copied whole, which the compact call shows)."""
    k = kits(name)
    x = _store_rows(k)
    picks = np.array([ROLE["L"], ROLE["B"], ROLE["E"]])
    cases = [("aligned", k.B, 3 * k.B, None), ("tail", k.B, k.n - 5, None), ("subset", 0, k.n, picks), ("whole", 0, k.n, None),
             ("unaligned", 100, k.n - 3, picks)]
    with Placed(torch, far_blob, k, layout) as p:
        for what, first, last, streams in cases:
            got = fa.window_flac_device(*p.far, k.n, first, last, streams=streams, level=k.level, is_int64=k.wide, verify=True)
            near = fa.window_flac_device(*p.near, k.n, first, last, streams=streams, level=k.level, is_int64=k.wide)
            _same_store(torch, got, near, "window " + what)
            if k.layout == "own":
                rows = slice(None) if streams is None else streams
                _is_oracle_store(got, _oracle_encode(oracle, x[rows, first:last], k.level), "window " + what)


@own_kits
def test_far_join(fa, torch, oracle, kits, far_blob, name, layout):
    """join_flac_device of the far store with a near part, in both orders: [near block, far] takes the aligned route with
    the far store as its second source, [far, near] decodes and appends behind the far part."""
    k = kits(name)
    x = _store_rows(k)
    other = FC.kit_ints(name if k.f is None else "i32_l5", rows=FC.ROWS, n=k.B + 9, seed=1)
    block = tuple(_dev(torch, a) for a in _oracle_encode(oracle, other[:, : k.B], k.level)) + (k.B,)
    short = tuple(_dev(torch, a) for a in _oracle_encode(oracle, other, k.level)) + (k.B + 9,)
    with Placed(torch, far_blob, k, layout) as p:
        for what, parts, whole in (("near+far", [block, p.far + (k.n,)], np.concatenate([other[:, : k.B], x], axis=1)),
                                   ("far+near", [p.far + (k.n,), short], np.concatenate([x, other], axis=1))):
            got = fa.join_flac_device(parts, level=k.level, is_int64=k.wide, verify=True)
            _is_oracle_store(got, _oracle_encode(oracle, whole, k.level), "join " + what)


@own_kits
def test_far_splice(fa, torch, oracle, kits, far_blob, name, layout):
    """append_flac_device of 100 samples and overwrite_flac_device across the first frame boundary (all rows, and rows B and
    E only) on the far store: the same call on the compact packing, and the oracle's encode of the patched integers (the
    float kit takes floats, quantised with the store's offsets and gains)."""
    k = kits(name)
    x = _store_rows(k)
    new = FC.kit_ints(name if k.f is None else "i32_l5", rows=FC.ROWS, n=100, seed=2)
    new_dev = _dev(torch, new if k.f is None else (k.off[: FC.ROWS, None] + new * k.q[: FC.ROWS, None]).astype(np.float32))
    scale = _writer_scale(torch, k)
    picks = np.array([ROLE["E"], ROLE["B"]])
    first = k.B - 40
    with Placed(torch, far_blob, k, layout) as p:
        got = fa.append_flac_device(*p.far, k.n, new_dev, level=k.level, verify=True, **scale)
        _same_store(torch, got, fa.append_flac_device(*p.near, k.n, new_dev, level=k.level, **scale), "append")
        if k.f is None:
            _is_oracle_store(got, _oracle_encode(oracle, np.concatenate([x, new], axis=1), k.level), "append")
        for what, streams in (("all", None), ("picks", picks)):
            data = new_dev if streams is None else new_dev[torch.from_numpy(streams).cuda()].contiguous()
            got = fa.overwrite_flac_device(*p.far, k.n, first, data, streams=streams, level=k.level, verify=True, **scale)
            near = fa.overwrite_flac_device(*p.near, k.n, first, data, streams=streams, level=k.level, **scale)
            _same_store(torch, got, near, "overwrite " + what)
            if k.f is None and k.layout == "own":
                patched = x.copy()
                rows = slice(None) if streams is None else streams
                patched[rows, first : first + 100] = new[rows]
                _is_oracle_store(got, _oracle_encode(oracle, patched, k.level), "overwrite " + what)


# ========================================================================================= Part C: far frames and samples

class Sparse:
    """Zeros with a few frames of noise: `x` on the host, `xd` the same array built on the device."""

    def __init__(self, torch, n_stream, n, block, frames, seed):
        self.n, self.B, self.ns = n, block, n_stream
        self.nf = -(-n // block)
        self.noise = FC.sparse_frames(n_stream, n, block, frames, seed)
        self.x = FC.sparse_host(n_stream, n, block, self.noise)
        self.xd = torch.zeros((n_stream, n), dtype=torch.int32, device="cuda")
        for (s, f), v in self.noise.items():
            self.xd[s, f * block : f * block + v.size] = _dev(torch, v)


def _up(torch, enc):
    return tuple(_dev(torch, a) for a in enc)


def _strip_store(enc):
    return FC.pack([FC.strip_seektable(s) for s in FC.split(*enc)])


def _clean(fa, torch, store, n, B):
    status = fa.frame_status_device(store[0], store[1], store[2], n, block_size=B)
    assert status.shape[-1] == -(-n // B) and int(torch.count_nonzero(status)) == 0, "frame_status is not all zero"


@pytest.fixture(scope="module")
def c1(torch, oracle):
    """Level 1, two streams of 65 540 frames of 1152 (the last one short): frame numbers cross 2^16."""
    t0 = time.perf_counter()
    c = Sparse(torch, FC.C1_STREAMS, FC.C1_N, FC.C1_BLOCK, FC.C1_NOISE, seed=21)
    c.level = FC.C1_LEVEL
    c.enc = oracle.encode_i32(c.x, c.level, use_threads=True)
    c.store = _up(torch, c.enc)
    print("\nFAR fixture c1: %.2f s" % (time.perf_counter() - t0))
    yield c
    del c.xd, c.store
    torch.cuda.empty_cache()


C1_CROSS = 65536 * FC.C1_BLOCK  # the first sample of frame 65536


def test_c1_frame_number_fields(c1):
    """The oracle's stream: frame 65535 carries a 3-byte number (ef bf bf), frame 65536 a 4-byte one (f0 90 80 80)."""
    s = FC.split(*c1.enc)[0]
    spans = FC.frame_spans(s, c1.nf)
    assert bytes(s[spans[65535][0] + 4 : spans[65535][0] + 7]) == b"\xef\xbf\xbf"
    assert bytes(s[spans[65536][0] + 4 : spans[65536][0] + 8]) == b"\xf0\x90\x80\x80"


@pytest.mark.parametrize("route", ["default", "slots"])
def test_c1_encode(fa, torch, c1, monkeypatch, route):
    if route == "slots":
        monkeypatch.setenv("FLACARRAY_HIP_SLOTS", "1")
    got = fa.encode_flac_device(c1.xd, level=c1.level)
    _is_oracle_store(got, c1.enc, "encode " + route)


def _c1_slices(c):
    ss, ff, cc = [], [], []
    for s in range(c.ns):
        for f, n in ((C1_CROSS - 5, 10), (C1_CROSS, 1152), (C1_CROSS + 7, 3), (C1_CROSS - 1152, 2 * 1152 + 1), (c.n - 1052, 1052), (0, 5),
                     (65537 * 1152 + 100, 900)):
            ss.append(s), ff.append(f), cc.append(n)
    ss, ff, cc = (np.array(v, dtype=np.int64) for v in (ss, ff, cc))
    return ss, ff, cc, np.concatenate([c.x[s, f : f + n] for s, f, n in zip(ss, ff, cc)])


@pytest.mark.parametrize("layout", ["own", "stripped_scan", "stripped_walk"])
def test_c1_decode(fa, torch, c1, monkeypatch, layout):
    """Whole, ranged across frames 65535 | 65536, and slices around frame 65536 (few tasks: K7L takes them); the same
    without the SEEKTABLE, frames found by the sync scan and by the serial walk."""
    store = c1.store if layout == "own" else _up(torch, _strip_store(c1.enc))
    if layout == "stripped_walk":
        monkeypatch.setenv("FLACARRAY_HIP_NO_SYNC_SCAN", "1")
    y = fa.decode_flac_device(*store, c1.n, verify=True)
    assert torch.equal(y, c1.xd)
    del y
    lo, hi = C1_CROSS - 1152 - 5, C1_CROSS + 1152 + 7
    y = fa.decode_flac_device(*store, c1.n, lo, hi)
    assert np.array_equal(_host(y), c1.x[:, lo:hi])
    ss, ff, cc, want = _c1_slices(c1)
    got, _ = fa.decode_slices_device(*store, c1.n, ss, ff, cc, verify=True)
    assert np.array_equal(_host(got), want)
    index = fa.DeviceDecodeIndex(*store, c1.n)
    try:
        got, _ = index.decode_slices(ss, ff, cc, to_host=True)
        assert np.array_equal(got, want)
    finally:
        index.close()


def test_c1_append_overwrite(fa, torch, oracle, c1):
    """append onto a store that ends inside frame 65535: the new frames 65536 .. carry 4-byte numbers; overwrite of samples
    that span frames 65535 and 65536."""
    k = 65535 * 1152 + 300
    old = _up(torch, oracle.encode_i32(np.ascontiguousarray(c1.x[:, :k]), c1.level, use_threads=True))
    got = fa.append_flac_device(*old, k, c1.xd[:, k:].contiguous(), level=c1.level, verify=True)
    _is_oracle_store(got, c1.enc, "append")
    _clean(fa, torch, got, c1.n, c1.B)
    new = np.random.default_rng(3).integers(-2000, 2000, (c1.ns, 100)).astype(np.int32)
    patched = c1.x.copy()
    patched[:, C1_CROSS - 50 : C1_CROSS + 50] = new
    got = fa.overwrite_flac_device(*c1.store, c1.n, C1_CROSS - 50, _dev(torch, new), level=c1.level, verify=True)
    _is_oracle_store(got, oracle.encode_i32(patched, c1.level, use_threads=True), "overwrite")
    _clean(fa, torch, got, c1.n, c1.B)


@pytest.mark.parametrize("first", [1152, C1_CROSS], ids=["one_frame_off", "from_frame_65536"])
def test_c1_window(fa, torch, oracle, c1, first):
    """first = 1152: every frame number drops by one, frame 65536 becomes 65535 and its header shrinks by a byte;
    first = 65536 * 1152: the 4-byte numbers become 1-byte ones."""
    got = fa.window_flac_device(*c1.store, c1.n, first, c1.n, level=c1.level, verify=True)
    _is_oracle_store(got, oracle.encode_i32(np.ascontiguousarray(c1.x[:, first:]), c1.level, use_threads=True), "window")


def test_c1_join_and_reindex(fa, torch, oracle, c1):
    """A part of 65 535 frames joined with the rest: the second part's frame numbers are raised across 2^16; and reindex
    of the store without its SEEKTABLEs."""
    k = 65535 * 1152
    parts = [_up(torch, oracle.encode_i32(np.ascontiguousarray(a), c1.level, use_threads=True)) + (a.shape[1],) for a in (c1.x[:, :k], c1.x[:, k:])]
    got = fa.join_flac_device(parts, level=c1.level, verify=True)
    _is_oracle_store(got, c1.enc, "join")
    got = fa.reindex_flac_device(*_up(torch, _strip_store(c1.enc)), c1.n, verify=True)
    _is_oracle_store(got, c1.enc, "reindex")


def test_c1_checks(fa, torch, c1):
    """frame_status_device, check_md5_device (unsigned, then signed with hashlib's digests) and reduce with bins over the
    crossing."""
    _clean(fa, torch, c1.store, c1.n, c1.B)
    assert np.all(_host(fa.check_md5_device(*c1.store, c1.n)) == -1)
    want = _digests(c1.x)
    signed = fa.sign_streams_device(c1.store[0].clone(), c1.store[1], _dev(torch, want))
    status, dig = fa.check_md5_device(signed, c1.store[1], c1.store[2], c1.n, return_digests=True)
    assert np.all(_host(status) == 1) and np.array_equal(_host(dig), want)
    first, last = 65534 * 1152 + 7, 65538 * 1152 - 9
    got = fa.reduce_flac_device(*c1.store, c1.n, width=1000, first_sample=first, last_sample=last, verify=True)
    _check_reduce(got, c1.x, first, last, 1000, False, "reduce over the crossing")


@pytest.fixture(scope="module")
def c2(torch, oracle):
    """Level 5, one stream of 2^31 + 3 * 4096 + 20 samples (`enc20`) and its first 2^31 + 3 * 4096 + 17 (`enc17`)."""
    t0 = time.perf_counter()
    c = Sparse(torch, 1, FC.C2_N20, FC.C2_BLOCK, FC.C2_NOISE, seed=22)
    c.level = FC.C2_LEVEL
    c.enc20 = oracle.encode_i32(c.x, c.level)
    c.enc17 = oracle.encode_i32(c.x[:, : FC.C2_N17], c.level)
    c.store20, c.store17 = _up(torch, c.enc20), _up(torch, c.enc17)
    print("\nFAR fixture c2: %.2f s" % (time.perf_counter() - t0))
    yield c
    del c.xd, c.store20, c.store17, c.x
    torch.cuda.empty_cache()


def test_c2_encode(fa, torch, c2):
    """Both lengths equal the oracle: + 20 (whole frames and a tail) and + 17."""
    _is_oracle_store(fa.encode_flac_device(c2.xd, level=c2.level), c2.enc20, "encode + 20")
    _is_oracle_store(fa.encode_flac_device(c2.xd[:, : FC.C2_N17], level=c2.level), c2.enc17, "encode + 17")


def test_c2_decode_past_2_31(fa, torch, c2):
    """Ranged decode [2^31 - 10, n), slices that start past 2^31, and DeviceDecodeIndex the same."""
    n, lo = c2.n, FC.M31 - 10
    y = fa.decode_flac_device(*c2.store20, n, lo, n, verify=True)
    assert np.array_equal(_host(y), c2.x[:, lo:])
    ff = np.array([FC.M31 + 5, FC.M31 + 4096 - 3, n - 25, FC.M31 - 2, FC.M31 + 2 * 4096], dtype=np.int64)
    cc = np.array([100, 10, 25, 4, 4096 + 20], dtype=np.int64)
    ss = np.zeros(ff.size, dtype=np.int64)
    want = np.concatenate([c2.x[0, f : f + c] for f, c in zip(ff, cc)])
    got, _ = fa.decode_slices_device(*c2.store20, n, ss, ff, cc)
    assert np.array_equal(_host(got), want)
    index = fa.DeviceDecodeIndex(*c2.store20, n)
    try:
        assert np.array_equal(_host(index.decode(lo, n)), c2.x[:, lo:])
        got, _ = index.decode_slices(ss, ff, cc, verify=True)
        assert np.array_equal(_host(got), want)
        got, _ = index.decode_slices(ss, ff, cc, to_host=True)
        assert np.array_equal(got, want)
    finally:
        index.close()


def test_c2_compare_reduce_status(fa, torch, c2):
    """The compare sink finds a changed sample at a position past 2^31; reduce with first_sample, last_sample and bins past
    2^31; frame_status_device over 524 292 frames."""
    n = c2.n
    assert int(fa.compare_flac_device(*c2.store20, c2.xd)[0]) == -1
    at = FC.M31 + 4096 + 5
    data = c2.xd.clone()
    data[0, at] += 1
    assert int(fa.compare_flac_device(*c2.store20, data)[0]) == at
    del data
    first = FC.M31 - 100
    got = fa.reduce_flac_device(*c2.store20, n, width=1000, first_sample=first, last_sample=n - 3, verify=True)
    _check_reduce(got, c2.x, first, n - 3, 1000, False, "reduce past 2^31")
    got = fa.reduce_flac_device(*c2.store20, n, first_sample=FC.M31 + 5, last_sample=n)
    _check_reduce(got, c2.x, FC.M31 + 5, n, n - FC.M31 - 5, False, "one bin past 2^31")
    _clean(fa, torch, c2.store20, n, c2.B)
    torch.cuda.empty_cache()


def test_c2_window(fa, torch, oracle, c2):
    """first = 2^31 exactly: a 4-frame store that equals the oracle's encode of x[:, 2^31:]; first = 4096: every frame of
    the half-million is renumbered and the seek points past 2^31 are rebuilt."""
    got = fa.window_flac_device(*c2.store20, c2.n, FC.M31, c2.n, level=c2.level, verify=True)
    _is_oracle_store(got, oracle.encode_i32(np.ascontiguousarray(c2.x[:, FC.M31 :]), c2.level), "window at 2^31")
    got = fa.window_flac_device(*c2.store20, c2.n, 4096, c2.n, level=c2.level, verify=True)
    _is_oracle_store(got, oracle.encode_i32(c2.x[:, 4096:], c2.level), "window at 4096")


def test_c2_splice_and_join(fa, torch, oracle, c2):
    """append past 2^31: the + 17 store extended by the last three samples is the + 20 store.  overwrite past 2^31: twenty
    samples across a frame boundary replaced (checked by a decode and the damage map) and put back: the oracle's store
    again.  join of [0, 2^31) -- cut by window_flac_device, a truncate -- with the oracle's encode of the rest: the
    oracle's whole store."""
    n = c2.n
    got = fa.append_flac_device(*c2.store17, FC.C2_N17, c2.xd[:, FC.C2_N17 :].contiguous(), level=c2.level, verify=True)
    _is_oracle_store(got, c2.enc20, "append")
    first = FC.M31 + 4090
    new = np.random.default_rng(4).integers(-1000, 1000, (1, 20)).astype(np.int32)
    got = fa.overwrite_flac_device(*c2.store20, n, first, _dev(torch, new), level=c2.level, verify=True)
    patched = c2.x[:, FC.M31 :].copy()
    patched[:, 4090:4110] = new
    assert np.array_equal(_host(fa.decode_flac_device(*got, n, FC.M31, n, verify=True)), patched)
    _clean(fa, torch, got, n, c2.B)
    back = fa.overwrite_flac_device(*got, n, first, c2.xd[:, first : first + 20].contiguous(), level=c2.level, verify=True)
    _is_oracle_store(back, c2.enc20, "overwrite and back")
    del got, back
    head = fa.window_flac_device(*c2.store20, n, 0, FC.M31, level=c2.level, verify=True)
    tail = _up(torch, oracle.encode_i32(np.ascontiguousarray(c2.x[:, FC.M31 :]), c2.level))
    got = fa.join_flac_device([head + (FC.M31,), tail + (n - FC.M31,)], level=c2.level, verify=True)
    _is_oracle_store(got, c2.enc20, "join")
    torch.cuda.empty_cache()


# ============================================================================================ Part B: far bytes, written

VENDOR = b"reference libFLAC 1.4.3 20230623"


def _noise(torch, shape, seed):
    """Full-range int32 noise made on the device, a block of rows at a time."""
    g = torch.Generator(device="cuda")
    g.manual_seed(seed)
    out = torch.empty(shape, dtype=torch.int32, device="cuda")
    step = max(1, (1 << 27) // shape[1])
    for r in range(0, shape[0], step):
        rows = min(step, shape[0] - r)
        out[r : r + rows] = torch.randint(-(2**31), 2**31, (rows, shape[1]), generator=g, device="cuda", dtype=torch.int64).to(torch.int32)
    return out


def _b_checks(torch, oracle, store, rows_of, level, what):
    """The store checks of Part B: the blob passes 2^32 + 2^26 bytes, starts is the exclusive scan of nbytes and ends at the
    blob's size, and the spot rows (first, last, around each mark) are byte for byte the oracle's encode of that row
    alone; `rows_of(rows)` returns the expected samples of those rows as a host array."""
    comp, st, nb = store[0], store[1].reshape(-1), store[2].reshape(-1)
    assert comp.numel() >= FC.B_MIN_OUTPUT, "%s: %d bytes do not pass 2^32 + 2^26" % (what, comp.numel())
    assert int(st[0]) == 0 and torch.equal(torch.cumsum(nb, 0) - nb, st) and int(st[-1] + nb[-1]) == comp.numel(), what + ": starts"
    st_h, nb_h = _host(st), _host(nb)
    rows = FC.spot_rows(st_h, nb_h)
    assert any(st_h[r] < FC.M32 < st_h[r] + nb_h[r] or st_h[r] == FC.M32 for r in rows)
    x = rows_of(rows)
    for k, r in enumerate(rows):
        blob_o, _, nb_o = _oracle_encode(oracle, x[k : k + 1], level)
        assert nb_h[r] == nb_o[0], "%s: row %d has %d bytes, oracle %d" % (what, r, nb_h[r], nb_o[0])
        assert np.array_equal(_host(comp[int(st_h[r]) : int(st_h[r] + nb_h[r])]), blob_o), "%s: row %d differs from the oracle" % (what, r)
    return rows


def _rows_from(torch, xd):
    return lambda rows: _host(xd[torch.as_tensor(rows, device="cuda")])


@pytest.fixture(scope="module")
def b(fa, torch, oracle):
    """The first store: `b_stream_count` streams of 8 frames of 4096 samples of noise, level 5 (K3F)."""
    probe = np.random.default_rng(1).integers(-(2**31), 2**31, (1, FC.B_N), dtype=np.int64).astype(np.int32)

    class B:
        pass

    t0 = time.perf_counter()
    o = B()
    o.level, o.n = 5, FC.B_N
    o.ns = FC.b_stream_count(int(oracle.encode_i32(probe, 5)[2][0]))
    o.x = _noise(torch, (o.ns, o.n), 7)
    o.store = fa.encode_flac_device(o.x, level=5, compact=True)
    torch.cuda.synchronize()
    print("\nFAR fixture b: %.2f s, %d streams, %d bytes" % (time.perf_counter() - t0, o.ns, o.store[0].numel()))
    yield o
    del o.x, o.store
    torch.cuda.empty_cache()


def _expect(fa, torch, oracle, got, want_x, level, what):
    """`got` equals encode_flac_device of the expected samples as a whole, and passes the store checks."""
    want = fa.encode_flac_device(want_x, level=level)
    _same_store(torch, got, want, what)
    del want
    _b_checks(torch, oracle, got, _rows_from(torch, want_x), level, what)
    torch.cuda.empty_cache()


def test_b_first_store(fa, torch, oracle, b):
    """The K3F encode itself: the store checks, a whole decode, the compare sink and the damage map."""
    assert b.store[0].numel() > FC.B_MIN_BLOB
    rows = _b_checks(torch, oracle, b.store, _rows_from(torch, b.x), b.level, "first store")
    assert len(rows) >= 6
    y = fa.decode_flac_device(*b.store, b.n, verify=True)
    assert torch.equal(y, b.x)
    del y
    assert int(torch.count_nonzero(fa.compare_flac_device(*b.store, b.x) + 1)) == 0
    _clean(fa, torch, b.store, b.n, 4096)
    torch.cuda.empty_cache()


@pytest.mark.parametrize("what", ["tail", "truncate", "every_second"])
def test_b_window(fa, torch, oracle, b, what):
    """[4096, N - 5): the aligned route with a re-encoded tail; [0, N - 4096): a truncate; every second stream over the
    whole range: pure selection."""
    first, last, streams = {"tail": (4096, b.n - 5, None), "truncate": (0, b.n - 4096, None), "every_second": (0, b.n, np.arange(0, b.ns, 2))}[what]
    got = fa.window_flac_device(*b.store, b.n, first, last, streams=streams, level=b.level, verify=True)
    want_x = (b.x if streams is None else b.x[::2])[:, first:last].contiguous()
    _expect(fa, torch, oracle, got, want_x, b.level, "window " + what)


@pytest.mark.parametrize("cut", [4 * 4096, 7 * 4096], ids=["halves", "seven_and_one"])
def test_b_join(fa, torch, oracle, b, cut):
    parts = []
    for lo, hi in ((0, cut), (cut, b.n)):
        parts.append(tuple(fa.encode_flac_device(b.x[:, lo:hi].contiguous(), level=b.level, compact=True)) + (hi - lo,))
    got = fa.join_flac_device(parts, level=b.level, verify=True)
    del parts
    _same_store(torch, got, b.store, "join")
    _b_checks(torch, oracle, got, _rows_from(torch, b.x), b.level, "join")
    torch.cuda.empty_cache()


def test_b_append(fa, torch, oracle, b):
    new = _noise(torch, (b.ns, 100), 8)
    got = fa.append_flac_device(*b.store, b.n, new, level=b.level, verify=True)
    _expect(fa, torch, oracle, got, torch.cat([b.x, new], dim=1), b.level, "append")


def test_b_overwrite(fa, torch, oracle, b):
    new = _noise(torch, (b.ns, 110), 9)
    got = fa.overwrite_flac_device(*b.store, b.n, 4090, new, level=b.level, verify=True)
    want_x = b.x.clone()
    want_x[:, 4090:4200] = new
    _expect(fa, torch, oracle, got, want_x, b.level, "overwrite")


def _foreign_twin(torch, comp, st, nb, nf):
    """The own-layout store rewritten on the device into libFLAC's layout: per stream "fLaC" + STREAMINFO, a VORBIS_COMMENT
    marked last, the frames verbatim (no SEEKTABLE)."""
    vc = len(VENDOR).to_bytes(4, "little") + VENDOR + (0).to_bytes(4, "little")
    block = torch.from_numpy(np.frombuffer(bytes([0x84]) + len(vc).to_bytes(3, "big") + vc, dtype=np.uint8).copy()).cuda()
    hb = 46 + 18 * nf
    ns = st.numel()
    size = int(nb[0])
    assert bool((nb == size).all()) and comp.numel() == ns * size  # (noise: every frame VERBATIM, every stream one size)
    rows = comp.view(ns, size)
    out = torch.cat([rows[:, :42], block[None, :].expand(ns, -1), rows[:, hb:]], dim=1).reshape(-1)
    f_nb = torch.full_like(nb, size - hb + 42 + block.numel())
    return out, torch.cumsum(f_nb, 0) - f_nb, f_nb


def test_b_reindex(fa, torch, oracle, b):
    """The store in libFLAC's layout, built on the device, adopted: the first store again."""
    st, nb = b.store[1].reshape(-1), b.store[2].reshape(-1)
    foreign = _foreign_twin(torch, b.store[0], st, nb, FC.B_FRAMES)
    assert foreign[0].numel() >= FC.B_MIN_OUTPUT
    got = fa.reindex_flac_device(*foreign, b.n, verify=True)
    del foreign
    _same_store(torch, got, b.store, "reindex")
    _b_checks(torch, oracle, got, _rows_from(torch, b.x), b.level, "reindex")
    torch.cuda.empty_cache()


@pytest.mark.parametrize("route", ["level1", "odd_length", "int64", "slots"])
def test_b_encode_routes(fa, torch, oracle, b, monkeypatch, route):
    """The other integer encode routes once each on the same noise, viewed in the route's geometry without a copy: level 1
    and an odd length at level 5 (K3G), int64 at half the sample count, and the slot sequence (FLACARRAY_HIP_SLOTS=1).
    Each passes the store checks and decodes back whole."""
    level, x = 5, b.x
    if route == "level1":
        level = 1
    elif route == "odd_length":
        n = b.n - 3
        rows = b.x.numel() // n
        x = b.x.reshape(-1)[: rows * n].view(rows, n)
    elif route == "int64":
        x = b.x.view(torch.int64)
        assert x.shape == (b.ns, b.n // 2)
    else:
        monkeypatch.setenv("FLACARRAY_HIP_SLOTS", "1")
    store = fa.encode_flac_device(x, level=level)
    torch.cuda.synchronize()
    _b_checks(torch, oracle, store, _rows_from(torch, x), level, route)
    y = fa.decode_flac_device(*store, x.shape[1], is_int64=x.dtype == torch.int64, verify=True)
    assert torch.equal(y, x)
    del y, store
    torch.cuda.empty_cache()


def test_b_encode_f32_fused(fa, torch, oracle, b):
    """float32 through the fused path (quantised in K3F's staging load): 24-bit integers times a per-stream quantum, a
    third more streams than the first store since they take three bytes per sample.  Offsets, gains and the spot rows
    are the oracle's; the store decodes back to the oracle's integers."""
    ns = -(-b.ns * 4 // 3) + 8
    ints = _noise(torch, (ns, b.n), 10) >> 8
    q = (2.0**-12 * (1 + torch.arange(ns, device="cuda") % 3)).to(torch.float32)
    f = ints.to(torch.float32) * q[:, None]
    del ints
    comp, st, nb, off, gain = fa.encode_flac_device_f32(f, quanta=q, level=5)
    torch.cuda.synchronize()
    kept = {}

    def rows_of(rows):
        x, o, g = oracle.float32_to_int32(_host(f[torch.as_tensor(rows, device="cuda")]), _host(q)[rows])
        kept["rows"], kept["x"] = rows, x
        assert np.array_equal(_bits(off.reshape(-1)[torch.as_tensor(rows, device="cuda")]), _bits(o))
        assert np.array_equal(_bits(gain.reshape(-1)[torch.as_tensor(rows, device="cuda")]), _bits(g))
        return x

    _b_checks(torch, oracle, (comp, st, nb), rows_of, 5, "f32")
    y = fa.decode_flac_device(comp, st, nb, b.n, verify=True)
    assert np.array_equal(_host(y[torch.as_tensor(kept["rows"], device="cuda")]), kept["x"])
    ints2, off2, gain2 = fa.float32_to_int32_device(f, q)
    assert torch.equal(y, ints2) and torch.equal(off2.reshape(-1), off.reshape(-1)) and torch.equal(gain2.reshape(-1), gain.reshape(-1))
    del y, ints2, f, comp
    torch.cuda.empty_cache()
