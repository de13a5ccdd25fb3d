"""How a lane of the throughput decoder finds the first input chunk of its frame, and when a wave's loads and stores are
issued (profiles/k7_prefetch.md).  The chunk base is computed from the frame's OFFSET in the blob and from how far the blob
base lies behind a 64-byte boundary; a tile is stored at the start of the next macro step, the last one behind the loop.
What can go wrong with that is pinned here at the smallest shapes that reach it:

  * blob bases 0, 16, 32 and 48 bytes behind a 64-byte boundary (16 bytes is what the API guarantees; anything less is
    copied).  With streams that keep their SEEKTABLE the first frame lies beyond the first 64 bytes; without it frame 0 of
    stream 0 starts at byte 42, and with the base 16 bytes behind a boundary its chunk base would lie in front of the
    blob: the clamp (16 + 41 < 64).
  * the last frame ending 1, 15, 16 and 17 bytes before the end of a buffer of exactly that size: the 16-byte loads stay
    below the limit rounded up to 16.  The output is checked with the sentinel harness of the footprint tests.
  * 1, 63, 64, 65 and 129 frames (one to three waves, idle lanes), stream lengths 4096 k + {0, 4, 31, 32, 33} (a partial
    last tile, stored by the flush behind the loop) and sample ranges that start and end inside a tile.
  * every instantiation of the loop: int32, float32 restore, int64 (two channels), the compare sink (an encode with
    verify=True; one flipped sample), the reducing sink with a bin width that straddles frames -- on a store that has a
    VERBATIM frame, frames of 32 partitions and an impulse whose code is longer than any window, so that the
    out-of-line readers run too.

Everything is compared with the encoder's input, one stream also with the CPU decoder's output.  FLACARRAY_HIP_LATENCY=0
sends a decode through K7, =1 through the latency decoder, which hands back to K7 what it does not take."""
import numpy as np
import pytest

from tests import compare_corpus as C
from tests import decode_edges as E
from tests import encoder_corpus as K
from tests import quant_model as M
from tests.conftest import sinusoid_noise_i32, strip_seektable
from tests.test_gpu_decode_footprint import Harness

pytestmark = pytest.mark.gpu

B = 4096
SHIFTS = (0, 16, 32, 48)
LATENCY = pytest.mark.parametrize("latency", ["0", "1"], ids=["k7", "k7l"])


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
def L():
    from flacarray_amd import _lib

    return _lib.lib()


def place(torch, blob, shift, tail=0):
    """The blob on the device, `shift` bytes behind a 64-byte boundary, as a view of exactly blob.size + tail bytes (the
    tail holds 0xFF: a frame sync, if anything took it for input)."""
    blob = np.asarray(blob, dtype=np.uint8)
    base = torch.full((64 + blob.size + tail + 64,), 0xFF, dtype=torch.uint8, device="cuda")
    assert base.data_ptr() % 64 == 0
    view = base[shift : shift + blob.size + tail]
    view[: blob.size] = torch.from_numpy(blob).cuda()
    assert view.data_ptr() % 64 == shift and view.is_contiguous()
    return view


def dev(torch, a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


# ---------------------------------------------------------------------------------------------- blob base alignment

@pytest.fixture(scope="module")
def three(oracle):
    """3 streams x (2 * 4096 + 1000) samples at level 5: (data, with SEEKTABLE, without, the CPU decode of stream 0)."""
    n = 2 * B + 1000
    data = sinusoid_noise_i32(3, n, seed=811)
    full = tuple(np.asarray(x) for x in oracle.encode_i32(data, 5))
    bare = strip_seektable(*full)
    assert C._frame_offsets(full[0][: full[2][0]])[0] > 64 and bytes(bare[0][42:44]) == b"\xff\xf8"
    cpu0 = oracle.decode_i32(full[0], full[1][:1], full[2][:1], n)
    assert np.array_equal(cpu0.reshape(-1), data[0])
    return data, full, bare, cpu0.reshape(-1)


@LATENCY
@pytest.mark.parametrize("seektable", [True, False], ids=["seektable", "bare"])
@pytest.mark.parametrize("shift", SHIFTS)
def test_blob_base(torch, fa, monkeypatch, three, shift, seektable, latency):
    monkeypatch.setenv("FLACARRAY_HIP_LATENCY", latency)
    data, full, bare, cpu0 = three
    blob, st, nb = full if seektable else bare
    n = data.shape[1]
    comp, st_d, nb_d = place(torch, blob, shift), dev(torch, st), dev(torch, nb)
    y = fa.decode_flac_device(comp, st_d, nb_d, n).cpu().numpy()
    assert np.array_equal(y, data)
    assert np.array_equal(y[0], cpu0)
    # ... and a range that starts and ends inside a tile, in different frames
    y = fa.decode_flac_device(comp, st_d, nb_d, n, first_sample=B - 19, last_sample=2 * B + 45).cpu().numpy()
    assert np.array_equal(y, data[:, B - 19 : 2 * B + 45])


# ------------------------------------------------------------------------------------------------------ end of blob

@pytest.fixture(scope="module")
def own4096(oracle):
    return E.build_store("own4096", oracle)


@LATENCY
@pytest.mark.parametrize("entry", ["device", "indexed_grid"])
@pytest.mark.parametrize("tail", [1, 15, 16, 17])
def test_end_of_blob(torch, L, monkeypatch, own4096, tail, entry, latency):
    """The buffer handed in ends `tail` bytes behind the last frame; whole streams and the last frames alone, into a
    buffer of sentinel."""
    monkeypatch.setenv("FLACARRAY_HIP_LATENCY", latency)
    st = own4096._replace(blob=np.concatenate([own4096.blob, np.full(tail, 0xFF, dtype=np.uint8)]))
    assert int((st.starts + st.nbytes).max()) + tail == st.blob.size
    d = {"blob": torch.from_numpy(st.blob).cuda(), "starts": dev(torch, st.starts), "nbytes": dev(torch, st.nbytes), "offsets": None, "gains": None}
    assert d["blob"].numel() == st.blob.size and d["blob"].data_ptr() % 16 == 0
    h = Harness(torch, L, st, d, entry)
    try:
        h.window(0, st.n, 0, False)
        h.window(2 * st.block + 1, st.n, 1, False)
    finally:
        h.close()


# ---------------------------------------------------------------------------------------------- wave and tile edges

# (streams, samples): frames in all = streams x ceil(samples / 4096)
EDGE_SHAPES = {1: (1, B), 63: (21, 2 * B + 4), 64: (32, B + 32), 65: (13, 4 * B + 33), 129: (43, 2 * B + 31)}


def edge_ranges(n):
    """Ranges that start and end in the middle of a tile: inside one frame, across the first frame edge (where there is
    one), up to the partial last tile."""
    out = [(13, min(n, B) - 7), (n - 45, n - 1)]
    if n > B:
        out += [(B - 50, min(B + 45, n - 1)), (5, n - 3)]
    return out


@pytest.fixture(scope="module")
def edge_store(oracle):
    made = {}

    def get(frames):
        if frames not in made:
            rows, n = EDGE_SHAPES[frames]
            assert rows * -(-n // B) == frames
            data = sinusoid_noise_i32(rows, n, seed=820 + frames)
            made[frames] = (data,) + tuple(np.asarray(x) for x in oracle.encode_i32(data, 5))
        return made[frames]

    yield get
    made.clear()


@LATENCY
@pytest.mark.parametrize("frames", sorted(EDGE_SHAPES))
def test_wave_and_tile_edges(torch, fa, monkeypatch, edge_store, frames, latency):
    monkeypatch.setenv("FLACARRAY_HIP_LATENCY", latency)
    data, blob, st, nb = edge_store(frames)
    n = data.shape[1]
    comp, st_d, nb_d = place(torch, blob, 16), dev(torch, st), dev(torch, nb)
    assert np.array_equal(fa.decode_flac_device(comp, st_d, nb_d, n).cpu().numpy(), data)
    for first, last in edge_ranges(n):
        y = fa.decode_flac_device(comp, st_d, nb_d, n, first_sample=first, last_sample=last).cpu().numpy()
        assert np.array_equal(y, data[:, first:last]), (first, last)


# ------------------------------------------------------------------------------------- every instantiation of the loop

class Bits:
    def __init__(self, seg, at):
        self.seg, self.pos = seg, 8 * at

    def get(self, n):
        v = 0
        for _ in range(n):
            v = (v << 1) | ((int(self.seg[self.pos >> 3]) >> (7 - (self.pos & 7))) & 1)
            self.pos += 1
        return v


def subframe_kind(seg, at):
    """('verbatim' | 'constant' | 'fixed' | 'lpc', partition order or None) of the mono frame at seg[at:] (32-bit
    samples; a subframe with wasted bits is 'wasted')."""
    r = Bits(seg, at + C._header_bytes(seg, at))
    t = r.get(8)
    assert t & 0x80 == 0
    if t & 1:
        return "wasted", None
    tc = t >> 1
    if tc < 2:
        return ("constant", "verbatim")[tc], None
    order = tc - 8 if tc < 32 else (tc & 31) + 1
    r.get(32 * order)
    if tc >= 32:
        prec = r.get(4) + 1
        r.get(5 + prec * order)
    assert r.get(2) < 2
    return ("fixed" if tc < 32 else "lpc"), r.get(4)


@pytest.fixture(scope="module")
def mixed(oracle):
    """6 streams x (5 frames + 1000 samples) at level 5.  Stream s holds, in rotation s, a noise frame, a full-range frame
    (VERBATIM), a frame whose amplitude changes every 128 samples (32 partitions), a frame of nearly full range (VERBATIM
    as well) and an odd impulse in silence (in its partition of 128 samples a unary run of more than a hundred zeros: the
    out-of-line sample reader); the tail is the usual signal.  Returns (data, blob, starts, nbytes, CPU decode of stream 1)."""
    rows = 6
    tail = sinusoid_noise_i32(rows, 1000, seed=830)
    data = []
    for s in range(rows):
        fr = [K.noise_frame(840 + s), K.full_range_frame(850 + s), K.partition_frame(860 + s, 5), K.near_max_frame(870 + s), K.impulse_frame(1500 + 37 * s, value=(1 << 20) + 1)]
        data.append(np.concatenate(fr[s % 5 :] + fr[: s % 5] + [tail[s]]))
    data = np.ascontiguousarray(np.stack(data), dtype=np.int32)
    blob, st, nb = (np.asarray(x) for x in oracle.encode_i32(data, 5))
    seg = blob[st[0] : st[0] + nb[0]]
    at = C._frame_offsets(seg)
    assert subframe_kind(seg, at[1])[0] == "verbatim"
    assert subframe_kind(seg, at[2])[1] == 5 and subframe_kind(seg, at[4])[1] == 5, "32 partitions: the level's highest order"
    cpu1 = oracle.decode_i32(blob, st[1:2], nb[1:2], data.shape[1]).reshape(-1)
    assert np.array_equal(cpu1, data[1])
    return data, blob, st, nb, cpu1


@LATENCY
@pytest.mark.parametrize("shift", (0, 16))
def test_int32_and_float32(torch, fa, monkeypatch, mixed, shift, latency):
    monkeypatch.setenv("FLACARRAY_HIP_LATENCY", latency)
    data, blob, st, nb, cpu1 = mixed
    n = data.shape[1]
    comp, st_d, nb_d = place(torch, blob, shift), dev(torch, st), dev(torch, nb)
    y = fa.decode_flac_device(comp, st_d, nb_d, n).cpu().numpy()
    assert np.array_equal(y, data)
    assert np.array_equal(y[1], cpu1)
    r = np.arange(data.shape[0])
    off, gain = ((r % 7) * 0.25).astype(np.float32), (64.0 * (1 + r % 3)).astype(np.float32)
    want = M.int32_to_float32(data, off, gain)
    for first, last in ((-1, -1), (B + 13, 3 * B - 7)):
        y = fa.decode_flac_device(comp, st_d, nb_d, n, first_sample=first, last_sample=last, offsets=dev(torch, off), gains=dev(torch, gain))
        w = want if first < 0 else want[:, first:last]
        assert np.array_equal(y.cpu().numpy().view(np.uint32), np.ascontiguousarray(w).view(np.uint32))


@LATENCY
@pytest.mark.parametrize("shift", (0, 16))
def test_int64(torch, fa, oracle, monkeypatch, mixed, shift, latency):
    """Two channels: the low words are the mixed store's samples (VERBATIM first subframes among them), the high words a
    small signal."""
    monkeypatch.setenv("FLACARRAY_HIP_LATENCY", latency)
    low = mixed[0][:3, : 2 * B + 33]
    x = K.pack_i64(low, sinusoid_noise_i32(3, low.shape[1], seed=880, amp=2**6))
    x = np.ascontiguousarray(x, dtype=np.int64)
    blob, st, nb = (np.asarray(a) for a in oracle.encode_i64(x, 5))
    n = x.shape[1]
    comp, st_d, nb_d = place(torch, blob, shift), dev(torch, st), dev(torch, nb)
    assert np.array_equal(fa.decode_flac_device(comp, st_d, nb_d, n, is_int64=True).cpu().numpy(), x)
    y = fa.decode_flac_device(comp, st_d, nb_d, n, first_sample=B - 19, last_sample=2 * B + 5, is_int64=True).cpu().numpy()
    assert np.array_equal(y, x[:, B - 19 : 2 * B + 5])
    assert np.array_equal(oracle.decode_i64(blob, st[:1], nb[:1], n).reshape(-1), x[0])


def test_compare_sink(torch, fa, mixed):
    """An encode that verifies itself passes; against the input with one sample flipped, per stream at another edge, the
    compare sink names that sample."""
    data, blob, st, nb, _ = mixed
    n = data.shape[1]
    comp, st_v, nb_v = fa.encode_flac_device(dev(torch, data), level=5, verify=True)
    assert np.array_equal(comp.cpu().numpy(), blob) and np.array_equal(st_v.cpu().numpy().reshape(-1), st.reshape(-1))
    where = np.array([0, 31, B - 1, B + 32, 5 * B + 999, 3 * B + 13])
    flipped = data.copy()
    flipped[np.arange(data.shape[0]), where] ^= 1
    for shift in (0, 16):
        c, st_d, nb_d = place(torch, blob, shift), dev(torch, st), dev(torch, nb)
        assert np.array_equal(fa.compare_flac_device(c, st_d, nb_d, dev(torch, data)).cpu().numpy().reshape(-1), np.full(data.shape[0], -1))
        assert np.array_equal(fa.compare_flac_device(c, st_d, nb_d, dev(torch, flipped)).cpu().numpy().reshape(-1), where)
    assert n == 5 * B + 1000


def reduce_bins(x, first, last, width):
    seg = x[:, first:last].astype(np.int64)
    edges = list(range(0, seg.shape[1], width))
    mn = np.stack([seg[:, a : a + width].min(axis=1) for a in edges], axis=1)
    mx = np.stack([seg[:, a : a + width].max(axis=1) for a in edges], axis=1)
    sm = np.stack([seg[:, a : a + width].sum(axis=1) for a in edges], axis=1)
    q = (seg * seg).astype(np.uint64)
    qh = np.stack([(q[:, a : a + width] >> np.uint64(32)).sum(axis=1) for a in edges], axis=1).astype(np.int64)
    ql = np.stack([(q[:, a : a + width] & np.uint64(0xFFFFFFFF)).sum(axis=1) for a in edges], axis=1).astype(np.int64)
    return mn, mx, sm, qh, ql


@pytest.mark.parametrize("shift", (0, 16))
def test_reducing_sink(torch, fa, mixed, shift):
    """Bins of 3000 samples: every bin but the first lies in two frames; a range that starts and ends inside a tile."""
    data, blob, st, nb, _ = mixed
    n = data.shape[1]
    c, st_d, nb_d = place(torch, blob, shift), dev(torch, st), dev(torch, nb)
    for first, last in ((0, n), (13, n - 7)):
        got = fa.reduce_flac_device(c, st_d, nb_d, n, width=3000, first_sample=first, last_sample=last)
        for g, w, what in zip(got, reduce_bins(data, first, last, 3000), ("min", "max", "sum", "sumsq_hi", "sumsq_lo")):
            assert np.array_equal(g.cpu().numpy(), w), (what, first, last)
