"""The refill round of the throughput decoder at the end of the blob (profiles/k7_refill.md).  A lane requests its next
input chunk -- 64 bytes, four loads of 16 -- one refill ahead.  Per round the lanes that refill take one vote: every
lane's chunk ends at or in front of the blob's end rounded up to 16 (`lim16`).  Where it holds the four loads go out
unguarded; where one lane's chunk crosses lim16 the round keeps the per-piece bounds and zeroes what it does not load.
No test can see a load past lim16 without provoking a fault, so none tries (the argument is in the note); what the tests
pin is that both forms of the round, and a wave that changes from one to the other, decode the same samples:

  * the buffer ends 0 .. 129 bytes behind the last frame, the blob base lies 0 / 16 / 32 / 48 bytes behind a 64-byte
    boundary: the last chunk's end falls on both sides of lim16 and of each 16-byte piece.  Output through the sentinel
    harness of the footprint tests.
  * waves that mix lanes on both sides of the vote: 64 streams of one frame (and of 40 samples: a whole stream within three
    chunks of the end), 65 and 129 frames in one stream (a whole wave that passes beside a one-lane wave that does not).
  * the last frame of the blob short (4, 31, 33 samples), VERBATIM, of 32 partitions, or holding a code longer than any
    window: the guarded round beside the out-of-line readers.
  * ranges that leave the last frames out: the last lane's prefetch runs on into frames nobody decodes.
  * every instantiation of the loop on a tight buffer: int32, float32 restore, int64, compare sink, reducing sink.
  * frames that start at every byte of a ring word (streams with and without SEEKTABLE, four blob bases) next to a
    VERBATIM frame of 16 KB, which wraps the lane's 128-byte ring a hundred times over.

Stores come from the CPU encoder; results are compared with its input.  FLACARRAY_HIP_LATENCY=0 sends a decode through
K7, =1 through the latency decoder, which hands back to K7 what it does not take."""
import numpy as np
import pytest

from tests import compare_corpus as C
from tests import decode_edges as E
from tests import encoder_corpus as K
from tests import quant_model as M
from tests.conftest import sinusoid_noise_i32, strip_seektable
from tests.test_gpu_decode_footprint import Harness
from tests.test_gpu_k7_prefetch import dev, place, reduce_bins, subframe_kind

pytestmark = pytest.mark.gpu

B = 4096
SHIFTS = (0, 16, 32, 48)
TAILS = (0, 1, 15, 16, 17, 47, 48, 49, 63, 64, 65, 129)
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


def encode(oracle, data, level=5):
    data = np.ascontiguousarray(data, dtype=np.int32)
    return (data,) + tuple(np.asarray(x) for x in oracle.encode_i32(data, level))


def decode(torch, fa, enc, shift, tail, **kw):
    data, blob, st, nb = enc
    assert int((st.reshape(-1) + nb.reshape(-1)).max()) == blob.size, "the last frame ends the blob"
    return fa.decode_flac_device(place(torch, blob, shift, tail), dev(torch, st), dev(torch, nb), data.shape[1], **kw).cpu().numpy()


# ---------------------------------------------------------------------------------------------------- vote boundary

@pytest.fixture(scope="module")
def boundary(oracle):
    """64 streams x (4096 + 37) samples at level 5: two waves, a short last frame in every stream and at the blob's end."""
    n = B + 37
    data = sinusoid_noise_i32(E.ROWS, n, seed=901)
    blob, st, nb = oracle.encode_i32(data, 5)
    return E.Store("boundary", np.asarray(blob), np.asarray(st, dtype=np.int64), np.asarray(nb, dtype=np.int64), data, n, B, 1, None, None, None)


@LATENCY
@pytest.mark.parametrize("shift", SHIFTS)
@pytest.mark.parametrize("tail", TAILS)
def test_vote_boundary(torch, L, monkeypatch, boundary, tail, shift, latency):
    """The buffer ends `tail` bytes behind the last frame and starts `shift` bytes behind a 64-byte boundary: whole
    streams and the last frames alone, into a buffer of sentinel."""
    monkeypatch.setenv("FLACARRAY_HIP_LATENCY", latency)
    st = boundary._replace(blob=np.concatenate([boundary.blob, np.full(tail, 0xFF, dtype=np.uint8)]))
    assert int((st.starts + st.nbytes).max()) + tail == st.blob.size
    d = {"blob": place(torch, st.blob, shift), "starts": dev(torch, st.starts), "nbytes": dev(torch, st.nbytes), "offsets": None, "gains": None}
    assert d["blob"].numel() == st.blob.size
    h = Harness(torch, L, st, d, "device")
    try:
        h.window(0, st.n, 0, False)
        h.window(B + 1, st.n, 1, False)
    finally:
        h.close()


# ------------------------------------------------------------------------------------------------------ mixed waves

MIXED = {"1x65": (1, 65 * B), "1x129": (1, 129 * B - 31), "64x1": (64, B), "64x40": (64, 40)}


@pytest.fixture(scope="module")
def mixed_waves(oracle):
    made = {}

    def get(name):
        if name not in made:
            rows, n = MIXED[name]
            made[name] = encode(oracle, sinusoid_noise_i32(rows, n, seed=910 + len(made)))
        return made[name]

    yield get
    made.clear()


@LATENCY
@pytest.mark.parametrize("tail", (0, 17, 64))
@pytest.mark.parametrize("name", sorted(MIXED))
def test_mixed_waves(torch, fa, monkeypatch, mixed_waves, name, tail, latency):
    monkeypatch.setenv("FLACARRAY_HIP_LATENCY", latency)
    enc = mixed_waves(name)
    if name == "64x40":
        assert enc[1].size - int(enc[2].reshape(-1)[-1]) < 3 * 64, "the last stream lies within three chunks of the end"
    assert np.array_equal(decode(torch, fa, enc, 16, tail), enc[0])


# --------------------------------------------------------------------------------------------- last frame of the blob

def _last(kind, s):
    """Stream s of the store whose last frame is of `kind`."""
    head = K.noise_frame(920 + s)
    if kind.startswith("short"):
        return np.concatenate([head, sinusoid_noise_i32(1, int(kind[5:]), seed=930 + s)[0]])
    frame = {"verbatim": lambda: K.full_range_frame(940 + s), "partitions": lambda: K.partition_frame(950 + s, 5),
             "longcode": lambda: K.impulse_frame(B - 9 - 37 * (2 - s), value=(1 << 20) + 1)}[kind]()
    return np.concatenate([head, frame])


LAST_KINDS = ("short4", "short31", "short33", "verbatim", "partitions", "longcode")


@pytest.fixture(scope="module")
def last_frames(oracle):
    made = {}

    def get(kind):
        if kind not in made:
            enc = encode(oracle, np.stack([_last(kind, s) for s in range(3)]))
            _, blob, st, nb = enc
            seg = blob[st.reshape(-1)[-1] :]
            at = C._frame_offsets(seg)[-1]
            if kind == "verbatim":
                assert subframe_kind(seg, at)[0] == "verbatim"
            if kind in ("partitions", "longcode"):
                assert subframe_kind(seg, at)[1] == 5, "32 partitions"
            made[kind] = enc
        return made[kind]

    yield get
    made.clear()


@LATENCY
@pytest.mark.parametrize("tail", (0, 1, 17))
@pytest.mark.parametrize("kind", LAST_KINDS)
def test_last_frame_of_blob(torch, fa, monkeypatch, last_frames, kind, tail, latency):
    """(The impulse sits nine samples before the end of the last stream's frame: a unary run of more than a hundred zeros
    is read by the out-of-line reader within a chunk or two of the blob's end.)"""
    monkeypatch.setenv("FLACARRAY_HIP_LATENCY", latency)
    enc = last_frames(kind)
    assert np.array_equal(decode(torch, fa, enc, 0, tail), enc[0])
    assert np.array_equal(decode(torch, fa, enc, 48, tail, first_sample=B - 5, last_sample=enc[0].shape[1]), enc[0][:, B - 5 :])


# ----------------------------------------------------------------------------- the prefetch runs on behind the range

@LATENCY
@pytest.mark.parametrize("tail", (0, 17))
def test_range_leaves_last_frames_out(torch, fa, monkeypatch, mixed_waves, tail, latency):
    """One stream of 65 frames: a range that ends inside the second-to-last frame, and frame 0 alone."""
    monkeypatch.setenv("FLACARRAY_HIP_LATENCY", latency)
    enc = mixed_waves("1x65")
    data = enc[0]
    for first, last in ((62 * B + 13, 64 * B - 100), (0, B), (5, B - 7)):
        assert np.array_equal(decode(torch, fa, enc, 32, tail, first_sample=first, last_sample=last), data[:, first:last]), (first, last)


# ------------------------------------------------------------------------------------- every instantiation of the loop

@pytest.fixture(scope="module")
def every(oracle):
    """6 streams x 2 frames: noise, then -- by stream -- VERBATIM, 32 partitions, nearly full range, a late impulse, noise
    and a short tail is left out so that a full frame ends the blob."""
    rows = []
    for s in range(6):
        second = [K.full_range_frame(960 + s), K.partition_frame(961 + s, 5), K.near_max_frame(962 + s),
                  K.impulse_frame(B - 40 - s, value=(1 << 20) + 1), K.noise_frame(963 + s), K.partition_frame(964 + s, 5)][s]
        rows.append(np.concatenate([K.noise_frame(970 + s), second]))
    return encode(oracle, np.stack(rows))


@LATENCY
@pytest.mark.parametrize("tail", (0, 17))
def test_every_int32_float32(torch, fa, monkeypatch, every, tail, latency):
    monkeypatch.setenv("FLACARRAY_HIP_LATENCY", latency)
    data = every[0]
    assert np.array_equal(decode(torch, fa, every, 16, tail), data)
    r = np.arange(data.shape[0])
    off, gain = ((r % 7) * 0.25).astype(np.float32), (64.0 * (1 + r % 3)).astype(np.float32)
    y = decode(torch, fa, every, 16, tail, offsets=dev(torch, off), gains=dev(torch, gain))
    assert np.array_equal(y.view(np.uint32), np.ascontiguousarray(M.int32_to_float32(data, off, gain)).view(np.uint32))


@LATENCY
@pytest.mark.parametrize("tail", (0, 17))
def test_every_int64(torch, fa, oracle, monkeypatch, every, tail, latency):
    monkeypatch.setenv("FLACARRAY_HIP_LATENCY", latency)
    low = every[0][:3, : B + 33]
    x = np.ascontiguousarray(K.pack_i64(low, sinusoid_noise_i32(3, low.shape[1], seed=980, amp=2**6)), dtype=np.int64)
    blob, st, nb = (np.asarray(a) for a in oracle.encode_i64(x, 5))
    assert int((st.reshape(-1) + nb.reshape(-1)).max()) == blob.size
    y = fa.decode_flac_device(place(torch, blob, 16, tail), dev(torch, st), dev(torch, nb), x.shape[1], is_int64=True).cpu().numpy()
    assert np.array_equal(y, x)


@pytest.mark.parametrize("tail", (0, 17))
def test_every_compare_and_reduce(torch, fa, every, tail):
    data, blob, st, nb = every
    n = data.shape[1]
    c, st_d, nb_d = place(torch, blob, 16, tail), dev(torch, st), dev(torch, nb)
    where = np.array([0, B - 1, B, 2 * B - 1, 2 * B - 33, B + 31])
    flipped = data.copy()
    flipped[np.arange(data.shape[0]), where] ^= 1
    assert np.array_equal(fa.compare_flac_device(c, st_d, nb_d, dev(torch, data)).cpu().numpy().reshape(-1), np.full(data.shape[0], -1))
    assert np.array_equal(fa.compare_flac_device(c, st_d, nb_d, dev(torch, flipped)).cpu().numpy().reshape(-1), where)
    got = fa.reduce_flac_device(c, st_d, nb_d, n, width=3000)
    for g, w, what in zip(got, reduce_bins(data, 0, n, 3000), ("min", "max", "sum", "sumsq_hi", "sumsq_lo")):
        assert np.array_equal(g.cpu().numpy(), w), what


# ------------------------------------------------------------------------------------ bit positions and ring wraps

@pytest.fixture(scope="module")
def positions(oracle):
    """5 streams x 3 frames + 77 samples; frame 1 of every stream is VERBATIM (16 KB: the ring of two chunks wraps 128
    times inside it), the streams are kept with and without their SEEKTABLE."""
    rows = [np.concatenate([K.noise_frame(990 + s, bits=9 + s), K.full_range_frame(991 + s), K.noise_frame(992 + s, bits=13 - s),
                            sinusoid_noise_i32(1, 77, seed=993 + s)[0]]) for s in range(5)]
    full = encode(oracle, np.stack(rows))
    bare = (full[0],) + tuple(np.asarray(x) for x in strip_seektable(*full[1:]))
    starts = set()
    for a, n, a_bare in zip(full[2].reshape(-1), full[3].reshape(-1), bare[2].reshape(-1)):
        at = C._frame_offsets(full[1][a : a + n])  # (from the SEEKTABLE; without it the first frame starts at byte 42)
        assert at[2] - at[1] > 4 * B, "a VERBATIM frame of more than 16 KB"
        assert bytes(bare[1][a_bare + 42 : a_bare + 44]) == b"\xff\xf8"
        starts |= {int(a + o) % 4 for o in at} | {int(a_bare + 42 + o - at[0]) % 4 for o in at}
    assert starts == {0, 1, 2, 3}, "frames start at every byte of a 32-bit word"
    return full, bare


@LATENCY
@pytest.mark.parametrize("seektable", [True, False], ids=["seektable", "bare"])
@pytest.mark.parametrize("shift", SHIFTS)
def test_bit_positions(torch, fa, monkeypatch, positions, shift, seektable, latency):
    monkeypatch.setenv("FLACARRAY_HIP_LATENCY", latency)
    enc = positions[0] if seektable else positions[1]
    assert np.array_equal(decode(torch, fa, enc, shift, 0), enc[0])
    first, last = B + 13, 2 * B + 45
    assert np.array_equal(decode(torch, fa, enc, shift, 1, first_sample=first, last_sample=last), enc[0][:, first:last])
