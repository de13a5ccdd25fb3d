"""FlacArray.reduce / reduce_flac_device / DeviceDecodeIndex.reduce against numpy on the known input: per bin the exact
min, max, int64 sum and the two limbs of the sum of squares (checked as Python integers), on the shapes at which the
reducing sink of K7 and the chunk reducers can go wrong -- frames shared by bins and bins shared by frames, short last
frames, ranges that begin and end inside frames, every subframe type and history depth, streams without a SEEKTABLE,
foreign streams, stream subsets, float stores, two-channel stores in column chunks, side streams, damaged frames and
stores of two block sizes."""
import functools

import numpy as np
import pytest

from tests import stream_tools as T
from tests.conftest import full_range_i32, sinusoid_noise_f32, sinusoid_noise_i32, strip_seektable
from tests.encoder_corpus import BY_NAME
from tests.golden import flac_writer as W

pytestmark = pytest.mark.gpu

B = 4096
PY_BINS = 4000
WIDTHS = (None, 4096, 1152, 1024, 1000, 33, 8, 1, 10**7)


@pytest.fixture(scope="module")
def fa():
    import flacarray_amd

    return flacarray_amd


@pytest.fixture(scope="module")
def torch():
    import torch

    return torch


@pytest.fixture(autouse=True)
def _own_dispatch(monkeypatch):
    monkeypatch.delenv("FLACARRAY_HIP_LATENCY", raising=False)


# ---- the model ------------------------------------------------------------------------------------------------------

def model(x, first=0, last=None, width=None):
    """numpy on the known integers x [rows, n]: (count, min, max, sum, sum of squares as Python integers, hi limb, lo limb)."""
    x = np.asarray(x)
    n_all = x.shape[-1]
    last = n_all if last is None else last
    seg = x[:, first:last]
    n = last - first
    w = n if width is None else min(width, n)
    at = np.arange(0, n, w)
    cnt = np.minimum(at + w, n) - at
    mn = np.minimum.reduceat(seg, at, axis=1).astype(np.int64)
    mx = np.maximum.reduceat(seg, at, axis=1).astype(np.int64)
    sm = np.add.reduceat(seg.astype(np.int64), at, axis=1)  # (wraps for int64 input, as np.sum(dtype=int64) does)
    if x.dtype == np.int64:
        return cnt, mn, mx, sm, None, None, None
    q = (seg.astype(np.int64) * seg.astype(np.int64)).astype(np.uint64)  # <= 2^62
    r = lambda a: np.add.reduceat(a, at, axis=1)  # noqa: E731
    # The exact sum of squares as Python integers, through limbs of ANOTHER radix (2^31) than the library's.  Python
    # integers cost a microsecond each: of more than PY_BINS bins per row an evenly strided choice (first and last
    # included) is formed this way; the limbs of EVERY bin are compared exactly with numpy's (uint64, no overflow).
    pick = np.arange(at.size) if at.size <= PY_BINS else np.unique(np.linspace(0, at.size - 1, PY_BINS).astype(np.int64))
    exact = r(q >> np.uint64(31))[:, pick].astype(object) * (1 << 31) + r(q & np.uint64((1 << 31) - 1))[:, pick].astype(object)
    return cnt, mn, mx, sm, (pick, exact), r(q >> np.uint64(32)), r(q & np.uint64(0xFFFFFFFF))


def check_ints(got, x, first=0, last=None, width=None, what=""):
    """`got`: (min, max, sum, sumsq_hi, sumsq_lo) as numpy arrays [rows, nbins]; everything exact."""
    cnt, mn, mx, sm, exact, hi, lo = model(x, first, last, width)
    tag = (what, first, last, width)
    assert got[0].shape == mn.shape, tag
    assert np.array_equal(got[0], mn), tag
    assert np.array_equal(got[1], mx), tag
    assert np.array_equal(got[2], sm), tag
    if exact is None:
        assert got[3] is None and got[4] is None, tag
    else:
        assert np.array_equal(got[3].view(np.uint64), hi) and np.array_equal(got[4].view(np.uint64), lo), tag
        pick, want = exact
        assert np.array_equal(got[3].view(np.uint64)[:, pick].astype(object) * (1 << 32) + got[4].view(np.uint64)[:, pick].astype(object), want), tag
    return cnt, exact


def check_sumsq(sumsq, exact, what=""):
    """sumsq == float(the exact Python integer): bins of at most 2^21 samples."""
    pick, want = exact
    assert np.array_equal(np.asarray(sumsq)[:, pick], np.array([[float(v) for v in r] for r in want]).reshape(want.shape)), what


def check_stats(s, x, first=0, last=None, width=None, what="", lead=None):
    """A StreamStats of an integer store against the model, every field."""
    rows = x.reshape(-1, x.shape[-1])
    nb = s.sum.shape[-1]
    flat = lambda a: None if a is None else np.asarray(a).reshape(rows.shape[0], nb)  # noqa: E731
    cnt, exact = check_ints((flat(s.min_int), flat(s.max_int), flat(s.sum), flat(s.sumsq_hi), flat(s.sumsq_lo)), rows, first, last, width, what)
    if lead is not None:
        assert s.sum.shape == tuple(lead) + (nb,), what
    assert np.array_equal(flat(s.count), np.broadcast_to(cnt, (rows.shape[0], nb))), what
    assert s.min.dtype == x.dtype and np.array_equal(s.min, s.min_int) and np.array_equal(s.max, s.max_int), what
    if exact is not None:
        check_sumsq(flat(s.sumsq), exact, what)


def host_tuple(out):
    return tuple(None if t is None else t.cpu().numpy() for t in out)


@functools.lru_cache(maxsize=None)
def int32_input(shape):
    return sinusoid_noise_i32(*shape)


@functools.lru_cache(maxsize=None)
def int32_store(fa_mod, shape, level):
    return fa_mod.FlacArray.from_array(int32_input(shape), level=level)


def ranges_of(n):
    out = [(0, n), (1, n), (n - 1, n), (0, 1)]
    if n > 4097:
        out += [(4095, 4097)]
    if n >= 2 * B:
        out += [(B, 2 * B)]
    last0 = (n - 1) // B * B  # the short last frame
    if last0 > 0 and n - last0 > 2:
        out += [(B // 2 + 3, last0 + (n - last0) // 2)]
    return out


# ---- int32 ----------------------------------------------------------------------------------------------------------

# (8, 300_000): 74 frames per stream, so tasks span several waves and every stream ends in a short frame
INT32_CASES = [(shape, level) for shape in ((8, 300_000), (12, 1000)) for level in (0, 5, 8)] + [((3, 2 * 4096 + 7), 5)]


@pytest.mark.parametrize("shape,level", INT32_CASES, ids=["%dx%d-L%d" % (c[0] + c[1:]) for c in INT32_CASES])
def test_int32_every_width_and_range(fa, shape, level):
    x = int32_input(shape)
    arr = int32_store(fa, shape, level)
    n = shape[1]
    for first, last in ranges_of(n):
        for width in WIDTHS:
            s = arr.reduce(width=width, first=first, last=last)
            check_stats(s, x, first, last, width, what=f"{shape} L{level}", lead=(shape[0],))


def test_mean_and_std_of_an_integer_store(fa):
    x = int32_input((12, 1000))
    s = int32_store(fa, (12, 1000), 5).reduce(width=300)
    at = np.arange(0, 1000, 300)
    for j, a in enumerate(at):
        seg = x[:, a : a + 300].astype(np.float64)
        assert np.allclose(s.mean()[:, j], seg.mean(axis=1), rtol=1e-13, atol=0)
        assert np.allclose(s.std()[:, j], seg.std(axis=1), rtol=1e-9, atol=0)


def test_full_range_data(fa):
    """VERBATIM frames, INT32_MIN / INT32_MAX in min / max, the square limbs at their largest."""
    x = full_range_i32((4, 20_000))
    arr = fa.FlacArray.from_array(x, level=5)
    for width in (None, 4096, 1000, 33, 1):
        s = arr.reduce(width=width)
        check_stats(s, x, 0, None, width, what=f"full range")
    s = arr.reduce()
    assert s.min[0, 0] == -(2**31) and s.max[0, 0] == 2**31 - 1


CORPUS = ["wasted_l3", "wasted_l1", "lpc_orders_l8", "lpc_limit_l8", "lpc_shifts_l8", "one_bit_l5", "verbatim_exact_l5", "tail_odd_l8", "len1_l5", "tail5_l5"]


@pytest.mark.parametrize("name", CORPUS)
def test_encoder_corpus(fa, name):
    """Wasted bits (1-31, FIXED, LPC and VERBATIM), CONSTANT frames, LPC orders 10 and 12 at level 8 (the MO = 16 pass)."""
    case = BY_NAME[name]
    x = case.x
    arr = fa.FlacArray.from_array(x, level=case.level)
    for width in (None, 1000, 7):
        check_stats(arr.reduce(width=width), x, 0, None, width, what=f"{name}")
    n = x.shape[1]
    if n > 10:
        check_stats(arr.reduce(width=1000, first=3, last=n - 2), x, 3, n - 2, 1000, what=f"{name} range")


def test_constant_frames(fa):
    x = np.zeros((3, 2 * B + 100), np.int32)
    x[1] = -77
    x[2, B:] = sinusoid_noise_i32(1, B + 100, seed=5)[0]
    arr = fa.FlacArray.from_array(x, level=5)
    for width in (None, 1000, 4096, 5):
        check_stats(arr.reduce(width=width), x, 0, None, width, what=f"constant")


def test_seektable_stripped(fa, torch):
    shape = (8, 300_000)
    arr = int32_store(fa, shape, 5)
    blob, st, nb = strip_seektable(arr.compressed, arr.stream_starts, arr.stream_nbytes)
    d = tuple(torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in (blob, st, nb))
    for width, first, last in ((None, 0, None), (1000, 0, None), (4096, 5000, 250_001), (16, B - 3, 3 * B + 1)):
        got = host_tuple(fa.reduce_flac_device(*d, shape[1], width=width, first_sample=first, last_sample=last))
        check_ints(got, int32_input(shape), first, last, width, what=f"no seektable")


GOLDEN_MONO = ["g1_const", "g2_verbatim", "g3_fixed", "g4_lpc", "g5_wasted", "g6_16bit", "g7_deep"]


@pytest.mark.parametrize("name", GOLDEN_MONO)
def test_hand_assembled_streams(fa, torch, name):
    """Streams assembled field by field (tests/golden/make_golden.py), three copies addressed out of order, the blob not
    16-byte aligned: no SEEKTABLE, 16-bit (sample size from STREAMINFO) and 24-bit samples, wasted bits, escapes, Rice2,
    predictor orders 12 and 20 (the MO = 16 and MO = 32 passes)."""
    import os

    v = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "flac_vectors.npz"))
    s, st, n = v[name + "_samples"], v[name + "_stream"], int(v[name + "_size"])
    blob = np.concatenate([np.zeros(3, np.uint8), st, st, st])
    starts = np.array([2 * st.size, 0, st.size], dtype=np.int64)
    d = (torch.from_numpy(blob).cuda()[3:], torch.from_numpy(starts).cuda(), torch.from_numpy(np.full(3, st.size, dtype=np.int64)).cuda())
    x = np.stack([s, s, s]).astype(np.int32)
    for width, first, last in ((None, 0, None), (7, 0, None), (64, 0, None), (50, min(1, n - 1), n)):
        got = host_tuple(fa.reduce_flac_device(*d, n, width=width, first_sample=first, last_sample=last))
        check_ints(got, x, first, last, width, what=f"{name}")


@pytest.fixture(scope="module")
def deep_mixes():
    return [W.deep_mix(101, 1), W.deep_mix(102, 2)]


def test_generated_foreign_streams(fa, torch, deep_mixes):
    """libFLAC-shaped streams (tests/golden/flac_writer.py) whose frames cycle through LPC orders 1-8, 9-12, 13-16 and
    17-32: every history depth meets in one call, one- and two-channel; drawn seek-table layouts, escapes, wasted bits."""
    for b in deep_mixes:
        blob, st, nb = W.pack(b["streams"])
        d = tuple(torch.from_numpy(a).cuda() for a in (blob, st, nb))
        x, n, wide = np.asarray(b["samples"]), b["n"], b["channels"] == 2
        for width, first, last in ((None, 0, None), (1000, 0, None), (7, min(1, n - 1), n)):
            got = host_tuple(fa.reduce_flac_device(*d, n, width=width, first_sample=first, last_sample=last, is_int64=wide))
            check_ints(got, x.astype(np.int64 if wide else np.int32), first, last, width, what=f"{b['name']}")


def test_streams_subset(fa):
    shape = (8, 300_000)
    x = int32_input(shape)
    arr = int32_store(fa, shape, 5)
    for streams in ([5, 0, 3], np.array([7]), np.arange(8)[::-1]):
        idx = np.asarray(streams)
        for width, first, last in ((None, 0, None), (1000, 0, None), (4096, 1, 299_999), (8, 4000, 9000)):
            s = arr.reduce(width=width, first=first, last=last, streams=streams)
            check_stats(s, x[idx], first, last, width, what=f"subset", lead=(idx.size,))
    e = arr.reduce(width=1000, streams=[])
    assert e.sum.shape == (0, 300) and e.min.shape == (0, 300) and e.sumsq.shape == (0, 300)


def test_two_dimensional_leading_shape_and_one_dimensional_array(fa):
    x = sinusoid_noise_i32(6, 9000, seed=3).reshape(2, 3, 9000)
    s = fa.FlacArray.from_array(x, level=5).reduce(width=1000)
    assert s.sum.shape == (2, 3, 9) and s.count.shape == (2, 3, 9)
    check_stats(s, x, 0, None, 1000, what="2-D lead", lead=(2, 3))
    x1 = x[0, 0]
    a1 = fa.FlacArray.from_array(x1, level=5)
    s1 = a1.reduce(width=4096)
    assert s1.sum.shape == tuple(a1.leading_shape) + (3,)
    check_stats(s1, x1.reshape(1, -1), 0, None, 4096, what="1-D")


# ---- float32 --------------------------------------------------------------------------------------------------------

def test_float32_store(fa, torch):
    shape = (8, 300_000)
    x = sinusoid_noise_f32(*shape)
    arr = fa.FlacArray.from_array(x, quanta=1e-4, level=5)
    dec = arr.to_array()
    assert dec.dtype == np.float32
    comp, st, nb = (torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in (arr.compressed, arr.stream_starts, arr.stream_nbytes))
    ints = fa.decode_flac_device(comp, st, nb, shape[1]).cpu().numpy()  # the quantised integers: a decode with no offsets
    assert ints.dtype == np.int32
    off64 = np.asarray(arr.stream_offsets, np.float64).reshape(-1, 1)
    gain64 = np.asarray(arr.stream_gains, np.float64).reshape(-1, 1)
    for width, first, last in ((None, 0, None), (1000, 0, None), (4096, 100, 299_000), (33, 0, 50_000)):
        s = arr.reduce(width=width, first=first, last=last)
        n = (shape[1] if last is None else last) - first
        at = np.arange(0, n, n if width is None else width)
        seg = dec[:, first:last]
        assert s.min.dtype == np.float32 and s.max.dtype == np.float32
        assert np.array_equal(s.min, np.minimum.reduceat(seg, at, axis=1)), (width, first)
        assert np.array_equal(s.max, np.maximum.reduceat(seg, at, axis=1)), (width, first)
        cnt, exact = check_ints((s.min_int, s.max_int, s.sum, s.sumsq_hi, s.sumsq_lo), ints, first, last, width, what=f"f32")
        check_sumsq(s.sumsq, exact, "f32")
        # mean: two float32 roundings per restored sample; std: both sides exact up to float64 rounding
        mean_ref = np.add.reduceat(seg.astype(np.float64), at, axis=1) / cnt
        iseg = ints[:, first:last]
        bound = 2.0 * 2.0**-24 * (np.abs(off64) + np.abs(iseg).max() / gain64)
        assert np.all(np.abs(s.mean() - mean_ref) <= bound), (width, first)
        model64 = off64 + iseg.astype(np.float64) / gain64
        std_ref = np.stack([model64[:, a : a + c].std(axis=1) for a, c in zip(at, cnt)], axis=1)
        assert np.all(np.abs(s.std() - std_ref) <= 1e-9 * std_ref), (width, first)


# ---- int64 / float64 ------------------------------------------------------------------------------------------------

def _i64_input(n_ch=8, n=50_000, seed=11):
    """Busy low words, both signs; row 0 (otherwise non-negative) holds two values near 2^62, so its sum passes 2^63 and wraps."""
    rng = np.random.default_rng(seed)
    x = sinusoid_noise_i32(n_ch, n, seed=seed).astype(np.int64) * 70001 + rng.integers(-(2**20), 2**20, (n_ch, n))
    x[0] = np.abs(x[0])
    x[0, 100] = 2**62 + 12345
    x[0, 101] = 2**62 + 999
    x[1, 7] = -(2**62) - 5
    x[1, 4099] = -(2**62) - 6
    return x


@pytest.mark.parametrize("level", [0, 5])
def test_int64_store_in_column_chunks(fa, level):
    x = _i64_input()
    arr = fa.FlacArray.from_array(x, level=level)
    blk = 1152 if level <= 2 else B
    s = arr.reduce()
    assert s.sumsq_hi is None and s.sumsq_lo is None and s.sumsq is None
    assert s.sum[0, 0] == np.sum(x[0], dtype=np.int64) and s.sum[0, 0] != sum(int(v) for v in x[0])  # (it wrapped)
    import torch

    d = tuple(torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in (arr.compressed, arr.stream_starts.reshape(-1), arr.stream_nbytes.reshape(-1)))
    two_frames = 8 * 2 * blk * 8  # rows x two frames x 8 bytes
    for cap in (None, two_frames):
        for width, first, last in ((None, 0, None), (1000, 0, None), (1000, 77, 49_000), (blk, 0, None), (5, 0, None), (64, 3 * blk - 1, 3 * blk + 65)):
            got = host_tuple(fa.reduce_flac_device(*d, x.shape[1], width=width, first_sample=first, last_sample=last, is_int64=True, max_temp_bytes=cap))
            check_ints(got, x, first, last, width, what=f"i64 L{level} cap {cap}")
        got = host_tuple(fa.reduce_flac_device(*d, x.shape[1], width=1000, streams=[6, 1], is_int64=True, max_temp_bytes=cap))
        check_ints(got, x[[6, 1]], 0, None, 1000, what="i64 subset")
    for width in (None, 1000):
        check_stats(arr.reduce(width=width), x, 0, None, width, what="i64 array")
    ix = fa.DeviceDecodeIndex(*d, x.shape[1], is_int64=True)
    got = host_tuple(ix.reduce(width=1000, first_sample=5, max_temp_bytes=two_frames // 2))
    check_ints(got, x, 5, None, 1000, what="i64 indexed")
    ix.close()


def test_float64_store(fa):
    rng = np.random.default_rng(4)
    x = sinusoid_noise_f32(4, 50_000, seed=9).astype(np.float64) + 1e-9 * rng.normal(0.0, 1.0, (4, 50_000))
    arr = fa.FlacArray.from_array(x, quanta=1e-12, level=5)  # (integers beyond 32 bits)
    dec = arr.to_array()
    assert dec.dtype == np.float64
    arr.to_device()
    for width in (None, 1000):
        s = arr.reduce(width=width)
        at = np.arange(0, 50_000, 50_000 if width is None else width)
        assert s.min.dtype == np.float64 and s.sumsq is None
        assert np.array_equal(s.min, np.minimum.reduceat(dec, at, axis=1)) and np.array_equal(s.max, np.maximum.reduceat(dec, at, axis=1))
        ints = arr._index().decode().cpu().numpy()
        assert ints.dtype == np.int64 and np.abs(ints).max() > 2**32
        check_ints((s.min_int, s.max_int, s.sum, None, None), ints, 0, None, width, what="f64")
    arr.release_device()


# ---- resident and host stores; append and overwrite -----------------------------------------------------------------------

def test_resident_and_host_stores_agree(fa):
    shape = (8, 300_000)
    x = int32_input(shape)
    host = fa.FlacArray(int32_store(fa, shape, 5))
    res = fa.FlacArray(host).to_device()
    for kw in (dict(), dict(width=1000), dict(width=4096, first=10, last=299_000), dict(width=8, first=0, last=20_000), dict(width=1000, streams=[5, 0, 3])):
        a, b = host.reduce(**kw), res.reduce(**kw)
        for f in ("count", "min", "max", "sum", "sumsq_hi", "sumsq_lo", "sumsq", "min_int", "max_int"):
            assert np.array_equal(getattr(a, f), getattr(b, f)), (kw, f)
    check_stats(res.reduce(width=1000), x, 0, None, 1000, what="resident")
    res.release_device()


def test_reduce_after_append_and_overwrite_on_a_resident_store(fa):
    x = sinusoid_noise_i32(4, 20_000, seed=21)
    more = sinusoid_noise_i32(4, 5000, seed=22)
    patch = sinusoid_noise_i32(2, 3000, seed=23, amp=2**20)
    arr = fa.FlacArray.from_array(x, level=5).to_device()
    check_stats(arr.reduce(width=1000), x, 0, None, 1000, what="before")
    arr.append(more, level=5)
    y = np.concatenate([x, more], axis=1)
    check_stats(arr.reduce(width=1000), y, 0, None, 1000, what="appended")
    arr.overwrite(4000, patch, streams=[3, 1], level=5)
    y[[3, 1], 4000:7000] = patch
    for width in (None, 1000, 4096, 16):
        check_stats(arr.reduce(width=width), y, 0, None, width, what="overwritten")
    arr.release_device()


# ---- stream contract ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("kind", ["i32", "i32_narrow", "i32_subset", "i64"])
def test_side_stream_behind_a_delayed_producer(fa, torch, kind):
    side = torch.cuda.Stream()
    wide = kind == "i64"
    n = 20_000
    mk = (lambda seed: _i64_input(6, n, seed)) if wide else (lambda seed: sinusoid_noise_i32(6, n, seed=seed))
    stores = []
    for seed in (31, 32):
        comp, st, nb = fa.encode_flac_device(torch.from_numpy(mk(seed)).cuda(), level=5, compact=True)[:3]
        stores.append((comp, st.reshape(-1).contiguous(), nb.reshape(-1).contiguous()))
    torch.cuda.synchronize()
    size = max(s[0].numel() for s in stores)
    real, decoy = ([T.pad_blob(torch, s[0], size), s[1], s[2]] for s in stores)
    kw = dict(width=16 if kind == "i32_narrow" else 1000, is_int64=wide, streams=[4, 1] if kind == "i32_subset" else None)
    got, _ = T.run_delayed("reduce_" + kind, side, real, decoy, lambda c, st, nb: [t for t in fa.reduce_flac_device(c, st, nb, n, **kw) if t is not None])
    x = mk(31)
    if kind == "i32_subset":
        x = x[[4, 1]]
    check_ints(tuple(got) + ((None, None) if wide else ()), x, 0, None, kw["width"], what=kind)
    torch.cuda.synchronize()


# ---- errors ---------------------------------------------------------------------------------------------------------

def _first_frame_offset(stream):
    off = 4
    while True:
        last = stream[off] >> 7
        off += 4 + ((int(stream[off + 1]) << 16) | (int(stream[off + 2]) << 8) | int(stream[off + 3]))
        if last:
            return off


def test_damaged_frame_raises(fa, torch):
    arr = int32_store(fa, (12, 1000), 5)
    blob = np.array(arr.compressed, copy=True)
    st, nb = np.asarray(arr.stream_starts).reshape(-1), np.asarray(arr.stream_nbytes).reshape(-1)
    at = int(st[5]) + _first_frame_offset(blob[int(st[5]) : int(st[5] + nb[5])])
    assert blob[at] == 0xFF and (blob[at + 1] & 0xFC) == 0xF8
    blob[at] = 0x00  # the sync code: the decoder rejects the header before it reads anything else
    d = tuple(torch.from_numpy(a).cuda() for a in (blob, st, nb))
    for width in (None, 100, 8):
        with pytest.raises(RuntimeError):
            fa.reduce_flac_device(*d, 1000, width=width)
    # the undamaged store still reduces (nothing of the failed calls is left behind)
    check_stats(arr.reduce(width=100), int32_input((12, 1000)), 0, None, 100, what="after a damaged store")


def test_mixed_block_sizes(fa, torch):
    n = 9000
    xa, xb = sinusoid_noise_i32(3, n, seed=41), sinusoid_noise_i32(4, n, seed=42)
    a, b = fa.FlacArray.from_array(xa, level=0), fa.FlacArray.from_array(xb, level=5)
    blob = np.concatenate([a.compressed, b.compressed])
    st = np.concatenate([a.stream_starts.reshape(-1), b.stream_starts.reshape(-1) + a.compressed.size]).astype(np.int64)
    nb = np.concatenate([a.stream_nbytes.reshape(-1), b.stream_nbytes.reshape(-1)]).astype(np.int64)
    # interleave the two classes, so that the rows have to be scattered back
    order = np.array([0, 3, 1, 4, 5, 2, 6])
    x = np.concatenate([xa, xb])[order]
    d = tuple(torch.from_numpy(np.ascontiguousarray(v)).cuda() for v in (blob, st[order], nb[order]))
    for width, first, last in ((None, 0, None), (1000, 0, None), (4096, 17, 8999), (9, 0, 5000)):
        got = host_tuple(fa.reduce_flac_device(*d, n, width=width, first_sample=first, last_sample=last))
        check_ints(got, x, first, last, width, what=f"mixed")
    got = host_tuple(fa.reduce_flac_device(*d, n, width=1000, streams=[6, 0, 1]))
    check_ints(got, x[[6, 0, 1]], 0, None, 1000, what=f"mixed subset")
