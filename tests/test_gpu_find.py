"""find_flac_device / DeviceDecodeIndex.find / FlacArray.find and find_counts against the numpy model (tests/find_model.py)
on the known samples.  Every search is also held to conservation: find_counts(inside=False) + find_counts(inside=True) ==
last - first per row.  A frame counted twice or not at all -- across the three history passes of K7F -- breaks it."""
import ctypes
import functools

import numpy as np
import pytest

from tests import compare_corpus as C
from tests import find_model as M
from tests import quant_model as Q
from tests.conftest import full_range_i32, sinusoid_noise_f32, sinusoid_noise_i32, strip_seektable
from tests.encoder_corpus import BY_NAME

pytestmark = pytest.mark.gpu

I32_MIN, I32_MAX = -(2**31), 2**31 - 1
I64_MIN, I64_MAX = -(2**63), 2**63 - 1
CONVERT_TYPE = 1 << 19  # FA_ERROR_CONVERT_TYPE


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


def host(out):
    return tuple(None if t is None else t.cpu().numpy() for t in out)


def device_store(torch, arr):
    return tuple(torch.from_numpy(np.ascontiguousarray(np.asarray(a).reshape(-1))).cuda() for a in (arr.compressed, arr.stream_starts, arr.stream_nbytes))


def check(got, x, lo=None, hi=None, inside=False, first=0, last=None, what=""):
    """`got`: (counts, positions, values) numpy arrays of one search; against np.nonzero of the predicate on x [rows, n]."""
    x = np.asarray(x)
    last = x.shape[1] if last is None else last
    counts, pos, val = got
    wc, wr, wp, wv = M.hits(x, lo, hi, inside, first, last)
    print(what, "hits", int(np.sum(counts)), "expected", int(wc.sum()))
    assert counts.dtype == np.int64 and pos.dtype == np.int64, what
    assert np.array_equal(counts.reshape(-1), wc), (what, counts.reshape(-1).tolist()[:8], wc.tolist()[:8])
    assert np.array_equal(pos, wp), what
    if val is not None:
        assert val.dtype == np.int64 and np.array_equal(val, wv.astype(np.int64)), what


def conserved(count_fn, n_range, what=""):
    """count_fn(inside) -> counts per row."""
    out, ins = np.asarray(count_fn(False)).reshape(-1), np.asarray(count_fn(True)).reshape(-1)
    print(what, "outside + inside", (out + ins).tolist()[:8], "of", n_range)
    assert np.all(out + ins == n_range), (what, (out + ins).tolist(), n_range)
    return out, ins


def device_find(fa, d, x, lo, hi, inside=False, first=0, last=None, what="", **kw):
    """find_flac_device checked against the model, and its counts against conservation."""
    n = x.shape[1]
    got = host(fa.find_flac_device(*d, n, lo, hi, first, last, inside=inside, **kw))
    sel = kw.get("streams")
    xs = x if sel is None else x[np.asarray(sel, dtype=np.int64)]
    check(got, xs, lo, hi, inside, first, last, what)
    ckw = {k: v for k, v in kw.items() if k in ("streams", "is_int64", "max_temp_bytes")}
    out, _ = conserved(lambda ins: fa.find_counts_flac_device(*d, n, lo, hi, first, last, inside=ins, **ckw).cpu().numpy(),
                       (n if last is None else last) - first, what)
    assert np.array_equal(out if not inside else (n if last is None else last) - first - out, got[0])
    return got


@functools.lru_cache(maxsize=None)
def int32_input(shape, seed=7):
    return sinusoid_noise_i32(*shape, seed=seed)


@functools.lru_cache(maxsize=None)
def int32_store(fa_mod, shape, level):
    return fa_mod.FlacArray.from_array(int32_input(shape), level=level)


def percentiles(x):
    s = np.sort(x, axis=1)
    n = x.shape[1]
    return s[:, n // 100].astype(np.int64), s[:, n - 1 - n // 100].astype(np.int64)


# ---- 1. wave geometry ------------------------------------------------------------------------------------------------------

GEOMETRY = [
    ((3, 65 * 1152 + 7), 1),   # a stream over two waves, a wave with the tail of one stream and the head of the next, a short last frame
    ((70, 100), 1),            # every wave holds many rows
    ((130, 2 * 1152), 1),
    ((1, 64 * 1152), 1),       # exactly one full single-row wave
    ((2, 3 * 4096 + 5), 5),
]


@pytest.mark.parametrize("shape,level", GEOMETRY, ids=["%dx%d-L%d" % (s + (l,)) for s, l in GEOMETRY])
def test_wave_geometry(fa, torch, shape, level):
    x = int32_input(shape)
    d = device_store(torch, int32_store(fa, shape, level))
    p1, p99 = percentiles(x)
    device_find(fa, d, x, p1, p99, what=f"{shape} 1% / 99%")
    got = device_find(fa, d, x, 5, -5, what=f"{shape} all hit")
    assert np.all(got[0] == shape[1]) and np.array_equal(got[1], np.tile(np.arange(shape[1]), shape[0]))
    got = device_find(fa, d, x, I32_MIN, I32_MAX, what=f"{shape} no hit")
    assert got[1].size == 0 and not got[0].any()
    v = x[:, shape[1] // 2].astype(np.int64)  # a value that occurs, per row
    got = device_find(fa, d, x, v, v, inside=True, what=f"{shape} sentinel")
    assert np.all(got[0] >= 1)


# ---- 2. positions inside a frame -------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def spiked_stream():
    """Block 192, frames cycling through the LPC order buckets 1-8, 9-12, 13-16, 17-32; spikes at samples 0..33 of frames
    4..7 (one of every bucket: every warm-up depth and the first predicted sample), at B - 1, at B, and at n - 1 in the
    short last frame."""
    blk, n = 192, 8 * 192 + 37
    x = sinusoid_noise_i32(1, n, seed=5, amp=2**12)[0]
    at = sorted({f * blk + i for f in (4, 5, 6, 7) for i in range(34)} | {blk - 1, blk, n - 1})
    base = int(x.max()) + 1000  # (above everything else in the stream)
    for k, p in enumerate(at):
        x[p] = base + k
    rep = C.replicated(blk, n, 1, 11, samples=x)
    return rep, np.asarray(at, dtype=np.int64), base


def test_positions_inside_a_frame(fa, torch):
    rep, at, base = spiked_stream()
    blob, st, nb = C.store(rep, rows=3)
    d = tuple(torch.from_numpy(a).cuda() for a in (blob, st, nb))
    x = C.rows(rep, rows=3)
    got = device_find(fa, d, x, None, base - 1, what="spikes")
    assert np.array_equal(got[1], np.tile(at, 3)) and np.array_equal(got[2], np.tile(base + np.arange(at.size), 3))
    got = device_find(fa, d, x, base, base + at.size - 1, inside=True, what="spikes, inside")
    assert np.array_equal(got[1], np.tile(at, 3))
    # one spike at a time: lo == hi == its value
    for k in (0, 1, 2, 9, 35, 36 + 16, 36 + 17, 70 + 32, 70 + 33, 104 + 31, at.size - 1):
        got = host(fa.find_flac_device(*d, rep.n, base + k, base + k, inside=True, streams=[1]))
        assert got[0].tolist() == [1] and got[1].tolist() == [at[k]] and got[2].tolist() == [base + k], k


# ---- 3. every subframe kind and order ---------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", sorted(C.GEOMETRIES))
def test_foreign_streams_all_orders(fa, torch, name):
    """LPC orders 1-32 mixed in one store: all three history passes contribute to one search; one and two channels."""
    g = C.GEOMETRIES[name]
    rep = C.replicated(**g)
    blob, st, nb = C.store(rep, rows=5)
    d = tuple(torch.from_numpy(a).cuda() for a in (blob, st, nb))
    wide = g["channels"] == 2
    x = np.tile(np.asarray(rep.samples).astype(np.int64 if wide else np.int32), (5, 1))
    p1, p99 = percentiles(x)
    for first, last in ((0, None), (1, rep.n - 1), (g["block"] + 3, 3 * g["block"] + 1)):
        device_find(fa, d, x, p1, p99, first=first, last=last, is_int64=wide, what=f"{name} {first}:{last}")
    device_find(fa, d, x, 1, 0, is_int64=wide, what=name + " all hit")


@pytest.mark.parametrize("name", sorted(C.UNIFORM))
def test_foreign_streams_one_pass_each(fa, torch, name):
    rep = C.uniform(name)
    blob, st, nb = C.store(rep, rows=70)
    d = tuple(torch.from_numpy(a).cuda() for a in (blob, st, nb))
    x = C.rows(rep, rows=70)
    p1, p99 = percentiles(x)
    device_find(fa, d, x, p1, p99, what=name)
    device_find(fa, d, x, -8, 8, inside=True, first=5, last=rep.n - 3, what=name + " inside")


CORPUS = ["wasted_l3", "wasted_l1", "lpc_orders_l8", "lpc_limit_l8", "one_bit_l5", "verbatim_exact_l5", "tail_odd_l8", "len1_l5", "tail5_l5"]


@pytest.mark.parametrize("name", CORPUS)
def test_encoder_corpus(fa, name):
    """FIXED, LPC, VERBATIM and CONSTANT frames, wasted bits, escaped partitions, short tails."""
    case = BY_NAME[name]
    x = case.x
    arr = fa.FlacArray.from_array(x, level=case.level)
    n = x.shape[1]
    p1, p99 = percentiles(x)
    for lo, hi, inside in ((p1, p99, False), (p1, p99, True), (1, 0, False), (x[:, 0].astype(np.int64), x[:, 0].astype(np.int64), True)):
        h = arr.find(lo, hi, inside=inside)
        check((h.counts, h.positions, h.int_values), x, lo, hi, inside, what=name)
        assert np.array_equal(h.values, x[h.rows, h.positions]) and h.values.dtype == x.dtype
    conserved(lambda ins: arr.find_counts(p1, p99, inside=ins), n, name)
    if n > 10:
        h = arr.find(p1, p99, first=3, last=n - 2)
        check((h.counts, h.positions, h.int_values), x, p1, p99, False, 3, n - 2, what=name + " range")
        conserved(lambda ins: arr.find_counts(p1, p99, first=3, last=n - 2, inside=ins), n - 5, name + " range")


def test_wasted_bits_and_full_range(fa):
    x = (sinusoid_noise_i32(3, 3 * 4096 + 11, seed=9) // 8 * 8).astype(np.int32)
    for level in (1, 5):
        arr = fa.FlacArray.from_array(x, level=level)
        h = arr.find(-7, 7, inside=True)  # (only multiples of 8 occur: the zeros)
        check((h.counts, h.positions, h.int_values), x, -7, 7, True, what=f"wasted L{level}")
        assert np.all(h.int_values == 0)
        conserved(lambda ins: arr.find_counts(-7, 7, inside=ins), x.shape[1], "wasted")
    y = full_range_i32((3, 2 * 4096 + 100))
    arr = fa.FlacArray.from_array(y, level=5)
    for lo, hi in ((I32_MIN + 1, I32_MAX - 1), (I32_MIN, I32_MAX), (None, 0), (-(2**30), None), (I64_MIN, I64_MAX), (I64_MAX, I64_MIN)):
        h = arr.find(lo, hi)
        check((h.counts, h.positions, h.int_values), y, lo, hi, what=f"full range {lo} {hi}")


def test_seektable_stripped(fa, torch):
    shape = (3, 65 * 1152 + 7)
    arr = int32_store(fa, shape, 1)
    blob, st, nb = strip_seektable(arr.compressed, arr.stream_starts, arr.stream_nbytes)
    d = tuple(torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in (blob, st, nb))
    x = int32_input(shape)
    p1, p99 = percentiles(x)
    for first, last in ((0, None), (1153, 70_001)):
        device_find(fa, d, x, p1, p99, first=first, last=last, what="no seektable")


# ---- 4. range edges ---------------------------------------------------------------------------------------------------------

def test_range_edges(fa, torch):
    shape, blk = (3, 65 * 1152 + 7), 1152
    x = int32_input(shape)
    n = shape[1]
    d = device_store(torch, int32_store(fa, shape, 1))
    p1, p99 = percentiles(x)
    for first, last in ((5, n - 3), (blk + 3, 3 * blk + 1), (blk, 3 * blk), (blk - 1, 3 * blk + 1), (blk + 1, 3 * blk - 1), (blk + 3, blk + 4), (0, 1),
                        (n - 1, n), (64 * blk - 1, 64 * blk + 1), (blk + 10, blk + 200), (17, n)):
        device_find(fa, d, x, p1, p99, first=first, last=last, what=f"range {first}:{last}")
        device_find(fa, d, x, 1, 0, first=first, last=last, what=f"range {first}:{last} all")


def test_hits_at_the_ends_of_the_range_and_just_outside(fa):
    blk = 1152
    x = np.array(int32_input((3, 3 * 1152 + 9)), copy=True)
    big = 2**20
    for first, last in ((100, 2000), (blk, 2 * blk), (blk - 1, 2 * blk + 1), (7, 8)):
        y = x.copy()
        for p in (first - 1, first, last - 1, last):
            y[:, p] = big
        arr = fa.FlacArray.from_array(y, level=1)
        h = arr.find(hi=big - 1, first=first, last=last)
        want = sorted({first, last - 1})
        assert np.array_equal(h.positions, np.tile(want, 3)) and np.all(h.values == big), (first, last)
        assert h.ranges().tolist() == [[r, a, a + 1] for r in range(3) for a in want]
        conserved(lambda ins: arr.find_counts(hi=big - 1, first=first, last=last, inside=ins), last - first, "ends")


# ---- 5. streams= ------------------------------------------------------------------------------------------------------------

def test_streams_subsets(fa, torch):
    shape = (3, 65 * 1152 + 7)
    x = int32_input(shape)
    arr = int32_store(fa, shape, 1)
    d = device_store(torch, arr)
    for streams in ([2, 0], np.array([1]), [2, 1, 0]):
        idx = np.asarray(streams)
        p1, p99 = percentiles(x[idx])
        device_find(fa, d, x, p1, p99, first=3, last=70_000, streams=streams, what=f"subset {streams}")
        h = arr.find(p1, p99, streams=streams)
        check((h.counts, h.positions, h.int_values), x[idx], p1, p99, what=f"subset {streams} array")
        assert h.counts.shape == (idx.size,) and np.array_equal(h.streams, idx)
        assert set(h.ranges()[:, 0].tolist()) == set(idx[h.counts > 0].tolist())
    shape = (130, 2 * 1152)  # rows that share a wave with rows not asked for
    x = int32_input(shape)
    sel = [129, 5, 64, 63, 0, 77]
    p1, p99 = percentiles(x[sel])
    h = int32_store(fa, shape, 1).find(p1, p99, streams=sel)
    check((h.counts, h.positions, h.int_values), x[sel], p1, p99, what="subset of short streams")
    assert np.array_equal(h.values, x[np.asarray(sel)[h.rows], h.positions])
    c, p, v = fa.find_flac_device(*d, 65 * 1152 + 7, 0, 0, streams=[])
    assert c.shape == (0,) and p.shape == (0,) and v.shape == (0,) and c.dtype == torch.int64
    assert fa.find_counts_flac_device(*d, 65 * 1152 + 7, 0, 0, streams=[]).shape == (0,)


# ---- 6. int64 and float64 stores ----------------------------------------------------------------------------------------------

def _i64_input(n_ch=4, n=3 * 4096 + 50, seed=11):
    """Values beyond 2^40 of both signs; row 0 holds a sample near INT64_MAX, row 1 one near INT64_MIN."""
    rng = np.random.default_rng(seed)
    x = sinusoid_noise_i32(n_ch, n, seed=seed).astype(np.int64) * (2**25 + 1) + rng.integers(-(2**20), 2**20, (n_ch, n))
    x[0, 100] = I64_MAX - 3
    x[1, 4099] = I64_MIN + 2
    return x


@pytest.mark.parametrize("level", [0, 5])
def test_int64_store(fa, torch, level):
    x = _i64_input()
    n = x.shape[1]
    blk = 1152 if level <= 2 else 4096
    big = 2**50
    # hits on the first and last sample of a chunk of two frames and across its seams
    seams = [p for p in (0, blk - 1, blk, 2 * blk - 1, 2 * blk, 2 * blk + 1, 3 * blk - 1, 3 * blk, 4 * blk - 1, 4 * blk) if p < n - 1] + [n - 1]
    for p in seams:
        x[2, p] = big + p
    arr = fa.FlacArray.from_array(x, level=level)
    d = device_store(torch, arr)
    two_frames = x.shape[0] * 2 * blk * 8
    p1, p99 = percentiles(x)
    for cap in (None, two_frames, 1):
        device_find(fa, d, x, p1, p99, is_int64=True, max_temp_bytes=cap, what=f"i64 L{level} cap {cap}")
        got = device_find(fa, d, x, None, big - 1, is_int64=True, max_temp_bytes=cap, what=f"i64 L{level} cap {cap} seams")
        assert got[1].tolist()[:1] == [100] and got[1].tolist()[1:] == seams
        device_find(fa, d, x, -(2**45), 2**44, first=77, last=n - 5, is_int64=True, max_temp_bytes=cap, what="i64 range")
        device_find(fa, d, x, -(2**45), 2**44, first=blk - 1, last=2 * blk + 3, inside=True, is_int64=True, max_temp_bytes=cap, what="i64 inside")
    for lo, hi in ((I64_MIN, I64_MAX), (I64_MIN + 3, I64_MAX - 4), (I64_MAX, I64_MIN), (None, None)):
        device_find(fa, d, x, lo, hi, is_int64=True, max_temp_bytes=two_frames, what=f"i64 limits {lo} {hi}")
    device_find(fa, d, x, [0, -5], [2**41, 2**33], streams=[3, 1], is_int64=True, max_temp_bytes=two_frames, what="i64 subset")
    h = arr.find(p1, p99)
    check((h.counts, h.positions, h.int_values), x, p1, p99, what="i64 array")
    assert h.values.dtype == np.int64 and np.array_equal(h.values, x[h.rows, h.positions])
    ix = fa.DeviceDecodeIndex(*d, n, is_int64=True)
    check(host(ix.find(p1, p99, first_sample=5, max_temp_bytes=two_frames // 2)), x, p1, p99, False, 5, None, what="i64 indexed")
    conserved(lambda ins: ix.find_counts(p1, p99, 5, None, inside=ins, max_temp_bytes=two_frames).cpu().numpy(), n - 5, "i64 indexed")
    ix.close()


def _float_checks(arr, dec, ints, what):
    """Float limits on a float store against np.nonzero on to_array(), bit for bit."""
    n = dec.shape[1]
    srt = np.sort(dec, axis=1)
    v_lo, v_hi = srt[:, n // 50].astype(np.float64), srt[:, n - 1 - n // 50].astype(np.float64)  # restored sample values, exactly
    nxt = np.array([srt[r][srt[r] > srt[r, n // 50]][0] for r in range(dec.shape[0])], dtype=np.float64)
    cases = [(v_lo, v_hi), ((v_lo + nxt) / 2, v_hi), (np.nextafter(v_lo, np.inf), np.nextafter(v_hi, -np.inf)), (-np.inf, v_hi), (v_lo, np.inf),
             (-np.inf, np.inf), (np.inf, -np.inf), (float(v_lo[0]), float(v_hi[0])), (None, None)]
    for lo, hi in cases:
        for inside in (False, True):
            h = arr.find(lo, hi, inside=inside)
            wc, wr, wp, wv = M.hits(dec, lo, hi, inside, dtype=np.float64)
            assert np.array_equal(h.counts.reshape(-1), wc), (what, lo, hi, inside)
            assert np.array_equal(h.rows, wr) and np.array_equal(h.positions, wp), (what, lo, hi)
            assert h.values.dtype == dec.dtype and Q.bits_equal(h.values, dec[wr, wp]), (what, lo, hi)
            assert np.array_equal(h.int_values, ints[wr, wp]), (what, lo, hi)
            if not inside:
                assert np.array_equal(arr.find_counts(lo, hi).reshape(-1), wc)
    # strict comparisons: a limit set exactly to a restored value does not hit that value
    h = arr.find(v_lo, v_hi)
    assert not np.any(h.values.astype(np.float64) == v_lo[h.rows]) and not np.any(h.values.astype(np.float64) == v_hi[h.rows])
    # quantised=True: integer limits as they are
    p1, p99 = percentiles(ints)
    h = arr.find(p1[[2, 0]], p99[[2, 0]], quantised=True, first=3, last=n - 1, streams=[2, 0])
    check((h.counts, h.positions, h.int_values), ints[[2, 0]], p1[[2, 0]], p99[[2, 0]], False, 3, n - 1, what=what + " quantised")
    assert Q.bits_equal(h.values, dec[np.array([2, 0])[h.rows], h.positions])
    conserved(lambda ins: arr.find_counts(v_lo, v_hi, inside=ins), n, what)


def test_float32_store(fa):
    shape = (3, 9 * 1152 + 7)
    x = sinusoid_noise_f32(*shape)
    arr = fa.FlacArray.from_array(x, quanta=1e-4, level=1)
    ints = np.asarray(Q.float32_to_int32(x, 1e-4)[0]).reshape(shape)
    dec = arr.to_array()
    assert dec.dtype == np.float32
    _float_checks(arr, dec, ints, "f32")


def test_float64_store(fa):
    rng = np.random.default_rng(4)
    x = sinusoid_noise_f32(3, 3 * 4096 + 50, seed=9).astype(np.float64) + 1e-9 * rng.normal(0.0, 1.0, (3, 3 * 4096 + 50))
    arr = fa.FlacArray.from_array(x, quanta=1e-12, level=5).to_device()
    ints = arr._index().decode().cpu().numpy()
    assert ints.dtype == np.int64 and np.abs(ints).max() > 2**32
    dec = arr.to_array()
    assert dec.dtype == np.float64
    _float_checks(arr, dec, ints, "f64")
    arr.release_device()


# ---- 8. routes agree ----------------------------------------------------------------------------------------------------------

def test_routes_agree(fa, torch):
    x = sinusoid_noise_i32(4, 20_000, seed=21)
    n = x.shape[1]
    host_arr = fa.FlacArray.from_array(x, level=5)
    arr = fa.FlacArray(host_arr).to_device()
    p1, p99 = percentiles(x)
    d = device_store(torch, host_arr)
    direct = host(fa.find_flac_device(*d, n, p1, p99, 9, n - 1))
    check(direct, x, p1, p99, False, 9, n - 1, what="direct")
    again = host(fa.find_flac_device(*d, n, p1, p99, 9, n - 1))
    for p, q in zip(direct, again):
        assert np.array_equal(p, q)
    no_val = fa.find_flac_device(*d, n, p1, p99, 9, n - 1, values=False)
    assert no_val[2] is None and np.array_equal(no_val[1].cpu().numpy(), direct[1])
    ix = fa.DeviceDecodeIndex(*d, n)
    for _ in range(2):
        for p, q in zip(direct, host(ix.find(p1, p99, 9, n - 1))):
            assert np.array_equal(p, q)
    assert ix.find(p1, p99, 9, n - 1, values=False)[2] is None
    assert np.array_equal(ix.find_counts(p1, p99, 9, n - 1).cpu().numpy(), direct[0])
    ix.close()
    for a in (arr, host_arr):
        h = a.find(p1, p99, first=9, last=n - 1)
        for p, q in zip(direct, (h.counts, h.positions, h.int_values)):
            assert np.array_equal(p, q)
        assert np.array_equal(h.offsets, np.concatenate([[0], np.cumsum(direct[0])])) and np.array_equal(h.rows, np.repeat(np.arange(4), direct[0]))
        assert h.values.dtype == np.int32 and np.array_equal(h.values, x[h.rows, h.positions])
        assert np.array_equal(a.find_counts(p1, p99, first=9, last=n - 1), direct[0])
        assert np.array_equal(h.ranges(2), M.ranges(4, h.rows, h.positions, 9, n - 1, 2))
    arr.release_device()


def test_leading_shapes(fa):
    x = sinusoid_noise_i32(6, 5000, seed=3).reshape(2, 3, 5000)
    arr = fa.FlacArray.from_array(x, level=5)
    h = arr.find(-(2**15), 2**15)
    assert h.counts.shape == (2, 3) and arr.find_counts(-(2**15), 2**15).shape == (2, 3)
    check((h.counts, h.positions, h.int_values), x.reshape(6, -1), -(2**15), 2**15, what="2-D lead")


# ---- 9. max_hits ----------------------------------------------------------------------------------------------------------------

def test_max_hits(fa, torch):
    shape = (3, 65 * 1152 + 7)
    x = int32_input(shape)
    arr = int32_store(fa, shape, 1)
    d = device_store(torch, arr)
    p1, p99 = percentiles(x)
    total = int(M.hits(x, p1, p99)[0].sum())
    assert total > 10
    for call in (lambda m: fa.find_flac_device(*d, shape[1], p1, p99, max_hits=m), lambda m: arr.find(p1, p99, max_hits=m)):
        with pytest.raises(ValueError, match=str(total)):
            call(total - 1)
        with pytest.raises(ValueError, match=str(total)):
            call(0)
        call(total)
        call(total + 1)
    ix = fa.DeviceDecodeIndex(*d, shape[1])
    with pytest.raises(ValueError, match=str(total)):
        ix.find(p1, p99, max_hits=total - 1)
    assert int(ix.find(p1, p99, max_hits=total)[0].sum()) == total
    ix.close()


# ---- 10. dirty buffers -----------------------------------------------------------------------------------------------------------

def _dirty_allocations(torch, monkeypatch, poison):
    """torch.empty and Tensor.new_empty give device memory full of the poison; the fill is queued on the current stream."""
    real_empty, real_new_empty = torch.empty, torch.Tensor.new_empty

    def dirty(t):
        if t.is_cuda and t.numel() and t.is_contiguous():
            t.reshape(-1).view(torch.uint8).fill_(poison)
        return t

    monkeypatch.setattr(torch, "empty", lambda *a, **kw: dirty(real_empty(*a, **kw)))
    try:
        monkeypatch.setattr(torch.Tensor, "new_empty", lambda self, *a, **kw: dirty(real_new_empty(self, *a, **kw)))
    except (AttributeError, TypeError):
        pass  # (a build whose Tensor does not take the attribute: torch.empty is the one the library calls)


@pytest.mark.parametrize("poison", [0x00, 0xFF, 0xA5], ids=["zeros", "ones", "a5"])
def test_dirty_buffers(fa, torch, monkeypatch, poison):
    _dirty_allocations(torch, monkeypatch, poison)
    shape = (3, 9 * 1152 + 7)
    x = int32_input(shape)
    arr = int32_store(fa, shape, 1)
    d = device_store(torch, arr)
    p1, p99 = percentiles(x)
    device_find(fa, d, x, p1, p99, first=5, what="dirty i32")
    device_find(fa, d, x, p1[[2, 0]], p99[[2, 0]], streams=[2, 0], what="dirty i32 subset")
    deep = C.replicated(**C.GEOMETRIES["mono192_unaligned"])  # (all three history passes write into one count array)
    dd = tuple(torch.from_numpy(a).cuda() for a in C.store(deep, rows=4))
    xd = C.rows(deep, rows=4)
    q1, q99 = percentiles(xd)
    device_find(fa, dd, xd, q1, q99, what="dirty deep")
    y = _i64_input(3, 2 * 4096 + 50)
    d64 = device_store(torch, fa.FlacArray.from_array(y, level=5))
    q1, q99 = percentiles(y)
    device_find(fa, d64, y, q1, q99, is_int64=True, max_temp_bytes=1, what="dirty i64")


@pytest.mark.parametrize("poison", [0x00, 0xFF, 0xA5], ids=["zeros", "ones", "a5"])
def test_raw_count_call_guard_and_wrong_frame_count(fa, torch, poison):
    from flacarray_amd import _lib
    from flacarray_amd.libflacarray import _dp

    L = _lib.lib()
    shape, blk = (3, 9 * 1152 + 7), 1152
    x = int32_input(shape)
    n = shape[1]
    comp, st, nb = device_store(torch, int32_store(fa, shape, 1))
    first, last = 5, n - 2
    B, nfr = ctypes.c_int64(0), ctypes.c_int64(0)
    assert L.fa_find_plan_device(_dp(comp), comp.numel(), _dp(st), n, first, last, ctypes.byref(B), ctypes.byref(nfr), None) == 0
    assert B.value == blk and nfr.value == (last - 1) // blk - first // blk + 1
    cells = 3 * nfr.value
    p1, p99 = percentiles(x)
    lo, hi = torch.from_numpy(p1).cuda(), torch.from_numpy(p99).cuda()
    word = int.from_bytes(bytes([poison]) * 8, "little", signed=True)

    def run(frames, is_sel):
        buf = torch.full((cells + 16,), word, dtype=torch.int64, device="cuda")
        sel = torch.tensor([2, 0, 1], dtype=torch.int64, device="cuda") if is_sel else None
        torch.cuda.synchronize()
        err = L.fa_find_count_i32_device(_dp(comp), comp.numel(), _dp(st), _dp(nb), 3, n, first, last, 3, _dp(sel), _dp(lo), _dp(hi), 0, frames, _dp(buf),
                                         None, 0)
        torch.cuda.synchronize()
        return err, buf.cpu().numpy()

    for is_sel in (False, True):
        err, buf = run(nfr.value, is_sel)
        assert err == 0
        assert np.all(buf[cells:] == word), "the guard behind frame_counts was written"
        xs, l, h = (x[[2, 0, 1]], p1, p99) if is_sel else (x, p1, p99)
        m = M.hit_mask(xs[:, first:last], l, h)
        want = np.zeros((3, nfr.value), dtype=np.int64)
        for k in range(nfr.value):
            a, b = max(k * blk, first) - first, min((k + 1) * blk, last) - first
            want[:, k] = m[:, a:b].sum(axis=1)
        assert np.array_equal(buf[:cells].reshape(3, -1), want)
        for wrong in (nfr.value - 1, nfr.value + 1, 1):
            err, buf = run(wrong, is_sel)
            assert err == CONVERT_TYPE
            assert np.all(buf == word), "a refused call wrote to frame_counts"
    ix = fa.DeviceDecodeIndex(comp, st, nb, n)
    buf = torch.full((cells + 16,), word, dtype=torch.int64, device="cuda")
    err = L.fa_find_count_indexed(ix._h, first, last, 3, None, 0, _dp(lo), _dp(hi), 0, nfr.value + 1, _dp(buf), None, 0)
    torch.cuda.synchronize()
    assert err != 0 and np.all(buf.cpu().numpy() == word)
    ix.close()
