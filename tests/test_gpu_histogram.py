"""histogram_flac_device / DeviceDecodeIndex.histogram / FlacArray.histogram, order_statistic, quantile and median against
the numpy model (tests/histogram_model.py) on the known samples.  Every histogram is also held to the conservation law
counts.sum(-1) + below + above == last - first per row: a frame counted twice or not at all -- across the three history
passes of K7H, or across its two accumulation routes (the wave's LDS histogram; straight to memory for a wave that holds
several rows) -- breaks it."""
import functools

import numpy as np
import pytest

from tests import histogram_model as M
from tests import quant_model as Q
from tests import stream_tools as T
from tests.conftest import full_range_i32, sinusoid_noise_f32, sinusoid_noise_i32, strip_seektable
from tests.encoder_corpus import BY_NAME
from tests.golden import flac_writer as W

pytestmark = pytest.mark.gpu

I32_MIN, I32_MAX = -(2**31), 2**31 - 1
I64_MIN, I64_MAX = -(2**63), 2**63 - 1


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
    return tuple(t.cpu().numpy() for t in out)


def check(got, x, lo, shift, nbins, first=0, last=None, what=""):
    """`got`: (counts, below, above) numpy arrays; against the model on x [rows, n], and the conservation law."""
    x = np.asarray(x).reshape(-1, np.asarray(x).shape[-1])
    last = x.shape[1] if last is None else last
    c, b, a = (np.asarray(v) for v in got)
    rows = x.shape[0]
    c, b, a = c.reshape(rows, nbins), b.reshape(rows), a.reshape(rows)
    assert c.dtype == np.int64 and b.dtype == np.int64 and a.dtype == np.int64, what
    total = c.sum(axis=1) + b + a
    print(what, "counted", total.tolist()[:8], "of", last - first)
    assert np.all(total == last - first), (what, "conservation", total.tolist(), last - first)
    wc, wb, wa = M.bin_counts(x[:, first:last], lo, shift, nbins)
    assert np.array_equal(b, wb) and np.array_equal(a, wa), (what, b.tolist(), wb.tolist(), a.tolist(), wa.tolist())
    assert np.array_equal(c, wc), what


def device_store(torch, arr):
    return tuple(torch.from_numpy(np.ascontiguousarray(np.asarray(a).reshape(-1))).cuda() for a in (arr.compressed, arr.stream_starts, arr.stream_nbytes))


@functools.lru_cache(maxsize=None)
def int32_input(shape, seed=7):
    return sinusoid_noise_i32(*shape, seed=seed)


@functools.lru_cache(maxsize=None)
def int32_store(fa_mod, shape, level):
    return fa_mod.FlacArray.from_array(int32_input(shape), level=level)


# ---- wave geometry --------------------------------------------------------------------------------------------------------

GEOMETRY = [
    ((3, 65 * 1152 + 7), 1),   # a stream over two waves, a wave with the tail of one stream and the head of the next, a short last frame
    ((70, 100), 1),            # every wave holds many rows: the direct route alone
    ((130, 2 * 1152), 1),
    ((1, 64 * 1152), 1),       # exactly one full single-row wave
    ((2, 3 * 4096 + 5), 5),
]


@pytest.mark.parametrize("shape,level", GEOMETRY, ids=["%dx%d-L%d" % (s + (l,)) for s, l in GEOMETRY])
def test_wave_geometry(fa, torch, shape, level):
    x = int32_input(shape)
    arr = int32_store(fa, shape, level)
    d = device_store(torch, arr)
    n = shape[1]
    lo, sh = M.auto_range(x, 256)
    for nbins, lo_, sh_ in ((256, lo, sh), (2048, lo, np.maximum(sh - 3, 0)), (1, lo + 1000, 10), (64, 0, 12)):
        got = host(fa.histogram_flac_device(*d, n, lo_, sh_, nbins))
        check(got, x, lo_, sh_, nbins, what=f"{shape} L{level} nbins {nbins}")
    h = arr.histogram(bins=256)
    check((h.counts, h.below, h.above), x, lo, sh, 256, what=f"{shape} auto")
    assert np.array_equal(h.lo, lo) and np.array_equal(h.shift, sh) and not h.below.any() and not h.above.any()
    assert h.counts.shape == (shape[0], 256) and h.lo.shape == (shape[0],)


# ---- bin arithmetic -------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("nbins", [1, 2, 255, 2047, 2048])
def test_bin_counts(fa, torch, nbins):
    shape = (3, 65 * 1152 + 7)
    x = int32_input(shape)
    d = device_store(torch, int32_store(fa, shape, 1))
    lo, sh = M.auto_range(x, nbins)
    check(host(fa.histogram_flac_device(*d, shape[1], lo, sh, nbins)), x, lo, sh, nbins, what=f"auto {nbins}")
    # a narrower window: samples fall below and above
    # (nbins << (sh - 1) <= span by the choice of sh, so this window starts a quarter in and ends before three quarters)
    span = x.max(axis=1).astype(np.int64) - x.min(axis=1)
    lo2, sh2 = lo + span // 4, np.maximum(sh - 2, 0)
    got = host(fa.histogram_flac_device(*d, shape[1], lo2, sh2, nbins))
    check(got, x, lo2, sh2, nbins, what=f"window {nbins}")
    assert got[1].all() and got[2].all()


@pytest.mark.parametrize("shift", [0, 1, 11, 31, 32, 40])
def test_shifts_and_full_range_data(fa, torch, shift):
    """lo = INT32_MIN on full-range data: the differences need more than 32 bits; VERBATIM frames."""
    x = full_range_i32((3, 2 * 4096 + 100))
    arr = fa.FlacArray.from_array(x, level=5)
    d = device_store(torch, arr)
    for lo, nbins in ((I32_MIN, 2048), (I32_MIN, 3), (-5, 2), (I64_MIN, 2048), (I32_MAX, 1)):
        check(host(fa.histogram_flac_device(*d, x.shape[1], lo, shift, nbins)), x, lo, shift, nbins, what=f"shift {shift} lo {lo}")


def test_lo_at_int64_min_on_a_32_bit_store(fa, torch):
    """x - lo is 2^63 and more for every non-negative sample: a signed shift of the difference would send those samples
    above; the unsigned one puts them into bins 1024.. (shift 53) or bin 1 (shift 63)."""
    x = full_range_i32((3, 2 * 4096 + 100))
    d = device_store(torch, fa.FlacArray.from_array(x, level=5))
    for lo, shift, nbins in ((I64_MIN, 53, 2048), (I64_MIN, 63, 2), (I64_MIN + 5, 62, 4), (I64_MIN, 32, 2048)):
        got = host(fa.histogram_flac_device(*d, x.shape[1], lo, shift, nbins))
        check(got, x, lo, shift, nbins, what=f"lo {lo} shift {shift}")
    got = host(fa.histogram_flac_device(*d, x.shape[1], I64_MIN, 63, 2))
    assert np.array_equal(got[0][:, 1], (x >= 0).sum(axis=1)) and not got[2].any()


def test_per_row_lo_and_shift(fa, torch):
    shape = (70, 100)
    x = int32_input(shape)
    d = device_store(torch, int32_store(fa, shape, 1))
    rng = np.random.default_rng(3)
    lo = rng.integers(-(2**18), 2**17, shape[0])
    sh = rng.integers(0, 20, shape[0]).astype(np.int32)
    got = host(fa.histogram_flac_device(*d, shape[1], torch.from_numpy(lo), sh, 300))
    check(got, x, lo, sh, 300, what="per row")
    shape = (3, 65 * 1152 + 7)
    x = int32_input(shape)
    d = device_store(torch, int32_store(fa, shape, 1))
    lo, sh = np.array([-(2**17), 0, I32_MIN]), np.array([8, 3, 21])
    check(host(fa.histogram_flac_device(*d, shape[1], lo, sh, 2048)), x, lo, sh, 2048, what="per row, long streams")


def test_all_samples_in_one_bin(fa):
    """A constant stream (CONSTANT subframes) and busy streams inside one wide bin: every add of a wave hits one word."""
    x = sinusoid_noise_i32(3, 66 * 4096 + 9, seed=5)
    x[1] = -77
    arr = fa.FlacArray.from_array(x, level=5)
    h = arr.histogram(bins=8, lo=I32_MIN, shift=31)
    check((h.counts, h.below, h.above), x, I32_MIN, 31, 8, what="one bin")
    assert np.all(h.counts[:, 0] + h.counts[:, 1] == x.shape[1])
    h = arr.histogram(bins=2048, streams=[1])
    assert h.counts[0, 0] == x.shape[1] and h.lo[0] == -77 and h.shift[0] == 0
    check((h.counts, h.below, h.above), x[[1]], -77, 0, 2048, what="constant")


# ---- sample ranges --------------------------------------------------------------------------------------------------------

def test_sample_ranges(fa, torch):
    shape, blk = (3, 65 * 1152 + 7), 1152
    x = int32_input(shape)
    n = shape[1]
    arr = int32_store(fa, shape, 1)
    d = device_store(torch, arr)
    lo, sh = M.auto_range(x, 512)
    for first, last in ((5, n - 3), (blk + 3, 3 * blk + 1), (blk + 3, blk + 4), (0, 1), (n - 1, n), (64 * blk - 1, 64 * blk + 1), (17, n), (2 * blk, 3 * blk)):
        got = host(fa.histogram_flac_device(*d, n, lo, sh, 512, first_sample=first, last_sample=last))
        check(got, x, lo, sh, 512, first, last, what=f"range {first}:{last}")
    # level 8: LPC frames, first inside the warm-up samples of a frame
    shape = (2, 3 * 4096 + 5)
    x = int32_input(shape)
    arr = fa.FlacArray.from_array(x, level=8)
    for first, last in ((4096 + 3, 4096 + 9), (4096 + 3, shape[1]), (1, 4097)):
        h = arr.histogram(bins=100, lo=-(2**19), shift=14, first=first, last=last)
        check((h.counts, h.below, h.above), x, -(2**19), 14, 100, first, last, what=f"L8 range {first}:{last}")


# ---- stream kinds ---------------------------------------------------------------------------------------------------------

def test_wasted_bits(fa):
    x = (sinusoid_noise_i32(3, 3 * 4096 + 11, seed=9) // 8 * 8).astype(np.int32)
    for level in (1, 5):
        h = fa.FlacArray.from_array(x, level=level).histogram(bins=2048)
        lo, sh = M.auto_range(x, 2048)
        check((h.counts, h.below, h.above), x, lo, sh, 2048, what=f"wasted L{level}")
    h = fa.FlacArray.from_array(x, level=5).histogram(bins=64, lo=-64, shift=0)
    check((h.counts, h.below, h.above), x, -64, 0, 64, what="wasted, unit bins")
    assert not h.counts[:, 1:8].any()  # (only multiples of 8 occur)


CORPUS = ["wasted_l3", "wasted_l1", "lpc_orders_l8", "lpc_limit_l8", "one_bit_l5", "verbatim_exact_l5", "tail_odd_l8", "len1_l5", "tail5_l5"]


@pytest.mark.parametrize("name", CORPUS)
def test_encoder_corpus(fa, name):
    """FIXED, LPC (orders 10 and 12 at level 8: the MO = 16 pass), VERBATIM and CONSTANT frames, wasted bits, short tails."""
    case = BY_NAME[name]
    x = case.x
    arr = fa.FlacArray.from_array(x, level=case.level)
    lo, sh = M.auto_range(x, 2048)
    h = arr.histogram(bins=2048)
    check((h.counts, h.below, h.above), x, lo, sh, 2048, what=name)
    h = arr.histogram(bins=7, lo=-3, shift=2)
    check((h.counts, h.below, h.above), x, -3, 2, 7, what=name + " fixed range")
    n = x.shape[1]
    if n > 10:
        h = arr.histogram(bins=33, lo=lo, shift=sh, first=3, last=n - 2)
        check((h.counts, h.below, h.above), x, lo, sh, 33, 3, n - 2, what=name + " range")


@pytest.fixture(scope="module")
def deep_mixes():
    return [W.deep_mix(101, 1), W.deep_mix(102, 2)]


def test_generated_foreign_streams(fa, torch, deep_mixes):
    """libFLAC-shaped streams whose frames cycle through LPC orders 1-8, 9-12, 13-16 and 17-32: all three history passes
    contribute to one histogram; one- and two-channel."""
    for b in deep_mixes:
        blob, st, nb = W.pack(b["streams"])
        d = tuple(torch.from_numpy(a).cuda() for a in (blob, st, nb))
        n, wide = b["n"], b["channels"] == 2
        x = np.asarray(b["samples"]).astype(np.int64 if wide else np.int32)
        lo, sh = M.auto_range(x, 1000)
        for first, last in ((0, n), (min(1, n - 1), n)):
            got = host(fa.histogram_flac_device(*d, n, lo, sh, 1000, first_sample=first, last_sample=last, is_int64=wide))
            check(got, x, lo, sh, 1000, first, last, what=b["name"])
        got = host(fa.histogram_flac_device(*d, n, 0, 3, 5, is_int64=wide))
        check(got, x, 0, 3, 5, what=b["name"] + " below and above")


def test_seektable_stripped(fa, torch):
    shape = (3, 65 * 1152 + 7)
    arr = int32_store(fa, shape, 1)
    blob, st, nb = strip_seektable(arr.compressed, arr.stream_starts, arr.stream_nbytes)
    d = tuple(torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in (blob, st, nb))
    x = int32_input(shape)
    lo, sh = M.auto_range(x, 128)
    for first, last in ((0, None), (1153, 70_001)):
        got = host(fa.histogram_flac_device(*d, shape[1], lo, sh, 128, first_sample=first, last_sample=last))
        check(got, x, lo, sh, 128, first, last, what="no seektable")


def test_mixed_block_sizes(fa, torch):
    n = 9000
    xa, xb = sinusoid_noise_i32(3, n, seed=41), sinusoid_noise_i32(4, n, seed=42)
    a, b = fa.FlacArray.from_array(xa, level=0), fa.FlacArray.from_array(xb, level=5)
    blob = np.concatenate([a.compressed, b.compressed])
    st = np.concatenate([a.stream_starts.reshape(-1), b.stream_starts.reshape(-1) + a.compressed.size]).astype(np.int64)
    nb = np.concatenate([a.stream_nbytes.reshape(-1), b.stream_nbytes.reshape(-1)]).astype(np.int64)
    order = np.array([0, 3, 1, 4, 5, 2, 6])  # the two classes interleaved: the rows have to be scattered back
    x = np.concatenate([xa, xb])[order]
    d = tuple(torch.from_numpy(np.ascontiguousarray(v)).cuda() for v in (blob, st[order], nb[order]))
    lo, sh = M.auto_range(x, 200)
    for first, last in ((0, None), (17, 8999)):
        check(host(fa.histogram_flac_device(*d, n, lo, sh, 200, first_sample=first, last_sample=last)), x, lo, sh, 200, first, last, what="mixed")
    sel = [6, 0, 1]
    check(host(fa.histogram_flac_device(*d, n, lo[sel], sh[sel], 200, streams=sel)), x[sel], lo[sel], sh[sel], 200, what="mixed subset")


# ---- subsets, repeat calls, side streams -------------------------------------------------------------------------------------

def test_streams_subset_and_empty(fa, torch):
    shape = (3, 65 * 1152 + 7)
    x = int32_input(shape)
    arr = int32_store(fa, shape, 1)
    d = device_store(torch, arr)
    for streams in ([2, 0], np.array([1]), [2, 1, 0]):
        idx = np.asarray(streams)
        lo, sh = M.auto_range(x[idx], 100)
        got = host(fa.histogram_flac_device(*d, shape[1], lo, sh, 100, first_sample=3, last_sample=70_000, streams=streams))
        check(got, x[idx], lo, sh, 100, 3, 70_000, what=f"subset {streams}")
        h = arr.histogram(bins=100, streams=streams)
        assert np.array_equal(h.lo, lo) and np.array_equal(h.shift, sh) and h.counts.shape == (idx.size, 100)
        check((h.counts, h.below, h.above), x[idx], lo, sh, 100, what=f"subset {streams} array")
    shape = (130, 2 * 1152)
    x = int32_input(shape)
    sel = [129, 5, 64, 63, 0, 77]
    h = int32_store(fa, shape, 1).histogram(bins=50, lo=-(2**17), shift=13, streams=sel)
    check((h.counts, h.below, h.above), x[sel], -(2**17), 13, 50, what="subset of short streams")
    c, b, a = fa.histogram_flac_device(*d, 65 * 1152 + 7, 0, 0, 9, streams=[])
    assert c.shape == (0, 9) and b.shape == (0,) and a.shape == (0,) and c.dtype == torch.int64


def test_a_second_call_does_not_accumulate(fa, torch):
    for shape in ((3, 65 * 1152 + 7), (70, 100)):
        x = int32_input(shape)
        d = device_store(torch, int32_store(fa, shape, 1))
        one = host(fa.histogram_flac_device(*d, shape[1], -(2**16), 9, 600))
        two = host(fa.histogram_flac_device(*d, shape[1], -(2**16), 9, 600))
        for p, q in zip(one, two):
            assert np.array_equal(p, q)
        check(two, x, -(2**16), 9, 600, what="second call")


def _i64_input(n_ch=4, n=3 * 4096 + 50, seed=11):
    """Values beyond 2^40 of both signs; row 0 holds a sample near INT64_MAX, row 1 one near INT64_MIN."""
    rng = np.random.default_rng(seed)
    x = sinusoid_noise_i32(n_ch, n, seed=seed).astype(np.int64) * (2**25 + 1) + rng.integers(-(2**20), 2**20, (n_ch, n))
    x[0, 100] = I64_MAX - 3
    x[1, 4099] = I64_MIN + 2
    return x


@pytest.mark.parametrize("kind", ["i32", "i32_subset", "i64"])
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
    lo, sh = (-(2**45), 36) if wide else (-(2**19), 10)
    kw = dict(is_int64=wide, streams=[4, 1] if kind == "i32_subset" else None)
    got, _ = T.run_delayed("histogram_" + kind, side, real, decoy, lambda c, st, nb: list(fa.histogram_flac_device(c, st, nb, n, lo, sh, 1024, **kw)))
    x = mk(31)
    if kind == "i32_subset":
        x = x[[4, 1]]
    check(tuple(got), x, lo, sh, 1024, what=kind)
    torch.cuda.synchronize()


# ---- wide stores ----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("level", [0, 5])
def test_int64_store(fa, torch, level):
    x = _i64_input()
    assert np.abs(x).max() > 2**40
    n = x.shape[1]
    arr = fa.FlacArray.from_array(x, level=level)
    d = device_store(torch, arr)
    blk = 1152 if level <= 2 else 4096
    two_frames = x.shape[0] * 2 * blk * 8
    for cap in (None, two_frames, 1):
        for lo, sh, nbins, first, last in ((I64_MIN, 53, 2048, 0, None), (I64_MIN + 1, 62, 3, 0, None), (-(2**45), 36, 1024, 0, None),
                                           (0, 40, 7, 77, n - 5), (-(2**45), 35, 2048, blk - 1, 2 * blk + 3)):
            got = host(fa.histogram_flac_device(*d, n, lo, sh, nbins, first_sample=first, last_sample=last, is_int64=True, max_temp_bytes=cap))
            check(got, x, lo, sh, nbins, first, last, what=f"i64 L{level} cap {cap} lo {lo}")
    got = host(fa.histogram_flac_device(*d, n, [0, -5], [30, 41], 100, streams=[3, 1], is_int64=True, max_temp_bytes=two_frames))
    check(got, x[[3, 1]], [0, -5], [30, 41], 100, what="i64 subset")
    h = arr.histogram(bins=2048)
    lo, sh = M.auto_range(x, 2048)
    assert np.array_equal(h.lo, lo) and np.array_equal(h.shift, sh) and sh[0] == 53
    check((h.counts, h.below, h.above), x, lo, sh, 2048, what="i64 auto")
    assert h.edges().dtype == object or h.edges().dtype == np.int64
    ix = fa.DeviceDecodeIndex(*d, n, is_int64=True)
    check(host(ix.histogram(lo, sh, 2048, first_sample=5, max_temp_bytes=two_frames // 2)), x, lo, sh, 2048, 5, None, what="i64 indexed")
    ix.close()


def test_float64_store(fa):
    rng = np.random.default_rng(4)
    x = sinusoid_noise_f32(3, 3 * 4096 + 50, seed=9).astype(np.float64) + 1e-9 * rng.normal(0.0, 1.0, (3, 3 * 4096 + 50))
    arr = fa.FlacArray.from_array(x, quanta=1e-12, level=5).to_device()
    ints = arr._index().decode().cpu().numpy()
    assert ints.dtype == np.int64 and np.abs(ints).max() > 2**32
    h = arr.histogram(bins=500)
    lo, sh = M.auto_range(ints, 500)
    assert np.array_equal(h.lo, lo) and np.array_equal(h.shift, sh)
    check((h.counts, h.below, h.above), ints, lo, sh, 500, what="f64")
    fe = h.float_edges()
    off, gain = np.asarray(arr.stream_offsets, np.float64), np.asarray(arr.stream_gains, np.float64)
    assert fe.shape == (3, 501) and np.array_equal(fe[:, 0], off + lo.astype(np.float64) / gain)
    dec = arr.to_array()
    n = x.shape[1]
    ranks = np.array([0, 1, n // 2, n - 1])
    got = arr.order_statistic(ranks)
    assert got.dtype == np.float64 and Q.bits_equal(got, np.sort(dec, axis=1)[:, ranks])
    arr.release_device()


def test_float32_store(fa, torch):
    shape = (3, 65 * 1152 + 7)
    x = sinusoid_noise_f32(*shape)
    arr = fa.FlacArray.from_array(x, quanta=1e-4, level=1)
    ints, off, gain = Q.float32_to_int32(x, 1e-4)  # the oracle-side quantised integers
    ints = np.asarray(ints).reshape(shape)
    h = arr.histogram(bins=777)
    lo, sh = M.auto_range(ints, 777)
    assert np.array_equal(h.lo, lo) and np.array_equal(h.shift, sh)
    check((h.counts, h.below, h.above), ints, lo, sh, 777, what="f32")
    assert np.array_equal(h.offsets, np.asarray(arr.stream_offsets, np.float64)) and h.float_edges().shape == (3, 778)
    dec = arr.to_array()
    ranks = np.array([0, 7, shape[1] // 2, shape[1] - 1])
    got = arr.order_statistic(ranks)
    assert got.dtype == np.float32 and Q.bits_equal(got, np.sort(dec, axis=1)[:, ranks])
    assert Q.bits_equal(arr.quantile(0.5), np.quantile(dec, 0.5, axis=1, method="lower"))


# ---- entry points agree -----------------------------------------------------------------------------------------------------

def _fields(h):
    return [h.counts, h.below, h.above, h.lo, h.shift]


def test_entry_points_agree_also_after_append_and_overwrite(fa, torch):
    x = sinusoid_noise_i32(4, 20_000, seed=21)
    more = sinusoid_noise_i32(4, 5000, seed=22)
    patch = sinusoid_noise_i32(2, 3000, seed=23, amp=2**20)
    host_arr = fa.FlacArray.from_array(x, level=5)
    arr = fa.FlacArray(host_arr).to_device()

    def agree(y, what):
        n = y.shape[1]
        lo, sh = M.auto_range(y, 300)
        d = device_store(torch, arr)
        direct = host(fa.histogram_flac_device(*d, n, lo, sh, 300, first_sample=9, last_sample=n - 1))
        check(direct, y, lo, sh, 300, 9, n - 1, what=what)
        ix = fa.DeviceDecodeIndex(*d, n)
        for p, q in zip(direct, host(ix.histogram(lo, sh, 300, first_sample=9, last_sample=n - 1))):
            assert np.array_equal(p, q), what
        ix.close()
        h = arr.histogram(bins=300, lo=lo, shift=sh, first=9, last=n - 1)
        for p, q in zip(direct, (h.counts, h.below, h.above)):
            assert np.array_equal(p, q), what
        check(_fields(arr.histogram(bins=300))[:3], y, lo, sh, 300, what=what + " auto")

    agree(x, "resident")
    for p, q in zip(_fields(host_arr.histogram(bins=300, first=9)), _fields(arr.histogram(bins=300, first=9))):
        assert np.array_equal(p, q)
    arr.append(more, level=5)
    y = np.concatenate([x, more], axis=1)
    agree(y, "appended")
    arr.overwrite(4000, patch, streams=[3, 1], level=5)
    y[[3, 1], 4000:7000] = patch
    agree(y, "overwritten")
    n = y.shape[1]
    assert np.array_equal(arr.order_statistic([0, n // 2, n - 1]), np.sort(y, axis=1)[:, [0, n // 2, n - 1]])
    arr.release_device()


def test_leading_shapes(fa):
    x = sinusoid_noise_i32(6, 5000, seed=3).reshape(2, 3, 5000)
    arr = fa.FlacArray.from_array(x, level=5)
    h = arr.histogram(bins=40)
    assert h.counts.shape == (2, 3, 40) and h.below.shape == (2, 3) and h.lo.shape == (2, 3) and h.edges().shape == (2, 3, 41)
    lo, sh = M.auto_range(x.reshape(6, -1), 40)
    check((h.counts, h.below, h.above), x.reshape(6, -1), lo, sh, 40, what="2-D lead")
    v = arr.order_statistic([0, 2500, 4999])
    assert v.shape == (2, 3, 3) and np.array_equal(v, np.sort(x, axis=-1)[..., [0, 2500, 4999]])
    assert arr.median().shape == (2, 3) and np.array_equal(arr.median(), np.median(x, axis=-1))
    a1 = fa.FlacArray.from_array(x[0, 0], level=5)
    assert a1.histogram(bins=5).counts.shape == tuple(a1.leading_shape) + (5,)
    assert np.array_equal(a1.order_statistic([17]).reshape(-1), np.sort(x[0, 0])[[17]])


# ---- damage -----------------------------------------------------------------------------------------------------------------

def test_damaged_frame_raises(fa, torch):
    """One bit of a residual of the last frame: only the frame's CRC-16 can tell (verify=True)."""
    shape = (3, 2 * 1152 + 1)
    arr = int32_store(fa, shape, 1)
    blob = np.array(arr.compressed, copy=True)
    blob[blob.size - 5] ^= 0x04
    st, nb = np.asarray(arr.stream_starts).reshape(-1), np.asarray(arr.stream_nbytes).reshape(-1)
    d = tuple(torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in (blob, st, nb))
    with pytest.raises(RuntimeError):
        fa.histogram_flac_device(*d, shape[1], -(2**19), 10, 1024, verify=True)
    # the undamaged store still counts (nothing of the failed call is left behind)
    h = arr.histogram(bins=1024, lo=-(2**19), shift=10)
    check((h.counts, h.below, h.above), int32_input(shape), -(2**19), 10, 1024, what="after a damaged store")


# ---- order statistics ---------------------------------------------------------------------------------------------------------

def test_every_rank_of_a_small_store(fa):
    shape = (3, 2 * 1152 + 1)
    x = int32_input(shape)
    arr = fa.FlacArray(int32_store(fa, shape, 1)).to_device()
    got = arr.order_statistic(np.arange(shape[1]))
    assert got.dtype == np.int32 and got.shape == shape
    assert np.array_equal(got, np.sort(x, axis=1))
    arr.release_device()


def test_every_rank_of_a_tiny_range(fa):
    """Every rank of a range of 37 samples that straddles a frame boundary, and of ranges of one and two samples."""
    shape = (3, 2 * 1152 + 1)
    x = int32_input(shape)
    arr = fa.FlacArray(int32_store(fa, shape, 1)).to_device()
    for first, last in ((1140, 1177), (5, 6), (2 * 1152 - 1, 2 * 1152 + 1)):
        n = last - first
        got = arr.order_statistic(np.arange(n), first=first, last=last)
        assert got.dtype == np.int32 and np.array_equal(got, np.sort(x[:, first:last], axis=1)), (first, last)
    arr.release_device()


def test_ranks_on_full_range_data(fa, monkeypatch):
    x = full_range_i32((3, 2 * 4096 + 100))
    arr = fa.FlacArray.from_array(x, level=5).to_device()
    n = x.shape[1]
    calls = []
    real = fa.DeviceDecodeIndex.histogram
    monkeypatch.setattr(fa.DeviceDecodeIndex, "histogram", lambda self, *a, **k: (calls.append(1), real(self, *a, **k))[1])
    got = arr.order_statistic([0, n // 2, n - 1])
    assert np.array_equal(got, np.sort(x, axis=1)[:, [0, n // 2, n - 1]])
    assert got[0, 0] == I32_MIN and got[0, 2] == I32_MAX
    assert len(calls) == 1 + 3 * 2  # the shared coarse pass, then 21 -> 10 -> 0 for each of the three ranks
    arr.release_device()


def test_per_row_ranks(fa):
    shape = (70, 100)
    x = int32_input(shape)
    arr = int32_store(fa, shape, 1)
    rng = np.random.default_rng(8)
    rk = rng.integers(0, 100, (70, 3))
    got = arr.order_statistic(rk)
    assert got.shape == (70, 3) and np.array_equal(got, np.take_along_axis(np.sort(x, axis=1), rk, axis=1))
    sel = [69, 0, 33]
    rk2 = rng.integers(0, 90, (3, 2))
    assert np.array_equal(arr.order_statistic(rk2, first=10, last=100, streams=sel), np.take_along_axis(np.sort(x[sel, 10:100], axis=1), rk2, axis=1))


def test_ranks_on_a_full_range_int64_store(fa):
    rng = np.random.default_rng(12)
    x = rng.integers(I64_MIN, I64_MAX, (2, 4096 + 77), dtype=np.int64, endpoint=True)
    x[0, 5], x[0, 6] = I64_MIN, I64_MAX
    arr = fa.FlacArray.from_array(x, level=5)
    n = x.shape[1]
    ranks = [0, 1, n // 2, n - 2, n - 1]
    got = arr.order_statistic(ranks)
    assert got.dtype == np.int64 and np.array_equal(got, np.sort(x, axis=1)[:, ranks])
    x2 = _i64_input()
    arr2 = fa.FlacArray.from_array(x2, level=5)
    n2 = x2.shape[1]
    assert np.array_equal(arr2.order_statistic([0, n2 // 3, n2 - 1]), np.sort(x2, axis=1)[:, [0, n2 // 3, n2 - 1]])


def test_quantile(fa):
    x = int32_input((3, 2 * 1152 + 1))  # n - 1 = 2304, a multiple of 4
    arr = int32_store(fa, (3, 2 * 1152 + 1), 1)
    for method in ("lower", "higher"):
        for q in (0, 0.25, 0.5, 0.75, 1):
            got = arr.quantile(q, method=method)
            assert got.shape == (3,) and got.dtype == np.int32
            assert np.array_equal(got, np.quantile(x, q, axis=1, method=method)), (q, method)
        qs = [0.1, 0.37, 0.9999]
        got = arr.quantile(qs, method=method, first=3, last=2001)  # an arbitrary n: the stated rank rule
        srt = np.sort(x[:, 3:2001], axis=1)
        want = np.stack([srt[:, M.quantile_rank(q, 1998, method)] for q in qs], axis=1)
        assert got.shape == (3, 3) and np.array_equal(got, want), method
        assert np.array_equal(got, np.quantile(x[:, 3:2001], qs, axis=1, method=method).T), method


def test_median(fa):
    x = int32_input((3, 2 * 1152 + 1))
    arr = int32_store(fa, (3, 2 * 1152 + 1), 1)
    m = arr.median()
    assert m.dtype == np.float64 and np.array_equal(m, np.median(x, axis=1))  # odd n
    assert np.array_equal(arr.median(first=1), np.median(x[:, 1:], axis=1))  # even n
    assert np.array_equal(arr.median(first=10, last=12, streams=[2]), np.median(x[[2], 10:12], axis=1))
    y = full_range_i32((2, 1000))
    assert np.array_equal(fa.FlacArray.from_array(y, level=5).median(), np.median(y, axis=1))
