"""FlacArray.dot / dot_flac_device / DeviceDecodeIndex.dot against Python integers on the known samples: every cell of
x[rows, first:last] @ T.T, exactly, on the stores of tests/dot_corpus.py -- waves whose 64 frames are decoded by different
history passes and carry different wasted bits, ranges that begin among warm-up samples and off tile boundaries, one to
three template passes and the seam between them, templates and samples at both ends of int32, templates across all of
int64, a two-channel store in column chunks, a float store with per-row gains, the frame check, dirty scratch, and refusals
that must leave the caller's arrays alone."""
import functools
import math

import numpy as np
import pytest

from tests import dot_corpus as C

pytestmark = pytest.mark.gpu


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


def up(torch, store):
    return tuple(torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in store)


STORES = {"A": C.store_a, "B": C.store_b, "D": C.store_d}


@functools.lru_cache(maxsize=None)
def want(store_name, K, first, last, sub):
    """(templates int64 [K, n], oracle [rows, K]) -- computed once per case and shared by the layouts and routes."""
    st = STORES[store_name]()
    T = C.templates(K, last - first)
    return T, C.oracle(st.samples, T, first, last, C.subset(st.samples.shape[0]) if sub else None)


def same(got, exp, what):
    assert got.shape == exp.shape, what
    bad = np.argwhere(got != exp)
    assert bad.size == 0, (what, bad[:4].tolist(), [(got[tuple(b)], exp[tuple(b)]) for b in bad[:2]])


def _array_of(fa, st, layout, dtype=np.int32):
    blob, starts, nbytes = st.layouts[layout]
    return fa.FlacArray(None, shape=st.samples.shape, global_shape=None, compressed=blob, dtype=np.dtype(dtype), stream_starts=starts,
                        stream_nbytes=nbytes)


# ---- stores A and B: every K over every range, both layouts, every route ---------------------------------------------------

@pytest.mark.parametrize("layout", ["libflac", "own"])
@pytest.mark.parametrize("name", ["A", "B"])
def test_writer_stores_every_k_and_range(fa, torch, name, layout):
    st = STORES[name]()
    d = up(torch, st.layouts[layout])
    ix = fa.DeviceDecodeIndex(*d, st.n)
    arr = _array_of(fa, st, layout)
    res = _array_of(fa, st, layout)
    res.to_device()
    for ri, (first, last) in enumerate(C.ranges(st.n, st.block)):
        for K in C.KS:
            sub = (ri + K) % 2 == 1  # (half of the cases on the permuted subset of 67, K = 9 and 17 on the whole range among them)
            sel = C.subset() if sub else None
            T, exp = want(name, K, first, last, sub)
            T32 = torch.from_numpy(T.astype(np.int32)).cuda()
            what = (name, layout, K, first, last, sub)
            same(fa.dot_exact(*fa.dot_flac_device(*d, st.n, T32, first, last, streams=sel)), exp, what + ("device",))
            same(fa.dot_exact(*ix.dot(T32, first, last, streams=sel)), exp, what + ("index",))
            for a, route in ((arr, "array"), (res, "resident")):
                got = a.dot(T, first=first, last=last, streams=sel)
                assert got.count == last - first and list(got.template_sum) == [sum(int(v) for v in row) for row in T], what
                same(got.exact, exp, what + (route,))
    res.release_device()
    ix.close()


def test_one_template_without_its_axis_and_the_leading_shape(fa):
    st = C.store_a()
    blob, starts, nbytes = st.layouts["own"]
    x = st.samples[:130]
    arr = fa.FlacArray(None, shape=(10, 13, st.n), global_shape=None, compressed=blob[: int(starts[130])], dtype=np.dtype(np.int32),
                       stream_starts=starts[:130].reshape(10, 13), stream_nbytes=nbytes[:130].reshape(10, 13))
    T = C.templates(3, st.n)
    got = arr.dot(T)
    assert got.exact.shape == (10, 13, 3) and got.value().shape == (10, 13, 3)
    exp = C.oracle(x, T, 0, st.n)
    same(got.exact.reshape(130, 3), exp, "leading shape")
    assert np.array_equal(got.value().reshape(130, 3), np.array([[float(v) for v in r] for r in exp]))
    one = arr.dot(T[1])
    assert one.exact.shape == (10, 13) and one.template_sum == sum(int(v) for v in T[1])
    same(one.exact.reshape(130), exp[:, 1], "one template")
    sub = arr.dot(T[1], streams=[7, 0, 129])
    same(sub.exact, exp[[7, 0, 129], 1], "one template, streams")


# ---- the limb signs: full-range samples against constant extreme templates ------------------------------------------------

@pytest.mark.parametrize("resident", [False, True])
def test_library_stores_against_constant_extreme_templates(fa, resident):
    for x, ranges in ((C.samples_c(), ((0, None), (4090, 4100))), (C.samples_extremes(), ((0, None), (0, 1), (C.EXT_BLOCK - 1, C.EXT_BLOCK + 1)))):
        arr = fa.FlacArray.from_array(x, level=5)
        if resident:
            arr.to_device()
        for first, last in ranges:
            last = x.shape[1] if last is None else last
            T = C.constant_templates(last - first)
            got = arr.dot(T, first=first, last=last, verify=True)
            same(got.exact, C.oracle(x, T, first, last), (x.shape, first, last, resident))
        # and mixed: a sign error in either limb shows against templates of both signs
        T = C.templates(3, x.shape[1], seed=1)
        same(arr.dot(T).exact, C.oracle(x, T, 0, x.shape[1]), (x.shape, "mixed"))
        if resident:
            arr.release_device()


# ---- wide templates ----------------------------------------------------------------------------------------------------

def test_wide_templates_and_the_common_mode(fa):
    st = C.store_a()
    arr = _array_of(fa, st, "libflac")
    for first, last in ((0, st.n), (st.block - 13, st.block + 45)):
        T = C.wide_templates(last - first)
        got = arr.dot(T, first=first, last=last)
        same(got.exact, C.oracle(st.samples, T, first, last), ("wide", first, last))
        assert list(got.template_sum) == [sum(int(v) for v in row) for row in T]
    cm = arr.common_mode().sum[0]
    assert cm.dtype == np.int64 and np.abs(cm).max() > 2**31  # (it has left int32: the split is needed)
    got = arr.dot(cm)
    same(got.exact, C.oracle(st.samples, cm[None, :], 0, st.n)[:, 0], "common mode")


# ---- store D: two channels, column chunks ------------------------------------------------------------------------------

@pytest.mark.parametrize("layout", ["libflac", "own"])
def test_two_channel_store_in_column_chunks(fa, torch, layout):
    st = C.store_d()
    d = up(torch, st.layouts[layout])
    ix = fa.DeviceDecodeIndex(*d, st.n, is_int64=True)
    for first, last in C.ranges(st.n, st.block):
        for K in (1, 9):
            T = C.templates(K, last - first)
            T32 = torch.from_numpy(T.astype(np.int32)).cuda()
            for cap in (None, 5 * 64 * 8):  # everything in one chunk; a frame per chunk
                for sel in (None, np.array([4, 1, 2])):
                    exp = C.oracle(st.samples, T, first, last, sel)
                    what = (layout, first, last, K, cap, sel is None)
                    out = fa.dot_flac_device(*d, st.n, T32, first, last, streams=sel, is_int64=True, max_temp_bytes=cap)
                    assert tuple(out.shape) == (exp.shape[0], K, 4), what
                    same(fa.dot_exact(out), exp, what)
                    same(fa.dot_exact(ix.dot(T32, first, last, streams=sel, max_temp_bytes=cap)), exp, what + ("index",))
    ix.close()
    # through the array, with wide templates and samples at the ends of int64
    big = np.array([[C.INT64_MAX, C.INT64_MIN, -1, 2**40], [C.INT64_MIN, C.INT64_MIN, C.INT64_MAX, 0]], dtype=np.int64)
    T = np.array([[C.INT64_MIN, C.INT64_MAX, 2**31, -(2**31) - 1], [1, -1, C.INT32_MIN, C.INT32_MAX]], dtype=np.int64)
    same(fa.FlacArray.from_array(big, level=5).dot(T).exact, C.oracle(big, T, 0, 4), "int64 extremes")


# ---- a float32 store with per-row gains ----------------------------------------------------------------------------------

def test_float32_store_with_per_row_gains(fa, torch):
    rng = np.random.default_rng(9)
    x = (rng.normal(0.0, 1.0, (6, 500)) * (10.0 ** np.arange(6))[:, None] + rng.uniform(-3, 3, (6, 1))).astype(np.float32)
    arr = fa.FlacArray.from_array(x, precision=3, level=5)
    gains = np.asarray(arr.stream_gains).reshape(-1)
    assert np.unique(gains).size > 1
    comp, st, nb = (torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in (arr.compressed, arr.stream_starts, arr.stream_nbytes))
    ints = fa.decode_flac_device(comp, st, nb, 500).cpu().numpy()  # the quantised integers: a decode with no offsets
    first, last = 7, 493
    T = rng.integers(-1000, 1000, (3, last - first)).astype(np.int64)
    T[2] = 1
    got = arr.dot(T, first=first, last=last)
    exp = C.oracle(ints, T, first, last)
    same(got.exact, exp, "f32 ints")
    q = arr.dot(T, first=first, last=last, quantised=True)
    assert q.gain is None and np.array_equal(q.value(), np.array([[float(v) for v in r] for r in exp]))
    # value() against the decoded floats, cell by cell: the restore rounds each float32 sample by at most 2^-24 relative and
    # value() does not; the factor two covers the float64 roundings of either side
    dec = arr.to_array().astype(np.float64)[:, first:last]
    v = got.value()
    assert v.shape == (6, 3) and v.dtype == np.float64
    for r in range(6):
        for k in range(3):
            terms = [float(a) * float(b) for a, b in zip(dec[r], T[k])]
            ref, scale = math.fsum(terms), math.fsum(abs(t) for t in terms)
            err = abs(v[r, k] - ref)
            print("float32 store: row %d template %d |value - fsum| = %.3e, bound %.3e" % (r, k, err, 2.0**-23 * scale))
            assert err <= 2.0**-23 * scale, (r, k)


# ---- the frame check -----------------------------------------------------------------------------------------------------

def test_verify_passes_clean_and_fails_damaged_with_the_plain_decodes_error(fa, torch):
    st = C.store_a()
    T32 = torch.from_numpy(C.templates(9, st.n).astype(np.int32)).cuda()
    exp = want("A", 9, 0, st.n, False)[1]
    clean = up(torch, st.layouts["own"])
    same(fa.dot_exact(*fa.dot_flac_device(*clean, st.n, T32, verify=True)), exp, "clean, verified")
    blob, starts, nbytes = (np.array(a, copy=True) for a in st.layouts["own"])
    end = int(starts[40] + nbytes[40])
    blob[end - 1] ^= 0x01  # the low byte of the last frame's CRC-16 of stream 40: the samples still decode
    d = up(torch, (blob, starts, nbytes))
    with pytest.raises(RuntimeError) as plain:
        fa.decode_flac_device(*d, st.n, verify=True)
    with pytest.raises(RuntimeError) as e:
        fa.dot_flac_device(*d, st.n, T32, verify=True)
    assert str(e.value) == str(plain.value)
    ix = fa.DeviceDecodeIndex(*d, st.n)
    with pytest.raises(RuntimeError) as e:
        ix.dot(T32, verify=True)
    assert str(e.value) == str(plain.value)
    same(fa.dot_exact(*ix.dot(T32, verify=False)), exp, "unverified")
    ix.close()


# ---- refusals --------------------------------------------------------------------------------------------------------------

def test_refusals_leave_the_result_arrays_unwritten(fa, torch):
    from flacarray_amd import _lib
    from flacarray_amd.libflacarray import _dot_args, _dp, _stream_ptr

    L = _lib.lib()
    st = C.store_a()
    comp, starts, nbytes = up(torch, st.layouts["libflac"])
    n = st.n
    _, _, order, rows = _dot_args(131, n, 0, None, None)
    order_d, rows_d = torch.from_numpy(order).cuda(), torch.from_numpy(rows).cuda()
    K, ld = 9, 16
    T = C.templates(K, n)
    img = torch.zeros((n, ld), dtype=torch.int32, device="cuda")
    img[:, :K] = torch.from_numpy(T.astype(np.int32)).cuda().t()
    sentinel = 0x5A5A5A5A5A5A5A5A
    hi, lo = (torch.full((131, K), sentinel, dtype=torch.int64, device="cuda") for _ in range(2))
    out4 = torch.full((131, K, 4), sentinel, dtype=torch.int64, device="cuda")
    ix = fa.DeviceDecodeIndex(comp, starts, nbytes, n)

    def i32(first=0, last=n, n_sel=131, order_p=_dp(order_d), n_rows=3, rows_p=_dp(rows_d), K=K, ld=ld, img_p=_dp(img), hi_p=_dp(hi), lo_p=_dp(lo),
            n_stream=131, size=n):
        return L.fa_dot_i32_device(_dp(comp), comp.numel(), _dp(starts), _dp(nbytes), n_stream, size, first, last, n_sel, order_p, n_rows, rows_p, K,
                                   ld, img_p, hi_p, lo_p, _stream_ptr(), 0)

    def i64(K=K, ld=ld, out_p=_dp(out4), first=0, last=n):
        return L.fa_dot_i64_device(_dp(comp), comp.numel(), _dp(starts), _dp(nbytes), 131, n, first, last, 131, _dp(order_d), 3, _dp(rows_d), K, ld,
                                   _dp(img), 0, out_p, _stream_ptr(), 0)

    def indexed(first=0, last=n, n_sel=131, n_rows=3, K=K, ld=ld, hi_p=_dp(hi), lo_p=_dp(lo), handle=ix._h):
        return L.fa_dot_indexed(handle, first, last, n_sel, _dp(order_d), n_rows, _dp(rows_d), K, ld, _dp(img), 0, hi_p, lo_p, None, _stream_ptr(), 0)

    RANGE = i32(first=10, last=10)  # FA_ERROR_DECODE_SAMPLE_RANGE, as an empty range is refused
    assert RANGE != 0 and RANGE != i32(order_p=None)
    sample_range = [i32(K=0), i32(K=-1), i32(ld=8), i32(ld=12), i32(ld=9), i32(K=1, ld=0), i64(K=0), i64(ld=12), indexed(K=0), indexed(ld=15),
                    i32(first=11, last=10), i32(first=0, last=n + 1), i32(first=-1, last=5), indexed(first=10, last=10)]
    assert all(rc == RANGE for rc in sample_range), (RANGE, sample_range)
    refused = [i32(n_sel=-1), i32(n_sel=132), i32(n_rows=0), i32(n_rows=2), i32(n_rows=4), i32(order_p=None), i32(rows_p=None), i32(img_p=None),
               i32(hi_p=None), i32(lo_p=None), i32(n_stream=0), i32(size=0), i64(out_p=None), indexed(hi_p=None), indexed(n_rows=0),
               indexed(handle=None)]
    assert all(rc != 0 for rc in refused), refused
    torch.cuda.synchronize()
    for o in (hi, lo, out4):
        assert bool((o == sentinel).all())
    # a range of 2^32 samples is refused before anything else is looked at: streams "of" 2^32 + 8 samples named by the
    # arguments alone (the store is not read before the arguments are accepted)
    assert i32(first=0, last=2**32, size=2**32 + 8) == RANGE
    torch.cuda.synchronize()
    assert bool((hi == sentinel).all()) and bool((lo == sentinel).all())
    # the accepted call fills both
    assert i32() == 0
    same(fa.dot_exact(hi, lo), want("A", K, 0, n, False)[1], "after the refusals")
    assert indexed() == 0
    same(fa.dot_exact(hi, lo), want("A", K, 0, n, False)[1], "indexed, after the refusals")
    ix.close()


# ---- scratch and repeatability -------------------------------------------------------------------------------------------

def test_dirty_scratch_a_larger_call_before_and_repeats(fa, torch):
    import ctypes

    from flacarray_amd import _lib

    L = _lib.lib()
    st = C.store_a()
    d = up(torch, st.layouts["libflac"])
    sel = C.subset()
    T32 = torch.from_numpy(want("A", 17, 1, st.n, True)[0].astype(np.int32)).cuda()
    call = lambda: tuple(t.cpu().numpy() for t in fa.dot_flac_device(*d, st.n, T32, 1, st.n, streams=sel))  # noqa: E731

    def slots():
        sizes = (ctypes.c_int64 * 64)()
        n = L.fa_debug_scratch_bytes(sizes, 64)
        return {i for i in range(min(n, 64)) if sizes[i] > 0}

    other = C.store_b()
    od = up(torch, other.layouts["libflac"])
    fa.reduce_flac_device(*od, other.n, width=7, streams=np.arange(130, -1, -1))
    before = slots()
    clean = call()
    same(fa.dot_exact(*clean), want("A", 17, 1, st.n, True)[1], "clean")
    again = call()  # the call zero-fills its outputs: a second one is the first one
    for a, b in zip(clean, again):
        assert np.array_equal(a, b)
    torch.cuda.synchronize()
    assert L.fa_debug_scratch_fill(0xA5) == 0
    dirty = call()
    for a, b in zip(clean, dirty):
        assert np.array_equal(a, b)
    # a larger reduce call on another store leaves its task table and frame table in the slots this call uses
    fa.reduce_flac_device(*od, other.n, width=7, streams=np.arange(130, -1, -1))
    after = call()
    for a, b in zip(clean, after):
        assert np.array_equal(a, b)
    assert slots() <= before, (slots(), before)  # no slot beyond those the reductions already leave
    # two channels: the chunk route stays inside the reductions' slots as well
    dd = C.store_d()
    d2 = up(torch, dd.layouts["libflac"])
    fa.reduce_flac_device(*d2, dd.n, width=7, is_int64=True)
    before = slots()
    t2 = torch.from_numpy(C.templates(3, dd.n).astype(np.int32)).cuda()
    fa.dot_flac_device(*d2, dd.n, t2, is_int64=True, max_temp_bytes=5 * 64 * 8)
    assert slots() <= before, (slots(), before)
