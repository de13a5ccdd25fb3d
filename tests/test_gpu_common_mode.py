"""FlacArray.common_mode / common_mode_flac_device / DeviceDecodeIndex.common_mode against numpy on the known samples:
per group and sample the exact int64 sum over the group's streams and the two limbs of the sum of squares (the squares
checked as Python integers), on the stores of tests/xsum_corpus.py -- waves whose 64 frames are decoded by different
history passes and carry different wasted bits, partial tiles, ranges that begin and end inside tiles, groups of 0, 1, 63,
64, 65 and 130 streams with interleaved labels, two-channel stores in column chunks, float stores, dirty scratch, a damaged
frame, and refusals that must leave the caller's arrays alone."""
import functools

import numpy as np
import pytest

from tests import xsum_corpus as C

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


@functools.lru_cache(maxsize=None)
def want(store_name, first, last, grouping):
    """The expected fields, computed once per (store, range, grouping) and shared by the routes."""
    st = {"A": C.store_a, "B": C.store_b, "D": C.store_d}[store_name]()
    _, sel, lab, G = next(g for g in C.groupings() if g[0] == grouping) if store_name != "D" else ("one", None, None, 1)
    return C.expected(st.samples, first, last, sel, lab, G)


def check(got, exp, what):
    """`got`: (sum, sumsq_hi, sumsq_lo) device tensors or numpy arrays; `exp`: C.expected's (count, sum, squares)."""
    sm, qh, ql = (None if t is None else (t if isinstance(t, np.ndarray) else t.cpu().numpy()) for t in got)
    _, e_sum, e_sq = exp
    assert sm.shape == e_sum.shape and sm.dtype == np.int64, what
    assert np.array_equal(sm, e_sum), what
    if e_sq is None:
        assert qh is None and ql is None, what
        return
    assert qh.shape == e_sum.shape and ql.shape == e_sum.shape, what
    # the limbs themselves (sums of x*x >> 32 and x*x mod 2^32) are pinned by the store C test; here their total, exactly
    total = qh.view(np.uint64).astype(object) * (1 << 32) + ql.view(np.uint64).astype(object)
    assert np.array_equal(total, e_sq), what


def limbs(x, sel):
    """The exact limbs of one group: sums over the streams `sel` of x*x >> 32 and x*x mod 2^32, uint64."""
    q = (x[sel].astype(np.int64) * x[sel].astype(np.int64)).astype(np.uint64)
    return (q >> np.uint64(32)).sum(axis=0), (q & np.uint64(0xFFFFFFFF)).sum(axis=0)


# ---- stores A and B: every grouping over every range, both layouts, both routes -------------------------------------------

@pytest.mark.parametrize("layout", ["libflac", "own"])
@pytest.mark.parametrize("name", ["A", "B"])
def test_writer_stores_every_grouping_and_range(fa, torch, name, layout):
    st = {"A": C.store_a, "B": C.store_b}[name]()
    d = up(torch, st.layouts[layout])
    ix = fa.DeviceDecodeIndex(*d, st.n)
    for gname, sel, lab, G in C.groupings():
        n_groups = None if lab is None else G
        for first, last in C.ranges(st.n, st.block):
            exp = want(name, first, last, gname)
            what = (name, layout, gname, first, last)
            got = fa.common_mode_flac_device(*d, st.n, groups=lab, n_groups=n_groups, first_sample=first, last_sample=last, streams=sel)
            check(got, exp, what + ("device",))
            got = ix.common_mode(groups=lab, n_groups=n_groups, first_sample=first, last_sample=last, streams=sel)
            check(got, exp, what + ("index",))
            if first == 0 and last == st.n and lab is not None:
                # the limbs one by one, and squares=False
                x = st.samples
                for g in range(G):
                    hi, lo = limbs(x, sel[lab == g])
                    assert np.array_equal(got[1][g].cpu().numpy().view(np.uint64), hi) and np.array_equal(got[2][g].cpu().numpy().view(np.uint64), lo), what
                only = fa.common_mode_flac_device(*d, st.n, groups=lab, n_groups=n_groups, streams=sel, squares=False)
                assert only[1] is None and only[2] is None and np.array_equal(only[0].cpu().numpy(), exp[1]), what
    ix.close()


def test_count_of_every_group(fa):
    st = C.store_a()
    arr = _array_of(fa, st, "own")
    for gname, sel, lab, G in C.groupings():
        s = arr.common_mode(groups=lab, streams=sel, first=3, last=40)
        exp = want("A", 3, 40, gname)
        seen = exp[0][: s.count.size]  # (G = largest label + 1: trailing empty groups are not there)
        assert np.array_equal(s.count, seen) and np.all(exp[0][s.count.size :] == 0), gname
        check((s.sum, s.sumsq_hi, s.sumsq_lo), tuple(e[: s.count.size] for e in exp), gname)
        empty = s.count == 0
        assert np.all(np.isnan(s.mean()[empty])) and np.all(np.isnan(s.std()[empty])) and not np.any(np.isnan(s.mean()[~empty])), gname


def _array_of(fa, st, layout, dtype=np.int32):
    blob, starts, nbytes = st.layouts[layout]
    return fa.FlacArray(None, shape=st.samples.shape, global_shape=None, compressed=blob, dtype=np.dtype(dtype), stream_starts=starts,
                        stream_nbytes=nbytes)


# ---- store C: written by the library, squares past 2^64 --------------------------------------------------------------------

@pytest.mark.parametrize("resident", [False, True])
@pytest.mark.parametrize("verify", [None, True])
def test_library_store_full_range(fa, resident, verify):
    x = C.samples_c()
    arr = fa.FlacArray.from_array(x, level=5)
    if resident:
        arr.to_device()
    lab = np.arange(70) % 2
    for kw, sel, labels, G in ((dict(), None, None, 1), (dict(groups=lab, first=4000, last=4196), None, lab, 2),
                               (dict(streams=np.arange(69, -1, -1), first=4090, last=4100), np.arange(69, -1, -1), None, 1)):
        first, last = kw.get("first", 0), kw.get("last", x.shape[1])
        s = arr.common_mode(verify=verify, **kw)
        exp = C.expected(x, first, last, sel, labels, G)
        assert np.array_equal(s.count, exp[0])
        check((s.sum, s.sumsq_hi, s.sumsq_lo), exp, (resident, verify, kw.keys()))
        idx = np.arange(70) if sel is None else sel
        for g in range(G):
            hi, lo = limbs(x[:, first:last], idx[(np.zeros(70, int) if labels is None else labels) == g])
            assert np.array_equal(s.sumsq_hi[g], hi) and np.array_equal(s.sumsq_lo[g], lo)
        if not kw:
            assert s.sumsq_hi.dtype == np.uint64 and s.sumsq_hi.max() > 2**32
            m = s.mean()
            assert np.array_equal(m[0], np.array([int(v) / 70 for v in exp[1][0]]))
    if resident:
        arr.release_device()


# ---- store D: two channels, the sum modulo 2^64 -----------------------------------------------------------------------------

@pytest.mark.parametrize("layout", ["libflac", "own"])
def test_two_channel_store_in_column_chunks(fa, torch, layout):
    st = C.store_d()
    d = up(torch, st.layouts[layout])
    x = st.samples
    lab = np.array([1, 0, 1, 1, 0])
    ix = fa.DeviceDecodeIndex(*d, st.n, is_int64=True)
    for first, last in C.ranges(st.n, st.block):
        for cap in (None, 5 * 64 * 8):  # everything in one chunk; a frame per chunk
            for sel, labels, G in ((None, None, 1), (None, lab, 3), (np.array([4, 1, 2]), np.array([0, 0, 1]), 2)):
                exp = C.expected(x, first, last, sel, labels, G)
                what = (layout, first, last, cap, G)
                got = fa.common_mode_flac_device(*d, st.n, groups=labels, n_groups=G, first_sample=first, last_sample=last, streams=sel,
                                                 squares=False, is_int64=True, max_temp_bytes=cap)
                check(got, exp, what)
                check(ix.common_mode(groups=labels, n_groups=G, first_sample=first, last_sample=last, streams=sel, max_temp_bytes=cap), exp, what)
    ix.close()
    # through the array: a sum that wraps is numpy's wrapped sum
    big = np.array([[2**62 + 5, -7, 1], [2**62 + 9, 2**40, -(2**62)], [2**62, 3, -(2**62) - 1]], dtype=np.int64)
    s = fa.FlacArray.from_array(big, level=5).common_mode()
    assert s.sumsq_hi is None and s.sumsq is None and np.array_equal(s.sum[0], big.sum(axis=0, dtype=np.int64))
    assert int(s.sum[0, 0]) != sum(int(v) for v in big[:, 0])  # (it wrapped)
    with pytest.raises(ValueError):
        s.std()


# ---- float32 stores ---------------------------------------------------------------------------------------------------------

def test_float32_store_with_a_scalar_quantum(fa, torch):
    rng = np.random.default_rng(8)
    t = np.arange(700)
    common = np.sin(2 * np.pi * t / 200.0)
    x = (common[None, :] * rng.uniform(0.5, 2.0, (66, 1)) + rng.normal(0.0, 0.1, (66, 700)) + rng.uniform(-3, 3, (66, 1))).astype(np.float32)
    arr = fa.FlacArray.from_array(x, quanta=1e-4, level=5)
    comp, st, nb = (torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in (arr.compressed, arr.stream_starts, arr.stream_nbytes))
    ints = fa.decode_flac_device(comp, st, nb, 700).cpu().numpy()  # the quantised integers: a decode with no offsets
    lab = np.arange(66) % 3
    lab[lab == 1] = 2  # group 1 is empty
    s = arr.common_mode(groups=lab, first=5, last=650)
    exp = C.expected(ints, 5, 650, None, lab, 3)
    assert np.array_equal(s.count, exp[0])
    check((s.sum, s.sumsq_hi, s.sumsq_lo), exp, "f32 ints")
    off = np.asarray(arr.stream_offsets, np.float64).reshape(-1)
    gain = np.asarray(arr.stream_gains, np.float64).reshape(-1)
    assert np.all(gain == gain[0])
    import math

    mean, std = s.mean(), s.std()
    for g in (0, 2):
        c = int(exp[0][g])
        ref_mean = math.fsum(off[lab == g]) / c + np.array([int(v) / c for v in exp[1][g]]) / gain[0]
        assert np.array_equal(mean[g], ref_mean)
        var = np.array([(c * int(q) - int(v) ** 2) / (c * c) for q, v in zip(exp[2][g], exp[1][g])])
        assert np.array_equal(std[g], np.sqrt(var) / abs(gain[0]))
        # and the formula means what it says: the mean over the streams of offset + x / gain, in float64
        model = off[lab == g, None] + ints[lab == g, 5:650].astype(np.float64) / gain[0]
        assert np.all(np.abs(mean[g] - model.mean(axis=0)) <= 1e-12 * np.abs(model).max())
    assert np.all(np.isnan(mean[1])) and np.all(np.isnan(std[1]))
    assert s.gain[0] == gain[0] and np.isnan(s.gain[1])
    # quantised=True: the integer fields, mean in integer units
    q = arr.common_mode(groups=lab, first=5, last=650, quantised=True)
    assert q.gain is None and q.offsets_mean is None and np.array_equal(q.sum, s.sum)
    assert np.array_equal(q.mean()[0], np.array([int(v) / int(exp[0][0]) for v in exp[1][0]]))


def test_float32_store_with_mixed_gains(fa, torch):
    rng = np.random.default_rng(9)
    x = (rng.normal(0.0, 1.0, (6, 500)) * (10.0 ** np.arange(6))[:, None]).astype(np.float32)
    arr = fa.FlacArray.from_array(x, precision=3, level=5)
    gains = np.asarray(arr.stream_gains).reshape(-1)
    assert np.unique(gains).size > 1
    with pytest.raises(ValueError) as e:
        arr.common_mode()
    assert "quanta=" in str(e.value) and "quantised=True" in str(e.value)
    comp, st, nb = (torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in (arr.compressed, arr.stream_starts, arr.stream_nbytes))
    ints = fa.decode_flac_device(comp, st, nb, 500).cpu().numpy()
    s = arr.common_mode(quantised=True)
    check((s.sum, s.sumsq_hi, s.sumsq_lo), C.expected(ints, 0, 500, None, None, 1), "precision=, quantised")
    assert s.gain is None
    # one stream per group shares its gain with itself
    s = arr.common_mode(groups=np.arange(6))
    assert np.array_equal(s.gain, gains.astype(np.float64)) and np.array_equal(s.sum, ints.astype(np.int64))


# ---- dirty scratch ----------------------------------------------------------------------------------------------------------

def test_dirty_scratch_and_a_larger_call_before(fa, torch):
    from flacarray_amd import _lib

    L = _lib.lib()
    st = C.store_a()
    d = up(torch, st.layouts["libflac"])
    _, sel, lab, G = next(g for g in C.groupings() if g[0] == "six")
    call = lambda: tuple(t.cpu().numpy() for t in fa.common_mode_flac_device(*d, st.n, groups=lab, n_groups=G, streams=sel, first_sample=1, last_sample=st.n - 1))  # noqa: E731
    clean = call()
    check(clean, want("A", 1, st.n - 1, "six"), "clean")
    torch.cuda.synchronize()
    assert L.fa_debug_scratch_fill(0xA5) == 0
    dirty = call()
    for a, b in zip(clean, dirty):
        assert np.array_equal(a, b)
    # a larger reduce call on another store leaves its task table and frame table in the slots this call uses
    other = C.store_b()
    fa.reduce_flac_device(*up(torch, other.layouts["libflac"]), other.n, width=7, streams=np.arange(130, -1, -1))
    after = call()
    for a, b in zip(clean, after):
        assert np.array_equal(a, b)


# ---- errors -----------------------------------------------------------------------------------------------------------------

def test_damaged_frame_fails_under_verify_with_the_plain_decodes_error(fa, torch):
    st = C.store_a()
    blob, starts, nbytes = (np.array(a, copy=True) for a in st.layouts["own"])
    end = int(starts[40] + nbytes[40])
    blob[end - 1] ^= 0x01  # the low byte of the last frame's CRC-16 of stream 40: the samples still decode
    d = up(torch, (blob, starts, nbytes))
    with pytest.raises(RuntimeError) as plain:
        fa.decode_flac_device(*d, st.n, verify=True)
    with pytest.raises(RuntimeError) as e:
        fa.common_mode_flac_device(*d, st.n, verify=True)
    assert str(e.value) == str(plain.value)
    ix = fa.DeviceDecodeIndex(*d, st.n)
    with pytest.raises(RuntimeError) as e:
        ix.common_mode(verify=True)
    assert str(e.value) == str(plain.value)
    # without the check the sums are those of the samples (the frame's payload is intact), and a range that leaves the
    # damaged frame out passes the check
    check(ix.common_mode(verify=False), want("A", 0, st.n, "one"), "unverified")
    check(ix.common_mode(first_sample=1, last_sample=150, verify=True), C.expected(st.samples, 1, 150, None, None, 1), "frame left out")
    ix.close()


def test_refusals_leave_the_result_arrays_unwritten(fa, torch):
    from flacarray_amd import _lib
    from flacarray_amd.libflacarray import _dp, _stream_ptr, xsum_plan

    L = _lib.lib()
    st = C.store_a()
    comp, starts, nbytes = up(torch, st.layouts["libflac"])
    perm, rows, _ = xsum_plan(np.zeros(131, np.int64), 1)
    order, rows_d = torch.from_numpy(perm).cuda(), torch.from_numpy(rows).cuda()
    n = st.n
    sentinel = 0x5A5A5A5A5A5A5A5A
    outs = [torch.full((1, n), sentinel, dtype=torch.int64, device="cuda") for _ in range(3)]
    ix = fa.DeviceDecodeIndex(comp, starts, nbytes, n)

    def i32(first=0, last=n, n_sel=131, order_p=_dp(order), n_rows=3, rows_p=_dp(rows_d), G=1, sum_p=_dp(outs[0]), hi_p=_dp(outs[1]), lo_p=_dp(outs[2]),
            n_stream=131, size=n):
        return L.fa_xsum_i32_device(_dp(comp), comp.numel(), _dp(starts), _dp(nbytes), n_stream, size, first, last, n_sel, order_p, n_rows, rows_p, G,
                                    sum_p, hi_p, lo_p, _stream_ptr(), 0)

    def indexed(first=0, last=n, n_sel=131, n_rows=3, G=1, hi_p=_dp(outs[1]), lo_p=_dp(outs[2]), handle=ix._h):
        return L.fa_xsum_indexed(handle, first, last, n_sel, _dp(order), n_rows, _dp(rows_d), G, 0, _dp(outs[0]), hi_p, lo_p, _stream_ptr(), 0)

    refused = [
        i32(first=10, last=10), i32(first=11, last=10), i32(first=0, last=n + 1), i32(first=-1, last=5),
        i32(G=0), i32(n_sel=-1), i32(n_sel=132), i32(n_rows=0), i32(n_rows=132), i32(order_p=None), i32(rows_p=None),
        i32(hi_p=None), i32(lo_p=None), i32(n_stream=0), i32(size=0),
        indexed(first=10, last=10), indexed(G=0), indexed(hi_p=None), indexed(n_rows=0), indexed(handle=None),
        # one-channel store through the two-channel entry point: refused by the stream headers, after the zero fill --
        # not listed here; squares for a two-channel call cannot be expressed (the entry point has no such arguments)
    ]
    assert all(rc != 0 for rc in refused), refused
    torch.cuda.synchronize()
    for o in outs:
        assert bool((o == sentinel).all())
    # the accepted call fills all three
    assert i32() == 0
    check(tuple(outs), want("A", 0, n, "one"), "after the refusals")
    ix.close()
