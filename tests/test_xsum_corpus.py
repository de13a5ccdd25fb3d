"""The stores of tests/xsum_corpus.py have what they are for (CPU only): the cross-stream fold of K7X is tested on the GPU
against these stores, and a store that missed its precondition would test nothing."""
import numpy as np
import pytest

from tests import xsum_corpus as C
from tests.golden import flac_writer as W

BUCKETS = {"%d-%d" % b for b in W.ORDER_BUCKETS}


@pytest.mark.parametrize("mk", [C.store_a, C.store_b], ids=["A", "B"])
def test_writer_stores_mix_passes_and_wasted_bits_inside_one_plan_row(mk):
    st = mk()
    n_stream, n = st.samples.shape
    assert (n_stream, st.samples.dtype) == (131, np.int32)
    assert (n % st.block) % 32 != 0 and st.block >= 64  # the last frame ends in a partial tile; two tiles and more per full frame
    if mk is C.store_a:
        assert n % 2 == 1 and n % st.block < 32  # odd rows, a last frame shorter than a tile
    nf = -(-n // st.block)
    assert all(len(f) == nf for f in st.frames)
    lanes = range(64)  # plan row 0 of the one-group plan: streams 0..63
    # some frame index has all four LPC order buckets among the 64 lanes: the three history passes all find work there and
    # every pass finds rows that are not its own
    both = [f for f in range(nf) if {W.order_bucket(st.frames[s][f]["order"]) for s in lanes if st.frames[s][f]["kind"] == "lpc"} == BUCKETS]
    assert both, "no frame index with all four order buckets in plan row 0"
    # ... and a frame with wasted bits beside one without, in the same wave
    assert any({st.frames[s][f]["wasted"] for s in lanes} == {True, False} for f in both)
    # the short last frame too is decoded by more than one pass
    last = {st.frames[s][nf - 1]["order"] > 8 for s in lanes}
    assert last == {True, False}
    # the sum of a column leaves int32
    assert np.abs(st.samples.astype(np.int64).sum(axis=0)).max() > 2**31
    # the two layouts are the same frames behind different metadata
    for blob, starts, nbytes in st.layouts.values():
        assert starts.size == 131 and int(starts[-1] + nbytes[-1]) == blob.size


def test_store_b_reaches_orders_the_small_block_cannot():
    orders = [f["order"] for fr in C.store_b().frames for f in fr]
    assert max(orders) == 32


def test_store_c_squares_pass_two_to_the_64():
    x = C.samples_c()
    assert x.shape == (70, 4096 + 100) and x.dtype == np.int32
    q = x.astype(np.int64) * x.astype(np.int64)
    hi = (q.astype(np.uint64) >> np.uint64(32)).sum(axis=0)  # (70 terms below 2^30 each)
    assert hi.max() > 2**32
    assert np.abs(x.astype(np.int64).sum(axis=0)).max() > 2**31


def test_store_d_is_two_channel():
    st = C.store_d()
    assert st.samples.shape == (5, 3 * 64 + 21) and st.samples.dtype == np.int64 and st.channels == 2
    assert np.abs(st.samples).max() > 2**32


def test_groupings_cover_the_six_sizes_and_name_no_stream_twice():
    seen = set()
    for name, sel, lab, G in C.groupings():
        idx = np.arange(131) if sel is None else sel
        assert np.unique(idx).size == idx.size and idx.min() >= 0 and idx.max() < 131, name
        if lab is not None:
            assert lab.size == idx.size and lab.min() >= 0 and lab.max() < G
            seen |= set(np.bincount(lab, minlength=G).tolist())
            assert np.any(np.diff(lab) < 0), name  # interleaved, not sorted
    assert set(C.SIX_SIZES) <= seen
    odd = C.groupings()[-1][1]
    assert odd.size % 2 == 1 and np.all(np.diff(odd) < 0)


def test_ranges_are_what_they_are_named():
    for st in (C.store_a(), C.store_b()):
        whole, inner, in_tile, cross, empty = C.ranges(st.n, st.block)
        assert whole == (0, st.n) and inner == (1, st.n - 1) and empty[0] == empty[1]
        assert in_tile[0] // 32 == (in_tile[1] - 1) // 32 and in_tile[0] // st.block == (in_tile[1] - 1) // st.block
        assert (cross[0] % st.block) >= 32 and cross[1] > (st.n // st.block) * st.block and cross[1] < st.n
