"""The stores and templates of tests/dot_corpus.py have what they are for (CPU only): the dot sink of K7 is tested on the
GPU against them, and a store or a template set that missed its precondition would test nothing."""
import numpy as np
import pytest

from tests import dot_corpus as C
from tests.golden import flac_writer as W


@pytest.mark.parametrize("mk", [C.store_a, C.store_b], ids=["A", "B"])
def test_writer_stores_mix_passes_and_wasted_bits_inside_one_wave(mk):
    st = mk()
    n_stream, n = st.samples.shape
    assert (n_stream, st.samples.dtype) == (131, np.int32)
    nf = -(-n // st.block)
    assert n % st.block != 0 and all(len(f) == nf for f in st.frames)  # a short last frame
    lanes = range(64)  # plan row 0 of the trivial plan: streams 0..63, one frame index per wave
    passes = lambda f: {0 if st.frames[s][f]["order"] <= 8 else 1 if st.frames[s][f]["order"] <= 16 else 2 for s in lanes}  # noqa: E731
    mixed = [f for f in range(nf) if passes(f) == {0, 1, 2}]
    assert mixed, "no frame index whose 64 frames need all three history passes"
    assert any({st.frames[s][f]["wasted"] for s in lanes} == {True, False} for f in mixed)
    # warm-up samples exist to be dropped: predictive frames of an order above the range's frame offset of 5
    first = C.ranges(n, st.block)[4][0]
    assert first % st.block == 5 and any(st.frames[s][first // st.block]["order"] > 5 for s in lanes)
    assert {W.order_bucket(f["order"]) for fr in st.frames for f in fr if f["kind"] == "lpc"} == {"%d-%d" % b for b in W.ORDER_BUCKETS}


def test_ranges_are_what_they_are_named():
    for st in (C.store_a(), C.store_b()):
        n, b = st.n, st.block
        whole, tail, head, in_frame, warm, across = C.ranges(n, b)
        assert whole == (0, n) and tail == (1, n) and head == (0, n - 1)
        assert in_frame[0] // b == (in_frame[1] - 1) // b
        assert warm[0] // b == (warm[1] - 1) // b and 0 < warm[0] % b < 8
        assert across[0] // b + 1 == (across[1] - 1) // b and across[0] % 32 and across[1] % 32
        assert all(0 <= f < l <= n for f, l in C.ranges(n, b))


def test_extremes_store_samples():
    x = C.samples_extremes()
    assert x.dtype == np.int32 and x.shape == (6, C.EXT_BLOCK + 50)
    b = C.EXT_BLOCK
    assert [int(v) for v in x[0, [0, b - 1, b]]] == [C.INT32_MIN, C.INT32_MAX, C.INT32_MIN]
    assert [int(v) for v in x[1, [0, b - 1, b]]] == [C.INT32_MAX, C.INT32_MIN, C.INT32_MAX]


def test_template_sets_hold_every_value_class():
    assert C.KS == (1, 3, 8, 9, 17)
    for K in C.KS:
        T = C.templates(K, 213)
        assert T.shape == (K, 213) and T.dtype == np.int64 and T.min() == C.INT32_MIN and T.max() == C.INT32_MAX
        for v in (0, 1, -1):
            assert np.any(T == v)
        assert np.any((np.abs(T) > 1) & (T != C.INT32_MIN) & (T != C.INT32_MAX))  # noise
    W_ = C.wide_templates(213)
    for v in (C.INT64_MIN, C.INT64_MAX, 2**31, -(2**31) - 1):
        assert np.any(W_ == v)
    assert not np.any(W_[4])
    c = C.constant_templates(9)
    assert np.all(c[0] == C.INT32_MIN) and np.all(c[1] == C.INT32_MAX)


def test_oracle_is_python_integers():
    x = np.array([[C.INT32_MIN, C.INT32_MAX, 5], [1, 2, 3]], dtype=np.int32)
    T = np.array([[C.INT64_MIN, C.INT64_MAX, 1]], dtype=np.int64)
    got = C.oracle(x, T, 0, 3)
    assert got.dtype == object and got.shape == (2, 1)
    assert got[0, 0] == C.INT32_MIN * C.INT64_MIN + C.INT32_MAX * C.INT64_MAX + 5 and isinstance(got[0, 0], int)
    assert C.oracle(x, T[:, 1:], 1, 3, streams=[1])[0, 0] == 2 * C.INT64_MAX + 3
    sub = C.subset()
    assert sub.size == 67 and np.unique(sub).size == 67 and np.any(np.diff(sub) < 0)
