"""CPU tests of the join model (tests/join_model.py) against the oracle's one-shot encode of the whole array, of the
corpus the GPU test shares with it (the corpus must reach the hard cases on its own), of the closed forms the kernel
places frames by at the UTF-8 thresholds, and of the host-side argument checks of FlacArray.concatenate / extend and
_join_args (they raise before any device call)."""
import numpy as np
import pytest

import flacarray_amd as fa
from flacarray_amd import _lib
from flacarray_amd.libflacarray import _join_args
from tests import append_model as A
from tests import join_model as J
from tests import window_model as W
from tests.conftest import sinusoid_noise_f32, sinusoid_noise_i32, strip_seektable


def _encode(oracle, x, level):
    return (oracle.encode_i64 if x.dtype == np.int64 else oracle.encode_i32)(x, level)


def _model_equals_oracle(oracle, x, level, cuts, stats, failures):
    got = J.join([_encode(oracle, p, level) for p in J.pieces(x, cuts)], stats)
    want = _encode(oracle, x, level)
    if not all(np.array_equal(g, w) for g, w in zip(got, want)):
        failures.append(cuts)


_CORPUS = {}


def _corpus(oracle):
    """The model run over the whole corpus, once: {"stats": ..., (level, wide) or "number": cuts that differ}."""
    if _CORPUS:
        return _CORPUS
    stats = J.new_stats()
    for level in J.LEVELS:
        for wide in (False, True):
            bad = []
            x = W.edge_rows(level, wide)
            for cuts in J.aligned_cuts(level):
                _model_equals_oracle(oracle, x, level, cuts, stats, bad)
            _CORPUS[(level, wide)] = bad
    # only small or late parts: the model's byte-wise CRCs over megabytes belong to no CPU suite.  A cut at a late frame
    # is joined up to the end; a cut at an early one with the next two frames and a bit; the three-part cut (a middle
    # part of 1795 frames) on the constant row, whose frames are 13 and 14 bytes.
    bad = []
    x = W.number_rows()
    B = J.NUMBER_B
    for cuts in J.NUMBER_CUTS:
        if len(cuts) == 1:
            end = x.shape[1] if cuts[0] >= 1922 * B else cuts[0] + 2 * B + 77
            _model_equals_oracle(oracle, x[:, :end], W.NUMBER_LEVEL, cuts, stats, bad)
        else:
            _model_equals_oracle(oracle, x[:1], W.NUMBER_LEVEL, cuts, stats, bad)
    _CORPUS["number"] = bad
    _CORPUS["stats"] = stats
    return _CORPUS


@pytest.mark.parametrize("wide", [False, True], ids=["int32", "int64"])
@pytest.mark.parametrize("level", J.LEVELS)
def test_model_edges_equal_one_shot_encode(oracle, level, wide):
    assert _corpus(oracle)[(level, wide)] == []


def test_model_number_field(oracle):
    """Parts that land on bases on both sides of 128 and 2048, and parts whose own frames cross a threshold while raised."""
    assert _corpus(oracle)["number"] == []


def test_corpus_reaches_the_hard_cases(oracle):
    """What the GPU test relies on: over the corpus the payload copies take every source / destination misalignment,
    some payload is shorter than one 16-byte chunk, some frame is VERBATIM, and headers grow by 0, 1 and 2 bytes."""
    st = _corpus(oracle)["stats"]
    assert st["align"] == set(range(16)), sorted(st["align"])
    assert st["min_payload"] < 16
    assert st["verbatim"] >= 1
    assert {0, 1, 2} <= st["grow"], st["grow"]


def test_single_part_is_returned_as_it_is(oracle):
    x = W.edge_rows(5)
    store = oracle.encode_i32(x, 5)
    assert all(np.array_equal(g, w) for g, w in zip(J.join([store]), store))
    with pytest.raises(ValueError, match="frame boundary"):
        J.join([oracle.encode_i32(p, 5) for p in J.pieces(x, (5,))])


def test_closed_forms_agree_with_the_running_offsets(oracle):
    """The kernel places frame k of part p at D_p(s) + off_p(s, k) + append_growth(base_p, k) with D_p(s) = sum_{q < p}
    (body_q(s) + growth_q); the model adds frame lengths up.  Compared where the number field changes its length."""
    S = A.utf8_len_sum
    growth = lambda base, k: S(base + k) - S(base) - S(k)  # noqa: E731
    x = W.number_rows()[:1]
    B = J.NUMBER_B
    for cuts in ((127 * B, 1922 * B), (128 * B,), (2047 * B,), (2048 * B, 2049 * B)):
        parts = [oracle.encode_i32(p, W.NUMBER_LEVEL)[0].tobytes() for p in J.pieces(x, cuts)]
        running = []
        new = J.join_stream(parts, offsets=running)
        parsed = [A.parse_stream(p) for p in parts]
        base, D, want = 0, 0, []
        for p, (old, (_, _, _, pts, hb)) in enumerate(zip(parts, parsed)):
            want += [(p, k, D + off + growth(base, k)) for k, (off, _) in enumerate(pts)]
            D += len(old) - hb + growth(base, len(pts))
            base += len(pts)
        assert running == want, cuts
        assert [o for o, _ in A.parse_stream(new)[3]] == [o for _, _, o in want]
        assert len(new) == 46 + 18 * base + D
    for t in (128, 2048, 65536, 1 << 21):
        for base in (t - 1, t, t + 1):
            for k in (0, 1, 127, 128, 129, 2047, 2048):
                assert growth(base, k) == sum(A.utf8_len(base + i) - A.utf8_len(i) for i in range(k)), (base, k)
    assert growth(0, 4321) == 0


# ---- host-side argument checks: none of these reaches the device ----
def _host_array(oracle, x, level=5, global_shape=None):
    blob, st, nb = oracle.encode_i32(x.reshape(-1, x.shape[-1]), level)
    return fa.FlacArray._assemble(x.shape, global_shape, np.int32, blob, st.reshape(x.shape[:-1]), nb.reshape(x.shape[:-1]), None, None)


def _float_array(x, gains):
    """A float32 store around any bytes: the checks that matter here read shapes, dtypes, offsets and gains only."""
    lead = x.shape[:-1]
    n = int(np.prod(lead))
    return fa.FlacArray._assemble(x.shape, None, np.float32, np.zeros(64 * n, np.uint8), (64 * np.arange(n)).reshape(lead),
                                  np.full(lead, 64, np.int64), np.zeros(lead, np.float32), np.asarray(gains, np.float32).reshape(lead))


@pytest.fixture(scope="module")
def two(oracle):
    x = sinusoid_noise_i32(3, 2 * 4096 + 9)
    return _host_array(oracle, x[:, :4096]), _host_array(oracle, x[:, 4096:])


def _both(a, b, **kw):
    """The refusal through concatenate and through extend."""
    yield lambda: fa.FlacArray.concatenate([a, b], **kw)
    yield lambda: a.extend(b, **kw)


def test_concatenate_rejects_an_empty_list_and_a_bad_axis(two):
    a, b = two
    with pytest.raises(ValueError, match="at least one"):
        fa.FlacArray.concatenate([])
    for axis in (2, -3, 0.0, None, True):  # (the arrays are 2-D: 1 is the sample axis, -2 the leading one)
        with pytest.raises(ValueError, match="axis"):
            fa.FlacArray.concatenate([a, b], axis=axis)
    with pytest.raises(ValueError, match="FlacArrays"):
        fa.FlacArray.concatenate([a, np.zeros((3, 5), np.int32)])


def test_concatenate_rejects_mismatched_parts(oracle, two):
    a, b = two
    before = a.compressed.copy()
    wide = fa.FlacArray._assemble((3, 4096), None, np.int64, a.compressed, a.stream_starts, a.stream_nbytes, None, None)
    for call in _both(a, wide):
        with pytest.raises(ValueError, match="dtype"):
            call()
    for other in (_host_array(oracle, sinusoid_noise_i32(2, 4096)), _host_array(oracle, sinusoid_noise_i32(1, 4096)[0]),
                  _host_array(oracle, sinusoid_noise_i32(3, 4096).reshape(3, 1, 4096))):
        for call in _both(a, other):
            with pytest.raises(ValueError, match="leading shape"):
                call()
    for call in _both(a, b, level=9):
        with pytest.raises(ValueError, match="levels"):
            call()
    for call in _both(a, b, level=1):  # (the stores were written with 4096-sample blocks)
        with pytest.raises(ValueError, match="block size"):
            call()
    low = _host_array(oracle, sinusoid_noise_i32(3, 1152), level=1)
    for call in _both(a, low):
        with pytest.raises(ValueError, match="block size"):
            call()
    assert np.array_equal(a.compressed, before) and a.shape == (3, 4096)


def test_concatenate_rejects_unequal_gains():
    x = sinusoid_noise_f32(2, 100)
    g = np.array([1e-3, 2e-3], np.float32)
    a, b = _float_array(x, g), _float_array(x, np.array([g[0], np.nextafter(g[1], np.float32(1))], np.float32))
    for call in _both(a, b):
        with pytest.raises(ValueError, match="quantised differently.*compress"):
            call()
    off = _float_array(x, g)
    off._st.offsets[1] = np.float32(-0.0)  # (equal as numbers, not bit for bit)
    with pytest.raises(ValueError, match="quantised differently"):
        fa.FlacArray.concatenate([a, off])


def test_concatenate_rejects_streams_without_seektable(oracle, two):
    a, _ = two
    x = sinusoid_noise_i32(3, 5000)
    blob, st, nb = strip_seektable(*oracle.encode_i32(x, 5))
    foreign = fa.FlacArray._assemble(x.shape, None, np.int32, blob, st, nb, None, None)
    for parts in ([a, foreign], [foreign, a], [foreign]):
        with pytest.raises(ValueError, match=r"reindex\(\)"):
            fa.FlacArray.concatenate(parts)
    with pytest.raises(ValueError, match=r"reindex\(\)"):
        foreign.extend(a)
    assert np.array_equal(foreign.compressed, blob)


def test_concatenate_rejects_distributed_parts(oracle, two):
    a, _ = two
    x = sinusoid_noise_i32(3, 4096)
    blob, st, nb = oracle.encode_i32(x, 5)
    dist = fa.FlacArray._assemble(x.shape, (6, 4096), np.int32, blob, st, nb, None, None)
    for axis in (-1, 0):
        for parts in ([a, dist], [dist, a]):
            with pytest.raises(NotImplementedError):
                fa.FlacArray.concatenate(parts, axis=axis)
    with pytest.raises(NotImplementedError):
        a.extend(dist)


def test_axis0_rejects_one_dimensional_and_mismatched_arrays(oracle, two):
    a, b = two
    one = _host_array(oracle, sinusoid_noise_i32(1, 4096)[0])
    with pytest.raises(ValueError, match="sample axis"):
        fa.FlacArray.concatenate([one, one], axis=0)
    with pytest.raises(ValueError, match="stream_size"):  # (b has 4105 samples)
        fa.FlacArray.concatenate([a, b], axis=0)
    cube = _host_array(oracle, sinusoid_noise_i32(6, 4096).reshape(3, 2, 4096))
    with pytest.raises(ValueError, match="stream_size"):
        fa.FlacArray.concatenate([a, cube], axis=0)
    wide = fa.FlacArray._assemble((3, 4096), None, np.int64, a.compressed, a.stream_starts, a.stream_nbytes, None, None)
    with pytest.raises(ValueError, match="dtype"):
        fa.FlacArray.concatenate([a, wide], axis=0)


def test_axis0_stacks_host_stores_without_a_device(oracle):
    """The host side of axis=0 is numpy alone: the stack of two stores is the store of the stacked arrays."""
    x = sinusoid_noise_i32(5, 5000).reshape(5, 1, 5000)
    got = fa.FlacArray.concatenate([_host_array(oracle, x[:2]), _host_array(oracle, x[2:])], axis=0)
    want = _host_array(oracle, x)
    assert got.shape == (5, 1, 5000) and got.stream_starts.shape == (5, 1)
    assert np.array_equal(got.compressed, want.compressed) and np.array_equal(got.stream_starts, want.stream_starts)
    assert np.array_equal(got.stream_nbytes, want.stream_nbytes) and got.stream_offsets is None


def test_join_args():
    assert _join_args([3], [5000], 5) == (4096, [5000], None)
    assert _join_args([3, 3, 3], [4096, 8192, 7], 5) == (4096, [4096, 8192, 7], None)
    assert _join_args([3, 3, 3], [1152, 1153, 1151], 2) == (1152, [1152, 1153, 1151], 1)
    assert _join_args([1, 1], [1, 4095], 8)[2] == 0
    assert _join_args([2, 2, 2, 2], [4096, 4096, 5, 4091], 3)[2] == 2  # (the running total is what counts)
    for n_streams, sizes, level, word in (([], [], 5, "at least one"), ([3, 3], [4096, 0], 5, "non-zero"), ([3, 3], [4096, -1], 5, "non-zero"),
                                          ([3, 4], [4096, 4096], 5, "number of streams"), ([3], [4096], 9, "levels"), ([3], [4096], -1, "levels"),
                                          ([1, 1], [1 << 35, 1 << 35], 5, "2\\^36")):
        with pytest.raises(ValueError, match=word):
            _join_args(n_streams, sizes, level)


def test_join_entry_points_are_exported():
    assert "join_flac_device" in fa.__all__ and callable(fa.join_flac_device)
    assert callable(fa.FlacArray.concatenate) and callable(fa.FlacArray.extend)
    assert {"fa_join_workspace_bytes", "fa_join_capacity_bytes", "fa_join_device"} <= set(_lib.SYMBOLS)
    import ctypes

    L = _lib.lib()
    arr = lambda *v: (ctypes.c_int64 * len(v))(*v)  # noqa: E731
    # pure arithmetic, no device: an unaligned part other than the last, an empty part and 2^36 samples are refused
    assert L.fa_join_workspace_bytes(2, 4, arr(4096, 7), 1, 5) > 0
    assert L.fa_join_workspace_bytes(2, 4, arr(7, 4096), 1, 5) == -1
    assert L.fa_join_workspace_bytes(2, 4, arr(4096, 0), 1, 5) == -1
    assert L.fa_join_workspace_bytes(2, 4, arr(1 << 35, 1 << 35), 1, 5) == -1
    assert L.fa_join_workspace_bytes(0, 4, arr(4096), 1, 5) == -1
    assert L.fa_join_workspace_bytes(2, 4, arr(1152, 7), 1, 5) == -1 and L.fa_join_workspace_bytes(2, 4, arr(1152, 7), 1, 2) > 0
    # the capacity: the parts' bytes plus, per stream, 46 bytes and the growth of the number fields
    assert L.fa_join_capacity_bytes(2, arr(1000, 500), 4, arr(4096, 7), 1, 5) == 1500 + 4 * 46
    growth = 4 + 1  # frames 0 .. 4 of part 1 become 127 .. 131: four of them gain a byte; frame 0 of part 2 becomes 132
    assert L.fa_join_capacity_bytes(3, arr(1000, 500, 10), 4, arr(127 * 1152, 5 * 1152, 3), 1, 1) == 1510 + 4 * (46 + growth)
    assert L.fa_join_capacity_bytes(2, arr(1000, -1), 4, arr(4096, 7), 1, 5) == -1
