"""CPU tests of the window model (tests/window_model.py) against the oracle's one-shot encode of the slice, of the corpus
the GPU test shares with it (the corpus must reach the hard cases on its own), of the number-field arithmetic at the UTF-8
thresholds, and of the host-side argument checks of FlacArray.window / trim (they raise before any device call)."""
import numpy as np
import pytest

import flacarray_amd as fa
from flacarray_amd import _lib
from flacarray_amd.libflacarray import _window_args
from tests import append_model as A
from tests import window_model as W
from tests.conftest import sinusoid_noise_i32, strip_seektable


def _encode(oracle, x, level):
    return (oracle.encode_i64 if x.dtype == np.int64 else oracle.encode_i32)(x, level)


def _model_equals_oracle(oracle, x, store, level, first, last, idx, stats, failures):
    B = W.block_size(level)
    rows = slice(None) if idx is None else np.asarray(idx)
    tr = W.tail_range(x.shape[1], B, first, last)
    tail = None if tr is None else _encode(oracle, x[rows, tr[0] : tr[1]], level)
    got = W.window(store, first, last, idx, tail, stats)
    want = _encode(oracle, x[rows, first:last], level)
    if not all(np.array_equal(g, w) for g, w in zip(got, want)):
        failures.append((first, last, idx))


_CORPUS = {}


def _corpus(oracle):
    """The model run over the whole corpus, once: {"stats": ..., (level, wide) or "number": windows that differ}."""
    if _CORPUS:
        return _CORPUS
    stats = W.new_stats()
    for level in (1, 5):
        B = W.block_size(level)
        for wide in (False, True):
            bad = []
            x = W.edge_rows(level, wide)
            store = _encode(oracle, x, level)
            for first, last in W.edge_windows(level):
                _model_equals_oracle(oracle, x, store, level, first, last, None, stats, bad)
            for idx in W.STREAM_PICKS:  # a subset, a permutation, the reversed order
                _model_equals_oracle(oracle, x, store, level, B, 3 * B + 5, idx, stats, bad)
                _model_equals_oracle(oracle, x, store, level, 0, x.shape[1], idx, stats, bad)
            _CORPUS[(level, wide)] = bad
    # the windows that run to the end of the stream are checked for the late frames only: the model's byte-wise CRCs
    # over megabytes belong to no CPU suite
    bad = []
    x = W.number_rows()
    store = oracle.encode_i32(x, W.NUMBER_LEVEL)
    for f0 in W.NUMBER_F0:
        to_end, mid = W.number_windows(f0)
        _model_equals_oracle(oracle, x, store, W.NUMBER_LEVEL, *mid, None, stats, bad)
        if f0 >= 1922:
            _model_equals_oracle(oracle, x, store, W.NUMBER_LEVEL, *to_end, None, stats, bad)
    _CORPUS["number"] = bad
    _CORPUS["stats"] = stats
    return _CORPUS


@pytest.mark.parametrize("wide", [False, True], ids=["int32", "int64"])
@pytest.mark.parametrize("level", [1, 5])
def test_model_edges_equal_one_shot_encode(oracle, level, wide):
    assert _corpus(oracle)[(level, wide)] == []


def test_model_number_field(oracle):
    """Frame numbers whose UTF-8 field loses 0, 1 and 2 bytes (level 1, 2050 frames)."""
    assert _corpus(oracle)["number"] == []


def test_corpus_reaches_the_hard_cases(oracle):
    """What the GPU test relies on: over the corpus the payload copies take every source / destination misalignment,
    some payload is shorter than one 16-byte chunk, some frame is VERBATIM, and headers shrink by 0, 1 and 2 bytes."""
    st = _corpus(oracle)["stats"]
    assert st["align"] == set(range(16)), sorted(st["align"])
    assert st["min_payload"] < 16
    assert st["verbatim"] >= 1
    assert {0, 1, 2} <= st["shrink"], st["shrink"]


def test_model_recomputes_the_crcs_the_identity_gives():
    """renumber_whole (CRCs over the whole frame) against append_model.renumber_frame (the linear identity) on one frame."""
    rng = np.random.default_rng(3)
    for number_old, number_new in ((2048, 0), (129, 1), (5, 5), (70000, 127)):
        payload = rng.integers(0, 256, int(rng.integers(1, 300)), dtype=np.uint8).tobytes()
        head = bytes([0xFF, 0xF8, 0xC9, 0x0E]) + A.utf8_number(number_old)
        head += bytes([A.crc8(head)])
        c = W.crc16(head + payload)
        fr = head + payload + bytes([c >> 8, c & 0xFF])
        assert W.crc16(fr[:-2]) == A.crc16(fr[:-2])
        assert W.renumber_whole(fr, number_new)[0] == A.renumber_frame(fr, number_new)


def test_growth_arithmetic_at_the_utf8_thresholds():
    """append_growth(f0, k) = the header bytes frames [f0, f0 + k) lose when renumbered to [0, k), at 127/128, 2047/2048,
    65535/65536 and 2^21 (host only: no store has that many frames in a test)."""
    S = A.utf8_len_sum
    growth = lambda f0, k: S(f0 + k) - S(f0) - S(k)  # noqa: E731
    for t in (128, 2048, 65536, 1 << 21):
        for f0 in (t - 1, t, t + 1):
            for k in (0, 1, 2, 127, 128, 129, 300):
                assert growth(f0, k) == sum(A.utf8_len(f0 + i) - A.utf8_len(i) for i in range(k)), (f0, k)
        assert A.utf8_len(t - 1) + 1 == A.utf8_len(t)
    assert growth(0, 12345) == 0


# ---- host-side argument checks: none of these reaches the device ----
def _host_array(oracle, x, level=5):
    blob, st, nb = oracle.encode_i32(x, level)
    shape = x.shape if x.shape[0] > 1 else (x.shape[1],)
    return fa.FlacArray._assemble(shape, None, np.int32, blob, st.reshape(x.shape[:-1]), nb.reshape(x.shape[:-1]), None, None)


@pytest.mark.parametrize("call", ["window", "trim"])
def test_window_rejects_bad_ranges_and_levels(oracle, call):
    arr = _host_array(oracle, sinusoid_noise_i32(3, 5000))
    blob = arr.compressed.copy()
    fn = getattr(arr, call)
    for first, last in ((-1, 10), (0, 5001), (10, 10), (11, 10), (5000, None)):
        with pytest.raises(ValueError, match="range"):
            fn(first, last)
    with pytest.raises(ValueError, match="levels"):
        fn(0, 10, level=9)
    with pytest.raises(ValueError, match="block size"):
        fn(0, 10, level=1)
    assert np.array_equal(arr.compressed, blob) and arr.shape == (3, 5000)


def test_window_rejects_bad_stream_indices(oracle):
    arr = _host_array(oracle, sinusoid_noise_i32(3, 5000))
    with pytest.raises(ValueError, match="twice"):
        arr.window(0, 10, streams=[1, 1])
    with pytest.raises(ValueError, match="outside"):
        arr.window(0, 10, streams=[3])
    with pytest.raises(ValueError, match="outside"):
        arr.window(0, 10, streams=[-1])


def test_window_of_no_streams_is_an_empty_store(oracle):
    arr = _host_array(oracle, sinusoid_noise_i32(3, 5000))
    out = arr.window(100, 300, streams=np.zeros(0, dtype=np.int64))
    assert out.shape == (0, 200) and out.compressed.size == 0 and out.stream_starts.shape == (0,) and out.stream_nbytes.shape == (0,)


@pytest.mark.parametrize("call", ["window", "trim"])
def test_window_rejects_streams_without_seektable(oracle, call):
    x = sinusoid_noise_i32(2, 5000)
    blob, st, nb = strip_seektable(*oracle.encode_i32(x, 5))
    arr = fa.FlacArray._assemble(x.shape, None, np.int32, blob, st, nb, None, None)
    with pytest.raises(ValueError, match=r"reindex\(\)"):
        getattr(arr, call)(0, 4096)
    assert np.array_equal(arr.compressed, blob)


@pytest.mark.parametrize("call", ["window", "trim"])
def test_window_rejects_distributed_store(oracle, call):
    x = sinusoid_noise_i32(2, 5000)
    blob, st, nb = oracle.encode_i32(x, 5)
    arr = fa.FlacArray._assemble(x.shape, (4, 5000), np.int32, blob, st, nb, None, None)
    with pytest.raises(NotImplementedError):
        getattr(arr, call)(0, 4096)


def test_window_args_defaults():
    assert _window_args(3, 5000, 0, None, None, 5) == (0, 5000, 4096, None)
    assert _window_args(3, 5000, 1152, 1153, None, 2)[:3] == (1152, 1153, 1152)


def test_window_entry_points_are_exported():
    assert "window_flac_device" in fa.__all__ and callable(fa.window_flac_device)
    assert callable(fa.FlacArray.window) and callable(fa.FlacArray.trim)
    assert {"fa_window_workspace_bytes", "fa_window_capacity_bytes", "fa_window_device"} <= set(_lib.SYMBOLS)
    L = _lib.lib()
    # pure arithmetic, no device: an unaligned first and an empty window are refused, a tail needs an encode's workspace
    assert L.fa_window_workspace_bytes(4, 5 * 4096 + 7, 4, 1, 4096, 1, 5) == -1
    assert L.fa_window_workspace_bytes(4, 5 * 4096 + 7, 4, 4096, 4096, 1, 5) == -1
    assert 0 < L.fa_window_workspace_bytes(4, 5 * 4096 + 7, 4, 4096, 8192, 1, 5) < L.fa_window_workspace_bytes(4, 5 * 4096 + 7, 4, 4096, 8193, 1, 5)
    assert L.fa_window_capacity_bytes(1000, 4, 5 * 4096 + 7, 2, 4096, 8192, 1, 5) == 1000 + 6 * 2 + 64
    assert L.fa_window_capacity_bytes(1000, 4, 5 * 4096 + 7, 2, 4096, 8193, 2, 5) > 1000 + 2 * 2 * 16640
