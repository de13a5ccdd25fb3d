"""Preconditions of the damage-map tests, on the CPU: the stores of tests/scrub_model.py are intact by its rule, every
damage site flips exactly the bits it claims, and the host helpers (flacarray_amd.scrub.damaged_ranges, the salvage model)
agree with naive loops.  tests/test_gpu_scrub.py compares the GPU with the same model."""
import numpy as np
import pytest

from tests import scrub_model as M
from tests import verify_corpus as V
from tests.golden import pyflac

from flacarray_amd import scrub as S

OK, U, H, C16 = M.OK, M.UNLOCATED, M.HEADER, M.CRC16


def test_constants_are_the_library_s():
    assert (S.FRAME_OK, S.FRAME_UNLOCATED, S.FRAME_HEADER, S.FRAME_CRC16) == (OK, U, H, C16) == (0, 1, 2, 4)


@pytest.mark.parametrize("name", M.STORES)
def test_intact_stores_are_all_zero(name):
    st = M.build_store(name)
    assert len(st.frames) == 3 and all(len(row) == 3 for row in st.frames) and st.n % st.block == 7
    assert int(st.starts[-1] + st.nbytes[-1]) == st.blob.size  # the last stream ends with the blob
    status = M.frame_status(st.blob, st.starts, st.nbytes, st.n, st.channels, st.block)
    assert status.shape == (3, 3) and not status.any()
    # wrong geometry: nothing is located
    assert (M.frame_status(st.blob, st.starts, st.nbytes, st.n, 3 - st.channels, st.block) == U).all()
    assert (M.frame_status(st.blob, st.starts, st.nbytes, st.n, st.channels, st.block + 1) == U).all()
    assert S.store_block_size(st.blob, st.starts, st.nbytes) == st.block


def test_some_frame_begins_at_an_odd_address():
    for name in M.STORES:
        assert any(fr.start % 2 for row in M.build_store(name).frames for fr in row), name


def test_the_model_decodes_what_it_calls_intact():
    """The hand-assembled store through the pure-Python decoder: the frames the rule accepts are the stream's frames."""
    st = M.build_store("foreign64")
    for s in range(3):
        seg = bytes(st.blob[st.starts[s] : st.starts[s] + st.nbytes[s]])
        assert np.array_equal(np.array(pyflac.decode_stream(seg)[0], dtype=np.int64).astype(np.int32).reshape(-1), st.data[s])


def _only(status, s, f, value):
    want = np.zeros_like(status)
    want[s, f] = value
    return np.array_equal(status, want)


@pytest.mark.parametrize("name", M.STORES)
def test_sites_flip_the_bits_they_claim(name):
    st = M.build_store(name)
    seen = set()
    for case in M.cases(name):
        status = M.expected(st, case)
        kind, where = case.name.split(" @ ")
        seen.add(kind)
        s = int(where.split()[0][1:])
        f = int(where.split()[1][1:]) if " " in where else None
        if kind == "footer":
            assert _only(status, s, f, C16), case.name
        elif kind in ("payload", "residual"):
            assert _only(status, s, f, C16), case.name
        elif kind in ("sync", "crc8"):
            assert _only(status, s, f, H | C16), case.name
        elif kind == "number":
            assert _only(status, s, f, H | C16), case.name
        elif kind == "number, CRC-16 restamped":
            assert _only(status, s, f, H), case.name
        elif kind in ("seek sample number", "seek offset beyond"):
            want = np.zeros_like(status)
            want[s, max(f - 1, 0) : f + 1] = U  # a bad point k: frames k - 1 and k
            assert np.array_equal(status, want), case.name
        elif kind == "seek offset inside":
            # frame f begins 4 bytes off: it and the frame in front of it are located, and both are wrong
            want = np.zeros_like(status)
            want[s, f] = H | C16
            if f > 0:
                want[s, f - 1] = C16
            assert np.array_equal(status, want), case.name
        elif kind in ("STREAMINFO block size", "fLaC marker", "STREAMINFO channels", "negative start", "nbytes past the blob"):
            want = np.zeros_like(status)
            want[s] = U
            assert np.array_equal(status, want), case.name
        elif kind == "half nbytes":
            assert not status[np.arange(3) != s].any() and status[s].any() and (status[s, -1] != 0), case.name
        elif kind == "zeros across f0 / f1":
            want = np.zeros_like(status)
            want[s, 0], want[s, 1] = C16, H | C16
            assert np.array_equal(status, want), case.name
        else:
            raise AssertionError("unclassified site " + case.name)
    assert {"footer", "sync", "number", "number, CRC-16 restamped", "crc8", "seek sample number", "seek offset inside", "seek offset beyond",
            "STREAMINFO block size", "fLaC marker", "STREAMINFO channels", "negative start", "nbytes past the blob", "half nbytes",
            "zeros across f0 / f1"} <= seen
    assert ("payload" in seen) if name != "lpc4096" else ("residual" in seen)


def test_length_corpus_reaches_every_edge():
    stores = M.length_stores()
    lengths = sorted({fr[-1].nbytes - 2 for st in stores for fr in st.frames})
    for a, b in V.EDGE_GROUPS:
        assert set(range(a, b + 1)) <= set(lengths)
    assert set(range(V.smallest_L(), V.SMALL_TOP + 1)) <= set(lengths)
    some = [st for st in stores if st.block in (64, 509, 511)][:3] + [stores[0], stores[-1]]
    for st in some:
        status = M.frame_status(st.blob, st.starts, st.nbytes, st.n, 1, st.block)
        assert not status.any()
        for label, blob in M.length_cases(st):
            got = M.frame_status(blob, st.starts, st.nbytes, st.n, 1, st.block)
            want = np.zeros_like(got)
            want[:, -1] = (H | C16) if label == "first" else C16
            assert np.array_equal(got, want), (st.name, label)


def test_damaged_ranges_agrees_with_a_naive_loop():
    rng = np.random.default_rng(5)
    for nf, block, n in ((1, 64, 64), (1, 64, 7), (3, 1152, 2 * 1152 + 7), (9, 16, 9 * 16), (17, 5, 17 * 5 - 4)):
        for _ in range(20):
            status = rng.choice(np.array([0, 0, 0, 1, 2, 4, 6], dtype=np.uint8), size=(2, 3, nf))
            got = S.damaged_ranges(status, block, n)
            assert got.dtype == np.int64 and got.shape[1] == 3
            assert np.array_equal(got, M.naive_ranges(status, block, n))
    assert S.damaged_ranges(np.zeros((4, 3), np.uint8), 10, 25).shape == (0, 3)
    assert np.array_equal(S.damaged_ranges(np.ones((2, 3), np.uint8), 10, 25), [[0, 0, 25], [1, 0, 25]])
    with pytest.raises(ValueError):
        S.damaged_ranges(np.zeros((4, 3), np.uint8), 10, 45)


def test_common_block_size():
    h = np.zeros((5, 12), np.uint8)
    h[:, 9] = h[:, 11] = (64, 64, 32, 32, 16)
    assert S.common_block_size(h) == 32  # a tie: the smaller one
    h[4, 9] = h[4, 11] = 64
    assert S.common_block_size(h) == 64
    h[:, 9] = 1
    assert S.common_block_size(h) is None  # min != max everywhere
    assert S.common_block_size(np.zeros((0, 12), np.uint8)) is None


def test_salvage_model():
    data = np.arange(3 * 25, dtype=np.int32).reshape(3, 25)
    status = np.zeros((3, 3), np.uint8)
    status[1, 1], status[2, 2] = 4, 1
    full = M.salvage_model(data, status, 0, 25, -7, 10)
    want = data.copy()
    want[1, 10:20] = -7
    want[2, 20:25] = -7
    assert np.array_equal(full, want)
    assert np.array_equal(M.salvage_model(data, status, 8, 22, -7, 10), want[:, 8:22])
    assert np.array_equal(M.salvage_model(data, status, 0, 10, -7, 10), data[:, :10])
    f = M.salvage_model(data.astype(np.float32), status, 0, 25, np.nan, 10)
    assert np.isnan(f[1, 10:20]).all() and np.isnan(f[2, 20:]).all() and np.isnan(f).sum() == 15
