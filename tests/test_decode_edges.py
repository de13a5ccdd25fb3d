"""Preconditions of tests/test_gpu_decode_footprint.py, checked without a GPU: the stores decode to the arrays they come
with and never to the sentinel, the window and slice lists of tests/decode_edges.py reach every residue of (output
address, first, count), every window shape and both kinds of row in one wave, and the checker sees a single element
written in front of a slice, behind it, or left out."""
import itertools

import numpy as np
import pytest

from tests import compare_corpus as C
from tests import decode_edges as E


@pytest.fixture(scope="module")
def stores(oracle):
    return {name: E.build_store(name, oracle) for name in E.STORES}


def _lists(st):
    w = E.width_of(st.channels)
    return w, E.windows(st.n, st.block, w), E.slice_batches(st.n, st.block, w)


def test_stores_decode_to_their_arrays(oracle, stores):
    assert set(E.FLOAT_STORES) <= set(stores)
    for name, st in stores.items():
        assert st.data.shape == (E.ROWS, st.n) and st.starts.shape == st.nbytes.shape == (E.ROWS,), name
        assert E.ROWS >= 64 and st.block % E.TILE == 0 and st.n > 2 * st.block, name
        got = (oracle.decode_i32 if st.channels == 1 else oracle.decode_i64)(st.blob, st.starts, st.nbytes, st.n)
        assert got.dtype == st.data.dtype and np.array_equal(got, st.data), name
    assert stores["own4096"].block == 4096 and stores["own1152"].block == 1152
    for name in ("own4096", "own1152", "mono192_unaligned", "stereo192"):
        assert stores[name].n % stores[name].block == 37 and stores[name].n % 4, name  # a short last frame, rows of no multiple of 16 bytes
    assert stores["own_i64"].n % stores["own_i64"].block == (4096 + 37) % 1152 == 677 and stores["own_i64"].n % 2
    x = stores["own_i64"].data
    assert np.any(x >> 32 > 0) and np.any(x >> 32 < -1)  # the high word is needed, with either sign


def test_nothing_expected_equals_the_sentinel(stores):
    for name, st in stores.items():
        arrays = [st.data] + ([st.floats] if st.floats is not None else [])
        assert (st.floats is not None) == (name in E.FLOAT_STORES)
        for a in arrays:
            assert a.dtype.itemsize == (4 if st.channels == 1 else 8)
            bits = a.view(E._uint(a.dtype))
            assert not np.any(bits == E.sentinel_bits(a.dtype)), (name, a.dtype)
            if a.dtype.kind == "f":
                assert np.all(np.isfinite(a)), name
                # neighbouring rows restore differently: a row restored with another row's offset and gain shows
                assert st.offsets[0] != st.offsets[1] and st.gains[0] != st.gains[1]
    assert np.isnan(E.sentinel(np.float32)) and E.sentinel(np.int32) == np.int32(-1515870811)
    for dt, wide in ((np.int32, np.int32), (np.float32, np.int32), (np.int64, np.int64), (np.float64, np.int64)):
        assert np.array([E.sentinel_int(dt)], dtype=wide).tobytes() == np.array([E.sentinel(dt)]).tobytes()
    assert E.sentinel(np.int64).tobytes() == E.sentinel(np.float64).tobytes() == b"\xa5" * 8


def test_edge_positions():
    assert E.edge_positions(8 * 192 + 37, 192) == [0, 1, 2, 3, 4, 5, 15, 16, 17, 31, 32, 33, 191, 192, 193, 223, 224, 225, 1535, 1536,
                                                   1537, 1568, 1569, 1570, 1571, 1572]
    for n, block in ((2 * 4096 + 37, 4096), (2 * 1152 + 37, 1152), (4 * 192, 192), (4096 + 37, 1152)):
        pos = E.edge_positions(n, block)
        last0 = E.last_frame_start(n, block)
        want = set(range(6)) | {31, 32, 33, block - 1, block, block + 1, block + 31, block + 32, block + 33, last0 - 1, last0, last0 + 1}
        want |= set(range(n - 5, n))
        assert want <= set(pos) and set(C.positions(n, block)) <= set(pos) and pos == sorted(set(pos)) and 0 <= pos[0] and pos[-1] == n - 1
    assert set(E.slice_counts(192)) == {1, 2, 3, 4, 5, 31, 32, 33, 191, 192, 193, 385}


def test_windows_reach_every_residue_shape_and_edge(stores):
    for name, st in stores.items():
        w, wins, _ = _lists(st)
        n, block = st.n, st.block
        assert all(0 <= f < l <= n and 0 <= m < w for f, l, m in wins), name
        assert len(set(wins)) == len(wins) <= 140, (name, len(wins))
        # the pointer's residue m is the address residue of row 0 (an underrun shows there) and, since m -> m + 63 count is a
        # bijection modulo w, every residue occurs for the last row too (an overrun shows there)
        res = {(m, f % w, (l - f) % w) for f, l, m in wins}
        assert res == set(itertools.product(range(w), repeat=3)), name
        last_row = {((m + (E.ROWS - 1) * (l - f)) % w, f % w, (l - f) % w) for f, l, m in wins}
        assert last_row == set(itertools.product(range(w), repeat=3)), name
        shapes = set().union(*(E.window_shapes(f, l, n, block) for f, l, m in wins))
        assert shapes == set(E.SHAPES), (name, set(E.SHAPES) - shapes)
        # ... and with every row of the call 16-byte aligned (what the whole-tile store asks of a wave), for each shape
        # that can be: not inside one 4-group, and the whole stream only where its length allows
        aligned = set().union(*(E.window_shapes(f, l, n, block) for f, l, m in wins if m == 0 and f % w == 0 and (l - f) % w == 0))
        assert aligned >= set(E.SHAPES) - {"in_group"} - ({"whole"} if n % w else set()), (name, aligned)
        pos = set(E.edge_positions(n, block))
        assert {f for f, l, m in wins} == pos and {l - 1 for f, l, m in wins} == pos, name
        assert (0, n) in {(f, l) for f, l, m in wins}, name


def test_window_shapes():
    n, b = 8 * 192 + 37, 192
    assert E.window_shapes(4, 8, n, b) == {"in_group"} and E.window_shapes(3, 5, n, b) == {"in_tile"}
    assert E.window_shapes(31, 33, n, b) == {"in_frame"} and E.window_shapes(0, 192, n, b) == {"in_frame", "ends_at_edge"}
    assert E.window_shapes(191, 193, n, b) == {"cross_one"} and E.window_shapes(191, 385, n, b) == {"cross_two"}
    assert E.window_shapes(1536, 1540, n, b) == {"in_group", "starts_in_last"}
    assert E.window_shapes(1535, 1537, n, b) == {"cross_one", "ends_in_last"}
    assert E.window_shapes(0, n, n, b) == {"cross_two", "ends_in_last", "whole"}
    assert "ends_at_edge" in E.window_shapes(0, 4 * 192, 4 * 192, 192)


def test_one_wave_holds_aligned_and_unaligned_rows(stores):
    """Grid mode, n_decode no multiple of 16 bytes, aligned pointer: the 64 tasks of the first wave -- row of task
    (s, f) at s * n_decode + frame start - first -- hold both kinds, in one frame and across a frame edge."""
    for name, st in stores.items():
        w, wins, _ = _lists(st)
        mixed = [(f, l) for f, l, m in wins if m == 0 and (l - f) % w and set(E.wave_alignment(f, l, m, st.block, w)) == {True, False}]
        assert any(f // st.block == (l - 1) // st.block for f, l in mixed), name
        assert any(f // st.block != (l - 1) // st.block for f, l in mixed), name
        # a moved pointer leaves no row aligned, a multiple of 16 bytes from an aligned first sample every row
        assert not any(E.wave_alignment(0, 5, 1, st.block, w)) and all(E.wave_alignment(0, 4, 0, st.block, w))


def test_slice_batches(stores):
    for name, st in stores.items():
        w, _, batches = _lists(st)
        n, block = st.n, st.block
        kinds = [b.kind for b in batches]
        assert set(kinds) == {"single", "pair", "big", "aligned"} and kinds.count("big") == 4, name
        counts, res, monotonic = set(), set(), {}
        for b in batches:
            tasks = E.batch_tasks(b, block)
            assert all(0 <= s < E.ROWS and f >= 0 and c > 0 and f + c <= n for s, f, c in b.slices), name
            assert 0 <= b.m < w and b.verify in (0, 1)
            if b.kind == "single":
                assert len(b.slices) == 1 and tasks == 1
            elif b.kind == "pair":
                assert len(b.slices) == 2 and tasks <= 8  # (the task table rides in the latency decoder's arguments)
            else:
                assert tasks >= 128, (name, b.kind, tasks)
            ends = sorted((o, o + c) for (s, f, c), o in zip(b.slices, b.out_offset))
            gaps = [b2 - e1 for (_, e1), (b2, _) in zip(ends, ends[1:])]
            assert min(b.out_offset) == 0 and all(g >= 0 for g in gaps) and ends[-1][1] + b.m == b.span, name
            if b.kind == "big":
                assert {0, 1, 2, 3, 5} == set(gaps), name
                counts |= {c for _, _, c in b.slices}
                # neighbouring tasks differ in where their rows start modulo 16 bytes: every wave mixes them
                al = [(b.m + o - f) % w == 0 for (s, f, c), o in zip(b.slices, b.out_offset)]
                assert all(len(set(al[i : i + 32])) == 2 for i in range(0, len(al) - 32, 32)), name
            if b.kind == "aligned":
                assert b.m == 0 and set(gaps) == {E.ALIGNED_GAP} and all(o % w == 0 and f % w == 0 and c % w == 0 for (s, f, c), o in zip(b.slices, b.out_offset))
                assert len({(f % block, min(block, f % block + c)) for s, f, c in b.slices}) >= 8, name  # lo and hi differ
            monotonic.setdefault(b.kind, []).append(list(b.out_offset) == sorted(b.out_offset))
            res |= {((b.m + o) % w, f % w, c % w) for (s, f, c), o in zip(b.slices, b.out_offset)}
        assert counts == set(E.slice_counts(block)), name
        assert res == set(itertools.product(range(w), repeat=3)), name
        assert monotonic["big"] == [True, False, True, False] and monotonic["pair"].count(False) == 4, name
        assert sum(b.verify for b in batches) == 1 and [b.verify for b in batches if b.kind == "pair"][0] == 1, name
        firsts = {f for b in batches if b.kind == "big" for _, f, _ in b.slices}
        lasts = {f + c - 1 for b in batches if b.kind == "big" for _, f, c in b.slices}
        assert set(E.edge_positions(n, block)) <= firsts and set(E.edge_positions(n, block)) <= lasts, name


def test_expected_image_and_checker():
    dt = np.int32
    a, b = np.arange(1, 6, dtype=dt), np.arange(11, 14, dtype=dt)
    guard, total = 16, 16 + 12 + 16
    pl = [(1, a), (8, b)]  # elements 17..21 and 24..26; a gap of two between them
    img = E.expected_image(total, guard, pl)
    s = E.sentinel(dt)
    assert img.dtype == dt and img.size == total
    assert img.tolist() == [s] * 17 + a.tolist() + [s] * 2 + b.tolist() + [s] * 17
    assert E.check_image(img.copy(), img, guard, pl) is None
    with pytest.raises(AssertionError):
        E.expected_image(total, guard, [(1, a), (5, b)])  # overlap
    with pytest.raises(AssertionError):
        E.expected_image(total, guard, [(10, b)])  # reaches into the back guard

    def report(index, value):
        out = img.copy()
        out[index] = value
        return E.check_image(out, img, guard, pl)

    r = report(22, 99)  # one past the end of slice 0
    assert r.startswith("1 elements differ; the first is element 22 (gap, 1 behind the end of slice 0), written"), r
    r = report(16, 99)  # one in front of the first slice, still behind the guard
    assert "element 16 (gap in front of the first slice), written" in r, r
    r = report(23, 99)  # one before the start of slice 1
    assert "element 23 (gap, 2 behind the end of slice 0), written" in r, r
    r = report(25, s)  # one element left unwritten
    assert "element 25 (slice 1, element 1 of 3), left unwritten" in r, r
    assert "front guard, 1 before its end" in report(15, 0) and "back guard, 0 behind its start" in report(total - guard, 0)
    r = report(27, 7)  # behind the last slice
    assert "(gap, 1 behind the end of slice 1)" in r, r
    # float32: the sentinel is a NaN and the comparison is on bits
    f = np.array([1.5, -2.0], dtype=np.float32)
    fimg = E.expected_image(40, 16, [(3, f)])
    assert fimg.dtype == np.float32 and np.isnan(fimg[0]) and fimg.view(np.uint32)[0] == 0xFFA5A5A5
    assert E.check_image(fimg.copy(), fimg, 16, [(3, f)]) is None
    out = fimg.copy()
    out[21] = np.float32(0.0)
    assert "element 21 (gap, 1 behind the end of slice 0), written" in E.check_image(out, fimg, 16, [(3, f)])
    out = fimg.copy()
    out.view(np.uint32)[19] = 0xFFA5A5A5
    assert "left unwritten" in E.check_image(out, fimg, 16, [(3, f)])


def test_placements_are_numpy_slices(stores):
    st = stores["mono192_unaligned"]
    w, wins, batches = _lists(st)
    f, l, m = next(x for x in wins if x[2] == 1)
    img = E.expected_image(E.buffer_elems(m + E.ROWS * (l - f)), E.GUARD, E.window_placements(st, f, l, m))
    assert img.size % 4 == 0 and np.array_equal(img[E.GUARD + m : E.GUARD + m + E.ROWS * (l - f)].reshape(E.ROWS, l - f), st.data[:, f:l])
    assert (img[: E.GUARD + m].view(np.uint32) == 0xA5A5A5A5).all() and (img[E.GUARD + m + E.ROWS * (l - f) :].view(np.uint32) == 0xA5A5A5A5).all()
    for b in batches:
        for floats in (False, True):
            pl = E.batch_placements(st, b, floats)
            img = E.expected_image(E.buffer_elems(b.span), E.GUARD, pl)
            src = st.floats if floats else st.data
            written = sum(c for _, _, c in b.slices)
            assert np.count_nonzero(img.view(np.uint32) != E.sentinel_bits(img.dtype)) == written
            (s, f, c), o = b.slices[-1], b.out_offset[-1]
            assert np.array_equal(img[E.GUARD + b.m + o : E.GUARD + b.m + o + c].view(np.uint32), src[s, f : f + c].view(np.uint32))
