"""Builders for the decoders' output-footprint tests (tests/test_decode_edges.py checks their preconditions on the CPU,
tests/test_gpu_decode_footprint.py runs them on the GPU).  Nothing here calls the library or the GPU: every store comes
with the array it decodes to, so what a decode call must leave in its output buffer -- the requested samples at their
places and the sentinel everywhere else -- is numpy slicing of known samples.

A store has 64 streams: in grid mode (one sample range of every stream) a wave of the throughput decoder then holds 64
consecutive (stream, frame) tasks.  Windows and slices are built from the frame, tile and 4-group edges of a stream, and
each list is a greedy cover of the classes tests/test_decode_edges.py asserts, so it is as short as those allow."""
from collections import namedtuple
from functools import lru_cache

import numpy as np

from tests import compare_corpus as C
from tests import quant_model as M
from tests.conftest import sinusoid_noise_i32

GUARD = 8192  # sentinel elements in front of and behind the output: more than any tile row or whole frame a wrong path could reach
ROWS = 64
TILE = 32  # samples between two cooperative stores of the throughput decoder
GAPS = (0, 1, 2, 3, 5)  # sentinel elements between two slices, in rotation
ALIGNED_GAP = 4  # ... and in the batches whose slices all start on a 16-byte boundary
SENTINEL_BITS = {"int32": 0xA5A5A5A5, "float32": 0xFFA5A5A5, "int64": 0xA5A5A5A5A5A5A5A5, "float64": 0xA5A5A5A5A5A5A5A5}

ONE_CHANNEL = ["own4096", "own1152", "mono192_aligned", "mono192_unaligned"] + list(C.UNIFORM)
TWO_CHANNEL = ["stereo192", "own_i64"]
STORES = ONE_CHANNEL + TWO_CHANNEL
FLOAT_STORES = ("own4096", "mono192_unaligned", "stereo192", "own_i64")

# data: the integers the store decodes to [ROWS, n]; floats: what the fused restore makes of them with offsets / gains (or None)
Store = namedtuple("Store", "name blob starts nbytes data n block channels offsets gains floats")
# slices: (stream, first, count) per slice; out_offset: element offset of each slice from the output pointer; m: elements
# by which the output pointer is moved off its 16-byte aligned base; span: elements from the pointer to the end of the last slice
Batch = namedtuple("Batch", "kind slices out_offset m span verify")


# ------------------------------------------------------------------------------------------------------------ stores

def _i64(n_ch, n, seed):
    rng = np.random.default_rng(seed)
    return sinusoid_noise_i32(n_ch, n, seed=seed).astype(np.int64) * 70001 + rng.integers(-9, 10, (n_ch, n))


def _float_params(dtype):
    """Per-stream offsets and gains: neighbouring rows differ in both, so a row restored with another row's pair shows."""
    r = np.arange(ROWS)
    return ((r % 7) * 0.25).astype(dtype), (64.0 * (1 + r % 3)).astype(dtype)


def _repeat(blob, starts, nbytes, times):
    """The encoded triple `times` times in a row."""
    blob, starts, nbytes = np.asarray(blob), np.asarray(starts, dtype=np.int64), np.asarray(nbytes, dtype=np.int64)
    st = np.concatenate([starts + k * blob.size for k in range(times)])
    return np.tile(blob, times), st, np.tile(nbytes, times)


def build_store(name, oracle=None):
    """The named store.  `oracle` (the CPU encoder of oracle/) is needed for the own* stores only."""
    if name in ("own4096", "own1152"):
        level, block = (5, 4096) if name == "own4096" else (1, 1152)
        n = 2 * block + 37
        data = sinusoid_noise_i32(ROWS, n, seed=601 if name == "own4096" else 602)
        blob, st, nb = oracle.encode_i32(data, level)
        channels = 1
    elif name == "own_i64":
        # 16 streams that need the high word, four times over; level 1: blocks of 1152, so a window can cross two frame edges
        block, n, channels = 1152, 4096 + 37, 2
        x = _i64(16, n, seed=603)
        blob, st, nb = _repeat(*oracle.encode_i64(x, 1), times=ROWS // 16)
        data = np.tile(x, (ROWS // 16, 1))
    else:
        rep = C.uniform(name) if name in C.UNIFORM else C.replicated(**C.GEOMETRIES[name])
        blob, st, nb = C.store(rep, rows=ROWS)
        data, n, block, channels = C.rows(rep, ROWS), rep.n, rep.block, rep.channels
    data = np.ascontiguousarray(data, dtype=np.int32 if channels == 1 else np.int64)
    off = gain = floats = None
    if name in FLOAT_STORES:
        off, gain = _float_params(np.float32 if channels == 1 else np.float64)
        floats = (M.int32_to_float32 if channels == 1 else M.int64_to_float64)(data, off, gain)
    return Store(name, np.asarray(blob), np.asarray(st, dtype=np.int64), np.asarray(nb, dtype=np.int64), data, n, block, channels, off, gain, floats)


def width_of(channels):
    """Elements per 16 bytes of output: residues are taken modulo this."""
    return 4 if channels == 1 else 2


# ----------------------------------------------------------------------------------------------------- edge positions

def last_frame_start(n, block):
    return ((n + block - 1) // block - 1) * block


def edge_positions(n, block):
    """compare_corpus.positions and: 0..5, the tile edge, the frame edge and the tile edge behind it, the first sample of
    the last frame (short where the stream has one) +-1, the last five samples."""
    last0 = last_frame_start(n, block)
    cand = set(C.positions(n, block)) | set(range(6)) | {TILE - 1, TILE, TILE + 1} | set(range(n - 5, n))
    cand |= {block - 1, block, block + 1, block + TILE - 1, block + TILE, block + TILE + 1, last0 - 1, last0, last0 + 1}
    return sorted(p for p in cand if 0 <= p < n)


SHAPES = ("in_group", "in_tile", "in_frame", "cross_one", "cross_two", "starts_in_last", "ends_in_last", "ends_at_edge", "whole")


def window_shapes(first, last, n, block):
    """The classes of [first, last): inside one 4-group / one tile / one frame (the narrowest that holds), crossing one
    frame edge or more than one, starting in the last frame, reaching into it from before, ending exactly at a frame
    edge, the whole stream."""
    f0, f1 = first // block, (last - 1) // block
    last0 = last_frame_start(n, block)
    out = set()
    if f0 == f1:
        a, b = first - f0 * block, last - 1 - f0 * block
        out.add("in_group" if a // 4 == b // 4 else "in_tile" if a // TILE == b // TILE else "in_frame")
    else:
        out.add("cross_one" if f1 - f0 == 1 else "cross_two")
    if first >= last0:
        out.add("starts_in_last")
    elif last > last0:
        out.add("ends_in_last")
    if last % block == 0:
        out.add("ends_at_edge")
    if first == 0 and last == n:
        out.add("whole")
    return out


def _greedy_cover(cands, features):
    """The candidates, in order of choice, that a greedy set cover takes to cover every feature any candidate has."""
    feats = [features(c) for c in cands]
    left = set().union(*feats)
    chosen = []
    while left:
        gain, k = max((len(f & left), -i) for i, f in enumerate(feats))
        chosen.append(cands[-k])
        left -= feats[-k]
    return chosen


def window_features(first, last, m, n, block, width):
    """What a window (with the output pointer moved by m elements) contributes to the cover: its first and last sample,
    its shapes, the residues of (pointer, first, count) -- row 0 starts at element m and the last row, the one whose overrun
    no other row hides, at m + 63 count: with every m both take every residue -- and, per shape, whether every row of the
    call is 16-byte aligned (the whole-tile store needs that of all 64 lanes of a wave)."""
    count = last - first
    out = {("first", first), ("end", last - 1), ("res", m, first % width, count % width)}
    aligned = m == 0 and first % width == 0 and count % width == 0
    for sh in window_shapes(first, last, n, block):
        out.add(("shape", sh))
        if aligned:
            out.add(("aligned", sh))
    if m == 0 and count % width:
        out.add(("mixed_wave",))
    return out


@lru_cache(maxsize=None)
def windows(n, block, width):
    """(first, last, m): windows between edge positions, a greedy cover of window_features."""
    pos = edge_positions(n, block)
    cands = [(a, b + 1, m) for a in pos for b in pos if b >= a for m in range(width)]
    return _greedy_cover(cands, lambda c: frozenset(window_features(*c, n, block, width)))


def wave_alignment(first, last, m, block, width, rows=ROWS):
    """Per task of the first wave of a grid-mode call (task = stream * frames + frame): is its row 16-byte aligned?  The
    decoder's row is the output element of the frame's sample 0: stream * n_decode + (frame start - first)."""
    f0, f1 = first // block, (last - 1) // block
    nfr = f1 - f0 + 1
    out = []
    for task in range(min(64, rows * nfr)):
        s, f = divmod(task, nfr)
        out.append(m == 0 and (s * (last - first) + (f0 + f) * block - first) % width == 0)
    return out


# -------------------------------------------------------------------------------------------------------------- slices

def slice_counts(block):
    return (1, 2, 3, 4, 5, TILE - 1, TILE, TILE + 1, block - 1, block, block + 1, 2 * block + 1)


def edge_slices(n, block):
    """(first, count): every count starting at every edge position, and ending on it, where that fits."""
    out = set()
    for p in edge_positions(n, block):
        for c in slice_counts(block):
            if p + c <= n:
                out.add((p, c))
            if p + 1 - c >= 0:
                out.add((p + 1 - c, c))
    return sorted(out)


def n_frames(first, count, block):
    return (first + count - 1) // block - first // block + 1


def _place(kind, slices, m, phase, monotonic, gaps=GAPS, verify=0):
    """Lay the slices out behind one another in the order of placement, slice j followed by a gap of sentinel."""
    idx = list(range(len(slices)))
    order = idx if monotonic else idx[1::2][::-1] + idx[0::2]
    off = [0] * len(slices)
    cursor = end = m
    for k, j in enumerate(order):
        off[j] = cursor - m
        end = cursor + slices[j][2]
        cursor = end + gaps[(k + phase) % len(gaps)]
    return Batch(kind, tuple(slices), tuple(off), m, end, verify)


@lru_cache(maxsize=None)
def slice_batches(n, block, width):
    """The batches of one stream geometry.
    single: one slice of one frame.  pair: two slices of at most 8 frames together (the first one also with verify=1).
    big: every edge slice, streams in rotation, `width` batches -- one per pointer residue, the gap rotation moved on and
    every other one placed out of order -- of far more than 128 tasks whose neighbours differ in lo, hi and alignment.
    aligned: at least 192 tasks that all start on a 16-byte boundary in stream and output while their lo and hi differ."""
    es = edge_slices(n, block)
    out = []
    one = [e for e in es if n_frames(*e, block) == 1]
    cover = _greedy_cover(one, lambda e: frozenset({("f", e[0] % width, e[1] % width), ("shape",) + tuple(sorted(window_shapes(e[0], e[0] + e[1], n, block)))}))
    for k, (f, c) in enumerate(cover):
        out.append(_place("single", [((7 * k + 3) % ROWS, f, c)], k % width, k, True))
    few = [e for e in es if n_frames(*e, block) <= 4]
    step = max(1, len(few) // 16)
    for k in range(8):
        a, b = few[(2 * k * step) % len(few)], few[((2 * k + 1) * step + 1) % len(few)]
        sl = [((11 * k) % ROWS, *a), ((11 * k + 5) % ROWS, *b)]
        out.append(_place("pair", sl, k % width, k, k % 2 == 0, verify=1 if k == 0 else 0))
    for b in range(4):
        sl = [((5 * i + 17 * b) % ROWS, f, c) for i, (f, c) in enumerate(es)]
        out.append(_place("big", sl, b % width, b, b % 2 == 0))
    al = [e for e in es if e[0] % width == 0 and e[1] % width == 0]
    sl, tasks = [], 0
    while tasks < 192:
        f, c = al[len(sl) % len(al)]
        sl.append(((3 * len(sl) + 1) % ROWS, f, c))
        tasks += n_frames(f, c, block)
    out.append(_place("aligned", sl, 0, 0, True, gaps=(ALIGNED_GAP,)))
    return out


def batch_tasks(batch, block):
    return sum(n_frames(f, c, block) for _, f, c in batch.slices)


# ------------------------------------------------------------------------------------------------- the expected image

def sentinel_bits(dtype):
    return SENTINEL_BITS[np.dtype(dtype).name]


def _uint(dtype):
    return {4: np.uint32, 8: np.uint64}[np.dtype(dtype).itemsize]


def sentinel_int(dtype):
    """The sentinel's bits as the signed integer of the element's size: what a buffer viewed as int32 / int64 is filled with."""
    size = np.dtype(dtype).itemsize
    return sentinel_bits(dtype) - (1 << 8 * size)  # (bit 7 of 0xA5 and of 0xFF is set: always negative)


def sentinel(dtype):
    """The sentinel as a value of dtype: bytes 0xA5 (the NaN 0xFFA5A5A5 for float32)."""
    return np.array([sentinel_bits(dtype)], dtype=_uint(dtype)).view(dtype)[0]


def expected_image(total_elems, guard, placements):
    """The whole output buffer after a call: `total_elems` elements of sentinel, and for every placement (pos, samples) the
    samples at element guard + pos -- pos counts from the end of the front guard, so it includes the pointer's m.  The
    placements lie between the guards and do not overlap."""
    dtype = placements[0][1].dtype
    u = _uint(dtype)
    img = np.full(total_elems, sentinel_bits(dtype), dtype=u)
    taken = np.zeros(total_elems, dtype=bool)
    for pos, samples in placements:
        assert samples.dtype == dtype and samples.ndim == 1
        a, b = guard + pos, guard + pos + samples.size
        assert guard <= a <= b <= total_elems - guard, "a placement reaches into a guard"
        assert not taken[a:b].any(), "placements overlap"
        taken[a:b] = True
        img[a:b] = samples.view(u)
    return img.view(dtype)


def window_placements(store, first, last, m, floats=False):
    src = store.floats if floats else store.data
    return [(m, np.ascontiguousarray(src[:, first:last]).reshape(-1))]


def batch_placements(store, batch, floats=False):
    src = store.floats if floats else store.data
    return [(batch.m + o, np.ascontiguousarray(src[s, f : f + c])) for (s, f, c), o in zip(batch.slices, batch.out_offset)]


def buffer_elems(span, guard=GUARD):
    """Elements of the buffer of a call whose placements end `span` elements behind the front guard (a few spare
    elements, so that the back guard starts on a 16-byte boundary whatever m is)."""
    return guard + (span + 7) // 4 * 4 + guard


def where(index, total_elems, guard, placements):
    """In words, where element `index` of the buffer lies: a guard, a placement (and how far in), or a gap."""
    if index < guard:
        return "front guard, %d before its end" % (guard - index)
    if index >= total_elems - guard:
        return "back guard, %d behind its start" % (index - (total_elems - guard))
    before = None
    for k, (pos, samples) in enumerate(placements):
        a = guard + pos
        if a <= index < a + samples.size:
            return "slice %d, element %d of %d" % (k, index - a, samples.size)
        if a + samples.size <= index and (before is None or a + samples.size > before[1]):
            before = (k, a + samples.size)
    if before is None:
        return "gap in front of the first slice"
    return "gap, %d behind the end of slice %d" % (index - before[1] + 1, before[0])


def check_image(got, want, guard, placements):
    """None if the two buffers hold the same bytes, else a report: how many elements differ and, for the first one, where
    it lies and what it holds."""
    u = _uint(want.dtype)
    g, w = np.asarray(got).view(u).reshape(-1), np.asarray(want).view(u).reshape(-1)
    assert g.shape == w.shape
    bad = np.flatnonzero(g != w)
    if bad.size == 0:
        return None
    i = int(bad[0])
    what = "left unwritten" if int(g[i]) == sentinel_bits(want.dtype) else "written"
    return "%d elements differ; the first is element %d (%s), %s: holds 0x%x, expected 0x%x" % (
        bad.size, i, where(i, w.size, guard, placements), what, int(g[i]), int(w[i]))
