"""Stores for the fold across streams (FlacArray.common_mode, K7X).

Builders only: nothing here calls the library's device side or the GPU.  tests/test_xsum_corpus.py asserts on the CPU that
each store has what it is for; tests/test_gpu_common_mode.py sends them through the device paths.

  A   131 one-channel streams of tests/golden/flac_writer.write_stream, block 64, n = 3 * 64 + 21: an odd row length, a
      last frame shorter than a 32-sample tile, two tiles per full frame, three plan rows (64 + 64 + 3 lanes) in one group
  B   the same at block 192, n = 2 * 192 + 40: six tiles per frame, and LPC orders 17-32 unrestricted by the block
  C   written by the library at level 5: 70 streams of 4096 + 100 samples of full-range noise (wide_corpus.wide_rows, its
      uniform rows), so that a column's sum of squares passes 2^64
  D   5 two-channel (int64) streams of the writer, block 64, n = 3 * 64 + 21

K7X folds the 64 lanes of a wave, which hold one frame index of the 64 streams of a plan row.  What can go wrong there
depends on what those 64 frames are: their LPC orders decide which <MO, MO_DONE> pass decodes each (the others' tile rows
hold leftovers), their wasted bits differ per row.  The writer draws both per frame; `frame_records` reads them back from
the stream it wrote (frame header, then the first subframe's header byte), and the seeds below were chosen so that the
preconditions of test_xsum_corpus.py hold.
"""
import functools
from types import SimpleNamespace

import numpy as np

from tests import wide_corpus
from tests.golden import flac_writer as W

SEED_A, SEED_B, SEED_D = 7100, 7300, 7500
N_A, BLOCK_A, LEN_A = 131, 64, 3 * 64 + 21
N_B, BLOCK_B, LEN_B = 131, 192, 2 * 192 + 40
N_C, LEN_C = 70, 4096 + 100
N_D, BLOCK_D, LEN_D = 5, 64, 3 * 64 + 21
SIX_SIZES = (0, 1, 63, 64, 65, 130)  # the group sizes the plan is checked at (323 streams)
SIX_FIT = (0, 1, 63, 64, 3, 0)     # six interleaved groups that fit the 131 streams of stores A and B


def _metadata_end(data):
    """(offset of the first frame, payload of the SEEKTABLE or None) of a stream."""
    assert data[:4] == b"fLaC"
    off, seek = 4, None
    while True:
        last, typ = data[off] >> 7, data[off] & 0x7F
        ln = int.from_bytes(data[off + 1 : off + 4], "big")
        if typ == 3:
            seek = data[off + 4 : off + 4 + ln]
        off += 4 + ln
        if last:
            return off, seek


def frame_records(data):
    """Per frame of a one-channel stream written with layout="own" (a complete SEEKTABLE): dict(kind, order, wasted) of
    its subframe, read from the bytes -- kind "const" / "verbatim" / "fixed" / "lpc", order 0 for the first two."""
    first, seek = _metadata_end(data)
    assert seek is not None and len(seek) % 18 == 0
    out = []
    for p in range(len(seek) // 18):
        at = first + int.from_bytes(seek[18 * p + 8 : 18 * p + 16], "big")
        assert data[at] == 0xFF and data[at + 1] == 0xF8
        bsc, src = data[at + 2] >> 4, data[at + 2] & 15
        u0 = data[at + 4]
        extra = 0
        while u0 & (0x40 >> extra) and u0 & 0x80:
            extra += 1
        h = 4 + 1 + extra + (1 if bsc == 6 else 2 if bsc == 7 else 0) + (1 if src == 12 else 2 if src in (13, 14) else 0) + 1
        sub = data[at + h]
        assert sub & 0x80 == 0
        tc = (sub >> 1) & 0x3F
        kind = "const" if tc == 0 else "verbatim" if tc == 1 else "fixed" if 8 <= tc <= 12 else "lpc"
        assert kind != "lpc" or tc >= 32
        order = tc - 8 if kind == "fixed" else (tc & 31) + 1 if kind == "lpc" else 0
        out.append({"kind": kind, "order": order, "wasted": bool(sub & 1)})
    return out


def _writer_store(seed, count, n, block, channels):
    """`count` streams, stream i from seed + i, in both layouts: the frames are the same bytes (the layouts "libflac" and
    "own" draw nothing), so the records read from the "own" form describe the "libflac" form too."""
    samples, own, lib, frames = [], [], [], []
    for i in range(count):
        x, d_own, _ = W.write_stream(np.random.default_rng(seed + i), n, block, channels, layout="own", bucket_cycle=False, bucket=None)
        y, d_lib, _ = W.write_stream(np.random.default_rng(seed + i), n, block, channels, layout="libflac", bucket_cycle=False, bucket=None)
        assert np.array_equal(x, y)
        f_own, f_lib = _metadata_end(d_own)[0], _metadata_end(d_lib)[0]
        assert d_own[f_own:] == d_lib[f_lib:]
        samples.append(x)
        own.append(d_own)
        lib.append(d_lib)
        frames.append(frame_records(d_own) if channels == 1 else None)
    return SimpleNamespace(samples=np.stack(samples), n=n, block=block, channels=channels, frames=frames,
                           layouts={"libflac": W.pack(lib), "own": W.pack(own)})


@functools.lru_cache(maxsize=None)
def store_a():
    return _writer_store(SEED_A, N_A, LEN_A, BLOCK_A, 1)


@functools.lru_cache(maxsize=None)
def store_b():
    return _writer_store(SEED_B, N_B, LEN_B, BLOCK_B, 1)


@functools.lru_cache(maxsize=None)
def store_d():
    return _writer_store(SEED_D, N_D, LEN_D, BLOCK_D, 2)


@functools.lru_cache(maxsize=None)
def samples_c():
    """70 of wide_rows' uniform rows (every FULL_EVERY-th, the constant ones left out): full-range int32 noise."""
    rows = [s for s in range(wide_corpus.FULL_EVERY, 200 * wide_corpus.FULL_EVERY, wide_corpus.FULL_EVERY) if s % wide_corpus.CONST_EVERY][:N_C]
    assert len(rows) == N_C
    return wide_corpus.wide_rows(rows[-1] + 1, LEN_C, False, seed=5, rows=np.asarray(rows))


def ranges(n, block):
    """The sample ranges every grouping runs over: everything; [1, n - 1); inside one tile; from a frame's second tile
    into the short last frame; empty."""
    nf = (n + block - 1) // block
    return ((0, n), (1, n - 1), (block + 3, block + 20), (block + 40, (nf - 1) * block + 5), (17, 17))


def interleaved(sizes, seed):
    """(labels, rng): sum(sizes) shuffled (interleaved) labels, sizes[g] of them g, and the generator for what follows."""
    rng = np.random.default_rng(seed)
    lab = rng.permutation(np.repeat(np.arange(len(sizes)), sizes)).astype(np.int64)
    return lab, rng


def groupings(n_stream=131):
    """(name, streams or None, labels or None, n_groups) over a store of 131 streams.  The six group sizes of the plan test
    (0, 1, 63, 64, 65, 130) add up to 323 streams, more than the store has and no stream may be named twice, so they come
    in three interleaved groupings that each fit: "six" = sizes (0, 1, 63, 64, 3, 0), "halves" = (65, 0, 66), "most" =
    (130, 1).  Beside them: one group of everything, and a reversed odd subset in one group."""
    assert n_stream == 131
    out = [("one", None, None, 1)]
    for name, sizes, seed in (("six", SIX_FIT, 11), ("halves", (65, 0, 66), 12), ("most", (130, 1), 13)):
        lab, rng = interleaved(sizes, seed)
        sel = rng.permutation(n_stream)[: lab.size].astype(np.int64)
        out.append((name, sel, lab, len(sizes)))
    out.append(("odd", np.arange(n_stream - 2, 0, -2).astype(np.int64), None, 1))  # 129, 127, ..., 1
    return tuple(out)


def expected(x, first, last, streams, labels, n_groups):
    """numpy on the known samples x [S, n]: (count [G], sum int64 [G, m], sum of squares as Python integers [G, m] or None
    for int64 samples)."""
    sel = np.arange(x.shape[0]) if streams is None else np.asarray(streams)
    lab = np.zeros(sel.size, dtype=np.int64) if labels is None else np.asarray(labels)
    m = last - first
    count = np.zeros(n_groups, dtype=np.int64)
    sm = np.zeros((n_groups, m), dtype=np.int64)
    sq = None if x.dtype == np.int64 else np.zeros((n_groups, m), dtype=object)
    for g in range(n_groups):
        seg = x[sel[lab == g], first:last]
        count[g] = seg.shape[0]
        sm[g] = np.sum(seg, axis=0, dtype=np.int64)
        if sq is not None and seg.shape[0]:
            sq[g] = np.sum(seg.astype(object) * seg.astype(object), axis=0)
    return count, sm, sq
