"""Builders for the compare-sink tests on foreign streams (tests/test_compare_corpus.py checks their preconditions on
the CPU, tests/test_gpu_compare_foreign.py runs them on the GPU).  Nothing here calls the library or the oracle: streams
come from tests/golden/flac_writer.py, float values from tests/quant_model.py, and every expected result is numpy on
the known arrays -- the first index where the mutated array differs from the samples, or -1.

A replicated store is one stream packed n times, n its length: row r of the comparison array is changed at sample r,
so one compare call shows whether every sample of every frame is compared."""
from collections import namedtuple

import numpy as np

from tests import quant_model as M
from tests.conftest import sinusoid_noise_i32
from tests.golden import flac_writer as W

Replicated = namedtuple("Replicated", "block n channels samples stream record")

# name -> arguments of replicated().  Block 192: nine frames cycling through the orders 1-8, 9-12, 13-16 and 17-32, the
# last one short (40 or 37 samples); 8 * 192 + 40 samples make rows of a multiple of 16 bytes, 8 * 192 + 37 do not.
# Block 16: orders stay below 16.  The seeds are ones whose drawn coding has a wasted-bits frame (and, two channels, more
# than one channel assignment); tests/test_compare_corpus.py asserts it.
GEOMETRIES = {
    "mono192_aligned": dict(block=192, n=8 * 192 + 40, channels=1, seed=11),
    "mono192_unaligned": dict(block=192, n=8 * 192 + 37, channels=1, seed=12),
    "mono16": dict(block=16, n=16 * 40 + 5, channels=1, seed=13, bucket_cycle=False),
    "stereo192": dict(block=192, n=8 * 192 + 37, channels=2, seed=25),
}
# A decoder pass leaves the frames of another pass idle, and a wave with an idle or a short frame stores (compares) its
# tiles piece by piece.  These streams reach the whole-tile path of each pass: four whole frames of one order bucket, so that
# every wave of a call holds 64 whole frames of the same pass; rows of a multiple of 16 bytes.  name -> (bucket, seed), the
# seed one whose drawn coding gives frame 1 wasted bits.
UNIFORM = {"orders_1-8": (0, 3), "orders_9-12": (1, 3), "orders_13-16": (2, 3), "orders_17-32": (3, 3)}
UNIFORM_LENGTH = 4 * 192
SMALL_LENGTHS = {"aligned": 8 * 192 + 40, "unaligned": 8 * 192 + 37}
I64_MIN = np.int64(-(2**63))
XOR_BITS = {1: (np.int32(1),), 2: (np.int64(1), np.int64(1) << 32, I64_MIN)}  # left, right, right's sign: the side channel too
QUANTA = 2.0**-6


def replicated(block, n, channels, seed, bucket_cycle=True, layout="libflac", samples=None, bucket=None):
    rng = np.random.default_rng(seed)
    x, data, rec = W.write_stream(rng, n, block, channels, layout=layout, bucket_cycle=bucket_cycle, samples=samples, bucket=bucket)
    return Replicated(block, n, channels, x, data, rec)


def small_amplitude(n, layout="libflac"):
    """The one-channel block-192 stream of the float tests: small samples (float32 holds them at QUANTA exactly), frame 4
    scaled by 8 so that it can carry wasted bits."""
    x = sinusoid_noise_i32(1, n, seed=5, amp=2**12)[0]
    x[4 * 192 : 5 * 192] *= 8
    return replicated(192, n, 1, 3, layout=layout, samples=x)


def uniform(name):
    """Four whole frames of small samples, all coded with LPC orders of one bucket, frame 1 scaled by 8 (wasted bits)."""
    bucket, seed = UNIFORM[name]
    x = sinusoid_noise_i32(1, UNIFORM_LENGTH, seed=5, amp=2**12)[0]
    x[192 : 2 * 192] *= 8
    return replicated(192, UNIFORM_LENGTH, 1, seed, bucket_cycle=False, samples=x, bucket=bucket)


def store(rep, rows=None):
    """(blob, starts, nbytes) of the stream packed `rows` times (default: once per sample)."""
    return W.pack([rep.stream] * (rep.n if rows is None else rows))


def rows(rep, rows=None):
    """The array the store decodes to: the samples, once per row."""
    return np.tile(rep.samples, (rep.n if rows is None else rows, 1))


def positions(n, block):
    """The frame, tile and piece edges of a stream of n samples, sorted."""
    last0 = ((n + block - 1) // block - 1) * block
    cand = {0, 1, 3, 4, 15, 16, 17, 31, 32, 33, block - 1, block, block + 1, last0 - 1, last0, last0 + 1, n - 2, n - 1}
    return sorted(p for p in cand if 0 <= p < n)


def expected_first(mutated, original):
    """Per row the first index where the two arrays differ, or -1."""
    diff = np.asarray(mutated) != np.asarray(original)
    return np.where(diff.any(axis=-1), diff.argmax(axis=-1), -1).astype(np.int64)


def edge_mutation(samples, n, block, j, bit):
    """Rotation j: stream i with `bit` flipped at positions(n, block)[(i + j) % len]."""
    pos = positions(n, block)
    y = samples.copy()
    for i in range(y.shape[0]):
        y[i, pos[(i + j) % len(pos)]] ^= bit
    return y


def edge_rotations(samples, n, block, bit):
    """Every rotation, stacked: row j * len(samples) + i is stream i of rotation j."""
    return np.concatenate([edge_mutation(samples, n, block, j, bit) for j in range(len(positions(n, block)))])


def xor_diagonal(data, bit):
    y = data.copy()
    r = np.arange(y.shape[0])
    y[r, r] ^= bit
    return y


def add_from_diagonal(data, delta, skip=0):
    """Row r with delta added (wrapping) to the samples from r + skip on."""
    y = data.copy()
    r = np.arange(y.shape[0])
    y[np.arange(y.shape[1])[None, :] >= r[:, None] + skip] += y.dtype.type(delta)
    return y


def float_case(rep):
    """(x float32 [n, n], ints, offsets, gains): the replicated rows restored with quanta 2^-6 and offsets (r % 7) / 4."""
    ints = rows(rep)
    off = ((np.arange(rep.n) % 7) * 0.25).astype(np.float32)
    gain = np.full(rep.n, 1.0 / QUANTA, dtype=np.float32)
    return M.int32_to_float32(ints, off, gain), ints, off, gain


def bump_diagonal(x, by):
    y = x.copy()
    r = np.arange(y.shape[0])
    y[r, r] += y.dtype.type(by)
    return y


def nextafter_diagonal(x):
    y = x.copy()
    r = np.arange(y.shape[0])
    y[r, r] = np.nextafter(y[r, r], y.dtype.type(np.inf))
    return y


def _frame_offsets(seg):
    """Byte offset of every frame of one stream, from its SEEKTABLE (one point per frame; placeholders skipped)."""
    off, points = 4, []
    while True:
        last, typ = seg[off] >> 7, seg[off] & 0x7F
        ln = int.from_bytes(bytes(seg[off + 1 : off + 4]), "big")
        if typ == 3:
            body = bytes(seg[off + 4 : off + 4 + ln])
            for k in range(ln // 18):
                if int.from_bytes(body[18 * k : 18 * k + 8], "big") != 2**64 - 1:
                    points.append(int.from_bytes(body[18 * k + 8 : 18 * k + 16], "big"))
        off += 4 + ln
        if last:
            return [off + p for p in points]


def _header_bytes(seg, at):
    """Length of the frame header at `at`, CRC-8 included (RFC 9639 9.1)."""
    assert seg[at] == 0xFF and seg[at + 1] == 0xF8
    bsc, src, u0 = seg[at + 2] >> 4, seg[at + 2] & 15, seg[at + 4]
    extra = 0
    while u0 & (0x80 >> extra) and extra < 7:
        extra += 1
    extra = max(extra - 1, 0)
    return 5 + extra + {6: 1, 7: 2}.get(bsc, 0) + (1 if src == 12 else 2 if src in (13, 14) else 0) + 1

