"""FlacArray.reindex restated over bytes (tests/test_reindex_model.py checks its preconditions on the CPU,
tests/test_gpu_reindex.py compares the GPU with it).  Nothing here calls the library or the GPU.

The output of one stream of n samples, block size B, nf = ceil(n / B) frames that begin at the bytes `frame_offsets` of it:
    "fLaC" | 00 00 00 22 | the source's bytes 8..41 (its STREAMINFO) | 83, 18 nf as 24 bits |
    nf seek points (f B as u64, frame_offsets[f] - frame_offsets[0] as u64, min(B, n - f B) as u16, big-endian) |
    the source's bytes from frame_offsets[0] to its end.
`find_frames` locates the frames of an intact stream from nothing but its bytes: frame f + 1 begins at the first position
behind frame f that carries the header of frame f + 1 (tests/scrub_model.header_ok: sync code, number, block size, CRC-8)
and has the CRC-16 of everything since the begin of frame f in the two bytes in front of it."""
import numpy as np

from tests import scrub_model as SM
from tests.golden import flac_writer as W
from tests.golden import make_golden as G


def first_frame(seg):
    """Offset of the first frame of a stream: behind the metadata block that carries the last-block flag."""
    assert seg[:4] == b"fLaC"
    off = 4
    while True:
        last = seg[off] >> 7
        off += 4 + int.from_bytes(seg[off + 1 : off + 4], "big")
        if last:
            return off


def find_frames(seg, n, block, nch):
    """Offsets of the nf frames of the intact stream `seg` (bytes)."""
    nf = -(-n // block)
    at = first_frame(seg)
    offs = [at]
    assert SM.header_ok(seg[at : at + 16], nch, 0, min(block, n)), "no frame 0 behind the metadata"
    for f in range(1, nf):
        want_bs = min(block, n - f * block)
        p = at + 8
        while True:
            p = seg.find(b"\xff\xf8", p)
            assert p >= 0, "frame %d not found" % f
            if SM.header_ok(seg[p : p + 16], nch, f, want_bs) and G.crc16(seg[at : p - 2]) == int.from_bytes(seg[p - 2 : p], "big"):
                break
            p += 1
        offs.append(p)
        at = p
    assert G.crc16(seg[at : len(seg) - 2]) == int.from_bytes(seg[-2:], "big"), "the last frame does not end with the stream"
    return offs


def reindex_stream(stream_bytes, frame_offsets, n, block):
    seg = bytes(stream_bytes)
    nf = -(-n // block)
    assert len(frame_offsets) == nf and 18 * nf < (1 << 24)
    out = b"fLaC" + bytes([0, 0, 0, 34]) + seg[8:42] + bytes([0x83]) + (18 * nf).to_bytes(3, "big")
    for f, o in enumerate(frame_offsets):
        out += (f * block).to_bytes(8, "big") + (o - frame_offsets[0]).to_bytes(8, "big") + min(block, n - f * block).to_bytes(2, "big")
    return out + seg[frame_offsets[0] :]


def split(blob, starts, nbytes):
    blob = bytes(np.asarray(blob, dtype=np.uint8))
    return [blob[int(s) : int(s) + int(b)] for s, b in zip(np.asarray(starts).reshape(-1), np.asarray(nbytes).reshape(-1))]


def store_offsets(blob, starts, nbytes, n, block, nch):
    """find_frames of every stream of an intact store."""
    return [find_frames(seg, n, block, nch) for seg in split(blob, starts, nbytes)]


def reindex_store(blob, starts, nbytes, n, block, nch, offsets=None):
    """The reindexed store (blob, starts, nbytes), streams back to back from 0.  `offsets`: the frame offsets of every
    stream (default: found in the store, which must then be intact)."""
    segs = split(blob, starts, nbytes)
    if offsets is None:
        offsets = [find_frames(seg, n, block, nch) for seg in segs]
    return W.pack([reindex_stream(seg, o, n, block) for seg, o in zip(segs, offsets)])


def own_offsets(seg):
    """Frame offsets of an own-layout stream, read from its SEEKTABLE."""
    assert seg[:4] == b"fLaC" and seg[4] == 0 and seg[42] == 0x83
    stl = int.from_bytes(seg[43:46], "big")
    assert stl % 18 == 0
    return [46 + stl + int.from_bytes(seg[46 + 18 * f + 8 : 46 + 18 * f + 16], "big") for f in range(stl // 18)]


def to_foreign(blob, starts, nbytes):
    """An own-layout store in libFLAC's layout: STREAMINFO, a VORBIS_COMMENT (marked last), the frames -- the frame
    extent taken from the own SEEKTABLE.  Returns (blob, starts, nbytes)."""
    out = []
    for seg in split(blob, starts, nbytes):
        assert seg[:4] == b"fLaC" and seg[4:8] == bytes([0, 0, 0, 34]) and seg[42] == 0x83
        stl = int.from_bytes(seg[43:46], "big")
        vc = W._vorbis()
        out.append(seg[:42] + bytes([0x84]) + len(vc).to_bytes(3, "big") + vc + seg[46 + stl :])
    return W.pack(out)
