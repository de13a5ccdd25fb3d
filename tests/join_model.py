"""Plain-Python model of FlacArray.concatenate's aligned route: the specification the HIP join kernel (K15) follows.

Given the streams of the parts x_0, x_1, ... (this encoder's layout: "fLaC", STREAMINFO, a SEEKTABLE of one point per
frame, frames), every part but the last a whole number of blocks long, `join` writes the streams a one-shot encode of
np.concatenate(x_i, axis=-1) writes, byte for byte:
  - a new stream header: STREAMINFO total samples sum N_p, a SEEKTABLE rebuilt from the new frame sizes (running offsets,
    not the kernel's closed forms);
  - frame k of part p with frame number base_p + k: new UTF-8 number, CRC-8 and CRC-16 RECOMPUTED over the whole frame
    (window_model.renumber_whole, not the linear identity the kernel uses -- the model is the independent side).
A single part is returned as it is.  Nothing here calls the library.

`join` also records what the copies look like (`stats`), so that a test can assert that its corpus reaches the hard
cases: (source address - destination address) mod 16 of every payload copy, taken from the blob offsets (the device
buffers are 16-byte aligned), the smallest payload, VERBATIM subframes and the bytes each header GROWS by.  The frames of
part 0 keep their numbers and move as one block on the device: they enter the statistics as that one copy only.

The module also holds the corpus tests/test_join_model.py and tests/test_gpu_join.py share.
"""
import numpy as np

from tests import window_model as W
from tests.append_model import parse_stream, stream_header


def new_stats():
    return {"align": set(), "min_payload": 1 << 60, "verbatim": 0, "grow": set(), "frames": 0}


def join_stream(parts, stats=None, src_at=None, dst_at=0, offsets=None):
    """One stream out of the streams `parts` (bytes).  src_at[p] / dst_at: where part p's stream and the new stream
    start in their blobs (for the statistics).  offsets: a list that receives (part, frame of the part, offset in the
    new body) of every frame."""
    parts = [bytes(p) for p in parts]
    parsed = [parse_stream(p) for p in parts]
    B, nch = parsed[0][0], parsed[0][1]
    if any((q[0], q[1]) != (B, nch) for q in parsed):
        raise ValueError("the parts differ in block size or channels")
    if any(q[2] % B for q in parsed[:-1]) or any(q[2] <= 0 or len(q[3]) != -(-q[2] // B) for q in parsed):
        raise ValueError("the model covers parts that end on a frame boundary (all but the last)")
    if len(parts) == 1:
        return parts[0]
    src_at = [0] * len(parts) if src_at is None else src_at
    hb_new = 46 + 18 * sum(len(q[3]) for q in parsed)
    points, frames, off, base = [], [], 0, 0
    for p, (old, (_, _, n, pts, hb_old)) in enumerate(zip(parts, parsed)):
        body = len(old) - hb_old
        if stats is not None and p == 0:
            stats["align"].add((src_at[0] + hb_old - (dst_at + hb_new)) % 16)
        for k, (o, count) in enumerate(pts):
            e = pts[k + 1][0] if k + 1 < len(pts) else body
            fr = old[hb_old + o : hb_old + e]
            new, h_old, h_new = W.renumber_whole(fr, base + k) if p else (fr, 0, 0)
            if stats is not None and p:
                stats["align"].add((src_at[p] + hb_old + o + h_old - (dst_at + hb_new + off + h_new)) % 16)
                stats["min_payload"] = min(stats["min_payload"], len(fr) - 2 - h_old)
                stats["verbatim"] += (fr[h_old] >> 1) == 1
                stats["grow"].add(h_new - h_old)
                stats["frames"] += 1
            if offsets is not None:
                offsets.append((p, k, off))
            points.append(((base + k) * B, off, count))
            frames.append(new)
            off += len(new)
        base += len(pts)
    return stream_header(B, nch, sum(q[2] for q in parsed), points) + b"".join(frames)


def join(triples, stats=None):
    """(blob, starts, nbytes) of the join of the parts' (blob, starts, nbytes), all streams."""
    triples = [(np.asarray(b, np.uint8), np.ravel(s), np.ravel(n)) for b, s, n in triples]
    out, at = [], 0
    for s in range(len(triples[0][1])):
        streams = [b[int(st[s]) : int(st[s]) + int(nb[s])].tobytes() for b, st, nb in triples]
        got = join_stream(streams, stats, [int(st[s]) for _, st, _ in triples], at)
        out.append(got)
        at += len(got)
    nbytes = np.array([len(p) for p in out], dtype=np.int64)
    starts = (np.cumsum(nbytes) - nbytes).astype(np.int64)
    return np.frombuffer(b"".join(out), dtype=np.uint8).copy(), starts, nbytes


# ---- the corpus the CPU model test and the GPU test share -----------------------------------------------------------------
LEVELS = (1, 5)


def aligned_cuts(level):
    """Positions the edge rows (5 B + 7 samples) are cut at, every part but the last a whole number of blocks."""
    B = W.block_size(level)
    return [(B,), (4 * B,), (5 * B,), (2 * B, 5 * B), (B, 2 * B, 3 * B, 4 * B, 5 * B)]


def unaligned_cuts(level):
    """Cuts with a part, other than the last, that ends inside a frame: first, in the middle, behind an aligned part."""
    B = W.block_size(level)
    return [(1,), (B - 1,), (B + 1,), (B, 2 * B + 5), (B + 5, 2 * B), (5 * B + 6,)]


def pieces(x, cuts):
    return [np.ascontiguousarray(p) for p in np.split(x, list(cuts), axis=-1)]


NUMBER_B = 1152
NUMBER_CUTS = [(f0 * NUMBER_B,) for f0 in W.NUMBER_F0] + [(127 * NUMBER_B, 1922 * NUMBER_B)]
