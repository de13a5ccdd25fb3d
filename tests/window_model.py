"""Plain-Python model of FlacArray.window's aligned route: the specification the HIP window kernel (K14) follows.

Given the streams of an array x (this encoder's layout: "fLaC", STREAMINFO, a SEEKTABLE of one point per frame, frames),
a window [first, last) with first on a frame boundary, the picked stream indices, and -- where `last` falls inside a frame
that is not the old end -- the one-frame streams an encoder writes for the samples between the last kept frame boundary
and `last`, `window` writes the streams a one-shot encode of x[idx, first:last] writes, byte for byte:
  - a new stream header: STREAMINFO total samples last - first, a SEEKTABLE rebuilt from the new frame sizes;
  - the kept frames f0 + k with frame number k: new UTF-8 number, CRC-8 and CRC-16 RECOMPUTED over the whole frame
    (not through the linear identity the kernel uses -- the model is the independent side);
  - the supplied tail frame renumbered 0 -> number of kept frames.
A window that is the whole stream returns the stream as it is.  Nothing here calls the library.

`window` also records what the copies look like (`stats`), so that a test can assert that its corpus reaches the hard
cases: (source address - destination address) mod 16 of every payload copy, taken from the blob offsets (the device
buffers are 16-byte aligned), payload lengths, VERBATIM subframes, and the bytes each header shrinks by.
"""
import numpy as np

from tests.append_model import crc8, frame_header_len, parse_stream, stream_header, utf8_number


def _crc16_table():
    tab = []
    for v in range(256):
        c = v << 8
        for _ in range(8):
            c = ((c << 1) ^ 0x8005) & 0xFFFF if c & 0x8000 else (c << 1) & 0xFFFF
        tab.append(c)
    return tab


_TAB = _crc16_table()


def crc16(data, crc=0):
    """CRC-16 (poly 0x8005, zero init, no final xor) over every byte of `data`, table driven."""
    tab = _TAB
    for v in bytes(data):
        crc = ((crc << 8) & 0xFFFF) ^ tab[(crc >> 8) ^ v]
    return crc


def renumber_whole(fr, number):
    """A frame with its number rewritten and both CRCs computed afresh.  Returns (frame, old header bytes, new header bytes)."""
    fr = bytes(fr)
    h_old = frame_header_len(fr)
    u_old = h_old - 4 - 1 - {6: 1, 7: 2}.get(fr[2] >> 4, 0)
    head = fr[:4] + utf8_number(number) + fr[4 + u_old : h_old - 1]
    head += bytes([crc8(head)])
    body = head + fr[h_old:-2]
    c = crc16(body)
    return body + bytes([c >> 8, c & 0xFF]), h_old, len(head)


def new_stats():
    return {"align": set(), "min_payload": 1 << 60, "verbatim": 0, "shrink": set(), "frames": 0}


def window_stream(old, first, last, tail=None, stats=None, src_at=0, dst_at=0):
    """One stream.  `tail`: the one-frame stream of the samples in front of the cut (needed when last is inside a frame and
    not the old end).  src_at / dst_at: where the old and the new stream start in their blobs (for the statistics)."""
    old = bytes(old)
    B, nch, n_old, pts, hb_old = parse_stream(old)
    if first % B or not 0 <= first < last <= n_old:
        raise ValueError("the model covers windows that start on a frame boundary")
    if first == 0 and last == n_old:
        return old
    f0, n = first // B, last - first
    body_old = len(old) - hb_old
    nk, r = (len(pts) - f0, 0) if last == n_old else divmod(n, B)
    hb_new = 46 + 18 * (nk + (1 if r else 0))
    points, frames, off = [], [], 0

    def take(src, src_off, fr, number, count):
        nonlocal off
        new, h_old, h_new = renumber_whole(fr, number)
        if stats is not None:
            stats["align"].add((src + src_off + h_old - (dst_at + hb_new + off + h_new)) % 16)
            stats["min_payload"] = min(stats["min_payload"], len(fr) - 2 - h_old)
            stats["verbatim"] += (fr[h_old] >> 1) == 1
            stats["shrink"].add(h_old - h_new)
            stats["frames"] += 1
        points.append((number * B, off, count))
        frames.append(new)
        off += len(new)

    for k in range(nk):
        f = f0 + k
        o = pts[f][0]
        e = pts[f + 1][0] if f + 1 < len(pts) else body_old
        take(src_at, hb_old + o, old[hb_old + o : hb_old + e], k, pts[f][1])
    if r:
        tail = bytes(tail)
        B2, nch2, n2, pts2, hb2 = parse_stream(tail)
        if (B2, nch2, n2, len(pts2)) != (B, nch, r, 1):
            raise ValueError("the tail is not a one-frame encode of the samples in front of the cut")
        fr = tail[hb2:]
        new, _, _ = renumber_whole(fr, nk)
        points.append((nk * B, off, r))
        frames.append(new)
    return stream_header(B, nch, n, points) + b"".join(frames)


def window(old_triple, first, last, streams=None, tail_triple=None, stats=None):
    """(blob, starts, nbytes) of the window of the picked streams (None: all), in the order asked."""
    ob, ost, onb = old_triple
    ob = np.asarray(ob, np.uint8)
    ost, onb = np.ravel(ost), np.ravel(onb)
    idx = range(len(ost)) if streams is None else [int(s) for s in streams]
    parts, at = [], 0
    for j, s in enumerate(idx):
        tail = None
        if tail_triple is not None:
            tb, tst, tnb = tail_triple
            tail = np.asarray(tb, np.uint8)[int(np.ravel(tst)[j]) : int(np.ravel(tst)[j]) + int(np.ravel(tnb)[j])].tobytes()
        p = window_stream(ob[int(ost[s]) : int(ost[s]) + int(onb[s])].tobytes(), first, last, tail, stats, int(ost[s]), at)
        parts.append(p)
        at += len(p)
    nbytes = np.array([len(p) for p in parts], dtype=np.int64)
    starts = (np.cumsum(nbytes) - nbytes).astype(np.int64)
    return np.frombuffer(b"".join(parts), dtype=np.uint8).copy(), starts, nbytes


def tail_range(stream_size, block, first, last):
    """(lo, hi) of the samples the tail frame is encoded from, or None when no frame is re-encoded."""
    r = (last - first) % block
    if first % block or last == stream_size or r == 0:
        return None
    return last - r, last


# ---- the corpus the CPU model test and the GPU test share -----------------------------------------------------------------
def block_size(level):
    return 1152 if level <= 2 else 4096


def edge_rows(level, wide=False):
    """4 rows x (5 B + 7) samples: constant, small noise, a ramp plus noise, full-scale random.  wide: int64 (two
    channels: low and high words)."""
    B = block_size(level)
    n = 5 * B + 7
    rng = np.random.default_rng(100 + level)
    t = np.arange(n)
    rows = [np.full(n, -77), rng.integers(-3, 4, n), 11 * t + rng.integers(-50, 51, n), rng.integers(-(2**31), 2**31, n)]
    x = np.stack(rows).astype(np.int64)
    if not wide:
        return x.astype(np.int32)
    x[3] = rng.integers(-(2**63), 2**63 - 1, n)  # (the small rows stay small: a constant high word)
    x[2] = (x[2] << 33) + rng.integers(0, 1 << 20, n)
    return x


def edge_windows(level):
    """first in {0, B, 4B, 5B} x last in {first+1, first+B-1, first+B, first+B+1, size-1, size}, those that lie inside."""
    B = block_size(level)
    size = 5 * B + 7
    out = []
    for first in (0, B, 4 * B, 5 * B):
        for last in (first + 1, first + B - 1, first + B, first + B + 1, size - 1, size):
            if first < last <= size and (first, last) not in out:
                out.append((first, last))
    return out


STREAM_PICKS = ([2, 0], [3, 1, 0, 2], [3, 2, 1, 0])

NUMBER_LEVEL = 1
NUMBER_SIZE = 2050 * 1152 + 5
NUMBER_F0 = (1, 127, 128, 129, 1922, 2047, 2048, 2049)


def number_rows():
    """2 rows x (2050 * 1152 + 5) samples at level 1: frame numbers up to 2050, where the UTF-8 field is 1, 2 and 3 bytes."""
    rng = np.random.default_rng(11)
    return np.stack([np.full(NUMBER_SIZE, 5), rng.integers(-1, 2, NUMBER_SIZE)]).astype(np.int32)


def number_windows(f0):
    """For frame f0: up to the end of the stream, and once with `last` inside a frame."""
    B = 1152
    first = f0 * B
    mid = first + 2 * B + 77 if first + 2 * B + 77 < NUMBER_SIZE - 5 else first + 77
    return [(first, NUMBER_SIZE), (first, mid)]
