"""Plain-Python model of FlacArray.overwrite's splice: the specification the HIP splice kernel (K11) follows.

Given the streams of an array `x` (every stream with this encoder's layout: "fLaC", STREAMINFO, a SEEKTABLE of one point
per frame, frames) and, for the streams that take part, the streams of the patched span -- samples [f0 B, min(f1 B, N)) of
`y`, where y is x with y[streams, first:first+n] replaced, f0 = first // B and f1 = min(F, ceil((first + n) / B)) -- `splice`
writes the streams a one-shot encode of `y` writes, byte for byte:
  - the 46 fixed header bytes with a zero MD5;
  - the seek points < f0 verbatim, the points of the span's frames new, the points >= f1 with their offset moved by delta,
    the change in the bytes of frames f0 .. f1 - 1;
  - the frames < f0 verbatim, the frames of the span's encode renumbered k -> f0 + k (append_model.renumber_frame), the
    frames >= f1 verbatim.
A stream that does not take part is returned as it is, its STREAMINFO MD5 included.  Nothing here calls the library.
"""
import numpy as np

from tests.append_model import parse_stream, renumber_frame, stream_header, utf8_len_sum


def span_frames(stream_size, block, first, n):
    """(f0, f1): the frames that overlap samples [first, first + n)."""
    nf = -(-stream_size // block)
    return first // block, min(nf, -(-(first + n) // block))


def span_samples(stream_size, block, first, n):
    """(lo, hi): the samples of the frames that overlap [first, first + n)."""
    f0, f1 = span_frames(stream_size, block, first, n)
    return f0 * block, min(f1 * block, stream_size)


def growth(base, k):
    """Extra header bytes of frames [0, k) once renumbered to [base, base + k): the closed form the kernels use."""
    return utf8_len_sum(base + k) - utf8_len_sum(base) - utf8_len_sum(k)


def move_seek_points(points, delta):
    """The 18-byte seek points `points` (bytes) with every offset field moved by delta; sample numbers and counts kept."""
    points = bytes(points)
    out = b""
    for k in range(len(points) // 18):
        pt = points[18 * k : 18 * k + 18]
        out += pt[:8] + (int.from_bytes(pt[8:16], "big") + delta).to_bytes(8, "big") + pt[16:]
    return out


def splice_stream(old, new, first, n):
    """One stream that takes part: `old` encodes x, `new` encodes the patched span of y."""
    old, new = bytes(old), bytes(new)
    B, nch, total, pts_old, hb = parse_stream(old)
    B2, nch2, span_len, pts_new, hb_new = parse_stream(new)
    if (B2, nch2) != (B, nch):
        raise ValueError("the two streams differ in block size or channels")
    if n <= 0 or first < 0 or first + n > total:
        raise ValueError("the range does not lie inside the stream")
    nf = len(pts_old)
    f0, f1 = span_frames(total, B, first, n)
    lo, hi = span_samples(total, B, first, n)
    if len(pts_new) != f1 - f0 or span_len != hi - lo:
        raise ValueError("the second stream is not an encode of the span")
    body = len(old) - hb
    off0 = pts_old[f0][0]
    off1 = pts_old[f1][0] if f1 < nf else body
    if not 0 <= off0 <= off1 <= body:
        raise ValueError("the old stream's seek offsets are not ordered inside its body")
    body_new = len(new) - hb_new
    frames = []
    for k, (off, _) in enumerate(pts_new):
        end = pts_new[k + 1][0] if k + 1 < len(pts_new) else body_new
        frames.append(renumber_frame(new[hb_new + off : hb_new + end], f0 + k))
    mid = b"".join(frames)
    if len(mid) != body_new + growth(f0, f1 - f0):
        raise AssertionError("closed form of the header growth")
    delta = len(mid) - (off1 - off0)
    head = stream_header(B, nch, total, [])[:42] + old[42:46]  # (zero MD5; the SEEKTABLE block header does not change)
    points = old[46 : 46 + 18 * f0]
    off = off0
    for k, fr in enumerate(frames):
        if off != off0 + pts_new[k][0] + growth(f0, k):
            raise AssertionError("closed form of a new seek offset")
        points += ((f0 + k) * B).to_bytes(8, "big") + off.to_bytes(8, "big") + pts_new[k][1].to_bytes(2, "big")
        off += len(fr)
    points += move_seek_points(old[46 + 18 * f1 : hb], delta)
    return head + points + old[hb : hb + off0] + mid + old[hb + off1 :]


def splice(old_triple, new_triple, first, n, streams=None):
    """Every stream of the old triple (blob, starts, nbytes), the rows of the new triple laid into streams `streams` (flat
    indices, row j of the new triple for streams[j]; None: all) -> the triple of the patched array."""
    (ob, ost, onb), (nb_, nst, nnb) = old_triple, new_triple
    ob, nb_ = np.asarray(ob, np.uint8), np.asarray(nb_, np.uint8)
    ost, onb, nst, nnb = (np.ravel(v) for v in (ost, onb, nst, nnb))
    streams = list(range(len(ost))) if streams is None else [int(s) for s in streams]
    if len(set(streams)) != len(streams) or any(s < 0 or s >= len(ost) for s in streams) or len(streams) != len(nst):
        raise ValueError("streams: indices out of range, named twice, or not one per row of the new triple")
    row = {s: j for j, s in enumerate(streams)}
    parts = []
    for s, (s0, n0) in enumerate(zip(ost, onb)):
        old = ob[s0 : s0 + n0].tobytes()
        if s in row:
            j = row[s]
            parts.append(splice_stream(old, nb_[nst[j] : nst[j] + nnb[j]].tobytes(), first, n))
        else:
            parts.append(old)
    nbytes = np.array([len(p) for p in parts], dtype=np.int64)
    starts = np.concatenate([[0], np.cumsum(nbytes)[:-1]]).astype(np.int64)
    return np.frombuffer(b"".join(parts), dtype=np.uint8).copy(), starts, nbytes


def patched(x, first, data, streams=None):
    """y: a copy of x (n_stream, N) with y[streams, first:first+n] = data."""
    y = np.array(x, copy=True)
    rows = slice(None) if streams is None else np.asarray(streams, dtype=np.int64)
    y[rows, first : first + np.shape(data)[-1]] = data
    return y


def overwrite(old_triple, x, first, data, streams, level, encode):
    """The model's store after overwriting: `encode(array, level)` is the encoder of the patched span (the oracle's)."""
    B = 1152 if level <= 2 else 4096
    y = patched(x, first, data, streams)
    lo, hi = span_samples(x.shape[-1], B, first, np.shape(data)[-1])
    rows = slice(None) if streams is None else np.asarray(streams, dtype=np.int64)
    return splice(old_triple, encode(np.ascontiguousarray(y[rows, lo:hi]), level), first, np.shape(data)[-1], streams)


# ---- the geometry cases of the issue: name -> (first, n) for streams of N samples in blocks of B (N >= 4 B) ------------
def geometry_cases(B, N):
    last = (N - 1) // B * B  # first sample of the last frame
    return {
        "inside_first_frame": (17, 100),
        "inside_middle_frame": (2 * B + 300, 411),
        "inside_last_frame": (last + 3, min(20, N - last - 3)),
        "across_one_boundary": (2 * B - 50, 121),
        "starts_on_boundary": (2 * B, 77),
        "ends_on_boundary": (2 * B + 100, B - 100),
        "whole_stream": (0, N),
        "one_sample": (B + 5, 1),
        "ends_at_stream_end": (3 * B - 9, N - (3 * B - 9)),
    }
