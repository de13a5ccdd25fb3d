"""Plain-Python model of FlacArray.append's splice: the specification the HIP splice kernel follows.

Given the streams of an array `a` (every stream with this encoder's layout: "fLaC", STREAMINFO, a SEEKTABLE of one point
per frame, frames) and the streams of `tail(a) + b` (the short last frame of `a`, if any, followed by the new samples),
`splice` writes the streams that a one-shot encode of `concat(a, b)` writes, byte for byte:
  - a new stream header: STREAMINFO total samples and the SEEKTABLE for base + F' frames (base = the kept frames of a);
  - the kept frames of `a`, verbatim;
  - the frames of the second encode with frame number k -> k + base: the UTF-8 number, the header CRC-8 and the frame
    CRC-16 change, the CRC-16 through the linear combine identity (no pass over the frame's payload).
Nothing here calls the library.
"""
import numpy as np

CRC16_POLY = 0x8005


def crc8(data, crc=0):
    for v in bytes(data):
        crc ^= v
        for _ in range(8):
            crc = ((crc << 1) ^ 0x07) & 0xFF if crc & 0x80 else (crc << 1) & 0xFF
    return crc


def crc16(data, crc=0):
    for v in bytes(data):
        crc ^= v << 8
        for _ in range(8):
            crc = ((crc << 1) ^ CRC16_POLY) & 0xFFFF if crc & 0x8000 else (crc << 1) & 0xFFFF
    return crc


def crc16_mulmod(a, b):
    """a * b mod G (G = x^16 + 0x8005) for 16-bit polynomials a, b."""
    p = 0
    for i in range(16):
        if (b >> i) & 1:
            p ^= a << i
    for i in range(31, 15, -1):
        if (p >> i) & 1:
            p ^= (0x10000 | CRC16_POLY) << (i - 16)
    return p


def crc16_xpow8(nbytes):
    """x^(8 * nbytes) mod G by square-and-multiply: O(log nbytes) products."""
    r, base, e = 1, crc16_mulmod(1 << 8, 1), int(nbytes)  # base = x^8
    while e:
        if e & 1:
            r = crc16_mulmod(r, base)
        base = crc16_mulmod(base, base)
        e >>= 1
    return r


def crc16_combine(crc_h, crc_p, len_p):
    """crc16(H + P) from crc16(H), crc16(P) and len(P): zero init, no final xor, so crc(H||P) = crc(H) x^(8|P|) + crc(P)."""
    return crc16_mulmod(crc_h, crc16_xpow8(len_p)) ^ crc_p


def utf8_number(v):
    """The frame number as FLAC's extended UTF-8 (RFC 9639 9.1.5), up to 36 bits."""
    v = int(v)
    if v < 0x80:
        return bytes([v])
    n = 2 if v < 0x800 else 3 if v < 0x10000 else 4 if v < 0x200000 else 5 if v < 0x4000000 else 6 if v < 0x80000000 else 7
    out = [0x80 | ((v >> (6 * i)) & 0x3F) for i in range(n - 1)][::-1]
    lead = (0xFF00 >> n) & 0xFF
    return bytes([lead | (v >> (6 * (n - 1)))]) + bytes(out)


def utf8_len(v):
    return len(utf8_number(v))


def utf8_len_sum(m):
    """sum of utf8_len(v) for v in [0, m): the closed form the kernels use."""
    return sum(max(0, m - t) for t in (0, 0x80, 0x800, 0x10000, 0x200000, 0x4000000, 0x80000000))


def parse_stream(st):
    """(block size, channels, total samples, frames as a list of (offset from the first frame, samples), header bytes)
    of one stream with this encoder's layout; ValueError otherwise."""
    st = bytes(st)
    if st[:4] != b"fLaC" or st[4] != 0x00 or st[42] != 0x83:
        raise ValueError("stream lacks the SEEKTABLE this encoder writes")
    B = (st[8] << 8) | st[9]
    packed = int.from_bytes(st[18:26], "big")
    nch = ((packed >> 41) & 7) + 1
    total = packed & ((1 << 36) - 1)
    stl = int.from_bytes(st[43:46], "big")
    nf = stl // 18
    pts = [(int.from_bytes(st[46 + 18 * k + 8 : 46 + 18 * k + 16], "big"), int.from_bytes(st[46 + 18 * k + 16 : 46 + 18 * k + 18], "big")) for k in range(nf)]
    return B, nch, total, pts, 46 + stl


def frame_header_len(fr):
    """Bytes of a frame header, CRC-8 included."""
    u = 0  # leading one bits of the UTF-8 lead byte = its length (none: one byte)
    while u < 7 and fr[4] & (0x80 >> u):
        u += 1
    u = max(u, 1)
    code = fr[2] >> 4
    extra = 1 if code == 6 else 2 if code == 7 else 0
    return 4 + u + extra + 1


def renumber_frame(fr, new_number):
    """A frame with its number rewritten: new UTF-8 field, CRC-8 over the new header, CRC-16 by the combine identity."""
    fr = bytes(fr)
    h_old = frame_header_len(fr)
    u_old = h_old - 4 - 1 - {6: 1, 7: 2}.get(fr[2] >> 4, 0)
    head = fr[:4] + utf8_number(new_number) + fr[4 + u_old : h_old - 1]
    head += bytes([crc8(head)])
    len_p = len(fr) - 2 - h_old
    crc_old = (fr[-2] << 8) | fr[-1]
    crc_new = crc_old ^ crc16_mulmod(crc16(fr[:h_old]) ^ crc16(head), crc16_xpow8(len_p))
    return head + fr[h_old:-2] + bytes([crc_new >> 8, crc_new & 0xFF])


def stream_header(B, nch, total, points):
    """"fLaC" + STREAMINFO + SEEKTABLE of (sample, offset, samples) points."""
    ts = total if total < (1 << 36) else 0
    packed = (44100 << 44) | ((nch - 1) << 41) | (31 << 36) | ts
    si = B.to_bytes(2, "big") * 2 + bytes(6) + packed.to_bytes(8, "big") + bytes(16)
    stl = 18 * len(points)
    out = b"fLaC" + bytes([0, 0, 0, 34]) + si + bytes([0x83]) + stl.to_bytes(3, "big")
    for sn, off, ns in points:
        out += sn.to_bytes(8, "big") + off.to_bytes(8, "big") + ns.to_bytes(2, "big")
    return out


def splice_stream(old, new):
    """One stream: `old` encodes a, `new` encodes tail(a) + b (tail = the short last frame of a, if any)."""
    B, nch, n_old, pts_old, hb_old = parse_stream(old)
    B2, nch2, n_new, pts_new, hb_new = parse_stream(new)
    if (B2, nch2) != (B, nch):
        raise ValueError("the two streams differ in block size or channels")
    base, r = divmod(n_old, B)
    kept = pts_old[base][0] if r else len(old) - hb_old
    body_new = len(new) - hb_new
    frames = []
    for k, (off, ns) in enumerate(pts_new):
        end = pts_new[k + 1][0] if k + 1 < len(pts_new) else body_new
        frames.append(renumber_frame(new[hb_new + off : hb_new + end], k + base))
    points = [(j * B, pts_old[j][0], B) for j in range(base)]
    off = kept
    for k, fr in enumerate(frames):
        points.append(((base + k) * B, off, pts_new[k][1]))
        off += len(fr)
    return stream_header(B, nch, n_old - r + n_new, points) + bytes(old[hb_old : hb_old + kept]) + b"".join(frames)


def tail_samples(stream_size, block):
    """r: the samples of the short last frame (0 when every frame is full)."""
    return stream_size % block


def splice(old_triple, new_triple):
    """Every stream of two encoded triples (blob, starts, nbytes) -> the triple of the concatenation."""
    (ob, ost, onb), (nb_, nst, nnb) = old_triple, new_triple
    ob, nb_ = np.asarray(ob, np.uint8), np.asarray(nb_, np.uint8)
    parts = []
    for s0, n0, s1, n1 in zip(np.ravel(ost), np.ravel(onb), np.ravel(nst), np.ravel(nnb)):
        parts.append(splice_stream(ob[s0 : s0 + n0].tobytes(), nb_[s1 : s1 + n1].tobytes()))
    nbytes = np.array([len(p) for p in parts], dtype=np.int64)
    starts = np.concatenate([[0], np.cumsum(nbytes)[:-1]]).astype(np.int64)
    return np.frombuffer(b"".join(parts), dtype=np.uint8).copy(), starts, nbytes
