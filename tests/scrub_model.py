"""The damage map's status rule restated over bytes, the stores and the damage sites of its tests
(tests/test_scrub_model.py checks their preconditions on the CPU, tests/test_gpu_scrub.py runs them on the GPU).  Nothing
here calls the library or the GPU; the own* stores are the CPU encoder's (oracle/), the foreign and length stores are
assembled by hand with tests/verify_corpus.py's builders.

The rule.  B = block size, N = samples per stream, nf = ceil(N / B), nch = channels.
  A stream is located when 0 <= start, 0 <= nbytes, start + nbytes <= len(blob); it begins with "fLaC"; its metadata chain
  parses inside nbytes (every block header and body inside, a last-block flag reached); its (last) STREAMINFO of at least 34
  bytes has min == max block size == B and nch channels; its (last) SEEKTABLE has exactly nf points (length // 18).
  Frame f is located when its stream is, seek point f carries sample number f B, begin = first_frame + offset_f, end = the
  begin of frame f + 1 found the same way (stream end for the last frame), and first_frame <= begin, begin + 8 <= end,
  end <= stream end.  Otherwise its status is UNLOCATED and nothing else is looked at.
  A located frame gets HEADER when its header (the bytes [begin, min(begin + 16, end))) is not: 0xFF 0xF8; a block-size code
  other than 0, a sample-rate code other than 15, a sample-size code other than 3, a channel code valid for nch (0 for one
  channel; 1, 8, 9, 10 for two), reserved bit 0; a UTF-8 number that decodes to exactly f; a coded block size of
  min(B, N - f B); a correct CRC-8 -- all inside those bytes.  It gets CRC16 when the CRC-16 of [begin, end - 2) differs from
  the two bytes at end - 2."""
from collections import namedtuple
from functools import lru_cache

import numpy as np

from tests import compare_corpus as C
from tests import verify_corpus as V
from tests.conftest import full_range_i32, sinusoid_noise_i32
from tests.golden import make_golden as G

OK, UNLOCATED, HEADER, CRC16 = 0, 1, 2, 4


# ------------------------------------------------------------------------------------------------------ the rule

@lru_cache(maxsize=4096)
def _crc16(data):
    """G.crc16, remembered: from one damage case to the next nearly every frame keeps its bytes."""
    return G.crc16(data)


def _chain(seg):
    """(first frame offset, STREAMINFO (min, max, channels) or None, SEEKTABLE (offset, points) or None) of a stream's
    bytes, or None when "fLaC" or the metadata chain does not parse inside them."""
    nb = len(seg)
    if nb < 4 or seg[:4] != b"fLaC":
        return None
    off, info, seek = 4, None, None
    while True:
        if off + 4 > nb:
            return None
        last, typ = seg[off] >> 7, seg[off] & 0x7F
        ln = int.from_bytes(seg[off + 1 : off + 4], "big")
        off += 4
        if off + ln > nb:
            return None
        if typ == 0 and ln >= 34:
            info = (int.from_bytes(seg[off : off + 2], "big"), int.from_bytes(seg[off + 2 : off + 4], "big"), ((seg[off + 12] >> 1) & 7) + 1)
        elif typ == 3:
            seek = (off, ln // 18)
        off += ln
        if last:
            return off, info, seek


def header_ok(h, nch, f, expect_bs):
    """The frame header check over the bytes h (at most 16, no more than the frame has)."""
    if len(h) < 5 or h[0] != 0xFF or h[1] != 0xF8:
        return False
    bsc, src, ch, ssc = h[2] >> 4, h[2] & 15, h[3] >> 4, (h[3] >> 1) & 7
    if bsc == 0 or src == 15 or ssc == 3 or (h[3] & 1):
        return False
    if not (ch == 0 if nch == 1 else ch in (1, 8, 9, 10)):
        return False
    u0, extra, num = h[4], 0, h[4]
    if u0 & 0x80:
        while extra < 7 and u0 & (0x40 >> extra):
            extra += 1
        if extra == 0 or extra > 6:
            return False
        num = u0 & ((0x40 >> extra) - 1)
    n = 5 + extra + {6: 1, 7: 2}.get(bsc, 0) + (1 if src == 12 else 2 if src in (13, 14) else 0)
    if n + 1 > len(h):
        return False
    at = 5
    for _ in range(extra):
        if h[at] & 0xC0 != 0x80:
            return False
        num = (num << 6) | (h[at] & 0x3F)
        at += 1
    if num != f:
        return False
    if bsc == 1:
        bs = 192
    elif bsc <= 5:
        bs = 576 << (bsc - 2)
    elif bsc == 6:
        bs = h[at] + 1
    elif bsc == 7:
        bs = ((h[at] << 8) | h[at + 1]) + 1
    else:
        bs = 256 << (bsc - 8)
    return bs == expect_bs and G.crc8(bytes(h[:n])) == h[n]


def stream_status(blob, start, nb, n, nch, block):
    nf = -(-n // block)
    bad = np.full(nf, UNLOCATED, dtype=np.uint8)
    if start < 0 or nb < 0 or start + nb > len(blob):
        return bad
    seg = blob[start : start + nb]
    parsed = _chain(seg)
    if parsed is None:
        return bad
    first, info, seek = parsed
    if info != (block, block, nch) or seek is None or seek[1] != nf:
        return bad

    def begin(f):
        p = seek[0] + 18 * f
        if int.from_bytes(seg[p : p + 8], "big") != f * block:
            return None
        return first + int.from_bytes(seg[p + 8 : p + 16], "big")

    out = np.zeros(nf, dtype=np.uint8)
    for f in range(nf):
        b = begin(f)
        e = begin(f + 1) if f + 1 < nf else nb
        if b is None or e is None or not (first <= b and b + 8 <= e and e <= nb):
            out[f] = UNLOCATED
            continue
        if not header_ok(seg[b : min(b + 16, e)], nch, f, min(block, n - f * block)):
            out[f] |= HEADER
        if _crc16(seg[b : e - 2]) != int.from_bytes(seg[e - 2 : e], "big"):
            out[f] |= CRC16
    return out


def frame_status(blob, starts, nbytes, n, nch, block):
    """uint8 [n_stream, nf]"""
    blob = bytes(np.asarray(blob, dtype=np.uint8))
    return np.stack([stream_status(blob, int(s), int(b), n, nch, block) for s, b in zip(np.asarray(starts).reshape(-1), np.asarray(nbytes).reshape(-1))])


def salvage_model(data, status, first, last, fill, block):
    """What a salvage of samples [first, last) returns: `data` (the intact decode, [n_stream, N], any dtype) with the
    samples of every frame whose status is not 0 replaced by `fill`."""
    data = np.asarray(data)
    out = data[:, first:last].copy()
    n = data.shape[1]
    for s, f in zip(*np.nonzero(np.asarray(status).reshape(data.shape[0], -1))):
        lo, hi = max(f * block, first), min((f + 1) * block, n, last)
        if lo < hi:
            out[s, lo - first : hi - first] = fill
    return out


def naive_ranges(status, block, n):
    rows = []
    st = np.asarray(status)
    st = st.reshape(-1, st.shape[-1])
    for s in range(st.shape[0]):
        f = 0
        while f < st.shape[1]:
            if st[s, f] == 0:
                f += 1
                continue
            g = f
            while g < st.shape[1] and st[s, g] != 0:
                g += 1
            rows.append((s, f * block, min(g * block, n)))
            f = g
    return np.array(rows, dtype=np.int64).reshape(-1, 3)


# ------------------------------------------------------------------------------------------------------ the stores

STORES = ("own1152", "own4096", "own1152x2", "foreign64", "lpc4096")


@lru_cache(maxsize=None)
def build_store(name):
    """3 streams of 3 frames, the last one short (the 9 frames leave the last workgroup of four half empty); the last
    stream ends at the end of the blob."""
    from oracle import oracle as O

    O.lib()
    if name == "own1152":
        data = full_range_i32((3, 2 * 1152 + 7), seed=801)
        return V._own(name, *O.encode_i32(data, 1), data, 1152, 1)
    if name == "own4096":
        data = full_range_i32((3, 2 * 4096 + 7), seed=802)
        return V._own(name, *O.encode_i32(data, 5), data, 4096, 1)
    if name == "own1152x2":
        data = V.full_range_i64((3, 2 * 1152 + 7), seed=803)
        return V._own(name, *O.encode_i64(data, 1), data, 1152, 2)
    if name == "foreign64":
        return V._foreign_mono(name, [64] * 3, 2 * 64 + 7, seed=804, seektable=True)
    if name == "lpc4096":
        data = sinusoid_noise_i32(3, 2 * 4096 + 7, seed=805)
        return V._own(name, *O.encode_i32(data, 5), data, 4096, 1)
    raise KeyError(name)


def length_store(specs):
    """V.length_store with one seek point per frame and no padding: the frames of `specs` as the last frames of one
    stream each, the last stream ending at the end of the blob."""
    sp0 = specs[0]
    n = (sp0.no + 1) * sp0.bs
    streams, firsts, sizes, rows = [], [], [], []
    for sp in specs:
        frames, row = V._spec_frames(sp)
        d, first = V.assemble(frames, sp.bs, n, 1, row, seektable=True)
        streams.append(d), firsts.append(first), sizes.append([len(f) for f in frames]), rows.append(row)
    return V._store("scrub_len_%d_%d" % (sp0.bs, sp0.no), streams, firsts, sizes, np.stack(rows), [sp0.bs] * len(specs), 1)


@lru_cache(maxsize=None)
def length_stores():
    """Frames whose CRC-covered length lies 8 bytes on each side of every stripe and trip edge of V.EDGE_GROUPS, every
    length under V.SMALL_TOP, and the other shapes of V.length_specs(), grouped by (block size, frame number)."""
    groups = {}
    for sp in V.length_specs():
        groups.setdefault((sp.bs, sp.no), []).append(sp)
    return tuple(length_store(tuple(g)) for _, g in sorted(groups.items()))


def length_cases(store):
    """(label, blob) of a length store: every stream's last frame damaged in its first byte, its last covered byte and
    its two footer bytes in turn (all streams at once: the frames are independent)."""
    out = []
    for label, where in (("first", lambda fr: 0), ("last covered", lambda fr: fr.nbytes - 3), ("footer 0", lambda fr: fr.nbytes - 2),
                         ("footer 1", lambda fr: fr.nbytes - 1)):
        blob = store.blob.copy()
        for row in store.frames:
            blob[row[-1].start + where(row[-1])] ^= 0x10
        out.append((label, blob))
    return out


# ------------------------------------------------------------------------------------------------------- the sites

Case = namedtuple("Case", "name blob starts nbytes")


def _seek_offset(store, s):
    """Offset in the blob of the first seek point of stream s."""
    st = int(store.starts[s])
    seg = bytes(store.blob[st : st + int(store.nbytes[s])])
    return st + _chain(seg)[2][0]


def _case(store, name, edit):
    blob, starts, nbytes = store.blob.copy(), store.starts.copy(), store.nbytes.copy()
    edit(blob, starts, nbytes)
    return Case(name, blob, starts, nbytes)


def _renumber(store, s, f, restamp16):
    """Frame (s, f) with its number byte changed and the CRC-8 re-stamped (and the CRC-16 too, on request)."""
    fr = store.frames[s][f]

    def edit(blob, starts, nbytes):
        hb = C._header_bytes(blob, fr.start)
        assert hb >= 6 and blob[fr.start + 4] < 0x80  # a one-byte frame number
        blob[fr.start + 4] = (int(blob[fr.start + 4]) + 1) & 0x7F
        blob[fr.start + hb - 1] = G.crc8(bytes(blob[fr.start : fr.start + hb - 1]))
        if restamp16:
            blob[fr.start + fr.nbytes - 2 : fr.start + fr.nbytes] = list(G.crc16(bytes(blob[fr.start : fr.start + fr.nbytes - 2])).to_bytes(2, "big"))

    return edit


@lru_cache(maxsize=None)
def cases(name):
    """One case per kind of damage, deterministic, at the first, a middle and the last frame where that makes sense (the
    stream rotates with the frame)."""
    store = build_store(name)
    ns, nf = len(store.frames), len(store.frames[0])
    out = []
    xor = lambda at, mask: (lambda blob, starts, nbytes: blob.__setitem__(at, blob[at] ^ mask))  # noqa: E731
    for f in range(nf):
        s = (f + 1) % ns
        fr = store.frames[s][f]
        tag = "@ s%d f%d" % (s, f)
        out.append(_case(store, "footer " + tag, xor(fr.start + fr.nbytes - 2 + f % 2, V.MASKS[f])))
        if fr.payload is not None:
            out.append(_case(store, "payload " + tag, xor(fr.start + fr.payload + 4 * (fr.m // 2) + f % 4, V.MASKS[f + 1])))
        else:
            out.append(_case(store, "residual " + tag, xor(fr.start + (2 * fr.nbytes) // 3, V.MASKS[f + 1])))
        out.append(_case(store, "sync " + tag, xor(fr.start, 0x01)))
        out.append(_case(store, "number " + tag, _renumber(store, s, f, False)))
        out.append(_case(store, "number, CRC-16 restamped " + tag, _renumber(store, s, f, True)))
        out.append(_case(store, "crc8 " + tag, xor(fr.start + C._header_bytes(store.blob, fr.start) - 1, 0x40)))
        sp = _seek_offset(store, s) + 18 * f
        out.append(_case(store, "seek sample number " + tag, xor(sp + 7, 0x01)))
        out.append(_case(store, "seek offset inside " + tag, xor(sp + 15, 0x04)))
        out.append(_case(store, "seek offset beyond " + tag, xor(sp + 10, 0x40)))  # (+ 2^46)
    s0, smid, slast = 0, ns // 2, ns - 1
    at = lambda s, o: int(store.starts[s]) + o  # noqa: E731
    out.append(_case(store, "STREAMINFO block size @ s%d" % smid, xor(at(smid, 11), 0x01)))
    out.append(_case(store, "fLaC marker @ s%d" % s0, xor(at(s0, 0), 0x20)))
    out.append(_case(store, "STREAMINFO channels @ s%d" % slast, xor(at(slast, 20), 0x02)))
    out.append(_case(store, "negative start @ s%d" % smid, lambda blob, starts, nbytes: starts.__setitem__(smid, -5)))
    out.append(_case(store, "nbytes past the blob @ s%d" % slast, lambda blob, starts, nbytes: nbytes.__setitem__(slast, nbytes[slast] + 1)))
    out.append(_case(store, "half nbytes @ s%d" % s0, lambda blob, starts, nbytes: nbytes.__setitem__(s0, nbytes[s0] // 2)))
    a, b = store.frames[smid][0], store.frames[smid][1]
    out.append(_case(store, "zeros across f0 / f1 @ s%d" % smid, lambda blob, starts, nbytes: blob.__setitem__(slice(b.start - 24, b.start + 24), 0)))
    assert a.start + a.nbytes == b.start
    return tuple(out)


def expected(store, case):
    return frame_status(case.blob, case.starts, case.nbytes, store.n, store.channels, store.block)


def windows(store, status):
    """Sample ranges of a salvage: everything, and -- around the first damaged frame -- ranges that cut it at either
    end, lie inside it, and miss it on either side (where there is something)."""
    n, b = store.n, store.block
    out = [(0, n)]
    bad = np.argwhere(np.asarray(status) != 0)
    if bad.size:
        f = int(bad[0][1])
        lo, hi = f * b, min((f + 1) * b, n)
        out += [(max(lo - 3, 0), lo + 5), (hi - 5, min(hi + 3, n)), (lo + 1, hi - 1)]
        if lo > 0:
            out.append((0, lo))
        if hi < n:
            out.append((hi, n))
    return out
