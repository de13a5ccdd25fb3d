"""Builders, damage sites and the expectation model of the frame CRC-16 tests (tests/test_verify_corpus.py checks their
preconditions on the CPU against tests/golden/pyflac.py, tests/test_gpu_verify_matrix.py runs them on the GPU).  Nothing
here calls the library or the GPU; the stores named own* are the CPU encoder's (oracle/), which the device encoder
matches byte for byte.

A damage site is one byte of one frame XORed with a mask, and only two kinds exist, so that the parse never changes and
every failure is the CRC-16 check's own:
  footer   one of the frame's two CRC-16 bytes: unchecked, the store decodes to the original array;
  payload  a byte of a 32-bit VERBATIM sample of channel 0 (mono, or a left/right frame): unchecked, the store decodes to
           the original array with that one sample XORed by a known value.
The rule: with the check on, a call fails if and only if a sample range it reads, on a stream it reads, intersects
[f B, min((f + 1) B, n)) of the damaged frame (s, f); in every other case it returns what the intact store returns."""
import hashlib
from collections import namedtuple
from functools import lru_cache

import numpy as np

from tests import compare_corpus as C
from tests.conftest import full_range_i32, sinusoid_noise_i32, strip_seektable
from tests.golden import make_golden as G
from tests.golden.flac_writer import _seek_point

# start: the frame's first byte in the blob; nbytes: its length, CRC-16 included; payload: offset inside the frame of the
# first byte of channel 0's VERBATIM samples, or None where the frame offers no payload site; m: its samples
Frame = namedtuple("Frame", "start nbytes payload m")
Store = namedtuple("Store", "name blob starts nbytes data n block channels frames")
# offset: the damaged byte inside the frame; sample / value: data[stream, sample] (as unsigned) ^= value when unchecked
Site = namedtuple("Site", "stream frame offset mask kind sample value")

MASKS = (0x01, 0x80, 0x10, 0x04, 0x40, 0x02)
SR_VALUE = {12: 44, 13: 44100, 14: 4410}
M1 = ("m1_foreign64", "m1_own4096", "m1_own1152", "m1_own1152_stripped")
M2 = ("m2_foreign64", "m2_own1152")
M3 = ("m3_mixed",)
M4 = ("m4_coded",)
STORES = M1 + M2 + M3 + M4
MIXED_BLOCKS = (192, 1000, 4096, 4608)
ASSIGNMENTS = (1, 8, 9, 10)


# ---------------------------------------------------------------------------------------------------------- frames

def verbatim_frame(x, frame_no=0, sr_code=9, bs_code=None):
    """One mono frame of 32-bit VERBATIM samples."""
    bits = "00000010" + "".join(format(int(v) & 0xFFFFFFFF, "032b") for v in x)
    return G.frame([0] * len(x), frame_no, 32, {"bits": bits}, sr_code=sr_code, sr_value=SR_VALUE.get(sr_code, 0), force_bs_code=bs_code)


def constant_frame(v, m, frame_no, sr_code=9, bs_code=None):
    return G.frame([v] * m, frame_no, 32, {"type": "const"}, sr_code=sr_code, sr_value=SR_VALUE.get(sr_code, 0), force_bs_code=bs_code)


def stereo_frame(left, right, frame_no, assignment):
    """One two-channel frame, both subframes VERBATIM (a side channel with 33 bits per sample)."""
    left, right = [int(v) for v in left], [int(v) for v in right]
    side = [a - b for a, b in zip(left, right)]
    mid = [(a + b) >> 1 for a, b in zip(left, right)]
    pair = {1: (left, right), 8: (left, side), 9: (side, right), 10: (mid, side)}[assignment]
    return G.frame(list(pair), frame_no, 32, [{"type": "verbatim"}] * 2, assignment=assignment)


def pcm_md5(row):
    """libFLAC's signature of a stream of 32-bit samples: int32 as '<i4'; int64 = right << 32 | left as '<i8'."""
    row = np.asarray(row)
    return hashlib.md5(row.astype("<i4" if row.dtype == np.int32 else "<i8").tobytes()).digest()


def assemble(frames, block, n, channels, row, seektable=False):
    """The frames as one signed stream (STREAMINFO, optionally a SEEKTABLE of one point per frame); returns (bytes,
    offset of the first frame)."""
    extra = []
    if seektable:
        at = np.concatenate([[0], np.cumsum([len(f) for f in frames])[:-1]]).astype(np.int64).tolist()
        extra = [(3, b"".join(_seek_point(f * block, at[f], min(block, n - f * block)) for f in range(len(frames))))]
    sizes = [len(f) for f in frames]
    data = G.stream(frames, block, 32, n, extra_blocks=extra, channels=channels, frame_sizes=(min(sizes), max(sizes)), md5=pcm_md5(row))
    return data, len(data) - sum(sizes)


def payload_offset(seg, at, channels):
    """Offset inside the frame at seg[at:] of channel 0's first VERBATIM sample byte, or None: mono frames whose subframe
    is VERBATIM without wasted bits, two-channel frames coded left/right whose first subframe is."""
    hb = C._header_bytes(seg, at)
    if seg[at + hb] != 0x02 or (channels == 2 and seg[at + 3] >> 4 != 1):
        return None
    return hb + 1


def _store(name, streams, first_frames, frame_sizes, data, block, channels):
    """streams: bytes per stream; first_frames[s]: offset of frame 0 in stream s; frame_sizes[s]: its frames' lengths."""
    nb = np.array([len(s) for s in streams], dtype=np.int64)
    st = np.concatenate([[0], np.cumsum(nb)[:-1]]).astype(np.int64)
    blob = np.frombuffer(b"".join(bytes(s) for s in streams), dtype=np.uint8).copy()
    n = data.shape[1]
    frames = []
    for s in range(len(streams)):
        at = int(st[s]) + first_frames[s]
        row = []
        for f, size in enumerate(frame_sizes[s]):
            row.append(Frame(at, size, payload_offset(blob, at, channels), min(block[s], n - f * block[s])))
            at += size
        assert at == st[s] + nb[s]
        frames.append(tuple(row))
    same = len(set(block)) == 1
    return Store(name, blob, st, nb, data, n, block[0] if same else tuple(block), channels, tuple(frames))


def _own(name, blob, st, nb, data, block, channels, stripped=False):
    """A store of the encoder's: frames located through its SEEKTABLE, every stream signed on the CPU; stripped: the
    same streams without their SEEKTABLE."""
    blob = np.array(blob, dtype=np.uint8)
    st, nb = np.asarray(st, dtype=np.int64).reshape(-1), np.asarray(nb, dtype=np.int64).reshape(-1)
    streams, firsts, sizes = [], [], []
    for s in range(st.size):
        seg = blob[st[s] : st[s] + nb[s]].copy()
        seg[26:42] = np.frombuffer(pcm_md5(data[s]), dtype=np.uint8)
        at = C._frame_offsets(seg) + [seg.size]
        assert len(at) - 1 == -(-data.shape[1] // block)
        firsts.append(at[0])
        sizes.append([b - a for a, b in zip(at[:-1], at[1:])])
        streams.append(seg)
    if stripped:
        blob2, st2, nb2 = strip_seektable(*_pack(streams))
        streams = [blob2[a : a + b] for a, b in zip(st2, nb2)]
        firsts = [42] * len(streams)
    return _store(name, streams, firsts, sizes, data, [block] * len(streams), channels)


def _pack(streams):
    nb = np.array([len(s) for s in streams], dtype=np.int64)
    st = np.concatenate([[0], np.cumsum(nb)[:-1]]).astype(np.int64)
    return np.concatenate(streams), st, nb


def full_range_i64(shape, seed):
    rng = np.random.default_rng(seed)
    x = rng.integers(-(2**63), 2**63 - 1, size=shape, dtype=np.int64, endpoint=True)
    x.reshape(-1)[:2] = [-(2**63), 2**63 - 1]
    return x


def _foreign_mono(name, blocks, n, seed, seektable=False):
    data = full_range_i32((len(blocks), n), seed=seed)
    streams, firsts, sizes = [], [], []
    for s, b in enumerate(blocks):
        fr = [verbatim_frame(data[s, a : a + b], f, sr_code=(9, 12, 13, 14)[(s + f) % 4]) for f, a in enumerate(range(0, n, b))]
        d, first = assemble(fr, b, n, 1, data[s], seektable=seektable)
        streams.append(d), firsts.append(first), sizes.append([len(x) for x in fr])
    return _store(name, streams, firsts, sizes, data, list(blocks), 1)


def _foreign_stereo(name, n_stream, block, n, seed):
    data = full_range_i64((n_stream, n), seed)
    left, right = (data & 0xFFFFFFFF).astype(np.uint32).view(np.int32), (data >> 32).astype(np.int32)
    streams, firsts, sizes = [], [], []
    for s in range(n_stream):
        fr = [stereo_frame(left[s, a : a + block], right[s, a : a + block], f, ASSIGNMENTS[(s + f) % 4]) for f, a in enumerate(range(0, n, block))]
        d, first = assemble(fr, block, n, 2, data[s], seektable=(s % 2 == 1))
        streams.append(d), firsts.append(first), sizes.append([len(x) for x in fr])
    return _store(name, streams, firsts, sizes, data, [block] * n_stream, 2)


@lru_cache(maxsize=None)
def _build(name):
    from oracle import oracle as O

    O.lib()
    if name == "m1_foreign64":
        return _foreign_mono(name, [64] * 5, 8 * 64 + 7, seed=701)
    if name in ("m1_own4096", "m1_own1152", "m1_own1152_stripped"):
        level, block = (5, 4096) if name == "m1_own4096" else (1, 1152)
        data = full_range_i32((5, 8 * block + 7), seed=702 + level)
        return _own(name, *O.encode_i32(data, level), data, block, 1, stripped=name.endswith("stripped"))
    if name == "m2_foreign64":
        return _foreign_stereo(name, 3, 64, 4 * 64 + 7, seed=711)
    if name == "m2_own1152":
        data = full_range_i64((3, 4 * 1152 + 7), seed=712)
        return _own(name, *O.encode_i64(data, 1), data, 1152, 2)
    if name == "m3_mixed":
        # (two streams of the first class: the regrouped call of that class has streams on both sides of the damaged one)
        return _foreign_mono(name, MIXED_BLOCKS[:1] + MIXED_BLOCKS, 2 * 4608 + 5, seed=721)
    if name == "m4_coded":
        data = sinusoid_noise_i32(5, 8 * 4096 + 7, seed=731)
        return _own(name, *O.encode_i32(data, 5), data, 4096, 1)
    raise KeyError(name)


def build_store(name):
    return _build(name)


def block_of(store, s):
    return store.block[s] if isinstance(store.block, tuple) else store.block


# ------------------------------------------------------------------------------------------------------------ sites

def frame_span(store, s, f):
    b = block_of(store, s)
    return f * b, min((f + 1) * b, store.n)


def footer_site(store, s, f, which, mask):
    fr = store.frames[s][f]
    return Site(s, f, fr.nbytes - 2 + which, mask, "footer", None, 0)


def payload_site(store, s, f, i, k, mask):
    """Byte k (0 = most significant) of local sample i of frame (s, f)."""
    fr = store.frames[s][f]
    assert fr.payload is not None and 0 <= i < fr.m and 0 <= k < 4
    return Site(s, f, fr.payload + 4 * i + k, mask, "payload", frame_span(store, s, f)[0] + i, mask << (8 * (3 - k)))


def site_streams(store):
    ns = len(store.frames)
    return sorted({0, ns // 2, ns - 1})


@lru_cache(maxsize=None)
def _sites(name):
    """Every frame -- first, last and all between -- of the first, a middle and the last stream (m3: of every stream, the
    first, a middle and the last frame): a footer site and, where the frame has one, a payload site; the byte, the sample
    and the mask rotate."""
    store = build_store(name)
    out = []
    for s in (range(len(store.frames)) if name in M3 else site_streams(store)):
        nf = len(store.frames[s])
        for f in (sorted({0, nf // 2, nf - 1}) if name in M3 else range(nf)):
            r = s + f
            out.append(footer_site(store, s, f, r % 2, MASKS[r % len(MASKS)]))
            fr = store.frames[s][f]
            if fr.payload is not None:
                out.append(payload_site(store, s, f, (0, fr.m - 1, fr.m // 2)[r % 3], r % 4, MASKS[(r + 1) % len(MASKS)]))
    return tuple(out)


def sites(name):
    return _sites(name)


def byte_of(store, site):
    """The damaged byte's index in the blob."""
    return store.frames[site.stream][site.frame].start + site.offset


def damage(blob, store, site):
    out = np.array(blob, dtype=np.uint8)
    out[byte_of(store, site)] ^= site.mask
    return out


def restamp(blob, store, site):
    """`blob` with the CRC-16 of the site's frame recomputed over the frame's bytes as they are."""
    fr = store.frames[site.stream][site.frame]
    out = np.array(blob, dtype=np.uint8)
    out[fr.start + fr.nbytes - 2 : fr.start + fr.nbytes] = list(G.crc16(bytes(out[fr.start : fr.start + fr.nbytes - 2])).to_bytes(2, "big"))
    return out


# -------------------------------------------------------------------------------------------------------- the model

def unchecked(store, site):
    """What the damaged store decodes to with the check off."""
    if site.sample is None:
        return store.data
    out = store.data.copy()
    u = out.view(np.uint32 if out.dtype == np.int32 else np.uint64)
    u[site.stream, site.sample] ^= u.dtype.type(site.value)
    return out


def raises(store, site, first=0, last=None, streams=None):
    """Does a checked read of samples [first, last) of `streams` (default: all) fail?"""
    lo, hi = frame_span(store, site.stream, site.frame)
    last = store.n if last is None else last
    return (streams is None or site.stream in list(streams)) and first < hi and last > lo


def slices_raise(store, site, slices):
    return any(raises(store, site, fst, fst + cnt, [s]) for s, fst, cnt in slices)


def ranges(store, site):
    """The sample ranges of the matrix: everything, the damaged frame's first sample, its last one, everything in front
    of it and everything behind it (where there is something)."""
    lo, hi = frame_span(store, site.stream, site.frame)
    out = [(0, store.n), (lo, lo + 1), (hi - 1, hi)]
    if lo > 0:
        out.append((0, lo))
    if hi < store.n:
        out.append((hi, store.n))
    return out


def slice_lists(store, site):
    """(touching, missing): slices of intact streams around one slice of the damaged stream that reaches the damaged
    frame by a single sample (from the front where something lies in front of it, else from behind) -- and the same
    with slices that end one sample short of it and start one sample behind it."""
    ns, n = len(store.frames), store.n
    lo, hi = frame_span(store, site.stream, site.frame)
    others = [s for s in range(ns) if s != site.stream]
    a, b = others[0], others[-1]
    touch = (site.stream, max(lo - 3, 0), lo + 1 - max(lo - 3, 0)) if lo > 0 else (site.stream, hi - 1, min(4, n - hi + 1))
    touching = [(a, 0, min(n, 5)), (b, n - min(n, 70), min(n, 70)), touch]  # (last: its frames are the call's last tasks)
    missing = [(a, max(lo - 1, 0), 2)]
    if lo > 0:
        missing.append((site.stream, max(lo - 3, 0), lo - max(lo - 3, 0)))
    if hi < n:
        missing.append((site.stream, hi, min(4, n - hi)))
    missing.append((b, 0, n))
    return touching, missing


def gather(data, slices):
    return np.concatenate([data[s, f : f + c] for s, f, c in slices])


def reduce_model(x, first=0, last=None):
    """One bin over [first, last) of every row: (min, max, sum, sumsq_hi, sumsq_lo) as int64 [rows, 1]; the sum wraps as
    int64 does, the limbs (None for int64 rows) are the sums of x*x >> 32 and of x*x mod 2^32."""
    seg = np.asarray(x)[:, first:last].astype(np.int64)
    col = lambda a: np.asarray(a).reshape(-1, 1)  # noqa: E731
    mn, mx, sm = col(seg.min(axis=1)), col(seg.max(axis=1)), col(seg.sum(axis=1, dtype=np.int64))
    if np.asarray(x).dtype == np.int64:
        return mn, mx, sm, None, None
    q = (seg * seg).astype(np.uint64)
    return mn, mx, sm, col((q >> np.uint64(32)).sum(axis=1).view(np.int64)), col((q & np.uint64(0xFFFFFFFF)).sum(axis=1).view(np.int64))


def md5_status(store, site):
    """check_md5_device's status of the damaged store with the frame check off: the signature notices a changed sample."""
    out = np.ones(len(store.frames), dtype=np.int8)
    if site.sample is not None:
        out[site.stream] = 0
    return out


def float_params(store):
    """Per-stream offsets and gains of the restoring decoders: neighbouring rows differ in both."""
    r = np.arange(len(store.frames))
    dt = np.float32 if store.channels == 1 else np.float64
    return ((r % 7) * 0.25).astype(dt), (64.0 * (1 + r % 3)).astype(dt)


def isolated_frame_stream(store, site, blob):
    """For the reference decoder, whose cost is per bit: a stream of f + 1 frames with the block size of the site's
    stream -- f CONSTANT frames numbered 0..f-1, then the site's frame as `blob` holds it.  Returns (bytes, samples in
    front of the frame)."""
    s, f = site.stream, site.frame
    fr = store.frames[s][f]
    b = block_of(store, s)
    if store.channels == 1:
        front = [constant_frame(0, b, k) for k in range(f)]
    else:
        front = [G.frame([[0] * b, [0] * b], k, 32, [{"type": "const"}] * 2, assignment=1) for k in range(f)]
    body = bytes(blob[fr.start : fr.start + fr.nbytes])
    return G.stream(front + [body], b, 32, f * b + fr.m, channels=store.channels), f * b


def as_rows(samples, channels):
    """The reference decoder's sample list (interleaved left, right for two channels) as the int32 / int64 row it stands for."""
    if channels == 1:
        return np.array(samples, dtype=np.int64).astype(np.int32)
    a = np.array(samples, dtype=np.int64).reshape(-1, 2)
    return (a[:, 1] << 32) | (a[:, 0] & 0xFFFFFFFF)


# ---------------------------------------------------------------------------------- the beside path (16388 tasks)

BESIDE_BLOCK = 16
BESIDE = (4, 4097)  # streams, frames: 16388 tasks, beside the throughput decoder
BESIDE_ODD = (3, 5462)  # 16386 tasks: the check's last workgroup of four frames is half empty
AFTER = (3, 5461)  # 16383 tasks: one short of it


@lru_cache(maxsize=None)
def beside_store(n_stream, frames):
    """Streams of `frames` frames of 16 small samples, CONSTANT or VERBATIM (flac_writer's cheap frames), no SEEKTABLE."""
    from tests.golden import flac_writer as W

    rng = np.random.default_rng(741)
    n = frames * BESIDE_BLOCK
    made = [W.write_stream(rng, n, BESIDE_BLOCK, layout="libflac", cheap=True) for _ in range(n_stream)]
    streams, firsts, sizes = [], [], []
    for _, d, _ in made:
        seg = np.frombuffer(d, dtype=np.uint8)
        first = 4
        while True:
            last, ln = seg[first] >> 7, int.from_bytes(bytes(seg[first + 1 : first + 4]), "big")
            first += 4 + ln
            if last:
                break
        at, lens = first, []
        for _f in range(frames):  # a cheap frame is CONSTANT or VERBATIM: its header gives its length
            hb = C._header_bytes(seg, at)
            lens.append(hb + 1 + (4 if seg[at + hb] == 0x00 else 4 * BESIDE_BLOCK) + 2)
            at += lens[-1]
        assert at == len(d)
        streams.append(d), firsts.append(first), sizes.append(lens)
    return _store("beside_%dx%d" % (n_stream, frames), streams, firsts, sizes, np.stack([m[0] for m in made]), [BESIDE_BLOCK] * n_stream, 1)


def beside_tasks(n_stream, frames):
    """The dense tasks whose frames are damaged in turn: the first, the last below 16384, every one from 16384 on and one
    in the middle; of the other stores the last ones."""
    total = n_stream * frames
    if (n_stream, frames) == BESIDE:
        return (0, 16383, 16384, 16385, 16386, 16387, 8000)
    return tuple(range(16384, total)) if total > 16384 else (total - 1,)


def task_site(store, task):
    """The footer site of dense task `task` = (stream task // frames, frame task % frames) of a whole decode."""
    nf = len(store.frames[0])
    return footer_site(store, task // nf, task % nf, task % 2, MASKS[task % len(MASKS)])


# ------------------------------------------------------------------------- frames of every length and placement

# bs: samples; no: the frame's number (the stream has `no` CONSTANT frames in front of it); L: bytes under the CRC-16
Spec = namedtuple("Spec", "L bs no sr_code bs_code")
TRIP = 2048  # bytes of a frame the check folds per trip of its unrolled loop; 256-byte stripes of 64 lanes x 4 bytes
EDGE_GROUPS = ((2040, 2056), (2296, 2312), (4088, 4104), (6136, 6152))
SMALL_TOP = 600
NUMBER_OF = {1: 0, 2: 128, 3: 2048}  # the first frame number of every width in bytes
LANES = (0, 1, 31, 32, 63)


def _spec_for(L, widths=(1, 2, 3), rotate=0):
    """A header shape that gives a frame of L bytes under its CRC: 4 fixed bytes, the frame number, the block size in one
    byte (code 6, up to 256 samples) or two (code 7), the sample rate in none, one or two (codes 9, 12, 13 / 14), the
    CRC-8, the subframe's header, 4 bytes per sample."""
    cands = []
    for u in widths:
        shapes = [(bx, sc) for bx in (1, 2) for sc in (9, 12, 13, 14)]
        shapes = shapes[rotate % len(shapes) :] + shapes[: rotate % len(shapes)]
        for bx, sc in shapes:
            rem = L - (4 + u + bx + {9: 0, 12: 1, 13: 2, 14: 2}[sc] + 1 + 1)
            if rem > 0 and rem % 4 == 0 and (bx == 2 or rem // 4 <= 256) and rem // 4 <= 65535:
                cands.append(Spec(L, rem // 4, NUMBER_OF[u], sc, 5 + bx))
        if cands:
            return cands[0]
    return None


def smallest_L():
    return min(L for L in range(1, 64) if _spec_for(L))


@lru_cache(maxsize=None)
def length_specs():
    """One frame for every L from the smallest one up to SMALL_TOP and in every edge group (the header shape rotates with
    L; the numbers of two and three bytes come in where a length needs them), a few more with such numbers, and frames
    of 4096, 16384 and 65535 samples."""
    want = list(range(smallest_L(), SMALL_TOP + 1)) + [L for a, b in EDGE_GROUPS for L in range(a, b + 1)]
    out = [_spec_for(L, rotate=L // 4) for L in want]
    assert all(out)
    out += [_spec_for(L, widths=(2,)) for L in (13, 14, 15, 16, 257, 2050)] + [_spec_for(L, widths=(3,)) for L in (14, 15, 16, 17, 2051)]
    out += [Spec(4 + 1 + 2 + 0 + 1 + 1 + 4 * bs, bs, 0, 9, 7) for bs in (4096, 16384, 65535)]
    return tuple(out)


PLACEMENT_L = tuple(list(range(12, 20)) + list(range(300, 304)) + list(range(2041, 2056)) + list(range(2148, 2152))
                    + list(range(3048, 3052)) + list(range(4093, 4101)))


def placement_specs():
    """The frames that are also decoded as the last bytes of their blob, at every byte alignment of the blob: every
    L mod 4 below 8, below 256 and below 2048 bytes past a trip edge (and just in front of one), tiny and middling."""
    return tuple(_spec_for(L, rotate=L // 4) for L in PLACEMENT_L)  # (a multiple of 4 above 1035 takes a two-byte frame number)


LengthStore = namedtuple("LengthStore", "store specs")


@lru_cache(maxsize=None)
def _spec_frames(sp):
    rng = np.random.default_rng(10_000 + sp.L + 7 * sp.no)
    x = rng.integers(-(2**31), 2**31 - 1, sp.bs, dtype=np.int64, endpoint=True).astype(np.int32)
    front = [constant_frame(k % 5 - 2, sp.bs, k, sp.sr_code, sp.bs_code) for k in range(sp.no)]
    fr = verbatim_frame(x, sp.no, sp.sr_code, sp.bs_code)
    assert len(fr) - 2 == sp.L, (sp, len(fr))
    row = np.concatenate([np.repeat(np.arange(sp.no, dtype=np.int32) % 5 - 2, sp.bs), x]).astype(np.int32)
    return front + [fr], row


def length_store(specs, pad=16):
    """The frames of `specs` (one block size, one frame number) as the last frames of one stream each, `pad` zero bytes
    behind the last stream."""
    sp0 = specs[0]
    assert all((sp.bs, sp.no) == (sp0.bs, sp0.no) for sp in specs)
    n = (sp0.no + 1) * sp0.bs
    streams, firsts, sizes, rows = [], [], [], []
    for sp in specs:
        frames, row = _spec_frames(sp)
        d, first = assemble(frames, sp.bs, n, 1, row)
        streams.append(d), firsts.append(first), sizes.append([len(f) for f in frames]), rows.append(row)
    st = _store("len_%d_%d" % (sp0.bs, sp0.no), streams, firsts, sizes, np.stack(rows), [sp0.bs] * len(specs), 1)
    if pad:
        st = st._replace(blob=np.concatenate([st.blob, np.zeros(pad, dtype=np.uint8)]))
    return LengthStore(st, tuple(specs))


@lru_cache(maxsize=None)
def length_stores():
    """length_specs() grouped by stream length: one store per (block size, frame number), one stream per frame."""
    groups = {}
    for sp in length_specs():
        groups.setdefault((sp.bs, sp.no), []).append(sp)
    return tuple(length_store(tuple(g)) for _, g in sorted(groups.items()))


def length_sites(store, s):
    """(label, site) of the last frame of stream s: the first payload byte, a payload byte of every lane of LANES that
    has one (lane = byte offset mod 256 over 4: in the last stripe the frame has for it, and in the first), the last
    payload byte, both footer bytes."""
    f = len(store.frames[s]) - 1
    fr = store.frames[s][f]
    L, p0 = fr.nbytes - 2, fr.payload
    at = lambda o, mask: payload_site(store, s, f, (o - p0) // 4, (o - p0) % 4, mask)  # noqa: E731
    out = [("first payload byte", at(p0, 0x80))]
    for lane in LANES:
        words = [[o for o in range(w, min(w + 4, L)) if o >= p0] for w in range(4 * lane, L, 256)]  # the lane's payload bytes
        offs = [w[(lane + L) % len(w)] for w in words if w]
        for o in sorted({offs[0], offs[-1]} if offs else ()):
            out.append(("lane %d" % lane, at(o, MASKS[(lane + o // 256) % len(MASKS)])))
    out.append(("last payload byte", at(L - 1, 0x01)))
    out += [("footer byte %d" % w, footer_site(store, s, f, w, (0x80, 0x01)[w])) for w in (0, 1)]
    return out


def header_site(store, s):
    """The first byte of the last frame of stream s (its sync code: the parse fails with it, checked or not)."""
    f = len(store.frames[s]) - 1
    return Site(s, f, 0, 0x01, "header", None, 0)
