"""Far offsets: stores whose BYTE offsets pass 2^31 and 2^32, streams whose FRAME numbers pass 2^16 and whose SAMPLE
positions pass 2^31.

Builders and arithmetic only: nothing here imports the library, the oracle or the GPU (`Kit` is handed the oracle and
the stream writer by its caller).  tests/test_far_corpus.py asserts on the CPU that every geometry crosses the threshold it names;
tests/test_gpu_far.py sends them through the device paths.

Part A -- a sparse blob.  BLOB_BYTES = 2^32 + 2^20 bytes of FILL hold the few streams of one kit at a time.  A kit is an
array of ROWS + 1 short streams of one geometry with pairwise different samples: rows 0 .. ROWS - 1 are the store, in the
order of ROLES (which is NOT the order of their addresses), the last row is a decoy that no index names.  Three layouts
put the rows at the marks M = 2^31 and 2^32:

  straddle  rows A and B start in front of M and end behind it: M lies STRADDLE_BACK bytes in front of the end of the
            stream's second frame, that is inside the residual of that frame's last subframe (see `straddle_start`)
  at        rows A and B start at M exactly
  plus3     rows A and B start at M + 3

Row Z sits at offset 0 (`plus3`: at 3), row E ends at the blob's last byte, rows H and L sit at odd addresses in between.
Decoys: every row that starts at p >= 2^32 has a valid stream of its geometry with other samples at p - 2^32 -- row Z for
row B (0 for `at`, 3 for `plus3`), the decoy row for row E.  A kernel that truncates a start to 32 bits then decodes
cleanly to the WRONG samples instead of tripping over filler.

Part B -- packed stores past 2^32 bytes: full-range noise, B_FRAMES frames of 4096 per stream, `b_stream_count` streams.

Part C -- long streams, tiny blobs: zeros with a few frames of noise (`sparse_frames`).
"""
import numpy as np

M31, M32 = 1 << 31, 1 << 32
MARKS = (M31, M32)
BLOB_BYTES = M32 + (1 << 20)
FILL = 0x5A  # (no sync code, no "fLaC": a read that lands in filler fails to parse)
LAYOUTS = ("straddle", "at", "plus3")
ROLES = ("E", "B", "Z", "A", "H", "L")  # row i of a kit plays ROLES[i]
ROWS = len(ROLES)
DECOY = ROWS  # the kit's last row
STRADDLE_BACK = 18  # M lies 16 bytes in front of the CRC-16 of the second frame
MIN_FRAME_BYTES = 600
H_AT, L_AT = M31 + (1 << 30) + 1, (1 << 30) + 5


def block_size(level):
    return 1152 if level <= 2 else 4096


# ------------------------------------------------------------------------------------------------------ Part A: kits

# name -> (dtype, level, stream size, layout of the metadata).  Every stream has three whole frames and a short fourth.
KITS = {
    "i32_l5": ("i32", 5, 3 * 4096 + 1500, "own"),
    "i32_l1": ("i32", 1, 3 * 1152 + 700, "own"),
    "i32_l5_stripped": ("i32", 5, 3 * 4096 + 1500, "stripped"),
    "i32_l1_stripped": ("i32", 1, 3 * 1152 + 700, "stripped"),
    "writer_mono": ("i32", None, 3 * 4096 + 2048, "writer"),
    "writer_stereo": ("i64", None, 3 * 1152 + 576, "writer"),
    "i64_l5": ("i64", 5, 3 * 4096 + 1500, "own"),
    "f32_l5": ("f32", 5, 3 * 4096 + 1500, "own"),
    "signed_l5": ("i32", 5, 3 * 4096 + 1500, "signed"),
}


def kit_ints(name, rows=ROWS + 1, n=None, seed=0):
    """The integers of kit `name`: a sinusoid whose period depends on the row plus 10 bits of noise (LPC frames of about
    1.5 bytes per sample); int64 kits carry 8 bits of noise in the high word as well.  Rows are pairwise different."""
    dt, _, n0, _ = KITS[name]
    n = n0 if n is None else n
    rng = np.random.default_rng([sum(name.encode()), seed])
    t = np.arange(n)[None, :]
    r = np.arange(rows)[:, None]
    x = np.rint(2.0**14 * np.sin(2 * np.pi * t / (200.0 + 37 * r)) + rng.normal(0, 2.0**10, (rows, n))).astype(np.int64)
    x[:, 0] = 1000 + r[:, 0]
    if dt == "i64":
        return ((rng.integers(-128, 128, (rows, n)) + r) << 32) + x
    return x.astype(np.int32)


def kit_floats(x, rows):
    """float32 data whose quantised integers are `x` (|x| < 2^24 times quanta that are exact in float32), and its quanta."""
    q = (2.0**-10 * (1 + np.arange(rows) % 3)).astype(np.float32)
    return (x.astype(np.float64) * q[:, None]).astype(np.float32), q


def metadata_walk(stream):
    """(offset of the first frame, frame offsets relative to it from a SEEKTABLE of real points or None) of one stream."""
    s = np.asarray(stream)
    assert bytes(s[:4]) == b"fLaC"
    off, points = 4, None
    while True:
        last, typ = s[off] >> 7, s[off] & 0x7F
        ln = (int(s[off + 1]) << 16) | (int(s[off + 2]) << 8) | int(s[off + 3])
        if typ == 3:
            body = s[off + 4 : off + 4 + ln].reshape(-1, 18)
            points = [int.from_bytes(bytes(p[8:16]), "big") for p in body if bytes(p[:8]) != b"\xff" * 8]
        off += 4 + ln
        if last:
            return off, points


def frame_spans(stream, nf):
    """[(first byte, one past the last byte)] of the nf frames of a stream with one seek point per frame."""
    first, points = metadata_walk(stream)
    assert points is not None and len(points) == nf and points[0] == 0
    ends = points[1:] + [len(stream) - first]
    return [(first + a, first + b) for a, b in zip(points, ends)]


def strip_seektable(stream):
    """One own-layout stream as libFLAC lays it out: fLaC, STREAMINFO marked last, the frames."""
    s = np.asarray(stream)
    first, _ = metadata_walk(s)
    out = np.concatenate([s[:42], s[first:]])
    out[4] = 0x80
    return out


def straddle_start(mark, second_frame_end):
    """Where a stream starts so that `mark` lies STRADDLE_BACK bytes in front of the end of its second frame.  The frame ends
    with its CRC-16, so the mark is byte 16 from the end of the residual of the frame's last subframe: that residual
    holds at least one bit per sample and the kits' frames are at least MIN_FRAME_BYTES long with LPC subframes whose
    header, warm-up and coefficients take less than 220 bytes (order <= 32, 33 bits), so the mark is far from both its ends."""
    return mark - (second_frame_end - STRADDLE_BACK)


def place(layout, nbytes, second_frame_ends):
    """The start of every row of a kit (ROWS + 1 values, the decoy's last) in the blob under `layout`."""
    nb = [int(v) for v in nbytes]
    assert len(nb) == ROWS + 1
    at = {}
    for role, mark in (("A", M31), ("B", M32)):
        i = ROLES.index(role)
        at[role] = {"straddle": straddle_start(mark, int(second_frame_ends[i])), "at": mark, "plus3": mark + 3}[layout]
    at["Z"] = 3 if layout == "plus3" else 0
    at["E"] = BLOB_BYTES - nb[ROLES.index("E")]
    at["H"], at["L"] = H_AT, L_AT
    return np.array([at[r] for r in ROLES] + [at["E"] - M32], dtype=np.int64)


class Kit:
    """Kit `name` as the tests see it: x (ROWS + 1 rows of integers; `f`, `q`, `off`, `gain` for the float kit), `streams`
    (one uint8 array per row), `second_end` (the end of every row's second frame inside its stream), `min_frame` (the shortest frame's bytes), and for a stripped
    kit `own`, the streams it was stripped from.  `oracle` is tests' CPU oracle, `writer` tests/golden/flac_writer."""

    def __init__(self, name, oracle, writer=None, md5=None):
        self.name = name
        self.dt, self.level, self.n, self.layout = KITS[name]
        self.wide = self.dt == "i64"
        self.f = self.q = self.off = self.gain = self.own = None
        if self.layout == "writer":
            nch = 2 if self.wide else 1
            self.B = 4096 if nch == 1 else 1152
            b = writer._batch(name, np.random.default_rng(11 + nch), ROWS + 1, self.n, self.B, nch, bucket_cycle=True, layout="own")
            self.x = np.asarray(b["samples"])
            self.streams = [np.frombuffer(s, dtype=np.uint8).copy() for s in b["streams"]]
        else:
            self.B = block_size(self.level)
            self.x = kit_ints(name)
            if self.dt == "f32":
                self.f, self.q = kit_floats(self.x, ROWS + 1)
                self.x, self.off, self.gain = oracle.float32_to_int32(self.f, self.q)
            enc = oracle.encode_i64 if self.wide else oracle.encode_i32
            self.streams = split(*enc(self.x, self.level))
        self.nf = -(-self.n // self.B)
        spans = [frame_spans(s, self.nf) for s in self.streams]
        self.second_end = [sp[1][1] for sp in spans]
        self.min_frame = min(b - a for sp in spans for a, b in sp)
        if self.layout == "stripped":
            self.own = self.streams
            cut = 4 + 18 * self.nf
            self.streams = [strip_seektable(s) for s in self.own]
            self.second_end = [e - cut for e in self.second_end]
        if self.layout == "signed":
            for s, row in zip(self.streams, self.x):
                s[26:42] = np.frombuffer(md5(row.tobytes()).digest(), dtype=np.uint8)
        self.nb = np.array([len(s) for s in self.streams], dtype=np.int64)
        self.compact = pack(self.streams[:ROWS])

    def starts(self, layout):
        return place(layout, self.nb, self.second_end)


def truncated(p):
    return int(p) & 0xFFFFFFFF


def pack(streams):
    """[uint8 arrays] -> (blob, starts, nbytes) back to back."""
    nb = np.array([len(s) for s in streams], dtype=np.int64)
    st = np.concatenate([[0], np.cumsum(nb)[:-1]]).astype(np.int64)
    return np.concatenate(streams), st, nb


def split(blob, starts, nbytes):
    blob = np.asarray(blob)
    return [blob[int(s) : int(s) + int(k)].copy() for s, k in zip(np.asarray(starts).reshape(-1), np.asarray(nbytes).reshape(-1))]


# ------------------------------------------------------------------------------------------- Part B: packed and large

B_FRAMES, B_BLOCK = 8, 4096
B_N = B_FRAMES * B_BLOCK
B_MIN_BLOB = M32 + (M32 >> 2)  # 1.25 * 2^32
B_MIN_OUTPUT = M32 + (1 << 26)


def b_stream_count(one_stream_bytes):
    """Streams of `one_stream_bytes` (the oracle's size of one stream of B_N samples of full-range noise) such that the blob
    exceeds 1.25 * 2^32 bytes AND every output of the tests passes B_MIN_OUTPUT -- the smallest of them is the pick of
    every second stream, so half the streams must pass it.  Two more, so that nothing ends on a bound."""
    one = int(one_stream_bytes)
    return max(-(-B_MIN_BLOB // one), 2 * -(-B_MIN_OUTPUT // one)) + 2


def spot_rows(starts, nbytes):
    """The rows the oracle encodes again: the first, the last, the row that holds each mark (straddling it, or starting at
    it) and the rows in front of and behind that one."""
    st = np.asarray(starts, dtype=np.int64).reshape(-1)
    end = st + np.asarray(nbytes, dtype=np.int64).reshape(-1)
    rows = {0, st.size - 1}
    for m in MARKS:
        if end[-1] > m:
            s = int(np.searchsorted(st, m, side="right") - 1)  # the row that holds byte m (it starts at m or in front of it)
            rows |= {max(s - 1, 0), s, min(s + 1, st.size - 1)}
    return sorted(rows)


# ------------------------------------------------------------------------------------------------ Part C: long streams

C1_LEVEL, C1_BLOCK, C1_STREAMS = 1, 1152, 2
C1_NF = 65540
C1_N = C1_NF * C1_BLOCK - 100
C1_NOISE = (0, 65534, 65535, 65536, 65537, C1_NF - 1)

C2_LEVEL, C2_BLOCK = 5, 4096
C2_N0 = M31 + 3 * 4096  # whole frames
C2_N20, C2_N17 = C2_N0 + 20, C2_N0 + 17
C2_NF = -(-C2_N20 // C2_BLOCK)
C2_NOISE = (0, 65535, 65536, 524287, 524288, C2_NF - 2, C2_NF - 1)


def utf8_bytes(v):
    """Bytes of FLAC's UTF-8-style number field."""
    if v < 0x80:
        return 1
    k = 2
    while v >= (1 << (5 * k + 1)):
        k += 1
    return k


def sparse_frames(n_stream, n, block, frames, seed, bits=12):
    """{(stream, frame): int32 noise of `bits` bits for that frame} -- everything else of the (n_stream, n) array is zero."""
    rng = np.random.default_rng(seed)
    out = {}
    for s in range(n_stream):
        for f in frames:
            m = min(block, n - f * block)
            assert m > 0
            out[(s, f)] = rng.integers(-(1 << (bits - 1)), 1 << (bits - 1), m).astype(np.int32)
    return out


def sparse_host(n_stream, n, block, noise):
    x = np.zeros((n_stream, n), dtype=np.int32)
    for (s, f), v in noise.items():
        x[s, f * block : f * block + v.size] = v
    return x
