"""Plain numpy model of the reference's float <-> integer conversions, and a seeded corpus of edge inputs for them.

The four functions restate src/flacarray/libflacarray/utils.c of the reference, one operation at a time:
  float32_to_int32   utils.c:159-243    float64_to_int64   utils.c:245-327
  int64_to_float64   utils.c:329-348    int32_to_float32   utils.c:350-368
The reference is C built for x86-64: float operations round to float (no contraction), a float mixed with a double
literal is promoted, and an out-of-range or NaN double-to-integer cast (cvttsd2si) gives the "integer indefinite",
INT32_MIN / INT64_MIN.  Every array is vectorised over streams; nothing here calls the library or the oracle.
"""
from collections import namedtuple

import numpy as np

f32, f64 = np.float32, np.float64

QCase = namedtuple("QCase", "name x quanta")  # x [n_stream, n]; quanta None or one per stream, x's dtype
RCase = namedtuple("RCase", "name ints offsets gains")  # ints [n_stream, n] int32 / int64; offsets, gains per stream


def cvtt(v, bits):
    """C's (int32_t) / (int64_t) cast of a double on x86-64: truncation toward zero, INT_MIN when the truncated
    value does not fit or v is NaN."""
    v = np.asarray(v, dtype=f64)
    lo = -(2.0 ** (bits - 1))
    # (-2^31 - 1, 2^31) truncates into int32; for int64 the double below -2^63 is already 2048 away
    ok = ((v > lo - 1.0) if bits == 32 else (v >= lo)) & (v < -lo)
    it = np.int32 if bits == 32 else np.int64
    out = np.trunc(np.where(ok, v, 0.0)).astype(it)
    out[~ok] = np.iinfo(it).min
    return out


def stream_range(x):
    """(smin, smax) per row as utils.c:181-193 scans it: strict < and >, so among equal values (only +0 and -0 can
    be told apart) the first one wins.  NaN-free input only (the Python layer rejects NaN, utils.py:268)."""
    rows = np.arange(x.shape[0])
    mn, mx = x.min(axis=-1), x.max(axis=-1)
    return x[rows, np.argmax(x == mn[:, None], axis=-1)], x[rows, np.argmax(x == mx[:, None], axis=-1)]


def range_params(x):
    """(unsnapped offset, min_quanta) per stream of a 2-D float32 / float64 array: utils.c:181-203 for float32 (a
    float sum halved in double, float subtractions, 1.01 * d in double, a float division by (float)2147483647 == 2^31),
    utils.c:265-287 for float64 (all double, the division by (double)(2^63 - 1) == 2^63)."""
    with np.errstate(all="ignore"):
        smin, smax = stream_range(x)
        if x.dtype == f32:
            off = (0.5 * (smin + smax).astype(f64)).astype(f32)  # :194
            d1, d2 = smin - off, smax - off  # :198
            amp = np.where(d1 > d2, 1.01 * d1.astype(f64), 1.01 * d2.astype(f64)).astype(f32)  # :199-202
            return off, amp / f32(2147483647)  # :203
        off = 0.5 * (smin + smax)  # :278
        amp = np.where((smin - off) > (smax - off), 1.01 * (smin - off), 1.01 * (smax - off))  # :282-286
        return off, amp / f64(9223372036854775807)  # :287


def quantise_with(x, offsets, gains):
    """The per-sample step of float32_to_int32 (utils.c:234-240) / float64_to_int64 (utils.c:318-325) with the offsets
    and gains given, one per row of x: subtract and multiply in x's type, +-0.5 in double, the truncating cast."""
    x = np.asarray(x)
    dt, bits = (f32, 32) if x.dtype == f32 else (f64, 64)
    off, gain = np.asarray(offsets, dtype=dt).reshape(-1), np.asarray(gains, dtype=dt).reshape(-1)
    with np.errstate(all="ignore"):
        st = x - off[:, None]  # :234 / :318
        pr = (gain[:, None] * st).astype(f64)  # :236/238 a float multiply for float32, then the double +-0.5
        v = np.where(st >= 0, pr + 0.5, pr - 0.5)  # :319-323
    return cvtt(v, bits)


def float32_to_int32(x, quanta=None):
    """utils.c:159-243 -> (int32 [n_stream, n], offsets float32, gains float32)."""
    x = np.ascontiguousarray(x, dtype=f32).reshape(-1, np.shape(x)[-1])
    off, min_quanta = range_params(x)
    with np.errstate(all="ignore"):
        sq = min_quanta if quanta is None else np.asarray(quanta, dtype=f32).reshape(-1)  # :205-216
        nquant = cvtt(off.astype(f64) / sq.astype(f64), 64)  # :221
        off = (sq.astype(f64) * nquant.astype(f64)).astype(f32)  # :222
        gain = np.where(sq == 0, f64(1.0), 1.0 / sq.astype(f64)).astype(f32)  # :224-230
    return quantise_with(x, off, gain), off, gain  # :234-240


def float64_to_int64(x, quanta=None):
    """utils.c:245-327, every operation in double -> (int64 [n_stream, n], offsets, gains)."""
    x = np.ascontiguousarray(x, dtype=f64).reshape(-1, np.shape(x)[-1])
    off, min_quanta = range_params(x)
    with np.errstate(all="ignore"):
        sq = min_quanta if quanta is None else np.asarray(quanta, dtype=f64).reshape(-1)
        nquant = cvtt(off / sq, 64)  # :305
        off = sq * nquant.astype(f64)  # :306
        gain = np.where(sq == 0, 1.0, 1.0 / sq)  # :308-314
    return quantise_with(x, off, gain), off, gain  # :318-325


def int32_to_float32(ints, offsets, gains):
    """utils.c:350-368: coeff = 1.0 / gain in double, stored as float; then float multiply and float add."""
    ints = np.asarray(ints, dtype=np.int32)
    with np.errstate(all="ignore"):
        coeff = (1.0 / np.asarray(gains, dtype=f32).reshape(-1).astype(f64)).astype(f32)  # :361
        return np.asarray(offsets, dtype=f32).reshape(-1)[:, None] + coeff[:, None] * ints.astype(f32)  # :364


def int64_to_float64(ints, offsets, gains):
    """utils.c:329-348, in double."""
    ints = np.asarray(ints, dtype=np.int64)
    with np.errstate(all="ignore"):
        coeff = 1.0 / np.asarray(gains, dtype=f64).reshape(-1)  # :340
        return np.asarray(offsets, dtype=f64).reshape(-1)[:, None] + coeff[:, None] * ints.astype(f64)  # :343


def quantise(x, quanta=None):
    return (float32_to_int32 if x.dtype == f32 else float64_to_int64)(x, quanta)


def restore(ints, offsets, gains):
    return (int32_to_float32 if ints.dtype == np.int32 else int64_to_float64)(ints, offsets, gains)


def bits_equal(a, b):
    """Bitwise equality of two float or integer arrays, except that any NaN equals any NaN (x86 produces the negative
    default NaN, the GPU the positive one)."""
    a, b = np.asarray(a), np.asarray(b)
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    if a.dtype.kind != "f":
        return np.array_equal(a, b)
    u = {4: np.uint32, 8: np.uint64}[a.dtype.itemsize]
    same = a.view(u) == b.view(u)
    return bool(np.all(same | (np.isnan(a) & np.isnan(b))))


# ---------------------------------------------------------------------------------------------------------------
# The corpus
# ---------------------------------------------------------------------------------------------------------------
def _special_quanta(dtype, typical):
    """The per-stream quanta every family is also tried with: its own typical value, a subnormal, the smallest
    subnormal, zero, a quanta so large that every integer is 0, and inf."""
    fi = np.finfo(dtype)
    return np.array([typical, fi.tiny / 1024, fi.smallest_subnormal, 0.0, fi.max / 4, np.inf], dtype=dtype)


def _families(dtype, rng):
    """Named edge families: (name, x [n_stream, n], typical quanta).  Lengths 4096k + {0, 1, 2, 3}, a few tiny ones,
    and one family longer than the range pre-pass's 65536-sample chunk."""
    big = f32(2.0**31) if dtype == f32 else f64(2.0**63)
    ulp_below = np.spacing(big / 2, dtype=dtype)  # the spacing just below big (= ulp of big / 2)
    fam = []

    def sine(n, k, amp, dc):
        t = np.arange(n)
        return (dc + amp * (np.sin(2 * np.pi * t / 1500.0)[None, :] * rng.random((k, 1)) + 0.1 * rng.normal(0, 1, (k, n)))).astype(dtype)

    fam.append(("sine", sine(8192, 2, 1.0, 0.37), 1e-4 * 1.37))
    # a typical quanta far below min_quanta: most samples are out of range, the peaks truncate to INT_MIN
    peaks = sine(8192, 2, 1.0e4, -3.0)
    peaks[0, 100], peaks[1, 8191] = 9.0e4, -7.0e4
    fam.append(("peaks", peaks, 1e-6 if dtype == f32 else 1e-16))
    # infinite samples: +inf, -inf, both (smin + smax is NaN), at the first and at the last sample
    inf = sine(4096, 4, 2.0, 0.0)
    inf[0, 7], inf[1, 0], inf[2, 4095], inf[2, 1], inf[3, 4095] = np.inf, -np.inf, np.inf, -np.inf, np.inf
    fam.append(("inf", inf, 0.25))
    # subnormal samples: min_quanta underflows to 0 (gain 1), the offset snaps with a zero quanta
    sub = (rng.integers(-1000, 1000, (2, 4099)) * np.finfo(dtype).smallest_subnormal).astype(dtype)
    sub[1] = np.abs(sub[1]) + np.finfo(dtype).smallest_subnormal * 3
    fam.append(("subnormal", sub, np.finfo(dtype).smallest_subnormal * 4))
    # zeros of both signs: st == +-0, the first-wins rule of the range scan
    z = np.zeros((3, 4096), dtype=dtype)
    z[0, ::3] = -0.0
    z[1, 0] = -0.0
    z[1, 5:] = np.where(rng.random(4091) < 0.5, 0.0, -0.0)
    z[2, 1000] = 1.0
    fam.append(("zeros", z, 0.125))
    # exact ties (k + 1/2) q with a power-of-two quanta: after the offset snap every product is a half-integer
    q = 2.0**-6
    fam.append(("ties", ((rng.integers(-5000, 5000, (2, 8192)) + 0.5) * q).astype(dtype), q))
    # products on either side of +-2^31 (+-2^63) after the +-0.5, around a zero offset (smin == -smax)
    edge = np.array([big + 2 * ulp_below, big, big - ulp_below, 0.5, 1.5, 2.5, -0.5, -1.5, -2.5, 0.0, -0.0,
                     -(big - ulp_below), -big, -(big + 2 * ulp_below)], dtype=dtype)
    e = np.resize(edge, (2, 4097))
    e[:, -1] = edge[-1]
    e[1] *= dtype(0.5)  # the same products with the typical quanta 0.5
    fam.append(("int_edges", e, 1.0))
    # near the largest finite value: smin + smax and 1.01 * d overflow
    fmax = np.finfo(dtype).max
    h = sine(8194, 2, 1.0, 0.0) * dtype(fmax / 8)
    h[0, 3], h[1, 0], h[1, 8193] = fmax, fmax, -fmax  # stream 1: 1.01 * d overflows
    fam.append(("huge", h, float(fmax) / 2.0**40))
    # tiny geometries
    fam.append(("n1", np.array([[1.5], [-0.0], [np.inf], [fmax], [np.finfo(dtype).smallest_subnormal]], dtype=dtype), 0.5))
    fam.append(("n2", np.array([[1.0, -3.25], [np.inf, -np.inf], [0.0, -0.0]], dtype=dtype), 0.25))
    fam.append(("n3", np.array([[7.0, -7.0, 0.49], [2.5, 2.5, 2.5]], dtype=dtype), 0.5))
    return fam


def _long_family(dtype, rng):
    """Streams longer than one range chunk (65536): one of the fused geometry (17 frames of 4096), one that is not;
    the extremes sit in the last chunk, one at the last sample."""
    out = []
    for n in (69632, 65539):
        x = (rng.normal(0, 1, (2, n)) * 100.0).astype(dtype)
        x[0, n - 1], x[0, n - 2] = 1.0e4, -2.0e4
        x[1, 65536 + 2], x[1, n - 1] = -3.0e4, 5.0e4
        out.append((f"long{n}", x, 0.01))
    return out


def quantise_cases(dtype, seed=20261015):
    """Named quantise cases for float32 or float64.  Each family gives a case with quanta from the range (None), one
    with its typical quanta, and one whose streams repeat the family under each special quanta in turn."""
    rng = np.random.default_rng(seed if dtype == f32 else seed + 1)
    cases = []
    for name, x, typical in _families(dtype, rng):
        cases.append(QCase(f"{name}/range", x, None))
        cases.append(QCase(f"{name}/typical", x, np.full(x.shape[0], typical, dtype=dtype)))
        sq = _special_quanta(dtype, typical)
        cases.append(QCase(f"{name}/special", np.repeat(x, sq.size, axis=0), np.tile(sq, x.shape[0])))
    for name, x, typical in _long_family(dtype, rng):
        cases.append(QCase(f"{name}/range", x, None))
        cases.append(QCase(f"{name}/typical", x, np.array([typical, typical * 3.7], dtype=dtype)))
    return cases


def restore_cases(dtype, seed=20261016):
    """Named restore cases (int32 -> float32 or int64 -> float64) whose offsets and gains are what a user may hand in,
    e.g. from HDF5 attributes: gain 0, inf, negative, subnormal and non-power-of-two; offsets +-inf and -0.0; integers
    at INT_MIN / INT_MAX, where int-to-float rounds (2^24 + 1, above 2^53) and random full-range ones."""
    rng = np.random.default_rng(seed if dtype == f32 else seed + 1)
    it = np.int32 if dtype == f32 else np.int64
    ii = np.iinfo(it)
    fi = np.finfo(dtype)
    cases = []
    for n in (4096, 4097, 8194, 8195, 3):
        vals = rng.integers(ii.min, ii.max, (8, n), dtype=it, endpoint=True)
        special = np.array([ii.min, ii.max, ii.min + 1, 0, -1, 1, 2**24 + 1, -(2**24 + 1)]
                           + ([2**53 + 1, -(2**53 + 1), 2**62 + 3] if it == np.int64 else []), dtype=it)
        vals[:, : min(n, special.size)] = special[: min(n, special.size)]
        vals[1, :] = rng.integers(-3000, 3000, n)  # small values: exact products
        gains = np.array([10.0 / 3.0, 0.0, np.inf, -7.1, fi.smallest_subnormal, fi.tiny / 3, 1.0e7 * np.pi, 2.0**-20], dtype=dtype)
        offsets = np.array([0.1, -0.0, np.inf, -np.inf, 1.0e30, -2.5, 0.0, -1.0 / 3.0], dtype=dtype)
        cases.append(RCase(f"user_gains/n{n}", vals, offsets, gains))
    return cases


def corpus_tags(dtype):
    """Which named edges the corpus reaches, worked out from the model's own results."""
    tags = set()
    big = 2.0**31 if dtype == f32 else 2.0**63
    for c in quantise_cases(dtype):
        ints, off, gain = quantise(c.x, c.quanta)
        imin = np.iinfo(ints.dtype).min
        x = c.x.astype(f64)
        with np.errstate(all="ignore"):
            st = c.x - off[:, None]
            pr = (gain[:, None] * (c.x - off[:, None])).astype(f64)
            finite = np.isfinite(pr)
            if np.any((ints == imin) & np.isfinite(x) & finite & (np.abs(pr) >= big)):
                tags.add("truncated_peak")
            if np.any(finite & (np.abs(pr) < big) & (np.abs(pr) % 1.0 == 0.5)):
                tags.add("tie")
        if np.any(np.isinf(c.x)):
            tags.add("inf")
        if np.any((c.x != 0) & (np.abs(c.x) < np.finfo(dtype).tiny)) or (c.quanta is not None and np.any(
                (c.quanta != 0) & (np.abs(c.quanta) < np.finfo(dtype).tiny))):
            tags.add("subnormal")
            if np.any(st == 0):
                tags.add("st_zero")
        if c.x.shape[1] > 65536:
            tags.add("long")
        if c.x.shape[1] % 4:
            tags.add("unaligned_length")
    return tags


def windows(n):
    """Sample windows [first, last) of a stream of n samples: starts 0, 1, 3, 4, 5 and n - 1, to the end and short,
    so that both ends fall on and off a 4-sample boundary."""
    firsts = sorted({f for f in (0, 1, 3, 4, 5, n - 1) if 0 <= f < n})
    out = [(f, n) for f in firsts]
    out += [(f, min(n, f + k)) for f, k in ((1, 6), (3, 4097), (5, 2), (4, 4)) if f < n]
    return sorted(set(out))


def slices(n_stream, n, seed=7):
    """Slice requests (stream, first, count): 1-7 samples at odd starts, over every stream, plus each stream's last
    sample."""
    rng = np.random.default_rng(seed)
    k = 2 * n_stream + 5
    stream = rng.integers(0, n_stream, k)
    count = np.minimum(rng.integers(1, 8, k), n)
    first = np.minimum(rng.integers(0, max(n // 2, 1), k) | 1, n - count)
    stream = np.concatenate([stream, np.arange(n_stream)])
    first = np.concatenate([first, np.full(n_stream, n - 1)])
    count = np.concatenate([count, np.ones(n_stream, np.int64)])
    return stream.astype(np.int64), first.astype(np.int64), count.astype(np.int64)
