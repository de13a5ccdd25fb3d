"""Adversarial corpus for the device np.std (std_device; S1 / S2 in csrc/std_kernels.hpp): named cases
(name, dtype, x, bufsize) whose standard deviation along the last axis, taken by numpy with np.getbufsize() == bufsize,
is what the kernel must give bit for bit.

Pure numpy and seeded; the only library import is flacarray_amd.npsum (the plan that tells which path a length takes).
tests/test_std_corpus.py checks the reference on every case and asserts the corpus's own conditions; the GPU tests
(tests/test_gpu_std_edges.py) run every case through the kernel.

Families (the case names start with these words):

  geom    buffer geometries: 16, 1024, 16384 (plans of 1, 8 and 128 leaves), 262160 (2050 leaves: two batches of the plan
          path, the second of 2 leaves) and 2**20 (8192 leaves: four exact batches); row lengths at the chunk's edges,
          several chunks and a tail, the 8192-element fast path as a TAIL and as a whole row under a larger buffer
  sweep   2**17 + 3 rows of each length 2, 3, 5, 7, 8, 9, 17 with row scales over the whole exponent range: the division
          by n, the square root and the last rounding to the dtype on a hundred thousand different values per length
  sqrt    4096 rows [-p, p, -q, q] per dtype whose exact sqrt(var) lies nearest a rounding boundary of the dtype, picked
          from 2**20 candidates
  hard    infinities, overflowing sums and squares, subnormal squares, subnormals, -0.0, cancellation
  nan     one NaN per row at leaf, chunk and batch edges
"""
import functools
import math

import numpy as np

from flacarray_amd import npsum

DTYPES = (np.float32, np.float64)
BUFSIZES = (16, 1024, 16384, 262160, 2**20)
DEFAULT_BUFSIZE = 8192  # numpy's own default: the kernel's lane-per-leaf chunk
SWEEP_ROWS = 2**17 + 3
SWEEP_LENGTHS = (2, 3, 5, 7, 8, 9, 17)
SQRT_CANDIDATES = 2**20
SQRT_KEPT = 4096
HARD_N = 9000  # one fast chunk and a plan tail of 808 at the default buffer
NAN_BIG_BUF = 262160
NAN_BIG_N = NAN_BIG_BUF + 300
HARD_KINDS = ("pinf", "ninf_last", "both_inf", "sum_overflow", "square_overflow", "subnormal_var", "subnormals",
              "negzero", "cancel")


def tag(dtype):
    return "f32" if np.dtype(dtype) == np.float32 else "f64"


def _seed(name):
    return [ord(ch) for ch in name]


def geometry_lengths(b):
    """Row lengths of the geometry cases of buffer size `b`, by label."""
    out = {"b-1": b - 1, "b": b, "b+1": b + 1, "3b+5": 3 * b + 5}
    if b > 1024:
        out["2b+8192"] = 2 * b + 8192
    if b != 8192:
        out["8192"] = 8192
    return out


def _geometry(name, dtype, b, n):
    rng = np.random.default_rng(_seed(name))
    rows = 3 if n <= 2**16 else 2
    x = 1e3 + rng.normal(size=(rows, n)) * (1 + rng.random((rows, 1)))
    return x.astype(dtype)


def _sweep(name, dtype, n):
    """Rows of n elements, scale * (dc + normal): scales 2**e with e uniform from the smallest subnormal's exponent to
    six below the largest (17 elements of up to 5 sigma + dc cannot overflow the SUM; where the squares overflow or
    vanish numpy says inf or 0 and so must the kernel), dc 0 for half the rows."""
    rng = np.random.default_rng(_seed(name))
    fi = np.finfo(dtype)
    lo, hi = fi.minexp - fi.nmant, fi.maxexp - 7
    e = rng.integers(lo, hi + 1, size=(SWEEP_ROWS, 1))
    dc = np.where(rng.random((SWEEP_ROWS, 1)) < 0.5, 0.0, rng.uniform(-4, 4, size=(SWEEP_ROWS, 1)))
    body = dc + rng.normal(size=(SWEEP_ROWS, n))
    with np.errstate(all="ignore"):
        return np.ldexp(body, e).astype(dtype)


def sqrt_boundary_distance(v, dtype):
    """Exact position of sqrt(v) between two neighbours of `dtype`, for one finite positive value v of that dtype (a
    python float holds it exactly): returns frac - 0.5, frac the fractional part of sqrt(v) in units of the result's
    ulp, truncated 40 bits or more behind the point -- 0 is the rounding boundary (the midpoint), negative rounds down,
    positive up.  Python integers only."""
    prec = np.finfo(dtype).nmant + 1
    num, den = float(v).as_integer_ratio()  # den is a power of two
    d = den.bit_length() - 1
    if d & 1:
        num, d = num * 2, d + 1
    extra = 40
    t = max(0, prec + extra + 2 - num.bit_length() // 2)
    r = math.isqrt(num << (2 * t))  # floor(sqrt(v) * 2**(t + d / 2))
    low_bits = r.bit_length() - prec
    assert low_bits >= extra
    frac = (r & ((1 << low_bits) - 1)) / float(1 << low_bits)
    return frac - 0.5


def _sqrt_rows(dtype):
    """(rows [-p, p, -q, q] of the kept candidates, exact signed boundary distance of each in ulps)."""
    rng = np.random.default_rng(_seed("sqrt_" + tag(dtype)))
    span = 30 if np.dtype(dtype) == np.float32 else 200  # the squares stay normal and far from overflow
    scale = np.ldexp(1.0, rng.integers(-span, span + 1, size=SQRT_CANDIDATES))
    p = (rng.uniform(0.5, 2.0, size=SQRT_CANDIDATES) * scale).astype(dtype)
    q = (rng.uniform(0.5, 2.0, size=SQRT_CANDIDATES) * scale).astype(dtype)
    rows = np.stack([-p, p, -q, q], axis=1)
    # the variance numpy forms: mean exactly 0 (-0.0 - p + p - q + q), the squares summed in order from -0.0, / 4 exact
    sq = rows * rows
    v = (((sq[:, 0] + sq[:, 1]) + sq[:, 2]) + sq[:, 3]) / dtype(4)
    # vectorised estimate of the distance, good enough to choose by; the kept rows are then measured with integers
    if np.dtype(dtype) == np.float32:
        s = np.sqrt(v.astype(np.float64))  # 29 bits beyond the float32 result
        near = s.astype(np.float32).astype(np.float64)
        delta = (s - near) / np.spacing(near.astype(np.float32)).astype(np.float64)
    else:
        s = np.sqrt(v)
        # v - s*s exactly: Veltkamp split and Dekker's product (no fused multiply-add needed)
        c = s * 134217729.0
        hi = c - (c - s)
        lo = s - hi
        prod = s * s
        err = ((hi * hi - prod) + 2.0 * hi * lo) + lo * lo
        resid = (v - prod) - err
        delta = resid / (2.0 * s) / np.spacing(s)
    est = 0.5 - np.abs(delta)  # distance of the exact root from the nearest midpoint, in ulps
    keep = np.sort(np.argpartition(est, SQRT_KEPT)[:SQRT_KEPT])
    rows, v = rows[keep], v[keep]
    dist = np.array([sqrt_boundary_distance(x, dtype) for x in v.tolist()])
    return np.ascontiguousarray(rows), dist


@functools.lru_cache(maxsize=None)
def sqrt_rows(which):
    """The hard-square-root rows of dtype tag `which` ("f32" / "f64") and their exact boundary distances, built once."""
    return _sqrt_rows(np.float32 if which == "f32" else np.float64)


def hard_row(kind, dtype, rng):
    """One 9000-element row of the hard-value family."""
    fi = np.finfo(dtype)
    n = HARD_N
    with np.errstate(all="ignore"):
        if kind == "pinf":
            r = rng.normal(size=n)
            r[4321] = np.inf
        elif kind == "ninf_last":
            r = rng.normal(size=n)
            r[n - 1] = -np.inf
        elif kind == "both_inf":
            r = rng.normal(size=n)
            r[100], r[8500] = np.inf, -np.inf
        elif kind == "sum_overflow":
            return (rng.uniform(0.5, 1.0, size=n).astype(dtype) * fi.max).astype(dtype)
        elif kind == "square_overflow":
            return (rng.normal(size=n) * 4.0 * math.sqrt(float(fi.max))).astype(dtype)
        elif kind == "subnormal_var":
            return (rng.normal(size=n) * (1e-21 if fi.bits == 32 else 1e-158)).astype(dtype)
        elif kind == "subnormals":
            return (rng.integers(-1000, 1001, size=n) * float(fi.smallest_subnormal)).astype(dtype)
        elif kind == "negzero":
            return np.full(n, -0.0, dtype=dtype)
        elif kind == "cancel":
            return np.tile(np.array([1e8, 1.0, -1e8, 3.0]), n // 4).astype(dtype)
        else:
            raise KeyError(kind)
        return r.astype(dtype)


def _hard(name, dtype, kind):
    """The hard row between two ordinary ones (which must come out untouched by their neighbour)."""
    rng = np.random.default_rng(_seed(name))
    x = (3.0 + rng.normal(size=(3, HARD_N))).astype(dtype)
    x[1] = hard_row(kind, dtype, rng)
    return x


def nan_positions(n, big):
    pos = [0, 7, 8, 127, 128, 8191, 8192, n - 1]
    if big:  # 2047 * 128; the first batch's last element and the second batch's first (leaf 2048 starts at 262024); the
        # chunk's last element; the next chunk's first
        pos += [262016, 262023, 262024, 262159, 262160]
    return pos


def _nan(name, dtype, n, big):
    """One row per position with a single NaN there, and a clean last row."""
    rng = np.random.default_rng(_seed(name))
    pos = nan_positions(n, big)
    x = (1e3 + rng.normal(size=(len(pos) + 1, n))).astype(dtype)
    for r, p in enumerate(pos):
        x[r, p] = np.nan
    return x


def _specs():
    """[(name, dtype, bufsize, builder)]: everything but the data, so that names can parametrise tests cheaply."""
    out = []
    for dtype in DTYPES:
        t = tag(dtype)
        for b in BUFSIZES:
            for label, n in geometry_lengths(b).items():
                name = f"geom_{t}_buf{b}_{label}"
                out.append((name, dtype, b, functools.partial(_geometry, name, dtype, b, n)))
        for n in SWEEP_LENGTHS:
            name = f"sweep_{t}_n{n}"
            out.append((name, dtype, DEFAULT_BUFSIZE, functools.partial(_sweep, name, dtype, n)))
        out.append((f"sqrt_{t}", dtype, DEFAULT_BUFSIZE, lambda t=t: sqrt_rows(t)[0]))
        for kind in HARD_KINDS:
            name = f"hard_{t}_{kind}"
            out.append((name, dtype, DEFAULT_BUFSIZE, functools.partial(_hard, name, dtype, kind)))
        out.append((f"nan_{t}_default", dtype, DEFAULT_BUFSIZE, functools.partial(_nan, f"nan_{t}_default", dtype, HARD_N, False)))
        out.append((f"nan_{t}_batches", dtype, NAN_BIG_BUF, functools.partial(_nan, f"nan_{t}_batches", dtype, NAN_BIG_N, True)))
    return out


SPECS = _specs()
NAMES = [s[0] for s in SPECS]


def build(names=None):
    """The corpus as a dict name -> (name, dtype, x, bufsize), x C-contiguous and read-only; `names` restricts it.
    Also asserts the conditions the hard-square-root family has to meet (from exact integer arithmetic alone)."""
    out = {}
    for name, dtype, b, make in SPECS:
        if names is not None and name not in names:
            continue
        x = np.ascontiguousarray(make())
        assert x.dtype == np.dtype(dtype) and x.ndim == 2
        x.setflags(write=False)
        out[name] = (name, dtype, x, b)
        if name.startswith("sqrt_"):
            dist = sqrt_rows(tag(dtype))[1]
            close = np.abs(dist) < 2.0**-10
            assert close.sum() >= 1000, (name, int(close.sum()))
            assert (dist[close] < 0).any() and (dist[close] > 0).any(), name
    return out


def reference(case):
    """np.std(x, axis=-1) with numpy's buffer at the case's size: THE expectation of every comparison."""
    _, _, x, b = case
    old = np.getbufsize()
    try:
        np.setbufsize(b)
        with np.errstate(all="ignore"):
            return np.std(x, axis=-1)
    finally:
        np.setbufsize(old)


def chunk_lengths(n, b):
    """(full chunk length or None, tail length or None) of a row of n elements under buffer size b."""
    full = b if n >= b else None
    tail = n % b if n % b else None
    return full, tail


def plan_leaves(length):
    return len(npsum.pairwise_plan(length)[0])
