"""Encoder decision corpus: named, seeded inputs that drive every rare branch of the encoder specification
(oracle/flac_oracle.c, rice_search through encode_frame) -- and so of the HIP encoder bodies that restate it: K3F
(csrc/encode_fused.hpp), the slot body shared by K3G and the slot sequence (csrc/encode_kernels.hpp) and the append
re-encode (csrc/splice_kernels.hpp).  Nothing here calls the library: tests/test_encoder_corpus.py audits, on the
oracle's decision trace, that every decision of its table is reached by a case that lists it, and
tests/test_gpu_encoder_corpus.py runs every case through every route that takes its geometry.

A Case is an array [n_stream, n], a level, and the names of the decisions it is built for.  Cases with k3f=True are int32
arrays of whole 4096-sample frames at levels 3 to 8 (K3F's geometry).  Their rare frames stand among ordinary
sinusoid-plus-noise frames (tests.conftest.sinusoid_noise_i32) at flat frame indices 1, 4, 7, ... of streams of eight
frames: one K3F wave solves the LPC problems of the four consecutive frames of its workgroup, and the stride of three puts
each class of rare frames (two or more frames per class) on different positions modulo 4.  Levels 0 to 2, short last frames,
streams of up to four samples and int64 go to K3G and the slot sequence only (k3f=False).

Branches of the oracle that no input reaches, and why (tools/oracle_branch_coverage.py lists them as untaken):

  * quantize_coefs `sh < -16` (return 1), the negative-shift loop `sh < 0`, and `prec < 2` in encode_subframe.  Levels 3-8
    use 4096-sample blocks, for which the precision is 15; the `bps <= 17` limit lowers it to 32 - bps - floor(log2(order))
    >= 32 - 17 - 3 = 12, so 12 <= prec <= 15 always.  A negative shift then needs a coefficient of magnitude >= 2^(prec-1):
    2^14 in general, 2^11 at the earliest (prec 12: order >= 8 and 17 bits per sample).  Levinson coefficients built from
    reflection coefficients of magnitude <= 1 are bounded by the binomials C(order, k): at most 924 (order 12), 70 (order 8).
    A reflection coefficient passes 1 only when rounding makes an error term negative (pure tones at 2^27 and more do that:
    the `levinson_negative` decision); best_lpc_order prices those orders at 1e32 bits per sample, and the orders after
    them that come out positive again kept |coefficient| < 200 in everything tried.  Tried for small shifts: 1 to 3 pure
    tones at amplitudes 2^20, 2^27 and 2^30 and periods from 10 to 3000 samples, 40 seeds each, at levels 3, 5 and 8, and
    autoregressive processes of orders 1 to 12 with pole radii up to 0.995: the smallest raw shift seen is 6 (three tones of
    periods 10 to 100 samples at 2^27, level 8), shifts 7 to 15 are in the corpus, 0 to 5 and every negative shift were not
    reached.
  * The clamp at qmin.  With sh = prec - 2 - floor(log2(cmax)) every product |c| 2^sh is below 2^(prec-1) = -qmin, the error
    carried between coefficients is at most 0.5 in magnitude, so the rounded value is >= -2^(prec-1) - 1 + 1 = qmin: the
    clamp can only act at qmax (where 2^(prec-1) = qmax + 1 is reached: the `coef_clamped_qmax` decision).  A shift limited
    to 15 only makes the products smaller.
  * `err == 0.0` in levinson and the `bps = 0.0` arm of best_lpc_order that it feeds.  err is multiplied by 1 - r^2; zero
    needs |r| = 1 exactly, which in exact arithmetic needs a windowed frame that is a multiple of its own shift (impossible
    for a finite nonzero frame) and in double needs r within 2^-53 of 1; the closest tried (constant plus one differing
    sample at 2^30: 1 - r about 4e-7, set by the window's taper) is far from it.  A frame whose windowed samples are all
    zero never reaches levinson (`lpc_lags_zero`).
  * `n <= pred_order` in rice_search.  max_porder_for lowers the partition order until (bs >> p) > pred_order and at p = 0
    that is bs > pred_order: FIXED orders are <= 4 < bs (frames of up to 4 samples are VERBATIM before any search) and the LPC
    order is limited to bs - 1.  For the same reason rice_search never fails (`LPC_RICE` is not a cause that occurs).
  * Saturation of the 32-bit bit estimate.  A partition's estimate is 4 + (1 + k) n + (S >> (k - 1)) - n / 2 with S <= n 2^31
    and k >= floor(log2(S / n)): the shifted sum is below 8 n, the whole below 40 n <= 163 840 for n <= 4096, and a frame's
    sum over its partitions below 2^18.
  * blocksize_code's cases above 4096 (4608, 8192, 16384, 32768): the block size is 1152 or 4096 and a last frame is
    shorter.  put_utf8's forms of four bytes and more: a frame number of 2^16 needs a stream of 75 million samples, which
    the corpus leaves out for its size (frame_numbers_l0 crosses 128 and 2048); numbers from 2^21 on are excluded by
    encode_stream's limit of 18 nf < 2^24 SEEKTABLE bytes.
  * realloc / malloc failures of the bit writer.
"""
import numpy as np

from tests.conftest import sinusoid_noise_i32

B = 4096       # block size of levels 3-8
B_LOW = 1152   # block size of levels 0-2
I32_MIN, I32_MAX = -(2**31), 2**31 - 1


def _i32(v):
    v = np.asarray(v)
    assert v.min() >= I32_MIN and v.max() <= I32_MAX
    return v.astype(np.int32)


# ---- frames ---------------------------------------------------------------------------------------------------------
def noise_frame(seed, n=B, bits=10):
    """Uniform noise of `bits` bits (sign included)."""
    return _i32(np.random.default_rng(seed).integers(-(1 << (bits - 1)), 1 << (bits - 1), n))


def wasted_frame(seed, w, n=B, bits=12):
    """Non-constant frame with exactly `w` wasted bits: noise of at most `bits` bits, one value made odd, shifted left.
    w = 31 leaves one bit per sample: values in {0, INT32_MIN}."""
    bits = max(1, min(bits, 29 - w))
    v = np.random.default_rng(seed).integers(-(1 << (bits - 1)), 1 << (bits - 1), n)
    v[n // 3] = -1
    v[n // 3 + 1] = 0
    return _i32(v << w)


def ar_frame(seed, order, n=B, amp=2.0**20, radius=(0.9, 0.995), noise=1.0):
    """Autoregressive process of `order` random stable poles driven by white noise, scaled to peak `amp`."""
    rng = np.random.default_rng(seed)
    poles = []
    for _ in range(order // 2):
        r, th = rng.uniform(*radius), rng.uniform(0.05, np.pi - 0.05)
        poles += [r * np.exp(1j * th), r * np.exp(-1j * th)]
    if order & 1:
        poles.append(rng.uniform(*radius) * rng.choice([-1.0, 1.0]))
    a = np.real(np.poly(poles))[1:]
    e = rng.normal(0.0, noise, n + 512)
    y = np.zeros(n + 512)
    for i in range(n + 512):
        acc = e[i]
        for j in range(min(i, order)):
            acc -= a[j] * y[i - 1 - j]
        y[i] = acc
    y = y[512:]
    return _i32(np.rint(y * (amp / np.abs(y).max())))


def tones_frame(seed, n=B, amp=2.0**24, ntone=2, noise=0.0, fmax=0.02):
    """A sum of `ntone` slow sinusoids (periods of 1/fmax samples and more) of peak about `amp`, plus Gaussian noise."""
    rng = np.random.default_rng(seed)
    t = np.arange(n)
    y = sum(rng.uniform(0.3, 1.0) * np.sin(2 * np.pi * rng.uniform(0.1 * fmax, fmax) * t + rng.uniform(0, 6.28)) for _ in range(ntone))
    y = y * (amp / np.abs(y).max()) + rng.normal(0.0, noise, n) if noise else y * (amp / np.abs(y).max())
    return _i32(np.clip(np.rint(y), I32_MIN, I32_MAX))


def lpc_wasted_frame(seed, w, order, n=B):
    """An LPC-friendly frame whose samples have exactly `w` wasted bits and fill the remaining 32 - w bits: an
    autoregressive process, OR 1, shifted left."""
    v = ar_frame(seed, order, n, amp=2.0 ** (31 - w) * 0.9).astype(np.int64) | 1
    return _i32(v << w)


def poly_frame(seed, degree, n=B, noise_bits=3):
    """A polynomial of `degree` plus small noise: FIXED order degree + 1 leaves the noise."""
    rng = np.random.default_rng(seed)
    t = np.arange(n, dtype=np.float64) / n
    y = sum(rng.uniform(-1, 1) * t**k for k in range(degree + 1))
    y = np.rint(y * 2.0**24 / max(np.abs(y).max(), 1e-9)).astype(np.int64)
    return _i32(y + rng.integers(-(1 << noise_bits), 1 << noise_bits, n))


def walk_frame(seed, times, n=B, step=64):
    """White noise integrated `times` (0 to 2) times: FIXED order `times` whitens it exactly."""
    v = np.random.default_rng(seed).integers(-step, step + 1, n)
    for _ in range(times):
        v = np.cumsum(v)
    return _i32(v)


def smooth_frame(seed, n=B, fmax=0.01, noise=0.0, amp=2.0**24):
    """Slow sinusoids with little noise: each further difference shrinks the signal by about 2 pi f and grows the noise,
    so fmax and noise set the FIXED order (3 or 4) that wins."""
    return tones_frame(seed, n, amp=amp, ntone=2, noise=noise, fmax=fmax)


def fixed_invalid_frame(seed, first, n=B):
    """FIXED orders `first`..4 meet a residual beyond INT32_MAX while the orders below stay valid.  first = 0: a plateau
    just above INT32_MIN that touches it (only |x| itself passes: order 0 alone is invalid).  first = 1: a step of more
    than 2^31 between two plateaus.  first = 2, 3, 4: small noise and one impulse J, which order k sees times the largest
    coefficient of (1 - z)^k (1, 1, 2, 3, 6): J = 0.75, 0.4, 0.2 x 2^31."""
    v = np.random.default_rng(seed).integers(-64, 64, n).astype(np.int64)
    if first == 0:
        v = I32_MIN + np.abs(v)
        v[n // 2] = I32_MIN
        v[n // 2 + 1] = I32_MIN + 1
    elif first == 1:
        v[n // 2 :] += 2**30 + 2**19
        v[: n // 2] -= 2**30 + 2**19
    else:
        v[n // 2] += int({2: 0.75, 3: 0.4, 4: 0.2}[first] * 2**31)
    return _i32(v)


def full_range_frame(seed, n=B):
    """Uniform over all of int32 with INT32_MIN present: no FIXED order is valid, nothing beats VERBATIM."""
    v = np.random.default_rng(seed).integers(I32_MIN, I32_MAX, n, dtype=np.int64)
    v[n // 5] = I32_MIN
    v[n // 5 + 1] = I32_MAX
    return _i32(v)


def near_max_frame(seed, n=B):
    """+-(INT32_MAX - small): the mean magnitude is 2^31, the Rice parameter estimate is 31 and is clamped at 30."""
    rng = np.random.default_rng(seed)
    return _i32((I32_MAX - rng.integers(0, 1000, n)) * rng.choice([-1, 1], n))


def partition_frame(seed, porder, n=B, lo_bits=3, hi_bits=14):
    """Noise whose amplitude alternates between `lo_bits` and `hi_bits` every n >> porder samples (porder 0: stationary)."""
    rng = np.random.default_rng(seed)
    if porder == 0:
        return noise_frame(seed, n, hi_bits)
    ps = n >> porder
    bits = np.where((np.arange(n) // ps) % 2 == 0, lo_bits, hi_bits)
    return _i32(np.rint(rng.uniform(-1, 1, n) * 2.0 ** (bits - 1)))


def impulse_frame(pos, value=1 << 20, n=B):
    """Zero but for one sample.  At position 0 the Tukey window (zero at its first point) leaves nothing: all lag sums are
    zero.  In the middle lags 1.. are zero: the predictor coefficients are all zero (cmax <= 0)."""
    v = np.zeros(n, dtype=np.int64)
    v[pos] = value
    return _i32(v)


def overflow_lpc_frame(seed, n=B):
    """A slow full-scale sinusoid with its second half negated: the predictor that follows the sinusoid meets a jump of
    almost 2^32 at the sign flip, a residual beyond 32 bits."""
    v = tones_frame(seed, n, amp=2.0**31 - 2**16, ntone=1, noise=200.0, fmax=0.004).astype(np.int64)
    k = int(np.argmax(np.abs(v[n // 4 : 3 * n // 4]))) + n // 4
    v[k:] = -v[k:]
    return _i32(v)


def loud_row_frame(seed, n, mag_bits=27, row=5):
    """Silence with one 256-sample row of +-2^mag_bits: where the frame's geometry allows partition order 0 only (odd
    lengths), the Rice parameter follows the frame's mean, 1/16 of the row's magnitude, and the row's codes pass the cap."""
    rng = np.random.default_rng(seed)
    v = rng.integers(-1, 2, n).astype(np.int64)
    v[256 * row : 256 * row + 256] = rng.choice([-1, 1], 256) * ((1 << mag_bits) - rng.integers(0, 1 << (mag_bits - 4), 256))
    return _i32(v)


def breakeven_frame(seed, n=B, bits=31.0):
    """Laplacian noise near the magnitude at which the Rice estimate ties VERBATIM: the estimate (means) says smaller, the
    exact count (every code) says larger."""
    rng = np.random.default_rng(seed)
    v = np.rint(rng.laplace(0.0, 2.0**bits / 4.0, n))
    return _i32(np.clip(v, I32_MIN + 1, I32_MAX))


def exact_over_frame(seed, n=B, w=30):
    """Two bits per sample after 30 wasted bits: runs of one or two 1s between single 0s.  FIXED order 0 wins (every 0 is
    two transitions), Rice parameter 0; the estimate takes half a bit per sample off for the code's remainder, which a
    parameter of 0 does not have, so the estimate is below VERBATIM (1.83 n against 2 n) and the exact size above it
    (2.33 n)."""
    rng = np.random.default_rng(seed)
    out = []
    while len(out) < n:
        out += [1] * int(rng.integers(1, 3)) + [0]
    return _i32(np.array(out[:n], dtype=np.int64) << w)


def tone_noise_frame(theta, seed=3, amp=2.0**22, noise=2000.0, n=B):
    """A sinusoid of `theta` radians per sample in noise.  QMAX_THETAS: found by bisection on the oracle trace's cmax, these
    give an order-8 predictor (levels 4 to 6) whose largest coefficient lies within 2^-15 below 1.0: times 2^14 it rounds
    to 2^14 = qmax + 1 and is clamped."""
    rng = np.random.default_rng(seed)
    t = np.arange(n)
    return _i32(np.rint(amp * np.sin(theta * t + 0.3) + rng.normal(0, noise, n)))


QMAX_THETAS = (0.10996909894110976, 0.10996917586418668, 0.10996809894110976, 0.10996802201803284,
               0.10996794509495592, 0.10996748355649438)


def pack_i64(low, high):
    """int64 samples from their (low word, high word) channels."""
    return (np.asarray(high, dtype=np.int64) << 32) | (np.asarray(low, dtype=np.int64) & 0xFFFFFFFF)


def background(n_stream, n, seed):
    return sinusoid_noise_i32(n_stream, n, seed=seed)


# ---- cases ----------------------------------------------------------------------------------------------------------
class Case:
    """name, level, array [n_stream, n] (int32 or int64), the decisions it is built for, `k3f` (K3F's geometry),
    `append_cut` (samples given to from_array before the rest is appended; None: too short to split) and `probe`: a
    stream of at most one frame holding the case's first rare frame, short enough for the pure-Python decoder."""

    def __init__(self, name, level, make, decisions, k3f=False, append_cut=None, probe=None):
        self.name, self.level, self._make, self.decisions = name, level, make, tuple(decisions)
        self.k3f, self.append_cut, self._probe = k3f, append_cut, probe
        self._x = None

    @property
    def x(self):
        if self._x is None:
            self._x = np.ascontiguousarray(self._make())
            assert self._x.ndim == 2 and self._x.dtype in (np.int32, np.int64)
        return self._x

    @property
    def is_int64(self):
        return self.x.dtype == np.int64

    @property
    def block(self):
        return B_LOW if self.level <= 2 else B

    def probe(self):
        return np.ascontiguousarray(self._probe() if self._probe else self.x[0, : self.block])

    def __repr__(self):
        return f"Case({self.name})"


def embed(rare, seed, amp=2**16):
    """int32 array of streams of eight 4096-sample frames: ordinary frames, the rare ones at flat indices 1, 4, 7, ..."""
    nfl = 8 * ((3 * len(rare) + 1 + 7) // 8)
    x = sinusoid_noise_i32(nfl // 8, 8 * B, seed=seed, amp=amp).reshape(nfl, B).copy()
    for j, fr in enumerate(rare):
        assert fr.shape == (B,)
        x[3 * j + 1] = fr
    return x.reshape(nfl // 8, 8 * B)


def rare_positions(n_rare):
    """(stream, frame) of embed()'s rare frames."""
    return [((3 * j + 1) // 8, (3 * j + 1) % 8) for j in range(n_rare)]


def _k3f(name, level, rare_fn, decisions, seed):
    return Case(name, level, lambda: embed(rare_fn(), seed), decisions, k3f=True, append_cut=B + 1000, probe=lambda: rare_fn()[0])


def _tail(name, level, tail_fn, decisions, seed, n_stream=2):
    """Streams of one ordinary full frame and a short last frame tail_fn(stream index)."""
    blk = B_LOW if level <= 2 else B

    def make():
        head = sinusoid_noise_i32(n_stream, blk, seed=seed)
        return np.concatenate([head, np.stack([tail_fn(i) for i in range(n_stream)])], axis=1)

    n_tail = tail_fn(0).shape[0]
    return Case(name, level, make, decisions, append_cut=blk + n_tail // 2 if n_tail >= 2 else blk - 5, probe=lambda: tail_fn(0))


LPC_MAX = {3: 6, 4: 8, 5: 8, 6: 8, 7: 12, 8: 12}
PORDER_MAX = {0: 3, 3: 4, 5: 5, 8: 6}
LIMIT_ORDERS = (2, 3, 5, 6, 8, 10, 12)
# (order, seed offset) of autoregressive frames whose level-8 predictors take the shifts 7, 7, 8, 8, ... 14, 14; the ordinary
# frames around them take 15
SHIFT_FRAMES = ((10, 2), (12, 2), (11, 0), (11, 1), (8, 1), (9, 1), (5, 2), (6, 0), (4, 3), (7, 1), (3, 3), (4, 2), (2, 0), (2, 2), (1, 0), (1, 1))


def blocksize_code(bs):
    """RFC 9639 9.1.1 block size bits."""
    table = {192: 1, 576: 2, 1152: 3, 2304: 4, 4608: 5, 256: 8, 512: 9, 1024: 10, 2048: 11, 4096: 12}
    return table.get(bs, 6 if bs <= 256 else 7)


def _build_cases():
    cases = []
    # -- K3F geometry ------------------------------------------------------------------------------------------------
    cases.append(_k3f("wasted_l3", 3, lambda: [wasted_frame(w, w) for w in range(1, 32)], [f"wasted{w}@hi" for w in range(1, 32)], 301))
    for lvl in (3, 5, 8):
        cases.append(_k3f(f"lpc_limit_l{lvl}", lvl, lambda: [lpc_wasted_frame(100 + o, w, o) for w in (15, 16, 17) for o in LIMIT_ORDERS],
                          [f"lpc_limit_w{w}@L{lvl}" for w in (15, 16, 17)] + ([f"lpc_precision{p}" for p in (13, 14, 15)] if lvl == 3 else [])
                          + (["lpc_precision12"] if lvl == 5 else []), 310 + lvl))
    for lvl in range(3, 9):
        cases.append(_k3f(f"lpc_orders_l{lvl}", lvl, lambda lvl=lvl: [ar_frame(1000 + 17 * p, p) for p in range(1, LPC_MAX[lvl] + 1)],
                          [f"lpc_order{p}@L{lvl}" for p in range(1, LPC_MAX[lvl] + 1)], 320 + lvl))
    cases.append(_k3f("lpc_shifts_l8", 8, lambda: [ar_frame(1000 + 17 * p + s, p) for p, s in SHIFT_FRAMES], [f"lpc_shift{s}" for s in range(7, 16)], 329))
    cases.append(_k3f("qmax_l5", 5, lambda: [tone_noise_frame(t) for t in QMAX_THETAS], ["coef_clamped_qmax"], 330))
    cases.append(_k3f("fixed_l5", 5, lambda: [noise_frame(1), walk_frame(11, 1), walk_frame(12, 2), tones_frame(0, B, 2.0**20, 1, 0.0, 0.003),
                                              smooth_frame(5, B, 0.002, 0.0)] + [fixed_invalid_frame(30 + k, k) for k in range(5)]
                      + [full_range_frame(3), full_range_frame(4)],
                      [f"fixed{k}_wins@hi" for k in range(5)] + [f"fixed{k}_invalid" for k in range(5)] + ["fixed_none_valid", "verbatim_no_candidate"], 340))
    for lvl in (3, 5, 8):
        cases.append(_k3f(f"partitions_l{lvl}", lvl, lambda: [partition_frame(40 + p, p) for p in range(7)],
                          [f"porder{p}@L{lvl}" for p in range(PORDER_MAX[lvl] + 1)], 350 + lvl))
    cases.append(_k3f("rice_l5", 5, lambda: [noise_frame(5, B, 1), noise_frame(6, B, 1), noise_frame(7, B, 20), noise_frame(8, B, 20), near_max_frame(6),
                                             near_max_frame(7)], ["rice0", "rice2_5bit", "rice_clamp30"], 360))
    cases.append(_k3f("verbatim_exact_l5", 5, lambda: [exact_over_frame(1), exact_over_frame(2)], ["verbatim_exact", "wasted_2bps"], 370))
    cases.append(_k3f("one_bit_l5", 5, lambda: [wasted_frame(31, 31), wasted_frame(32, 31)], ["wasted31_verbatim_1bps"], 371))
    cases.append(_k3f("lpc_drop_l5", 5, lambda: [impulse_frame(0), impulse_frame(B - 1), impulse_frame(2000), impulse_frame(777, -5), overflow_lpc_frame(8),
                                                 overflow_lpc_frame(9), tones_frame(0, B, 2.0**27, 1, 0.0, 0.003), tones_frame(0, B, 2.0**27, 3, 0.0, 0.003)],
                      ["lpc_lags_zero", "lpc_cmax_zero", "lpc_residual_overflow", "levinson_negative"], 380))
    cases.append(_k3f("lpc_estimate_l5", 5, lambda: [walk_frame(13, 1), walk_frame(14, 2)], ["lpc_estimate_not_smaller"], 381))
    # -- levels 0 to 2 (K3G and the slot sequence) -------------------------------------------------------------------------
    def low(frames_fn, seed):
        def make():
            fr = frames_fn()
            x = sinusoid_noise_i32(1, B_LOW * (len(fr) + 1), seed=seed).reshape(-1, B_LOW).copy()
            x[1:] = np.stack(fr)
            return x.reshape(1, -1)
        return make

    cases.append(Case("wasted_l1", 1, low(lambda: [wasted_frame(w, w, B_LOW) for w in range(1, 32)], 401), [f"wasted{w}@lo" for w in range(1, 32)],
                      append_cut=B_LOW + 100, probe=lambda: wasted_frame(17, 17, B_LOW)))
    cases.append(Case("fixed_l1", 1, low(lambda: [noise_frame(1, B_LOW), walk_frame(11, 1, B_LOW), walk_frame(12, 2, B_LOW), smooth_frame(5, B_LOW, 0.002, 8.0),
                                                  smooth_frame(5, B_LOW, 0.01, 0.0)] + [fixed_invalid_frame(30 + k, k, B_LOW) for k in range(5)]
                                         + [full_range_frame(3, B_LOW)], 402),
                      [f"fixed{k}_wins@lo" for k in range(5)] + ["fixed_none_valid@lo"], append_cut=B_LOW + 100, probe=lambda: smooth_frame(5, B_LOW, 0.002, 8.0)))
    cases.append(Case("partitions_l0", 0, low(lambda: [partition_frame(40 + p, p, B_LOW) for p in range(2)], 403), ["porder0@L0", "porder1@L0"],
                      append_cut=B_LOW + 100, probe=lambda: partition_frame(41, 1, B_LOW)))
    cases.append(_tail("partitions_tail_l0", 0, lambda i: partition_frame(42 + i, 2 + i, 1024), ["porder2@L0", "porder3@L0"], 404))
    cases.append(Case("frame_numbers_l0", 0, lambda: sinusoid_noise_i32(1, 2049 * B_LOW + 7, seed=405, amp=4), ["frame_no_128", "frame_no_2048"],
                      append_cut=2040 * B_LOW + 5, probe=lambda: sinusoid_noise_i32(1, 300, seed=405, amp=4)[0]))
    # -- short last frames: every block size code, both explicit forms ---------------------------------------------------------
    for n_tail in (192, 256, 512, 576, 1024, 1152, 2048, 2304):
        cases.append(_tail(f"tail{n_tail}_l5", 5, lambda i, n=n_tail: ar_frame(500 + n + i, 4 + 4 * i, n), [f"bscode{blocksize_code(n_tail)}"], 410 + n_tail))
    cases.append(_tail("tail100_l5", 5, lambda i: ar_frame(600 + i, 3, 100), ["bscode6"], 420))
    cases.append(_tail("tail1000_l5", 5, lambda i: ar_frame(610 + i, 8, 1000), ["bscode7"], 421))
    cases.append(_tail("tail_odd_l8", 8, lambda i: ar_frame(620 + i, 12, 2305), ["tail_odd_lpc12"], 422))
    cases.append(_tail("tail5_l5", 5, lambda i: np.array([7, -3, 100000, 2, -9 - i], np.int32), ["tail5_searched"], 423))
    cases.append(_tail("tail192_l1", 1, lambda i: walk_frame(630 + i, 1, 192), ["bscode1@lo"], 424))
    cases.append(_tail("tail700_l2", 2, lambda i: walk_frame(640 + i, 2, 700), ["bscode7@lo"], 425))
    cases.append(_tail("tail3_l5", 5, lambda i: np.array([5, -70000, 11 + i], np.int32), ["verbatim_short_tail"], 426))
    cases.append(_tail("rowcap_l5", 5, lambda i: loud_row_frame(1 + i, 4095, 24 + 3 * i, row=3 + i), ["verbatim_row_cap"], 427))
    for n in (1, 2, 3, 4):
        cases.append(Case(f"len{n}_l{5 if n & 1 else 1}", 5 if n & 1 else 1, lambda n=n: np.array([[9, -8, 70000, 3][:n], [-1, 2**31 - 1, -(2**31), 0][:n]], np.int32),
                          [f"verbatim_short_len{n}"] if n > 1 else ["len1_constant"], append_cut=1 if n > 1 else None))
    # -- int64: two-channel frames -----------------------------------------------------------------------------------------
    def stereo(n):
        rng = np.random.default_rng(77)
        hi_min = np.where(np.arange(n) % 500 == 250, I32_MIN, rng.integers(-2, 1, n))
        rows = [
            rng.integers(-100, 100, n).astype(np.int64),                                            # side chosen
            pack_i64(rng.integers(0, 100, n), hi_min),                                                # low - high passes 32 bits
            pack_i64(-rng.integers(1, 100, n), np.where(np.arange(n) % 500 == 250, I32_MAX, rng.integers(-2, 1, n))),  # ... below INT32_MIN
            rng.integers(-(2**40), 2**40, n),                                                          # low word not small
            rng.integers(0, 200, n).astype(np.int64),                                                 # high word zero
            pack_i64(rng.integers(-100, 100, n), rng.integers(-1000, 1000, n)),                       # side costs more
            np.where(rng.random(n) < 0.5, 2 * rng.integers(0, 60, n), -2 * rng.integers(0, 60, n) - 1).astype(np.int64),  # side = even
            pack_i64(rng.integers(-(2**20), 2**20, n), rng.integers(-50, 50, n) * 8),                  # high word with 3 wasted bits
            pack_i64(rng.integers(-(2**20), 2**20, n), np.resize(lpc_wasted_frame(9, 16, 6), n)),      # high word: 16 bits, LPC
            pack_i64(np.resize(lpc_wasted_frame(10, 15, 8), n), rng.integers(-3, 3, n)),              # low word: 17 bits, LPC
        ]
        return np.stack(rows)

    st_names = ["side_chosen", "side_refused_fits", "side_refused_fits_negative", "side_refused_small", "side_refused_right_zero", "side_refused_estimate", "side_wasted", "high_wasted"]
    cases.append(Case("i64_stereo_l5", 5, lambda: stereo(2 * B + 100), [s + "@hi" for s in st_names] + ["i64_high_lpc_bps16", "i64_low_lpc_bps17"],
                      append_cut=B + 50, probe=lambda: stereo(600)[6]))
    cases.append(Case("i64_stereo_l1", 1, lambda: stereo(2 * B_LOW + 100), [s + "@lo" for s in st_names], append_cut=B_LOW + 50, probe=lambda: stereo(600)[0]))
    return cases


CASES = _build_cases()
BY_NAME = {c.name: c for c in CASES}
assert len(BY_NAME) == len(CASES)


def trace_case(oracle, case):
    """The oracle's decision trace of every subframe of a case: dicts with `stream`, `frame` and `level` added."""
    out = []
    fn, nch = (oracle.stream_trace_i64, 2) if case.is_int64 else (oracle.stream_trace, 1)
    for s in range(case.x.shape[0]):
        for k, r in enumerate(fn(case.x[s], case.level)):
            r.update(stream=s, frame=k // nch, level=case.level)
            out.append(r)
    return out
