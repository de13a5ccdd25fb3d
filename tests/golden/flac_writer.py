"""Seeded writer of libFLAC-shaped native-FLAC streams (RFC 9639) for the decoder sweeps.

The input is the samples: every frame is coded from them with coding choices drawn at random over what the format
allows and libFLAC writes -- CONSTANT, VERBATIM, FIXED 0-4 and LPC 1-32 subframes, least-squares LPC coefficients
quantised at precision 2-15 and shift 0-15, wasted bits, partition orders up to 8, per partition the best Rice
parameter, a deliberately small one (unary codes past 32 bits), parameter 0 or an escape of width 0-31, Rice and
Rice2 -- and assembled with the field-by-field helpers of make_golden.py.  Predictors run on exact integers (numpy
int64 under an asserted bound of 2^53, far inside its range; the residuals are handed over as Python ints), every
residual fits in signed 32 bits as libFLAC guarantees.  Nothing here shares code with oracle/ or flacarray_amd/.

Every stream comes with a coverage record (`features`, a Counter of what its frames contain), so the tests can assert
that a sweep reached each feature instead of assuming it.
"""
import hashlib
from collections import Counter

import numpy as np

from .make_golden import frame, residual, sbits, stream, ubits, utf8

BLOCK_SIZES = (16, 192, 576, 1000, 1152, 4095, 4096, 4608, 8192, 16384, 65535)
LAYOUTS = ("libflac", "own", "placeholder", "sparse", "padded")
FIXED = {0: [], 1: [1], 2: [2, -1], 3: [3, -3, 1], 4: [4, -6, 4, -1]}
ORDER_BUCKETS = ((1, 8), (9, 12), (13, 16), (17, 32))
I32_MIN, I32_MAX = -(2**31), 2**31 - 1
VENDOR = b"reference libFLAC 1.4.3 20230623"
PLACEHOLDER = 0xFFFFFFFFFFFFFFFF


def order_bucket(order):
    for lo, hi in ORDER_BUCKETS:
        if lo <= order <= hi:
            return "%d-%d" % (lo, hi)
    raise ValueError(order)


def _signed_width(v):
    """Bits of the smallest two's-complement field that holds every value of v (0 for all zeros)."""
    lo, hi = int(v.min()), int(v.max())
    if lo == 0 and hi == 0:
        return 0
    return max(hi.bit_length(), (~lo).bit_length()) + 1


def _trailing_zeros(x):
    nz = x[x != 0]
    if nz.size == 0:
        return 64
    acc = int(np.bitwise_or.reduce(nz))
    return (acc & -acc).bit_length() - 1


def _predict(y, order, coefs, shift):
    """Exact prediction sums and residuals (int64: |c| < 2^15, |y| <= 2^32, order <= 32, so |sum| < 2^52)."""
    n = y.size
    c = np.asarray(coefs, dtype=np.int64)
    s = np.zeros(n - order, dtype=np.int64)
    for j in range(order):
        s += c[j] * y[order - 1 - j : n - 1 - j]
    return s, y[order:] - (s >> shift)


def _lpc_coefs(rng, y, order):
    """Least-squares predictor of y, quantised at a drawn precision and shift.  Half the time the shift is libFLAC's
    choice (the largest that keeps the largest coefficient inside the precision, at most 15), else any of 0-15."""
    n = y.size
    yf = y.astype(np.float64)
    a = np.stack([yf[order - 1 - j : n - 1 - j] for j in range(order)], axis=1)
    c = np.linalg.lstsq(a, yf[order:], rcond=None)[0] if n > order else np.zeros(order)
    c = np.nan_to_num(c)
    if rng.random() < 0.12:
        # alternating near-full-scale coefficients: on a smooth signal the terms cancel, so the residual stays small
        # while the partial sums of the prediction grow towards 2^51
        k = (1 << 14) - 1 - int(rng.integers(0, 64))
        return [k if j % 2 == 0 else -k for j in range(order)], 15, int(rng.integers(12, 16))
    prec = int(rng.integers(2, 16))
    cmax = float(np.max(np.abs(c)))
    if rng.random() < 0.5 and cmax > 0:
        shift = int(np.clip(prec - 2 - int(np.floor(np.log2(cmax))), 0, 15))
    else:
        shift = int(rng.integers(0, 16))
    lim = 1 << (prec - 1)
    q = np.clip(np.rint(c * (1 << shift)), -lim, lim - 1).astype(np.int64)
    return q.tolist(), prec, shift


def _best_k(u, kmax):
    n = u.size
    if n == 0:
        return 0
    cost = [n * (k + 1) + int((u >> k).sum()) for k in range(kmax + 1)]
    return int(np.argmin(cost))


def _residual_bits(rng, res, order, bs, feats, max_porder=8):
    """Partitioning and per-partition coding of one residual, drawn at random; returns the bit string."""
    po_max = 0
    for po in range(1, max_porder + 1):
        if bs % (1 << po) == 0 and (bs >> po) >= order:
            po_max = po
    po = int(rng.integers(0, po_max + 1)) if rng.random() < 0.6 else po_max
    ps = bs >> po
    u = np.where(res >= 0, res << 1, ((-res) << 1) - 1)
    params = []
    i = 0
    for p in range(1 << po):
        n = ps - order if p == 0 else ps
        up, rp = u[i : i + n], res[i : i + n]
        i += n
        best = _best_k(up, 30)
        mode = rng.random()
        umax = int(up.max()) if n else 0
        par = best
        if mode < 0.45:
            pass
        elif mode < 0.65:
            cap = int(rng.integers(40, 160))  # a parameter small enough for codes past 32 bits, bounded in length
            k = best
            while k > 0 and (umax >> (k - 1)) <= cap:
                k -= 1
            par = k
        elif mode < 0.75:
            if umax <= 160:
                par = 0
        else:
            w = _signed_width(rp) if n else 0
            if w <= 31:
                par = ("esc", w if rng.random() < 0.5 else int(rng.integers(w, 32)))
        params.append(par)
        if isinstance(par, tuple):
            feats["esc_width_%d" % par[1]] += 1
        else:
            feats["rice_param_%s" % ("0" if par == 0 else "gt14" if par > 14 else "1-14")] += 1
            if n and (umax >> par) > 32:
                feats["long_code"] += 1
    rice2 = any(not isinstance(k, tuple) and k > 14 for k in params) or rng.random() < 0.3
    feats["rice2" if rice2 else "rice"] += 1
    feats["porder_%d" % po] += 1
    return residual(res.tolist(), order, po, params, bs, rice2=rice2)


def _order_draw(rng, bs, bucket=None):
    lo, hi = ORDER_BUCKETS[int(rng.integers(0, 4)) if bucket is None else bucket]
    hi = min(hi, bs - 1)
    lo = min(lo, hi)
    return int(rng.integers(lo, hi + 1))


def code_channel(rng, x, bps, feats, kinds=None, bucket=None):
    """Subframe of one channel (`x`: int64 samples that fit in `bps` bits, bps 32 or 33) with drawn coding choices;
    returns a make_golden description carrying the assembled bits."""
    bs = x.size
    tz = min(_trailing_zeros(x), bps - 1)
    wasted = int(rng.integers(1, tz + 1)) if tz > 0 and rng.random() < 0.75 else 0
    y = x >> wasted
    b = bps - wasted
    head = lambda tc: "0" + ubits(tc, 6) + ("1" + "0" * (wasted - 1) + "1" if wasted else "0")  # noqa: E731
    if wasted:
        feats["wasted"] += 1
    const = bool(np.all(y == y[0]))
    if kinds is None:
        kinds = ("const",) if const and rng.random() < 0.7 else ("verbatim", "fixed", "lpc", "lpc", "lpc", "lpc", "fixed")
    for attempt in range(6):
        kind = kinds[int(rng.integers(0, len(kinds)))] if attempt < 5 else "verbatim"
        if kind == "const" and not const:
            kind = "verbatim"
        if kind == "const":
            feats["const"] += 1
            return {"bits": head(0) + sbits(int(y[0]), b)}
        if kind == "verbatim" or bs < 2:
            feats["verbatim"] += 1
            return {"bits": head(1) + "".join(sbits(v, b) for v in y.tolist())}
        if kind == "fixed":
            order = int(rng.integers(0, min(4, bs - 1) + 1))
            coefs, shift, tc, qlp = FIXED[order], 0, 8 + order, ""
        else:
            order = _order_draw(rng, bs, bucket)
            coefs, prec, shift = _lpc_coefs(rng, y, order)
            tc = 32 + order - 1
            qlp = ubits(prec - 1, 4) + sbits(shift, 5) + "".join(sbits(c, prec) for c in coefs)
        sums, res = _predict(y, order, coefs, shift)
        if res.size and (res.min() < I32_MIN or res.max() > I32_MAX):
            feats["redrawn"] += 1
            continue
        if kind == "fixed":
            feats["fixed_%d" % order] += 1
        else:
            feats["lpc"] += 1
            feats["lpc_order_" + order_bucket(order)] += 1
            feats["lpc_prec_%d" % prec] += 1
            feats["lpc_shift_%d" % shift] += 1
            # the largest sum of |c_j x_(i-1-j)| over the frame bounds every partial sum a decoder forms
            terms = np.zeros(max(bs - order, 0), dtype=np.int64)
            for j, c in enumerate(coefs):
                terms += abs(c) * np.abs(y[order - 1 - j : bs - 1 - j])
            if terms.size and int(terms.max()) >= 2**48:
                feats["lpc_terms_ge_2^48"] += 1
            if bps == 33 and order > 12:
                feats["side_lpc_order_gt12"] += 1
        bits = head(tc) + "".join(sbits(v, b) for v in y[:order].tolist()) + qlp + _residual_bits(rng, res, order, bs, feats)
        return {"bits": bits}
    raise AssertionError("unreachable")


def _segment(rng, n, amp_bits=None):
    """Samples of one frame: one of a few signal families, sometimes scaled by 2^w (wasted bits)."""
    kind = rng.choice(["smooth", "smooth", "walk", "noise", "steps", "const", "full"])
    w = int(rng.integers(1, 9)) if rng.random() < 0.25 else 0
    if amp_bits is None:
        amp_bits = 30.9 if rng.random() < 0.3 else rng.uniform(3, 31)
    a = 2.0**amp_bits / (1 << w)
    t = np.arange(n)
    if kind == "smooth":
        f = rng.uniform(1e-3, 0.2, 3)
        x = a * 0.45 * (np.sin(f[0] * t + rng.uniform(0, 6)) + 0.5 * np.sin(f[1] * t) + 0.1 * np.sin(f[2] * t))
        x += rng.normal(0, max(1.0, a * 10.0 ** rng.uniform(-7, -2)), n)
    elif kind == "walk":
        x = np.cumsum(rng.normal(0, max(1.0, a / max(np.sqrt(n), 1) / 4), n))
    elif kind == "noise":
        x = rng.uniform(-a, a, n)
    elif kind == "steps":
        edges = np.sort(rng.integers(0, n, 3))
        x = np.zeros(n) + rng.uniform(-a, a)
        for e in edges:
            x[e:] += rng.uniform(-a, a) / 2
    elif kind == "const":
        x = np.full(n, rng.uniform(-a, a))
    else:
        x = rng.uniform(-(2.0**31), 2.0**31, n) / (1 << w)
    x = np.clip(np.rint(x), -(2**31) // (1 << w), (2**31 - 1) // (1 << w)).astype(np.int64)
    return x << w


def _stereo_segment(rng, n):
    left = _segment(rng, n)
    mode = rng.random()
    if mode < 0.2:  # left near +2^31, right near -2^31: the side channel needs its 33rd bit
        t = np.arange(n)
        left = (2**31 - 4000 + np.rint(1500 * np.sin(t / rng.uniform(3, 40)))).astype(np.int64) + rng.integers(-3, 4, n)
        right = (-(2**31) + 4000 + np.rint(1500 * np.cos(t / rng.uniform(3, 40)))).astype(np.int64) + rng.integers(-3, 4, n)
    elif mode < 0.6:  # correlated channels
        right = np.clip(np.rint(left * rng.uniform(-1, 1)) + _segment(rng, n, amp_bits=rng.uniform(2, 16)), I32_MIN, I32_MAX).astype(np.int64)
    else:
        right = _segment(rng, n)
    return left, right


def _vorbis():
    return len(VENDOR).to_bytes(4, "little") + VENDOR + (0).to_bytes(4, "little")


def _seek_point(sample, offset, count):
    return sample.to_bytes(8, "big") + offset.to_bytes(8, "big") + count.to_bytes(2, "big")


def _metadata(rng, layout, frames, block, n):
    offs = np.concatenate([[0], np.cumsum([len(f) for f in frames])[:-1]]).astype(np.int64).tolist()
    nf = len(frames)
    real = lambda f: _seek_point(f * block, offs[f], min(block, n - f * block))  # noqa: E731
    if layout == "libflac":
        return [(4, _vorbis())]
    if layout == "own":
        return [(3, b"".join(real(f) for f in range(nf)))]
    if layout == "placeholder":
        total = nf if rng.random() < 0.7 else nf + int(rng.integers(1, 4))  # as many points as frames: the tempting case
        k = int(rng.integers(0, nf)) if nf > 1 else 0
        pts = [real(f) for f in range(k)] + [_seek_point(PLACEHOLDER, 0, 0)] * (total - k)
        return [(3, b"".join(pts)), (4, _vorbis())]
    if layout == "sparse":
        return [(3, b"".join(real(f) for f in range(0, nf, 10))), (4, _vorbis())]
    if layout == "padded":
        app = b"riff" + bytes(rng.integers(0, 256, int(rng.integers(0, 40)), dtype=np.uint8))
        return [(4, _vorbis()), (2, app), (3, b"".join(real(f) for f in range(nf))), (1, bytes(int(rng.integers(0, 300))))]
    raise ValueError(layout)


def write_stream(rng, n, block, channels=1, layout="libflac", sr_code=9, ss_code=7, kinds=None, bucket_cycle=False, cheap=False,
                 samples=None, bucket=None):
    """One stream of n samples (32 bps, 44.1 kHz, fixed block size `block`).  Mono: int32 samples.  Two channels:
    int64 samples packed as make_golden's g8-g13 (right << 32 | left as unsigned), the channel assignment drawn per
    frame.  bucket_cycle: frame f takes an LPC order from ORDER_BUCKETS[f % 4]; bucket: every frame takes one from
    ORDER_BUCKETS[bucket].  cheap: CONSTANT / VERBATIM frames of small values only.  samples (mono only): the n int32
    samples to code instead of drawn ones -- frame f codes samples[f * block : f * block + m]; the coding choices are
    still drawn.  Returns (samples, stream bytes, record)."""
    if samples is not None:
        if channels != 1 or cheap:
            raise ValueError("samples= is for one-channel streams with drawn coding")
        samples = np.asarray(samples)
        if samples.shape != (n,) or samples.dtype != np.int32:
            raise ValueError("samples= needs %d int32 samples" % n)
    feats = Counter()
    sr_value = {12: 44, 13: 44100, 14: 4410}.get(sr_code, 0)
    frames, chans = [], []
    nf = (n + block - 1) // block
    for f in range(nf):
        m = min(block, n - f * block)
        bk = f % 4 if bucket_cycle else bucket
        kk = ("lpc",) if bk is not None else kinds
        if cheap:
            v = int(rng.integers(-1000, 1000))
            if rng.random() < 0.9:
                x = np.full(m, v, dtype=np.int64)
            else:
                x = rng.integers(-8, 8, m).astype(np.int64) * 16 + v
            feats["const" if np.all(x == x[0]) else "verbatim"] += 1
            head = "0" + ubits(0 if np.all(x == x[0]) else 1, 6) + "0"
            sub = {"bits": head + sbits(v, 32) if np.all(x == x[0]) else head + "".join(sbits(t, 32) for t in x.tolist())}
            frames.append(frame([0] * m, f, 32, sub, ss_code=ss_code, sr_code=sr_code, sr_value=sr_value))
            chans.append((x,))
            continue
        if channels == 1:
            x = _segment(rng, m) if samples is None else samples[f * block : f * block + m].astype(np.int64)
            sub = code_channel(rng, x, 32, feats, kk, bk)
            frames.append(frame([0] * m, f, 32, sub, ss_code=ss_code, sr_code=sr_code, sr_value=sr_value))
            chans.append((x,))
        else:
            left, right = _stereo_segment(rng, m)
            asg = int(rng.choice([1, 8, 9, 10]))
            side, mid = left - right, (left + right) >> 1
            coded = {1: ((left, 32), (right, 32)), 8: ((left, 32), (side, 33)), 9: ((side, 33), (right, 32)), 10: ((mid, 32), (side, 33))}[asg]
            subs = [code_channel(rng, c, b, feats, kk, bk) for c, b in coded]
            feats["assignment_%d" % asg] += 1
            if np.abs(side).max() >= 2**31:
                feats["side_33bit"] += 1
            frames.append(frame([[0] * m, [0] * m], f, 32, subs, ss_code=ss_code, assignment=asg, sr_code=sr_code, sr_value=sr_value))
            chans.append((left, right))
    if channels == 1:
        samples = np.concatenate([c[0] for c in chans]).astype(np.int32)
        pcm = samples.astype("<i4").tobytes()
    else:
        left = np.concatenate([c[0] for c in chans])
        right = np.concatenate([c[1] for c in chans])
        samples = (right << 32) | (left & 0xFFFFFFFF)
        pcm = samples.astype("<i8").tobytes()  # = left, right interleaved as little-endian int32: libFLAC's MD5 input
    md5 = hashlib.md5(pcm).digest()
    sizes = [len(f) for f in frames]
    extra = _metadata(rng, layout, frames, block, n)
    data = stream(frames, block, 32, n, extra_blocks=extra, channels=channels, frame_sizes=(min(sizes), max(sizes)), md5=md5)
    feats["layout_" + layout] += 1
    feats["sr_code_%d" % sr_code] += 1
    feats["ss_code_%d" % ss_code] += 1
    feats["block_%d" % block] += 1
    feats["utf8_bytes_%d" % (len(utf8(nf - 1)) // 8)] += 1
    if n % block:
        feats["short_last_frame"] += 1
    rec = {"layout": layout, "block": block, "n": n, "channels": channels, "frames": nf, "features": feats}
    return samples, data, rec


def pack(streams):
    """[bytes] -> (blob uint8, starts int64, nbytes int64) of the streams back to back."""
    nb = np.array([len(s) for s in streams], dtype=np.int64)
    st = np.concatenate([[0], np.cumsum(nb)[:-1]]).astype(np.int64)
    return np.frombuffer(b"".join(streams), dtype=np.uint8).copy(), st, nb


def _batch(name, rng, count, n, block, channels, **kw):
    out = {"name": name, "block": block, "n": n, "channels": channels, "samples": [], "streams": [], "records": []}
    first = int(rng.integers(0, len(LAYOUTS)))
    fixed_layout = kw.pop("layout", None)
    for i in range(count):
        layout = fixed_layout or LAYOUTS[(first + i) % len(LAYOUTS)]
        s, d, r = write_stream(rng, n, block, channels, layout=layout, sr_code=int(rng.choice([9, 9, 12, 13, 14])),
                               ss_code=int(rng.choice([7, 0])), **kw)
        out["samples"].append(s)
        out["streams"].append(d)
        out["records"].append(r)
    out["samples"] = np.stack(out["samples"])
    return out


def sweep(seed):
    """The batches of one seed: for every block size a mono and a two-channel batch of streams that share a length
    (a decode call takes one), with drawn layouts, header codes and a short last frame."""
    rng = np.random.default_rng(seed)
    batches = []
    for channels in (1, 2):
        for block in BLOCK_SIZES:
            if block >= 8192:
                nfr, count = int(rng.integers(1, 3)), 2 if block < 65535 else 1
            else:
                nfr, count = int(rng.integers(2, max(3, 24000 // block) + 1)), 3
            if channels == 2:
                nfr, count = max(1, nfr // 2), max(1, count - 1)
            n = nfr * block + int(rng.integers(1, block))
            batches.append(_batch("s%d_%s_b%d" % (seed, "mono" if channels == 1 else "stereo", block), rng, count, n, block, channels))
    return batches


def deep_mix(seed, channels):
    """Streams whose frames cycle through LPC orders 1-8, 9-12, 13-16 and 17-32: every variant and history depth of
    the decoder meets in one call."""
    rng = np.random.default_rng(seed)
    block = 4096 if channels == 1 else 1152
    return _batch("deep_mix_%d" % channels, rng, 4, 8 * block + int(rng.integers(1, block)), block, channels, bucket_cycle=True)


def many_frames(seed, channels):
    """Block size 16 and about 2100 frames per stream: 3-byte UTF-8 frame numbers, more than 4096 frames in a call."""
    rng = np.random.default_rng(seed)
    count = 3 if channels == 1 else 2
    return _batch("many_frames_%d" % channels, rng, count, 2100 * 16 + int(rng.integers(1, 16)), 16, channels)


def utf8_4byte(seed, frames=65600):
    """One mono stream of `frames` 16-sample CONSTANT / VERBATIM frames: frame numbers from 65536 on take 4 bytes."""
    rng = np.random.default_rng(seed)
    return _batch("utf8_4byte", rng, 1, (frames - 1) * 16 + 7, 16, 1, cheap=True, layout="libflac")


def mixed_blocks(seed, n=10000):
    """Mono streams of one length and four block sizes (one decode call splits them by block size)."""
    rng = np.random.default_rng(seed)
    parts = [_batch("mix_b%d" % b, rng, 1, n, b, 1) for b in (192, 1000, 4096, 4608)]
    return {"name": "mixed_blocks", "block": None, "n": n, "channels": 1, "samples": np.concatenate([p["samples"] for p in parts]),
            "streams": sum((p["streams"] for p in parts), []), "records": sum((p["records"] for p in parts), [])}


def coverage(batches):
    c = Counter()
    for b in batches:
        for r in b["records"]:
            c.update(r["features"])
    return c


# ---- streams with one invalid field, CRC-8 and CRC-16 correct ----------------------------------------------------

def _raw_frame(sub_bits, bs, frame_no=0, blocking=0):
    """A mono 32-bit frame around a pre-assembled subframe."""
    return frame([0] * bs, frame_no, 32, {"bits": sub_bits}, blocking=blocking)


def invalid_streams():
    """[(name, stream bytes, stream size)]: each stream has exactly one field the format does not allow (or, for the
    variable-blocksize header, one the device decoder documents it does not take)."""
    bs = 64
    rng = np.random.default_rng(5)
    x = np.cumsum(rng.integers(-50, 51, bs)).tolist()
    warm = lambda k: "".join(sbits(v, 32) for v in x[:k])  # noqa: E731

    out = []
    ok = "0" + ubits(9, 6) + "0" + warm(1)  # FIXED order 1
    res1 = [x[i] - x[i - 1] for i in range(1, bs)]
    good_res = "00" + ubits(0, 4) + ubits(8, 4) + "".join(_rice(r, 8) for r in res1)
    out.append(("valid", _stream_of([_raw_frame(ok + good_res, bs)], bs), bs))
    # reserved subframe type 0b000010, followed by VERBATIM-sized content
    out.append(("reserved_type", _stream_of([_raw_frame("0" + ubits(2, 6) + "0" + "".join(sbits(v, 32) for v in x), bs)], bs), bs))
    # LPC order 1 with precision code 15 (the invalid 16-bit precision), shift 0, coefficient 1
    lpc = lambda prec_code, shift: ("0" + ubits(32, 6) + "0" + warm(1) + ubits(prec_code, 4) + sbits(shift, 5)  # noqa: E731
                                    + sbits(1, prec_code + 1) + good_res)
    out.append(("lpc_precision_15", _stream_of([_raw_frame(lpc(15, 0), bs)], bs), bs))
    out.append(("negative_shift", _stream_of([_raw_frame(lpc(11, -1), bs)], bs), bs))
    # FIXED order 4 with partition order 5: partitions of 2 samples, the first shorter than the order
    res4 = [x[i] - (4 * x[i - 1] - 6 * x[i - 2] + 4 * x[i - 3] - x[i - 4]) for i in range(4, bs)]
    short = "0" + ubits(12, 6) + "0" + warm(4) + "00" + ubits(5, 4)
    short += ubits(15, 4) + ubits(0, 5)  # partition 0: an escape of width 0 with 2 - 4 = -2 samples
    short += "".join(ubits(14, 4) + "".join(_rice(r, 14) for r in res4[2 * p - 2 : 2 * p]) for p in range(1, 32))
    out.append(("partition_shorter_than_order", _stream_of([_raw_frame(short, bs)], bs), bs))
    # variable-blocksize frame headers (the number field is the first sample's number), STREAMINFO min = max
    vb = [_raw_frame(ok + good_res, bs, frame_no=0, blocking=1), _raw_frame(ok + good_res, bs, frame_no=bs, blocking=1)]
    out.append(("variable_blocksize", _stream_of(vb, 2 * bs), 2 * bs))
    return out


def _rice(r, k):
    u = (r << 1) if r >= 0 else ((-r) << 1) - 1
    return "0" * (u >> k) + "1" + ubits(u & ((1 << k) - 1), k)


def _stream_of(frames, n):
    return stream(frames, 64, 32, n, extra_blocks=[(4, _vorbis())])



SWEEP_SEEDS = (1, 2)


def all_batches(seeds=SWEEP_SEEDS):
    """The set the tests decode: the sweep of every seed plus the special batches (deep-order mixes, 3- and 4-byte
    frame numbers, more than 4096 frames in a call, block sizes mixed in a call)."""
    out = []
    for s in seeds:
        out += sweep(s)
    return out + [deep_mix(101, 1), deep_mix(102, 2), many_frames(103, 1), many_frames(104, 2), utf8_4byte(106), mixed_blocks(105)]
