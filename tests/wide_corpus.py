"""Wide stores: very many streams of one short frame each (a short chunk of a focal plane of 10^4 .. 10^5 detectors).

Builders only: nothing here calls the library, the oracle or the GPU.  tests/test_wide_corpus.py asserts on the CPU that
every geometry of GEOMETRIES crosses the threshold it names; tests/test_gpu_wide.py sends them through the device paths.

`wide_rows(n_stream, n, wide, seed)`: row s is `s` itself plus a sawtooth and noise whose amplitude is s % AMP_PERIOD bits
(0 bits .. 30 bits; AMP_PERIOD = 31 is odd, so the cycle is co-prime to 1024, 65 536 and 131 072 and no
power-of-two aliasing of the stream index maps a row onto one of its own class).  Sample 0 of every row is `s` exactly:
rows are pairwise distinct whatever the noise does, also rows of ONE sample.  Every 97th row is constant, every 101st is
uniform over the whole int32 range behind its first sample (VERBATIM).  The int64 form adds (s + a few bits of noise) << 32
to every 7th row: both channels carry a signal there, one does elsewhere.

Every value is a pure function of (s, i, seed) in wrapping int64 arithmetic, written against the array module it is handed
(numpy or torch): the geometry that is too large for a host copy is generated on the device with the same function, and
any of its rows can be made again on the host (`rows=`).
"""
import numpy as np

AMP_PERIOD = 31  # amplitude classes: 0 .. 30 bits
CONST_EVERY, FULL_EVERY, HIGH_EVERY = 97, 101, 7
_M32 = 0xFFFFFFFF


def _hash32(xp, s, i, seed):
    """A 32-bit mix of (s, i, seed) as non-negative int64; products wrap in int64, the low 32 bits are kept."""
    h = (s * 0x9E3779B1 + i * 0x85EBCA77 + (int(seed) * 0xC2B2AE3D + 0x27D4EB2F) % (1 << 31)) & _M32
    h = h ^ (h >> 15)
    h = (h * 0x2C1B3C6D) & _M32
    h = h ^ (h >> 12)
    h = (h * 0x297A2D39) & _M32
    return h ^ (h >> 15)


def wide_rows(n_stream, n, wide=False, seed=0, rows=None, xp=np, device=None):
    """The (n_stream, n) corpus as int32 (wide: int64), or its rows `rows` (a 1-D integer array) only.  xp: numpy, or torch
    with `device`."""
    if xp is np:
        s = np.arange(n_stream, dtype=np.int64) if rows is None else np.asarray(rows, dtype=np.int64)
        step = max(1, (1 << 18) // n)
        if s.size > step:  # in blocks of rows: a dozen int64 temporaries of the block, not of the array
            out = np.empty((s.size, n), dtype=np.int64 if wide else np.int32)
            for lo in range(0, s.size, step):
                out[lo : lo + step] = wide_rows(n_stream, n, wide, seed, rows=s[lo : lo + step])
            return out
        i = np.arange(n, dtype=np.int64)
        where, i32, i64 = np.where, np.int32, np.int64
        cast = lambda a, dt: a.astype(dt)  # noqa: E731
    else:
        s = xp.arange(n_stream, dtype=xp.int64, device=device) if rows is None else xp.as_tensor(np.asarray(rows, dtype=np.int64), device=device)
        i = xp.arange(n, dtype=xp.int64, device=device)
        where, i32, i64 = xp.where, xp.int32, xp.int64
        cast = lambda a, dt: a.to(dt)  # noqa: E731
    s, i = s[:, None], i[None, :]
    bits = s % AMP_PERIOD
    h = _hash32(xp, s, i, seed)
    signed = h - ((h >> 31) << 32)  # the 32 bits as a signed value
    noise = where(bits > 0, signed >> (32 - bits), signed * 0)  # [-2^(bits-1), 2^(bits-1))
    ramp = ((i * (1 + s % 13)) % 128 - 64) << where(bits > 6, bits - 6, bits * 0)  # |ramp| <= 2^30: a predictable part
    x = s + noise + where(bits > 6, ramp, ramp * 0)
    x = where(s % FULL_EVERY == 0, signed, x)
    x = where(s % CONST_EVERY == 0, s + i * 0, x)
    x = where(i == 0, s + i * 0, x)
    if not wide:
        return cast(x, i32)
    quiet = (i == 0) | (s % CONST_EVERY == 0)
    hi = s + where(quiet, i * 0, _hash32(xp, s, i, seed + 1) >> 27)  # s plus 5 bits of noise in the high word
    return cast(x + where(s % HIGH_EVERY == 0, hi << 32, hi * 0), i64)


def wide_floats(n_stream, n, dtype, seed=0):
    """Floats whose quantised integers are as varied as the integer corpus: its rows times 1e-3 (row s starts with s / 1000:
    pairwise distinct in float32 too)."""
    return (wide_rows(n_stream, n, False, seed) * 1e-3).astype(dtype)


def wide_quanta(n_stream, dtype):
    return (1e-3 * (1 + np.arange(n_stream) % 7)).astype(dtype)


def block_size(level):
    return 1152 if level <= 2 else 4096


# The literals of flacarray_amd/csrc/flacarray_hip.hip (and encode_placed.hpp) that the geometries are sized against.  If
# one of them is changed, change it here and the shapes with it: tests/test_wide_corpus.py asserts the arithmetic.
SCAN_THREADS = 1024        # starts_scan_kernel: one block of 1024 threads walks n_stream in passes of 1024 with a carry
K5_MAXBLK, K5_WAVES = 32768, 4  # FA_K5_MAXBLK: compact_frames_kernel's grid cap, 4 frames (waves) per block; K3F's tail compaction too
QUANT_MAXBLK, QUANT_PER_BLOCK = 16384, 1024  # quantise_rows_kernel: min(16384, (n_stream * n + 1023) / 1024) blocks
FILL_MAXGRID = 1 << 20     # fill_ranges_kernel
LATENCY_MAX_TASKS = 4096   # latency_allowed: K7L takes launches of at most 4096 frames
BESIDE_MIN_TASKS = 16384   # decode_device_impl: `a.n_tasks >= 16384` sends the frame check beside K7
PLACED_BELOW = 4096        # kPlacedBelowFrames: K3G below 4096 frames (1024 when every frame is whole)
PLACED_GRID = 2048         # kPlacedGrid (encode_placed.hpp): K3G's persistent grid

# name -> cases (shape, dtype, level); `crosses` names the threshold and the code site, the test module asserts it
GEOMETRIES = {
    "scan3": dict(
        cases=[((2051, 37), "i32", 1), ((2051, 37), "i32", 5), ((2051, 37), "i64", 1), ((2051, 37), "i64", 5),
               ((2051, 3 * 1152 + 11), "i32", 1), ((2051, 3 * 4096 + 11), "i32", 5),
               ((2051, 3 * 1152 + 11), "i64", 1), ((2051, 3 * 4096 + 11), "i64", 5)],
        crosses="2051 = 2 * 1024 + 3: two carries and a ragged third pass of starts_scan_kernel (encode_kernels.hpp) at every caller: "
                "slot sequence, splice, reindex, window, join (flacarray_hip.hip); 2051 one-frame streams <= 4096 tasks: K7L; F >= 1024"),
    "u16": dict(
        cases=[((70001, 19), "i32", 1), ((70001, 19), "i32", 5)],
        crosses="stream index > 65 535; 70 001 % 256 != 0: ragged last block of every (n_stream + 255) / 256 grid; 70 001 > 16 384 tasks: "
                "frame check beside K7 (decode_device_impl)"),
    "k5cap": dict(
        cases=[((131075, 16), "i32", 0), ((131075, 16), "i32", 5), ((131075, 8), "i64", 0), ((131075, 8), "i64", 5)],
        crosses="F = 131 075 > 4 * FA_K5_MAXBLK = 131 072: second trip of compact_frames_kernel's grid-stride loop under FLACARRAY_HIP_SLOTS=1 "
                "(encode_device_finish); 131 075 K3G tickets on a grid of 2048; stream index > 2^17"),
    "ones": dict(
        cases=[((300000, 1), "i32", 5), ((300000, 4), "i32", 5)],
        crosses="one-sample CONSTANT frames and <= 4-sample VERBATIM frames only; stream index > 2^18"),
    "k3f_wide": dict(
        cases=[((16389, 4096), "i32", 5), ((16389, 4096), "i32", 8), ((16389, 4096), "f32", 5)],
        crosses="whole 4096-sample frames, F = 16 389 >= 1024: K3F (placed_preferred) with ONE frame per stream: the scanner adds the "
                "stream header's bytes in front of every frame, fused_finish_kernel runs per stream; 16 389 >= 16 384 tasks in K7"),
    "k3f_tailcap": dict(
        cases=[((131075, 8196), "i32", 5)],
        crosses="8196 = 2 * 4096 + 4: K3F with a short last frame per stream: tail encoder grid = n_stream, (n_stream + 3) / 4 = 32 769 > "
                "32 768: second trip of the tail compaction (fused_encode_run)"),
    "qcap": dict(
        cases=[((70001, 241), "f32", 5), ((70001, 241), "f64", 5)],
        crosses="70 001 * 241 > 16 384 * 1024 samples: second trip of quantise_rows_kernel (append / overwrite of floats on float stores)"),
}

# the streams whose encoder decisions, damage and bytes the device tests look at one by one: the ends, and both sides of
# every power of two that a truncated, wrapped or carried stream index would fold
BOUNDARY_STREAMS = (0, 1, 1023, 1024, 2047, 2048, 65535, 65536, 131071, 131072, 131073, 262143, 262144)


def boundary_streams(n_stream):
    return sorted({s for s in BOUNDARY_STREAMS if s < n_stream} | {n_stream - 2, n_stream - 1})


def strip_seektables(blob, starts, nbytes, nf):
    """The store without its SEEKTABLEs (fLaC, STREAMINFO marked last, frames) in one vectorised pass: every stream of this
    library's layout with nf frames has the same 46 + 18 nf header bytes, of which the first 42 stay."""
    blob, starts, nbytes = np.asarray(blob), np.asarray(starts, dtype=np.int64).reshape(-1), np.asarray(nbytes, dtype=np.int64).reshape(-1)
    cut = 4 + 18 * nf
    assert np.all(blob[starts + 42] == 0x83) and np.all(blob[starts + 4] == 0)
    delta = np.zeros(blob.size + 1, dtype=np.int8)
    delta[starts + 42] -= 1
    delta[starts + 42 + cut] += 1
    keep = (np.cumsum(delta[:-1], dtype=np.int64) == 0)
    new_nb = nbytes - cut
    new_st = np.concatenate([[0], np.cumsum(new_nb)[:-1]]).astype(np.int64)
    out = blob[keep]
    out[new_st + 4] = 0x80
    return out, new_st, new_nb
