"""ctypes loader for the CPU oracle (oracle/flac_oracle.c).

TEST INFRASTRUCTURE ONLY: imported by tests/, __graft_entry__.smoke() and the cpu_baseline leg
of bench.py.  Nothing under flacarray_amd/ may import this module.
"""
import ctypes
import os
import subprocess

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
_LIB = None


class FrameInfo(ctypes.Structure):
    _fields_ = [
        ("type", ctypes.c_int32),
        ("order", ctypes.c_int32),
        ("porder", ctypes.c_int32),
        ("wasted", ctypes.c_int32),
        ("shift", ctypes.c_int32),
        ("precision", ctypes.c_int32),
        ("nbytes", ctypes.c_int32),
        ("blocksize", ctypes.c_int32),
    ]


class TraceRec(ctypes.Structure):
    """oracle_trace_rec: FrameInfo's fields plus the cause of every encoder decision (flac_oracle.c)."""

    _fields_ = [(k, ctypes.c_int32) for k in (
        "type", "order", "porder", "wasted", "shift", "precision", "nbytes", "blocksize", "bps", "is_const", "fixed_valid",
        "fixed_order", "lpc_tried", "lpc_drop", "quant_rc", "lev_usable", "lev_neg", "lev_zero", "lpc_order", "prec_before",
        "prec_after", "raw_shift", "clamp_qmax", "clamp_qmin", "cand_type", "rice_min", "rice_max", "rice2", "rice_clamp30",
        "row_over", "exact_over", "verbatim_cause", "channel", "nch", "st_fits", "st_small", "st_right_zero", "st_tried",
        "st_use_side", "st_fit_sign",
    )] + [(k, ctypes.c_int64) for k in ("st_est_left", "st_est_side", "est_bits", "exact_bits", "verbatim_bits")] + [("cmax", ctypes.c_double)]


# lpc_drop and verbatim_cause codes (the TR_LPC_* / TR_VERB_* enums of flac_oracle.c)
LPC_WON, LPC_NOT_TRIED, LPC_LAGS_ZERO, LPC_CMAX, LPC_QUANT_RC, LPC_PREC, LPC_RESIDUAL, LPC_RICE, LPC_ESTIMATE = range(9)
VERB_NONE, VERB_SHORT, VERB_NO_CANDIDATE, VERB_ROW_CAP, VERB_EXACT = range(5)


def _src_hash():
    import hashlib

    h = hashlib.sha256()
    for name in ("flac_oracle.c", "Makefile"):
        with open(os.path.join(_HERE, name), "rb") as f:
            h.update(f.read())
    return h.hexdigest()


def is_stale():
    """True when liboracle.so is missing or was built from another flac_oracle.c (a content hash
    written next to the library at build time; file times do not survive a snapshot)."""
    so = os.path.join(_HERE, "liboracle.so")
    tag = so + ".srchash"
    if not (os.path.exists(so) and os.path.exists(tag)):
        return True
    with open(tag) as f:
        return f.read().strip() != _src_hash()


def build():
    """Compile liboracle.so with gcc if it is missing or was built from other sources.

    Spawns make/gcc: call it BEFORE anything in the process touches the GPU (bench.py and smoke()
    do so at their very top, tests/conftest.py at collection time) -- lib() never builds."""
    so = os.path.join(_HERE, "liboracle.so")
    if is_stale():
        subprocess.check_call(["make", "-C", _HERE, "-s", "-B"])
        with open(so + ".srchash", "w") as f:
            f.write(_src_hash())
    return so


def lib():
    global _LIB
    if _LIB is None:
        if is_stale():
            raise RuntimeError(
                "oracle/liboracle.so is missing or stale: run oracle.build() (or __graft_entry__.build()) "
                "before any GPU work; it is never built lazily"
            )
        _LIB = load(os.path.join(_HERE, "liboracle.so"))
    return _LIB


def load(path):
    """Load a build of flac_oracle.c and declare its exports (lib() loads oracle/liboracle.so; tools/oracle_branch_coverage.py
    an instrumented build)."""
    L = ctypes.CDLL(path)
    i64, i32p, u8p = ctypes.c_int64, ctypes.POINTER(ctypes.c_int32), ctypes.POINTER(ctypes.c_uint8)
    i64p, f32p = ctypes.POINTER(ctypes.c_int64), ctypes.POINTER(ctypes.c_float)
    L.oracle_encode_i32.argtypes = [i32p, i64, i64, ctypes.c_uint32, i64p, i64p, ctypes.POINTER(u8p), ctypes.c_int]
    L.oracle_encode_i32.restype = ctypes.c_int
    L.oracle_decode_i32.argtypes = [u8p, i64p, i64p, i64, i64, i64, i64, i32p, ctypes.c_int]
    L.oracle_decode_i32.restype = ctypes.c_int
    L.oracle_float32_to_int32.argtypes = [f32p, i64, i64, f32p, i32p, f32p, f32p]
    L.oracle_float32_to_int32.restype = ctypes.c_int
    L.oracle_int32_to_float32.argtypes = [i32p, i64, i64, f32p, f32p, f32p]
    L.oracle_int32_to_float32.restype = None
    L.oracle_encode_stream_info.argtypes = [i32p, i64, ctypes.c_uint32, ctypes.POINTER(FrameInfo)]
    L.oracle_encode_stream_info.restype = ctypes.c_int
    f64p = ctypes.POINTER(ctypes.c_double)
    L.oracle_encode_i64.argtypes = [i64p, i64, i64, ctypes.c_uint32, i64p, i64p, ctypes.POINTER(u8p), ctypes.c_int]
    L.oracle_encode_i64.restype = ctypes.c_int
    L.oracle_decode_i64.argtypes = [u8p, i64p, i64p, i64, i64, i64, i64, i64p, ctypes.c_int]
    L.oracle_decode_i64.restype = ctypes.c_int
    L.oracle_float64_to_int64.argtypes = [f64p, i64, i64, f64p, i64p, f64p, f64p]
    L.oracle_float64_to_int64.restype = ctypes.c_int
    L.oracle_int64_to_float64.argtypes = [i64p, i64, i64, f64p, f64p, f64p]
    L.oracle_int64_to_float64.restype = None
    L.oracle_encode_stream_info_i64.argtypes = [i64p, i64, ctypes.c_uint32, ctypes.POINTER(FrameInfo)]
    L.oracle_encode_stream_info_i64.restype = ctypes.c_int
    L.oracle_encode_stream_trace.argtypes = [i32p, i64, ctypes.c_uint32, ctypes.POINTER(TraceRec)]
    L.oracle_encode_stream_trace.restype = ctypes.c_int
    L.oracle_encode_stream_trace_i64.argtypes = [i64p, i64, ctypes.c_uint32, ctypes.POINTER(TraceRec)]
    L.oracle_encode_stream_trace_i64.restype = ctypes.c_int
    L.oracle_trace_rec_size.restype = ctypes.c_int
    assert L.oracle_trace_rec_size() == ctypes.sizeof(TraceRec)
    L.oracle_free.argtypes = [ctypes.c_void_p]
    L.oracle_tukey_window.argtypes = [ctypes.c_int, f32p]
    L.oracle_det_log2.argtypes = [ctypes.c_double]
    L.oracle_det_log2.restype = ctypes.c_double
    L.oracle_num_threads.restype = ctypes.c_int
    L.oracle_set_threads.argtypes = [ctypes.c_int]
    L.oracle_set_threads.restype = None
    return L


def _p(a, t):
    return a.ctypes.data_as(ctypes.POINTER(t))


def encode_i32(data, level=5, use_threads=False, _dtype=np.int32):
    """(blob uint8, starts int64[n_stream], nbytes int64[n_stream]) for a 2-D C-contiguous int32 array."""
    data = np.ascontiguousarray(data, dtype=_dtype)
    if data.ndim == 1:
        data = data.reshape(1, -1)
    n_stream, stream_size = data.shape
    starts = np.zeros(n_stream, dtype=np.int64)
    n_bytes = ctypes.c_int64(0)
    raw = ctypes.POINTER(ctypes.c_uint8)()
    fn, ct = (lib().oracle_encode_i32, ctypes.c_int32) if _dtype == np.int32 else (lib().oracle_encode_i64, ctypes.c_int64)
    err = fn(
        _p(data, ct), n_stream, stream_size, level, ctypes.byref(n_bytes), _p(starts, ctypes.c_int64),
        ctypes.byref(raw), int(use_threads),
    )
    if err != 0:
        raise RuntimeError(f"Encoding failed, return code = {err}")
    blob = np.ctypeslib.as_array(raw, shape=(n_bytes.value,)).copy()
    lib().oracle_free(raw)
    nbytes = np.empty(n_stream, dtype=np.int64)
    nbytes[:-1] = np.diff(starts)
    nbytes[-1] = n_bytes.value - starts[-1]
    return blob, starts, nbytes


def encode_i64(data, level=5, use_threads=False):
    """Two-channel streams for a 2-D int64 array (channel 0 = low words, channel 1 = high words)."""
    return encode_i32(data, level, use_threads, _dtype=np.int64)


def decode_i64(blob, starts, nbytes, stream_size, first=-1, last=-1, use_threads=False):
    return decode_i32(blob, starts, nbytes, stream_size, first, last, use_threads, _dtype=np.int64)


def decode_i32(blob, starts, nbytes, stream_size, first=-1, last=-1, use_threads=False, _dtype=np.int32):
    blob = np.ascontiguousarray(blob, dtype=np.uint8)
    starts = np.ascontiguousarray(starts, dtype=np.int64).reshape(-1)
    nbytes = np.ascontiguousarray(nbytes, dtype=np.int64).reshape(-1)
    n_stream = starts.shape[0]
    n_decode = stream_size if (first < 0 or last < 0) else last - first
    out = np.empty((n_stream, max(n_decode, 0)), dtype=_dtype)
    fn, ct = (lib().oracle_decode_i32, ctypes.c_int32) if _dtype == np.int32 else (lib().oracle_decode_i64, ctypes.c_int64)
    err = fn(
        _p(blob, ctypes.c_uint8), _p(starts, ctypes.c_int64), _p(nbytes, ctypes.c_int64), n_stream, stream_size,
        first, last, _p(out, ct), int(use_threads),
    )
    if err != 0:
        raise RuntimeError(f"Decoding failed, return code = {err}")
    return out


def float32_to_int32(data, quanta=None):
    data = np.ascontiguousarray(data, dtype=np.float32)
    if data.ndim == 1:
        data = data.reshape(1, -1)
    n_stream, stream_size = data.shape
    out = np.empty_like(data, dtype=np.int32)
    offsets = np.empty(n_stream, dtype=np.float32)
    gains = np.empty(n_stream, dtype=np.float32)
    qp = None
    if quanta is not None:
        quanta = np.ascontiguousarray(quanta, dtype=np.float32).reshape(-1)
        assert quanta.shape[0] == n_stream
        qp = _p(quanta, ctypes.c_float)
    lib().oracle_float32_to_int32(
        _p(data, ctypes.c_float), n_stream, stream_size, qp, _p(out, ctypes.c_int32), _p(offsets, ctypes.c_float),
        _p(gains, ctypes.c_float),
    )
    return out, offsets, gains


def int32_to_float32(idata, offsets, gains):
    idata = np.ascontiguousarray(idata, dtype=np.int32)
    if idata.ndim == 1:
        idata = idata.reshape(1, -1)
    n_stream, stream_size = idata.shape
    offsets = np.ascontiguousarray(offsets, dtype=np.float32).reshape(-1)
    gains = np.ascontiguousarray(gains, dtype=np.float32).reshape(-1)
    out = np.empty(idata.shape, dtype=np.float32)
    lib().oracle_int32_to_float32(
        _p(idata, ctypes.c_int32), n_stream, stream_size, _p(offsets, ctypes.c_float), _p(gains, ctypes.c_float),
        _p(out, ctypes.c_float),
    )
    return out


def float64_to_int64(data, quanta=None):
    data = np.ascontiguousarray(data, dtype=np.float64)
    if data.ndim == 1:
        data = data.reshape(1, -1)
    n_stream, stream_size = data.shape
    out = np.empty(data.shape, dtype=np.int64)
    offsets = np.empty(n_stream, dtype=np.float64)
    gains = np.empty(n_stream, dtype=np.float64)
    qp = None
    if quanta is not None:
        quanta = np.ascontiguousarray(quanta, dtype=np.float64).reshape(-1)
        assert quanta.shape[0] == n_stream
        qp = _p(quanta, ctypes.c_double)
    lib().oracle_float64_to_int64(
        _p(data, ctypes.c_double), n_stream, stream_size, qp, _p(out, ctypes.c_int64), _p(offsets, ctypes.c_double),
        _p(gains, ctypes.c_double),
    )
    return out, offsets, gains


def int64_to_float64(idata, offsets, gains):
    idata = np.ascontiguousarray(idata, dtype=np.int64)
    if idata.ndim == 1:
        idata = idata.reshape(1, -1)
    n_stream, stream_size = idata.shape
    offsets = np.ascontiguousarray(offsets, dtype=np.float64).reshape(-1)
    gains = np.ascontiguousarray(gains, dtype=np.float64).reshape(-1)
    out = np.empty(idata.shape, dtype=np.float64)
    lib().oracle_int64_to_float64(
        _p(idata, ctypes.c_int64), n_stream, stream_size, _p(offsets, ctypes.c_double), _p(gains, ctypes.c_double),
        _p(out, ctypes.c_double),
    )
    return out


def stream_info_i64(x, level=5):
    """Per-SUBFRAME encoder decisions for one 1-D int64 stream: entry [2 * frame + channel]."""
    x = np.ascontiguousarray(x, dtype=np.int64).reshape(-1)
    bs = 1152 if level <= 2 else 4096
    nf = (x.shape[0] + bs - 1) // bs
    infos = (FrameInfo * (2 * nf))()
    err = lib().oracle_encode_stream_info_i64(_p(x, ctypes.c_int64), x.shape[0], level, infos)
    if err != 0:
        raise RuntimeError(f"Encoding failed, return code = {err}")
    return [{k: getattr(i, k) for k, _ in FrameInfo._fields_} for i in infos]


def stream_info(x, level=5):
    """Per-frame encoder decisions for one 1-D int32 stream (list of dicts)."""
    x = np.ascontiguousarray(x, dtype=np.int32).reshape(-1)
    bs = 1152 if level <= 2 else 4096
    nf = (x.shape[0] + bs - 1) // bs
    infos = (FrameInfo * nf)()
    err = lib().oracle_encode_stream_info(_p(x, ctypes.c_int32), x.shape[0], level, infos)
    if err != 0:
        raise RuntimeError(f"Encoding failed, return code = {err}")
    return [{k: getattr(i, k) for k, _ in FrameInfo._fields_} for i in infos]


def _stream_trace(x, level, nch):
    x = np.ascontiguousarray(x, dtype=np.int64 if nch == 2 else np.int32).reshape(-1)
    bs = 1152 if level <= 2 else 4096
    nf = (x.shape[0] + bs - 1) // bs
    recs = (TraceRec * (nch * nf))()
    if nch == 2:
        err = lib().oracle_encode_stream_trace_i64(_p(x, ctypes.c_int64), x.shape[0], level, recs)
    else:
        err = lib().oracle_encode_stream_trace(_p(x, ctypes.c_int32), x.shape[0], level, recs)
    if err != 0:
        raise RuntimeError(f"Encoding failed, return code = {err}")
    return [{k: getattr(r, k) for k, _ in TraceRec._fields_} for r in recs]


def stream_trace(x, level=5):
    """Per-frame decision trace of one 1-D int32 stream: stream_info's keys plus the cause of each decision."""
    return _stream_trace(x, level, 1)


def stream_trace_i64(x, level=5):
    """Per-SUBFRAME decision trace of one 1-D int64 stream: entry [2 * frame + channel]."""
    return _stream_trace(x, level, 2)


def tukey_window(n):
    w = np.empty(n, dtype=np.float32)
    lib().oracle_tukey_window(n, _p(w, ctypes.c_float))
    return w
