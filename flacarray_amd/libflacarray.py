"""Binding layer: the names the reference's Cython module exports, on top of the HIP C ABI.

Mirrors src/flacarray/libflacarray/libflacarray.pyx of the reference: `encode_flac` (:529),
`decode_flac` (:713), `wrap_encode_i32[_threaded]` (:285/:346), `wrap_decode_i32` (:597),
`wrap_float32_to_int32` (:113), `wrap_int32_to_float32` (:215) -- same arguments, return
shapes/dtypes and error text.  numpy in / numpy out goes through the host-pointer C entry
points; the `*_device` functions at the bottom take torch tensors already resident in HBM.

The int64 / float64 twins (`wrap_encode_i64[_threaded]` :407/:468, `wrap_decode_i64` :656,
`wrap_float64_to_int64` :164, `wrap_int64_to_float64` :250) run the two-channel variants of the
same kernels.
"""
import ctypes
import os
import sys
import threading
import weakref

import numpy as np

from . import _lib
from .scrub import FRAME_CRC16, FRAME_HEADER, FRAME_OK, FRAME_UNLOCATED, common_block_size  # noqa: F401

flac_i32_dtype = np.dtype(np.int32)
flac_i64_dtype = np.dtype(np.int64)
compressed_dtype = np.dtype(np.uint8)
offset_dtype = np.dtype(np.int64)



def _ptr(a):
    return ctypes.c_void_p(a.ctypes.data)


def _adopt_malloc(addr, n):
    """numpy view of a malloc()'d buffer that free()s it when the last view dies."""
    if n == 0:
        _lib.libc_free(addr)
        return np.zeros(0, dtype=np.uint8)
    buf = (ctypes.c_uint8 * n).from_address(addr)
    arr = np.frombuffer(buf, dtype=np.uint8)
    weakref.finalize(buf, _lib.libc_free, addr)
    return arr


class _PinnedPool:
    """Pinned, device-visible host blocks behind the numpy arrays the small-read paths return.

    A read whose samples are wanted on the host is fastest when the decoder writes them where they are going: into
    pinned memory (fa_decode_indexed_host, include/flacarray_hip.h).  A fresh numpy array is neither pinned nor present
    (its pages appear on first touch, ~19 GB/s on the benchmark host: 75 of the 250 us of a 100-slice read), so results
    from 64 KB to 64 MB come from this pool instead: power-of-two blocks, handed back when the last view of the
    array dies and kept for the next read (at most FLACARRAY_HIP_PINNED_POOL_MB, default 256, sit idle; at most
    FLACARRAY_HIP_PINNED_MAX_MB, default 1024, are out at any time -- beyond that, and whenever pinned memory is not to be
    had, the caller gets an ordinary array).  FLACARRAY_HIP_PINNED_POOL_MB=0 switches the pool off."""

    _MIN, _MAX = 65536, 64 << 20

    def __init__(self):
        self._free = {}
        self._idle = 0
        self._out = 0
        self._lock = threading.Lock()
        self._idle_limit = int(os.environ.get("FLACARRAY_HIP_PINNED_POOL_MB", "256")) << 20
        self._out_limit = int(os.environ.get("FLACARRAY_HIP_PINNED_MAX_MB", "1024")) << 20

    def _take(self, nbytes):
        cap = max(self._MIN, 1 << max(nbytes - 1, 0).bit_length())
        if self._idle_limit <= 0 or cap > self._MAX:
            return None
        with self._lock:
            if self._out + cap > self._out_limit:
                return None
            self._out += cap
            blocks = self._free.get(cap)
            if blocks:
                self._idle -= cap
                return blocks.pop(), cap
        addr = _lib.lib().fa_pinned_alloc(cap)
        if not addr:
            with self._lock:
                self._out -= cap
            return None
        return addr, cap

    def _give(self, addr, cap):
        if sys is None or sys.is_finalizing():
            return
        with self._lock:
            self._out -= cap
            if self._idle + cap <= self._idle_limit:
                self._free.setdefault(cap, []).append(addr)
                self._idle += cap
                return
        _lib.lib().fa_pinned_free(addr)

    def empty(self, n, dtype):
        """1-D array of n elements on a pinned block, or None."""
        dtype = np.dtype(dtype)
        nbytes = int(n) * dtype.itemsize
        if nbytes <= 0:
            return None
        got = self._take(nbytes)
        if got is None:
            return None
        addr, cap = got
        buf = (ctypes.c_uint8 * nbytes).from_address(addr)
        fin = weakref.finalize(buf, self._give, addr, cap)
        fin.atexit = False  # (at interpreter exit the block goes with the process)
        return np.frombuffer(buf, dtype=dtype)

    def drain(self):
        """Free the idle blocks (tests; fa_release_scratch callers)."""
        with self._lock:
            blocks = [a for lst in self._free.values() for a in lst]
            self._free.clear()
            self._idle = 0
        for a in blocks:
            _lib.lib().fa_pinned_free(a)


_pinned_pool = _PinnedPool()


def _advise_huge_pages(arr):
    """madvise(MADV_HUGEPAGE) over the 2 MB-aligned inside of a large array this module has just allocated (never on
    a caller's memory).  What bounds decode_i32 into a fresh array is the appearance of its pages (profiles/
    r03_host_abi.md: 19 GB/s in 4 KB pages, 26 GB/s in transparent huge pages on the benchmark host)."""
    if arr.nbytes < (64 << 20):
        return
    try:
        huge = 2 << 20
        lo = (arr.ctypes.data + huge - 1) & ~(huge - 1)
        hi = (arr.ctypes.data + arr.nbytes) & ~(huge - 1)
        if hi > lo:
            _lib.libc_madvise(lo, hi - lo, 14)  # MADV_HUGEPAGE; failure (no THP) changes nothing
    except Exception:  # noqa: BLE001
        pass


def wrap_float32_to_int32(flatdata, n_stream, stream_size, quanta, _f64=False):
    """libflacarray.pyx:113-161.  `quanta` is used only if len(quanta) == n_stream."""
    _lib.require_device()
    ft, it = (np.float64, np.int64) if _f64 else (np.float32, np.int32)
    flatdata = np.ascontiguousarray(flatdata, dtype=ft)
    size = n_stream * stream_size
    output = np.empty(size, dtype=it)
    offsets = np.empty(n_stream, dtype=ft)
    gains = np.empty(n_stream, dtype=ft)
    q = None
    if len(quanta) == n_stream:
        q = np.ascontiguousarray(quanta, dtype=ft)
    errcode = (_lib.lib().float64_to_int64 if _f64 else _lib.lib().float32_to_int32)(
        _ptr(flatdata), n_stream, stream_size, _ptr(q) if q is not None else None, _ptr(output), _ptr(offsets), _ptr(gains)
    )
    if errcode & _lib.ERROR_NAN_INPUT:
        raise RuntimeError("Cannot convert data with NaNs to integers")
    if errcode != 0:
        raise RuntimeError(f"Encoding failed, return code = {errcode}")
    return (output, offsets, gains)


def wrap_int32_to_float32(idata, n_stream, stream_size, offsets, gains, _f64=False):
    """libflacarray.pyx:215-247"""
    _lib.require_device()
    ft, it = (np.float64, np.int64) if _f64 else (np.float32, np.int32)
    idata = np.ascontiguousarray(idata, dtype=it)
    offsets = np.ascontiguousarray(offsets, dtype=ft)
    gains = np.ascontiguousarray(gains, dtype=ft)
    output = np.empty(n_stream * stream_size, dtype=ft)
    (_lib.lib().int64_to_float64 if _f64 else _lib.lib().int32_to_float32)(
        _ptr(idata), n_stream, stream_size, _ptr(offsets), _ptr(gains), _ptr(output)
    )
    return output


def wrap_float64_to_int64(flatdata, n_stream, stream_size, quanta):
    """libflacarray.pyx:164-212"""
    return wrap_float32_to_int32(flatdata, n_stream, stream_size, quanta, _f64=True)


def wrap_int64_to_float64(idata, n_stream, stream_size, offsets, gains):
    """libflacarray.pyx:250-282"""
    return wrap_int32_to_float32(idata, n_stream, stream_size, offsets, gains, _f64=True)


class _EncodeSetting:
    """Hold one of the library's process-wide encode settings (fa_set_encode_verify, fa_set_encode_md5) at `value` for one
    host encode call (None: the default as it is).  The setting's Python lock covers set, call and restore; the library
    serialises host encodes anyway."""

    setter = None  # name of the C setter
    lock = None

    def __init__(self, value):
        self.value = value

    def __enter__(self):
        if self.value is not None:
            self.lock.acquire()
            self.prev = getattr(_lib.lib(), self.setter)(1 if self.value else 0)
        return self

    def __exit__(self, *exc):
        if self.value is not None:
            getattr(_lib.lib(), self.setter)(self.prev)
            self.lock.release()
        return False


_encode_verify_lock = threading.Lock()


def set_encode_verify(on):
    """Process-wide DEFAULT of verification after encode, used by the host encode calls whose `verify` argument is None
    (encode_flac, array_compress, FlacArray.from_array) and by FlacArray.from_device_array: when on, every chunk of
    streams is decoded on the device right after it is written and compared with its input -- libFLAC's encoder verify
    mode (FLAC__stream_encoder_set_verify) -- and a difference raises RuntimeError.  What is compared is the integers:
    float input as quantised with the stored offsets and gains.  Returns the previous setting; initially off.  Callers of
    the reference's C entry points (encode_i32, encode_i64, ...) get verification through this default alone."""
    with _encode_verify_lock:
        return bool(_lib.lib().fa_set_encode_verify(1 if on else 0))


def _encode_verify_default():
    return bool(_lib.lib().fa_set_encode_verify(-1))


class _EncodeVerify(_EncodeSetting):
    """The encode-verify setting, held for one host encode call."""

    setter, lock = "fa_set_encode_verify", _encode_verify_lock


_encode_md5_lock = threading.Lock()


def set_encode_md5(on):
    """Process-wide DEFAULT of STREAMINFO MD5 signing, used by every encode call whose `md5` argument is None: when on,
    the MD5 of each stream's integers (int32: the row's bytes; int64: the same, channel 0 = low word; float input: the
    integers it is quantised to, which is what any FLAC decoder will produce) is computed on the device and written
    into bytes [26, 42) of the stream, where libFLAC writes it and `flac -t` checks it.  Off, the field holds sixteen
    zero bytes ("not computed").  Returns the previous setting; initially off.  Callers of the reference's C entry
    points (encode_i32, encode_i64, ...) get signing through this default alone (fa_set_encode_md5)."""
    with _encode_md5_lock:
        return bool(_lib.lib().fa_set_encode_md5(1 if on else 0))


def _encode_md5_default():
    return bool(_lib.lib().fa_set_encode_md5(-1))


class _EncodeMd5(_EncodeSetting):
    """The encode-md5 setting, held for one host encode call; always entered after _EncodeVerify."""

    setter, lock = "fa_set_encode_md5", _encode_md5_lock


def _check_encode(errcode):
    if errcode & _lib.ERROR_NAN_INPUT:
        raise RuntimeError("Cannot convert data with NaNs to integers")
    if errcode & _lib.ERROR_ENCODE_VERIFY:
        raise RuntimeError("Encoding verification failed: the compressed streams do not decode to the input "
                           f"(return code = {errcode})")
    if errcode != 0:
        raise RuntimeError(f"Encoding failed, return code = {errcode}")


def _wrap_encode(fn, flatdata, n_stream, stream_size, level, dtype=np.int32):
    _lib.require_device()
    flatdata = np.ascontiguousarray(flatdata, dtype=dtype)
    flat_starts = np.empty(n_stream, dtype=np.int64)
    flat_nbytes = np.empty(n_stream, dtype=np.int64)
    n_bytes = ctypes.c_int64(0)
    raw = ctypes.c_void_p(None)
    errcode = fn(_ptr(flatdata), n_stream, stream_size, level, ctypes.byref(n_bytes), _ptr(flat_starts), ctypes.byref(raw))
    _check_encode(errcode)
    flat_nbytes[:-1] = np.diff(flat_starts)
    flat_nbytes[-1] = n_bytes.value - flat_starts[-1]
    return (_adopt_malloc(raw.value, n_bytes.value), flat_starts, flat_nbytes)


def _encode_flac_float(data, quanta, level, ft, fn):
    """The body of encode_flac_f32 / encode_flac_f64: `ft` the numpy float type, `fn` the library's host entry point."""
    _lib.require_device()
    if data.dtype != np.dtype(ft):
        raise ValueError(f"Only {np.dtype(ft).name} data is supported")
    if level < 0 or level > 8:
        raise RuntimeError("FLAC only supports compression levels 0-8")
    data = np.ascontiguousarray(data)
    stream_size = data.shape[-1]
    lead = data.shape[:-1] if data.ndim > 1 else (1,)
    n_stream = int(np.prod(lead))
    q = None
    if quanta is not None:
        q = np.ascontiguousarray(quanta, dtype=ft).reshape(-1)
        if q.size != n_stream:
            raise ValueError("quanta must have one value per stream")
    flat_starts = np.empty(n_stream, dtype=np.int64)
    flat_nbytes = np.empty(n_stream, dtype=np.int64)
    offsets = np.empty(n_stream, dtype=ft)
    gains = np.empty(n_stream, dtype=ft)
    n_bytes = ctypes.c_int64(0)
    raw = ctypes.c_void_p(None)
    errcode = fn(_ptr(data), n_stream, stream_size, level, _ptr(q) if q is not None else None, ctypes.byref(n_bytes), _ptr(flat_starts),
                 ctypes.byref(raw), _ptr(offsets), _ptr(gains))
    _check_encode(errcode)
    flat_nbytes[:-1] = np.diff(flat_starts)
    flat_nbytes[-1] = n_bytes.value - flat_starts[-1]
    return (_adopt_malloc(raw.value, n_bytes.value), flat_starts.reshape(lead), flat_nbytes.reshape(lead), offsets.reshape(lead),
            gains.reshape(lead))


def encode_flac_f32(data, quanta, level):
    """float32 array -> (compressed, starts, nbytes, offsets, gains) in one trip over PCIe (fa_encode_f32_host): the
    samples go up once and are quantised where the encoder loads them -- the same integers, offsets, gains and bytes as
    `float_to_int` (utils.py:246-342) followed by `encode_flac` (libflacarray.pyx:529-594), which moves the array up,
    the integers down, and the integers up again.  `quanta`: None (from each stream's range) or one value per stream."""
    return _encode_flac_float(data, quanta, level, np.float32, _lib.lib().fa_encode_f32_host)


def encode_flac_f64(data, quanta, level):
    """float64 array -> (compressed, starts, nbytes, offsets, gains) in one trip over PCIe (fa_encode_f64_host): the
    float64 samples go up once, are quantised on the device (float64_to_int64, utils.c:245-327) and encoded from there as
    two-channel streams -- the same integers, offsets, gains and bytes as `float_to_int` followed by `encode_flac`
    (compress.py:50-84), which moves the array up, the int64 image down, and the int64 image up again."""
    return _encode_flac_float(data, quanta, level, np.float64, _lib.lib().fa_encode_f64_host)


def wrap_encode_i32(flatdata, n_stream, stream_size, level):
    """libflacarray.pyx:285-343"""
    return _wrap_encode(_lib.lib().encode_i32, flatdata, n_stream, stream_size, level)


def wrap_encode_i32_threaded(flatdata, n_stream, stream_size, level):
    """libflacarray.pyx:346-404"""
    return _wrap_encode(_lib.lib().encode_i32_threaded, flatdata, n_stream, stream_size, level)


def _blocksize_classes(header_bytes):
    """Streams of one decode call normally share their block size (one array, one level).  A store assembled from
    several encodes may not -- libFLAC decodes every stream on its own terms (decompress.c:256-305), the GPU decoder
    takes one block size per launch.  header_bytes: uint8 [n_stream, 12], the first bytes of every stream
    ("fLaC", STREAMINFO header, min / max block size).  Returns a list of index arrays, one per block size, or None
    when the headers are not what they should be or all streams agree."""
    h = np.asarray(header_bytes, dtype=np.uint8)
    if h.ndim != 2 or h.shape[1] < 12 or h.shape[0] < 2:
        return None
    if not (np.all(h[:, 0:4] == np.frombuffer(b"fLaC", np.uint8)) and np.all((h[:, 4] & 0x7F) == 0)):
        return None
    bmin = (h[:, 8].astype(np.int64) << 8) | h[:, 9]
    bmax = (h[:, 10].astype(np.int64) << 8) | h[:, 11]
    key = bmin * 65536 + bmax
    kinds = np.unique(key)
    if kinds.size < 2:
        return None
    return [np.flatnonzero(key == k) for k in kinds]


def wrap_decode_i32(compressed, starts, nbytes, n_stream, stream_size, first_sample, last_sample, use_threads, _i64=False):
    """libflacarray.pyx:597-653"""
    _lib.require_device()
    n_decode = stream_size
    if first_sample >= 0 and last_sample >= 0:
        n_decode = last_sample - first_sample
    compressed = np.ascontiguousarray(compressed, dtype=np.uint8)
    starts = np.ascontiguousarray(starts, dtype=np.int64)
    nbytes = np.ascontiguousarray(nbytes, dtype=np.int64)
    output = np.empty(max(n_stream * n_decode, 0), dtype=flac_i64_dtype if _i64 else flac_i32_dtype)
    _advise_huge_pages(output)
    errcode = (_lib.lib().decode_i64 if _i64 else _lib.lib().decode_i32)(
        _ptr(compressed), _ptr(starts), _ptr(nbytes), n_stream, stream_size, first_sample, last_sample, _ptr(output),
        bool(use_threads),
    )
    if errcode != 0:
        # streams of different block sizes in one call: one launch per block size, rows scattered back
        groups = None
        if n_stream > 1 and np.all(starts >= 0) and np.all(nbytes >= 12) and np.all(starts + nbytes <= compressed.size):
            groups = _blocksize_classes(compressed[starts[:, None] + np.arange(12)[None, :]])
        if groups is None:
            raise RuntimeError(f"Decoding failed, return code = {errcode}")
        out2 = output.reshape(n_stream, max(n_decode, 0))
        for idx in groups:
            out2[idx] = wrap_decode_i32(compressed, starts[idx], nbytes[idx], int(idx.size), stream_size, first_sample, last_sample,
                                        use_threads, _i64=_i64).reshape(idx.size, -1)
    return output


def wrap_decode_i64(compressed, starts, nbytes, n_stream, stream_size, first_sample, last_sample, use_threads):
    """libflacarray.pyx:656-710"""
    return wrap_decode_i32(compressed, starts, nbytes, n_stream, stream_size, first_sample, last_sample, use_threads, _i64=True)


def wrap_encode_i64(flatdata, n_stream, stream_size, level):
    """libflacarray.pyx:407-465"""
    return _wrap_encode(_lib.lib().encode_i64, flatdata, n_stream, stream_size, level, dtype=np.int64)


def wrap_encode_i64_threaded(flatdata, n_stream, stream_size, level):
    """libflacarray.pyx:468-526"""
    return _wrap_encode(_lib.lib().encode_i64_threaded, flatdata, n_stream, stream_size, level, dtype=np.int64)





def encode_flac(data, level, use_threads=False, verify=None, md5=None):
    """Compress an integer array to FLAC streams (libflacarray.pyx:529-594).

    Returns (compressed bytestream, stream starting bytes, stream nbytes); starts and nbytes
    have the leading shape of `data` and are at least 1-D.  `verify`: True = decode what was written, on the device,
    and compare it with the input before returning (libFLAC's verify mode; a difference raises RuntimeError), False =
    do not, None = the default of set_encode_verify.  `md5`: True = sign every stream (the MD5 of its samples in
    STREAMINFO, computed on the device while the input is there), False = leave the field zero, None = the default of
    set_encode_md5.
    """
    if data.dtype != flac_i32_dtype and data.dtype != flac_i64_dtype:
        raise RuntimeError("Only 32bit or 64bit integer data is supported")
    if not data.flags.c_contiguous:
        raise RuntimeError("Only C-contiguous arrays are supported")
    if level < 0 or level > 8:
        raise RuntimeError("FLAC only supports compression levels 0-8")
    is_i64 = data.dtype == flac_i64_dtype
    stream_size = data.shape[-1]
    if len(data.shape[:-1]) == 0:
        n_stream = 1
        starts_shape = (1,)
    else:
        n_stream = int(np.prod(data.shape[:-1]))
        starts_shape = data.shape[:-1]
    flatdata = data.reshape((-1,))
    if is_i64:
        enc = wrap_encode_i64_threaded if use_threads else wrap_encode_i64
    else:
        enc = wrap_encode_i32_threaded if use_threads else wrap_encode_i32
    with _EncodeVerify(verify), _EncodeMd5(md5):
        compressed, flatstarts, flatnbytes = enc(flatdata, n_stream, stream_size, level)
    return (compressed, flatstarts.reshape(starts_shape), flatnbytes.reshape(starts_shape))


def decode_flac(compressed, starts, nbytes, stream_size, first_sample=-1, last_sample=-1, use_threads=False, is_int64=False):
    """Decompress FLAC streams (libflacarray.pyx:713-823); output shape starts.shape + (n_decode,)."""
    if compressed.dtype != compressed_dtype:
        raise RuntimeError("Compressed data should be of type uint8")
    if not compressed.flags.c_contiguous:
        raise RuntimeError("Only C-contiguous arrays are supported")
    if starts.dtype != offset_dtype:
        raise RuntimeError("starts data should be of type int64")
    if not starts.flags.c_contiguous:
        raise RuntimeError("Only C-contiguous arrays are supported")
    if nbytes.dtype != offset_dtype:
        raise RuntimeError("nbytes data should be of type int64")
    if not nbytes.flags.c_contiguous:
        raise RuntimeError("Only C-contiguous arrays are supported")
    if stream_size <= 0:
        raise RuntimeError("You must specify the non-zero output stream size")
    if len(compressed.shape) != 1:
        raise RuntimeError("Compressed byte array should be one dimensional")
    n_decode = stream_size
    if first_sample >= 0 and last_sample >= 0:
        if last_sample > stream_size:
            raise RuntimeError("last_sample is beyond end of stream")
        if first_sample > stream_size - 1:
            raise RuntimeError("first_sample is beyond last element of stream")
        if first_sample >= last_sample:
            raise RuntimeError("first_sample is larger than last_sample")
        n_decode = last_sample - first_sample
    output_shape = starts.shape + (n_decode,)
    n_stream = int(np.prod(starts.shape))
    flat_output = (wrap_decode_i64 if is_int64 else wrap_decode_i32)(
        compressed, starts.reshape((-1,)), nbytes.reshape((-1,)), n_stream, int(stream_size), int(first_sample),
        int(last_sample), use_threads,
    )
    return flat_output.reshape(output_shape)


def decode_flac_restore(compressed, starts, nbytes, stream_size, offsets, gains, first_sample=-1, last_sample=-1, is_int64=False):
    """`decode_flac` followed by `int_to_float` (decompress.py:107-136) in one trip over PCIe: compressed bytes up, the
    restore of utils.c:329-368 fused into the decoder's store, float32 / float64 down (fa_decode_f32_host /
    fa_decode_f64_host) -- the same values, bit for bit, as the two calls.  Shapes as decode_flac; offsets / gains have
    the shape of `starts`.  Returns None when the library refuses the call (e.g. streams of different block sizes): the
    caller then takes the two-call path, which knows how to split such a store."""
    _lib.require_device()
    n_decode = stream_size if (first_sample < 0 or last_sample < 0) else last_sample - first_sample
    ftype = np.float64 if is_int64 else np.float32
    st = np.ascontiguousarray(starts, dtype=np.int64)
    nb = np.ascontiguousarray(nbytes, dtype=np.int64).reshape(-1)
    off = np.ascontiguousarray(offsets, dtype=ftype).reshape(-1)
    gain = np.ascontiguousarray(gains, dtype=ftype).reshape(-1)
    n_stream = int(st.size)
    if off.size != n_stream or gain.size != n_stream or n_decode <= 0:
        return None
    compressed = np.ascontiguousarray(compressed, dtype=np.uint8)
    out = np.empty(n_stream * n_decode, dtype=ftype)
    _advise_huge_pages(out)
    fn = _lib.lib().fa_decode_f64_host if is_int64 else _lib.lib().fa_decode_f32_host
    errcode = fn(_ptr(compressed), _ptr(st.reshape(-1)), _ptr(nb), n_stream, int(stream_size), int(first_sample), int(last_sample),
                 _ptr(off), _ptr(gain), _ptr(out))
    if errcode != 0:
        return None
    return out.reshape(st.shape + (n_decode,))


def decode_flac_into(compressed, starts, nbytes, stream_size, out, first_sample=-1, last_sample=-1):
    """`decode_flac` into an array the caller owns: the C boundary takes a caller-allocated output (decode_i32 /
    decode_i64, flacarray.h:249-271; libflacarray.pyx:634 allocates a fresh one per call), and a caller that decodes
    store after store into the same array pays for the transfer, not for the population of fresh pages.  `out`:
    C-contiguous int32 / int64 of starts.size * n_decode elements."""
    _lib.require_device()
    n_decode = stream_size if (first_sample < 0 or last_sample < 0) else last_sample - first_sample
    starts = np.ascontiguousarray(starts, dtype=np.int64).reshape(-1)
    nbytes = np.ascontiguousarray(nbytes, dtype=np.int64).reshape(-1)
    compressed = np.ascontiguousarray(compressed, dtype=np.uint8)
    is64 = out.dtype == np.dtype(np.int64)
    if out.dtype not in (np.dtype(np.int32), np.dtype(np.int64)) or not out.flags.c_contiguous or out.size != starts.size * n_decode:
        raise RuntimeError("out must be a C-contiguous int32 / int64 array of starts.size x n_decode elements")
    errcode = (_lib.lib().decode_i64 if is64 else _lib.lib().decode_i32)(
        _ptr(compressed), _ptr(starts), _ptr(nbytes), int(starts.size), int(stream_size), int(first_sample), int(last_sample), _ptr(out), False)
    if errcode != 0:
        raise RuntimeError(f"Decoding failed, return code = {errcode}")
    return out


# ---------------------------------------------------------------------------------------------
# Device-resident variants (torch tensors on the GPU; torch supplies memory and streams only)
# ---------------------------------------------------------------------------------------------
def _torch():
    import torch

    return torch


def _stream_ptr():
    """The current HIP stream of the current device as a void* (torch's raw-stream query where it exists: the public
    route through torch.cuda.current_stream() costs ~9 us per call, a tenth of a small read)."""
    torch = _torch()
    raw = getattr(torch._C, "_cuda_getCurrentRawStream", None)
    if raw is not None:
        try:
            return ctypes.c_void_p(raw(torch.cuda.current_device()))
        except Exception:  # noqa: BLE001
            pass
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _dp(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


class _NoSwitch:
    def __enter__(self):
        return None

    def __exit__(self, *exc):
        return False


_NO_SWITCH = _NoSwitch()


def _on_device(device):
    """`torch.cuda.device(device)` only when that is a switch: entering and leaving the context manager costs ~8 us, a
    tenth of a small call, and nearly every call runs on the current device already."""
    torch = _torch()
    idx = device.index if device.index is not None else torch.cuda.current_device()
    return _NO_SWITCH if idx == torch.cuda.current_device() else torch.cuda.device(device)


class EncodeWorkspace:
    """Reusable HBM scratch for encode_flac_device (per-frame slots + scan arrays)."""

    def __init__(self):
        self.buf = None

    def get(self, nbytes, device):
        torch = _torch()
        if self.buf is None or self.buf.numel() < nbytes or self.buf.device != device:
            self.buf = None
            self.buf = torch.empty(nbytes, dtype=torch.uint8, device=device)
        return self.buf


def encode_flac_device(data, level=5, workspace=None, return_info=False, compact=False, capacity_bytes=None, verify=False, md5=None):
    """Encode a C-contiguous int32 (or int64: two-channel streams) CUDA tensor [..., stream_size] held in HBM.

    Returns (compressed uint8 tensor, starts int64 tensor, nbytes int64 tensor), all on the
    device, starts/nbytes with the leading shape of `data` (at least 1-D) -- the device-resident
    analogue of encode_flac (libflacarray.pyx:529-594).

    Every geometry is encoded in a single pass (K3F for full 4096-sample mono frames of levels 3-8, K3G for the rest:
    short streams, levels 0-2, int64; include/flacarray_hip.h): the frames end up at their final offsets inside a buffer
    sized for the worst case, and `compressed` is the view [0, total) of that buffer (it keeps the whole buffer alive;
    `compact=True` returns an exact-size copy instead).  `capacity_bytes` sizes that buffer instead of the worst case
    (1.016 x the input: every frame VERBATIM): if the blob does not fit, nothing outside the buffer is written and the
    call raises "Encoding failed, return code = 1" (ERROR_ALLOC) -- retry without it.  Under FLACARRAY_HIP_SLOTS (the
    diagnostic cross-check) everything runs the slot sequence (K3, K4, K5) and returns an exact-size tensor.

    `verify=True`: the streams are decoded and compared with `data` on the device before the call returns
    (compare_flac_device); a difference raises RuntimeError naming the first differing stream(s) and sample.  The
    returned bytes are the same either way.

    `md5`: True = sign the streams (md5_device over `data`, patched into STREAMINFO by sign_streams_device: sixteen
    bytes per stream, every other byte as without it), False = leave the field zero, None = the default of
    set_encode_md5.
    """
    out = _encode_flac_device(data, level, workspace, return_info, compact, capacity_bytes)
    if verify:
        _raise_on_mismatch(compare_flac_device(out[0], out[1], out[2], data))
    if _encode_md5_default() if md5 is None else md5:
        sign_streams_device(out[0], out[1], md5_device(data))
    return out


def _encode_flac_device(data, level, workspace, return_info, compact, capacity_bytes):
    torch = _torch()
    if data.dtype != torch.int32 and data.dtype != torch.int64:
        raise RuntimeError("Only 32bit or 64bit integer data is supported")
    if not data.is_contiguous():
        raise RuntimeError("Only C-contiguous arrays are supported")
    if level < 0 or level > 8:
        raise RuntimeError("FLAC only supports compression levels 0-8")
    if not data.is_cuda:
        raise RuntimeError("encode_flac_device needs a tensor on the GPU")
    i64 = data.dtype == torch.int64
    stream_size = data.shape[-1]
    if data.dim() == 1:
        n_stream, starts_shape = 1, (1,)
    else:
        n_stream = int(np.prod(data.shape[:-1]))
        starts_shape = tuple(data.shape[:-1])
    L = _lib.lib()
    if workspace is None:
        workspace = EncodeWorkspace()
    index = torch.empty(2 * n_stream, dtype=torch.int64, device=data.device)  # (one allocation: starts | nbytes)
    starts, nbytes = index[:n_stream], index[n_stream:]
    info = None
    if return_info:
        bs = 1152 if level <= 2 else 4096
        nf = (stream_size + bs - 1) // bs
        info = torch.zeros((n_stream * nf * (2 if i64 else 1), 8), dtype=torch.int32, device=data.device)
    total = ctypes.c_int64(0)
    if L.fa_encode_single_pass_supported(n_stream, stream_size, level):
        cap = (L.fa_encode_capacity_bytes_i64 if i64 else L.fa_encode_capacity_bytes)(n_stream, stream_size, level)
        if capacity_bytes is not None:
            cap = min(cap, int(capacity_bytes))
        ws = workspace.get((L.fa_encode_single_pass_workspace_bytes_i64 if i64 else L.fa_encode_single_pass_workspace_bytes)(n_stream, stream_size, level), data.device)
        with _on_device(data.device):
            buf = torch.empty(cap, dtype=torch.uint8, device=data.device)
            errcode = (L.fa_encode_i64_device if i64 else L.fa_encode_i32_device)(
                _dp(data), n_stream, stream_size, level, _dp(ws), ws.numel(), _dp(buf), cap, _dp(starts), _dp(nbytes),
                ctypes.byref(total), _dp(info), _stream_ptr(),
            )
        if errcode != 0:
            raise RuntimeError(f"Encoding failed, return code = {errcode}")
        compressed = buf[: total.value]
        if compact:
            compressed = compressed.clone()
    else:
        ws_bytes = (L.fa_encode_workspace_bytes_i64 if i64 else L.fa_encode_workspace_bytes)(n_stream, stream_size, level)
        if ws_bytes < 0:
            raise RuntimeError("Encoding failed, return code = 512")
        ws = workspace.get(ws_bytes, data.device)
        with _on_device(data.device):
            errcode = (L.fa_encode_i64_device_begin if i64 else L.fa_encode_i32_device_begin)(
                _dp(data), n_stream, stream_size, level, _dp(ws), ws.numel(), _dp(starts), _dp(nbytes), ctypes.byref(total),
                _dp(info), _stream_ptr(),
            )
            if errcode != 0:
                raise RuntimeError(f"Encoding failed, return code = {errcode}")
            compressed = torch.empty(total.value, dtype=torch.uint8, device=data.device)
            errcode = (L.fa_encode_i64_device_finish if i64 else L.fa_encode_i32_device_finish)(n_stream, stream_size, level, _dp(ws), _dp(starts), _dp(compressed), _stream_ptr())
            if errcode != 0:
                raise RuntimeError(f"Encoding failed, return code = {errcode}")
    out = (compressed, starts.reshape(starts_shape), nbytes.reshape(starts_shape))
    return out + (info,) if return_info else out


def set_decode_verify(on):
    """Process-wide DEFAULT of the decoder's integrity pass, used by device decode calls whose `verify` argument is
    None: when on, the call re-computes the CRC-16 of each frame it read and raises ("Decoding failed, return code =
    16384", ERROR_DECODE_PROCESS) on a mismatch -- the condition libFLAC reports through the error callback the
    reference prints (decompress.c:104-121).  Returns the previous setting.  Initially off for device-resident stores
    (the pass re-reads the compressed bytes); the host-pointer path behind `decode_flac` always checks."""
    return bool(_lib.lib().fa_set_decode_verify(1 if on else 0))


def _verify_arg(verify):
    return -1 if verify is None else (1 if verify else 0)


def std_device(data):
    """Per-stream standard deviation of a C-contiguous float32 / float64 CUDA tensor [..., stream_size], bit for bit
    np.std(data.cpu().numpy(), axis=-1) (numpy's chunked pairwise summation, chunk = np.getbufsize() at call time;
    flacarray_amd/npsum.py).  Returns a tensor of the data's dtype with the leading shape, (1,) for a 1-D tensor; it is
    complete in stream order (no wait on the stream)."""
    torch = _torch()
    if data.dtype not in (torch.float32, torch.float64):
        raise ValueError("Only float32 and float64 data are supported")
    if not data.is_contiguous():
        raise RuntimeError("Only C-contiguous arrays are supported")
    if not data.is_cuda:
        raise RuntimeError("std_device needs a tensor on the GPU")
    if data.dim() == 0 or data.numel() == 0:
        raise ValueError("std_device needs a non-empty array with a stream axis")
    lead = tuple(data.shape[:-1]) if data.dim() > 1 else (1,)
    n_stream = int(np.prod(lead))
    out = torch.empty(n_stream, dtype=data.dtype, device=data.device)
    L = _lib.lib()
    fn = L.fa_stream_std_f32_device if data.dtype == torch.float32 else L.fa_stream_std_f64_device
    with _on_device(data.device):
        errcode = fn(_dp(data), n_stream, data.shape[-1], int(np.getbufsize()), _dp(out), _stream_ptr())
    if errcode != 0:
        raise RuntimeError(f"Standard deviation failed, return code = {errcode}")
    return out.reshape(lead)


def _precision_quanta_device(data, precision):
    """Per-stream quanta rms / 10^p for device data as a tensor on its device: the std on the device, its n_stream
    values copied to the host (the one wait), then the host path's own numpy expression (utils.precision_quanta)."""
    from .utils import precision_quanta, stream_quanta

    torch = _torch()
    lead = tuple(data.shape[:-1])  # numpy's leading shape: () for a 1-D array
    ndt = np.float32 if data.dtype == torch.float32 else np.float64
    rms = std_device(data).cpu().numpy().reshape(lead)
    q = stream_quanta(precision_quanta(rms, lead, precision), lead, ndt)
    return torch.from_numpy(q).to(data.device)


def encode_flac_device_f32(data, quanta=None, level=5, workspace=None, compact=False, precision=None, verify=False, md5=None):
    """Quantise and encode a C-contiguous float32 CUDA tensor [..., stream_size] held in HBM: the device-resident
    analogue of array_compress on float32 input (compress.py:50-84 -> float_to_int + encode_flac).

    `quanta`: None (per-stream quanta from the data range), or a tensor with one value per stream.  Returns
    (compressed, starts, nbytes, offsets, gains), offsets / gains float32 with the leading shape of `data`.  Where
    the single-pass kernel applies (levels 3-8, stream length a multiple of 4096) the quantisation happens in the
    encoder's staging load after a range pre-pass -- the int32 array never exists in HBM; otherwise the two steps
    run one after the other.  Same bytes, offsets and gains either way.  `precision` p (instead of `quanta`): quanta =
    std / 10^p per stream as array_compress derives them (std_device, then the host path's numpy expression).
    `verify=True`: compare the streams with `data` before returning, as encode_flac_device does -- the quantised integers,
    not the floats.  `md5`: sign the streams (None = the default of set_encode_md5) with the MD5 of the quantised
    integers -- hashed from the floats, quantised where they are loaded: the integers need not exist."""
    out = _encode_flac_device_f32(data, quanta, level, workspace, compact, precision)
    if verify:
        _raise_on_mismatch(compare_flac_device(out[0], out[1], out[2], data, out[3], out[4]))
    if _encode_md5_default() if md5 is None else md5:
        sign_streams_device(out[0], out[1], md5_device(data, out[3], out[4]))
    return out


def _encode_flac_device_f32(data, quanta, level, workspace, compact, precision):
    torch = _torch()
    if data.dtype != torch.float32 or not data.is_contiguous():
        raise ValueError("Only float32 and float64 data are supported")
    if not data.is_cuda:
        raise RuntimeError("encode_flac_device_f32 needs a tensor on the GPU")
    if level < 0 or level > 8:
        raise RuntimeError("FLAC only supports compression levels 0-8")
    if precision is not None:
        if quanta is not None:
            raise RuntimeError("Cannot set both quanta and precision")
        quanta = _precision_quanta_device(data, precision)
    stream_size = data.shape[-1]
    lead = tuple(data.shape[:-1]) if data.dim() > 1 else (1,)
    n_stream = int(np.prod(lead))
    q = None
    if quanta is not None:
        q = quanta.to(device=data.device, dtype=torch.float32).reshape(-1).contiguous()
        if q.numel() != n_stream:
            raise RuntimeError("quanta must have one entry per stream")
    L = _lib.lib()
    # (the fused kernel, K3F, takes levels 3-8 only: levels 0-2 of any length quantise first, then go to K3G)
    if not (level >= 3 and data.data_ptr() % 16 == 0 and stream_size % 4096 == 0 and L.fa_encode_single_pass_supported(n_stream, stream_size, level)):
        ints, offsets, gains = float32_to_int32_device(data, q)
        comp, st, nb = encode_flac_device(ints, level=level, workspace=workspace, compact=compact, md5=False)
        return comp, st, nb, offsets, gains
    if workspace is None:
        workspace = EncodeWorkspace()
    starts = torch.empty(n_stream, dtype=torch.int64, device=data.device)
    nbytes = torch.empty(n_stream, dtype=torch.int64, device=data.device)
    offsets = torch.empty(n_stream, dtype=torch.float32, device=data.device)
    gains = torch.empty(n_stream, dtype=torch.float32, device=data.device)
    cap = L.fa_encode_capacity_bytes(n_stream, stream_size, level)
    ws = workspace.get(L.fa_encode_single_pass_workspace_bytes(n_stream, stream_size, level), data.device)
    total = ctypes.c_int64(0)
    with _on_device(data.device):
        buf = torch.empty(cap, dtype=torch.uint8, device=data.device)
        errcode = L.fa_encode_f32_device(
            _dp(data), n_stream, stream_size, level, _dp(q), _dp(ws), ws.numel(), _dp(buf), cap, _dp(starts), _dp(nbytes),
            _dp(offsets), _dp(gains), ctypes.byref(total), None, _stream_ptr(),
        )
    if errcode & _lib.ERROR_NAN_INPUT:
        raise RuntimeError("Cannot convert data with NaNs to integers")
    if errcode != 0:
        raise RuntimeError(f"Encoding failed, return code = {errcode}")
    compressed = buf[: total.value]
    if compact:
        compressed = compressed.clone()
    return compressed, starts.reshape(lead), nbytes.reshape(lead), offsets.reshape(lead), gains.reshape(lead)


def encode_flac_device_f64(data, quanta=None, level=5, workspace=None, compact=False, precision=None, verify=False, md5=None):
    """Quantise and encode a C-contiguous float64 CUDA tensor [..., stream_size] held in HBM: the device-resident
    analogue of array_compress on float64 input (float64_to_int64, then the two-channel encoder).

    `quanta`: None (per-stream quanta from the data range) or a tensor with one value per stream; `precision` p
    instead: quanta = std / 10^p per stream, as for encode_flac_device_f32.  Returns (compressed, starts, nbytes,
    offsets, gains), offsets / gains float64 with the leading shape of `data`.  `verify=True`: compare the streams with
    `data` before returning (the quantised integers, not the floats).  `md5`: sign the streams with the MD5 of the
    quantised integers (None = the default of set_encode_md5)."""
    torch = _torch()
    if data.dtype != torch.float64 or not data.is_contiguous():
        raise ValueError("Only float32 and float64 data are supported")
    if not data.is_cuda:
        raise RuntimeError("encode_flac_device_f64 needs a tensor on the GPU")
    if level < 0 or level > 8:
        raise RuntimeError("FLAC only supports compression levels 0-8")
    if precision is not None:
        if quanta is not None:
            raise RuntimeError("Cannot set both quanta and precision")
        quanta = _precision_quanta_device(data, precision)
    ints, offsets, gains = float64_to_int64_device(data, quanta)
    comp, st, nb = encode_flac_device(ints, level=level, workspace=workspace, compact=compact, md5=md5)
    if verify:
        _raise_on_mismatch(compare_flac_device(comp, st, nb, data, offsets, gains))
    return comp, st, nb, offsets, gains


def _raise_on_mismatch(first):
    """RuntimeError naming the first streams whose entry in `first` (compare_flac_device's result) is not -1."""
    m = first.reshape(-1).cpu().numpy()
    bad = np.flatnonzero(m >= 0)
    if bad.size:
        where = ", ".join(f"stream {i} at sample {m[i]}" for i in bad[:4])
        more = f" and {bad.size - 4} more stream(s)" if bad.size > 4 else ""
        raise RuntimeError(f"Encoding verification failed: the compressed streams do not decode to the input ({where}{more})")


def compare_flac_device(compressed, starts, nbytes, data, offsets=None, gains=None):
    """Compare device-resident FLAC streams with the samples they should decode to, without a decoded copy: the decoder
    compares each sample with `data` where it would store it.  Returns an int64 tensor with the shape of `starts`, one
    entry per stream: the index of the first sample that differs, or -1.

    `data`: a C-contiguous tensor of shape (n_stream, stream_size) or starts.shape + (stream_size,) on the device of
    `compressed` -- int32 or float32 against one-channel streams, int64 or float64 against two-channel streams.  Float
    data need the store's `offsets` and `gains` and are quantised with them exactly as the encoder quantises: what is
    compared is the quantised integers, not the floats, so a float change that leaves its quantised integer the same is
    not a mismatch.  Streams of any origin compare (without a SEEKTABLE the frames are found by a sync scan).  A frame
    the decoder rejects marks its stream at that frame's first sample or earlier; the other streams are still compared.
    Damaged stream headers raise RuntimeError, as decode_flac_device does.  All streams must share one block size (every
    store this library writes does); a store whose streams differ raises RuntimeError ("Comparison failed, return code =
    8192"), where decode_flac_device would decode it in one launch per block size."""
    torch = _torch()
    if compressed.dtype != torch.uint8:
        raise ValueError("Compressed data should be of type uint8")
    if starts.dtype != torch.int64 or nbytes.dtype != torch.int64:
        raise ValueError("starts and nbytes should be of type int64")
    if starts.shape != nbytes.shape:
        raise ValueError("starts and nbytes must have the same shape")
    n_stream = int(np.prod(starts.shape))
    if data.dtype not in (torch.int32, torch.int64, torch.float32, torch.float64):
        raise ValueError(f"Unsupported data type '{data.dtype}': int32, int64, float32 or float64")
    if data.dim() == 0 or data.shape[-1] <= 0:
        raise ValueError("data needs a non-empty stream axis")
    stream_size = int(data.shape[-1])
    if tuple(data.shape) not in ((n_stream, stream_size), tuple(starts.shape) + (stream_size,)) and not (data.dim() == 1 and n_stream == 1):
        raise ValueError(f"data of shape {tuple(data.shape)} does not match {n_stream} streams (starts of shape {tuple(starts.shape)})")
    if not data.is_contiguous():
        raise ValueError("Only C-contiguous data is supported")
    is_float = data.dtype in (torch.float32, torch.float64)
    if (offsets is None) != (gains is None):
        raise ValueError("When specifying offsets, you must also provide the gains")
    if is_float and offsets is None:
        raise ValueError("Comparing float data needs the store's offsets and gains")
    if not is_float and offsets is not None:
        raise ValueError("offsets and gains apply to float data only")
    if is_float and (offsets.numel() != n_stream or gains.numel() != n_stream):
        raise ValueError("offsets and gains need one value per stream")
    dev = compressed.device
    if not (compressed.is_cuda and data.device == dev and starts.device == dev and nbytes.device == dev):
        raise RuntimeError("compare_flac_device needs compressed, starts, nbytes and data on the same GPU")
    if not (compressed.is_contiguous() and starts.is_contiguous() and nbytes.is_contiguous()):
        raise ValueError("Only C-contiguous arrays are supported")
    wide = data.dtype in (torch.int64, torch.float64)
    if is_float:
        offsets = offsets.to(device=dev, dtype=data.dtype).reshape(-1).contiguous()
        gains = gains.to(device=dev, dtype=data.dtype).reshape(-1).contiguous()
    first = torch.empty(starts.shape, dtype=torch.int64, device=dev)
    L = _lib.lib()
    with _on_device(dev):
        errcode = (L.fa_compare_i64_device if wide else L.fa_compare_i32_device)(
            _dp(compressed), compressed.numel(), _dp(starts), _dp(nbytes), n_stream, stream_size, _dp(data), _dp(offsets),
            _dp(gains), _dp(first), _stream_ptr(),
        )
    if errcode != 0:
        raise RuntimeError(f"Comparison failed, return code = {errcode}")
    return first


def md5_device(data, offsets=None, gains=None, state=None, n_before=0, final=True):
    """MD5 of every stream of a device tensor [..., stream_size], one GPU lane per stream (fa_md5_i32_device /
    fa_md5_i64_device): a uint8 tensor of shape (n_stream, 16), equal to hashlib.md5 of each row's little-endian bytes --
    which is what libFLAC writes into STREAMINFO for the 32-bit one-channel (int32) and two-channel (int64) streams of
    this library.

    `data`: int32 or int64, or float32 / float64 with `offsets` and `gains` (one value per stream): the floats are
    quantised where they are loaded, exactly as the encoder quantises them, and the hash is that of the integers (a NaN
    raises RuntimeError).  C-contiguous, or a 2-D column range of a wider C-contiguous image (unit stride along the
    stream, any row stride).  A stream of length 0 gives the digest of the empty message.

    Resumable: `final=False` hashes a whole number of 64-byte blocks (a multiple of 16 int32 / 8 int64 samples) and
    returns the chaining state, an int32 tensor (n_stream, 4), instead of the digest; the next call passes it as `state`
    together with `n_before`, the samples of every stream hashed so far.  The last call (`final=True`) adds the padding
    and the length of all n_before + stream_size samples."""
    torch = _torch()
    if data.dtype not in (torch.int32, torch.int64, torch.float32, torch.float64):
        raise ValueError(f"Unsupported data type '{data.dtype}': int32, int64, float32 or float64")
    if data.dim() == 0:
        raise ValueError("data needs a stream axis")
    n = int(data.shape[-1])
    n_stream = int(np.prod(data.shape[:-1])) if data.dim() > 1 else 1
    if n_stream <= 0:
        raise ValueError("data needs at least one stream")
    stride = n
    if data.dim() == 2 and not data.is_contiguous():
        if (n > 1 and data.stride(1) != 1) or (n_stream > 1 and data.stride(0) < n):
            raise ValueError("Only C-contiguous data, or a column range of a C-contiguous 2-D array, is supported")
        stride = int(data.stride(0)) if n_stream > 1 else n
    elif not data.is_contiguous():
        raise ValueError("Only C-contiguous data, or a column range of a C-contiguous 2-D array, is supported")
    is_float = data.dtype in (torch.float32, torch.float64)
    if (offsets is None) != (gains is None):
        raise ValueError("When specifying offsets, you must also provide the gains")
    if is_float and offsets is None:
        raise ValueError("Hashing float data needs the offsets and gains that quantise it")
    if not is_float and offsets is not None:
        raise ValueError("offsets and gains apply to float data only")
    if is_float and (offsets.numel() != n_stream or gains.numel() != n_stream):
        raise ValueError("offsets and gains need one value per stream")
    wide = data.dtype in (torch.int64, torch.float64)
    per_block = 8 if wide else 16
    if n_before < 0 or n_before % per_block != 0:
        raise ValueError(f"n_before must be a whole number of 64-byte blocks ({per_block} samples)")
    if not final and n % per_block != 0:
        raise ValueError(f"A call that is not the last must hash a whole number of 64-byte blocks ({per_block} samples)")
    if (n_before > 0) != (state is not None):
        raise ValueError("state and n_before go together: both from the previous call, or neither")
    if state is not None and (state.dtype != torch.int32 or tuple(state.shape) != (n_stream, 4) or not state.is_contiguous()):
        raise ValueError("state must be the int32 tensor of shape (n_stream, 4) a call with final=False returned")
    if not data.is_cuda:
        raise RuntimeError("md5_device needs a tensor on the GPU")
    dev = data.device
    if state is not None and state.device != dev:
        raise RuntimeError("md5_device needs state on the GPU of data")
    if is_float:
        offsets = offsets.to(device=dev, dtype=data.dtype).reshape(-1).contiguous()
        gains = gains.to(device=dev, dtype=data.dtype).reshape(-1).contiguous()
    digest = torch.empty((n_stream, 16), dtype=torch.uint8, device=dev) if final else None
    if not final:
        state = state.clone() if state is not None else torch.empty((n_stream, 4), dtype=torch.int32, device=dev)
    L = _lib.lib()
    with _on_device(dev):
        errcode = (L.fa_md5_i64_device if wide else L.fa_md5_i32_device)(
            _dp(data), n_stream, n, stride, _dp(offsets), _dp(gains), _dp(state), n_before, 1 if final else 0, _dp(digest), _stream_ptr())
    if errcode & _lib.ERROR_NAN_INPUT:
        raise RuntimeError("Cannot convert data with NaNs to integers")
    if errcode != 0:
        raise RuntimeError(f"MD5 failed, return code = {errcode}")
    return digest if final else state


def sign_streams_device(compressed, starts, digests):
    """Write `digests` (uint8, sixteen bytes per stream, as md5_device returns them) into the MD5 field of every
    stream's STREAMINFO, bytes [start + 26, start + 42), IN PLACE on the device; returns `compressed`.  Raises
    ValueError, with nothing written, if a stream does not begin with "fLaC" and a STREAMINFO block."""
    torch = _torch()
    if compressed.dtype != torch.uint8 or digests.dtype != torch.uint8:
        raise ValueError("compressed and digests should be of type uint8")
    if starts.dtype != torch.int64:
        raise ValueError("starts should be of type int64")
    n_stream = int(np.prod(starts.shape))
    if digests.numel() != 16 * n_stream:
        raise ValueError("digests need sixteen bytes per stream")
    if not (compressed.is_contiguous() and starts.is_contiguous() and digests.is_contiguous()):
        raise ValueError("Only C-contiguous arrays are supported")
    dev = compressed.device
    if not (compressed.is_cuda and starts.device == dev and digests.device == dev):
        raise RuntimeError("sign_streams_device needs compressed, starts and digests on the same GPU")
    with _on_device(dev):
        errcode = _lib.lib().fa_sign_streams_device(_dp(compressed), compressed.numel(), _dp(starts), n_stream, _dp(digests), _stream_ptr())
    if errcode == 8192:  # FA_ERROR_DECODE_INIT
        raise ValueError("Signing needs streams that start with fLaC and a STREAMINFO block inside the compressed bytes")
    if errcode != 0:
        raise RuntimeError(f"Signing failed, return code = {errcode}")
    return compressed


def check_md5_device(compressed, starts, nbytes, stream_size, is_int64=False, return_digests=False, verify=None, max_temp_bytes=None):
    """Check device-resident streams against the MD5 signature in their STREAMINFO -- the end-to-end check of `flac -t`,
    the only one in the format that does not depend on the bitstream: the store is decoded in column chunks (each a
    whole number of 64-byte blocks, the decoded chunk under `max_temp_bytes`, default 256 MiB), every chunk is hashed
    by the resumable md5 kernel, and the digests are compared with the stored ones (fa_check_md5_device).

    Returns an int8 tensor of the shape of `starts`: 1 = the stream decodes to the samples that were signed, 0 = it
    does not, -1 = unsigned (the field is zero: every store written with signing off), -2 = not checkable: not 32 bits
    per sample (libFLAC hashes those at ceil(bps / 8) bytes per sample; they decode here to int32), or not the channel
    count of the call (is_int64: two).  With `return_digests` also the computed digests, uint8 of shape starts.shape +
    (16,) (zero for -2).  A store with nothing to decide is not decoded.  `verify`: the decoder's frame CRC-16 check, as
    decode_flac_device takes it; decode errors raise RuntimeError as there.  Streams of several block sizes are checked
    one block size at a time; with more than one column chunk each of these needs a single block size, as ranged decodes do."""
    torch = _torch()
    if compressed.dtype != torch.uint8:
        raise ValueError("Compressed data should be of type uint8")
    if starts.dtype != torch.int64 or nbytes.dtype != torch.int64:
        raise ValueError("starts and nbytes should be of type int64")
    if starts.shape != nbytes.shape:
        raise ValueError("starts and nbytes must have the same shape")
    if not (compressed.is_contiguous() and starts.is_contiguous() and nbytes.is_contiguous()):
        raise ValueError("Only C-contiguous arrays are supported")
    if stream_size <= 0:
        raise ValueError("You must specify the non-zero stream size")
    n_stream = int(np.prod(starts.shape))
    if n_stream <= 0:
        raise ValueError("starts needs at least one stream")
    dev = compressed.device
    if not (compressed.is_cuda and starts.device == dev and nbytes.device == dev):
        raise RuntimeError("check_md5_device needs compressed, starts and nbytes on the same GPU")
    status = torch.empty(n_stream, dtype=torch.int8, device=dev)
    digests = torch.empty((n_stream, 16), dtype=torch.uint8, device=dev) if return_digests else None
    cap = 0 if max_temp_bytes is None else int(max_temp_bytes)
    with _on_device(dev):
        errcode = _lib.lib().fa_check_md5_device(
            _dp(compressed), compressed.numel(), _dp(starts), _dp(nbytes), n_stream, stream_size, 2 if is_int64 else 1, cap,
            _dp(status), _dp(digests), _stream_ptr(), _verify_arg(verify))
    if errcode != 0:
        # streams of different block sizes: one call per block size (see _blocksize_classes), rows scattered back
        st, nb = starts.reshape(-1), nbytes.reshape(-1)
        groups = None
        if n_stream > 1 and bool(((st >= 0) & (nb >= 12) & (st + nb <= compressed.numel())).all()):
            groups = _blocksize_classes(compressed[st[:, None] + torch.arange(12, device=dev)[None, :]].cpu().numpy())
        if groups is None:
            raise RuntimeError(f"Decoding failed, return code = {errcode}")
        for g in groups:
            gi = torch.from_numpy(g).to(dev)
            part = check_md5_device(compressed, st[gi].contiguous(), nb[gi].contiguous(), stream_size, is_int64=is_int64,
                                    return_digests=return_digests, verify=verify, max_temp_bytes=max_temp_bytes)
            if return_digests:
                status[gi], digests[gi] = part
            else:
                status[gi] = part
    status = status.reshape(starts.shape)
    return (status, digests.reshape(tuple(starts.shape) + (16,))) if return_digests else status


def _device_regroup(errcode, out, compressed, starts, nbytes, stream_size, first_sample, last_sample, offsets, gains, is_int64, verify):
    """A failed decode call whose streams differ in block size: one launch per block size (see _blocksize_classes),
    rows scattered back into `out`, each launch with the caller's `verify`.  Anything else raises the reference's error."""
    torch = _torch()
    st, nb = starts.reshape(-1), nbytes.reshape(-1)
    n_stream = st.numel()
    groups = None
    if n_stream > 1 and bool(((st >= 0) & (nb >= 12) & (st + nb <= compressed.numel())).all()):
        groups = _blocksize_classes(compressed[st[:, None] + torch.arange(12, device=st.device)[None, :]].cpu().numpy())
    if groups is None:
        raise RuntimeError(f"Decoding failed, return code = {errcode}")
    out2 = out.reshape(n_stream, -1)
    for g in groups:
        gi = torch.from_numpy(g).to(st.device)
        out2[gi] = decode_flac_device(
            compressed, st[gi].contiguous(), nb[gi].contiguous(), stream_size, first_sample, last_sample,
            offsets=None if offsets is None else offsets.reshape(-1)[gi.to(offsets.device)],
            gains=None if gains is None else gains.reshape(-1)[gi.to(gains.device)], is_int64=is_int64, verify=verify,
        )
    return out


def decode_flac_device(compressed, starts, nbytes, stream_size, first_sample=-1, last_sample=-1, offsets=None, gains=None,
                       is_int64=False, verify=None):
    """Decode device-resident streams into an int32 tensor (or float32 when offsets/gains are
    given: the int->float restore of utils.c:350-368 is fused into the store).  is_int64:
    two-channel streams -> int64 (or float64 with float64 offsets/gains, utils.c:329-348).
    verify: True / False = check every frame's CRC-16 or not; None = the default of set_decode_verify."""
    torch = _torch()
    vfy = _verify_arg(verify)
    if compressed.dtype != torch.uint8:
        raise RuntimeError("Compressed data should be of type uint8")
    if starts.dtype != torch.int64:
        raise RuntimeError("starts data should be of type int64")
    if nbytes.dtype != torch.int64:
        raise RuntimeError("nbytes data should be of type int64")
    if not (compressed.is_contiguous() and starts.is_contiguous() and nbytes.is_contiguous()):
        raise RuntimeError("Only C-contiguous arrays are supported")
    if stream_size <= 0:
        raise RuntimeError("You must specify the non-zero output stream size")
    n_decode = stream_size
    if first_sample >= 0 and last_sample >= 0:
        if last_sample > stream_size:
            raise RuntimeError("last_sample is beyond end of stream")
        if first_sample > stream_size - 1:
            raise RuntimeError("first_sample is beyond last element of stream")
        if first_sample >= last_sample:
            raise RuntimeError("first_sample is larger than last_sample")
        n_decode = last_sample - first_sample
    if (offsets is None) != (gains is None):
        raise RuntimeError("When specifying offsets, you must also provide the gains")
    n_stream = int(np.prod(starts.shape))
    shape = tuple(starts.shape) + (n_decode,)
    dev = compressed.device
    L = _lib.lib()
    if is_int64:
        with _on_device(dev):
            if offsets is None:
                out = torch.empty(shape, dtype=torch.int64, device=dev)
                errcode = L.fa_decode_i64_device(
                    _dp(compressed), compressed.numel(), _dp(starts), _dp(nbytes), n_stream, stream_size, first_sample,
                    last_sample, _dp(out), None, None, None, _stream_ptr(), vfy,
                )
            else:
                out = torch.empty(shape, dtype=torch.float64, device=dev)
                offsets = offsets.to(device=dev, dtype=torch.float64).contiguous()
                gains = gains.to(device=dev, dtype=torch.float64).contiguous()
                errcode = L.fa_decode_i64_device(
                    _dp(compressed), compressed.numel(), _dp(starts), _dp(nbytes), n_stream, stream_size, first_sample,
                    last_sample, None, _dp(out), _dp(offsets), _dp(gains), _stream_ptr(), vfy,
                )
        if errcode != 0:
            return _device_regroup(errcode, out, compressed, starts, nbytes, stream_size, first_sample, last_sample, offsets, gains, True, verify)
        return out
    with _on_device(dev):
        if offsets is None:
            out = torch.empty(shape, dtype=torch.int32, device=dev)
            errcode = L.fa_decode_i32_device(
                _dp(compressed), compressed.numel(), _dp(starts), _dp(nbytes), n_stream, stream_size, first_sample, last_sample,
                _dp(out), None, None, None, _stream_ptr(), vfy,
            )
        else:
            out = torch.empty(shape, dtype=torch.float32, device=dev)
            offsets = offsets.to(device=dev, dtype=torch.float32).contiguous()
            gains = gains.to(device=dev, dtype=torch.float32).contiguous()
            errcode = L.fa_decode_i32_device(
                _dp(compressed), compressed.numel(), _dp(starts), _dp(nbytes), n_stream, stream_size, first_sample, last_sample,
                None, _dp(out), _dp(offsets), _dp(gains), _stream_ptr(), vfy,
            )
    if errcode != 0:
        return _device_regroup(errcode, out, compressed, starts, nbytes, stream_size, first_sample, last_sample, offsets, gains, False, verify)
    return out


def _store_checks(compressed, starts, nbytes, stream_size):
    """The argument checks of decode_flac_device on a store."""
    torch = _torch()
    if compressed.dtype != torch.uint8:
        raise RuntimeError("Compressed data should be of type uint8")
    if starts.dtype != torch.int64:
        raise RuntimeError("starts data should be of type int64")
    if nbytes.dtype != torch.int64:
        raise RuntimeError("nbytes data should be of type int64")
    if not (compressed.is_contiguous() and starts.is_contiguous() and nbytes.is_contiguous()):
        raise RuntimeError("Only C-contiguous arrays are supported")
    if stream_size <= 0:
        raise RuntimeError("You must specify the non-zero output stream size")


def _block_size_arg(compressed, starts, nbytes, block_size):
    """The block size of a damage-map call: the caller's, or the most common STREAMINFO block size among the streams
    whose first 12 bytes can be read (found on the host, as _blocksize_classes reads them)."""
    if block_size is not None:
        if not 1 <= int(block_size) <= 65535:
            raise RuntimeError("block_size must lie in 1..65535")
        return int(block_size)
    torch = _torch()
    st, nb = starts.reshape(-1), nbytes.reshape(-1)
    ok = (st >= 0) & (nb >= 12) & (st <= compressed.numel() - 12)
    st = st[ok]
    b = None
    if st.numel():
        b = common_block_size(compressed[st[:, None] + torch.arange(12, device=st.device)[None, :]].cpu().numpy())
    if b is None:
        raise RuntimeError("No stream header gives a block size: pass block_size")
    return b


def frame_status_device(compressed, starts, nbytes, stream_size, is_int64=False, block_size=None):
    """The damage map of a device-resident store: a uint8 tensor of shape starts.shape + (nf,), nf = ceil(stream_size /
    block_size), one status per (stream, frame) -- 0 (FRAME_OK), FRAME_UNLOCATED, or FRAME_HEADER | FRAME_CRC16 bits
    (flacarray_amd/scrub.py; the rule is in DESIGN.md, "Damage map and salvage").  Computed on the GPU from nothing but
    the store, and never raises for damage: a frame is decodable exactly when its status is 0.  As strong as CRC-16
    (a random change escapes with probability 2^-16; check_md5_device is the stronger check).  block_size=None: the
    most common STREAMINFO block size among the streams whose header can be read."""
    torch = _torch()
    _store_checks(compressed, starts, nbytes, stream_size)
    dev = compressed.device
    with _on_device(dev):
        B = _block_size_arg(compressed, starts, nbytes, block_size)
        nf = -(-stream_size // B)
        n_stream = int(np.prod(starts.shape))
        status = torch.empty(tuple(starts.shape) + (nf,), dtype=torch.uint8, device=dev)
        errcode = _lib.lib().fa_frame_status_device(_dp(compressed), compressed.numel(), _dp(starts), _dp(nbytes), n_stream, stream_size,
                                                    2 if is_int64 else 1, B, _dp(status), _stream_ptr())
    if errcode != 0:
        raise RuntimeError(f"Frame status failed, return code = {errcode}")
    return status


def decode_flac_salvage_device(compressed, starts, nbytes, stream_size, first_sample=-1, last_sample=-1, offsets=None, gains=None,
                               is_int64=False, fill=None, block_size=None):
    """Decode through errors: (out, status).  `status` is frame_status_device's map of the whole store; `out` has the
    dtype and shape of decode_flac_device(...) -- every frame of status 0 decoded exactly, the samples of every other
    frame set to `fill` (None: 0 for integer output, NaN for float output).  Argument checks and their messages are
    decode_flac_device's; damage never raises."""
    torch = _torch()
    _store_checks(compressed, starts, nbytes, stream_size)
    n_decode = stream_size
    if first_sample >= 0 and last_sample >= 0:
        if last_sample > stream_size:
            raise RuntimeError("last_sample is beyond end of stream")
        if first_sample > stream_size - 1:
            raise RuntimeError("first_sample is beyond last element of stream")
        if first_sample >= last_sample:
            raise RuntimeError("first_sample is larger than last_sample")
        n_decode = last_sample - first_sample
    if (offsets is None) != (gains is None):
        raise RuntimeError("When specifying offsets, you must also provide the gains")
    n_stream = int(np.prod(starts.shape))
    dev = compressed.device
    if offsets is None:
        np_dt, t_dt = (np.int64, torch.int64) if is_int64 else (np.int32, torch.int32)
    else:
        np_dt, t_dt = (np.float64, torch.float64) if is_int64 else (np.float32, torch.float32)
    if fill is None:
        fill = 0 if offsets is None else np.nan
    fill_value = np.array([fill], dtype=np_dt)
    L = _lib.lib()
    with _on_device(dev):
        B = _block_size_arg(compressed, starts, nbytes, block_size)
        nf = -(-stream_size // B)
        status = torch.empty(tuple(starts.shape) + (nf,), dtype=torch.uint8, device=dev)
        out = torch.empty(tuple(starts.shape) + (n_decode,), dtype=t_dt, device=dev)
        if offsets is not None:
            offsets = offsets.to(device=dev, dtype=t_dt).contiguous()
            gains = gains.to(device=dev, dtype=t_dt).contiguous()
        fn = L.fa_decode_salvage_i64_device if is_int64 else L.fa_decode_salvage_i32_device
        o_int, o_float = (_dp(out), None) if offsets is None else (None, _dp(out))
        errcode = fn(_dp(compressed), compressed.numel(), _dp(starts), _dp(nbytes), n_stream, stream_size, first_sample, last_sample,
                     o_int, o_float, _dp(offsets), _dp(gains), B, _ptr(fill_value), _dp(status), _stream_ptr())
    if errcode != 0:
        raise RuntimeError(f"Decoding failed, return code = {errcode}")
    return out, status


def decode_slices_device(compressed, starts, nbytes, stream_size, slice_stream, slice_first, slice_count, offsets=None, gains=None,
                         is_int64=False, verify=None):
    """Batched random access: slice i = samples [first[i], first[i]+count[i]) of (flat) stream
    slice_stream[i].  Returns (flat output tensor, int64 numpy array of output offsets).  The
    reference needs one decode call per slice (decompress.py:42-48)."""
    torch = _torch()
    slice_stream = np.ascontiguousarray(slice_stream, dtype=np.int64)
    slice_first = np.ascontiguousarray(slice_first, dtype=np.int64)
    slice_count = np.ascontiguousarray(slice_count, dtype=np.int64)
    n = slice_stream.shape[0]
    out_off = np.zeros(n, dtype=np.int64)
    if n > 1:
        np.cumsum(slice_count[:-1], out=out_off[1:])
    total = int(slice_count.sum())
    dev = compressed.device
    n_stream = int(np.prod(starts.shape))
    L = _lib.lib()
    f32 = offsets is not None
    ft, it = (torch.float64, torch.int64) if is_int64 else (torch.float32, torch.int32)
    out = torch.empty(total, dtype=ft if f32 else it, device=dev)
    if f32:
        # per-stream offsets / gains; the kernel looks them up by the slice's stream
        soff = offsets.reshape(-1).to(device=dev, dtype=ft).contiguous()
        sgain = gains.reshape(-1).to(device=dev, dtype=ft).contiguous()
    with _on_device(dev):
        errcode = (L.fa_decode_slices_i64_device if is_int64 else L.fa_decode_slices_i32_device)(
            _dp(compressed), compressed.numel(), _dp(starts), _dp(nbytes), n_stream, stream_size, n,
            ctypes.c_void_p(slice_stream.ctypes.data), ctypes.c_void_p(slice_first.ctypes.data),
            ctypes.c_void_p(slice_count.ctypes.data), ctypes.c_void_p(out_off.ctypes.data),
            None if f32 else _dp(out), _dp(out) if f32 else None, _dp(soff) if f32 else None, _dp(sgain) if f32 else None,
            _stream_ptr(), _verify_arg(verify),
        )
    if errcode != 0:
        raise RuntimeError(f"Decoding failed, return code = {errcode}")
    return out, out_off


def _stream_indices(streams, n_stream):
    """`streams` (None, or a 1-D integer array or tensor of flat C-order stream indices) as an int64 numpy array or None;
    an index out of range or named twice raises ValueError."""
    if streams is None:
        return None
    idx = streams.detach().cpu().numpy() if isinstance(streams, _torch().Tensor) else np.asarray(streams)
    if idx.ndim != 1 or (idx.size and idx.dtype.kind not in "iu"):
        raise ValueError("streams should be a 1-D array of integer stream indices")
    idx = idx.astype(np.int64)
    if idx.size and (idx.min() < 0 or idx.max() >= n_stream):
        raise ValueError(f"streams holds an index outside [0, {n_stream})")
    if np.unique(idx).size != idx.size:
        raise ValueError("streams names a stream twice")
    return idx


def _reduce_args(n_stream, stream_size, width, first_sample, last_sample, streams):
    """The argument checks of the binned reduction (ValueError, before anything touches the GPU).  Returns (first, last,
    width, nbins, stream indices as an int64 numpy array or None)."""
    stream_size = int(stream_size)
    if stream_size <= 0:
        raise ValueError("You must specify the non-zero stream size")
    first = int(first_sample)
    last = stream_size if last_sample is None else int(last_sample)
    if first < 0 or last > stream_size or first >= last:
        raise ValueError(f"samples [{first}, {last}) are not a non-empty range inside streams of {stream_size} samples")
    n = last - first
    if width is None:
        width = n
    width = int(width)
    if width < 1:
        raise ValueError("width should be at least one sample")
    width = min(width, n)
    return first, last, width, -(-n // width), _stream_indices(streams, n_stream)


def _reduce_outputs(rows, nbins, wide, dev):
    torch = _torch()
    mk = lambda: torch.empty((rows, nbins), dtype=torch.int64, device=dev)  # noqa: E731
    return mk(), mk(), mk(), (None if wide else mk()), (None if wide else mk())


def reduce_flac_device(compressed, starts, nbytes, stream_size, width=None, first_sample=0, last_sample=None, streams=None,
                       is_int64=False, verify=None, max_temp_bytes=None):
    """Binned min / max / sum / sum of squares of what device-resident streams decode to, without a decoded copy
    (fa_reduce_i32_device / fa_reduce_i64_device).  Samples [first_sample, last_sample) (default: everything) of every
    stream, or of the streams that `streams` names (1-D flat indices, no repeats; rows come in that order), are cut into
    nbins = ceil(n / width) bins of `width` samples, the last one possibly short; width=None is one bin.

    Returns (min, max, sum, sumsq_hi, sumsq_lo): int64 device tensors of shape (rows, nbins) over the decoded INTEGERS
    (for a float store the quantised ones).  min / max are exact; sum equals np.sum(x, dtype=np.int64) -- exact for
    one-channel streams, modulo 2^64 for two-channel ones (is_int64); the limbs (None for two-channel streams) are the
    exact sums of x*x mod 2^32 and x*x >> 32, so that the sum of squares is sumsq_hi * 2^32 + sumsq_lo.  An empty
    `streams` returns tensors of shape (0, nbins).

    One-channel streams are reduced inside the decoder, at about the cost of a decode and with nothing but the bins
    written.  Two-channel streams go through decoded column chunks of whole frames that stay under `max_temp_bytes`
    (default 256 MiB): that keeps the extra memory small but is SLOWER than decode_flac_device followed by torch
    reductions when the whole decoded array would fit (at 1024 x 2^20 int64: 59 ms against 16; with a cap that holds the whole
    range, 13 ms: profiles/reduce.md), because a chunk of few frames does not fill the decoder.  `verify` is the
    decoder's frame CRC-16 check; argument errors raise ValueError before any GPU work, decode failures the decoder's
    RuntimeError.  Streams of several block sizes are reduced one block size at a time."""
    torch = _torch()
    if compressed.dtype != torch.uint8:
        raise ValueError("Compressed data should be of type uint8")
    if starts.dtype != torch.int64 or nbytes.dtype != torch.int64:
        raise ValueError("starts and nbytes should be of type int64")
    if starts.shape != nbytes.shape:
        raise ValueError("starts and nbytes must have the same shape")
    n_stream = int(np.prod(starts.shape))
    if n_stream <= 0:
        raise ValueError("starts needs at least one stream")
    first, last, width, nbins, idx = _reduce_args(n_stream, stream_size, width, first_sample, last_sample, streams)
    if not (compressed.is_contiguous() and starts.is_contiguous() and nbytes.is_contiguous()):
        raise ValueError("Only C-contiguous arrays are supported")
    dev = compressed.device
    if not (compressed.is_cuda and starts.device == dev and nbytes.device == dev):
        raise RuntimeError("reduce_flac_device needs compressed, starts and nbytes on the same GPU")
    rows = n_stream if idx is None else int(idx.size)
    mn, mx, sm, qh, ql = _reduce_outputs(rows, nbins, is_int64, dev)
    if rows == 0:
        return mn, mx, sm, qh, ql
    sel = None if idx is None else torch.from_numpy(idx).to(dev)
    cap = 0 if max_temp_bytes is None else int(max_temp_bytes)
    L = _lib.lib()
    with _on_device(dev):
        if is_int64:
            errcode = L.fa_reduce_i64_device(_dp(compressed), compressed.numel(), _dp(starts), _dp(nbytes), n_stream, stream_size, first, last,
                                             width, rows, _dp(sel), cap, _dp(mn), _dp(mx), _dp(sm), _stream_ptr(), _verify_arg(verify))
        else:
            errcode = L.fa_reduce_i32_device(_dp(compressed), compressed.numel(), _dp(starts), _dp(nbytes), n_stream, stream_size, first, last,
                                             width, rows, _dp(sel), _dp(mn), _dp(mx), _dp(sm), _dp(qh), _dp(ql), _stream_ptr(),
                                             _verify_arg(verify))
    if errcode != 0:
        # streams of different block sizes: one call per block size (see _blocksize_classes), rows scattered back
        st, nb = starts.reshape(-1), nbytes.reshape(-1)
        groups = None
        if n_stream > 1 and bool(((st >= 0) & (nb >= 12) & (st + nb <= compressed.numel())).all()):
            groups = _blocksize_classes(compressed[st[:, None] + torch.arange(12, device=dev)[None, :]].cpu().numpy())
        if groups is None:
            raise RuntimeError(f"Decoding failed, return code = {errcode}")
        for g in groups:
            if idx is None:
                at, local = g, None
            else:
                at = np.flatnonzero(np.isin(idx, g))  # rows of the result that name a stream of this class
                if at.size == 0:
                    continue
                local = np.searchsorted(g, idx[at])
            gi = torch.from_numpy(g).to(dev)
            part = reduce_flac_device(compressed, st[gi].contiguous(), nb[gi].contiguous(), stream_size, width, first, last, streams=local,
                                      is_int64=is_int64, verify=verify, max_temp_bytes=max_temp_bytes)
            ai = torch.from_numpy(at).to(dev)
            for out, p in zip((mn, mx, sm, qh, ql), part):
                if out is not None:
                    out[ai] = p
    return mn, mx, sm, qh, ql


def xsum_plan(labels, n_groups):
    """The host plan of a fold across streams (pure: no GPU).  `labels[i]` in [0, n_groups) is the group of the i-th selected
    stream.  Returns (perm, rows, count): `perm` (int64) the positions 0..len(labels)-1 stable-sorted by label, so that a
    group's streams are adjacent and keep the caller's order; `rows` (int64 [n_rows, 3]) one entry per 64 lanes of one
    group -- [group, first position in perm, real lanes (1..64)] -- each group padded to a multiple of 64 lanes and an
    empty group having no row; `count` (int64 [n_groups]) the streams per group."""
    lab = np.asarray(labels, dtype=np.int64).reshape(-1)
    n_groups = int(n_groups)
    if n_groups < 1:
        raise ValueError("n_groups should be at least 1")
    if lab.size and (lab.min() < 0 or lab.max() >= n_groups):
        raise ValueError(f"groups holds a label outside [0, {n_groups})")
    perm = np.argsort(lab, kind="stable").astype(np.int64)
    count = np.bincount(lab, minlength=n_groups).astype(np.int64)
    start = np.concatenate([[0], np.cumsum(count)[:-1]]).astype(np.int64)
    rows = [(g, int(start[g]) + at, min(64, int(count[g]) - at)) for g in range(n_groups) for at in range(0, int(count[g]), 64)]
    return perm, np.asarray(rows, dtype=np.int64).reshape(-1, 3), count


def _xsum_args(n_stream, stream_size, groups, n_groups, first_sample, last_sample, streams, squares, is_int64):
    """The argument checks of the fold across streams (ValueError, before anything touches the GPU).  Returns (first, last,
    n_groups, order, rows, count): `order` the selected stream indices sorted by group and `rows` the plan's row table
    (xsum_plan), int64 numpy arrays.  Unlike the reductions along a stream, an empty range first == last is accepted."""
    stream_size = int(stream_size)
    if stream_size <= 0:
        raise ValueError("You must specify the non-zero stream size")
    first = int(first_sample)
    last = stream_size if last_sample is None else int(last_sample)
    if first < 0 or last > stream_size or first > last:
        raise ValueError(f"samples [{first}, {last}) are not a range inside streams of {stream_size} samples")
    if squares and is_int64:
        raise ValueError("two-channel (64-bit) stores carry no sum of squares: pass squares=False")
    idx = _stream_indices(streams, n_stream)
    if idx is None:
        idx = np.arange(n_stream, dtype=np.int64)
    if groups is None:
        n_groups = 1 if n_groups is None else int(n_groups)
        lab = np.zeros(idx.size, dtype=np.int64)
    else:
        lab = groups.detach().cpu().numpy() if isinstance(groups, _torch().Tensor) else np.asarray(groups)
        if lab.ndim != 1 or lab.size != idx.size or (lab.size and lab.dtype.kind not in "iu"):
            raise ValueError(f"groups should hold one integer label per selected stream ({idx.size})")
        lab = lab.astype(np.int64)
        if n_groups is None:
            if lab.size and lab.min() < 0:
                raise ValueError("groups holds a negative label")
            n_groups = int(lab.max()) + 1 if lab.size else 1
    perm, rows, count = xsum_plan(lab, n_groups)
    return first, last, int(n_groups), idx[perm], rows, count


def _xsum_outputs(n_groups, n, squares, dev):
    torch = _torch()
    mk = lambda: torch.empty((n_groups, n), dtype=torch.int64, device=dev)  # noqa: E731
    return mk(), (mk() if squares else None), (mk() if squares else None)


def common_mode_flac_device(compressed, starts, nbytes, stream_size, groups=None, n_groups=None, first_sample=0, last_sample=None,
                            streams=None, squares=True, is_int64=False, verify=None, max_temp_bytes=None):
    """Per-sample sums ACROSS device-resident streams, without a decoded copy (fa_xsum_i32_device / fa_xsum_i64_device):
    for every group g and every sample j of [first_sample, last_sample) (default: everything; an empty range gives
    (G, 0) tensors) the sum over the group's streams of what they decode to at j.  `streams`: 1-D flat stream indices, no
    repeats (default: all).  `groups`: None for one group, or one integer label in [0, n_groups) per selected stream, in
    any order; n_groups defaults to the largest label + 1 and groups may be empty.

    Returns (sum, sumsq_hi, sumsq_lo): int64 device tensors of shape (G, n) over the decoded INTEGERS (for a float store
    the quantised ones).  sum equals np.sum(x[sel_g], axis=0, dtype=np.int64) -- exact for one-channel streams, modulo
    2^64 for two-channel ones (is_int64); the limbs (None for two-channel streams or squares=False) are the exact sums of
    x*x >> 32 and x*x mod 2^32, as reduce_flac_device's.  The tensors are zero-filled by the library.

    One-channel streams are summed inside the decoder: a wavefront decodes the same frame of 64 streams of one group and
    folds every column of its tile across its lanes (K7X), adding to the result with 64-bit atomics: at 4096 x 2^20 int32
    6.95 ms with one group, 7.11 with 64 groups of 64, 6.43 with squares=False (the bare decode: 6.41 ms; decoding 512 rows
    at a time and accumulating torch.sum(dim=0): 28-37 ms and 3-6 GiB; profiles/common_mode.md).  Two-channel streams go through decoded column chunks under `max_temp_bytes` (default
    256 MiB), as reduce_flac_device's do, and are SLOWER than decode_flac_device followed by torch.sum(dim=0) where the
    decoded copy fits (1024 x 2^20 int64: 65 ms against 12.5; 12.8 with a cap that holds the whole range).  All streams
    must share one block size.  Argument errors raise ValueError
    before any GPU work, decode failures the decoder's RuntimeError."""
    torch = _torch()
    if compressed.dtype != torch.uint8:
        raise ValueError("Compressed data should be of type uint8")
    if starts.dtype != torch.int64 or nbytes.dtype != torch.int64:
        raise ValueError("starts and nbytes should be of type int64")
    if starts.shape != nbytes.shape:
        raise ValueError("starts and nbytes must have the same shape")
    n_stream = int(np.prod(starts.shape))
    if n_stream <= 0:
        raise ValueError("starts needs at least one stream")
    first, last, G, order, rows, _ = _xsum_args(n_stream, stream_size, groups, n_groups, first_sample, last_sample, streams, squares, is_int64)
    if not (compressed.is_contiguous() and starts.is_contiguous() and nbytes.is_contiguous()):
        raise ValueError("Only C-contiguous arrays are supported")
    dev = compressed.device
    if not (compressed.is_cuda and starts.device == dev and nbytes.device == dev):
        raise RuntimeError("common_mode_flac_device needs compressed, starts and nbytes on the same GPU")
    sm, qh, ql = _xsum_outputs(G, last - first, squares, dev)
    if last == first:
        return sm, qh, ql
    d_order = torch.from_numpy(order).to(dev)
    d_rows = torch.from_numpy(rows).to(dev)
    cap = 0 if max_temp_bytes is None else int(max_temp_bytes)
    L = _lib.lib()
    with _on_device(dev):
        if is_int64:
            errcode = L.fa_xsum_i64_device(_dp(compressed), compressed.numel(), _dp(starts), _dp(nbytes), n_stream, stream_size, first, last,
                                           int(order.size), _dp(d_order), int(rows.shape[0]), _dp(d_rows), G, cap, _dp(sm), _stream_ptr(),
                                           _verify_arg(verify))
        else:
            errcode = L.fa_xsum_i32_device(_dp(compressed), compressed.numel(), _dp(starts), _dp(nbytes), n_stream, stream_size, first, last,
                                           int(order.size), _dp(d_order), int(rows.shape[0]), _dp(d_rows), G, _dp(sm), _dp(qh), _dp(ql),
                                           _stream_ptr(), _verify_arg(verify))
    if errcode != 0:
        raise RuntimeError(f"Decoding failed, return code = {errcode}")
    return sm, qh, ql


_INT32_MIN, _INT32_MAX = -(1 << 31), (1 << 31) - 1
_INT64_MIN, _INT64_MAX = -(1 << 63), (1 << 63) - 1


def dot_template_limbs(templates):
    """The host split of integer templates into what the int32 kernel multiplies (pure: no GPU).  `templates` is an
    integer array [K, n] with values anywhere in int64.  A template that fits int32 stays as it is, one plane; any other is
    split T = t0 + t1 * 2^31 + t2 * 2^62 with t0, t1 in [0, 2^31) and t2 in [-2, 1].  Planes that are all zero are dropped.
    Returns (planes, index): `planes` int32 [M, n], and `index` int64 [M, 2] holding, per plane, the template it belongs
    to and its limb number j (weight 2^(31 j)).  dot_template_unlimbs is the inverse on the products."""
    T = np.asarray(templates)
    if T.ndim != 2:
        raise ValueError("templates should be a [K, n] array")
    if T.dtype.kind not in "iu":
        raise TypeError("templates should be an integer array")
    if T.dtype.kind == "u" and T.size and int(T.max()) > _INT64_MAX:
        raise ValueError("templates holds a value outside int64")
    T = T.astype(np.int64)
    planes, index = [], []
    for k in range(T.shape[0]):
        row = T[k]
        if row.size == 0 or (int(row.min()) >= _INT32_MIN and int(row.max()) <= _INT32_MAX):
            if np.any(row != 0):
                planes.append(row.astype(np.int32))
                index.append((k, 0))
            continue
        for j, limb in enumerate((row & 0x7FFFFFFF, (row >> 31) & 0x7FFFFFFF, row >> 62)):
            if np.any(limb != 0):
                planes.append(limb.astype(np.int32))
                index.append((k, j))
    return (np.asarray(planes, dtype=np.int32).reshape(len(planes), T.shape[1]), np.asarray(index, dtype=np.int64).reshape(-1, 2))


def dot_template_unlimbs(products, index, n_templates):
    """The inverse of dot_template_limbs on the results: `products` [rows, M] (Python integers, one column per plane) and
    the split's `index` give the object array [rows, n_templates] of sum_m products[:, m] * 2^(31 j_m) per template.  A
    template whose planes were all dropped (all zeros) gives 0."""
    P = np.asarray(products, dtype=object)
    out = np.zeros((P.shape[0], int(n_templates)), dtype=object)
    for m, (k, j) in enumerate(np.asarray(index, dtype=np.int64).reshape(-1, 2)):
        out[:, int(k)] = out[:, int(k)] + P[:, m] * (1 << (31 * int(j)))
    return out


def dot_exact(hi, lo=None):
    """The exact inner products as an object array of Python integers, from what the device calls return: (hi, lo)
    [rows, K] of a one-channel store -- hi * 2^32 + lo with lo unsigned -- or the [rows, K, 4] array of a two-channel one."""
    as_np = lambda t: t.detach().cpu().numpy() if hasattr(t, "detach") else np.asarray(t)  # noqa: E731
    signed = lambda a: a.astype(np.int64).astype(object)  # noqa: E731
    unsigned = lambda a: np.ascontiguousarray(a).view(np.uint64).astype(object)  # noqa: E731
    if lo is None:
        o = as_np(hi)
        low = signed(o[..., 0]) * (1 << 32) + unsigned(o[..., 1])
        high = signed(o[..., 2]) * (1 << 32) + unsigned(o[..., 3])
        return high * (1 << 32) + low
    return signed(as_np(hi)) * (1 << 32) + unsigned(as_np(lo))


def _dot_templates(templates, n):
    """The `templates` argument of the public calls, checked (TypeError / ValueError, before anything touches the GPU):
    an integer array or tensor [K, n] or [n].  Returns (int64 numpy array [K, n], whether the K axis was missing)."""
    T = templates.detach().cpu().numpy() if isinstance(templates, _torch().Tensor) else np.asarray(templates)
    if T.dtype.kind == "f":
        raise TypeError("templates should be integers: the products are exact.  Quantise a float template T yourself, "
                        "np.rint(T * 2**k).astype(np.int64), and divide the result by 2**k")
    if T.dtype.kind == "O" and T.size and all(isinstance(v, (int, np.integer)) and not isinstance(v, bool) for v in T.reshape(-1)):
        if any(int(v) < _INT64_MIN or int(v) > _INT64_MAX for v in T.reshape(-1)):
            raise ValueError("templates holds a value outside int64")
        T = T.astype(np.int64)
    if T.dtype.kind not in "iu":
        raise TypeError(f"templates should be an integer array, not {T.dtype}")
    if T.dtype.kind == "u" and T.size and int(T.max()) > _INT64_MAX:
        raise ValueError("templates holds a value outside int64")
    single = T.ndim == 1
    if single:
        T = T.reshape(1, -1)
    if T.ndim != 2 or T.shape[0] < 1:
        raise ValueError("templates should be an array [K, n] or [n] with at least one template")
    if T.shape[1] != n:
        raise ValueError(f"templates hold {T.shape[1]} samples, the range [first, last) has {n}")
    return T.astype(np.int64), single


def _dot_args(n_stream, stream_size, first_sample, last_sample, streams):
    """The range and selection checks of the projections (ValueError, before anything touches the GPU).  Returns (first,
    last, order, rows): the selected stream indices (all of them by default) and the trivial plan of fa_dot_*."""
    stream_size = int(stream_size)
    if stream_size <= 0:
        raise ValueError("You must specify the non-zero stream size")
    first = int(first_sample)
    last = stream_size if last_sample is None else int(last_sample)
    if first < 0 or last > stream_size or first >= last:
        raise ValueError(f"samples [{first}, {last}) are not a non-empty range inside streams of {stream_size} samples")
    if last - first > 0xFFFFFFFF:
        raise ValueError("a range of more than 2^32 - 1 samples: split it and add the results")
    idx = _stream_indices(streams, n_stream)
    if idx is None:
        idx = np.arange(n_stream, dtype=np.int64)
    rows = np.asarray([(0, at, min(64, idx.size - at)) for at in range(0, idx.size, 64)], dtype=np.int64).reshape(-1, 3)
    return first, last, idx, rows


def _dot_i32_templates(templates, n):
    """The `templates` argument of the device calls, checked (TypeError / ValueError, before anything touches the GPU): an
    int32 array or tensor [K, n], K >= 1.  Returns it as a tensor."""
    torch = _torch()
    T = templates if isinstance(templates, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(templates))
    if T.dtype != torch.int32:
        raise TypeError("the device call takes int32 templates: FlacArray.dot splits wider ones (dot_template_limbs), and a "
                        "float template is quantised by its owner, np.rint(T * 2**k)")
    if T.ndim != 2 or T.shape[0] < 1 or T.shape[1] != n:
        raise ValueError(f"templates should be [K, {n}] with at least one template, not {tuple(T.shape)}")
    return T


def _dot_image(T, n, dev):
    """The device template image of fa_dot_*: int32 [n, ld], sample-major, ld the next multiple of 8 from K, padding
    columns zero.  `T`: _dot_i32_templates' tensor.  Returns (image, K, ld)."""
    torch = _torch()
    K = int(T.shape[0])
    ld = (K + 7) // 8 * 8
    img = torch.zeros((n, ld), dtype=torch.int32, device=dev)
    img[:, :K] = T.to(dev).t()
    return img, K, ld


def dot_flac_device(compressed, starts, nbytes, stream_size, templates, first_sample=0, last_sample=None, streams=None, is_int64=False,
                    verify=None, max_temp_bytes=None):
    """Exact inner products of device-resident streams with K templates, without a decoded copy (fa_dot_i32_device /
    fa_dot_i64_device): dot[r, k] = sum_j x[r, first_sample + j] * templates[k, j] over the decoded INTEGERS (for a float
    store the quantised ones).  `templates`: an int32 tensor or array [K, n], n = last_sample - first_sample exactly (K is
    unlimited; wider values: FlacArray.dot, or dot_template_limbs).  `streams`: 1-D flat stream indices, no repeats
    (default: all), one result row each, in the order given.

    Returns int64 device tensors: (hi, lo) of shape (rows, K) for one-channel streams -- dot = hi * 2^32 + lo with lo
    read as unsigned -- or one tensor (rows, K, 4) for two-channel streams (is_int64); dot_exact turns either into Python
    integers.  The tensors are zero-filled by the library.

    One-channel streams are multiplied inside the decoder (K7D): a wavefront decodes the same frame of 64 streams, so a
    sample's template values are the same for all its lanes and are read once per wave; 8 templates ride with one decode
    of the range, K templates cost ceil(K / 8) decodes (timings against the bare decode, reduce and decode-then-matmul:
    profiles/dot.md).  Two-channel streams go through decoded column chunks under `max_temp_bytes` (default 256 MiB).  All
    streams must share one block size.  Argument errors raise ValueError / TypeError before any GPU work, decode failures
    the decoder's RuntimeError."""
    torch = _torch()
    if compressed.dtype != torch.uint8:
        raise ValueError("Compressed data should be of type uint8")
    if starts.dtype != torch.int64 or nbytes.dtype != torch.int64:
        raise ValueError("starts and nbytes should be of type int64")
    if starts.shape != nbytes.shape:
        raise ValueError("starts and nbytes must have the same shape")
    n_stream = int(np.prod(starts.shape))
    if n_stream <= 0:
        raise ValueError("starts needs at least one stream")
    first, last, order, rows = _dot_args(n_stream, stream_size, first_sample, last_sample, streams)
    templates = _dot_i32_templates(templates, last - first)
    if not (compressed.is_contiguous() and starts.is_contiguous() and nbytes.is_contiguous()):
        raise ValueError("Only C-contiguous arrays are supported")
    dev = compressed.device
    if not (compressed.is_cuda and starts.device == dev and nbytes.device == dev):
        raise RuntimeError("dot_flac_device needs compressed, starts and nbytes on the same GPU")
    img, K, ld = _dot_image(templates, last - first, dev)
    shape = (int(order.size), K, 4) if is_int64 else (int(order.size), K)
    out = [torch.empty(shape, dtype=torch.int64, device=dev) for _ in range(1 if is_int64 else 2)]
    if order.size:
        d_order = torch.from_numpy(order).to(dev)
        d_rows = torch.from_numpy(rows).to(dev)
        L = _lib.lib()
        with _on_device(dev):
            if is_int64:
                errcode = L.fa_dot_i64_device(_dp(compressed), compressed.numel(), _dp(starts), _dp(nbytes), n_stream, stream_size, first, last,
                                              int(order.size), _dp(d_order), int(rows.shape[0]), _dp(d_rows), K, ld, _dp(img),
                                              0 if max_temp_bytes is None else int(max_temp_bytes), _dp(out[0]), _stream_ptr(), _verify_arg(verify))
            else:
                errcode = L.fa_dot_i32_device(_dp(compressed), compressed.numel(), _dp(starts), _dp(nbytes), n_stream, stream_size, first, last,
                                              int(order.size), _dp(d_order), int(rows.shape[0]), _dp(d_rows), K, ld, _dp(img), _dp(out[0]),
                                              _dp(out[1]), _stream_ptr(), _verify_arg(verify))
        if errcode != 0:
            raise RuntimeError(f"Decoding failed, return code = {errcode}")
    return out[0] if is_int64 else (out[0], out[1])


def _histogram_args(rows, lo, shift, nbins):
    """The argument checks of the value histogram (ValueError, before anything touches the GPU): `nbins` in 1..2048, `lo`
    and `shift` Python integers or integer arrays / tensors of length `rows`, lo inside int64, shift in 0..63.  Returns
    (nbins, lo as int64[rows], shift as int32[rows]) numpy arrays."""
    torch = _torch()
    if isinstance(nbins, bool) or not isinstance(nbins, (int, np.integer)) or not 1 <= int(nbins) <= 2048:
        raise ValueError("nbins should be an integer in 1..2048")

    def column(v, name, vmin, vmax, dt):
        if isinstance(v, torch.Tensor):
            v = v.detach().cpu().numpy()
        a = np.asarray(v)
        if a.dtype == object:
            if not all(isinstance(e, (int, np.integer)) and not isinstance(e, bool) for e in a.reshape(-1)):
                raise ValueError(f"{name} should hold integers")
        elif a.dtype.kind not in "iu":
            raise ValueError(f"{name} should be an integer or an integer array")
        if a.ndim > 1 or (a.ndim == 1 and a.size != rows):
            raise ValueError(f"{name} should be one integer or {rows} of them, one per row")
        if a.size and (min(int(e) for e in a.reshape(-1)) < vmin or max(int(e) for e in a.reshape(-1)) > vmax):
            raise ValueError(f"{name} holds a value outside [{vmin}, {vmax}]")
        return np.array(np.broadcast_to(a.astype(dt), (rows,)))  # (a copy: writable and contiguous)

    return int(nbins), column(lo, "lo", -(1 << 63), (1 << 63) - 1, np.int64), column(shift, "shift", 0, 63, np.int32)


def histogram_flac_device(compressed, starts, nbytes, stream_size, lo, shift, nbins, first_sample=0, last_sample=None, streams=None,
                          is_int64=False, verify=None, max_temp_bytes=None):
    """Counts per value bin of what device-resident streams decode to, without a decoded copy (fa_histogram_i32_device /
    fa_histogram_i64_device).  Samples [first_sample, last_sample) (default: everything) of every stream, or of the
    streams that `streams` names (rows in that order), are counted in `nbins` (1..2048) bins per row: a sample x of row r
    below lo[r] counts in below[r]; otherwise its bin is ((uint64)x - (uint64)lo[r]) >> shift[r], counted in
    counts[r, bin] or, from nbins on, in above[r].  `lo` (int64) and `shift` (0..63) are Python integers or integer
    arrays / tensors of length rows.  counts.sum(-1) + below + above == last_sample - first_sample for every row.

    Returns (counts [rows, nbins], below [rows], above [rows]): int64 device tensors over the decoded INTEGERS (for a
    float store the quantised ones); an empty `streams` returns shapes (0, nbins), (0,), (0,).

    One-channel streams are counted inside the decoder (K7H): a wave whose 64 frames belong to one row counts in a
    histogram in LDS and adds its non-zero words to `counts` once; a wave that holds several rows (streams shorter than
    64 frames) adds every sample straight to `counts`, which is correct and slow.  Two-channel streams go through decoded
    column chunks of whole frames under `max_temp_bytes` (default 256 MiB), as reduce_flac_device's do.  At 4096 x 2^20
    int32 a call takes 8.6 ms at any bin count (the bare decode: 6.6 ms) and 15.8 ms when every sample falls into one
    bin; at 1024 x 2^20 int64, 54-56 ms against 10.6 ms for the bare decode (profiles/histogram.md).  `verify` is the decoder's frame CRC-16 check; argument errors raise ValueError before
    any GPU work, decode failures the decoder's RuntimeError.  Streams of several block sizes go one block size at a
    time."""
    torch = _torch()
    if compressed.dtype != torch.uint8:
        raise ValueError("Compressed data should be of type uint8")
    if starts.dtype != torch.int64 or nbytes.dtype != torch.int64:
        raise ValueError("starts and nbytes should be of type int64")
    if starts.shape != nbytes.shape:
        raise ValueError("starts and nbytes must have the same shape")
    n_stream = int(np.prod(starts.shape))
    if n_stream <= 0:
        raise ValueError("starts needs at least one stream")
    first, last, _, _, idx = _reduce_args(n_stream, stream_size, None, first_sample, last_sample, streams)
    rows = n_stream if idx is None else int(idx.size)
    nbins, lo_h, shift_h = _histogram_args(rows, lo, shift, nbins)
    if not (compressed.is_contiguous() and starts.is_contiguous() and nbytes.is_contiguous()):
        raise ValueError("Only C-contiguous arrays are supported")
    dev = compressed.device
    if not (compressed.is_cuda and starts.device == dev and nbytes.device == dev):
        raise RuntimeError("histogram_flac_device needs compressed, starts and nbytes on the same GPU")
    counts = torch.empty((rows, nbins), dtype=torch.int64, device=dev)
    below = torch.empty((rows,), dtype=torch.int64, device=dev)
    above = torch.empty((rows,), dtype=torch.int64, device=dev)
    if rows == 0:
        return counts, below, above
    sel = None if idx is None else torch.from_numpy(idx).to(dev)
    d_lo, d_shift = torch.from_numpy(lo_h).to(dev), torch.from_numpy(shift_h).to(dev)
    cap = 0 if max_temp_bytes is None else int(max_temp_bytes)
    L = _lib.lib()
    with _on_device(dev):
        if is_int64:
            errcode = L.fa_histogram_i64_device(_dp(compressed), compressed.numel(), _dp(starts), _dp(nbytes), n_stream, stream_size, first, last,
                                                rows, _dp(sel), cap, nbins, _dp(d_lo), _dp(d_shift), _dp(counts), _dp(below), _dp(above),
                                                _stream_ptr(), _verify_arg(verify))
        else:
            errcode = L.fa_histogram_i32_device(_dp(compressed), compressed.numel(), _dp(starts), _dp(nbytes), n_stream, stream_size, first, last,
                                                rows, _dp(sel), nbins, _dp(d_lo), _dp(d_shift), _dp(counts), _dp(below), _dp(above),
                                                _stream_ptr(), _verify_arg(verify))
    if errcode != 0:
        # streams of different block sizes: one call per block size (see _blocksize_classes), rows scattered back
        st, nb = starts.reshape(-1), nbytes.reshape(-1)
        groups = None
        if n_stream > 1 and bool(((st >= 0) & (nb >= 12) & (st + nb <= compressed.numel())).all()):
            groups = _blocksize_classes(compressed[st[:, None] + torch.arange(12, device=dev)[None, :]].cpu().numpy())
        if groups is None:
            raise RuntimeError(f"Decoding failed, return code = {errcode}")
        for g in groups:
            if idx is None:
                at, local = g, None
            else:
                at = np.flatnonzero(np.isin(idx, g))  # rows of the result that name a stream of this class
                if at.size == 0:
                    continue
                local = np.searchsorted(g, idx[at])
            gi = torch.from_numpy(g).to(dev)
            part = histogram_flac_device(compressed, st[gi].contiguous(), nb[gi].contiguous(), stream_size, lo_h[at], shift_h[at], nbins, first,
                                         last, streams=local, is_int64=is_int64, verify=verify, max_temp_bytes=max_temp_bytes)
            ai = torch.from_numpy(at).to(dev)
            for out, p in zip((counts, below, above), part):
                out[ai] = p
    return counts, below, above


_I64_MIN, _I64_MAX = -(1 << 63), (1 << 63) - 1


def _find_args(rows, lo, hi, inside=False, max_hits=None, floats=False):
    """The argument checks of the search (ValueError, before anything touches the GPU).  `lo` / `hi`: None (no limit on
    that side), one number or `rows` of them (array or tensor).  Integer limits (floats=False) must be integers inside
    int64 -- no bools, no floats; float limits (floats=True) are numbers, +-inf meaning "no limit", NaN refused.
    `inside` is a bool, `max_hits` None or a non-negative integer.  Returns (lo[rows], hi[rows], inside, max_hits) with
    int64 or float64 numpy arrays."""
    torch = _torch()
    if not isinstance(inside, (bool, np.bool_)):
        raise ValueError("inside should be True or False")
    if max_hits is not None and (isinstance(max_hits, bool) or not isinstance(max_hits, (int, np.integer)) or int(max_hits) < 0):
        raise ValueError("max_hits should be None or a non-negative integer")

    def column(v, name, missing):
        if v is None:
            v = missing
        if isinstance(v, torch.Tensor):
            v = v.detach().cpu().numpy()
        a = np.asarray(v)
        if a.dtype == object:
            if not all(isinstance(e, (int, np.integer) if not floats else (int, float, np.integer, np.floating)) and
                       not isinstance(e, (bool, np.bool_)) for e in a.reshape(-1)):
                raise ValueError(f"{name} should hold {'numbers' if floats else 'integers'}")
        elif a.dtype.kind == "b":
            raise ValueError(f"{name} should be {'a number' if floats else 'an integer'}, not a bool")
        elif a.dtype.kind not in ("iuf" if floats else "iu"):
            raise ValueError(f"{name} should be {'a number or an array of numbers' if floats else 'an integer or an integer array'}")
        if a.ndim > 1 or (a.ndim == 1 and a.size != rows):
            raise ValueError(f"{name} should be one value or {rows} of them, one per row")
        if floats:
            a = a.astype(np.float64)
            if np.isnan(a).any():
                raise ValueError(f"{name} holds a NaN")
            return np.array(np.broadcast_to(a, (rows,)))
        if a.size and (min(int(e) for e in a.reshape(-1)) < _I64_MIN or max(int(e) for e in a.reshape(-1)) > _I64_MAX):
            raise ValueError(f"{name} holds a value outside int64")
        return np.array(np.broadcast_to(a.astype(np.int64), (rows,)))  # (a copy: writable and contiguous)

    if floats:
        return column(lo, "lo", -np.inf), column(hi, "hi", np.inf), bool(inside), None if max_hits is None else int(max_hits)
    return column(lo, "lo", _I64_MIN), column(hi, "hi", _I64_MAX), bool(inside), None if max_hits is None else int(max_hits)


def float_limit_images(restore, lo, hi, qmin, qmax):
    """The exact integer images of float limits under a monotone restore (pure host function).  `restore(q)` maps an
    int64 array q (one value per row, inside [qmin, qmax]) to the rows' restored floats and is non-decreasing in q for
    every row -- offset + coeff * float(q) with a positive coeff is.  Per row, the limits lo / hi (float64; +-inf allowed)
    become
        lo_q = the smallest q in [qmin, qmax] with restore(q) >= lo   (qmax + 1 when there is none)
        hi_q = the largest  q in [qmin, qmax] with restore(q) <= hi   (qmin - 1 when there is none)
    so that restore(q) < lo  <=>  q < lo_q and restore(q) > hi  <=>  q > hi_q for every q in the range.  The comparisons
    are made in float64, i.e. exactly.  Found by bisection: one test of the range's end and at most 64 halvings for each
    limit, every step one call of `restore` for all rows.  Returns two object arrays of Python integers (the sentinels
    lie outside int64 when the range is int64's)."""
    lo = np.asarray(lo, dtype=np.float64).reshape(-1)
    hi = np.asarray(hi, dtype=np.float64).reshape(-1)
    rows = lo.size
    qmin, qmax = int(qmin), int(qmax)

    def first_true(pred):
        # the smallest q with pred(q), pred being false ... false true ... true over the range; qmax + 1 when never true
        a = np.full(rows, qmin, dtype=object)
        b = np.full(rows, qmax + 1, dtype=object)
        if rows == 0:
            return b
        top = pred(np.full(rows, qmax, dtype=np.int64))
        b[top] = qmax
        a[~top] = qmax + 1
        for _ in range(64):
            if not (a < b).any():
                break
            mid = (a + b) // 2  # (< b <= qmax wherever a < b; rows that are done get a value in range all the same)
            m = np.clip(mid, qmin, qmax).astype(np.int64)
            t = pred(m)
            open_ = a < b
            b = np.where(open_ & t, mid, b)
            a = np.where(open_ & ~t, mid + 1, a)
        assert not (a < b).any()
        return b

    lo_q = first_true(lambda q: np.asarray(restore(q), dtype=np.float64) >= lo)
    hi_q = first_true(lambda q: np.asarray(restore(q), dtype=np.float64) > hi) - 1
    return lo_q, hi_q


def float_limits_to_int(restore, lo, hi, qmin, qmax):
    """float_limit_images as the int64 limits the search takes: a row with no q at or above lo, or none at or below hi,
    has every sample outside its limits and gets (INT64_MAX, INT64_MIN)-style limits with lo > hi placed so that every
    integer of the range is outside them; every other row gets its images, clipped into int64 (an image one past the
    range is as good as the range's end: no sample lies there)."""
    lo_q, hi_q = float_limit_images(restore, lo, hi, qmin, qmax)
    lo_i = np.empty(lo_q.size, dtype=np.int64)
    hi_i = np.empty(lo_q.size, dtype=np.int64)
    for r in range(lo_q.size):
        if lo_q[r] > qmax or hi_q[r] < qmin:  # everything is below lo, or everything is above hi
            lo_i[r], hi_i[r] = qmax, qmin  # q < qmax or q > qmin: every q of the range (qmin < qmax)
        else:
            lo_i[r], hi_i[r] = lo_q[r], hi_q[r]
    return lo_i, hi_i


def _find_passes(dev, rows, plan, count_call, fill_call, counts_only, values, max_hits):
    """The two passes of the search on device tensors.  plan() -> (errcode, block size, frames per row); count_call(nfr,
    frame_counts) and fill_call(nfr, n_hit, hit, offs, pos, val) -> errcode.  Between them: the exclusive prefix sum of the
    per-frame counts, the cells that hold a hit, and the one host read of the total."""
    torch = _torch()
    err, _, nfr = plan()
    if err != 0:
        raise RuntimeError(f"Decoding failed, return code = {err} (the search needs streams of one stated block size)")
    cells = rows * nfr
    frame_counts = torch.empty((cells,), dtype=torch.int64, device=dev)
    err = count_call(nfr, frame_counts)
    if err != 0:
        raise RuntimeError(f"Decoding failed, return code = {err}")
    counts = frame_counts.view(rows, nfr).sum(dim=1)
    if counts_only:
        return counts, None, None
    offs = torch.empty((cells + 1,), dtype=torch.int64, device=dev)
    offs[:1] = 0
    torch.cumsum(frame_counts, dim=0, out=offs[1:])
    total = int(offs[-1].item())
    if max_hits is not None and total > max_hits:
        raise ValueError(f"the search found {total} hits, more than max_hits = {max_hits}")
    pos = torch.empty((total,), dtype=torch.int64, device=dev)
    val = torch.empty((total,), dtype=torch.int64, device=dev) if values else None
    if total:
        hit = torch.nonzero(frame_counts).reshape(-1).contiguous()
        err = fill_call(nfr, int(hit.numel()), hit, offs, pos, val)
        if err != 0:
            raise RuntimeError(f"Decoding failed, return code = {err}")
    return counts, pos, val


def _find_store_checks(compressed, starts, nbytes, name):
    torch = _torch()
    if compressed.dtype != torch.uint8:
        raise ValueError("Compressed data should be of type uint8")
    if starts.dtype != torch.int64 or nbytes.dtype != torch.int64:
        raise ValueError("starts and nbytes should be of type int64")
    if starts.shape != nbytes.shape:
        raise ValueError("starts and nbytes must have the same shape")
    n_stream = int(np.prod(starts.shape))
    if n_stream <= 0:
        raise ValueError("starts needs at least one stream")
    return n_stream


def find_flac_device(compressed, starts, nbytes, stream_size, lo=None, hi=None, first_sample=0, last_sample=None, streams=None, inside=False,
                     values=True, max_hits=None, is_int64=False, verify=None, max_temp_bytes=None, _counts_only=False):
    """Where are the samples outside per-row limits -- the positions, and values, of the hits in what device-resident
    streams decode to, without a decoded copy (fa_find_count_* / fa_find_fill_*).  Sample x of row r at position t in
    [first_sample, last_sample) is a hit iff (x < lo[r] or x > hi[r]) != inside: by default the samples outside the closed
    interval, with inside=True those in it (lo == hi == v finds a sentinel value).  `lo` / `hi` are int64: a Python
    integer or `rows` of them, None meaning no limit on that side; lo > hi is legal (everything hits, or with inside=True
    nothing).  Rows are all streams, or the streams that `streams` names, in that order.

    Returns (counts [rows], positions [total], values [total] or None when values=False): int64 device tensors over the
    decoded INTEGERS (for a float store the quantised ones).  The hits are listed exactly once, sorted by (row,
    position): row r owns positions[offsets[r]:offsets[r + 1]], offsets being the exclusive prefix sum of counts.  This
    equals np.nonzero of the same predicate on the decoded integers.  No atomics place the hits, so the result does not
    depend on the order of arrival.  More than `max_hits` hits raise ValueError, which names the total, before the second
    pass runs or the position buffers exist.

    Two passes: K7F counts the hits per (row, frame) inside the decoder, torch forms the prefix sum and lists the frames
    that hold a hit, and K7F decodes those frames alone again and writes their hits in place.  Two-channel streams
    (is_int64) go through decoded column chunks of whole frames under `max_temp_bytes` (default 256 MiB) in BOTH passes,
    as reduce_flac_device's do: the documented slow route (profiles/find.md).  The streams must state one block size in
    their STREAMINFO.  `verify` is the decoder's frame CRC-16 check; argument errors raise ValueError before any GPU work,
    decode failures the decoder's RuntimeError."""
    torch = _torch()
    n_stream = _find_store_checks(compressed, starts, nbytes, "find_flac_device")
    first, last, _, _, idx = _reduce_args(n_stream, stream_size, None, first_sample, last_sample, streams)
    rows = n_stream if idx is None else int(idx.size)
    lo_h, hi_h, inside, max_hits = _find_args(rows, lo, hi, inside, max_hits)
    if not (compressed.is_contiguous() and starts.is_contiguous() and nbytes.is_contiguous()):
        raise ValueError("Only C-contiguous arrays are supported")
    dev = compressed.device
    if not (compressed.is_cuda and starts.device == dev and nbytes.device == dev):
        raise RuntimeError("find_flac_device needs compressed, starts and nbytes on the same GPU")
    if rows == 0:
        z = torch.zeros((0,), dtype=torch.int64, device=dev)
        return z, (None if _counts_only else z.clone()), (z.clone() if values and not _counts_only else None)
    sel = None if idx is None else torch.from_numpy(idx).to(dev)
    d_lo, d_hi = torch.from_numpy(lo_h).to(dev), torch.from_numpy(hi_h).to(dev)
    cap = 0 if max_temp_bytes is None else int(max_temp_bytes)
    L = _lib.lib()
    store = (_dp(compressed), compressed.numel(), _dp(starts), _dp(nbytes), n_stream, stream_size, first, last, rows, _dp(sel))
    mid = (cap,) if is_int64 else ()

    def plan():
        B, nfr = ctypes.c_int64(0), ctypes.c_int64(0)
        e = L.fa_find_plan_device(_dp(compressed), compressed.numel(), _dp(starts), stream_size, first, last, ctypes.byref(B), ctypes.byref(nfr),
                                  _stream_ptr())
        return e, B.value, nfr.value

    def count_call(nfr, fc):
        f = L.fa_find_count_i64_device if is_int64 else L.fa_find_count_i32_device
        return f(*store, *mid, _dp(d_lo), _dp(d_hi), int(inside), nfr, _dp(fc), _stream_ptr(), _verify_arg(verify))

    def fill_call(nfr, n_hit, hit, offs, pos, val):
        f = L.fa_find_fill_i64_device if is_int64 else L.fa_find_fill_i32_device
        return f(*store, *mid, _dp(d_lo), _dp(d_hi), int(inside), nfr, n_hit, _dp(hit), _dp(offs), _dp(pos), _dp(val), _stream_ptr(),
                 _verify_arg(verify))

    with _on_device(dev):
        return _find_passes(dev, rows, plan, count_call, fill_call, _counts_only, values, max_hits)


def find_counts_flac_device(compressed, starts, nbytes, stream_size, lo=None, hi=None, first_sample=0, last_sample=None, streams=None,
                            inside=False, is_int64=False, verify=None, max_temp_bytes=None):
    """The first pass of find_flac_device alone: counts [rows], an int64 device tensor -- how many samples of each row
    are hits.  Measured (profiles/find.md): 6.3-6.5 ms at 4096 x 2^20 int32 (the bare
    decode: 6.35 ms; reduce with one bin: 7.2), 53 ms at 1024 x 2^20 int64 (a chunked decode, as reduce's)."""
    return find_flac_device(compressed, starts, nbytes, stream_size, lo, hi, first_sample, last_sample, streams, inside, False, None, is_int64,
                            verify, max_temp_bytes, _counts_only=True)[0]


class DeviceDecodeIndex:
    """Decode index of one HBM-resident store (fa_decode_index_create): the stream headers are parsed and the byte
    offset of every frame is tabulated ONCE; `decode` / `decode_slices` then cost one kernel launch each.  Holds
    references to the store's tensors (the C side refers to their memory)."""

    def __init__(self, compressed, starts, nbytes, stream_size, is_int64=False):
        torch = _torch()
        if compressed.dtype != torch.uint8 or starts.dtype != torch.int64 or nbytes.dtype != torch.int64:
            raise RuntimeError("Compressed data should be of type uint8")
        self.compressed = compressed.contiguous()
        self.starts = starts.reshape(-1).contiguous()
        self.nbytes = nbytes.reshape(-1).contiguous()
        self.stream_size = int(stream_size)
        self.n_stream = int(self.starts.numel())
        self.is_int64 = bool(is_int64)
        self.device = compressed.device
        self._L = _lib.lib()
        h = ctypes.c_void_p(None)
        with _on_device(self.device):
            errcode = self._L.fa_decode_index_create(
                _dp(self.compressed), self.compressed.numel(), _dp(self.starts), _dp(self.nbytes), self.n_stream, self.stream_size,
                2 if is_int64 else 1, ctypes.byref(h), _stream_ptr(),
            )
        if errcode != 0:
            raise RuntimeError(f"Decoding failed, return code = {errcode}")
        self._h = h

    def close(self):
        if getattr(self, "_h", None) is not None and self._h.value:
            self._L.fa_decode_index_destroy(self._h)
            self._h = ctypes.c_void_p(None)

    def __del__(self):
        if sys is None or sys.is_finalizing():  # the HIP runtime may be gone already: the process ends anyway
            return
        try:
            self.close()
        except Exception:  # noqa: BLE001
            pass

    def _types(self, to_float):
        torch = _torch()
        ft, it = (torch.float64, torch.int64) if self.is_int64 else (torch.float32, torch.int32)
        return ft if to_float else it, ft

    def decode(self, first_sample=-1, last_sample=-1, offsets=None, gains=None, verify=None):
        """[first_sample, last_sample) (or everything) of ALL streams -> tensor [n_stream, n_decode]."""
        torch = _torch()
        n_decode = self.stream_size
        if first_sample >= 0 and last_sample >= 0:
            if last_sample > self.stream_size:
                raise RuntimeError("last_sample is beyond end of stream")
            if first_sample > self.stream_size - 1:
                raise RuntimeError("first_sample is beyond last element of stream")
            if first_sample >= last_sample:
                raise RuntimeError("first_sample is larger than last_sample")
            n_decode = last_sample - first_sample
        dt, ft = self._types(offsets is not None)
        out = torch.empty((self.n_stream, n_decode), dtype=dt, device=self.device)
        if offsets is not None:
            offsets = offsets.reshape(-1).to(device=self.device, dtype=ft).contiguous()
            gains = gains.reshape(-1).to(device=self.device, dtype=ft).contiguous()
        with _on_device(self.device):
            errcode = self._L.fa_decode_indexed(
                self._h, first_sample, last_sample, -1, None, None, None, None, None if offsets is not None else _dp(out),
                _dp(out) if offsets is not None else None, _dp(offsets), _dp(gains), _stream_ptr(), _verify_arg(verify),
            )
        if errcode != 0:
            raise RuntimeError(f"Decoding failed, return code = {errcode}")
        return out

    def reduce(self, width=None, first_sample=0, last_sample=None, streams=None, verify=None, max_temp_bytes=None):
        """reduce_flac_device on the indexed store (fa_reduce_indexed): nothing is parsed again.  Returns (min, max, sum,
        sumsq_hi, sumsq_lo), int64 tensors of shape (rows, nbins); the limbs are None for two-channel streams."""
        torch = _torch()
        first, last, width, nbins, idx = _reduce_args(self.n_stream, self.stream_size, width, first_sample, last_sample, streams)
        rows = self.n_stream if idx is None else int(idx.size)
        mn, mx, sm, qh, ql = _reduce_outputs(rows, nbins, self.is_int64, self.device)
        if rows == 0:
            return mn, mx, sm, qh, ql
        sel = None if idx is None else torch.from_numpy(idx).to(self.device)
        with _on_device(self.device):
            errcode = self._L.fa_reduce_indexed(self._h, first, last, width, rows, _dp(sel), 0 if max_temp_bytes is None else int(max_temp_bytes),
                                                _dp(mn), _dp(mx), _dp(sm), _dp(qh), _dp(ql), _stream_ptr(), _verify_arg(verify))
        if errcode != 0:
            raise RuntimeError(f"Decoding failed, return code = {errcode}")
        return mn, mx, sm, qh, ql

    def common_mode(self, groups=None, n_groups=None, first_sample=0, last_sample=None, streams=None, squares=None, verify=None,
                    max_temp_bytes=None):
        """common_mode_flac_device on the indexed store (fa_xsum_indexed): nothing is parsed again.  Returns (sum, sumsq_hi,
        sumsq_lo), int64 tensors of shape (G, n); the limbs are None for two-channel streams or squares=False (squares=None:
        whatever the store carries)."""
        if squares is None:
            squares = not self.is_int64
        first, last, G, order, rows, _ = _xsum_args(self.n_stream, self.stream_size, groups, n_groups, first_sample, last_sample, streams,
                                                    squares, self.is_int64)
        sm, qh, ql = _xsum_outputs(G, last - first, squares, self.device)
        if last == first:
            return sm, qh, ql
        torch = _torch()
        d_order = torch.from_numpy(order).to(self.device)
        d_rows = torch.from_numpy(rows).to(self.device)
        with _on_device(self.device):
            errcode = self._L.fa_xsum_indexed(self._h, first, last, int(order.size), _dp(d_order), int(rows.shape[0]), _dp(d_rows), G,
                                              0 if max_temp_bytes is None else int(max_temp_bytes), _dp(sm), _dp(qh), _dp(ql), _stream_ptr(),
                                              _verify_arg(verify))
        if errcode != 0:
            raise RuntimeError(f"Decoding failed, return code = {errcode}")
        return sm, qh, ql

    def dot(self, templates, first_sample=0, last_sample=None, streams=None, verify=None, max_temp_bytes=None):
        """dot_flac_device on the indexed store (fa_dot_indexed): nothing is parsed again, whatever the number of decodes.
        Returns (hi, lo), int64 tensors of shape (rows, K), or for two-channel streams one tensor (rows, K, 4)."""
        first, last, order, rows = _dot_args(self.n_stream, self.stream_size, first_sample, last_sample, streams)
        templates = _dot_i32_templates(templates, last - first)
        img, K, ld = _dot_image(templates, last - first, self.device)
        torch = _torch()
        shape = (int(order.size), K, 4) if self.is_int64 else (int(order.size), K)
        out = [torch.empty(shape, dtype=torch.int64, device=self.device) for _ in range(1 if self.is_int64 else 2)]
        if order.size:
            d_order = torch.from_numpy(order).to(self.device)
            d_rows = torch.from_numpy(rows).to(self.device)
            wide = self.is_int64
            with _on_device(self.device):
                errcode = self._L.fa_dot_indexed(self._h, first, last, int(order.size), _dp(d_order), int(rows.shape[0]), _dp(d_rows), K, ld,
                                                 _dp(img), 0 if max_temp_bytes is None else int(max_temp_bytes), None if wide else _dp(out[0]),
                                                 None if wide else _dp(out[1]), _dp(out[0]) if wide else None, _stream_ptr(), _verify_arg(verify))
            if errcode != 0:
                raise RuntimeError(f"Decoding failed, return code = {errcode}")
        return out[0] if self.is_int64 else (out[0], out[1])

    def histogram(self, lo, shift, nbins, first_sample=0, last_sample=None, streams=None, verify=None, max_temp_bytes=None):
        """histogram_flac_device on the indexed store (fa_histogram_indexed): nothing is parsed again.  Returns (counts
        [rows, nbins], below [rows], above [rows]), int64 tensors."""
        torch = _torch()
        first, last, _, _, idx = _reduce_args(self.n_stream, self.stream_size, None, first_sample, last_sample, streams)
        rows = self.n_stream if idx is None else int(idx.size)
        nbins, lo_h, shift_h = _histogram_args(rows, lo, shift, nbins)
        counts = torch.empty((rows, nbins), dtype=torch.int64, device=self.device)
        below = torch.empty((rows,), dtype=torch.int64, device=self.device)
        above = torch.empty((rows,), dtype=torch.int64, device=self.device)
        if rows == 0:
            return counts, below, above
        sel = None if idx is None else torch.from_numpy(idx).to(self.device)
        d_lo, d_shift = torch.from_numpy(lo_h).to(self.device), torch.from_numpy(shift_h).to(self.device)
        with _on_device(self.device):
            errcode = self._L.fa_histogram_indexed(self._h, first, last, rows, _dp(sel), 0 if max_temp_bytes is None else int(max_temp_bytes),
                                                   nbins, _dp(d_lo), _dp(d_shift), _dp(counts), _dp(below), _dp(above), _stream_ptr(),
                                                   _verify_arg(verify))
        if errcode != 0:
            raise RuntimeError(f"Decoding failed, return code = {errcode}")
        return counts, below, above

    def find(self, lo=None, hi=None, first_sample=0, last_sample=None, streams=None, inside=False, values=True, max_hits=None, verify=None,
             max_temp_bytes=None, _counts_only=False):
        """find_flac_device on the indexed store (fa_find_count_indexed / fa_find_fill_indexed): nothing is parsed again.
        Returns (counts [rows], positions [total], values [total] or None), int64 tensors."""
        torch = _torch()
        first, last, _, _, idx = _reduce_args(self.n_stream, self.stream_size, None, first_sample, last_sample, streams)
        rows = self.n_stream if idx is None else int(idx.size)
        lo_h, hi_h, inside, max_hits = _find_args(rows, lo, hi, inside, max_hits)
        dev = self.device
        if rows == 0:
            z = torch.zeros((0,), dtype=torch.int64, device=dev)
            return z, (None if _counts_only else z.clone()), (z.clone() if values and not _counts_only else None)
        sel = None if idx is None else torch.from_numpy(idx).to(dev)
        d_lo, d_hi = torch.from_numpy(lo_h).to(dev), torch.from_numpy(hi_h).to(dev)
        cap = 0 if max_temp_bytes is None else int(max_temp_bytes)
        L = self._L

        def plan():
            B, nfr = ctypes.c_int64(0), ctypes.c_int64(0)
            e = L.fa_find_plan_indexed(self._h, first, last, ctypes.byref(B), ctypes.byref(nfr))
            return e, B.value, nfr.value

        def count_call(nfr, fc):
            return L.fa_find_count_indexed(self._h, first, last, rows, _dp(sel), cap, _dp(d_lo), _dp(d_hi), int(inside), nfr, _dp(fc), _stream_ptr(),
                                           _verify_arg(verify))

        def fill_call(nfr, n_hit, hit, offs, pos, val):
            return L.fa_find_fill_indexed(self._h, first, last, rows, _dp(sel), cap, _dp(d_lo), _dp(d_hi), int(inside), nfr, n_hit, _dp(hit), _dp(offs),
                                          _dp(pos), _dp(val), _stream_ptr(), _verify_arg(verify))

        with _on_device(dev):
            return _find_passes(dev, rows, plan, count_call, fill_call, _counts_only, values, max_hits)

    def find_counts(self, lo=None, hi=None, first_sample=0, last_sample=None, streams=None, inside=False, verify=None, max_temp_bytes=None):
        """The first pass of `find` alone: counts [rows], an int64 tensor."""
        return self.find(lo, hi, first_sample, last_sample, streams, inside, False, None, verify, max_temp_bytes, _counts_only=True)[0]

    def decode_slices(self, slice_stream, slice_first, slice_count, offsets=None, gains=None, verify=None, to_host=False):
        """Batched random access (see decode_slices_device): returns (flat tensor, int64 numpy array of offsets);
        `to_host`: the flat result as a numpy array instead, copied inside the decode call (one synchronisation)."""
        torch = _torch()
        slice_stream = np.ascontiguousarray(slice_stream, dtype=np.int64)
        slice_first = np.ascontiguousarray(slice_first, dtype=np.int64)
        slice_count = np.ascontiguousarray(slice_count, dtype=np.int64)
        n = slice_stream.shape[0]
        out_off = np.zeros(n, dtype=np.int64)
        if n > 1:
            np.cumsum(slice_count[:-1], out=out_off[1:])
        dt, ft = self._types(offsets is not None)
        out = torch.empty(int(slice_count.sum()), dtype=dt, device=self.device)
        if n == 0:
            return out, out_off
        if offsets is not None:
            offsets = offsets.reshape(-1).to(device=self.device, dtype=ft).contiguous()
            gains = gains.reshape(-1).to(device=self.device, dtype=ft).contiguous()
        if to_host:
            ndt = np.dtype(str(dt).replace("torch.", ""))
            # (64 KB and more: a pinned block the decoder writes straight into; below that the library's own landing
            # buffer and a memcpy are cheaper than the pool's bookkeeping: 122 against 129 us per single read)
            host = _pinned_pool.empty(out.numel(), ndt) if out.numel() * ndt.itemsize >= 65536 else None
            if host is None:
                host = np.empty(out.numel(), dtype=ndt)
            with _on_device(self.device):
                errcode = self._L.fa_decode_indexed_host(
                    self._h, n, ctypes.c_void_p(slice_stream.ctypes.data), ctypes.c_void_p(slice_first.ctypes.data),
                    ctypes.c_void_p(slice_count.ctypes.data), ctypes.c_void_p(out_off.ctypes.data),
                    None if offsets is not None else _dp(out), _dp(out) if offsets is not None else None, _dp(offsets), _dp(gains),
                    ctypes.c_void_p(host.ctypes.data), host.nbytes, _stream_ptr(), _verify_arg(verify),
                )
            if errcode != 0:
                raise RuntimeError(f"Decoding failed, return code = {errcode}")
            return host, out_off
        with _on_device(self.device):
            errcode = self._L.fa_decode_indexed(
                self._h, -1, -1, n, ctypes.c_void_p(slice_stream.ctypes.data), ctypes.c_void_p(slice_first.ctypes.data),
                ctypes.c_void_p(slice_count.ctypes.data), ctypes.c_void_p(out_off.ctypes.data),
                None if offsets is not None else _dp(out), _dp(out) if offsets is not None else None, _dp(offsets), _dp(gains),
                _stream_ptr(), _verify_arg(verify),
            )
        if errcode != 0:
            raise RuntimeError(f"Decoding failed, return code = {errcode}")
        return out, out_off


def float32_to_int32_device(data, quanta=None):
    """Device float32 -> int32 quantisation (utils.c:160-243); returns (int32 tensor, offsets, gains)."""
    torch = _torch()
    if data.dtype != torch.float32 or not data.is_contiguous():
        raise ValueError("Only float32 and float64 data are supported")
    stream_size = data.shape[-1]
    lead = tuple(data.shape[:-1]) if data.dim() > 1 else (1,)
    n_stream = int(np.prod(lead))
    out = torch.empty(data.shape, dtype=torch.int32, device=data.device)
    offsets = torch.empty(n_stream, dtype=torch.float32, device=data.device)
    gains = torch.empty(n_stream, dtype=torch.float32, device=data.device)
    q = None
    if quanta is not None:
        q = quanta.to(device=data.device, dtype=torch.float32).reshape(-1).contiguous()
        if q.numel() != n_stream:
            raise RuntimeError("quanta must have one entry per stream")
    with _on_device(data.device):
        errcode = _lib.lib().fa_float32_to_int32_device(
            _dp(data), n_stream, stream_size, _dp(q), _dp(out), _dp(offsets), _dp(gains), _stream_ptr()
        )
    if errcode & _lib.ERROR_NAN_INPUT:
        raise RuntimeError("Cannot convert data with NaNs to integers")
    if errcode != 0:
        raise RuntimeError(f"Encoding failed, return code = {errcode}")
    return out, offsets.reshape(lead), gains.reshape(lead)


def float64_to_int64_device(data, quanta=None):
    """Device float64 -> int64 quantisation (utils.c:245-327); returns (int64 tensor, offsets, gains)."""
    torch = _torch()
    if data.dtype != torch.float64 or not data.is_contiguous():
        raise ValueError("Only float32 and float64 data are supported")
    stream_size = data.shape[-1]
    lead = tuple(data.shape[:-1]) if data.dim() > 1 else (1,)
    n_stream = int(np.prod(lead))
    out = torch.empty(data.shape, dtype=torch.int64, device=data.device)
    offsets = torch.empty(n_stream, dtype=torch.float64, device=data.device)
    gains = torch.empty(n_stream, dtype=torch.float64, device=data.device)
    q = None
    if quanta is not None:
        q = quanta.to(device=data.device, dtype=torch.float64).reshape(-1).contiguous()
        if q.numel() != n_stream:
            raise RuntimeError("quanta must have one entry per stream")
    with _on_device(data.device):
        errcode = _lib.lib().fa_float64_to_int64_device(
            _dp(data), n_stream, stream_size, _dp(q), _dp(out), _dp(offsets), _dp(gains), _stream_ptr()
        )
    if errcode & _lib.ERROR_NAN_INPUT:
        raise RuntimeError("Cannot convert data with NaNs to integers")
    if errcode != 0:
        raise RuntimeError(f"Encoding failed, return code = {errcode}")
    return out, offsets.reshape(lead), gains.reshape(lead)


def _splice_checks(compressed, starts, nbytes, level, data, offsets, gains, streams=None):
    """The argument checks append and overwrite share (ValueError).  Returns (n_stream, n, stream indices as an int64
    numpy array or None)."""
    torch = _torch()
    if compressed.dtype != torch.uint8:
        raise ValueError("Compressed data should be of type uint8")
    if starts.dtype != torch.int64 or nbytes.dtype != torch.int64 or starts.shape != nbytes.shape:
        raise ValueError("starts and nbytes should be int64 tensors of one shape")
    if level < 0 or level > 8:
        raise ValueError("FLAC only supports compression levels 0-8")
    n_stream = int(np.prod(starts.shape))
    if data.dim() == 0:
        raise ValueError("data needs a stream axis")
    n = int(data.shape[-1])
    idx = _stream_indices(streams, n_stream)
    if idx is None:
        if tuple(data.shape) not in ((n_stream, n), tuple(starts.shape) + (n,)) and not (data.dim() == 1 and n_stream == 1):
            raise ValueError(f"data of shape {tuple(data.shape)} does not match {n_stream} streams (starts of shape {tuple(starts.shape)})")
    elif tuple(data.shape) != (idx.size, n):
        raise ValueError(f"data of shape {tuple(data.shape)} does not match {idx.size} streams to overwrite")
    is_float = data.dtype in (torch.float32, torch.float64)
    if data.dtype not in (torch.int32, torch.int64) and not is_float:
        raise ValueError(f"Unsupported data type '{data.dtype}': int32, int64, float32 or float64")
    if is_float != (offsets is not None) or (offsets is None) != (gains is None):
        raise ValueError("float data need the store's offsets and gains, integer data take neither")
    return n_stream, n, idx


def _splice_flac_device(op, compressed, starts, nbytes, stream_size, data, idx, first, level, offsets, gains, verify, compact):
    """What append and overwrite do on the device: quantise float `data` with the store's offsets and gains, run
    fa_<op>_i32_device / fa_<op>_i64_device into fresh buffers, and (verify) decode the re-encoded span from the result and
    compare it with the old span patched by `data`.  `idx`: the streams that take part (None: all); `first`: the sample
    the data starts at (append: stream_size).  Returns (compressed, starts, nbytes) of the new store."""
    torch = _torch()
    word = {"append": "Appending", "overwrite": "Overwriting"}[op]
    dev = compressed.device
    n_stream = int(np.prod(starts.shape))
    n = int(data.shape[-1])
    m = n_stream if idx is None else int(idx.size)
    wide = data.dtype in (torch.int64, torch.float64)
    L = _lib.lib()
    data = data.reshape(m, n).contiguous()
    with _on_device(dev):
        d_idx = None if idx is None else torch.from_numpy(idx).to(dev)
        if data.dtype in (torch.float32, torch.float64):
            off = offsets.to(device=dev, dtype=data.dtype).reshape(-1).contiguous()
            gain = gains.to(device=dev, dtype=data.dtype).reshape(-1).contiguous()
            if off.numel() != n_stream or gain.numel() != n_stream:
                raise ValueError("offsets and gains need one value per stream")
            if d_idx is not None:
                off, gain = off[d_idx].contiguous(), gain[d_idx].contiguous()
            ints = torch.empty((m, n), dtype=torch.int64 if wide else torch.int32, device=dev)
            errcode = (L.fa_quantise_f64_device if wide else L.fa_quantise_f32_device)(
                _dp(data), m, n, _dp(off), _dp(gain), _dp(ints), n, _stream_ptr())
            if errcode & _lib.ERROR_NAN_INPUT:
                raise RuntimeError("Cannot convert data with NaNs to integers")
            if errcode != 0:
                raise RuntimeError(f"Quantisation failed, return code = {errcode}")
            data = ints
        comp = compressed.contiguous()
        st, nb = starts.reshape(-1).contiguous(), nbytes.reshape(-1).contiguous()
        # (the C signatures differ in the geometry only: append takes n, overwrite the stream index, m, first and n)
        geom = (n,) if op == "append" else (m, first, n)
        where = (_dp(data), n) if op == "append" else (_dp(d_idx), m, _dp(data), first, n)
        sfx = "_i64" if wide else ""
        ws_bytes = getattr(L, f"fa_{op}_workspace_bytes{sfx}")(n_stream, stream_size, *geom, level)
        cap = getattr(L, f"fa_{op}_capacity_bytes{sfx}")(comp.numel(), n_stream, stream_size, *geom, level)
        if ws_bytes < 0 or cap < 0:
            raise RuntimeError(f"{word} failed: invalid geometry")
        ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
        buf = torch.empty(cap, dtype=torch.uint8, device=dev)
        index = torch.empty(2 * n_stream, dtype=torch.int64, device=dev)
        total = ctypes.c_int64(0)
        errcode = getattr(L, f"fa_{op}_{'i64' if wide else 'i32'}_device")(
            _dp(comp), comp.numel(), _dp(st), _dp(nb), n_stream, stream_size, *where, level, _dp(ws), ws_bytes, _dp(buf), cap,
            _dp(index[:n_stream]), _dp(index[n_stream:]), ctypes.byref(total), _stream_ptr())
    if errcode == 8192:  # FA_ERROR_DECODE_INIT
        raise ValueError(f"{word} needs streams written by this library (a SEEKTABLE with one point per frame) with the block size of "
                         f"level {level}, {2 if wide else 1} channel(s) ({data.dtype} data) and {stream_size} samples")
    if errcode != 0:
        raise RuntimeError(f"{word} failed, return code = {errcode}")
    blob = buf[: total.value]
    if compact:
        blob = blob.clone()
        del buf
    out = (blob, index[:n_stream].reshape(starts.shape), index[n_stream:].reshape(starts.shape))
    if verify:
        # the re-encoded span: [lo, hi_old) of the old streams, [lo, hi_new) of the new ones
        B = 1152 if level <= 2 else 4096
        size_new = max(stream_size, first + n)
        lo = first // B * B
        hi_old, hi_new = (min(-(-(first + n) // B) * B, size) for size in (stream_size, size_new))
        rows = slice(None) if d_idx is None else d_idx
        span = decode_flac_device(out[0], index[:n_stream][rows], index[n_stream:][rows], size_new, lo, hi_new, is_int64=wide,
                                  verify=True).reshape(m, -1)
        if lo == first and hi_new == first + n:
            want = data
        else:
            old = decode_flac_device(comp, st[rows], nb[rows], stream_size, lo, hi_old, is_int64=wide).reshape(m, -1)
            want = torch.cat([old, old.new_empty((m, hi_new - hi_old))], dim=1)
            want[:, first - lo : first - lo + n] = data
        bad = (span != want).any(dim=1)
        if bool(bad.any()):
            at = torch.where(bad, (span != want).int().argmax(dim=1) + lo, torch.full_like(bad, -1, dtype=torch.int64))
            _raise_on_mismatch(at)
    return out


def append_flac_device(compressed, starts, nbytes, stream_size, data, level=5, offsets=None, gains=None, verify=False, compact=False,
                       md5=False):
    """Extend every stream of a device-resident store by data.shape[-1] samples: returns the new (compressed, starts,
    nbytes), all on the device, the store's arguments left as they are.

    The store must have this library's layout (one SEEKTABLE point per frame) and `level` the level it was written at
    (its block size is checked against the streams' STREAMINFO).  `data`: a C-contiguous tensor on the store's device,
    (n_stream, n) or starts.shape + (n,) -- int32 for one-channel streams, int64 for two-channel streams; or float32 /
    float64 with the store's `offsets` and `gains`, which then quantise it exactly as the encoder quantises (a NaN raises
    RuntimeError).  The result is byte for byte the encode of the concatenated integers (fa_append_i32_device /
    fa_append_i64_device, include/flacarray_hip.h): the old short last frame is decoded, the new frames are encoded
    and spliced in behind the kept old ones.  `compressed` is a view of a buffer sized for the worst case (the old blob
    plus a verbatim encode of the new frames), which it keeps alive; `compact=True` returns an exact-size copy instead, as
    encode_flac_device does.  A store whose STREAMINFO names another block size, channel count (one for int32 / float32
    data, two for int64 / float64) or stream size than the call's raises ValueError before anything is decoded.
    `verify=True`: decode the re-encoded span, samples [stream_size - r, stream_size + n) (r = the old short tail), and
    compare it with the old tail and the new integers; a difference raises RuntimeError.

    The splice writes a fresh stream header, so the result is UNSIGNED (MD5 field zero) whatever the old store was: a
    finished digest cannot be resumed.  `md5=True` signs it, at the cost of one decode of the whole new store
    (check_md5_device's chunked pass); explicit only -- it does not follow set_encode_md5."""
    n_stream, n, _ = _splice_checks(compressed, starts, nbytes, level, data, offsets, gains)
    dev = compressed.device
    if not (compressed.is_cuda and data.device == dev and starts.device == dev and nbytes.device == dev):
        raise RuntimeError("append_flac_device needs compressed, starts, nbytes and data on the same GPU")
    if n == 0:
        return compressed, starts, nbytes
    out = _splice_flac_device("append", compressed, starts, nbytes, stream_size, data, None, stream_size, level, offsets, gains, verify, compact)
    if md5:
        wide = data.dtype in (_torch().int64, _torch().float64)
        _, digests = check_md5_device(out[0], out[1], out[2], stream_size + n, is_int64=wide, return_digests=True)
        sign_streams_device(out[0], out[1], digests)
    return out


def overwrite_flac_device(compressed, starts, nbytes, stream_size, first, data, streams=None, level=5, offsets=None, gains=None, verify=False,
                          compact=False):
    """Replace samples [first, first + n) of some or all streams of a device-resident store, n = data.shape[-1]: returns
    the new (compressed, starts, nbytes), all on the device, the store's arguments left as they are.

    The store must have this library's layout (one SEEKTABLE point per frame) and `level` the level it was written at
    (its block size is checked against the streams' STREAMINFO).  `streams=None`: every stream takes part, `data` is a
    C-contiguous tensor on the store's device of shape (n_stream, n) or starts.shape + (n,) ((n,) for one stream).
    Otherwise `streams` is a 1-D integer array or tensor of flat (C-order) stream indices and `data` is (len(streams), n),
    row j for stream streams[j]; an index out of range or named twice raises ValueError, no stream does nothing.  int32
    data for one-channel streams, int64 for two-channel streams; or float32 / float64 with the store's `offsets` and `gains`
    (one per stream of the STORE), which then quantise it exactly as the encoder quantises (quantise_rows_kernel: a NaN
    raises RuntimeError, out-of-range values become INT_MIN).  0 <= first and first + n <= stream_size, else ValueError;
    n == 0 does nothing.

    The result is byte for byte the encode of the patched integers (fa_overwrite_i32_device / fa_overwrite_i64_device,
    include/flacarray_hip.h), except the STREAMINFO MD5: a stream that takes part gets a zero one (its samples changed), a
    stream that does not is copied whole and keeps its own.  Only the frames that overlap the range are decoded and encoded
    again; all other bytes of the store are copied once.  `compressed` is a view of a buffer sized for the worst case;
    `compact=True` returns an exact-size copy instead.  A participating stream whose STREAMINFO names another block size,
    channel count or stream size than the call's raises ValueError before anything is decoded.  `verify=True`: decode the
    re-encoded span of the participating streams from the result and compare it with the patched old span; a difference
    raises RuntimeError."""
    n_stream, n, idx = _splice_checks(compressed, starts, nbytes, level, data, offsets, gains, streams)
    first = int(first)
    if first < 0 or first + n > stream_size:
        raise ValueError(f"samples [{first}, {first + n}) do not lie inside streams of {stream_size} samples")
    dev = compressed.device
    if not (compressed.is_cuda and data.device == dev and starts.device == dev and nbytes.device == dev):
        raise RuntimeError("overwrite_flac_device needs compressed, starts, nbytes and data on the same GPU")
    if n == 0 or (idx is not None and idx.size == 0):
        return compressed, starts, nbytes
    return _splice_flac_device("overwrite", compressed, starts, nbytes, stream_size, data, idx, first, level, offsets, gains, verify, compact)


def reindex_flac_device(compressed, starts, nbytes, stream_size, is_int64=False, verify=True, compact=False):
    """Adopt a device-resident store written by another FLAC encoder (stock flacarray / libFLAC): returns the new
    (compressed, starts, nbytes), all on the device, the store's arguments left as they are.

    Every stream is copied into this library's own layout -- "fLaC", the source's STREAMINFO verbatim (a signed stream
    stays signed), a SEEKTABLE of one point per frame, the frames verbatim (fa_reindex_device, include/flacarray_hip.h).
    No sample is decoded and nothing is re-encoded; after it append_flac_device, overwrite_flac_device,
    frame_status_device and decode_flac_salvage_device take the store, and a decode no longer scans for the frames.
    Every other metadata block of the source (VORBIS_COMMENT, APPLICATION, PADDING, a sparse or placeholder SEEKTABLE) is
    dropped: the layout has no room for it.  A store that already has the layout comes out byte-identical.  is_int64:
    two-channel streams (int64 / float64 arrays).  The streams of one call share their block size, as the streams stock
    flacarray writes at one level do: a store that mixes block sizes raises ValueError (reindex its parts).  Anything the
    decoders would refuse when they index the store (a header that does not parse, a variable block size, the other
    channel count, a wrong stream_size, a SEEKTABLE whose offsets leave the stream) raises RuntimeError.

    `compressed` is a view of a buffer sized for the worst case (the old bytes plus the new headers), which it keeps
    alive; `compact=True` returns an exact-size copy instead, as the splice functions do.  `verify=True` (the default)
    runs frame_status_device over the RESULT and raises RuntimeError unless every status is 0: every located frame then
    carries its number, its block size and a clean CRC-16, so a false sync code or a damaged source frame cannot slip
    into an index silently -- cheap next to a one-time migration.  `verify=False` skips it: the way to adopt a damaged
    store in order to salvage it -- with one exception: the header of every stream's LAST frame must still carry its frame
    number and block size, because that is what ties `stream_size` to the store (RuntimeError otherwise, as for a wrong
    stream_size)."""
    torch = _torch()
    _store_checks(compressed, starts, nbytes, stream_size)
    if starts.shape != nbytes.shape:
        raise RuntimeError("starts and nbytes should have one shape")
    dev = compressed.device
    if not (compressed.is_cuda and starts.device == dev and nbytes.device == dev):
        raise RuntimeError("reindex_flac_device needs compressed, starts and nbytes on the same GPU")
    n_stream = int(np.prod(starts.shape))
    if n_stream == 0:
        return compressed.new_empty(0), starts.clone(), nbytes.clone()
    L = _lib.lib()
    with _on_device(dev):
        st, nb = starts.reshape(-1), nbytes.reshape(-1)
        B = None
        if bool(((st >= 0) & (nb >= 12) & (st <= compressed.numel() - 12)).all()):
            head = compressed[st[:, None] + torch.arange(12, device=dev)[None, :]].cpu().numpy()
            if _blocksize_classes(head) is not None:
                raise ValueError("the store's streams differ in block size: reindex takes one block size per call "
                                 "(reindex the streams of each block size on their own)")
            B = common_block_size(head)
        cap = L.fa_reindex_capacity_bytes(compressed.numel(), n_stream, stream_size, B) if B else -1
        if cap < 0:
            raise RuntimeError("Reindexing failed: no stream header gives a block size the stream size fits")
        buf = torch.empty(cap, dtype=torch.uint8, device=dev)
        index = torch.empty(2 * n_stream, dtype=torch.int64, device=dev)
        total = ctypes.c_int64(0)
        errcode = L.fa_reindex_device(_dp(compressed), compressed.numel(), _dp(st), _dp(nb), n_stream, stream_size, 2 if is_int64 else 1,
                                      _dp(buf), cap, _dp(index[:n_stream]), _dp(index[n_stream:]), ctypes.byref(total), _stream_ptr())
    if errcode != 0:
        raise RuntimeError(f"Reindexing failed, return code = {errcode}")
    blob = buf[: total.value]
    if compact:
        blob = blob.clone()
        del buf
    out = (blob, index[:n_stream].reshape(starts.shape), index[n_stream:].reshape(starts.shape))
    if verify:
        status = frame_status_device(out[0], out[1], out[2], stream_size, is_int64=is_int64, block_size=B)
        bad = torch.nonzero(status.reshape(n_stream, -1))
        if bad.numel():
            s_bad, f_bad = (int(v) for v in bad[0])
            raise RuntimeError(f"Reindexing failed: {bad.shape[0]} frame(s) of the result do not check (first: stream {s_bad}, frame {f_bad}, "
                               f"status {int(status.reshape(n_stream, -1)[s_bad, f_bad])}); verify=False adopts the store as it is, for salvage")
    return out


def _window_args(n_stream, stream_size, first, last, streams, level):
    """The argument checks of a window (ValueError, before anything touches the GPU).  Returns (first, last, block size,
    stream indices as an int64 numpy array or None)."""
    stream_size = int(stream_size)
    if stream_size <= 0:
        raise ValueError("You must specify the non-zero stream size")
    if level < 0 or level > 8:
        raise ValueError("FLAC only supports compression levels 0-8")
    first = int(first)
    last = stream_size if last is None else int(last)
    if first < 0 or last > stream_size or last <= first:
        raise ValueError(f"samples [{first}, {last}) are not a non-empty range inside streams of {stream_size} samples "
                         "(there is no zero-sample stream to write)")
    return first, last, (1152 if level <= 2 else 4096), _stream_indices(streams, n_stream)


def window_flac_device(compressed, starts, nbytes, stream_size, first=0, last=None, streams=None, level=5, is_int64=False, verify=False,
                       compact=False, max_temp_bytes=None):
    """Cut samples [first, last) of every stream of a device-resident store, or of the streams that `streams` names
    (1-D flat C-order indices, no repeats; the new streams come in that order), out as a NEW store: returns its
    (compressed, starts, nbytes), all on the device, the arguments left as they are.  starts / nbytes have the shape of
    `starts` for streams=None and (len(streams),) otherwise; an empty `streams` gives an empty store.

    The store must have this library's layout (one SEEKTABLE point per frame; reindex_flac_device adopts others) and
    `level` the level it was written at (its block size B is checked against the streams' STREAMINFO).  For streams of
    integers the result is then byte for byte encode_flac_device(x[idx, first:last], level) with x the decoded array
    (for a float store: of the quantised integers), after any sequence of appends, overwrites and windows.

    first % B == 0 (fa_window_device, include/flacarray_hip.h): no sample of a frame that is kept whole is decoded.  The
    frames first / B, ... are copied with their numbers lowered (number field, CRC-8, CRC-16 by its linear identity), the
    seek table is rebuilt from the old one, and only where `last` falls inside an old frame is that one frame decoded up to
    the cut and encoded again as the short last frame.  first == 0 renumbers nothing.  A window that is the whole stream
    copies each picked stream verbatim -- pure stream selection, a signed stream keeps its signature; every other window
    comes out with a zero STREAMINFO MD5.

    first % B != 0: every frame boundary moves, so every frame changes, and this route COSTS A DECODE PLUS AN ENCODE of
    the window: the picked streams are decoded on [first, last) in row chunks of at most `max_temp_bytes` (default
    256 MiB, at least one row) and each chunk is encoded with encode_flac_device; streams are independent, so the
    pieces put back to back are byte for byte the one-shot encode, and the extra memory is one chunk beside the result
    (at 4096 x 2^20 and the default chunk size about twice the time of one decode plus one encode, for a seventh of their
    memory: profiles/window.md).

    `compressed` is a view of a buffer sized for the picked streams plus the worst case of the re-encoded frame;
    `compact=True` returns an exact-size copy instead.  `verify=True`: frame_status_device over the RESULT must be all
    zero (every frame carries its new number, a clean CRC-8 and CRC-16), and the re-encoded last frame is decoded from the
    result and compared with the old samples it was made from (the unaligned route compares every chunk's encode with
    its input); RuntimeError otherwise.

    ValueError: an empty or outside range, a bad stream index, a level outside 0-8, or streams that are not this
    library's for the call's block size, channel count (is_int64: two) and stream size.  RuntimeError: a seek table
    whose offsets are not ordered inside the stream body or a frame shorter than its header plus CRC-16 (refused by the
    check kernel's error word before anything is read through such an offset)."""
    torch = _torch()
    if compressed.dtype != torch.uint8:
        raise ValueError("Compressed data should be of type uint8")
    if starts.dtype != torch.int64 or nbytes.dtype != torch.int64 or starts.shape != nbytes.shape:
        raise ValueError("starts and nbytes should be int64 tensors of one shape")
    n_stream = int(np.prod(starts.shape))
    first, last, B, idx = _window_args(n_stream, stream_size, first, last, streams, level)
    stream_size = int(stream_size)
    dev = compressed.device
    if not (compressed.is_cuda and starts.device == dev and nbytes.device == dev):
        raise RuntimeError("window_flac_device needs compressed, starts and nbytes on the same GPU")
    m = n_stream if idx is None else int(idx.size)
    out_shape = tuple(starts.shape) if idx is None else (m,)
    if m == 0:
        return compressed.new_empty(0), starts.new_empty(out_shape), nbytes.new_empty(out_shape)
    n = last - first
    nch = 2 if is_int64 else 1
    L = _lib.lib()
    with _on_device(dev):
        comp = compressed.contiguous()
        if comp.data_ptr() & 15:  # (the copy reads its source in aligned 16-byte blocks)
            comp = comp.clone()
        st, nb = starts.reshape(-1).contiguous(), nbytes.reshape(-1).contiguous()
        d_idx = None if idx is None else torch.from_numpy(idx).to(dev)
        rows = slice(None) if d_idx is None else d_idx
        if first % B:
            # unaligned: decode and encode, a chunk of rows at a time
            cap = (256 << 20) if max_temp_bytes is None else int(max_temp_bytes)
            per = max(1, cap // (n * 4 * nch))
            sub_st, sub_nb = st[rows].contiguous(), nb[rows].contiguous()
            blobs, sizes = [], []
            for r0 in range(0, m, per):
                x = decode_flac_device(comp, sub_st[r0 : r0 + per], sub_nb[r0 : r0 + per], stream_size, first, last, is_int64=is_int64)
                # (compact: a piece must not keep its worst-case buffer alive while the others are made)
                b, _, nbs = encode_flac_device(x, level=level, compact=True, verify=bool(verify), md5=False)
                blobs.append(b)
                sizes.append(nbs.reshape(-1))
                del x
            nbytes2 = torch.cat(sizes)
            starts2 = torch.cumsum(nbytes2, 0) - nbytes2
            blob = torch.cat(blobs) if len(blobs) > 1 else blobs[0]  # (exact-size either way)
        else:
            picked = int(nb[rows].sum().item())
            ws_bytes = L.fa_window_workspace_bytes(n_stream, stream_size, m, first, last, nch, level)
            cap = L.fa_window_capacity_bytes(max(picked, 0), n_stream, stream_size, m, first, last, nch, level)
            if ws_bytes < 0 or cap < 0:
                raise RuntimeError("Windowing failed: invalid geometry")
            ws = torch.empty(max(ws_bytes, 16), dtype=torch.uint8, device=dev)
            buf = torch.empty(cap, dtype=torch.uint8, device=dev)
            index = torch.empty(2 * m, dtype=torch.int64, device=dev)
            total = ctypes.c_int64(0)
            errcode = L.fa_window_device(_dp(comp), comp.numel(), _dp(st), _dp(nb), n_stream, stream_size, _dp(d_idx), m, first, last, nch, level,
                                         _dp(ws), ws.numel(), _dp(buf), cap, _dp(index[:m]), _dp(index[m:]), ctypes.byref(total), _stream_ptr())
            if errcode == 8192:  # FA_ERROR_DECODE_INIT
                raise ValueError(f"Windowing needs streams written by this library (a SEEKTABLE with one point per frame; reindex() adopts "
                                 f"other stores) with the block size of level {level}, {nch} channel(s) and {stream_size} samples")
            if errcode == 1 << 18:  # FA_ERROR_DECODE_SEEK
                raise RuntimeError("Windowing failed: a seek table's offsets are not ordered inside the stream body, or a frame is shorter "
                                   "than its header plus the CRC-16")
            if errcode != 0:
                raise RuntimeError(f"Windowing failed, return code = {errcode}")
            blob = buf[: total.value]
            if compact:
                blob = blob.clone()
                del buf
            starts2, nbytes2 = index[:m], index[m:]
        out = (blob, starts2.reshape(out_shape), nbytes2.reshape(out_shape))
        if verify:
            status = frame_status_device(out[0], starts2, nbytes2, n, is_int64=is_int64, block_size=B)
            bad = torch.nonzero(status.reshape(m, -1))
            if bad.numel():
                s_bad, f_bad = (int(v) for v in bad[0])
                raise RuntimeError(f"Windowing failed: {bad.shape[0]} frame(s) of the result do not check (first: stream {s_bad}, frame {f_bad}, "
                                   f"status {int(status.reshape(m, -1)[s_bad, f_bad])})")
            r = n % B
            if first % B == 0 and r and last != stream_size:  # the re-encoded last frame against the old samples
                got = decode_flac_device(out[0], starts2, nbytes2, n, n - r, n, is_int64=is_int64, verify=True).reshape(m, -1)
                want = decode_flac_device(comp, st[rows].contiguous(), nb[rows].contiguous(), stream_size, last - r, last,
                                          is_int64=is_int64).reshape(m, -1)
                diff = got != want
                if bool(diff.any()):
                    hit = diff.any(dim=1)
                    _raise_on_mismatch(torch.where(hit, diff.int().argmax(dim=1) + (n - r), torch.full_like(hit, -1, dtype=torch.int64)))
    return out


def _join_args(n_streams, stream_sizes, level):
    """The argument checks of a join (ValueError, before anything touches the GPU): `n_streams` and `stream_sizes` hold
    one value per part.  Returns (block size, the stream sizes as ints, j): j is None when every part but the last is a
    whole number of blocks long (the aligned route takes all parts), else the index of the first part, other than the
    last, behind which the running total is not a multiple of the block size."""
    n_streams = [int(v) for v in n_streams]
    sizes = [int(v) for v in stream_sizes]
    if not sizes or len(n_streams) != len(sizes):
        raise ValueError("a join needs at least one store (and one stream size per store)")
    if level < 0 or level > 8:
        raise ValueError("FLAC only supports compression levels 0-8")
    if any(v <= 0 for v in sizes):
        raise ValueError("You must specify the non-zero stream size of every part (there is no zero-sample stream to join)")
    if any(v != n_streams[0] for v in n_streams):
        raise ValueError(f"the parts of a join need one number of streams each, got {n_streams}")
    if sum(sizes) >= 1 << 36:
        raise ValueError("a FLAC stream holds fewer than 2^36 samples")
    B = 1152 if level <= 2 else 4096
    j, total = None, 0
    for p, v in enumerate(sizes[:-1]):
        total += v
        if total % B:
            j = p
            break
    return B, sizes, j


def _join_aligned(L, stores, sizes, n_stream, nch, level, dev):
    """One call of fa_join_device: (worst-case buffer, starts, nbytes, bytes used)."""
    torch = _torch()
    P = len(stores)
    arr = ctypes.c_int64 * P
    ptrs = ctypes.c_void_p * P
    c_sizes = arr(*sizes)
    c_bytes = arr(*[int(s[0].numel()) for s in stores])
    ws_bytes = L.fa_join_workspace_bytes(P, n_stream, c_sizes, nch, level)
    cap = L.fa_join_capacity_bytes(P, c_bytes, n_stream, c_sizes, nch, level)
    if ws_bytes < 0 or cap < 0:
        raise RuntimeError("Joining failed: invalid geometry")
    ws = torch.empty(max(ws_bytes, 16), dtype=torch.uint8, device=dev)
    buf = torch.empty(max(cap, 16), dtype=torch.uint8, device=dev)
    index = torch.empty(2 * n_stream, dtype=torch.int64, device=dev)
    total = ctypes.c_int64(0)
    errcode = L.fa_join_device(P, ptrs(*[s[0].data_ptr() for s in stores]), c_bytes, ptrs(*[s[1].data_ptr() for s in stores]),
                               ptrs(*[s[2].data_ptr() for s in stores]), c_sizes, n_stream, nch, level, _dp(ws), ws.numel(), _dp(buf), cap,
                               _dp(index[:n_stream]), _dp(index[n_stream:]), ctypes.byref(total), _stream_ptr())
    if errcode == 8192:  # FA_ERROR_DECODE_INIT
        raise ValueError(f"Joining needs streams written by this library (a SEEKTABLE with one point per frame; reindex() adopts other "
                         f"stores) with the block size of level {level}, {nch} channel(s) and the stream sizes {sizes}")
    if errcode == 1 << 18:  # FA_ERROR_DECODE_SEEK
        raise RuntimeError("Joining failed: a seek table's offsets are not ordered inside the stream body, or a frame is shorter than "
                           "its header plus the CRC-16")
    if errcode != 0:
        raise RuntimeError(f"Joining failed, return code = {errcode}")
    return buf, index[:n_stream], index[n_stream:], total.value


def join_flac_device(stores, level=5, is_int64=False, verify=False, compact=False, max_temp_bytes=None):
    """Put device-resident stores behind one another along the sample axis as a NEW store: `stores` is a sequence of
    (compressed, starts, nbytes, stream_size) on one GPU, all of one number of streams; returns the new (compressed,
    starts, nbytes), all on the device (starts / nbytes have the shape of the first part's), the arguments left as they
    are.  A single part is copied verbatim, its STREAMINFO MD5 included; every other result has a zero one.

    Every part must have this library's layout (one SEEKTABLE point per frame; reindex_flac_device adopts others) and
    `level` the level ALL parts were written at (its block size B is checked against the streams' STREAMINFO).  For
    streams of integers the result is then byte for byte encode_flac_device(cat(x_i, dim=-1), level) with x_i the decoded
    parts (for float stores written with one set of offsets and gains: of the quantised integers), for any number of
    parts of any lengths.

    Every part but the last a whole number of blocks long (fa_join_device, include/flacarray_hip.h, K15): no sample is
    decoded and nothing is encoded.  The frames of part p are copied with their numbers raised by the frames in front of
    them (number field, CRC-8, CRC-16 by its linear identity), the seek table is rebuilt in closed form from the parts'
    tables, and the first part, whose numbers and offsets do not change, moves as two plain copies.

    Otherwise, with j the first part (other than the last) behind which the running total is not a multiple of B, every
    frame behind that point changes, and this route COSTS A DECODE PLUS AN ENCODE of everything behind the first
    unaligned boundary: parts 0 .. j are joined as above (part j is the last of that call, so it may be short), and the
    remaining parts are decoded and appended with append_flac_device, whose any-split contract makes the result the
    one-shot encode.  That is done in row chunks of at most `max_temp_bytes` of decoded samples (default 256 MiB, at least
    one row): each chunk selects its rows of the joined prefix through window_flac_device(streams=...) (pure selection)
    and the pieces are put back to back.  At 4096 x 2^20 and the default chunk size IT IS SLOWER THAN DECODING THOSE PARTS
    AND APPENDING THEM IN ONE GO, 71 ms against 28 ms, for 24.6 GB of extra memory against 39.7 GB (profiles/join.md).

    `compressed` is a view of a buffer sized for the worst case (the parts' bytes plus the grown headers), which it keeps
    alive; `compact=True` returns an exact-size copy instead.  `verify=True`: frame_status_device over the RESULT must be
    all zero (every frame carries its new number, its block size, a clean CRC-8 and CRC-16), else RuntimeError naming the
    first (stream, frame, status); on the unaligned route the appended span is also verified as append_flac_device(verify=
    True) does.

    ValueError: no store, a level outside 0-8, parts of different stream counts, a stream size <= 0, or streams that are
    not this library's for the call's block size, channel count (is_int64: two) and stream sizes.  RuntimeError: a seek
    table whose offsets are not ordered inside the stream body or a frame shorter than its header plus CRC-16 (refused by
    the check kernel's error word before anything is read through such an offset).  At most 65536 parts per call."""
    torch = _torch()
    stores = [tuple(s) for s in stores]
    for s in stores:
        if len(s) != 4:
            raise ValueError("every store of a join is (compressed, starts, nbytes, stream_size)")
        if s[0].dtype != torch.uint8:
            raise ValueError("Compressed data should be of type uint8")
        if s[1].dtype != torch.int64 or s[2].dtype != torch.int64 or s[1].shape != s[2].shape:
            raise ValueError("starts and nbytes should be int64 tensors of one shape")
    B, sizes, j = _join_args([int(np.prod(s[1].shape)) for s in stores], [s[3] for s in stores], level)
    if len(stores) > 65536:
        raise ValueError("a join takes at most 65536 parts per call (join the parts in groups)")
    dev = stores[0][0].device
    if not all(t.is_cuda and t.device == dev for s in stores for t in s[:3]):
        raise RuntimeError("join_flac_device needs every compressed, starts and nbytes on the same GPU")
    out_shape = tuple(stores[0][1].shape)
    n_stream = int(np.prod(out_shape))
    if n_stream == 0:
        return stores[0][0].new_empty(0), stores[0][1].new_empty(out_shape), stores[0][2].new_empty(out_shape)
    nch = 2 if is_int64 else 1
    L = _lib.lib()
    with _on_device(dev):
        flat = []
        for comp, st, nb, _ in stores:
            comp = comp.contiguous()
            if comp.data_ptr() & 15:  # (the copy reads its sources in aligned 16-byte blocks)
                comp = comp.clone()
            flat.append((comp, st.reshape(-1).contiguous(), nb.reshape(-1).contiguous()))
        n_pre = len(flat) if j is None else j + 1
        buf, starts2, nbytes2, total = _join_aligned(L, flat[:n_pre], sizes[:n_pre], n_stream, nch, level, dev)
        blob = buf[:total]
        if j is not None:
            # unaligned: the rest is decoded and appended, a chunk of rows at a time
            size_pre, n_rest = sum(sizes[:n_pre]), sum(sizes[n_pre:])
            cap = (256 << 20) if max_temp_bytes is None else int(max_temp_bytes)
            per = max(1, cap // (n_rest * 4 * nch))
            blobs, counts = [], []
            for r0 in range(0, n_stream, per):
                r1 = min(r0 + per, n_stream)
                if r1 - r0 == n_stream:
                    sub = (blob, starts2, nbytes2)
                else:
                    sub = window_flac_device(blob, starts2, nbytes2, size_pre, streams=np.arange(r0, r1), level=level, is_int64=is_int64)
                xs = [decode_flac_device(c, st[r0:r1], nb[r0:r1], n, is_int64=is_int64).reshape(r1 - r0, n)
                      for (c, st, nb), n in zip(flat[n_pre:], sizes[n_pre:])]
                x = xs[0] if len(xs) == 1 else torch.cat(xs, dim=1)
                del xs
                # (compact: a piece must not keep its worst-case buffer alive while the others are made)
                b, _, nbs = append_flac_device(sub[0], sub[1], sub[2], size_pre, x.contiguous(), level=level, verify=bool(verify), compact=True)
                blobs.append(b)
                counts.append(nbs.reshape(-1))
                del x, sub
            del buf
            nbytes2 = torch.cat(counts)
            starts2 = torch.cumsum(nbytes2, 0) - nbytes2
            blob = torch.cat(blobs) if len(blobs) > 1 else blobs[0]  # (exact-size either way)
        elif compact:
            blob = blob.clone()
            del buf
        out = (blob, starts2.reshape(out_shape), nbytes2.reshape(out_shape))
        if verify:
            status = frame_status_device(out[0], starts2, nbytes2, sum(sizes), is_int64=is_int64, block_size=B)
            bad = torch.nonzero(status.reshape(n_stream, -1))
            if bad.numel():
                s_bad, f_bad = (int(v) for v in bad[0])
                raise RuntimeError(f"Joining failed: {bad.shape[0]} frame(s) of the result do not check (first: stream {s_bad}, frame {f_bad}, "
                                   f"status {int(status.reshape(n_stream, -1)[s_bad, f_bad])})")
    return out
