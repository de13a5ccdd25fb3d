"""FlacArray container (reference: src/flacarray/array.py:19-884).

Holds the concatenated per-stream FLAC bytes plus the int64 `stream_starts` / `stream_nbytes`
index (and float32 offsets/gains for quantised float data) and decompresses numpy-style
selections on the fly through the MI355X decode path.  Same constructor arguments,
properties, `from_array` / `to_array` / `__getitem__` / `__eq__` semantics as the reference;
HDF5/Zarr I/O and the mpi4py distribution are outside this hot path (multi-GPU sharding lives
in flacarray_amd.dist).  `read_slices` is an addition: one batched launch for many scattered
(stream, sample-range) requests, which the reference can only serve one call at a time.
"""
import copy
from dataclasses import dataclass, field
from typing import Any, Optional, Tuple

import numpy as np

from .compress import array_compress
from .decompress import array_decompress_slice
from .utils import log, stream_md5

_KINDS = {"int32": (False, False), "int64": (True, False), "float32": (False, True), "float64": (True, True)}


@dataclass(frozen=True)
class _Store:
    """Everything a FlacArray knows about its compressed store, validated once and never mutated.

    The five arrays are the reference's triple (+ the two quantisation vectors); all other fields are derived
    from `shape` / `dtype` by `_Store.build`.  A single process holds the whole array here, so each `global_*`
    quantity equals its local twin (the reference fills them through mpi.py:93-187 when a communicator is given).
    """

    shape: Tuple[int, ...]            # the user's shape (a 1-D array stays 1-D)
    global_shape: Tuple[int, ...]
    dtype: np.dtype
    blob: Any                         # uint8, all streams back to back
    starts: Any                       # int64 over the leading shape
    nbytes_per_stream: Any            # int64 over the leading shape
    offsets: Optional[Any]            # float data only
    gains: Optional[Any]
    dist: Any = None
    # derived
    single: bool = field(default=False)          # the original was 1-D: one stream, results are flattened
    grid: Tuple[int, ...] = field(default=())     # shape with the stream axis made explicit
    kind: str = field(default="int32")
    wide: bool = field(default=False)             # 64-bit samples: two FLAC channels per stream

    @classmethod
    def build(cls, shape, global_shape, dtype, blob, starts, nbytes, offsets, gains, dist=None):
        dt = np.dtype(dtype)
        kind = next((k for k in _KINDS if dt == np.dtype(k)), None)
        if kind is None:
            raise RuntimeError(f"Unsupported dtype '{dt}'")
        shp = tuple(int(n) for n in shape)
        single = len(shp) == 1
        grid = (1,) + shp if single else shp
        gshape = tuple(int(n) for n in global_shape) if global_shape is not None else grid
        return cls(shp, gshape, dt, blob, starts, nbytes, offsets, gains, dist, single, grid, kind, _KINDS[kind][0])

    def clone(self):
        dup = copy.deepcopy
        return _Store.build(self.shape, self.global_shape, self.dtype, dup(self.blob), dup(self.starts), dup(self.nbytes_per_stream),
                            dup(self.offsets), dup(self.gains), dup(self.dist))

    # what the accessors below hand out
    lead = property(lambda s: s.grid[:-1])
    glead = property(lambda s: s.global_shape[:-1])
    samples = property(lambda s: s.grid[-1])
    blob_bytes = property(lambda s: int(s.blob.nbytes))
    count = property(lambda s: int(np.prod(s.grid[:-1], dtype=np.int64)))
    gcount = property(lambda s: int(np.prod(s.global_shape[:-1], dtype=np.int64)))


def _as_index(streams):
    """`streams` as the device calls take it: a numpy array (a tensor comes to the host)."""
    return streams.detach().cpu().numpy() if hasattr(streams, "detach") else np.asarray(streams)


def _exact_ratio(num, den):
    """num / den element by element as correctly rounded float64: Python integers divide exactly (object arrays)."""
    out = np.frompyfunc(lambda a, b: int(a) / int(b), 2, 1)(np.asarray(num, dtype=object), np.asarray(den, dtype=object))
    return np.asarray(out, dtype=np.float64)


@dataclass(frozen=True)
class StreamStats:
    """Binned statistics of a store (FlacArray.reduce): numpy arrays of shape leading_shape + (nbins,), or
    (len(streams), nbins) when streams were named.

    count     int64: samples in the bin (the last bin may be short).
    min, max  of the decoded values, exact: the integers of an integer store; for a float store int_to_float(min_int)
              in the array's dtype, which equals np.min / np.max of the decoded floats bit for bit (the restore is
              monotone for a positive gain).
    min_int, max_int   int64: min / max of the decoded integers (for a float store the quantised ones).
    sum       int64, equal to np.sum(x, dtype=np.int64) of the decoded integers: exact for 32-bit stores, modulo 2^64
              for 64-bit stores.
    sumsq_hi, sumsq_lo   uint64, 32-bit stores only (None for 64-bit stores): the exact sums of x*x >> 32 and of
              x*x mod 2^32 -- the sum of squares is sumsq_hi * 2^32 + sumsq_lo, exact below 2^32 samples per bin.
    sumsq     float64(sumsq_hi) * 2^32 + float64(sumsq_lo): the correctly rounded sum of squares whenever a bin has at
              most 2^21 samples (then sumsq_hi < 2^51 and sumsq_lo < 2^53 convert exactly and the one add rounds once).
              Above that it may be off by an ulp or two; the limbs stay exact.  None for 64-bit stores.
    offsets, gains   float64 columns broadcasting against the fields (float stores; else None)."""

    count: Any
    min: Any
    max: Any
    sum: Any
    sumsq_hi: Any
    sumsq_lo: Any
    min_int: Any
    max_int: Any
    offsets: Any = None
    gains: Any = None

    @property
    def sumsq(self):
        if self.sumsq_hi is None:
            return None
        return np.asarray(self.sumsq_hi).astype(np.float64) * 4294967296.0 + np.asarray(self.sumsq_lo).astype(np.float64)

    def mean(self):
        """float64 mean per bin from the exact fields: sum / count, correctly rounded, for an integer store.  For a float
        store it is offset + (sum / count) / gain in float64 -- the mean of offset + x / gain, NOT bit-equal to np.mean
        of the decoded float32 / float64 array, whose every sample was rounded on restore.  (A 64-bit store whose sum
        wrapped has no meaningful mean.)"""
        m = _exact_ratio(self.sum, self.count)
        if self.gains is not None:
            m = self.offsets + m / self.gains
        return m

    def std(self):
        """float64 population standard deviation per bin (np.std's ddof = 0), without cancellation: count * sum of
        squares - sum^2 is formed exactly in Python integers, divided by count^2, and the square root taken.  For a
        float store the result is divided by the gain: the deviation of offset + x / gain in float64, not bit-equal to
        np.std of the decoded float array.  64-bit stores carry no sum of squares: ValueError."""
        if self.sumsq_hi is None:
            raise ValueError("std needs the sum of squares, which 64-bit stores do not carry")
        c = np.asarray(self.count, dtype=object)
        s = np.asarray(self.sum, dtype=object)
        q = np.asarray(self.sumsq_hi, dtype=object) * (1 << 32) + np.asarray(self.sumsq_lo, dtype=object)
        sd = np.sqrt(_exact_ratio(c * q - s * s, c * c))
        if self.gains is not None:
            sd = sd / np.abs(self.gains)
        return sd


@dataclass(frozen=True)
class CrossStreamStats:
    """Per-sample statistics ACROSS the streams of each group (FlacArray.common_mode): numpy arrays, G groups, n samples.

    count     int64 [G]: streams in the group.
    sum       int64 [G, n], equal to np.sum(x[sel_g, first:last], axis=0, dtype=np.int64) of the decoded integers (for a
              float store the quantised ones): exact for 32-bit stores, modulo 2^64 for 64-bit stores.
    sumsq_hi, sumsq_lo   uint64 [G, n], 32-bit stores only (None for 64-bit stores): the exact sums of x*x >> 32 and of
              x*x mod 2^32 over the group's streams, the limbs StreamStats carries.
    sumsq     float64(sumsq_hi) * 2^32 + float64(sumsq_lo), as StreamStats.sumsq.  None for 64-bit stores.
    offsets_mean, gain   float64 [G] (a float store whose every group shares one gain; else None): the mean of the
              group's offsets (math.fsum / count; NaN for an empty group) and the group's gain."""

    count: Any
    sum: Any
    sumsq_hi: Any
    sumsq_lo: Any
    offsets_mean: Any = None
    gain: Any = None

    @property
    def sumsq(self):
        if self.sumsq_hi is None:
            return None
        return np.asarray(self.sumsq_hi).astype(np.float64) * 4294967296.0 + np.asarray(self.sumsq_lo).astype(np.float64)

    def _counts(self):
        """count broadcast over the samples, and which groups are empty."""
        c = np.broadcast_to(np.asarray(self.count, dtype=np.int64)[:, None], np.asarray(self.sum).shape)
        return c, c == 0

    def mean(self):
        """float64 mean across the group's streams per sample, [G, n], from the exact fields: sum / count, correctly
        rounded, for an integer store (or a float store read with quantised=True: integer units).  For a float store it
        is fsum(offsets_g) / count + (sum / count) / gain in float64 -- the mean of offset + x / gain, NOT bit-equal to
        np.mean over the decoded float32 / float64 streams, whose every sample was rounded on restore.  An empty group
        gives NaN.  (A 64-bit store whose sum wrapped has no meaningful mean.)"""
        c, empty = self._counts()
        m = _exact_ratio(self.sum, np.where(empty, 1, c))
        if self.gain is not None:
            m = np.asarray(self.offsets_mean)[:, None] + m / np.asarray(self.gain)[:, None]
        m[empty] = np.nan
        return m

    def std(self):
        """float64 population standard deviation across the group's streams per sample (np.std's ddof = 0), [G, n],
        without cancellation: count * sum of squares - sum^2 is formed exactly in Python integers, divided by count^2,
        and the square root taken.  For a float store the result is divided by |gain|: the deviation of x / gain in
        float64 -- the scatter of the quantised signal about its common mode, the streams' offsets not included -- NOT
        bit-equal to np.std over the decoded float streams.  An empty group gives NaN.  64-bit stores carry no sum of
        squares: ValueError."""
        if self.sumsq_hi is None:
            raise ValueError("std needs the sum of squares, which 64-bit stores do not carry")
        c, empty = self._counts()
        c = np.where(empty, 1, c).astype(object)
        s = np.asarray(self.sum, dtype=object)
        q = np.asarray(self.sumsq_hi, dtype=object) * (1 << 32) + np.asarray(self.sumsq_lo, dtype=object)
        sd = np.sqrt(_exact_ratio(c * q - s * s, c * c))
        if self.gain is not None:
            sd = sd / np.abs(np.asarray(self.gain))[:, None]
        sd[empty] = np.nan
        return sd


@dataclass(frozen=True)
class StreamDots:
    """Inner products of every stream with K templates (FlacArray.dot): numpy arrays over leading_shape + (K,), or over
    (len(streams), K) when streams were named; without the K axis when one 1-D template was given.

    exact         object array of Python integers: sum_j x[r, first + j] * T[k, j] over the decoded integers (for a
                  float store the quantised ones).  Exact whatever the magnitudes.
    template_sum  object array [K] (a Python integer for a 1-D template): sum_j T[k, j].
    count         samples in the range, last - first.
    offsets, gain float64 arrays broadcastable against `exact` (a float store read without quantised=True; else None)."""

    exact: Any
    template_sum: Any
    count: int
    offsets: Any = None
    gain: Any = None

    def value(self):
        """float64 inner products.  Integer stores (or quantised=True): float(exact), correctly rounded.  Float stores
        restore as offset + x / gain, so the product with template k is offset[r] * template_sum[k] + exact[r, k] /
        gain[r], formed in float64 per row from the exact integers -- every row has its own gain and nothing is mixed.
        NOT bit-equal to a matmul over the decoded floats, whose every sample was rounded on restore."""
        ex = np.asarray(self.exact, dtype=object)
        v = np.asarray(np.frompyfunc(float, 1, 1)(ex), dtype=np.float64) if ex.size else np.zeros(ex.shape, dtype=np.float64)
        if self.gain is None:
            return v
        ts = np.asarray(np.frompyfunc(float, 1, 1)(np.asarray(self.template_sum, dtype=object)), dtype=np.float64)
        return np.asarray(self.offsets, dtype=np.float64) * ts + v / np.asarray(self.gain, dtype=np.float64)


@dataclass(frozen=True)
class StreamHistogram:
    """Value histogram of a store (FlacArray.histogram): numpy arrays over leading_shape, or over (len(streams),) when
    streams were named.

    counts    int64, shape (..., bins): samples x of the row with lo + (b << shift) <= x < lo + ((b + 1) << shift).
    below, above   int64, shape (...): samples under lo, and at or over lo + (bins << shift).  counts.sum(-1) + below +
              above is the length of the sample range for every row.
    lo, shift int64 / int32, shape (...): each row's first edge and the log2 of its bin width.
    offsets, gains   float64, shape (...) (float stores; else None).  A float store is counted in its quantised
              integers -- what any FLAC decoder produces, the domain FlacArray.reduce works in."""

    counts: Any
    below: Any
    above: Any
    lo: Any
    shift: Any
    offsets: Any = None
    gains: Any = None

    def edges(self):
        """The bins + 1 edges of every row, lo + (arange(bins + 1) << shift), shape (..., bins + 1), formed in Python
        integers: int64 where every edge fits, an object array of Python integers otherwise (the last edges of a row
        whose range ends near INT64_MAX lie beyond it)."""
        bins = np.asarray(self.counts).shape[-1]
        lo, sh = np.asarray(self.lo), np.asarray(self.shift)
        out = np.empty(lo.shape + (bins + 1,), dtype=object)
        for i in np.ndindex(lo.shape):
            out[i] = [int(lo[i]) + (j << int(sh[i])) for j in range(bins + 1)]
        flat = [e for e in out.reshape(-1)]
        if all(-(1 << 63) <= e < (1 << 63) for e in flat):
            return out.astype(np.int64)
        return out

    def float_edges(self):
        """The edges in the units of a float store: offset + edge / gain in float64 -- the restore formula applied to
        the integer edges, NOT bit-equal to what the float32 / float64 restore of a sample gives (as StreamStats.mean).
        ValueError for an integer store."""
        if self.gains is None:
            raise ValueError("float_edges needs a float store")
        ef = np.asarray(np.frompyfunc(float, 1, 1)(self.edges().astype(object)), dtype=np.float64)
        return np.asarray(self.offsets)[..., None] + ef / np.asarray(self.gains)[..., None]


@dataclass(frozen=True)
class StreamHits:
    """The samples a search found (FlacArray.find): numpy arrays, the hits listed once each, sorted by (row, position).
    Rows are the streams in flat C order, or the streams named, in the order asked.

    counts     int64, shape leading_shape -- (len(streams),) when streams were named: hits per row.
    offsets    int64 [rows + 1]: the exclusive prefix sum of the counts; row r owns hits offsets[r]:offsets[r + 1].
    rows       int64 [total]: the row of every hit.
    positions  int64 [total]: its sample index in the stream, ascending within a row.
    values     [total], the store's dtype: the sample itself -- for a float store the restored float, equal to
               to_array()[row, position] bit for bit.
    int_values int64 [total]: the decoded integer (for a float store the quantised one).
    first, last   the sample range searched; streams: the flat stream index of every row (None: all streams)."""

    counts: Any
    offsets: Any
    rows: Any
    positions: Any
    values: Any
    int_values: Any
    first: int = 0
    last: int = 0
    streams: Any = None

    def ranges(self, pad=0):
        """The hits as sample ranges: int64 [k, 3], rows (flat stream -- the row where no streams were named --, first,
        last) with `last` exclusive, in the format FlacArray.damaged_ranges returns.  Every hit is widened by `pad`
        samples on both sides and clipped to the searched [first, last); ranges of a row that touch or overlap are
        merged.  Sorted by (row, first).  A pure host function."""
        if isinstance(pad, bool) or not isinstance(pad, (int, np.integer)) or int(pad) < 0:
            raise ValueError("pad should be a non-negative integer")
        pad = int(pad)
        rows = np.asarray(self.rows, dtype=np.int64)
        pos = np.asarray(self.positions, dtype=np.int64)
        if pos.size == 0:
            return np.zeros((0, 3), dtype=np.int64)
        b = np.maximum(pos - pad, int(self.first))
        e = np.minimum(pos + pad + 1, int(self.last))
        # (within a row positions ascend, so do the ends: a range opens where the row changes or a gap is left)
        opens = np.ones(pos.size, dtype=bool)
        opens[1:] = (rows[1:] != rows[:-1]) | (b[1:] > e[:-1])
        at = np.flatnonzero(opens)
        close = np.append(at[1:] - 1, pos.size - 1)
        out = np.empty((at.size, 3), dtype=np.int64)
        r = rows[at]
        out[:, 0] = r if self.streams is None else np.asarray(self.streams, dtype=np.int64)[r]
        out[:, 1] = b[at]
        out[:, 2] = e[close]
        return out


def _auto_shift(mn, mx, bins):
    """Per row, the smallest shift with (max - min) >> shift < bins (int64 inputs, the difference taken unsigned); at most
    63, which only bins == 1 over a span of 2^63 and more reaches without meeting the condition."""
    span = np.asarray(mx, dtype=np.int64).view(np.uint64) - np.asarray(mn, dtype=np.int64).view(np.uint64)
    shift = np.zeros(span.shape, dtype=np.int32)
    for s in range(63):
        shift += ((span >> np.uint64(s)) >= np.uint64(bins)).astype(np.int32)
    return shift


# public read-only attribute -> (field or derived property of _Store, one-line description)
_ACCESSORS = {
    "shape": ("shape", "Shape of the array this object decompresses to."),
    "global_shape": ("global_shape", "Shape across all processes (equal to the local one without a communicator)."),
    "leading_shape": ("lead", "Local shape without the compressed (last) axis."),
    "global_leading_shape": ("glead", "Global shape without the compressed axis."),
    "stream_size": ("samples", "Number of samples in every stream."),
    "nbytes": ("blob_bytes", "Size of the local compressed bytes."),
    "global_nbytes": ("blob_bytes", "Size of the compressed bytes of all processes."),
    "nstreams": ("count", "Number of local streams."),
    "global_nstreams": ("gcount", "Number of streams of all processes."),
    "compressed": ("blob", "uint8 array: every stream's FLAC bytes, back to back."),
    "stream_starts": ("starts", "int64 byte offset of each stream inside `compressed`."),
    "stream_nbytes": ("nbytes_per_stream", "int64 byte count of each stream."),
    "global_stream_starts": ("starts", "Stream offsets inside the global byte range."),
    "global_stream_nbytes": ("nbytes_per_stream", "Stream byte counts of all processes."),
    "stream_offsets": ("offsets", "Per-stream offset removed before quantisation (float data; else None)."),
    "stream_gains": ("gains", "Per-stream scale applied at quantisation (float data; else None)."),
    "mpi_dist": ("dist", "Ranges of the leading axis held by each process (None here)."),
    "dtype": ("dtype", "numpy dtype of the decompressed samples."),
    "typestr": ("kind", "dtype as one of 'int32', 'int64', 'float32', 'float64'."),
}


def _store_reader(attr, doc):
    return property(lambda self: getattr(self._st, attr), doc=doc)


class FlacArray:
    """FLAC compressed array representation; the last axis is the compressed one.

    Constructed directly only to copy (`FlacArray(other)`); use `from_array` otherwise.
    Keyword arguments are those of the reference constructor (array.py:78-90).
    """

    def __init__(self, other, shape=None, global_shape=None, compressed=None, dtype=None, stream_starts=None,
                 stream_nbytes=None, stream_offsets=None, stream_gains=None, mpi_comm=None, mpi_dist=None):
        if (other._comm if other is not None else mpi_comm) is not None:
            raise NotImplementedError("mpi4py communicators are not supported; see flacarray_amd.dist for multi-GPU sharding")
        self._comm = None
        self._st = other._st.clone() if other is not None else _Store.build(
            shape, global_shape, dtype, compressed, stream_starts, stream_nbytes, stream_offsets, stream_gains, mpi_dist)
        self._resident = None  # device copies of (compressed, starts, nbytes, offsets, gains): see to_device(); never copied

    mpi_comm = property(lambda self: self._comm, doc="Always None: distribution goes through flacarray_amd.dist.")
    global_process_nbytes = property(lambda self: [self._st.blob_bytes], doc="Compressed bytes held by each process.")

    # the names the rest of this class uses for the store's fields
    _shape = property(lambda self: self._st.shape)
    _global_shape = property(lambda self: self._st.global_shape)
    _local_shape = property(lambda self: self._st.grid)
    _leading_shape = property(lambda self: self._st.lead)
    _global_leading_shape = property(lambda self: self._st.glead)
    _stream_size = property(lambda self: self._st.samples)
    _flatten_single = property(lambda self: self._st.single)
    _compressed = property(lambda self: self._st.blob)
    _stream_starts = property(lambda self: self._st.starts)
    _global_stream_starts = property(lambda self: self._st.starts)
    _stream_nbytes = property(lambda self: self._st.nbytes_per_stream)
    _stream_offsets = property(lambda self: self._st.offsets)
    _stream_gains = property(lambda self: self._st.gains)
    _dtype = property(lambda self: self._st.dtype)
    _typestr = property(lambda self: self._st.kind)
    _is_int64 = property(lambda self: self._st.wide)
    _local_nbytes = property(lambda self: self._st.blob_bytes)

    # ---- numpy-style selection -> decode ----
    def _plan_selection(self, raw_key):
        """Turn a numpy-style key into (result shape, keep mask over the streams, first, last sample).

        Same results as the reference's key handling (array.py:297-407): integers drop their axis,
        slices keep it, an out-of-range integer on a leading axis gives an empty result instead of an
        IndexError, the stream axis takes an integer or a step-1 slice, and the streams are picked
        through a boolean mask (so a negative leading step does not reverse their order)."""
        key = raw_key if isinstance(raw_key, tuple) else (raw_key,)
        if self._flatten_single:  # a 1-D array: the user's key addresses the samples only
            if len(key) != 1:
                raise ValueError(f"Slice key {raw_key} is not valid for single, flattened stream.")
            key = (0,) + key
        ndim = len(self._local_shape)
        if len(key) > ndim:
            raise ValueError(f"Invalid slice key {raw_key}, too many dimensions")
        key = key + (slice(None),) * (ndim - len(key))
        *lead_key, samp_key = key

        # stream axis
        n = self._stream_size
        if samp_key is None:
            first, last, samp_shape = 0, n, (n,)
        elif isinstance(samp_key, slice):
            first, last, step = samp_key.indices(n)
            if step != 1:
                raise ValueError("Only stride==1 supported on stream slices")
            if last <= first:
                first, last = 0, 0
            samp_shape = (last - first,)
        elif isinstance(samp_key, (int, np.integer)):
            first, last, samp_shape = samp_key, samp_key + 1, ()
        else:
            raise ValueError("Stream dimension supports contiguous slices or single indices.")

        # leading axes
        lead_shape = []
        nothing = False
        for k, dim in zip(lead_key, self._leading_shape):
            if isinstance(k, (int, np.integer)):
                if not 0 <= k < dim:
                    lead_shape.append(0)
                    nothing = True
            else:
                lo, hi, st = k.indices(dim)
                lead_shape.append(len(range(lo, hi, st)))
        keep = None
        if len(lead_key) > 0:
            keep = np.zeros(self._leading_shape, dtype=bool)
            if not nothing:
                keep[tuple(lead_key)] = True
        return tuple(lead_shape) + samp_shape, keep, first, last

    # ---- HBM residency (addition to the reference API) ----
    def to_device(self, device=None):
        """Keep the compressed store resident in HBM: bytes, starts, nbytes (and offsets / gains) are uploaded
        once; `__getitem__`, `to_array` and `read_slices` then decode straight from those tensors and only the
        decoded samples cross PCIe.  The reference's usage pattern is many small reads from one store
        (array.py:409-449: one decode call per key); without residency every read re-uploads its byte span.
        Returns self."""
        import torch

        dev = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
        flat = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a, dtype=dt).reshape(-1)).to(dev)  # noqa: E731
        res = {
            "device": dev,
            "compressed": torch.from_numpy(np.ascontiguousarray(self._compressed)).to(dev),
            "starts": flat(self._stream_starts, np.int64),
            "nbytes": flat(self._stream_nbytes, np.int64),
            "offsets": None,
            "gains": None,
        }
        if self._stream_offsets is not None:
            ft = np.float64 if self._is_int64 else np.float32
            res["offsets"] = flat(self._stream_offsets, ft)
            res["gains"] = flat(self._stream_gains, ft)
        self._resident = res
        return self

    def _index(self):
        """The store's decode index (stream headers parsed, frame offsets tabulated once), built on first use."""
        res = self._resident
        if res.get("index") is None:
            from .libflacarray import DeviceDecodeIndex

            res["index"] = DeviceDecodeIndex(res["compressed"], res["starts"], res["nbytes"], self._stream_size, is_int64=self._is_int64)
        return res["index"]

    def release_device(self):
        """Drop the HBM copy made by to_device() (and its decode index)."""
        if self._resident is not None and self._resident.get("index") is not None:
            self._resident["index"].close()
        self._resident = None
        return self

    @property
    def is_resident(self):
        return self._resident is not None

    def _decode_resident(self, keep, first, last, as_tensor=False):
        """Decode [first, last) (negative: everything) of the kept streams from the resident store.
        Returns (2-D result: kept streams x samples, list of kept multi-indices or None)."""
        import torch

        res = self._resident
        indices = None
        off, gain = res["offsets"], res["gains"]
        if keep is None:
            out = self._index().decode(first, last, offsets=off, gains=gain)
        else:
            if keep.shape != tuple(self._leading_shape):
                raise RuntimeError("The keep array should have the same shape as stream_starts")
            sel = np.flatnonzero(np.asarray(keep).reshape(-1))
            indices = list(zip(*(ax.tolist() for ax in np.unravel_index(sel, self._leading_shape))))
            f0, n = (0, self._stream_size) if (first < 0 or last < 0) else (first, last - first)
            if sel.size == 0:
                out = torch.zeros((0, n), dtype=getattr(torch, self._typestr), device=res["device"])
            else:
                # the kept streams as one batch of slices against the index (one launch, nothing re-parsed)
                flat, _ = self._index().decode_slices(sel, np.full(sel.size, f0, np.int64), np.full(sel.size, n, np.int64), offsets=off, gains=gain,
                                                      to_host=not as_tensor)  # (host result: copied inside the decode call)
                out = flat.reshape(sel.size, n)
                if not as_tensor:
                    return out, indices
        return (out if as_tensor else out.cpu().numpy()), indices

    def __getitem__(self, raw_key):
        """Decompress a selection on the fly; the result has numpy's shape for the same key."""
        shape, keep, first, last = self._plan_selection(raw_key)
        if 0 in shape:
            return np.zeros(shape, dtype=self._dtype)
        if self._resident is not None:
            arr, _ = self._decode_resident(keep, first, last)
            return arr.reshape(shape)
        arr, _ = self._decode_host(keep, first, last)
        return arr.reshape(shape)

    def _decode_host(self, keep, first, last, **extra):
        """array_decompress_slice (decompress.py:18) over this store: bytes go up, samples come back."""
        st = self._st
        return array_decompress_slice(st.blob, st.samples, st.starts, st.nbytes_per_stream, stream_offsets=st.offsets,
                                      stream_gains=st.gains, keep=keep, first_stream_sample=first, last_stream_sample=last,
                                      is_int64=st.wide, **extra)

    def __delitem__(self, key):
        raise RuntimeError("Cannot delete individual streams")

    def __setitem__(self, key, value):
        raise RuntimeError("Cannot modify individual byte streams")

    def __repr__(self):
        return f"<FlacArray {self._typestr} shape={self._shape} bytes={self._local_nbytes}>"

    def __eq__(self, other):
        if self._shape != other._shape or self._dtype != other._dtype or self._global_shape != other._global_shape:
            log.debug("FlacArray shape/dtype mismatch")
            return False
        if not np.array_equal(self._stream_starts, other._stream_starts):
            return False
        if not np.array_equal(self._compressed, other._compressed):
            return False
        for mine, theirs in ((self._stream_offsets, other._stream_offsets), (self._stream_gains, other._stream_gains)):
            if (mine is None) != (theirs is None):
                return False
            if mine is not None and not np.allclose(mine, theirs):
                return False
        return True

    def to_array(self, keep=None, stream_slice=None, keep_indices=False, use_threads=False):
        """Decompress into a numpy array (array.py:518-584).

        `stream_slice`: step-1 slice of samples taken from every stream (normalised with
        slice.indices(); the reference forwards raw start/stop, so negative values there decode
        the whole stream).  `keep`: bool mask over the leading shape; the result is then the
        2-D array of kept streams (and their indices if `keep_indices`).
        """
        span = None
        if stream_slice is not None:
            if stream_slice.step not in (None, 1):
                raise RuntimeError("Only stream slices with a step size of 1 are supported")
            span = stream_slice.indices(self._stream_size)[:2]
        if self._resident is not None:
            lo, hi = span if span is not None else (-1, -1)
            if lo >= 0 and hi <= lo:
                raise RuntimeError("first_sample is larger than last_sample")
            arr, indices = self._decode_resident(keep, lo, hi)
            if keep is None:
                arr = arr.reshape(-1) if self._flatten_single else arr.reshape(self._shape[:-1] + (arr.shape[-1],))
        else:
            lo, hi = span if span is not None else (None, None)
            arr, indices = self._decode_host(keep, lo, hi, use_threads=use_threads, no_flatten=not self._flatten_single)
        return (arr, indices) if (keep is not None and keep_indices) else arr

    def read_slices(self, streams, first, count, as_tensor=False):
        """Batched random access (addition to the reference API).

        streams: flat (C-order) stream indices; first/count: sample ranges.  Returns a list of
        1-D arrays, one per request, decoded with ONE kernel launch on the GPU (as_tensor: the flat
        device tensor and the int64 array of its per-request offsets instead).  On a store made
        resident with to_device() nothing but the request table is uploaded.
        """
        import torch

        from .libflacarray import decode_slices_device

        res = self._resident
        if res is None:
            dev = torch.device("cuda", torch.cuda.current_device())
            comp = torch.from_numpy(np.ascontiguousarray(self._compressed)).to(dev)
            st = torch.from_numpy(np.ascontiguousarray(self._stream_starts).reshape(-1)).to(dev)
            nb = torch.from_numpy(np.ascontiguousarray(self._stream_nbytes).reshape(-1)).to(dev)
            off = gain = None
            if self._stream_offsets is not None:
                off = torch.from_numpy(np.ascontiguousarray(self._stream_offsets).reshape(-1))
                gain = torch.from_numpy(np.ascontiguousarray(self._stream_gains).reshape(-1))
        if res is not None:
            out, out_off = self._index().decode_slices(streams, first, count, offsets=res["offsets"], gains=res["gains"], to_host=not as_tensor)
            if not as_tensor:
                count = np.asarray(count, dtype=np.int64)
                return [out[o : o + c] for o, c in zip(out_off, count)]
        else:
            out, out_off = decode_slices_device(
                comp, st, nb, self._stream_size, streams, first, count, offsets=off, gains=gain, is_int64=self._is_int64
            )
        if as_tensor:
            return out, out_off
        flat = out.cpu().numpy()
        count = np.asarray(count, dtype=np.int64)
        return [flat[o : o + c] for o, c in zip(out_off, count)]

    def first_mismatch(self, data):
        """Check the store against `data` (a numpy array or a torch tensor of this array's shape and dtype) without
        decoding into memory: returns a numpy int64 array of the leading shape holding, per stream, the index of the
        first sample whose decoded value differs from `data`, or -1 where the stream decodes to `data`.  Float stores
        compare through their offsets and gains: what is compared is the quantised integers, not the floats, so a float
        change that leaves its quantised integer the same is not a mismatch.  Uses the resident store after to_device(),
        and uploads the store otherwise."""
        import torch

        from .libflacarray import compare_flac_device

        shape = tuple(int(n) for n in data.shape)
        if shape != tuple(self._shape):
            raise ValueError(f"data of shape {shape} does not match the array's shape {tuple(self._shape)}")
        dt = np.dtype(str(data.dtype).replace("torch.", "")) if isinstance(data, torch.Tensor) else data.dtype
        if dt != self._dtype:
            raise ValueError(f"data of dtype {dt} does not match the array's dtype {self._dtype}")
        dev, comp, st, nb, off, gain = self._device_store(scale=True)
        if isinstance(data, torch.Tensor):
            x = data.to(dev).contiguous()
        else:
            x = torch.from_numpy(np.ascontiguousarray(data)).to(dev)
        first = compare_flac_device(comp, st, nb, x.reshape(self._st.count, self._stream_size), off, gain)
        return first.cpu().numpy().reshape(self._leading_shape)

    def reduce(self, width=None, first=0, last=None, streams=None):
        """Binned statistics of the store without decoding it into memory (addition to the reference API): samples
        [first, last) (default: everything) of every stream, or of the streams named, are cut into
        nbins = ceil((last - first) / width) bins of `width` samples, the last one possibly short; width=None is one bin
        over the range.  Returns a StreamStats of numpy arrays of shape leading_shape + (nbins,): per-bin count, exact
        min and max, the exact integer sum and (32-bit stores) the two exact limbs of the sum of squares, with mean() and
        std() computed from them on the host.  A float store reports min / max as floats that equal np.min / np.max of
        the decoded array exactly, keeps sum and the squares in the integer domain (min_int / max_int are the integer
        extremes) and maps mean() / std() through its offsets and gains in float64.

        `streams`: a 1-D integer array of flat C-order stream indices (as overwrite takes them; out of range or named
        twice: ValueError); the fields then have shape (len(streams), nbins), rows in the order asked, and an empty
        `streams` returns empty arrays.  width < 1 or an empty or out-of-range [first, last) raise ValueError.

        int32 / float32 stores are reduced inside the decoder, each frame's running values in registers: nothing but
        the bins is written, and the call costs about what a decode costs (bins of 8 samples: five times that, still
        half of decode-then-torch).  int64 / float64 stores are decoded in column chunks of at most 256 MiB that are
        folded into the bins on the device: 30 times less extra memory than a decoded copy, but 3.6 times SLOWER than
        decoding everything and reducing with torch where that copy fits (profiles/reduce.md); reduce_flac_device takes
        a larger `max_temp_bytes`.  Uses the resident store and its decode index after to_device(), and uploads the
        store otherwise.  Decode failures raise the decoder's RuntimeError."""
        from .libflacarray import _reduce_args, reduce_flac_device, wrap_int32_to_float32

        st = self._st
        first, last, width, nbins, idx = _reduce_args(st.count, st.samples, width, first, last, streams)
        rows = st.count if idx is None else int(idx.size)
        shape = (tuple(st.lead) if idx is None else (rows,)) + (nbins,)
        n = last - first
        count = np.full(nbins, width, dtype=np.int64)
        count[-1] = n - (nbins - 1) * width
        count = np.broadcast_to(count, (rows, nbins)).reshape(shape).copy()
        if rows == 0:
            z = lambda dt: np.zeros(shape, dtype=dt)  # noqa: E731
            limb = None if st.wide else z(np.uint64)
            return StreamStats(count, z(st.dtype), z(st.dtype), z(np.int64), limb, limb, z(np.int64), z(np.int64))
        res = self._resident
        if res is not None:
            out = self._index().reduce(width, first, last, streams=idx)
        else:
            _, comp, starts, nbytes = self._device_store()
            out = reduce_flac_device(comp, starts, nbytes, st.samples, width, first, last, streams=idx, is_int64=st.wide)
        mn, mx, sm, qh, ql = (None if t is None else t.cpu().numpy() for t in out)
        lo, hi, off, gain = mn, mx, None, None
        if st.offsets is not None:
            pick = (lambda a: np.asarray(a).reshape(-1)) if idx is None else (lambda a: np.asarray(a).reshape(-1)[idx])  # noqa: E731
            it = np.int64 if st.wide else np.int32
            lo, hi = (wrap_int32_to_float32(v.astype(it).reshape(-1), rows, nbins, pick(st.offsets), pick(st.gains), _f64=st.wide).reshape(shape)
                      for v in (mn, mx))
            off = pick(st.offsets).astype(np.float64).reshape(shape[:-1] + (1,))
            gain = pick(st.gains).astype(np.float64).reshape(shape[:-1] + (1,))
        else:
            lo, hi = mn.astype(st.dtype).reshape(shape), mx.astype(st.dtype).reshape(shape)
        limbs = (None, None) if qh is None else (qh.view(np.uint64).reshape(shape), ql.view(np.uint64).reshape(shape))
        return StreamStats(count, lo, hi, sm.reshape(shape), limbs[0], limbs[1], mn.reshape(shape), mx.reshape(shape), off, gain)

    def common_mode(self, groups=None, first=0, last=None, streams=None, quantised=False, verify=None):
        """Per-sample statistics ACROSS streams without decoding the store into memory (addition to the reference API):
        for every sample of [first, last) (default: everything; first == last gives arrays of zero columns) the sum, and
        for 32-bit stores the exact sum of squares, over the streams of each group -- the common mode of a detector
        time-stream matrix and the scatter about it.  Returns a CrossStreamStats of numpy arrays: count [G], sum [G, n],
        sumsq_hi / sumsq_lo [G, n], with mean() and std() computed from them on the host.

        `streams`: 1-D flat C-order stream indices with no repeats, as FlacArray.reduce takes them (default: all).
        `groups`: None for one group, or one integer label in [0, G) per selected stream, G = largest label + 1; labels may
        come in any order and a label nobody carries is an empty group (count 0, sums 0, mean and std NaN).

        Float stores restore as offset + x / gain, and a sum of quantised integers has a unit only where the group
        shares one gain bit for bit -- the scalar quanta= case.  There mean() is fsum(offsets_g) / count + (sum / count) /
        gain and std() is divided by |gain|.  A float store with a group of mixed gains raises ValueError: compress with a
        scalar quanta=, or pass quantised=True, which returns the integer fields for any store with mean() and std() in
        integer units.

        int32 / float32 stores are summed inside the decoder (K7X: a wavefront holds the same frame of 64 streams and
        folds its tile's columns across lanes); int64 / float64 stores through decoded column chunks of at most 256 MiB.
        Timings against the bare decode and against decode-then-torch: profiles/common_mode.md.  Uses the resident store
        and its decode index after to_device(), and uploads the store otherwise.  `verify`: the decoder's frame CRC-16
        check (None: the process default).  Decode failures raise the decoder's RuntimeError."""
        import math

        from .libflacarray import _xsum_args, common_mode_flac_device

        st = self._st
        first, last, G, order, _, count = _xsum_args(st.count, st.samples, groups, None, first, last, streams, not st.wide, st.wide)
        off_mean = gain = None
        if st.offsets is not None and not quantised:
            # the check needs no GPU: it stands in front of the decode
            offs = np.asarray(st.offsets).reshape(-1)[order]
            gains = np.asarray(st.gains).reshape(-1)[order]
            ends = np.cumsum(count)
            off_mean, gain = np.full(G, np.nan), np.full(G, np.nan)
            for g in range(G):
                gg = gains[ends[g] - count[g] : ends[g]]
                if gg.size == 0:
                    continue
                bits = np.ascontiguousarray(gg).view("u%d" % gg.dtype.itemsize)  # (bit for bit: -0.0 and NaN included)
                if not np.all(bits == bits[0]):
                    raise ValueError(f"group {g} mixes gains: a sum of quantised integers has no unit there -- compress with a scalar "
                                     "quanta=, or pass quantised=True for the integer sums")
                off_mean[g] = math.fsum(float(v) for v in offs[ends[g] - count[g] : ends[g]]) / int(count[g])
                gain[g] = float(gg[0])
        # (the plan is made again from the same arguments by the device call: it is cheap and pure)
        idx = None if streams is None else _as_index(streams)
        if self._resident is not None:
            out = self._index().common_mode(groups, G, first, last, streams=idx, verify=verify)
        else:
            _, comp, starts, nbytes = self._device_store()
            out = common_mode_flac_device(comp, starts, nbytes, st.samples, groups, G, first, last, streams=idx, squares=not st.wide,
                                          is_int64=st.wide, verify=verify)
        sm, qh, ql = (None if t is None else t.cpu().numpy() for t in out)
        limbs = (None, None) if qh is None else (qh.view(np.uint64), ql.view(np.uint64))
        return CrossStreamStats(count, sm, limbs[0], limbs[1], off_mean, gain)

    def dot(self, templates, first=0, last=None, streams=None, quantised=False, verify=None):
        """Projections without decoding the store into memory (addition to the reference API): the exact inner product
        of samples [first, last) (default: everything) of every stream, or of the streams named, with each of K integer
        templates -- a detector's coupling to the common mode common_mode() returned, polynomial or ground-template
        coefficients, a Fourier coefficient at a chosen frequency.  Returns a StreamDots: `exact` (Python integers, shape
        leading_shape + (K,), or (len(streams), K) with rows in the order asked), `template_sum`, `count`, and value() in
        float64.

        `templates`: an integer array or tensor [K, n] or [n] (the K axis is then dropped from the result) with n = last -
        first exactly; K is unlimited.  Values may span all of int64 -- common_mode().sum passes int32 as soon as a few
        thousand 24-bit detectors are summed: the host splits such a template into 31-bit limb planes
        (dot_template_limbs), drops the planes that are all zero, runs the int32 kernel on what is left and recombines in
        Python integers.  A float template is refused with TypeError (quantise it: np.rint(T * 2**k)), a wrong length with
        ValueError, before anything touches the GPU.  `streams`: as FlacArray.reduce takes them.

        Float stores: value() is offset[r] * template_sum[k] + exact[r, k] / gain[r] per row (see StreamDots.value);
        quantised=True gives value() of the integers.

        int32 / float32 stores are multiplied inside the decoder (K7D), 8 template planes per decode of the range and
        ceil(planes / 8) decodes in all; int64 / float64 stores through decoded column chunks of at most 256 MiB.  What
        that costs against decode-then-matmul, and from which K on it LOSES: profiles/dot.md.  Uses the resident store
        and its decode index after to_device(), and uploads the store otherwise.  `verify`: the decoder's frame CRC-16
        check (None: the process default).  Decode failures raise the decoder's RuntimeError."""
        from .libflacarray import _dot_args, _dot_templates, dot_exact, dot_flac_device, dot_template_limbs, dot_template_unlimbs

        st = self._st
        first, last, idx, _ = _dot_args(st.count, st.samples, first, last, streams)
        T, single = _dot_templates(templates, last - first)
        K = T.shape[0]
        planes, index = dot_template_limbs(T)
        rows = int(idx.size)
        parts = np.zeros((rows, planes.shape[0]), dtype=object)
        if rows and planes.shape[0]:
            sel = None if streams is None else idx
            if self._resident is not None:
                out = self._index().dot(planes, first, last, streams=sel, verify=verify)
            else:
                _, comp, starts, nbytes = self._device_store()
                out = dot_flac_device(comp, starts, nbytes, st.samples, planes, first, last, streams=sel, is_int64=st.wide, verify=verify)
            parts = dot_exact(out) if st.wide else dot_exact(*out)
        exact = dot_template_unlimbs(parts, index, K)
        # (exact: the upper words sum inside int64 and the lower ones inside uint64 for any n the call accepts)
        tsum = np.asarray([int(np.sum(T[k] >> 32, dtype=np.int64)) * (1 << 32) + int(np.sum((T[k] & 0xFFFFFFFF).astype(np.uint64), dtype=np.uint64))
                           for k in range(K)], dtype=object)
        lead = tuple(st.lead) if streams is None else (rows,)
        off = gain = None
        if st.offsets is not None and not quantised:
            off = np.asarray(st.offsets).reshape(-1)[idx].astype(np.float64).reshape(lead + (() if single else (1,)))
            gain = np.asarray(st.gains).reshape(-1)[idx].astype(np.float64).reshape(lead + (() if single else (1,)))
        if single:
            return StreamDots(exact.reshape(lead), tsum[0], last - first, off, gain)
        return StreamDots(exact.reshape(lead + (K,)), tsum, last - first, off, gain)

    # ---- distributions: value histogram and exact order statistics from the compressed store ----
    def _hist_pass(self, store, lo, shift, nbins, first, last, idx):
        """One histogram pass (device tensors counts, below, above) on the resident index or on the uploaded `store`."""
        from .libflacarray import histogram_flac_device

        if self._resident is not None:
            return self._index().histogram(lo, shift, nbins, first, last, streams=idx)
        _, comp, starts, nbytes = store
        return histogram_flac_device(comp, starts, nbytes, self._st.samples, lo, shift, nbins, first, last, streams=idx, is_int64=self._st.wide)

    def _int_extremes(self, store, first, last, idx):
        """int64 numpy (min, max) per row of the decoded integers over [first, last)."""
        from .libflacarray import reduce_flac_device

        if self._resident is not None:
            out = self._index().reduce(None, first, last, streams=idx)
        else:
            _, comp, starts, nbytes = store
            out = reduce_flac_device(comp, starts, nbytes, self._st.samples, None, first, last, streams=idx, is_int64=self._st.wide)
        return out[0].cpu().numpy().reshape(-1), out[1].cpu().numpy().reshape(-1)

    def histogram(self, bins=256, lo=None, shift=None, first=0, last=None, streams=None):
        """Value histogram of every stream without decoding the store into memory (addition to the reference API): samples
        [first, last) (default: everything) of every stream, or of the streams named (as FlacArray.reduce takes them), are
        counted in `bins` (1..2048) bins of width 2^shift starting at `lo`.  `lo` (inside int64) and `shift` (0..63) are
        integers or integer arrays with one value per row.  Returns a StreamHistogram: counts of shape leading_shape +
        (bins,), below / above / lo / shift of shape leading_shape -- (len(streams), ...) when streams were named.

        With lo and shift both None the range is chosen per row: lo is the row's minimum over the range (one
        FlacArray.reduce pass) and shift the smallest value with (max - min) >> shift < bins, so that below and above
        are zero and every sample is counted.  Otherwise a missing lo is 0 and a missing shift is 0.

        A float store is counted in its quantised integers; StreamHistogram.float_edges() maps the edges through the
        offsets and gains in float64.

        int32 / float32 stores are counted inside the decoder (K7H), nothing but the counts written; int64 / float64
        stores are decoded in column chunks of at most 256 MiB that are counted on the device.  Measured
        (profiles/histogram.md): at 4096 x 2^20 int32 a pass takes 8.6 ms at 64, 256 and 2048 bins alike (the bare
        decode: 6.6 ms; reduce: 7.3), 15.8 ms when every sample falls into one bin, and 16-22 ms with the automatic
        range, which adds the reduce pass -- against 370-850 ms and 10 GiB of temporaries for decoding row chunks and
        scatter_add.  At 1024 x 2^20 int64 a pass takes 54-56 ms (the chunked decode: five times the bare decode's
        10.6 ms), 107-111 ms with the automatic range, against 97-213 ms and 17 GiB for decode-then-torch.  Uses the
        resident store and its decode index after
        to_device(), and uploads the store otherwise.  Argument errors raise ValueError before any GPU work."""
        from .libflacarray import _histogram_args, _reduce_args

        st = self._st
        first, last, _, _, idx = _reduce_args(st.count, st.samples, None, first, last, streams)
        rows = st.count if idx is None else int(idx.size)
        lead = tuple(st.lead) if idx is None else (rows,)
        auto = lo is None and shift is None
        bins, lo_h, shift_h = _histogram_args(rows, 0 if lo is None else lo, 0 if shift is None else shift, bins)
        off = gain = None
        if st.offsets is not None:
            pick = (lambda a: np.asarray(a).reshape(-1)) if idx is None else (lambda a: np.asarray(a).reshape(-1)[idx])  # noqa: E731
            off, gain = pick(st.offsets).astype(np.float64).reshape(lead), pick(st.gains).astype(np.float64).reshape(lead)
        if rows == 0:
            z = np.zeros(lead, dtype=np.int64)
            return StreamHistogram(np.zeros(lead + (bins,), dtype=np.int64), z, z.copy(), z.copy(), z.astype(np.int32), off, gain)
        store = None if self._resident is not None else self._device_store()
        if auto:
            mn, mx = self._int_extremes(store, first, last, idx)
            lo_h, shift_h = mn.astype(np.int64), _auto_shift(mn, mx, bins)
        counts, below, above = (t.cpu().numpy() for t in self._hist_pass(store, lo_h, shift_h, bins, first, last, idx))
        return StreamHistogram(counts.reshape(lead + (bins,)), below.reshape(lead), above.reshape(lead), lo_h.reshape(lead),
                               shift_h.reshape(lead), off, gain)

    def order_statistic(self, ranks, first=0, last=None, streams=None):
        """Exact order statistics of every stream from the compressed store (addition to the reference API): element
        `ranks` of the sorted samples [first, last) of each row.  `ranks`: integers in [0, last - first), 1-D of length r
        (shared by all rows) or of shape (rows, r).  Returns np.sort(x[..., first:last], axis=-1)[..., ranks] exactly, in
        the array's dtype, shape leading_shape + (r,) -- (len(streams), r) when streams were named.  For a float store
        it is the restored float of the integer order statistic, which equals the order statistic of to_array() bit for
        bit (the restore is monotone for a positive gain: the argument StreamStats.min / max rest on).

        The value range is narrowed by histogram passes of 2048 bins: one FlacArray.reduce pass for the extremes, one
        coarse histogram pass shared by all ranks, then per rank at most ceil(shift0 / 11) passes -- 2 for 32-bit stores,
        5 for 64-bit ones -- each of which costs a histogram pass over the range.  Measured (profiles/histogram.md): at
        4096 x 2^20 int32, 24 ms for one rank and 41 ms for three, with 0.26 GiB of temporaries, against 172 / 493 ms
        (4 GiB) for decoding row chunks and torch.kthvalue and 738 ms (8 GiB) for torch.sort.  For 64-bit stores it is
        SLOWER than decode-then-torch wherever the decoded copy fits: at 1024 x 2^20 int64, 280 ms for one rank and
        597 ms for three against 91 / 249 ms for kthvalue and 240 ms for sort -- every pass is a chunked decode of 54 ms
        -- and what it buys is memory: 0.64 GiB beside the store instead of 13-17 GiB.  Only the bin found travels
        to the host."""
        import torch

        from .libflacarray import _reduce_args, wrap_int32_to_float32

        st = self._st
        first, last, _, _, idx = _reduce_args(st.count, st.samples, None, first, last, streams)
        n = last - first
        rows = st.count if idx is None else int(idx.size)
        lead = tuple(st.lead) if idx is None else (rows,)
        rk = np.asarray(ranks)
        if rk.size and rk.dtype.kind not in "iu":
            raise ValueError("ranks should be integers")
        if rk.ndim == 1:
            rk = np.broadcast_to(rk.astype(np.int64), (rows, rk.size))
        elif rk.ndim == 2 and rk.shape[0] == rows:
            rk = rk.astype(np.int64)
        else:
            raise ValueError(f"ranks should be 1-D, or of shape ({rows}, r)")
        if rk.size and (rk.min() < 0 or rk.max() >= n):
            raise ValueError(f"ranks holds a value outside [0, {n})")
        r = rk.shape[1]
        vals = np.zeros((rows, r), dtype=np.int64)
        if rows and r:
            store = None if self._resident is not None else self._device_store()
            mn, mx = self._int_extremes(store, first, last, idx)
            lo0, shift0 = mn.astype(np.int64), _auto_shift(mn, mx, 2048)

            def narrow(counts, below, k):
                # the first bin whose cumulative count exceeds the rank left once the samples under lo are taken off
                cum = torch.cumsum(counts, dim=1)
                kk = torch.from_numpy(k).to(counts.device) - below
                return (cum <= kk[:, None]).sum(dim=1).clamp_(max=counts.shape[1] - 1).cpu().numpy()

            coarse = self._hist_pass(store, lo0, shift0, 2048, first, last, idx)  # shared by every rank column
            for c in range(r):
                k = np.array(rk[:, c])  # (a writable copy)
                lo_c, sh_c = lo0.copy(), shift0.copy()
                counts, below, _ = coarse
                while True:
                    lo_c = lo_c + (narrow(counts, below, k).astype(np.int64) << sh_c.astype(np.int64))
                    if not sh_c.any():  # a pass has run at shift 0 for every row: lo is the answer
                        break
                    sh_c = np.maximum(sh_c - 11, 0).astype(np.int32)
                    counts, below, _ = self._hist_pass(store, lo_c, sh_c, 2048, first, last, idx)
                vals[:, c] = lo_c
        if st.offsets is not None:
            pick = (lambda a: np.asarray(a).reshape(-1)) if idx is None else (lambda a: np.asarray(a).reshape(-1)[idx])  # noqa: E731
            it = np.int64 if st.wide else np.int32
            if rows == 0 or r == 0:
                return np.zeros(lead + (r,), dtype=st.dtype)
            out = wrap_int32_to_float32(vals.astype(it).reshape(-1), rows, r, pick(st.offsets), pick(st.gains), _f64=st.wide)
            return np.asarray(out).reshape(lead + (r,))
        return vals.astype(st.dtype).reshape(lead + (r,))

    def quantile(self, q, method="lower", first=0, last=None, streams=None):
        """Exact quantiles per stream: FlacArray.order_statistic at rank floor (method "lower") or ceil ("higher") of the
        float64 product q * (n - 1), n = last - first -- numpy's rule for these two methods, so the result equals
        np.quantile(x[..., first:last], q, axis=-1, method=method).  A scalar q gives leading_shape; a 1-D q gives
        leading_shape + (len(q),) (numpy puts that axis first).  Other methods, or q outside [0, 1], raise ValueError.
        Cost: order_statistic's, one rank per q (64-bit stores: SLOWER than decode-then-torch where the copy fits)."""
        from .libflacarray import _reduce_args

        if method not in ("lower", "higher"):
            raise ValueError('method should be "lower" or "higher"')
        qa = np.asarray(q, dtype=np.float64)
        if qa.ndim > 1 or not np.all((qa >= 0.0) & (qa <= 1.0)):
            raise ValueError("q should be a number, or a 1-D array of numbers, in [0, 1]")
        f, l, _, _, _ = _reduce_args(self._st.count, self._st.samples, None, first, last, None)
        pos = qa.reshape(-1) * np.float64(l - f - 1)
        ranks = (np.floor(pos) if method == "lower" else np.ceil(pos)).astype(np.int64)
        out = self.order_statistic(ranks, first, last, streams)
        return out[..., 0] if qa.ndim == 0 else out

    def median(self, first=0, last=None, streams=None):
        """float64 median per stream: (lower + higher) / 2 of the two middle order statistics (ranks (n - 1) // 2 and
        n // 2), each converted to float64 first.  For an int32 store this equals np.median exactly.  Cost:
        order_statistic's for two ranks: 34 ms at 4096 x 2^20 int32; 436 ms at 1024 x 2^20 int64, SLOWER than
        decode-then-torch where the decoded copy fits (profiles/histogram.md)."""
        from .libflacarray import _reduce_args

        f, l, _, _, _ = _reduce_args(self._st.count, self._st.samples, None, first, last, None)
        n = l - f
        two = self.order_statistic(np.array([(n - 1) // 2, n // 2], dtype=np.int64), first, last, streams).astype(np.float64)
        return (two[..., 0] + two[..., 1]) / 2.0

    # ---- searching: the positions of the samples outside per-row limits, from the compressed store ----
    def _find_limits(self, lo, hi, rows, idx, inside, max_hits, quantised):
        """The int64 limits per row of a search: integer limits as they are (integer stores, quantised=True), float
        limits of a float store through their exact integer images."""
        from .libflacarray import _find_args, float_limits_to_int, wrap_int32_to_float32

        st = self._st
        if st.offsets is None or quantised:
            return _find_args(rows, lo, hi, inside, max_hits)
        lo_f, hi_f, inside, max_hits = _find_args(rows, lo, hi, inside, max_hits, floats=True)
        pick = (lambda a: np.asarray(a).reshape(-1)) if idx is None else (lambda a: np.asarray(a).reshape(-1)[idx])  # noqa: E731
        off, gain = pick(st.offsets), pick(st.gains)
        g64 = gain.astype(np.float64)
        with np.errstate(all="ignore"):  # (the restore multiplies by 1 / gain in the store's type: that has to be finite too)
            ok = np.isfinite(g64) & (g64 > 0.0) & np.isfinite((1.0 / np.where(g64 > 0.0, g64, 1.0)).astype(gain.dtype))
        if rows and not np.all(ok):
            raise ValueError("a row's gain is not finite and positive: float limits have no integer image (use quantised=True)")
        if rows == 0:
            return np.zeros(0, dtype=np.int64), np.zeros(0, dtype=np.int64), inside, max_hits
        it = np.int64 if st.wide else np.int32
        ii = np.iinfo(it)
        restore = lambda q: wrap_int32_to_float32(q.astype(it), rows, 1, off, gain, _f64=st.wide)  # noqa: E731  (the library's own restore)
        lo_i, hi_i = float_limits_to_int(restore, lo_f, hi_f, int(ii.min), int(ii.max))
        return lo_i, hi_i, inside, max_hits

    def _find_run(self, lo_i, hi_i, first, last, idx, inside, max_hits, counts_only):
        from .libflacarray import find_flac_device

        if self._resident is not None:
            return self._index().find(lo_i, hi_i, first, last, streams=idx, inside=inside, max_hits=max_hits, _counts_only=counts_only)
        _, comp, starts, nbytes = self._device_store()
        return find_flac_device(comp, starts, nbytes, self._st.samples, lo_i, hi_i, first, last, streams=idx, inside=inside, max_hits=max_hits,
                                is_int64=self._st.wide, _counts_only=counts_only)

    def find(self, lo=None, hi=None, first=0, last=None, streams=None, inside=False, quantised=False, max_hits=None):
        """Where are the samples outside my limits -- without decoding the store into memory (addition to the reference
        API).  Sample x at position t in [first, last) (default: everything) of a row is a hit iff
        (x < lo or x > hi) != inside: by default the samples outside the closed interval [lo, hi], with inside=True those
        within it (lo == hi == v finds a sentinel value).  `lo` / `hi`: one value or one per row, None meaning no limit on
        that side; lo > hi is legal (everything hits, or with inside=True nothing).  Rows are all streams, or the streams
        named (`streams` as FlacArray.reduce takes it: flat indices, rows in the order asked, an empty list gives empty
        results).  Returns a StreamHits: counts, offsets, rows, positions, values, int_values, and ranges(pad) for flag
        intervals.  Every hit is listed once, sorted by (row, position); the result equals np.nonzero of the predicate on
        to_array(), and values equals to_array()[rows, positions], bit for bit.

        Integer stores take integer limits.  A float store takes float limits in the array's own units, compared exactly
        (as a.astype(float64) < lo): the restore offset + q / gain is monotone in the quantised integer q for a finite
        positive gain, so each limit has an exact integer image, found by bisection with the library's own restore (at
        most 65 small restore calls per limit); +-inf is "no limit", NaN or a row whose gain is not finite and positive
        raise ValueError.  quantised=True takes integer limits on a float store as they are.  More than `max_hits` hits
        raise ValueError, which names the total, before any position is written.

        int32 / float32 stores are searched inside the decoder (K7F) in two passes: a count pass over every frame --
        nothing but one count per frame written -- and a fill pass that decodes only the frames with a hit.  Measured
        (profiles/find.md) at 4096 x 2^20 int32: the count pass 6.3-6.5 ms (the bare decode 6.35, reduce with one bin
        7.2), the search 7.7 ms at two hits per row and 11.1 ms at one hit per thousand samples, against 58 ms and
        4 GiB for decoding row chunks and torch.nonzero; with every sample a hit, 80 ms.  int64 / float64 stores go
        through decoded column chunks of at most 256 MiB in BOTH passes and are SLOWER than decode-then-torch wherever
        the decoded copy fits: at 1024 x 2^20 int64, 105-110 ms against 20 ms, with 0.6 GiB of temporaries instead of
        12.6 GiB.  Uses the resident store and its
        decode index after to_device(), and uploads the store otherwise.  Argument errors raise ValueError before any GPU
        work."""
        from .libflacarray import _reduce_args, wrap_int32_to_float32

        st = self._st
        first, last, _, _, idx = _reduce_args(st.count, st.samples, None, first, last, streams)
        rows = st.count if idx is None else int(idx.size)
        lead = tuple(st.lead) if idx is None else (rows,)
        if not isinstance(quantised, (bool, np.bool_)):
            raise ValueError("quantised should be True or False")
        lo_i, hi_i, inside, max_hits = self._find_limits(lo, hi, rows, idx, inside, max_hits, bool(quantised))
        if rows == 0:
            z = np.zeros(0, dtype=np.int64)
            return StreamHits(np.zeros(lead, dtype=np.int64), np.zeros(1, dtype=np.int64), z, z.copy(), np.zeros(0, dtype=st.dtype), z.copy(),
                              first, last, idx)
        counts, pos, val = (t.cpu().numpy() for t in self._find_run(lo_i, hi_i, first, last, idx, inside, max_hits, False))
        offsets = np.zeros(rows + 1, dtype=np.int64)
        np.cumsum(counts, out=offsets[1:])
        hit_rows = np.repeat(np.arange(rows, dtype=np.int64), counts)
        if st.offsets is not None:
            pick = (lambda a: np.asarray(a).reshape(-1)) if idx is None else (lambda a: np.asarray(a).reshape(-1)[idx])  # noqa: E731
            it = np.int64 if st.wide else np.int32
            if val.size:
                values = np.asarray(wrap_int32_to_float32(val.astype(it), val.size, 1, pick(st.offsets)[hit_rows], pick(st.gains)[hit_rows],
                                                          _f64=st.wide)).astype(st.dtype, copy=False)
            else:
                values = np.zeros(0, dtype=st.dtype)
        else:
            values = val.astype(st.dtype)
        return StreamHits(counts.reshape(lead), offsets, hit_rows, pos, values, val, first, last, idx)

    def find_counts(self, lo=None, hi=None, first=0, last=None, streams=None, inside=False, quantised=False):
        """The number of hits per row of FlacArray.find, from its count pass alone: int64 of shape leading_shape, or
        (len(streams),) when streams were named.  Measured (profiles/find.md): 6.3-6.5 ms at 4096 x 2^20 int32, where
        the bare decode takes 6.35 ms and reduce with one bin 7.2; 53 ms at 1024 x 2^20 int64, a chunked decode as
        reduce's."""
        from .libflacarray import _reduce_args

        st = self._st
        first, last, _, _, idx = _reduce_args(st.count, st.samples, None, first, last, streams)
        rows = st.count if idx is None else int(idx.size)
        lead = tuple(st.lead) if idx is None else (rows,)
        if not isinstance(quantised, (bool, np.bool_)):
            raise ValueError("quantised should be True or False")
        lo_i, hi_i, inside, _ = self._find_limits(lo, hi, rows, idx, inside, None, bool(quantised))
        if rows == 0:
            return np.zeros(lead, dtype=np.int64)
        return self._find_run(lo_i, hi_i, first, last, idx, inside, None, True)[0].cpu().numpy().reshape(lead)

    def _frame_index_layout(self):
        """The layout test of the host copy: (blob, starts, nbytes, block sizes, own) as flat numpy arrays, `own` True when
        every stream is "fLaC", STREAMINFO (not last), then the SEEKTABLE (last) of one point per frame; None (and no
        block sizes) when the stream index does not fit the compressed bytes."""
        st = self._st
        blob = np.asarray(st.blob, dtype=np.uint8)
        s0 = np.asarray(st.starts, dtype=np.int64).reshape(-1)
        nb = np.asarray(st.nbytes_per_stream, dtype=np.int64).reshape(-1)
        if np.any(nb < 46) or np.any(s0 < 0) or np.any(s0 + nb > blob.size):
            return blob, s0, nb, None, None
        at = lambda k: blob[s0 + k].astype(np.int64)  # noqa: E731
        bs = (at(8) << 8) | at(9)
        stl = (at(43) << 16) | (at(44) << 8) | at(45)
        own = not (np.any(at(4) != 0) or np.any(at(42) != 0x83) or np.any(stl != 18 * (-(-st.samples // np.maximum(bs, 1)))))
        return blob, s0, nb, bs, own

    @property
    def has_frame_index(self):
        """True when every stream has this library's layout (STREAMINFO, then a SEEKTABLE of one point per frame), which
        append, overwrite, frame_status and salvage need; False for a store libFLAC wrote (reindex() adopts it).  Host
        only: read from the stream headers of the host copy, at whatever level the store was written."""
        return bool(self._frame_index_layout()[4])

    def reindex(self, verify=True):
        """Adopt a store written by stock flacarray / libFLAC, in place; returns self (addition to the reference API).

        Every stream is copied on the device into this library's layout (reindex_flac_device): its STREAMINFO verbatim (a
        signed stream stays signed, `md5` does not change), a SEEKTABLE of one point per frame, its frames verbatim.  No
        sample is decoded or re-encoded, so every value the array decodes to, and `stream_offsets`, `stream_gains`,
        `shape` and `dtype`, stay what they were; `compressed`, `stream_starts` and `stream_nbytes` change.  After it
        `has_frame_index` is True: append and overwrite work (at the level whose block size the streams have),
        frame_status, salvage and damaged_ranges locate the frames, and decodes no longer scan for them.  Every other
        metadata block of the source (VORBIS_COMMENT, APPLICATION, PADDING, a sparse SEEKTABLE) is dropped.  A store that
        already has the layout comes out byte-identical.

        `verify=True`: frame_status of the RESULT must be all zero, else RuntimeError and the array stays as it was -- a
        damaged source frame or a false sync code cannot slip into the index silently.  `verify=False` adopts the store
        as it is: the way to salvage() a damaged libFLAC-written store (except damage to the header of a stream's last
        frame, which is refused as a wrong stream size is: that header ties the stream size to the store).  Streams that differ in block size raise
        ValueError; what the decoders cannot index (variable block sizes, broken headers) raises RuntimeError.

        The store is replaced, not changed: a FlacArray(self) copy made before still holds the old one.  A resident
        array (to_device / from_device_array) stays resident, with an exact-size blob, and its decode index is rebuilt
        on next use; any other array uploads its store, reindexes it and brings the result back.  A store assembled by
        `dist` (global shape other than the local one) raises NotImplementedError."""
        from .libflacarray import reindex_flac_device

        st = self._st
        if st.global_shape != st.grid:
            raise NotImplementedError("reindex is not supported for a store that is one part of a distributed array")
        res = self._resident
        _, comp, starts, nbytes = self._device_store()
        comp2, starts2, nbytes2 = reindex_flac_device(comp, starts, nbytes, st.samples, is_int64=st.wide, verify=verify, compact=res is not None)
        ishape = np.shape(st.starts)
        new = _Store.build(st.shape, None, st.dtype, comp2.cpu().numpy(), starts2.cpu().numpy().reshape(ishape),
                           nbytes2.cpu().numpy().reshape(ishape), st.offsets, st.gains, st.dist)
        if res is not None:
            if res.get("index") is not None:
                res["index"].close()
            self._resident = dict(res, compressed=comp2, starts=starts2.reshape(-1), nbytes=nbytes2.reshape(-1), index=None)
        self._st = new
        return self

    def _splice_layout(self, level, what):
        """The layout a splice (append, overwrite) needs, checked on the host copy: STREAMINFO with the block size of
        `level`, then the SEEKTABLE (last) of one point per frame.  Returns (blob, starts, nbytes) as flat numpy arrays."""
        B = 1152 if level <= 2 else 4096
        blob, s0, nb, bs, own = self._frame_index_layout()
        if own is None:
            raise ValueError("the store's stream index does not fit its compressed bytes")
        if not own:
            raise ValueError(f"{what} needs streams written by this library (a SEEKTABLE with one point per frame); "
                             "libFLAC-written streams are not supported")
        if np.any(bs != B):
            raise ValueError(f"level {level} has block size {B}, the store's streams have {int(bs[bs != B][0])}: {what} at the store's level")
        return blob, s0, nb

    def append(self, data, level=5, verify=None, md5=False):
        """Extend every stream by data.shape[-1] samples, in place; returns self (addition to the reference API).

        `data`: a numpy array or a torch tensor on the device, of shape leading_shape + (n,) ((n,) for a 1-D array) and
        of this array's dtype; n == 0 does nothing.  Integer arrays: after any sequence of appends the store (every byte
        of `compressed`, `stream_starts`, `stream_nbytes`) is the one from_array(concatenation, level=level) writes, for
        any split into chunks -- provided `level` is the level the store was written at (the store does not record it;
        a level of another block size raises ValueError).  Float arrays: the new samples are quantised with the store's
        own `stream_offsets` and `stream_gains`, which do not change (a NaN raises RuntimeError, out-of-range values
        become INT_MIN as in float_to_int): the store is the integer encode of the old integers followed by these, NOT
        from_array of the concatenated floats, whose offsets and gains would differ.  Hence no `quanta` / `precision`.

        The old short last frame of every stream is decoded, encoded again with the new samples, and spliced in behind
        the kept old frames on the device (append_flac_device); each append copies the whole compressed blob once.  A
        resident array (to_device / from_device_array) stays resident, with an exact-size copy of the new blob, and its
        decode index is rebuilt on next use; any other array uploads its store, appends on the device and brings the
        result back.  Either way the new blob is also copied to the host mirror that answers `compressed`: at GB sizes
        that PCIe transfer (and, for a host array, the upload) costs more than the device work.  The store is replaced, not
        changed: a FlacArray(self) copy made before still holds the old one.  `verify`: decode the re-encoded span and
        compare it with its input on the device before returning (None = the default of set_encode_verify).  Streams
        without this library's SEEKTABLE (libFLAC-written) raise ValueError -- reindex() adopts such a store first; a
        store assembled by `dist` (global shape other than the local one) raises NotImplementedError.

        The splice writes a fresh stream header, so the appended store comes out UNSIGNED (`md5` all zero) even if the
        old one was signed: a finished digest cannot be resumed.  `md5=True` is append followed by sign(): correct, at the
        cost of one decode of the whole store; explicit only (it does not follow set_encode_md5)."""
        import torch

        from .libflacarray import append_flac_device

        st = self._st
        if st.global_shape != st.grid:
            raise NotImplementedError("append is not supported for a store that is one part of a distributed array")
        is_tensor = isinstance(data, torch.Tensor)
        dt = np.dtype(str(data.dtype).replace("torch.", "")) if is_tensor else np.asarray(data).dtype
        if dt != st.dtype:
            raise ValueError(f"data of dtype {dt} does not match the array's dtype {st.dtype}")
        shape = tuple(int(k) for k in data.shape)
        if len(shape) != len(st.shape) or shape[:-1] != tuple(st.shape[:-1]):
            raise ValueError(f"data of shape {shape} does not match the array's leading shape {tuple(st.shape[:-1])}")
        if level < 0 or level > 8:
            raise ValueError("FLAC only supports compression levels 0-8")
        n = shape[-1]
        if n == 0:
            return self.sign() if md5 else self
        self._splice_layout(level, "append")
        self._splice_on_device(lambda *store, **kw: append_flac_device(*store, level=level, **kw), data, st.count,
                               tuple(st.shape[:-1]) + (st.samples + n,), verify)
        return self.sign() if md5 else self

    def overwrite(self, first, data, streams=None, level=5, verify=None, md5=False):
        """Replace samples [first, first + n) of every stream, or of the streams named, in place; returns self (addition
        to the reference API; `__setitem__` keeps raising).

        `data`: a numpy array or a torch tensor on the device, of this array's dtype.  `streams=None`: shape
        leading_shape + (n,) ((n,) for a 1-D array).  Otherwise `streams` is a 1-D integer array of flat C-order stream
        indices and `data` is (len(streams), n), row j for stream streams[j]; an index out of range or named twice raises
        ValueError and an empty `streams` does nothing.  0 <= first and first + n <= stream_size are required (ValueError:
        growing the store is append's job); n == 0 does nothing.  Integer arrays: with y the decoded array after
        y[streams, first:first+n] = data, the store (every byte of `compressed`, `stream_starts`, `stream_nbytes`) is the
        one from_array(y, level=level) writes, after any sequence of overwrites and appends -- provided `level` is the
        level the store was written at (a level of another block size raises ValueError).  Float arrays: the new samples
        are quantised with the store's own `stream_offsets` and `stream_gains`, which do not change (a NaN raises
        RuntimeError, out-of-range values become INT_MIN): the store is the integer encode of the patched integers.

        Only the frames that overlap the range are decoded, patched and encoded again; the frames in front of them are
        copied verbatim, the frames behind them verbatim at their new place, with their seek points moved
        (overwrite_flac_device); each call copies the whole compressed blob once.  Residency follows append: a resident
        array stays resident, with an exact-size copy of the new blob and its decode index rebuilt on next use; any other
        array uploads its store, patches it on the device and brings the result back.  The store is replaced, not
        changed: a FlacArray(self) copy made before still holds the old one.  `verify`: decode the re-encoded span and
        compare it with its input on the device before returning (None = the default of set_encode_verify).  Streams
        without this library's SEEKTABLE (libFLAC-written) raise ValueError -- reindex() adopts such a store first; a
        store assembled by `dist` raises NotImplementedError.

        A stream that takes part comes out UNSIGNED (its STREAMINFO MD5 zeroed: its samples changed); a stream that does
        not keeps its header, and so a valid signature, verbatim.  `md5=True` is overwrite followed by sign()."""
        import torch

        from .libflacarray import _stream_indices, overwrite_flac_device

        st = self._st
        if st.global_shape != st.grid:
            raise NotImplementedError("overwrite is not supported for a store that is one part of a distributed array")
        is_tensor = isinstance(data, torch.Tensor)
        dt = np.dtype(str(data.dtype).replace("torch.", "")) if is_tensor else np.asarray(data).dtype
        if dt != st.dtype:
            raise ValueError(f"data of dtype {dt} does not match the array's dtype {st.dtype}")
        shape = tuple(int(k) for k in data.shape)
        idx = None
        if streams is None:
            if len(shape) != len(st.shape) or shape[:-1] != tuple(st.shape[:-1]):
                raise ValueError(f"data of shape {shape} does not match the array's leading shape {tuple(st.shape[:-1])}")
        else:
            idx = _stream_indices(streams, st.count)
            if len(shape) != 2 or shape[0] != idx.size:
                raise ValueError(f"data of shape {shape} does not match the shape ({idx.size}, n) of {idx.size} streams to overwrite")
        if level < 0 or level > 8:
            raise ValueError("FLAC only supports compression levels 0-8")
        n = shape[-1]
        first = int(first)
        if first < 0 or first + n > st.samples:
            raise ValueError(f"samples [{first}, {first + n}) do not lie inside streams of {st.samples} samples (append grows the store)")
        if n == 0 or (idx is not None and idx.size == 0):
            return self.sign() if md5 else self
        self._splice_layout(level, "overwrite")
        self._splice_on_device(lambda *store, **kw: overwrite_flac_device(*store, first, streams=idx, level=level, **kw), data,
                               st.count if idx is None else idx.size, tuple(st.shape), verify)
        return self.sign() if md5 else self

    def _splice_on_device(self, call, data, rows, new_shape, verify):
        """What append and overwrite do once their arguments are checked: `call(compressed, starts, nbytes, stream_size,
        data=..., offsets=..., gains=..., verify=..., compact=...)` on the resident store or an upload, with `data` as a
        (rows, n) tensor on that device; the result becomes the store (of shape `new_shape`) and, for a resident array, the
        resident store, whose decode index is rebuilt on next use."""
        import torch

        from .libflacarray import _encode_verify_default

        st = self._st
        if verify is None:
            verify = _encode_verify_default()
        res = self._resident
        dev, comp, starts, nbytes, off, gain = self._device_store(scale=True)
        x = data.to(dev) if isinstance(data, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(data)).to(dev)
        x = x.reshape(rows, -1).contiguous()
        # (a resident store keeps an exact-size blob, as from_device_array does; a host store only copies the bytes back)
        comp2, starts2, nbytes2 = call(comp, starts, nbytes, st.samples, data=x, offsets=off, gains=gain, verify=verify, compact=res is not None)
        ishape = np.shape(st.starts)
        new = _Store.build(new_shape, None, st.dtype, comp2.cpu().numpy(), starts2.cpu().numpy().reshape(ishape),
                           nbytes2.cpu().numpy().reshape(ishape), st.offsets, st.gains, st.dist)
        if res is not None:
            if res.get("index") is not None:
                res["index"].close()
            self._resident = dict(res, compressed=comp2, starts=starts2.reshape(-1), nbytes=nbytes2.reshape(-1), index=None)
        self._st = new

    def _window_on_device(self, first, last, streams, level, verify, what):
        """What window and trim share: the argument and layout checks, then window_flac_device on the resident store or
        an upload.  Returns (new _Store, its resident dict or None)."""
        from .libflacarray import _encode_verify_default, _window_args, window_flac_device

        st = self._st
        if st.global_shape != st.grid:
            raise NotImplementedError(f"{what} is not supported for a store that is one part of a distributed array")
        first, last, B, idx = _window_args(st.count, st.samples, first, last, streams, level)
        n = last - first
        pick = lambda a: a if (a is None or idx is None) else np.asarray(a).reshape(-1)[idx]  # noqa: E731
        new_shape = (tuple(st.shape[:-1]) + (n,)) if idx is None else (int(idx.size), n)
        if idx is not None and idx.size == 0:
            empty = np.zeros(0, dtype=np.int64)
            return _Store.build(new_shape, None, st.dtype, np.zeros(0, dtype=np.uint8), empty, empty.copy(), pick(st.offsets), pick(st.gains)), None
        _, _, _, bs, own = self._frame_index_layout()
        if own is None:
            raise ValueError("the store's stream index does not fit its compressed bytes")
        if not own:
            raise ValueError(f"{what} needs streams written by this library (a SEEKTABLE with one point per frame): reindex() adopts a "
                             "libFLAC-written store first")
        if np.any(bs != B):
            raise ValueError(f"level {level} has block size {B}, the store's streams have {int(bs[bs != B][0])}: {what} at the store's level")
        if verify is None:
            verify = _encode_verify_default()
        res = self._resident
        _, comp, starts, nbytes = self._device_store()
        # (a resident result keeps an exact-size blob, as append does; a host result only copies the bytes back)
        comp2, starts2, nbytes2 = window_flac_device(comp, starts, nbytes, st.samples, first, last, streams=idx, level=level, is_int64=st.wide,
                                                     verify=verify, compact=res is not None)
        ishape = np.shape(st.starts) if idx is None else (int(idx.size),)
        new = _Store.build(new_shape, None, st.dtype, comp2.cpu().numpy(), starts2.cpu().numpy().reshape(ishape),
                           nbytes2.cpu().numpy().reshape(ishape), pick(st.offsets), pick(st.gains), st.dist)
        if res is None:
            return new, None
        import torch

        sel = lambda t: t if (t is None or idx is None) else t[torch.from_numpy(idx).to(t.device)]  # noqa: E731
        return new, dict(res, compressed=comp2, starts=starts2.reshape(-1), nbytes=nbytes2.reshape(-1), offsets=sel(res["offsets"]),
                         gains=sel(res["gains"]), index=None)

    def window(self, first=0, last=None, streams=None, level=5, verify=None, md5=False):
        """Samples [first, last) of every stream, or of the streams named, as a NEW FlacArray -- a compressed store, not a
        decoded array (addition to the reference API).  This array is not modified.

        `streams=None`: the result has shape leading_shape + (last - first,) (a 1-D array stays 1-D).  Otherwise `streams`
        is a 1-D integer array of flat C-order stream indices (an index out of range or named twice raises ValueError)
        and the result has shape (len(streams), last - first), rows in the order asked; an empty `streams` gives an empty
        store of shape (0, last - first).  `stream_offsets` / `stream_gains` are those of the picked streams, unchanged.
        0 <= first < last <= stream_size, else ValueError (an empty window is refused: there is no zero-sample stream).

        Integer arrays: the result is byte for byte from_array(x[idx, first:last], level=level) with x the decoded array
        -- `compressed`, `stream_starts` and `stream_nbytes` -- after any sequence of append, overwrite, trim and window,
        provided `level` is the level the store was written at (a level of another block size raises ValueError).  Float
        arrays: the integer encode of the quantised integers of the window; the decoded floats equal
        to_array()[idx, first:last] bit for bit.

        When `first` is a multiple of the block size (4096 samples at levels 3-8, 1152 at 0-2) no kept frame is decoded:
        the frames are copied with their numbers lowered and the seek table rebuilt on the device, and only a `last` that
        falls inside a frame has that one frame decoded and encoded again (window_flac_device).  Any other `first` moves
        every frame boundary and COSTS A DECODE PLUS AN ENCODE of the window, done in row chunks of bounded memory.

        A stream whose window is the whole stream is copied verbatim (pure stream selection: a signed stream keeps its
        signature); every other stream comes out UNSIGNED, and `md5=True` is the call followed by sign().  `verify`:
        frame_status of the result must be all zero and the re-encoded last frame must decode to the old samples, else
        RuntimeError (None = the default of set_encode_verify).  The result is resident when this array is (an
        exact-size blob), a host store otherwise.  Streams without this library's SEEKTABLE raise ValueError -- reindex()
        adopts such a store first; a store assembled by `dist` raises NotImplementedError; a seek table whose offsets
        are out of order raises RuntimeError."""
        st = self._st
        new, res = self._window_on_device(first, last, streams, level, verify, "window")
        out = FlacArray._assemble(new.shape, None, st.dtype, new.blob, new.starts, new.nbytes_per_stream, new.offsets, new.gains)
        out._resident = res
        return out.sign() if (md5 and new.count) else out

    def trim(self, first=0, last=None, level=5, verify=None, md5=False):
        """Keep samples [first, last) of every stream, in place; returns self (addition to the reference API): what
        window(first, last) returns becomes this array's store -- "keep the last hour" of an array fed by append, without a
        decoded copy and, for a `first` on a frame boundary, without an encode.  Contract, cost, signatures and errors are
        window's.  The store is replaced, not changed: a FlacArray(self) copy made before still holds the old one.  A
        resident array stays resident, with an exact-size blob, and its decode index is closed and rebuilt on next use."""
        new, res = self._window_on_device(first, last, None, level, verify, "trim")
        old = self._resident
        if old is not None and old.get("index") is not None:
            old["index"].close()
        if old is not None:
            self._resident = res
        self._st = new
        return self.sign() if md5 else self

    @classmethod
    def _stack(cls, arrays, md5):
        """concatenate(axis=0): the parts' streams verbatim in order, stream_starts shifted by the bytes in front."""
        st0 = arrays[0]._st
        if len(st0.shape) < 2:
            raise ValueError("a 1-D array has the sample axis only: concatenate it with axis=-1")
        for a in arrays:
            st = a._st
            if st.global_shape != st.grid:
                raise NotImplementedError("concatenate is not supported for a store that is one part of a distributed array")
            if st.dtype != st0.dtype:
                raise ValueError(f"the parts differ in dtype ({st.dtype} beside {st0.dtype})")
            if len(st.shape) != len(st0.shape) or st.shape[1:] != st0.shape[1:]:
                raise ValueError(f"axis 0 joins arrays of one stream_size and equal shape[1:], got {st.shape} beside {st0.shape}")
        sizes = [a._st.blob_bytes for a in arrays]
        fronts = np.cumsum([0] + sizes[:-1])
        lead = lambda a, v: np.asarray(v).reshape(a._st.lead)  # noqa: E731
        blob = np.concatenate([np.asarray(a._st.blob, dtype=np.uint8) for a in arrays])
        starts = np.concatenate([lead(a, a._st.starts).astype(np.int64) + int(f) for a, f in zip(arrays, fronts)], axis=0)
        nbytes = np.concatenate([lead(a, a._st.nbytes_per_stream).astype(np.int64) for a in arrays], axis=0)
        offsets = gains = None
        if st0.offsets is not None:
            offsets = np.concatenate([lead(a, a._st.offsets) for a in arrays], axis=0)
            gains = np.concatenate([lead(a, a._st.gains) for a in arrays], axis=0)
        shape = (sum(a._st.shape[0] for a in arrays),) + tuple(st0.shape[1:])
        out = cls._assemble(shape, None, st0.dtype, blob, starts, nbytes, offsets, gains)
        res0 = arrays[0]._resident
        if res0 is not None:
            import torch

            dev = res0["device"]
            parts = [a._device_store(scale=True) for a in arrays]  # (resident tensors, or an upload)
            cat = lambda k: torch.cat([p[k].to(dev) for p in parts])  # noqa: E731
            front = torch.from_numpy(np.asarray(fronts, dtype=np.int64)).to(dev)
            out._resident = {
                "device": dev, "compressed": cat(1), "starts": torch.cat([p[2].to(dev) + front[i] for i, p in enumerate(parts)]),
                "nbytes": cat(3), "offsets": None if offsets is None else cat(4), "gains": None if gains is None else cat(5),
            }
        return out.sign() if md5 else out

    @classmethod
    def concatenate(cls, arrays, axis=-1, level=5, verify=None, md5=False):
        """Join FlacArrays into a NEW FlacArray without re-encoding them (addition to the reference API).  No input is
        modified.

        `axis=-1`, the sample axis: all arrays have one dtype and one leading shape, lengths may differ, 1-D arrays stay
        1-D.  Integer arrays: with x_i the decoded arrays, `compressed`, `stream_starts` and `stream_nbytes` are byte for
        byte those of from_array(np.concatenate(x_i, axis=-1), level=level), for any number of parts and any lengths,
        after any sequence of append, overwrite, trim, window, concatenate and extend -- provided `level` is the level
        the stores were written at (a block size other than that of `level` in any part raises ValueError).  Float
        arrays: `stream_offsets` and `stream_gains` of all parts must be equal bit for bit, else ValueError (the parts
        were quantised differently: decode them and compress the concatenation again); the result is the integer encode
        of the concatenated quantised integers, its decoded floats are np.concatenate of the parts' to_array() bit for
        bit, and offsets and gains carry over unchanged.  Nothing is re-quantised, hence no `quanta` / `precision`.

        When every part but the last is a whole number of blocks long (4096 samples at levels 3-8, 1152 at 0-2) no
        sample is decoded and nothing is encoded: the frames are copied with their numbers raised and the seek table is
        rebuilt on the device (join_flac_device), and the first part moves at copy speed.  Any other split COSTS A DECODE
        PLUS AN ENCODE of everything behind the first unaligned boundary, done in row chunks of bounded memory, AND IS
        SLOWER than decoding those parts and appending them in one go (profiles/join.md).

        A single part is returned as a verbatim copy, signature included.  Any result made from two or more parts
        comes out UNSIGNED (STREAMINFO MD5 zero): a finished digest cannot be resumed; `md5=True` is the call followed
        by sign(), explicit only.  `verify` (None = the default of set_encode_verify): frame_status of the RESULT must be
        all zero -- every frame carries its new number, its block size, a clean CRC-8 and a clean CRC-16 -- else
        RuntimeError; on the unaligned route the appended span is also verified as append(verify=True) does.

        The result is resident when arrays[0] is (an exact-size blob), a host store otherwise; parts that are not
        resident are uploaded for the call, and the host mirror is filled as append fills it.  Every part must have this
        library's layout (`has_frame_index`), else ValueError -- reindex() adopts such a store first; a part of a `dist`
        store raises NotImplementedError; an empty `arrays` raises ValueError.

        `axis=0`, the first leading axis: the arrays have one dtype, one stream_size and equal shape[1:] (1-D arrays
        raise ValueError: their only axis is the sample axis).  The streams are copied verbatim in order, with
        `stream_starts` shifted by the bytes in front; offsets and gains are concatenated.  Every stream keeps its bytes
        and therefore its signature, and layouts may differ between parts, since nothing is parsed.  `level` and `verify`
        are ignored; `md5=True` signs afterwards."""
        from .libflacarray import _encode_verify_default, _join_args, join_flac_device

        arrays = list(arrays)
        if not arrays:
            raise ValueError("concatenate needs at least one array")
        if not all(isinstance(a, FlacArray) for a in arrays):
            raise ValueError("concatenate takes FlacArrays (append takes raw samples)")
        st0 = arrays[0]._st
        nd = len(st0.shape)
        if isinstance(axis, bool) or not isinstance(axis, (int, np.integer)):
            raise ValueError(f"axis {axis!r} is not an integer")
        if axis == 0 and nd == 1:
            raise ValueError("a 1-D array has the sample axis only: concatenate it with axis=-1")
        if axis == 0 or (axis == -nd and nd > 1):
            return cls._stack(arrays, md5)
        if axis not in (-1, nd - 1):
            raise ValueError(f"axis {axis} is neither the sample axis (-1) nor the first leading axis (0)")
        for a in arrays:
            st = a._st
            if st.global_shape != st.grid:
                raise NotImplementedError("concatenate is not supported for a store that is one part of a distributed array")
            if st.dtype != st0.dtype:
                raise ValueError(f"the parts differ in dtype ({st.dtype} beside {st0.dtype})")
            if len(st.shape) != nd or st.shape[:-1] != st0.shape[:-1]:
                raise ValueError(f"the parts differ in leading shape ({st.shape[:-1]} beside {st0.shape[:-1]})")
        B, sizes, _ = _join_args([a._st.count for a in arrays], [a._st.samples for a in arrays], level)
        if st0.offsets is not None:
            ft = np.float64 if st0.wide else np.float32
            bits = lambda v: np.ascontiguousarray(v, dtype=ft).tobytes()  # noqa: E731
            if any(bits(a._st.offsets) != bits(st0.offsets) or bits(a._st.gains) != bits(st0.gains) for a in arrays[1:]):
                raise ValueError("the parts were quantised differently (their stream_offsets / stream_gains are not equal bit for bit): "
                                 "decode them and compress the concatenation again")
        for a in arrays:
            _, _, _, bs, own = a._frame_index_layout()
            if own is None:
                raise ValueError("a part's stream index does not fit its compressed bytes")
            if not own:
                raise ValueError("concatenate needs streams written by this library (a SEEKTABLE with one point per frame): reindex() adopts "
                                 "a libFLAC-written store first")
            if np.any(bs != B):
                raise ValueError(f"level {level} has block size {B}, a part's streams have {int(bs[bs != B][0])}: concatenate at the "
                                 "stores' level")
        if verify is None:
            verify = _encode_verify_default()
        import torch

        res0 = arrays[0]._resident
        dev = res0["device"] if res0 is not None else torch.device("cuda", torch.cuda.current_device())
        stores = []
        for a in arrays:
            _, comp, starts, nbytes = a._device_store()
            stores.append((comp.to(dev), starts.to(dev), nbytes.to(dev), a._st.samples))
        # (a resident result keeps an exact-size blob, as append does; a host result only copies the bytes back)
        comp2, starts2, nbytes2 = join_flac_device(stores, level=level, is_int64=st0.wide, verify=verify, compact=res0 is not None)
        ishape = np.shape(st0.starts)
        out = cls._assemble(tuple(st0.shape[:-1]) + (sum(sizes),), None, st0.dtype, comp2.cpu().numpy(), starts2.cpu().numpy().reshape(ishape),
                            nbytes2.cpu().numpy().reshape(ishape), copy.deepcopy(st0.offsets), copy.deepcopy(st0.gains))
        if res0 is not None:
            out._resident = {"device": dev, "compressed": comp2, "starts": starts2.reshape(-1), "nbytes": nbytes2.reshape(-1),
                             "offsets": res0["offsets"], "gains": res0["gains"]}
        return out.sign() if md5 else out

    def extend(self, other, level=5, verify=None, md5=False):
        """Extend every stream by the samples of another FlacArray, in place; returns self (addition to the reference
        API): what concatenate([self, other], level=level) returns becomes this array's store -- append for data that
        arrives compressed; with trim, a rolling store whose new data is never decoded.  Contract, cost, signatures and
        errors are those of concatenate on the sample axis; `other` is not modified.  The store is replaced, not changed:
        a FlacArray(self) copy made before still holds the old one.  The result is resident when this array is, with an
        exact-size blob; its decode index is closed and rebuilt on next use.  When `verify` fails RuntimeError is raised
        and both arrays stay as they were."""
        new = FlacArray.concatenate([self, other], axis=-1, level=level, verify=verify, md5=md5)
        old = self._resident
        if old is not None and old.get("index") is not None:
            old["index"].close()
        self._resident = new._resident
        self._st = new._st
        return self

    def _device_store(self, scale=False):
        """(device, compressed, starts, nbytes) for a pass over the whole store: the resident tensors, or an upload.
        `scale`: followed by the offsets and gains (None for an integer store)."""
        import torch

        res = self._resident
        if res is not None:
            out = res["device"], res["compressed"], res["starts"], res["nbytes"]
            return out + (res["offsets"], res["gains"]) if scale else out
        dev = torch.device("cuda", torch.cuda.current_device())
        up = lambda a, dt: None if a is None else torch.from_numpy(np.ascontiguousarray(a, dtype=dt).reshape(-1)).to(dev)  # noqa: E731
        out = dev, up(self._compressed, np.uint8), up(self._stream_starts, np.int64), up(self._stream_nbytes, np.int64)
        ft = np.float64 if self._is_int64 else np.float32
        return out + (up(self._stream_offsets, ft), up(self._stream_gains, ft)) if scale else out

    # ---- damage map and decode through errors (addition to the reference API) ----
    def _block_size(self):
        """The block size the store was written with: the most common one of its readable STREAMINFO blocks (host)."""
        from .scrub import store_block_size

        return store_block_size(self._compressed, self._stream_starts, self._stream_nbytes)

    def frame_status(self):
        """The damage map of the store as it is held: numpy uint8 of shape leading_shape + (nf,), one status per
        (stream, frame) -- 0 = decodable, FRAME_UNLOCATED, or FRAME_HEADER | FRAME_CRC16 bits (flacarray_amd.scrub).
        Computed on the device from the resident store (or an upload), never through the decode index, and never
        raises for damage.  As strong as CRC-16: check_md5() is the stronger check, per stream.  A libFLAC-written store
        has no seek point per frame, so all its frames are FRAME_UNLOCATED: reindex() adopts it first."""
        from .libflacarray import frame_status_device

        _, comp, st, nb, _, _ = self._device_store(scale=True)
        status = frame_status_device(comp, st, nb, self._stream_size, is_int64=self._is_int64, block_size=self._block_size())
        return status.cpu().numpy().reshape(tuple(self._leading_shape) + (-1,))

    def salvage(self, stream_slice=None, fill=None):
        """Decode through errors: (array, status).  `array` is shaped as to_array(stream_slice=...) shapes it (same
        step-1 slice rules): every frame whose status is 0 decoded exactly, the samples of every other frame set to
        `fill` (None: 0 for an integer store, NaN for a float store); `status` is frame_status() of the whole store.
        A libFLAC-written store is all FRAME_UNLOCATED, hence all fill: reindex(verify=False) adopts it first."""
        from .libflacarray import decode_flac_salvage_device

        lo, hi = -1, -1
        if stream_slice is not None:
            if stream_slice.step not in (None, 1):
                raise RuntimeError("Only stream slices with a step size of 1 are supported")
            lo, hi = stream_slice.indices(self._stream_size)[:2]
            if hi <= lo:
                raise RuntimeError("first_sample is larger than last_sample")
        _, comp, st, nb, off, gain = self._device_store(scale=True)
        out, status = decode_flac_salvage_device(comp, st, nb, self._stream_size, lo, hi, offsets=off, gains=gain, is_int64=self._is_int64,
                                                 fill=fill, block_size=self._block_size())
        arr = out.cpu().numpy()
        arr = arr.reshape(-1) if self._flatten_single else arr.reshape(self._shape[:-1] + (arr.shape[-1],))
        return arr, status.cpu().numpy().reshape(tuple(self._leading_shape) + (-1,))

    def damaged_ranges(self, status=None):
        """The sample ranges `status` (default: frame_status()) fences off: int64 [k, 3], rows (flat stream, first,
        last) with `last` exclusive, adjacent damaged frames of a stream merged, sorted by (stream, first).  With a
        status given this is a pure host function."""
        from .scrub import damaged_ranges

        if status is None:
            status = self.frame_status()
        return damaged_ranges(status, self._block_size(), self._stream_size)

    @property
    def md5(self):
        """The STREAMINFO MD5 signature of every stream as stored: uint8, leading shape + (16,); all zero = unsigned."""
        return stream_md5(np.asarray(self._compressed, dtype=np.uint8), self._stream_starts)

    def check_md5(self, verify=None):
        """Check the store against the MD5 signatures in its streams, with nothing but the store at hand: an int8 numpy
        array over the leading shape, 1 = the stream decodes to the samples that were signed, 0 = it does not, -1 =
        unsigned, -2 = not checkable (not 32 bits per sample; see check_md5_device).  The store is decoded in column
        chunks on the device and hashed there; uses the resident store after to_device(), uploads it otherwise.
        `verify`: the decoder's frame CRC-16 check (None = the default of set_decode_verify)."""
        from .libflacarray import check_md5_device

        _, comp, st, nb = self._device_store()
        status = check_md5_device(comp, st, nb, self._stream_size, is_int64=self._is_int64, verify=verify)
        return status.cpu().numpy().reshape(self._leading_shape)

    def sign(self):
        """Compute the MD5 signature of what every stream decodes to (the chunked decode-and-hash pass of check_md5) and
        write it into the streams' STREAMINFO; returns self.  For a float store that is the quantised integers, as any
        FLAC decoder produces them.  The store is replaced, not changed: a FlacArray(self) copy made before keeps the
        bytes it had.  A resident store is signed on the device and only the sixteen bytes per stream travel to the host
        mirror.  Streams that are not checkable (check_md5's -2) raise ValueError."""
        from .libflacarray import check_md5_device, sign_streams_device

        st = self._st
        _, comp, starts, nbytes = self._device_store()
        status, digests = check_md5_device(comp, starts, nbytes, st.samples, is_int64=st.wide, return_digests=True)
        if bool((status == -2).any()):
            raise ValueError("sign needs streams of 32 bits per sample with the channel count of the array's dtype")
        blob = np.array(st.blob, dtype=np.uint8, copy=True)
        s0 = np.asarray(st.starts, dtype=np.int64).reshape(-1)
        blob[s0[:, None] + 26 + np.arange(16)[None, :]] = digests.cpu().numpy().reshape(-1, 16)
        res = self._resident
        if res is not None:
            signed = sign_streams_device(comp.clone(), starts, digests)
            if res.get("index") is not None:
                res["index"].close()
            self._resident = dict(res, compressed=signed, index=None)
        self._st = _Store.build(st.shape, st.global_shape, st.dtype, blob, st.starts, st.nbytes_per_stream, st.offsets, st.gains, st.dist)
        return self

    @classmethod
    def from_device_array(cls, data, level=5, quanta=None, precision=None, verify=None, md5=None):
        """Construct a RESIDENT FlacArray from a torch tensor that already lives in HBM (int32 / int64, or float32 /
        float64 with `quanta` or `precision` as array_compress takes them): quantise + encode on the device, keep the
        store there, and mirror it to host arrays so that every property of the reference API still answers with numpy.
        Same store as from_array on the tensor's host copy; with `precision` the per-stream std is computed on the
        device (std_device) and only its n_stream values reach the host.  Integer tensors ignore quanta / precision.
        `verify`: compare the store with `data` on the device before returning (see array_compress); None = the default
        of set_encode_verify.  `md5`: sign the streams (see array_compress); None = the default of set_encode_md5."""
        import torch

        from .compress import _per_stream_quanta
        from .libflacarray import _encode_verify_default, encode_flac_device, encode_flac_device_f32, encode_flac_device_f64
        from .utils import stream_quanta

        if verify is None:
            verify = _encode_verify_default()
        offsets = gains = None
        if data.dtype in (torch.float32, torch.float64):
            ndt = np.dtype(np.float32) if data.dtype == torch.float32 else np.dtype(np.float64)
            if quanta is None and precision is None:
                raise RuntimeError(f"Compressing floating point data ('{ndt}') requires specifying either quanta or precision.")
            if quanta is not None and precision is not None:
                raise RuntimeError("Cannot set both quanta and precision")
            encode = encode_flac_device_f32 if data.dtype == torch.float32 else encode_flac_device_f64
            q = None
            if quanta is not None:  # array_compress's checks and casts, on the host
                if isinstance(quanta, torch.Tensor):
                    quanta = quanta.item() if quanta.dim() == 0 else quanta.cpu().numpy()
                lead = tuple(data.shape[:-1])
                q = torch.from_numpy(stream_quanta(_per_stream_quanta(quanta, lead, ndt), lead, ndt)).to(data.device)
            comp, st, nb, offsets, gains = encode(data.contiguous(), q, level=level, compact=True, precision=precision, verify=verify, md5=md5)
        elif data.dtype in (torch.int32, torch.int64):
            comp, st, nb = encode_flac_device(data.contiguous(), level=level, compact=True, verify=verify, md5=md5)
        else:
            raise ValueError(f"Unsupported data type '{data.dtype}'")
        host = lambda t: None if t is None else t.cpu().numpy()  # noqa: E731
        out = cls._assemble(tuple(data.shape), None, np.dtype(str(data.dtype).replace("torch.", "")), host(comp), host(st), host(nb),
                            host(offsets), host(gains))
        out._resident = {
            "device": data.device, "compressed": comp, "starts": st.reshape(-1), "nbytes": nb.reshape(-1),
            "offsets": None if offsets is None else offsets.reshape(-1), "gains": None if gains is None else gains.reshape(-1),
        }
        return out

    @classmethod
    def from_array(cls, arr, level=5, quanta=None, precision=None, mpi_comm=None, use_threads=False, verify=None, md5=None):
        """Construct a FlacArray from a numpy ndarray (array.py:587-637).  `verify`, `md5`: see array_compress."""
        if mpi_comm is not None:
            raise NotImplementedError("mpi4py communicators are not supported; see flacarray_amd.dist")
        pieces = array_compress(arr, level=level, quanta=quanta, precision=precision, use_threads=use_threads, verify=verify, md5=md5)
        return cls._assemble(arr.shape, None, arr.dtype, *pieces)

    @classmethod
    def _assemble(cls, shape, global_shape, dtype, blob, starts, nbytes, offsets, gains):
        """A FlacArray around an existing (bytes, starts, nbytes, offsets, gains) store; without a global shape the
        array is the whole array (global_array_properties, mpi.py:109-117: a 1-D array counts as one stream)."""
        shape = tuple(shape)
        if global_shape is None:
            global_shape = (1,) + shape if len(shape) == 1 else shape
        return cls(None, shape=shape, global_shape=global_shape, compressed=blob, dtype=dtype, stream_starts=starts,
                   stream_nbytes=nbytes, stream_offsets=offsets, stream_gains=gains)

    def write_hdf5(self, hgrp):
        """Write the compressed representation to an open HDF5 group (array.py:639-682), format
        version 1 (flacarray_amd/hdf5.py)."""
        from .hdf5 import write_compressed

        st = self._st
        write_compressed(hgrp, st.lead, st.glead, st.samples, st.starts, st.starts, st.nbytes_per_stream, st.offsets, st.gains,
                         st.blob, 2 if st.wide else 1)

    @classmethod
    def read_hdf5(cls, hgrp, keep=None, mpi_comm=None, mpi_dist=None, no_flatten=False):
        """Construct a FlacArray from an HDF5 group (array.py:684-764).  With `keep` the array
        holds only the selected streams, as a 2-D (n_kept, stream_size) array."""
        from .hdf5 import read_compressed
        from .utils import compressed_dtype

        got = read_compressed(hgrp, keep=keep, mpi_comm=mpi_comm, mpi_dist=mpi_dist)
        local, whole, blob, n_channels, starts, nbytes, offsets, gains = got[:8]
        if len(local) == 2 and local[0] == 1 and not no_flatten:
            local = (local[1],)  # a single stream reads back as the 1-D array it was written from
        return cls._assemble(local, whole, compressed_dtype(n_channels, offsets, gains), blob, starts, nbytes, offsets, gains)

    def write_zarr(self, zgrp):
        """Write the compressed representation to an open Zarr group (array.py:766-804); same schema as HDF5."""
        self.write_hdf5(zgrp)

    @classmethod
    def read_zarr(cls, zgrp, keep=None, mpi_comm=None, mpi_dist=None, no_flatten=False):
        """Construct a FlacArray from a Zarr group (array.py:806-884)."""
        return cls.read_hdf5(zgrp, keep=keep, mpi_comm=mpi_comm, mpi_dist=mpi_dist, no_flatten=no_flatten)


for _name, (_attr, _doc) in _ACCESSORS.items():
    setattr(FlacArray, _name, _store_reader(_attr, _doc))
del _name, _attr, _doc
