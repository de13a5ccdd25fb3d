"""tests/wide_corpus.py on the CPU: every geometry crosses the threshold it names (the literals are quoted from
flacarray_amd/csrc/flacarray_hip.hip and read back from the source, so a changed literal fails here and not silently on
the GPU), its rows are pairwise distinct, the oracle's stream sizes are irregular, and the oracle round-trips it."""
import os
import re

import numpy as np
import pytest

from tests import wide_corpus as WC

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "flacarray_amd", "csrc")
CASES = [(name, shape, dt, level) for name, g in WC.GEOMETRIES.items() for shape, dt, level in g["cases"]]
IDS = ["%s-%dx%d-%s-l%d" % (name, shape[0], shape[1], dt, level) for name, shape, dt, level in CASES]
TAILCAP_ROWS = 64


def _src(name):
    with open(os.path.join(CSRC, name)) as f:
        return f.read()


def test_literals_are_the_sources():
    """The thresholds of wide_corpus.py as the C++ spells them."""
    hip, placed, enc = _src("flacarray_hip.hip"), _src("encode_placed.hpp"), _src("encode_kernels.hpp")
    assert "#define FA_K5_MAXBLK %d" % WC.K5_MAXBLK in hip and "int64_t nblk = (fp.F + 3) / 4;" in hip
    assert "int64_t nblk = (n_stream + 3) / 4;" in hip and "if (nblk > %d) nblk = %d;" % (WC.K5_MAXBLK, WC.K5_MAXBLK) in hip
    assert "std::min<int64_t>(%d, (n_stream * n + %d) / %d)" % (WC.QUANT_MAXBLK, WC.QUANT_PER_BLOCK - 1, WC.QUANT_PER_BLOCK) in hip
    assert "(n_ranges < (int64_t)1 << 20 ? n_ranges : (int64_t)1 << 20)" in hip and WC.FILL_MAXGRID == 1 << 20
    assert "return n_tasks <= %d;" % WC.LATENCY_MAX_TASKS in hip
    assert "a.n_tasks >= %d" % WC.BESIDE_MIN_TASKS in hip
    assert "constexpr int64_t kPlacedBelowFrames = %d;" % WC.PLACED_BELOW in hip
    assert "(fp.tail_bs == kMaxBlock) ? kPlacedBelowFrames / 4 : kPlacedBelowFrames" in hip
    assert re.search(r"kPlacedGrid\s*=\s*%d\b" % WC.PLACED_GRID, placed)
    assert "__launch_bounds__(%d) void starts_scan_kernel" % WC.SCAN_THREADS in enc and "base += %d" % WC.SCAN_THREADS in enc
    assert "hipLaunchKernelGGL(starts_scan_kernel, dim3(1), dim3(%d)" % WC.SCAN_THREADS in hip


@pytest.mark.parametrize("name,shape,dt,level", CASES, ids=IDS)
def test_geometry_crosses_its_threshold(name, shape, dt, level):
    ns, n = shape
    B = WC.block_size(level)
    nf = -(-n // B)
    F = ns * nf
    assert ns < 1 << 19  # (sample 0 of a row is s: it has to stay clear of the noise's range only for the reader's sake)
    if name == "scan3":
        assert 2 * WC.SCAN_THREADS < ns < 3 * WC.SCAN_THREADS and ns % WC.SCAN_THREADS != 0  # two carries, a ragged third pass
        assert n in (37, 3 * B + 11) and F >= WC.PLACED_BELOW // 4
        assert (F <= WC.LATENCY_MAX_TASKS) == (n == 37)  # the short form goes to K7L, the long one (four frames a stream) to K7
        assert n % 4 != 0  # never K3F: the splice, window and join callers see K3G's stores
    elif name == "u16":
        assert ns > 65536 + 256 and ns % 256 != 0 and ns % 64 != 0 and F >= WC.BESIDE_MIN_TASKS and nf == 1
    elif name == "k5cap":
        assert nf == 1 and F > WC.K5_WAVES * WC.K5_MAXBLK and F < 2 * WC.K5_WAVES * WC.K5_MAXBLK and F % 4 != 0
        assert F > 32 * WC.PLACED_GRID and ns > (1 << 17) + 1
        assert level in (0, 5) and n < B  # one short frame per stream: K3G, never K3F
    elif name == "ones":
        assert n in (1, 4) and ns > 1 << 18
    elif name == "k3f_wide":
        assert n == 4096 and nf == 1 and level >= 3 and dt in ("i32", "f32")  # fused_geometry: whole mono frames of levels 3-8
        assert F >= WC.PLACED_BELOW // 4  # placed_preferred: whole frames go to K3F from 1024 frames on
        assert WC.BESIDE_MIN_TASKS <= F < WC.BESIDE_MIN_TASKS + 64 and F > WC.LATENCY_MAX_TASKS
    elif name == "k3f_tailcap":
        assert n % 4 == 0 and n >= 2 * 4096 and n % 4096 != 0 and level >= 3 and dt == "i32"  # fused_geometry with a tail
        assert F >= WC.PLACED_BELOW and (ns + 3) // 4 > WC.K5_MAXBLK and ns > (1 << 17) + 2
    elif name == "qcap":
        assert dt in ("f32", "f64") and ns * n > WC.QUANT_MAXBLK * WC.QUANT_PER_BLOCK and ns > 65536
        assert (ns * n + 1023) // 1024 < 2 * WC.QUANT_MAXBLK + 1024  # a second trip, not many
    else:
        raise AssertionError("a geometry without a threshold assertion: " + name)


def test_amplitude_cycle_is_coprime_to_the_index_widths():
    for m in (1024, 65536, 131072):
        assert np.gcd(WC.AMP_PERIOD, m) == 1 and np.gcd(WC.CONST_EVERY, m) == 1 and np.gcd(WC.FULL_EVERY, m) == 1


_made = {}


def _ints(oracle, shape, dt, seed=0, rows=None):
    """_make_ints, the last whole corpus kept (the cases of one shape and type follow each other)."""
    key = (shape, dt, seed)
    if rows is not None:
        return _make_ints(oracle, shape, dt, seed, rows)
    if key not in _made:
        _made.clear()
        _made[key] = _make_ints(oracle, shape, dt, seed, None)
    return _made[key]


def _make_ints(oracle, shape, dt, seed, rows):
    """(the integers a case encodes, its floats or None): the corpus, or for float cases the oracle's quantisation of the
    float corpus with the corpus' quanta."""
    ns, n = shape
    if dt in ("i32", "i64"):
        return WC.wide_rows(ns, n, dt == "i64", seed, rows=rows), None
    ndt = np.float32 if dt == "f32" else np.float64
    quant = oracle.float32_to_int32 if dt == "f32" else oracle.float64_to_int64
    f = WC.wide_floats(ns, n, ndt, seed)
    return quant(f, WC.wide_quanta(ns, ndt))[0], f


def _distinct_rows(x):
    x = np.ascontiguousarray(x)
    return np.unique(x.view(np.dtype((np.void, x.dtype.itemsize * x.shape[1])))).size


@pytest.mark.parametrize("name,shape,dt,level", CASES, ids=IDS)
def test_rows_sizes_and_oracle_round_trip(oracle, name, shape, dt, level):
    ns, n = shape
    wide = dt in ("i64", "f64")
    enc, dec = (oracle.encode_i64, oracle.decode_i64) if wide else (oracle.encode_i32, oracle.decode_i32)
    if name == "k3f_tailcap":  # 4.3 GB of input: its sampled rows only; sample 0 of row s is s, so all rows differ
        rows = np.unique(np.concatenate([WC.boundary_streams(ns), np.random.default_rng(5).integers(0, ns, TAILCAP_ROWS)]))[:TAILCAP_ROWS]
        x, f = _ints(oracle, shape, dt, rows=rows)
        assert np.array_equal(x[:, 0], rows)
    else:
        x, f = _ints(oracle, shape, dt)
        if dt in ("i32", "i64"):
            assert np.array_equal(x[:, 0].astype(np.int64) & 0xFFFFFFFF, np.arange(ns))  # (the int64 form: in the low word)
            assert np.all(x[::WC.CONST_EVERY] == x[::WC.CONST_EVERY, :1])
    if dt in ("i32", "i64"):
        assert _distinct_rows(x) == x.shape[0]
    else:
        # the float rows are pairwise distinct; the quantiser takes the mid-range (and with it s) out of the integers, so
        # two quiet rows may share theirs: nine rows in ten are still distinct, and the offsets carry s
        assert _distinct_rows(f) == ns
        assert _distinct_rows(x) > 0.9 * ns
    blob, st, nb = enc(x, level, use_threads=True)
    assert st[0] == 0 and np.array_equal(st[1:], np.cumsum(nb)[:-1]) and st[-1] + nb[-1] == blob.size
    sizes = np.unique(nb).size
    if n == 1:
        # one CONSTANT sample of 32 bits per stream: the format leaves the size no freedom, whatever the amplitude cycle
        assert sizes == 1
    elif n == 4:
        # four VERBATIM samples: the size moves with the wasted bits of the row alone
        assert sizes >= 2
    else:
        assert sizes >= 32, "only %d distinct stream sizes: widen the amplitude cycle" % sizes
    if name != "k3f_wide":  # (its serial oracle decode costs more than every other case together)
        assert np.array_equal(dec(blob, st, nb, n, use_threads=True), x)


def test_device_form_equals_host_form():
    """The generator written against torch (the form tests/test_gpu_wide.py runs on the device) gives numpy's values."""
    torch = pytest.importorskip("torch")
    for wide in (False, True):
        a = WC.wide_rows(2051, 37, wide, seed=3)
        b = WC.wide_rows(2051, 37, wide, seed=3, xp=torch, device="cpu").numpy()
        assert a.dtype == b.dtype and np.array_equal(a, b)
        rows = np.array([0, 5, 97, 101, 707, 2050])
        assert np.array_equal(WC.wide_rows(2051, 37, wide, seed=3, rows=rows), a[rows])


def test_strip_seektables_equals_the_per_stream_rewrite(oracle):
    from tests.conftest import strip_seektable

    for n, level in ((37, 5), (3 * 1152 + 11, 1)):
        x = WC.wide_rows(300, n, False, 1)
        blob, st, nb = oracle.encode_i32(x, level)
        got = WC.strip_seektables(blob, st, nb, -(-n // WC.block_size(level)))
        want = strip_seektable(blob, st, nb)
        assert all(np.array_equal(g, w) for g, w in zip(got, want))
        assert np.array_equal(oracle.decode_i32(*got, n), x)


FA_ERROR_CONVERT_TYPE = 1 << 19  # include/flacarray_hip.h


def test_conversion_grids_beyond_32_bits_are_refused():
    """The device quantisers launch one workgroup per stream, the restorers one per 16384-sample chunk: a stream count that
    does not fit the grid (2^32 one-sample float32 streams are 17 GB, within one card) used to be cast to `unsigned` and the
    streams behind the wrap were left unconverted.  The entry points now refuse it before they look at the device or at
    a pointer -- which is why this runs without a GPU, with no pointers at all."""
    from flacarray_amd import _lib

    L = _lib.lib()
    for ns in (1 << 31, (1 << 32) + 5, 1 << 40):
        assert L.fa_float32_to_int32_device(None, ns, 1, None, None, None, None, None) == FA_ERROR_CONVERT_TYPE
        assert L.fa_float64_to_int64_device(None, ns, 1, None, None, None, None, None) == FA_ERROR_CONVERT_TYPE
        assert L.fa_int32_to_float32_device(None, ns, 1, None, None, None, None) == FA_ERROR_CONVERT_TYPE
        assert L.fa_int64_to_float64_device(None, ns, 1, None, None, None, None) == FA_ERROR_CONVERT_TYPE
    # chunks, not streams: 2^20 streams of 2049 chunks each
    assert L.fa_int32_to_float32_device(None, 1 << 20, 2048 * 16384 + 1, None, None, None, None) == FA_ERROR_CONVERT_TYPE
    assert L.fa_int64_to_float64_device(None, 1 << 20, 2048 * 16384 + 1, None, None, None, None) == FA_ERROR_CONVERT_TYPE
    assert L.fa_int32_to_float32_device(None, 1, (1 << 62) + 7, None, None, None, None) == FA_ERROR_CONVERT_TYPE
