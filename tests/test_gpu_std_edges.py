"""std_device (S1 stream_chunk_sum_kernel, S2 stream_fold_kernel; csrc/std_kernels.hpp) on the corpus of
tests/std_corpus.py: every summation path -- the multi-batch plan, the fast chunk as a tail and as a whole row under a
larger buffer, two different plans in one call -- a hundred thousand roundings per short length, square roots picked
next to rounding boundaries, non-finite and subnormal values, and the plan cache walked through its key.

Every comparison is on unsigned bit patterns (any NaN equal to any NaN) against np.std of the same array under the same
np.getbufsize(); no tolerance anywhere.  tests/test_std_corpus.py shows on the CPU that the reference holds on every
case and that the corpus reaches the paths named here."""
import ctypes

import numpy as np
import pytest

from tests import std_corpus as C

pytestmark = pytest.mark.gpu

GUARD = 64  # sentinel elements before and after the results of a direct call
SENTINEL = {np.float32: -1234.5, np.float64: -1234.5}


@pytest.fixture(scope="module")
def corpus():
    return C.build()


def _bits(a):
    a = np.atleast_1d(np.asarray(a))
    return a.view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


def _assert_same(got, want, what):
    got, want = np.atleast_1d(got), np.atleast_1d(want)
    assert got.dtype == want.dtype and got.shape == want.shape, what
    nan = np.isnan(want)
    assert np.array_equal(np.isnan(got), nan), (what, "NaN rows", np.flatnonzero(np.isnan(got) != nan)[:8].tolist())
    bad = np.flatnonzero(_bits(got)[~nan] != _bits(want)[~nan])
    assert bad.size == 0, (what, "%d of %d rows differ" % (bad.size, got.size), bad[:8].tolist(),
                           got[~nan][bad[:4]].tolist(), want[~nan][bad[:4]].tolist())


def _std_device(fa, t, bufsize):
    """std_device under numpy's buffer size `bufsize` (the library reads np.getbufsize() at call time), on the host."""
    old = np.getbufsize()
    try:
        np.setbufsize(bufsize)
        return fa.std_device(t).cpu().numpy()
    finally:
        np.setbufsize(old)


@pytest.mark.parametrize("name", C.NAMES)
def test_corpus_case_is_np_std(corpus, name):
    import torch

    import flacarray_amd as fa

    case = corpus[name]
    _, dtype, x, b = case
    want = C.reference(case)
    got = _std_device(fa, torch.from_numpy(x.copy()).cuda(), b)
    _assert_same(got, want, name)


@pytest.mark.parametrize("dtype", C.DTYPES)
def test_fast_tail_of_rows_off_a_16_byte_boundary(corpus, dtype):
    """The fast chunk reached as the TAIL of a plan chunk, in rows that start one element off a 16-byte boundary: the
    element-wise staging of the lane-per-leaf path, which the aligned corpus rows (even lengths) do not take there."""
    import torch

    import flacarray_amd as fa

    case = corpus[f"geom_{C.tag(dtype)}_buf16384_2b+8192"]
    _, _, x, b = case
    flat = torch.zeros(x.size + 4, dtype=torch.float32 if dtype == np.float32 else torch.float64, device="cuda")
    t = flat[1 : 1 + x.size].view(x.shape)
    t.copy_(torch.from_numpy(x.copy()))
    assert t.is_contiguous() and t.data_ptr() % 16 and (x.shape[1] * x.itemsize) % 16 == 0
    _assert_same(_std_device(fa, t, b), C.reference(case), case[0])


# ------------------------------------------------------------------------------------------------ the C entry points
def _entry(dtype):
    from flacarray_amd import _lib

    L = _lib.lib()
    return L.fa_stream_std_f32_device if np.dtype(dtype) == np.float32 else L.fa_stream_std_f64_device


def _guarded_out(torch, dtype, n):
    tdt = torch.float32 if np.dtype(dtype) == np.float32 else torch.float64
    return torch.full((n + 2 * GUARD,), SENTINEL[dtype], dtype=tdt, device="cuda")


def _raw_call(torch, dtype, t, n_stream, stream_size, chunk, buf):
    """fa_stream_std_*_device writing at buf[GUARD:]; returns (return code, the whole buffer on the host)."""
    from flacarray_amd import libflacarray as LF

    out_ptr = ctypes.c_void_p(buf.data_ptr() + GUARD * buf.element_size())
    rc = _entry(dtype)(ctypes.c_void_p(t.data_ptr()), n_stream, stream_size, chunk, out_ptr, LF._stream_ptr())
    torch.cuda.synchronize()
    return rc, buf.cpu().numpy()


@pytest.mark.parametrize("dtype", C.DTYPES)
@pytest.mark.parametrize("which", ["sweep_{}_n7", "geom_{}_buf262160_3b+5"])
def test_entry_point_writes_n_stream_results_and_nothing_else(corpus, dtype, which):
    import torch

    case = corpus[which.format(C.tag(dtype))]
    _, _, x, b = case
    t = torch.from_numpy(x.copy()).cuda()
    buf = _guarded_out(torch, dtype, x.shape[0])
    rc, host = _raw_call(torch, dtype, t, x.shape[0], x.shape[1], b, buf)
    assert rc == 0
    sentinel = np.full(GUARD, SENTINEL[dtype], dtype=dtype)
    assert np.array_equal(_bits(host[:GUARD]), _bits(sentinel)), "guard before the results"
    assert np.array_equal(_bits(host[-GUARD:]), _bits(sentinel)), "guard behind the results"
    _assert_same(host[GUARD:-GUARD], C.reference(case), case[0])


@pytest.mark.parametrize("dtype", C.DTYPES)
def test_entry_point_refusals_leave_the_output_alone(dtype):
    """n_stream, stream_size or chunk not positive: a non-zero return code and no write.  (The counts never exceed the
    buffers.  The fourth refusal, n_stream > INT32_MAX / chunks per stream, needs 2**31 chunk sums and is left out:
    profiles/std_edges.md.)"""
    import torch

    rows, n = 3, 1000
    x = np.random.default_rng(5).normal(size=(rows, n)).astype(dtype)
    t = torch.from_numpy(x).cuda()
    untouched = np.full(rows + 2 * GUARD, SENTINEL[dtype], dtype=dtype)
    for n_stream, stream_size, chunk in ((0, n, 8192), (-1, n, 8192), (rows, 0, 8192), (rows, -5, 8192), (rows, n, 0),
                                         (rows, n, -8192), (0, 0, 0)):
        buf = _guarded_out(torch, dtype, rows)
        rc, host = _raw_call(torch, dtype, t, n_stream, stream_size, chunk, buf)
        assert rc != 0, (n_stream, stream_size, chunk)
        assert np.array_equal(_bits(host), _bits(untouched)), (n_stream, stream_size, chunk)
    # and the accepted call on the same buffers is right
    buf = _guarded_out(torch, dtype, rows)
    rc, host = _raw_call(torch, dtype, t, rows, n, 8192, buf)
    assert rc == 0
    _assert_same(host[GUARD:-GUARD], np.std(x, axis=-1), "accepted call")


def test_std_device_refusals():
    """What std_device raises for tensors it does not take."""
    import torch

    import flacarray_amd as fa

    good = torch.ones((4, 100), dtype=torch.float32, device="cuda")
    with pytest.raises(RuntimeError, match="^Only C-contiguous arrays are supported$"):
        fa.std_device(good.t())
    with pytest.raises(RuntimeError, match="^Only C-contiguous arrays are supported$"):
        fa.std_device(good[:, ::2])
    for idt in (torch.int32, torch.int64, torch.float16):
        with pytest.raises(ValueError, match="^Only float32 and float64 data are supported$"):
            fa.std_device(torch.ones((4, 100), dtype=idt, device="cuda"))
    for fdt in (torch.float32, torch.float64):
        with pytest.raises(RuntimeError, match="^std_device needs a tensor on the GPU$"):
            fa.std_device(torch.ones((4, 100), dtype=fdt))
        for shape in ((0,), (0, 100), (4, 0)):
            with pytest.raises(ValueError, match="^std_device needs a non-empty array with a stream axis$"):
                fa.std_device(torch.ones(shape, dtype=fdt, device="cuda"))
        with pytest.raises(ValueError, match="^std_device needs a non-empty array with a stream axis$"):
            fa.std_device(torch.ones((), dtype=fdt, device="cuda"))
    assert fa.std_device(good).cpu().numpy().tolist() == [0.0] * 4  # and the good tensor still goes through


# ------------------------------------------------------------------------------------------------------ the plan cache
# (stream size, buffer size, dtype): neighbours share one field of the cache key (stream size, chunk); step 4 has no plan
# at all (the upload is skipped and the cached key must survive or be rebuilt correctly), steps 6 and 7 run one geometry
# in both dtypes, step 8 makes the plan slot grow (8192 leaves and 16383 program bytes), step 9 is step 1 again.
WALK = [
    (12345, 8192, np.float32),
    (12345, 4096, np.float32),
    (10000, 4096, np.float32),
    (8192, 8192, np.float32),
    (12345, 8192, np.float32),
    (12345, 8192, np.float64),
    (12345, 8192, np.float32),
    (3 * 2**20 + 5, 2**20, np.float32),
    (12345, 8192, np.float32),
]


def test_plan_cache_walk(corpus):
    import torch

    import flacarray_amd as fa

    data = {}
    for n, b, dtype in WALK:
        if (n, dtype) not in data:
            if n == 3 * 2**20 + 5:
                x = np.array(corpus["geom_f32_buf1048576_3b+5"][2])
            else:
                x = (1e3 + np.random.default_rng(n).normal(size=(3, n))).astype(dtype)
            data[(n, dtype)] = (x, torch.from_numpy(x).cuda())
    want = []
    old = np.getbufsize()
    try:
        for n, b, dtype in WALK:
            np.setbufsize(b)
            want.append(np.std(data[(n, dtype)][0], axis=-1))
    finally:
        np.setbufsize(old)
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    for where in ("default", "side"):
        for i, (n, b, dtype) in enumerate(WALK):
            t = data[(n, dtype)][1]
            if where == "side":
                with torch.cuda.stream(side):  # (a non-blocking stream: nothing orders it behind the null stream)
                    got = _std_device(fa, t, b)
            else:
                got = _std_device(fa, t, b)
            _assert_same(got, want[i], "%s stream, step %d: %s" % (where, i + 1, (n, b, np.dtype(dtype).name)))


# ---------------------------------------------------------------------------------------------------------- end to end
def _same_store(dev, host):
    assert dev.dtype == host.dtype and dev.shape == host.shape
    assert np.array_equal(dev.compressed, host.compressed)
    assert np.array_equal(dev.stream_starts, host.stream_starts)
    assert np.array_equal(dev.stream_nbytes, host.stream_nbytes)
    assert dev.stream_offsets.dtype == host.stream_offsets.dtype
    assert np.array_equal(_bits(dev.stream_offsets), _bits(host.stream_offsets))
    assert np.array_equal(_bits(dev.stream_gains), _bits(host.stream_gains))


@pytest.mark.parametrize("dtype", C.DTYPES)
@pytest.mark.parametrize("kind", ["pinf", "sum_overflow", "square_overflow", "subnormal_var", "negzero"])
def test_precision_on_hard_rows_behaves_like_from_array(corpus, dtype, kind):
    """precision=3 quantises with std / 1000 per stream: the hard row between two ordinary ones gives the same store
    (bytes, index, offsets and gains as bits) from the device route as from the host route, or the same exception."""
    import torch

    import flacarray_amd as fa

    x = np.array(corpus[f"hard_{C.tag(dtype)}_{kind}"][2])
    t = torch.from_numpy(x).cuda()
    with np.errstate(all="ignore"):
        try:
            host = fa.FlacArray.from_array(x, precision=3)
        except Exception as exc:  # noqa: BLE001
            with pytest.raises(type(exc)) as got:
                fa.FlacArray.from_device_array(t, precision=3)
            assert str(got.value) == str(exc)
            return
        _same_store(fa.FlacArray.from_device_array(t, precision=3), host)
