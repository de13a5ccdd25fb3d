"""Device-resident float compression with `precision=` and float64 tensors: std_device against np.std bit for bit, and
FlacArray.from_device_array against from_array on the tensor's host copy (same bytes, index, offsets and gains)."""
import numpy as np
import pytest

from tests.golden import reference_published as P

pytestmark = pytest.mark.gpu

LENGTHS = [1, 7, 8, 9, 127, 128, 129, 136, 1000, 8191, 8192, 8193, 10000, 12345, 100000, 2**20 - 3, 2**20]


def _bits(a):
    a = np.atleast_1d(np.asarray(a))
    return a.view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


def _data(shape, dtype, seed, dc=0.0):
    rng = np.random.default_rng(seed)
    return (dc + rng.normal(size=shape) * (1 + rng.random(shape[:-1] + (1,)))).astype(dtype)


def _std_check(x):
    import torch

    import flacarray_amd as fa

    got = fa.std_device(torch.from_numpy(x).cuda()).cpu().numpy()
    want = np.std(x, axis=-1).reshape(got.shape)
    assert got.dtype == want.dtype
    assert np.array_equal(_bits(got), _bits(want)), (x.shape, x.dtype)


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("n", LENGTHS)
def test_std_device_is_np_std(dtype, n):
    rows = 3 if n <= 2**16 else 2
    _std_check(_data((rows, n), dtype, n))
    _std_check(_data((rows, n), dtype, n + 1, dc=1e6))  # large offset: the mean's rounding matters
    _std_check(_data((n,), dtype, n + 2))
    if n <= 12345:
        _std_check(_data((2, 2, n), dtype, n + 3))
        _std_check(np.full((2, n), 0.1, dtype=dtype))


def test_std_device_large_float32():
    _std_check(_data((256, 2**20), np.float32, 11))


def test_std_device_unaligned_rows():
    """Rows that start off a 16-byte boundary take the element-wise staging of the lane-per-leaf path."""
    for dtype in (np.float32, np.float64):
        _std_check(_data((5, 8192 * 3 + 1), dtype, 12))


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_std_device_follows_the_buffer_size(dtype):
    old = np.getbufsize()
    try:
        np.setbufsize(4096)
        for n in (1000, 4096, 8192, 12345, 100000):
            _std_check(_data((3, n), dtype, n, dc=1e3))
    finally:
        np.setbufsize(old)
    _std_check(_data((3, 12345), dtype, 5, dc=1e3))  # and back at 8192


def test_std_device_nan_rows():
    import torch

    import flacarray_amd as fa

    for dtype in (np.float32, np.float64):
        x = _data((4, 9000), dtype, 3)
        x[1, 17] = np.nan
        x[3, 8999] = np.nan
        got = fa.std_device(torch.from_numpy(x).cuda()).cpu().numpy()
        assert np.isnan(got[[1, 3]]).all() and np.array_equal(_bits(got[[0, 2]]), _bits(np.std(x[[0, 2]], axis=-1)))


def _same_store(dev, host):
    assert dev.dtype == host.dtype and dev.shape == host.shape
    assert np.array_equal(dev.compressed, host.compressed)
    assert np.array_equal(dev.stream_starts, host.stream_starts)
    assert np.array_equal(dev.stream_nbytes, host.stream_nbytes)
    assert dev.stream_offsets.dtype == host.stream_offsets.dtype
    assert np.array_equal(_bits(dev.stream_offsets), _bits(host.stream_offsets))
    assert np.array_equal(_bits(dev.stream_gains), _bits(host.stream_gains))


SHAPES = [(4, 3, 10000), (64, 2**16), (5, 100001), (1000,)]


def _precisions(dtype, shape):
    lead = shape[:-1]
    per_stream = (np.arange(int(np.prod(lead))) % 4 + 1).reshape(lead)
    return [3, -1, per_stream, 6 if dtype == np.float32 else 10]


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("level", [0, 5, 8])
def test_from_device_array_precision_matches_from_array(dtype, shape, level):
    import torch

    import flacarray_amd as fa

    x = _data(shape, dtype, sum(shape) + level, dc=3.0)
    t = torch.from_numpy(x).cuda()
    for p in _precisions(dtype, shape):
        dev = fa.FlacArray.from_device_array(t, level=level, precision=p)
        host = fa.FlacArray.from_array(t.cpu().numpy(), level=level, precision=p)
        _same_store(dev, host)


@pytest.mark.parametrize("shape", [(4, 3, 10000), (5, 100001), (1000,)])
def test_from_device_array_float64_quanta_matches_from_array(shape):
    import torch

    import flacarray_amd as fa

    x = _data(shape, np.float64, 21, dc=-2.0)
    t = torch.from_numpy(x).cuda()
    lead = shape[:-1]
    for q in (1e-6, np.full(lead, 1e-5) * (1 + np.arange(int(np.prod(lead))).reshape(lead))):
        _same_store(fa.FlacArray.from_device_array(t, quanta=q), fa.FlacArray.from_array(x, quanta=q))


def test_tutorial_size_through_the_device():
    """The tutorial's (4, 3, 10000) float64 array at precision=10 (522 899 B published) from a torch tensor."""
    import torch

    import flacarray_amd as fa

    shape, dtype, kw, published, where = P.SIZES[2]
    arr = P.fake_data(shape, dtype)
    f = fa.FlacArray.from_device_array(torch.from_numpy(arr).cuda(), **kw)
    n_stream = int(np.prod(shape[:-1]))
    assert f.nbytes == published + 14 * n_stream, where
    assert f.nbytes - n_stream * P.own_stream_header(shape[-1], 5) == P.frame_bytes_published(P.SIZES[2])


def test_resident_float64_reads_match_the_host_store():
    import torch

    import flacarray_amd as fa

    x = _data((3, 4, 20000), np.float64, 8, dc=1.0)
    dev = fa.FlacArray.from_device_array(torch.from_numpy(x).cuda(), precision=5)
    host = fa.FlacArray.from_array(x, precision=5)
    assert dev.is_resident and dev.dtype == np.float64
    full = host.to_array()
    assert np.array_equal(_bits(dev.to_array()), _bits(full))
    for key in ((1, 2), (slice(0, 2), 3, slice(100, 5000)), (2, slice(None), slice(19000, None)), (0, 1, 4096)):
        assert np.array_equal(_bits(dev[key]), _bits(host[key])), key
    got = dev.read_slices([0, 5, 11], [0, 4000, 19990], [10, 3000, 10])
    for g, s, a, c in zip(got, [0, 5, 11], [0, 4000, 19990], [10, 3000, 10]):
        assert np.array_equal(_bits(g), _bits(full.reshape(12, -1)[s, a : a + c]))


def _raises_like(fn_dev, fn_host):
    with pytest.raises(Exception) as want:
        fn_host()
    with pytest.raises(type(want.value)) as got:
        fn_dev()
    assert str(got.value) == str(want.value)


def test_argument_errors_match_array_compress():
    import torch

    import flacarray_amd as fa

    for dtype in (np.float32, np.float64):
        x = _data((3, 5000), dtype, 4)
        t = torch.from_numpy(x).cuda()
        xn = x.copy()
        xn[1, 7] = np.nan
        tn = torch.from_numpy(xn).cuda()
        cases = [
            (dict(precision=3), xn, tn),
            (dict(quanta=1e-4), xn, tn),
            (dict(), x, t),
            (dict(quanta=1e-4, precision=3), x, t),
            (dict(quanta=np.ones(4)), x, t),
            (dict(precision=np.ones(4, dtype=np.int64)), x, t),
            (dict(precision=np.ones((3, 1), dtype=np.int64)), x, t),
        ]
        for kw, xa, ta in cases:
            _raises_like(lambda: fa.FlacArray.from_device_array(ta, **kw), lambda: fa.FlacArray.from_array(xa, **kw))
        # a CPU tensor raises as the integer path does
        with pytest.raises(RuntimeError, match="needs a tensor on the GPU"):
            fa.FlacArray.from_device_array(torch.from_numpy(x), precision=3)
    with pytest.raises(RuntimeError, match="needs a tensor on the GPU"):
        fa.FlacArray.from_device_array(torch.zeros((2, 100), dtype=torch.int32))
    # integer tensors ignore quanta and precision, as array_compress does
    xi = np.arange(6000, dtype=np.int32).reshape(2, 3000)
    _same_int = fa.FlacArray.from_device_array(torch.from_numpy(xi).cuda(), precision=3)
    assert np.array_equal(_same_int.compressed, fa.FlacArray.from_array(xi, precision=3).compressed)


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_constant_row_with_precision_behaves_like_from_array(dtype):
    import torch

    import flacarray_amd as fa

    x = _data((3, 9000), dtype, 6)
    x[1] = 0.25
    t = torch.from_numpy(x).cuda()
    try:
        host = fa.FlacArray.from_array(x, precision=4)
    except Exception as exc:  # noqa: BLE001
        with pytest.raises(type(exc)) as got:
            fa.FlacArray.from_device_array(t, precision=4)
        assert str(got.value) == str(exc)
        return
    _same_store(fa.FlacArray.from_device_array(t, precision=4), host)
