"""Every float quantise and restore route of the library against the numpy model of tests/quant_model.py, bit for bit,
on the edge corpus: truncated peaks, infinite samples, subnormal data and quanta, zero / huge / infinite quanta, exact
ties, products at +-2^31 (+-2^63), tiny and unaligned lengths, streams longer than one range chunk, and restores with
user-supplied gains of 0, inf, negative and subnormal values.

Integers, offsets, gains and restored values are compared as unsigned bit patterns.  The one permitted difference is
that any NaN equals any NaN: the reference on x86 produces the negative default NaN, the GPU the positive one.

Quantise routes compare integers, offsets and gains with the model; routes that encode also compare the compressed
bytes with the CPU oracle's encoding of the model's integers, and the device routes decode them back.  Restore routes
decode the oracle's encoding of integers and restore them with the given offsets and gains, whole and in windows and
slices that start and end on and off a 4-sample boundary."""
import functools

import numpy as np
import pytest

from oracle import oracle as O
from tests import quant_model as M

pytestmark = pytest.mark.gpu

DTYPES = {"f32": np.float32, "f64": np.float64}
QCASES = {k: M.quantise_cases(dt) for k, dt in DTYPES.items()}
RCASES = {k: M.restore_cases(dt) for k, dt in DTYPES.items()}


@pytest.fixture(autouse=True, params=["auto", "k7", "k7l"])
def dispatch(request, monkeypatch):
    """As tests/test_gpu_parity.py: the library's own dispatch; K7L off and K3F taking every array of its geometry; and
    K7L taking every decode launch (the variables are read per call)."""
    for v in ("FLACARRAY_HIP_LATENCY", "FLACARRAY_HIP_PLACED_BELOW", "FLACARRAY_HIP_HOST_CHUNK_BYTES"):
        monkeypatch.delenv(v, raising=False)
    if request.param == "k7":
        monkeypatch.setenv("FLACARRAY_HIP_LATENCY", "0")
        monkeypatch.setenv("FLACARRAY_HIP_PLACED_BELOW", "0")
    elif request.param == "k7l":
        monkeypatch.setenv("FLACARRAY_HIP_LATENCY", "1")
    return request.param


@pytest.fixture(scope="module")
def fa():
    import flacarray_amd

    return flacarray_amd


@functools.lru_cache(maxsize=None)
def _expected(kind, i):
    """The model's (ints, offsets, gains) for quantise case i."""
    c = QCASES[kind][i]
    return M.quantise(c.x, c.quanta)


@functools.lru_cache(maxsize=None)
def _oracle_blob(kind, src, i, level):
    """The oracle's encoding of the model's integers (src "q") or of a restore case's integers (src "r")."""
    ints = _expected(kind, i)[0] if src == "q" else RCASES[kind][i].ints
    return (O.encode_i32 if kind == "f32" else O.encode_i64)(ints, level)


def _np(t):
    return t.cpu().numpy() if hasattr(t, "cpu") else np.asarray(t)


def _check(what, got, want):
    assert M.bits_equal(_np(got).reshape(np.shape(want)), want), what


# ---------------------------------------------------------------------------------------------------------------
# Quantise routes: each returns a dict with some of ints, offsets, gains, blob (compressed, starts, nbytes), level,
# device (the blob is a device tensor triple to decode back); None = the route does not take this case
# ---------------------------------------------------------------------------------------------------------------
def _q_tensor(torch, c):
    return None if c.quanta is None else torch.from_numpy(c.quanta).cuda()


def r_device_quantise(fa, torch, kind, c):
    from flacarray_amd.libflacarray import float32_to_int32_device, float64_to_int64_device

    f = float32_to_int32_device if kind == "f32" else float64_to_int64_device
    ints, off, gain = f(torch.from_numpy(c.x).cuda(), _q_tensor(torch, c))
    return {"ints": _np(ints), "offsets": _np(off), "gains": _np(gain)}


def _device_encode(level):
    def route(fa, torch, kind, c):
        from flacarray_amd.libflacarray import encode_flac_device_f32, encode_flac_device_f64

        f = encode_flac_device_f32 if kind == "f32" else encode_flac_device_f64
        comp, st, nb, off, gain = f(torch.from_numpy(c.x).cuda(), _q_tensor(torch, c), level=level)
        return {"offsets": _np(off), "gains": _np(gain), "blob": (comp, st, nb), "level": level, "device": True}

    return route


def _host_encode(chunked):
    def route(fa, torch, kind, c):
        import os

        from flacarray_amd.libflacarray import encode_flac_f32, encode_flac_f64

        if chunked:  # one or two streams per chunk of the host pipeline
            os.environ["FLACARRAY_HIP_HOST_CHUNK_BYTES"] = str(8 * c.x.shape[1])
        try:
            comp, st, nb, off, gain = (encode_flac_f32 if kind == "f32" else encode_flac_f64)(c.x, c.quanta, 5)
        finally:
            os.environ.pop("FLACARRAY_HIP_HOST_CHUNK_BYTES", None)
        return {"offsets": off, "gains": gain, "blob": (comp, st, nb), "level": 5}

    return route


def r_c_abi(fa, torch, kind, c):
    from flacarray_amd.libflacarray import wrap_float32_to_int32, wrap_float64_to_int64

    f = wrap_float32_to_int32 if kind == "f32" else wrap_float64_to_int64
    q = np.zeros(0, dtype=c.x.dtype) if c.quanta is None else c.quanta
    ints, off, gain = f(c.x.reshape(-1), c.x.shape[0], c.x.shape[1], q)
    return {"ints": ints, "offsets": off, "gains": gain}


def r_array_compress(fa, torch, kind, c):
    if c.quanta is None:  # array_compress needs quanta or precision
        return None
    comp, st, nb, off, gain = fa.array_compress(c.x, level=5, quanta=c.quanta)
    return {"offsets": off, "gains": gain, "blob": (comp, st, nb), "level": 5}


def r_from_array(fa, torch, kind, c):
    if c.quanta is None:
        return None
    a = fa.FlacArray.from_array(c.x, level=5, quanta=c.quanta)
    return {"offsets": a.stream_offsets, "gains": a.stream_gains, "blob": (a.compressed, a.stream_starts, a.stream_nbytes), "level": 5}


def r_from_device_array(fa, torch, kind, c):
    if c.quanta is None:
        return None
    a = fa.FlacArray.from_device_array(torch.from_numpy(c.x).cuda(), level=5, quanta=c.quanta)
    return {"offsets": a.stream_offsets, "gains": a.stream_gains, "blob": (a.compressed, a.stream_starts, a.stream_nbytes), "level": 5}


Q_ROUTES = {
    "device_quantise": r_device_quantise,
    "device_encode_l5": _device_encode(5),  # K3F where the geometry allows (length a multiple of 4096), else two steps
    "device_encode_l1": _device_encode(1),  # levels 0-2: always quantise, then encode
    "host_encode": _host_encode(False),
    "host_encode_chunked": _host_encode(True),
    "c_abi": r_c_abi,
    "array_compress": r_array_compress,
    "from_array": r_from_array,
    "from_device_array": r_from_device_array,
}


def _check_quantised(fa, torch, kind, name, c, got, ints, off, gain):
    if "ints" in got:
        _check(f"{name}: integers", got["ints"], ints)
    _check(f"{name}: offsets", got["offsets"], off)
    _check(f"{name}: gains", got["gains"], gain)
    if "blob" in got:
        comp, st, nb = (_np(t) for t in got["blob"])
        blob_o, st_o, nb_o = O.encode_i32(ints, got["level"]) if kind == "f32" else O.encode_i64(ints, got["level"])
        assert np.array_equal(comp, blob_o) and np.array_equal(st.reshape(-1), st_o) and np.array_equal(nb.reshape(-1), nb_o), \
            f"{name}: compressed bytes differ from the oracle's encoding of the model's integers"
        if got.get("device"):
            back = fa.decode_flac_device(*got["blob"], c.x.shape[1], is_int64=(kind == "f64"))
            _check(f"{name}: decoded integers", _np(back).reshape(ints.shape), ints)


@pytest.mark.parametrize("kind", list(DTYPES))
@pytest.mark.parametrize("route", list(Q_ROUTES))
def test_quantise_route_matches_model(fa, kind, route):
    import torch

    ran = 0
    for i, c in enumerate(QCASES[kind]):
        got = Q_ROUTES[route](fa, torch, kind, c)
        if got is None:
            continue
        ints, off, gain = _expected(kind, i)
        _check_quantised(fa, torch, kind, f"{route} {kind} {c.name}", c, got, ints, off, gain)
        ran += 1
    assert ran >= len(QCASES[kind]) // 2


@pytest.mark.parametrize("kind", list(DTYPES))
def test_precision_matches_model(fa, kind):
    """precision=p on finite cases: quanta = np.std(x) / 10**p as the reference's Python forms it, fed to the model."""
    import torch

    from flacarray_amd.libflacarray import encode_flac_device_f32, encode_flac_device_f64

    dev_encode = encode_flac_device_f32 if kind == "f32" else encode_flac_device_f64
    ran = 0
    for c in QCASES[kind]:
        if c.quanta is not None or not np.all(np.isfinite(c.x)):
            continue
        p = 3
        with np.errstate(over="ignore", invalid="ignore"):  # (the huge family's std overflows to inf: a legal quanta)
            q = (np.std(c.x, axis=-1, keepdims=True) / 10**p).reshape(-1)
        assert q.dtype == c.x.dtype
        ints, off, gain = M.quantise(c.x, q)
        name = f"precision {kind} {c.name}"
        comp, st, nb, o2, g2 = fa.array_compress(c.x, level=5, precision=p)
        _check_quantised(fa, torch, kind, name + " array_compress", c, {"offsets": o2, "gains": g2, "blob": (comp, st, nb), "level": 5},
                         ints, off, gain)
        xd = torch.from_numpy(c.x).cuda()
        comp, st, nb, o2, g2 = dev_encode(xd, level=5, precision=p)
        _check_quantised(fa, torch, kind, name + " device", c, {"offsets": o2, "gains": g2, "blob": (comp, st, nb), "level": 5, "device": True},
                         ints, off, gain)
        a = fa.FlacArray.from_device_array(xd, level=5, precision=p)
        _check(name + " from_device_array offsets", a.stream_offsets, off)
        _check(name + " from_device_array gains", a.stream_gains, gain)
        ran += 1
    assert ran >= 10


# ---------------------------------------------------------------------------------------------------------------
# Restore routes: the oracle's encoding of known integers, restored with offsets / gains by the library
# ---------------------------------------------------------------------------------------------------------------
def _restore_inputs(kind):
    """(name, ints, offsets, gains, (blob, starts, nbytes)): the user-gain cases and the model's output of every
    quantise case."""
    for i, c in enumerate(RCASES[kind]):
        yield c.name, c.ints, c.offsets, c.gains, _oracle_blob(kind, "r", i, 5)
    for i, c in enumerate(QCASES[kind]):
        ints, off, gain = _expected(kind, i)
        yield "quantised " + c.name, ints, off, gain, _oracle_blob(kind, "q", i, 5)


def _dev(torch, a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def rr_c_abi(fa, torch, kind, ints, off, gain, blob, win):
    if win != (0, ints.shape[1]):
        return None
    from flacarray_amd.libflacarray import wrap_int32_to_float32, wrap_int64_to_float64

    f = wrap_int32_to_float32 if kind == "f32" else wrap_int64_to_float64
    return f(ints.reshape(-1), ints.shape[0], ints.shape[1], off, gain)


def rr_decode_device(fa, torch, kind, ints, off, gain, blob, win):
    comp, st, nb = (_dev(torch, a) for a in blob)
    return fa.decode_flac_device(comp, st, nb, ints.shape[1], win[0], win[1], offsets=_dev(torch, off), gains=_dev(torch, gain),
                                 is_int64=(kind == "f64"))


def rr_index_decode(fa, torch, kind, ints, off, gain, blob, win):
    from flacarray_amd.libflacarray import DeviceDecodeIndex

    comp, st, nb = (_dev(torch, a) for a in blob)
    idx = DeviceDecodeIndex(comp, st, nb, ints.shape[1], is_int64=(kind == "f64"))
    try:
        return idx.decode(win[0], win[1], offsets=_dev(torch, off), gains=_dev(torch, gain))
    finally:
        idx.close()


def rr_host_restore(fa, torch, kind, ints, off, gain, blob, win):
    from flacarray_amd.libflacarray import decode_flac_restore

    out = decode_flac_restore(blob[0], blob[1], blob[2], ints.shape[1], off, gain, win[0], win[1], is_int64=(kind == "f64"))
    assert out is not None, "decode_flac_restore refused the call"
    return out


def rr_array_decompress(fa, torch, kind, ints, off, gain, blob, win):
    return fa.array_decompress(blob[0], ints.shape[1], blob[1], blob[2], stream_offsets=off, stream_gains=gain, first_stream_sample=win[0],
                               last_stream_sample=win[1], is_int64=(kind == "f64"))


def _resident(fa, kind, ints, off, gain, blob):
    dt = np.float32 if kind == "f32" else np.float64
    return fa.FlacArray._assemble(ints.shape, None, np.dtype(dt), blob[0], blob[1], blob[2], off, gain).to_device()


def rr_resident_getitem(fa, torch, kind, ints, off, gain, blob, win):
    a = _resident(fa, kind, ints, off, gain, blob)
    try:
        return a[:, win[0] : win[1]]
    finally:
        a.release_device()


R_ROUTES = {
    "c_abi": rr_c_abi,
    "decode_device": rr_decode_device,
    "index_decode": rr_index_decode,
    "host_restore": rr_host_restore,
    "array_decompress": rr_array_decompress,
    "resident_getitem": rr_resident_getitem,
}


@pytest.mark.parametrize("kind", list(DTYPES))
@pytest.mark.parametrize("route", list(R_ROUTES))
def test_restore_route_matches_model(fa, kind, route):
    import torch

    ran = 0
    for name, ints, off, gain, blob in _restore_inputs(kind):
        for win in M.windows(ints.shape[1]):
            got = R_ROUTES[route](fa, torch, kind, ints, off, gain, blob, win)
            if got is None:
                continue
            want = M.restore(ints[:, win[0] : win[1]], off, gain)
            _check(f"{route} {kind} {name} window {win}", _np(got), want)
            ran += 1
    assert ran >= 40


S_ROUTES = ["decode_slices_device", "index_slices", "index_slices_to_host", "resident_read_slices", "read_slices"]


@pytest.mark.parametrize("kind", list(DTYPES))
@pytest.mark.parametrize("route", S_ROUTES)
def test_restore_slices_match_model(fa, kind, route):
    import torch

    from flacarray_amd.libflacarray import DeviceDecodeIndex, decode_slices_device

    for name, ints, off, gain, blob in _restore_inputs(kind):
        ss, sf, sc = M.slices(*ints.shape)
        want = [M.restore(ints[s : s + 1, f : f + n], off[s : s + 1], gain[s : s + 1]).reshape(-1) for s, f, n in zip(ss, sf, sc)]
        what = f"{route} {kind} {name}"
        if route in ("resident_read_slices", "read_slices"):
            dt = np.float32 if kind == "f32" else np.float64
            a = fa.FlacArray._assemble(ints.shape, None, np.dtype(dt), blob[0], blob[1], blob[2], off, gain)
            if route == "resident_read_slices":
                a.to_device()
            got = a.read_slices(ss, sf, sc)
            a.release_device()
            for k, (g, w) in enumerate(zip(got, want)):
                _check(f"{what} slice {k}", _np(g), w)
            continue
        comp, st, nb = (_dev(torch, x) for x in blob)
        if route == "decode_slices_device":
            flat, oo = decode_slices_device(comp, st, nb, ints.shape[1], ss, sf, sc, offsets=_dev(torch, off), gains=_dev(torch, gain),
                                            is_int64=(kind == "f64"))
        else:
            idx = DeviceDecodeIndex(comp, st, nb, ints.shape[1], is_int64=(kind == "f64"))
            flat, oo = idx.decode_slices(ss, sf, sc, offsets=_dev(torch, off), gains=_dev(torch, gain), to_host=(route == "index_slices_to_host"))
            idx.close()
        flat = _np(flat)
        for k, (o, n, w) in enumerate(zip(oo, sc, want)):
            _check(f"{what} slice {k}", flat[o : o + n], w)


def test_corpus_reaches_every_edge():
    """The corpus the routes above run on reaches every named edge (from the model's own results)."""
    for kind, dt in DTYPES.items():
        tags = M.corpus_tags(dt)
        assert {"truncated_peak", "tie", "inf", "subnormal", "st_zero", "long", "unaligned_length"} <= tags, kind
        assert any(c.x.shape[1] % 4096 == 0 and c.x.shape[1] > 65536 for c in QCASES[kind])
        assert any(np.any(np.isinf(c.gains)) or np.any(c.gains == 0) for c in RCASES[kind])
    assert any(f % 4 for f, _ in M.windows(8195)) and any(last % 4 for _, last in M.windows(8195))
    assert any(f % 4 for f in M.slices(3, 8195)[1])
