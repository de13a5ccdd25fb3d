"""Stream order of the device API: every `*_device` call made on a torch side stream, behind a producer that is still
running (tests/stream_tools.py), must wait for its inputs through that stream alone and leave outputs that are complete in
its order.  Every case compares the side-stream result bit for bit with the same call on the default stream and, where one
exists, with the oracle (bytes of oracle.encode_i32 / encode_i64, or the numpy slice of the input).

The decoys are valid data throughout: another array of the same shape for encoders and quantisers, the encode of another
array for decoders (one buffer sized for the larger blob; starts / nbytes / offsets / gains are inputs like the bytes).  A
call that reads too early answers for the decoy; no decoder is ever handed garbage.

Calls of one device on different streams do not run concurrently inside the library: they are serialised on the host by
the per-device `api_mu`, and by nothing on the device.  What a call leaves queued when it returns (K3F's header / index
kernel, a splice) is ordered only against later work of ITS stream; test_alternating_streams pins the outcome of that
arrangement whenever the code is right, it cannot prove a race on the shared header table absent.

The side-stream frame check of large verified decodes ("beside" path: 16384 tasks and more) is driven at the end of the
file with an intact and a damaged store, on both kinds of stream, with and without FLACARRAY_HIP_VERIFY_AFTER.
"""
import hashlib
import time

import numpy as np
import pytest

from tests import stream_tools as T
from tests.conftest import full_range_i32, sinusoid_noise_f32, sinusoid_noise_i32, strip_seektable

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def fa():
    import flacarray_amd

    return flacarray_amd


@pytest.fixture(scope="module")
def torch():
    import torch

    return torch


@pytest.fixture(scope="module")
def side(torch):
    s = torch.cuda.Stream()
    yield s
    torch.cuda.synchronize()
    if T.WARM_SECONDS:
        worst = max(T.WARM_SECONDS, key=T.WARM_SECONDS.get)
        print(f"\n[streams] delay {T.DELAY_MS} ms ({T.cycles_per_ms():.0f} spin cycles per ms, margin included); longest warm "
              f"default-stream call: {worst} {T.WARM_SECONDS[worst] * 1e3:.3f} ms ({len(T.WARM_SECONDS)} cases)")


@pytest.fixture(autouse=True)
def _own_dispatch(monkeypatch):
    """Every case starts from the library's own dispatch; the K3F and K7 cases set their variable themselves."""
    for v in ("FLACARRAY_HIP_PLACED_BELOW", "FLACARRAY_HIP_LATENCY", "FLACARRAY_HIP_SLOTS", "FLACARRAY_HIP_VERIFY_AFTER"):
        monkeypatch.delenv(v, raising=False)


def _dev(torch, x):
    return torch.from_numpy(np.ascontiguousarray(x)).cuda()


def _i64(n_ch, n, seed):
    """int64 samples that use both words (|x| up to ~2^37) and both signs."""
    rng = np.random.default_rng(seed)
    return sinusoid_noise_i32(n_ch, n, seed=seed).astype(np.int64) * 70001 + rng.integers(-9, 10, (n_ch, n))


def _f64(n_ch, n, seed):
    rng = np.random.default_rng(seed + 1)
    return sinusoid_noise_f32(n_ch, n, seed=seed).astype(np.float64) + 1e-9 * rng.normal(0.0, 1.0, (n_ch, n))


def _store(fa, torch, x, level=5, **kw):
    """Exact-size device store (compressed, starts, nbytes) of a numpy int array, made on the default stream."""
    comp, st, nb = fa.encode_flac_device(_dev(torch, x), level=level, compact=True, **kw)[:3]
    torch.cuda.synchronize()
    return comp, st.reshape(-1).contiguous(), nb.reshape(-1).contiguous()


def _pair(torch, a, b, *more):
    """Real and decoy input lists of two stores: the blobs in buffers of one size, then starts, nbytes and `more`
    (pairs of further per-store tensors: offsets, gains, new samples)."""
    size = max(a[0].numel(), b[0].numel())
    real = [T.pad_blob(torch, a[0], size), a[1], a[2]] + [m[0] for m in more]
    decoy = [T.pad_blob(torch, b[0], size), b[1], b[2]] + [m[1] for m in more]
    return real, decoy


# ------------------------------------------------------------------------------------------------------------ encode

ENCODE = [  # name, dtype, streams, samples, level, K3F asked for
    ("k3f_whole", "i32", 8, 16384, 5, True),
    ("k3f_tail", "i32", 8, 9192, 5, True),
    ("k3g_level1", "i32", 8, 5000, 1, False),
    ("k3g_odd", "i32", 12, 1000, 5, False),
    ("k3g_int64", "i64", 6, 9000, 5, False),
]


@pytest.mark.parametrize("name,dt,ns,n,level,k3f", ENCODE, ids=[c[0] for c in ENCODE])
def test_encode(fa, torch, side, oracle, monkeypatch, name, dt, ns, n, level, k3f):
    if k3f:
        monkeypatch.setenv("FLACARRAY_HIP_PLACED_BELOW", "0")
    gen = sinusoid_noise_i32 if dt == "i32" else _i64
    x, y = gen(ns, n, seed=11), gen(ns, n, seed=12)
    got, _ = T.run_delayed("encode_" + name, side, [_dev(torch, x)], [_dev(torch, y)], lambda d: fa.encode_flac_device(d, level=level))
    blob_o, st_o, nb_o = (oracle.encode_i32 if dt == "i32" else oracle.encode_i64)(x, level)
    assert np.array_equal(got[0], blob_o) and np.array_equal(got[1], st_o) and np.array_equal(got[2], nb_o)


OPTIONS = ["compact", "return_info", "verify", "md5"]


@pytest.mark.parametrize("route", ["k3f_tail", "k3g_level1"])
@pytest.mark.parametrize("option", OPTIONS)
def test_encode_options(fa, torch, side, oracle, monkeypatch, option, route):
    ns, n, level = (8, 9192, 5) if route == "k3f_tail" else (8, 5000, 1)
    if route == "k3f_tail":
        monkeypatch.setenv("FLACARRAY_HIP_PLACED_BELOW", "0")
    x, y = sinusoid_noise_i32(ns, n, seed=21), sinusoid_noise_i32(ns, n, seed=22)
    got, _ = T.run_delayed(f"encode_{option}_{route}", side, [_dev(torch, x)], [_dev(torch, y)],
                           lambda d: fa.encode_flac_device(d, level=level, **{option: True}))
    blob_o, st_o, nb_o = oracle.encode_i32(x, level)
    assert np.array_equal(got[1], st_o) and np.array_equal(got[2], nb_o)
    if option == "md5":  # the oracle's bytes with the sixteen signature bytes of every stream
        for s in range(ns):
            blob_o[st_o[s] + 26 : st_o[s] + 42] = np.frombuffer(hashlib.md5(x[s].tobytes()).digest(), np.uint8)
    assert np.array_equal(got[0], blob_o)
    if option == "return_info":
        keys = ["type", "order", "porder", "wasted", "shift", "precision", "nbytes", "blocksize"]
        want = [[f[k] for k in keys] for s in range(ns) for f in oracle.stream_info(x[s], level)]
        assert np.array_equal(got[3], np.array(want, dtype=np.int32))


@pytest.mark.parametrize("name,dt,ns,n,level,k3f", ENCODE[:3], ids=[c[0] for c in ENCODE[:3]])
def test_encode_workspace_written_on_the_stream(fa, torch, side, oracle, monkeypatch, name, dt, ns, n, level, k3f):
    """A caller-owned EncodeWorkspace is an input of the call as well: what the stream writes into it in front of the call
    must be cleared BY the call, in stream order.  Both the real and the decoy content are what a finished encode of the same
    geometry left there (every publish word set, the ticket counter run out): run_delayed's default-stream calls write into
    the tensors they are given, so at the time the targets are cloned the decoy holds the leftovers of the encode of the decoy
    samples and the real content those of the real samples.  A call whose clearing memset is not on the caller's stream
    clears too early, finds every frame already handed out once the producer has run, and returns stale bytes."""
    from flacarray_amd.libflacarray import EncodeWorkspace

    if k3f:
        monkeypatch.setenv("FLACARRAY_HIP_PLACED_BELOW", "0")
    x, y = sinusoid_noise_i32(ns, n, seed=13), sinusoid_noise_i32(ns, n, seed=14)
    ws = EncodeWorkspace()
    fa.encode_flac_device(_dev(torch, y), level=level, workspace=ws)
    torch.cuda.synchronize()
    used = ws.buf.clone()
    assert bool((used != 0).any())
    got, _ = T.run_delayed("encode_workspace_" + name, side, [_dev(torch, x), used], [_dev(torch, y), torch.zeros_like(used)],
                           lambda d, w: fa.encode_flac_device(d, level=level, workspace=_workspace_over(EncodeWorkspace, w)))
    blob_o, st_o, nb_o = oracle.encode_i32(x, level)
    assert np.array_equal(got[0], blob_o) and np.array_equal(got[1], st_o) and np.array_equal(got[2], nb_o)


def _workspace_over(cls, buf):
    ws = cls()
    ws.buf = buf
    return ws


@pytest.mark.parametrize("route", ["fused", "two_step"])
@pytest.mark.parametrize("how", ["quanta", "precision"])
@pytest.mark.parametrize("wide", [False, True], ids=["f32", "f64"])
def test_encode_float(fa, torch, side, oracle, monkeypatch, wide, how, route):
    """encode_flac_device_f32 / _f64 with quanta= (a device tensor: an input like the data) and with precision= (std on
    the device).  `fused`: 8 x 16384 sent to K3F, where float32 is quantised in the staging load; `two_step`: 8 x 5000.
    The expected quanta of the precision= cases come from the package's own host expression (utils._quanta_for, numpy's std):
    this is a stream-order test, the precision -> quanta mapping is pinned independently in tests/test_gpu_device_float.py
    and tests/test_gpu_float_edges.py.  Quantisation and encoding of the expected result are the oracle's."""
    ns, n = (8, 16384) if route == "fused" else (8, 5000)
    monkeypatch.setenv("FLACARRAY_HIP_PLACED_BELOW", "0")
    gen, ndt = (_f64, np.float64) if wide else (sinusoid_noise_f32, np.float32)
    enc = fa.encode_flac_device_f64 if wide else fa.encode_flac_device_f32
    x, y = gen(ns, n, seed=31), gen(ns, n, seed=32) * ndt(1.5)
    if how == "quanta":
        q = (1e-4 * (1.0 + np.arange(ns) / 10.0)).astype(ndt)
        real, decoy = [_dev(torch, x), _dev(torch, q)], [_dev(torch, y), _dev(torch, q * ndt(3))]
        call = lambda d, qd: enc(d, quanta=qd, level=5)  # noqa: E731
    else:
        from flacarray_amd.utils import _quanta_for

        q = _quanta_for(x, (ns,), None, 3)
        real, decoy = [_dev(torch, x)], [_dev(torch, y)]
        call = lambda d: enc(d, precision=3, level=5)  # noqa: E731
    got, _ = T.run_delayed(f"encode_{'f64' if wide else 'f32'}_{how}_{route}", side, real, decoy, call)
    ints, off, gain = (oracle.float64_to_int64 if wide else oracle.float32_to_int32)(x, q)
    blob_o, st_o, nb_o = (oracle.encode_i64 if wide else oracle.encode_i32)(ints, 5)
    assert np.array_equal(got[0], blob_o) and np.array_equal(got[1], st_o) and np.array_equal(got[2], nb_o)
    assert got[3].tobytes() == off.tobytes() and got[4].tobytes() == gain.tobytes()


# ----------------------------------------------------------------------------------------- quantise and statistics

@pytest.mark.parametrize("with_quanta", [False, True], ids=["range", "quanta"])
@pytest.mark.parametrize("wide", [False, True], ids=["f32", "f64"])
def test_quantise(fa, torch, side, oracle, wide, with_quanta):
    ns, n = 6, 5001
    gen, ndt = (_f64, np.float64) if wide else (sinusoid_noise_f32, np.float32)
    fn = fa.float64_to_int64_device if wide else fa.float32_to_int32_device
    x, y = gen(ns, n, seed=41), gen(ns, n, seed=42) * ndt(1.5)
    q = (1e-3 * (1.0 + np.arange(ns))).astype(ndt) if with_quanta else None
    real, decoy = [_dev(torch, x)], [_dev(torch, y)]
    if with_quanta:
        real.append(_dev(torch, q))
        decoy.append(_dev(torch, q * ndt(3)))
    got, _ = T.run_delayed(f"quantise_{'f64' if wide else 'f32'}_{'q' if with_quanta else 'r'}", side, real, decoy, lambda d, qd=None: fn(d, qd))
    ints, off, gain = (oracle.float64_to_int64 if wide else oracle.float32_to_int32)(x, q)
    assert np.array_equal(got[0], ints) and got[1].tobytes() == off.tobytes() and got[2].tobytes() == gain.tobytes()


@pytest.mark.parametrize("wide", [False, True], ids=["f32", "f64"])
def test_std(fa, torch, side, wide):
    ns, n = 6, 20001  # (three summation chunks of 8192 per stream, the last one short)
    gen = _f64 if wide else sinusoid_noise_f32
    x, y = gen(ns, n, seed=51), gen(ns, n, seed=52)
    got, _ = T.run_delayed(f"std_{'f64' if wide else 'f32'}", side, [_dev(torch, x)], [_dev(torch, y)], lambda d: fa.std_device(d))
    assert got.tobytes() == np.std(x, axis=-1).tobytes()


# ------------------------------------------------------------------------------------------------------------ decode

def _int_stores(fa, torch, ns, n, level, seeds=(61, 62), wide=False, strip=False):
    gen = _i64 if wide else sinusoid_noise_i32
    x, y = gen(ns, n, seed=seeds[0]), gen(ns, n, seed=seeds[1])
    a, b = _store(fa, torch, x, level), _store(fa, torch, y, level)
    if strip:
        a, b = [tuple(_dev(torch, t) for t in strip_seektable(s[0].cpu().numpy(), s[1].cpu().numpy(), s[2].cpu().numpy())) for s in (a, b)]
    return x, y, a, b


DECODE = [  # name, streams, samples, level, (first, last), int64, without SEEKTABLE
    ("whole", 8, 9192, 5, (-1, -1), False, False),
    ("range", 8, 9192, 5, (1000, 8500), False, False),
    ("level1_range", 6, 5000, 1, (1151, 3457), False, False),
    ("int64", 6, 9000, 5, (-1, -1), True, False),
    ("int64_range", 6, 9000, 5, (4000, 8999), True, False),
    ("scan_walk", 8, 9192, 5, (-1, -1), False, True),
    ("scan_walk_range", 8, 9192, 5, (4097, 9000), False, True),
]


@pytest.mark.parametrize("latency", ["auto", "k7"])
@pytest.mark.parametrize("name,ns,n,level,rng_,wide,strip", DECODE, ids=[c[0] for c in DECODE])
def test_decode(fa, torch, side, monkeypatch, name, ns, n, level, rng_, wide, strip, latency):
    """decode_flac_device, by the latency decoder (K7L takes launches this small on its own) and by K7."""
    if latency == "k7":
        monkeypatch.setenv("FLACARRAY_HIP_LATENCY", "0")
    x, _, a, b = _int_stores(fa, torch, ns, n, level, wide=wide, strip=strip)
    real, decoy = _pair(torch, a, b)
    got, _ = T.run_delayed(f"decode_{name}_{latency}", side, real, decoy,
                           lambda c, st, nb: fa.decode_flac_device(c, st, nb, n, rng_[0], rng_[1], is_int64=wide))
    assert np.array_equal(got, x if rng_[0] < 0 else x[:, rng_[0] : rng_[1]])


@pytest.mark.parametrize("latency", ["auto", "k7"])
@pytest.mark.parametrize("wide", [False, True], ids=["f32", "f64"])
def test_decode_restore(fa, torch, side, oracle, monkeypatch, wide, latency):
    """Decode with offsets and gains: float32 from one-channel streams, float64 from two-channel ones.  The offsets and
    gains are inputs of the call like the bytes, and the decoy has its own."""
    if latency == "k7":
        monkeypatch.setenv("FLACARRAY_HIP_LATENCY", "0")
    ns, n, lo, hi = 6, 9000, 777, 8300
    gen = _f64 if wide else sinusoid_noise_f32
    quant, restore = (oracle.float64_to_int64, oracle.int64_to_float64) if wide else (oracle.float32_to_int32, oracle.int32_to_float32)
    stores, more, ints = [], [[], []], []
    for k, seed in enumerate((71, 72)):
        i, off, gain = quant(gen(ns, n, seed=seed) * (1.0 + k))
        ints.append((i, off, gain))
        stores.append(_store(fa, torch, i))
        more[0].append(_dev(torch, off))
        more[1].append(_dev(torch, gain))
    real, decoy = _pair(torch, stores[0], stores[1], more[0], more[1])
    got, _ = T.run_delayed(f"decode_restore_{'f64' if wide else 'f32'}_{latency}", side, real, decoy,
                           lambda c, st, nb, off, gain: fa.decode_flac_device(c, st, nb, n, lo, hi, offsets=off, gains=gain, is_int64=wide))
    assert got.tobytes() == np.ascontiguousarray(restore(*ints[0])[:, lo:hi]).tobytes()


SLICES = (np.array([5, 0, 3, 3, 7]), np.array([0, 4090, 8000, 100, 9191]), np.array([9192, 20, 1192, 4096, 1]))


@pytest.mark.parametrize("latency", ["auto", "k7"])
def test_decode_slices(fa, torch, side, monkeypatch, latency):
    if latency == "k7":
        monkeypatch.setenv("FLACARRAY_HIP_LATENCY", "0")
    ns, n = 8, 9192
    x, _, a, b = _int_stores(fa, torch, ns, n, 5)
    real, decoy = _pair(torch, a, b)
    got, _ = T.run_delayed(f"decode_slices_{latency}", side, real, decoy, lambda c, st, nb: fa.decode_slices_device(c, st, nb, n, *SLICES)[0])
    assert np.array_equal(got, np.concatenate([x[s, f : f + c] for s, f, c in zip(*SLICES)]))


def _verbatim_pair(fa, torch, ns, n, level=5):
    """Two stores of full-range samples: every frame VERBATIM, so both have the same starts, nbytes and frame offsets and
    ONE decode index describes either -- which lets the bytes under an index be a delayed input without the index ever
    pointing into a store it was not built from."""
    x, y = full_range_i32((ns, n), seed=81), full_range_i32((ns, n), seed=82)
    a, b = _store(fa, torch, x, level), _store(fa, torch, y, level)
    assert a[0].numel() == b[0].numel() and torch.equal(a[1], b[1]) and torch.equal(a[2], b[2])
    return x, y, a, b


INDEXED = ["decode", "decode_range", "slices", "slices_host_small", "slices_host_pinned"]


@pytest.mark.parametrize("latency", ["auto", "k7"])
@pytest.mark.parametrize("what", INDEXED)
def test_indexed_decode(fa, torch, side, monkeypatch, what, latency):
    """DeviceDecodeIndex.decode / decode_slices with the index built on the DEFAULT stream, over the buffer while it holds
    the real store, and used on the side stream behind the producer: in between the decoy store (same layout, so the same
    index describes it) is copied into the buffer.  `slices_host_small` lands in the library's pinned
    buffer (to_host=True, a few KB), `slices_host_pinned` in a block of the binding's pinned pool (64 KB and more)."""
    if latency == "k7":
        monkeypatch.setenv("FLACARRAY_HIP_LATENCY", "0")
    ns, n = 8, 9192
    x, y, a, b = _verbatim_pair(fa, torch, ns, n)
    sl = SLICES if what != "slices_host_pinned" else (np.arange(8), np.zeros(8, np.int64), np.full(8, 9192))
    st, nb = a[1], a[2]

    def use(index):
        if what == "decode":
            return index.decode()
        if what == "decode_range":
            return index.decode(1000, 8500)
        return index.decode_slices(*sl, to_host=what.startswith("slices_host"))[0]

    def want(z):
        if what == "decode":
            return z
        if what == "decode_range":
            return z[:, 1000:8500]
        return np.concatenate([z[s, f : f + c] for s, f, c in zip(*sl)])

    name = f"indexed_{what}_{latency}"
    buf = a[0].clone()
    index = fa.DeviceDecodeIndex(buf, st, nb, n)
    torch.cuda.synchronize()
    expected = T.to_host(use(index))
    assert np.array_equal(expected, want(x))
    t0 = time.perf_counter()
    use(index)
    torch.cuda.synchronize()
    T.WARM_SECONDS[name] = time.perf_counter() - t0
    buf.copy_(b[0])  # the decoy, under the same index
    torch.cuda.synchronize()
    assert np.array_equal(T.to_host(use(index)), want(y)) and not T.same(want(y), want(x))
    with torch.cuda.stream(side):
        ev = T.delayed_fill(side, [(buf, a[0])])
        assert not ev.query(), "the producer had finished before the call was made; lengthen the delay"
        out = use(index)
        out = out.clone() if isinstance(out, torch.Tensor) else np.array(out, copy=True)
    side.synchronize()
    assert T.same(T.to_host(out), expected)
    index.close()


def test_index_built_on_side_stream_used_on_default(fa, torch, side):
    """The reverse: the index is created on the side stream behind the producer (the call waits for its stream: the tables
    are complete when it returns) and read on the default stream."""
    ns, n = 8, 9192
    x, y, a, b = _verbatim_pair(fa, torch, ns, n)
    buf = b[0].clone()
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        ev = T.delayed_fill(side, [(buf, a[0])])
        assert not ev.query(), "the producer had finished before the call was made; lengthen the delay"
        index = fa.DeviceDecodeIndex(buf, a[1], a[2], n)
    assert ev.query(), "fa_decode_index_create returned before the work queued in front of it on its stream was done"
    out = index.decode()
    flat = index.decode_slices(*SLICES)[0]
    torch.cuda.synchronize()
    assert np.array_equal(out.cpu().numpy(), x)
    assert np.array_equal(flat.cpu().numpy(), np.concatenate([x[s, f : f + c] for s, f, c in zip(*SLICES)]))
    index.close()


# --------------------------------------------------------------------------------------------- compare, sign, update

@pytest.mark.parametrize("case", ["equal", "one_sample"])
@pytest.mark.parametrize("wide", [False, True], ids=["i32", "i64"])
def test_compare(fa, torch, side, wide, case):
    """compare_flac_device: the store and the samples are both inputs.  The decoy is another store with samples that match
    NEITHER store, so reading either input early reports differences the real pair does not have."""
    ns, n = 6, 9000
    x, _, a, b = _int_stores(fa, torch, ns, n, 5, wide=wide)
    z = (_i64 if wide else sinusoid_noise_i32)(ns, n, seed=63)
    data = x.copy()
    want = np.full(ns, -1, dtype=np.int64)
    if case == "one_sample":
        data[4, 4321] += 1
        want[4] = 4321
    real, decoy = _pair(torch, a, b, (_dev(torch, data), _dev(torch, z)))
    got, _ = T.run_delayed(f"compare_{case}_{'i64' if wide else 'i32'}", side, real, decoy, lambda c, st, nb, d: fa.compare_flac_device(c, st, nb, d))
    assert np.array_equal(got, want)


@pytest.mark.parametrize("resumed", [False, True], ids=["one_shot", "resumed"])
@pytest.mark.parametrize("wide", [False, True], ids=["i32", "i64"])
def test_md5(fa, torch, side, wide, resumed):
    ns, n, k = 6, 5003, 2048
    gen = _i64 if wide else sinusoid_noise_i32
    x, y = gen(ns, n, seed=91), gen(ns, n, seed=92)

    def call(d):
        if not resumed:
            return fa.md5_device(d)
        state = fa.md5_device(d[:, :k], final=False)
        return fa.md5_device(d[:, k:], state=state, n_before=k)

    got, _ = T.run_delayed(f"md5_{'i64' if wide else 'i32'}_{'resumed' if resumed else 'one'}", side, [_dev(torch, x)], [_dev(torch, y)], call)
    assert np.array_equal(got, np.array([np.frombuffer(hashlib.md5(x[s].tobytes()).digest(), np.uint8) for s in range(ns)]))


def test_sign_streams(fa, torch, side, oracle):
    """sign_streams_device patches its first argument in place: the bytes, the starts and the digests are all delayed."""
    ns, n = 8, 5000
    x, y, a, b = _int_stores(fa, torch, ns, n, 5)
    dig = [np.array([np.frombuffer(hashlib.md5(z[s].tobytes()).digest(), np.uint8) for s in range(ns)]) for z in (x, y)]
    real, decoy = _pair(torch, a, b, (_dev(torch, dig[0]), _dev(torch, dig[1])))
    real, decoy = [real[0], real[1], real[3]], [decoy[0], decoy[1], decoy[3]]
    got, _ = T.run_delayed("sign_streams", side, real, decoy, lambda c, st, d: fa.sign_streams_device(c, st, d))
    blob_o, st_o, _ = oracle.encode_i32(x, 5)
    for s in range(ns):
        blob_o[st_o[s] + 26 : st_o[s] + 42] = dig[0][s]
    assert np.array_equal(got[: blob_o.size], blob_o)


@pytest.mark.parametrize("wide", [False, True], ids=["i32", "i64"])
def test_check_md5(fa, torch, side, wide):
    """check_md5_device on signed stores; the second real stream carries a wrong signature, so the status differs from the
    decoy's as well as the digests."""
    ns, n = 6, 9000
    gen = _i64 if wide else sinusoid_noise_i32
    x, y = gen(ns, n, seed=93), gen(ns, n, seed=94)
    a, b = _store(fa, torch, x, md5=True), _store(fa, torch, y, md5=True)
    a[0][int(a[1][1]) + 30] ^= 0x40  # (inside STREAMINFO's MD5 field: the frames are as they were)
    torch.cuda.synchronize()
    real, decoy = _pair(torch, a, b)
    got, _ = T.run_delayed(f"check_md5_{'i64' if wide else 'i32'}", side, real, decoy,
                           lambda c, st, nb: fa.check_md5_device(c, st, nb, n, is_int64=wide, return_digests=True, max_temp_bytes=ns * 4096 * 8))
    assert np.array_equal(got[0], np.array([1, 0, 1, 1, 1, 1], dtype=np.int8))
    assert np.array_equal(got[1], np.array([np.frombuffer(hashlib.md5(x[s].tobytes()).digest(), np.uint8) for s in range(ns)]))


@pytest.mark.parametrize("wide", [False, True], ids=["i32", "i64"])
def test_append(fa, torch, side, oracle, wide):
    ns, n, m = 6, 9000, 5000
    gen = _i64 if wide else sinusoid_noise_i32
    x, y, a, b = _int_stores(fa, torch, ns, n, 5, wide=wide)
    xa, ya = gen(ns, m, seed=64), gen(ns, m, seed=65)
    real, decoy = _pair(torch, a, b, (_dev(torch, xa), _dev(torch, ya)))
    got, _ = T.run_delayed(f"append_{'i64' if wide else 'i32'}", side, real, decoy, lambda c, st, nb, d: fa.append_flac_device(c, st, nb, n, d, level=5))
    blob_o, st_o, nb_o = (oracle.encode_i64 if wide else oracle.encode_i32)(np.concatenate([x, xa], axis=1), 5)
    assert np.array_equal(got[0], blob_o) and np.array_equal(got[1], st_o) and np.array_equal(got[2], nb_o)


@pytest.mark.parametrize("streams", [None, [4, 1]], ids=["all", "streams"])
@pytest.mark.parametrize("wide", [False, True], ids=["i32", "i64"])
def test_overwrite(fa, torch, side, oracle, wide, streams):
    ns, n, first, m = 6, 9000, 3000, 2500
    gen = _i64 if wide else sinusoid_noise_i32
    x, y, a, b = _int_stores(fa, torch, ns, n, 5, wide=wide)
    rows = ns if streams is None else len(streams)
    xa, ya = gen(rows, m, seed=66), gen(rows, m, seed=67)
    real, decoy = _pair(torch, a, b, (_dev(torch, xa), _dev(torch, ya)))
    got, _ = T.run_delayed(f"overwrite_{'i64' if wide else 'i32'}_{'all' if streams is None else 'some'}", side, real, decoy,
                           lambda c, st, nb, d: fa.overwrite_flac_device(c, st, nb, n, first, d, streams=streams, level=5))
    patched = x.copy()
    patched[slice(None) if streams is None else streams, first : first + m] = xa
    blob_o, st_o, nb_o = (oracle.encode_i64 if wide else oracle.encode_i32)(patched, 5)
    assert np.array_equal(got[0], blob_o) and np.array_equal(got[1], st_o) and np.array_equal(got[2], nb_o)


# --------------------------------------------------------------------------------------------------------- FlacArray

def _flacarray_sequence(fa, torch, xd, ad, od, resident):
    """from_device_array, append, overwrite, read_slices, first_mismatch, check_md5, sign, check_md5 on the CURRENT stream;
    returns everything the sequence can show, as host values."""
    arr = fa.FlacArray.from_device_array(xd, level=5)
    if not resident:
        arr.release_device()
    arr.append(ad, level=5)
    arr.overwrite(3000, od, streams=[4, 1], level=5)
    n = arr.shape[-1]
    reads = arr.read_slices(np.array([5, 0, 3]), np.array([0, 4090, n - 1200]), np.array([n, 20, 1200]))
    whole = torch.cat([xd, ad], dim=1)
    whole[torch.tensor([4, 1], device=xd.device), 3000 : 3000 + od.shape[1]] = od
    mism = arr.first_mismatch(whole)
    unsigned = arr.check_md5()
    arr.sign()
    signed = arr.check_md5()
    assert arr.is_resident == resident
    return {"compressed": np.array(arr.compressed), "starts": np.array(arr.stream_starts), "nbytes": np.array(arr.stream_nbytes),
            "reads": [np.array(r) for r in reads], "mismatch": mism, "unsigned": unsigned, "signed": signed, "whole": whole.cpu().numpy()}


@pytest.mark.parametrize("resident", [True, False], ids=["resident", "host"])
def test_flacarray_end_to_end(fa, torch, side, oracle, resident):
    ns, n = 6, 9000
    x, xa, xo = sinusoid_noise_i32(ns, n, seed=101), sinusoid_noise_i32(ns, 5000, seed=102), sinusoid_noise_i32(2, 2500, seed=103)
    inputs = [_dev(torch, x), _dev(torch, xa), _dev(torch, xo)]
    torch.cuda.synchronize()
    want = _flacarray_sequence(fa, torch, *inputs, resident)
    torch.cuda.synchronize()
    decoys = [_dev(torch, sinusoid_noise_i32(*t.shape, seed=110 + k)) for k, t in enumerate(inputs)]
    targets = [d.clone() for d in decoys]
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        ev = T.delayed_fill(side, list(zip(targets, inputs)))
        assert not ev.query(), "the producer had finished before the call was made; lengthen the delay"
        got = _flacarray_sequence(fa, torch, *targets, resident)
    side.synchronize()
    for k in want:
        assert T.same(T.to_host(got[k]), T.to_host(want[k])), k
    blob_o, st_o, nb_o = oracle.encode_i32(want["whole"], 5)
    for s in range(ns):
        blob_o[st_o[s] + 26 : st_o[s] + 42] = np.frombuffer(hashlib.md5(want["whole"][s].tobytes()).digest(), np.uint8)
    assert np.array_equal(got["compressed"], blob_o) and np.array_equal(got["starts"], st_o) and np.array_equal(got["nbytes"], nb_o)
    assert np.all(got["mismatch"] == -1) and np.all(got["unsigned"] == -1) and np.all(got["signed"] == 1)
    for r, (s, f, c) in zip(got["reads"], [(5, 0, 14000), (0, 4090, 20), (3, 14000 - 1200, 1200)]):
        assert np.array_equal(r, want["whole"][s, f : f + c])


# ------------------------------------------------------------------------------------------------- alternating streams

def test_alternating_streams(fa, torch, oracle, monkeypatch):
    """A dozen calls interleaved over two side streams and the default stream, no device-wide synchronisation between them:
    K3F encodes of two geometries (whole frames; a short last frame), so the shared frame-header table is uploaded again
    from another stream while the tail kernels of the previous call may still be queued, and decodes of what was just
    written.  Every call's input is produced, and its outputs are consumed, on its own stream; every result is the
    oracle's."""
    monkeypatch.setenv("FLACARRAY_HIP_PLACED_BELOW", "0")
    geoms = [(8, 16384), (8, 9192)]
    base = [sinusoid_noise_i32(ns, n, seed=120 + g) for g, (ns, n) in enumerate(geoms)]
    base_d = [_dev(torch, b) for b in base]
    for b in base_d:  # warm: windows, tables and scratch of both geometries exist before the interleaving starts
        fa.decode_flac_device(*fa.encode_flac_device(b, level=5), b.shape[1])
    torch.cuda.synchronize()
    streams = [torch.cuda.Stream(), torch.cuda.Stream(), torch.cuda.default_stream()]
    done = []
    for k in range(12):
        g, s = k % 2, streams[(k * 2 + k // 3) % 3]
        with torch.cuda.stream(s):
            xd = base_d[g] + k  # (produced on s)
            comp, st, nb = fa.encode_flac_device(xd, level=5)
            y = fa.decode_flac_device(comp, st, nb, xd.shape[1], verify=(k % 4 == 3))
            done.append((k, g, s, xd, comp.clone(), st.clone(), nb.clone(), y.clone()))
    for s in streams:
        s.synchronize()
    assert len({id(d[2]) for d in done}) == 3
    for k, g, s, xd, comp, st, nb, y in done:
        x = base[g] + np.int32(k)
        blob_o, st_o, nb_o = oracle.encode_i32(x, 5)
        assert np.array_equal(comp.cpu().numpy(), blob_o), k
        assert np.array_equal(st.cpu().numpy(), st_o) and np.array_equal(nb.cpu().numpy(), nb_o), k
        assert np.array_equal(y.cpu().numpy(), x), k


# ------------------------------------------------------------------------------------------------------ beside-verify

# 128 streams x 128 frames of 1152 samples: 16384 tasks, exactly the threshold `a.n_tasks >= 16384` of the `beside` decision in
# decode_device_impl (flacarray_amd/csrc/flacarray_hip.hip); far above the 4096 frames the latency decoder takes, so the launch
# goes to K7.  If that literal is raised, raise the stream count with it: below the threshold all four variants of the
# test take the after-K7 path and still pass.
BESIDE_NS, BESIDE_N, BESIDE_BAD = 128, 147456, 64


@pytest.fixture(scope="module")
def beside(fa, torch):
    """Full-range samples (every frame VERBATIM: a flipped payload bit changes one sample and cannot desynchronise the
    parse), encoded on the GPU at level 1; a decoy store of the same layout; the real store with one bit flipped 1000
    bytes before the end of stream 64."""
    x = _dev(torch, full_range_i32((BESIDE_NS, BESIDE_N), seed=131))
    y = x ^ 0x55555555
    a = fa.encode_flac_device(x, level=1, compact=True)
    b = fa.encode_flac_device(y, level=1, compact=True)
    torch.cuda.synchronize()
    assert a[0].numel() == b[0].numel() and torch.equal(a[1], b[1]) and torch.equal(a[2], b[2])
    assert BESIDE_NS * ((BESIDE_N + 1151) // 1152) == 16384
    bad = a[0].clone()
    pos = int(a[1][BESIDE_BAD]) + int(a[2][BESIDE_BAD]) - 1000
    bad[pos] ^= 0x10
    off = torch.zeros(BESIDE_NS, dtype=torch.float32, device="cuda")
    gain = torch.full((BESIDE_NS,), 0.5, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    return {"x": x, "y": y, "good": a[0], "decoy": b[0], "bad": bad, "st": a[1], "nb": a[2], "off": off, "gain": gain}


@pytest.mark.parametrize("after", [False, True], ids=["beside", "after_k7"])
@pytest.mark.parametrize("on_side", [False, True], ids=["default_stream", "side_stream"])
def test_verified_decode_of_16384_frames(fa, torch, side, beside, monkeypatch, on_side, after):
    """The frame CRC-16 check of a decode of 16384 tasks runs on the library's own low-priority stream beside K7, tied to the
    caller's stream by two events (FLACARRAY_HIP_VERIFY_AFTER=1: after K7, on the caller's stream).  Either way, on either
    kind of caller stream: an intact store decodes to its input, a flipped bit raises, without verification the damage
    shows in its stream alone, and the float32-restoring decoder raises as well.  On the side stream every store is a
    delayed input over a valid decoy: the intact store of other samples, or -- for the damaged store -- the intact one,
    which does not raise."""
    if after:
        monkeypatch.setenv("FLACARRAY_HIP_VERIFY_AFTER", "1")
    B = beside
    st, nb, n = B["st"], B["nb"], BESIDE_N
    buf = torch.empty_like(B["good"])
    # warm calls on the default stream, as in every other case: the library's check stream, its tables and every scratch slot
    # exist before a measured call is made (a slot that grows waits for the device, which would hide a missing dependency)
    for kw in ({}, {"offsets": B["off"], "gains": B["gain"]}):
        fa.decode_flac_device(B["good"], st, nb, n, verify=True, **kw)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fa.decode_flac_device(B["good"], st, nb, n, verify=True)
    torch.cuda.synchronize()
    T.WARM_SECONDS[f"verified_decode_16384_{'after' if after else 'beside'}"] = time.perf_counter() - t0

    def staged(real, decoy, call):
        """`call(buf)` with buf = real: directly on the default stream, behind the delayed producer on the side stream."""
        if not on_side:
            buf.copy_(real)
            torch.cuda.synchronize()
            return call(buf)
        buf.copy_(decoy)
        torch.cuda.synchronize()
        with torch.cuda.stream(side):
            ev = T.delayed_fill(side, [(buf, real)])
            assert not ev.query(), "the producer had finished before the call was made; lengthen the delay"
            try:
                out = call(buf)
                return None if out is None else out.clone()
            finally:
                side.synchronize()

    y = staged(B["good"], B["decoy"], lambda c: fa.decode_flac_device(c, st, nb, n, verify=True))
    torch.cuda.synchronize()
    assert torch.equal(y, B["x"])
    with pytest.raises(RuntimeError, match="Decoding failed"):
        staged(B["bad"], B["good"], lambda c: fa.decode_flac_device(c, st, nb, n, verify=True))
    y = staged(B["bad"], B["decoy"], lambda c: fa.decode_flac_device(c, st, nb, n, verify=False))
    torch.cuda.synchronize()
    rows = (y != B["x"]).any(dim=1).nonzero().reshape(-1).tolist()
    assert rows == [BESIDE_BAD]
    assert int((y[BESIDE_BAD] != B["x"][BESIDE_BAD]).sum()) == 1
    with pytest.raises(RuntimeError, match="Decoding failed"):
        staged(B["bad"], B["good"], lambda c: fa.decode_flac_device(c, st, nb, n, offsets=B["off"], gains=B["gain"], verify=True))
    # and the float32 restore of the intact store, checked, is the restore of its input
    z = staged(B["good"], B["decoy"], lambda c: fa.decode_flac_device(c, st, nb, n, offsets=B["off"], gains=B["gain"], verify=True))
    torch.cuda.synchronize()
    want = fa.decode_flac_device(B["good"], st, nb, n, offsets=B["off"], gains=B["gain"], verify=False)
    torch.cuda.synchronize()
    assert torch.equal(z.view(torch.int32), want.view(torch.int32))
