"""The state that surrounds a device call: scratch the caller hands over as it finds it, one workspace reused across
geometries and routes, and the per-device caches that outlive a call (the frame-header table of the encoders, keyed by
frame count, block size, tail length, channel count, address and scratch epoch; the grow-only scratch slots of the decoders).

A stale table or a word of scratch that is read before it is written gives wrong bytes with return code 0, so every step
of every sequence here is compared with the oracle's bytes (encoders) or with numpy slices of the input (decoders).
"""
import ctypes

import numpy as np
import pytest

from tests.conftest import sinusoid_noise_f32, sinusoid_noise_i32

pytestmark = pytest.mark.gpu

K3G_ONLY = "1000000000"  # FLACARRAY_HIP_PLACED_BELOW: every array has fewer frames than this, K3G takes them all


@pytest.fixture(scope="module")
def fa():
    import flacarray_amd

    return flacarray_amd


@pytest.fixture(scope="module")
def torch():
    import torch

    return torch


@pytest.fixture(scope="module")
def L():
    from flacarray_amd import _lib

    return _lib.lib()


@pytest.fixture(autouse=True)
def _own_dispatch(monkeypatch):
    for v in ("FLACARRAY_HIP_PLACED_BELOW", "FLACARRAY_HIP_LATENCY", "FLACARRAY_HIP_SLOTS"):
        monkeypatch.delenv(v, raising=False)


def _dev(torch, x):
    return torch.from_numpy(np.ascontiguousarray(x)).cuda()


def _vp(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def _i64(n_ch, n, seed):
    rng = np.random.default_rng(seed)
    return sinusoid_noise_i32(n_ch, n, seed=seed).astype(np.int64) * 70001 + rng.integers(-9, 10, (n_ch, n))


def _f64(n_ch, n, seed):
    rng = np.random.default_rng(seed + 1)
    return sinusoid_noise_f32(n_ch, n, seed=seed).astype(np.float64) + 1e-9 * rng.normal(0.0, 1.0, (n_ch, n))


# A route: (kind, streams, samples, level, FLACARRAY_HIP_PLACED_BELOW or None).  kind: i32 / i64 / f32 / f64.
ROUTES = {
    "k3f_whole": ("i32", 8, 16384, 5, "0"),
    "k3f_tail": ("i32", 8, 9192, 5, "0"),
    "k3g_level1": ("i32", 8, 5000, 1, None),
    "k3g_int64": ("i64", 6, 9000, 5, None),
    "f32_fused": ("f32", 8, 16384, 5, "0"),
    "f64": ("f64", 6, 9000, 5, None),
    # further sizes of the same routes, for the walks over one workspace
    "k3f_whole_big": ("i32", 24, 32768, 5, "0"),
    "k3f_tail_big": ("i32", 16, 12292, 8, "0"),
    "k3g_small": ("i32", 3, 700, 0, None),
    "k3g_int64_big": ("i64", 12, 20000, 5, None),
    "f32_fused_small": ("f32", 4, 8192, 5, "0"),
    "f64_small": ("f64", 3, 3000, 2, None),
}
MAIN = ["k3f_whole", "k3f_tail", "k3g_level1", "k3g_int64", "f32_fused", "f64"]
_GEN = {"i32": sinusoid_noise_i32, "i64": _i64, "f32": sinusoid_noise_f32, "f64": _f64}
_cache = {}


def _case(oracle, name):
    """(input array, oracle result) of a route, computed once: [blob, starts, nbytes] and, for float input, offsets and gains."""
    if name not in _cache:
        kind, ns, n, level, _ = ROUTES[name]
        x = _GEN[kind](ns, n, seed=200 + sorted(ROUTES).index(name))
        tail = []
        ints = x
        if kind == "f32":
            ints, off, gain = oracle.float32_to_int32(x)
            tail = [off, gain]
        elif kind == "f64":
            ints, off, gain = oracle.float64_to_int64(x)
            tail = [off, gain]
        enc = oracle.encode_i32 if kind in ("i32", "f32") else oracle.encode_i64
        _cache[name] = (x, list(enc(ints, level)) + tail)
    return _cache[name]


def _run(fa, torch, monkeypatch, name, xd, ws):
    """The route's Python call with the caller's workspace; the results on the host."""
    kind, ns, n, level, below = ROUTES[name]
    if below is None:
        monkeypatch.delenv("FLACARRAY_HIP_PLACED_BELOW", raising=False)
    else:
        monkeypatch.setenv("FLACARRAY_HIP_PLACED_BELOW", below)
    fn = {"i32": fa.encode_flac_device, "i64": fa.encode_flac_device, "f32": fa.encode_flac_device_f32, "f64": fa.encode_flac_device_f64}[kind]
    out = fn(xd, level=level, workspace=ws)
    torch.cuda.synchronize()
    return [t.cpu().numpy() for t in out]


def _check(got, want, what):
    assert len(got) == len(want), what
    for k, (g, w) in enumerate(zip(got, want)):
        assert g.shape == w.shape and g.tobytes() == w.tobytes(), f"{what}: output {k} differs from the oracle"


def _ws_bytes(L, names, slots=False):
    """The largest workspace any of the routes asks for (single pass, or the slot sequence)."""
    need = 0
    for name in names:
        kind, ns, n, level, _ = ROUTES[name]
        wide = kind in ("i64", "f64")
        if slots:
            fn = L.fa_encode_workspace_bytes_i64 if wide else L.fa_encode_workspace_bytes
        else:
            fn = L.fa_encode_single_pass_workspace_bytes_i64 if wide else L.fa_encode_single_pass_workspace_bytes
        need = max(need, int(fn(ns, n, level)))
    return need + 4096


POISONS = ["zeros", "ones", "a5", "leftovers"]


def _poison(fa, torch, monkeypatch, oracle, L, ws, poison, name, slots=False):
    """Leave `ws` (an EncodeWorkspace) holding a buffer large enough for every route, filled with the poison: a byte value,
    or what a larger encode of ANOTHER route left behind in it."""
    size = _ws_bytes(L, ROUTES, slots)
    if poison == "leftovers":
        other = "k3g_int64_big" if name.startswith(("k3f", "f32")) else "k3f_whole_big"
        ws.buf = torch.full((size,), 0x5A, dtype=torch.uint8, device="cuda")
        x, want = _case(oracle, other)
        _check(_run(fa, torch, monkeypatch, other, _dev(torch, x), ws), want, f"leftover encode {other}")
    else:
        ws.buf = torch.full((size,), {"zeros": 0x00, "ones": 0xFF, "a5": 0xA5}[poison], dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    return ws.buf.data_ptr()


# ----------------------------------------------------------------------------------------------------- dirty workspace

@pytest.mark.parametrize("poison", POISONS)
@pytest.mark.parametrize("name", MAIN)
def test_dirty_workspace(fa, torch, oracle, L, monkeypatch, name, poison):
    """A caller-owned EncodeWorkspace arrives full of zeros, ones, 0xA5 or the leftovers of a larger encode of another
    route: bytes, starts, nbytes (offsets, gains) are the oracle's."""
    from flacarray_amd.libflacarray import EncodeWorkspace

    ws = EncodeWorkspace()
    ptr = _poison(fa, torch, monkeypatch, oracle, L, ws, poison, name)
    x, want = _case(oracle, name)
    _check(_run(fa, torch, monkeypatch, name, _dev(torch, x), ws), want, f"{name} on a workspace of {poison}")
    assert ws.buf.data_ptr() == ptr, "the poisoned buffer was replaced, not used"


@pytest.mark.parametrize("poison", POISONS)
@pytest.mark.parametrize("name", ["k3f_whole", "k3f_tail", "k3g_level1", "k3g_int64", "k3g_small"])
def test_dirty_workspace_slot_sequence(fa, torch, oracle, L, monkeypatch, name, poison):
    """The same through the two-phase slot sequence (fa_encode_*_device_begin / _finish), which FLACARRAY_HIP_SLOTS selects."""
    from flacarray_amd.libflacarray import EncodeWorkspace

    ws = EncodeWorkspace()
    monkeypatch.setenv("FLACARRAY_HIP_SLOTS", "1")
    ptr = _poison(fa, torch, monkeypatch, oracle, L, ws, poison, name, slots=True)
    x, want = _case(oracle, name)
    assert not L.fa_encode_single_pass_supported(*ROUTES[name][1:4])
    _check(_run(fa, torch, monkeypatch, name, _dev(torch, x), ws), want, f"{name} (slots) on a workspace of {poison}")
    assert ws.buf.data_ptr() == ptr, "the poisoned buffer was replaced, not used"


GUARD = 65536


def _info_want(oracle, x, level, wide):
    keys = ["type", "order", "porder", "wasted", "shift", "precision", "nbytes", "blocksize"]
    info = oracle.stream_info_i64 if wide else oracle.stream_info
    return np.array([[f[k] for k in keys] for s in range(x.shape[0]) for f in info(x[s], level)], dtype=np.int32)


@pytest.mark.parametrize("poison", ["zeros", "ones", "a5"])
@pytest.mark.parametrize("name", ["k3f_whole", "k3f_tail", "k3g_level1", "k3g_int64", "f32_fused"])
def test_c_entry_points_on_poisoned_buffers(torch, oracle, L, monkeypatch, name, poison):
    """fa_encode_i32_device / _i64_device / _f32_device called directly: the workspace poisoned, the output buffer full of
    0xA5 with a guard zone behind capacity_bytes, starts / nbytes / info (and offsets / gains) full of 0xFF.  [0, total) is
    the oracle's blob, the guard is untouched, and every index and info word comes back defined (equal to the oracle's)."""
    kind, ns, n, level, below = ROUTES[name]
    if below is not None:
        monkeypatch.setenv("FLACARRAY_HIP_PLACED_BELOW", below)
    wide = kind == "i64"
    x, want = _case(oracle, name)
    ints = oracle.float32_to_int32(x)[0] if kind == "f32" else x
    xd = _dev(torch, x)
    cap = int((L.fa_encode_capacity_bytes_i64 if wide else L.fa_encode_capacity_bytes)(ns, n, level))
    need = int((L.fa_encode_single_pass_workspace_bytes_i64 if wide else L.fa_encode_single_pass_workspace_bytes)(ns, n, level))
    ws = torch.full((need,), {"zeros": 0x00, "ones": 0xFF, "a5": 0xA5}[poison], dtype=torch.uint8, device="cuda")
    buf = torch.full((cap + GUARD,), 0xA5, dtype=torch.uint8, device="cuda")
    want_info = _info_want(oracle, ints, level, wide)
    ff = lambda shape, dt: torch.full(shape, -1, dtype=dt, device="cuda")  # noqa: E731  (every byte 0xFF)
    d_st, d_nb, d_info = ff((ns,), torch.int64), ff((ns,), torch.int64), ff(tuple(want_info.shape), torch.int32)
    total = ctypes.c_int64(-1)
    if kind == "f32":
        d_off = torch.full((ns,), float("nan"), dtype=torch.float32, device="cuda")
        d_gain = torch.full((ns,), float("nan"), dtype=torch.float32, device="cuda")
        rc = L.fa_encode_f32_device(_vp(xd), ns, n, level, None, _vp(ws), need, _vp(buf), cap, _vp(d_st), _vp(d_nb), _vp(d_off), _vp(d_gain),
                                    ctypes.byref(total), _vp(d_info), None)
    else:
        rc = (L.fa_encode_i64_device if wide else L.fa_encode_i32_device)(_vp(xd), ns, n, level, _vp(ws), need, _vp(buf), cap, _vp(d_st), _vp(d_nb),
                                                                         ctypes.byref(total), _vp(d_info), None)
    torch.cuda.synchronize()
    assert rc == 0
    assert total.value == want[0].size
    assert np.array_equal(buf[: total.value].cpu().numpy(), want[0]), "[0, total) is not the oracle's blob"
    assert bool((buf[cap:] == 0xA5).all()), "bytes behind capacity_bytes were written"
    assert np.array_equal(d_st.cpu().numpy(), want[1]) and np.array_equal(d_nb.cpu().numpy(), want[2])
    assert np.array_equal(d_info.cpu().numpy(), want_info), "a frame's info words differ from the oracle's (or were never written)"
    if kind == "f32":
        assert d_off.cpu().numpy().tobytes() == want[3].tobytes() and d_gain.cpu().numpy().tobytes() == want[4].tobytes()


@pytest.mark.parametrize("poison", ["zeros", "ones", "a5"])
@pytest.mark.parametrize("name", ["k3f_tail", "k3g_level1", "k3g_int64"])
def test_c_slot_sequence_on_poisoned_buffers(torch, oracle, L, name, poison):
    """fa_encode_*_device_begin / _finish directly, with the same poisons: begin sizes the blob, finish writes exactly
    [0, total) of a buffer of 0xA5 and nothing behind it."""
    kind, ns, n, level, _ = ROUTES[name]
    wide = kind == "i64"
    x, want = _case(oracle, name)
    xd = _dev(torch, x)
    need = int((L.fa_encode_workspace_bytes_i64 if wide else L.fa_encode_workspace_bytes)(ns, n, level))
    ws = torch.full((need,), {"zeros": 0x00, "ones": 0xFF, "a5": 0xA5}[poison], dtype=torch.uint8, device="cuda")
    want_info = _info_want(oracle, x, level, wide)
    d_st = torch.full((ns,), -1, dtype=torch.int64, device="cuda")
    d_nb = torch.full((ns,), -1, dtype=torch.int64, device="cuda")
    d_info = torch.full(tuple(want_info.shape), -1, dtype=torch.int32, device="cuda")
    total = ctypes.c_int64(-1)
    rc = (L.fa_encode_i64_device_begin if wide else L.fa_encode_i32_device_begin)(_vp(xd), ns, n, level, _vp(ws), need, _vp(d_st), _vp(d_nb),
                                                                                 ctypes.byref(total), _vp(d_info), None)
    assert rc == 0 and total.value == want[0].size
    buf = torch.full((total.value + GUARD,), 0xA5, dtype=torch.uint8, device="cuda")
    rc = (L.fa_encode_i64_device_finish if wide else L.fa_encode_i32_device_finish)(ns, n, level, _vp(ws), _vp(d_st), _vp(buf), None)
    torch.cuda.synchronize()
    assert rc == 0
    assert np.array_equal(buf[: total.value].cpu().numpy(), want[0])
    assert bool((buf[total.value :] == 0xA5).all()), "bytes behind the blob were written"
    assert np.array_equal(d_st.cpu().numpy(), want[1]) and np.array_equal(d_nb.cpu().numpy(), want[2])
    assert np.array_equal(d_info.cpu().numpy(), want_info)


FA_ERROR_ALLOC, FA_ERROR_ENCODE_INIT, FA_ERROR_CONVERT_TYPE = 1 << 0, 1 << 8, 1 << 19  # include/flacarray_hip.h
# refusal -> the entry points it applies to ("single": fa_encode_i32 / _i64 / _f32_device, "begin": fa_encode_*_device_begin)
REFUSALS = {
    "workspace_one_byte_short": ("single", "begin"),
    "null_workspace": ("single", "begin"),
    "null_bytes": ("single",),
    "capacity_below_headers": ("single",),
}


def _refused_call(torch, L, entry, kind, ns, n, level, refusal):
    """One call of `entry` on the geometry with one argument made bad; returns (return code, the poisoned buffers with the
    byte each was filled with).  Everything the call could write is there, full size, so a call that is NOT refused writes
    into memory that is its to write."""
    wide = kind in ("i64", "f64")
    sfx = "_i64" if wide else ""
    dt = {"i32": torch.int32, "i64": torch.int64, "f32": torch.float32, "f64": torch.int64}[kind]
    xd = torch.zeros((ns, n), dtype=dt, device="cuda")
    nf = -(-n // (1152 if level <= 2 else 4096))
    need = int(getattr(L, ("fa_encode_workspace_bytes" if entry == "begin" else "fa_encode_single_pass_workspace_bytes") + sfx)(ns, n, level))
    cap = int(getattr(L, "fa_encode_capacity_bytes" + sfx)(ns, n, level))
    assert need > 0 and cap > 0
    fill = lambda nbytes, v: torch.full((nbytes,), v, dtype=torch.uint8, device="cuda")  # noqa: E731
    ws, buf = fill(need, 0x5A), fill(cap, 0xA5)
    d_st, d_nb, d_info = fill(ns * 8, 0xC3), fill(ns * 8, 0xC3), fill(ns * nf * (2 if wide else 1) * 32, 0xC3)
    d_off, d_gain = fill(ns * 4, 0x3C), fill(ns * 4, 0x3C)
    ws_arg, ws_bytes, buf_arg, cap_arg, off_arg = _vp(ws), need, _vp(buf), cap, _vp(d_off)
    if refusal == "workspace_one_byte_short":
        ws_bytes = need - 1
    elif refusal == "null_workspace":
        ws_arg = None
    elif refusal == "null_bytes":
        buf_arg = None
    elif refusal == "capacity_below_headers":
        cap_arg = ns * (46 + 18 * nf) + 63  # the stream headers (fLaC, STREAMINFO, SEEKTABLE of nf points) + 64 is the least
    elif refusal == "null_offsets":
        off_arg = None
    else:
        assert refusal == "not_a_float_geometry"
    total = ctypes.c_int64(-7)
    if entry == "begin":
        rc = getattr(L, f"fa_encode_{'i64' if wide else 'i32'}_device_begin")(_vp(xd), ns, n, level, ws_arg, ws_bytes, _vp(d_st), _vp(d_nb),
                                                                            ctypes.byref(total), _vp(d_info), None)
    elif kind == "f32":
        rc = L.fa_encode_f32_device(_vp(xd), ns, n, level, None, ws_arg, ws_bytes, buf_arg, cap_arg, _vp(d_st), _vp(d_nb), off_arg, _vp(d_gain),
                                    ctypes.byref(total), _vp(d_info), None)
    else:
        rc = getattr(L, f"fa_encode_{'i64' if wide else 'i32'}_device")(_vp(xd), ns, n, level, ws_arg, ws_bytes, buf_arg, cap_arg, _vp(d_st), _vp(d_nb),
                                                                      ctypes.byref(total), _vp(d_info), None)
    torch.cuda.synchronize()
    assert total.value == -7, "a refused call wrote its total"
    return rc, [(ws, 0x5A), (buf, 0xA5), (d_st, 0xC3), (d_nb, 0xC3), (d_info, 0xC3), (d_off, 0x3C), (d_gain, 0x3C)]


def _assert_untouched(buffers, what):
    for k, (t, v) in enumerate(buffers):
        assert bool((t == v).all()), f"{what}: buffer {k} (workspace, output, starts, nbytes, info, offsets, gains) was written"


@pytest.mark.parametrize("refusal", sorted(REFUSALS))
@pytest.mark.parametrize("name", MAIN)
def test_refused_before_launch(torch, L, name, refusal):
    """The argument checks in front of every encode sequence, on the MAIN routes' shapes and the dispatch of a caller that
    sets nothing: a workspace one byte short of what the query asks, no workspace, no output buffer, or a capacity one
    byte short of the stream headers + 64 is FA_ERROR_ALLOC -- from the single-pass entry point of the shape's type
    (fa_encode_i32_device, _i64_device: the f64 route encodes int64, _f32_device) and from fa_encode_*_device_begin (with
    its own workspace query; it takes no output buffer) -- and nothing is enqueued: the poisoned output, index, info and
    workspace buffers hold their poison, *h_total_bytes is not written."""
    kind, ns, n, level, _ = ROUTES[name]
    for entry in REFUSALS[refusal]:
        if entry == "begin" and kind == "f32":
            continue  # (float32 input has no slot sequence of its own)
        rc, buffers = _refused_call(torch, L, entry, kind, ns, n, level, refusal)
        assert rc == FA_ERROR_ALLOC, f"{name} {entry} {refusal}: return code {rc}"
        _assert_untouched(buffers, f"{name} {entry} {refusal}")


def test_refused_f32_before_launch(torch, L):
    """fa_encode_f32_device without offsets is FA_ERROR_CONVERT_TYPE; at (8, 9192), streams that end in a short frame -- not a
    geometry K3F quantises in -- FA_ERROR_ENCODE_INIT (with every other argument good: a workspace and a buffer of the
    queried sizes).  Nothing is written in either case."""
    kind, ns, n, level, _ = ROUTES["f32_fused"]
    rc, buffers = _refused_call(torch, L, "single", "f32", ns, n, level, "null_offsets")
    assert rc == FA_ERROR_CONVERT_TYPE
    _assert_untouched(buffers, "f32 without offsets")
    rc, buffers = _refused_call(torch, L, "single", "f32", 8, 9192, 5, "not_a_float_geometry")
    assert rc == FA_ERROR_ENCODE_INIT
    _assert_untouched(buffers, "f32 at (8, 9192)")


@pytest.mark.parametrize("poison", ["zeros", "ones", "a5"])
@pytest.mark.parametrize("op", ["append", "overwrite", "overwrite_streams"])
@pytest.mark.parametrize("wide", [False, True], ids=["i32", "i64"])
def test_splice_workspace_poisoned(fa, torch, oracle, L, wide, op, poison):
    """fa_append_*_device / fa_overwrite_*_device take a caller's workspace too (the Python layer hands them a fresh
    torch.empty): poisoned, with the output full of 0xA5 and a guard behind its capacity, the result is the oracle's encode
    of the concatenated / patched samples.  The workspace is exactly the bytes the query asks for, with a guard of its own
    behind them that the call must leave as it is."""
    ns, n, m, first, level = 6, 9000, 5000, 3000, 5
    gen = _i64 if wide else sinusoid_noise_i32
    x, new = gen(ns, n, seed=301), gen(ns if op != "overwrite_streams" else 2, m, seed=302)
    idx = np.array([4, 1], dtype=np.int64) if op == "overwrite_streams" else None
    comp, st, nb = fa.encode_flac_device(_dev(torch, x), level=level, compact=True)
    nd = _dev(torch, new)
    sfx = "_i64" if wide else ""
    rows = ns if idx is None else idx.size
    if op == "append":
        need = int(getattr(L, "fa_append_workspace_bytes" + sfx)(ns, n, m, level))
        cap = int(getattr(L, "fa_append_capacity_bytes" + sfx)(comp.numel(), ns, n, m, level))
        expect = np.concatenate([x, new], axis=1)
    else:
        need = int(getattr(L, "fa_overwrite_workspace_bytes" + sfx)(ns, n, rows, first, m, level))
        cap = int(getattr(L, "fa_overwrite_capacity_bytes" + sfx)(comp.numel(), ns, n, rows, first, m, level))
        expect = x.copy()
        expect[slice(None) if idx is None else idx, first : first + m] = new
    assert need > 0 and cap > 0
    ws = torch.full((need + 4096,), {"zeros": 0x00, "ones": 0xFF, "a5": 0xA5}[poison], dtype=torch.uint8, device="cuda")
    ws[need:] = 0x3C
    buf = torch.full((cap + GUARD,), 0xA5, dtype=torch.uint8, device="cuda")
    d_st = torch.full((ns,), -1, dtype=torch.int64, device="cuda")
    d_nb = torch.full((ns,), -1, dtype=torch.int64, device="cuda")
    total = ctypes.c_int64(-1)
    torch.cuda.synchronize()
    if op == "append":
        rc = getattr(L, "fa_append_i64_device" if wide else "fa_append_i32_device")(
            _vp(comp), comp.numel(), _vp(st), _vp(nb), ns, n, _vp(nd), m, level, _vp(ws), need, _vp(buf), cap, _vp(d_st), _vp(d_nb),
            ctypes.byref(total), None)
    else:
        d_idx = None if idx is None else _dev(torch, idx)
        rc = getattr(L, "fa_overwrite_i64_device" if wide else "fa_overwrite_i32_device")(
            _vp(comp), comp.numel(), _vp(st), _vp(nb), ns, n, _vp(d_idx), rows, _vp(nd), first, m, level, _vp(ws), need, _vp(buf), cap,
            _vp(d_st), _vp(d_nb), ctypes.byref(total), None)
    torch.cuda.synchronize()
    assert rc == 0
    assert bool((ws[need:] == 0x3C).all()), "bytes behind workspace_bytes were written"
    blob_o, st_o, nb_o = (oracle.encode_i64 if wide else oracle.encode_i32)(expect, level)
    assert total.value == blob_o.size
    assert np.array_equal(buf[: total.value].cpu().numpy(), blob_o)
    assert bool((buf[cap:] == 0xA5).all()), "bytes behind capacity_bytes were written"
    assert np.array_equal(d_st.cpu().numpy(), st_o) and np.array_equal(d_nb.cpu().numpy(), nb_o)


# ------------------------------------------------------------------------------------- one workspace, many geometries

ORDER = ["k3g_int64", "k3f_whole_big", "k3g_small", "f32_fused", "k3f_tail", "f64_small", "k3g_int64_big", "k3f_whole", "k3g_level1",
         "f32_fused_small", "k3f_tail_big", "f64"]


@pytest.mark.parametrize("order", ["forward", "reverse"])
def test_one_workspace_many_geometries(fa, torch, oracle, monkeypatch, order):
    """One EncodeWorkspace carried through every route at growing and shrinking sizes, in a fixed shuffled order and in its
    reverse; the workspace grows when it must and is otherwise reused with whatever the call before left in it."""
    from flacarray_amd.libflacarray import EncodeWorkspace

    ws = EncodeWorkspace()
    names = ORDER if order == "forward" else ORDER[::-1]
    sizes = []
    for step, name in enumerate(names):
        x, want = _case(oracle, name)
        _check(_run(fa, torch, monkeypatch, name, _dev(torch, x), ws), want, f"step {step} ({name}) of the {order} order")
        sizes.append(ws.buf.numel())
    assert sizes == sorted(sizes), "a workspace only ever grows"


# ------------------------------------------------------------------------------------------- header-table cache walk

# Consecutive geometries differ in exactly one key field of the cached frame-header table.
WALK = [  # name, kind, streams, samples, level -> (nf, tail, channels, block size)
    ("first", "i32", 8, 16384, 5),      # 4 frames, whole, 1 channel, 4096
    ("nf", "i32", 8, 20480, 5),         # 5 frames
    ("tail", "i32", 8, 17384, 5),       # 5 frames, the last of 1000
    ("nch", "i64", 8, 17384, 5),        # two channels
    ("blocksize", "i64", 8, 5608, 1),   # 5 frames of 1152, the last of 1000
]
_walk_cache = {}


def _walk_case(oracle, k):
    if k not in _walk_cache:
        _, kind, ns, n, level = WALK[k]
        x = _GEN[kind](ns, n, seed=400 + k)
        _walk_cache[k] = (x, list((oracle.encode_i32 if kind == "i32" else oracle.encode_i64)(x, level)))
    return _walk_cache[k]


@pytest.mark.parametrize("bump", ["grow", "release"])
@pytest.mark.parametrize("route", ["k3f", "k3g", "slots"])
def test_header_table_cache_walk(fa, torch, oracle, L, monkeypatch, route, bump):
    """Walk the table's key one field at a time (frame count, tail length, channel count, block size), bump the scratch
    epoch -- `grow`: the test starts from released scratch and a decode of three streams, so a decode of 20000 streams
    makes the decode slots grow; `release`: fa_release_scratch
    frees every slot, after which the table's slot may well come back at its old address -- and encode the first geometry
    again.  `k3f`: K3F wherever it applies, K3G for the rest (the two share the table); `k3g`: K3G throughout; `slots`:
    the begin / finish sequence."""
    if route == "slots":
        monkeypatch.setenv("FLACARRAY_HIP_SLOTS", "1")
    else:
        monkeypatch.setenv("FLACARRAY_HIP_PLACED_BELOW", "0" if route == "k3f" else K3G_ONLY)

    if bump == "grow":
        # every slot starts empty (and the decode slots stay small through the walk), so the decode of 20000 streams below MUST
        # grow the stream table and the frame table, whatever ran in this process before
        torch.cuda.synchronize()
        L.fa_release_scratch()
        w = sinusoid_noise_i32(3, 64, seed=409)
        comp, st, nb = fa.encode_flac_device(_dev(torch, w), level=5)
        assert np.array_equal(fa.decode_flac_device(comp, st, nb, 64).cpu().numpy(), w)

    def step(k, what):
        x, want = _walk_case(oracle, k)
        out = fa.encode_flac_device(_dev(torch, x), level=WALK[k][4])
        torch.cuda.synchronize()
        _check([t.cpu().numpy() for t in out], want, f"{what} ({WALK[k][0]}) by {route}")

    for k in range(len(WALK)):
        step(k, f"step {k}")
    step(2, "back to the tail geometry")
    if bump == "grow":
        ns_many = 20000
        z = sinusoid_noise_i32(ns_many, 64, seed=410)
        zd = _dev(torch, z)
        comp, st, nb = fa.encode_flac_device(zd, level=5)
        assert np.array_equal(fa.decode_flac_device(comp, st, nb, 64).cpu().numpy(), z)
    else:
        torch.cuda.synchronize()
        L.fa_release_scratch()
    step(2, "the tail geometry after the epoch bump")
    step(0, "the first geometry again")
    step(3, "two channels after one")
    step(0, "the first geometry once more")


# ------------------------------------------------------------------------------------------------ decode scratch reuse

@pytest.mark.parametrize("latency", ["auto", "k7"])
@pytest.mark.parametrize("order", ["large_small_large", "small_large_small"])
def test_decode_scratch_reuse(fa, torch, monkeypatch, order, latency):
    """A large two-channel store, a small one-channel store and the large one again (and the other way round) through whole,
    ranged and slice decodes, aligned and not: the stream table, the frame table, the task table, the realigned copy of the
    bytes and the two-channel planar image (scratch slots 1, 2, 3, 7, 8) are reused shrinking and growing.  Every result is
    the numpy slice of its input."""
    if latency == "k7":
        monkeypatch.setenv("FLACARRAY_HIP_LATENCY", "0")
    big, small = _i64(32, 20000, seed=501), sinusoid_noise_i32(3, 1000, seed=502)
    stores = {}
    for key, x in (("big", big), ("small", small)):
        comp, st, nb = fa.encode_flac_device(_dev(torch, x), level=5, compact=True)
        off1 = torch.zeros(comp.numel() + 17, dtype=torch.uint8, device="cuda")
        off1[1 : 1 + comp.numel()] = comp
        stores[key] = (x, comp, off1[1 : 1 + comp.numel()], st, nb)
    torch.cuda.synchronize()
    assert stores["big"][2].data_ptr() % 16 != 0

    def read(key, step):
        x, comp, shifted, st, nb = stores[key]
        wide, n = x.dtype == np.int64, x.shape[1]
        lo, hi = n // 3 + 1, n - 7
        sl = (np.array([x.shape[0] - 1, 0, 1]), np.array([0, n // 2, n - 5]), np.array([n, 100, 5]))
        for c, how in ((comp, "aligned"), (shifted, "realigned")):
            what = f"step {step}: {key} store, {how}"
            assert np.array_equal(fa.decode_flac_device(c, st, nb, n, is_int64=wide).cpu().numpy(), x), what
            assert np.array_equal(fa.decode_flac_device(c, st, nb, n, lo, hi, is_int64=wide).cpu().numpy(), x[:, lo:hi]), what + ", ranged"
            flat = fa.decode_slices_device(c, st, nb, n, *sl, is_int64=wide)[0].cpu().numpy()
            assert np.array_equal(flat, np.concatenate([x[s, f : f + k] for s, f, k in zip(*sl)])), what + ", slices"

    for step, key in enumerate(order.replace("large", "big").split("_")):
        read(key, step)
