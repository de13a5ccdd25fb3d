"""Named device calls for the scratch-state tests (tests/test_gpu_scratch_state.py runs them on the GPU under poisoned
scratch, tests/test_scratch_cases.py checks on the CPU that every scratch slot of the library is claimed by one).

A case is a function of a context `c` (torch, the package, the ctypes library, the oracle, a monkeypatch) that builds
its small input on the host, makes its device calls and asserts every result against an independent source: the
oracle's bytes and values, numpy, hashlib, and the byte-level models of tests/.  Never an earlier call of the library.
`slots` is the set of scratch slots (get_scratch(<slot>, ...) in flacarray_amd/csrc/flacarray_hip.hip) a run of the case
from released scratch leaves allocated -- the GPU test compares it with fa_debug_scratch_bytes, so a claim cannot drift.
`partner` names a larger case of another kind that shares slots: it runs first in the `leftover` state.

Shapes: 3 to 12 streams of 2 to 5 frames with a short last frame, at level 1 (blocks of 1152) unless the route needs
level 5 (K3F: whole frames of 4096)."""
import ctypes
import hashlib
from collections import namedtuple

import numpy as np

from tests import compare_corpus as CC
from tests import histogram_model as HM
from tests import reindex_model as RM
from tests import scrub_model as SM
from tests import verify_corpus as VC
from tests.conftest import sinusoid_noise_f32, sinusoid_noise_i32, strip_seektable

# Slot 6 is the one slot no case claims: it exists in -DFA_STAMPS builds only (the per-phase cycle sums of K3).
STAMPS_SLOT = 6
GUARD = 4096
B1 = 1152
N1 = 3 * B1 + 200  # four frames, the last one short

Case = namedtuple("Case", "name fn slots partner")
CASES = {}


def case(name, slots, partner=None):
    def deco(fn):
        assert name not in CASES
        CASES[name] = Case(name, fn, frozenset(slots), partner)
        return fn

    return deco


class Ctx:
    def __init__(self, torch, fa, L, oracle, monkeypatch, poison=0xA5):
        self.torch, self.fa, self.L, self.oracle, self.mp, self.poison = torch, fa, L, oracle, monkeypatch, poison

    def up(self, a):
        return self.torch.from_numpy(np.ascontiguousarray(a)).cuda()

    def ups(self, *arrays):
        return tuple(self.up(a) for a in arrays)

    def env(self, name, value):
        if value is None:
            self.mp.delenv(name, raising=False)
        else:
            self.mp.setenv(name, value)

    def full(self, nbytes, guard=GUARD):
        """A byte buffer of `nbytes` of the poison with a guard of 0x3C behind it."""
        t = self.torch.full((nbytes + guard,), self.poison, dtype=self.torch.uint8, device="cuda")
        t[nbytes:] = 0x3C
        return t

    def guard_ok(self, t, nbytes):
        return bool((t[nbytes:] == 0x3C).all())

    def misaligned(self, blob, shift=1):
        pad = self.torch.full((blob.numel() + 32,), self.poison, dtype=self.torch.uint8, device="cuda")
        pad[shift : shift + blob.numel()] = blob
        view = pad[shift : shift + blob.numel()]
        assert view.data_ptr() % 16 != 0
        return view


def host(t):
    return t.cpu().numpy() if hasattr(t, "cpu") else np.asarray(t)


def same(a, b):
    a, b = host(a), host(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def _vp(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


# ---------------------------------------------------------------------------------------------------------- inputs
_made = {}


def memo(key, fn):
    """fn() once per key: the expected results are computed once and shared by every poison and state."""
    if key not in _made:
        _made[key] = fn()
    return _made[key]


def ints(kind, ns, n, seed):
    key = ("ints", kind, ns, n, seed)
    if key not in _made:
        x = sinusoid_noise_i32(ns, n, seed=seed)
        if kind == "i64":
            x = x.astype(np.int64) * 70001 + np.random.default_rng(seed).integers(-9, 10, (ns, n))
        _made[key] = x
    return _made[key]


def floats(kind, ns, n, seed):
    x = sinusoid_noise_f32(ns, n, seed=seed)
    if kind == "f64":
        x = x.astype(np.float64) + 1e-9 * np.random.default_rng(seed + 1).normal(0.0, 1.0, (ns, n))
    return x


def store(c, kind, ns=5, n=N1, level=1, seed=900):
    """(x, blob, starts, nbytes) on the host: the oracle's encode of ints(kind, ...)."""
    key = ("store", kind, ns, n, level, seed)
    if key not in _made:
        x = ints(kind, ns, n, seed)
        _made[key] = (x,) + tuple((c.oracle.encode_i64 if kind == "i64" else c.oracle.encode_i32)(x, level))
    return _made[key]


def float_store(c, kind, ns=5, n=N1, level=1, seed=910):
    """(floats, ints, offsets, gains, blob, starts, nbytes): the oracle's quantisation and encode."""
    key = ("fstore", kind, ns, n, level, seed)
    if key not in _made:
        f = floats(kind, ns, n, seed)
        q, off, gain = (c.oracle.float64_to_int64 if kind == "f64" else c.oracle.float32_to_int32)(f)
        _made[key] = (f, q, off, gain) + tuple((c.oracle.encode_i64 if kind == "f64" else c.oracle.encode_i32)(q, level))
    return _made[key]


def encoded(c, x, level=1):
    return (c.oracle.encode_i64 if x.dtype == np.int64 else c.oracle.encode_i32)(np.ascontiguousarray(x), level)


def check_store(got, want, what):
    assert len(got) >= 3
    for k in range(3):
        g, w = host(got[k]).reshape(-1), np.asarray(want[k]).reshape(-1)
        assert g.shape == w.shape and np.array_equal(g, w), f"{what}: output {k} differs from the oracle"


SLICES = (np.array([4, 0, 1]), np.array([0, N1 // 2, N1 - 5]), np.array([N1, 100, 5]))


def _gather(x, sl):
    return np.concatenate([x[s, f : f + k] for s, f, k in zip(*sl)])


def _decode_all(c, x, d, wide, what, verify=None):
    n = x.shape[1]
    lo, hi = n // 3 + 1, n - 7
    fa = c.fa
    assert np.array_equal(host(fa.decode_flac_device(*d, n, is_int64=wide, verify=verify)), x), what
    assert np.array_equal(host(fa.decode_flac_device(*d, n, lo, hi, is_int64=wide, verify=verify)), x[:, lo:hi]), what + ", ranged"
    sl = tuple(np.minimum(a, x.shape[0] - 1) if k == 0 else a for k, a in enumerate(SLICES))
    flat = fa.decode_slices_device(*d, n, *sl, is_int64=wide, verify=verify)[0]
    assert np.array_equal(host(flat), _gather(x, sl)), what + ", slices"


# ----------------------------------------------------------------------------------------------------------- decode
def _decode_case(kind, latency, verify=None):
    def fn(c):
        c.env("FLACARRAY_HIP_LATENCY", latency)
        x, blob, st, nb = store(c, kind)
        _decode_all(c, x, c.ups(blob, st, nb), kind == "i64", "decode " + kind, verify)

    return fn


case("decode_i32", {1, 2, 3}, "decode_i64_k7")(_decode_case("i32", None))
case("decode_i64", {1, 2, 3}, "host_f32")(_decode_case("i64", None))
case("decode_i32_k7", {1, 2, 3}, "decode_i64_k7")(_decode_case("i32", "0"))
case("decode_i64_k7", {1, 2, 3, 8}, "host_f32")(_decode_case("i64", "0"))
case("decode_i32_latency", {1, 2, 3}, "decode_i64_k7")(_decode_case("i32", "1"))
case("decode_i64_latency", {1, 2, 3}, "decode_i32_k7")(_decode_case("i64", "1"))
case("decode_i32_verify", {1, 2, 3}, "decode_i64_k7")(_decode_case("i32", "0", True))
case("decode_i64_verify", {1, 2, 3}, "decode_i32_k7")(_decode_case("i64", None, True))


@case("decode_float_restore", {1, 2}, "decode_i64_k7")
def _decode_float_restore(c):
    """The restore fused into the decoder's store: float32 from one channel, float64 from two."""
    for kind in ("f32", "f64"):
        f, q, off, gain, blob, st, nb = float_store(c, kind)
        want = (c.oracle.int64_to_float64 if kind == "f64" else c.oracle.int32_to_float32)(q, off, gain)
        got = c.fa.decode_flac_device(*c.ups(blob, st, nb), N1, offsets=c.up(off), gains=c.up(gain), is_int64=kind == "f64")
        assert same(got, want), kind


@case("decode_misaligned", {1, 2, 3, 7}, "decode_i64_k7")
def _decode_misaligned(c):
    """A blob at an address that is not 16-byte aligned: the decoders work on a realigned copy (slot 7)."""
    for kind in ("i32", "i64"):
        x, blob, st, nb = store(c, kind)
        d = c.ups(blob, st, nb)
        _decode_all(c, x, (c.misaligned(d[0]), d[1], d[2]), kind == "i64", "misaligned " + kind)


def _stripped_case(no_scan):
    def fn(c):
        c.env("FLACARRAY_HIP_NO_SYNC_SCAN", "1" if no_scan else None)
        for kind in ("i32", "i64"):
            x, blob, st, nb = store(c, kind)
            _decode_all(c, x, c.ups(*strip_seektable(blob, st, nb)), kind == "i64", "no SEEKTABLE, %s" % kind)

    return fn


case("decode_stripped_scan", {1, 2, 3}, "decode_i64_k7")(_stripped_case(False))
case("decode_stripped_walk", {1, 2, 3}, "decode_i64_k7")(_stripped_case(True))


@case("decode_deep_history", {1, 2}, "decode_i64_k7")
def _decode_deep_history(c):
    """Generated foreign streams with LPC orders 9-12, 13-16 and 17-32: the 16-deep and 32-deep history passes."""
    for latency in (None, "0"):
        c.env("FLACARRAY_HIP_LATENCY", latency)
        for name in ("orders_9-12", "orders_13-16", "orders_17-32"):
            rep = CC.uniform(name)
            got = c.fa.decode_flac_device(*c.ups(*CC.store(rep, 7)), rep.n)
            assert np.array_equal(host(got), CC.rows(rep, 7)), (name, latency)


@case("decode_index", set(), "decode_i64_k7")
def _decode_index(c):
    """DeviceDecodeIndex: build, then whole, ranged, slice and host-landing reads."""
    for kind in ("i32", "i64"):
        x, blob, st, nb = store(c, kind)
        ix = c.fa.DeviceDecodeIndex(*c.ups(blob, st, nb), N1, is_int64=kind == "i64")
        try:
            assert np.array_equal(host(ix.decode()), x)
            assert np.array_equal(host(ix.decode(7, N1 - 3)), x[:, 7 : N1 - 3])
            assert np.array_equal(host(ix.decode_slices(*SLICES)[0]), _gather(x, SLICES))
            assert np.array_equal(ix.decode_slices(*SLICES, to_host=True)[0], _gather(x, SLICES))
        finally:
            ix.close()


# ---------------------------------------------------------------------------------------------------------- compare
@case("compare", {1, 2, 8}, "decode_i64_k7")
def _compare(c):
    """Equal input is -1 everywhere; one changed sample of one stream is found at its index, the other streams stay -1."""
    for kind in ("i32", "i64"):
        x, blob, st, nb = store(c, kind)
        d = c.ups(blob, st, nb)
        assert np.array_equal(host(c.fa.compare_flac_device(*d, c.up(x))), np.full(5, -1))
        y = x.copy()
        y[3, 2 * B1 + 17] ^= 1
        want = np.full(5, -1)
        want[3] = 2 * B1 + 17
        assert np.array_equal(host(c.fa.compare_flac_device(*d, c.up(y))), want), kind
    for kind in ("f32", "f64"):
        f, q, off, gain, blob, st, nb = float_store(c, kind)
        got = c.fa.compare_flac_device(*c.ups(blob, st, nb), c.up(f), c.up(off), c.up(gain))
        assert np.array_equal(host(got), np.full(5, -1)), kind


# -------------------------------------------------------------------------------------------------------------- MD5
def _md5_rows(x):
    return np.stack([np.frombuffer(hashlib.md5(np.ascontiguousarray(r).tobytes()).digest(), dtype=np.uint8) for r in x])


@case("md5", {15}, "check_md5")
def _md5(c):
    """md5_device one-shot and resumed, integers and floats (the NaN flag word of slot 15); sign_streams_device."""
    for kind in ("i32", "i64"):
        x, blob, st, nb = store(c, kind)
        xd = c.up(x)
        want = _md5_rows(x)
        assert np.array_equal(host(c.fa.md5_device(xd)), want), kind
        cut = 2 * B1
        state = c.fa.md5_device(xd[:, :cut], final=False)
        assert np.array_equal(host(c.fa.md5_device(xd[:, cut:], state=state, n_before=cut)), want), kind + " resumed"
        signed = c.fa.sign_streams_device(c.up(blob), c.up(st), c.up(want))
        ref = blob.copy()
        for s in range(x.shape[0]):
            ref[st[s] + 26 : st[s] + 42] = want[s]
        assert np.array_equal(host(signed), ref), kind + " signed"
    for kind in ("f32", "f64"):
        f, q, off, gain = float_store(c, kind)[:4]
        assert np.array_equal(host(c.fa.md5_device(c.up(f), c.up(off), c.up(gain))), _md5_rows(q)), kind


@case("check_md5", {1, 2, 14, 15}, "reduce_i64")
def _check_md5(c):
    """A store of signed streams, unsigned streams and one wrong signature, in three or more column chunks."""
    for kind in ("i32", "i64"):
        x, blob, st, nb = store(c, kind, ns=6)
        dig = _md5_rows(x)
        blob = blob.copy()
        want = np.array([1, -1, 1, 0, -1, 1], dtype=np.int8)
        for s in np.flatnonzero(want >= 0):
            blob[st[s] + 26 : st[s] + 42] = dig[s]
        blob[st[3] + 30] ^= 0x01
        d = c.ups(blob, st, nb)
        cap = 6 * B1 * x.dtype.itemsize  # one frame column per chunk: four chunks
        got = c.fa.check_md5_device(*d, N1, is_int64=kind == "i64", max_temp_bytes=cap)
        assert np.array_equal(host(got), want), kind
        got, digests = c.fa.check_md5_device(*d, N1, is_int64=kind == "i64", return_digests=True, max_temp_bytes=cap)
        assert np.array_equal(host(got), want) and np.array_equal(host(digests), dig), kind + ", digests"
        # nothing signed: only the second of the two count words (streams a digest can be given for) sends the call on
        x, blob, st, nb = store(c, kind, ns=6)
        got, digests = c.fa.check_md5_device(*c.ups(blob, st, nb), N1, is_int64=kind == "i64", return_digests=True, max_temp_bytes=cap)
        assert np.array_equal(host(got), np.full(6, -1, dtype=np.int8)) and np.array_equal(host(digests), dig), kind + ", unsigned"
        # and nothing to decide at all (one-channel streams asked as two-channel ones and the reverse): -2, digests zero
        got, digests = c.fa.check_md5_device(*c.ups(blob, st, nb), N1, is_int64=kind != "i64", return_digests=True)
        assert np.array_equal(host(got), np.full(6, -2, dtype=np.int8)) and not host(digests).any(), kind + ", not checkable"


# ----------------------------------------------------------------------------------------------------------- damage
DAMAGE_STORES = ("own1152", "own1152x2")
DAMAGE_KINDS = ("fLaC marker", "STREAMINFO block size", "seek offset beyond", "seek sample number", "footer", "sync", "half nbytes",
                "zeros across")


def _damage_cases(name):
    picked = []
    for kind in DAMAGE_KINDS:
        picked.append(next(k for k in SM.cases(name) if k.name.startswith(kind)))
    return picked


@case("status_intact", {18, 19}, "salvage_i32")
def _status_intact(c):
    for name in DAMAGE_STORES:
        s = SM.build_store(name)
        got = c.fa.frame_status_device(*c.ups(s.blob, s.starts, s.nbytes), s.n, is_int64=s.channels == 2, block_size=s.block)
        assert got.dtype == c.torch.uint8 and tuple(got.shape) == (3, 3) and not bool(got.any()), name


@case("status_damaged", {17, 18, 19}, "salvage_i32")
def _status_damaged(c):
    """A damaged stream header, seek point and frame (and the rest of DAMAGE_KINDS) against tests/scrub_model.py, the
    blob aligned and not: unlocated frames are where a frame-table entry may never be written."""
    for name in DAMAGE_STORES:
        s = SM.build_store(name)
        for k in _damage_cases(name):
            want = memo(("status", name, k.name), lambda: SM.expected(s, k))
            for shift in (0, 7):
                d = c.ups(k.blob, k.starts, k.nbytes)
                if shift:
                    d = (c.misaligned(d[0], shift),) + d[1:]
                got = c.fa.frame_status_device(*d, s.n, is_int64=s.channels == 2, block_size=s.block)
                assert np.array_equal(host(got), want), (name, k.name, shift)


def _salvage_case(name):
    def fn(c):
        s = SM.build_store(name)
        wide = s.channels == 2
        off, gain = VC.float_params(s)
        restore = c.oracle.int64_to_float64 if wide else c.oracle.int32_to_float32
        fl = restore(s.data, off, gain)
        for latency in ("0", "1"):
            c.env("FLACARRAY_HIP_LATENCY", latency)
            for j, k in enumerate(_damage_cases(name)):
                want_status = memo(("status", name, k.name), lambda: SM.expected(s, k))
                d = c.ups(k.blob, k.starts, k.nbytes)
                if j % 2:
                    d = (c.misaligned(d[0], 3),) + d[1:]
                for first, last in ((-1, -1), (5, s.n - 3)):
                    lo, hi = (0, s.n) if first < 0 else (first, last)
                    out, status = c.fa.decode_flac_salvage_device(*d, s.n, first, last, is_int64=wide, fill=-7, block_size=s.block)
                    assert np.array_equal(host(status), want_status), (name, k.name)
                    assert same(out, SM.salvage_model(s.data, want_status, lo, hi, -7, s.block)), (name, k.name, first)
                    out, status = c.fa.decode_flac_salvage_device(*d, s.n, first, last, offsets=c.up(off), gains=c.up(gain), is_int64=wide,
                                                                  block_size=s.block)
                    assert np.array_equal(host(status), want_status)
                    assert same(out, SM.salvage_model(fl, want_status, lo, hi, np.nan, s.block)), (name, k.name, first, "float")

    return fn


case("salvage_i32", {17, 18, 19, 20, 21}, "reindex")(_salvage_case("own1152"))
case("salvage_i64", {8, 17, 18, 19, 20, 21}, "decode_i64_k7")(_salvage_case("own1152x2"))


# ---------------------------------------------------------------------------------------------------------- reindex
@case("reindex", {7, 18, 19, 22}, "salvage_i32")
def _reindex(c):
    """A libFLAC-layout store (tests/reindex_model.py) comes back in this library's layout: the oracle's own bytes."""
    for kind in ("i32", "i64"):
        x, blob, st, nb = store(c, kind)
        foreign = RM.to_foreign(blob, st, nb)
        for verify in (True, False):
            got = c.fa.reindex_flac_device(*c.ups(*foreign), N1, is_int64=kind == "i64", verify=verify)
            check_store(got, (blob, st, nb), "reindex %s verify=%s" % (kind, verify))
        got = c.fa.reindex_flac_device(c.misaligned(c.up(foreign[0]), 5), c.up(foreign[1]), c.up(foreign[2]), N1, is_int64=kind == "i64")
        check_store(got, (blob, st, nb), "reindex %s, misaligned" % kind)


# ----------------------------------------------------------------------------------------------------------- window
def raw_window(c, d, size, idx, first, last, level, nch):
    """fa_window_device with a workspace of exactly fa_window_workspace_bytes, poisoned, a guard behind it; the output
    poisoned with a guard behind its capacity.  Returns the (blob, starts, nbytes) it wrote."""
    torch, L = c.torch, c.L
    comp, st, nb = d
    n_stream = st.numel()
    m = n_stream if idx is None else len(idx)
    d_idx = None if idx is None else torch.tensor(idx, dtype=torch.int64, device="cuda")
    sizes = host(nb)
    picked = int(sizes.sum()) if idx is None else int(sum(sizes[i] for i in idx))
    ws_bytes = L.fa_window_workspace_bytes(n_stream, size, m, first, last, nch, level)
    cap = L.fa_window_capacity_bytes(picked, n_stream, size, m, first, last, nch, level)
    assert ws_bytes >= 0 and cap > 0
    ws, buf = c.full(ws_bytes), c.full(cap)
    index = torch.full((2 * m,), -1, dtype=torch.int64, device="cuda")
    total = ctypes.c_int64(-1)
    torch.cuda.synchronize()
    rc = L.fa_window_device(_vp(comp), comp.numel(), _vp(st), _vp(nb), n_stream, size, _vp(d_idx), m, first, last, nch, level,
                            _vp(ws) if ws_bytes else None, ws_bytes, _vp(buf), cap, _vp(index[:m]), _vp(index[m:]), ctypes.byref(total), None)
    torch.cuda.synchronize()
    assert rc == 0 and 0 < total.value <= cap
    assert c.guard_ok(ws, ws_bytes), "bytes behind the window workspace were written"
    assert c.guard_ok(buf, cap), "bytes behind the window capacity were written"
    return buf[: total.value], index[:m], index[m:]


@case("window_aligned", {1, 2, 9, 18, 19}, "join_unaligned")
def _window_aligned(c):
    """Aligned first with last inside a frame, a permuted stream subset, first = 0, and the whole range: through
    window_flac_device and through fa_window_device itself."""
    for kind in ("i32", "i64"):
        x, blob, st, nb = store(c, kind)
        d = c.ups(blob, st, nb)
        wide, nch = kind == "i64", 2 if kind == "i64" else 1
        for idx, first, last in ((None, B1, 2 * B1 + 77), ([3, 0, 4], B1, N1), ([2, 1], 0, B1 + 5), ([4, 2, 0, 1, 3], 0, N1), (None, 2 * B1, 3 * B1)):
            want = encoded(c, x[slice(None) if idx is None else idx, first:last])
            what = "window %s %s [%d, %d)" % (kind, idx, first, last)
            got = c.fa.window_flac_device(*d, N1, first, last, streams=None if idx is None else np.array(idx), level=1, is_int64=wide, verify=True)
            check_store(got, want, what)
            check_store(raw_window(c, d, N1, idx, first, last, 1, nch), want, what + ", raw call")


@case("window_unaligned", {1, 2, 9}, "join_unaligned")
def _window_unaligned(c):
    """first = 1: the row-chunk route, a decode and an encode per chunk of rows."""
    for kind in ("i32", "i64"):
        x, blob, st, nb = store(c, kind)
        got = c.fa.window_flac_device(*c.ups(blob, st, nb), N1, 1, N1 - 9, streams=np.array([4, 0, 2]), level=1, is_int64=kind == "i64",
                                      max_temp_bytes=2 * N1 * x.dtype.itemsize)
        check_store(got, encoded(c, x[[4, 0, 2], 1 : N1 - 9]), "window_unaligned " + kind)


# ------------------------------------------------------------------------------------------------------------- join
def raw_join(c, stores, level, nch):
    """fa_join_device with a workspace of exactly fa_join_workspace_bytes, poisoned and guarded, as raw_window."""
    torch, L = c.torch, c.L
    P = len(stores)
    n_stream = stores[0][1].numel()
    i64s, ptrs = ctypes.c_int64 * P, ctypes.c_void_p * P
    sizes = i64s(*[s[3] for s in stores])
    nbytes = i64s(*[s[0].numel() for s in stores])
    ws_bytes = L.fa_join_workspace_bytes(P, n_stream, sizes, nch, level)
    cap = L.fa_join_capacity_bytes(P, nbytes, n_stream, sizes, nch, level)
    assert ws_bytes > 0 and cap > 0
    ws, buf = c.full(ws_bytes), c.full(cap)
    index = torch.full((2 * n_stream,), -1, dtype=torch.int64, device="cuda")
    total = ctypes.c_int64(-1)
    torch.cuda.synchronize()
    rc = L.fa_join_device(P, ptrs(*[s[0].data_ptr() for s in stores]), nbytes, ptrs(*[s[1].data_ptr() for s in stores]),
                          ptrs(*[s[2].data_ptr() for s in stores]), sizes, n_stream, nch, level, _vp(ws), ws_bytes, _vp(buf), cap,
                          _vp(index[:n_stream]), _vp(index[n_stream:]), ctypes.byref(total), None)
    torch.cuda.synchronize()
    assert rc == 0 and 0 < total.value <= cap
    assert c.guard_ok(ws, ws_bytes), "bytes behind the join workspace were written"
    assert c.guard_ok(buf, cap), "bytes behind the join capacity were written"
    return buf[: total.value], index[:n_stream], index[n_stream:]


def _parts(c, x, cuts):
    bounds = (0,) + tuple(cuts) + (x.shape[1],)
    return [c.ups(*encoded(c, x[:, a:b])) + (b - a,) for a, b in zip(bounds, bounds[1:])]


@case("join_aligned", {18, 19}, "window_aligned")
def _join_aligned(c):
    """Two and three parts, every part but the last a whole number of blocks: nothing decoded, nothing encoded."""
    for kind in ("i32", "i64"):
        x, blob, st, nb = store(c, kind)
        for cuts in ((B1,), (B1, 3 * B1)):
            parts = _parts(c, x, cuts)
            what = "join %s at %s" % (kind, cuts)
            check_store(c.fa.join_flac_device(parts, level=1, is_int64=kind == "i64", verify=True), (blob, st, nb), what)
            check_store(raw_join(c, parts, 1, 2 if kind == "i64" else 1), (blob, st, nb), what + ", raw call")


@case("join_unaligned", {1, 2, 9}, "window_unaligned")
def _join_unaligned(c):
    """One unaligned cut: the parts behind it are decoded and appended, in row chunks."""
    for kind in ("i32", "i64"):
        x, blob, st, nb = store(c, kind)
        parts = _parts(c, x, (B1, 2 * B1 + 31))
        got = c.fa.join_flac_device(parts, level=1, is_int64=kind == "i64", max_temp_bytes=2 * N1 * x.dtype.itemsize)
        check_store(got, (blob, st, nb), "join_unaligned " + kind)


@case("join_axis0", {0, 3, 4, 5, 9}, "window_unaligned")
def _join_axis0(c):
    """FlacArray.concatenate(axis=0) of resident stores: more streams, every stream verbatim."""
    x = ints("i32", 5, N1, 900)
    a = c.fa.FlacArray.from_array(x[:2], level=1).to_device()
    b = c.fa.FlacArray.from_array(x[2:], level=1).to_device()
    j = c.fa.FlacArray.concatenate([a, b], axis=0, level=1)
    assert np.array_equal(j.to_array(), x)
    want = encoded(c, x)
    assert np.array_equal(np.asarray(j.compressed), want[0]) and np.array_equal(np.asarray(j.stream_nbytes).reshape(-1), want[2])


# ----------------------------------------------------------------------------------------------------------- splice
def _splice_case(op):
    def fn(c):
        m, first = B1 + 300, B1 - 100
        for kind in ("i32", "i64"):
            x, blob, st, nb = store(c, kind)
            d = c.ups(blob, st, nb)
            idx = np.array([4, 1]) if op == "overwrite_streams" else None
            new = ints(kind, 5 if idx is None else 2, m, 931)
            if op == "append":
                got = c.fa.append_flac_device(*d, N1, c.up(new), level=1, verify=True)
                want = np.concatenate([x, new], axis=1)
            else:
                got = c.fa.overwrite_flac_device(*d, N1, first, c.up(new), streams=idx, level=1, verify=True)
                want = x.copy()
                want[slice(None) if idx is None else idx, first : first + m] = new
            check_store(got, encoded(c, want), "%s %s" % (op, kind))

    return fn


case("append", {1, 2, 9}, "window_unaligned")(_splice_case("append"))
case("overwrite", {1, 2, 9}, "window_unaligned")(_splice_case("overwrite"))
case("overwrite_streams", {1, 2, 9}, "window_unaligned")(_splice_case("overwrite_streams"))


@case("append_float", {1, 2, 4, 9}, "window_unaligned")
def _append_float(c):
    """Float rows quantised with the store's offsets and gains on their way into the splice (quantise_rows_kernel)."""
    for kind in ("f32", "f64"):
        f, q, off, gain, blob, st, nb = float_store(c, kind)
        quant = c.oracle.float64_to_int64 if kind == "f64" else c.oracle.float32_to_int32
        full = quant(np.concatenate([f, f[:, : B1 + 5]], axis=1))
        # (the oracle derives offsets and gains from each row's range: rows whose range the new samples repeat keep them)
        assert same(full[1], off) and same(full[2], gain)
        got = c.fa.append_flac_device(*c.ups(blob, st, nb), N1, c.up(f[:, : B1 + 5]), level=1, offsets=c.up(off), gains=c.up(gain))
        check_store(got, encoded(c, full[0]), "append " + kind)


# ----------------------------------------------------------------------------------------------------------- reduce
def _reduce_want(x, width, first, last, idx=None):
    key = ("reduce", x.dtype.str, x.shape, width, first, last, None if idx is None else tuple(idx))
    return memo(key, lambda: _reduce_model(x, width, first, last, idx))


def _reduce_model(x, width, first, last, idx):
    x = x[slice(None) if idx is None else idx, first:last].astype(object)
    n = x.shape[1]
    width = n if width is None else width
    cols = [x[:, a : a + width] for a in range(0, n, width)]
    mn = np.array([[min(r) for r in col] for col in cols], dtype=np.int64).T
    mx = np.array([[max(r) for r in col] for col in cols], dtype=np.int64).T
    sm = np.array([[sum(r) % 2**64 for r in col] for col in cols], dtype=np.uint64).T.view(np.int64)
    sq = np.array([[sum(int(v) * int(v) for v in r) for r in col] for col in cols], dtype=object).T
    return mn, mx, sm, sq


def _check_reduce(got, want, wide, what):
    mn, mx, sm, qh, ql = [None if t is None else host(t) for t in got]
    assert np.array_equal(mn, want[0]) and np.array_equal(mx, want[1]) and np.array_equal(sm, want[2]), what
    if not wide:
        sq = qh.astype(object) * 2**32 + ql.astype(object)
        assert np.array_equal(sq, want[3]), what + ": sum of squares"


@case("reduce_i32", {1, 2, 3}, "decode_i64_k7")
def _reduce_i32(c):
    """The int32 sink at width None, 64 and 5, whole and ranged, every stream and a subset (list-mode task tables), and the
    indexed form."""
    x, blob, st, nb = store(c, "i32", n=B1 + 137)
    n = x.shape[1]
    d = c.ups(blob, st, nb)
    ix = c.fa.DeviceDecodeIndex(*d, n)
    try:
        for width in (None, 64, 5):
            for idx, first, last in ((None, 0, n), (np.array([3, 0]), 9, n - 2)):
                want = _reduce_want(x, width, first, last, idx)
                what = "reduce width %s streams %s" % (width, idx)
                _check_reduce(c.fa.reduce_flac_device(*d, n, width, first, last, streams=idx), want, False, what)
                _check_reduce(ix.reduce(width, first, last, streams=idx), want, False, what + ", indexed")
    finally:
        ix.close()


@case("reduce_i64", {1, 2, 3, 16}, "check_md5")
def _reduce_i64(c):
    """Two-channel streams through decoded column chunks: max_temp_bytes of one frame column, so four chunks."""
    x, blob, st, nb = store(c, "i64")
    d = c.ups(blob, st, nb)
    for width, idx in ((None, None), (700, np.array([2, 4, 1]))):
        got = c.fa.reduce_flac_device(*d, N1, width, 3, N1 - 1, streams=idx, is_int64=True, max_temp_bytes=5 * B1 * 8)
        _check_reduce(got, _reduce_want(x, width, 3, N1 - 1, idx), True, "reduce_i64 width %s" % width)


# -------------------------------------------------------------------------------------------------------- histogram
def _check_hist(got, want, what):
    for g, w, name in zip(got, want, ("counts", "below", "above")):
        assert np.array_equal(host(g), w), "%s: %s" % (what, name)


@case("histogram_i32", {1, 2, 3}, "decode_i64_k7")
def _histogram_i32(c):
    """Several short rows per wave (direct atomics), nbins 1 and 2048, a subset, a range, and the indexed form."""
    x, blob, st, nb = store(c, "i32")
    d = c.ups(blob, st, nb)
    ix = c.fa.DeviceDecodeIndex(*d, N1)
    try:
        for nbins, shift in ((1, 18), (2048, 9), (37, 14)):
            lo = int(x.min()) + (1 << 16)
            for idx, first, last in ((None, 0, N1), (np.array([4, 1]), 5, N1 - 11)):
                want = HM.bin_counts(x[slice(None) if idx is None else idx, first:last], lo, shift, nbins)
                what = "histogram nbins %d streams %s" % (nbins, idx)
                _check_hist(c.fa.histogram_flac_device(*d, N1, lo, shift, nbins, first, last, streams=idx), want, what)
                _check_hist(ix.histogram(lo, shift, nbins, first, last, streams=idx), want, what + ", indexed")
    finally:
        ix.close()


@case("histogram_lds", {1, 2}, "decode_i64_k7")
def _histogram_lds(c):
    """Rows of 70 frames: a wave's 64 frames belong to one row, which counts in LDS and adds its words once."""
    n = 69 * B1 + 11
    x, blob, st, nb = store(c, "i32", ns=3, n=n, seed=941)
    d = c.ups(blob, st, nb)
    for nbins, shift in ((2048, 9), (1, 30), (300, 12)):
        lo = np.array([int(r.min()) + 1000 for r in x])
        _check_hist(c.fa.histogram_flac_device(*d, n, lo, shift, nbins), HM.bin_counts(x, lo, shift, nbins), "histogram_lds %d" % nbins)


@case("histogram_i64", {1, 2, 16}, "check_md5")
def _histogram_i64(c):
    x, blob, st, nb = store(c, "i64")
    lo, shift = int(x.min()) + 12345, 22
    got = c.fa.histogram_flac_device(*c.ups(blob, st, nb), N1, lo, shift, 2048, 1, N1 - 1, is_int64=True, max_temp_bytes=5 * B1 * 8)
    _check_hist(got, HM.bin_counts(x[:, 1 : N1 - 1], lo, shift, 2048), "histogram_i64")


@case("order_statistic", {0, 3, 4, 5, 9}, "decode_i64_k7")
def _order_statistic(c):
    """FlacArray.order_statistic on a resident store: several histogram passes reuse the same scratch."""
    x = ints("i32", 5, N1, 900)
    a = c.fa.FlacArray.from_array(x, level=1).to_device()
    ranks = np.array([0, 1, N1 // 2, N1 - 1])
    assert np.array_equal(np.asarray(a.order_statistic(ranks)), np.sort(x, axis=-1)[:, ranks])


# ------------------------------------------------------------------------------------------------ float and host paths
@case("std", {12, 13}, "std_wide")
def _std(c):
    """stream_std f32 and f64: np.std bit for bit, at numpy's buffer size (a summation plan unless it is 8192 elements)."""
    for kind in ("f32", "f64"):
        f = floats(kind, 5, N1, 951)
        assert same(c.fa.std_device(c.up(f)), np.std(f, axis=-1)), kind


@case("std_wide", {12, 13}, "std")
def _std_wide(c):
    f = floats("f64", 12, 5 * B1 + 3, 952)
    assert same(c.fa.std_device(c.up(f)), np.std(f, axis=-1))


@case("float_convert", {4}, "host_f32")
def _float_convert(c):
    """float32_to_int32 / float64_to_int64 on the device, and back through fa_int32_to_float32_device / _int64_."""
    for kind in ("f32", "f64"):
        f, q, off, gain = float_store(c, kind)[:4]
        to_int = c.fa.float64_to_int64_device if kind == "f64" else c.fa.float32_to_int32_device
        got = to_int(c.up(f))
        assert same(got[0], q) and same(got[1], off) and same(got[2], gain), kind
        back = c.torch.full(f.shape, float("nan"), dtype=c.torch.float64 if kind == "f64" else c.torch.float32, device="cuda")
        fn = c.L.fa_int64_to_float64_device if kind == "f64" else c.L.fa_int32_to_float32_device
        assert fn(_vp(got[0]), f.shape[0], f.shape[1], _vp(got[1]), _vp(got[2]), _vp(back), None) == 0
        c.torch.cuda.synchronize()
        assert same(back, (c.oracle.int64_to_float64 if kind == "f64" else c.oracle.int32_to_float32)(q, off, gain)), kind + " back"


@case("encode_f32_fused", {1, 2, 9, 10}, "encode_k3g_int64")
def _encode_f32_fused(c):
    c.env("FLACARRAY_HIP_PLACED_BELOW", "0")
    f, q, off, gain, blob, st, nb = float_store(c, "f32", ns=4, n=2 * 4096, level=5, seed=961)
    got = c.fa.encode_flac_device_f32(c.up(f), level=5, verify=True)
    check_store(got, (blob, st, nb), "f32 fused")
    assert same(got[3], off) and same(got[4], gain)


@case("encode_float_two_step", {4, 9}, "encode_k3f_whole")
def _encode_float_two_step(c):
    for kind in ("f32", "f64"):
        f, q, off, gain, blob, st, nb = float_store(c, kind)
        fn = c.fa.encode_flac_device_f64 if kind == "f64" else c.fa.encode_flac_device_f32
        got = fn(c.up(f), level=1)
        check_store(got, (blob, st, nb), kind + " two-step")
        assert same(got[3], off) and same(got[4], gain)


def _host_case(kind):
    def fn(c):
        """fa_encode_*_host and fa_decode_*_host at a size that takes two chunks of streams."""
        f, q, off, gain, blob, st, nb = float_store(c, kind, ns=6)
        c.env("FLACARRAY_HIP_HOST_CHUNK_BYTES", str(4 * N1 * f.dtype.itemsize))
        got = (c.fa.libflacarray.encode_flac_f64 if kind == "f64" else c.fa.libflacarray.encode_flac_f32)(f, None, 1)
        check_store(got, (blob, st, nb), "host encode " + kind)
        assert same(got[3], off) and same(got[4], gain)
        out = c.fa.libflacarray.decode_flac_restore(blob, st, nb, N1, off, gain, is_int64=kind == "f64")
        assert same(out, (c.oracle.int64_to_float64 if kind == "f64" else c.oracle.int32_to_float32)(q, off, gain)), "host decode " + kind

    return fn


case("host_f32", {0, 1, 2, 3, 4, 5, 9, 11}, "decode_i64_k7")(_host_case("f32"))
case("host_f64", {0, 1, 2, 3, 4, 5, 9, 11}, "decode_i64_k7")(_host_case("f64"))


@case("host_int", {0, 1, 2, 3, 4, 5, 9}, "decode_i64_k7")
def _host_int(c):
    """The reference's host entry points (encode_i32 / decode_i32 and the int64 twins) on device scratch 0, 3 and 5."""
    for kind in ("i32", "i64"):
        x, blob, st, nb = store(c, kind)
        got = c.fa.encode_flac(x, 1)
        check_store(got, (blob, st, nb), "host encode " + kind)
        assert np.array_equal(c.fa.decode_flac(blob, st, nb, N1, is_int64=kind == "i64"), x)


# --------------------------------------------------------------------------------------------------------- encoders
# The six MAIN routes of tests/test_gpu_call_state.py at these shapes: (kind, streams, samples, level, PLACED_BELOW).
ENCODERS = {
    "encode_k3f_whole": ("i32", 4, 2 * 4096, 5, "0"),
    "encode_k3f_tail": ("i32", 4, 2 * 4096 + 1000, 5, "0"),
    "encode_k3g_level1": ("i32", 5, N1, 1, None),
    "encode_k3g_int64": ("i64", 6, 2 * 4096 + 808, 5, None),
    "encode_f64": ("f64", 5, N1, 2, None),
}


def _encoder_case(name):
    kind, ns, n, level, below = ENCODERS[name]

    def fn(c):
        c.env("FLACARRAY_HIP_PLACED_BELOW", below)
        if kind == "f64":
            f, q, off, gain, blob, st, nb = float_store(c, kind, ns, n, level, 971)
            got = c.fa.encode_flac_device_f64(c.up(f), level=level)
            assert same(got[3], off) and same(got[4], gain)
        else:
            x, blob, st, nb = store(c, kind, ns, n, level, 972)
            got = c.fa.encode_flac_device(c.up(x), level=level)
        check_store(got, (blob, st, nb), name)

    return fn


for _name in ENCODERS:
    case(_name, {4, 9} if ENCODERS[_name][0] == "f64" else {9}, None)(_encoder_case(_name))
# (the sixth route, f32 fused, is encode_f32_fused above)
ENCODER_CASES = tuple(ENCODERS) + ("encode_f32_fused",)
