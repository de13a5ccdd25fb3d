"""Who the decoder's frame CRC-16 check checks: every frame of a store damaged in turn, through every route that promises
the check, under both decoders.  tests/verify_corpus.py holds the stores, the damage sites and the rule; a site never
changes the parse (tests/test_verify_corpus.py), so with the check on a call fails exactly when it reads a sample of the
damaged frame, and with it off it returns the model's samples with return code 0 -- which is what isolates the check
from the decoders' own.  After every failure an intact call must pass and equal the input (a stale error word would
show).  Every expectation is exact: a RuntimeError, or the model's bytes."""
import numpy as np
import pytest

from flacarray_amd import libflacarray
from tests import quant_model as M
from tests import verify_corpus as V

pytestmark = pytest.mark.gpu

FAILED = "Decoding failed"
UNIFORM = V.M1 + V.M2 + V.M4  # one block size: ranged reads through an index and slices


@pytest.fixture(scope="module")
def torch():
    import torch

    return torch


@pytest.fixture(scope="module")
def fa():
    import flacarray_amd

    return flacarray_amd


@pytest.fixture(params=["k7", "k7l"])
def decoder_dispatch(request, monkeypatch):
    """FLACARRAY_HIP_LATENCY=0: every launch goes to the throughput decoder K7; =1: every launch the latency decoder K7L
    takes (blocks up to 4096 samples) goes to it (the variable is read per call)."""
    monkeypatch.setenv("FLACARRAY_HIP_LATENCY", "0" if request.param == "k7" else "1")
    monkeypatch.delenv("FLACARRAY_HIP_VERIFY_AFTER", raising=False)
    monkeypatch.delenv("FLACARRAY_HIP_HOST_CHUNK_BYTES", raising=False)
    return request.param


def _host(x):
    if x is None or isinstance(x, np.ndarray):
        return x
    if isinstance(x, (tuple, list)):
        return tuple(_host(v) for v in x)
    return x.cpu().numpy()


def _same(got, want, what):
    """Bit for bit (floats through their bytes), shapes and types included; tuples element by element."""
    got = _host(got)
    if isinstance(want, tuple):
        assert isinstance(got, tuple) and len(got) == len(want), what
        for g, w in zip(got, want):
            _same(g, w, what)
        return
    if want is None:
        assert got is None, what
        return
    want = np.ascontiguousarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, got.dtype, want.shape, want.dtype)
    if got.tobytes() != want.tobytes():
        bad = np.argwhere(got != want)
        raise AssertionError("%s: %d elements differ, the first at %s" % (what, len(bad), bad[:1].tolist()))


def must_fail(call, what):
    """The call raises the decoder's RuntimeError; what it was goes into the report if it does not."""
    try:
        call()
    except RuntimeError as e:
        assert FAILED in str(e), (what, e)
    else:
        raise AssertionError("%s: the checked call did not fail" % (what,))


def both_ways(call, good, bad, hit, intact, unchecked, what):
    """call(blob, verify) on the damaged blob: unchecked it returns the model's samples; checked it raises if the call
    reads the damaged frame (and the intact call after it passes), else returns what the intact store returns."""
    _same(call(bad, False), unchecked, (what, "unchecked"))
    if hit:
        must_fail(lambda: call(bad, True), what)
        _same(call(good, True), intact, (what, "intact, after the failure"))
    else:
        _same(call(bad, True), intact, (what, "checked, not read"))


class Dev:
    """A store on the device, with what its calls return when it is intact."""

    def __init__(self, torch, fa, store):
        self.store, self.torch, self.fa = store, torch, fa
        up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()  # noqa: E731
        self.blob, self.st, self.nb = up(store.blob), up(store.starts), up(store.nbytes)
        self.i64 = store.channels == 2
        off, gain = V.float_params(store)
        self.off, self.gain, self.d_off, self.d_gain = off, gain, up(off), up(gain)
        self.args = (self.st, self.nb, store.n)

    def damaged(self, site):
        bad = self.blob.clone()
        bad[V.byte_of(self.store, site)] ^= site.mask
        return bad

    def floats(self, data):
        return M.restore(data, self.off, self.gain)

    def index(self, blob):
        return self.fa.DeviceDecodeIndex(blob, self.st, self.nb, self.store.n, is_int64=self.i64)


@pytest.fixture(scope="module")
def devs(torch, fa):
    made = {}

    def get(name):
        if name not in made:
            made[name] = Dev(torch, fa, V.build_store(name))
        return made[name]

    return get


def test_own_stores_are_the_device_encoders(fa, torch, devs):
    """The own* stores come from the CPU encoder: the device encoder writes the same bytes (but for the signature)."""
    for name, level in (("m1_own4096", 5), ("m1_own1152", 1), ("m2_own1152", 1), ("m4_coded", 5)):
        d = devs(name)
        comp, st, nb = fa.encode_flac_device(torch.from_numpy(d.store.data).cuda(), level=level, md5=True)
        assert np.array_equal(comp.cpu().numpy(), d.store.blob[: comp.numel()]) and comp.numel() == d.store.blob.size, name
        assert np.array_equal(st.cpu().numpy().reshape(-1), d.store.starts) and np.array_equal(nb.cpu().numpy().reshape(-1), d.store.nbytes)


# -------------------------------------------------------------------------------------- decode, whole and in ranges

def _range_kw(store, a, b):
    return {} if (a, b) == (0, store.n) else {"first_sample": a, "last_sample": b}


@pytest.mark.parametrize("name", V.STORES)
def test_decode_ranges(fa, devs, decoder_dispatch, name):
    """decode_flac_device and DeviceDecodeIndex.decode, integers and restored floats, over the whole stream, the damaged
    frame's first and last sample, everything in front of it and everything behind it."""
    d = devs(name)
    st = d.store
    good_ix = d.index(d.blob) if name in UNIFORM else None
    for site in V.sites(name):
        bad = d.damaged(site)
        model = V.unchecked(st, site)
        bad_ix = d.index(bad) if name in UNIFORM else None
        for a, b in V.ranges(st, site):
            hit = V.raises(st, site, a, b)
            kw = _range_kw(st, a, b)
            for fl in (False, True):
                fkw = {"offsets": d.d_off, "gains": d.d_gain} if fl else {}
                want = d.floats(st.data[:, a:b]) if fl else st.data[:, a:b]
                want_bad = d.floats(model[:, a:b]) if fl else model[:, a:b]
                both_ways(lambda blob, v: fa.decode_flac_device(blob, *d.args, is_int64=d.i64, verify=v, **kw, **fkw),
                          d.blob, bad, hit, want, want_bad, (name, "decode_flac_device", site, a, b, fl))
                if good_ix is not None:
                    both_ways(lambda blob, v: (good_ix if blob is d.blob else bad_ix).decode(verify=v, **kw, **fkw),
                              d.blob, bad, hit, want, want_bad, (name, "index.decode", site, a, b, fl))
        if bad_ix is not None:
            bad_ix.close()
    if good_ix is not None:
        good_ix.close()


# ------------------------------------------------------------------------------------------------------------- slices

@pytest.mark.parametrize("name", UNIFORM)
def test_decode_slices(fa, devs, decoder_dispatch, name):
    """decode_slices_device and DeviceDecodeIndex.decode_slices (to the device and to the host): slices of intact streams
    around one that reaches the damaged frame by a single sample; then around ones that miss it by one on each side."""
    d = devs(name)
    st = d.store
    good_ix = d.index(d.blob)
    for site in V.sites(name):
        bad = d.damaged(site)
        bad_ix = d.index(bad)
        model = V.unchecked(st, site)
        for sl in V.slice_lists(st, site):
            hit = V.slices_raise(st, site, sl)
            cols = [np.array(c, dtype=np.int64) for c in zip(*sl)]
            for fl in (False, True):
                fkw = {"offsets": d.d_off, "gains": d.d_gain} if fl else {}
                conv = (lambda x: V.gather(d.floats(x), sl)) if fl else (lambda x: V.gather(x, sl))
                want, want_bad = conv(st.data), conv(model)
                both_ways(lambda blob, v: fa.decode_slices_device(blob, *d.args, *cols, is_int64=d.i64, verify=v, **fkw)[0],
                          d.blob, bad, hit, want, want_bad, (name, "decode_slices_device", site, sl, fl))
                for to_host in (False, True):
                    both_ways(lambda blob, v: (good_ix if blob is d.blob else bad_ix).decode_slices(*cols, verify=v, to_host=to_host, **fkw)[0],
                              d.blob, bad, hit, want, want_bad, (name, "index.decode_slices", to_host, site, sl, fl))
        bad_ix.close()
    good_ix.close()


# ------------------------------------------------------------------------------------------------------------- reduce

def _subsets(store, site):
    """streams=: everything, the damaged stream behind another one, everything but the damaged stream."""
    ns = len(store.frames)
    others = [s for s in range(ns) if s != site.stream]
    return (None, [others[-1], site.stream], others)


@pytest.mark.parametrize("name", V.STORES)
def test_reduce(fa, devs, decoder_dispatch, name):
    """reduce_flac_device and DeviceDecodeIndex.reduce (one bin): all streams, streams= naming the damaged stream and
    leaving it out, the sample ranges of the decode test; two-channel stores also in column chunks of two frames."""
    d = devs(name)
    st = d.store
    good_ix = d.index(d.blob) if name in UNIFORM else None
    caps = (None, len(st.frames) * 2 * st.block * 8) if d.i64 else (None,)
    if d.i64:
        assert -(-st.n // (2 * st.block)) >= 3  # several chunks
    for site in V.sites(name):
        bad = d.damaged(site)
        bad_ix = d.index(bad) if name in UNIFORM else None
        model = V.unchecked(st, site)
        for a, b in V.ranges(st, site):
            for sub in _subsets(st, site):
                if sub is not None and (a, b) not in ((0, st.n), V.ranges(st, site)[1]):
                    continue  # (subsets: over everything and over the frame's first sample)
                hit = V.raises(st, site, a, b, sub)
                rows = slice(None) if sub is None else sub
                want, want_bad = V.reduce_model(st.data[rows], a, b), V.reduce_model(model[rows], a, b)
                for cap in caps:
                    kw = dict(first_sample=a, last_sample=b, streams=sub, max_temp_bytes=cap)
                    both_ways(lambda blob, v: fa.reduce_flac_device(blob, *d.args, is_int64=d.i64, verify=v, **kw),
                              d.blob, bad, hit, want, want_bad, (name, "reduce_flac_device", site, a, b, sub, cap))
                    if good_ix is not None:
                        both_ways(lambda blob, v: (good_ix if blob is d.blob else bad_ix).reduce(verify=v, **kw),
                                  d.blob, bad, hit, want, want_bad, (name, "index.reduce", site, a, b, sub, cap))
        if bad_ix is not None:
            bad_ix.close()
    if good_ix is not None:
        good_ix.close()


# ---------------------------------------------------------------------------------------------------------- check_md5

@pytest.mark.parametrize("name", V.STORES)
def test_check_md5(fa, devs, decoder_dispatch, name):
    """check_md5_device decodes every signed stream: any damaged frame fails the checked call, in one chunk and in at
    least three column chunks (the sites damage the first, every middle and the last one in turn); unchecked, a footer
    site leaves every signature matching and a payload site breaks its stream's."""
    d = devs(name)
    st = d.store
    item = 8 if d.i64 else 4
    caps = [None]
    if name in UNIFORM:
        per_block = 64 // item
        width = (st.n // 3) // per_block * per_block
        assert width > 0 and -(-st.n // width) >= 3
        caps.append(len(st.frames) * width * item)
    ones = np.ones(len(st.frames), dtype=np.int8)
    for site in V.sites(name):
        bad = d.damaged(site)
        for cap in caps:
            both_ways(lambda blob, v: fa.check_md5_device(blob, *d.args, is_int64=d.i64, verify=v, max_temp_bytes=cap),
                      d.blob, bad, True, ones, V.md5_status(st, site), (name, "check_md5_device", site, cap))


# ----------------------------------------------------------------------------------------------------------- host ABI

def _host_chunks(nbytes, target):
    """The host pipeline's chunk of every stream: a stream that would take a chunk's compressed bytes past the target
    (FLACARRAY_HIP_HOST_CHUNK_BYTES) starts the next one."""
    out, total = [], 0
    for s, nb in enumerate(nbytes):
        if s and total + nb > target:
            out.append(out[-1] + 1)
            total = 0
        else:
            out.append(out[-1] if s else 0)
        total += nb
    return out


@pytest.mark.parametrize("name", V.STORES)
def test_host_abi_always_checks(fa, devs, decoder_dispatch, monkeypatch, name):
    """decode_flac, decode_flac_into and decode_flac_restore (which answers a failed decode with None: its caller then
    takes the two-call path, which raises) from host memory, in at least three chunks of the host pipeline -- the sites'
    streams lie in the first, the middle and the last one."""
    st = devs(name).store
    d = devs(name)
    target = int(st.nbytes.max()) * (2 if len(st.frames) >= 5 else 1)
    monkeypatch.setenv("FLACARRAY_HIP_HOST_CHUNK_BYTES", str(target))
    chunk_of = _host_chunks(st.nbytes, target)
    assert chunk_of[-1] >= 2 and sorted({chunk_of[s] for s in V.site_streams(st)}) == [0, chunk_of[-1] // 2, chunk_of[-1]]
    dt = st.data.dtype
    for site in V.sites(name):
        bad = V.damage(st.blob, st, site)
        for a, b in V.ranges(st, site):
            hit = V.raises(st, site, a, b)
            kw = _range_kw(st, a, b)
            want, wantf = st.data[:, a:b], d.floats(st.data[:, a:b])
            calls = {
                "decode_flac": (lambda blob: fa.decode_flac(blob, st.starts, st.nbytes, st.n, is_int64=d.i64, **kw), want),
                "decode_flac_into": (lambda blob: libflacarray.decode_flac_into(blob, st.starts, st.nbytes, st.n, np.zeros((len(st.frames), b - a), dtype=dt), **kw), want),
                "decode_flac_restore": (lambda blob: libflacarray.decode_flac_restore(blob, st.starts, st.nbytes, st.n, d.off, d.gain, is_int64=d.i64, **kw), wantf),
            }
            if name in V.M3:
                del calls["decode_flac_restore"], calls["decode_flac_into"]  # (several block sizes: only decode_flac regroups)
            for label, (call, w) in calls.items():
                what = (name, label, site, a, b)
                if not hit:
                    _same(call(bad), w, what)
                elif label == "decode_flac_restore":
                    assert call(bad) is None, what
                    _same(call(st.blob), w, (what, "intact, after the failure"))
                else:
                    must_fail(lambda: call(bad), what)
                    _same(call(st.blob), w, (what, "intact, after the failure"))


# ------------------------------------------------------------------------------------------------ the process default

@pytest.mark.parametrize("name", ["m1_foreign64", "m2_foreign64", "m3_mixed"])
def test_process_default(fa, devs, decoder_dispatch, name):
    """set_decode_verify(True): verify=None checks, verify=False still does not."""
    d = devs(name)
    st = d.store
    assert fa.set_decode_verify(True) is False
    try:
        for site in V.sites(name)[:: max(1, len(V.sites(name)) // 8)]:
            bad = d.damaged(site)
            model = V.unchecked(st, site)
            lo, _ = V.frame_span(st, site.stream, site.frame)
            verify = lambda v: None if v else False  # noqa: E731
            routes = [
                (lambda blob, v: fa.decode_flac_device(blob, *d.args, is_int64=d.i64, verify=verify(v)), st.data, model),
                (lambda blob, v: fa.decode_flac_device(blob, *d.args, lo, lo + 1, is_int64=d.i64, verify=verify(v)), st.data[:, lo : lo + 1], model[:, lo : lo + 1]),
                (lambda blob, v: fa.reduce_flac_device(blob, *d.args, is_int64=d.i64, verify=verify(v)), V.reduce_model(st.data), V.reduce_model(model)),
                (lambda blob, v: fa.check_md5_device(blob, *d.args, is_int64=d.i64, verify=verify(v)), np.ones(len(st.frames), dtype=np.int8), V.md5_status(st, site)),
            ]
            if name in UNIFORM:
                touching, _ = V.slice_lists(st, site)
                cols = [np.array(c, dtype=np.int64) for c in zip(*touching)]
                routes.append((lambda blob, v: fa.decode_slices_device(blob, *d.args, *cols, is_int64=d.i64, verify=verify(v))[0],
                               V.gather(st.data, touching), V.gather(model, touching)))

                def indexed(blob, v):
                    ix = d.index(blob)
                    try:
                        return ix.decode(verify=verify(v))
                    finally:
                        ix.close()

                routes.append((indexed, st.data, model))
            for k, (call, want, want_bad) in enumerate(routes):
                both_ways(call, d.blob, bad, True, want, want_bad, (name, "default on, route", k, site))
    finally:
        assert fa.set_decode_verify(False) is True
    site = V.sites(name)[0]
    _same(fa.decode_flac_device(d.damaged(site), *d.args, is_int64=d.i64), V.unchecked(st, site), "default off again")


# ------------------------------------------------------------------------------------ the check beside the decoder

@pytest.mark.parametrize("after", [False, True], ids=["beside", "after_k7"])
@pytest.mark.parametrize("shape", [V.BESIDE, V.BESIDE_ODD, V.AFTER], ids=["16388", "16386", "16383"])
def test_last_tasks_of_a_launch_that_fills_the_chip(fa, torch, monkeypatch, shape, after):
    """From 16384 tasks on the check is queued beside the throughput decoder on a stream of its own
    (FLACARRAY_HIP_VERIFY_AFTER=1: after it, as below that count).  The frames of the first task, of the last one below
    16384, of every one from 16384 on and of one in the middle, damaged in turn, each fail the decode; an intact call
    between every two."""
    monkeypatch.setenv("FLACARRAY_HIP_LATENCY", "0")
    monkeypatch.delenv("FLACARRAY_HIP_VERIFY_AFTER", raising=False)
    if after:
        monkeypatch.setenv("FLACARRAY_HIP_VERIFY_AFTER", "1")
    st = V.beside_store(*shape)
    tasks = sum(len(row) for row in st.frames)
    assert tasks == shape[0] * shape[1] and (tasks >= 16384) == (shape != V.AFTER)
    d = Dev(torch, fa, st)
    want = torch.from_numpy(st.data).cuda()
    assert torch.equal(fa.decode_flac_device(d.blob, *d.args, verify=True), want)
    for task in V.beside_tasks(*shape):
        site = V.task_site(st, task)
        bad = d.damaged(site)
        assert torch.equal(fa.decode_flac_device(bad, *d.args, verify=False), want), task
        must_fail(lambda: fa.decode_flac_device(bad, *d.args, verify=True), ("task", task, site))
        assert torch.equal(fa.decode_flac_device(d.blob, *d.args, verify=True), want), task
        must_fail(lambda: fa.decode_flac_device(bad, *d.args, offsets=d.d_off, gains=d.d_gain, verify=True), ("task", task, site, "floats"))
        assert torch.equal(fa.decode_flac_device(d.blob, *d.args, verify=True), want), task


# --------------------------------------------------------------------------- frames of every length and placement

def _xor_value(torch, site):
    v = site.value
    return v - (1 << 32) if v >= 1 << 31 else v


def _length_store_cases(fa, torch, ls, blob, what):
    """Every site of every frame of a length store whose blob is `blob` (damaged in place and mended again)."""
    st = ls.store
    args = (torch.from_numpy(st.starts).cuda(), torch.from_numpy(st.nbytes).cuda(), st.n)
    want = torch.from_numpy(st.data).cuda()
    assert torch.equal(fa.decode_flac_device(blob, *args, verify=True), want), (what, "intact")
    for s, sp in enumerate(ls.specs):
        for label, site in [("first byte", V.header_site(st, s))] + V.length_sites(st, s):
            at = V.byte_of(st, site)
            blob[at] ^= site.mask
            try:
                if site.kind != "header":
                    model = want
                    if site.kind == "payload":
                        model = want.clone()
                        model[site.stream, site.sample] ^= _xor_value(torch, site)
                    assert torch.equal(fa.decode_flac_device(blob, *args, verify=False), model), (what, sp, label, "unchecked")
                must_fail(lambda: fa.decode_flac_device(blob, *args, verify=True), label)
            except BaseException as e:  # noqa: BLE001
                raise AssertionError("%s, frame %s, %s (byte %d of %d under the CRC): %r" % (what, sp, label, site.offset, sp.L, e)) from e
            finally:
                blob[at] ^= site.mask
            assert torch.equal(fa.decode_flac_device(blob, *args, verify=True), want), (what, sp, label, "intact, after the failure")


LENGTH_PARTS = {"to_200": (0, 200), "to_400": (201, 400), "to_600": (401, V.SMALL_TOP), "edges": (V.SMALL_TOP + 1, 10_000), "long": (10_001, 1 << 30)}


@pytest.mark.parametrize("part", list(LENGTH_PARTS))
def test_every_frame_length(fa, torch, decoder_dispatch, part):
    """One-channel VERBATIM frames of every length the check's loops distinguish (whole trips of 2048 bytes, the word loop
    of stride 256, the masked last word), each the last frame of its stream, 16 bytes of padding behind the store: a flip
    of the first byte, of the first payload byte, of a payload byte of lanes 0, 1, 31, 32 and 63, of the last payload byte
    and of each CRC byte must fail the checked decode."""
    lo, hi = LENGTH_PARTS[part]
    n = 0
    for ls in V.length_stores():
        if lo <= ls.specs[0].L <= hi:
            blob = torch.from_numpy(ls.store.blob).cuda()
            _length_store_cases(fa, torch, ls, blob, (part, ls.store.name))
            n += len(ls.specs)
    assert n > 0


@pytest.mark.parametrize("shift", [0, 1, 2, 3])
def test_frame_at_the_end_of_the_blob_at_every_alignment(fa, torch, decoder_dispatch, shift):
    """The same sites with the frame as the last bytes of the blob (the check's byte-wise tail and its clamp of the
    whole-trip loop) and the blob a view `shift` bytes into its allocation."""
    for sp in V.placement_specs():
        ls = V.length_store((sp,), pad=0)
        size = ls.store.blob.size
        fr = ls.store.frames[0][-1]
        assert fr.start + fr.nbytes == size
        buf = torch.zeros(size + 3, dtype=torch.uint8, device="cuda")
        blob = buf[shift : shift + size]
        blob.copy_(torch.from_numpy(ls.store.blob))
        assert blob.is_contiguous() and blob.data_ptr() % 4 == (buf.data_ptr() + shift) % 4
        _length_store_cases(fa, torch, ls, blob, ("end of blob, shift %d" % shift, sp.L))
