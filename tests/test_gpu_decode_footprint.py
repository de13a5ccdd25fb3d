"""Where the decoders write, and where they do not.  Every device decode entry point of the C ABI is called with a raw
output pointer into a buffer of sentinel: 8192 guard elements on each side, the pointer moved 0 to 3 elements off a 16-byte
boundary, slices at offsets the test chooses -- gaps of 0, 1, 2, 3 and 5 sentinel elements between them, half of the
batches placed out of order.  After each call the WHOLE buffer is compared, as bits, with the image tests/decode_edges.py
builds from the known samples: a store one element past a slice's end, a whole-tile store taken for a lane it does not
fit, or a vector store through a pointer that is not 16-byte aligned shows as a changed sentinel (or a missing sample).

Windows and slices enumerate the frame, tile and 4-group edges of each stream (tests/test_decode_edges.py asserts the
residues, shapes and lane mixes they reach); the stores bring 4096- and 1152-sample frames of this encoder, foreign
block-192 streams whose LPC orders reach the 16- and 32-deep passes (with idle lanes, and -- one order bucket per store --
the whole-tile path of each pass), and two-channel streams.  FLACARRAY_HIP_LATENCY=0 sends everything through the
throughput decoder K7, =1 through the latency decoder K7L, which hands the streams it does not take back to K7."""
import ctypes

import numpy as np
import pytest

from tests import decode_edges as E

pytestmark = pytest.mark.gpu

ENTRIES = ["device", "slices", "indexed_grid", "indexed_slices"]


@pytest.fixture(scope="module")
def torch():
    import torch

    assert torch.cuda.is_available()
    return torch


@pytest.fixture(scope="module")
def L():
    from flacarray_amd import _lib

    return _lib.lib()


@pytest.fixture(scope="module")
def stores(oracle, torch):
    """name -> (Store, its device copies: blob, starts, nbytes, offsets, gains), each built at its first use; the device
    copies are released when the file ends."""
    made = {}

    def get(name):
        if name not in made:
            st = E.build_store(name, oracle)
            dev = {k: torch.from_numpy(np.ascontiguousarray(getattr(st, k))).cuda() for k in ("blob", "starts", "nbytes")}
            for k in ("offsets", "gains"):
                dev[k] = None if getattr(st, k) is None else torch.from_numpy(getattr(st, k)).cuda()
            assert dev["blob"].data_ptr() % 16 == 0
            made[name] = (st, dev)
        return made[name]

    yield get
    made.clear()


def _vp(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def _hp(a):
    return ctypes.c_void_p(a.ctypes.data)


class Harness:
    """One store, one entry point: runs a call into a fresh buffer of sentinel and compares the whole buffer."""

    def __init__(self, torch, L, st, dev, entry):
        self.torch, self.L, self.st, self.dev, self.entry = torch, L, st, dev, entry
        self.wide = st.channels == 2
        self.itemsize = 8 if self.wide else 4
        self.tdtype = torch.int64 if self.wide else torch.int32
        self.calls = 0
        self.index = None
        if entry.startswith("indexed"):
            self.index = ctypes.c_void_p()
            rc = L.fa_decode_index_create(_vp(dev["blob"]), st.blob.size, _vp(dev["starts"]), _vp(dev["nbytes"]), E.ROWS, st.n, st.channels,
                                          ctypes.byref(self.index), None)
            assert rc == 0 and self.index.value

    def close(self):
        if self.index is not None:
            self.torch.cuda.synchronize()
            self.L.fa_decode_index_destroy(self.index)
            self.index = None

    def run(self, what, span, m, placements, floats, call):
        """Fill a buffer for `span` elements behind the pointer, hand `call` the pointer base + (guard + m) elements and
        compare.  The buffer and the image are integer views: the comparison is on bits."""
        torch, st = self.torch, self.st
        total = E.buffer_elems(span)
        buf = torch.full((total,), E.sentinel_int(placements[0][1].dtype), dtype=self.tdtype, device="cuda")
        assert buf.data_ptr() % 16 == 0
        want = E.expected_image(total, E.GUARD, placements)
        want_d = torch.from_numpy(want.view(np.int64 if self.wide else np.int32)).cuda()
        out = ctypes.c_void_p(buf.data_ptr() + (E.GUARD + m) * self.itemsize)
        args = (None, out, _vp(self.dev["offsets"]), _vp(self.dev["gains"])) if floats else (out, None, None, None)
        torch.cuda.synchronize()
        rc = call(*args)
        torch.cuda.synchronize()
        self.calls += 1
        assert rc == 0, "%s: return code %d" % (what, rc)
        if not torch.equal(buf, want_d):
            pytest.fail("%s (%s, %s output, pointer %d elements off 16 bytes): %s" % (
                what, st.name, "float" if floats else "integer", m, E.check_image(buf.cpu().numpy(), want, E.GUARD, placements)))

    def window(self, first, last, m, floats):
        st, dev, L = self.st, self.dev, self.L

        def call(o_int, o_float, off, gain):
            if self.index is not None:
                return L.fa_decode_indexed(self.index, first, last, -1, None, None, None, None, o_int, o_float, off, gain, None, 0)
            fn = L.fa_decode_i64_device if self.wide else L.fa_decode_i32_device
            return fn(_vp(dev["blob"]), st.blob.size, _vp(dev["starts"]), _vp(dev["nbytes"]), E.ROWS, st.n, first, last, o_int, o_float, off, gain, None, 0)

        self.run("window [%d, %d)" % (first, last), m + E.ROWS * (last - first), m, E.window_placements(st, first, last, m, floats), floats, call)

    def batch(self, k, b, floats):
        st, dev, L = self.st, self.dev, self.L
        ss, ff, cc = (np.array(x, dtype=np.int64) for x in zip(*b.slices))
        oo = np.array(b.out_offset, dtype=np.int64)

        def call(o_int, o_float, off, gain):
            if self.index is not None:
                return L.fa_decode_indexed(self.index, -1, -1, len(b.slices), _hp(ss), _hp(ff), _hp(cc), _hp(oo), o_int, o_float, off, gain, None, b.verify)
            fn = L.fa_decode_slices_i64_device if self.wide else L.fa_decode_slices_i32_device
            return fn(_vp(dev["blob"]), st.blob.size, _vp(dev["starts"]), _vp(dev["nbytes"]), E.ROWS, st.n, len(b.slices), _hp(ss), _hp(ff), _hp(cc),
                      _hp(oo), o_int, o_float, off, gain, None, b.verify)

        what = "batch %d (%s, %d slices, first (stream, first, count) %s)" % (k, b.kind, len(b.slices), b.slices[0])
        self.run(what, b.span, b.m, E.batch_placements(st, b, floats), floats, call)


@pytest.mark.parametrize("latency", ["0", "1"], ids=["k7", "k7l"])
@pytest.mark.parametrize("entry", ENTRIES)
@pytest.mark.parametrize("name", E.STORES)
def test_footprint(torch, L, monkeypatch, stores, name, entry, latency):
    """Every window (grid entry points) or slice batch (slice entry points) of the store, integer output and -- where the
    store has offsets and gains -- float output: the buffer holds the samples at their places and the sentinel everywhere
    else."""
    st, dev = stores(name)
    monkeypatch.setenv("FLACARRAY_HIP_LATENCY", latency)
    w = E.width_of(st.channels)
    h = Harness(torch, L, st, dev, entry)
    try:
        for floats in (False, True) if st.floats is not None else (False,):
            if entry in ("device", "indexed_grid"):
                for first, last, m in E.windows(st.n, st.block, w):
                    h.window(first, last, m, floats)
            else:
                for k, b in enumerate(E.slice_batches(st.n, st.block, w)):
                    h.batch(k, b, floats)
    finally:
        h.close()
    print("footprint %s %s latency=%s: %d calls" % (st.name, entry, latency, h.calls))
