"""The compare sink (compare_flac_device, FlacArray.first_mismatch) on streams this library did not write: the
libFLAC-shaped corpus of tests/golden/flac_writer.py (LPC orders 1-32, so the deep-history compare passes run; blocks 16
to 65535; every metadata layout; channel assignments 1 / 8 / 9 / 10) and the replicated stores of tests/compare_corpus.py,
where row r differs at sample r, so that one call shows every sample of every frame being compared -- on the whole-tile
path, the per-piece path, unaligned rows, the short last frame, wasted-bits frames and the warm-up samples of orders above
16.  Expected results are numpy on the known arrays (tests/test_compare_corpus.py checks their preconditions)."""
import numpy as np
import pytest

from tests import compare_corpus as C
from tests import quant_model as M
from tests.compare_corpus import _frame_offsets, _header_bytes
from tests.golden import flac_writer as W

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def torch():
    import torch

    assert torch.cuda.is_available()
    return torch


@pytest.fixture(scope="module")
def fa():
    import flacarray_amd

    return flacarray_amd


@pytest.fixture(scope="module")
def batches():
    return W.all_batches()


@pytest.fixture(scope="module")
def reps():
    out = {name: C.replicated(**g) for name, g in C.GEOMETRIES.items()}
    out.update({name: C.uniform(name) for name in C.UNIFORM})
    return out


@pytest.fixture(scope="module")
def small():
    """The small-amplitude stores of the float tests: the two mixed-order lengths and the one-bucket streams."""
    out = {name: C.small_amplitude(n) for name, n in C.SMALL_LENGTHS.items()}
    out.update({name: C.uniform(name) for name in C.UNIFORM})
    return out


@pytest.fixture(autouse=True, params=["default", "serial_walk"])
def dispatch(request, monkeypatch):
    """serial_walk: the parallel sync-code scan switched off, so streams without a complete SEEKTABLE are located by the
    serial frame walk (the variable is read per call).  Compare always takes K7's grid path."""
    monkeypatch.delenv("FLACARRAY_HIP_NO_SYNC_SCAN", raising=False)
    if request.param == "serial_walk":
        monkeypatch.setenv("FLACARRAY_HIP_NO_SYNC_SCAN", "1")
    return request.param


def _up(torch, *arrays):
    return tuple(torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in arrays)


def _compare(fa, torch, d, x, offsets=None, gains=None):
    og = (None, None) if offsets is None else _up(torch, offsets, gains)
    return fa.compare_flac_device(*d, _up(torch, x)[0], *og).cpu().numpy()


def _single_block(batches):
    return [b for b in batches if b["block"] is not None]


def _each(batches, check):
    """Run check(batch) on every batch; report every batch that fails, not just the first."""
    failed = []
    for b in batches:
        try:
            check(b)
        except (AssertionError, RuntimeError) as e:
            failed.append((b["name"], type(e).__name__, str(e).splitlines()[0][:200] if str(e) else ""))
    assert not failed, "%d of %d batches fail: %s" % (len(failed), len(batches), failed)


def _where(got, want):
    """Assertion text: the rows that differ, with what they gave and what was expected."""
    bad = np.flatnonzero(np.asarray(got) != np.asarray(want))
    return "%d rows differ, (row, got, want): %s" % (bad.size, [(int(r), int(got[r]), int(want[r])) for r in bad[:12]])


def test_intact_corpus(fa, torch, batches):
    def check(b):
        d = _up(torch, *W.pack(b["streams"]))
        got = _compare(fa, torch, d, b["samples"])
        assert got.shape == (len(b["streams"]),) and (got == -1).all(), (b["name"], got.tolist())

    _each(_single_block(batches), check)
    mixed = [b for b in batches if b["block"] is None]
    assert [b["name"] for b in mixed] == ["mixed_blocks"]
    b = mixed[0]
    with pytest.raises(RuntimeError, match="return code = 8192"):
        _compare(fa, torch, _up(torch, *W.pack(b["streams"])), b["samples"])
    blocks = [r["block"] for r in b["records"]]
    assert len(set(blocks)) == 4
    for block in sorted(set(blocks)):
        idx = [i for i, v in enumerate(blocks) if v == block]
        got = _compare(fa, torch, _up(torch, *W.pack([b["streams"][i] for i in idx])), b["samples"][idx])
        assert (got == -1).all(), (block, got.tolist())


@pytest.mark.parametrize("channels", [1, 2])
def test_edge_mutations_over_the_corpus(fa, torch, batches, channels):
    """Rotation j changes stream i at positions(n, block)[(i + j) % len], so every stream meets every frame, tile and
    piece edge; two-channel samples with bit 0 (left), bit 32 (right) and bit 63 (right's sign) in turn.  The rotations of
    a batch go into one call, each on a copy of the batch's streams: K7 decodes a frame per lane, so a call on one
    65535-sample frame takes as long as a call on hundreds of them, and a call per rotation would take 18 times as long."""
    def check(b):
        x, n, block = b["samples"], b["n"], b["block"]
        rot = len(C.positions(n, block))
        d = _up(torch, *W.pack(b["streams"] * rot))
        orig = np.tile(x, (rot, 1))
        for bit in C.XOR_BITS[channels]:
            y = C.edge_rotations(x, n, block, bit)
            want = C.expected_first(y, orig)
            assert sorted(want[:: x.shape[0]].tolist()) == C.positions(n, block)  # stream 0 met every position
            got = _compare(fa, torch, d, y)
            assert np.array_equal(got, want), (b["name"], int(bit), _where(got, want))

    sel = [b for b in _single_block(batches) if b["channels"] == channels and b["name"] != "utf8_4byte"]
    assert len(sel) >= 20 and {b["block"] for b in sel} == set(W.BLOCK_SIZES)
    _each(sel, check)


@pytest.mark.parametrize("name", list(C.GEOMETRIES) + list(C.UNIFORM))
def test_every_sample_is_compared(fa, torch, reps, name):
    """The mixed-order stores take the per-piece path (every wave holds frames of another pass and short frames), the
    one-bucket stores the whole-tile path of their pass."""
    rep = reps[name]
    n = rep.n
    d = _up(torch, *C.store(rep))
    data = C.rows(rep)
    got = _compare(fa, torch, d, data)
    assert (got == -1).all(), _where(got, np.full(n, -1))
    every = np.arange(n)
    bits = C.XOR_BITS[rep.channels] + ((np.int32(-(2**31)),) if rep.channels == 1 else ())
    for bit in bits:  # (bit 0 also flips a wasted-bits frame's zeroed low bits)
        y = C.xor_diagonal(data, bit)
        assert np.array_equal(C.expected_first(y, data), every)
        got = _compare(fa, torch, d, y)
        assert np.array_equal(got, every), ("xor", int(bit), _where(got, every))
    y = C.add_from_diagonal(data, 7)
    assert np.array_equal(C.expected_first(y, data), every)
    got = _compare(fa, torch, d, y)
    assert np.array_equal(got, every), ("from r on", _where(got, every))
    y = C.add_from_diagonal(data, 7, skip=1)
    want = C.expected_first(y, data)
    assert np.array_equal(want[:-1], every[1:]) and want[-1] == -1
    got = _compare(fa, torch, d, y)
    assert np.array_equal(got, want), ("after r", _where(got, want))


@pytest.mark.parametrize("name", list(C.SMALL_LENGTHS) + list(C.UNIFORM))
def test_float32_sink(fa, torch, small, name):
    rep = small[name]
    n = rep.n
    d = _up(torch, *C.store(rep))
    x, ints, off, gain = C.float_case(rep)
    got = _compare(fa, torch, d, x, off, gain)
    assert (got == -1).all(), _where(got, np.full(n, -1))
    y = C.bump_diagonal(x, 1.5 * C.QUANTA)
    want = C.expected_first(M.quantise_with(y, off, gain), ints)
    assert np.array_equal(want, np.arange(n))
    got = _compare(fa, torch, d, y, off, gain)
    assert np.array_equal(got, want), _where(got, want)
    # the next float up, kept where the model says the integer stays: not a mismatch
    z = C.nextafter_diagonal(x)
    moved = C.expected_first(M.quantise_with(z, off, gain), ints) >= 0
    assert moved.sum() <= n // 10, "%d of %d nextafter rows change their integer and are dropped" % (moved.sum(), n)
    z[moved] = x[moved]
    assert np.count_nonzero(z.view(np.uint32) != x.view(np.uint32)) == n - moved.sum()
    got = _compare(fa, torch, d, z, off, gain)
    assert (got == -1).all(), _where(got, np.full(n, -1))


def test_rejected_deep_frame(fa, torch):
    """A flipped bit in the CRC-8-covered header of frame 3 (LPC order 17-32) of one row: the frame is rejected before
    anything of it is decoded, and its stream is marked at the frame's first sample or earlier."""
    rep = C.replicated(layout="own", **C.GEOMETRIES["mono192_unaligned"])
    k, s = 6, 4
    blob, st, nb = C.store(rep, rows=k)
    seg = blob[st[s] : st[s] + nb[s]]
    offs = _frame_offsets(seg)
    assert len(offs) == rep.record["frames"] == 9
    at = offs[3]
    assert _header_bytes(seg, at) == 6  # sync, two code bytes, assignment and size, the frame number, CRC-8
    blob[st[s] + at + 3] ^= 0x10  # frame 3's channel assignment (its CRC-8 no longer matches)
    got = _compare(fa, torch, _up(torch, blob, st, nb), C.rows(rep, k))
    assert 0 <= got[s] <= 3 * 192, got.tolist()
    assert (np.delete(got, s) == -1).all(), got.tolist()


def test_first_mismatch_on_a_foreign_store(fa, torch, batches):
    b = {bb["name"]: bb for bb in batches}["deep_mix_1"]
    x, n, block = b["samples"], b["n"], b["block"]
    blob, st, nb = W.pack(b["streams"])
    a = fa.FlacArray._assemble(x.shape, None, np.int32, blob, st, nb, None, None)
    muts = [C.edge_mutation(x, n, block, j, np.int32(1)) for j in range(len(C.positions(n, block)))]
    for resident in (False, True):
        if resident:
            a.to_device()
        assert (a.first_mismatch(x) == -1).all(), resident
        for j, y in enumerate(muts):
            got, want = a.first_mismatch(y), C.expected_first(y, x)
            assert np.array_equal(got, want), (resident, j, got.tolist(), want.tolist())
        assert np.array_equal(a.first_mismatch(torch.from_numpy(muts[0]).cuda()), C.expected_first(muts[0], x)), resident
    a.release_device()
