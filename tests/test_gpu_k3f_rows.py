"""The single-pass encoder's row writer (K3F) and the window prologue of its lag products: bytes against the CPU oracle on
frames that reach every path of the writer.

The writer places a frame's Rice codes row by row (512 samples, 8 per lane).  Where a partition is at least a row long
(partition order <= 3) the row has one Rice parameter, held in a scalar, and the partition's parameter field is written by
the wave at the row's first bit; for partition orders >= 4 every lane looks its parameter up and opens its own partitions.
Row 0 skips the warm-up samples, VERBATIM frames are written from memory, and blocks of a long frame are parked in
registers while the frame's byte offset is not known.  The catalogue below holds one frame (4096 samples) per path; the
oracle's decision trace is asserted to show each path, so that a case cannot pass by missing its branch.

Every array is small, so K3F is forced with FLACARRAY_HIP_PLACED_BELOW=0 (read per call).  A workgroup encodes four
consecutive frames of the call (frame g = stream * frames_per_stream + frame).
"""
import numpy as np
import pytest

from tests.conftest import full_range_i32, sinusoid_noise_f32, sinusoid_noise_i32

B = 4096
LEVELS = [3, 5, 8]  # maximum LPC order 6, 8, 12


@pytest.fixture(scope="module")
def fa():
    import flacarray_amd

    return flacarray_amd


@pytest.fixture(autouse=True)
def force_k3f(monkeypatch):
    monkeypatch.setenv("FLACARRAY_HIP_LATENCY", "0")
    monkeypatch.setenv("FLACARRAY_HIP_PLACED_BELOW", "0")


# ---- the catalogue: one frame per path of the writer -----------------------------------------------------------------------
def _bursts(stretch, amps, seed):
    """White noise whose amplitude changes every `stretch` samples: the partition search settles on partitions that long."""
    r = np.random.default_rng(seed)
    a = np.repeat(np.array(amps)[np.arange(B // stretch) % len(amps)], stretch)
    return np.rint(r.normal(size=B) * a).astype(np.int32)


def _cum(d, a, seed):
    """Noise integrated d times: FIXED order d."""
    x = np.random.default_rng(seed).integers(-a, a + 1, B).astype(np.int64)
    for _ in range(d):
        x = np.cumsum(x)
    assert np.abs(x).max() < 2**31
    return x.astype(np.int32)


def _ar(coef, amps, seed):
    r = np.random.default_rng(seed)
    e = np.repeat(np.array(amps)[np.arange(B // 128) % len(amps)], 128) * r.normal(size=B)
    y = np.zeros(B)
    for i in range(len(coef), B):
        y[i] = sum(c * y[i - 1 - j] for j, c in enumerate(coef)) + e[i]
    return np.rint(y).astype(np.int32)


def _catalogue():
    rng = np.random.default_rng(20)
    t = np.arange(B)
    noisy = sinusoid_noise_i32(1, 2 * B, seed=3)[0]
    frames = [
        ("noisy0", noisy[:B]),            # the headline workload's frame: LPC, partition order 0, k = 16 (5-bit field)
        ("noisy1", noisy[B:]),            # ... and the frame behind it in its stream (LPC order 8 at level 5)
        ("b128", _bursts(128, [4, 4000], 1)),             # partition order 5: neighbours of one row differ
        ("b128b", _bursts(128, [4, 60000, 300, 9], 2)),   # ... with k >= 15 among them
        ("b256", _bursts(256, [4, 4000], 3)),             # partition order 4
        ("b512", _bursts(512, [4, 4000], 4)),             # partition order 3: every row opens a partition
        ("b512b", _bursts(512, [3, 90000, 40, 2000], 5)),  # ... 5-bit fields
        ("b1024", _bursts(1024, [4, 4000], 6)),           # partition order 2: every second row opens one
        ("wide", rng.integers(-2**28, 2**28, B).astype(np.int32)),  # k = 27, 15 KB: blocks are parked
        ("near", rng.integers(-2**30, 2**30, B).astype(np.int32)),  # nearly full range: 16 KB, still Rice coded
        ("full", full_range_i32((B,), seed=5)),           # VERBATIM
        ("wasted", rng.integers(-3000, 3000, B).astype(np.int32) << 5),  # 5 wasted bits
        ("const", np.full(B, -4242, np.int32)),
        ("zero", np.zeros(B, np.int32)),
        ("tiny", rng.integers(-3, 4, B).astype(np.int32)),  # FIXED order 0
        ("cum1", _cum(1, 3, 31)),          # FIXED order 1
        ("cum2", _cum(2, 3, 32)),          # FIXED order 2
        ("cum3", _cum(3, 3, 33)),          # FIXED order 3
        ("sin4", np.rint(2**30 * np.sin(2 * np.pi * t / 200)).astype(np.int32)),  # FIXED order 4
        ("ar1", _ar([0.9], [50], 34)),     # LPC order 1
        ("arburst", _ar([1.6, -0.8], [3, 3000], 35)),  # LPC with partition order >= 5
        ("rampn", (3 * t + rng.integers(-2, 3, B)).astype(np.int32)),  # LPC of the highest order
    ]
    return frames


_CAT = None
_TRACE = {}


def _cat():
    global _CAT
    if _CAT is None:
        _CAT = _catalogue()
    return _CAT


def _trace(oracle, level):
    """The oracle's decisions for the catalogue's frames (computed once per level): name -> record."""
    if level not in _TRACE:
        names = [n for n, _ in _cat()]
        rec = oracle.stream_trace(np.concatenate([x for _, x in _cat()]), level)
        assert len(rec) == len(names)
        _TRACE[level] = dict(zip(names, rec))
    return _TRACE[level]


def _assert_branches(oracle, level):
    tr = _trace(oracle, level)
    rice = [r for r in tr.values() if r["type"] >= 2]
    porders = {r["porder"] for r in rice}
    hi = 5 if level > 3 else 4  # level 3 searches partition orders up to 4
    assert {0, 3, 4}.issubset(porders) and hi in porders, porders
    assert tr["b512"]["porder"] == 3 and tr["b256"]["porder"] == 4 and tr["b1024"]["porder"] == 2
    # neighbouring partitions of one row with different parameters: 128-sample bursts of alternating amplitude at
    # partitions of at most 256 samples (two to four partitions per row), k from 2 to 12
    r = tr["b128"] if level > 3 else tr["b128b"]
    assert r["porder"] >= 4 and r["rice_max"] - r["rice_min"] >= 8, r
    # the 5-bit parameter field, in both kinds of row
    assert tr["noisy0"]["porder"] == 0 and tr["noisy0"]["rice_max"] >= 15 and tr["noisy0"]["rice2"] == 1
    assert tr["b512b"]["porder"] == 3 and tr["b512b"]["rice_max"] >= 15 and tr["b512b"]["rice2"] == 1
    assert tr["b128b"]["porder"] >= 4 and tr["b128b"]["rice_max"] >= 15 and tr["b128b"]["rice2"] == 1
    lpc = {r["order"] for r in rice if r["type"] == 3}
    assert 1 in lpc, lpc
    if level == 5:  # (order 8 is the highest of level 5; level 3 stops at 6, level 8 prefers 10 and 11 on these frames)
        assert 8 in lpc, lpc
    assert max(lpc) >= (6 if level == 3 else 8 if level == 5 else 11)
    assert tr["arburst"]["type"] == 3
    if level >= 5:  # an LPC frame whose lanes look their parameters up
        assert tr["arburst"]["porder"] >= 4
    fixed = {r["order"] for r in rice if r["type"] == 2}
    assert fixed == {0, 1, 2, 3, 4}, fixed
    assert tr["full"]["type"] == 1
    assert tr["wasted"]["wasted"] == 5 and tr["wasted"]["type"] >= 2
    assert tr["const"]["type"] == 0 and tr["zero"]["type"] == 0
    # frames long enough to park blocks (the ring holds 16 blocks of 256 bytes)
    assert tr["near"]["type"] == 2 and tr["near"]["nbytes"] > 15000 and tr["wide"]["nbytes"] > 15000


# (streams, frames per stream, first catalogue frame): 1 to 8 streams of 4096 n samples, n <= 4.  The catalogue is laid
# out in order from its `first` frame on, wrapping round, so every shape holds other neighbours in its workgroups.
SHAPES = [(1, 1, 0), (1, 1, 8), (1, 4, 2), (3, 2, 5), (5, 3, 9), (8, 4, 0), (7, 3, 11), (2, 4, 14)]


def _array(n_stream, nf, first):
    cat = _cat()
    # long frames beside constants in one workgroup: "near", "const", "wide", "zero" lead every array of 8 frames or more
    lead = ["near", "const", "wide", "zero"] if n_stream * nf >= 8 else []
    by_name = dict(cat)
    frames = [by_name[n] for n in lead]
    i = first
    while len(frames) < n_stream * nf:
        frames.append(cat[i % len(cat)][1])
        i += 1
    return np.ascontiguousarray(np.concatenate(frames).reshape(n_stream, nf * B))


def _encode_device(fa, x, level):
    import torch

    comp, st, nb = fa.encode_flac_device(torch.from_numpy(x).cuda(), level=level)
    torch.cuda.synchronize()
    return comp.cpu().numpy(), st.cpu().numpy().reshape(-1), nb.cpu().numpy().reshape(-1)


def _assert_same(fa, oracle, x, level, what):
    blob_o, st_o, nb_o = oracle.encode_i32(x, level)
    blob_g, st_g, nb_g = _encode_device(fa, x, level)
    assert np.array_equal(nb_g, nb_o), (what, level, "stream sizes differ")
    assert np.array_equal(st_g, st_o), (what, level)
    assert np.array_equal(blob_g, blob_o), (what, level, "compressed bytes differ from the oracle")


# ---- the oracle alone ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("level", LEVELS)
def test_catalogue_reaches_every_branch(oracle, level):
    _assert_branches(oracle, level)
    for n_stream, nf, first in SHAPES:
        x = _array(n_stream, nf, first)
        assert 1 <= n_stream <= 8 and x.shape == (n_stream, nf * B) and nf <= 4
        blob, st, nb = oracle.encode_i32(x, level)
        assert np.array_equal(oracle.decode_i32(blob, st, nb, x.shape[1]), x)
    # the widest shape holds the whole catalogue, and a stream's first frame beside a later one
    assert 8 * 4 >= len(_cat()) + 4


# ---- the GPU against the oracle -------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("level", LEVELS)
@pytest.mark.parametrize("n_stream,nf,first", SHAPES, ids=[f"{s}x{f}@{i}" for s, f, i in SHAPES])
def test_rows_against_the_oracle(fa, oracle, n_stream, nf, first, level):
    _assert_branches(oracle, level)
    _assert_same(fa, oracle, _array(n_stream, nf, first), level, (n_stream, nf, first))


@pytest.mark.gpu
@pytest.mark.parametrize("level", LEVELS)
def test_every_frame_alone_and_as_first_and_later_frame(fa, oracle, level):
    """Every catalogue frame as a stream's first frame and, in the next stream, behind another frame."""
    _assert_branches(oracle, level)
    cat = _cat()
    for lo in range(0, len(cat), 4):
        part = [x for _, x in cat[lo : lo + 4]]
        rows = [np.concatenate([part[i], part[(i + 1) % len(part)]]) for i in range(len(part))]
        _assert_same(fa, oracle, np.ascontiguousarray(np.stack(rows)), level, ("pairs", lo))


@pytest.mark.gpu
@pytest.mark.parametrize("level", LEVELS)
def test_float32_input_kernel(fa, oracle, level):
    import torch

    cat = dict(_cat())
    names = ["b128", "b512", "tiny", "b256", "wasted", "cum2", "arburst", "b1024"]
    x = np.stack([np.concatenate([cat[n], cat[m]]) for n, m in zip(names, names[1:] + names[:1])]).astype(np.float32) * 2.0**-10
    x[1, B:] = sinusoid_noise_f32(1, B, seed=23)[0]
    x[5, :B] = 3.25  # a constant frame inside a stream
    x = np.ascontiguousarray(x)
    q = np.full(len(names), 2.0**-10, np.float32)
    io, offo, go = oracle.float32_to_int32(x, q)
    blob_o, st_o, nb_o = oracle.encode_i32(io, level)
    info = [fi for s in range(len(names)) for fi in oracle.stream_info(io[s], level)]
    porders = {fi["porder"] for fi in info if fi["type"] >= 2}
    assert {0, 3, 4}.issubset(porders), porders
    assert {fi["type"] for fi in info} >= {0, 2, 3}
    comp, st, nb, off, gain = fa.encode_flac_device_f32(torch.from_numpy(x).cuda(), torch.from_numpy(q), level=level)
    assert np.array_equal(off.cpu().numpy().view(np.uint32), offo.view(np.uint32))
    assert np.array_equal(gain.cpu().numpy().view(np.uint32), go.view(np.uint32))
    assert np.array_equal(nb.cpu().numpy().reshape(-1), nb_o) and np.array_equal(st.cpu().numpy().reshape(-1), st_o)
    assert np.array_equal(comp.cpu().numpy(), blob_o)
