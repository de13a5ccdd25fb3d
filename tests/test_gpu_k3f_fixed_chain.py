"""The FIXED analysis of the single-pass encoder (K3F) on its narrow path: bytes against the CPU oracle on frames that
reach every part of the alternating-sign chain.

For samples of at most 25 bits (-2^24 <= x < 2^24) K3F sums |e_k| of the fixed predictors k = 0..4 in 32-bit integer
arithmetic.  The chain keeps (-1)^t e_k(t), sign-biased, so that each further order is one addition (encode_fused.hpp,
FA_F_ALTSIGN).  What can go wrong there and is driven here: the seeds of a lane's chunk (samples 32 l - 4 .. 32 l - 1,
negated by parity), the seam between the halves A (LDS) and B (registers) at sample 2048, the frame seam, the masks of the
first group (order k sums from sample k on), the range (|e_4| reaches 2^28 - 8, a 16-sample partial sum 2^32 - 128), the
switch to the wide path and back, wasted bits, the three kernels of the maximum LPC orders 6 / 8 / 12 and float32 input.

The reference of every case is the oracle's bytes.  Every case is a stream of two 4096-sample frames (the smallest shape
K3F takes) and also runs through the slot sequence (FLACARRAY_HIP_SLOTS=1) as a second witness.  The oracle's decision
trace is asserted, without a GPU, to show what each input is built for.
"""
import numpy as np
import pytest

from tests.encoder_corpus import wasted_frame

B = 4096
LO, HI = -(2**24), 2**24 - 1  # the narrow path's range
LEVELS = [3, 5, 8]  # maximum LPC order 6, 8, 12


@pytest.fixture(scope="module")
def fa():
    import flacarray_amd

    return flacarray_amd


@pytest.fixture(autouse=True)
def force_k3f(monkeypatch):
    monkeypatch.setenv("FLACARRAY_HIP_LATENCY", "0")
    monkeypatch.setenv("FLACARRAY_HIP_PLACED_BELOW", "0")
    monkeypatch.delenv("FLACARRAY_HIP_SLOTS", raising=False)


# ---- the plain definition -----------------------------------------------------------------------------------------------
def fixed_totals(x, unmasked=()):
    """sum over t >= k of |e_k(t)|, k = 0..4, of one frame (oracle/flac_oracle.c, encode_subframe).  Orders listed in
    `unmasked` also count t < k, with zeros in front of the frame: what a missing mask of the first group would give."""
    e = np.concatenate([np.zeros(4, np.int64), np.asarray(x, np.int64)])
    out = []
    for k in range(5):
        d = e.copy()
        for _ in range(k):
            d = np.concatenate([[0], np.diff(d)])
        d = np.abs(d[4:])
        out.append(int(d.sum() if k in unmasked else d[k:].sum()))
    return out


def best_order(tot):
    return min(range(5), key=lambda k: (tot[k], k))  # strict <, lowest order first


# ---- frames ---------------------------------------------------------------------------------------------------------------
def _noise(seed, a=3):
    return np.random.default_rng(seed).integers(-a, a + 1, B).astype(np.int64)


def _sine(period, noise, seed):
    return np.rint(2.0**23 * np.sin(2 * np.pi * np.arange(B) / period + 0.7)).astype(np.int64) + _noise(seed, noise)


def order_frame(k, seed):
    """A frame of the narrow range on which FIXED order k wins the frame: noise (0), noise integrated once and twice (1, 2),
    a slow sinusoid whose third (3) or fourth (4) difference falls below the rounding noise."""
    if k <= 2:
        v = _noise(seed)
        for _ in range(k):
            v = np.cumsum(v)
        return v
    return _sine(1200, 0, seed) if k == 3 else _sine(200, 2, seed)


def _i32(frames):
    x = np.stack([np.concatenate(p) for p in frames])
    assert x.min() >= -(2**31) and x.max() < 2**31 and x.shape[1] == 2 * B and x.shape[0] <= 8
    return np.ascontiguousarray(x.astype(np.int32))


def orders_array():
    """Stream k: FIXED order k in both frames; streams 5..7 mix the orders so that a workgroup holds different winners."""
    f = [[order_frame(k, 40 + k), order_frame(k, 50 + k)] for k in range(5)]
    f += [[order_frame(4, 61), order_frame(0, 62)], [order_frame(1, 63), order_frame(3, 64)], [order_frame(2, 65), order_frame(4, 66)]]
    return _i32(f), [(0, 0), (1, 1), (2, 2), (3, 3), (4, 4), (4, 0), (1, 3), (2, 4)]


def warmup_array():
    """Large values in samples 0..3 only.  Streams 0..3: order k = stream + 1 wins on the rest of the frame and sample 0
    alone stands 2^18 off its neighbours: every order k >= 1 meets it once, at t = k, with weight 1, so the winner stays
    and the frame stays FIXED -- but a sum of order k that also counted t < k would grow by (2^k - 1) 2^18 and lose.
    Streams 4..7: samples 0..j at the ends of the range, +-2^24, alternating (those frames go to LPC)."""
    f = []
    for k in range(1, 5):
        a, b = order_frame(k, 70 + k), order_frame(k, 85 + k)
        a[0], b[0] = a[4] + 2**18, b[4] - 2**18
        f.append([a, b])
    for j in range(4):
        a, b = order_frame(3, 90 + j), order_frame(0, 95 + j)
        a[: j + 1] = [HI, LO, HI, LO][: j + 1]
        b[: j + 1] = [LO, HI, LO, HI][: j + 1]
        f.append([a, b])
    return _i32(f)


PATTERNS = {1: [HI], 2: [LO, HI], 3: [LO, HI, HI], 4: [LO, LO, HI, HI]}
SEAMS = [(30, 35), (2046, 2051), (4094, 4098)]  # a lane's seed, the A / B seam with lane 0's uniform read, the frame seam


def extremes_array():
    """-2^24 and 2^24 - 1 in patterns of period 1..4 across stream samples 30..34, 2046..2050 and 4094..4097, on small noise;
    each period once in phase with an even index and once with an odd one (streams p - 1 and p + 3)."""
    f = []
    for phase in (0, 1):
        for p in (1, 2, 3, 4):
            s = np.concatenate([_noise(100 + 4 * phase + p), _noise(110 + 4 * phase + p)])
            for lo, hi in SEAMS:
                for i in range(lo, hi):
                    s[i] = PATTERNS[p][(i + phase) % p] if p > 1 else (HI, LO)[phase]
            f.append([s[:B], s[B:]])
    return _i32(f)


def full_extremes_array():
    """Whole frames of the patterns: the alternating one holds |e_4| = 2^28 - 8 in every sample, so every 16-sample partial
    sum of order 4 is 2^32 - 128; the frame behind it starts on the other parity of the pattern."""
    f = []
    for p in (1, 2, 3, 4):
        s = np.array([PATTERNS[p][i % p] for i in range(2 * B + 1)], np.int64)
        if p == 1:
            s[1::7] = LO  # (a constant frame would not reach the analysis)
        f.append([s[:B], s[B + 1 : 2 * B + 1] if p % 2 == 0 else s[B : 2 * B]])
    return _i32(f)


def switch_array():
    """Stream 0: one sample equal to 2^24 puts frame 0 on the wide path, frame 1 is narrow again; stream 1 the other way
    round, -2^24 - 1; streams 2, 3: the narrow extremes beside them.  Streams 4..7: wasted bits 1 and 7 on narrow data."""
    def ext(seed, v, at):
        s = order_frame(2, seed)
        s[at] = v
        return s

    f = [[ext(120, 2**24, 33), ext(121, HI, 33)], [ext(122, LO, 2047), ext(123, LO - 1, 2047)],
         [ext(124, HI, 0), ext(125, 2**24, 4095)], [ext(126, LO - 1, 0), ext(127, LO, 1)]]
    for i, w in enumerate((1, 7, 7, 1)):
        f.append([wasted_frame(130 + i, w).astype(np.int64), wasted_frame(140 + i, 8 - w).astype(np.int64)])
    return _i32(f), [(1, 7), (7, 1), (7, 1), (1, 7)]


def lane_sum_array():
    """Frames of alternating +-A with A = 2^20 - 1, 2^20, 2^20 + 1: a lane's 64 samples sum (order 0) to just below, at
    and just above 2^26, the wave's 4096 to just below, at and above 2^32 (streams 0..2); streams 3..5: the same with only
    lane 63's chunks (samples 2016..2047 and 4064..4095) at A, the rest at 2^19."""
    f = []
    sign = np.where(np.arange(B) % 2 == 0, 1, -1).astype(np.int64)
    for only63 in (False, True):
        for A in (2**20 - 1, 2**20, 2**20 + 1):
            a = np.full(B, A if not only63 else 2**19, np.int64)
            if only63:
                a[2016:2048] = A
                a[4064:4096] = A
            f.append([a * sign, -(a * sign)])
    return _i32(f)


ARRAYS = {
    "orders": lambda: orders_array()[0],
    "warmup": warmup_array,
    "extremes": extremes_array,
    "full_extremes": full_extremes_array,
    "switch": lambda: switch_array()[0],
    "lane_sums": lane_sum_array,
}
_CACHE = {}


def _array(name):
    if name not in _CACHE:
        _CACHE[name] = ARRAYS[name]()
    return _CACHE[name]


def _reference(oracle, name, level):
    """The oracle's bytes, computed once per array and level and shared by the routes."""
    if (name, level) not in _CACHE:
        _CACHE[(name, level)] = oracle.encode_i32(_array(name), level)
    return _CACHE[(name, level)]


def _traces(oracle, name, level):
    return [oracle.stream_trace(s, level) for s in _array(name)]


# ---- the oracle alone: every input shows what it is built for -------------------------------------------------------------
@pytest.mark.parametrize("level", LEVELS)
def test_each_fixed_order_wins(oracle, level):
    x, want = orders_array()
    assert LO <= x.min() and x.max() <= HI
    for s, tr in enumerate(_traces(oracle, "orders", level)):
        for fr in (0, 1):
            assert tr[fr]["type"] == 2 and tr[fr]["order"] == want[s][fr] and tr[fr]["fixed_valid"] == 31, (s, fr, tr[fr])
            assert best_order(fixed_totals(x[s, fr * B : (fr + 1) * B])) == want[s][fr]


def test_warmup_inputs_depend_on_the_masks(oracle):
    x = warmup_array()
    assert LO <= x.min() and x.max() <= HI
    tr = _traces(oracle, "warmup", 5)
    for s in range(8):
        for fr in (0, 1):
            frame = x[s, fr * B : (fr + 1) * B]
            assert np.abs(frame[4:]).max() < 2**23 + 8 and abs(int(frame[0]) - int(frame[4])) >= 2**18
            fo = best_order(fixed_totals(frame))
            assert tr[s][fr]["fixed_order"] == fo and tr[s][fr]["fixed_valid"] == 31, (s, fr, tr[s][fr])
            if s < 4:  # order s + 1 wins the frame, and would not if its own first group were unmasked
                assert fo == s + 1 and tr[s][fr]["type"] == 2 and tr[s][fr]["order"] == fo, (s, fr, tr[s][fr])
                assert best_order(fixed_totals(frame, unmasked=(fo,))) != fo
    # samples 0..j large: the winner changes when all masks go
    assert any(best_order(fixed_totals(x[s, :B], unmasked=(1, 2, 3, 4))) != tr[s][0]["fixed_order"] for s in range(4, 8))


def test_extremes_stay_on_the_narrow_range(oracle):
    for name in ("extremes", "full_extremes"):
        x = _array(name)
        assert x.min() == LO and x.max() == HI
        for s, tr in enumerate(_traces(oracle, name, 5)):
            for fr in (0, 1):
                assert tr[fr]["is_const"] == 0 and tr[fr]["fixed_valid"] == 31 and tr[fr]["wasted"] == 0, (name, s, fr, tr[fr])
    x = _array("extremes")
    for s in range(8):  # the patterns sit where they are meant to, in both phases
        p, phase = s % 4 + 1, s // 4
        for lo, hi in SEAMS:
            assert np.all(np.abs(x[s, lo:hi].astype(np.int64)) >= HI)
            if p == 2:
                assert np.array_equal(x[s, lo:hi], [PATTERNS[2][(i + phase) % 2] for i in range(lo, hi)])
    # the alternating frame reaches the range's end: |e_4| = 2^28 - 8, sixteen of them stay below 2^32
    alt = _array("full_extremes")[1, :B].astype(np.int64)
    e4 = np.abs(np.diff(alt, 4))
    assert e4.max() == 2**28 - 8 and 16 * int(e4.max()) < 2**32


def test_switch_inputs(oracle):
    x, wasted = switch_array()
    inside = [[(LO <= x[s, fr * B : (fr + 1) * B].min()) and (x[s, fr * B : (fr + 1) * B].max() <= HI) for fr in (0, 1)] for s in range(4)]
    assert inside == [[False, True], [True, False], [True, False], [False, True]]
    tr = _traces(oracle, "switch", 5)
    for s in range(4):
        assert all(tr[s][fr]["type"] >= 2 and tr[s][fr]["fixed_valid"] == 31 for fr in (0, 1))
    for i, w in enumerate(wasted):
        assert (tr[4 + i][0]["wasted"], tr[4 + i][1]["wasted"]) == w
        assert np.abs(x[4 + i].astype(np.int64)).max() <= HI


def test_lane_sum_inputs(oracle):
    x = lane_sum_array().astype(np.int64)
    lane = np.abs(x[:, :B]).reshape(6, 2, 64, 32).sum(axis=(1, 3))  # [stream, lane]: chunks A_l and B_l
    assert [int(v) for v in lane[:3, 0]] == [2**26 - 64, 2**26, 2**26 + 64]
    assert [int(v) for v in lane[3:, 63]] == [2**26 - 64, 2**26, 2**26 + 64] and lane[3:, :63].max() == 2**25
    assert [int(np.abs(x[s, :B]).sum()) - 2**32 for s in range(3)] == [-4096, 0, 4096]
    for tr in _traces(oracle, "lane_sums", 5):
        assert all(r["fixed_valid"] == 31 and r["is_const"] == 0 for r in tr)


# ---- the GPU against the oracle -------------------------------------------------------------------------------------------
def _encode_device(fa, x, level):
    import torch

    comp, st, nb = fa.encode_flac_device(torch.from_numpy(x).cuda(), level=level)
    torch.cuda.synchronize()
    return comp.cpu().numpy(), st.cpu().numpy().reshape(-1), nb.cpu().numpy().reshape(-1)


def _assert_both_routes(fa, oracle, monkeypatch, name, level):
    blob_o, st_o, nb_o = _reference(oracle, name, level)
    for slots in (False, True):
        if slots:
            monkeypatch.setenv("FLACARRAY_HIP_SLOTS", "1")
        blob_g, st_g, nb_g = _encode_device(fa, _array(name), level)
        what = (name, level, "slot sequence" if slots else "K3F")
        assert np.array_equal(nb_g, nb_o), (what, "stream sizes differ")
        assert np.array_equal(st_g, st_o), what
        assert np.array_equal(blob_g, blob_o), (what, "compressed bytes differ from the oracle")


@pytest.mark.gpu
@pytest.mark.parametrize("level", LEVELS)
@pytest.mark.parametrize("name", sorted(ARRAYS))
def test_fixed_chain_against_the_oracle(fa, oracle, monkeypatch, name, level):
    _assert_both_routes(fa, oracle, monkeypatch, name, level)


@pytest.mark.gpu
@pytest.mark.parametrize("level", LEVELS)
def test_float32_input_kernel(fa, oracle, monkeypatch, level):
    """The float32 kernels quantise on the way in: multiples of 2^-10 with quantum 2^-10 give back the integers."""
    import torch

    xi = np.concatenate([_array("extremes")[[1, 5]], _array("full_extremes")[[1, 2]], _array("orders")[[3, 4]], _array("warmup")[[2, 7]]])
    x = np.ascontiguousarray(xi.astype(np.float32) * np.float32(2.0**-10))
    q = np.full(len(x), 2.0**-10, np.float32)
    io, offo, go = oracle.float32_to_int32(x, q)
    blob_o, st_o, nb_o = oracle.encode_i32(io, level)
    info = [fi for s in range(len(x)) for fi in oracle.stream_info(io[s], level)]
    assert {fi["type"] for fi in info} >= {2} and np.abs(io.astype(np.int64)).max() <= 2**25
    for slots in (False, True):
        if slots:
            monkeypatch.setenv("FLACARRAY_HIP_SLOTS", "1")
        comp, st, nb, off, gain = fa.encode_flac_device_f32(torch.from_numpy(x).cuda(), torch.from_numpy(q), level=level)
        assert np.array_equal(off.cpu().numpy().view(np.uint32), offo.view(np.uint32))
        assert np.array_equal(gain.cpu().numpy().view(np.uint32), go.view(np.uint32))
        assert np.array_equal(nb.cpu().numpy().reshape(-1), nb_o) and np.array_equal(st.cpu().numpy().reshape(-1), st_o)
        assert np.array_equal(comp.cpu().numpy(), blob_o), ("slot sequence" if slots else "K3F", level)
