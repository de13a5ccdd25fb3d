"""The single-pass encoder's shared LPC solve (K3F, FA_F_SHLEV): encoder bytes against the CPU oracle on inputs that reach
every path of the hand-over between the four waves of a workgroup.

One wave of a workgroup solves the LPC problems (Levinson-Durbin, order choice, coefficient quantisation) of all four
frames; every wave announces itself with its lag sums or with "no LPC candidate", and a wave without a frame announces
before it leaves.  A workgroup holds four consecutive frames of the call (frame g = stream * frames_per_stream + frame;
frames 4 t .. 4 t + 3 share a workgroup), so the cases below place the frames by their number:

* frame counts per call that are 1, 2 and 3 modulo 4: the last workgroup has waves that leave at once;
* streams of 4096 k + 576 samples: every stream's last frame belongs to the slot encoder, its wave leaves at once;
* constant, all-zero, "all-zero lag sums" and FIXED frames among noisy ones inside one workgroup, in every position 0..3,
  alone, in pairs and in threes; workgroups whose four frames are all constant or all zero;
* levels 3, 5 and 8 (maximum LPC order 6, 8, 12) and the float32 input kernel.

The arrays are small, so K3F is forced with FLACARRAY_HIP_PLACED_BELOW=0 (read per call).  The decisions the inputs are
built for (constant = type 0, FIXED = 2, LPC = 3) are checked on the oracle alone, without a GPU.
"""
import numpy as np
import pytest

from tests.conftest import sinusoid_noise_f32, sinusoid_noise_i32

B = 4096
LEVELS = [3, 5, 8]


@pytest.fixture(scope="module")
def fa():
    import flacarray_amd

    return flacarray_amd


@pytest.fixture(autouse=True)
def force_k3f(monkeypatch):
    monkeypatch.setenv("FLACARRAY_HIP_LATENCY", "0")
    monkeypatch.setenv("FLACARRAY_HIP_PLACED_BELOW", "0")


# ---- frames by kind -----------------------------------------------------------------------------------------------------
def _frame(kind, seed):
    rng = np.random.default_rng(1000 + seed)
    if kind == "noisy":  # the headline workload's kind of frame: LPC
        return sinusoid_noise_i32(1, B, seed=seed)[0]
    if kind == "const":
        return np.full(B, 12345 - 7 * seed, np.int32)
    if kind == "zero":
        return np.zeros(B, np.int32)
    if kind == "impulse":  # not constant, but the window is zero at sample 0: all lag sums are zero, no LPC candidate
        x = np.zeros(B, np.int32)
        x[0] = 5
        return x
    if kind == "tiny":  # white noise of a few counts: no predictor helps, FIXED order 0
        return rng.integers(-3, 4, B).astype(np.int32)
    raise ValueError(kind)


# every workgroup of the mixed stream, as the kinds of its frames 0..3
def _mixed_groups():
    groups = []
    for kind in ("const", "zero", "impulse", "tiny"):
        for p in range(4):  # one special frame, in every position
            groups.append(["noisy"] * p + [kind] + ["noisy"] * (3 - p))
    for p, q in ((0, 1), (2, 3), (0, 3), (1, 2), (0, 2), (1, 3)):  # two
        g = ["noisy"] * 4
        g[p], g[q] = "const", "zero"
        groups.append(g)
    for p in range(4):  # three: the only frame with an LPC candidate in every position
        g = ["const", "zero", "impulse", "const"]
        g[p] = "noisy"
        groups.append(g)
    groups.append(["const"] * 4)
    groups.append(["zero"] * 4)
    groups.append(["const", "zero", "zero", "const"])
    groups.append(["impulse", "const", "tiny", "zero"])  # nobody has an LPC candidate, two frames run the FIXED analysis
    return groups


def _mixed_stream():
    kinds = [k for g in _mixed_groups() for k in g]
    x = np.concatenate([_frame(k, i) for i, k in enumerate(kinds)])
    return x.reshape(1, -1), kinds


def _mod4_cases():
    # (streams, frames per stream): 1, 2, 3, 5, 6, 7, 9, 11 frames per call
    return [(1, 1), (1, 2), (3, 1), (5, 1), (3, 2), (7, 1), (3, 3), (11, 1)]


def _tail_cases():
    # (streams, whole frames per stream) of streams of 4096 k + 576 samples
    return [(1, 1), (3, 2), (5, 1), (2, 3), (4, 4)]


def _noisy_with_specials(n_stream, n, seed):
    """Noisy streams with a constant and an all-zero whole frame dropped in where the geometry has room."""
    x = sinusoid_noise_i32(n_stream, n, seed=seed)
    nf = n // B
    if n_stream * nf >= 3:
        x[n_stream // 2, (nf // 2) * B : (nf // 2 + 1) * B] = -4242
    if n_stream * nf >= 6:
        x[n_stream - 1, (nf - 1) * B : nf * B] = 0
    return np.ascontiguousarray(x)


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


# ---- the oracle alone: the inputs encode, and the decisions they were built for occur ----------------------------------------
@pytest.mark.parametrize("level", LEVELS)
def test_inputs_reach_the_intended_decisions(oracle, level):
    x, kinds = _mixed_stream()
    blob, st, nb = oracle.encode_i32(x, level)
    assert np.array_equal(oracle.decode_i32(blob, st, nb, x.shape[1]), x)
    info = oracle.stream_info(x[0], level)
    assert len(info) == len(kinds)
    want = {"noisy": 3, "const": 0, "zero": 0, "tiny": 2, "impulse": 2}
    for f, k in enumerate(kinds):
        assert info[f]["type"] == want[k], (f, k, info[f])
    for n_stream, nf in _mod4_cases():
        assert (n_stream * nf) % 4 != 0
        xs = _noisy_with_specials(n_stream, nf * B, seed=50 + n_stream)
        types = [fi["type"] for s in range(n_stream) for fi in oracle.stream_info(xs[s], level)]
        assert 3 in types and all(t in (0, 3) for t in types)
    for n_stream, k in _tail_cases():
        xs = _noisy_with_specials(n_stream, k * B + 576, seed=70 + n_stream)
        info = oracle.stream_info(xs[0], level)
        assert len(info) == k + 1 and info[-1]["blocksize"] == 576


# ---- the GPU against the oracle ----------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("level", LEVELS)
@pytest.mark.parametrize("n_stream,nf", _mod4_cases(), ids=[f"{s}x{f}" for s, f in _mod4_cases()])
def test_frame_counts_not_a_multiple_of_four(fa, oracle, n_stream, nf, level):
    _assert_same(fa, oracle, _noisy_with_specials(n_stream, nf * B, seed=50 + n_stream), level, (n_stream, nf))


@pytest.mark.gpu
@pytest.mark.parametrize("level", LEVELS)
@pytest.mark.parametrize("n_stream,k", _tail_cases(), ids=[f"{s}x{k}" for s, k in _tail_cases()])
def test_short_last_frames(fa, oracle, n_stream, k, level):
    _assert_same(fa, oracle, _noisy_with_specials(n_stream, k * B + 576, seed=70 + n_stream), level, (n_stream, k))


@pytest.mark.gpu
@pytest.mark.parametrize("level", LEVELS)
def test_frames_without_an_lpc_candidate_in_every_position(fa, oracle, level):
    x, kinds = _mixed_stream()
    _assert_same(fa, oracle, x, level, "mixed")
    # the same frames behind one frame more: every workgroup's composition moves by one position
    x1 = np.ascontiguousarray(np.concatenate([_frame("noisy", 999)[None, :], x], axis=1))
    _assert_same(fa, oracle, x1, level, "mixed + 1")
    # and as four streams (the workgroups do not care where a stream ends)
    n4 = (x.shape[1] // (4 * B)) * B
    _assert_same(fa, oracle, np.ascontiguousarray(x[0, : 4 * n4].reshape(4, n4)), level, "mixed as 4 streams")


@pytest.mark.gpu
@pytest.mark.parametrize("level", LEVELS)
def test_float32_input_kernel(fa, oracle, level):
    import torch

    x = sinusoid_noise_f32(7, 3 * B, seed=23)  # 21 frames: 1 modulo 4
    x[2] = 0.0             # an all-zero stream
    x[5, :B] = 3.25        # a constant frame inside a stream
    x[6, B : 2 * B] = 0.0  # an all-zero frame inside a stream
    q = (2.0**-16 * (1 + np.arange(7) % 4)).astype(np.float32)
    io, offo, go = oracle.float32_to_int32(x, q)
    blob_o, st_o, nb_o = oracle.encode_i32(io, level)
    types = [fi["type"] for s in range(7) for fi in oracle.stream_info(io[s], level)]
    assert types.count(0) >= 5 and 3 in types
    comp, st, nb, off, gain = fa.encode_flac_device_f32(torch.from_numpy(x).cuda(), torch.from_numpy(q), level=level)
    assert np.array_equal(off.cpu().numpy().view(np.uint32), offo.view(np.uint32))
    assert np.array_equal(gain.cpu().numpy().view(np.uint32), go.view(np.uint32))
    assert np.array_equal(nb.cpu().numpy().reshape(-1), nb_o) and np.array_equal(st.cpu().numpy().reshape(-1), st_o)
    assert np.array_equal(comp.cpu().numpy(), blob_o)
