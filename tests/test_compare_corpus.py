"""Preconditions of tests/test_gpu_compare_foreign.py, checked with the oracle and the quantise model only: the
replicated streams decode to their samples and hold the frames the GPU tests are about (every LPC order bucket, wasted
bits, several channel assignments), and the float mutations change exactly the integers the expected results assume."""
import numpy as np
import pytest

from tests import compare_corpus as C
from tests import quant_model as M
from tests.golden import flac_writer as W


@pytest.fixture(scope="module")
def reps():
    return {name: C.replicated(**g) for name, g in C.GEOMETRIES.items()}


@pytest.fixture(scope="module")
def small():
    out = {name: C.small_amplitude(n) for name, n in C.SMALL_LENGTHS.items()}
    out.update({name: C.uniform(name) for name in C.UNIFORM})
    return out


def _decoded(oracle, rep):
    blob, st, nb = C.store(rep, rows=2)
    return (oracle.decode_i32 if rep.channels == 1 else oracle.decode_i64)(blob, st, nb, rep.n)


def test_replicated_streams_decode_to_their_samples(oracle, reps, small):
    for name, rep in list(reps.items()) + list(small.items()) + [("own", C.replicated(layout="own", **C.GEOMETRIES["mono192_unaligned"]))]:
        assert rep.samples.shape == (rep.n,) and rep.samples.dtype == (np.int32 if rep.channels == 1 else np.int64), name
        assert np.array_equal(_decoded(oracle, rep), C.rows(rep, 2)), name


def test_row_alignment_of_the_geometries(reps):
    assert (reps["mono192_aligned"].n * 4) % 16 == 0
    assert (reps["mono192_unaligned"].n * 4) % 16 != 0
    for rep in reps.values():
        assert rep.n % rep.block  # a short last frame


def test_block_192_streams_hold_every_order_bucket_and_wasted_bits(reps, small):
    for name, rep in [(k, v) for k, v in reps.items() if v.block == 192] + [(k, small[k]) for k in C.SMALL_LENGTHS]:
        f = rep.record["features"]
        assert rep.record["frames"] == 9, name
        for bucket in ("1-8", "9-12", "13-16", "17-32"):
            assert f["lpc_order_" + bucket] >= 1, (name, bucket)
        assert f["lpc"] == 9 * rep.channels, name  # (no frame fell back to VERBATIM)
        assert f["wasted"] >= 1, name
        assert f["short_last_frame"] == 1, name
    assert reps["mono16"].record["features"]["lpc_order_17-32"] == 0
    asg = [k for k, v in reps["stereo192"].record["features"].items() if k.startswith("assignment_") and v]
    assert len(asg) >= 2, asg


def test_one_bucket_streams(small):
    """Whole frames only, aligned rows, every frame in the named bucket, one of them with wasted bits."""
    for name, (bucket, _) in C.UNIFORM.items():
        rep, f = small[name], small[name].record["features"]
        assert rep.n % rep.block == 0 and (rep.n * 4) % 16 == 0 and rep.record["frames"] == 4, name
        assert f["lpc_order_%d-%d" % W.ORDER_BUCKETS[bucket]] == f["lpc"] == 4, name
        assert f["wasted"] == 1, name
        assert (rep.n * rep.record["frames"]) % 64 == 0, name  # (n rows of four frames: whole waves of 64 frames)


def test_small_amplitude_record(small):
    for name, rep in [(k, small[k]) for k in C.SMALL_LENGTHS]:
        f = rep.record["features"]
        assert (f["lpc_order_1-8"], f["lpc_order_9-12"], f["lpc_order_13-16"], f["lpc_order_17-32"], f["wasted"]) == (3, 2, 2, 2, 1), name
        assert np.all(rep.samples[4 * 192 : 5 * 192] % 8 == 0)


def test_positions():
    assert C.positions(8 * 192 + 37, 192) == [0, 1, 3, 4, 15, 16, 17, 31, 32, 33, 191, 192, 193, 1535, 1536, 1537, 1571, 1572]
    assert C.positions(16 * 40 + 5, 16) == [0, 1, 3, 4, 15, 16, 17, 31, 32, 33, 639, 640, 641, 643, 644]
    assert C.positions(7, 65535) == [0, 1, 3, 4, 5, 6]


def test_expected_first_and_mutations(reps):
    rep = reps["mono16"]
    data = C.rows(rep)
    n = rep.n
    assert (C.expected_first(data, data) == -1).all()
    assert np.array_equal(C.expected_first(C.xor_diagonal(data, np.int32(1)), data), np.arange(n))
    assert np.array_equal(C.expected_first(C.add_from_diagonal(data, 7), data), np.arange(n))
    e = C.expected_first(C.add_from_diagonal(data, 7, skip=1), data)
    assert np.array_equal(e[:-1], np.arange(1, n)) and e[-1] == -1
    k = len(C.positions(n, rep.block))
    seen = set()
    for j in range(k):
        e = C.expected_first(C.edge_mutation(data[:5], n, rep.block, j, np.int32(1)), data[:5])
        seen |= {(i, int(p)) for i, p in enumerate(e)}
    assert seen == {(i, p) for i in range(5) for p in C.positions(n, rep.block)}  # every stream meets every position


def test_float_case_round_trips_and_mutations_move_one_integer(small):
    for name, rep in small.items():
        x, ints, off, gain = C.float_case(rep)
        n = rep.n
        assert x.dtype == np.float32 and np.all(gain == 64.0) and np.array_equal(off, (np.arange(n) % 7) * np.float32(0.25))
        assert np.array_equal(M.quantise_with(x, off, gain), ints), name
        # one and a half quanta on the diagonal: exactly one integer per row changes, at r
        changed = M.quantise_with(C.bump_diagonal(x, 1.5 * C.QUANTA), off, gain) != ints
        assert np.array_equal(changed, np.eye(n, dtype=bool)), name
        # the next float up: the integer stays in (at least) nine rows of ten
        moved = (M.quantise_with(C.nextafter_diagonal(x), off, gain) != ints).any(axis=1)
        assert moved.sum() <= n // 10, "%s: %d of %d nextafter rows change their integer" % (name, moved.sum(), n)
