"""The numpy model of tests/quant_model.py against the CPU oracle, bit for bit, on the whole edge corpus; and the
model's round trip against the quantisation error bound, independently of both."""
import numpy as np
import pytest

from tests import quant_model as M

DTYPES = [np.float32, np.float64]


def _oracle_pair(oracle, dtype):
    if dtype == np.float32:
        return oracle.float32_to_int32, oracle.int32_to_float32
    return oracle.float64_to_int64, oracle.int64_to_float64


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "f64"])
def test_model_matches_oracle_quantise(oracle, dtype):
    quant, rest = _oracle_pair(oracle, dtype)
    for c in M.quantise_cases(dtype):
        ints, off, gain = M.quantise(c.x, c.quanta)
        io, oo, go = quant(c.x, c.quanta)
        assert M.bits_equal(ints, io), c.name
        assert M.bits_equal(off, oo), c.name
        assert M.bits_equal(gain, go), c.name
        assert M.bits_equal(M.restore(ints, off, gain), rest(io, oo, go)), c.name


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "f64"])
def test_model_matches_oracle_restore(oracle, dtype):
    _, rest = _oracle_pair(oracle, dtype)
    for c in M.restore_cases(dtype):
        assert M.bits_equal(M.restore(c.ints, c.offsets, c.gains), rest(c.ints, c.offsets, c.gains)), c.name


def test_cvtt_is_x86_truncation():
    v = np.array([2.0**31, 2.0**31 - 1, -(2.0**31) - 0.75, -(2.0**31) - 1, -2.5, 2.5, np.nan, np.inf, -np.inf])
    assert M.cvtt(v, 32).tolist() == [-(2**31), 2**31 - 1, -(2**31), -(2**31), -2, 2, -(2**31), -(2**31), -(2**31)]
    w = np.array([2.0**63, 2.0**63 - 1024, -(2.0**63), -(2.0**63) - 2048, np.nan])
    assert M.cvtt(w, 64).tolist() == [-(2**63), 2**63 - 1024, -(2**63), -(2**63), -(2**63)]


def test_range_scan_first_zero_wins():
    x = np.array([[1.0, -0.0, 0.0, 2.0], [0.0, -0.0, 3.0, 3.0], [-0.0, 0.0, -0.0, 0.0]], dtype=np.float32)
    smin, smax = M.stream_range(x)
    assert np.signbit(smin).tolist() == [True, False, True]
    assert np.signbit(smax).tolist() == [False, False, True]


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "f64"])
def test_round_trip_error_bound(dtype):
    """For finite data and a normal quanta no smaller than min_quanta, restore(quantise(x)) is within q/2 of x plus
    the rounding of the float operations, bounded in float64."""
    eps = float(np.finfo(dtype).eps)
    checked = 0
    for c in M.quantise_cases(dtype):
        if not np.all(np.isfinite(c.x)):
            continue
        _, min_q = M.range_params(c.x)
        sq = min_q if c.quanta is None else c.quanta
        ints, off, gain = M.quantise(c.x, c.quanta)
        back = M.restore(ints, off, gain).astype(np.float64)
        x = c.x.astype(np.float64)
        q = sq.astype(np.float64)[:, None]
        use = np.isfinite(q) & (q >= np.finfo(dtype).tiny) & (q >= min_q.astype(np.float64)[:, None]) & np.isfinite(gain)[:, None]
        use = np.broadcast_to(use, x.shape)
        with np.errstate(over="ignore", invalid="ignore"):
            bound = q / 2 + 8 * eps * (np.abs(x) + np.abs(off.astype(np.float64))[:, None] + q * np.abs(ints.astype(np.float64)))
            err = np.abs(back - x)
        assert np.all(err[use] <= bound[use]), c.name
        checked += int(use.sum())
    assert checked > 100000


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "f64"])
def test_corpus_reaches_every_edge(dtype):
    assert {"truncated_peak", "tie", "inf", "subnormal", "st_zero", "long", "unaligned_length"} <= M.corpus_tags(dtype)
    names = {c.name.split("/")[0] for c in M.quantise_cases(dtype)}
    assert {"n1", "n2", "n3", "long69632", "long65539"} <= names
    assert any(f % 4 and last - f < 4 for f, last in M.windows(8195))
    assert any(s % 4 for s in M.slices(3, 8195)[1])
