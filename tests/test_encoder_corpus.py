"""CPU audit of the encoder decision corpus (tests/encoder_corpus.py) on the oracle's decision trace: every decision of
DECISIONS is reached by a case that lists it, every case is needed, every stream decodes back (oracle decoder, and one
short stream per case through the independent pure-Python decoder), and the K3F cases have K3F's geometry."""
import re

import numpy as np
import pytest

from oracle import oracle as O
from tests import encoder_corpus as C
from tests.golden import pyflac

_searched = lambda r: not r["is_const"] and r["blocksize"] > 4  # noqa: E731  (the FIXED / LPC search ran)
_hi = lambda r: r["level"] >= 3  # noqa: E731
_lo = lambda r: r["level"] <= 2  # noqa: E731


def _decisions():
    D = {}
    for w in range(1, 32):  # wasted bits on non-constant frames, at a level with LPC and at one without
        D[f"wasted{w}@hi"] = lambda r, w=w: _hi(r) and r["wasted"] == w and not r["is_const"] and r["nch"] == 1
        D[f"wasted{w}@lo"] = lambda r, w=w: _lo(r) and r["wasted"] == w and not r["is_const"] and r["nch"] == 1
    D["wasted31_verbatim_1bps"] = lambda r: r["wasted"] == 31 and r["bps"] == 1 and r["type"] == 1 and not r["is_const"]
    D["wasted_2bps"] = lambda r: r["wasted"] == 30 and r["bps"] == 2
    for w in (15, 16, 17):  # the bps <= 17 precision limit with an LPC winner
        for lvl in (3, 5, 8):
            D[f"lpc_limit_w{w}@L{lvl}"] = lambda r, w=w, lvl=lvl: r["level"] == lvl and r["type"] == 3 and r["wasted"] == w and r["bps"] == 32 - w
    for p in (12, 13, 14):
        D[f"lpc_precision{p}"] = lambda r, p=p: r["type"] == 3 and r["bps"] <= 17 and r["prec_before"] == 15 and r["precision"] == p
    D["lpc_precision15"] = lambda r: r["type"] == 3 and r["bps"] <= 17 and r["precision"] == 15  # (the limit entered and not binding)
    for lvl, mx in C.LPC_MAX.items():
        for p in range(1, mx + 1):
            D[f"lpc_order{p}@L{lvl}"] = lambda r, p=p, lvl=lvl: r["level"] == lvl and r["type"] == 3 and r["order"] == p
    for s in range(7, 16):
        D[f"lpc_shift{s}"] = lambda r, s=s: r["type"] == 3 and r["shift"] == s
    D["coef_clamped_qmax"] = lambda r: r["type"] == 3 and r["clamp_qmax"] == 1
    for k in range(5):
        D[f"fixed{k}_wins@hi"] = lambda r, k=k: _hi(r) and r["type"] == 2 and r["order"] == k and r["lpc_tried"] == 1
        D[f"fixed{k}_wins@lo"] = lambda r, k=k: _lo(r) and r["type"] == 2 and r["order"] == k
        D[f"fixed{k}_invalid"] = lambda r, k=k: _searched(r) and not (r["fixed_valid"] >> k) & 1 and r["fixed_order"] >= 0
    D["fixed_none_valid"] = lambda r: _hi(r) and _searched(r) and r["fixed_valid"] == 0 and r["fixed_order"] == -1
    D["fixed_none_valid@lo"] = lambda r: _lo(r) and _searched(r) and r["fixed_valid"] == 0 and r["fixed_order"] == -1
    for lvl, mx in C.PORDER_MAX.items():
        for p in range(mx + 1):
            D[f"porder{p}@L{lvl}"] = lambda r, p=p, lvl=lvl: r["level"] == lvl and r["type"] >= 2 and r["porder"] == p
    D["rice0"] = lambda r: r["type"] >= 2 and r["rice_min"] == 0
    D["rice2_5bit"] = lambda r: r["type"] >= 2 and r["rice2"] == 1 and r["rice_max"] >= 15
    D["rice_clamp30"] = lambda r: r["rice_clamp30"] == 1
    D["verbatim_no_candidate"] = lambda r: r["type"] == 1 and r["verbatim_cause"] == O.VERB_NO_CANDIDATE
    D["verbatim_exact"] = lambda r: r["type"] == 1 and r["verbatim_cause"] == O.VERB_EXACT and r["exact_bits"] > r["verbatim_bits"] > r["est_bits"]
    D["verbatim_row_cap"] = lambda r: r["type"] == 1 and r["verbatim_cause"] == O.VERB_ROW_CAP and r["exact_over"] == 0
    D["verbatim_short_tail"] = lambda r: r["type"] == 1 and r["verbatim_cause"] == O.VERB_SHORT and r["frame"] > 0
    for n in (2, 3, 4):
        D[f"verbatim_short_len{n}"] = lambda r, n=n: r["type"] == 1 and r["verbatim_cause"] == O.VERB_SHORT and r["blocksize"] == n
    D["len1_constant"] = lambda r: r["blocksize"] == 1 and r["type"] == 0
    D["tail5_searched"] = lambda r: r["blocksize"] == 5 and _searched(r) and r["lpc_tried"] == 1
    D["tail_odd_lpc12"] = lambda r: r["blocksize"] % 2 == 1 and r["type"] == 3 and r["order"] >= 9 and r["porder"] == 0
    D["lpc_lags_zero"] = lambda r: r["lpc_drop"] == O.LPC_LAGS_ZERO
    D["lpc_cmax_zero"] = lambda r: r["lpc_drop"] == O.LPC_CMAX and r["quant_rc"] == 2
    D["lpc_residual_overflow"] = lambda r: r["lpc_drop"] == O.LPC_RESIDUAL
    D["lpc_estimate_not_smaller"] = lambda r: r["lpc_drop"] == O.LPC_ESTIMATE and r["type"] == 2
    D["levinson_negative"] = lambda r: r["lev_neg"] == 1
    for code in (1, 2, 3, 4, 6, 7, 8, 9, 10, 11):  # block size bits of a short last frame (12 = every full frame of levels 3-8)
        D[f"bscode{code}"] = lambda r, code=code: _hi(r) and r["blocksize"] != 4096 and C.blocksize_code(r["blocksize"]) == code
    D["bscode1@lo"] = lambda r: _lo(r) and r["blocksize"] == 192
    D["bscode7@lo"] = lambda r: _lo(r) and r["blocksize"] != 1152 and C.blocksize_code(r["blocksize"]) == 7
    D["frame_no_128"] = lambda r: r["frame"] == 128    # (the first two-byte UTF-8 frame number)
    D["frame_no_2048"] = lambda r: r["frame"] == 2048  # (the first three-byte one)
    for sfx, lv in (("@hi", _hi), ("@lo", _lo)):
        two = lambda r, lv=lv: lv(r) and r["nch"] == 2  # noqa: E731
        D["side_chosen" + sfx] = lambda r, two=two: two(r) and r["st_use_side"] == 1 and r["channel"] == 0 and r["bps"] + r["wasted"] == 33
        D["side_refused_fits" + sfx] = lambda r, two=two: two(r) and r["st_fits"] == 0 and r["st_fit_sign"] == 1 and r["st_small"] == 1
        D["side_refused_fits_negative" + sfx] = lambda r, two=two: two(r) and r["st_fits"] == 0 and r["st_fit_sign"] == -1 and r["st_small"] == 1
        D["side_refused_small" + sfx] = lambda r, two=two: two(r) and r["st_fits"] == 1 and r["st_small"] == 0
        D["side_refused_right_zero" + sfx] = lambda r, two=two: two(r) and r["st_fits"] == 1 and r["st_small"] == 1 and r["st_right_zero"] == 1
        D["side_refused_estimate" + sfx] = lambda r, two=two: two(r) and r["st_tried"] == 1 and r["st_use_side"] == 0 and r["st_est_side"] >= r["st_est_left"]
        D["side_wasted" + sfx] = lambda r, two=two: two(r) and r["st_use_side"] == 1 and r["channel"] == 0 and r["wasted"] > 0 and not r["is_const"]
        D["high_wasted" + sfx] = lambda r, two=two: two(r) and r["channel"] == 1 and r["wasted"] > 0 and not r["is_const"]
    D["i64_high_lpc_bps16"] = lambda r: r["nch"] == 2 and r["channel"] == 1 and r["type"] == 3 and r["bps"] == 16 and r["precision"] < 15
    D["i64_low_lpc_bps17"] = lambda r: r["nch"] == 2 and r["channel"] == 0 and r["type"] == 3 and r["bps"] == 17 and r["precision"] < 15
    return D


DECISIONS = _decisions()


@pytest.fixture(scope="module")
def traces(oracle):
    return {c.name: C.trace_case(oracle, c) for c in C.CASES}


def _reached(traces):
    """decision -> names of the cases that list it and reach it"""
    out = {d: [] for d in DECISIONS}
    for c in C.CASES:
        for d in c.decisions:
            if any(DECISIONS[d](r) for r in traces[c.name]):
                out[d].append(c.name)
    return out


def test_every_listed_decision_is_in_the_table():
    for c in C.CASES:
        assert c.decisions, c.name
        for d in c.decisions:
            assert d in DECISIONS, (c.name, d)


def test_every_decision_is_reached(traces):
    """Each decision is reached by at least one case built for it (a case that lists it), and every case reaches all it
    lists: the audit fails, naming the decision, when a case is dropped or its input drifts."""
    reached = _reached(traces)
    lost = sorted(d for d, names in reached.items() if not names)
    assert not lost, f"decisions no corpus case reaches: {lost}"
    for c in C.CASES:
        missed = [d for d in c.decisions if c.name not in reached[d]]
        assert not missed, f"{c.name} no longer reaches {missed}"
    for d in sorted(reached):
        print(f"{d}: {', '.join(reached[d])}")


def test_every_case_is_needed():
    """Each case is the only one to list at least one decision: removing any single case loses a decision."""
    listed = {}
    for c in C.CASES:
        for d in c.decisions:
            listed.setdefault(d, []).append(c.name)
    for c in C.CASES:
        assert any(listed[d] == [c.name] for d in c.decisions), c.name


def test_rare_classes_sit_on_two_positions_of_a_workgroup(traces):
    """K3F: one wave solves the LPC problems of four consecutive frames; every decision a K3F case lists is reached on at
    least two different frame positions modulo 4 (frames counted over the whole array, stream after stream)."""
    for c in C.CASES:
        if not c.k3f:
            continue
        nf = c.x.shape[1] // C.B
        for d in c.decisions:
            pos = {(r["stream"] * nf + r["frame"]) % 4 for r in traces[c.name] if DECISIONS[d](r)}
            single = d.startswith(("wasted", "lpc_order", "porder", "lpc_limit", "lpc_precision", "fixed")) and not d.startswith("wasted31_")
            assert len(pos) >= (1 if single else 2), (c.name, d, pos)
        # the classes whose members are single frames (one per wasted count, order, ...) cover the positions as classes
        for prefix in {re.sub(r"\d.*$", "", d) for d in c.decisions}:
            pos = {(r["stream"] * nf + r["frame"]) % 4 for r in traces[c.name] for d in c.decisions if d.startswith(prefix) and DECISIONS[d](r)}
            assert len(pos) >= 2, (c.name, prefix, pos)


def test_trace_agrees_with_stream_info(oracle):
    """The trace's first eight fields are oracle_frame_info's, subframe by subframe."""
    for c in C.CASES:
        if c.x.size > 1 << 20:
            continue
        for s in range(c.x.shape[0]):
            info = (oracle.stream_info_i64 if c.is_int64 else oracle.stream_info)(c.x[s], c.level)
            tr = (oracle.stream_trace_i64 if c.is_int64 else oracle.stream_trace)(c.x[s], c.level)
            assert len(info) == len(tr)
            for a, b in zip(info, tr):
                assert all(a[k] == b[k] for k in a), (c.name, s, a, b)


@pytest.mark.parametrize("case", C.CASES, ids=lambda c: c.name)
def test_streams_decode_back_through_the_oracle(oracle, case):
    enc, dec = (oracle.encode_i64, oracle.decode_i64) if case.is_int64 else (oracle.encode_i32, oracle.decode_i32)
    blob, st, nb = enc(case.x, case.level)
    assert np.array_equal(dec(blob, st, nb, case.x.shape[1]), case.x)


@pytest.mark.parametrize("case", C.CASES, ids=lambda c: c.name)
def test_probe_stream_decodes_through_the_independent_decoder(oracle, case):
    """One short stream per case (its first rare frame) through tests/golden/pyflac.py, which shares no code with the
    oracle: a stream the oracle writes and that decoder cannot read back would mean the oracle is wrong."""
    x = case.probe().reshape(1, -1)
    assert x.shape[1] <= case.block and x.dtype == case.x.dtype
    blob, st, nb = (oracle.encode_i64 if case.is_int64 else oracle.encode_i32)(x, case.level)
    samples, info = pyflac.decode_stream(blob.tobytes())
    if case.is_int64:
        assert info["channels"] == 2
        ch = np.array(samples, dtype=np.int64).reshape(-1, 2)
        got = (ch[:, 1] << 32) | (ch[:, 0] & 0xFFFFFFFF)
    else:
        assert info["channels"] == 1
        got = np.array(samples, dtype=np.int64)
    assert info["total"] == x.shape[1] and np.array_equal(got, x[0].astype(np.int64))


def test_k3f_cases_have_the_single_pass_geometry():
    """On shapes alone (csrc/flacarray_hip.hip fused_geometry: levels 3 to 8, int32, whole 4096-sample frames), and the
    other cases do not: levels 0 to 2, a short last frame, or int64."""
    assert sum(c.k3f for c in C.CASES) >= 15
    for c in C.CASES:
        n_stream, n = c.x.shape
        whole = c.x.dtype == np.int32 and 3 <= c.level <= 8 and n % C.B == 0 and n_stream >= 1
        assert whole == c.k3f, c.name
        if c.k3f:
            assert (n_stream * (n // C.B)) % 4 == 0 and c.x.ctypes.data % 16 == 0
        if c.append_cut is not None:
            assert 0 < c.append_cut < n
