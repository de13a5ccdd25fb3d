"""The libFLAC-shaped stream writer (tests/golden/flac_writer.py) against two independent readers: every generated
stream must decode exactly with the oracle's C decoder and with the pure-Python reader tests/golden/pyflac.py, and
the sweep must reach every feature the device decoders are tested on (tests/test_gpu_foreign_streams.py)."""
import numpy as np
import pytest

from tests.golden import flac_writer as W
from tests.golden import pyflac


@pytest.fixture(scope="module")
def batches():
    return W.all_batches()


def _ranges(n, block):
    """Sample ranges on either side of frame boundaries, in the short last frame, first and last sample."""
    nf = (n + block - 1) // block
    last0 = (nf - 1) * block
    out = {(0, 1), (n - 1, n), (0, n), (max(last0 - 1, 0), n), (last0, n), (min(last0 + 1, n - 1), n)}
    if n > block + 1:
        out |= {(block - 1, block + 1), (block, min(2 * block, n)), (1, block), (block - 1, block)}
    return sorted((f, l) for f, l in out if 0 <= f < l <= n)


def _pairs(samples, channels):
    if channels == 1:
        return [int(v) for v in samples]
    left = (samples.astype(np.int64) << 32) >> 32
    right = samples.astype(np.int64) >> 32
    return np.stack([left, right], axis=1).reshape(-1).tolist()


def test_oracle_decodes_every_stream(oracle, batches):
    for b in batches:
        blob, st, nb = W.pack(b["streams"])
        dec = oracle.decode_i32 if b["channels"] == 1 else oracle.decode_i64
        if b["block"] is not None:
            assert np.array_equal(dec(blob, st, nb, b["n"]), b["samples"]), b["name"]
        for i in range(len(st)):
            one = (blob, st[i : i + 1], nb[i : i + 1])
            assert np.array_equal(dec(*one, b["n"])[0], b["samples"][i]), (b["name"], i)
            for f, l in _ranges(b["n"], b["records"][i]["block"]):
                assert np.array_equal(dec(*one, b["n"], f, l)[0], b["samples"][i, f:l]), (b["name"], i, f, l)


def test_pyflac_decodes_every_stream(batches):
    for b in batches:
        for i, data in enumerate(b["streams"]):
            got, info = pyflac.decode_stream(data)
            assert got == _pairs(b["samples"][i], b["channels"]), (b["name"], i)
            assert info["total"] == b["n"] and info["channels"] == b["channels"] and info["bps"] == 32


def test_sweep_covers_every_feature(batches):
    cov = W.coverage(batches)
    need = {
        "const": 20, "verbatim": 20, "lpc": 100, "wasted": 20, "redrawn": 1, "rice": 20, "rice2": 20, "long_code": 20,
        "rice_param_0": 20, "rice_param_1-14": 20, "rice_param_gt14": 20, "short_last_frame": 20,
        "side_33bit": 10, "side_lpc_order_gt12": 10, "lpc_terms_ge_2^48": 5,
        "utf8_bytes_1": 5, "utf8_bytes_2": 3, "utf8_bytes_3": 3, "utf8_bytes_4": 1,
    }
    need.update({"fixed_%d" % k: 10 for k in range(5)})
    need.update({"lpc_order_" + W.order_bucket(lo): 10 for lo, _ in W.ORDER_BUCKETS})
    need.update({"lpc_prec_%d" % p: 5 for p in range(2, 16)})
    need.update({"lpc_shift_%d" % s: 5 for s in range(16)})
    need.update({"porder_%d" % p: 3 for p in range(9)})
    need.update({"esc_width_%d" % w: 3 for w in range(32)})
    need.update({"assignment_%d" % a: 10 for a in (1, 8, 9, 10)})
    need.update({"layout_" + lay: 5 for lay in W.LAYOUTS})
    need.update({"sr_code_%d" % c: 3 for c in (9, 12, 13, 14)})
    need.update({"ss_code_%d" % c: 5 for c in (0, 7)})
    need.update({"block_%d" % b: 3 for b in W.BLOCK_SIZES})
    short = {k: (cov[k], v) for k, v in need.items() if cov[k] < v}
    assert not short, short
    # the deep-order batches hold frames of every history depth in each stream
    for b in batches:
        if b["name"].startswith("deep_mix"):
            for r in b["records"]:
                assert all(r["features"]["lpc_order_" + W.order_bucket(lo)] >= 1 for lo, _ in W.ORDER_BUCKETS), r
    # more than 4096 frames in one call, and a seek table with placeholders as long as the frame count
    assert max(sum(r["frames"] for r in b["records"]) for b in batches) > 4096
    assert any(r["layout"] == "placeholder" for b in batches for r in b["records"])


def test_writer_is_deterministic():
    a, b = (W.write_stream(np.random.default_rng(7), 5000, 576, 2, layout="placeholder") for _ in range(2))
    assert a[1] == b[1] and np.array_equal(a[0], b[0])


def test_invalid_fields_are_rejected_by_the_readers(oracle):
    for name, data, n in W.invalid_streams():
        blob = np.frombuffer(data, dtype=np.uint8).copy()
        st, nb = np.array([0], np.int64), np.array([blob.size], np.int64)
        if name == "valid":
            ref = oracle.decode_i32(blob, st, nb, n)
            assert np.array_equal(np.array(pyflac.decode_stream(data)[0], dtype=np.int32), ref[0])
            continue
        with pytest.raises(RuntimeError, match="Decoding failed"):
            oracle.decode_i32(blob, st, nb, n)
        with pytest.raises((AssertionError, IndexError)):  # (a garbled parse can also run off the end)
            pyflac.decode_stream(data)
