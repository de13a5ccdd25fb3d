"""The device decoders on libFLAC-shaped streams from tests/golden/flac_writer.py (checked against the oracle and
tests/golden/pyflac.py in tests/test_foreign_streams.py): LPC orders 1-32 (every history depth of K7 in one call),
precisions 2-15, shifts 0-15, partition orders up to 8, escapes of width 0-31, Rice parameter 0 and unary codes past
32 bits, wasted bits, sample-rate codes 12-14, sample-size code 0, 3- and 4-byte frame numbers, block sizes from 16 to
65535 with short last frames, seek tables that are complete, sparse, padded with placeholders or absent, PADDING and
APPLICATION blocks, and two-channel streams of all four channel assignments."""
import numpy as np
import pytest

from tests.golden import flac_writer as W

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def fa():
    import flacarray_amd

    return flacarray_amd


@pytest.fixture(scope="module")
def batches():
    return W.all_batches()


@pytest.fixture(autouse=True, params=["auto", "k7", "serial_walk"])
def decoder_dispatch(request, monkeypatch):
    """auto: K7L takes the calls of up to 4096 frames, K7 the rest; k7: K7L switched off; serial_walk: the library's
    dispatch with the parallel sync-code scan switched off, so streams without a complete SEEKTABLE are located by the
    serial frame walk (the variables are read per call)."""
    monkeypatch.delenv("FLACARRAY_HIP_LATENCY", raising=False)
    monkeypatch.delenv("FLACARRAY_HIP_NO_SYNC_SCAN", raising=False)
    if request.param == "k7":
        monkeypatch.setenv("FLACARRAY_HIP_LATENCY", "0")
    elif request.param == "serial_walk":
        monkeypatch.setenv("FLACARRAY_HIP_NO_SYNC_SCAN", "1")
    return request.param


def _dev(b):
    import torch

    blob, st, nb = W.pack(b["streams"])
    return blob, st, nb, tuple(torch.from_numpy(a).cuda() for a in (blob, st, nb))


def _each(batches, check):
    """Run check(batch) on every batch; report every batch that fails, not just the first."""
    failed = []
    for b in batches:
        try:
            check(b)
        except (AssertionError, RuntimeError) as e:
            failed.append((b["name"], type(e).__name__, str(e).splitlines()[0][:160] if str(e) else ""))
    assert not failed, "%d of %d batches fail: %s" % (len(failed), len(batches), failed)


def _single_block(batches):
    return [b for b in batches if b["block"] is not None]


def _ranges(n, block):
    nf = (n + block - 1) // block
    last0 = (nf - 1) * block
    out = {(0, 1), (n - 1, n), (0, n), (max(last0 - 1, 0), n), (last0, n), (min(last0 + 1, n - 1), n), (n // 3, 2 * n // 3 + 1)}
    if n > block + 1:
        out |= {(block - 1, block + 1), (block, min(2 * block, n)), (1, block), (block - 1, block), (block + 1, n - 1)}
    return sorted((f, l) for f, l in out if 0 <= f < l <= n)


def _restore_args(b):
    k = len(b["streams"])
    if b["channels"] == 1:
        return np.linspace(-3.5, 2.25, k).astype(np.float32), np.linspace(1e-3, 7.0, k).astype(np.float32)
    return np.linspace(-1e6, 3.0, k), np.linspace(2.0**-20, 2.0**12, k)


def _restored(oracle, b, x):
    off, gain = _restore_args(b)
    if b["channels"] == 1:
        return oracle.int32_to_float32(x, off, gain).view(np.uint32)
    return oracle.int64_to_float64(x, off, gain).view(np.uint64)


def _bits(t):
    a = t.cpu().numpy() if hasattr(t, "cpu") else np.asarray(t)
    return a.view(np.uint32 if a.dtype == np.float32 else np.uint64)


def test_whole_decode(fa, batches):
    def check(b):
        _, _, _, d = _dev(b)
        i64 = b["channels"] == 2
        for verify in (False, True):
            got = fa.decode_flac_device(*d, b["n"], is_int64=i64, verify=verify).cpu().numpy()
            assert np.array_equal(got, b["samples"]), (b["name"], verify)

    _each(batches, check)


def test_sample_ranges(fa, batches):
    def check(b):
        _, _, _, d = _dev(b)
        i64 = b["channels"] == 2
        for f, l in _ranges(b["n"], b["block"]):
            got = fa.decode_flac_device(*d, b["n"], f, l, is_int64=i64).cpu().numpy()
            assert np.array_equal(got, b["samples"][:, f:l]), (b["name"], f, l)

    _each(_single_block(batches), check)


def test_slices_and_decode_index(fa, batches):
    def one(b):
        _, _, _, d = _dev(b)
        n, i64, x = b["n"], b["channels"] == 2, b["samples"]
        rng = np.random.default_rng(n)
        rs = _ranges(n, b["block"])
        ss = np.concatenate([np.arange(len(rs)) % x.shape[0], rng.integers(0, x.shape[0], 20)])
        first = np.concatenate([[f for f, _ in rs], rng.integers(0, n, 20)])
        cnt = np.concatenate([[l - f for f, l in rs], np.zeros(20, np.int64)])
        cnt[len(rs) :] = [int(rng.integers(1, n - f0 + 1)) for f0 in first[len(rs) :]]

        def check(flat, offs, what):
            flat = flat.cpu().numpy() if hasattr(flat, "cpu") else flat
            for o, s_i, f0, c in zip(offs, ss, first, cnt):
                assert np.array_equal(flat[o : o + c], x[s_i, f0 : f0 + c]), (b["name"], what, s_i, f0, c)

        check(*fa.decode_slices_device(*d, n, ss, first, cnt, is_int64=i64), "decode_slices_device")
        idx = fa.DeviceDecodeIndex(*d, n, is_int64=i64)
        try:
            assert np.array_equal(idx.decode().cpu().numpy(), x), b["name"]
            for f, l in rs:
                assert np.array_equal(idx.decode(f, l).cpu().numpy(), x[:, f:l]), (b["name"], f, l)
            check(*idx.decode_slices(ss, first, cnt), "index")
            check(*idx.decode_slices(ss, first, cnt, to_host=True), "index to_host")
            check(*idx.decode_slices(ss, first, cnt, verify=True), "index verify")
        finally:
            idx.close()

    _each(_single_block(batches), one)


def test_host_abi(fa, batches):
    def check(b):
        blob, st, nb, _ = _dev(b)
        i64 = b["channels"] == 2
        assert np.array_equal(fa.decode_flac(blob, st, nb, b["n"], is_int64=i64), b["samples"]), b["name"]
        if b["block"] is not None:
            f, l = b["block"] - 1, b["n"]
            assert np.array_equal(fa.decode_flac(blob, st, nb, b["n"], f, l, is_int64=i64), b["samples"][:, f:l]), b["name"]

    _each(batches, check)


def test_fused_restore(fa, oracle, batches):
    """The int -> float restore fused into the decoders' stores (also the float instantiations of the deep-history
    passes) is bit-equal to the oracle's restore of the known integers."""
    import torch

    def check(b):
        _, _, _, d = _dev(b)
        n, i64, x = b["n"], b["channels"] == 2, b["samples"]
        off, gain = _restore_args(b)
        want = _restored(oracle, b, x)
        to = lambda a: torch.from_numpy(np.ascontiguousarray(a))  # noqa: E731
        got = fa.decode_flac_device(*d, n, offsets=to(off), gains=to(gain), is_int64=i64)
        assert np.array_equal(_bits(got), want), b["name"]
        if b["block"] is None:
            return
        f, l = max(n - b["block"] - 3, 0), n
        got = fa.decode_flac_device(*d, n, f, l, offsets=to(off), gains=to(gain), is_int64=i64)
        assert np.array_equal(_bits(got), want[:, f:l]), (b["name"], f, l)
        ss, first, cnt = np.arange(x.shape[0]), np.zeros(x.shape[0], np.int64), np.full(x.shape[0], n)
        flat, offs = fa.decode_slices_device(*d, n, ss, first, cnt, offsets=to(off), gains=to(gain), is_int64=i64)
        assert np.array_equal(_bits(flat), want.reshape(-1)), b["name"]
        idx = fa.DeviceDecodeIndex(*d, n, is_int64=i64)
        try:
            assert np.array_equal(_bits(idx.decode(offsets=to(off), gains=to(gain))), want), b["name"]
        finally:
            idx.close()

    _each(batches, check)


def test_batch_shapes_reach_every_pass(batches):
    """What the calls above hand the decoders: deep and shallow frames in the same streams, more than 4096 frames in a
    call (K7 under the auto dispatch), four block sizes in one call."""
    names = {b["name"]: b for b in batches}
    for key in ("deep_mix_1", "deep_mix_2"):
        for r in names[key]["records"]:
            f = r["features"]
            assert f["lpc_order_1-8"] and f["lpc_order_13-16"] and f["lpc_order_17-32"], key
    assert sum(r["frames"] for r in names["many_frames_1"]["records"]) > 4096
    assert sum(r["frames"] for r in names["many_frames_2"]["records"]) > 4096
    assert len({r["block"] for r in names["mixed_blocks"]["records"]}) == 4


def test_invalid_fields_are_reported(fa, oracle):
    """One field the format does not allow, CRCs intact: where the oracle rejects the stream every device entry point
    raises and returns no samples; where it accepts, the samples agree.  The variable-blocksize stream is refused by
    the device path whatever the oracle does."""
    import torch

    for name, data, n in W.invalid_streams():
        blob = np.frombuffer(data, dtype=np.uint8).copy()
        st, nb = np.array([0], np.int64), np.array([blob.size], np.int64)
        d = tuple(torch.from_numpy(a).cuda() for a in (blob, st, nb))
        try:
            ref = oracle.decode_i32(blob, st, nb, n)
        except RuntimeError:
            ref = None
        if name == "variable_blocksize":
            ref = None
        calls = {
            "device": lambda: fa.decode_flac_device(*d, n).cpu().numpy(),
            "device verify": lambda: fa.decode_flac_device(*d, n, verify=True).cpu().numpy(),
            "device range": lambda: fa.decode_flac_device(*d, n, 1, n).cpu().numpy(),
            "slices": lambda: fa.decode_slices_device(*d, n, [0], [0], [n])[0].cpu().numpy().reshape(1, -1),
            "host": lambda: fa.decode_flac(blob, st, nb, n),
        }
        for what, call in calls.items():
            if ref is None:
                with pytest.raises(RuntimeError, match="Decoding failed"):
                    call()
            else:
                got = call()
                want = ref[:, 1:] if what == "device range" else ref
                assert np.array_equal(got, want), (name, what)
        if ref is None:
            with pytest.raises(RuntimeError, match="Decoding failed"):
                idx = None
                try:
                    idx = fa.DeviceDecodeIndex(*d, n)
                    idx.decode()
                finally:
                    if idx is not None:
                        idx.close()
        assert (ref is not None) == (name == "valid"), name
