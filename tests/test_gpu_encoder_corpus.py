"""GPU parity on the encoder decision corpus (tests/encoder_corpus.py): every case through every encode route that takes
its geometry -- K3F forced, the library's own dispatch (K3G for arrays this small), the slot sequence, the host ABI,
verify=True and FlacArray.append -- byte for byte against the oracle, decision for decision against its stream_info,
and decoded back under both decoder dispatches.  tests/test_encoder_corpus.py audits which decisions the cases reach."""
import numpy as np
import pytest

from tests import encoder_corpus as C

pytestmark = pytest.mark.gpu

KEYS = ["type", "order", "porder", "wasted", "shift", "precision", "nbytes", "blocksize"]
ROUTE_ENV = {
    "k3f": {"FLACARRAY_HIP_PLACED_BELOW": "0"},
    "auto": {},
    "slots": {"FLACARRAY_HIP_SLOTS": "1"},
    "host": {},
    "verify": {},
    "append": {},
    "append_k3f": {"FLACARRAY_HIP_PLACED_BELOW": "0"},
}


def _routes(case):
    r = ["auto", "slots", "host", "verify"]
    if case.k3f:
        r = ["k3f"] + r
    if case.append_cut is not None:
        r.append("append")
        if case.k3f:
            r.append("append_k3f")
    return r


PARAMS = [pytest.param(c, route, id=f"{c.name}-{route}") for c in C.CASES for route in _routes(c)]


@pytest.fixture(scope="module")
def fa():
    import flacarray_amd

    return flacarray_amd


_expected = {}


def _oracle_encode(oracle, case):
    if case.name not in _expected:
        _expected.clear()  # (one case at a time: the parameters run case by case)
        _expected[case.name] = (oracle.encode_i64 if case.is_int64 else oracle.encode_i32)(case.x, case.level)
    return _expected[case.name]


def _frame_diff(oracle, case, info_gpu):
    """The first subframes whose decisions differ from the oracle's stream_info (empty: none)."""
    nch = 2 if case.is_int64 else 1
    per = info_gpu.shape[0] // case.x.shape[0]
    msgs = []
    for s in range(case.x.shape[0]):
        oi = (oracle.stream_info_i64 if case.is_int64 else oracle.stream_info)(case.x[s], case.level)
        assert len(oi) == per
        for k in range(per):
            g, o = [int(v) for v in info_gpu[s * per + k]], [oi[k][key] for key in KEYS]
            if g != o:
                msgs.append(f"stream {s} frame {k // nch} channel {k % nch}: gpu {dict(zip(KEYS, g))} oracle {dict(zip(KEYS, o))}")
                if len(msgs) >= 5:
                    return "\n".join(msgs)
    return "\n".join(msgs)


def _set_env(monkeypatch, env):
    for k in ("FLACARRAY_HIP_PLACED_BELOW", "FLACARRAY_HIP_SLOTS", "FLACARRAY_HIP_LATENCY"):
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)


def _decodes_back(fa, monkeypatch, case, comp, st, nb):
    """Under both decoder dispatches: the library's own (K7L for launches this small) and K7 (FLACARRAY_HIP_LATENCY=0)."""
    import torch

    want = torch.from_numpy(case.x)
    for latency in (None, "0"):
        if latency is None:
            monkeypatch.delenv("FLACARRAY_HIP_LATENCY", raising=False)
        else:
            monkeypatch.setenv("FLACARRAY_HIP_LATENCY", latency)
        y = fa.decode_flac_device(comp, st, nb, case.x.shape[1], is_int64=case.is_int64)
        assert torch.equal(y.cpu(), want), f"{case.name}: decode (FLACARRAY_HIP_LATENCY={latency}) differs from the input"
    monkeypatch.delenv("FLACARRAY_HIP_LATENCY", raising=False)


@pytest.mark.parametrize("case,route", PARAMS)
def test_route_writes_the_oracle_bytes(fa, oracle, monkeypatch, case, route):
    import torch

    x = case.x
    blob_o, st_o, nb_o = _oracle_encode(oracle, case)
    _set_env(monkeypatch, ROUTE_ENV[route])
    info = None
    if route in ("k3f", "auto", "slots", "verify"):
        d = torch.from_numpy(x).cuda()
        if route == "k3f":
            assert d.data_ptr() % 16 == 0 and fa._lib.lib().fa_encode_single_pass_supported(x.shape[0], x.shape[1], case.level) == 1
        if route == "slots":
            assert fa._lib.lib().fa_encode_single_pass_supported(x.shape[0], x.shape[1], case.level) == 0
        comp, st, nb, info = fa.encode_flac_device(d, level=case.level, return_info=True, verify=(route == "verify"))
        torch.cuda.synchronize()
        blob_g, st_g, nb_g, info = comp.cpu().numpy(), st.cpu().numpy(), nb.cpu().numpy(), info.cpu().numpy()
    elif route == "host":
        blob_g, st_g, nb_g = fa.encode_flac(x, case.level)
        blob_g = np.asarray(blob_g)
    else:
        cut = case.append_cut
        arr = fa.FlacArray.from_array(np.ascontiguousarray(x[:, :cut]), level=case.level)
        arr.append(np.ascontiguousarray(x[:, cut:]), level=case.level)
        assert arr.shape == x.shape
        blob_g, st_g, nb_g = np.asarray(arr.compressed), np.asarray(arr.stream_starts), np.asarray(arr.stream_nbytes)
    same = (blob_g.shape == blob_o.shape and np.array_equal(blob_g, blob_o) and np.array_equal(np.asarray(nb_g).reshape(-1), nb_o)
            and np.array_equal(np.asarray(st_g).reshape(-1), st_o))
    diff = _frame_diff(oracle, case, info) if info is not None else ""
    if not same:
        first = int(np.argmax(blob_g[: blob_o.size] != blob_o[: blob_g.size])) if blob_g.size and blob_o.size else 0
        pytest.fail(f"{case.name} via {route}: compressed bytes differ from the oracle ({blob_g.size} against {blob_o.size} bytes, first at {first})\n{diff}")
    assert not diff, f"{case.name} via {route}: return_info differs from stream_info\n{diff}"
    _set_env(monkeypatch, {})
    dev = torch.device("cuda")
    _decodes_back(fa, monkeypatch, case, torch.from_numpy(blob_g).to(dev), torch.from_numpy(np.asarray(st_g).reshape(-1)).to(dev),
                  torch.from_numpy(np.asarray(nb_g).reshape(-1)).to(dev))
