"""What the decode driver's entry points answer to calls they must refuse, pinned code by code.

Every device read, compare, reduce, histogram, find, salvage and index call goes through one driver; which check refuses a
bad call, and with which code, is part of the C ABI.  tests/decode_refusals.json holds what the library answered at the
commit its header names: one row per (entry point, bad call) with the returned code and, for the folding sinks, whether
the sentinel-filled result arrays were written.  This test asks again and compares row by row.
`python -m tests.test_gpu_decode_refusals --record <commit>` rewrites the file from the library in the tree
(FLACARRAY_HIP_LIB selects another build).

The store is 3 streams x 100 samples at block size 32, one- and two-channel, plus one decode index of each.  Every case
is refused by a host check or by the error word of the index step (K6) run over the valid store: no case asks a kernel
to read outside it."""
import ctypes
import json
import os
import sys

import numpy as np
import pytest

from flacarray_amd import _lib
from tests.golden import flac_writer as W

pytestmark = pytest.mark.gpu

TABLE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "decode_refusals.json")
N_STREAM, SIZE, BLOCK = 3, 100, 32
N_FRAMES = (SIZE + BLOCK - 1) // BLOCK
NBINS = 8
SENTINEL = 0x5A5A5A5A5A5A5A5A
WRONG = "store of the other channel count"


def vp(x):
    return ctypes.c_void_p(x)


class Store:
    """One store on the device, its index, and the arrays a call on it needs (all kept alive here)."""

    def __init__(self, torch, L, nch, seed):
        dev = "cuda"
        b = W._batch("refusals", np.random.default_rng(seed), N_STREAM, SIZE, BLOCK, nch, layout="libflac")
        blob, st, nb = W.pack(b["streams"])
        self.nch, self.n_bytes = nch, int(blob.size)
        self.blob = torch.from_numpy(blob).to(dev)
        self.starts, self.nb = torch.from_numpy(st).to(dev), torch.from_numpy(nb).to(dev)
        assert self.blob.data_ptr() % 16 == 0
        self.shifted = torch.zeros(blob.size + 32, dtype=torch.uint8, device=dev)  # the same bytes at an odd address
        self.shifted[1 : 1 + blob.size] = self.blob
        it, ft = (torch.int32, torch.float32) if nch == 1 else (torch.int64, torch.float64)
        self.itemsize = 4 * nch
        self.out_int = torch.zeros(N_STREAM * SIZE, dtype=it, device=dev)
        self.out_flt = torch.zeros(N_STREAM * SIZE, dtype=ft, device=dev)
        self.offsets, self.gains = torch.zeros(N_STREAM, dtype=ft, device=dev), torch.ones(N_STREAM, dtype=ft, device=dev)
        self.data = torch.zeros(N_STREAM * SIZE, dtype=it, device=dev)  # compare
        self.mismatch = torch.zeros(N_STREAM, dtype=torch.int64, device=dev)
        self.sel = torch.tensor([0, 2], dtype=torch.int64, device=dev)
        self.lo, self.hi = torch.full((N_STREAM,), -5, dtype=torch.int64, device=dev), torch.full((N_STREAM,), 5, dtype=torch.int64, device=dev)
        self.shift = torch.zeros(N_STREAM, dtype=torch.int32, device=dev)
        self.hit, self.offs = torch.zeros(1, dtype=torch.int64, device=dev), torch.zeros(N_STREAM * N_FRAMES + 1, dtype=torch.int64, device=dev)
        self.status = torch.zeros(N_STREAM * N_FRAMES, dtype=torch.uint8, device=dev)
        self.fill = np.zeros(1, dtype=np.int64)
        self.h_out = np.zeros(SIZE, dtype=np.int64)
        self.plan = (ctypes.c_int64 * 2)()
        # host slice arrays: one slice inside stream 1, and one that runs a sample past its end
        self.good_slice = [np.array([v], dtype=np.int64) for v in (1, 10, 20, 0)]
        self.long_slice = [np.array([v], dtype=np.int64) for v in (1, 90, 11, 0)]
        self.results = {}  # sink -> sentinel-filled result tensors
        for name, sizes in (("reduce", (N_STREAM * 4,) * 5), ("histogram", (N_STREAM * NBINS, N_STREAM, N_STREAM)),
                            ("find_count", (N_STREAM * N_FRAMES,)), ("find_fill", (16, 16))):
            self.results[name] = [torch.empty(s, dtype=torch.int64, device=dev) for s in sizes]
        index = ctypes.c_void_p()
        rc = L.fa_decode_index_create(*self.store_args(), nch, ctypes.byref(index), None)
        assert rc == 0 and index.value
        self.index = index

    def store_args(self):
        return [vp(self.blob.data_ptr()), self.n_bytes, vp(self.starts.data_ptr()), vp(self.nb.data_ptr()), N_STREAM, SIZE]


STORE6 = ("blob", "n_bytes", "starts", "nbytes", "n_stream", "stream_size")
OUT4 = ("out_int", "out_float", "offsets", "gains")
SLICES5 = ("n_slices", "slice_stream", "slice_first", "slice_count", "out_offset")


def entry_points(S):
    """[(label, function name, [(parameter, value)], sink or None)] of one store: a call that would succeed."""
    sfx = "i32" if S.nch == 1 else "i64"
    p = lambda t: None if t is None else t.data_ptr()  # noqa: E731
    store = list(zip(STORE6, (p(S.blob), S.n_bytes, p(S.starts), p(S.nb), N_STREAM, SIZE)))
    out = list(zip(OUT4, (p(S.out_int), None, None, None)))
    sl = list(zip(SLICES5, (1, *[a.ctypes.data for a in S.good_slice])))
    tail = [("stream", None), ("verify", -1)]
    rng, sel0 = [("first", -1), ("last", -1)], [("n_sel", 0), ("d_sel", None)]
    temp = [("max_temp", 0)]
    red, hist, cnt, fil = (S.results[k] for k in ("reduce", "histogram", "find_count", "find_fill"))
    red_out = [("d_min", p(red[0])), ("d_max", p(red[1])), ("d_sum", p(red[2]))]
    sq = [("d_sq_hi", p(red[3])), ("d_sq_lo", p(red[4]))]
    hist_args = [("nbins", NBINS), ("d_lo", p(S.lo)), ("d_shift", p(S.shift)), ("counts", p(hist[0])), ("below", p(hist[1])), ("above", p(hist[2]))]
    lim = [("d_lo", p(S.lo)), ("d_hi", p(S.hi)), ("inside", 0), ("n_frames", N_FRAMES)]
    fill = [("n_hit", 1), ("d_hit", p(S.hit)), ("d_offs", p(S.offs)), ("d_pos", p(fil[0])), ("d_val", p(fil[1]))]
    idx = [("index", S.index.value)]
    plan = [("block_size_out", ctypes.addressof(S.plan)), ("n_frames_out", ctypes.addressof(S.plan) + 8)]
    one = S.nch == 1
    return [
        ("decode_" + sfx, f"fa_decode_{sfx}_device", store + rng + out + tail, None),
        ("slices_" + sfx, f"fa_decode_slices_{sfx}_device", store + sl + out + tail, None),
        (f"indexed_range_{sfx}", "fa_decode_indexed", idx + rng + [("n_slices", -1)] + [(k, None) for k in SLICES5[1:]] + out + tail, None),
        (f"indexed_slices_{sfx}", "fa_decode_indexed", idx + [("first_unused", -1), ("last_unused", -1)] + sl + out + tail, None),
        (f"indexed_host_{sfx}", "fa_decode_indexed_host",
         idx + sl + out + [("h_out", S.h_out.ctypes.data), ("out_bytes", 20 * S.itemsize)] + tail, None),
        ("compare_" + sfx, f"fa_compare_{sfx}_device",
         store + [("d_data", p(S.data)), ("cmp_offsets", None), ("cmp_gains", None), ("mismatch", p(S.mismatch)), ("stream", None)], None),
        ("reduce_" + sfx, f"fa_reduce_{sfx}_device", store + rng + [("width", 25)] + sel0 + ([] if one else temp) + red_out + (sq if one else []) + tail, "reduce"),
        (f"reduce_indexed_{sfx}", "fa_reduce_indexed",
         idx + rng + [("width", 25)] + sel0 + temp + red_out + (sq if one else [("d_sq_hi", None), ("d_sq_lo", None)]) + tail, "reduce"),
        ("histogram_" + sfx, f"fa_histogram_{sfx}_device", store + rng + sel0 + ([] if one else temp) + hist_args + tail, "histogram"),
        (f"histogram_indexed_{sfx}", "fa_histogram_indexed", idx + rng + sel0 + temp + hist_args + tail, "histogram"),
        (f"find_plan_{sfx}", "fa_find_plan_device", [("plan_blob", p(S.blob)), ("n_bytes", S.n_bytes), ("starts", p(S.starts)), ("stream_size", SIZE)] + rng + plan + [("stream", None)], None),
        (f"find_plan_indexed_{sfx}", "fa_find_plan_indexed", idx + rng + plan, None),
        ("find_count_" + sfx, f"fa_find_count_{sfx}_device", store + rng + sel0 + ([] if one else temp) + lim + [("counts", p(cnt[0]))] + tail, "find_count"),
        (f"find_count_indexed_{sfx}", "fa_find_count_indexed", idx + rng + sel0 + temp + lim + [("counts", p(cnt[0]))] + tail, "find_count"),
        ("find_fill_" + sfx, f"fa_find_fill_{sfx}_device", store + rng + sel0 + ([] if one else temp) + lim + fill + tail, "find_fill"),
        (f"find_fill_indexed_{sfx}", "fa_find_fill_indexed", idx + rng + sel0 + temp + lim + fill + tail, "find_fill"),
        ("salvage_" + sfx, f"fa_decode_salvage_{sfx}_device",
         [("salvage_blob", store[0][1])] + store[1:] + rng + out + [("block_size", BLOCK), ("fill_value", S.fill.ctypes.data), ("d_status", p(S.status)), ("stream", None)], None),
        ("index_create_" + sfx, "fa_decode_index_create", store + [("channels", S.nch), ("index_out", None), ("stream", None)], None),
    ]


def bad_calls(S, other):
    """[(label, {parameter: value})]: applied to an entry point that has every parameter named."""
    p = lambda t: t.data_ptr()  # noqa: E731
    long_slice = dict(zip(SLICES5, (1, *[a.ctypes.data for a in S.long_slice])))
    return [
        ("n_stream 0", {"n_stream": 0}),
        ("stream_size 0", {"stream_size": 0}),
        ("both outputs", {"out_float": p(S.out_flt), "offsets": p(S.offsets), "gains": p(S.gains)}),
        ("no output", {"out_int": None, "out_float": None}),
        ("float output without gains", {"out_int": None, "out_float": p(S.out_flt), "offsets": p(S.offsets), "gains": None}),
        ("reversed range", {"first": 60, "last": 40}),
        ("overlong range", {"first": 0, "last": SIZE + 1}),
        ("slice past the stream end", long_slice),
        (WRONG, {"blob": p(other.blob), "n_bytes": other.n_bytes, "starts": p(other.starts), "nbytes": p(other.nb)}),
        ("n_sel 0", {"n_sel": 0, "d_sel": p(S.sel)}),
        ("n_sel -1", {"n_sel": -1, "d_sel": p(S.sel)}),
        ("null limits", {"d_lo": None}),
        ("n_frames off by one", {"n_frames": N_FRAMES + 1}),
        ("misaligned store", {"blob": p(S.shifted) + 1, "channels": S.nch}),
    ]


def ask(torch, L, stores):
    """{label: [code, touched]} of every (entry point, bad call) that applies; touched is None where no sink is involved."""
    pointers = {"blob", "plan_blob", "salvage_blob", "starts", "nbytes", "stream", "index", "index_out", "h_out", "d_data", "mismatch",
                "cmp_offsets", "cmp_gains", "d_sel", "d_min", "d_max", "d_sum", "d_sq_hi", "d_sq_lo", "d_lo", "d_hi", "d_shift", "counts",
                "below", "above", "d_hit", "d_offs", "d_pos", "d_val", "fill_value", "d_status", "block_size_out", "n_frames_out",
                "slice_stream", "slice_first", "slice_count", "out_offset", *OUT4}
    answers = {}
    for nch in (1, 2):
        S, other = stores[nch], stores[3 - nch]
        for label, fn, params, sink in entry_points(S):
            names = [k for k, _ in params]
            for bad, change in bad_calls(S, other):
                if not all(k in names for k in change):
                    continue
                args = dict(params)
                args.update(change)
                created = ctypes.c_void_p()
                if "index_out" in args:
                    args["index_out"] = ctypes.addressof(created)
                for t in S.results.get(sink, ()):
                    t.fill_(SENTINEL)
                torch.cuda.synchronize()
                code = int(getattr(L, fn)(*[vp(args[k]) if k in pointers else args[k] for k in names]))
                torch.cuda.synchronize()
                if created.value:
                    L.fa_decode_index_destroy(created)
                touched = None if sink is None else any(bool((t != SENTINEL).any().item()) for t in S.results[sink])
                answers[f"{label}: {bad}"] = [code, touched]
    return answers


@pytest.fixture(scope="module")
def answers():
    import torch

    L = _lib.lib()
    stores = {nch: Store(torch, L, nch, 20 + nch) for nch in (1, 2)}
    try:
        return ask(torch, L, stores)
    finally:
        for s in stores.values():
            L.fa_decode_index_destroy(s.index)


def _load():
    with open(TABLE) as f:
        return json.load(f)


def test_refusals_answer_what_the_table_holds(answers):
    t = _load()
    assert t["header"]["commit"] and t["header"]["how"]
    want = {r[0]: r[1:] for r in t["rows"]}
    assert sorted(want) == sorted(answers), sorted(set(want) ^ set(answers))[:5]
    bad = [(k, want[k], answers[k]) for k in want if want[k] != answers[k]]
    assert not bad, f"{len(bad)} answers changed, first (case, recorded [code, touched], now): {bad[:5]}"


def test_every_entry_point_meets_its_bad_calls(answers):
    """The table cannot pin an accident: every case but the empty selection is refused, every family of entry points is
    there on both channel counts, and a call refused for its arguments has written nothing to the sink's arrays."""
    assert len(answers) >= 200
    for k, (code, touched) in answers.items():
        if k.endswith(": n_sel 0"):
            assert code == 0 and touched is False, k  # (nothing selected: nothing to do, nothing written)
            continue
        assert code != 0, k
        if touched is not None and not k.endswith(WRONG):
            assert touched is False, k
    for sfx in ("i32", "i64"):
        for family in ("decode", "slices", "indexed_range", "indexed_slices", "indexed_host", "compare", "reduce", "reduce_indexed", "histogram",
                       "histogram_indexed", "find_plan", "find_plan_indexed", "find_count", "find_count_indexed", "find_fill",
                       "find_fill_indexed", "salvage", "index_create"):
            assert any(k.startswith(f"{family}_{sfx}: ") for k in answers), (family, sfx)
        # a count call on one channel is refused by K6 before the driver zeroes the counts
        assert answers[f"find_count_{sfx}: n_frames off by one"][1] is False
    assert answers[f"find_count_i32: {WRONG}"][1] is False
    assert "index_create_i32: misaligned store" in answers and "index_create_i64: misaligned store" in answers


if __name__ == "__main__":
    if len(sys.argv) == 3 and sys.argv[1] == "--record":
        import torch

        L = _lib.lib()
        stores = {nch: Store(torch, L, nch, 20 + nch) for nch in (1, 2)}
        got = ask(torch, L, stores)
        header = {
            "commit": sys.argv[2],
            "how": "python -m tests.test_gpu_decode_refusals --record <commit>, with the library built from that commit; each row is "
                   "'entry point: bad call', the returned code, and whether the sink's sentinel-filled result arrays were written "
                   "(null: no sink)",
        }
        with open(TABLE, "w") as f:
            f.write('{"header": ' + json.dumps(header) + ',\n "rows": [\n')
            f.write(",\n".join(json.dumps([k] + v, separators=(",", ":")) for k, v in got.items()))
            f.write("\n]}\n")
        print(TABLE, os.path.getsize(TABLE), "bytes,", len(got), "rows")
