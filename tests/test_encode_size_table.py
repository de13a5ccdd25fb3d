"""The encode driver's size queries, pinned value by value (CPU: the queries are pure arithmetic, no device).

Workspace and capacity sizes are part of the C ABI's contract with callers that allocate for themselves, and every encode
sequence, append and overwrite derives them from one frame plan.  tests/encode_size_table.json holds what the library
answered, over a grid of geometries and levels plus the refusals, at the commit its header names; this test asks again
and compares row by row.  `python -m tests.test_encode_size_table --record <commit>` rewrites the file from the library
in the tree (FLACARRAY_HIP_LIB selects another build)."""
import json
import os
import sys

from flacarray_amd import _lib

TABLE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "encode_size_table.json")
OLD_BYTES = 123457  # n_old_bytes of the append / overwrite capacity queries (it only adds)

N_STREAM = (1, 3, 12, 1000)
STREAM_SIZE = (1, 700, 1152, 4095, 4096, 4097, 8192, 9192, 12292, 1 << 20)
LEVELS = (0, 2, 3, 5, 8)
# (n_stream, stream_size, level): bad level, no streams, no samples, the SEEKTABLE limit (18 nf >= 2^24) and the last
# length below it for both block sizes, more than 2^31 - 1 frames and the largest count below that, negative counts
REFUSALS = (
    (8, 9192, 9), (0, 9192, 5), (8, 0, 5), (0, 0, 9), (-1, 9192, 5), (8, -1, 5),
    (1, 4096 * 932068, 5), (1, 4096 * 932068 - 4096, 5), (1, 1152 * 932068, 0), (1, 1152 * 932068 - 1152, 2),
    (1 << 22, 4096 * 512, 5), ((1 << 22) - 1, 4096 * 512, 5), (1 << 31, 4096, 3), ((1 << 31) - 1, 4096, 3),
)


def _appends(n_stream, size):
    return (1, 5000, 0)  # n: inside the old last frame (where there is room), several new frames, and the refusal


def _overwrites(n_stream, size):
    """(m, first, n): everything, one sample of one stream, a tail range of two streams, and the refusals m > n_stream,
    first + n > stream_size, m = 0."""
    return (
        (n_stream, 0, size), (1, size // 2, 1), (min(2, n_stream), max(0, size - 700), min(700, size)),
        (n_stream + 1, 0, 1), (1, size - 1, 2), (0, 0, 1),
    )


def _columns(n_stream, size, level):
    """(label, function name, arguments, FLACARRAY_HIP_SLOTS set?) of every query of one geometry, in the file's order."""
    g = (n_stream, size, level)
    cols = []
    for sfx in ("", "_i64"):
        cols.append(("slot_ws" + sfx, "fa_encode_workspace_bytes" + sfx, g, False))
        cols.append(("sp_ws" + sfx, "fa_encode_single_pass_workspace_bytes" + sfx, g, False))
        cols.append(("sp_ws" + sfx + "|SLOTS", "fa_encode_single_pass_workspace_bytes" + sfx, g, True))
        cols.append(("cap" + sfx, "fa_encode_capacity_bytes" + sfx, g, False))
    cols.append(("supported", "fa_encode_single_pass_supported", g, False))
    cols.append(("supported|SLOTS", "fa_encode_single_pass_supported", g, True))
    for sfx in ("", "_i64"):
        for i, n in enumerate(_appends(n_stream, size)):
            cols.append((f"append{i}_ws{sfx}", "fa_append_workspace_bytes" + sfx, (n_stream, size, n, level), False))
            cols.append((f"append{i}_cap{sfx}", "fa_append_capacity_bytes" + sfx, (OLD_BYTES, n_stream, size, n, level), False))
        for i, (m, first, n) in enumerate(_overwrites(n_stream, size)):
            cols.append((f"overwrite{i}_ws{sfx}", "fa_overwrite_workspace_bytes" + sfx, (n_stream, size, m, first, n, level), False))
            cols.append((f"overwrite{i}_cap{sfx}", "fa_overwrite_capacity_bytes" + sfx, (OLD_BYTES, n_stream, size, m, first, n, level), False))
    return cols


def _geometries():
    return [(ns, sz, lv) for ns in N_STREAM for sz in STREAM_SIZE for lv in LEVELS] + list(REFUSALS)


def _ask(L, cols, setenv, delenv):
    """The answers to `cols`; the environment variable is switched once per geometry, not per query."""
    out = [None] * len(cols)
    for slots in (False, True):
        if slots:
            setenv("FLACARRAY_HIP_SLOTS", "1")
        else:
            delenv("FLACARRAY_HIP_SLOTS")
        for i, (_, fn, args, want_slots) in enumerate(cols):
            if want_slots == slots:
                out[i] = int(getattr(L, fn)(*args))
    return out


def _load():
    with open(TABLE) as f:
        return json.load(f)


def test_size_table_covers_the_grid():
    t = _load()
    assert t["header"]["commit"] and t["header"]["how"]
    assert [tuple(r[:3]) for r in t["rows"]] == _geometries()
    assert t["columns"] == [c[0] for c in _columns(8, 9192, 5)]
    assert os.path.getsize(TABLE) < 100_000


def test_size_queries_answer_what_the_table_holds(monkeypatch):
    L = _lib.lib()
    t = _load()
    assert L.fa_encode_single_pass_workspace_bytes(8, 9192, 5) == 837888  # (the spot value the table was checked against)
    bad = []
    for n_stream, size, level, want in t["rows"]:
        cols = _columns(n_stream, size, level)
        got = _ask(L, cols, monkeypatch.setenv, lambda k: monkeypatch.delenv(k, raising=False))
        assert len(got) == len(want)
        bad += [(c[1], c[2], "SLOTS" if c[3] else "", w, g) for c, w, g in zip(cols, want, got) if w != g]
    assert not bad, f"{len(bad)} size queries changed, first (function, arguments, env, recorded, now): {bad[:5]}"


def test_refusals_are_refused():
    """What the table records for the refusals is -1 (0 for `supported`) -- the table cannot pin an accident."""
    t = _load()
    rows = {tuple(r[:3]): dict(zip(t["columns"], r[3])) for r in t["rows"]}
    for g in ((8, 9192, 9), (0, 9192, 5), (8, 0, 5), (1, 4096 * 932068, 5), (1 << 22, 4096 * 512, 5)):
        r = rows[g]
        assert r["supported"] == 0
        # (the two limits are the encode's: a splice plans the encode of its span, not of the old store)
        mine = [k for k in r if not k.startswith("supported") and (g[2] == 9 or min(g[:2]) <= 0 or not k.startswith(("append", "overwrite")))]
        assert len(mine) >= 8 and all(r[k] == -1 for k in mine), (g, r)
    # a geometry that encodes: only the bad append / overwrite arguments are refused (and nothing is single-pass under SLOTS)
    for label, v in rows[(12, 9192, 5)].items():
        if label.startswith(("append2_", "overwrite3_", "overwrite4_", "overwrite5_")):
            assert v == -1, label
        elif label == "supported|SLOTS":
            assert v == 0
        else:
            assert v > 0, label


if __name__ == "__main__":
    if len(sys.argv) == 3 and sys.argv[1] == "--record":
        L = _lib.lib()
        rows = []
        for g in _geometries():
            rows.append(list(g) + [_ask(L, _columns(*g), os.environ.__setitem__, lambda k: os.environ.pop(k, None))])
        header = {
            "commit": sys.argv[2],
            "how": "python -m tests.test_encode_size_table --record <commit>, with the library built from that commit; each row is "
                   "n_stream, stream_size, level, then the answers in the order of `columns` (a label ending in |SLOTS: asked with "
                   "FLACARRAY_HIP_SLOTS set; the append / overwrite arguments of a geometry are _appends / _overwrites of the test)",
        }
        with open(TABLE, "w") as f:
            f.write('{"header": ' + json.dumps(header) + ',\n "columns": ' + json.dumps([c[0] for c in _columns(8, 9192, 5)]) + ',\n "rows": [\n')
            f.write(",\n".join(json.dumps(r, separators=(",", ":")) for r in rows))
            f.write("\n]}\n")
        print(TABLE, os.path.getsize(TABLE), "bytes,", len(rows), "rows")
