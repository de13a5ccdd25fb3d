"""The preconditions of tests/test_gpu_far.py, asserted on the CPU: every placement of tests/far_corpus.py crosses the mark
it names, every truncated start addresses a decoy, and the long streams cross their thresholds."""
import hashlib

import numpy as np
import pytest

from tests import far_corpus as FC
from tests.golden import flac_writer as W


@pytest.fixture(scope="module")
def kits(oracle):
    return {name: FC.Kit(name, oracle, W, hashlib.md5) for name in FC.KITS}


def test_blob_geometry():
    assert FC.BLOB_BYTES == 2**32 + 2**20 and FC.BLOB_BYTES % 16 == 0
    assert FC.MARKS == (2**31, 2**32)
    assert sorted(FC.ROLES) == sorted("EBZAHL") and FC.DECOY == len(FC.ROLES)


@pytest.mark.parametrize("name", list(FC.KITS))
def test_kit_streams(kits, oracle, name):
    """Every row is a stream of its own with other samples than every other row, a few frames, the last one short, and
    frames long enough for a mark to sit inside a residual; the oracle decodes each from its own bytes."""
    k = kits[name]
    assert len(k.streams) == FC.ROWS + 1 and k.x.shape == (FC.ROWS + 1, k.n)
    assert k.nf >= 3 and k.n % k.B != 0 and k.min_frame >= FC.MIN_FRAME_BYTES
    assert len({row.tobytes() for row in k.x}) == FC.ROWS + 1
    for s, row in zip(k.streams, k.x):
        assert bytes(s[:4]) == b"fLaC"
        dec = oracle.decode_i64 if k.wide else oracle.decode_i32
        assert np.array_equal(dec(s, np.zeros(1, np.int64), np.array([s.size], np.int64), k.n).reshape(-1), row)
    if k.layout == "stripped":
        assert all(s[4] == 0x80 and FC.metadata_walk(s) == (42, None) for s in k.streams)
        assert all(np.array_equal(a[-100:], b[-100:]) and a.size == b.size - 4 - 18 * k.nf for a, b in zip(k.streams, k.own))
    if k.layout == "signed":
        assert all(bytes(s[26:42]) == hashlib.md5(row.tobytes()).digest() for s, row in zip(k.streams, k.x))
    else:
        assert k.layout == "writer" or all(not s[26:42].any() for s in k.streams)


@pytest.mark.parametrize("layout", FC.LAYOUTS)
@pytest.mark.parametrize("name", list(FC.KITS))
def test_placement(kits, name, layout):
    k = kits[name]
    st = k.starts(layout)
    end = st + k.nb
    at = dict(zip(FC.ROLES, st[: FC.ROWS]))
    # inside the blob, pairwise disjoint, and the index is not sorted by address
    assert st.min() >= 0 and end.max() == FC.BLOB_BYTES
    order = np.argsort(st)
    assert np.all(end[order][:-1] <= st[order][1:])
    assert np.any(np.diff(st[: FC.ROWS]) < 0) and np.any(np.diff(st[: FC.ROWS]) > 0)
    # the marks
    for role, mark in (("A", FC.M31), ("B", FC.M32)):
        i = FC.ROLES.index(role)
        if layout == "straddle":
            spans = FC.frame_spans(k.own[i] if k.layout == "stripped" else k.streams[i], k.nf)
            a, b = spans[1]
            if k.layout == "stripped":
                a, b = a - 4 - 18 * k.nf, b - 4 - 18 * k.nf
            assert st[i] < mark < end[i]
            # inside the second frame, 16 bytes in front of its CRC-16 and hundreds of bytes behind its header
            assert st[i] + b - mark == FC.STRADDLE_BACK and mark - (st[i] + a) >= FC.MIN_FRAME_BYTES - FC.STRADDLE_BACK
            assert end[i] - mark > FC.MIN_FRAME_BYTES  # (two more frames lie behind the mark)
        else:
            assert st[i] == mark + (3 if layout == "plus3" else 0)
    # the ends of the blob
    assert at["Z"] == (3 if layout == "plus3" else 0)
    assert end[FC.ROLES.index("E")] == FC.BLOB_BYTES
    assert at["H"] % 2 == 1 and at["L"] % 2 == 1 and FC.M31 < at["H"] < FC.M32 and at["L"] < FC.M31
    # decoys: a start that does not fit 32 bits, truncated, addresses another stream of the kit's geometry
    far = [i for i in range(FC.ROWS) if st[i] >= FC.M32]
    assert FC.ROLES.index("E") in far and ((FC.ROLES.index("B") in far) == (layout != "straddle"))
    for i in far:
        t = FC.truncated(st[i])
        assert t != st[i]
        hit = [j for j in range(FC.ROWS + 1) if st[j] == t]
        assert len(hit) == 1 and hit[0] != i
        assert not np.array_equal(k.x[hit[0]], k.x[i]) and bytes(k.streams[hit[0]][:4]) == b"fLaC"


def test_every_placement_of_the_issue_is_present(kits):
    for k in kits.values():
        sts = {layout: k.starts(layout) for layout in FC.LAYOUTS}
        for i in (FC.ROLES.index("A"), FC.ROLES.index("B")):
            mark = FC.M31 if FC.ROLES[i] == "A" else FC.M32
            assert sts["at"][i] == mark and sts["plus3"][i] == mark + 3 and sts["straddle"][i] < mark < sts["straddle"][i] + k.nb[i]
        assert sts["at"][FC.ROLES.index("Z")] == 0 and sts["straddle"][FC.ROLES.index("Z")] == 0


def test_spot_rows():
    nb = np.full(100, 2**27, dtype=np.int64)
    st = np.cumsum(nb) - nb
    assert FC.spot_rows(st, nb) == [0, 15, 16, 17, 31, 32, 33, 99]  # (byte 2^31 is the first of row 16)
    st = st + 5
    assert FC.spot_rows(st, nb) == [0, 14, 15, 16, 30, 31, 32, 99]


def test_part_b_stream_count(oracle):
    """The stream count from the oracle's size of one stream of full-range noise: slightly more than four bytes per
    sample, and the packed blob exceeds 1.25 * 2^32."""
    x = np.random.default_rng(1).integers(-(2**31), 2**31, (1, FC.B_N), dtype=np.int64).astype(np.int32)
    one = int(oracle.encode_i32(x, 5)[2][0])
    assert 4 * FC.B_N < one < 4.01 * FC.B_N
    ns = FC.b_stream_count(one)
    assert ns * one > FC.B_MIN_BLOB and (ns // 2) * one > FC.B_MIN_OUTPUT >= (ns // 2 - 2) * one
    assert FC.B_MIN_BLOB == 5 * 2**30 and FC.B_MIN_OUTPUT == 2**32 + 2**26


def test_part_c_thresholds():
    assert FC.C1_NF > 65536 and -(-FC.C1_N // FC.C1_BLOCK) == FC.C1_NF and FC.C1_N % FC.C1_BLOCK != 0
    assert 18 * FC.C1_NF < 2**24
    assert FC.utf8_bytes(65535) == 3 and FC.utf8_bytes(65536) == 4 and FC.utf8_bytes(FC.C1_NF - 1) == 4
    assert {65535, 65536} <= set(FC.C1_NOISE) and {0, FC.C1_NF - 1} <= set(FC.C1_NOISE)
    for n in (FC.C2_N20, FC.C2_N17):
        assert n > 2**31 and -(-n // FC.C2_BLOCK) == FC.C2_NF and n % FC.C2_BLOCK in (17, 20)
    assert FC.C2_NF > 65536 and 18 * FC.C2_NF < 2**24
    assert FC.C2_N0 % FC.C2_BLOCK == 0 and 524288 * FC.C2_BLOCK == 2**31
    # a rare frame on each side of every threshold: frame number 2^16, sample 2^31
    assert {65535, 65536, 524287, 524288, FC.C2_NF - 2, FC.C2_NF - 1, 0} <= set(FC.C2_NOISE)
    assert 524287 * FC.C2_BLOCK < 2**31 <= 524288 * FC.C2_BLOCK


def test_sparse_frames_small():
    noise = FC.sparse_frames(2, 10 * 16 - 3, 16, (0, 4, 9), seed=3)
    x = FC.sparse_host(2, 157, 16, noise)
    assert x.shape == (2, 157) and x[:, 16:64].any() == 0 and x[0, :16].any() and x[1, 144:].any() and noise[(0, 9)].size == 13
    assert not np.array_equal(x[0], x[1])
