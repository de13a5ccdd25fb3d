"""CPU preconditions of the frame CRC-16 tests (tests/verify_corpus.py, run on the GPU by tests/test_gpu_verify_matrix.py):
every store decodes, both CRCs right, to its array in the independent decoder tests/golden/pyflac.py; every damage site
fails that decoder's CRC-16 assertion in its frame and in no other; with that assertion satisfied by a re-stamped CRC the
frame decodes to what the model predicts; and the frames of chosen length cover the lengths they are meant to."""
import hashlib

import numpy as np
import pytest

from tests import verify_corpus as V
from tests.golden import make_golden as G
from tests.golden import pyflac


def _decode(data, channels):
    out, info = pyflac.decode_stream(bytes(data))
    return V.as_rows(out, channels), info


@pytest.mark.parametrize("name", V.STORES)
def test_store_decodes_intact_and_is_signed(name):
    st = V.build_store(name)
    assert st.data.dtype == (np.int32 if st.channels == 1 else np.int64) and st.data.shape == (len(st.frames), st.n)
    for s in sorted({x.stream for x in V.sites(name)}):
        seg = st.blob[st.starts[s] : st.starts[s] + st.nbytes[s]]
        got, info = _decode(seg, st.channels)
        assert np.array_equal(got, st.data[s]), (name, s)
        b = V.block_of(st, s)
        assert info["min_bs"] == info["max_bs"] == b and info["total"] == st.n and len(info["frames"]) == -(-st.n // b)
        assert [d["offset"] for d in info["frames"]] == [fr.start - st.starts[s] for fr in st.frames[s]]
        assert st.n % b != 0  # a short last frame
        assert bytes(seg[26:42]) == hashlib.md5(st.data[s].astype("<i4" if st.channels == 1 else "<i8").tobytes()).digest()
        assert (3 in [t for t, _ in info["blocks"]]) == (name in ("m1_own4096", "m1_own1152", "m2_own1152", "m4_coded") or (name == "m2_foreign64" and s % 2 == 1))
        for f, (fr, d) in enumerate(zip(st.frames[s], info["frames"])):
            verbatim = d["type"] == "verbatim" and d["wasted"] == 0 if st.channels == 1 else (
                d["assignment"] == 1 and d["subs"][0]["type"] == "verbatim" and d["subs"][0]["wasted"] == 0)
            assert (fr.payload is not None) == verbatim, (name, s, f)
    if name in V.M4:
        assert all(fr.payload is None for row in st.frames for fr in row)  # every frame coded: footer sites only
    elif name not in V.M2:
        assert all(fr.payload is not None for row in st.frames for fr in row)  # full-range data: all VERBATIM
    if name == "m2_foreign64":
        asg = {(st.blob[fr.start + 3] >> 4) for row in st.frames for fr in row}
        assert asg == {1, 8, 9, 10}
    if name in V.M3:
        assert sorted(set(st.block)) == sorted(V.MIXED_BLOCKS)


@pytest.mark.parametrize("name", V.STORES)
def test_which_frames_have_sites(name):
    st = V.build_store(name)
    sites = V.sites(name)
    ns = len(st.frames)
    if name in V.M3:
        want = {(s, f) for s in range(ns) for f in {0, len(st.frames[s]) // 2, len(st.frames[s]) - 1}}
    else:
        want = {(s, f) for s in {0, ns // 2, ns - 1} for f in range(len(st.frames[s]))}
    assert {(x.stream, x.frame) for x in sites if x.kind == "footer"} == want
    assert {(x.stream, x.frame) for x in sites if x.kind == "payload"} == {sf for sf in want if st.frames[sf[0]][sf[1]].payload is not None}
    assert {x.offset - (st.frames[x.stream][x.frame].nbytes - 2) for x in sites if x.kind == "footer"} == {0, 1}
    assert (ns, len(st.frames[0])) == {"m1": (5, 9), "m2": (3, 5), "m3": (5, 49), "m4": (5, 9)}[name[:2]]


@pytest.mark.parametrize("name", V.STORES)
def test_every_site_fails_its_frame_only_and_decodes_to_the_model(name):
    st = V.build_store(name)
    intact = {}
    for site in V.sites(name):
        fr = st.frames[site.stream][site.frame]
        lo, hi = V.frame_span(st, site.stream, site.frame)
        bad = V.damage(st.blob, st, site)
        diff = np.flatnonzero(bad != st.blob)
        assert diff.tolist() == [V.byte_of(st, site)] and fr.start <= diff[0] < fr.start + fr.nbytes  # every other frame is as it was
        if site.kind == "footer":
            assert diff[0] >= fr.start + fr.nbytes - 2
        else:
            assert fr.start + fr.payload <= diff[0] < fr.start + fr.payload + 4 * fr.m and lo <= site.sample < hi
        # the frame alone behind CONSTANT frames: intact it passes, damaged it fails the CRC-16 assertion (both CRCs of
        # the frames in front are right, so the failure is this frame's), re-stamped it decodes to the model
        if (site.stream, site.frame) not in intact:
            good, front = V.isolated_frame_stream(st, site, st.blob)
            got, _ = _decode(good, st.channels)
            assert np.array_equal(got[front:], st.data[site.stream, lo:hi]) and not got[:front].any()
            intact[site.stream, site.frame] = got
        with pytest.raises(AssertionError, match="CRC-16"):
            _decode(V.isolated_frame_stream(st, site, bad)[0], st.channels)
        stamped = V.restamp(bad, st, site)
        if site.kind == "footer":
            assert np.array_equal(stamped, st.blob)  # the right CRC is the one that was there: the intact frame, decoded above
            got = intact[site.stream, site.frame]
        else:
            framed, front = V.isolated_frame_stream(st, site, stamped)
            got, _ = _decode(framed, st.channels)
        front = site.frame * V.block_of(st, site.stream)
        model = V.unchecked(st, site)
        assert np.array_equal(got[front:], model[site.stream, lo:hi]), site
        changed = np.argwhere(model != st.data).tolist()
        assert changed == ([] if site.kind == "footer" else [[site.stream, site.sample]])
        if site.kind == "payload":
            assert G.crc16(bytes(bad[fr.start : fr.start + fr.nbytes - 2])) != int.from_bytes(bytes(bad[fr.start + fr.nbytes - 2 : fr.start + fr.nbytes]), "big")


@pytest.mark.parametrize("name", V.STORES)
def test_ranges_and_slice_lists_meet_and_miss_the_damaged_frame(name):
    st = V.build_store(name)
    seen = set()
    for site in V.sites(name):
        lo, hi = V.frame_span(st, site.stream, site.frame)
        rs = V.ranges(st, site)
        assert [V.raises(st, site, a, b) for a, b in rs[:3]] == [True] * 3 and not any(V.raises(st, site, a, b) for a, b in rs[3:])
        assert ((0, lo) in rs) == (site.frame > 0) and ((hi, st.n) in rs) == (hi < st.n)
        assert all(0 <= a < b <= st.n for a, b in rs)
        assert V.raises(st, site, streams=[site.stream]) and not V.raises(st, site, streams=[s for s in range(len(st.frames)) if s != site.stream])
        touching, missing = V.slice_lists(st, site)
        assert V.slices_raise(st, site, touching) and not V.slices_raise(st, site, missing)
        inside = [min(f + c, hi) - max(f, lo) for s, f, c in touching if s == site.stream]
        assert inside == [1]  # by a single sample
        mine = [(f, c) for s, f, c in missing if s == site.stream]
        assert {f + c for f, c in mine if f < lo} == ({lo} if lo > 0 else set()) and {f for f, c in mine if f >= hi} == ({hi} if hi < st.n else set())
        for sl in (touching, missing):
            assert all(0 <= f and c > 0 and f + c <= st.n and 0 <= s < len(st.frames) for s, f, c in sl)
            assert len({s for s, _, _ in sl}) >= 2  # intact streams beside it
        seen.add("front" if lo > 0 else "back")
    assert seen == {"front", "back"}


def test_reduce_model_and_md5_status():
    st = V.build_store("m1_foreign64")
    mn, mx, sm, hi, lo = V.reduce_model(st.data, 3, 200)
    for r in range(len(st.frames)):
        seg = [int(v) for v in st.data[r, 3:200]]
        assert (int(mn[r, 0]), int(mx[r, 0]), int(sm[r, 0])) == (min(seg), max(seg), sum(seg))
        assert (int(hi[r, 0]) << 32) + int(lo[r, 0]) == sum(v * v for v in seg)
    st2 = V.build_store("m2_own1152")
    mn, mx, sm, hi, lo = V.reduce_model(st2.data)
    assert hi is None and lo is None and int(sm[1, 0]) == (sum(int(v) for v in st2.data[1]) + 2**63) % 2**64 - 2**63
    payload = [x for x in V.sites("m1_foreign64") if x.kind == "payload"][0]
    footer = [x for x in V.sites("m1_foreign64") if x.kind == "footer"][0]
    assert V.md5_status(st, footer).tolist() == [1] * 5
    assert V.md5_status(st, payload).tolist() == [0 if s == payload.stream else 1 for s in range(5)]
    assert V.pcm_md5(V.unchecked(st, payload)[payload.stream]) != V.pcm_md5(st.data[payload.stream])


# ------------------------------------------------------------------------------------------------- the beside path

def test_beside_stores():
    """4 x 4097 frames are 16388 tasks, at and above the 16384 from which the check runs beside the decoder -- a whole
    number of the check's workgroups of four; 3 x 5462 = 16386 are not, and 3 x 5461 = 16383 stay below."""
    for (ns, nf), tasks in ((V.BESIDE, 16388), (V.BESIDE_ODD, 16386), (V.AFTER, 16383)):
        st = V.beside_store(ns, nf)
        assert ns * nf == tasks and sum(len(row) for row in st.frames) == tasks and st.n == nf * V.BESIDE_BLOCK
        for s in (0, ns - 1) if (ns, nf) == V.BESIDE else (ns - 1,):
            got, info = _decode(st.blob[st.starts[s] : st.starts[s] + st.nbytes[s]], 1)
            assert np.array_equal(got, st.data[s])
            assert [d["offset"] for d in info["frames"]] == [fr.start - st.starts[s] for fr in st.frames[s]]
            assert {d["type"] for d in info["frames"]} == {"const", "verbatim"} and [t for t, _ in info["blocks"]] == [0, 4]
        for task in V.beside_tasks(ns, nf):
            site = V.task_site(st, task)
            assert (site.stream, site.frame) == divmod(task, nf) and site.kind == "footer" and 0 <= task < tasks
            fr = st.frames[site.stream][site.frame]
            body = bytes(V.damage(st.blob, st, site)[fr.start : fr.start + fr.nbytes])
            assert G.crc16(body[:-2]) != int.from_bytes(body[-2:], "big")
            assert G.crc16(body[:-2]) == int.from_bytes(bytes(st.blob[fr.start + fr.nbytes - 2 : fr.start + fr.nbytes]), "big")
    assert 16388 >= 16386 >= 16384 > 16383 and 16386 % 4 != 0 and 16383 % 4 != 0
    assert set(V.beside_tasks(*V.BESIDE)) >= {0, 16383, 16384, 16385, 16386, 16387} and len(V.beside_tasks(*V.BESIDE)) == 7
    assert V.beside_tasks(*V.BESIDE_ODD) == (16384, 16385) and V.beside_tasks(*V.AFTER) == (16382,)


# -------------------------------------------------------------------------------- frames of every length and placement

def test_lengths_covered():
    specs = V.length_specs()
    Ls = {sp.L for sp in specs}
    low = V.smallest_L()
    assert low == 12 and not any(V._spec_for(L) for L in range(1, low))  # header 7 + the shortest extras 1 + one sample
    assert set(range(low, V.SMALL_TOP + 1)) <= Ls
    for a, b in V.EDGE_GROUPS:
        assert set(range(a, b + 1)) <= Ls
        assert {L % 4 for L in range(a, b + 1)} == {0, 1, 2, 3}
        assert any(L % 256 == 0 for L in range(a + 1, b)) and (any(L % V.TRIP == 0 for L in range(a + 1, b)) or (a, b) == (2296, 2312))  # a stripe edge inside; a trip edge but for one
    assert {sp.L % 4 for sp in specs if sp.L <= V.SMALL_TOP} == {0, 1, 2, 3}
    assert {(sp.bs, sp.L // V.TRIP) for sp in specs if sp.bs in (4096, 16384)} == {(4096, 8), (16384, 32)}
    assert [sp.L for sp in specs if sp.bs == 65535] == [9 + 4 * 65535] and 9 + 4 * 65535 > 2**18
    # every way the header's length varies is used: frame numbers of one, two and three bytes, every sample-rate code,
    # both block-size codes
    assert {sp.no for sp in specs} == {0, 128, 2048}
    assert {sp.sr_code for sp in specs} == {9, 12, 13, 14} and {sp.bs_code for sp in specs} == {6, 7}
    assert 1 <= min(sp.bs for sp in specs) and max(sp.bs for sp in specs if sp.bs < 4096) <= 1600
    # the placement subset: every residue close behind a trip edge, within a stripe of one, within a trip of one
    pl = V.placement_specs()
    assert [sp.L for sp in pl] == list(V.PLACEMENT_L) and all(sp.no == (128 if sp.L % 4 == 0 and sp.bs > 256 else 0) for sp in pl)
    for lo_d, hi_d in ((0, 8), (8, 256), (256, 2048)):
        for base in (0, V.TRIP) if lo_d else (V.TRIP, 2 * V.TRIP):
            assert {sp.L % 4 for sp in pl if lo_d <= sp.L - base < hi_d} == {0, 1, 2, 3}, (lo_d, base)
    assert {sp.L % 4 for sp in pl if V.TRIP - 8 <= sp.L < V.TRIP} == {0, 1, 2, 3}


def test_length_stores_hold_what_the_specs_say():
    stores = V.length_stores()
    seen = []
    for ls in stores:
        st = ls.store
        assert len(ls.specs) == len(st.frames) and st.blob.size == st.starts[-1] + st.nbytes[-1] + 16 and not st.blob[-16:].any()
        for s, sp in enumerate(ls.specs):
            fr = st.frames[s][-1]
            assert fr.nbytes - 2 == sp.L and fr.m == sp.bs and len(st.frames[s]) == sp.no + 1 and fr.payload == sp.L - 4 * sp.bs
            assert fr.start + fr.nbytes == st.starts[s] + st.nbytes[s]
            seen.append(sp)
            labels = [lab for lab, _ in V.length_sites(st, s)]
            assert labels[0] == "first payload byte" and labels[-3:] == ["last payload byte", "footer byte 0", "footer byte 1"]
            for lab, site in V.length_sites(st, s):
                if lab.startswith("lane"):
                    assert site.offset % 256 // 4 == int(lab.split()[1]) and fr.payload <= site.offset < sp.L
            lanes = {int(lab.split()[1]) for lab in labels if lab.startswith("lane")}
            assert lanes == {ln for ln in V.LANES if any(o % 256 // 4 == ln for o in range(fr.payload, sp.L))}
    assert sorted(seen) == sorted(V.length_specs())


def test_length_streams_decode():
    """Every stream of chosen frame length in the independent decoder (the 65535-sample frame, 2 Mbit, by its CRCs and
    bytes alone)."""
    for ls in V.length_stores():
        st = ls.store
        for s, sp in enumerate(ls.specs):
            seg = bytes(st.blob[st.starts[s] : st.starts[s] + st.nbytes[s]])
            fr = st.frames[s][-1]
            body = seg[fr.start - st.starts[s] :]
            assert G.crc16(body[:-2]) == int.from_bytes(body[-2:], "big")
            assert body[fr.payload : -2] == st.data[s, sp.no * sp.bs :].astype(">i4").tobytes()
            if sp.bs < 16384:
                got, info = _decode(seg, 1)
                assert np.array_equal(got, st.data[s]) and len(info["frames"]) == sp.no + 1
