"""tests/scratch_cases.py on the CPU: every scratch slot the library hands out (the get_scratch(<literal>, ...) calls of
flacarray_amd/csrc/flacarray_hip.hip, read from the source) is claimed by a case, so a slot added later without a case
fails here and not silently on the GPU; kScratchSlots covers exactly the slots used; the debug entry points are declared,
bound and exported, and nothing but the tests calls them."""
import ctypes
import os
import re
import subprocess

from flacarray_amd import _lib
from tests import scratch_cases as SC
from tests.conftest import ROOT

HIP = os.path.join(ROOT, "flacarray_amd", "csrc", "flacarray_hip.hip")
HEADER = os.path.join(ROOT, "include", "flacarray_hip.h")
DEBUG_SYMBOLS = ("fa_debug_scratch_fill", "fa_debug_scratch_bytes")


def _source():
    with open(HIP) as f:
        return f.read()


def _slots(text):
    calls = re.findall(r"\bget_scratch\(\s*([^,]+),", text)
    literal = [c for c in calls if re.fullmatch(r"\d+", c.strip())]
    # every call names its slot by a literal, except the definition itself (`int slot`)
    assert sorted(set(calls) - set(literal)) == ["int slot"], "a get_scratch call whose slot is not a literal: %s" % (set(calls) - set(literal))
    return {int(c) for c in literal}


def test_every_slot_has_a_case():
    found = _slots(_source())
    claimed = set().union(*[c.slots for c in SC.CASES.values()])
    assert SC.STAMPS_SLOT in found and SC.STAMPS_SLOT not in claimed  # -DFA_STAMPS builds only: the one named exception
    assert claimed == found - {SC.STAMPS_SLOT}, "slots without a case: %s; claimed but not in the source: %s" % (
        sorted(found - claimed - {SC.STAMPS_SLOT}), sorted(claimed - found))


def test_slot_count_is_the_largest_slot_plus_one():
    text = _source()
    n = int(re.search(r"constexpr int kScratchSlots = (\d+);", text).group(1))
    assert n == max(_slots(text)) + 1
    out = (ctypes.c_int64 * n)(*([-1] * n))
    assert _lib.lib().fa_debug_scratch_bytes(out, n) == n  # (no device: every slot reads empty)


def test_a_new_slot_without_a_case_is_noticed():
    text = _source().replace("get_scratch(22, 256, &ps)", "get_scratch(23, 256, &ps)")
    assert 23 in _slots(text) and 23 not in set().union(*[c.slots for c in SC.CASES.values()])


def test_partners_exist_and_share_a_slot():
    for c in SC.CASES.values():
        if c.partner is not None:
            p = SC.CASES[c.partner]
            assert p.name != c.name
            assert not c.slots or (c.slots & p.slots), "%s and its leftover partner %s share no slot" % (c.name, p.name)
    assert set(SC.ENCODER_CASES) <= set(SC.CASES)


def test_debug_entry_points_are_declared_bound_and_test_only():
    with open(HEADER) as f:
        header = f.read()
    assert re.search(r"^#define FA_ABI_VERSION 4\b", header, re.M)  # entry points that are only added leave it as it is
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = {line.split()[-1] for line in out.splitlines() if line.strip()}
    for name in DEBUG_SYMBOLS:
        assert name in _lib.SYMBOLS and name in exported
        assert re.search(r"^int %s\(" % name, header, re.M), name
        getattr(_lib.lib(), name)
    assert _lib.lib().fa_debug_scratch_fill(256) != 0 and _lib.lib().fa_debug_scratch_fill(-2) != 0
    # no library code, tool or benchmark calls them
    paths = [os.path.join(ROOT, "bench.py"), os.path.join(ROOT, "__graft_entry__.py")]
    for top in ("flacarray_amd", "tools", "oracle"):
        for base, _, files in os.walk(os.path.join(ROOT, top)):
            paths += [os.path.join(base, fn) for fn in files if fn.endswith((".py", ".hpp", ".hip", ".sh", ".cpp", ".c"))]
    for path in paths:
        with open(path, errors="replace") as f:
            text = f.read()
        calls = len(re.findall(r"fa_debug_scratch_\w+\(", text))
        if path == HIP:
            assert calls == 2, "flacarray_hip.hip: the two definitions and no caller"
        elif not path.endswith("_lib.py"):
            assert "fa_debug_scratch" not in text, path
