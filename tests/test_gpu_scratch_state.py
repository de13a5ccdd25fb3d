"""Every device operation on scratch that is dirty on purpose.  The library keeps grow-only scratch slots per GPU that
are never cleared, and the Python layer hands every call buffers from torch.empty: a word that is read before it is
written gives wrong results with return code 0, and what it reads depends on what ran before.

Each case of tests/scratch_cases.py runs under three poisons (0x00, 0xFF, 0xA5) in three states:
  filled    one call (checked) so that every slot has its final size, fa_debug_scratch_fill(p), the call again;
  grown     fa_release_scratch, then fa_debug_scratch_fill(p) with nothing held: every slot the call allocates is fresh
            and filled, and afterwards fa_debug_scratch_bytes shows exactly the slots the case claims;
  leftover  no fill: a larger case of another kind that shares slots runs first.
In every state torch.empty (and Tensor.new_empty) return device memory filled with the poison, and the raw calls of
fa_window_device / fa_join_device take a workspace of exactly the queried size, poisoned, with a guard behind it.
Every result is compared with the oracle, numpy, hashlib or a byte-level model -- see the cases."""
import ctypes

import numpy as np
import pytest

from tests import scratch_cases as SC

pytestmark = pytest.mark.gpu

POISONS = {"zeros": 0x00, "ones": 0xFF, "a5": 0xA5}
STATES = ("filled", "grown", "leftover")
NAMES = sorted(SC.CASES)


@pytest.fixture(scope="module")
def torch():
    import torch

    assert torch.cuda.is_available()
    return torch


@pytest.fixture(scope="module")
def fa():
    import flacarray_amd

    return flacarray_amd


@pytest.fixture(scope="module")
def L():
    from flacarray_amd import _lib

    return _lib.lib()


@pytest.fixture(scope="module", autouse=True)
def _fill_stays_in_this_file(torch, L):
    """No other test file ever runs with the sticky fill on, or on slots this file left poisoned."""
    yield
    torch.cuda.synchronize()
    assert L.fa_debug_scratch_fill(-1) == 0
    L.fa_release_scratch()


@pytest.fixture(autouse=True)
def _own_state(monkeypatch, torch, L):
    for v in ("FLACARRAY_HIP_PLACED_BELOW", "FLACARRAY_HIP_LATENCY", "FLACARRAY_HIP_SLOTS", "FLACARRAY_HIP_NO_SYNC_SCAN",
              "FLACARRAY_HIP_HOST_CHUNK_BYTES"):
        monkeypatch.delenv(v, raising=False)
    yield
    torch.cuda.synchronize()
    assert L.fa_debug_scratch_fill(-1) == 0


def _dirty_allocations(torch, monkeypatch, poison):
    """torch.empty and Tensor.new_empty give device memory full of the poison; the fill is queued on the current stream."""
    real_empty, real_new_empty = torch.empty, torch.Tensor.new_empty

    def dirty(t):
        if t.is_cuda and t.numel() and t.is_contiguous():
            t.reshape(-1).view(torch.uint8).fill_(poison)
        return t

    monkeypatch.setattr(torch, "empty", lambda *a, **kw: dirty(real_empty(*a, **kw)))
    try:
        monkeypatch.setattr(torch.Tensor, "new_empty", lambda self, *a, **kw: dirty(real_new_empty(self, *a, **kw)))
    except (AttributeError, TypeError):
        pass  # (a build whose Tensor does not take the attribute: torch.empty is the one the library calls)


def _fill(torch, L, byte):
    torch.cuda.synchronize()
    assert L.fa_debug_scratch_fill(byte) == 0


def _held(L):
    n = L.fa_debug_scratch_bytes(None, 0)
    out = (ctypes.c_int64 * n)()
    assert L.fa_debug_scratch_bytes(out, n) == n
    return {i for i in range(n) if out[i] > 0}


def _run_state(c, L, case, state, poison):
    torch = c.torch
    if state == "filled":
        _fill(torch, L, -1)
        case.fn(c)
        _fill(torch, L, poison)
        case.fn(c)
    elif state == "grown":
        torch.cuda.synchronize()
        L.fa_release_scratch()
        _fill(torch, L, poison)
        assert _held(L) == set()
        case.fn(c)
        torch.cuda.synchronize()
        assert _held(L) == set(case.slots), "%s leaves slots %s allocated, its claim is %s" % (case.name, sorted(_held(L)), sorted(case.slots))
    else:
        _fill(torch, L, -1)
        SC.CASES[case.partner].fn(c)
        case.fn(c)


def _ids():
    out = []
    for name in NAMES:
        for state in STATES:
            if state == "leftover" and SC.CASES[name].partner is None:
                continue  # (the encoders: filled and grown only; their leftovers are tests/test_gpu_call_state.py's)
            out.append((name, state))
    return out


@pytest.mark.parametrize("poison", sorted(POISONS))
@pytest.mark.parametrize("name,state", _ids(), ids=["%s-%s" % p for p in _ids()])
def test_case_on_dirty_scratch(torch, fa, L, oracle, monkeypatch, name, state, poison):
    p = POISONS[poison]
    _dirty_allocations(torch, monkeypatch, p)
    c = SC.Ctx(torch, fa, L, oracle, monkeypatch, p)
    _run_state(c, L, SC.CASES[name], state, p)


def test_fill_reaches_held_and_fresh_slots(torch, fa, L, oracle, monkeypatch):
    """The tool's bookkeeping: a fill neither allocates nor frees a slot, -1 switches the sticky fill off, a byte outside
    -1..255 is refused.  (That the fill reaches the words is what the scratch mutants of profiles/scratch_state.md show.)"""
    c = SC.Ctx(torch, fa, L, oracle, monkeypatch)
    L.fa_release_scratch()
    assert _held(L) == set()
    assert L.fa_debug_scratch_fill(256) != 0 and L.fa_debug_scratch_fill(-2) != 0
    _fill(torch, L, 0xA5)
    assert _held(L) == set()  # a fill allocates nothing
    SC.CASES["decode_i32"].fn(c)
    held = _held(L)
    assert held == set(SC.CASES["decode_i32"].slots)
    _fill(torch, L, -1)
    assert _held(L) == held  # and frees nothing


# ------------------------------------------------------------------------------------------------------ std plan walk
# (stream_size, chunk): B changes only the chunk, C only the stream size; none of the chunks is 8192, so each needs a plan.
WALK = {"A": (3 * 1152 + 200, 1008), "B": (3 * 1152 + 200, 704), "C": (2 * 1152 + 77, 704)}


@pytest.mark.parametrize("bump", ["fill", "release"])
@pytest.mark.parametrize("kind", ["f32", "f64"])
def test_std_plan_walk(torch, fa, L, monkeypatch, kind, bump):
    """The summation plans of slot 13 are cached by (stream_size, chunk, scratch epoch), not by address: walk the key one
    field at a time, make the cached plan stale between two steps (a fill of 0xFF over it, or a release after which the
    slot may come back at its old address), and come back to the first key.  Every step is np.std bit for bit at numpy's
    buffer size of that step."""
    _dirty_allocations(torch, monkeypatch, 0xFF)
    data = {k: SC.floats(kind, 5, n, 981 + i) for i, (k, (n, _)) in enumerate(WALK.items())}

    def step(k, what):
        n, chunk = WALK[k]
        old = np.getbufsize()
        np.setbufsize(chunk)  # numpy sums in chunks of its buffer size; std_device reads it at call time
        try:
            size = int(np.getbufsize())
            assert size == chunk
            want = np.std(data[k], axis=-1)
            got = fa.std_device(torch.from_numpy(data[k]).cuda())
        finally:
            np.setbufsize(old)
        assert SC.same(got, want), "%s (%s, stream_size %d, chunk %d)" % (what, k, n, size)

    for k in ("A", "B", "C", "A"):
        step(k, "walk")
    if bump == "fill":
        _fill(torch, L, 0xFF)
    else:
        torch.cuda.synchronize()
        L.fa_release_scratch()
    step("A", "the same key after the %s" % bump)
    step("B", "the chunk changed")
    if bump == "fill":
        _fill(torch, L, 0x00)
    step("B", "the same key after a second fill")
    step("A", "back to the first key")
