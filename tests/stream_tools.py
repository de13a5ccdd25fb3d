"""Delayed-producer harness for the stream-order tests (tests/test_gpu_streams.py).

Every `fa_*_device` entry point promises that it reads its inputs, and completes its outputs, in the order of the stream
it is given.  On torch's default stream that promise cannot be broken visibly: the default stream is the null stream, so a
copy, memset or launch that the library put on the null stream by mistake is still in order.  A side stream made by torch
is non-blocking: the null stream gives it no implicit ordering, and a call whose inputs are still being produced on that
stream must wait for them through the stream alone.

`delayed_fill` makes that situation on purpose.  The targets hold a VALID DECOY (another array of the same shape, or the
encode of one) written on the default stream and synchronised; on the side stream a delay kernel runs first, then the real
data is copied over the decoy, then an event is recorded.  A call under test that is queued behind this on the same stream
sees the real data if every part of it is in stream order, and the decoy -- a wrong answer, never garbage -- if some
part is not.  `run_delayed` wraps the whole protocol of one case and asserts its conditions.

The delay is `torch.cuda._sleep`, calibrated once per session with events (spin cycles per millisecond), and checked once
to last at least as long as asked.  DELAY_MS is at least ten times the longest default-stream wall time of any single call
of tests/test_gpu_streams.py (profiles/streams.md has both figures): the host side of the call under test -- argument
checks, allocations, the launches up to the first wait -- must be over well inside the delay, or a missing dependency could
hide behind a slow host.
"""
import time

import numpy as np

# The issue's floor is ten times the longest warm default-stream call of tests/test_gpu_streams.py: 2.81 ms measured, the
# verified decode of 16384 frames included (profiles/streams.md), so 28.1 ms.  150 ms is 53 times that call: a host five
# times slower than the one measured still has the tenfold margin, at 13.5 s of delay kernels for the whole module (90 delayed calls).
DELAY_MS = 150.0

_cycles_per_ms = None
# wall time (s) of the second default-stream call of every case that ran, by case name (profiles/streams.md is sized on it)
WARM_SECONDS = {}


def _time_sleep(torch, stream, cycles):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    with torch.cuda.stream(stream):
        a.record(stream)
        torch.cuda._sleep(int(cycles))
        b.record(stream)
    b.synchronize()
    return a.elapsed_time(b)


def cycles_per_ms():
    """Spin cycles of torch.cuda._sleep per millisecond on the current device, measured once per session with events."""
    global _cycles_per_ms
    if _cycles_per_ms is None:
        import torch

        s = torch.cuda.Stream()
        _time_sleep(torch, s, 1_000_000)  # (loads the kernel)
        cycles = 20_000_000
        ms = _time_sleep(torch, s, cycles)
        assert ms > 0.05, f"torch.cuda._sleep({cycles}) took {ms} ms: it cannot serve as a delay on this device"
        rate = cycles / ms
        # the delay the tests will ask for must really last that long (a clock that changes speed between the two runs shows here)
        got = _time_sleep(torch, s, rate * DELAY_MS * 1.25)
        assert got >= DELAY_MS, f"calibrated for {DELAY_MS} ms (x1.25), measured {got:.2f} ms"
        _cycles_per_ms = rate * 1.25
    return _cycles_per_ms


def delayed_fill(side, pairs, delay=None):
    """On stream `side`: a delay of `delay` ms (default DELAY_MS), then target.copy_(real) for every (target, real) of
    `pairs` (device tensors, the targets holding their decoys), then an event, which is returned.  Nothing here waits."""
    import torch

    cycles = int(cycles_per_ms() * (DELAY_MS if delay is None else delay))
    with torch.cuda.stream(side):
        torch.cuda._sleep(cycles)
        for target, real in pairs:
            assert target.shape == real.shape and target.dtype == real.dtype and target.is_cuda and real.is_cuda
            target.copy_(real, non_blocking=True)
        ev = torch.cuda.Event()
        ev.record(side)
    return ev


def pad_blob(torch, blob, size):
    """`blob` (uint8 device tensor) at the front of a zeroed buffer of `size` bytes: the real and the decoy streams of a
    decode case share one buffer, sized for the larger of the two."""
    out = torch.zeros(size, dtype=torch.uint8, device=blob.device)
    out[: blob.numel()] = blob
    return out


def to_host(x):
    """Outputs of a call as comparable host values: tensors and arrays become numpy arrays, tuples / lists recurse."""
    if x is None or isinstance(x, (int, float, bool, str)):
        return x
    if isinstance(x, (tuple, list)):
        return [to_host(v) for v in x]
    if isinstance(x, np.ndarray):
        return np.array(x, copy=True)
    return x.detach().cpu().numpy()


def same(a, b):
    """Bit-for-bit equality of two to_host() results (floats compared through their bytes: NaN == NaN, -0.0 != 0.0)."""
    if isinstance(a, list):
        return isinstance(b, list) and len(a) == len(b) and all(same(x, y) for x, y in zip(a, b))
    if isinstance(a, np.ndarray):
        return isinstance(b, np.ndarray) and a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()
    return a == b


def _clone_outputs(x):
    import torch

    if isinstance(x, (tuple, list)):
        return [_clone_outputs(v) for v in x]
    return x.clone() if isinstance(x, torch.Tensor) else x


def run_delayed(name, side, real, decoy, call):
    """One side-stream case.  `real` / `decoy`: lists of device tensors of equal shapes and dtypes, complete on the default
    stream; `call(*inputs)` makes the call under test and returns its outputs (tensors, numpy arrays, nested tuples).

    1. `call(*real)` twice on the default stream: the first is the warm call that grows every scratch slot and yields
       the expected result, the second is timed (WARM_SECONDS[name]) and must repeat it.
    2. `call(*decoy)` on the default stream: its result must DIFFER from the expected one, or the case proves nothing.
    3. targets = copies of the decoys, device synchronised.  Under torch.cuda.stream(side): delayed_fill, the event must not
       have happened, the call, every output cloned on the side stream; then side.synchronize().
    Returns (result of the side-stream call, expected result), both as to_host() gives them, after asserting them equal."""
    import torch

    assert len(real) == len(decoy)
    torch.cuda.synchronize()
    expected = to_host(call(*real))
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    again = call(*real)
    torch.cuda.synchronize()
    WARM_SECONDS[name] = time.perf_counter() - t0
    assert same(to_host(again), expected), f"{name}: two default-stream calls disagree"
    fooled = to_host(call(*decoy))
    assert not same(fooled, expected), f"{name}: the decoy gives the result of the real input; the case could not tell them apart"
    targets = [d.clone() for d in decoy]
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        ev = delayed_fill(side, list(zip(targets, real)))
        assert not ev.query(), f"{name}: the producer had finished before the call was made; lengthen the delay"
        out = _clone_outputs(call(*targets))
    side.synchronize()
    got = to_host(out)
    assert same(got, expected), f"{name}: the call on the side stream did not wait for its inputs (or its outputs were not complete in stream order)"
    return got, expected
