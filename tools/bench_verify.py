"""Cost of checking a store against its input: compare_flac_device against decode_flac_device, encode_flac_device with and
without verify=True, and the numpy -> bytes host path (array_compress) with and without verification.

Headline geometry: 4096 x 2^20 int32 (bench.py's data, level 5), plus compare and decode of the same data as float32
(quanta 2^-16: the restore fused into the decoder, the quantisation into the compare) and of 1024 x 2^20 int64.  Each pair
is timed alternately in one process (device events around device calls, a host clock around host calls); the median and
the minimum of --reps runs are printed as one JSON line per case, and the ratio of each pair's medians.  Results:
profiles/encode_verify.md.  Usage: python -m tools.bench_verify [--reps N] [--small]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def _device_ms(torch, fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def _host_ms(fn):
    t0 = time.perf_counter()
    fn()
    return (time.perf_counter() - t0) * 1e3


def _pair(label, shape, fa_, fb_, timer, reps):
    """Alternate the two calls `reps` times after one warm-up of each; print both and the ratio of their medians."""
    fa_(), fb_()
    ta, tb = [], []
    for _ in range(reps):
        ta.append(timer(fa_))
        tb.append(timer(fb_))
    out = []
    for name, t in zip(label, (ta, tb)):
        rec = {"case": name, "shape": list(shape), "ms": round(float(np.median(t)), 3), "ms_min": round(float(np.min(t)), 3)}
        print(json.dumps(rec), flush=True)
        out.append(rec)
    print(json.dumps({"ratio": f"{label[1]} / {label[0]}", "median": round(out[1]["ms"] / out[0]["ms"], 3)}), flush=True)


def main():
    import torch

    import flacarray_amd as fa
    from bench import make_data

    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--small", action="store_true", help="1/64 of the rows (a rehearsal)")
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    rows = 4096 // (64 if args.small else 1)
    n = 1 << 20
    dt = lambda f: _device_ms(torch, f)  # noqa: E731

    x = make_data(torch, rows, n, 123456789, dev)
    comp, st, nb = fa.encode_flac_device(x, level=5)
    assert (fa.compare_flac_device(comp, st, nb, x) == -1).all()
    _pair(("decode_flac_device", "compare_flac_device"), x.shape, lambda: fa.decode_flac_device(comp, st, nb, n),
          lambda: fa.compare_flac_device(comp, st, nb, x), dt, args.reps)
    del comp, st, nb
    torch.cuda.empty_cache()
    _pair(("encode_flac_device(verify=False)", "encode_flac_device(verify=True)"), x.shape,
          lambda: fa.encode_flac_device(x, level=5), lambda: fa.encode_flac_device(x, level=5, verify=True), dt, args.reps)

    xh = x.cpu().numpy()
    del x
    torch.cuda.empty_cache()
    _pair(("array_compress(verify=False)", "array_compress(verify=True)"), xh.shape, lambda: fa.array_compress(xh, level=5, verify=False),
          lambda: fa.array_compress(xh, level=5, verify=True), _host_ms, args.reps)
    del xh

    xf = make_data(torch, rows, n, 123456789, dev).to(torch.float32) / 65536.0
    qf = torch.full((rows,), 2.0**-16, dtype=torch.float32, device=dev)
    comp, st, nb, off, gain = fa.encode_flac_device_f32(xf, qf, level=5)
    assert (fa.compare_flac_device(comp, st, nb, xf, off, gain) == -1).all()
    _pair(("decode_flac_device float32", "compare_flac_device float32"), xf.shape,
          lambda: fa.decode_flac_device(comp, st, nb, n, offsets=off, gains=gain), lambda: fa.compare_flac_device(comp, st, nb, xf, off, gain),
          dt, args.reps)
    del xf, comp, st, nb
    torch.cuda.empty_cache()

    rows64 = 1024 // (64 if args.small else 1)
    x32 = make_data(torch, rows64, n, 5, dev)
    x64 = x32.to(torch.int64) * 8192 + torch.randint(-4096, 4096, x32.shape, device=dev, dtype=torch.int64)
    del x32
    comp, st, nb = fa.encode_flac_device(x64, level=5)
    assert (fa.compare_flac_device(comp, st, nb, x64) == -1).all()
    _pair(("decode_flac_device int64", "compare_flac_device int64"), x64.shape, lambda: fa.decode_flac_device(comp, st, nb, n, is_int64=True),
          lambda: fa.compare_flac_device(comp, st, nb, x64), dt, args.reps)


if __name__ == "__main__":
    main()
