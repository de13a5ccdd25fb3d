"""Cost of the STREAMINFO MD5: the lane-per-stream hash kernel on its own (md5_device), signing at encode time, and the
chunked decode-and-hash check beside a plain decode.

Geometries: 4096 x 2^20 int32 (bench.py's data, level 5); 65536 x 2^16 int32 (the same sample count with sixteen times
the streams: how far the serial chain of one stream, rather than throughput, sets the first number); 1024 x 2^20 int64;
4096 x 2^20 float32 quantised where it is loaded.  Method of tools/bench_verify.py: one warm-up, --reps alternations in one
process, device events around device calls and a host clock around host calls, median and minimum as one JSON line per
case.  Results: profiles/md5.md.

    python -m tools.bench_md5 [--reps N] [--small]
    python tools/bench_md5.py --encode-only [--tree DIR]    # encode_flac_device alone, from the package under DIR: the
                                                            # A/B of the md5=False path against another checkout
"""
import argparse
import inspect
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


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


def _report(name, shape, t, **more):
    rec = {"case": name, "shape": list(shape), "ms": round(float(np.median(t)), 3), "ms_min": round(float(np.min(t)), 3),
           "ms_max": round(float(np.max(t)), 3)}
    rec.update(more)
    print(json.dumps(rec), flush=True)
    return rec


def _cases(labels, shape, fns, timer, reps, **more):
    """Alternate the calls `reps` times after one warm-up of each; one line per call, and the ratio of the medians to the first."""
    for f in fns:
        f()
    ts = [[] for _ in fns]
    for _ in range(reps):
        for t, f in zip(ts, fns):
            t.append(timer(f))
    out = [_report(name, shape, t, **more) for name, t in zip(labels, ts)]
    for name, rec in zip(labels[1:], out[1:]):
        print(json.dumps({"ratio": f"{name} / {labels[0]}", "median": round(rec["ms"] / out[0]["ms"], 3)}), flush=True)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--small", action="store_true", help="1/64 of the rows (a rehearsal)")
    ap.add_argument("--encode-only", action="store_true", help="time encode_flac_device (signing off) and nothing else")
    ap.add_argument("--tree", default=ROOT, help="directory that holds the flacarray_amd package and bench.py to measure")
    args = ap.parse_args()
    sys.path.insert(0, os.path.abspath(args.tree))
    import torch

    import flacarray_amd as fa
    from bench import make_data

    dev = torch.device("cuda", 0)
    div = 64 if args.small else 1
    rows, n = 4096 // div, 1 << 20
    dt = lambda f: _device_ms(torch, f)  # noqa: E731
    x = make_data(torch, rows, n, 123456789, dev)

    if args.encode_only:
        kw = {"md5": False} if "md5" in inspect.signature(fa.encode_flac_device).parameters else {}
        label = "encode_flac_device(md5=False)" if kw else "encode_flac_device (no md5 keyword)"
        _cases((label,), x.shape, (lambda: fa.encode_flac_device(x, level=5, **kw),), dt, args.reps, tree=os.path.abspath(args.tree))
        return

    want = None
    if args.small:  # (the rehearsal also checks what it times)
        import hashlib

        want = np.stack([np.frombuffer(hashlib.md5(r.tobytes()).digest(), np.uint8) for r in x.cpu().numpy()])
        assert np.array_equal(fa.md5_device(x).cpu().numpy(), want)
    _cases(("md5_device int32",), x.shape, (lambda: fa.md5_device(x),), dt, args.reps)
    x16 = x.reshape(rows * 16, n // 16)
    _cases(("md5_device int32, 16x the streams",), x16.shape, (lambda: fa.md5_device(x16),), dt, args.reps)

    _cases(("encode_flac_device(md5=False)", "encode_flac_device(md5=True)"), x.shape,
           (lambda: fa.encode_flac_device(x, level=5, md5=False), lambda: fa.encode_flac_device(x, level=5, md5=True)), dt, args.reps)
    comp, st, nb = fa.encode_flac_device(x, level=5, md5=True, compact=True)
    assert (fa.check_md5_device(comp, st, nb, n) == 1).all()
    _cases(("decode_flac_device", "check_md5_device"), x.shape,
           (lambda: fa.decode_flac_device(comp, st, nb, n), lambda: fa.check_md5_device(comp, st, nb, n)), dt, args.reps)
    del comp, st, nb
    torch.cuda.empty_cache()

    xh = x.cpu().numpy()
    xf = x.to(torch.float32) / 65536.0
    del x, x16
    torch.cuda.empty_cache()
    one = torch.full((rows,), 65536.0, dtype=torch.float32, device=dev)
    zero = torch.zeros(rows, dtype=torch.float32, device=dev)
    if want is not None:
        assert np.array_equal(fa.md5_device(xf, zero, one).cpu().numpy(), want)
    _cases(("md5_device float32 (quantised on load)",), xf.shape, (lambda: fa.md5_device(xf, zero, one),), dt, args.reps)
    del xf
    torch.cuda.empty_cache()

    rows64 = 1024 // div
    x32 = make_data(torch, rows64, n, 5, dev)
    x64 = x32.to(torch.int64) * 8192 + torch.randint(-4096, 4096, x32.shape, device=dev, dtype=torch.int64)
    del x32
    _cases(("md5_device int64",), x64.shape, (lambda: fa.md5_device(x64),), dt, args.reps)
    del x64
    torch.cuda.empty_cache()

    _cases(("array_compress(md5=False)", "array_compress(md5=True)"), xh.shape,
           (lambda: fa.array_compress(xh, level=5, md5=False), lambda: fa.array_compress(xh, level=5, md5=True)), _host_ms, args.reps)


if __name__ == "__main__":
    main()
