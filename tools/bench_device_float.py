"""Time std_device and from_device_array(precision=) against from_device_array(quanta=) on HBM-resident float tensors.

Device events around each call after warm-up; std_device's rate is over 2 x the input bytes (two read passes).  Prints
one JSON line per case.  Usage: python -m tools.bench_device_float [--reps N] [--small]
"""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def _time(fn, reps):
    import torch

    fn()  # warm-up (code objects, scratch, summation plans)
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return float(np.median(ms)), float(np.min(ms))


def main():
    import torch

    import flacarray_amd as fa

    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--small", action="store_true", help="1/64 of the sizes (a rehearsal)")
    args = ap.parse_args()
    cases = [(torch.float32, 4096, 2**20), (torch.float64, 1024, 2**20)]
    for dt, rows, n in cases:
        if args.small:
            rows //= 64
        g = torch.Generator(device="cuda").manual_seed(1)
        x = torch.randn((rows, n), generator=g, device="cuda", dtype=dt)
        in_bytes = x.numel() * x.element_size()
        med, best = _time(lambda: fa.std_device(x), args.reps)
        print(json.dumps({"case": "std_device", "dtype": str(dt), "shape": [rows, n], "ms": round(med, 3), "ms_min": round(best, 3),
                          "GBps": round(2 * in_bytes / (med * 1e6), 1)}), flush=True)
        quanta = (fa.std_device(x).cpu().numpy() / 10**3).astype(np.float32 if dt == torch.float32 else np.float64)
        quanta_t = torch.from_numpy(quanta)
        for label, kw in (("from_device_array(quanta)", {"quanta": quanta_t}), ("from_device_array(precision=3)", {"precision": 3})):
            med, best = _time(lambda: fa.FlacArray.from_device_array(x, **kw), max(2, args.reps // 2))
            print(json.dumps({"case": label, "dtype": str(dt), "shape": [rows, n], "ms": round(med, 3), "ms_min": round(best, 3)}), flush=True)
        del x
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
