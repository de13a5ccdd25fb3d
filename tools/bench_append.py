"""Cost of FlacArray.append's pieces on a resident int32 store of 4096 x 2^20 samples (bench.py's geometry, level 5):
appends of 2^16 and 2^20 samples per stream, the three pieces timed separately with device events --
  tail decode   decode_flac_device of the old short last frame ([base * B, N): nothing when N is a multiple of B)
  encode        encode_flac_device of the (n_stream, r + n) image
  append        append_flac_device, all of it (tail decode + copies + encode + sizes + the splice)
-- so that splice + host waits ~ append - tail decode - encode; the splice kernel alone is what a
`rocprofv3 --kernel-trace --stats` run of this tool reports for splice_kernel (the one kernel append and overwrite
share).  --tail R makes the store N = 2^20 + R samples long (R > 0: a short last frame).  The median and minimum of
--reps runs are printed as one JSON line per case.
Results: profiles/append.md.  Usage: python -m tools.bench_append [--reps N] [--streams S] [--tail R]
"""
import argparse
import json
import os
import sys

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


def _signal(torch, n_stream, n, seed):
    """Sinusoid + small noise, generated on the device: ~0.6 B/sample at level 5 (bench.py's data compresses to 2.29)."""
    g = torch.Generator(device="cuda").manual_seed(seed)
    t = torch.arange(n, device="cuda", dtype=torch.float32)
    amp = torch.rand((n_stream, 1), device="cuda", generator=g) * 2**16
    x = amp * torch.sin(2 * np.pi * t / 4000.0) + torch.randn((n_stream, n), device="cuda", generator=g) * 4.0
    return torch.round(x).to(torch.int32)


def main():
    import torch

    import flacarray_amd as fa

    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--streams", type=int, default=4096)
    ap.add_argument("--tail", type=int, default=0)
    args = ap.parse_args()
    S, N, level, B = args.streams, 2**20 + args.tail, 5, 4096
    base, r = divmod(N, B)
    x = _signal(torch, S, N, 1)
    comp, st, nb = fa.encode_flac_device(x, level=level, compact=True)
    del x
    torch.cuda.synchronize()
    old_bytes = comp.numel()
    for n in (2**16, 2**20):
        new = _signal(torch, S, n, 2)
        tail = fa.decode_flac_device(comp, st, nb, N, base * B, N) if r else None
        image = torch.cat([tail, new], dim=1).contiguous() if r else new
        holder = []
        res = {"tail_decode": [], "encode": [], "append": []}
        # (no empty_cache between reps: after the warm-up round the caching allocator serves the multi-GB buffers, so
        # no hipMalloc lands inside the timed calls)
        for rep in range(args.reps + 1):
            tdec = _device_ms(torch, lambda: fa.decode_flac_device(comp, st, nb, N, base * B, N)) if r else 0.0
            tenc = _device_ms(torch, lambda: fa.encode_flac_device(image, level=level, compact=True))
            holder.clear()
            tapp = _device_ms(torch, lambda: holder.append(fa.append_flac_device(comp, st, nb, N, new, level=level)))
            if rep:  # (the first round warms up)
                res["tail_decode"].append(tdec)
                res["encode"].append(tenc)
                res["append"].append(tapp)
        total = int(holder[0][0].numel())
        line = {"case": f"append {S} x {n} to {S} x {N} int32 level {level}", "old_bytes": old_bytes, "new_bytes": total,
                "r": r}
        for k, v in res.items():
            line[k + "_ms_median"] = round(float(np.median(v)), 3)
            line[k + "_ms_min"] = round(float(np.min(v)), 3)
        line["append_minus_parts_ms"] = round(line["append_ms_median"] - line["tail_decode_ms_median"] - line["encode_ms_median"], 3)
        print(json.dumps(line), flush=True)
        del new, image, tail, holder
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
