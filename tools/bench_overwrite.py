"""Cost of FlacArray.overwrite's pieces on a resident int32 store of 4096 x 2^20 samples (bench.py's geometry, level 5):
overwrites of 2^12 and 2^16 samples at mid-stream (first = 2^19 + 100: inside a frame, so the span is decoded), for all
streams and for 64 of them, the pieces timed separately with device events --
  span decode   decode_flac_device of the frames that overlap the range, of the participating streams
  encode        encode_flac_device of the (m, span) image
  overwrite     overwrite_flac_device, all of it (check + span decode + copy + encode + sizes + the splice)
-- so that splice + host waits ~ overwrite - span decode - encode; the splice kernel alone is what a
`rocprofv3 --kernel-trace --stats` run of this tool reports for splice_kernel (the one kernel append and overwrite
share).  Two baselines on the same store in the same run: append_flac_device of the same n (all streams), and what a
user must do without overwrite: decode the whole array and encode_flac_device all of it (--no-full skips it).  The
median and minimum of --reps runs after a warm-up round are printed as one JSON line per case.  Results:
profiles/overwrite.md.
Usage: python -m tools.bench_overwrite [--reps N] [--streams S] [--subset M] [--no-full]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tools.bench_append import _device_ms, _signal  # noqa: E402


def _stats(line, res):
    for k, v in res.items():
        line[k + "_ms_median"] = round(float(np.median(v)), 3)
        line[k + "_ms_min"] = round(float(np.min(v)), 3)
    return line


def main():
    import torch

    import flacarray_amd as fa

    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--streams", type=int, default=4096)
    ap.add_argument("--subset", type=int, default=64)
    ap.add_argument("--no-full", action="store_true")
    args = ap.parse_args()
    S, N, level, B = args.streams, 2**20, 5, 4096
    x = _signal(torch, S, N, 1)
    comp, st, nb = fa.encode_flac_device(x, level=level, compact=True)
    del x
    torch.cuda.synchronize()
    old_bytes = comp.numel()
    first = N // 2 + 100
    subset = torch.arange(0, S, max(1, S // args.subset), device="cuda")[: args.subset]
    for n in (2**12, 2**16):
        lo, hi = first // B * B, min(-(-(first + n) // B) * B, N)
        for idx in (None, subset):
            m = S if idx is None else int(idx.numel())
            new = _signal(torch, m, n, 2)
            sst, snb = (st, nb) if idx is None else (st[idx].contiguous(), nb[idx].contiguous())
            image = fa.decode_flac_device(comp, sst, snb, N, lo, hi).reshape(m, -1).clone()
            image[:, first - lo : first - lo + n] = new
            holder = []
            res = {"span_decode": [], "encode": [], "overwrite": []}
            for rep in range(args.reps + 1):
                tdec = _device_ms(torch, lambda: fa.decode_flac_device(comp, sst, snb, N, lo, hi))
                tenc = _device_ms(torch, lambda: fa.encode_flac_device(image, level=level, compact=True))
                holder.clear()
                tow = _device_ms(torch, lambda: holder.append(fa.overwrite_flac_device(comp, st, nb, N, first, new, streams=idx, level=level)))
                if rep:  # (the first round warms up)
                    res["span_decode"].append(tdec)
                    res["encode"].append(tenc)
                    res["overwrite"].append(tow)
            line = {"case": f"overwrite {m} of {S} streams x [{first}, {first + n}) of {N} int32 level {level}", "old_bytes": old_bytes,
                    "new_bytes": int(holder[0][0].numel()), "span": hi - lo}
            _stats(line, res)
            line["overwrite_minus_parts_ms"] = round(line["overwrite_ms_median"] - line["span_decode_ms_median"] - line["encode_ms_median"], 3)
            print(json.dumps(line), flush=True)
            del new, image, holder
        # baseline 1: an append of the same n to every stream
        new = _signal(torch, S, n, 2)
        holder, res = [], {"append": []}
        for rep in range(args.reps + 1):
            holder.clear()
            t = _device_ms(torch, lambda: holder.append(fa.append_flac_device(comp, st, nb, N, new, level=level)))
            if rep:
                res["append"].append(t)
        print(json.dumps(_stats({"case": f"append {S} x {n} to {S} x {N} int32 level {level}", "old_bytes": old_bytes,
                                 "new_bytes": int(holder[0][0].numel())}, res)), flush=True)
        del new, holder
        torch.cuda.empty_cache()
    if not args.no_full:
        # baseline 2: decode everything and encode everything again (the patch itself, a copy of n samples, is not timed)
        res = {"full_decode": [], "full_encode": []}
        for rep in range(args.reps + 1):
            out = []
            tdec = _device_ms(torch, lambda: out.append(fa.decode_flac_device(comp, st, nb, N)))
            whole = out[0].reshape(S, N)
            tenc = _device_ms(torch, lambda: fa.encode_flac_device(whole, level=level, compact=True))
            if rep:
                res["full_decode"].append(tdec)
                res["full_encode"].append(tenc)
            del out, whole
        line = _stats({"case": f"decode + encode all of {S} x {N} int32 level {level}", "old_bytes": old_bytes}, res)
        line["full_ms_median"] = round(line["full_decode_ms_median"] + line["full_encode_ms_median"], 3)
        print(json.dumps(line), flush=True)


if __name__ == "__main__":
    main()
