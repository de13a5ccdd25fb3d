#!/usr/bin/env python3
"""Binned reduction from the compressed store (DeviceDecodeIndex.reduce) against what it replaces -- a full decode into a
second array and amin / amax / sum over the reshaped tensor -- on one MI355X, on the bench workload (bench.make_data,
4096 x 2^20 int32, level 5) and on 1024 x 2^20 int64.  Device events around each call, one warm call first, median of
the repeats.  Per width: reduce (for int64 also with a temp-byte cap that holds the whole decoded range in one chunk), the
decode alone and decode + torch; and the peak extra device memory of both ways (torch's allocator peak plus what the
library's scratch grew by).  One JSON line per measurement."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

import bench
import flacarray_amd as fa

WIDTHS = (None, 4096, 1024, 1000, 64, 8)


def timed(fn, reps):
    fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        out = fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
        del out
    return float(np.median(ms))


def extra_memory(fn):
    """Peak device memory one call needs beyond what is resident: torch's allocator peak over the call plus the growth
    of everything else on the device (the library's cached scratch), in MiB."""
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    free0 = torch.cuda.mem_get_info()[0]
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    out = fn()
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - base
    del out
    torch.cuda.empty_cache()
    other = max(0, free0 - torch.cuda.mem_get_info()[0])
    return round((peak + other) / 2**20, 1)


def torch_stats(x, width):
    """amin / amax / sum per bin of a decoded tensor [rows, n], the way a user of torch writes it: the whole bins as a
    view of shape (rows, nbins, width), a short last bin on its own."""
    n = x.shape[1]
    w = n if width is None else width
    k = n // w
    v = x[:, : k * w].reshape(x.shape[0], k, w)
    out = [v.amin(dim=-1), v.amax(dim=-1), v.sum(dim=-1, dtype=torch.int64)]
    if k * w < n:
        t = x[:, k * w :]
        out = [torch.cat([o, p.reshape(-1, 1)], dim=1) for o, p in zip(out, (t.amin(dim=-1), t.amax(dim=-1), t.sum(dim=-1, dtype=torch.int64)))]
    return out


def run(name, make, level, reps, wide):
    x = make()
    comp, st, nb = fa.encode_flac_device(x, level=level, compact=True)[:3]
    n = x.shape[1]
    del x  # (the input is not part of either way: only the store stays resident)
    torch.cuda.empty_cache()
    ix = fa.DeviceDecodeIndex(comp, st.reshape(-1), nb.reshape(-1), n, is_int64=wide)
    t_dec = timed(lambda: ix.decode(), reps)
    print(json.dumps({"case": name, "what": "decode alone", "ms": round(t_dec, 3), "store_MB": round(comp.numel() / 1e6, 1)}), flush=True)
    for width in WIDTHS:
        row = {"case": name, "width": width}
        row["decode_then_torch_ms"] = round(timed(lambda: torch_stats(ix.decode(), width), reps), 3)
        row["reduce_ms"] = round(timed(lambda: ix.reduce(width), reps), 3)
        # the two ways agree (min / max / sum)
        a = ix.reduce(width)
        b = torch_stats(ix.decode(), width)
        row["equal"] = bool(all(torch.equal(p, q.to(torch.int64)) for p, q in zip(a[:3], b)))
        del a, b
        fa._lib.lib().fa_release_scratch()
        row["reduce_extra_MiB"] = extra_memory(lambda: ix.reduce(width))
        fa._lib.lib().fa_release_scratch()
        row["decode_then_torch_extra_MiB"] = extra_memory(lambda: torch_stats(ix.decode(), width))
        row["reduce_over_decode_then_torch"] = round(row["reduce_ms"] / row["decode_then_torch_ms"], 3)
        row["reduce_over_decode"] = round(row["reduce_ms"] / t_dec, 3)
        if wide:  # one chunk: the whole decoded range as the temporary
            whole = ix.n_stream * n * 8 + (1 << 20)
            row["reduce_one_chunk_ms"] = round(timed(lambda: ix.reduce(width, max_temp_bytes=whole), reps), 3)
            fa._lib.lib().fa_release_scratch()
            row["reduce_one_chunk_extra_MiB"] = extra_memory(lambda: ix.reduce(width, max_temp_bytes=whole))
            fa._lib.lib().fa_release_scratch()
        print(json.dumps(row), flush=True)
    ix.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--channels", type=int, default=4096)
    ap.add_argument("--samples", type=int, default=1 << 20)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--only", choices=["int32", "int64"], default=None)
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    with torch.cuda.device(dev):
        if args.only != "int64":
            run("int32 (%d, %d) level 5" % (args.channels, args.samples), lambda: bench.make_data(torch, args.channels, args.samples, 5, dev), 5,
                args.reps, False)
        if args.only != "int32":
            c64 = max(1, args.channels // 4)

            def make64():
                big = bench.make_data(torch, c64, args.samples, 5, dev)
                return big.to(torch.int64) * 8192 + torch.randint(-4096, 4096, big.shape, device=dev, dtype=torch.int64)

            run("int64 (%d, %d) level 5" % (c64, args.samples), make64, 5, args.reps, True)


if __name__ == "__main__":
    main()
