#!/usr/bin/env python3
"""The search (FlacArray.find / DeviceDecodeIndex.find) against what it replaces, on one MI355X: the bench workload
(bench.make_data, 4096 x 2^20 int32, level 5) and 1024 x 2^20 int64, both resident.  Device events around each call, one
warm call first, median of the repeats; peak extra device memory as tools/bench_reduce.py takes it.  Measured, per store,
in one run:

  decode alone, and reduce with one bin (the two yardsticks on the same build);
  the count pass alone (find_counts) at limits that about 10^-6 of the samples exceed;
  the full search at about 10^-6, 10^-3 and 1 hits per sample (the last: lo > hi, every sample a hit);
  what a caller does today: decode row chunks of --chunk-rows into a second array, form the mask and torch.nonzero it.

The limits come from per-row order statistics of the store itself (FlacArray.order_statistic), so that the hit rates are
what the labels say.  One JSON line per measurement."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

import bench
import flacarray_amd as fa
from tools.bench_reduce import extra_memory, timed


def torch_find(ix, lo, hi, chunk_rows):
    """Decode row chunks, mask and nonzero each: (rows [total], positions [total]); lo / hi int64 device tensors [rows]."""
    rows, n = ix.n_stream, ix.stream_size
    out_r, out_p = [], []
    for r0 in range(0, rows, chunk_rows):
        r1 = min(rows, r0 + chunk_rows)
        sel = np.arange(r0, r1)
        if r1 - r0 == rows:
            x = ix.decode()
        else:
            flat, _ = ix.decode_slices(sel, np.zeros(sel.size, np.int64), np.full(sel.size, n, np.int64))
            x = flat.reshape(sel.size, n)
        m = (x < lo[r0:r1, None]) | (x > hi[r0:r1, None])
        nz = torch.nonzero(m)
        out_r.append(nz[:, 0] + r0)
        out_p.append(nz[:, 1])
        del x, m, nz
    return torch.cat(out_r), torch.cat(out_p)


def run(name, make, reps, chunk_rows, rates):
    x = make()
    arr = fa.FlacArray.from_device_array(x, level=5)
    n = x.shape[1]
    del x
    torch.cuda.empty_cache()
    ix = arr._index()
    dev = ix.device
    rows = ix.n_stream
    emit = lambda **kw: print(json.dumps(dict(case=name, **kw)), flush=True)  # noqa: E731
    release = fa._lib.lib().fa_release_scratch
    t_dec = timed(lambda: ix.decode(), reps)
    emit(what="decode alone", ms=round(t_dec, 3), store_MB=round(ix.compressed.numel() / 1e6, 1))
    t_red = timed(lambda: ix.reduce(None), reps)
    emit(what="reduce, one bin", ms=round(t_red, 3))
    for rate in rates:
        if rate >= 1.0:
            lo_h, hi_h = np.full(rows, 1, np.int64), np.full(rows, 0, np.int64)  # lo > hi: every sample
        else:
            k = max(1, int(round(rate * n / 2)))  # that many samples under lo and over hi in every row
            q = arr.order_statistic([k, n - 1 - k]).astype(np.int64)
            lo_h, hi_h = q[:, 0], q[:, 1]
        lo_d, hi_d = torch.from_numpy(lo_h).to(dev), torch.from_numpy(hi_h).to(dev)
        row = dict(what="find", hits_per_sample=rate)
        counts = ix.find_counts(lo_h, hi_h)
        row["hits"] = int(counts.sum())
        row["count_pass_ms"] = round(timed(lambda: ix.find_counts(lo_h, hi_h), reps), 3)
        row["find_ms"] = round(timed(lambda: ix.find(lo_h, hi_h), reps), 3)
        row["find_no_values_ms"] = round(timed(lambda: ix.find(lo_h, hi_h, values=False), reps), 3)
        release()
        row["find_extra_MiB"] = extra_memory(lambda: ix.find(lo_h, hi_h))
        if rate < 1.0:
            row["decode_then_torch_ms"] = round(timed(lambda: torch_find(ix, lo_d, hi_d, chunk_rows), max(1, reps // 2)), 3)
            c, p, _ = ix.find(lo_h, hi_h, values=False)
            tr, tp = torch_find(ix, lo_d, hi_d, chunk_rows)
            row["equal"] = bool(torch.equal(p, tp) and torch.equal(torch.repeat_interleave(torch.arange(rows, device=dev), c), tr))
            del c, p, tr, tp
            release()
            row["decode_then_torch_extra_MiB"] = extra_memory(lambda: torch_find(ix, lo_d, hi_d, chunk_rows))
        else:
            # (every sample a hit: nonzero of a full mask of one row chunk alone is 16 bytes per sample)
            small = max(1, chunk_rows // 8)
            row["decode_then_torch_ms"] = round(timed(lambda: torch_find(ix, lo_d, hi_d, small), 1), 3)
            row["decode_then_torch_chunk_rows"] = small
            release()
            row["decode_then_torch_extra_MiB"] = extra_memory(lambda: torch_find(ix, lo_d, hi_d, small))
        row["count_over_reduce"] = round(row["count_pass_ms"] / t_red, 3)
        row["count_over_decode"] = round(row["count_pass_ms"] / t_dec, 3)
        emit(**row)
        release()
        torch.cuda.empty_cache()
    arr.release_device()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--channels", type=int, default=4096)
    ap.add_argument("--samples", type=int, default=1 << 20)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--chunk-rows", type=int, default=512, help="rows the decode-then-torch way decodes at a time")
    ap.add_argument("--rates", type=float, nargs="*", default=[1e-6, 1e-3, 1.0])
    ap.add_argument("--only", choices=["int32", "int64"], default=None)
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    with torch.cuda.device(dev):
        if args.only != "int64":
            run("int32 (%d, %d) level 5" % (args.channels, args.samples), lambda: bench.make_data(torch, args.channels, args.samples, 5, dev),
                args.reps, args.chunk_rows, args.rates)
        if args.only != "int32":
            c64 = max(1, args.channels // 4)

            def make64():
                big = bench.make_data(torch, c64, args.samples, 5, dev)
                return big.to(torch.int64) * 8192 + torch.randint(-4096, 4096, big.shape, device=dev, dtype=torch.int64)

            run("int64 (%d, %d) level 5" % (c64, args.samples), make64, args.reps, min(args.chunk_rows, c64), args.rates)


if __name__ == "__main__":
    main()
