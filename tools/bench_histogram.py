#!/usr/bin/env python3
"""Value histograms and exact order statistics from the compressed store (FlacArray.histogram / order_statistic /
median) against what they replace, on one MI355X: the bench workload (bench.make_data, 4096 x 2^20 int32, level 5) and
1024 x 2^20 int64, both resident.  Device events around each call, one warm call first, median of the repeats; peak
extra device memory as tools/bench_reduce.py takes it.  Measured, per store:

  decode alone, and reduce with one bin (the two yardsticks on the same build);
  histogram at 64, 256 and 2048 bins with automatic ranges (the reduce pass for the ranges included), and the bare
    histogram pass at the same ranges;
  histogram with all samples in one bin -- the worst case for same-address LDS adds;
  order_statistic for one rank and for three, and median;
  what a caller does today: decode into a second array -- in row chunks of --chunk-rows when that is asked for -- and
    bucket it with ((x - lo) >> shift) and scatter_add, or torch.kthvalue / torch.sort for the quantiles.

One JSON line per measurement."""
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


def torch_histogram(ix, lo, shift, nbins, chunk_rows):
    """Decode row chunks and bucket each with scatter_add: (counts [rows, nbins]); lo / shift int64 device tensors [rows]."""
    rows = ix.n_stream
    counts = torch.zeros((rows, nbins), dtype=torch.int64, device=lo.device)
    n = ix.stream_size
    for r0 in range(0, rows, chunk_rows):
        r1 = min(rows, r0 + chunk_rows)
        sel = np.arange(r0, r1)
        if r1 - r0 == rows:
            x = ix.decode()
        else:
            flat, _ = ix.decode_slices(sel, np.zeros(sel.size, np.int64), np.full(sel.size, n, np.int64))
            x = flat.reshape(sel.size, n)
        b = (x.to(torch.int64) - lo[r0:r1, None]) >> shift[r0:r1, None]
        b.clamp_(0, nbins - 1)  # (automatic ranges: nothing falls outside)
        counts[r0:r1].scatter_add_(1, b, torch.ones_like(b))
        del x, b
    return counts


def torch_ranks(ix, ranks, chunk_rows, how):
    rows, n = ix.n_stream, ix.stream_size
    out = []
    for r0 in range(0, rows, chunk_rows):
        sel = np.arange(r0, min(rows, r0 + chunk_rows))
        if sel.size == rows:
            x = ix.decode()
        else:
            flat, _ = ix.decode_slices(sel, np.zeros(sel.size, np.int64), np.full(sel.size, n, np.int64))
            x = flat.reshape(sel.size, n)
        if how == "sort":
            s = torch.sort(x, dim=1).values
            out.append(s[:, ranks].clone())
            del s
        else:
            out.append(torch.stack([torch.kthvalue(x, k + 1, dim=1).values for k in ranks], dim=1))
        del x
    return torch.cat(out)


def run(name, make, reps, wide, chunk_rows):
    x = make()
    arr = fa.FlacArray.from_device_array(x, level=5)
    n = x.shape[1]
    del x
    torch.cuda.empty_cache()
    ix = arr._index()
    dev = ix.device
    emit = lambda **kw: print(json.dumps(dict(case=name, **kw)), flush=True)  # noqa: E731
    release = fa._lib.lib().fa_release_scratch
    t_dec = timed(lambda: ix.decode(), reps)
    emit(what="decode alone", ms=round(t_dec, 3), store_MB=round(ix.compressed.numel() / 1e6, 1))
    emit(what="reduce, one bin", ms=round(timed(lambda: ix.reduce(None), reps), 3))
    mn, mx = (t.cpu().numpy().reshape(-1) for t in ix.reduce(None)[:2])
    for bins in (64, 256, 2048):
        from flacarray_amd.array import _auto_shift

        lo_h, sh_h = mn.astype(np.int64), _auto_shift(mn, mx, bins)
        lo_d, sh_d = torch.from_numpy(lo_h).to(dev), torch.from_numpy(sh_h.astype(np.int64)).to(dev)
        row = dict(what="histogram", bins=bins)
        row["histogram_auto_ms"] = round(timed(lambda: arr.histogram(bins=bins), reps), 3)
        row["histogram_pass_ms"] = round(timed(lambda: ix.histogram(lo_h, sh_h, bins), reps), 3)
        row["decode_then_torch_ms"] = round(timed(lambda: torch_histogram(ix, lo_d, sh_d, bins, chunk_rows), max(1, reps // 2)), 3)
        a = ix.histogram(lo_h, sh_h, bins)[0]
        row["equal"] = bool(torch.equal(a, torch_histogram(ix, lo_d, sh_d, bins, chunk_rows)))
        del a
        release()
        row["histogram_extra_MiB"] = extra_memory(lambda: ix.histogram(lo_h, sh_h, bins))
        release()
        row["decode_then_torch_extra_MiB"] = extra_memory(lambda: torch_histogram(ix, lo_d, sh_d, bins, chunk_rows))
        row["pass_over_decode"] = round(row["histogram_pass_ms"] / t_dec, 3)
        emit(**row)
    lo1 = -(1 << 62) if wide else -(1 << 31)  # (with shift 63: every sample in bin 0)
    emit(what="histogram, all samples in one bin", bins=2048, ms=round(timed(lambda: ix.histogram(lo1, 63, 2048), reps), 3))
    for label, ranks in (("one rank", [n // 2]), ("three ranks", [n // 4, n // 2, 3 * n // 4])):
        row = dict(what="order_statistic, " + label)
        row["order_statistic_ms"] = round(timed(lambda: arr.order_statistic(ranks), reps), 3)
        for how in ("kthvalue", "sort"):
            row["decode_then_%s_ms" % how] = round(timed(lambda: torch_ranks(ix, ranks, chunk_rows, how), max(1, reps // 2)), 3)
        got = arr.order_statistic(ranks)
        row["equal"] = bool(np.array_equal(got, torch_ranks(ix, ranks, chunk_rows, "sort").cpu().numpy()))
        release()
        row["order_statistic_extra_MiB"] = extra_memory(lambda: arr.order_statistic(ranks))
        release()
        row["decode_then_sort_extra_MiB"] = extra_memory(lambda: torch_ranks(ix, ranks, chunk_rows, "sort"))
        release()
        row["decode_then_kthvalue_extra_MiB"] = extra_memory(lambda: torch_ranks(ix, ranks, chunk_rows, "kthvalue"))
        emit(**row)
    emit(what="median", ms=round(timed(lambda: arr.median(), reps), 3))
    arr.release_device()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--channels", type=int, default=4096)
    ap.add_argument("--samples", type=int, default=1 << 20)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--chunk-rows", type=int, default=512, help="rows the decode-then-torch way decodes at a time")
    ap.add_argument("--only", choices=["int32", "int64"], default=None)
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    with torch.cuda.device(dev):
        if args.only != "int64":
            run("int32 (%d, %d) level 5" % (args.channels, args.samples), lambda: bench.make_data(torch, args.channels, args.samples, 5, dev),
                args.reps, False, args.chunk_rows)
        if args.only != "int32":
            c64 = max(1, args.channels // 4)

            def make64():
                big = bench.make_data(torch, c64, args.samples, 5, dev)
                return big.to(torch.int64) * 8192 + torch.randint(-4096, 4096, big.shape, device=dev, dtype=torch.int64)

            run("int64 (%d, %d) level 5" % (c64, args.samples), make64, args.reps, True, min(args.chunk_rows, c64))


if __name__ == "__main__":
    main()
