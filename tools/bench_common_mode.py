#!/usr/bin/env python3
"""The fold across streams from the compressed store (DeviceDecodeIndex.common_mode, K7X) against what it replaces, on one
MI355X: the bench workload (bench.make_data, 4096 x 2^20 int32, level 5) and 1024 x 2^20 int64.  Device events around
each call, one warm call first, median of the repeats.

  int32: the bare decode; common_mode with one group, with 64 groups of 64 streams, and with squares=False; and the caller's
         alternative -- decode in row chunks of 512 streams and accumulate torch.sum(dim=0, dtype=int64) per group -- with
         the peak extra device memory of both ways
  int64: common_mode (column chunks under the default cap, and under a cap that holds the whole range) against decoding
         everything and torch.sum(dim=0)

Without --case this process starts one child per case, each under its own time limit, and stops at the first that fails
or runs out of time: it never touches the GPU itself.  One JSON line per measurement."""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
CASES = {"int32": 420, "int64": 420}  # seconds allowed per case
ROW_CHUNK = 512


def timed(torch, np, fn, reps):
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


def extra_memory(torch, fn):
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


def run_case(case, channels, samples, reps):
    import numpy as np
    import torch

    import bench
    import flacarray_amd as fa

    dev = torch.device("cuda", 0)
    wide = case == "int64"
    rows = max(1, channels // 4) if wide else channels
    with torch.cuda.device(dev):
        x = bench.make_data(torch, rows, samples, 5, dev)
        if wide:
            x = x.to(torch.int64) * 8192 + torch.randint(-4096, 4096, x.shape, device=dev, dtype=torch.int64)
        comp, st, nb = fa.encode_flac_device(x, level=5, compact=True)[:3]
        del x  # (the input is not part of either way: only the store stays resident)
        torch.cuda.empty_cache()
        ix = fa.DeviceDecodeIndex(comp, st.reshape(-1), nb.reshape(-1), samples, is_int64=wide)
        name = "%s (%d, %d) level 5" % (case, rows, samples)
        release = fa._lib.lib().fa_release_scratch
        emit = lambda **kw: print(json.dumps(dict(case=name, **kw)), flush=True)  # noqa: E731
        if wide:
            t_xs = timed(torch, np, lambda: ix.common_mode(), reps)
            whole = rows * samples * 8 + (1 << 20)
            t_one = timed(torch, np, lambda: ix.common_mode(max_temp_bytes=whole), reps)
            t_alt = timed(torch, np, lambda: ix.decode().sum(dim=0, dtype=torch.int64), reps)
            equal = bool(torch.equal(ix.common_mode()[0][0], ix.decode().sum(dim=0, dtype=torch.int64)))
            release()
            m_xs = extra_memory(torch, lambda: ix.common_mode())
            release()
            m_alt = extra_memory(torch, lambda: ix.decode().sum(dim=0, dtype=torch.int64))
            emit(what="one group", common_mode_ms=round(t_xs, 3), common_mode_one_chunk_ms=round(t_one, 3), decode_then_torch_ms=round(t_alt, 3),
                 equal=equal, common_mode_extra_MiB=m_xs, decode_then_torch_extra_MiB=m_alt)
            ix.close()
            return
        t_dec = timed(torch, np, lambda: ix.decode(), reps)
        emit(what="decode alone", ms=round(t_dec, 3), store_MB=round(comp.numel() / 1e6, 1))
        lab64 = (np.arange(rows) // 64).astype(np.int64)  # 64 groups of 64 at 4096 streams

        def alternative(labels, G):
            """Decode ROW_CHUNK streams at a time and accumulate the per-group column sums."""
            out = torch.zeros((G, samples), dtype=torch.int64, device=dev)
            for r0 in range(0, rows, ROW_CHUNK):
                r1 = min(rows, r0 + ROW_CHUNK)
                part = fa.decode_flac_device(comp, st.reshape(-1)[r0:r1].contiguous(), nb.reshape(-1)[r0:r1].contiguous(), samples)
                if labels is None:
                    out[0] += part.sum(dim=0, dtype=torch.int64)
                else:
                    for g in np.unique(labels[r0:r1]):
                        sel = torch.from_numpy(np.flatnonzero(labels[r0:r1] == g)).to(dev)
                        out[g] += part[sel].sum(dim=0, dtype=torch.int64)
                del part
            return out

        for what, labels, G, squares in (("one group", None, 1, True), ("64 groups of 64", lab64, int(lab64.max()) + 1, True),
                                         ("one group, squares=False", None, 1, False)):
            call = lambda: ix.common_mode(groups=labels, n_groups=G, squares=squares)  # noqa: E731
            row = dict(what=what, common_mode_ms=round(timed(torch, np, call, reps), 3))
            row["common_mode_over_decode"] = round(row["common_mode_ms"] / t_dec, 3)
            if squares:
                row["chunked_decode_then_torch_ms"] = round(timed(torch, np, lambda: alternative(labels, G), max(1, reps // 2)), 3)
                row["common_mode_over_alternative"] = round(row["common_mode_ms"] / row["chunked_decode_then_torch_ms"], 3)
                row["equal"] = bool(torch.equal(call()[0], alternative(labels, G)))
                release()
                row["common_mode_extra_MiB"] = extra_memory(torch, call)
                release()
                row["alternative_extra_MiB"] = extra_memory(torch, lambda: alternative(labels, G))
            emit(**row)
        ix.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--channels", type=int, default=4096)
    ap.add_argument("--samples", type=int, default=1 << 20)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--only", choices=sorted(CASES), default=None)
    ap.add_argument("--case", choices=sorted(CASES), default=None, help="run this case in this process (what the parent starts)")
    args = ap.parse_args()
    if args.case:
        run_case(args.case, args.channels, args.samples, args.reps)
        return 0
    for case, limit in CASES.items():
        if args.only and case != args.only:
            continue
        cmd = [sys.executable, os.path.abspath(__file__), "--case", case, "--channels", str(args.channels), "--samples", str(args.samples),
               "--reps", str(args.reps)]
        try:
            rc = subprocess.run(cmd, timeout=limit).returncode
        except subprocess.TimeoutExpired:
            print(json.dumps({"case": case, "error": "no result within %d s" % limit}), flush=True)
            return 124
        if rc != 0:  # nothing more is started on the GPU after a failure
            print(json.dumps({"case": case, "error": "exit status %d" % rc}), flush=True)
            return rc
    return 0


if __name__ == "__main__":
    sys.exit(main())
