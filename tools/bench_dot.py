#!/usr/bin/env python3
"""Projections from the compressed store (DeviceDecodeIndex.dot, K7D) against what they replace, on one MI355X: the bench
workload (bench.make_data, 4096 x 2^20 int32, level 5) and 1024 x 2^20 int64.  Device events around each call, one warm
call first, median of the repeats.

  int32: the bare decode; reduce with one bin; dot with K = 1, 4, 8, 9 and 32 templates of small integers; and what a
         caller does today -- decode in row chunks of 512 streams and torch.matmul in float64 (INEXACT: float64 carries 53
         bits, the products of 2^20 samples do not fit) -- with the peak extra device memory of both ways and the largest
         relative error of the matmul against the exact result
  int64: dot with K = 1 and 8 through column chunks (the default cap, and a cap that holds the whole range) against
         decoding everything and torch.matmul in float64

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
KS = (1, 4, 8, 9, 32)


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
        gen = torch.Generator(device=dev).manual_seed(3)
        templates = lambda K: torch.randint(-1000, 1001, (K, samples), generator=gen, device=dev, dtype=torch.int32)  # noqa: E731

        def exact_f64(out):
            """The exact result rounded once to float64 (on the host: the limbs are combined in Python integers)."""
            ex = fa.dot_exact(out) if wide else fa.dot_exact(*out)
            return np.array([[float(v) for v in r] for r in ex])

        def rel_err(approx, out):
            ref = exact_f64(out)
            return float(np.max(np.abs(approx.cpu().numpy() - ref) / np.maximum(np.abs(ref), 1.0)))

        if wide:
            whole = rows * samples * 8 + (1 << 20)
            for K in (1, 8):
                T = templates(K)
                Tf = T.to(torch.float64).t().contiguous()
                alt = lambda: ix.decode().to(torch.float64) @ Tf  # noqa: E731
                row = dict(what="K = %d" % K, dot_ms=round(timed(torch, np, lambda: ix.dot(T), reps), 3),
                           dot_one_chunk_ms=round(timed(torch, np, lambda: ix.dot(T, max_temp_bytes=whole), reps), 3),
                           decode_then_matmul_ms=round(timed(torch, np, alt, reps), 3))
                row["matmul_max_rel_err"] = rel_err(alt(), ix.dot(T))
                release()
                row["dot_extra_MiB"] = extra_memory(torch, lambda: ix.dot(T))
                release()
                row["decode_then_matmul_extra_MiB"] = extra_memory(torch, alt)
                emit(**row)
            ix.close()
            return
        t_dec = timed(torch, np, lambda: ix.decode(), reps)
        emit(what="decode alone", ms=round(t_dec, 3), store_MB=round(comp.numel() / 1e6, 1))
        t_red = timed(torch, np, lambda: ix.reduce(None), reps)
        emit(what="reduce, one bin", ms=round(t_red, 3), over_decode=round(t_red / t_dec, 3))

        def alternative(Tf):
            """Decode ROW_CHUNK streams at a time and multiply in float64."""
            out = torch.empty((rows, Tf.shape[1]), dtype=torch.float64, device=dev)
            for r0 in range(0, rows, ROW_CHUNK):
                r1 = min(rows, r0 + ROW_CHUNK)
                part = fa.decode_flac_device(comp, st.reshape(-1)[r0:r1].contiguous(), nb.reshape(-1)[r0:r1].contiguous(), samples)
                out[r0:r1] = part.to(torch.float64) @ Tf
                del part
            return out

        for K in KS:
            T = templates(K)
            Tf = T.to(torch.float64).t().contiguous()
            call = lambda: ix.dot(T)  # noqa: E731
            row = dict(what="K = %d" % K, dot_ms=round(timed(torch, np, call, reps), 3))
            row["dot_over_decode"] = round(row["dot_ms"] / t_dec, 3)
            row["dot_over_reduce"] = round(row["dot_ms"] / t_red, 3)
            row["chunked_decode_then_matmul_ms"] = round(timed(torch, np, lambda: alternative(Tf), max(1, reps // 2)), 3)
            row["dot_over_alternative"] = round(row["dot_ms"] / row["chunked_decode_then_matmul_ms"], 3)
            row["matmul_max_rel_err"] = rel_err(alternative(Tf), call())
            release()
            row["dot_extra_MiB"] = extra_memory(torch, call)
            release()
            row["alternative_extra_MiB"] = extra_memory(torch, lambda: alternative(Tf))
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
