#!/usr/bin/env python3
"""The damage map and the salvage decode on one MI355X, on the bench workload (bench.make_data, 4096 x 2^20 int32, level 5)
and on 1024 x 2^20 int64, beside what they are measured against in the same process: the unverified decode, and the frame
CRC-16 check K9 alone (a verified decode with the check queued after K7, FLACARRAY_HIP_VERIFY_AFTER=1, minus the unverified
one).  Device events around each call, one warm call first, median of the repeats.  Per workload one JSON line:
  status_ms            frame_status_device over the whole store
  k9_ms                verify_crc16_kernel alone, as above; status_over_k9 = status_ms / k9_ms (expected <= 1.25)
  decode_ms            decode_flac_device(verify=False)
  salvage_intact_ms    decode_flac_salvage_device of the intact store; salvage_over_sum = / (decode_ms + status_ms)
                       (expected <= 1.10)
  salvage_damaged_ms   the same with one damaged frame per stream (the last byte of every stream: list mode + fill)"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

import bench
import flacarray_amd as fa


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


def run(name, make, reps, wide):
    x = make()
    comp, st, nb = fa.encode_flac_device(x, level=5, compact=True)[:3]
    n = x.shape[1]
    del x
    torch.cuda.empty_cache()
    st, nb = st.reshape(-1), nb.reshape(-1)
    block = 4096
    row = {"case": name, "store_MB": round(comp.numel() / 1e6, 1), "frames": int(st.numel() * -(-n // block))}
    status = fa.frame_status_device(comp, st, nb, n, is_int64=wide, block_size=block)
    row["intact_status_all_zero"] = not bool(status.any())
    row["status_ms"] = round(timed(lambda: fa.frame_status_device(comp, st, nb, n, is_int64=wide, block_size=block), reps), 3)
    row["decode_ms"] = round(timed(lambda: fa.decode_flac_device(comp, st, nb, n, is_int64=wide, verify=False), reps), 3)
    os.environ["FLACARRAY_HIP_VERIFY_AFTER"] = "1"
    after = timed(lambda: fa.decode_flac_device(comp, st, nb, n, is_int64=wide, verify=True), reps)
    del os.environ["FLACARRAY_HIP_VERIFY_AFTER"]
    row["decode_then_k9_ms"] = round(after, 3)
    row["k9_ms"] = round(after - row["decode_ms"], 3)
    row["status_over_k9"] = round(row["status_ms"] / max(row["k9_ms"], 1e-9), 3)
    row["salvage_intact_ms"] = round(timed(lambda: fa.decode_flac_salvage_device(comp, st, nb, n, is_int64=wide, block_size=block), reps), 3)
    row["salvage_over_sum"] = round(row["salvage_intact_ms"] / (row["decode_ms"] + row["status_ms"]), 3)
    bad = comp.clone()
    bad[st + nb - 1] ^= 1  # the second footer byte of every stream's last frame
    out, status = fa.decode_flac_salvage_device(bad, st, nb, n, is_int64=wide, block_size=block)
    row["damaged_frames"] = int((status != 0).sum())
    row["damaged_frames_are_the_last"] = bool((status[:, -1] == fa.FRAME_CRC16).all()) and not bool(status[:, :-1].any())
    del out
    row["salvage_damaged_ms"] = round(timed(lambda: fa.decode_flac_salvage_device(bad, st, nb, n, is_int64=wide, block_size=block), reps), 3)
    print(json.dumps(row), flush=True)


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
            run("int32 (%d, %d) level 5" % (args.channels, args.samples), lambda: bench.make_data(torch, args.channels, args.samples, 5, dev),
                args.reps, False)
        if args.only != "int32":
            c64 = max(1, args.channels // 4)

            def make64():
                big = bench.make_data(torch, c64, args.samples, 5, dev)
                return big.to(torch.int64) * 8192 + torch.randint(-4096, 4096, big.shape, device=dev, dtype=torch.int64)

            run("int64 (%d, %d) level 5" % (c64, args.samples), make64, args.reps, True)


if __name__ == "__main__":
    main()
