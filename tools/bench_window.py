"""Cost of FlacArray.window / trim on a resident int32 store of 4096 x 2^20 samples (bench.py's geometry, level 5), next to
two yardsticks measured in the same run on the same store:
  clone        `clone()` of the bytes kept: the floor for anything that copies the result once
  dec + enc    what a user has to do without window: decode_flac_device of the window of the picked streams plus
               encode_flac_device of it, with its peak extra device memory (the decoded copy and the encode's buffers)
Four cases:
  a  drop the first 64 frames                          window(64 B, N)
  b  the same with `last` inside a frame               window(64 B, N - 1000): one frame per stream decoded and re-encoded
  c  pure selection of every second stream             window(0, N, streams=0, 2, 4, ...)
  d  first = 1 (unaligned: every frame changes)        window(1, N): decode + encode in row chunks of 256 MiB
Device events around each call, the median and minimum of --reps runs after a warm-up round (the caching allocator
serves every buffer after that round); peak extra memory from torch.cuda.max_memory_allocated over one call.  These are
window_flac_device times: FlacArray.window adds the PCIe copy of the new blob to its host mirror.  One JSON line per
case on stdout, and the table of profiles/window.md written to --out.
Usage: python -m tools.bench_window [--reps N] [--streams S] [--out PATH]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tools.bench_append import _device_ms, _signal  # noqa: E402


def _timed(torch, fn, reps):
    """(median ms, min ms, peak extra bytes of one call, the last result) of fn after one warm-up call."""
    out = fn()
    del out
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    out = fn()
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - base
    del out
    ts, hold = [], []
    for _ in range(reps):
        hold.clear()
        ts.append(_device_ms(torch, lambda: hold.append(fn())))
    return float(np.median(ts)), float(np.min(ts)), int(peak), hold[0]


def main():
    import torch

    import flacarray_amd as fa

    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--streams", type=int, default=4096)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "window.md"))
    args = ap.parse_args()
    S, N, level, B = args.streams, 2**20, 5, 4096
    x = _signal(torch, S, N, 1)
    comp, st, nb = fa.encode_flac_device(x, level=level, compact=True)
    del x
    torch.cuda.empty_cache()
    torch.cuda.synchronize()
    every_second = torch.arange(0, S, 2, device="cuda")
    cases = [
        ("a", "drop the first 64 frames", 64 * B, N, None),
        ("b", "the same, last inside a frame", 64 * B, N - 1000, None),
        ("c", "every second stream, whole range", 0, N, every_second),
        ("d", "first = 1 (unaligned)", 1, N, None),
    ]
    rows = []
    for tag, what, first, last, idx in cases:
        sst, snb = (st, nb) if idx is None else (st[idx].contiguous(), nb[idx].contiguous())

        def window():
            return fa.window_flac_device(comp, st, nb, N, first, last, streams=idx, level=level)

        def dec_enc():
            ints = fa.decode_flac_device(comp, sst, snb, N, first, last)
            return fa.encode_flac_device(ints, level=level)

        w_med, w_min, w_peak, got = _timed(torch, window, args.reps)
        kept = got[0].clone()
        c_med, c_min, _, _ = _timed(torch, kept.clone, args.reps)
        d_med, d_min, d_peak, want = _timed(torch, dec_enc, args.reps)
        same = bool(torch.equal(got[0], want[0]) and torch.equal(got[2].reshape(-1), want[2].reshape(-1)))
        line = {"case": tag, "what": what, "streams": int(sst.numel()), "first": first, "last": last, "old_bytes": int(comp.numel()),
                "kept_bytes": int(kept.numel()), "window_ms_median": round(w_med, 3), "window_ms_min": round(w_min, 3),
                "window_peak_extra_bytes": w_peak, "clone_ms_median": round(c_med, 3), "clone_ms_min": round(c_min, 3),
                "dec_enc_ms_median": round(d_med, 3), "dec_enc_ms_min": round(d_min, 3), "dec_enc_peak_extra_bytes": d_peak,
                "equals_dec_enc": same}
        print(json.dumps(line), flush=True)
        rows.append(line)
        del got, want, kept
        torch.cuda.empty_cache()
    gb = lambda v: f"{v / 1e9:.2f} GB"  # noqa: E731
    with open(args.out, "w") as f:
        f.write("| case | streams | kept bytes | window (median / min) | peak extra | clone of kept bytes | decode + encode | peak extra | same bytes |\n")
        f.write("|---|---|---|---|---|---|---|---|---|\n")
        for r in rows:
            f.write(f"| {r['case']}. {r['what']} | {r['streams']} | {gb(r['kept_bytes'])} | {r['window_ms_median']:.2f} / {r['window_ms_min']:.2f} ms | "
                    f"{gb(r['window_peak_extra_bytes'])} | {r['clone_ms_median']:.2f} ms | {r['dec_enc_ms_median']:.2f} ms | "
                    f"{gb(r['dec_enc_peak_extra_bytes'])} | {'yes' if r['equals_dec_enc'] else 'NO'} |\n")
        f.write(f"\nold store: {S} x {N} int32, level {level}, {gb(rows[0]['old_bytes'])}; {args.reps} timed runs per figure after a warm-up.\n")


if __name__ == "__main__":
    main()
