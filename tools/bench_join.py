"""Cost of join_flac_device (FlacArray.concatenate / extend) on a resident int32 store of 4096 x 2^20 samples (bench.py's
data and geometry, level 5), next to two yardsticks measured in the same run on the same stores:
  clone        `clone()` of the result's bytes: the floor for anything that writes the result once
  today        what a caller does without join: decode_flac_device of the parts behind the first and append_flac_device
               of the decoded samples to the first part, with its peak extra device memory (the decoded copy and the
               append's buffers)
Four cases:
  a  the two halves                                    join([x[:, :N/2], x[:, N/2:]])
  b  64 equal parts                                    join([x[:, k N/64 : (k+1) N/64] for k in range(64)])
  c  the whole store extended by a 64-frame store      join([x, x[:, :64 B]]): part 0 moves as two plain copies
  d  cut at N/2 + 1 (unaligned: every frame of the second part changes)    decode + append in row chunks of 256 MiB
Device events around each call, the median and minimum of --reps runs after a warm-up round (the caching allocator
serves every buffer after that round); peak extra memory from torch.cuda.max_memory_allocated over one call.  These are
join_flac_device times: FlacArray.concatenate adds the PCIe copy of the new blob to its host mirror.  One JSON line per
case on stdout, and the table of profiles/join.md written to --out.
Usage: python -m tools.bench_join [--reps N] [--streams S] [--out PATH]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from bench import make_data  # noqa: E402
from tools.bench_window import _timed  # noqa: E402


def main():
    import torch

    import flacarray_amd as fa

    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--streams", type=int, default=4096)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "join.md"))
    args = ap.parse_args()
    S, N, level, B = args.streams, 2**20, 5, 4096
    x = make_data(torch, S, N, 1, "cuda")

    def enc(a, b):
        return fa.encode_flac_device(x[:, a:b].contiguous(), level=level, compact=True) + (b - a,)

    whole = enc(0, N)
    cases = [
        ("a", "the two halves", [enc(0, N // 2), enc(N // 2, N)]),
        ("b", "64 equal parts", [enc(k * (N // 64), (k + 1) * (N // 64)) for k in range(64)]),
        ("c", "the whole store + 64 frames", [whole, enc(0, 64 * B)]),
        ("d", "cut at N/2 + 1 (unaligned)", [enc(0, N // 2 + 1), enc(N // 2 + 1, N)]),
    ]
    del x
    torch.cuda.empty_cache()
    torch.cuda.synchronize()
    rows = []
    for tag, what, stores in cases:
        def join():
            return fa.join_flac_device(stores, level=level)

        def today():
            ints = [fa.decode_flac_device(c, st, nb, n) for c, st, nb, n in stores[1:]]
            ints = ints[0] if len(ints) == 1 else torch.cat(ints, dim=1)
            first = stores[0]
            return fa.append_flac_device(first[0], first[1], first[2], first[3], ints, level=level)

        j_med, j_min, j_peak, got = _timed(torch, join, args.reps)
        result = got[0].clone()
        c_med, c_min, _, _ = _timed(torch, result.clone, args.reps)
        t_med, t_min, t_peak, want = _timed(torch, today, args.reps)
        same = bool(torch.equal(got[0], want[0]) and torch.equal(got[2].reshape(-1), want[2].reshape(-1)))
        line = {"case": tag, "what": what, "parts": len(stores), "result_bytes": int(result.numel()), "join_ms_median": round(j_med, 3),
                "join_ms_min": round(j_min, 3), "join_peak_extra_bytes": j_peak, "clone_ms_median": round(c_med, 3), "clone_ms_min": round(c_min, 3),
                "today_ms_median": round(t_med, 3), "today_ms_min": round(t_min, 3), "today_peak_extra_bytes": t_peak, "equals_today": same}
        print(json.dumps(line), flush=True)
        rows.append(line)
        del got, want, result
        torch.cuda.empty_cache()
    gb = lambda v: f"{v / 1e9:.2f} GB"  # noqa: E731
    with open(args.out, "w") as f:
        f.write("| case | parts | result bytes | join (median / min) | peak extra | clone of the result | decode + append | peak extra | same bytes |\n")
        f.write("|---|---|---|---|---|---|---|---|---|\n")
        for r in rows:
            f.write(f"| {r['case']}. {r['what']} | {r['parts']} | {gb(r['result_bytes'])} | {r['join_ms_median']:.2f} / {r['join_ms_min']:.2f} ms | "
                    f"{gb(r['join_peak_extra_bytes'])} | {r['clone_ms_median']:.2f} ms | {r['today_ms_median']:.2f} ms | "
                    f"{gb(r['today_peak_extra_bytes'])} | {'yes' if r['equals_today'] else 'NO'} |\n")
        f.write(f"\nstore: {S} x {N} int32 (bench.py's data), level {level}; {args.reps} timed runs per figure after a warm-up.\n")


if __name__ == "__main__":
    main()
