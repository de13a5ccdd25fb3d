"""Every route through the decode driver once, for a kernel trace (profiles/decode_driver.md).

    rocprofv3 --kernel-trace --stats -d DIR -- python tools/decode_routes.py

Two stores from tests/golden/flac_writer.py, each one- and two-channel: 3 streams x 100 samples at block size 32, and 4
streams of block size 192 whose frames cycle through LPC orders 1-8, 9-12, 13-16 and 17-32 (all three history passes of
K7).  Per store: whole and range decode, slices (3 tasks: K7L with the task table in the kernel arguments; 5000 tasks: K7),
the indexed host read, compare (integers and floats), reduce (all streams, named streams), histogram, find (count and
fill), salvage with one damaged frame, reindex and index create.  Prints one line per route with a digest of what it
returned: two libraries (FLACARRAY_HIP_LIB) must print the same lines, and their traces the same kernel names in order."""
import hashlib
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

from flacarray_amd import libflacarray as F  # noqa: E402
from tests.golden import flac_writer as W  # noqa: E402


def digest(x):
    h = hashlib.sha1()
    for t in x if isinstance(x, (tuple, list)) else (x,):
        if t is None:
            continue
        a = t.cpu().numpy() if hasattr(t, "cpu") else np.asarray(t)
        h.update(str(a.dtype).encode() + str(a.shape).encode() + np.ascontiguousarray(a).tobytes())
    return h.hexdigest()[:12]


def routes(name, batch):
    nch = batch["channels"]
    i64 = nch == 2
    n, ns, B = batch["n"], len(batch["streams"]), batch["block"]
    blob_h, st_h, nb_h = W.pack(batch["streams"])
    blob, st, nb = (torch.from_numpy(a).cuda() for a in (blob_h, st_h, nb_h))
    ft = torch.float64 if i64 else torch.float32
    offsets = torch.linspace(-1.0, 1.0, ns, dtype=ft).cuda()
    gains = torch.full((ns,), 0.25, dtype=ft).cuda()

    def say(route, fn):
        try:
            out = digest(fn())
        except RuntimeError as e:  # (a refusal is an answer too: both libraries must give the same one)
            out = "raised " + str(e)[:80]
        torch.cuda.synchronize()
        print(f"{name} {route}: {out}", flush=True)

    whole = F.decode_flac_device(blob, st, nb, n, is_int64=i64)
    say("whole", lambda: whole)
    say("range", lambda: F.decode_flac_device(blob, st, nb, n, B // 2, n - 3, is_int64=i64))
    say("whole float", lambda: F.decode_flac_device(blob, st, nb, n, offsets=offsets, gains=gains, is_int64=i64))
    say("slices one-off", lambda: F.decode_slices_device(blob, st, nb, n, [0, ns - 1], [1, n - B], [B, B], is_int64=i64)[0])
    ix = F.DeviceDecodeIndex(blob, st, nb, n, is_int64=i64)
    say("index create", lambda: torch.zeros(1))
    say("indexed range", lambda: ix.decode(3, n - 1))
    say("slices 3 tasks", lambda: ix.decode_slices([1, 0, ns - 1], [0, B + 1, n - 2], [5, 7, 2])[0])
    rng = np.random.default_rng(5)
    k = 5000
    say("slices 5000 tasks", lambda: ix.decode_slices(rng.integers(0, ns, k), rng.integers(0, n - 8, k), rng.integers(1, 8, k))[0])
    say("indexed host read", lambda: ix.decode_slices([ns - 1], [B - 3], [10], to_host=True)[0])
    say("indexed host read float", lambda: ix.decode_slices([0], [2], [B], offsets=offsets, gains=gains, to_host=True)[0])
    say("compare int", lambda: F.compare_flac_device(blob, st, nb, whole))
    fl = F.decode_flac_device(blob, st, nb, n, offsets=offsets, gains=gains, is_int64=i64)
    say("compare float", lambda: F.compare_flac_device(blob, st, nb, fl, offsets=offsets, gains=gains))
    say("reduce all", lambda: F.reduce_flac_device(blob, st, nb, n, width=40, is_int64=i64))
    say("reduce named", lambda: F.reduce_flac_device(blob, st, nb, n, width=40, first_sample=5, last_sample=n - 5, streams=[ns - 1, 0], is_int64=i64))
    say("reduce indexed", lambda: ix.reduce(width=64))
    lo, shift = np.full(ns, -(1 << 20), dtype=np.int64), np.full(ns, 14, dtype=np.int32)
    say("histogram", lambda: F.histogram_flac_device(blob, st, nb, n, lo, shift, 128, is_int64=i64))
    say("histogram named", lambda: F.histogram_flac_device(blob, st, nb, n, lo[:2], shift[:2], 128, streams=[1, 0], is_int64=i64))
    say("find", lambda: F.find_flac_device(blob, st, nb, n, lo=-1000, hi=1000, is_int64=i64))
    say("find named indexed", lambda: ix.find(lo=-1000, hi=1000, streams=[ns - 1], first_sample=1, last_sample=n - 1))
    hurt = blob.clone()
    at = int(st_h[1] + nb_h[1] - 6)  # inside the last frame of stream 1
    hurt[at] = hurt[at] ^ 0x40
    say("salvage", lambda: F.decode_flac_salvage_device(hurt, st, nb, n, is_int64=i64, block_size=B))
    say("salvage intact", lambda: F.decode_flac_salvage_device(blob, st, nb, n, is_int64=i64, block_size=B))
    say("reindex", lambda: F.reindex_flac_device(blob, st, nb, n, is_int64=i64))
    ix.close()


def main():
    for nch in (1, 2):
        routes(f"b32x{nch}", W._batch("b32", np.random.default_rng(20 + nch), 3, 100, 32, nch, layout="libflac"))
        routes(f"b192x{nch}", W._batch("b192", np.random.default_rng(30 + nch), 4, 8 * 192 + 50, 192, nch, bucket_cycle=True))
    print("decode_routes: done")


if __name__ == "__main__":
    main()
