#!/usr/bin/env python3
"""reindex on one MI355X, on the bench workload (bench.make_data, 4096 x 2^20 int32, level 5) rewritten into libFLAC's
layout, beside what it is measured against in the same process.  The foreign twin is built on the device from the
library's own encode: per stream "fLaC" + STREAMINFO, a VORBIS_COMMENT marked last, the frames verbatim (three device
copies per stream; no SEEKTABLE) -- so the reindexed store must equal the encode byte for byte, which is checked.  Device
events around each call, one warm call first, median of the repeats.  One JSON line:
  reindex_ms           (a) reindex_flac_device(verify=False)
  reindex_verify_ms    (b) the same with verify=True; verify_ms = (b) - (a), beside status_ms = frame_status_device alone
  index_ms             (c) DeviceDecodeIndex on the foreign store: K6 with its sync scan, the part reindex reuses
  clone_ms             (d) compressed.clone(): the floor of any copy of the store
  a_over_c_plus_d      (a) / ((c) + (d)); a_budget = (c) + 1.5 (d): the body's source and destination differ in alignment,
                       so every 16-byte chunk takes two loads
  decode_foreign_ms    (e) one-off decode_flac_device(verify=False) of the foreign store, which scans for the frames, and
  decode_reindexed_ms      of the reindexed store, which reads them from the SEEKTABLE"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

import bench
import flacarray_amd as fa

VENDOR = b"reference libFLAC 1.4.3 20230623"


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


def foreign_twin(comp, st, nb, n, block):
    """The own-layout store on the device as libFLAC lays it out; returns (blob, starts, nbytes) on the device."""
    nf = -(-n // block)
    vc = len(VENDOR).to_bytes(4, "little") + VENDOR + (0).to_bytes(4, "little")
    block_vc = torch.from_numpy(np.frombuffer(bytes([0x84]) + len(vc).to_bytes(3, "big") + vc, dtype=np.uint8).copy()).to(comp.device)
    h_st, h_nb = st.cpu().numpy(), nb.cpu().numpy()
    hb = 46 + 18 * nf
    f_nb = h_nb - hb + 42 + block_vc.numel()
    f_st = np.concatenate([[0], np.cumsum(f_nb)[:-1]]).astype(np.int64)
    out = torch.empty(int(f_nb.sum()), dtype=torch.uint8, device=comp.device)
    for s, (o, k, fo) in enumerate(zip(h_st.tolist(), h_nb.tolist(), f_st.tolist())):
        out[fo : fo + 42] = comp[o : o + 42]
        out[fo + 42 : fo + 42 + block_vc.numel()] = block_vc
        out[fo + 42 + block_vc.numel() : fo + int(f_nb[s])] = comp[o + hb : o + k]
    return out, torch.from_numpy(f_st).to(comp.device), torch.from_numpy(f_nb.astype(np.int64)).to(comp.device)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--channels", type=int, default=4096)
    ap.add_argument("--samples", type=int, default=1 << 20)
    ap.add_argument("--reps", type=int, default=5)
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    block = 4096
    with torch.cuda.device(dev):
        x = bench.make_data(torch, args.channels, args.samples, 5, dev)
        comp, st, nb = fa.encode_flac_device(x, level=5, compact=True)[:3]
        n = x.shape[1]
        del x
        torch.cuda.empty_cache()
        st, nb = st.reshape(-1), nb.reshape(-1)
        fb, fst, fnb = foreign_twin(comp, st, nb, n, block)
        row = {"case": "int32 (%d, %d) level 5, foreign twin built on the device" % (args.channels, n), "store_MB": round(comp.numel() / 1e6, 1),
               "foreign_MB": round(fb.numel() / 1e6, 1), "frames": int(st.numel() * -(-n // block))}
        got = fa.reindex_flac_device(fb, fst, fnb, n, verify=True)
        row["equals_the_own_encode"] = bool(torch.equal(got[0], comp) and torch.equal(got[1], st) and torch.equal(got[2], nb))
        row["foreign_status_all_unlocated"] = bool((fa.frame_status_device(fb, fst, fnb, n, block_size=block) == fa.FRAME_UNLOCATED).all())
        del got
        row["reindex_ms"] = round(timed(lambda: fa.reindex_flac_device(fb, fst, fnb, n, verify=False), args.reps), 3)
        row["reindex_verify_ms"] = round(timed(lambda: fa.reindex_flac_device(fb, fst, fnb, n, verify=True), args.reps), 3)
        row["verify_ms"] = round(row["reindex_verify_ms"] - row["reindex_ms"], 3)
        row["status_ms"] = round(timed(lambda: fa.frame_status_device(comp, st, nb, n, block_size=block), args.reps), 3)

        def index():
            fa.DeviceDecodeIndex(fb, fst, fnb, n).close()

        row["index_ms"] = round(timed(index, args.reps), 3)
        row["index_reindexed_ms"] = round(timed(lambda: fa.DeviceDecodeIndex(comp, st, nb, n).close(), args.reps), 3)
        row["clone_ms"] = round(timed(lambda: fb.clone(), args.reps), 3)
        row["a_over_c_plus_d"] = round(row["reindex_ms"] / (row["index_ms"] + row["clone_ms"]), 3)
        row["a_budget_ms"] = round(row["index_ms"] + 1.5 * row["clone_ms"], 3)
        row["decode_foreign_ms"] = round(timed(lambda: fa.decode_flac_device(fb, fst, fnb, n, verify=False), args.reps), 3)
        row["decode_reindexed_ms"] = round(timed(lambda: fa.decode_flac_device(comp, st, nb, n, verify=False), args.reps), 3)
        print(json.dumps(row), flush=True)


if __name__ == "__main__":
    main()
