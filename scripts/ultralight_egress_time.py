#!/usr/bin/env python3
"""Ultralight frame delivery, per 16 frames at 1280x720: the per-frame path against the batched ones, in ONE process and job.

    python scripts/ultralight_egress_time.py [--iters 30] [--warmup 5] [--frames 16] [--hw 720 1280] [--once]

Seeded bank (4 frames) and 16 seeded predictions.  Every leg is a host clock around calls that end in a stream synchronisation
(each entry returns after its device-to-host copy completed); the legs alternate inside every iteration, the figure is the median
over the iterations, min and max beside it:

  per-frame  16 x ltk_ultralight_paste_back into pageable memory (the only path before the batch entries; the baseline)
  batch      ltk_ultralight_paste_back_batch into one pinned block
  bgr24      ltk_egress_batch(LTK_SRC_ULTRALIGHT, LTK_FMT_BGR24) into one pinned block (composite + watermark + copy)
  i420       ltk_egress_batch(LTK_SRC_ULTRALIGHT, LTK_FMT_I420) into one pinned block (half the bytes cross the link)

The outputs of the three batched legs are compared with the per-frame composites (and the host I420 twin) before anything is timed.

--once: one call of each batched entry and nothing else - the process to wrap in
`rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python scripts/ultralight_egress_time.py --once`;
`--stats DIR` then prints the device-only time of the composite (ul_paste_batch_kernel) and conversion (egress_batch_kernel)
launches from that table.  profiles/ultralight_egress.txt holds both outputs.
"""
from __future__ import annotations

import argparse
import csv
import glob
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def stats(path: str) -> None:
    files = sorted(glob.glob(os.path.join(path, "**", "*kernel_stats.csv"), recursive=True)) if os.path.isdir(path) else [path]
    if not files:
        sys.exit(f"no *kernel_stats.csv under {path}")
    rows = list(csv.DictReader(open(files[0])))
    key_t = next(k for k in rows[0] if "TotalDuration" in k)
    key_n = next(k for k in rows[0] if k in ("Calls", "Count"))
    print(f"device-only kernel time ({os.path.basename(files[0])}), one call of each batched entry:")
    for r in rows:
        if "paste" in r["Name"] or "egress" in r["Name"]:
            n, t = int(r[key_n]), float(r[key_t])
            print(f"  {r['Name'][:90]:90s} {n:3d} launches  {t / 1e3:9.1f} us total  {t / n / 1e3:8.1f} us per launch")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--frames", type=int, default=16)
    ap.add_argument("--hw", type=int, nargs=2, default=[720, 1280])
    ap.add_argument("--once", action="store_true")
    ap.add_argument("--stats", default="")
    args = ap.parse_args()
    if args.stats:
        return stats(args.stats)
    import numpy as np
    import torch
    import synth_inputs as synth
    from livetalking_amd import egress
    from livetalking_amd.engine import Engine
    if not torch.cuda.is_available():
        sys.exit("needs a GPU: a CPU run measures nothing")
    H, W = args.hw
    n = args.frames
    eng = Engine(0)
    frames, faces, coords = synth.ultralight_avatar(4, (H, W), seed=3)
    aid = eng.register_ultralight_avatar(synth.ultralight_state_dict(1234), faces, frames, coords, max_frames=1)
    idx = [(3 * i + 1) % 4 for i in range(n)]
    preds = torch.from_numpy(np.random.default_rng(7).integers(0, 256, (n, 160, 160, 3), dtype=np.uint8)).cuda()
    sess = eng.egress_open(H, W)
    pageable = [np.empty((H, W, 3), np.uint8) for _ in range(n)]
    pin_bgr = torch.empty((n, H, W, 3), dtype=torch.uint8, pin_memory=True)
    pin_eg = torch.empty((n, H, W, 3), dtype=torch.uint8, pin_memory=True)
    pin_yuv = torch.empty((n, H * 3 // 2, W), dtype=torch.uint8, pin_memory=True)

    def per_frame():
        for i in range(n):
            eng.ultralight_paste_back(aid, idx[i], preds[i].data_ptr(), pageable[i])

    def batch():
        eng.ultralight_paste_back_batch(aid, idx, preds.data_ptr(), pin_bgr.data_ptr())

    def bgr24():
        eng.egress_batch(sess, egress.SRC_ULTRALIGHT, aid, idx, preds.data_ptr(), pin_eg.data_ptr(), egress.FMT_BGR24, 1)

    def i420():
        eng.egress_batch(sess, egress.SRC_ULTRALIGHT, aid, idx, preds.data_ptr(), pin_yuv.data_ptr(), egress.FMT_I420, 1)

    legs = [("per-frame", per_frame), ("batch", batch), ("bgr24", bgr24), ("i420", i420)]
    if args.once:
        for _, fn in legs[1:]:
            fn()
        print(f"one call of each batched entry done, checksum {int(pin_bgr.sum()) + int(pin_yuv.sum())}")
        eng.egress_close(sess)
        eng.close()
        return
    # same bytes on every path, at the size that is timed
    for _, fn in legs:
        fn()
    for i in range(n):
        assert np.array_equal(pin_bgr.numpy()[i], pageable[i]) and np.array_equal(pin_eg.numpy()[i], pageable[i]), i
        assert np.array_equal(pin_yuv.numpy()[i], np.asarray(egress.host_bgr_to_i420(pageable[i], 1))), i
    print(f"{n} frames {W}x{H}: batch, bgr24 and i420 outputs equal the per-frame composites (i420: their host conversion)")
    for _ in range(args.warmup):
        for _, fn in legs:
            fn()
    times = {name: [] for name, _ in legs}
    for it in range(args.iters):
        order = legs if it % 2 == 0 else legs[::-1]              # alternate the order: no leg always runs behind the same one
        for name, fn in order:
            t0 = time.perf_counter()
            fn()
            times[name].append((time.perf_counter() - t0) * 1e3)
    mb = {"per-frame": n * H * W * 3, "batch": n * H * W * 3, "bgr24": n * H * W * 3, "i420": n * H * W * 3 // 2}
    base = statistics.median(times["per-frame"])
    print(f"{args.iters} iterations after {args.warmup} warm-up, ms per {n} frames (host clock, each call ends in a stream synchronisation):")
    for name, _ in legs:
        t = times[name]
        med = statistics.median(t)
        print(f"  {name:10s} median {med:8.3f}  min {min(t):8.3f}  max {max(t):8.3f}   {mb[name] / 1e6:6.1f} MB to the host "
              f"{mb[name] / med / 1e6:6.2f} GB/s   {base / med:5.2f}x the per-frame path")
    eng.egress_close(sess)
    eng.close()


if __name__ == "__main__":
    main()
