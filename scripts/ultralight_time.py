#!/usr/bin/env python3
"""Ultralight pass time (ltk_ultralight_time): milliseconds, MACs and fps of one pass at 1 / 16 / 64 frames, as
ltk_ultralight_infer enqueues it (bank crops in, uint8 frames out, replayed graph under knob GRAPH).

    python scripts/ultralight_time.py [--frames 1 16 64] [--iters 50] [--once N]

--once N: a single eager N-frame pass and nothing else - the process to wrap in `rocprofv3 --kernel-trace --stats -- ...` for
the per-kernel table; scripts/ultralight_time.py --stats <csv> then prints launch count and the share of time in depthwise /
pointwise (dense) / upsample kernels from that table.  profiles/ultralight_pass.txt holds both outputs.
"""
from __future__ import annotations

import argparse
import csv
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def kernel_class(name: str) -> str:
    if "dwconv3x3" in name:
        return "depthwise"
    if "upsample2x" in name:
        return "upsample"
    if "ul_in" in name or "ul_head" in name or "ul_pack_feat" in name:
        return "input / head"
    if "conv" in name or "lin_" in name:
        return "pointwise / dense"
    return "other"


def stats(path: str, passes: int) -> None:
    rows = list(csv.DictReader(open(path)))
    key_t = next(k for k in rows[0] if "TotalDuration" in k or k == "TotalDurationNs")
    key_n = next(k for k in rows[0] if k in ("Calls", "Count"))
    total = sum(float(r[key_t]) for r in rows)
    by = {}
    launches = 0
    for r in rows:
        c = kernel_class(r["Name"])
        by.setdefault(c, [0.0, 0])
        by[c][0] += float(r[key_t]); by[c][1] += int(r[key_n])
        launches += int(r[key_n])
    print(f"kernel launches: {launches} over {passes} pass(es) = {launches / passes:.0f} per pass; kernel time {total / passes / 1e3:.1f} us per pass")
    for c, (t, n) in sorted(by.items(), key=lambda kv: -kv[1][0]):
        print(f"  {c:20s} {100 * t / total:5.1f} %   {n / passes:5.0f} launches per pass   {t / passes / 1e3:8.1f} us")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, nargs="*", default=[1, 16, 64])
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--once", type=int, default=0)
    ap.add_argument("--stats", default="")
    ap.add_argument("--passes", type=int, default=1)
    args = ap.parse_args()
    if args.stats:
        return stats(args.stats, args.passes)
    import numpy as np
    import torch
    import synth_inputs as synth
    from livetalking_amd.engine import Engine
    eng = Engine(0)
    frames, faces, coords = synth.ultralight_avatar(4, (360, 640), seed=3)
    nmax = max(args.frames + [args.once])
    aid = eng.register_ultralight_avatar(synth.ultralight_state_dict(1234), faces, frames, coords, max_frames=nmax)
    if args.once:
        n = args.once
        d_feat = torch.from_numpy(synth.ultralight_feats(n).reshape(n, 16, 32, 32)).cuda()
        d_pred = torch.zeros(n, 160, 160, 3, dtype=torch.uint8, device="cuda")
        eng.ultralight_infer([(aid, 0, n, d_feat.data_ptr(), d_pred.data_ptr())])
        print(f"one eager {n}-frame pass done, checksum {int(d_pred.sum())}")
    else:
        for n in args.frames:
            ms, macs = eng.ultralight_time(aid, n, args.iters)
            print(f"{n:3d} frames: {ms:8.4f} ms per pass  {macs / n / 1e9:.3f} GMAC per frame  {n / ms * 1e3:9.0f} fps  "
                  f"{2 * macs / ms / 1e9:7.2f} TFLOP/s")
    eng.close()


if __name__ == "__main__":
    main()
