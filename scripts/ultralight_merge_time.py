#!/usr/bin/env python3
"""Merged Ultralight passes against one pass per request, engine calls only, in ONE process and job.

    python scripts/ultralight_merge_time.py [--rounds 5] [--calls 8] [--warmup 3] [--frames 16] [--once LEG]

Seeded weights (synth.ultralight_state_dict), small banks, an arena of 256 frames.  Every leg is a host clock around an engine call
that returns when its frames are ready.  Each shape is warmed with `--warmup` calls per leg (eager, captured, replayed: every graph is
captured before anything is timed); the legs of a shape are then interleaved in `--rounds` rounds of `--calls` calls each.  Reported:
the median over all calls of a leg, and the spread of its per-round medians (max - min) - a difference between two legs counts only
where it is larger than that spread.

  same avatar    S = 2 / 4 / 8 / 16 requests of 16 frames of ONE avatar
      infer      ltk_ultralight_infer with the S requests: one pass per request, back to back (the behaviour before the merged entry)
      merged     ltk_ultralight_infer_merged, mode 0: one pass over all frames
  mixed avatars  A = 2 / 4 / 8 avatars x one request of 16 frames, and 4 avatars x 4 requests
      infer      as above
      mode 1     ltk_ultralight_infer_merged, per-avatar passes
      mode 2     ... grouped passes (weights per image: ul_gconv_kernel and the grouped depthwise / input / head kernels)
      and the largest byte difference between the frames of mode 1 and mode 2

--once LEG (same-infer | same-merged | mixed-mode1 | mixed-mode2): warm-up and ONE call of that leg at S = 4 / A = 4 and nothing else -
the process to wrap in `rocprofv3 --kernel-trace --stats -- ...`.  profiles/ultralight_merge.txt holds the output.
"""
from __future__ import annotations

import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--calls", type=int, default=8)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--frames", type=int, default=16)
    ap.add_argument("--once", default="")
    args = ap.parse_args()
    import numpy as np
    import torch
    import synth_inputs as synth
    from livetalking_amd.engine import Engine
    if not torch.cuda.is_available():
        sys.exit("needs a GPU: a CPU run measures nothing")
    B = args.frames
    eng = Engine(0)
    n_av = 8
    aids = []
    for i in range(n_av):
        frames, faces, coords = synth.ultralight_avatar(4, (96, 128), seed=60 + i)
        aids.append(eng.register_ultralight_avatar(synth.ultralight_state_dict(100 + i), faces, frames, coords, max_frames=256 if i == 0 else 1))
    info = eng.ultralight_info()
    print(f"arena {info['frames']} frames, {info['bytes'] / 1e6:.1f} MB = {info['bytes_per_frame'] / 1e6:.3f} MB per frame; grouped path built: {info['grouped']}; "
          f"{B} frames per request")
    feat = torch.from_numpy(np.ascontiguousarray(synth.ultralight_feats(B, 77).reshape(B, 16, 32, 32))).cuda()

    def requests(avatars):
        """-> (reqs, preds): one request of B frames per entry of `avatars`, every one with its own output tensor"""
        preds = [torch.zeros(B, 160, 160, 3, dtype=torch.uint8, device="cuda") for _ in avatars]
        return [(a, 3 * r, B, feat.data_ptr(), p.data_ptr()) for r, (a, p) in enumerate(zip(avatars, preds))], preds

    def measure(title, legs):
        for _, fn in legs:
            for _ in range(args.warmup):
                fn()
        times = {name: [[] for _ in range(args.rounds)] for name, _ in legs}
        for rd in range(args.rounds):
            order = legs if rd % 2 == 0 else legs[::-1]
            for _ in range(args.calls):
                for name, fn in order:
                    t0 = time.perf_counter()
                    fn()
                    times[name][rd].append((time.perf_counter() - t0) * 1e3)
        base = statistics.median([t for r in times[legs[0][0]] for t in r])
        out = {}
        for name, _ in legs:
            allt = [t for r in times[name] for t in r]
            meds = [statistics.median(r) for r in times[name]]
            med, spread = statistics.median(allt), max(meds) - min(meds)
            out[name] = (med, spread)
            print(f"  {title:34s} {name:8s} median {med:8.3f} ms  round medians {min(meds):8.3f} .. {max(meds):8.3f} (spread {spread:6.3f})  "
                  f"{len(allt)} calls  {base / med:5.2f}x")
        return out

    if args.once:
        kind, leg = args.once.split("-")
        reqs, preds = requests([aids[0]] * 4 if kind == "same" else aids[:4])
        fn = {"infer": lambda: eng.ultralight_infer(reqs), "merged": lambda: eng.ultralight_infer_merged(reqs),
              "mode1": lambda: eng.ultralight_infer_merged(reqs, mode=1), "mode2": lambda: eng.ultralight_infer_merged(reqs, mode=2)}[leg]
        for _ in range(args.warmup + 1):
            fn()
        print(f"{args.once}: {args.warmup} warm-up calls and one call done, checksum {sum(int(p.sum()) for p in preds)}")
        eng.close()
        return

    print(f"{args.rounds} rounds x {args.calls} calls per leg after {args.warmup} warm-up calls; host clock around calls that return when the frames are ready")
    same_ok, grouped_ok = True, True
    print("same avatar:")
    for S in (2, 4, 8, 16):
        reqs, preds = requests([aids[0]] * S)
        eng.ultralight_infer(reqs)
        want = [p.clone() for p in preds]
        rep = eng.ultralight_infer_merged(reqs, report=True)
        diff = max(int((p.int() - w.int()).abs().max()) for p, w in zip(preds, want))
        res = measure(f"S = {S:2d} ({S * B:3d} frames, {rep['n_passes']} pass)", [("infer", lambda: eng.ultralight_infer(reqs)),
                                                                                  ("merged", lambda: eng.ultralight_infer_merged(reqs))])
        gain = res["infer"][0] - res["merged"][0]
        beats = gain > max(res["infer"][1], res["merged"][1])
        same_ok = same_ok and beats
        print(f"    merged - infer frames: max {diff} LSB; merged {'beats' if beats else 'does NOT beat'} the baseline by more than the spread ({gain:+.3f} ms)")
    print("mixed avatars:")
    for avatars, label in ((aids[:2], "A = 2"), (aids[:4], "A = 4"), (aids[:8], "A = 8"), ([aids[r % 4] for r in range(16)], "A = 4 x 4 requests")):
        reqs, preds = requests(avatars)
        eng.ultralight_infer_merged(reqs, mode=1)
        one = [p.clone() for p in preds]
        rep = eng.ultralight_infer_merged(reqs, mode=2, report=True)
        diff = max(int((p.int() - w.int()).abs().max()) for p, w in zip(preds, one))
        share = sum(int((p != w).sum()) for p, w in zip(preds, one)) / sum(p.numel() for p in preds)
        res = measure(f"{label} ({len(avatars) * B:3d} frames)", [("infer", lambda: eng.ultralight_infer(reqs)),
                                                                 ("mode 1", lambda: eng.ultralight_infer_merged(reqs, mode=1)),
                                                                 ("mode 2", lambda: eng.ultralight_infer_merged(reqs, mode=2))])
        gain = res["mode 1"][0] - res["mode 2"][0]
        beats = gain > max(res["mode 1"][1], res["mode 2"][1])
        grouped_ok = grouped_ok and beats
        print(f"    mode 2 ran {rep['n_passes']} grouped pass(es); mode 1 - mode 2 frames: max {diff} LSB on {100 * share:.3f} % of the bytes; mode 2 "
              f"{'beats' if beats else 'does NOT beat'} mode 1 by more than the spread ({gain:+.3f} ms)")
    print(f"LTK_UL_SCHED default-on is supported: {same_ok} (the merged call beats the baseline in every same-avatar leg)")
    print(f"LTK_UL_GROUPED default-on is supported: {grouped_ok} (mode 2 beats mode 1 in every mixed-avatar leg)")
    eng.close()


if __name__ == "__main__":
    main()
