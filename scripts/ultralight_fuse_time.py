#!/usr/bin/env python3
"""The Ultralight pass with its inverted residuals fused (knob UL_FUSE_IR = 1: ul_ir_kernel, one launch per block) against the pass as
three launches per block (knob 0), in ONE process and job.

    python scripts/ultralight_fuse_time.py [--rounds 5] [--iters 30] [--calls 8] [--warmup 3] [--once K]

Seeded weights (synth.ultralight_state_dict), a small bank, an arena of 256 frames.  The knob is changed in-process
(ltk_debug_set_knob); a change drops every captured pass, so each leg re-captures before it is timed.

  pass      1 / 16 / 64 / 256 frames through ltk_ultralight_time (device events around `--iters` replays of the captured pass, after its
            own eager and capturing pass); legs knob 0 and knob 1 interleaved in `--rounds` rounds, the median of the round values and
            their spread (max - min) per leg
  merged    ltk_ultralight_infer_merged with 4 requests of 16 frames of one avatar (one per-avatar pass of 64 frames): host clock
            around calls that return when the frames are ready, `--warmup` calls after every knob change, then `--calls` calls per
            leg and round

Knob 0 of this library stands for the parent commit's pass: tests/test_ul_ir_gpu.py::test_back_to_knob_0_is_the_parent_pass shows
that it lists and launches the 86 ops of before and leaves the same bytes.

The rule for a later default (stated with the knob, profiles/ultralight_fuse_ir.txt): knob 1 at most 0.92 of knob 0 at 16 frames and
not above 1.00 at 1, 64 and 256 frames.  The last line prints the verdict.

--once K (0 | 1): that knob value, one ltk_ultralight_time call of a 16-frame pass with `--iters` replays (2 + iters passes in all) and
nothing else - the process to wrap in `rocprofv3 --kernel-trace --stats -- ...` for the launch count and the kernel shares
(scripts/prof_report.py prints them; calls / (2 + iters) = launches per pass).
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

FRAMES = (1, 16, 64, 256)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--calls", type=int, default=8)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--once", default="")
    args = ap.parse_args()
    import numpy as np
    import torch
    import synth_inputs as synth
    from livetalking_amd.engine import Engine
    if not torch.cuda.is_available():
        sys.exit("needs a GPU: a CPU run measures nothing")
    eng = Engine(0)
    frames, faces, coords = synth.ultralight_avatar(4, (96, 128), seed=60)
    aid = eng.register_ultralight_avatar(synth.ultralight_state_dict(100), faces, frames, coords, max_frames=256)

    def knob(v):
        Engine.set_knob("UL_FUSE_IR", v)

    if args.once:
        v = int(args.once)
        knob(v)
        ops = eng.ultralight_ops(aid)
        ms, _ = eng.ultralight_time(aid, 16, args.iters)
        print(f"knob {v}: {len(ops)} ops listed, {sum(t == 15 for _, t in ops)} fused; 16-frame pass {ms:.4f} ms; {2 + args.iters} passes ran")
        knob(0)
        eng.close()
        return

    for v in (0, 1):
        knob(v)
        ops = eng.ultralight_ops(aid)
        print(f"knob {v}: {len(ops)} launches per pass, {sum(t == 15 for _, t in ops)} of them ul_ir_kernel")
    print(f"pass: {args.rounds} rounds, knob 0 and knob 1 interleaved, {args.iters} replays per value (device events)")
    ratio = {}
    for nf in FRAMES:
        vals = {0: [], 1: []}
        for rd in range(args.rounds):
            for v in ((0, 1) if rd % 2 == 0 else (1, 0)):
                knob(v)
                vals[v].append(eng.ultralight_time(aid, nf, args.iters)[0])
        med = {v: statistics.median(vals[v]) for v in vals}
        ratio[nf] = med[1] / med[0]
        for v in (0, 1):
            print(f"  {nf:3d} frames  knob {v}  median {med[v]:8.4f} ms  rounds {min(vals[v]):8.4f} .. {max(vals[v]):8.4f} "
                  f"(spread {max(vals[v]) - min(vals[v]):6.4f})  {nf / med[v] * 1e3:9.0f} frames/s")
        print(f"  {nf:3d} frames  knob 1 / knob 0 = {ratio[nf]:.3f}")

    B, S = 16, 4
    feat = torch.from_numpy(np.ascontiguousarray(synth.ultralight_feats(B, 77).reshape(B, 16, 32, 32))).cuda()
    preds = [torch.zeros(B, 160, 160, 3, dtype=torch.uint8, device="cuda") for _ in range(S)]
    reqs = [(aid, 3 * r, B, feat.data_ptr(), p.data_ptr()) for r, p in enumerate(preds)]
    print(f"merged: {S} requests of {B} frames, {args.rounds} rounds x {args.calls} calls per value after {args.warmup} warm-up calls (host clock)")
    times = {0: [], 1: []}
    for rd in range(args.rounds):
        for v in ((0, 1) if rd % 2 == 0 else (1, 0)):
            knob(v)
            for _ in range(args.warmup):
                eng.ultralight_infer_merged(reqs)
            row = []
            for _ in range(args.calls):
                t0 = time.perf_counter()
                eng.ultralight_infer_merged(reqs)
                row.append((time.perf_counter() - t0) * 1e3)
            times[v].append(statistics.median(row))
    med = {v: statistics.median(times[v]) for v in times}
    for v in (0, 1):
        print(f"  merged {S} x {B}  knob {v}  median {med[v]:8.4f} ms  round medians {min(times[v]):8.4f} .. {max(times[v]):8.4f} "
              f"(spread {max(times[v]) - min(times[v]):6.4f})")
    print(f"  merged {S} x {B}  knob 1 / knob 0 = {med[1] / med[0]:.3f}")
    knob(0)
    ok = ratio[16] <= 0.92 and all(ratio[n] <= 1.00 for n in (1, 64, 256))
    print("rule: knob 1 <= 0.92 x knob 0 at 16 frames and <= 1.00 x at 1, 64 and 256 frames: "
          + ", ".join(f"{n}: {ratio[n]:.3f}" for n in FRAMES) + f" -> default-on may {'be proposed' if ok else 'NOT be proposed'}")
    eng.close()


if __name__ == "__main__":
    main()
