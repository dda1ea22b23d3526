#!/usr/bin/env python3
"""SHA-256 of the frames the Ultralight entries return, for comparing two builds of the library byte for byte.

    python scripts/ultralight_identity.py [--time-register K]
    LTK_LIB=/path/to/other/libltk_hip.so python scripts/ultralight_identity.py

Two avatars (synth.ultralight_state_dict seeds 1234 and 7, arena of 17 frames), seeded features.  One line per call, every call made
three times (eager, captured, replayed) with the three hashes on the line:

  infer   B = 1, 3, 17 frames of the first avatar, each under knob UL_FUSE_IR 0 and 1
  merged  mode 1 with requests of 1 + 2 + 3 frames of the first avatar; mode 0 and mode 2 with two avatars x (2, 1) frames

Every line of two builds must be equal for the later one to count as a pure refactoring of the earlier one.  The hashes depend on
the compiler, so they are a record (profiles/ultralight_program_refactor.txt), not a test.

--time-register K: also the host time of register_ultralight_avatar, median of K further registrations, on a line that starts
with '#' (not part of the comparison).
"""
from __future__ import annotations

import argparse
import hashlib
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--time-register", type=int, default=0)
    args = ap.parse_args()
    import numpy as np
    import torch
    import synth_inputs as synth
    from livetalking_amd.engine import Engine
    if not torch.cuda.is_available():
        sys.exit("needs a GPU")
    eng = Engine(0)
    aids = []
    for i, seed in enumerate((1234, 7)):
        frames, faces, coords = synth.ultralight_avatar(5, (96, 128), seed=40 + i)
        aids.append(eng.register_ultralight_avatar(synth.ultralight_state_dict(seed), faces, frames, coords, max_frames=17))
    feat = torch.from_numpy(np.ascontiguousarray(synth.ultralight_feats(17, 5).reshape(17, 16, 32, 32))).cuda()

    def run(label, shape, call):
        """shape: [(avatar, first bank frame, frames)]; call(reqs) runs them -> the label and three hashes of all returned frames"""
        preds = [torch.zeros(n, 160, 160, 3, dtype=torch.uint8, device="cuda") for _, _, n in shape]
        reqs = [(a, idx, n, feat.data_ptr(), p.data_ptr()) for (a, idx, n), p in zip(shape, preds)]
        hashes = []
        for _ in range(3):
            for p in preds:
                p.zero_()
            call(reqs)
            h = hashlib.sha256()
            for p in preds:
                h.update(p.cpu().numpy().tobytes())
            hashes.append(h.hexdigest())
        print(f"{label:44s} " + " ".join(hashes), flush=True)

    for B in (1, 3, 17):
        for knob in (0, 1):
            Engine.set_knob("UL_FUSE_IR", knob)
            run(f"infer B = {B:2d} UL_FUSE_IR {knob}", [(aids[0], 3, B)], eng.ultralight_infer)
    Engine.set_knob("UL_FUSE_IR", 0)
    run("merged mode 1, one avatar 1 + 2 + 3 frames", [(aids[0], 0, 1), (aids[0], 2, 2), (aids[0], 4, 3)], lambda r: eng.ultralight_infer_merged(r, mode=1))
    two = [(aids[0], 1, 2), (aids[1], 2, 1)]
    run("merged mode 0, two avatars x (2, 1) frames", two, lambda r: eng.ultralight_infer_merged(r, mode=0))
    run("merged mode 2, two avatars x (2, 1) frames", two, lambda r: eng.ultralight_infer_merged(r, mode=2))

    if args.time_register > 0:
        sd = synth.ultralight_state_dict(1234)
        frames, faces, coords = synth.ultralight_avatar(5, (96, 128), seed=40)
        ms = []
        for _ in range(args.time_register):
            t0 = time.perf_counter()
            aid = eng.register_ultralight_avatar(sd, faces, frames, coords, max_frames=17)
            ms.append((time.perf_counter() - t0) * 1e3)
            eng.release_avatar(aid)
        print(f"# register_ultralight_avatar: median of {len(ms)} = {statistics.median(ms):.2f} ms ({min(ms):.2f} .. {max(ms):.2f})")
    eng.close()


if __name__ == "__main__":
    main()
