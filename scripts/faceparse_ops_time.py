#!/usr/bin/env python3
"""The face parser's own kernels (csrc/parse_kernels.hip) at the shapes a 512 x 512 BiSeNet forward gives them, N = 1 and 4 images:

    stem 512^2 x 3 -> 256^2 x 64, max pool -> 128^2, global average of 512 ch x 16^2 (feat32) and of 256 ch x 64^2 (FFM),
    gate 512 ch x 16^2 (ARM32, + b), 256 ch x 32^2 (ARM16, + r), 256 ch x 64^2 (FFM, + 1), segmentation head 64^2 -> 512^2

    rocprofv3 --kernel-trace --stats -d OUT -o r -- python scripts/faceparse_ops_time.py --images 1 [--iters 20]
    python scripts/prof_report.py OUT/<host>            # calls, average / min / max us per kernel

The stand-alone hooks upload their operands and synchronise in every call, so host time around them says nothing about the kernels: the
kernel trace is the record (every launch of the list above runs `--iters` times per image count of `--images`).  Beside them, printed by this script from HIP events around
`--iters` back-to-back calls: the same ops in torch fp32 on the same GPU (normalise + conv2d + affine + relu, max_pool2d, mean,
sigmoid gate, interpolate + argmax).  Recorded only: nothing gates on these numbers.
"""
from __future__ import annotations

import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--images", default="1,4", help="the image counts, e.g. 1 or 4 alone for a kernel trace of one of them")
    args = ap.parse_args()
    import numpy as np
    import torch
    import torch.nn.functional as F
    import faceparse_cases as FP
    from livetalking_amd.engine import Engine
    from livetalking_amd.layout import empty_cb16
    if not torch.cuda.is_available():
        sys.exit("needs a GPU: a CPU run measures nothing")
    eng = Engine(0)
    g = torch.Generator(device="cuda").manual_seed(0)

    def cb16(n, c, h, w):
        return (torch.randn(n, c // 16, h, w, 16, device="cuda", generator=g) * 2).half()

    def timed(fn):
        fn()
        torch.cuda.synchronize()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(args.iters):
            fn()
        b.record()
        torch.cuda.synchronize()
        return a.elapsed_time(b) * 1e3 / args.iters

    print(f"# torch fp32 on the same GPU, us per op, mean of {args.iters} back-to-back calls (HIP events)")
    print(f"# {'op':<40}" + "".join(f"{'N=' + v:>10}" for v in args.images.split(",")))
    rows = {}
    counts = [int(v) for v in args.images.split(",")]
    for N in counts:
        c = FP.Stem(1, 512, 512)
        rgb = torch.from_numpy(np.repeat(c.rgb, N, 0)).cuda()
        y = empty_cb16(N, 64, 256, 256)
        p = empty_cb16(N, 64, 128, 128)
        f32, f16_, f8 = cb16(N, 512, 16, 16), cb16(N, 256, 32, 32), cb16(N, 256, 64, 64)
        a512, a256 = cb16(N, 512, 1, 1), cb16(N, 256, 1, 1)
        o32, o16, o8 = torch.empty_like(f32), torch.empty_like(f16_), torch.empty_like(f8)
        logits = cb16(N, 32, 64, 64)
        lab = torch.empty(N, 512, 512, dtype=torch.uint8, device="cuda")
        for _ in range(args.iters):
            eng.parse_stem_f16(rgb.data_ptr(), N, 512, 512, c.w, c.scale, c.shift, y.data_ptr())
            eng.maxpool3x3s2_f16(y.data_ptr(), N, 256, 256, 64, p.data_ptr())
            eng.global_avgpool_f16(f32.data_ptr(), N, 256, 512, a512.data_ptr())
            eng.global_avgpool_f16(f8.data_ptr(), N, 4096, 256, a256.data_ptr())
            eng.chan_gate_f16(f32.data_ptr(), N, 256, 512, a512.data_ptr(), o32.data_ptr(), d_b_ptr=a512.data_ptr())
            eng.chan_gate_f16(f16_.data_ptr(), N, 1024, 256, a256.data_ptr(), o16.data_ptr(), d_r_ptr=f16_.data_ptr())
            eng.chan_gate_f16(f8.data_ptr(), N, 4096, 256, a256.data_ptr(), o8.data_ptr(), plus1=True)
            eng.seg_argmax_f16(logits.data_ptr(), N, 64, 64, lab.data_ptr())
        # the torch side: NCHW fp32
        w = torch.from_numpy(c.w).cuda()
        sc, sf = (torch.from_numpy(t).cuda().view(1, 64, 1, 1) for t in (c.scale, c.shift))
        mean, std = (torch.tensor(t, device="cuda").view(1, 3, 1, 1) for t in (FP.MEAN, FP.STD))
        t_y = torch.randn(N, 64, 256, 256, device="cuda")
        t32, t16, t8 = torch.randn(N, 512, 16, 16, device="cuda"), torch.randn(N, 256, 32, 32, device="cuda"), torch.randn(N, 256, 64, 64, device="cuda")
        ta5, ta2 = torch.randn(N, 512, 1, 1, device="cuda"), torch.randn(N, 256, 1, 1, device="cuda")
        tl = torch.randn(N, 19, 64, 64, device="cuda")
        ops = {
            "stem 512^2 (normalise, conv, bn, relu)": lambda: F.relu(F.conv2d((rgb.permute(0, 3, 1, 2).float() / 255 - mean) / std, w, None, 2, 3) * sc + sf),
            "max pool 256^2 x 64": lambda: F.max_pool2d(t_y, 3, 2, 1),
            "gap 16^2 x 512": lambda: t32.mean((2, 3), keepdim=True),
            "gap 64^2 x 256": lambda: t8.mean((2, 3), keepdim=True),
            "gate 16^2 x 512 (+ b)": lambda: t32 * torch.sigmoid(ta5) + ta5,
            "gate 32^2 x 256 (+ r)": lambda: t16 * torch.sigmoid(ta2) + t16,
            "gate 64^2 x 256 (+ 1)": lambda: t8 * torch.sigmoid(ta2) + t8,
            "seg head 64^2 -> 512^2": lambda: F.interpolate(tl, (512, 512), mode="bilinear", align_corners=True).argmax(1),
        }
        for name, fn in ops.items():
            rows.setdefault(name, []).append(timed(fn))
    for name, v in rows.items():
        print(f"  {name:<40}" + "".join(f"{t:>10.1f}" for t in v))
    eng.close()


if __name__ == "__main__":
    main()
