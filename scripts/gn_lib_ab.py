#!/usr/bin/env python3
"""One library's side of an in-job A/B of the GroupNorm kernels between builds of libltk_hip.so (LTK_LIB; scripts/gpu_job.sh gn-ab runs the
libraries as interleaved processes and takes medians over the rounds): the five large-map shapes of profiles/r06_gn_coop_ab.txt and the
U-Net / 32^2 shapes of a 16-frame pass through ltk_groupnorm_f16 (impl 0: what the program launches; impl 1: the two-pass kernels), and
the whole 16-frame MuseTalk pass through ltk_musetalk_time.  One "key us" line per figure.  GPU only.

    LTK_LIB=ab_libs/libltk_hip_parent.so python scripts/gn_lib_ab.py [frames] [iters]
    python scripts/gn_lib_ab.py --summary log          medians per (library, key) of a gn-ab log
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

SHAPES = [(128, 256), (256, 256), (256, 128), (512, 128), (512, 64), (512, 32), (320, 32), (640, 16), (1280, 8)]


def summary(path):
    t, lib, libs, keys = {}, None, [], []
    for ln in open(path):
        w = ln.split()
        if ln.startswith("######## "):
            lib = w[-1]
            if lib not in libs:
                libs.append(lib)
        elif len(w) == 3 and w[0] == "gn-ab" and lib:
            t.setdefault((lib, w[1]), []).append(float(w[2]))
            if w[1] not in keys:
                keys.append(w[1])
    print(f"{'median us over the rounds':34s}" + "".join(f"{os.path.basename(l):>28s}" for l in libs) + "   last vs first   spread of a library's rounds")
    for k in keys:
        med = [float(np.median(t[(l, k)])) for l in libs]
        spread = max((max(t[(l, k)]) - min(t[(l, k)])) / np.median(t[(l, k)]) for l in libs)
        print(f"{k:34s}" + "".join(f"{m:28.1f}" for m in med) + f"   {100 * (med[-1] / med[0] - 1):+12.1f}%   {100 * spread:6.1f}%")


def main():
    if len(sys.argv) > 2 and sys.argv[1] == "--summary":
        return summary(sys.argv[2])
    import torch
    import synth_inputs as synth
    from livetalking_amd.engine import Engine
    from livetalking_amd.layout import empty_cb16, to_cb16
    frames = int(sys.argv[1]) if len(sys.argv) > 1 else 16
    iters = int(sys.argv[2]) if len(sys.argv) > 2 else 20
    eng = Engine(0)
    for C, H in SHAPES:
        x = to_cb16(torch.randn(frames, C, H, H).cuda())
        y = empty_cb16(frames, C, H, H)
        ga, be = np.ones(C, np.float32), np.zeros(C, np.float32)
        for impl in (0, 1):
            eng.groupnorm_f16(x.data_ptr(), frames, C, H * H, 32, 1e-6, ga, be, True, y.data_ptr(), impl=impl, iters=3)
            us = eng.groupnorm_f16(x.data_ptr(), frames, C, H * H, 32, 1e-6, ga, be, True, y.data_ptr(), impl=impl, iters=iters) * 1e3
            print(f"gn-ab gn_{C}ch@{H}^2_impl{impl} {us:.2f}", flush=True)
        del x, y
    eng.load_musetalk(synth.musetalk_unet_state_dict(), synth.vae_decoder_state_dict(), max_frames=frames)
    eng.musetalk_time(frames, 2)
    for i in range(3):
        print(f"gn-ab musetalk_pass_{frames}f {eng.musetalk_time(frames, 5)[0] * 1e3:.1f}", flush=True)
    eng.close()


if __name__ == "__main__":
    main()
