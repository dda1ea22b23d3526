#!/usr/bin/env python3
"""Ultralight frame parity record (profiles/ultralight_parity.txt): for seeds 1234 / 7 / 99 of the synthetic weights, B = 2, the
fp16 rounding model of the reference (tests/ultralight_ref.py, CPU) and the device (Engine.ultralight_infer), each against the
float64 frames: max LSB, PSNR, share of differing bytes.  tests/test_ultralight_gpu.py asserts the same comparison."""
import os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np, torch
import synth_inputs as synth, ultralight_ref as ref
from livetalking_amd.engine import Engine
eng = Engine(0)
print("seed   | fp16 rounding model vs float64        | device (ultralight_infer) vs float64")
print("       | max LSB   PSNR dB   bytes differing    | max LSB   PSNR dB   bytes differing")
for seed in (1234, 7, 99):
    sd = synth.ultralight_state_dict(seed)
    faces = synth.ultralight_faces(2, seed)
    img6, feat = synth.ultralight_inputs(2, seed)
    want = ref.frames_u8(ref.forward(sd, img6, feat))
    model = ref.frames_u8(ref.forward(sd, img6, feat, fp16_model=True))
    frames, _, coords = synth.ultralight_avatar(2, (120, 200), seed=3)
    aid = eng.register_ultralight_avatar(sd, faces, frames, coords, max_frames=2)
    d_feat = torch.from_numpy(feat).cuda()
    d_pred = torch.zeros(2, 160, 160, 3, dtype=torch.uint8, device="cuda")
    eng.ultralight_infer([(aid, 0, 2, d_feat.data_ptr(), d_pred.data_ptr())])
    m, d = ref.frame_stats(model, want), ref.frame_stats(d_pred.cpu().numpy(), want)
    print(f"{seed:6d} | {m[0]:7d} {m[1]:9.2f} {100 * m[2]:12.2f} %      | {d[0]:7d} {d[1]:9.2f} {100 * d[2]:12.2f} %", flush=True)
    eng.release_avatar(aid)
eng.close()
