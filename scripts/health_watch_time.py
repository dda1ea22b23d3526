#!/usr/bin/env python3
"""What the headroom watch costs (include/ltk.h: ltk_health_watch), in one MI355X job -> profiles/health_watch.txt.

Per program, on seeded weights: the wall time of one inference call before a watch is armed (steady state: its graph captured), of
a watched call at the same size, and of the calls after the window has closed.  Sizes: 16 frames for Wav2Lip, Ultralight and
MuseTalk, one live step for the Whisper and HuBERT encoders.  The watched call's overhead has no threshold - it is a diagnostic
that runs for the first N calls of a deployment; what must hold is the last column: the call after the window costs what the call
before arming cost.

    python scripts/health_watch_time.py [--reps 20] [--hubert-layers 24] > profiles/health_watch.txt
"""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def measure(call, arm, reps):
    """(before, watched, after) median milliseconds of call(i)."""
    import torch

    def timed(i):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        call(i)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3

    i = 0
    for _ in range(6):                       # eager, capture, replay; a Wav2Lip session's prefetch slots and their graphs
        timed(i); i += 1
    before = [timed(i + k) for k in range(reps)]; i += reps
    arm(reps)
    watched = [timed(i + k) for k in range(reps)]; i += reps
    for _ in range(6):                       # a Wav2Lip session finds its prefetch again within these
        timed(i); i += 1
    after = [timed(i + k) for k in range(reps)]
    return statistics.median(before), statistics.median(watched), statistics.median(after)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--frames", type=int, default=16)
    ap.add_argument("--hubert-layers", type=int, default=24)
    a = ap.parse_args()
    import numpy as np
    import torch
    import hubert_ref as H
    import synth_inputs as synth
    from livetalking_amd.engine import Engine
    B = a.frames
    rows = []
    audio = synth.synthetic_audio(4.0)

    eng = Engine(0)
    eng.load_wav2lip(synth.wav2lip_state_dict(1234), max_frames=B)
    frames, faces, coords = synth.wav2lip_avatar(n_frames=8, full_hw=(360, 640), box=160, seed=0)
    aid = eng.register_avatar(faces, frames, coords)
    d_mel = torch.randn(B, 80, 16, device="cuda")
    d_pred = torch.zeros(B, 256, 256, 3, dtype=torch.uint8, device="cuda")
    rows.append((f"wav2lip, {B} frames", measure(lambda i: eng.wav2lip_infer([(aid, i * B, B, d_mel.data_ptr(), d_pred.data_ptr())]),
                                                   lambda n: eng.health_watch("wav2lip", n), a.reps), eng.prefetch_stats()))
    eng.close()

    eng = Engine(0)
    eng.load_musetalk(synth.musetalk_unet_state_dict(4321), synth.vae_decoder_state_dict(987), max_frames=B)
    eng.load_whisper(synth.whisper_encoder_state_dict())
    lats = synth.musetalk_latents(4)
    mframes, _, _ = synth.wav2lip_avatar(n_frames=4, full_hw=(360, 640), box=160, seed=2)
    box, crop = (240, 100, 390, 270), (210, 60, 420, 305)
    mask = np.full((crop[3] - crop[1], crop[2] - crop[0], 3), 255, np.uint8)
    maid = eng.register_musetalk_avatar(lats, mframes, [box] * 4, [mask] * 4, [crop] * 4)
    d_feat = torch.from_numpy(synth.musetalk_whisper_feats(B, seed=21)).cuda()
    rows.append((f"musetalk, {B} frames", measure(lambda i: eng.musetalk_infer([(maid, i * B, B, d_feat.data_ptr(), d_pred.data_ptr())]),
                                                    lambda n: eng.health_watch("musetalk", n), a.reps), None))
    wav = audio[: (20 + 2 * B) * 320]
    rows.append(("whisper, one step", measure(lambda i: eng.whisper_step(wav, B, 10, d_feat.data_ptr(), row_step=2, rows=10),
                                              lambda n: eng.health_watch("whisper", n), a.reps), None))
    eng.close()

    eng = Engine(0)
    eng.load_hubert(H.state_dict(a.hubert_layers, 20))
    uframes, ufaces, ucoords = synth.ultralight_avatar(4, (360, 640), seed=11)
    uaid = eng.register_ultralight_avatar(synth.ultralight_state_dict(1234), ufaces, uframes, ucoords, max_frames=B)
    d_uf = torch.from_numpy(synth.ultralight_feats(B, 30).reshape(B, 16, 32, 32)).cuda()
    d_up = torch.zeros(B, 160, 160, 3, dtype=torch.uint8, device="cuda")
    rows.append((f"ultralight, {B} frames", measure(lambda i: eng.ultralight_infer([(uaid, i * B, B, d_uf.data_ptr(), d_up.data_ptr())]),
                                                      lambda n: eng.health_watch("ultralight", n, uaid), a.reps), None))
    pcm = H.speech(16640, 9)
    d_hf = torch.zeros(B, 16, 1024, device="cuda")
    rows.append((f"hubert ({a.hubert_layers} layers), one step", measure(lambda i: eng.hubert_step(pcm, B, 2, d_hf.data_ptr()),
                                                                       lambda n: eng.health_watch("hubert", n), a.reps), None))
    eng.close()

    print(f"# headroom watch: wall milliseconds per engine call, median of {a.reps} (scripts/health_watch_time.py), {torch.cuda.get_device_name(0)}")
    print("# before = steady state before the watch is armed; watched = inside the window (eager launches + one scan per op);")
    print("# after = steady state behind the window.  The watched call has no threshold: it is a diagnostic.")
    print(f"# {'program':<32}{'before':>10}{'watched':>10}{'after':>10}{'watched/before':>16}{'after/before':>14}")
    for name, (b, w, af), extra in rows:
        print(f"  {name:<32}{b:>10.3f}{w:>10.3f}{af:>10.3f}{w / b:>16.2f}{af / b:>14.3f}" + (f"   prefetch {extra}" if extra else ""))
    return 0


if __name__ == "__main__":
    sys.exit(main())
