#!/usr/bin/env python3
"""First-run check of a deployment's checkpoints: does any activation reach the limit of fp16 (or e4m3) on this engine?

The conv epilogues clamp to +-65504 and nothing reports it; every parity figure of this repository rests on
seeded synthetic weights.  This tool loads what it finds, runs N watched calls per program (include/ltk.h: ltk_health_watch) on
synth_inputs.synthetic_audio, prints every op's counters and exits non-zero when any op has values AT the limit of its type
(`at limit` > 0) or non-finite values (`nonfinite` > 0).  `near` - finite values in the top binade, still exact - is printed as the
margin and does not fail the run on its own.  It sits beside verify_musetalk_checkpoint.py and verify_hubert_checkpoint.py (which compare
numerics against the reference's own load path); this one needs nothing but the checkpoints.

    python scripts/checkpoint_health.py [--calls 4] [--batch 16]             # ./models and ./data/avatars of the deployment
    python scripts/checkpoint_health.py --synthetic [--hubert-layers 2]      # seeded weights: checks the tool itself

What it looks for (the reference's layout): models/wav2lip.pth; models/musetalkV15/unet.pth + models/sd-vae + models/whisper;
models/hubert-large-ls960-ft; data/avatars/*/ultralight.pth (every Ultralight avatar has its own U-Net).
"""
import argparse
import glob
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))       # --synthetic: the seeded HuBERT draw lives with the tests


def _report(eng, program, avatar_id=-1, label=None):
    from livetalking_amd import health
    ops, seen, left = eng.health_report(program, avatar_id)
    print(health.format_table(label or program, ops))
    clean, line = health.format_line(label or program, ops, seen)
    print(line + "\n")
    return 0 if clean else 1


def check_wav2lip(sd, calls, B, audio):
    import torch
    import synth_inputs as synth
    from livetalking_amd.engine import Engine
    from oracle import mel_oracle
    frames, faces, coords = synth.wav2lip_avatar(n_frames=8, full_hw=(360, 640), box=160, seed=0)
    eng = Engine(0)
    try:
        eng.load_wav2lip(sd, max_frames=B)
        aid = eng.register_avatar(faces, frames, coords)
        eng.health_watch("wav2lip", calls)
        d_mel = torch.zeros(B, 80, 16, device="cuda")
        d_pred = torch.zeros(B, 256, 256, 3, dtype=torch.uint8, device="cuda")
        for c in range(calls):
            n_chunks = 20 + 2 * B
            wav = audio[c * 2 * B * 320: (c * 2 * B + n_chunks) * 320]
            eng.mel_step(wav, mel_oracle.window_starts(n_chunks, 10, 10), d_mel.data_ptr())
            eng.wav2lip_infer([(aid, c * B, B, d_mel.data_ptr(), d_pred.data_ptr())])
        return _report(eng, "wav2lip")
    finally:
        eng.close()


def check_musetalk(unet_sd, vae_sd, whisper_sd, calls, B, audio):
    import torch
    import synth_inputs as synth
    from livetalking_amd.engine import Engine
    eng = Engine(0)
    try:
        eng.load_musetalk(unet_sd, vae_sd, max_frames=B, fp8=os.environ.get("LTK_MT_FP8", "0") not in ("", "0"))
        eng.load_whisper(whisper_sd)
        lats = synth.musetalk_latents(4)
        frames, _, _ = synth.wav2lip_avatar(n_frames=4, full_hw=(360, 640), box=160, seed=2)
        box, crop = (240, 100, 390, 270), (210, 60, 420, 305)
        mask = np.full((crop[3] - crop[1], crop[2] - crop[0], 3), 255, np.uint8)
        aid = eng.register_musetalk_avatar(lats, frames, [box] * 4, [mask] * 4, [crop] * 4)
        eng.health_watch("musetalk", calls)
        eng.health_watch("whisper", calls)
        d_feat = torch.zeros(B, 50, 384, device="cuda")
        d_pred = torch.zeros(B, 256, 256, 3, dtype=torch.uint8, device="cuda")
        for c in range(calls):
            wav = audio[c * 2 * B * 320: (c * 2 * B + 20 + 2 * B) * 320]
            eng.whisper_step(wav, B, 10, d_feat.data_ptr(), row_step=2, rows=10)
            eng.musetalk_infer([(aid, c * B, B, d_feat.data_ptr(), d_pred.data_ptr())])
        return _report(eng, "whisper") | _report(eng, "musetalk")
    finally:
        eng.close()


def check_ultralight(avatars, hubert_sd, calls, B, audio):
    """avatars: [(label, state_dict)]; hubert_sd None: the features are seeded noise (the reference's HuBERT was not found)."""
    import torch
    import synth_inputs as synth
    from livetalking_amd.engine import Engine
    frames, faces, coords = synth.ultralight_avatar(4, (360, 640), seed=11)
    rc = 0
    eng = Engine(0)
    try:
        if hubert_sd is not None:
            eng.load_hubert(hubert_sd)
            eng.health_watch("hubert", calls)
        d_feat = torch.from_numpy(synth.ultralight_feats(B, 30).reshape(B, 16, 32, 32)).cuda()
        d_pred = torch.zeros(B, 160, 160, 3, dtype=torch.uint8, device="cuda")
        ids = [(label, eng.register_ultralight_avatar(sd, faces, frames, coords, max_frames=B)) for label, sd in avatars]
        for _, aid in ids:
            eng.health_watch("ultralight", calls, aid)
        for c in range(calls):
            if hubert_sd is not None:
                wav = audio[c * 2 * B * 320: (c * 2 * B + 20 + 2 * B) * 320]
                eng.hubert_step(wav, B, 2, d_feat.data_ptr(), row_step=2, rows=16)
            for _, aid in ids:
                eng.ultralight_infer([(aid, c * B, B, d_feat.data_ptr(), d_pred.data_ptr())])
        if hubert_sd is not None:
            rc |= _report(eng, "hubert")
        for label, aid in ids:
            rc |= _report(eng, "ultralight", aid, f"ultralight {label}")
        return rc
    finally:
        eng.close()


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--models", default="./models")
    ap.add_argument("--avatars", default="./data/avatars")
    ap.add_argument("--calls", type=int, default=4, help="watched calls per program")
    ap.add_argument("--batch", type=int, default=16, help="frames per call")
    ap.add_argument("--synthetic", action="store_true", help="seeded weights instead of checkpoints")
    ap.add_argument("--hubert-layers", type=int, default=2, help="--synthetic: encoder layers of the seeded HuBERT")
    a = ap.parse_args()
    import torch
    import synth_inputs as synth
    if not torch.cuda.is_available():
        print("checkpoint_health needs the GPU the deployment runs on", file=sys.stderr)
        return 2
    audio = synth.synthetic_audio(max(4.0, 0.04 * a.batch * (a.calls + 1) + 1.0))
    rc, found = 0, 0
    if a.synthetic:
        import hubert_ref as H
        rc |= check_wav2lip(synth.wav2lip_state_dict(1234), a.calls, a.batch, audio)
        rc |= check_musetalk(synth.musetalk_unet_state_dict(4321), synth.vae_decoder_state_dict(987), synth.whisper_encoder_state_dict(),
                             a.calls, a.batch, audio)
        rc |= check_ultralight([("seed 1234", synth.ultralight_state_dict(1234))], H.state_dict(a.hubert_layers, 20), a.calls, a.batch, audio)
        found = 3
    else:
        w2l = os.path.join(a.models, "wav2lip.pth")
        if os.path.exists(w2l):
            from livetalking_amd.avatars.wav2lip_avatar import _state_dict_from_checkpoint
            rc |= check_wav2lip(_state_dict_from_checkpoint(w2l), a.calls, a.batch, audio)
            found += 1
        unet = os.path.join(a.models, "musetalkV15", "unet.pth")
        if os.path.exists(unet):
            from transformers import WhisperModel
            from livetalking_amd.avatars import musetalk_avatar as mta
            cwd = os.getcwd()
            os.chdir(os.path.dirname(os.path.abspath(a.models)))          # the plugin's readers take ./models
            try:
                vae = mta.convert_deprecated_vae_attention(mta._read_vae_checkpoint())
                vae = {k: v for k, v in vae.items() if k.startswith("decoder.") or k.startswith("post_quant_conv.")}
                wsd = WhisperModel.from_pretrained(os.path.join("models", "whisper")).encoder.state_dict()
                rc |= check_musetalk(torch.load(os.path.join("models", "musetalkV15", "unet.pth"), map_location="cpu"), vae, wsd,
                                     a.calls, min(a.batch, 64), audio)
            finally:
                os.chdir(cwd)
            found += 1
        uls = [(os.path.basename(os.path.dirname(p)), torch.load(p, map_location="cpu"))
               for p in sorted(glob.glob(os.path.join(a.avatars, "*", "ultralight.pth")))]
        if uls:
            hub = os.path.join(a.models, "hubert-large-ls960-ft")
            hsd = None
            if os.path.isdir(hub):
                from transformers import HubertModel
                hsd = HubertModel.from_pretrained(hub).state_dict()
            else:
                print(f"{hub} not found: the Ultralight avatars are fed seeded features, HuBERT is not checked")
            rc |= check_ultralight(uls, hsd, a.calls, min(a.batch, 256), audio)
            found += 1
    if not found:
        print(f"no checkpoint found under {a.models} / {a.avatars}", file=sys.stderr)
        return 2
    print("RESULT:", "every watched op stayed inside its number format" if rc == 0 else "ACTIVATIONS AT THE LIMIT OF THEIR NUMBER FORMAT (see the warnings above)")
    return rc


if __name__ == "__main__":
    sys.exit(main())
