#!/usr/bin/env python3
"""First-run check of the REAL HuBERT-large checkpoint on the deployment box (GPU + transformers + the checkpoint).

The build container has no checkpoint, so HuBERT-large on the engine (csrc/hubert.hip) is validated there on seeded weights
(tests/test_hubert_gpu.py).  What seeded weights cannot show is the range of the real model's residual stream over 24 layers in
fp16: nobody has measured it.  This script closes that where the real files exist.  Run it from the LiveTalking checkout, once,
before setting LTK_HUBERT_ENGINE=1:

    python /path/to/repo/scripts/verify_hubert_checkpoint.py [--model ./models/hubert-large-ls960-ft] [--seconds 6] [--wav file.wav]

1. loads HubertModel.from_pretrained(model) and hands its state dict to Engine.load_hubert (a missing tensor or a wrong shape
   ends here with the engine's message);
2. runs `--seconds` of audio (16 kHz mono from --wav, else a seeded speech-like signal) through get_hubert_from_16k_speech on the
   engine as ONE call under the fp16 headroom watch (Engine.health_watch("hubert", 1): all its clips count into the model's
   table), and through the same model in torch fp32 on the CPU;
3. reports rel L2 of the (T, 1024) features, the largest |feature| of both, and the watch's line (livetalking_amd/health.py): the op
   with the least headroom, or every op with values clamped at the fp16 limit / non-finite values.
Exit code 0 only if rel L2 <= 2e-2 and both totals over the ops (at the limit, non-finite) are 0.  The fp16 rounding model of tests/hubert_ref.py sits at 1.5e-3 on seeded
24-layer weights; 2e-2 leaves an order of magnitude over that for weights nobody has run here.  It is a first-run gate, not a parity
bound: report the figure it prints.
"""
import argparse
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)


def speech(n, seed=0):
    rng = np.random.default_rng(seed)
    t = np.arange(n) / 16000.0
    x = sum(a * np.sin(2 * np.pi * f * t + p) for a, f, p in zip((0.3, 0.2, 0.1), (140.0, 410.0, 2300.0), rng.uniform(0, 6.28, 3)))
    return ((0.55 + 0.45 * np.sin(2 * np.pi * 3.1 * t)) * x + 0.02 * rng.standard_normal(n)).astype(np.float32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--model", default="./models/hubert-large-ls960-ft")
    ap.add_argument("--seconds", type=float, default=6.0)
    ap.add_argument("--wav")
    args = ap.parse_args()
    os.environ.setdefault("LTK_ALLOW_STANDIN", "1")
    import torch
    from transformers import HubertModel
    from livetalking_amd import health
    from livetalking_amd.engine import Engine
    if not torch.cuda.is_available():
        sys.exit("needs a GPU")
    if args.wav:
        import soundfile as sf
        pcm, sr = sf.read(args.wav, dtype="float32")
        if sr != 16000:
            sys.exit(f"{args.wav} is at {sr} Hz; 16 kHz is what the plugin feeds")
        pcm = pcm[:, 0] if pcm.ndim == 2 else pcm
        pcm = pcm[: int(args.seconds * 16000)]
    else:
        pcm = speech(int(args.seconds * 16000))
    model = HubertModel.from_pretrained(args.model).eval()
    sd = model.state_dict()
    layers = len({k.split(".")[2] for k in sd if k.startswith("encoder.layers.")})
    print(f"[hubert] {args.model}: {len(sd)} tensors, {layers} encoder layers, {len(pcm)} samples")

    eng = Engine(0)
    try:
        eng.load_hubert(sd)
        eng.health_watch("hubert", 1)
        got = eng.hubert_features(pcm)
        ops, seen, _ = eng.health_report("hubert")
    finally:
        eng.close()
    at_limit, non_finite = sum(o["at_limit"] for o in ops), sum(o["nonfinite"] for o in ops)

    x = pcm.astype(np.float64)
    x = ((x - x.mean()) / np.sqrt(x.var() + 1e-7)).astype(np.float32)
    with torch.no_grad():
        ref = model(torch.from_numpy(x)[None]).last_hidden_state[0].numpy()
    ref = ref[: got.shape[0]]
    rel = float(np.linalg.norm(got[: ref.shape[0]].astype(np.float64) - ref) / np.linalg.norm(ref))
    print(f"[hubert] {got.shape[0]} rows: rel L2 engine vs torch fp32 {rel:.3e}; max |feature| engine {np.abs(got).max():.2f}, torch {np.abs(ref).max():.2f}")
    print("[hubert] " + health.format_line("hubert", ops, seen)[1])
    ok = rel <= 2e-2 and at_limit == 0 and non_finite == 0
    print("[hubert] OK" if ok else "[hubert] FAILED: keep LTK_HUBERT_ENGINE unset")
    sys.exit(0 if ok else 1)


if __name__ == "__main__":
    main()
