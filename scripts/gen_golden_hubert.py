#!/usr/bin/env python3
"""Writes tests/golden/hubert_golden.npz: what the reference's own get_hubert_from_16k_speech returns.

avatars/ultralight/audio2feature.py's Audio2Feature.get_hubert_from_16k_speech (the clip loop: normalise over the whole input,
clips of 320 000 samples forwarded with the 80 samples behind them, a tail of at least 400 samples, pad / trim to (n - 80) // 320
rows) is called UNCHANGED on a stand-in object: `processor` is a Wav2Vec2FeatureExtractor() from its constructor (what
Wav2Vec2Processor delegates audio to; do_normalize on), `model` the seeded 2-layer HubertModel of tests/hubert_ref.py in float64
(inputs upcast), so that what is pinned is the method, not float32 noise.  No checkpoint exists in the reference tree or here.

Cases: 1 040 samples (3 rows), 16 640 (51 rows, the live step), 330 000 (one clip of 1 000 rows + a tail of 31; stored as every 8th
column to keep the file small).  tests/test_hubert_host.py regenerates and compares when the reference is present.
"""
import argparse
import importlib.util
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

SEED = 20
CASES = {"n1040": (1040, 1), "n16640": (16640, 1), "n330000": (330000, 8)}       # name -> (samples, column step of what is stored)


def reference_method(ref: str):
    path = os.path.join(ref, "avatars", "ultralight", "audio2feature.py")
    spec = importlib.util.spec_from_file_location("_ref_ultralight_audio2feature", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod.Audio2Feature.get_hubert_from_16k_speech


class _Double:
    """HubertModel in float64 behind the float32 input_values the processor hands out."""

    def __init__(self, model):
        self.m = model

    def forward(self, x):
        return self.m(x.double())

    __call__ = forward


def stand_in(sd):
    import torch
    import types
    from transformers import HubertModel, Wav2Vec2FeatureExtractor
    import hubert_ref as H
    layers = len({k.split(".")[2] for k in sd if k.startswith("encoder.layers.")})
    model = HubertModel(H.config(layers)).double().eval()
    model.load_state_dict({k: torch.as_tensor(v).double() for k, v in sd.items()}, strict=True)
    return types.SimpleNamespace(processor=Wav2Vec2FeatureExtractor(), model=_Double(model), device="cpu"), model


def generate(ref: str, only=None) -> dict:
    import hubert_ref as H
    method = reference_method(ref)
    obj, _ = stand_in(H.state_dict(2, SEED))
    out = {}
    for i, (name, (n, step)) in enumerate(CASES.items()):
        if only and name not in only:
            continue
        feat = method(obj, H.speech(n, SEED + i))
        out[name] = np.ascontiguousarray(feat.numpy()[:, ::step].astype(np.float32))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ref", default=os.environ.get("LTK_REFERENCE", "/root/reference"))
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "hubert_golden.npz"))
    args = ap.parse_args()
    data = generate(args.ref)
    np.savez_compressed(args.out, **data)
    print(f"wrote {args.out}: {os.path.getsize(args.out)} bytes, " + ", ".join(f"{k} {v.shape}" for k, v in data.items()))


if __name__ == "__main__":
    main()
