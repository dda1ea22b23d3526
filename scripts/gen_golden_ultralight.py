#!/usr/bin/env python3
"""Generate tests/golden/ultralight_golden.npz by running the REFERENCE's own Model(6, 'hubert').

TEST INFRASTRUCTURE ONLY.   python scripts/gen_golden_ultralight.py [--ref <LiveTalking checkout>]

The reference's avatars/ultralight/unet.py is loaded from the checkout (default: $LTK_REFERENCE or /root/reference; it does
not exist on the GPU box, which is why its outputs are stored), given synth_inputs.ultralight_state_dict(1234) and run in
float32 - the reference's own precision - on synth_inputs.ultralight_inputs(2, 1234).  The file holds the seeds, the B = 2
frames as the plugin would hand them on ((pred * 255).astype(uint8), ultralight_avatar.py:170,181) and six module outputs
(inc, down2, down4, the audio tower, fuse_conv, up2), each sampled at 4096 fixed pseudo-random positions so that the file
stays small (the positions are stored).  tests/test_ultralight_host.py compares tests/ultralight_ref.py in float64 against
it, and re-derives it when the checkout is present.

Also writes tests/golden/hubert_chunks_golden.npz: the reference's own BaseASR._feature2chunks (base_asr.py:91-156) with
HubertASR's arguments (hubert.py:43-45) on seeded feature arrays.
"""
from __future__ import annotations

import argparse
import importlib.util
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

SEED = 1234
BATCH = 2
N_SAMPLES = 4096
# golden key -> (module path in the reference's Model, tap name of tests/ultralight_ref.py)
TAPS = {
    "inc": ("inc", "inc.inconv.0.conv.6"),
    "down2": ("down2", "down2.maxpool_conv.0.double_conv.1.conv.6"),
    "down4": ("down4", "down4.maxpool_conv.0.double_conv.1.conv.6"),
    "audio": ("audio_model", "audio_model.conv7.conv.6"),
    "fuse_conv": ("fuse_conv", "fuse_conv.1.double_conv.1.conv.6"),
    "up2": ("up2", "up2.conv.double_conv.1.conv.6"),
}


def sample_positions(key: str, size: int) -> np.ndarray:
    rng = np.random.default_rng([SEED, sum(key.encode())])
    return np.sort(rng.choice(size, size=min(N_SAMPLES, size), replace=False)).astype(np.int64)


def generate(ref: str) -> dict:
    import torch
    import synth_inputs as synth
    spec = importlib.util.spec_from_file_location("ltk_ref_ultralight_unet", os.path.join(ref, "avatars", "ultralight", "unet.py"))
    unet = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(unet)
    net = unet.Model(6, "hubert").eval()
    net.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in synth.ultralight_state_dict(SEED).items()})
    img6, feat = synth.ultralight_inputs(BATCH, SEED)
    got = {}
    hooks = [getattr(net, mod).register_forward_hook(lambda m, i, o, key=key: got.__setitem__(key, o.detach().numpy().copy()))
             for key, (mod, _) in TAPS.items()]
    with torch.no_grad():
        pred = net(torch.from_numpy(img6), torch.from_numpy(feat))
    for h in hooks:
        h.remove()
    out = {"seed": np.asarray(SEED), "batch": np.asarray(BATCH),
           "frames": (pred.numpy().transpose(0, 2, 3, 1) * 255.).astype(np.uint8)}
    for key in TAPS:
        pos = sample_positions(key, got[key].size)
        out["pos_" + key] = pos
        out["shape_" + key] = np.asarray(got[key].shape, dtype=np.int64)
        out["tap_" + key] = got[key].reshape(-1)[pos].astype(np.float32)
    return out


def reference_feature2chunks(ref: str):
    """The reference's own BaseASR._feature2chunks (avatars/audio_features/base_asr.py:91-156), bound to a bare object: the
    module itself imports cv2 / av through base_avatar, so the two methods are compiled from its source."""
    import ast
    path = os.path.join(ref, "avatars", "audio_features", "base_asr.py")
    tree = ast.parse(open(path, encoding="utf-8").read())
    cls = next(n for n in tree.body if isinstance(n, ast.ClassDef) and n.name == "BaseASR")
    keep = [n for n in cls.body if isinstance(n, ast.FunctionDef) and n.name in ("_get_sliced_feature", "_feature2chunks")]
    ns = {"np": np}
    cls.name, cls.bases, cls.keywords, cls.decorator_list, cls.body = "_Slicer", [], [], [], keep
    exec(compile(ast.Module(body=[cls], type_ignores=[]), path, "exec"), ns)
    return ns["_Slicer"]()._feature2chunks


# (rows of the feature array, batch_size, stride_left_size): a step's usual geometry (l = r = 10, 2B + 20 chunks of 20 ms) and
# two short arrays on which the window leaves the array at the left / right end
HUBERT_CASES = {"step": (27, 4, 10), "left": (12, 3, 0), "right": (20, 8, 10)}


def hubert_features(rows: int, seed: int) -> np.ndarray:
    return (np.random.default_rng(seed).integers(-128, 128, (rows, 1024)) / 16.0).astype(np.float32)


def generate_hubert(ref: str) -> dict:
    f2c = reference_feature2chunks(ref)
    out = {}
    for i, (name, (rows, batch, left)) in enumerate(HUBERT_CASES.items()):
        feat = hubert_features(rows, SEED + i)
        chunks = f2c(feature_array=feat, batch_size=batch, audio_feat_win=[4, 4], start=left / 2, feature_idx_multiplier=2)
        out[name] = np.stack(chunks).astype(np.float32)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ref", default=os.environ.get("LTK_REFERENCE", "/root/reference"))
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "ultralight_golden.npz"))
    args = ap.parse_args()
    data = generate(args.ref)
    np.savez_compressed(args.out, **data)
    print(f"wrote {args.out}: {os.path.getsize(args.out)} bytes, frames {data['frames'].shape}")
    hub = os.path.join(os.path.dirname(args.out), "hubert_chunks_golden.npz")
    np.savez_compressed(hub, **generate_hubert(args.ref))
    print(f"wrote {hub}: {os.path.getsize(hub)} bytes")


if __name__ == "__main__":
    main()
