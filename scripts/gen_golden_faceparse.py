#!/usr/bin/env python3
"""Generate tests/golden/faceparse_golden.npz and tests/golden/faceparse_key_manifest.json by running the REFERENCE's own BiSeNet.

    python scripts/gen_golden_faceparse.py [--reference /path/to/LiveTalking]

The reference's avatars/musetalk/utils/face_parsing package is loaded from the checkout (default: $LTK_REFERENCE or /root/reference) under
a private package name, with empty stand-ins for `torchvision`, `torchvision.transforms` and `cv2` (the network needs none of them; the
package imports them for FaceParsing's pre- and post-processing, which this script does not call).  Resnet18.init_weight wants a
ResNet-18 file: the seeded `cp.resnet.*` tensors, written to a temporary directory.  The seeded state dict
(synth_inputs.faceparse_state_dict) is then loaded STRICTLY - its key set has to equal BiSeNet.state_dict()'s - and the network runs in
float64 on synth_inputs.faceparse_image: net(img)[0] is taken apart by a forward hook on `conv_out` into the 19 logits before the
upsample, and `out.argmax(0)` as face_parsing/__init__.py:89-90 forms the labels.

Then the reference's own FaceParsing.__call__ (all three modes) and blending.get_image_prepare_material run on that network (in float64,
model_init replaced by the seeded net) with `cv2` standing for the numpy restatements of livetalking_amd/avatar_prep.py and
`torchvision.transforms` for three lines that do what ToTensor / Normalize / Compose do: that pins the CONTROL FLOW of the host mask
code to the reference; the OpenCV leaves stay unpinned.

The file holds: seed, sizes, per case (size 64 x 3 images, 96 x 3, 512 x 1) the logits (float64; float32 at 512) and the uint8 labels;
mask_raw / mask_neck / mask_jaw of the 512 x 512 image (cheek widths 90, as genavatar.py's v15 branch); prep_box and per mode
prep_mask_<mode> and prep_crop_box: one get_image_prepare_material call each on prep_frame() (regenerated, not stored).  The script asserts that classes 1, 10, 11, 12
and 13 each win at least 2 % of the 512 x 512 image: without that the mask modes test nothing.
The manifest: name -> shape of every key of BiSeNet.state_dict().  No program text of the reference is written anywhere.
tests/test_faceparse_host.py holds tests/faceparse_ref.py to the file, and re-derives it from the checkout when that is present.
"""
from __future__ import annotations

import argparse
import importlib.util
import json
import os
import sys
import tempfile
import types

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

SEED = 83
CASES = ((64, 3), (96, 3), (512, 1))
MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)


def _stand_ins():
    """cv2 = the restatements of livetalking_amd/avatar_prep.py; torchvision.transforms = ToTensor / Normalize / Compose in float64"""
    import torch
    from livetalking_amd import avatar_prep as A
    cv2 = types.ModuleType("cv2")
    cv2.MORPH_ELLIPSE = 2
    cv2.getStructuringElement = lambda shape, ksize: A.ellipse_kernel(ksize[0], ksize[1])
    cv2.dilate = lambda img, k, iterations=1: A.dilate(img, k, iterations)
    cv2.erode = lambda img, k, iterations=1: A.erode(img, k, iterations)
    cv2.rectangle = lambda img, p1, p2, color, thickness: A.filled_rectangle(img, p1, p2, color)
    cv2.GaussianBlur = lambda img, ksize, sigma: A.gaussian_blur_u8(img, ksize[0])
    cv2.bitwise_and = lambda a, b: a & b
    cv2.bitwise_or = lambda a, b: a | b
    tv, tr = types.ModuleType("torchvision"), types.ModuleType("torchvision.transforms")
    tr.ToTensor = lambda: (lambda im: torch.from_numpy(np.array(im.convert("RGB"))).permute(2, 0, 1).double() / 255.0)
    tr.Normalize = lambda m, s: (lambda t: (t - torch.tensor(m, dtype=t.dtype).view(3, 1, 1)) / torch.tensor(s, dtype=t.dtype).view(3, 1, 1))

    def compose(fs):
        def run(x):
            for f in fs:
                x = f(x)
            return x
        return run
    tr.Compose = compose
    tv.transforms = tr
    return {"cv2": cv2, "torchvision": tv, "torchvision.transforms": tr}


def _load(reference: str, rel: str, name: str, package: bool):
    """A module or package of the checkout under a private name, imported with the stand-ins in sys.modules and nothing left behind."""
    saved = {k: sys.modules.get(k) for k in ("cv2", "torchvision", "torchvision.transforms")}
    sys.modules.update(_stand_ins())
    path = os.path.join(reference, *rel.split("/"))
    spec = importlib.util.spec_from_file_location(name, os.path.join(path, "__init__.py") if package else path,
                                                  submodule_search_locations=[path] if package else None)
    mod = importlib.util.module_from_spec(spec)
    sys.modules[name] = mod
    try:
        spec.loader.exec_module(mod)
    finally:                                  # whoever imports cv2 afterwards finds what it found before
        for k, v in saved.items():
            if v is None:
                sys.modules.pop(k, None)
            else:
                sys.modules[k] = v
        for m in [m for m in sys.modules if m.startswith(name)]:
            sys.modules.pop(m, None)
    return mod


def load_reference_bisenet(reference: str):
    """-> the reference's BiSeNet class"""
    return _load(reference, "avatars/musetalk/utils/face_parsing", "ltk_ref_face_parsing", True).BiSeNet


def reference_net(reference: str, sd: dict):
    """-> (the reference's face_parsing package, its BiSeNet with the seeded weights loaded strictly, float64, eval)"""
    import torch
    pkg = _load(reference, "avatars/musetalk/utils/face_parsing", "ltk_ref_face_parsing", True)
    tsd = {k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()}
    with tempfile.TemporaryDirectory() as d:
        path = os.path.join(d, "resnet18.pth")
        torch.save({k[len("cp.resnet."):]: v for k, v in tsd.items() if k.startswith("cp.resnet.")}, path)
        net = pkg.BiSeNet(resnet_path=path)
    net.load_state_dict(tsd, strict=True)
    return pkg, net.double().eval()


PREP_BOX = (150, 110, 290, 280)
MODES = ("raw", "neck", "jaw")


def prep_frame():
    import synth_inputs as synth
    return np.ascontiguousarray(synth.faceparse_image(448, seed=5)[:400, :, ::-1])       # BGR, 400 x 448


def reference_masks(reference: str, sd: dict, image_rgb: np.ndarray):
    """The reference's FaceParsing (cheek widths 90) and get_image_prepare_material on the seeded net -> dict of arrays"""
    from PIL import Image
    pkg, net = reference_net(reference, sd)
    pkg.FaceParsing.model_init = lambda self, *a, **k: net
    fp = pkg.FaceParsing(left_cheek_width=90, right_cheek_width=90)
    blending = _load(reference, "avatars/musetalk/utils/blending.py", "ltk_ref_blending", False)
    frame = prep_frame()
    out = {"prep_box": np.asarray(PREP_BOX)}
    for mode in MODES:
        out[f"mask_{mode}"] = np.asarray(fp(Image.fromarray(image_rgb), mode=mode))
        mask, crop_box = blending.get_image_prepare_material(frame, list(PREP_BOX), fp=fp, mode=mode)
        out[f"prep_mask_{mode}"] = mask
        out["prep_crop_box"] = np.asarray(crop_box)
    return out


def reference_outputs(reference: str, sd: dict, images: np.ndarray):
    """-> (logits (N, 19, S/8, S/8) float64, labels (N, S, S) uint8, {key: shape} of BiSeNet.state_dict())"""
    import torch
    BiSeNet = load_reference_bisenet(reference)
    tsd = {k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()}
    with tempfile.TemporaryDirectory() as d:
        path = os.path.join(d, "resnet18.pth")
        torch.save({k[len("cp.resnet."):]: v for k, v in tsd.items() if k.startswith("cp.resnet.")}, path)
        net = BiSeNet(resnet_path=path)
    manifest = {k: list(v.shape) for k, v in net.state_dict().items()}
    net.load_state_dict(tsd, strict=True)
    net = net.double().eval()
    kept = []
    handle = net.conv_out.register_forward_hook(lambda m, i, o: kept.append(o.detach()))
    x = torch.from_numpy(images).permute(0, 3, 1, 2).double() / 255.0
    x = (x - torch.tensor(MEAN, dtype=torch.float64).view(1, 3, 1, 1)) / torch.tensor(STD, dtype=torch.float64).view(1, 3, 1, 1)
    with torch.no_grad():
        out = net(x)[0]
    handle.remove()
    labels = np.stack([o.numpy().argmax(0) for o in out]).astype(np.uint8)
    return kept[0].numpy(), labels, manifest


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", default=os.environ.get("LTK_REFERENCE", "/root/reference"))
    args = ap.parse_args()
    import synth_inputs as synth
    sd = synth.faceparse_state_dict(SEED)
    out = {"seed": np.asarray(SEED), "sizes": np.asarray([c[0] for c in CASES]), "counts": np.asarray([c[1] for c in CASES])}
    manifest = None
    for size, n in CASES:
        rgb = np.stack([synth.faceparse_image(size, seed=i) for i in range(n)])
        logits, labels, manifest = reference_outputs(args.reference, sd, rgb)
        out[f"logits_{size}"] = logits.astype(np.float32 if size == 512 else np.float64)
        out[f"labels_{size}"] = labels
        share = {int(c): round(float((labels == c).mean()), 3) for c in np.unique(labels)}
        print(f"size {size} x {n}: logits {logits.shape}, max |logit| {np.abs(logits).max():.2f}, classes {share}")
        if size == 512:
            for c in (1, 10, 11, 12, 13):
                assert share.get(c, 0.0) >= 0.02, f"class {c} wins {share.get(c, 0.0):.3f} of the 512 x 512 image: choose another seed / gains"
            masks = reference_masks(args.reference, sd, rgb[0])
            for mode in MODES:
                print(f"mode {mode}: {float((masks['mask_' + mode] == 255).mean()):.3f} of the mask set; prepare material {masks['prep_mask_' + mode].shape}, "
                      f"crop box {masks['prep_crop_box'].tolist()}, mean {masks['prep_mask_' + mode].mean():.1f}")
            out.update(masks)
    gold = os.path.join(ROOT, "tests", "golden")
    np.savez_compressed(os.path.join(gold, "faceparse_golden.npz"), **out)
    with open(os.path.join(gold, "faceparse_key_manifest.json"), "w") as f:
        json.dump(manifest, f, indent=0, sort_keys=True)
    print(f"wrote faceparse_golden.npz ({os.path.getsize(os.path.join(gold, 'faceparse_golden.npz'))} bytes), {len(manifest)} keys in the manifest")


if __name__ == "__main__":
    main()
