#!/usr/bin/env python3
"""Generate tests/golden/s3fd_golden.npz and tests/golden/s3fd_key_manifest.json by running the REFERENCE's own S3FD code.

    python scripts/gen_golden_s3fd.py [--reference /path/to/LiveTalking]

From the checkout (default: $LTK_REFERENCE or /root/reference) the files avatars/wav2lip/face_detection/detection/sfd/net_s3fd.py,
bbox.py and detect.py are loaded as the modules of a private package, and avatars/wav2lip/genavatar.py as a private module, with empty
stand-ins for `cv2` (none of the functions called here uses it) and for the `avatars.wav2lip.face_detection` package genavatar.py
imports.  SFDDetector and FaceAlignment are NEVER constructed: their constructors fetch weights from a URL when s3fd.pth is absent.
Called are s3fd(), batch_detect, nms and get_smoothened_boxes; the three lines of SFDDetector.detect_from_batch (sfd_detector.py:42-45)
and the loop of FaceAlignment.get_detections_for_batch (api.py:69-77) are replayed on their outputs.

The seeded state dict (synth_inputs.s3fd_state_dict) is loaded STRICTLY and the network runs in float64 (.double()) on
synth_inputs.s3fd_frame, batched as tests/s3fd_cases.py NET_CASES runs them (chunks of 2: a pair and a short tail).  Stored per case
HxW: heads_<HxW>_<i> (the 12 outputs of s3fd.forward for all the case's images, float64; float32 at 180 x 320), bd_<HxW>_<c> (what
batch_detect returns for chunk c), kept_<HxW>_<n> (image n's rows behind NMS 0.3 and score > 0.5), boxes_<HxW> (the final integer
boxes, -1 where get_detections_for_batch gives None); and one smoothing example: smooth_in / smooth_out (get_smoothened_boxes, T = 5, on
an integer array) with avatar_boxes_<...> = the padded boxes of genavatar.py:107-120 for the 64 x 64 case's predictions.
Only data is stored; no program text of the reference goes anywhere.  The manifest: name -> shape of every key of s3fd().state_dict().

Asserted here, so that the reference alone meets them (tau_s, tau_b: tests/s3fd_cases.py taus(), from the fp16 rounding model):
>= 40 candidates above 0.05 per image, on at least 3 levels; at most 5 % of an image's candidates within tau_s of 0.05; >= 3 boxes
above 0.5 surviving NMS in at least one image; the top score ahead of the second by more than tau_s in every image that has a face;
one image with no score above 0.5.  tests/test_face_detect_host.py holds tests/s3fd_ref.py and livetalking_amd/face_detect.py to the
file, and re-derives it from the checkout when that is present.
"""
from __future__ import annotations

import argparse
import importlib.util
import json
import os
import sys
import types

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

SFD = "avatars/wav2lip/face_detection/detection/sfd"
STUBS = ("cv2", "avatars", "avatars.wav2lip", "avatars.wav2lip.face_detection")


def load_reference(reference: str):
    """-> (net_s3fd, bbox, detect, genavatar) modules of the checkout under private names, nothing left behind in sys.modules."""
    saved = {k: sys.modules.get(k) for k in STUBS}
    for k in STUBS:
        sys.modules[k] = types.ModuleType(k)
    sys.modules["avatars"].wav2lip = sys.modules["avatars.wav2lip"]
    sys.modules["avatars.wav2lip"].face_detection = sys.modules["avatars.wav2lip.face_detection"]
    pkg_name = "ltk_ref_sfd"
    pkg = types.ModuleType(pkg_name)
    pkg.__path__ = []                       # a package with no search path: only what is loaded below can be imported from it
    sys.modules[pkg_name] = pkg
    mods = {}
    try:
        for name in ("net_s3fd", "bbox", "detect"):
            spec = importlib.util.spec_from_file_location(f"{pkg_name}.{name}", os.path.join(reference, *SFD.split("/"), name + ".py"))
            mod = importlib.util.module_from_spec(spec)
            sys.modules[spec.name] = mod
            spec.loader.exec_module(mod)
            mods[name] = mod
        spec = importlib.util.spec_from_file_location("ltk_ref_genavatar", os.path.join(reference, "avatars", "wav2lip", "genavatar.py"))
        gen = importlib.util.module_from_spec(spec)
        stdout = sys.stdout
        sys.stdout = open(os.devnull, "w")                 # the module prints its device on import
        try:
            spec.loader.exec_module(gen)
        finally:
            sys.stdout.close()
            sys.stdout = stdout
    finally:
        for k, v in saved.items():
            if v is None:
                sys.modules.pop(k, None)
            else:
                sys.modules[k] = v
        for m in [m for m in sys.modules if m.startswith(pkg_name)]:
            sys.modules.pop(m, None)
    return mods["net_s3fd"], mods["bbox"], mods["detect"], gen


def reference_net(net_s3fd, sd: dict):
    """-> (the reference's s3fd with the seeded weights loaded strictly, float64, eval; {key: shape} of its state_dict)"""
    import torch
    net = net_s3fd.s3fd()
    manifest = {k: list(v.shape) for k, v in net.state_dict().items()}
    net.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()}, strict=True)
    return net.double().eval(), manifest


def detections(bbox, bboxlists: np.ndarray):
    """sfd_detector.py:42-45 and api.py:69-77 on batch_detect's array -> (kept rows per image, boxes (n, 4) int, -1 = None)"""
    keeps = [bbox.nms(bboxlists[:, i, :], 0.3) for i in range(bboxlists.shape[1])]
    lists = [bboxlists[keep, i, :] for i, keep in enumerate(keeps)]
    lists = [[x for x in bboxlist if x[-1] > 0.5] for bboxlist in lists]
    boxes = []
    for d in lists:
        if len(d) == 0:
            boxes.append((-1, -1, -1, -1))
            continue
        d = np.clip(d[0], 0, None)
        boxes.append(tuple(map(int, d[:-1])))
    return lists, np.asarray(boxes, np.int64)


def case_key(hw):
    return f"{hw[0]}x{hw[1]}"


def reference_case(net, bbox, detect, frames_bgr: np.ndarray, chunk: int = 2) -> dict:
    import torch
    out = {}
    rgb = frames_bgr[..., ::-1]                                    # api.py:65
    with torch.no_grad():
        heads = net(torch.from_numpy((rgb - np.array([104, 117, 123])).transpose(0, 3, 1, 2).copy()).double())
    for i, h in enumerate(heads):
        out[f"heads_{i}"] = h.numpy()
    kept, boxes = [], []
    for c, i0 in enumerate(range(0, len(rgb), chunk)):
        # batch_detect hands the network a float32 tensor (integers, exact): cast at the door, the network itself stays float64
        bd = detect.batch_detect(lambda x: net(x.double()), rgb[i0:i0 + chunk].copy().astype(np.float64), "cpu")
        out[f"bd_{c}"] = np.asarray(bd, np.float64)
        k, b = detections(bbox, bd)
        kept += k
        boxes.append(b)
    for n, k in enumerate(kept):
        out[f"kept_{n}"] = np.asarray(k, np.float64).reshape(-1, 5)
    out["boxes"] = np.concatenate(boxes)
    return out


def smoothing_example(gen, boxes64: np.ndarray, hw) -> dict:
    """get_smoothened_boxes on a seeded integer array, and genavatar.py:107-120 on the 64 x 64 case's predictions (repeated to 7 frames)"""
    rng = np.random.default_rng(7)
    base = np.array([40, 30, 120, 140]) + rng.integers(-9, 10, (9, 4))
    out = {"smooth_in": base.copy(), "smooth_out": gen.get_smoothened_boxes(base.copy(), T=5)}
    preds = [None if b[0] < 0 else tuple(int(v) for v in b) for b in boxes64] * 3
    preds = preds[:7]
    pady1, pady2, padx1, padx2 = 0, 10, 0, 0
    results = []
    for rect in preds:
        if rect is None:
            rect = [0, 0, hw[1], hw[0]]
        results.append([max(0, rect[0] - padx1), max(0, rect[1] - pady1), min(hw[1], rect[2] + padx2), min(hw[0], rect[3] + pady2)])
    out["avatar_pred"] = np.asarray([(-1,) * 4 if p is None else p for p in preds], np.int64)
    out["avatar_boxes"] = gen.get_smoothened_boxes(np.array(results), T=5)
    return out


def assert_conditions(key: str, case: dict, tau_s: float, n_images: int, summary: dict):
    import s3fd_cases as FD
    import s3fd_ref as R
    import torch
    cands = R.candidates([torch.from_numpy(np.asarray(case[f"heads_{i}"], np.float64)) for i in range(12)], FD.THRESH)
    for n in range(n_images):
        keys, rows = cands[n]
        levels = np.unique(keys >> 28)
        near = int((np.abs(rows[:, 4] - FD.THRESH) <= tau_s).sum())
        assert len(keys) >= 40, f"{key} image {n}: {len(keys)} candidates"
        assert len(levels) >= 3, f"{key} image {n}: candidates on levels {levels}"
        assert near <= FD.NEAR_CAP * len(keys), f"{key} image {n}: {near} of {len(keys)} candidates within tau_s of the threshold"
        top = np.sort(rows[:, 4])[::-1]
        kept = case[f"kept_{n}"]
        if len(kept):
            assert top[0] - top[1] > tau_s, f"{key} image {n}: the top two scores are {top[0] - top[1]:.2e} apart, tau_s {tau_s:.2e}"
        summary["most_kept"] = max(summary["most_kept"], len(kept))
        summary["no_face"] += int(top[0] <= 0.5)
        print(f"  image {n}: {len(keys)} candidates on levels {levels.tolist()}, {near} within tau_s, {len(kept)} kept, top {top[0]:.4f} {top[1]:.4f}, "
              f"box {case['boxes'][n].tolist()}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", default=os.environ.get("LTK_REFERENCE", "/root/reference"))
    args = ap.parse_args()
    import torch
    import s3fd_cases as FD
    import s3fd_ref as R
    import synth_inputs as synth
    from livetalking_amd.engine import Engine
    net_s3fd, bbox, detect, gen = load_reference(args.reference)
    sd = synth.s3fd_state_dict(FD.SEED)
    net, manifest = reference_net(net_s3fd, sd)
    sd32 = {k: torch.from_numpy(v) for k, v in sd.items()}
    out = {"seed": np.asarray(FD.SEED)}
    summary = {"most_kept": 0, "no_face": 0}
    for hw, seeds in FD.NET_CASES.items():
        key = case_key(hw)
        frames = FD.frames(hw)
        case = reference_case(net, bbox, detect, frames)
        mod = FD.model_walk(sd32, frames, Engine.face_detect_program(*hw))
        heads = R.walk(FD.state_dict(), R.preprocess(frames))
        tau_s, tau_b = FD.taus([heads[R.head_prefix(i)] for i in range(6)], [mod[R.head_prefix(i)] for i in range(6)])
        print(f"{key} x {len(seeds)}: tau_s {tau_s:.3e}, tau_b {tau_b:.3e}")
        assert_conditions(key, case, tau_s, len(seeds), summary)
        big = hw[0] >= 180
        for k, v in case.items():
            out[f"{k.split('_')[0]}_{key}" + (f"_{k.split('_')[1]}" if "_" in k else "")] = v.astype(np.float32) if big and k.startswith("heads") else v
        if hw == (64, 64):
            out.update(smoothing_example(gen, case["boxes"], hw))
    assert summary["most_kept"] >= 3, f"no image keeps 3 boxes above 0.5 ({summary['most_kept']})"
    assert summary["no_face"] >= 1, "no image without a score above 0.5"
    gold = os.path.join(ROOT, "tests", "golden")
    np.savez_compressed(os.path.join(gold, "s3fd_golden.npz"), **out)
    with open(os.path.join(gold, "s3fd_key_manifest.json"), "w") as f:
        json.dump(manifest, f, indent=0, sort_keys=True)
    size = os.path.getsize(os.path.join(gold, "s3fd_golden.npz"))
    assert size < 1000000, size
    print(f"wrote s3fd_golden.npz ({size} bytes), {len(manifest)} keys in the manifest")


if __name__ == "__main__":
    main()
