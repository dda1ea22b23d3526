"""GPU: the face parser as the engine runs it (ltk_face_parse_load / ltk_face_parse / ltk_face_parse_debug_get through
livetalking_amd.engine.Engine), on the seeded weights of synth_inputs.faceparse_state_dict(83).

  * op by op at 64 x 64 and 96 x 96 (3 x 3 / 6 x 6 / 12 x 12 maps: every conv and pool tile partial and odd), max_images = 2: every
    launch of the list in float64 on the device's own inputs under the stand-alone kernel tests' bounds (tests/face_parse_cases.py
    check_ops), on the short last chunk of a 2 + 1 call and on a 2-image call; every listed launch is checked;
  * end to end against float64 (tests/faceparse_ref.py end_to_end): labels equal wherever the float64 top-2 margin exceeds tau, the
    logits within tau, the label disagreement over all pixels within 4 x the rounding model's own; at 512 x 512 once, against the
    float64 results stored in tests/golden/faceparse_golden.npz;
  * an image alone, as the second of two and as the short tail of a 2 + 1 call;
  * through livetalking_amd.avatar_prep: FaceParsing's three modes and a prepared directory that load_avatar reads back, both
    networks on the engine;
  * the loader's refusals, and a watched call (ltk_health_watch "faceparse").
"""
from __future__ import annotations

import os
import sys

import numpy as np
import pytest

import face_parse_cases as C
import faceparse_ref as R
import synth_inputs as synth

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STATE, INVALID = -3, -1          # include/ltk.h LTK_E_STATE, LTK_E_INVALID


def _engine():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from livetalking_amd.engine import Engine
    return Engine(0)


@pytest.fixture(scope="module")
def sd():
    return synth.faceparse_state_dict(C.SEED)


@pytest.fixture(scope="module")
def parsers(sd):
    """size -> an engine with the parser loaded at that size, max_images = 2"""
    engines = {}
    for size in (64, 96):
        engines[size] = _engine()
        engines[size].load_face_parser(sd, size=size, max_images=2)
    yield engines
    for e in engines.values():
        e.close()


@pytest.fixture(scope="module")
def images():
    return {size: np.stack([synth.faceparse_image(size, seed=i) for i in range(3)]) for size in (64, 96)}


@pytest.fixture(scope="module")
def e2e(sd, images):
    """size -> the float64 side of images 0 and 1: computed once, left unchanged"""
    return {size: C.E2E(sd, images[size][:2]) for size in (64, 96)}


def _logits(eng, n, size):
    return eng.face_parse_debug_get("conv_out.conv_out", (n, 19, size // 8, size // 8))


# ------------------------------------------------------------------------------------------ op by op
@pytest.mark.parametrize("size", [64, 96])
def test_every_launch_against_float64_on_the_devices_own_inputs(parsers, images, sd, size):
    from livetalking_amd._lib import LtkError
    from livetalking_amd.engine import Engine
    eng, rgb = parsers[size], images[size]
    plan, prog = Engine.face_parse_plan(size, 2), Engine.face_parse_program(size)
    names = {p["name"] for p in prog}
    labels = eng.face_parse(rgb)                                     # chunks of 2 + 1: the read-back holds the last one, image 2
    assert labels.shape == (3, size, size) and labels.dtype == np.uint8
    with pytest.raises(LtkError) as ei:
        eng.face_parse_debug_get("cp.resnet.conv1", (2, 64, size // 2, size // 2))
    assert ei.value.code == INVALID and "1 images" in str(ei.value)
    with pytest.raises(LtkError) as ei:
        eng.face_parse_debug_get("labels", (1, 1, size, size))
    assert ei.value.code == INVALID and "ltk_face_parse" in str(ei.value)
    figs = C.check_ops(eng.face_parse_debug_get, plan, prog, sd, rgb[2:3], labels[2:3])
    assert set(figs) == names and len(figs) == 41                    # coverage: every listed launch was checked
    worst = max(figs, key=lambda n: figs[n].get("worst", 0.0))
    print(f"size {size}, last chunk of 2 + 1: worst |dev - ref| / tol {figs[worst]['worst']:.3f} at {worst}")
    two = eng.face_parse(rgb[:2])
    assert np.array_equal(two, labels[:2])                           # the same chunk of two, run again
    figs = C.check_ops(eng.face_parse_debug_get, plan, prog, sd, rgb[:2], two)
    assert set(figs) == names
    worst = max(figs, key=lambda n: figs[n].get("worst", 0.0))
    print(f"size {size}, 2 images: worst |dev - ref| / tol {figs[worst]['worst']:.3f} at {worst}; labels: {figs['labels']}")


# ------------------------------------------------------------------------------------------ end to end
@pytest.mark.parametrize("size", [64, 96])
def test_end_to_end_against_float64(parsers, images, e2e, size):
    eng, ref = parsers[size], e2e[size]
    labels = eng.face_parse(images[size][:2])
    print(f"size {size}:")
    ref.gates(labels, _logits(eng, 2, size))
    assert len(np.unique(labels)) >= 4                               # several classes win: the comparison says something


def test_512_once_against_the_stored_float64_results(sd):
    """One image, max_images = 1.  Whether the label gate applies is decided here, from the two models alone: the stored image's
    share of pixels inside tau against the cap.  Where it exceeds the cap (profiles/face_parse.txt records the share and tau of the
    run that made the record) the label gate is left to the 64 / 96 cases and 512 is held to the logit bound and the disagreement
    rule.  LTK_FACE_PARSE_OUT=<file>: the figures are appended there (scripts/face_parse_time.py writes the record this way)."""
    g = np.load(os.path.join(ROOT, "tests", "golden", "faceparse_golden.npz"))
    assert int(g["seed"]) == C.SEED
    rgb = synth.faceparse_image(512, seed=0)[None]
    ref = C.E2E(sd, rgb, g["logits_512"][:1], g["labels_512"][:1])
    eng = _engine()
    try:
        eng.load_face_parser(sd, size=512, max_images=1)
        labels = eng.face_parse(rgb)
        logits = _logits(eng, 1, 512)
    finally:
        eng.close()
    gated = ref.excluded <= C.EXCLUDED_CAP
    print(f"size 512: excluded share {ref.excluded:.4%} (cap {C.EXCLUDED_CAP:.0%})")
    out = os.environ.get("LTK_FACE_PARSE_OUT")
    try:
        ref.gates(labels, logits, label_gate=gated)
    finally:
        if out:
            with open(out, "a") as f:
                f.write(C.record_512(ref, labels, logits, gated))


# ------------------------------------------------------------------------------------------ company
@pytest.mark.parametrize("size", [64, 96])
def test_an_image_alone_second_of_two_and_as_the_short_tail(parsers, images, e2e, size):
    """Image 1 alone, as the second of a chunk of two and as the one-image tail of a 2 + 1 call: each result, beside image 0's from the
    two-image call, passes the end-to-end gates.  (No byte identity of the logits: a conv's split-K factor may follow the image count.)"""
    eng, rgb, ref = parsers[size], images[size], e2e[size]
    pair = eng.face_parse(rgb[:2])
    pair_logits = _logits(eng, 2, size)
    runs = {"second of two": (pair[1], pair_logits[1])}
    alone = eng.face_parse(rgb[1:2])
    runs["alone"] = (alone[0], _logits(eng, 1, size)[0])
    tail = eng.face_parse(rgb[[0, 2, 1]])
    runs["tail of 2 + 1"] = (tail[2], _logits(eng, 1, size)[0])
    assert np.array_equal(tail[0], pair[0])
    for how, (lab, log) in runs.items():
        print(f"size {size}, image 1 {how}: {int((lab != pair[1]).sum())} labels differ from the second-of-two run")
        ref.gates(np.stack([pair[0], lab]), np.stack([pair_logits[0], log]))


# ------------------------------------------------------------------------------------------ the Python surface
def test_face_parse_refuses_wrong_arrays_before_the_library(parsers, images):
    eng, rgb = parsers[64], images[64]
    for bad in (rgb.astype(np.float32), rgb[0], rgb[:, :, :, :2], images[96], rgb[:, :32]):
        with pytest.raises(ValueError):
            eng.face_parse(bad)
    assert eng.face_parse(rgb[:1]).shape == (1, 64, 64)


# ------------------------------------------------------------------------------------------ through avatar_prep
MODES = ("raw", "neck", "jaw")


def test_face_parsing_refuses_another_size_on_a_64_pixel_engine(parsers, images):
    from PIL import Image
    from livetalking_amd import avatar_prep as A
    fp = A.FaceParsing(parsers[64])
    with pytest.raises(ValueError, match="512 x 512"):
        fp(Image.fromarray(images[64][0]), size=(64, 64))
    # at the module's own size the call reaches the engine, whose parser was loaded for 64 x 64: the engine's refusal, before the library
    with pytest.raises(ValueError, match="loaded for 64 x 64"):
        fp(Image.fromarray(images[64][0]))
    from livetalking_amd._lib import LtkError
    with pytest.raises(LtkError) as ei:                              # and FaceParsing cannot load a second parser into it
        A.FaceParsing(parsers[64], synth.faceparse_state_dict(C.SEED, heads=False))
    assert ei.value.code == STATE
    assert parsers[64].face_parse(images[64][:1]).shape == (1, 64, 64)


def test_modes_and_a_prepared_directory_with_both_networks_on_the_engine(sd, tmp_path, monkeypatch):
    """prepare_musetalk_avatar(frames, boxes, dir, engine, vae_sd, parse_sd) loads the VAE encoder and the face parser into a fresh
    engine and writes a directory musetalk_avatar.load_avatar reads back; FaceParsing's three modes on that engine equal mode_mask on
    the engine's labels of the same resized image.  Masks against the stored reference masks: a differing-pixel share, printed and not
    gated (one flipped label dilates through the 33 x 33 kernel)."""
    from PIL import Image
    from livetalking_amd import avatar_prep as A
    import livetalking_amd.avatars.musetalk_avatar as M
    sys.path.insert(0, os.path.join(ROOT, "scripts"))
    import gen_golden_faceparse as G
    gold = np.load(os.path.join(ROOT, "tests", "golden", "faceparse_golden.npz"))
    frame = G.prep_frame()
    frames = [frame, np.ascontiguousarray(frame[:, ::-1])]
    boxes = [G.PREP_BOX, (448 - 290, 110, 448 - 150, 280)]
    out_dir = tmp_path / "data" / "avatars" / "av1"
    eng = _engine()
    try:
        A.prepare_musetalk_avatar(frames, boxes, str(out_dir), eng, synth.vae_encoder_state_dict(), sd, version="v15", extra_margin=10,
                                  parsing_mode="jaw")
        assert sorted(os.listdir(out_dir)) == ["avator_info.json", "coords.pkl", "full_imgs", "latents.pt", "mask", "mask_coords.pkl"]

        def read_imgs(paths):                  # what cv2.imread returns: 3-channel BGR
            return [np.ascontiguousarray(np.asarray(Image.open(p).convert("RGB"))[:, :, ::-1]) for p in paths]

        monkeypatch.setattr(M, "read_imgs", read_imgs)
        monkeypatch.chdir(tmp_path)
        fr, masks, coords, mask_coords, latents = M.load_avatar("av1")
        assert len(fr) == 2 and all(np.array_equal(a, b) for a, b in zip(fr, frames))
        assert coords == [[150, 110, 290, 290], [158, 110, 298, 290]]
        fp = A.FaceParsing(eng, None, 90, 90)                          # the engine is ready: both networks were loaded above
        for i in range(2):
            want, box = A.get_image_prepare_material(frames[i], coords[i], fp=fp, mode="jaw")
            assert list(mask_coords[i]) == list(box) and np.array_equal(masks[i][:, :, 0], want) and want.max() > 200
        crops = np.stack([A._resize_lanczos_256(frames[i][c[1]:c[3], c[0]:c[2]])[0] for i, c in enumerate(coords)])
        assert len(latents) == 2 and tuple(latents[0].shape) == (1, 8, 32, 32)
        assert np.array_equal(np.concatenate([t.numpy() for t in latents]), eng.vae_encode_faces(crops))
        want0, _ = A.get_image_prepare_material(frames[0], list(G.PREP_BOX), fp=fp, mode="jaw")
        print(f"prepared mask of frame 0 against the stored reference mask: {float((want0 != gold['prep_mask_jaw']).mean()):.4%} of the pixels differ")
        # the three modes on the engine's own labels
        image = Image.fromarray(synth.faceparse_image(512, seed=0))
        labels = eng.face_parse(np.asarray(image.resize((512, 512), Image.BILINEAR).convert("RGB"), dtype=np.uint8)[None])[0]
        for mode in MODES:
            out = fp(image, mode=mode)
            assert out.mode == "L" and out.size == (512, 512)
            assert np.array_equal(np.asarray(out), A.mode_mask(labels, mode, fp.kernel, fp.cheek_kernel, fp.cheek_mask))
            print(f"mode {mode}: {float((np.asarray(out) != gold[f'mask_{mode}']).mean()):.4%} of the mask's pixels differ from the stored reference mask")
    finally:
        eng.close()


# ------------------------------------------------------------------------------------------ loader
def test_loader_key_sets_and_states(sd):
    from livetalking_amd._lib import LtkError
    rgb = synth.faceparse_image(64, seed=0)[None]
    assert len(sd) == 191
    full, lean, broken, fresh = _engine(), _engine(), _engine(), _engine()
    try:
        full.load_face_parser(sd, size=64, max_images=1)
        lean.load_face_parser(synth.faceparse_state_dict(C.SEED, heads=False), size=64, max_images=1)
        assert np.array_equal(full.face_parse(rgb), lean.face_parse(rgb))
        key = "cp.arm16.bn_atten.running_var"
        with pytest.raises(LtkError) as ei:
            broken.load_face_parser({k: v for k, v in sd.items() if k != key}, size=64, max_images=1)
        assert ei.value.code == INVALID and key in str(ei.value)
        for size, n in ((48, 1), (544, 1), (0, 1), (64, 0), (64, 9)):
            with pytest.raises(LtkError) as ei:
                broken.load_face_parser(sd, size=size, max_images=n)
            assert ei.value.code == INVALID, (size, n)
        broken.load_face_parser(sd, size=64, max_images=1)           # a refused load leaves nothing behind
        with pytest.raises(LtkError) as ei:
            full.load_face_parser(sd, size=64, max_images=1)
        assert ei.value.code == STATE
        with pytest.raises(LtkError) as ei:
            fresh.face_parse(rgb)
        assert ei.value.code == STATE
        with pytest.raises(LtkError) as ei:
            fresh.face_parse_debug_get("cp.avg", (1, 512, 1, 1))
        assert ei.value.code == STATE
    finally:
        for e in (full, lean, broken, fresh):
            e.close()


# ------------------------------------------------------------------------------------------ headroom watch
def test_a_watched_call_lists_41_ops_and_changes_no_label(parsers, images):
    eng, rgb = parsers[64], images[64]
    plain = eng.face_parse(rgb)
    eng.health_watch("faceparse", 1)
    watched = eng.face_parse(rgb)                                    # 2 + 1 images: one call, whatever its chunks
    ops, seen, left = eng.health_report("faceparse")
    assert np.array_equal(watched, plain)
    assert (seen, left) == (1, 0) and len(ops) == 41
    from livetalking_amd.engine import Engine
    assert [(o["name"], o["type"]) for o in ops] == [(p["name"], p["type"]) for p in Engine.face_parse_program(64)]
    assert [o["name"] for o in ops if not o["observed"]] == ["labels"] and sum(o["observed"] for o in ops) == 40
    for o in ops:
        assert o["at_limit"] == 0 and o["nonfinite"] == 0 and o["q8"] == 0, o
        if o["observed"]:
            assert o["elements"] > 0, o
    print("largest |activation| of the seeded net: " + ", ".join(f"{o['name']} {o['max_abs']:.1f}" for o in sorted(ops, key=lambda o: -o["max_abs"])[:3]))
    assert np.array_equal(eng.face_parse(rgb), plain)                # the watch has disarmed itself: the replayed program again
