"""CPU: livetalking_amd/avatar_prep.py - the restated OpenCV leaves, the three mask modes, get_image_prepare_material and
prepare_musetalk_avatar - against tests/golden/faceparse_golden.npz, which scripts/gen_golden_faceparse.py made by running the reference's
own FaceParsing.__call__ and get_image_prepare_material (with cv2 standing for the same restatements: the control flow is pinned, the
leaves are not), and a round trip of a prepared directory through musetalk_avatar.load_avatar.  The engine is a stand-in whose
face_parse is the float64 restatement of the network (tests/faceparse_ref.py)."""
from __future__ import annotations

import os
import pickle
import sys

import numpy as np
import pytest

import faceparse_ref as R
import synth_inputs as synth
from livetalking_amd import avatar_prep as A

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "scripts"))
import gen_golden_faceparse as G      # noqa: E402  (prep_frame, PREP_BOX: the inputs of the golden get_image_prepare_material calls)

MODES = ("raw", "neck", "jaw")


class FakeParseEngine:
    """face_parse by the float64 restatement (one forward per distinct image), vae_encode_faces by a fixed function of the crop."""

    def __init__(self, seed):
        self.sd = synth.faceparse_state_dict(seed)
        self.cache, self.parsed, self.encoded = {}, 0, 0

    def face_parse(self, rgb):
        rgb = np.ascontiguousarray(rgb, dtype=np.uint8)
        assert rgb.shape[1:] == (512, 512, 3)
        out = []
        for im in rgb:
            key = im.tobytes()
            if key not in self.cache:
                self.cache[key] = R.upsampled(R.Chain(self.sd, "ref").run(im[None].copy())).argmax(1).numpy().astype(np.uint8)[0]
            out.append(self.cache[key])
            self.parsed += 1
        return np.stack(out)

    def vae_encode_faces(self, faces_bgr, noise=None):
        faces = np.asarray(faces_bgr)
        assert faces.shape[1:] == (256, 256, 3) and faces.dtype == np.uint8
        self.encoded += len(faces)
        m = faces.reshape(len(faces), 8, 32, 8, 32, 3).mean((2, 4, 5)).astype(np.float32) / 255.0       # (n, 8, 8)
        return np.repeat(np.repeat(m[:, :, :, None], 32, 3), 4, 2).reshape(len(faces), 8, 32, 32)


@pytest.fixture(scope="module")
def gold():
    return np.load(os.path.join(ROOT, "tests", "golden", "faceparse_golden.npz"))


@pytest.fixture(scope="module")
def engine(gold):
    return FakeParseEngine(int(gold["seed"]))


# ------------------------------------------------------------------------------------------ the leaves
def test_ellipse_35_by_3_and_jaw_kernel():
    k = A.ellipse_kernel(35, 3)
    assert k.shape == (3, 35) and k[1].all() and k[0].sum() == 1 and k[2].sum() == 1 and k[0, 17] == 1 and k[2, 17] == 1
    assert np.array_equal(A.ellipse_kernel(5, 5), np.array([[0, 0, 1, 0, 0], [1, 1, 1, 1, 1], [1, 1, 1, 1, 1], [1, 1, 1, 1, 1], [0, 0, 1, 0, 0]], np.uint8))
    j = A.jaw_kernel()
    assert j.shape == (33, 33) and not j[:10].any() and j[10].sum() == 1 and j[20].sum() == 21 and (j[21:].sum(1) == 21).all()
    assert j[10, 16] == 1 and j[20, 6:27].all() and np.array_equal(j, j[:, ::-1])


def test_binary_morphology_border_and_anchor():
    img = np.zeros((9, 11), np.uint8)
    img[4, 5] = 255
    k = np.array([[1, 0, 0], [0, 1, 0], [0, 0, 0]], np.uint8)                  # not symmetric: a pixel dilates into the REFLECTED kernel
    d = A.dilate(img, k)
    assert sorted(zip(*np.nonzero(d))) == [(4, 5), (5, 6)]
    full = np.full((6, 40), 255, np.uint8)
    assert A.erode(full, A.ellipse_kernel(35, 3), 2).min() == 255              # the border never wins a minimum
    assert A.dilate(np.zeros((6, 40), np.uint8), A.jaw_kernel()).max() == 0    # ... nor a maximum
    hole = full.copy()
    hole[3, 20] = 0
    e = A.erode(hole, A.ellipse_kernel(35, 3), 1)
    assert (e[3, 3:38] == 0).all() and e[3, 2] == 255 and e[2, 20] == 0 and e[4, 20] == 0 and e[2, 19] == 255
    e2 = A.erode(hole, A.ellipse_kernel(35, 3), 2)
    assert (e2[3] == 0).all() and (e2[1, 20], e2[5, 20], e2[0, 20]) == (0, 0, 255)


def test_rectangle_is_inclusive_and_clipped():
    m = A.filled_rectangle(np.zeros((8, 8), np.uint8), (2, 0), (4, 8), 255)
    assert (m[:, 2:5] == 255).all() and m[:, :2].max() == 0 and m[:, 5:].max() == 0


def test_gaussian_blur_u8():
    flat = np.full((20, 30), 200, np.uint8)
    assert np.array_equal(A.gaussian_blur_u8(flat, 9), flat)                   # weights sum to one, reflect border
    step = np.zeros((31, 31), np.uint8)
    step[:, 16:] = 255
    b = A.gaussian_blur_u8(step, 11)
    assert (np.diff(b[15].astype(int)) >= 0).all() and b[15, 0] == 0 and b[15, -1] == 255 and np.array_equal(b[0], b[15])
    assert abs(int(b[15, 15]) + int(b[15, 16]) - 255) <= 1                     # symmetric about the edge
    x = np.arange(11) - 5.0
    k = np.exp(-x * x / (2 * 2.0 ** 2))                                        # sigma = 0.3 (5 - 1) + 0.8 = 2.0
    assert b[15, 16] == int(np.rint(255 * k[:6].sum() / k.sum()))


# ------------------------------------------------------------------------------------------ modes
def test_modes_on_a_synthetic_label_map():
    lab = np.zeros((512, 512), np.uint8)
    lab[100:300, 150:360] = 1          # skin
    lab[180:220, 230:280] = 10         # nose, inside the skin
    lab[300:330, 200:300] = 12         # a lip under it
    lab[330:400, 180:330] = 14         # neck
    fp = A.FaceParsing(None, None, 90, 90)
    raw, neck, jaw = (A.mode_mask(lab, m, fp.kernel, fp.cheek_kernel, fp.cheek_mask) for m in MODES)
    assert np.array_equal(raw == 255, np.isin(lab, [1, 12])) and np.array_equal(neck == 255, np.isin(lab, [1, 12, 14]))
    assert (jaw[lab == 10] == 0).all() and (jaw[lab == 12] == 255).all() and (jaw[lab == 1] == 255).sum() == (lab == 1).sum() - 200 * (17 + 14)
    # the skin loses the 17 + 14 columns the twice-eroded cheek zones (x <= 166, x >= 346) take; the dilation reaches 16 rows UP (a pixel
    # dilates into the reflected kernel, whose tail then points up) and 6 down
    assert jaw[84, 255] == 255 and jaw[83, 255] == 0 and jaw[335, 255] == 0 and jaw[150, 150] == 0 and jaw[150, 167] == 255
    assert set(np.unique(jaw)) <= {0, 255}


@pytest.mark.parametrize("mode", MODES)
def test_modes_equal_the_reference_on_the_golden_labels(gold, mode):
    fp = A.FaceParsing(None, None, 90, 90)
    m = A.mode_mask(gold["labels_512"][0], mode, fp.kernel, fp.cheek_kernel, fp.cheek_mask)
    assert np.array_equal(m, gold[f"mask_{mode}"]) and 0.2 < (m == 255).mean() < 0.9


def test_face_parsing_call_has_the_reference_contract(gold, engine):
    from PIL import Image
    fp = A.FaceParsing(engine, None, 90, 90)
    out = fp(Image.fromarray(synth.faceparse_image(512, seed=0)), mode="jaw")
    assert out.mode == "L" and out.size == (512, 512) and np.array_equal(np.asarray(out), gold["mask_jaw"])


@pytest.mark.parametrize("mode", MODES)
def test_get_image_prepare_material_equals_the_reference(gold, engine, mode):
    fp = A.FaceParsing(engine, None, 90, 90)
    mask, crop_box = A.get_image_prepare_material(G.prep_frame(), list(G.PREP_BOX), fp=fp, mode=mode)
    assert list(crop_box) == gold["prep_crop_box"].tolist() and mask.dtype == np.uint8
    assert np.array_equal(mask, gold[f"prep_mask_{mode}"])
    assert mask[: mask.shape[0] // 2 - 20].max() == 0 and mask.max() > 200       # only the lower half survives, blurred


# ------------------------------------------------------------------------------------------ the directory
def test_prepare_musetalk_avatar_round_trips_through_load_avatar(engine, tmp_path, monkeypatch):
    from PIL import Image
    import livetalking_amd.avatars.musetalk_avatar as M
    frame = G.prep_frame()
    frames = [frame, np.ascontiguousarray(frame[:, ::-1])]
    boxes = [G.PREP_BOX, (448 - 290, 110, 448 - 150, 280)]
    out_dir = tmp_path / "data" / "avatars" / "av1"
    A.prepare_musetalk_avatar(frames, boxes, str(out_dir), engine, version="v15", extra_margin=10, parsing_mode="jaw")
    assert sorted(os.listdir(out_dir)) == ["avator_info.json", "coords.pkl", "full_imgs", "latents.pt", "mask", "mask_coords.pkl"]
    assert sorted(os.listdir(out_dir / "mask")) == ["00000000.png", "00000001.png"]

    def read_imgs(paths):                      # what cv2.imread returns: 3-channel BGR
        return [np.ascontiguousarray(np.asarray(Image.open(p).convert("RGB"))[:, :, ::-1]) for p in paths]

    monkeypatch.setattr(M, "read_imgs", read_imgs)
    monkeypatch.chdir(tmp_path)
    fr, masks, coords, mask_coords, latents = M.load_avatar("av1")
    assert len(fr) == 2 and all(np.array_equal(a, b) for a, b in zip(fr, frames))
    assert coords == [[150, 110, 290, 290], [158, 110, 298, 290]]                 # y2 + extra_margin (v15)
    fp = A.FaceParsing(engine, None, 90, 90)
    for i in range(2):
        want, box = A.get_image_prepare_material(frames[i], coords[i], fp=fp, mode="jaw")
        assert list(mask_coords[i]) == list(box) and masks[i].shape == want.shape + (3,) and np.array_equal(masks[i][:, :, 0], want)
    crops = np.stack([A._resize_lanczos_256(frames[i][c[1]:c[3], c[0]:c[2]])[0] for i, c in enumerate(coords)])
    assert len(latents) == 2 and tuple(latents[0].shape) == (1, 8, 32, 32)
    assert np.array_equal(np.concatenate([t.numpy() for t in latents]), engine.vae_encode_faces(crops))
    import json
    info = json.load(open(out_dir / "avator_info.json"))
    assert info["vae_crop_resize"] in ("cv2.INTER_LANCZOS4", "PIL.LANCZOS") and info["parsing_mode"] == "jaw" and info["frames"] == 2
    with open(out_dir / "mask_coords.pkl", "rb") as f:
        assert pickle.load(f) == [list(b) for b in mask_coords]
