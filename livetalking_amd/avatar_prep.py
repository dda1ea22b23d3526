"""MuseTalk avatar preparation, host side: the blend masks from face-parser labels, and the avatar directory.

Mirrors avatars/musetalk/utils/face_parsing/__init__.py (FaceParsing), utils/blending.py:7-13,16-32,112-136 (get_crop_box, face_seg,
get_image_prepare_material) and the loop of genavatar.py:116-156.  The network itself is the engine's job: everything here needs an
object with `face_parse(rgb uint8 (n, 512, 512, 3)) -> uint8 labels (n, 512, 512)` (and, for the directory, `vae_encode_faces`);
an engine that also has `load_face_parser` / `load_vae_encoder` is handed the state dicts.  The landmark / box stage
(get_landmark_and_bbox) is not here: boxes are an input.

OpenCV is not a dependency.  Its leaves are restated in numpy below and are UNPINNED against OpenCV (nothing here has been compared
with cv2 itself), as cv2.resize is in oracle/paste_oracle.py.  What each restatement assumes:

  dilate / erode   binary (0 / 255) images, anchor at the kernel's centre (k // 2), the border of cv2's default
                   morphologyDefaultBorderValue: pixels outside the image never win a maximum (dilate) nor a minimum (erode).
                   Exact integer work; `iterations` repeats the pass.
  ellipse          getStructuringElement(MORPH_ELLIPSE, (w, h)): r = h // 2, c = w // 2; row i with dy = i - r spans columns
                   c - dx .. c + dx, dx = round_half_even(c * sqrt((r^2 - dy^2) / r^2)).  For (35, 3): one pixel, the full row, one pixel.
  rectangle        filled, both corners inclusive, clipped to the image.
  GaussianBlur     uint8, square odd kernel, sigma 0 -> 0.3 ((k - 1) / 2 - 1) + 0.8, kernel exp(-x^2 / 2 sigma^2) normalised to 1,
                   BORDER_REFLECT_101, separable in float64, one round-half-even at the end.  OpenCV's uint8 path works in fixed
                   point, so single bytes may differ by 1; the mask is a soft alpha, never compared bit for bit with cv2 output.
  resize LANCZOS4  the 256 x 256 VAE crop uses cv2.resize(INTER_LANCZOS4) where cv2 imports and Pillow's LANCZOS otherwise;
                   avator_info.json records which.
"""
from __future__ import annotations

import json
import os
import pickle
from typing import Optional, Sequence

import numpy as np

PARSE_SIZE = 512


# ------------------------------------------------------------------------------------------ OpenCV leaves, restated
def ellipse_kernel(width: int, height: int) -> np.ndarray:
    r, c = height // 2, width // 2
    k = np.zeros((height, width), np.uint8)
    for i in range(height):
        dy = i - r
        if abs(dy) <= r:
            dx = int(np.rint(c * np.sqrt((r * r - dy * dy) / float(r * r)))) if r else c
            k[i, max(c - dx, 0):min(c + dx + 1, width)] = 1
    return k


def _morph(img: np.ndarray, kernel: np.ndarray, iterations: int, dilate: bool) -> np.ndarray:
    img = np.asarray(img, np.uint8)
    kh, kw = kernel.shape
    ay, ax = kh // 2, kw // 2
    H, W = img.shape
    neutral = 0 if dilate else 255
    for _ in range(iterations):
        pad = np.full((H + kh - 1, W + kw - 1), neutral, np.uint8)
        pad[ay:ay + H, ax:ax + W] = img
        out = np.full((H, W), neutral, np.uint8)
        for ky, kx in zip(*np.nonzero(kernel)):
            win = pad[ky:ky + H, kx:kx + W]
            out = np.maximum(out, win) if dilate else np.minimum(out, win)
        img = out
    return img


def dilate(img: np.ndarray, kernel: np.ndarray, iterations: int = 1) -> np.ndarray:
    return _morph(img, kernel, iterations, True)


def erode(img: np.ndarray, kernel: np.ndarray, iterations: int = 1) -> np.ndarray:
    return _morph(img, kernel, iterations, False)


def filled_rectangle(img: np.ndarray, pt1, pt2, value: int) -> np.ndarray:
    (x0, y0), (x1, y1) = pt1, pt2
    x0, x1, y0, y1 = min(x0, x1), max(x0, x1), min(y0, y1), max(y0, y1)
    H, W = img.shape[:2]
    img[max(y0, 0):min(y1, H - 1) + 1, max(x0, 0):min(x1, W - 1) + 1] = value
    return img


def gaussian_blur_u8(img: np.ndarray, ksize: int) -> np.ndarray:
    assert ksize % 2 == 1 and ksize >= 1
    img = np.asarray(img, np.uint8)
    if ksize == 1:
        return img.copy()
    sigma = 0.3 * ((ksize - 1) * 0.5 - 1) + 0.8
    x = np.arange(ksize, dtype=np.float64) - (ksize - 1) * 0.5
    k = np.exp(-(x * x) / (2.0 * sigma * sigma))
    k /= k.sum()
    p = ksize // 2
    a = img.astype(np.float64)

    def along(a, axis):
        n = a.shape[axis]
        idx = np.arange(-p, n + p)
        if n > 1:                                       # BORDER_REFLECT_101: gfedcb|abcdefgh|gfedcba
            period = 2 * (n - 1)
            idx = np.abs(idx) % period
            idx = np.where(idx >= n, period - idx, idx)
        else:
            idx = np.zeros_like(idx)
        ext = np.take(a, idx, axis=axis)
        out = np.zeros_like(a)
        for t in range(ksize):
            out += k[t] * np.take(ext, np.arange(t, t + n), axis=axis)
        return out

    return np.clip(np.rint(along(along(a, 1), 0)), 0, 255).astype(np.uint8)


# ------------------------------------------------------------------------------------------ face_parsing/__init__.py
def jaw_kernel(cone_height: int = 21, tail_height: int = 12) -> np.ndarray:
    """The cone-and-tail 33 x 33 dilation kernel of FaceParsing.__init__ (:15-42): a cone that widens by two pixels a row from the
    middle row of its 21 rows, then 12 rows as wide as the cone's base."""
    total = cone_height + tail_height
    k = np.zeros((total, total), np.uint8)
    cx = total // 2
    for row in range(cone_height // 2, cone_height):
        w = 2 * (row - cone_height // 2) + 1
        k[row, cx - w // 2:cx + w // 2 + 1] = 1
    base = int(k[cone_height - 1].sum()) if cone_height > 0 else 1
    k[cone_height:, max(0, cx - base // 2):min(total, cx + base // 2 + 1)] = 1
    return k


def mode_mask(labels: np.ndarray, mode: str, kernel: np.ndarray, cheek_kernel: np.ndarray, cheek_mask: np.ndarray) -> np.ndarray:
    """uint8 labels (512, 512) -> uint8 0 / 255 mask, as FaceParsing.__call__ (:92-108) turns `parsing` into it."""
    parsing = np.asarray(labels).astype(np.int64)
    if mode == "neck":
        keep = np.isin(parsing, [1, 11, 12, 13, 14])
    elif mode == "jaw":
        face = (np.isin(parsing, [1]) * 255).astype(np.uint8)
        dilated = dilate(face, kernel, 1)
        eroded = erode(dilated, cheek_kernel, 2)
        region = (eroded & cheek_mask) | (dilated & ~cheek_mask)
        # the reference writes 255 into `parsing` first and then tests for 11, 12, 13 and != 255: a label is never 255, so this is the union
        keep = ((region == 255) & ~np.isin(parsing, [10])) | np.isin(parsing, [11, 12, 13])
    else:
        keep = np.isin(parsing, [1, 11, 12, 13])
    return (keep * 255).astype(np.uint8)


class FaceParsing:
    """FaceParsing of the reference with the network on the engine.  `state_dict_or_path`: BiSeNet.state_dict() (or a file torch.load
    reads), handed to engine.load_face_parser where the engine has that method; None: the engine is ready."""

    def __init__(self, engine, state_dict_or_path=None, left_cheek_width: int = 80, right_cheek_width: int = 80):
        self.engine = engine
        if state_dict_or_path is not None and hasattr(engine, "load_face_parser"):
            sd = state_dict_or_path
            if isinstance(sd, (str, os.PathLike)):
                import torch
                sd = torch.load(sd, map_location="cpu")
            engine.load_face_parser(sd, size=PARSE_SIZE, max_images=1)
        self.kernel = jaw_kernel()
        self.cheek_kernel = ellipse_kernel(35, 3)
        center = PARSE_SIZE // 2
        m = np.zeros((PARSE_SIZE, PARSE_SIZE), np.uint8)
        filled_rectangle(m, (0, 0), (center - left_cheek_width, PARSE_SIZE), 255)
        filled_rectangle(m, (center + right_cheek_width, 0), (PARSE_SIZE, PARSE_SIZE), 255)
        self.cheek_mask = m

    def labels(self, image) -> np.ndarray:
        """PIL image (already 512 x 512) -> uint8 labels (512, 512)"""
        rgb = np.asarray(image.convert("RGB"), dtype=np.uint8)
        return np.asarray(self.engine.face_parse(rgb[None]))[0]

    def __call__(self, image, size=(PARSE_SIZE, PARSE_SIZE), mode: str = "raw"):
        from PIL import Image
        if isinstance(image, str):
            image = Image.open(image)
        if tuple(size) != (PARSE_SIZE, PARSE_SIZE):
            raise ValueError("FaceParsing: the cheek mask and the engine's program are built for 512 x 512")
        image = image.resize(size, Image.BILINEAR)            # on the host, as the reference does
        return Image.fromarray(mode_mask(self.labels(image), mode, self.kernel, self.cheek_kernel, self.cheek_mask))


# ------------------------------------------------------------------------------------------ utils/blending.py
def get_crop_box(box, expand):
    x, y, x1, y1 = box
    x_c, y_c = (x + x1) // 2, (y + y1) // 2
    w, h = x1 - x, y1 - y
    s = int(max(w, h) // 2 * expand)
    return [x_c - s, y_c - s, x_c + s, y_c + s], s


def get_image_prepare_material(image, face_box, upper_boundary_ratio=0.5, expand=1.5, fp=None, mode="raw"):
    """image: BGR uint8 frame; -> (mask_array uint8 (2s, 2s), crop_box) as blending.py:112-136."""
    from PIL import Image
    body = Image.fromarray(np.ascontiguousarray(image[:, :, ::-1]))
    x, y, x1, y1 = face_box
    crop_box, _ = get_crop_box(face_box, expand)
    x_s, y_s, _, _ = crop_box
    face_large = body.crop(crop_box)
    ori_shape = face_large.size
    mask_image = fp(face_large, mode=mode).resize(face_large.size)                     # face_seg
    mask_small = mask_image.crop((x - x_s, y - y_s, x1 - x_s, y1 - y_s))
    mask_image = Image.new("L", ori_shape, 0)
    mask_image.paste(mask_small, (x - x_s, y - y_s, x1 - x_s, y1 - y_s))
    width, height = mask_image.size
    top = int(height * upper_boundary_ratio)                                             # keep the talking area
    modified = Image.new("L", ori_shape, 0)
    modified.paste(mask_image.crop((0, top, width, height)), (0, top))
    ksize = int(0.1 * ori_shape[0] // 2 * 2) + 1
    return gaussian_blur_u8(np.array(modified), ksize), crop_box


# ------------------------------------------------------------------------------------------ genavatar.py:116-156
def _resize_lanczos_256(crop_bgr: np.ndarray):
    try:
        import cv2
        if hasattr(cv2, "resize") and hasattr(cv2, "INTER_LANCZOS4"):
            return cv2.resize(crop_bgr, (256, 256), interpolation=cv2.INTER_LANCZOS4), "cv2.INTER_LANCZOS4"
    except ImportError:
        pass
    from PIL import Image
    return np.asarray(Image.fromarray(np.ascontiguousarray(crop_bgr)).resize((256, 256), Image.LANCZOS)), "PIL.LANCZOS"


def _write_png_bgr(path: str, img: np.ndarray) -> None:
    from PIL import Image
    img = np.asarray(img, np.uint8)
    Image.fromarray(np.ascontiguousarray(img[:, :, ::-1]) if img.ndim == 3 else img).save(path)


def prepare_musetalk_avatar(frames_bgr: Sequence[np.ndarray], boxes, out_dir: str, engine, vae_sd=None, parse_sd=None, version: str = "v15",
                            extra_margin: int = 10, parsing_mode: str = "jaw", noise: Optional[np.ndarray] = None) -> str:
    """Writes full_imgs/%08d.png, mask/%08d.png, coords.pkl, mask_coords.pkl, latents.pt and avator_info.json into out_dir: the
    directory musetalk_avatar.load_avatar and bank.pack_avatar_dir read.  boxes: (x1, y1, x2, y2) per frame (no placeholder boxes:
    every frame needs its face; face_detect.FaceDetector(engine, s3fd_sd).get_detections_for_batch gives the reference's fallback box).  noise: as Engine.vae_encode_faces takes it (None: the distribution's mean)."""
    import torch
    if len(frames_bgr) != len(boxes) or not len(frames_bgr):
        raise ValueError("prepare_musetalk_avatar: one box per frame, at least one frame")
    os.makedirs(os.path.join(out_dir, "full_imgs"), exist_ok=True)
    os.makedirs(os.path.join(out_dir, "mask"), exist_ok=True)
    if vae_sd is not None and hasattr(engine, "load_vae_encoder"):
        engine.load_vae_encoder(vae_sd)
    fp = FaceParsing(engine, parse_sd, 90, 90) if version == "v15" else FaceParsing(engine, parse_sd)
    coords, crops, how = [], [], ""
    for frame, box in zip(frames_bgr, boxes):
        x1, y1, x2, y2 = (int(v) for v in box)
        if version == "v15":
            y2 = min(y2 + extra_margin, frame.shape[0])
        coords.append([x1, y1, x2, y2])
        crop, how = _resize_lanczos_256(frame[y1:y2, x1:x2])
        crops.append(crop)
    latents = np.asarray(engine.vae_encode_faces(np.stack(crops), noise), dtype=np.float32)
    masks, mask_coords = [], []
    for i, frame in enumerate(frames_bgr):
        _write_png_bgr(os.path.join(out_dir, "full_imgs", f"{i:08d}.png"), frame)
        mask, crop_box = get_image_prepare_material(frame, coords[i], fp=fp, mode=parsing_mode if version == "v15" else "raw")
        _write_png_bgr(os.path.join(out_dir, "mask", f"{i:08d}.png"), mask)
        masks.append(mask)
        mask_coords.append(crop_box)
    with open(os.path.join(out_dir, "mask_coords.pkl"), "wb") as f:
        pickle.dump(mask_coords, f)
    with open(os.path.join(out_dir, "coords.pkl"), "wb") as f:
        pickle.dump(coords, f)
    torch.save([torch.from_numpy(latents[i:i + 1].copy()) for i in range(len(latents))], os.path.join(out_dir, "latents.pt"))
    with open(os.path.join(out_dir, "avator_info.json"), "w") as f:
        json.dump({"avatar_id": os.path.basename(os.path.normpath(out_dir)), "version": version, "parsing_mode": parsing_mode,
                   "extra_margin": extra_margin, "frames": len(frames_bgr), "vae_crop_resize": how}, f)
    return out_dir
