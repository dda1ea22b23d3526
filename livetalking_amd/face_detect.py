"""Face boxes and Wav2Lip avatar preparation, host side.

Mirrors avatars/wav2lip/face_detection/detection/sfd/bbox.py:44-64 (nms), sfd_detector.py:41-47 (detect_from_batch), api.py:64-79
(get_detections_for_batch) and avatars/wav2lip/genavatar.py:41-48,106-138 (get_smoothened_boxes, the pad / crop / resize / save loop).
The network itself - S3FD and what batch_detect does behind it - is the engine's job: everything here needs an object with
`face_detect(frames_bgr uint8 (n, H, W, 3), thresh) -> per image float32 (k, 5) rows (x1, y1, x2, y2, score)`; an engine that also
has `load_face_detector` is handed the state dict.

The engine lists, per image, that image's OWN positions above 0.05.  The reference's batch_detect (detect.py:79-89) decodes a position
for every image of the batch whenever ANY image passes 0.05 there, so its per-image lists also hold rows whose score is at most 0.05
(and repeat a position once per image that passes).  Those extra rows change nothing: detect_from_batch keeps, of the boxes greedy NMS
keeps, the ones with score > 0.5.  NMS visits boxes in descending score, and a box is dropped only by a KEPT box that scores higher;
every box above 0.5 is therefore decided by boxes above 0.5 alone, whatever sits below them in the list, and a repeated row is
suppressed by its own first copy (overlap 1).  tests/test_face_detect_host.py shows it against the stored reference output.

OpenCV is not a dependency: frames are an input (video decoding and genavatar.py's putText stamp are out of scope), PNGs are written
with Pillow, and the crop is resized by the project's restatement of cv2.resize (bilinear; oracle/paste_oracle.py resize_linear_u8,
unpinned against OpenCV).  Also unmeasured: a real s3fd.pth (tests run seeded weights).
"""
from __future__ import annotations

import os
import pickle
from typing import List, Optional, Sequence

import numpy as np

DET_THRESH = 0.05       # detect.py:79
NMS_THRESH = 0.3        # sfd_detector.py:43
KEEP_THRESH = 0.5       # sfd_detector.py:45


def nms(dets: np.ndarray, thresh: float) -> List[int]:
    """bbox.py:44-64: greedy NMS on (k, 5) rows, areas and overlaps with the + 1 of pixel-inclusive boxes; -> kept row indices."""
    if 0 == len(dets):
        return []
    x1, y1, x2, y2, scores = dets[:, 0], dets[:, 1], dets[:, 2], dets[:, 3], dets[:, 4]
    areas = (x2 - x1 + 1) * (y2 - y1 + 1)
    order = scores.argsort()[::-1]
    keep = []
    while order.size > 0:
        i = order[0]
        keep.append(int(i))
        xx1, yy1 = np.maximum(x1[i], x1[order[1:]]), np.maximum(y1[i], y1[order[1:]])
        xx2, yy2 = np.minimum(x2[i], x2[order[1:]]), np.minimum(y2[i], y2[order[1:]])
        w, h = np.maximum(0.0, xx2 - xx1 + 1), np.maximum(0.0, yy2 - yy1 + 1)
        ovr = w * h / (areas[i] + areas[order[1:]] - w * h)
        order = order[np.where(ovr <= thresh)[0] + 1]
    return keep


def keep_faces(dets: np.ndarray) -> List[np.ndarray]:
    """sfd_detector.py:43-45 for one image: NMS 0.3, then score > 0.5, in NMS order (descending score)."""
    dets = np.asarray(dets)
    return [dets[i] for i in nms(dets, NMS_THRESH) if dets[i, 4] > KEEP_THRESH]


def first_box(faces: Sequence[np.ndarray]):
    """api.py:69-77 for one image: the first kept box clipped at 0 and truncated by int(), or None."""
    if len(faces) == 0:
        return None
    d = np.clip(faces[0], 0, None)
    x1, y1, x2, y2 = map(int, d[:-1])
    return (x1, y1, x2, y2)


class FaceDetector:
    """face_detection.FaceAlignment(...).get_detections_for_batch and SFDDetector.detect_from_batch over an engine.  sd: s3fd()'s
    state_dict (or a path torch.load reads), handed to engine.load_face_detector where the engine has that method; None: the engine is
    ready.  An engine that already holds a detector keeps it: the weights are loaded once per engine, and `sd` and `max_images` of
    this call are then ignored (the engine goes on chunking by the value of its own load)."""

    def __init__(self, engine, sd=None, max_images: int = 16):
        self.engine = engine
        if sd is not None and hasattr(engine, "load_face_detector"):
            if isinstance(sd, (str, os.PathLike)):
                import torch
                sd = torch.load(sd, map_location="cpu")
            try:
                engine.load_face_detector(sd, max_images=max_images)
            except Exception as e:                   # an engine holds one detector: a second avatar on it finds the first one's (LTK_E_STATE)
                if getattr(e, "code", None) != -3 or "already loaded" not in str(e):
                    raise

    def candidates(self, images_bgr: np.ndarray) -> List[np.ndarray]:
        return [np.asarray(r, np.float64).reshape(-1, 5) for r in self.engine.face_detect(np.ascontiguousarray(images_bgr), DET_THRESH)]

    def detect_from_batch(self, images_rgb: np.ndarray) -> List[List[np.ndarray]]:
        """sfd_detector.py:41-47; images_rgb (n, H, W, 3) as api.py:65-66 hands them over (the engine takes the frames BGR and
        reverses them itself, so they are reversed back here).  See the module docstring for the batch quirk."""
        return [keep_faces(d) for d in self.candidates(np.asarray(images_rgb)[..., ::-1])]

    def get_detections_for_batch(self, images_bgr: np.ndarray):
        """api.py:64-79: per image (x1, y1, x2, y2) ints of its best face, or None."""
        return [first_box(keep_faces(d)) for d in self.candidates(images_bgr)]


def get_smoothened_boxes(boxes: np.ndarray, T: int) -> np.ndarray:
    """genavatar.py:41-48, faithfully: in place on the (integer) array, so every mean is truncated on assignment, a window reads
    entries that are already smoothed, and the last T - 1 windows are the array's tail."""
    for i in range(len(boxes)):
        if i + T > len(boxes):
            window = boxes[len(boxes) - T:]
        else:
            window = boxes[i: i + T]
        boxes[i] = np.mean(window, axis=0)
    return boxes


def _write_png_bgr(path: str, img: np.ndarray) -> None:
    from PIL import Image
    Image.fromarray(np.ascontiguousarray(np.asarray(img, np.uint8)[:, :, ::-1])).save(path)


def avatar_boxes(predictions, frames_bgr: Sequence[np.ndarray], pads=(0, 10, 0, 0), nosmooth: bool = False) -> np.ndarray:
    """genavatar.py:106-120: the whole frame where no face was found, the pads clipped to the frame, the 5-frame smoothing."""
    pady1, pady2, padx1, padx2 = pads
    results = []
    for rect, image in zip(predictions, frames_bgr):
        if rect is None:
            rect = [0, 0, image.shape[1], image.shape[0]]
        y1 = max(0, rect[1] - pady1)
        y2 = min(image.shape[0], rect[3] + pady2)
        x1 = max(0, rect[0] - padx1)
        x2 = min(image.shape[1], rect[2] + padx2)
        results.append([x1, y1, x2, y2])
    boxes = np.array(results)
    if not nosmooth:
        boxes = get_smoothened_boxes(boxes, T=5)
    return boxes


def prepare_wav2lip_avatar(frames_bgr: Sequence[np.ndarray], out_dir: str, engine, detector_sd=None, img_size: int = 256,
                           pads=(0, 10, 0, 0), nosmooth: bool = False, batch: int = 16) -> str:
    """genavatar.py generate_avatar behind its video decoding: writes full_imgs/%08d.png, face_imgs/%08d.png and coords.pkl - (y1, y2,
    x1, x2) per frame - into out_dir, the directory wav2lip_avatar.load_avatar and bank.pack_avatar_dir read.  frames_bgr: equally
    sized uint8 BGR frames; a frame without a face takes the whole frame as its box (genavatar.py:109-110).  batch: frames per
    detector call (face_det_batch_size), at least 1.  detector_sd is loaded into the engine unless it already
    holds a detector (a second avatar on the same engine), which is then the one that runs."""
    from oracle.paste_oracle import resize_linear_u8
    if not len(frames_bgr):
        raise ValueError("prepare_wav2lip_avatar: at least one frame")
    if int(batch) < 1:
        raise ValueError("prepare_wav2lip_avatar: batch must be at least 1")
    os.makedirs(os.path.join(out_dir, "full_imgs"), exist_ok=True)
    os.makedirs(os.path.join(out_dir, "face_imgs"), exist_ok=True)
    det = FaceDetector(engine, detector_sd, max_images=min(int(batch), 16))
    predictions = []
    for i in range(0, len(frames_bgr), batch):
        predictions.extend(det.get_detections_for_batch(np.array(frames_bgr[i:i + batch])))
    boxes = avatar_boxes(predictions, frames_bgr, pads, nosmooth)
    coords = []
    for idx, (rect, frame) in enumerate(zip(boxes, frames_bgr)):
        _write_png_bgr(os.path.join(out_dir, "full_imgs", f"{idx:08d}.png"), frame)
        face = frame[int(rect[1]):int(rect[3]), int(rect[0]):int(rect[2])]
        _write_png_bgr(os.path.join(out_dir, "face_imgs", f"{idx:08d}.png"), resize_linear_u8(np.ascontiguousarray(face), (img_size, img_size)))
        coords.append((int(rect[1]), int(rect[3]), int(rect[0]), int(rect[2])))
    with open(os.path.join(out_dir, "coords.pkl"), "wb") as f:
        pickle.dump(coords, f)
    return out_dir
