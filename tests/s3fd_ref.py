"""Float64 restatement of the S3FD face detector (avatars/wav2lip/face_detection/detection/sfd/net_s3fd.py s3fd.forward, detect.py
batch_detect, bbox.py batch_decode) and of its op walk: the launches of csrc/facedet.h fd_program by name, each with the tensor it
writes.  CPU code, torch only.  tests/test_face_detect_host.py holds it to the reference's own outputs stored in
tests/golden/s3fd_golden.npz (scripts/gen_golden_s3fd.py).

Input convention (api.py:65 + detect.py:59): a frame arrives BGR, is reversed to RGB, and (104, 117, 123) is subtracted from the
REVERSED channels, so the network's channel c is byte 2 - c of the pixel minus MEANS[c]."""
from __future__ import annotations

from collections import OrderedDict
from typing import Dict, List

import numpy as np
import torch
import torch.nn.functional as F

MEANS = (104.0, 117.0, 123.0)
SOURCES = ("conv3_3", "conv4_3", "conv5_3", "fc7", "conv6_2", "conv7_2")
NORMS = {"conv3_3": "conv3_3_norm", "conv4_3": "conv4_3_norm", "conv5_3": "conv5_3_norm"}
# the trunk, in order: (name, stride, pad) of a conv + ReLU, or a pool
TRUNK = (("conv1_1", 1, 1), ("conv1_2", 1, 1), "pool1", ("conv2_1", 1, 1), ("conv2_2", 1, 1), "pool2", ("conv3_1", 1, 1), ("conv3_2", 1, 1),
         ("conv3_3", 1, 1), "pool3", ("conv4_1", 1, 1), ("conv4_2", 1, 1), ("conv4_3", 1, 1), "pool4", ("conv5_1", 1, 1), ("conv5_2", 1, 1),
         ("conv5_3", 1, 1), "pool5", ("fc6", 1, 3), ("fc7", 1, 0), ("conv6_1", 1, 0), ("conv6_2", 2, 1), ("conv7_1", 1, 0), ("conv7_2", 2, 1))
KEY_BITS = 14
EPS = 1e-10


def head_prefix(level: int) -> str:
    s = SOURCES[level]
    return NORMS.get(s, s) + "_mbox"


def preprocess(bgr: np.ndarray, dtype=torch.float64) -> torch.Tensor:
    """uint8 (n, H, W, 3) BGR -> (n, 3, H, W): reversed, minus MEANS in the reversed order."""
    x = torch.from_numpy(np.ascontiguousarray(bgr[..., ::-1])).to(dtype).permute(0, 3, 1, 2)
    return x - torch.tensor(MEANS, dtype=dtype).view(1, 3, 1, 1)


def l2norm(x: torch.Tensor, weight: torch.Tensor) -> torch.Tensor:
    norm = x.pow(2).sum(dim=1, keepdim=True).sqrt() + EPS
    return x / norm * weight.view(1, -1, 1, 1)


def merged_head(sd: Dict[str, torch.Tensor], level: int):
    """(weight (16, cin, 3, 3), bias (16,)) of the level's ONE head conv: conf rows at 0.. (2, or 4 at level 0), loc rows at 4..7, zeros elsewhere."""
    p = head_prefix(level)
    wc, bc, wl, bl = (sd[p + s] for s in ("_conf.weight", "_conf.bias", "_loc.weight", "_loc.bias"))
    w = torch.zeros((16,) + tuple(wc.shape[1:]), dtype=wc.dtype, device=wc.device)
    b = torch.zeros(16, dtype=wc.dtype, device=wc.device)
    w[:wc.shape[0]], b[:wc.shape[0]] = wc, bc
    if level == 0:                          # four conf rows would run into the loc rows at 4..7 were there more
        assert wc.shape[0] == 4
    w[4:8], b[4:8] = wl, bl
    return w, b


def walk(sd: Dict[str, torch.Tensor], x: torch.Tensor, fault: str = "") -> "OrderedDict[str, torch.Tensor]":
    """Every launch of fd_program by name -> its output, on the network's input x (preprocess()); a head's output is the merged
    16-channel map.  Detect launches write no tensor and are not listed.  `fault` plants a wiring fault: "fc6_pad1", "ceil_pool"."""
    out: "OrderedDict[str, torch.Tensor]" = OrderedDict()
    h = x
    for step in TRUNK:
        if isinstance(step, str):
            h = F.max_pool2d(h, 2, 2, ceil_mode=fault == "ceil_pool")
            out[step] = h
        else:
            name, stride, pad = step
            if name == "fc6" and fault == "fc6_pad1":
                pad = 1
            h = F.relu(F.conv2d(h, sd[name + ".weight"], sd[name + ".bias"], stride=stride, padding=pad))
            out[name] = h
    for s, n in NORMS.items():
        out[n] = l2norm(out[s], sd[n + ".weight"])
    for i, s in enumerate(SOURCES):
        w, b = merged_head(sd, i)
        out[head_prefix(i)] = F.conv2d(out[NORMS.get(s, s)], w, b, padding=1)
    return out


def olist_from_heads(heads: List[torch.Tensor]) -> List[torch.Tensor]:
    """The six merged head maps -> the twelve tensors s3fd.forward returns (level 0's conf behind the max-out)."""
    o = []
    for i, m in enumerate(heads):
        if i == 0:
            conf = torch.cat([m[:, 0:3].max(dim=1, keepdim=True).values, m[:, 3:4]], 1)
        else:
            conf = m[:, 0:2]
        o += [conf, m[:, 4:8]]
    return o


def net(sd: Dict[str, torch.Tensor], x: torch.Tensor) -> List[torch.Tensor]:
    w = walk(sd, x)
    return olist_from_heads([w[head_prefix(i)] for i in range(6)])


def decode(loc: torch.Tensor, level: int, hindex, windex) -> torch.Tensor:
    """bbox.py batch_decode on the prior of detect.py:81-84: loc (..., 4) -> (x1, y1, x2, y2)."""
    stride = 2 ** (level + 2)
    axc, ayc, size = stride / 2 + windex * stride, stride / 2 + hindex * stride, stride * 4
    cx, cy = axc + loc[..., 0] * 0.1 * size, ayc + loc[..., 1] * 0.1 * size
    bw, bh = size * torch.exp(loc[..., 2] * 0.2), size * torch.exp(loc[..., 3] * 0.2)
    x1, y1 = cx - bw / 2, cy - bh / 2
    return torch.stack([x1, y1, bw + x1, bh + y1], -1)


def batch_detect(olist: List[torch.Tensor], thresh: float = 0.05) -> np.ndarray:
    """detect.py:70-94 on the network's outputs: (K, B, 5); a position is decoded for EVERY image of the batch whenever any image
    passes the threshold there (once per passing image: rows repeat)."""
    rows = []
    B = olist[0].shape[0]
    for i in range(6):
        ocls, oreg = F.softmax(olist[2 * i], dim=1), olist[2 * i + 1]
        for _, hindex, windex in zip(*np.where(ocls[:, 1].numpy() > thresh)):
            box = decode(oreg[:, :, hindex, windex], i, int(hindex), int(windex))
            rows.append(torch.cat([box, ocls[:, 1, hindex, windex].unsqueeze(1)], 1).numpy())
    return np.array(rows) if rows else np.zeros((1, B, 5))


def candidates(olist: List[torch.Tensor], thresh: float = 0.05):
    """What the engine returns: per image (keys uint32 (k,), rows float64 (k, 5)) of its OWN positions above thresh, sorted by
    key = level << 28 | h << 14 | w."""
    B = olist[0].shape[0]
    res = []
    for n in range(B):
        keys, rows = [], []
        for i in range(6):
            score = F.softmax(olist[2 * i][n:n + 1], dim=1)[0, 1]
            for hindex, windex in zip(*np.where(score.numpy() > thresh)):
                box = decode(olist[2 * i + 1][n, :, hindex, windex], i, int(hindex), int(windex))
                keys.append((i << 28) | (int(hindex) << KEY_BITS) | int(windex))
                rows.append(torch.cat([box, score[hindex, windex].view(1)]).numpy())
        order = np.argsort(np.asarray(keys, np.int64), kind="stable")
        res.append((np.asarray(keys, np.uint32)[order], np.asarray(rows, np.float64).reshape(-1, 5)[order]))
    return res
