"""Cases, float64 references, float32 rounding models, bounds and planted faults of the face parser's own kernels
(csrc/parse_kernels.hip through include/ltk.h ltk_parse_stem_f16, ltk_maxpool3x3s2_f16, ltk_global_avgpool_f16, ltk_chan_gate_f16,
ltk_seg_argmax_f16).  CPU code; tests/test_faceparse_host.py holds the models and a simulated device with planted faults to the gates,
tests/test_faceparse_gpu.py holds the device to the same gates.

Every op is compared on the DEVICE's own inputs (what the test uploaded), so `dev - ref` is that op's error alone.  Per op:

  ref : float64, the reference's arithmetic (torch CPU), unrounded weights;
  mod : the kernel's arithmetic restated in float32 - fp16 weights, fp16 normalised input, fp32 sums, one fp16 rounding;
  tol : per element, in the forms of oracle/op_replay.py:
        stem     2^-10 |ref| + 2^-12 (short_sum(147) |W| (*) |x_n| |scale| + 4 |shift|) + 2^-24 sum |x_n| |scale| + 2^-24, x_n the
                 normalised image, zero outside it.  The input's own rounding to fp16 (2^-11 per product, independent of the weight's)
                 shares the weight term: short_sum() sizes it so that six sigma of the weight roundings are a quarter of it; with the
                 input's roundings beside them that is sqrt 2 quarters, 0.35 of the term, still inside the half the model is held to.
        maxpool  exact: dev == ref.
        gap      2^-10 |ref| + 2^-24 ceil(log2 P) mean |x| + 2^-24: a binary tree of fp32 additions, one rounding of at most
                 2^-24 (partial sum) per level.
        gate     2^-10 |ref| + 2^-10 |x| s'(a) |a| + 2^-22 (|x| g + |b| + |r|) + 2^-24: first order in a (a sigmoid evaluated from an
                 argument good to 2^-10 relative), and the fp32 roundings of the product and the two sums, which nothing relative to
                 |ref| covers where the terms cancel (g = sigmoid(a), + 1 in the FFM form).
        seg head labels: equal to the float64 labels wherever the float64 top-2 margin exceeds 2^-20 max |logit|; at most 0.1 % of
                 the pixels may be excluded.  (Three fp32 roundings and two weights good to 2^-24 per class: 6 x 2^-24 max |logit|
                 per class, 12 x 2^-24 on a difference of two.)
Gates (check()): no element beyond tol; rel_l2(dev, ref) <= 2 rel_l2(mod, ref) + 1e-4; the model itself within 0.5 tol.
"""
from __future__ import annotations

import math

import numpy as np
import torch
import torch.nn.functional as F

from oracle.op_replay import AGG_FACTOR, AGG_FLOOR, C_LIN, F16_FLOOR, MODEL_HEADROOM, rel_l2, short_sum

MEAN = (0.485, 0.456, 0.406)
STD = (0.229, 0.224, 0.225)
N_CLASSES = 19
GAP_MAX_P = 4096


# ------------------------------------------------------------------------------------------ layout
def to_cb16(x: np.ndarray) -> np.ndarray:
    """(N, C, H, W) -> float16 (N, ceil(C/16), H, W, 16), zero padded."""
    n, c, h, w = x.shape
    cb = (c + 15) // 16
    buf = np.zeros((n, cb * 16, h, w), np.float16)
    buf[:, :c] = x.astype(np.float16)
    return np.ascontiguousarray(buf.reshape(n, cb, 16, h, w).transpose(0, 1, 3, 4, 2))


def from_cb16(y: np.ndarray, c: int) -> np.ndarray:
    """float16 (N, CB, H, W, 16) -> float64 (N, c, H, W)."""
    n, cb, h, w, _ = y.shape
    return y.transpose(0, 1, 4, 2, 3).reshape(n, cb * 16, h, w)[:, :c].astype(np.float64)


def f16(t: torch.Tensor) -> torch.Tensor:
    return t.half().to(t.dtype)


def check(dev: np.ndarray, ref: np.ndarray, mod: np.ndarray, tol: np.ndarray) -> dict:
    """The gates on one op's output; -> the figures.  Raises AssertionError with them."""
    d, r, m = (torch.from_numpy(np.asarray(a, np.float64)) for a in (dev, ref, mod))
    t = torch.from_numpy(np.asarray(tol, np.float64))
    assert bool(torch.isfinite(d).all()), "non-finite device output"
    worst = float(((d - r).abs() / t).max())
    fig = dict(worst=worst, rel_dev=rel_l2(d, r), rel_mod=rel_l2(m, r), worst_mod=float(((m - r).abs() / t).max()))
    assert worst <= 1.0, f"|dev - ref| reaches {worst:.3f} of the bound ({int(((d - r).abs() > t).sum())} elements beyond it)"
    assert fig["rel_dev"] <= AGG_FACTOR * fig["rel_mod"] + AGG_FLOOR, f"aggregate: rel_l2 dev {fig['rel_dev']:.3e} vs model {fig['rel_mod']:.3e}"
    return fig


def model_inside(ref, mod, tol) -> float:
    w = float((np.abs(np.asarray(mod, np.float64) - ref) / tol).max())
    assert w <= MODEL_HEADROOM, f"the rounding model reaches {w:.3f} of the bound"
    return w


# ------------------------------------------------------------------------------------------ stem
STEM_SHAPES = [(1, 10, 14), (3, 10, 14), (1, 64, 64), (3, 64, 64)]      # 10 x 14 -> 5 x 7: every tile partial; 512 x 512 once on the GPU


class Stem:
    """Seeded inputs of one stem call: a smooth image plus noise (both saturate), He-scaled weights, a BatchNorm-like affine."""

    def __init__(self, N, H, W, seed=0):
        g = np.random.default_rng(1000 + seed + 7 * N + H)
        yy, xx = np.mgrid[0:H, 0:W]
        base = 128 + 100 * np.sin(yy[None, :, :, None] / 5.0 + np.arange(N)[:, None, None, None]) * np.cos(xx[None, :, :, None] / 7.0 + np.arange(3))
        self.rgb = np.clip(base + g.normal(0, 40, (N, H, W, 3)), 0, 255).astype(np.uint8)
        self.rgb[:, 0, 0] = 0                                        # the extremes of the input range at a corner
        self.rgb[:, -1, -1] = 255
        self.w = (g.normal(0, math.sqrt(2.0 / 147), (64, 3, 7, 7))).astype(np.float32)
        self.scale = g.uniform(0.5, 1.5, 64).astype(np.float32) * np.where(g.random(64) < 0.2, -1, 1).astype(np.float32)
        self.shift = g.normal(0, 0.3, 64).astype(np.float32)
        self.N, self.H, self.W = N, H, W

    def normalised(self, rgb=None, dtype=torch.float64) -> torch.Tensor:
        x = torch.from_numpy(self.rgb if rgb is None else rgb).permute(0, 3, 1, 2).to(dtype)
        m = torch.tensor(MEAN, dtype=dtype).view(1, 3, 1, 1)
        s = torch.tensor(STD, dtype=dtype).view(1, 3, 1, 1)
        return (x / 255.0 - m) / s

    def ref_tol(self):
        v = lambda t: torch.from_numpy(t).double()[None, :, None, None]
        x, W = self.normalised(), torch.from_numpy(self.w).double()
        ref = F.relu(F.conv2d(x, W, None, stride=2, padding=3) * v(self.scale) + v(self.shift))
        A = short_sum(147) * F.conv2d(x.abs(), W.abs(), None, stride=2, padding=3) * v(self.scale).abs() + 4 * v(self.shift).abs()
        s = F.conv2d(x.abs().sum(1, keepdim=True), torch.ones(1, 1, 7, 7, dtype=torch.float64), None, stride=2, padding=3) * v(self.scale).abs()
        tol = 2.0 ** -10 * ref.abs() + C_LIN * A + 2.0 ** -24 * s + F16_FLOOR
        return ref.numpy(), tol.numpy()

    def model(self, fault: str = "") -> np.ndarray:
        """The kernel in float32 (NCHW float16-representable); `fault`: "zero_byte_pad" (the image is padded with zero bytes, i.e. -mean / std
        after normalisation - the image / 255 padded with zeros and normalised afterwards is the same tensor, so it is not a fault of
        its own), "bgr"."""
        v = lambda t: torch.from_numpy(t)[None, :, None, None]
        rgb = self.rgb[..., ::-1].copy() if fault == "bgr" else self.rgb
        if fault == "zero_byte_pad":
            rgb = np.pad(rgb, ((0, 0), (3, 3), (3, 3), (0, 0)))
            pad = 0
        else:
            assert fault in ("", "bgr"), fault
            pad = 3
        x = f16(self.normalised(rgb, torch.float32))
        acc = F.conv2d(x, f16(torch.from_numpy(self.w)), None, stride=2, padding=pad) * v(self.scale) + v(self.shift)
        return f16(F.relu(acc)).numpy()


# ------------------------------------------------------------------------------------------ max pool
POOL_SHAPES = [(1, 32, 7, 9), (2, 16, 32, 32), (1, 16, 8, 5)]          # (N, C, H, W): odd and even sizes


def pool_input(N, C, H, W, seed=0) -> np.ndarray:
    """All negative in image 0 (a zero padding would win every border maximum), mixed signs behind it."""
    g = np.random.default_rng(2000 + seed + H)
    x = g.normal(0, 1, (N, C, H, W))
    x[0] = -np.abs(x[0]) - 0.25
    return x.astype(np.float16)


def pool_ref(x: np.ndarray, fault: str = "") -> np.ndarray:
    t = torch.from_numpy(x.astype(np.float64))
    if fault == "zero_pad":
        return F.max_pool2d(F.pad(t, (1, 1, 1, 1)), 3, 2, 0).numpy()
    assert not fault
    return F.max_pool2d(t, 3, 2, 1).numpy()


# ------------------------------------------------------------------------------------------ global average pool
GAP_SHAPES = [(n, c, p) for c in (128, 512) for p in (4, 9, 256, 4096) for n in (1, 3)]


def gap_input(N, C, P, seed=0) -> np.ndarray:
    """(N, C, P, 1) float16: post-ReLU-like (positive mean: every rounding of a partial sum counts) with some signed channels."""
    g = np.random.default_rng(3000 + seed + P + C)
    x = np.abs(g.normal(0, 2.0, (N, C, P, 1)))
    x[:, ::5] = g.normal(0, 30.0, (N, (C + 4) // 5, P, 1))
    return x.astype(np.float16)


def gap_ref_tol(x: np.ndarray):
    P = x.shape[2]
    x64 = x.astype(np.float64)
    ref = x64.mean(2, keepdims=True)
    tol = 2.0 ** -10 * np.abs(ref) + 2.0 ** -24 * math.ceil(math.log2(P)) * np.abs(x64).mean(2, keepdims=True) + F16_FLOOR
    return ref, tol


def gap_model(x: np.ndarray, fault: str = "") -> np.ndarray:
    """The kernel's tree in float32: pixel p = q + 128 i; adjacent pairs over i (5 levels), then halves over q (7 levels); sum / P.
    `fault` "padded_p": divided by P rounded up to the 128 pixels of a pass."""
    N, C, P, _ = x.shape
    a = np.zeros((N, C, GAP_MAX_P), np.float32)
    a[..., :P] = x[..., 0].astype(np.float32)
    a = a.reshape(N, C, GAP_MAX_P // 128, 128)
    while a.shape[2] > 1:
        a = a[:, :, 0::2] + a[:, :, 1::2]
    a = a[:, :, 0]
    s = 64
    while s >= 1:
        a = a[..., :s] + a[..., s:2 * s]
        s //= 2
    div = np.float32(P if fault != "padded_p" else (P + 127) // 128 * 128)
    assert fault in ("", "padded_p")
    return (a / div).astype(np.float16).astype(np.float32).reshape(N, C, 1, 1)


# ------------------------------------------------------------------------------------------ channel gate
GATE_FORMS = {"arm32": dict(b=True, r=False, plus1=False), "arm16": dict(b=False, r=True, plus1=False), "ffm": dict(b=False, r=False, plus1=True)}


class Gate:
    def __init__(self, form, N=2, C=32, P=35, seed=0):
        g = np.random.default_rng(4000 + seed + len(form) + P)
        f = GATE_FORMS[form]
        self.form, self.N, self.C, self.P, self.plus1 = form, N, C, P, f["plus1"]
        self.x = g.normal(0, 3.0, (N, C, P, 1)).astype(np.float16)
        self.a = g.normal(0, 4.0, (N, C, 1, 1)).astype(np.float16)
        self.a[0, :4, 0, 0] = [0.0, 30.0, -30.0, 12.0]                # s'(a) |a| = 0 or vanishing: the fp32 term carries the bound
        self.b = g.normal(0, 2.0, (N, C, 1, 1)).astype(np.float16) if f["b"] else None
        self.r = g.normal(0, 2.0, (N, C, P, 1)).astype(np.float16) if f["r"] else None
        if self.r is not None:                                        # cancelling terms in one channel
            self.r[1, 5] = (-self.x[1, 5].astype(np.float32) / (1 + np.exp(-self.a[1, 5].astype(np.float32)))).astype(np.float16)

    def ref_tol(self):
        x, a = self.x.astype(np.float64), self.a.astype(np.float64)
        sg = 1.0 / (1.0 + np.exp(-a))
        g = sg + (1.0 if self.plus1 else 0.0)
        ref = x * g
        mag = np.abs(x) * g
        for t in (self.b, self.r):
            if t is not None:
                ref = ref + t.astype(np.float64)
                mag = mag + np.abs(t.astype(np.float64))
        tol = 2.0 ** -10 * np.abs(ref) + 2.0 ** -10 * np.abs(x) * sg * (1 - sg) * np.abs(a) + 2.0 ** -22 * mag + F16_FLOOR
        return ref, tol

    def model(self, fault: str = "") -> np.ndarray:
        """float32 throughout, one rounding; `fault` "no_plus1": the FFM form without its + feat."""
        assert fault in ("", "no_plus1")
        x, a = self.x.astype(np.float32), self.a.astype(np.float32)
        g = np.float32(1) / (np.float32(1) + np.exp(-a))
        if self.plus1 and fault != "no_plus1":
            g = g + np.float32(1)
        v = x * g
        if self.b is not None:
            v = v + self.b.astype(np.float32)
        if self.r is not None:
            v = v + self.r.astype(np.float32)
        return v.astype(np.float16).astype(np.float32)


# ------------------------------------------------------------------------------------------ segmentation head
SEG_SHAPES = [(2, 2, 2), (2, 8, 8), (1, 64, 64)]                       # (N, h, w) -> 8h x 8w
SEG_MARGIN = 2.0 ** -20
SEG_MAX_EXCLUDED = 1e-3


def seg_input(N, h, w, seed=0, ties=False) -> np.ndarray:
    """(N, 32, h, w) float16 logits.  Channels 19..31 (the padding of the 1x1 head) hold what must never win: large values.  One region
    of image 0 has every real logit negative (a zero in a padded channel would win there).  `ties`: classes 3, 7 and 12 carry the same
    map, above every other class: the label is 3 everywhere."""
    g = np.random.default_rng(5000 + seed + h)
    lo = g.normal(0, 1, (N, 32, max(h // 4, 1) + 1, max(w // 4, 1) + 1))
    x = F.interpolate(torch.from_numpy(lo), (h, w), mode="bilinear", align_corners=True).numpy() * 40 + g.normal(0, 4, (N, 32, h, w))
    x[0, :N_CLASSES, : (h + 1) // 2, : (w + 1) // 2] = -np.abs(x[0, :N_CLASSES, : (h + 1) // 2, : (w + 1) // 2]) - 1
    if ties:
        top = np.abs(x[:, :N_CLASSES]).max(1) + g.uniform(1, 5, (N, h, w))
        for c in (3, 7, 12):
            x[:, c] = top
    x[:, N_CLASSES:] = np.abs(x[:, N_CLASSES:]) + 300
    x[:, N_CLASSES::2] = 0                                            # what a padded output channel really holds
    return x.astype(np.float16)


def seg_logits(x: np.ndarray, dtype=torch.float64, align_corners=True, classes=N_CLASSES) -> torch.Tensor:
    t = torch.from_numpy(x[:, :classes].astype(np.float64)).to(dtype)
    h, w = x.shape[2:]
    return F.interpolate(t, (8 * h, 8 * w), mode="bilinear", align_corners=align_corners)


def seg_ref(x: np.ndarray):
    """-> (float64 labels, the mask of pixels whose float64 top-2 margin exceeds 2^-20 max |logit| of the image)"""
    up = seg_logits(x)
    top2 = up.topk(2, dim=1).values
    margin = (top2[:, 0] - top2[:, 1]).numpy()
    mx = np.abs(x[:, :N_CLASSES].astype(np.float64)).max(axis=(1, 2, 3))[:, None, None]
    return up.argmax(1).numpy().astype(np.uint8), margin > SEG_MARGIN * mx


def seg_model(x: np.ndarray, fault: str = "") -> np.ndarray:
    """float32 interpolation, first index wins; `fault`: "half_pixel" (align_corners=False), "last_tie", "all32" (argmax over the 32
    layout channels)."""
    assert fault in ("", "half_pixel", "last_tie", "all32")
    up = seg_logits(x, torch.float32, align_corners=fault != "half_pixel", classes=32 if fault == "all32" else N_CLASSES).numpy()
    if fault == "last_tie":
        return (up.shape[1] - 1 - up[:, ::-1].argmax(1)).astype(np.uint8)
    return up.argmax(1).astype(np.uint8)


def seg_check(dev: np.ndarray, x: np.ndarray) -> dict:
    ref, decided = seg_ref(x)
    excluded = 1.0 - float(decided.mean())
    wrong = int(((dev != ref) & decided).sum())
    fig = dict(excluded=excluded, wrong=wrong, differ=int((dev != ref).sum()))
    assert excluded <= SEG_MAX_EXCLUDED, f"{excluded:.4%} of the pixels are inside the margin"
    assert wrong == 0, f"{wrong} labels differ from float64 outside the margin"
    assert int(dev.max()) < N_CLASSES, "a padded channel won"
    return fig
