"""BiSeNet's main output path (avatars/musetalk/utils/face_parsing/model.py BiSeNet.forward()[0], resnet.py) restated over a
state dict, as ONE op walk that three evaluators share.  CPU code, test infrastructure only.

walk(sd, rgb, ops) names every op as a program over csrc/parse_kernels.hip and the conv library launches it (one name per launch: a conv's
name stands for the tensor behind its BatchNorm, ReLU and residual add; csrc/faceparse.hip fp_program is the same list) and hands it to
`ops`.  Chain is the evaluator:

  Chain(sd, "ref")   the float64 forward, nothing rounded (BatchNorm from the raw statistics): held to the reference's own BiSeNet by
                     tests/golden/faceparse_golden.npz
  Chain(sd, "mod")   the unforced rounding model: fp16 weights, fp32 sums, every op's output rounded to fp16, BatchNorm folded in
                     float32 as the engine's loaders fold it (state_dict.h fold_bn); end_to_end() takes tau from the two
"""
from __future__ import annotations

import numpy as np
import torch
import torch.nn.functional as F

import faceparse_cases as FP

EPS = 1e-5
OP_TYPES = {"conv": 0, "stem": 10, "maxpool": 11, "gap": 12, "gate": 13, "labels": 14}


def _t(a, dtype=torch.float64):
    return torch.from_numpy(np.asarray(a)).to(dtype)


def _bn(sd, bn, cout, dtype):
    """-> (scale, shift) of the eval-mode BatchNorm `bn` (None: identity), computed in `dtype`"""
    if bn is None:
        return torch.ones(cout, dtype=dtype), torch.zeros(cout, dtype=dtype)
    g, b, m, v = (_t(sd[bn + s], dtype) for s in (".weight", ".bias", ".running_mean", ".running_var"))
    scale = g / torch.sqrt(v + torch.tensor(EPS, dtype=dtype))
    return scale, (-m) * scale + b


def walk(sd, rgb, ops):
    """rgb: uint8 (N, S, S, 3).  -> what ops.labels returns."""
    x = ops.stem("cp.resnet.conv1", rgb, "cp.resnet.conv1", "cp.resnet.bn1")
    x = ops.maxpool("cp.resnet.maxpool", x)
    feats = []
    for l in range(4):
        for b in range(2):
            p = f"cp.resnet.layer{l + 1}.{b}"
            down = l > 0 and b == 0
            st = 2 if down else 1
            mid = ops.conv(p + ".conv1", x, p + ".conv1", p + ".bn1", stride=st, relu=True)
            sc = ops.conv(p + ".downsample.0", x, p + ".downsample.0", p + ".downsample.1", stride=st, relu=False) if down else x
            x = ops.conv(p + ".conv2", mid, p + ".conv2", p + ".bn2", relu=True, res=sc)
        feats.append(x)
    _, feat8, feat16, feat32 = feats

    def arm(p, x):
        feat = ops.conv(p + ".conv", x, p + ".conv.conv", p + ".conv.bn", relu=True)
        a = ops.gap(p + ".avg", feat)
        return feat, ops.conv(p + ".conv_atten", a, p + ".conv_atten", p + ".bn_atten", relu=False)

    avg = ops.conv("cp.conv_avg", ops.gap("cp.avg", feat32), "cp.conv_avg.conv", "cp.conv_avg.bn", relu=True)
    f32, a32 = arm("cp.arm32", feat32)
    s32 = ops.gate("cp.feat32_sum", f32, a32, b=avg)
    up32 = ops.conv("cp.conv_head32", s32, "cp.conv_head32.conv", "cp.conv_head32.bn", relu=True, ups=True)
    f16_, a16 = arm("cp.arm16", feat16)
    s16 = ops.gate("cp.feat16_sum", f16_, a16, r=up32)
    up16 = ops.conv("cp.conv_head16", s16, "cp.conv_head16.conv", "cp.conv_head16.bn", relu=True, ups=True)
    ff = ops.conv("ffm.convblk", torch.cat([feat8, up16], 1), "ffm.convblk.conv", "ffm.convblk.bn", relu=True)
    fa = ops.conv("ffm.conv1", ops.gap("ffm.avg", ff), "ffm.conv1", None, relu=True)
    fa = ops.conv("ffm.conv2", fa, "ffm.conv2", None, relu=False)
    fuse = ops.gate("ffm", ff, fa, plus1=True)
    mid = ops.conv("conv_out.conv", fuse, "conv_out.conv.conv", "conv_out.conv.bn", relu=True)
    logits = ops.conv("conv_out.conv_out", mid, "conv_out.conv_out", None, relu=False)
    return ops.labels("labels", logits)


class Chain:
    """kind "ref": the float64 forward; "mod": the fp16-rounded float32 chain.  run(rgb) -> logits (N, 19, S/8, S/8) float64.
    self.ops: one dict per op in walk order - name, type, the output's shape, and a conv's cin / cout / k / stride / relu / ups / has_res
    and input map - what tests/test_faceparse_host.py holds ltk_debug_face_parse_program to."""

    def __init__(self, sd, kind):
        assert kind in ("ref", "mod")
        self.sd, self.kind, self.ops = sd, kind, []

    def run(self, rgb):
        self.ops = []
        return walk(self.sd, rgb, self)

    def _done(self, name, kind, ref, mod, **info):
        out = ref if self.kind == "ref" else mod
        self.ops.append(dict(name=name, type=OP_TYPES[kind], shape=tuple(out.shape), **info))
        return out

    def stem(self, name, rgb, conv, bn):
        c = object.__new__(FP.Stem)
        c.rgb, c.w = np.ascontiguousarray(rgb), np.asarray(self.sd[conv + ".weight"], np.float32)
        c.N, c.H, c.W = rgb.shape[:3]
        if self.kind == "mod":
            sc, sf = _bn(self.sd, bn, 64, torch.float32)
            c.scale, c.shift = sc.numpy(), sf.numpy()
            return self._done(name, "stem", None, _t(c.model()))
        sc, sf = _bn(self.sd, bn, 64, torch.float64)
        c.scale, c.shift = sc.numpy(), sf.numpy()
        return self._done(name, "stem", _t(c.ref_tol()[0]), None)

    def maxpool(self, name, x):
        ref = F.max_pool2d(x, 3, 2, 1)
        return self._done(name, "maxpool", ref, ref)

    def conv(self, name, x, conv, bn, stride=1, relu=False, res=None, ups=False):
        W = _t(self.sd[conv + ".weight"])
        cout, cin, k, _ = W.shape
        if ups:
            x = F.interpolate(x, scale_factor=2, mode="nearest")
        kw = dict(stride=stride, padding=k // 2)
        v = lambda t: t[None, :, None, None]
        info = dict(cin=cin, cout=cout, k=k, stride=stride, relu=int(relu), ups=int(ups), has_res=int(res is not None), hw=tuple(x.shape[2:]))
        if self.kind == "ref":
            sc, sf = _bn(self.sd, bn, cout, torch.float64)
            ref = F.conv2d(x, W, None, **kw) * v(sc) + v(sf)
            ref = ref if res is None else ref + res
            return self._done(name, "conv", F.relu(ref) if relu else ref, None, **info)
        sc32, sf32 = _bn(self.sd, bn, cout, torch.float32)
        acc = F.conv2d(x.float(), FP.f16(W.float()), None, **kw) * v(sc32) + v(sf32)
        acc = acc if res is None else acc + res.float()
        return self._done(name, "conv", None, FP.f16(F.relu(acc) if relu else acc).double(), **info)

    def gap(self, name, x):
        N, C, H, W = x.shape
        if self.kind == "ref":
            return self._done(name, "gap", x.mean((2, 3), keepdim=True), None)
        return self._done(name, "gap", None, _t(FP.gap_model(x.reshape(N, C, H * W, 1).numpy().astype(np.float16))))

    def gate(self, name, x, a, b=None, r=None, plus1=False):
        if self.kind == "ref":
            out = x * (torch.sigmoid(a) + (1.0 if plus1 else 0.0))
        else:
            out = x.float() * (1.0 / (1.0 + torch.exp(-a.float())) + (1.0 if plus1 else 0.0))
        for t in (b, r):
            if t is not None:
                out = out + t.to(out.dtype)
        return self._done(name, "gate", out, FP.f16(out).double() if self.kind == "mod" else None, has_res=int(r is not None), plus1=int(plus1))

    def labels(self, name, logits):
        S = 8 * logits.shape[2]
        self.ops.append(dict(name=name, type=OP_TYPES["labels"], shape=(logits.shape[0], S, S)))
        return logits


def upsampled(logits: torch.Tensor) -> torch.Tensor:
    h, w = logits.shape[2:]
    return F.interpolate(logits, (8 * h, 8 * w), mode="bilinear", align_corners=True)


def end_to_end(sd, rgb):
    """-> (float64 labels, the mask of pixels whose float64 top-2 margin exceeds tau, tau): tau = 2 max |mod - ref| over the logits of the
    two unforced chains."""
    ref, mod = Chain(sd, "ref").run(rgb), Chain(sd, "mod").run(rgb)
    tau = 2.0 * float((mod - ref).abs().max())
    up = upsampled(ref)
    top2 = up.topk(2, dim=1).values
    return up.argmax(1).numpy().astype(np.uint8), ((top2[:, 0] - top2[:, 1]) > tau).numpy(), tau


def op_names():
    """[(name, type)] of the walk, in order (a tiny forward with zero weights is not needed: the names do not depend on the data)."""
    class _Names:
        def __init__(self):
            self.names = []
        def _add(self, name, kind):
            self.names.append((name, OP_TYPES[kind]))
            return torch.zeros(1, 1, 1, 1, dtype=torch.float64)
        def stem(self, name, *a, **k): return self._add(name, "stem")
        def maxpool(self, name, *a, **k): return self._add(name, "maxpool")
        def conv(self, name, *a, **k): return self._add(name, "conv")
        def gap(self, name, *a, **k): return self._add(name, "gap")
        def gate(self, name, *a, **k): return self._add(name, "gate")
        def labels(self, name, *a, **k): return self._add(name, "labels")
    n = _Names()
    walk({}, None, n)
    return n.names
