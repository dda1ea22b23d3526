"""Float64 restatement of the Ultralight generator for the tests (TEST INFRASTRUCTURE ONLY).

Restates, as functional F.conv2d calls over a layer table,
  avatars/ultralight/unet.py:7-36    InvertedResidual (1x1 expand + BN + ReLU, 3x3 depthwise + BN + ReLU, 1x1 project + BN, + x)
  avatars/ultralight/unet.py:38-49   DoubleConvDW
  avatars/ultralight/unet.py:72-87   Up (bilinear x2, align_corners=True; F.pad is a no-op at 160 x 160; cat([up, skip]))
  avatars/ultralight/unet.py:132-166 AudioConvHubert
  avatars/ultralight/unet.py:198-215 Model.forward
  avatars/ultralight_avatar.py:150-171 the 6-channel input and the * 255 output
tests/golden/ultralight_golden.npz (scripts/gen_golden_ultralight.py) pins it to the reference's own Model(6, 'hubert').

Tap names are the state_dict prefixes of the convs; a conv's tap is the tensor after its BatchNorm, its ReLU where it has one,
and the residual add where the block has one (what one launch of the engine writes).  "<block>.up" is an upsample's output,
"outc.conv" the sigmoid output.

`force` is the hook protocol of oracle/wav2lip_oracle.py and oracle/musetalk_oracle.py (the op-by-op replay, oracle/op_replay.py):
force.describe(name, op) before an op (where it has that method), force(name, ref) -> tensor or None after it; the forward goes on
with the tensor returned.  Names are the tap names and "audio_feat", the features as the device takes them in.  Op descriptions:
  ul_conv  dense conv + BatchNorm: p, bn, x, stride, pad, relu, res (None or the tensor added behind the BatchNorm)
  ul_dw    depthwise 3x3 + BatchNorm + ReLU: p, bn, x, stride          ul_in    inc.inconv.0.conv.0 (1x1 on the 6-channel input): p, bn, x
  ul_up    bilinear x2, align_corners=True: x                          ul_feat  the feature chunk: x          ul_head  outc + sigmoid: p, x
Without a hook the forward is what it was, bit for bit.

`fp16_model=True` is the rounding model of an fp16 implementation the frame tests measure against: weights rounded to fp16,
and the output of every BatchNorm, every biased conv and every upsample rounded to fp16; everything else stays float64.
"""
from __future__ import annotations

from typing import Dict, Optional

import numpy as np
import torch
import torch.nn.functional as F

BN_EPS = 1e-5
RES = 160

# DoubleConvDW blocks: (prefix, cin, cout, stride)
DOWN = [("down1.maxpool_conv.0", 32, 64, 2), ("down2.maxpool_conv.0", 64, 128, 2), ("down3.maxpool_conv.0", 128, 256, 2),
        ("down4.maxpool_conv.0", 256, 512, 2)]
FUSE = [("fuse_conv.0", 1024, 512, 1), ("fuse_conv.1", 512, 256, 1)]
UP = [("up1", 512, 128), ("up2", 256, 64), ("up3", 128, 32), ("up4", 64, 32)]
# audio tower: ("ir", prefix, cin, cout, residual) | ("conv", conv, bn, cin, cout, stride, pad)
AUDIO = [("ir", "audio_model.conv1", 16, 64, False), ("ir", "audio_model.conv2", 64, 128, False),
         ("conv", "audio_model.conv3", "audio_model.bn3", 128, 256, 2, 1), ("ir", "audio_model.conv4", 256, 256, True),
         ("conv", "audio_model.conv5", "audio_model.bn5", 256, 512, 2, 3), ("ir", "audio_model.conv6", 512, 512, True),
         ("ir", "audio_model.conv7", 512, 512, True)]


def conv_prefixes():
    """Every state_dict prefix that holds a conv weight, in execution order."""
    out = []

    def ir(p):
        out.extend([p + ".conv.0", p + ".conv.3", p + ".conv.6"])

    def dconv(p):
        ir(p + ".double_conv.0"); ir(p + ".double_conv.1")

    ir("inc.inconv.0")
    for p, *_ in DOWN:
        dconv(p)
    for item in AUDIO:
        ir(item[1]) if item[0] == "ir" else out.append(item[1])
    for p, *_ in FUSE:
        dconv(p)
    for p, *_ in UP:
        dconv(p + ".conv")
    out.append("outc.conv")
    return out


class _Net:
    def __init__(self, sd, dtype, fp16_model, taps, force=None):
        self.sd = {k: torch.as_tensor(np.asarray(v)) for k, v in sd.items()}
        self.dtype, self.h, self.taps, self.force = dtype, fp16_model, taps, force

    def r16(self, t):
        return t.half().to(self.dtype) if self.h else t

    def w(self, name):
        t = self.sd[name].to(torch.float32)
        return (t.half() if self.h else t).to(self.dtype)

    def bn(self, x, p):
        g, b = self.sd[p + ".weight"].to(self.dtype), self.sd[p + ".bias"].to(self.dtype)
        m, v = self.sd[p + ".running_mean"].to(self.dtype), self.sd[p + ".running_var"].to(self.dtype)
        y = (x - m[None, :, None, None]) / torch.sqrt(v[None, :, None, None] + BN_EPS) * g[None, :, None, None] + b[None, :, None, None]
        return self.r16(y)

    def forced(self, name, t, op):
        if self.force is None:
            return t
        if hasattr(self.force, "describe"):
            self.force.describe(name, op)
        r = self.force(name, t)
        return t if r is None else r

    def tap(self, name, t, op=None):
        t = self.forced(name, t, op)
        if self.taps is not None:
            self.taps[name] = t.detach().to(torch.float64).numpy().copy()
        return t

    def ir(self, p, x, stride, residual):
        f = self.force is not None
        e = self.tap(p + ".conv.0", F.relu(self.bn(F.conv2d(x, self.w(p + ".conv.0.weight")), p + ".conv.1")),
                     f and (dict(kind="ul_in", p=p + ".conv.0", bn=p + ".conv.1", x=x) if x.shape[1] == 6 else
                            dict(kind="ul_conv", p=p + ".conv.0", bn=p + ".conv.1", x=x, stride=1, pad=0, relu=True, res=None)))
        wd = self.w(p + ".conv.3.weight")
        d = self.tap(p + ".conv.3", F.relu(self.bn(F.conv2d(e, wd, stride=stride, padding=1, groups=wd.shape[0]), p + ".conv.4")),
                     f and dict(kind="ul_dw", p=p + ".conv.3", bn=p + ".conv.4", x=e, stride=stride))
        y = self.bn(F.conv2d(d, self.w(p + ".conv.6.weight")), p + ".conv.7")
        return self.tap(p + ".conv.6", x + y if residual else y,
                        f and dict(kind="ul_conv", p=p + ".conv.6", bn=p + ".conv.7", x=d, stride=1, pad=0, relu=False, res=x if residual else None))

    def dconv(self, p, x, stride):
        return self.ir(p + ".double_conv.1", self.ir(p + ".double_conv.0", x, stride, False), 1, True)

    def forward(self, img6, feat):
        x = self.ir("inc.inconv.0", img6, 1, False)
        skips = [x]
        for p, _, _, s in DOWN:
            x = self.dconv(p, x, s)
            skips.append(x)
        a = self.forced("audio_feat", feat, dict(kind="ul_feat", x=feat))
        for item in AUDIO:
            if item[0] == "ir":
                a = self.ir(item[1], a, 1, item[4])
            else:
                _, conv, norm, _, _, stride, pad = item
                a_in = a
                a = self.r16(F.conv2d(a, self.w(conv + ".weight"), self.sd[conv + ".bias"].to(self.dtype), stride=stride, padding=pad))
                a = self.tap(conv, F.relu(self.bn(a, norm)), dict(kind="ul_conv", p=conv, bn=norm, x=a_in, stride=stride, pad=pad, relu=True, res=None))
        x = torch.cat([skips.pop(), a], dim=1)
        for p, _, _, s in FUSE:
            x = self.dconv(p, x, s)
        for p, _, _ in UP:
            u = self.tap(p + ".up", self.r16(F.interpolate(x, scale_factor=2, mode="bilinear", align_corners=True)), dict(kind="ul_up", x=x))
            x = self.dconv(p + ".conv", torch.cat([u, skips.pop()], dim=1), 1)
        logits = F.conv2d(x, self.sd["outc.conv.weight"].to(self.dtype) if not self.h else self.w("outc.conv.weight"),
                          self.sd["outc.conv.bias"].to(self.dtype))
        return self.tap("outc.conv", torch.sigmoid(logits), dict(kind="ul_head", p="outc.conv", x=x))


def forward(sd: Dict[str, np.ndarray], img6: np.ndarray, feat: np.ndarray, dtype=torch.float64, fp16_model: bool = False,
            taps: Optional[dict] = None, force=None) -> np.ndarray:
    """Model(6, 'hubert').forward: img6 (B, 6, 160, 160) in [0, 1], feat (B, 16, 32, 32) -> sigmoid output (B, 3, 160, 160)
    as a float64 array, computed in `dtype`.  force: the hook of the op-by-op replay (module docstring)."""
    with torch.no_grad():
        net = _Net(sd, dtype, fp16_model, taps, force)
        x = torch.as_tensor(np.asarray(img6)).to(dtype)
        a = torch.as_tensor(np.asarray(feat)).to(dtype).reshape(-1, 16, 32, 32)
        if fp16_model:
            x, a = net.r16(x), net.r16(a)
        return net.forward(x, a).to(torch.float64).numpy()


def frames_u8(pred: np.ndarray) -> np.ndarray:
    """avatars/ultralight_avatar.py:170,181: pred (B, 3, H, W) float32 -> (pred.transpose(0, 2, 3, 1) * 255).astype(uint8)."""
    p = np.asarray(pred, dtype=np.float32).transpose(0, 2, 3, 1) * np.float32(255.0)
    return p.astype(np.uint8)


def img6_from_faces(faces) -> np.ndarray:
    """avatars/ultralight_avatar.py:150-161 for a list of 168x168 BGR uint8 faces -> float32 (n, 6, 160, 160)."""
    out = []
    for f in faces:
        real = np.asarray(f)[4:164, 4:164].copy()
        masked = real.copy()
        masked[5:150, 5:155] = 0          # cv2.rectangle(img, (5, 5, 150, 145), (0, 0, 0), -1): Rect x, y, w, h, corners inclusive
        out.append(np.concatenate([real.transpose(2, 0, 1).astype(np.float32) / 255.0, masked.transpose(2, 0, 1).astype(np.float32) / 255.0]))
    return np.stack(out).astype(np.float32)


def frame_stats(got_u8: np.ndarray, ref_u8: np.ndarray):
    """(max LSB, PSNR dB, share of differing bytes) of two uint8 frame stacks."""
    d = np.abs(got_u8.astype(np.int32) - ref_u8.astype(np.int32))
    mse = float((d.astype(np.float64) ** 2).mean())
    psnr = 99.0 if mse == 0 else float(10 * np.log10(255.0 ** 2 / mse))
    return int(d.max()), psnr, float((d != 0).mean())


# ---------------------------------------------------------------------------------------------------- op replay
def replay_ultralight(sd, img6, feat, fetch, only=None, fused=None):
    """The teacher-forced float64 replay (oracle/op_replay.py) of one pass.  sd: the float32 state dict; img6 (B, 6, 160, 160) float32
    as the pass took it in (or img6_from_faces of the bank faces it gathered); feat (B, 16, 32, 32): the float32 features the device
    read; fetch(name, ref) -> the device's tensor of that name in ref's shape and dtype.  The consumer of a concat sees the
    concatenation of the device's own two tensors.  fused: {name: what stands for it} for an op whose tensor the pass does not keep
    (outc.conv when the pass writes uint8 frames): fetch returns None there and the op's description, the device's own input in it,
    is left in Replay.fused.  -> the Replay (records, one per op)."""
    from oracle import op_replay as R
    rp = R.Replay({k: torch.as_tensor(np.asarray(v)) for k, v in sd.items()}, fetch, only=only)
    rp.may_fuse = dict(fused or {})
    forward(sd, np.asarray(img6, dtype=np.float32), np.asarray(feat, dtype=np.float32), force=rp)
    return rp


def op_names():
    """The ops of the device program in execution order (Engine.ultralight_ops): a tap per launch."""
    out = []

    def ir(p):
        out.extend([p + ".conv.0", p + ".conv.3", p + ".conv.6"])

    def dconv(p):
        ir(p + ".double_conv.0"); ir(p + ".double_conv.1")

    ir("inc.inconv.0")
    for p, *_ in DOWN:
        dconv(p)
    out.append("audio_feat")
    for item in AUDIO:
        ir(item[1]) if item[0] == "ir" else out.append(item[1])
    for p, *_ in FUSE:
        dconv(p)
    for p, *_ in UP:
        out.append(p + ".up")
        dconv(p + ".conv")
    return out + ["outc.conv"]


# ---------------------------------------------------------------------------------------------------- the launch program, symbolically
# the inverted residuals the program runs as one launch under knob UL_FUSE_IR (input map >= 32 x 32 and the planner accepts them)
FUSED = ["down1.maxpool_conv.0.double_conv.0", "down1.maxpool_conv.0.double_conv.1", "down2.maxpool_conv.0.double_conv.0",
         "down2.maxpool_conv.0.double_conv.1", "down3.maxpool_conv.0.double_conv.0", "audio_model.conv1", "audio_model.conv2",
         "up2.conv.double_conv.0", "up2.conv.double_conv.1", "up3.conv.double_conv.0", "up3.conv.double_conv.1",
         "up4.conv.double_conv.0", "up4.conv.double_conv.1"]


def _c16(c):
    return (c + 15) // 16 * 16


def expected_reads(fuse: bool):
    """What every launch reads, from the layer tables alone: {op name: (input, residual)}, each a list of (producer, layout channels)
    in channel order (torch.cat order); [] where the op reads the caller's tables or has no residual."""
    reads = {}

    def ir(p, src, cout, residual):
        mid = 2 * sum(c for _, c in src) if src else 12           # (inc: 6 input channels from the bank crop)
        res = src if residual else []
        if fuse and p in FUSED:
            reads[p + ".conv.6"] = (src, res)
        else:
            reads[p + ".conv.0"] = (src, [])
            reads[p + ".conv.3"] = ([(p + ".conv.0", _c16(mid))], [])
            reads[p + ".conv.6"] = ([(p + ".conv.3", _c16(mid))], res)
        return [(p + ".conv.6", cout)]

    def dconv(p, src, cout):
        return ir(p + ".double_conv.1", ir(p + ".double_conv.0", src, cout, False), cout, True)

    x = ir("inc.inconv.0", [], 32, False)
    skips = [x]
    for p, _, cout, _ in DOWN:
        x = dconv(p, x, cout)
        skips.append(x)
    reads["audio_feat"] = ([], [])
    a = [("audio_feat", 16)]
    for item in AUDIO:
        if item[0] == "ir":
            a = ir(item[1], a, item[3], item[4])
        else:
            reads[item[1]] = (a, [])
            a = [(item[1], item[4])]
    x = skips.pop() + a
    for p, _, cout, _ in FUSE:
        x = dconv(p, x, cout)
    for p, _, cout in UP:
        reads[p + ".up"] = (x, [])
        x = dconv(p + ".conv", [(p + ".up", x[0][1])] + skips.pop(), cout)
    reads["outc.conv"] = (x, [])
    return reads


def program_reads(ops):
    """The same from a listing (Engine.ul_program(...)["ops"]), walked on the host: every op stamps its name on the channels of its
    output view; a reader collects the stamps on its input and residual views.  A buffer is one tensor of (ld, H, W) at a time: a write
    in another shape clobbers it, a read in another shape sees "<stale>"."""
    bufs = {}           # buffer -> [(ld, H, W), {channel: stamp}]

    def read(buf, ld, coff, n, H, W):
        if buf < 0:
            return []
        shape, ch = bufs.get(buf, (None, {}))
        runs = []
        for c in range(coff, coff + n):
            s = ch.get(c, "<unwritten>") if shape == (ld, H, W) else "<stale>"
            if runs and runs[-1][0] == s:
                runs[-1][1] += 1
            else:
                runs.append([s, 1])
        return [(s, k) for s, k in runs]

    out = {}
    for o in ops:
        assert o["name"] not in out, o["name"]
        out[o["name"]] = (read(o["in_buf"], o["in_ld"], o["in_coff"], o["cin"], o["H"], o["W"]),
                          read(o["res_buf"], o["res_ld"], o["res_coff"], o["C"], o["Ho"], o["Wo"]))
        if o["out_buf"] >= 0:
            shape = (o["out_ld"], o["Ho"], o["Wo"])
            if bufs.get(o["out_buf"], (None,))[0] != shape:
                bufs[o["out_buf"]] = [shape, {}]
            for c in range(o["out_coff"], o["out_coff"] + o["C"]):
                bufs[o["out_buf"]][1][c] = o["name"]
    return out


def check_dataflow(ops, fuse: bool):
    """AssertionError unless every launch of the listing reads exactly the producers the layer tables imply."""
    got, want = program_reads(ops), expected_reads(fuse)
    assert list(got) == list(want), "op order"
    for name in want:
        assert got[name] == (list(map(tuple, want[name][0])), list(map(tuple, want[name][1]))), (name, got[name], want[name])
