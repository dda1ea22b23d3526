"""What the face-parser program's tests share (tests/test_face_parse_plan_host.py, tests/test_face_parse_gpu.py).  CPU code.

  * replay_through_views: the rounding chain of tests/faceparse_ref.py run launch by launch through numpy buffers addressed by the
    binding table of Engine.face_parse_plan alone;
  * check_ops: every launch of the list in float64 on the DEVICE's own inputs (read back by name), the device's output held to the
    per-element bound the stand-alone kernel tests use for the op's type (tests/faceparse_cases.py; the library's convs in the dense
    conv form of oracle/op_replay.py: fp16 weights, BatchNorm as an fp32 scale / shift in the epilogue, the residual behind it);
  * E2E: the float64 end-to-end gates of one input set.
"""
from __future__ import annotations

import numpy as np
import torch
import torch.nn.functional as F

import faceparse_cases as FP
import faceparse_ref as R
from oracle.op_replay import C_LIN, F16_FLOOR, short_sum

SEED = 83
EXCLUDED_CAP = 0.05          # the share of pixels inside tau an input set may have for the label gate to say something
DISAGREE_FACTOR = 4.0        # device-against-float64 label disagreement over ALL pixels vs the rounding model's own: a different fp32
                             # summation order moves other near-ties than the model's


def up16(c):
    return (c + 15) // 16 * 16


class Calls:
    """What walk() hands each op beside its tensors: the state-dict names, stride, ReLU, upsample, the gate's form."""

    def __init__(self):
        self.calls = {}
        R.walk({}, None, self)

    def _add(self, name, **kw):
        self.calls[name] = kw
        return torch.zeros(1, 1, 1, 1, dtype=torch.float64)

    def stem(self, name, rgb, conv, bn): return self._add(name, conv=conv, bn=bn)
    def maxpool(self, name, x): return self._add(name)
    def conv(self, name, x, conv, bn, stride=1, relu=False, res=None, ups=False): return self._add(name, conv=conv, bn=bn, stride=stride, relu=relu, ups=ups)
    def gap(self, name, x): return self._add(name)
    def gate(self, name, x, a, b=None, r=None, plus1=False): return self._add(name, plus1=plus1)
    def labels(self, name, logits): return self._add(name)


def replay_through_views(plan, prog, sd, rgb):
    """-> the logits `labels` reads, float64 (N, <= 19, h, w), after every launch of the list has run as Chain(sd, "mod") runs it, on
    inputs taken from - and with its output stored into - numpy buffers addressed by the plan's views alone."""
    calls = Calls().calls
    chain = R.Chain(sd, "mod")
    N = rgb.shape[0]
    arena = {}

    def buf(v):
        if v["buf"] not in arena:
            arena[v["buf"]] = np.zeros((N, v["ld"], v["H"], v["W"]), np.float64)
        a = arena[v["buf"]]
        assert a.shape[1:] == (v["ld"], v["H"], v["W"]), "two views disagree about a buffer"
        return a

    def read(v, c):
        """the first c channels of the view, channels last in memory as the plain chain's tensors are from the stem on (its output
        comes out of a numpy array in that order and every op behind it keeps the format): torch's float32 convolution sums in another
        order on a channels-first tensor, and the comparison is bit for bit"""
        if v is None:
            return None
        return torch.from_numpy(buf(v)[:, v["coff"]:v["coff"] + min(c, v["C"])].copy()).contiguous(memory_format=torch.channels_last)

    for o, p in zip(plan["ops"], prog):
        n, t, kw = p["name"], p["type"], calls[p["name"]]
        if t == 14:
            return read(o["x"], 19).numpy()
        if t == 10:
            assert o["x"]["buf"] == plan["image_buf"]
            out = chain.stem(n, rgb, kw["conv"], kw["bn"])
        elif t == 11:
            out = chain.maxpool(n, read(o["x"], p["cin"]))
        elif t == 12:
            out = chain.gap(n, read(o["x"], p["cin"]))
        elif t == 13:
            out = chain.gate(n, read(o["x"], p["cin"]), read(o["a"], p["cin"]), b=read(o["b"], p["cin"]), r=read(o["r"], p["cin"]), plus1=kw["plus1"])
        else:
            out = chain.conv(n, read(o["x"], p["cin"]), kw["conv"], kw["bn"], stride=kw["stride"], relu=kw["relu"], res=read(o["r"], p["cout"]), ups=kw["ups"])
        y = o["y"]
        assert tuple(out.shape) == (N, p["cout"], y["H"], y["W"]), f"{n}: the op's output does not fit its view"
        dst = buf(y)
        dst[:, y["coff"]:y["coff"] + y["C"]] = 0.0                      # the padding channels of the layout
        dst[:, y["coff"]:y["coff"] + p["cout"]] = out.numpy()
    raise AssertionError("the list has no labels launch")


# ------------------------------------------------------------------------------------------ op by op on the device's own inputs
def conv_ref_tol(x, W, scale, shift, res, stride, relu, ups):
    """float64 tensors; -> (ref, tol): oracle/op_replay.py's dense conv form, 2^-10 |ref| + 2^-12 (short_sum(n) |W| (*) |x| |scale| +
    4 |shift| + 4 |res|) + 2^-24 sum |x| |scale| + 2^-24."""
    if ups:
        x = F.interpolate(x, scale_factor=2, mode="nearest")
    k = W.shape[-1]
    kw = dict(stride=stride, padding=k // 2)
    v = lambda t: t[None, :, None, None]
    ref = F.conv2d(x, W, None, **kw) * v(scale) + v(shift)
    A = short_sum(W.shape[1] * k * k) * F.conv2d(x.abs(), W.abs(), None, **kw) * v(scale).abs() + 4 * v(shift).abs()
    s = 2.0 ** -24 * F.conv2d(x.abs().sum(1, keepdim=True), torch.ones(1, 1, k, k, dtype=torch.float64), None, **kw) * v(scale).abs()
    if res is not None:
        ref = ref + res
        A = A + 4 * res.abs()
    if relu:
        ref = F.relu(ref)
    return ref, 2.0 ** -10 * ref.abs() + C_LIN * A + s + F16_FLOOR


def check_ops(fetch, plan, prog, sd, rgb, labels):
    """fetch(name, shape) -> the device's float32 output of launch `name`; rgb / labels: the images of the run that is read back and
    what ltk_face_parse returned for them.  -> {name: figures} of every launch checked; raises AssertionError naming the launch."""
    calls = Calls().calls
    chain = R.Chain(sd, "mod")
    N = rgb.shape[0]
    outs = {}                                            # buffer -> [(first channel, name, cout)]
    for o, p in zip(plan["ops"], prog):
        if p["type"] != 14:
            outs.setdefault(o["y"]["buf"], []).append((o["y"]["coff"], p["name"], p["cout"]))
    cache = {}

    def dev_of(name, cout, H, W):
        if name not in cache:
            got = np.asarray(fetch(name, (N, cout, H, W)), np.float32)
            assert got.shape == (N, cout, H, W) and np.isfinite(got).all(), name
            assert np.array_equal(got.astype(np.float16).astype(np.float32), got), f"{name}: not fp16 values"
            cache[name] = got
        return cache[name]

    def view(v, c):
        """the device's tensor behind view v, float64 (N, c, H, W): its producers' outputs, in channel order"""
        if v is None:
            return None
        parts = sorted(q for q in outs[v["buf"]] if v["coff"] <= q[0] < v["coff"] + v["C"])
        t = np.concatenate([dev_of(name, cout, v["H"], v["W"]) for _, name, cout in parts], 1)
        assert t.shape[1] >= c, f"view of {[q[1] for q in parts]} has {t.shape[1]} channels, {c} wanted"
        return torch.from_numpy(t[:, :c].astype(np.float64))

    figs = {}
    for o, p in zip(plan["ops"], prog):
        n, t, kw = p["name"], p["type"], calls[p["name"]]
        try:
            if t == 14:
                x = np.zeros((N, 32, p["H"], p["W"]), np.float16)
                x[:, :19] = view(o["x"], 19).numpy()
                figs[n] = FP.seg_check(labels, x)
                continue
            dev = dev_of(n, p["cout"], p["Ho"], p["Wo"]).astype(np.float64)
            if t == 10:
                c = object.__new__(FP.Stem)
                c.rgb, c.w, (c.N, c.H, c.W) = np.ascontiguousarray(rgb), np.asarray(sd[kw["conv"] + ".weight"], np.float32), rgb.shape[:3]
                c.scale, c.shift = (a.numpy() for a in R._bn(sd, kw["bn"], 64, torch.float64))
                ref, tol = c.ref_tol()
                figs[n] = FP.check(dev, ref, chain.stem(n, rgb, kw["conv"], kw["bn"]).numpy(), tol)
            elif t == 11:
                x = view(o["x"], p["cin"]).numpy().astype(np.float16)
                assert np.array_equal(dev, FP.pool_ref(x)), "max pool is not exact"
                figs[n] = dict(worst=0.0)
            elif t == 12:
                x = view(o["x"], p["cin"]).numpy().astype(np.float16).reshape(N, p["cin"], -1, 1)
                ref, tol = FP.gap_ref_tol(x)
                figs[n] = FP.check(dev.reshape(ref.shape), ref, FP.gap_model(x), tol)
            elif t == 13:
                g = object.__new__(FP.Gate)
                C = p["cin"]
                g.x = view(o["x"], C).numpy().astype(np.float16).reshape(N, C, -1, 1)
                g.a = view(o["a"], C).numpy().astype(np.float16).reshape(N, C, 1, 1)
                g.b = None if o["b"] is None else view(o["b"], C).numpy().astype(np.float16).reshape(N, C, 1, 1)
                g.r = None if o["r"] is None else view(o["r"], C).numpy().astype(np.float16).reshape(N, C, -1, 1)
                g.plus1 = bool(kw["plus1"])
                ref, tol = g.ref_tol()
                figs[n] = FP.check(dev.reshape(ref.shape), ref, g.model(), tol)
            else:
                x, res = view(o["x"], p["cin"]), view(o["r"], p["cout"])
                W = torch.from_numpy(np.asarray(sd[kw["conv"] + ".weight"], np.float64))
                scale, shift = R._bn(sd, kw["bn"], p["cout"], torch.float64)
                ref, tol = conv_ref_tol(x, W, scale, shift, res, kw["stride"], kw["relu"], kw["ups"])
                mod = chain.conv(n, x, kw["conv"], kw["bn"], stride=kw["stride"], relu=kw["relu"], res=res, ups=kw["ups"])
                figs[n] = FP.check(dev, ref.numpy(), mod.numpy(), tol.numpy())
        except AssertionError as e:
            raise AssertionError(f"{n} (type {t}): {e}") from e
    return figs


# ------------------------------------------------------------------------------------------ end to end against float64
class E2E:
    """The float64 side of one input set: labels, the pixels whose top-2 margin exceeds tau = 2 max |mod - ref| (twice the rounding
    model's own logit error), the logits, and the model's own label disagreement.  Everything here comes from the two models, nothing
    from the device."""

    def __init__(self, sd, rgb, ref_logits=None, ref_labels=None):
        mod = R.Chain(sd, "mod").run(rgb)
        if ref_logits is None:
            self.labels, self.ok, self.tau = R.end_to_end(sd, rgb)
            self.logits = R.Chain(sd, "ref").run(rgb)
        else:                                            # stored float64 results (tests/golden/faceparse_golden.npz): no float64 forward
            self.logits = torch.from_numpy(np.asarray(ref_logits, np.float64))
            self.tau = 2.0 * float((mod - self.logits).abs().max())
            up = R.upsampled(self.logits)
            top2 = up.topk(2, dim=1).values
            self.labels, self.ok = np.asarray(ref_labels, np.uint8), ((top2[:, 0] - top2[:, 1]) > self.tau).numpy()
            assert np.array_equal(up.argmax(1).numpy().astype(np.uint8), self.labels)
        self.excluded = 1.0 - float(self.ok.mean())
        self.model_disagree = float((R.upsampled(mod).argmax(1).numpy().astype(np.uint8) != self.labels).mean())

    def gates(self, dev_labels, dev_logits, label_gate=True):
        """-> figures; AssertionError with them when a gate fails.  label_gate False: the input set has more than EXCLUDED_CAP of its
        pixels inside tau, and only the logit bound and the disagreement rule are applied."""
        dev_labels = np.asarray(dev_labels)
        assert dev_labels.shape == self.labels.shape and dev_labels.dtype == np.uint8 and int(dev_labels.max()) < 19
        wrong = int(((dev_labels != self.labels) & self.ok).sum())
        err = float(np.abs(np.asarray(dev_logits, np.float64) - self.logits.numpy()).max())
        disagree = float((dev_labels != self.labels).mean())
        fig = dict(tau=self.tau, excluded=self.excluded, wrong=wrong, logit_err=err, disagree=disagree, model_disagree=self.model_disagree)
        print("  " + ", ".join(f"{k} {v:.4g}" for k, v in fig.items()))
        if label_gate:
            assert self.excluded <= EXCLUDED_CAP, f"{self.excluded:.3%} of the pixels are inside tau: the label gate says too little"
            assert wrong == 0, f"{wrong} labels differ from float64 outside tau"
        assert err <= self.tau, f"max |device logits - float64| {err:.4f} beyond tau {self.tau:.4f}"
        assert disagree <= DISAGREE_FACTOR * self.model_disagree, f"labels disagree on {disagree:.3%} of the pixels, the model on {self.model_disagree:.3%}"
        return fig


def record_512(ref: E2E, dev_labels, dev_logits, gated: bool) -> str:
    """The 512 x 512 lines of profiles/face_parse.txt: what the test measured, whether or not its gates passed."""
    dev_labels = np.asarray(dev_labels)
    err = float(np.abs(np.asarray(dev_logits, np.float64) - ref.logits.numpy()).max())
    wrong = int(((dev_labels != ref.labels) & ref.ok).sum())
    disagree = float((dev_labels != ref.labels).mean())
    return (f"512 x 512, the stored image (tests/test_face_parse_gpu.py): tau {ref.tau:.4f}; {ref.excluded:.3%} of the pixels inside tau (cap "
            f"{EXCLUDED_CAP:.0%}: the label gate is {'applied' if gated else 'NOT applied at 512 - the cap stands, 512 is held to the two gates below'}); "
            f"{wrong} labels differ from float64 outside tau\n"
            f"512 x 512: max |device logits - float64| {err:.4f} (bound tau {ref.tau:.4f}); labels disagree with float64 on {disagree:.3%} of all "
            f"pixels, the rounding model on {ref.model_disagree:.3%} (bound {DISAGREE_FACTOR:.0f} x)\n")
