"""What tests/test_ul_merge_host.py (CPU) and tests/test_ul_gconv_gpu.py share: the cases of the grouped dense conv of the Ultralight
program (csrc/ul_gconv.hip: weights, scale and shift chosen per image), their inputs, the channel-blocked buffers with guard blocks,
the float64 reference, the bound, a float32 rounding model, and a simulated device that computes the op as the kernel does and can be
told to get it wrong.  The form of tests/conv_cases.py.

Cases: the smallest shapes that reach every edge of the kernel - N = 3 images on weight sets [0, 1, 0] (images 0 and 2 carry the same
input: they have to come out byte-identical, image 1 has to differ), maps of 10 x 10 (100 = 6 x 16 + 4 pixels: a pixel tail in the
fourth block), 5 x 7 and 1 x 1, Cin in {16, 32, 48, 64} (a k-step is 32 channels: 16 and 48 leave half a step) x Cout in {16, 32, 48}
(a block carries four 16-channel tiles: every count leaves waves without one), the two 3 x 3 stride-2 forms of the audio tower
(8 x 8 -> 4 x 4 at pad 1, 16 x 16 -> 10 x 10 at pad 3), channel views on x, y and the residual, ReLU and residual on / off, N = 1,
and one case whose outputs pass +-65504.

Inputs: x, w and the residual are drawn in fp32 and rounded to fp16, so the device holds them exactly (no loader rounding enters);
scale = U(0.5, 1.5), shift = 0.1 N(0, 1) per set.

Reference: F.conv2d in float64 per image with its own set, then the affine, the residual and the ReLU in float64; clamped to +-65504
as the kernel's one rounding clamps.  Model: the same in float32, rounded to fp16 once.

Bound, the project's own for an Ultralight dense conv (oracle/op_replay.py docstring):
  per element : |dev - ref| <= 2^-10 |ref| + 2^-12 A + s,  A = short_sum(n) |W| (*) |x| |scale| + 4 |shift| + 4 |res|,
                s = 2^-24 sum |x| |scale| + 2^-24,  n = Cin k k;  no violator, NaN / inf is one;
  aggregate   : rel_l2(dev, ref) <= 2 rel_l2(model, ref) + 1e-4.

Buffers (halfs, [N + 1][cbt][H][W][16]; the image past N belongs to nobody): x and res hold GUARD_GAIN x the data's magnitude
everywhere outside the view, so a read outside it dominates the result; y is pre-filled with PATTERN and every half outside the view
has to hold PATTERN afterwards.  Views: x_coff 16 in x_ld Cin + 32, y_coff 32 in y_ld Cout + 48, res_coff 16 in res_ld Cout + 32."""
from __future__ import annotations

from typing import List

import numpy as np
import torch
import torch.nn.functional as F

from oracle import op_replay as R

GUARD_GAIN = 1.0e3
PATTERN = 0x5A5A            # fp16 203.25
F16_MAX = 65504.0
KERNEL = "ul_gconv_kernel"
TILE_PX, TILE_CO = 32, 64   # a block's tile: 2 x 16 pixels of one image, 4 waves x 16 output channels


class Case:
    def __init__(self, N, H, W, Cin, Cout, k=1, stride=1, pad=0, res=False, relu=False, view=False, sets=None, big=False):
        self.N, self.H, self.W, self.Cin, self.Cout, self.k, self.stride, self.pad = N, H, W, Cin, Cout, k, stride, pad
        self.res, self.relu, self.view, self.big = res, relu, view, big
        self.sets = list(sets) if sets is not None else ([0, 1, 0] if N == 3 else [1] * N)
        self.n_sets = 2
        self.Ho = (H + 2 * pad - k) // stride + 1
        self.Wo = (W + 2 * pad - k) // stride + 1
        self.n_prod = Cin * k * k
        # images that carry a copy of image 0's input (same set: byte-identical output)
        self.twins = [n for n in range(1, N) if self.sets[n] == self.sets[0]]

    @property
    def id(self) -> str:
        s = f"{self.N}x{self.H}x{self.W}-{self.Cin}to{self.Cout}-k{self.k}s{self.stride}p{self.pad}"
        return s + ("-res" if self.res else "") + ("-relu" if self.relu else "") + ("-view" if self.view else "") + ("-big" if self.big else "")

    def geometry(self) -> dict:
        gx, gy = -(-self.Ho * self.Wo // TILE_PX), -(-(self.Cout // 16) // 4)
        return dict(kernel=KERNEL, tile_px=TILE_PX, tile_co=TILE_CO, ksteps=self.k * self.k * -(-self.Cin // 32), grid=(gx, gy, self.N),
                    blocks=gx * gy * self.N)


def cases() -> List[Case]:
    out = []
    for ci, cin in enumerate((16, 32, 48, 64)):                       # 1x1: every Cin x Cout on the ragged 10 x 10 map, flags rotating
        for co, cout in enumerate((16, 32, 48)):
            i = ci * 3 + co
            out.append(Case(3, 10, 10, cin, cout, res=i % 2 == 0, relu=i % 3 != 0, view=i % 4 == 1))
    out += [Case(3, 5, 7, 48, 32, res=True, relu=True, view=True), Case(3, 5, 7, 16, 48),
            Case(3, 1, 1, 64, 16, res=True), Case(3, 1, 1, 16, 32, relu=True, view=True),
            Case(1, 10, 10, 48, 48, res=True, relu=True), Case(1, 5, 7, 32, 16, view=True),
            Case(3, 10, 10, 32, 32, res=True, relu=False, view=True),      # residual + view without the ReLU
            Case(3, 10, 10, 32, 16, res=False, relu=True, big=True),        # outputs pass +-65504: clamped, no inf
            Case(3, 10, 10, 32, 16, res=True, relu=False, big=True)]
    for res, relu, view in ((False, True, False), (True, True, True), (True, False, False)):      # the audio tower's two 3x3 stride-2 forms
        out.append(Case(3, 8, 8, 32, 32, k=3, stride=2, pad=1, res=res, relu=relu, view=view))
        out.append(Case(3, 16, 16, 32, 48, k=3, stride=2, pad=3, res=res, relu=relu, view=view))
    out.append(Case(3, 8, 8, 48, 16, k=3, stride=2, pad=1, relu=True))   # the K tail inside a tap loop
    return out


def _h(t: torch.Tensor) -> torch.Tensor:
    return t.half().float()


class Inputs:
    """x (N, Cin, H, W), w (n_sets, Cout, Cin, k, k), res (N, Cout, Ho, Wo) or None: fp16 values in float32; scale, shift (n_sets, Cout)."""

    def __init__(self, c: Case):
        g = torch.Generator().manual_seed(1000 * c.Cin + 10 * c.Cout + c.H * 7 + c.k + 100 * c.N + (5 if c.big else 0))
        self.x = _h(torch.randn(c.N, c.Cin, c.H, c.W, generator=g))
        for n in c.twins:
            self.x[n] = self.x[0]
        self.w = _h(torch.randn(c.n_sets, c.Cout, c.Cin, c.k, c.k, generator=g) * (1.0 / np.sqrt(c.n_prod)))
        self.scale = torch.rand(c.n_sets, c.Cout, generator=g) + 0.5
        self.shift = 0.1 * torch.randn(c.n_sets, c.Cout, generator=g)
        if c.big:
            self.scale = self.scale * 2.0e5              # |acc| ~ 1: most outputs pass the fp16 range
        self.res = None
        if c.res:
            self.res = _h(torch.randn(c.N, c.Cout, c.Ho, c.Wo, generator=g))
            for n in c.twins:
                self.res[n] = self.res[0]


# ---------------------------------------------------------------------------------------------------- buffers
def _to_cb(t: torch.Tensor, cbt: int, cb0: int, fill_bits=None, guard: float = 0.0) -> np.ndarray:
    """NCHW float32 (fp16 values) -> uint16 bits [N + 1][cbt][H][W][16] with the tensor at blocks [cb0, cb0 + C / 16)."""
    N, C, H, W = t.shape
    if fill_bits is not None:
        buf = np.full((N + 1, cbt, H, W, 16), fill_bits, np.uint16)
    else:
        rng = np.random.default_rng(C * 31 + H)
        buf = (guard * (1.0 + rng.random((N + 1, cbt, H, W, 16)))).astype(np.float16).view(np.uint16)
    blk = t.numpy().astype(np.float16).reshape(N, C // 16, 16, H, W).transpose(0, 1, 3, 4, 2)
    buf[:N, cb0:cb0 + C // 16] = blk.view(np.uint16)
    return buf


def _from_cb(buf: np.ndarray, N: int, C: int, cb0: int) -> torch.Tensor:
    blk = buf[:N, cb0:cb0 + C // 16].view(np.float16).astype(np.float32)          # [N][C/16][H][W][16]
    return torch.from_numpy(np.ascontiguousarray(blk.transpose(0, 1, 4, 2, 3))).reshape(N, C, blk.shape[2], blk.shape[3])


class Buffers:
    """The device images of a case's tensors (uint16 bit patterns of fp16) and its views."""

    def __init__(self, c: Case, inp: Inputs):
        self.x_cbt, self.x_cb0 = (c.Cin // 16 + 2, 1) if c.view else (c.Cin // 16, 0)
        self.y_cbt, self.y_cb0 = (c.Cout // 16 + 3, 2) if c.view else (c.Cout // 16, 0)
        self.r_cbt, self.r_cb0 = (c.Cout // 16 + 2, 1) if c.view else (c.Cout // 16, 0)
        self.x = _to_cb(inp.x, self.x_cbt, self.x_cb0, guard=GUARD_GAIN)
        self.res = _to_cb(inp.res, self.r_cbt, self.r_cb0, guard=GUARD_GAIN) if c.res else None
        self.y = np.full((c.N + 1, self.y_cbt, c.Ho, c.Wo, 16), PATTERN, np.uint16)

    def views(self) -> dict:
        return dict(x_ld=self.x_cbt * 16, x_coff=self.x_cb0 * 16, y_ld=self.y_cbt * 16, y_coff=self.y_cb0 * 16, res_ld=self.r_cbt * 16,
                    res_coff=self.r_cb0 * 16)


# ---------------------------------------------------------------------------------------------------- reference, model, bound
def _per_image(c: Case, inp: Inputs, fn):
    return torch.cat([fn(n, c.sets[n]) for n in range(c.N)])


def reference(c: Case, inp: Inputs):
    """-> (ref, tol) in float64, ref clamped to the fp16 range."""
    v = lambda t: t.double()[None, :, None, None]
    kw = dict(stride=c.stride, padding=c.pad)
    ones = torch.ones(1, 1, c.k, c.k, dtype=torch.float64)

    def one(n, s):
        x, W = inp.x[n:n + 1].double(), inp.w[s].double()
        acc = F.conv2d(x, W, None, **kw) * v(inp.scale[s]) + v(inp.shift[s])
        A = R.short_sum(c.n_prod) * F.conv2d(x.abs(), W.abs(), None, **kw) * v(inp.scale[s].abs()) + 4 * v(inp.shift[s].abs())
        sl = 2.0 ** -24 * F.conv2d(x.abs().sum(1, keepdim=True), ones, None, **kw) * v(inp.scale[s].abs()) + 2.0 ** -24
        if c.res:
            r = inp.res[n:n + 1].double()
            acc = acc + r
            A = A + 4 * r.abs()
        if c.relu:
            acc = F.relu(acc)
        return torch.stack([acc, A, sl])

    t = _per_image(c, inp, lambda n, s: one(n, s).transpose(0, 1))          # (N, 3, Cout, Ho, Wo)
    ref, A, sl = t[:, 0].clamp(-F16_MAX, F16_MAX), t[:, 1], t[:, 2]
    return ref, 2.0 ** -10 * ref.abs() + R.C_LIN * A + sl


def model(c: Case, inp: Inputs) -> torch.Tensor:
    """The op in float32 on the same operands, the result clamped and rounded to fp16 once."""
    return SimDevice(c, inp).result()


class SimDevice:
    """ul_gconv_kernel in float32: per image the weights of its set, fp32 sums, acc * scale + shift, the residual behind the affine,
    the ReLU, the clamp, one rounding; the stores skip the pixels past the map.  `fault`: one of FAULTS."""

    def __init__(self, c: Case, inp: Inputs, fault: str = ""):
        assert not fault or fault in FAULTS
        self.c, self.inp, self.fault = c, inp, fault

    def _set_of(self, n):
        c = self.c
        if self.fault == "prev_image_weights":
            return c.sets[n - 1] if n else 1 - c.sets[0]
        if self.fault == "all_set0":
            return 0
        return c.sets[n]

    def result(self) -> torch.Tensor:
        c, inp, f = self.c, self.inp, self.fault
        v = lambda t: t[None, :, None, None]
        out = []
        for n in range(c.N):
            s = self._set_of(n)
            x, W = inp.x[n:n + 1], inp.w[s]
            if f == "drop_k_tail" and c.Cin % 32 == 16:
                x, W = x[:, :c.Cin - 16], W[:, :c.Cin - 16]
            if f == "stride_odd" and c.stride == 2:
                x = F.pad(x, (0, 1, 0, 1))[:, :, 1:, 1:]                      # the window starts one pixel further in
            if x.shape[1] == 0:                                              # Cin = 16 is nothing but the tail
                acc = torch.zeros(1, c.Cout, c.Ho, c.Wo)
            elif f == "pad_replicate" and c.k == 3:
                acc = F.conv2d(F.pad(x, (c.pad,) * 4, mode="replicate"), W, None, stride=c.stride)
            else:
                acc = F.conv2d(x, W, None, stride=c.stride, padding=c.pad)
            r = inp.res[n:n + 1] if c.res else None
            if f == "res_before_affine" and c.res:
                t = (acc + r) * v(inp.scale[s]) + v(inp.shift[s])
            else:
                t = acc * v(inp.scale[s]) + v(inp.shift[s])
                if f == "relu_before_res" and c.res and c.relu:
                    t = F.relu(t)
                if c.res:
                    t = t + r
            if c.relu and not (f == "relu_before_res" and c.res):
                t = F.relu(t)
            out.append(t)
        return _h(torch.cat(out).clamp(-F16_MAX, F16_MAX))

    def run(self, b: Buffers) -> np.ndarray:
        """-> the y buffer as the device would leave it."""
        c = self.c
        y = b.y.copy()
        full = _to_cb(self.result(), b.y_cbt, b.y_cb0, fill_bits=PATTERN)
        y[:c.N, b.y_cb0:b.y_cb0 + c.Cout // 16] = full[:c.N, b.y_cb0:b.y_cb0 + c.Cout // 16]
        if self.fault == "pixel_tail_unwritten" and (c.Ho * c.Wo) % 16:
            flat = y.reshape(c.N + 1, b.y_cbt, c.Ho * c.Wo, 16)
            flat[:c.N, b.y_cb0:b.y_cb0 + c.Cout // 16, (c.Ho * c.Wo) // 16 * 16:] = PATTERN
        return y


# fault -> the cases it shows on
FAULTS = {
    "prev_image_weights": lambda c: c.N > 1,                  # image n takes image n - 1's weight set
    "all_set0": lambda c: any(c.sets),                        # every image takes set 0
    "drop_k_tail": lambda c: c.Cin % 32 == 16,                # the half k-step behind the last full one is dropped
    "pixel_tail_unwritten": lambda c: (c.Ho * c.Wo) % 16 != 0,
    "res_before_affine": lambda c: c.res,
    "relu_before_res": lambda c: c.res and c.relu,
    "pad_replicate": lambda c: c.k == 3,
    "stride_odd": lambda c: c.stride == 2,
}


def check(c: Case, inp: Inputs, b: Buffers, y: np.ndarray, ref=None, tol=None, mod=None) -> dict:
    """Every gate on the y buffer a device (or the simulation) left behind.  -> the figures; raises AssertionError."""
    if ref is None:
        ref, tol = reference(c, inp)
    if mod is None:
        mod = model(c, inp)
    cb1 = b.y_cb0 + c.Cout // 16
    outside = np.ones(y.shape, bool)
    outside[:c.N, b.y_cb0:cb1] = False
    touched = int((y[outside] != PATTERN).sum())
    assert touched == 0, f"{c.id}: {touched} halfs outside the output view were written"
    dev = _from_cb(y, c.N, c.Cout, b.y_cb0).double()
    finite = torch.isfinite(dev)
    err = (dev - ref).abs()
    over = torch.where(finite, err / tol, torch.full_like(err, float("inf")))
    viol = int((over > 1).sum())
    rel_dev = R.rel_l2(torch.where(finite, dev, torch.zeros_like(dev)), ref)
    rel_mod = R.rel_l2(mod, ref)
    fig = dict(violators=viol, worst=float(over.max()), rel_dev=rel_dev, rel_mod=rel_mod, nonfinite=int((~finite).sum()))
    assert fig["nonfinite"] == 0, f"{c.id}: {fig['nonfinite']} non-finite outputs"
    assert viol == 0, f"{c.id}: {viol} of {dev.numel()} elements outside the bound, worst |dev - ref| / tol = {fig['worst']:.2f}"
    assert rel_dev <= R.AGG_FACTOR * rel_mod + R.AGG_FLOOR, f"{c.id}: rel_l2(dev, ref) = {rel_dev:.3e} > 2 * {rel_mod:.3e} + 1e-4"
    view = y[:c.N, b.y_cb0:cb1]
    for n in c.twins:
        assert np.array_equal(view[0], view[n]), f"{c.id}: images 0 and {n} (same input, same weight set) differ"
    if c.N == 3 and c.sets == [0, 1, 0]:
        assert not np.array_equal(view[0], view[1]), f"{c.id}: image 1 (another weight set) equals image 0"
    if c.big:
        clamped = int((ref.abs() == F16_MAX).sum())
        assert clamped > 0.5 * ref.numel() * (0.5 if c.relu else 1.0), f"{c.id}: only {clamped} outputs pass the fp16 range"
        assert bool((dev[ref.abs() == F16_MAX] == ref[ref.abs() == F16_MAX]).all()), f"{c.id}: an output past +-65504 is not clamped to it"
    return fig
