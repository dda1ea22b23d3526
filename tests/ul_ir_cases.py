"""What tests/test_ul_ir_host.py (CPU) and tests/test_ul_ir_gpu.py share: the cases of the fused inverted residual of the Ultralight
program (csrc/ul_ir.hip: 1x1 expand, depthwise 3x3 and 1x1 project in one launch, the hidden tensors in LDS), their inputs, the
channel-blocked buffers with guard blocks, the three-stage float64 reference, its bounds, a float32 rounding model, and a simulated
device that walks the planner's tiles and chunks and can be told to get it wrong.  The form of tests/ul_gconv_cases.py.

Cases: the smallest shapes that reach every edge of the kernel, derived from the planner's tile (TH x TW output pixels) and chunk (MC
hidden channels): N = 3 images (0 and 2 carry the same input and have to come out byte-identical, image 1 has to differ); a map one
pixel larger than a tile in each axis of the OUTPUT (a ragged last tile both ways, more than one block, halo pixels that a neighbour
owns), a map smaller than one tile, 5 x 7 and 1 x 1, each at stride 1 and 2 (odd sizes: the clipped 2 x 2 ownership of e1);
Cin in {16, 32, 48} x Cout in {16, 32, 48} with mid = 2 Cin (32, 64, 96: 32 and 96 are no multiple of MC = 64), one case with
mid = 2 MC + 16; residual on / off; channel views on x, y and the residual; N = 1; one case whose outputs pass +-65504 and one whose
hidden values do (a large scale1: e1 has to be clamped, not inf).

Inputs: x, w1, w2 and the residual are drawn in fp32 and rounded to fp16, the depthwise weights stay fp32 (the kernel keeps them so);
scale = U(0.5, 1.5); the expand's shift = 0.1 + 0.1 |N(0, 1)| (strictly positive: a halo pixel outside the map that was not zeroed
shows on every case); the other shifts 0.1 N(0, 1).

Check, stage by stage on the tensors the device left (the tap instantiation stores e1 and e2), with the project's own bounds
(oracle/op_replay.py docstring):
  e1 against the float64 expand of x                      dense conv bound, n = Cin;
  e2 against the float64 depthwise conv of the DEVICE's e1    depthwise bound (c = 2^-20);
  y  against the float64 project (+ residual) of the DEVICE's e2   dense conv bound, n = mid;
per stage no violator, no non-finite value, rel_l2(dev, ref) <= 2 rel_l2(model, ref) + 1e-4 (the model: the same stage in float32 on
the same inputs, rounded to fp16 once), nothing outside a view written.  Images 0 and 2 byte-identical in y, e1 and e2; image 1 differs.

Buffers (halfs, [N + 1][cbt][H][W][16]; the image past N belongs to nobody): x and res hold GUARD_GAIN x the data's magnitude outside
the view; y, e1 and e2 are pre-filled with PATTERN.  Views: x_coff 16 in x_ld Cin + 32, y_coff 32 in y_ld Cout + 48, res_coff 16 in
res_ld Cout + 32."""
from __future__ import annotations

from typing import List

import numpy as np
import torch
import torch.nn.functional as F

from oracle import op_replay as R

GUARD_GAIN = 1.0e3
PATTERN = 0x5A5A            # fp16 203.25
F16_MAX = 65504.0
STAGES = ("e1", "e2", "y")
N_CASES = 28            # len(cases()): the tests parametrise over indices, so that collecting them does not need the library


def planner():
    """Tile and chunk of the kernel, from the library's planner (no GPU)."""
    from livetalking_amd.engine import Engine
    p = Engine.ul_ir_plan(1, 8, 8, 16, 32, 16)
    assert p["accepted"], p
    return p["tile"][0], p["tile"][1], p["MC"]


class Case:
    def __init__(self, N, H, W, Cin, Cout, stride=1, mid=None, res=False, view=False, big="", note=""):
        self.N, self.H, self.W, self.Cin, self.Cout, self.stride = N, H, W, Cin, Cout, stride
        self.mid = mid if mid is not None else 2 * Cin
        self.res, self.view, self.big, self.note = res, view, big, note
        self.Ho, self.Wo = (H - 1) // stride + 1, (W - 1) // stride + 1
        self.twins = [2] if N == 3 else []

    @property
    def id(self) -> str:
        s = f"{self.N}x{self.H}x{self.W}-{self.Cin}to{self.mid}to{self.Cout}-s{self.stride}"
        return s + ("-res" if self.res else "") + ("-view" if self.view else "") + ("-big" + self.big if self.big else "")

    def geometry(self, TH, TW, MC, tap) -> dict:
        """What the planner has to report for this case."""
        S = self.stride
        gx, gy = -(-self.Wo // TW), -(-self.Ho // TH)
        return dict(accepted=True, reason="", kernel=f"ul_ir_kernel<{self.Cout // 16},{'true' if tap else 'false'}>", Ho=self.Ho, Wo=self.Wo,
                    tile=(TH, TW), MC=MC, chunks=-(-self.mid // MC), hidden_px=(S * (TH - 1) + 3) * (S * (TW - 1) + 3), grid=(gx, gy, self.N),
                    blocks=gx * gy * self.N, threads=256)


def cases(TH: int, TW: int, MC: int) -> List[Case]:
    out = []
    big_map = lambda s: (s * TH + 1, s * TW + 1)            # output map (TH + 1) x (TW + 1): a ragged last tile both ways
    for ci, cin in enumerate((16, 32, 48)):                 # every Cin x Cout on the ragged map, stride / residual / views rotating
        for co, cout in enumerate((16, 32, 48)):
            i = ci * 3 + co
            s = 1 + i % 2
            out.append(Case(3, *big_map(s), cin, cout, stride=s, res=(s == 1 and cin == cout), view=i % 4 == 1))
    for s in (1, 2):
        out.append(Case(3, *big_map(s), 32, 32, stride=s, view=True))
        out.append(Case(3, max(1, s * TH - 2), max(1, s * TW - 3), 32, 16, stride=s, view=s == 2))        # smaller than one tile
        out.append(Case(3, 5, 7, 16, 48, stride=s, view=s == 1))
        out.append(Case(3, 1, 1, 32, 32, stride=s, res=s == 1))
        out.append(Case(3, 5, 7, 48, 48, stride=s, res=s == 1, view=True))
    out += [Case(3, *big_map(1), 32, 32, res=True, view=True),                              # residual + every view
            Case(3, *big_map(1), 32, 16, mid=2 * MC + 16, note="mid = 2 MC + 16"),
            Case(3, *big_map(2), 16, 32, stride=2, mid=2 * MC + 16, view=True),
            Case(1, *big_map(1), 48, 48, res=True), Case(1, 5, 7, 16, 16, stride=2, view=True),
            Case(3, *big_map(1), 32, 16, big="out"), Case(3, *big_map(1), 32, 32, res=True, big="out"),       # outputs pass +-65504
            Case(3, *big_map(1), 32, 16, big="hid"), Case(3, *big_map(2), 16, 16, stride=2, big="hid")]       # hidden values do
    return out


def _h(t: torch.Tensor) -> torch.Tensor:
    return t.half().float()


class Inputs:
    """x (N, Cin, H, W), w1 (mid, Cin), w2 (Cout, mid), res (N, Cout, Ho, Wo) or None: fp16 values in float32; wd (mid, 3, 3) float32;
    s1, b1, sd, bd (mid) and s2, b2 (Cout) float32."""

    def __init__(self, c: Case):
        g = torch.Generator().manual_seed(1000 * c.Cin + 10 * c.Cout + 7 * c.H + c.stride + 100 * c.N + c.mid + (5 if c.big else 0))
        self.x = _h(torch.randn(c.N, c.Cin, c.H, c.W, generator=g))
        for n in c.twins:
            self.x[n] = self.x[0]
        self.w1 = _h(torch.randn(c.mid, c.Cin, generator=g) / np.sqrt(c.Cin))
        self.wd = torch.randn(c.mid, 3, 3, generator=g) / 3.0
        self.w2 = _h(torch.randn(c.Cout, c.mid, generator=g) / np.sqrt(c.mid))
        self.s1 = torch.rand(c.mid, generator=g) + 0.5
        self.b1 = 0.1 + 0.1 * torch.randn(c.mid, generator=g).abs()
        self.sd = torch.rand(c.mid, generator=g) + 0.5
        self.bd = 0.1 * torch.randn(c.mid, generator=g)
        self.s2 = torch.rand(c.Cout, generator=g) + 0.5
        self.b2 = 0.1 * torch.randn(c.Cout, generator=g)
        if c.big == "out":
            self.s2 = self.s2 * 2.0e5                # |acc2| ~ 0.5: most outputs pass the fp16 range
        if c.big == "hid":
            self.s1 = self.s1 * 2.0e5                # the positive pre-activations pass it
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
    with np.errstate(over="ignore"):
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
        self.e1 = np.full((c.N + 1, c.mid // 16, c.H, c.W, 16), PATTERN, np.uint16)
        self.e2 = np.full((c.N + 1, c.mid // 16, c.Ho, c.Wo, 16), PATTERN, np.uint16)

    def views(self) -> dict:
        return dict(x_ld=self.x_cbt * 16, x_coff=self.x_cb0 * 16, y_ld=self.y_cbt * 16, y_coff=self.y_cb0 * 16, res_ld=self.r_cbt * 16,
                    res_coff=self.r_cb0 * 16)


# ---------------------------------------------------------------------------------------------------- the three stages
def _v(t):
    return t[None, :, None, None]


def _expand(x, inp, dt):
    """-> (pre-clamp value, A, s) of stage 1 in dtype dt."""
    w = inp.w1.to(dt)[:, :, None, None]
    acc = F.conv2d(x.to(dt), w) * _v(inp.s1.to(dt)) + _v(inp.b1.to(dt))
    return F.relu(acc)


def _depthwise(e1, inp, c, dt, pad_value=None, replicate=False, shift_window=False):
    w = inp.wd.to(dt)[:, None]
    e = e1.to(dt)
    if shift_window:
        e = F.pad(e, (0, 1, 0, 1))[:, :, 1:, 1:]
    if pad_value is not None:
        p = _v(pad_value.to(dt)).expand(e.shape[0], -1, e.shape[2] + 2, e.shape[3] + 2).clone()
        p[:, :, 1:-1, 1:-1] = e
        acc = F.conv2d(p, w, None, stride=c.stride, groups=c.mid)
    elif replicate:
        acc = F.conv2d(F.pad(e, (1, 1, 1, 1), mode="replicate"), w, None, stride=c.stride, groups=c.mid)
    else:
        acc = F.conv2d(e, w, None, stride=c.stride, padding=1, groups=c.mid)
    return F.relu(acc * _v(inp.sd.to(dt)) + _v(inp.bd.to(dt)))


def _project(e2, res, inp, dt):
    w = inp.w2.to(dt)[:, :, None, None]
    t = F.conv2d(e2.to(dt), w) * _v(inp.s2.to(dt)) + _v(inp.b2.to(dt))
    return t + res.to(dt) if res is not None else t


def stage_refs(c: Case, inp: Inputs, e1_dev: torch.Tensor, e2_dev: torch.Tensor) -> dict:
    """stage -> (ref, tol, model): float64 reference of each stage ON THE DEVICE'S INPUT of that stage (x; the device's e1; the device's
    e2), clamped to the fp16 range, its bound, and the float32 model of the same stage on the same input, rounded once."""
    d = torch.float64
    clamp = lambda t: t.clamp(-F16_MAX, F16_MAX)
    out = {}
    x = inp.x.double()
    ref = clamp(_expand(x, inp, d))
    A = R.short_sum(c.Cin) * F.conv2d(x.abs(), inp.w1.double().abs()[:, :, None, None]) * _v(inp.s1.double().abs()) + 4 * _v(inp.b1.double().abs())
    sl = 2.0 ** -24 * x.abs().sum(1, keepdim=True) * _v(inp.s1.double().abs()) + 2.0 ** -24
    out["e1"] = (ref, 2.0 ** -10 * ref.abs() + R.C_LIN * A + sl, _h(clamp(_expand(inp.x, inp, torch.float32))))
    e1 = e1_dev.double()
    ref = clamp(_depthwise(e1, inp, c, d))
    A = F.conv2d(e1.abs(), inp.wd.double().abs()[:, None], None, stride=c.stride, padding=1, groups=c.mid) * _v(inp.sd.double().abs()) + _v(inp.bd.double().abs())
    out["e2"] = (ref, 2.0 ** -10 * ref.abs() + R.C_F32 * A + R.F16_FLOOR, _h(clamp(_depthwise(e1_dev, inp, c, torch.float32))))
    e2 = e2_dev.double()
    res = inp.res.double() if c.res else None
    ref = clamp(_project(e2, res, inp, d))
    A = R.short_sum(c.mid) * F.conv2d(e2.abs(), inp.w2.double().abs()[:, :, None, None]) * _v(inp.s2.double().abs()) + 4 * _v(inp.b2.double().abs())
    if c.res:
        A = A + 4 * res.abs()
    sl = 2.0 ** -24 * e2.abs().sum(1, keepdim=True) * _v(inp.s2.double().abs()) + 2.0 ** -24
    out["y"] = (ref, 2.0 ** -10 * ref.abs() + R.C_LIN * A + sl, _h(clamp(_project(e2_dev, inp.res, inp, torch.float32))))
    return out


# ---------------------------------------------------------------------------------------------------- the simulated device
class SimDevice:
    """ul_ir_kernel in float32: per tile of TH x TW output pixels of one image and per chunk of MC hidden channels the expand over the
    tile and its halo (zero outside the map, clamped, rounded to fp16), the depthwise conv of that hidden tile (rounded), the project into
    the tile's accumulators; then acc2 * scale2 + shift2 + res, clamped and rounded once; stores skip the pixels past the map; the taps
    are stored by the owner.  `fault`: one of FAULTS."""

    def __init__(self, c: Case, inp: Inputs, TH: int, TW: int, MC: int, fault: str = ""):
        assert not fault or fault in FAULTS
        self.c, self.inp, self.TH, self.TW, self.MC, self.fault = c, inp, TH, TW, MC, fault

    def run(self, b: Buffers, tap: bool = True):
        """-> (y, e1, e2) buffers as the device would leave them (e1, e2 untouched without `tap`)."""
        c, inp, f, TH, TW, MC, S = self.c, self.inp, self.fault, self.TH, self.TW, self.MC, self.c.stride
        y, e1b, e2b = b.y.copy(), b.e1.copy(), b.e2.copy()
        xbuf = _from_cb(b.x, c.N + 1, b.x_cbt * 16, 0)                       # the whole buffer, guard blocks included
        x0 = 0 if f == "x_view_ignored" else b.x_cb0 * 16
        x = xbuf[:c.N, x0:x0 + c.Cin]
        rbuf = _from_cb(b.res, c.N + 1, b.r_cbt * 16, 0)[:c.N, b.r_cb0 * 16:b.r_cb0 * 16 + c.Cout] if c.res else None
        if c.res and f == "res_prev_image":
            rbuf = torch.roll(rbuf, 1, 0)
        mid_run = c.mid // MC * MC if f == "drop_mc_tail" else c.mid           # hidden channels the chunk loop reaches
        hid_h, hid_w = S * (TH - 1) + 3, S * (TW - 1) + 3
        yv = torch.zeros(c.N, c.Cout, c.Ho, c.Wo)
        e1v = torch.full((c.N, c.mid, c.H, c.W), float("nan"))
        e2v = torch.full((c.N, c.mid, c.Ho, c.Wo), float("nan"))
        ywritten = torch.zeros(c.Ho, c.Wo, dtype=torch.bool)
        for ty in range(-(-c.Ho // TH)):
            for tx in range(-(-c.Wo // TW)):
                oy0, ox0 = ty * TH, tx * TW
                hy0, hx0 = oy0 * S - 1, ox0 * S - 1
                # the hidden tile: map pixels [iy0, iy1) x [ix0, ix1) of it are inside the map
                iy0, iy1, ix0, ix1 = max(hy0, 0), min(hy0 + hid_h, c.H), max(hx0, 0), min(hx0 + hid_w, c.W)
                pre = _expand(x[:, :, iy0:iy1, ix0:ix1], inp, torch.float32)
                if f != "e1_unclamped":
                    pre = pre.clamp(max=F16_MAX)
                tile = pre if f == "e1_unrounded" else _h(pre)
                rounded = _h(pre)
                # owner region: input pixels [S oy0, S (oy0 + TH)) x [S ox0, S (ox0 + TW)), clipped
                wy0, wy1, wx0, wx1 = S * oy0, min(S * (oy0 + TH), c.H), S * ox0, min(S * (ox0 + TW), c.W)
                e1v[:, :, wy0:wy1, wx0:wx1] = rounded[:, :, wy0 - iy0:wy1 - iy0, wx0 - ix0:wx1 - ix0]
                if f == "halo_one_ulp":                                           # what this block recomputes for a neighbour's pixels: one ulp up
                    own = torch.zeros(tile.shape[2], tile.shape[3], dtype=torch.bool)
                    own[wy0 - iy0:wy1 - iy0, wx0 - ix0:wx1 - ix0] = True
                    bits = tile.half().view(torch.int16) + 1
                    tile = torch.where(own[None, None] | (tile == 0) | (tile >= F16_MAX), tile, bits.view(torch.float16).float())
                # the padded hidden tile, hid_h x hid_w
                if f == "halo_relu_shift":
                    pad_val = _h(F.relu(inp.b1))
                    full = _v(pad_val).expand(c.N, -1, hid_h, hid_w).clone()
                elif f == "halo_replicate":
                    full = None
                else:
                    full = torch.zeros(c.N, c.mid, hid_h, hid_w)
                if full is None:
                    full = F.pad(tile, (ix0 - hx0, hx0 + hid_w - ix1, iy0 - hy0, hy0 + hid_h - iy1), mode="replicate")
                else:
                    full[:, :, iy0 - hy0:iy1 - hy0, ix0 - hx0:ix1 - hx0] = tile
                if f == "stride_odd" and S == 2:
                    full = F.pad(full, (0, 1, 0, 1))[:, :, 1:, 1:]
                acc = F.conv2d(full, inp.wd[:, None], None, stride=S, groups=c.mid)            # TH x TW outputs
                e2t = _h(F.relu(acc * _v(inp.sd) + _v(inp.bd)).clamp(max=F16_MAX))
                e2t[:, mid_run:] = 0
                oy1, ox1 = min(oy0 + TH, c.Ho), min(ox0 + TW, c.Wo)
                e2v[:, :, oy0:oy1, ox0:ox1] = e2t[:, :, :oy1 - oy0, :ox1 - ox0]
                acc2 = torch.zeros(c.N, c.Cout, TH, TW)
                for m0 in range(0, mid_run, MC):                                 # chunks ascend, one accumulator
                    acc2 = acc2 + F.conv2d(e2t[:, m0:m0 + MC], inp.w2[:, m0:m0 + MC, None, None])
                acc2 = acc2[:, :, :oy1 - oy0, :ox1 - ox0]
                r = rbuf[:, :, oy0:oy1, ox0:ox1] if c.res else None
                if f == "res_before_affine" and c.res:
                    t = (acc2 + r) * _v(inp.s2) + _v(inp.b2)
                else:
                    t = acc2 * _v(inp.s2) + _v(inp.b2)
                    if c.res:
                        t = t + r
                if f == "relu_on_project":
                    t = F.relu(t)
                ragged = oy1 - oy0 < TH or ox1 - ox0 < TW
                if not (f == "ragged_unwritten" and ragged):
                    yv[:, :, oy0:oy1, ox0:ox1] = _h(t.clamp(-F16_MAX, F16_MAX))
                    ywritten[oy0:oy1, ox0:ox1] = True
        if f == "drop_mc_tail":
            e1v[:, mid_run:] = float("nan")
            e2v[:, mid_run:] = float("nan")
        cb1 = b.y_cb0 + c.Cout // 16
        full = _to_cb(yv, b.y_cbt, b.y_cb0, fill_bits=PATTERN)
        mask = ywritten.numpy()[None, None, :, :, None]
        y[:c.N, b.y_cb0:cb1] = np.where(mask, full[:c.N, b.y_cb0:cb1], y[:c.N, b.y_cb0:cb1])
        if f == "past_map_written" and c.Wo % TW:
            # the last row's pixels behind the map's right edge land behind the plane of their (image, channel block)
            flat = y.reshape(-1, 16)
            plane = c.Ho * c.Wo
            for n in range(c.N):
                for cb in range(b.y_cb0, cb1):
                    at = (n * b.y_cbt + cb + 1) * plane
                    flat[at:at + TW - c.Wo % TW] = np.float16(1000.0).view(np.uint16)
        if tap:
            for src, dst in ((e1v, e1b), (e2v, e2b)):
                keep = ~torch.isnan(src)
                img = _to_cb(torch.where(keep, src, torch.zeros_like(src)), c.mid // 16, 0, fill_bits=PATTERN)
                km = keep.numpy().reshape(c.N, c.mid // 16, 16, src.shape[2], src.shape[3]).transpose(0, 1, 3, 4, 2)
                dst[:c.N] = np.where(km, img[:c.N], dst[:c.N])
        return y, e1b, e2b


def _multi_tile(c, TH, TW):
    return c.Ho > TH or c.Wo > TW


# fault -> (TH, TW, MC, case) -> does it show on that case
FAULTS = {
    "halo_relu_shift": lambda t, c: True,                       # hidden pixels outside the map left at relu(shift1) (> 0 on every channel)
    "halo_replicate": lambda t, c: True,                        # ... replicated from the edge
    "stride_odd": lambda t, c: c.stride == 2,                   # the stride-2 window starts one pixel off
    "drop_mc_tail": lambda t, c: c.mid % t[2] != 0,             # the chunk behind the last full one is dropped
    # the depthwise conv reads e1 before its rounding: up to 2^-11 of each tap against a bound of 2^-20 A + 2^-10 |ref| - it shows where
    # taps cancel, which needs a few hundred outputs of more than one tap; a clamped e1 (65504) has no rounding to lose
    "e1_unrounded": lambda t, c: c.H * c.W >= 35 and c.big != "hid",
    "e1_unclamped": lambda t, c: c.big == "hid",                # inf in e1
    "res_before_affine": lambda t, c: c.res,
    "relu_on_project": lambda t, c: True,
    "res_prev_image": lambda t, c: c.res and c.N > 1,
    "x_view_ignored": lambda t, c: c.view,
    "ragged_unwritten": lambda t, c: c.Ho % t[0] != 0 or c.Wo % t[1] != 0,
    "past_map_written": lambda t, c: c.Wo % t[1] != 0,
    # a halo pixel one ulp off its owner's value: the taps hold the owner's, the neighbour's depthwise conv saw another (as above: where
    # taps cancel); needs a neighbour
    "halo_one_ulp": lambda t, c: _multi_tile(c, t[0], t[1]) and c.big != "hid",
}


def check(c: Case, inp: Inputs, b: Buffers, y: np.ndarray, e1: np.ndarray, e2: np.ndarray) -> dict:
    """Every gate on the buffers a device (or the simulation) left behind.  -> the figures per stage; raises AssertionError."""
    cb1 = b.y_cb0 + c.Cout // 16
    outside = np.ones(y.shape, bool)
    outside[:c.N, b.y_cb0:cb1] = False
    touched = int((y[outside] != PATTERN).sum())
    assert touched == 0, f"{c.id}: {touched} halfs outside the output view were written"
    for name, t in (("e1", e1), ("e2", e2)):
        touched = int((t[c.N:] != PATTERN).sum())
        assert touched == 0, f"{c.id}: {touched} halfs behind the last image of {name} were written"
    dev = {"e1": _from_cb(e1, c.N, c.mid, 0), "e2": _from_cb(e2, c.N, c.mid, 0), "y": _from_cb(y, c.N, c.Cout, b.y_cb0)}
    views = {"e1": e1[:c.N], "e2": e2[:c.N], "y": y[:c.N, b.y_cb0:cb1]}
    finite_in = lambda t: torch.where(torch.isfinite(t), t, torch.zeros_like(t))
    refs = stage_refs(c, inp, finite_in(dev["e1"]), finite_in(dev["e2"]))
    figs = {}
    for st in STAGES:
        ref, tol, mod = refs[st]
        d = dev[st].double()
        finite = torch.isfinite(d)
        err = (d - ref).abs()
        over = torch.where(finite, err / tol, torch.full_like(err, float("inf")))
        viol = int((over > 1).sum())
        rel_dev = R.rel_l2(torch.where(finite, d, torch.zeros_like(d)), ref)
        rel_mod = R.rel_l2(mod, ref)
        fig = dict(violators=viol, worst=float(over.max()), rel_dev=rel_dev, rel_mod=rel_mod, nonfinite=int((~finite).sum()),
                   model_worst=float(((mod.double() - ref).abs() / tol).max()))
        figs[st] = fig
        assert fig["nonfinite"] == 0, f"{c.id} {st}: {fig['nonfinite']} non-finite values"
        assert viol == 0, f"{c.id} {st}: {viol} of {d.numel()} elements outside the bound, worst |dev - ref| / tol = {fig['worst']:.2f}"
        assert rel_dev <= R.AGG_FACTOR * rel_mod + R.AGG_FLOOR, f"{c.id} {st}: rel_l2(dev, ref) = {rel_dev:.3e} > 2 * {rel_mod:.3e} + 1e-4"
        for n in c.twins:
            assert np.array_equal(views[st][0], views[st][n]), f"{c.id} {st}: images 0 and {n} (same input) differ"
        if c.N == 3:
            assert not np.array_equal(views[st][0], views[st][1]), f"{c.id} {st}: image 1 (another input) equals image 0"
    if c.big:
        st = "y" if c.big == "out" else "e1"
        ref, d = refs[st][0], dev[st].double()
        at = ref.abs() == F16_MAX
        assert int(at.sum()) > 0.25 * ref.numel(), f"{c.id}: only {int(at.sum())} values of {st} pass the fp16 range"
        assert bool((d[at] == ref[at]).all()), f"{c.id}: a value of {st} past +-65504 is not clamped to it"
    return figs
