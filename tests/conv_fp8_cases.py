"""The fp8 side of tests/conv_cases.py: the 12 instantiations conv3_kernel<1,NBT,PXW,NC8,9,1,Q> behind k3_pick_q8 (Q = 1, the e4m3 MFMA)
and k3_pick_mx (Q = 2, the MX-scaled MFMA) of csrc/conv3_mfma.hip, through ltk_conv2d_fp8_ex.  Shared by tests/test_conv_host.py (CPU)
and tests/test_conv3_fp8_gpu.py; the gates (check), the geometry, the record line and the simulated device are conv_cases' own.

A case names the tile (force_pxw / force_nbt), the split factor, `quant` (1 / 2) and, through knob CONV3_NC8, the chunk depth of the e4m3
kernels; NC8 counts 16-byte planes = 16 fp8 channels, so a chunk is 32 (NC8 2) or 64 (NC8 4, MX) input channels.  conv_cases.geometry
serves the cases as they are: the LDS images are byte-identical to fp16 and a Case counts its chunks in 16-bit units (Cin / 2).

Exact operands - the only rounding left is the device's fp32 sum and the fp16 store:
  x    : e4m3 CODES (torch.float8_e4m3fn), [N + 1][cbt][H][W][32] bytes, holding x * act_scale (act_scale 8).  Ordinary cases draw
         |code| <= 1, with the e4m3 subnormals k 2^-9 (k = 1..7) and zeros planted; class `fp8-range` spreads the codes over all exponents
         up to +-448 instead.
  w    : w[co] = g_co q, q on the e4m3 grid with max |q| = 224 in every output channel, g_co = 2^-6, 2^-7, 2^-8 in rotation: the packer's
         224 / max |w| is 1 / g_co exactly, w s = q, and f32_to_e4m3 has nothing to round (test_conv_host checks e4m3(w s) == q bit for bit).
  ref  : float64 F.conv2d(x_codes / act_scale, w), then affine, residual, activation in float64.
  mod  : fp32 conv of the codes and q, times scale / (s_w act_scale), + shift (+ res), activation, rounded to fp16 once.
  tol  : conv_cases' bound with n = 9 Cin; the aggregate gate unchanged.

Buffers: guard blocks (a 32-channel one on either side of x, a 16-channel one on either side of res, two in front of y and one behind)
and the image past N; x's hold +-448 (0x7E / 0xFE, never the NaN code), several hundred times an ordinary code; res's and y's as in conv_cases."""
from __future__ import annotations

import functools
from typing import Dict, List, Optional

import numpy as np
import torch
import torch.nn.functional as F

import conv_cases as K
from oracle import op_replay as R

ACT_SCALE = 8.0
G_ROT = (2.0 ** -6, 2.0 ** -7, 2.0 ** -8)
FV = ((2, 4, 2, 1), (2, 2, 2, 1), (1, 4, 2, 1), (1, 2, 2, 1), (2, 2, 4, 1), (1, 2, 4, 1), (2, 1, 2, 1), (1, 1, 2, 1),     # (NBT, PXW, NC8, Q)
      (2, 2, 4, 2), (1, 2, 4, 2), (2, 1, 4, 2), (1, 1, 4, 2))


def vname(NBT, PXW, NC8, Q) -> str:
    return f"conv3_kernel<1,{NBT},{PXW},{NC8},9,1,{Q}>"


class Case(K.Case):
    """A 3x3 stride-1 pad-1 conv on e4m3 operands; Cin counts fp8 channels."""

    def __init__(self, cls, N, H, W, Cin, Cout, nbt, pxw, nc8, Q, rng=False, **kw):
        super().__init__(cls, N, H, W, Cin // 2, Cout, pxw=pxw, nbt=nbt, nc8=4 if (nc8 == 4 and Q == 1) else 0, expect=K.vname(1, nbt, pxw, nc8, 9), **kw)
        self.units, self.Cin, self.Q, self.rng = Cin // 2, Cin, Q, rng
        self.expect = vname(nbt, pxw, nc8, Q)
        self.n_prod, self.macs = 9 * Cin, 2 * self.macs

    @property
    def id(self) -> str:
        s = f"{self.N}x{self.H}x{self.W}-{self.Cin}to{self.Cout}-{('', 'e4m3', 'mx')[self.Q]}-pxw{self.pxw}nbt{self.nbt}nc{self.NC8}"
        s += (f"-ks{self.fks}" if self.fks != 1 else "") + ("-res" if self.res else "") + (f"-{K.ACT_NAMES[self.act]}" if self.act else "")
        return s + ("-view" if self.view else "") + ("-range" if self.rng else "")

    def opts(self, b: "Buffers") -> dict:
        o = dict(act=self.act, force_pxw=self.pxw, force_nbt=self.nbt, force_ksplit=self.fks)
        if self.view:
            o.update(x_ld=b.x_cbt * 32, x_coff=b.x_cb0 * 32, y_ld=b.y_cbt * 16, y_coff=b.y_cb0 * 16, res_ld=b.r_cbt * 16, res_coff=b.r_cb0 * 16)
        return o


geometry = K.geometry        # the tile depends on the map, the tile width, NC8 and Cout only; Case.nchunks counts chunks of 8 NC8 16-bit units


def _cin(nc8: int, chunks: int) -> int:
    return 16 * nc8 * chunks


def _cases() -> List[Case]:
    out: List[Case] = []
    # every instantiation at every map; Cout rotates through whole and partial cout blocks, Cin through 1, 3 and 7 chunks (the one
    # combination over 0.5 GMAC - 7 chunks to 64 / 96 channels on the 3 x 19 x 37 map - takes 3: the other maps have the 7)
    for vi, (nbt, pxw, nc8, Q) in enumerate(FV):
        for mi, (N, H, W) in enumerate(K.MAPS):
            Cout = ((32, 48, 80) if nbt == 1 else (64, 96))[(vi + mi) % (3 if nbt == 1 else 2)]
            chunks = (1, 3, 7)[(vi // 2 + mi) % 3]
            if 9 * N * H * W * Cout * _cin(nc8, chunks) > 0.5e9:
                chunks = 3
            out.append(Case("fp8-3x3", N, H, W, _cin(nc8, chunks), Cout, nbt, pxw, nc8, Q))
    # the persistent walk: 33 x 2 half-empty tiles x 8 cout tiles = 528 items > 512
    out.append(Case("fp8-3x3", 33, 4, 33, 32, 256, 1, 1, 2, 1))
    # split-K per chunk kind: 7 chunks into 2, 3 (uneven), 5 (-> 4: no empty split) and 7, with and without residual
    for res in (False, True):
        for fks in (2, 3, 5, 7):
            kw = dict(res=res, fks=fks)
            out += [Case("fp8-splitk", 5, 6, 5, 224, 48, 1, 1, 2, 1, **kw), Case("fp8-splitk", 5, 6, 5, 448, 48, 1, 2, 4, 1, **kw),
                    Case("fp8-splitk", 5, 6, 5, 448, 48, 1, 1, 4, 2, **kw)]
    # channel views: one instantiation per (Q, PXW) (and the 64-channel e4m3 chunks), partial cout blocks included, one split per Q
    for N, H, W in ((5, 6, 5), (3, 19, 37)):
        kw = dict(view=True, res=True)
        out += [Case("fp8-views", N, H, W, 96, 96, 2, 4, 2, 1, **kw), Case("fp8-views", N, H, W, 96, 48, 1, 2, 2, 1, **kw),
                Case("fp8-views", N, H, W, 96, 48, 1, 1, 2, 1, **kw), Case("fp8-views", N, H, W, 192, 96, 2, 2, 4, 1, **kw),
                Case("fp8-views", N, H, W, 192, 96, 2, 2, 4, 2, **kw), Case("fp8-views", N, H, W, 192, 48, 1, 1, 4, 2, **kw),
                Case("fp8-views", N, H, W, 224, 48, 1, 1, 2, 1, fks=3, **kw), Case("fp8-views", N, H, W, 448, 48, 1, 1, 4, 2, fks=3, **kw)]
    # activations once per Q, and behind a three-way split with residual (the finish kernel applies the activation itself)
    for act in (1, 2, 3):
        out += [Case("fp8-act", 2, 9, 16, 96, 48, 1, 2, 2, 1, act=act), Case("fp8-act", 2, 9, 16, 192, 48, 1, 2, 4, 2, act=act)]
    for act in (1, 2, 3):
        kw = dict(res=True, fks=3, act=act)
        out += [Case("fp8-act", 5, 6, 5, 224, 48, 1, 1, 2, 1, **kw), Case("fp8-act", 5, 6, 5, 448, 48, 1, 1, 4, 2, **kw)]
    # the full e4m3 range
    for N, H, W in ((2, 9, 16), (5, 6, 5)):
        out += [Case("fp8-range", N, H, W, 96, 48, 1, 2, 2, 1, rng=True), Case("fp8-range", N, H, W, 64, 48, 1, 2, 4, 2, rng=True)]
    return out


CASES = _cases()
CLASSES = ("fp8-3x3", "fp8-splitk", "fp8-views", "fp8-act", "fp8-range")


def groups() -> Dict[str, List[int]]:
    """Case indices per test, as conv_cases.groups: a class, split by the expected kernel where it has many cases."""
    g: Dict[str, List[int]] = {}
    for i, c in enumerate(CASES):
        key = f"{c.cls}:{c.expect}" if c.cls == "fp8-3x3" else f"{c.cls}:{c.N}x{c.H}x{c.W}" if c.cls == "fp8-views" else \
            f"{c.cls}:res{int(c.res)}" if c.cls == "fp8-splitk" else f"{c.cls}:split" if c.cls == "fp8-act" and c.ksplit > 1 else c.cls
        g.setdefault(key, []).append(i)
    return g


# ---------------------------------------------------------------------------------------------------- inputs, buffers, reference
def e4m3(t: torch.Tensor) -> torch.Tensor:
    """Rounded to the e4m3 grid (saturating), as float32."""
    return t.clamp(-448, 448).to(torch.float8_e4m3fn).float()


def codes_to_bytes(t: torch.Tensor) -> np.ndarray:
    """[N, C, H, W] values on the e4m3 grid -> bytes [N, C / 32, H, W, 32]"""
    N, C, H, W = t.shape
    b = t.to(torch.float8_e4m3fn).view(torch.uint8)
    return b.reshape(N, C // 32, 32, H, W).permute(0, 1, 3, 4, 2).contiguous().numpy()


def bytes_to_codes(a: np.ndarray) -> torch.Tensor:
    """bytes [N, cb, H, W, 32] -> float32 [N, cb * 32, H, W]"""
    N, cb, H, W, _ = a.shape
    return torch.from_numpy(np.ascontiguousarray(a)).view(torch.float8_e4m3fn).float().permute(0, 1, 4, 2, 3).reshape(N, cb * 32, H, W)


class Buffers:
    def __init__(self, c: Case, codes, res, seed):
        rng = np.random.default_rng(seed)
        N = c.N
        g = 1 if c.view else 0
        cb = c.Cin // 32
        self.x_cbt, self.x_cb0 = cb + 2 * g, g
        self.x = rng.choice(np.array([0x7E, 0xFE], np.uint8), (N + 1, self.x_cbt, c.H, c.W, 32))
        self.x[:N, g:g + cb] = codes_to_bytes(codes)
        self.r_cbt, self.r_cb0, self.res = c.Cout // 16, 0, None
        if res is not None:
            rb = c.Cout // 16
            mag = K.GUARD_GAIN * float(res.abs().max())
            shape = (N + 1, rb + 2 * g, c.H, c.W, 16)
            self.res = (rng.choice([-1.0, 1.0], shape) * rng.uniform(0.5, 1.0, shape) * mag).astype(np.float16)
            self.res[:N, g:g + rb] = K._cb(res)
            self.r_cbt, self.r_cb0 = rb + 2 * g, g
        self.y_cb0 = 2 * g
        self.y_cbt = c.Cout // 16 + 3 * g
        self.y_shape = (N + 1, self.y_cbt, c.H, c.W, 16)

    def empty_y(self) -> np.ndarray:
        return np.full(self.y_shape, K.PATTERN, np.int16)


class Reference:
    """Inputs, buffers, float64 reference, rounding model and bound of one case: computed once, read by every comparison."""

    def __init__(self, ci: int):
        c = self.c = CASES[ci]
        g = torch.Generator().manual_seed(9000 + ci)
        rn = lambda *s: torch.randn(*s, generator=g)
        ru = lambda *s: torch.rand(*s, generator=g)
        shape = (c.N, c.Cin, c.H, c.W)
        if c.rng:       # every exponent from the subnormals to 448, +-448 itself planted
            x = e4m3(torch.sign(rn(*shape)) * torch.exp2(ru(*shape) * 18.0 - 9.2))
            x = torch.where(ru(*shape) < 0.01, torch.sign(rn(*shape)) * 448.0, x)
        else:           # |code| <= 1; the subnormals k 2^-9 and zeros planted
            x = e4m3((rn(*shape) * 0.5).clamp(-1, 1))
            sub = torch.sign(rn(*shape)) * torch.randint(0, 8, shape, generator=g).float() * 2.0 ** -9
            x = torch.where(ru(*shape) < 0.05, sub, x)
        self.codes = x
        # q on the e4m3 grid, max |q| = 224 in every output channel; w = g_co q
        q = e4m3((rn(c.Cout, c.Cin, 3, 3) * 70.0).clamp(-224, 224))
        flat = q.view(c.Cout, -1)
        at = torch.randint(0, flat.shape[1], (c.Cout,), generator=g)
        flat[torch.arange(c.Cout), at] = torch.where(ru(c.Cout) < 0.5, -224.0, 224.0)
        self.q = q
        self.g = torch.tensor([G_ROT[co % 3] for co in range(c.Cout)])
        self.w = q * self.g.view(-1, 1, 1, 1)
        self.act_scale = ACT_SCALE
        self.scale = ru(c.Cout) + 0.5
        self.shift = rn(c.Cout) * 0.1
        self.r = R.f16(rn(c.N, c.Cout, c.H, c.W)) if c.res else None
        self.buf = Buffers(c, x, self.r, 11000 + ci)
        with torch.no_grad():
            d = lambda t: t.double()
            sc, sf = self.scale.view(1, -1, 1, 1), self.shift.view(1, -1, 1, 1)
            xr = d(x) / self.act_scale
            pre = F.conv2d(xr, d(self.w), padding=1) * d(sc) + d(sf)
            A = F.conv2d(xr.abs(), d(self.w).abs(), padding=1) * d(sc).abs() + d(sf).abs()
            pm = F.conv2d(x, q, padding=1) * self.fold().view(1, -1, 1, 1) + sf
            if c.res:
                pre, A, pm = pre + d(self.r), A + d(self.r).abs(), pm + self.r
            self.ref = K.activate(c, pre)
            self.mod = K.activate(c, pm).half().float()
            slope = (1.0, 1.0, R.GELU_SLOPE, K.SILU_SLOPE)[c.act]
            self.tol = 2.0 ** -10 * self.ref.abs() + slope * c.n_prod * 2.0 ** -23 * A + R.F16_FLOOR

    def fold(self, g: Optional[torch.Tensor] = None) -> torch.Tensor:
        """The epilogue scale as conv_fold folds it, fp32: scale / (s_w act_scale), s_w = 224 / max |w| = 1 / g_co"""
        return self.scale / ((1.0 / (self.g if g is None else g)) * self.act_scale)

    # ---- what conv_cases.sim_device reads
    sim_chunk = property(lambda self: 16 * self.c.NC8)

    def sim_x(self, cb0: int, fault: Optional[str]) -> torch.Tensor:
        c = self.c
        x = bytes_to_codes(self.buf.x[:c.N, cb0:cb0 + c.Cin // 32])
        if fault == "mxhalf":
            x = x.reshape(c.N, c.Cin // 32, 2, 16, c.H, c.W)[:, :, [0, 0]].reshape(c.N, c.Cin, c.H, c.W)
        return x

    def sim_w(self, fault: Optional[str]) -> torch.Tensor:
        if fault == "bytepair":
            c = self.c
            return self.q.reshape(c.Cout, c.Cin // 2, 2, 3, 3)[:, :, [1, 0]].reshape(c.Cout, c.Cin, 3, 3)
        return self.q

    def sim_scale(self, fault: Optional[str]) -> torch.Tensor:
        if fault == "wscale":
            co = torch.arange(self.c.Cout)
            return self.fold(self.g[(co ^ 1).clamp(max=self.c.Cout - 1)])
        return self.fold()


@functools.lru_cache(maxsize=8)
def reference(ci: int) -> Reference:
    return Reference(ci)


FAULTS = {f: why for f, why in K.FAULTS.items() if f != "ups"}
FAULTS.update({
    "wscale": "the neighbouring output channel's weight scale folded into the epilogue",
    "bytepair": "the two channels of a 16-bit weight unit swapped while x keeps its order",
    "mxhalf": "MX: channels 16..31 of every 32-channel block read from 0..15 (the `^ 16` partner going wrong)",
})


def applies(fault: str, c: Case) -> bool:
    if fault == "mxhalf":
        return c.Q == 2
    if fault in ("wscale", "bytepair"):
        return True
    return K.applies(fault, c)


def sim_device(rf: Reference, fault: Optional[str] = None) -> np.ndarray:
    """conv_cases.sim_device on the e4m3 operands (Reference.sim_x / sim_w / sim_scale): the codes read from the byte buffer through the
    view, chunks of 32 or 64 channels, the per-channel scale fold."""
    return K.sim_device(rf, fault)
