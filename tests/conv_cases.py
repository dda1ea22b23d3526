"""What tests/test_conv_host.py (CPU) and tests/test_conv3_gpu.py share: the cases at which the conv3 family of csrc/conv3_mfma.hip and the
row kernels of csrc/rowgemm.hip change path, their inputs, the channel-blocked buffers the kernels read and write, the float64 reference,
the gates, and a simulated device that computes the op as the kernels do and can be told to get it wrong.

A case names what it wants launched - conv3: the tile (force_pxw / force_nbt, the tile table's path), the split factor and, through knob
CONV3_NC8, the chunk depth - and the instantiation it expects, in the spelling of ltk_debug_conv3_variants; the hook's report has to
say the same.  A case that does not test the split passes force_ksplit = 1, so that the split rule cannot choose for it.

Inputs: x, w (and the residual) are drawn in fp32 and rounded to fp16, so the device holds them exactly; scale = U(0.5, 1.5), shift =
0.1 N(0, 1) as tests/test_conv_gpu.py has them.  The four-phase upsample-conv pre-sums up to four 3x3 taps per phase weight and rounds
the sum to fp16: its cases draw w on the grid 2^-8 with |w| < 1, where those sums are exact too.

Reference: F.conv2d / conv_transpose2d / interpolate(nearest) in float64 on the CPU, then the affine, the residual and the activation
in float64.  Model (`mod`, the convention of oracle/op_replay.py): the same in float32, rounded to fp16 once.

Per element:  |dev - ref| <= 2^-10 |ref| + slope * n 2^-23 A + 2^-24,  A = |scale| (|W| (*) |x|) + |shift| + |res| in float64, n the
products per output as the device forms them (taps x Cin; 4 Cin for the transposed and the four-phase convs), no violator, NaN is one.
  2^-10 |ref| : the output's rounding to fp16 (2^-11) with op_replay's factor 2;
  n 2^-23 A   : an fp32 sum of n terms in ANY order (gamma_n ~ n 2^-24) with a factor 2 - it covers the MFMA's order and split-K;
  slope       : GELU 1.13 (op_replay.GELU_SLOPE), SiLU 1.1, else 1 - the pre-activation's bound carried through the activation;
  no weight-rounding term: the weights are exact.
Aggregate:  rel_l2(dev, ref) <= AGG_FACTOR rel_l2(mod, ref) + AGG_FLOOR (op_replay's 2 and 1e-4): small errors on few elements, which the
worst-case bound lets through where |ref| << A.

Buffers (halfs, [N + 1][cbt][H][W][16]; the image past N belongs to nobody):
  x, res : the tensor's channel blocks at [cb0, cb0 + C / 16); every other block and all of image N hold GUARD_GAIN x the data's magnitude,
           finite, so a read outside the view dominates the result.  Views: x_coff 16 in x_ld Cin + 32, res_coff 16 in res_ld Cout + 32.
  y      : pre-filled with PATTERN; y_coff 32 in y_ld Cout + 48 for a view.  Every half outside [0, N) x [cb0, cb0 + Cout / 16) has to
           hold PATTERN afterwards: the blocks around the view and the rows of the image a short last tile does not have."""
from __future__ import annotations

import functools
import math
from typing import Dict, List, Optional, Tuple

import numpy as np
import torch
import torch.nn.functional as F

from oracle import op_replay as R

GUARD_GAIN = 1.0e3
PATTERN = 0x5A5A            # fp16 203.25
SILU_SLOPE = 1.1            # max |silu'(x)| = 1.0998 (at x = 2.4)
ACT_NAMES = ("none", "relu", "gelu", "silu")
ROW_KERNELS = ("rowgemm_kernel<1>", "rowgemm_kernel<2>", "rowconv_kernel<2,6>", "rowconv_kernel<4,4>", "rowconv_kernel<2,6> x 4 phases")


def vname(G, NBT, PXW, NC8, T, S=1) -> str:
    return f"conv3_kernel<{G},{NBT},{PXW},{NC8},{T},{S}>"


class Case:
    """H x W is the map the conv sees (the UPSAMPLED size when ups != 0, the source size of a transposed conv)."""

    def __init__(self, cls, N, H, W, Cin, Cout, k=3, stride=1, pad=1, transposed=False, out_pad=0, res=False, act=0, ups=0, pxw=0,
                 nbt=0, fks=1, family=0, view=False, nc8=0, expect=""):
        self.cls, self.N, self.H, self.W, self.Cin, self.Cout, self.k = cls, N, H, W, Cin, Cout, k
        self.stride, self.pad, self.transposed, self.out_pad, self.res, self.act, self.ups = stride, pad, transposed, out_pad, res, act, ups
        self.pxw, self.nbt, self.fks, self.family, self.view, self.nc8, self.expect = pxw, nbt, fks, family, view, nc8, expect
        self.Hs, self.Ws = (H // 2, W // 2) if ups else (H, W)
        if transposed:
            self.Ho, self.Wo = 2 * H, 2 * W
        else:
            self.Ho = (H + 2 * pad + out_pad - k) // stride + 1
            self.Wo = (W + 2 * pad + out_pad - k) // stride + 1
        if family == 0:
            self.G, self.NBT, self.PXW, self.NC8, self.T, self.S = (int(v) for v in expect[expect.index("<") + 1:-1].split(","))
        else:                                   # the row kernels: 32-channel k-steps, 32-channel output blocks, no tiles over images
            self.G, self.NBT, self.PXW, self.NC8, self.T, self.S = 1, 1, 0, 4, k * k, stride
        self.nchunks = Cin // (8 * self.NC8)
        # conv3_launch: the forced factor, at most one split per chunk, then no empty split
        ks = max(1, min(fks, 32, self.nchunks)) if family == 0 else 1
        cps = -(-self.nchunks // ks)
        if cps * (ks - 1) >= self.nchunks:
            ks = -(-self.nchunks // cps)
        self.ksplit, self.cps = ks, cps
        # products per output as the device forms them
        self.n_prod = Cin * (4 if (transposed or ups == 2) else k * k)
        self.macs = N * self.Ho * self.Wo * Cout * Cin * (k * k / 4 if transposed else k * k)

    @property
    def id(self) -> str:
        kind = ("convT" if self.transposed else f"k{self.k}s{self.stride}p{self.pad}") + (f"op{self.out_pad}" if self.out_pad and not self.transposed else "")
        s = f"{self.N}x{self.H}x{self.W}-{self.Cin}to{self.Cout}-{kind}"
        if self.family:
            s += "-" + ("", "rowgemm", "rowconv", "rowconvT")[self.family]
        else:
            s += f"-pxw{self.pxw}nbt{self.nbt}nc{self.NC8}"
        s += (f"-ups{self.ups}" if self.ups else "") + (f"-ks{self.fks}" if self.fks != 1 else "") + ("-res" if self.res else "")
        return s + (f"-{ACT_NAMES[self.act]}" if self.act else "") + ("-view" if self.view else "")

    def opts(self, b: "Buffers") -> dict:
        o = dict(act=self.act, ups=self.ups, force_pxw=self.pxw, force_nbt=self.nbt, force_ksplit=self.fks if self.family == 0 else 0, family=self.family)
        if self.view:
            o.update(x_ld=b.x_cbt * 16, x_coff=b.x_cb0 * 16, y_ld=b.y_cbt * 16, y_coff=b.y_cb0 * 16, res_ld=b.r_cbt * 16, res_coff=b.r_cb0 * 16)
        return o


# ---------------------------------------------------------------------------------------------------- geometry (conv3_launch's)
def _clog2(v: int) -> int:
    l = 0
    while (1 << l) < v:
        l += 1
    return l


def _maxa(PXW, NC8, S, T) -> int:
    if T == 1:
        return (NC8 // 2) * PXW
    if S == 2:
        return 10 if NC8 == 2 else 20
    if PXW == 4:
        return 6 if NC8 == 2 else 12
    return {2: 4, 4: 8}.get(NC8, 16)


def geometry(c: Case) -> dict:
    """The tile of a conv3 launch as conv3_launch's geom() lays it out: l2w, l2h, NB (images per tile), the item count, and whether
    the patch fits the staging budget and LDS."""
    if c.family:
        return dict(NB=1, l2w=0, l2h=0, items=0, grid=0, fit=True)
    Hg, Wg = (c.Hs, c.Ws) if c.ups == 2 else (c.Ho, c.Wo) if c.S == 2 else (c.H, c.W)     # the grid the tiles cover
    ext = (2 if c.ups == 2 else 1) if c.G == 4 else 2 if (c.S == 2 or c.T == 9) else 0
    M = 128 * c.PXW
    l2w = min(5, _clog2(Wg))
    l2h = min(_clog2(M) - l2w, _clog2(Hg))
    NB = max(1, min(M >> (l2w + l2h), c.N))
    PH, PW = ((1 << l2h) - 1) * c.S + 1 + ext, ((1 << l2w) - 1) * c.S + 1 + ext
    if c.S == 2:
        PW = (PW + 1) & ~1
    if c.S == 1 and l2w == 3 and ext > 0:
        PW = 12
    budget = _maxa(c.PXW, c.NC8, c.S, c.T) * 256
    slots = lambda nb: (2 * nb * PH * PW + 63) // 64 * 64
    while NB > 1 and (c.NC8 // 2) * slots(NB) > budget:
        NB -= 1
    blocks = -(-Wg // (1 << l2w)) * -(-Hg // (1 << l2h)) * -(-c.N // NB)
    BN = 32 * c.NBT
    items = blocks * -(-c.Cout // BN) * c.ksplit
    lds = 2 * ((c.NC8 // 2) * slots(NB) * 16 + c.T * c.NC8 * BN * 16) + 256 + 2 * BN * 4
    fit = (c.NC8 // 2) * slots(NB) <= budget and NB * PH * PW < 32768 and lds <= 160 * 1024
    return dict(NB=NB, l2w=l2w, l2h=l2h, PW=PW, items=items, grid=min(items, 512), fit=fit)


# ---------------------------------------------------------------------------------------------------- the cases
MAPS = ((3, 19, 37), (5, 6, 5), (2, 9, 16), (1, 1, 1), (19, 1, 1))
#        two ragged 32-wide tile columns | l2w = 3: the 12-pixel pitch, several images per tile, a short last tile | l2w = 4: the row key | 1x1 maps


def _nc8_1x1(Cin, Cout) -> int:
    return 4 if (Cin % 32 == 0 and Cout >= 128 and Cout % 128 == 0) else 8 if Cin % 64 == 0 else 2


def _conv3x3(cls, N, H, W, Cin, Cout, nbt, pxw, nc8, **kw) -> Case:
    return Case(cls, N, H, W, Cin, Cout, pxw=pxw, nbt=nbt, nc8=4 if nc8 == 4 else 0, expect=vname(1, nbt, pxw, nc8, 9), **kw)


def _conv1x1(cls, N, H, W, Cin, Cout, nbt, **kw) -> Case:
    return Case(cls, N, H, W, Cin, Cout, k=1, pad=0, pxw=2, nbt=nbt, expect=vname(1, nbt, 2, _nc8_1x1(Cin, Cout), 1), **kw)


def _s2(cls, N, H, W, Cin, Cout, nbt, pad, **kw) -> Case:
    return Case(cls, N, H, W, Cin, Cout, stride=2, pad=pad, out_pad=1 - pad, pxw=2, nbt=nbt, expect=vname(1, nbt, 2, 2, 9, 2), **kw)


def _convT(cls, N, H, W, Cin, Cout, **kw) -> Case:
    return Case(cls, N, H, W, Cin, Cout, stride=2, transposed=True, out_pad=1, pxw=2, nbt=1, expect=vname(4, 1, 2, 4 if Cin % 32 == 0 else 2, 9), **kw)


def _ups4(cls, N, Hs, Ws, Cin, Cout, **kw) -> Case:
    return Case(cls, N, 2 * Hs, 2 * Ws, Cin, Cout, ups=2, pxw=2, nbt=1, expect=vname(4, 1, 2, 2, 16), **kw)


V3X3 = ((2, 4, 2), (2, 2, 2), (1, 4, 2), (1, 2, 2), (2, 2, 4), (1, 2, 4), (2, 1, 2), (1, 1, 2), (2, 1, 4), (1, 1, 4))     # (NBT, PXW, NC8)


def _cases() -> List[Case]:
    out: List[Case] = []
    # 3x3 stride 1: every (NBT, PXW, NC8) at every map; Cout rotates through whole and partial cout blocks, Cin through 1, 3 and 7
    # chunks (NC8 4: 1 and 3)
    for vi, (nbt, pxw, nc8) in enumerate(V3X3):
        for mi, (N, H, W) in enumerate(MAPS):
            Cout = ((32, 48, 80) if nbt == 1 else (64, 96))[(vi + mi) % (3 if nbt == 1 else 2)]
            Cin = ((16, 48, 112) if nc8 == 2 else (32, 96))[(vi // 2 + mi) % (3 if nc8 == 2 else 2)]
            out.append(_conv3x3("3x3", N, H, W, Cin, Cout, nbt, pxw, nc8))
    out.append(_conv3x3("3x3", 3, 64, 64, 16, 192, 1, 1, 2))                 # 576 items > 512: the persistent walk
    # 1x1: all seven (NBT, NC8); Cin 48 / 80 -> 16-channel chunks, 64 / 192 -> 64, 96 with Cout 128 / 256 -> 32 (and the 128-cout block)
    for vi, (nbt, cins, couts) in enumerate(((2, (48, 80), (64, 96)), (1, (48, 80), (32, 48, 80)), (2, (64, 192), (64, 96)), (1, (64, 192), (32, 48, 80)),
                                             (4, (96,), (128, 256)), (2, (96,), (128, 256)), (1, (96,), (128, 256)))):
        for mi, (N, H, W) in enumerate(MAPS):
            out.append(_conv1x1("1x1", N, H, W, cins[mi % len(cins)], couts[(vi + mi) % len(couts)], nbt))
    # stride 2: pad 1 and pad 0 + one zero row / column behind the map, odd and even H, W
    for N, H, W in ((3, 19, 37), (5, 6, 5), (2, 9, 16), (2, 8, 12)):
        for pad in (1, 0):
            out += [_s2("s2", N, H, W, 64, 48, 1, pad), _s2("s2", N, H, W, 64, 64, 2, pad)]
    # merged transposed conv (16- and 32-channel chunks), four-phase upsample-conv, the nearest-upsample read at every tile width
    for mi, (N, H, W) in enumerate(((3, 5, 7), (2, 19, 21))):
        out += [_convT("g4", N, H, W, 48, (32, 48)[mi]), _convT("g4", N, H, W, 64, (48, 32)[mi]), _ups4("g4", N, H, W, 32, (48, 32)[mi])]
        for pxw in (1, 2, 4):
            out.append(_conv3x3("g4", N, 2 * H, 2 * W, (48, 16)[mi], 32 if pxw == 4 else 48, 1, pxw, 2, ups=1))
    # split-K, one layer per (T, S, G): 7 chunks into 2, 3 (uneven), 5 (-> 4: no empty split) and 7, with and without residual
    for res in (False, True):
        for fks in (2, 3, 5, 7):
            kw = dict(res=res, fks=fks)
            out += [_conv3x3("splitk", 5, 6, 5, 112, 48, 1, 1, 2, **kw), _conv1x1("splitk", 5, 6, 5, 112, 96, 2, **kw),
                    _s2("splitk", 5, 6, 5, 112, 64, 2, 1, **kw), _convT("splitk", 5, 6, 5, 112, 48, **kw), _ups4("splitk", 5, 3, 4, 112, 32, **kw)]
    # channel views, every class that computes its own offsets, partial cout blocks included
    for N, H, W in ((5, 6, 5), (3, 19, 37)):
        kw = dict(view=True, res=True)
        out += [_conv3x3("views", N, H, W, 48, 96, 2, 4, 2, **kw), _conv3x3("views", N, H, W, 48, 48, 1, 2, 2, **kw),
                _conv3x3("views", N, H, W, 48, 48, 1, 1, 2, **kw), _conv3x3("views", N, H, W, 96, 96, 2, 2, 4, **kw),
                _conv3x3("views", N, H, W, 96, 48, 1, 1, 4, **kw),
                _conv1x1("views", N, H, W, 48, 48, 1, **kw), _conv1x1("views", N, H, W, 64, 96, 2, **kw), _conv1x1("views", N, H, W, 96, 128, 4, **kw),
                _s2("views", N, H, W, 64, 48, 1, 1, **kw), _s2("views", N, H, W, 64, 96, 2, 0, **kw),
                _convT("views", N, H, W, 48, 48, **kw), _convT("views", N, H, W, 64, 48, **kw), _ups4("views", N, H // 2 + 1, W // 2 + 1, 32, 48, **kw),
                _conv3x3("views", N, 2 * (H // 2 + 1), 2 * (W // 2 + 1), 48, 48, 1, 2, 2, ups=1, **kw),
                _conv3x3("views", N, H, W, 112, 48, 1, 1, 2, fks=3, **kw), _convT("views", N, H, W, 112, 48, fks=3, **kw)]
    # activations: ReLU, GELU, SiLU once per class (the default 0 clamps nothing)
    for act in (1, 2, 3):
        out += [_conv3x3("act", 2, 9, 16, 48, 48, 1, 2, 2, act=act), _conv1x1("act", 2, 9, 16, 48, 48, 1, act=act), _s2("act", 2, 9, 16, 64, 48, 1, 1, act=act),
                _convT("act", 2, 9, 16, 48, 32, act=act), _ups4("act", 2, 5, 8, 32, 32, act=act), _conv3x3("act", 2, 10, 16, 48, 48, 1, 1, 2, ups=1, act=act)]
    # rowgemm: one-pixel maps as skinny GEMMs, 1 / 3 / 32 frames (33 is refused), K 512 / 8192
    for M in (1, 3, 32):
        for K in (512, 8192):
            out.append(Case("row", M, 1, 1, K, 512, k=1, pad=0, family=1, expect=ROW_KERNELS[0 if M <= 16 else 1], act=1 if K == 512 else 0))
    out += [Case("row", 3, 1, 1, 512, 512, k=1, pad=0, family=1, view=True, expect=ROW_KERNELS[0]),
            Case("row", 32, 1, 1, 8192, 512, k=1, pad=0, family=1, view=True, expect=ROW_KERNELS[1], act=1)]
    # rowconv: 3x3 to 4x4 / 8x8 outputs, stride 1 / 2; 1024 rows, ragged counts below, and 1040 rows to 256 channels (the 64-row tiles)
    rc = lambda N, H, C, J, s, **kw: Case("row", N, H, H, C, J, stride=s, family=2, expect=ROW_KERNELS[3 if -(-N * (H // s) ** 2 // 16) * (J // 32) > 512 else 2], **kw)
    out += [rc(16, 8, 256, 128, 1, res=True), rc(16, 16, 256, 128, 2), rc(3, 4, 512, 256, 1, res=True, act=1), rc(5, 8, 512, 256, 2), rc(7, 8, 256, 128, 2, res=True),
            rc(65, 4, 256, 256, 1, res=True), rc(3, 4, 256, 128, 1, res=True, view=True), rc(5, 8, 256, 256, 2, view=True, res=True)]
    # rowconvT: 4x4 -> 8x8
    out += [Case("row", 3, 4, 4, 512, 256, stride=2, transposed=True, out_pad=1, family=3, expect=ROW_KERNELS[4], view=v, act=1 - int(v)) for v in (False, True)]
    # (appended so that the cases above keep their index, which seeds their inputs)
    # the split-K finish applies the activation itself, behind the residual: ReLU, GELU, SiLU on a three-way split per (T, S, G), with residual
    for act in (1, 2, 3):
        kw = dict(res=True, fks=3, act=act)
        out += [_conv3x3("act", 5, 6, 5, 112, 48, 1, 1, 2, **kw), _conv1x1("act", 5, 6, 5, 112, 96, 2, **kw), _s2("act", 5, 6, 5, 112, 64, 2, 1, **kw),
                _convT("act", 5, 6, 5, 112, 48, **kw), _ups4("act", 5, 3, 4, 112, 32, **kw)]
    # the upsample read computes its own source offsets: views at the 128- and 512-pixel tiles as well
    for N, H, W in ((5, 6, 5), (3, 19, 37)):
        out += [_conv3x3("views", N, 2 * (H // 2 + 1), 2 * (W // 2 + 1), 48, 48, 1, pxw, 2, ups=1, view=True, res=True) for pxw in (1, 4)]
    return out


CASES = _cases()
CLASSES = ("3x3", "1x1", "s2", "g4", "splitk", "views", "act", "row")


def groups() -> Dict[str, List[int]]:
    """Case indices per test: a class, split by the expected kernel where the class has many cases."""
    g: Dict[str, List[int]] = {}
    for i, c in enumerate(CASES):
        key = f"{c.cls}:{c.expect}" if c.cls in ("3x3", "1x1") else f"{c.cls}:{c.N}x{c.H}x{c.W}" if c.cls == "views" else \
            f"{c.cls}:{('', 'rowgemm', 'rowconv', 'rowconvT')[c.family]}" if c.cls == "row" else f"{c.cls}:res{int(c.res)}" if c.cls == "splitk" else \
            f"{c.cls}:split" if c.cls == "act" and c.ksplit > 1 else c.cls
        g.setdefault(key, []).append(i)
    return g


# ---------------------------------------------------------------------------------------------------- the op
def core(c: Case, x: torch.Tensor, w: torch.Tensor) -> torch.Tensor:
    """The convolution alone, in x's dtype: x [N, Cin, Hs, Ws] (the source map), w in torch layout."""
    if c.ups:
        x = F.interpolate(x, scale_factor=2, mode="nearest")
    if c.transposed:
        return F.conv_transpose2d(x, w, stride=2, padding=1, output_padding=1)
    if c.out_pad:
        x = F.pad(x, (0, 1, 0, 1))
    return F.conv2d(x, w, stride=c.stride, padding=c.pad)


def activate(c: Case, t: torch.Tensor) -> torch.Tensor:
    return (t, torch.relu(t), F.gelu(t), F.silu(t))[c.act]


def _cb(t: torch.Tensor) -> np.ndarray:
    """[N, C, H, W] -> fp16 [N, C / 16, H, W, 16]"""
    N, C, H, W = t.shape
    return t.reshape(N, C // 16, 16, H, W).permute(0, 1, 3, 4, 2).contiguous().numpy().astype(np.float16)


def _nchw(a: np.ndarray) -> torch.Tensor:
    """[N, cb, H, W, 16] -> float32 [N, cb * 16, H, W]"""
    N, cb, H, W, _ = a.shape
    return torch.from_numpy(a.astype(np.float32)).permute(0, 1, 4, 2, 3).reshape(N, cb * 16, H, W)


class Buffers:
    def __init__(self, c: Case, x, res, seed):
        rng = np.random.default_rng(seed)
        N = c.N

        def guarded(t, lead, tail):
            cb = t.shape[1] // 16
            mag = GUARD_GAIN * float(t.abs().max())
            shape = (N + 1, lead + cb + tail) + tuple(t.shape[2:]) + (16,)
            buf = (rng.choice([-1.0, 1.0], shape) * rng.uniform(0.5, 1.0, shape) * mag).astype(np.float16)
            buf[:N, lead:lead + cb] = _cb(t)
            return buf, lead + cb + tail, lead

        self.x, self.x_cbt, self.x_cb0 = guarded(x, 1, 1) if c.view else guarded(x, 0, 0)
        self.r_cbt, self.r_cb0, self.res = c.Cout // 16, 0, None
        if res is not None:
            self.res, self.r_cbt, self.r_cb0 = guarded(res, 1, 1) if c.view else guarded(res, 0, 0)
        self.y_cb0 = 2 if c.view else 0
        self.y_cbt = c.Cout // 16 + (3 if c.view else 0)
        self.y_shape = (N + 1, self.y_cbt, c.Ho, c.Wo, 16)

    def empty_y(self) -> np.ndarray:
        return np.full(self.y_shape, PATTERN, np.int16)


class Reference:
    """Inputs, buffers, float64 reference, rounding model and bound of one case: computed once, read by every comparison."""

    def __init__(self, ci: int):
        c = self.c = CASES[ci]
        g = torch.Generator().manual_seed(5000 + ci)
        rn = lambda *s: torch.randn(*s, generator=g)
        self.x = R.f16(rn(c.N, c.Cin, c.Hs, c.Ws))
        fan = c.Cin * c.k * c.k / (4 if c.transposed else 1)
        w = rn(*((c.Cin, c.Cout) if c.transposed else (c.Cout, c.Cin)), c.k, c.k) * (2.0 / fan) ** 0.5
        if c.ups == 2:
            w = (w * 256).round().clamp(-255, 255) / 256        # sums of up to four taps stay exact in fp16
        self.w = R.f16(w)
        self.scale = torch.rand(c.Cout, generator=g) + 0.5
        self.shift = rn(c.Cout) * 0.1
        self.r = R.f16(rn(c.N, c.Cout, c.Ho, c.Wo)) if c.res else None
        self.buf = Buffers(c, self.x, self.r, 7000 + ci)
        with torch.no_grad():
            d = lambda t: t.double()
            sc, sf = self.scale.view(1, -1, 1, 1), self.shift.view(1, -1, 1, 1)
            pre = core(c, d(self.x), d(self.w)) * d(sc) + d(sf)
            A = core(c, d(self.x).abs(), d(self.w).abs()) * d(sc).abs() + d(sf).abs()
            pm = core(c, self.x, self.w) * sc + sf
            if c.res:
                pre, A, pm = pre + d(self.r), A + d(self.r).abs(), pm + self.r
            self.ref = activate(c, pre)
            self.mod = activate(c, pm).half().float()
            slope = (1.0, 1.0, R.GELU_SLOPE, SILU_SLOPE)[c.act]
            self.tol = 2.0 ** -10 * self.ref.abs() + slope * c.n_prod * 2.0 ** -23 * A + R.F16_FLOOR

    # what sim_device reads: the operands as the device holds them (tests/conv_fp8_cases.py has the e4m3 ones and their faults)
    sim_chunk = property(lambda self: 8 * self.c.NC8)           # input channels per chunk

    def sim_x(self, cb0: int, fault: Optional[str]) -> torch.Tensor:
        return _nchw(self.buf.x[:self.c.N, cb0:cb0 + self.c.Cin // 16])

    def sim_w(self, fault: Optional[str]) -> torch.Tensor:
        return self.w

    def sim_scale(self, fault: Optional[str]) -> torch.Tensor:
        return self.scale


@functools.lru_cache(maxsize=8)
def reference(ci: int) -> Reference:
    return Reference(ci)


def check(rf: Reference, y: np.ndarray, kernel: str = "") -> Tuple[dict, List[str]]:
    """Both gates on the view of output buffer `y` and the pattern outside it -> (op_replay's record, one line per failure)."""
    c, b = rf.c, rf.buf
    dev = _nchw(y.view(np.float16)[:c.N, b.y_cb0:b.y_cb0 + c.Cout // 16])
    rp = R.Replay({}, None)
    rp.record(f"{c.id} {kernel}", dev, rf.ref, rf.mod, rf.tol)
    r = rp.records[0]
    r["violators"] = int((~((dev.double() - rf.ref).abs() <= rf.tol)).sum())          # a NaN is a violator
    bad = R.failures(rp.records)
    if not math.isfinite(r["rel_dev"]) and not bad:
        bad.append(f"{c.id}: rel_l2(dev, ref) is not finite")
    keep = np.ones(y.shape, bool)
    keep[:c.N, b.y_cb0:b.y_cb0 + c.Cout // 16] = False
    touched = (y != np.int16(PATTERN)) & keep
    if touched.any():
        bad.append(f"{c.id}: {int(touched.sum())} halfs outside the view were written ({int(touched[c.N:].sum())} of them in the image behind the "
                   f"last, {int(touched[:c.N].sum())} in the channel blocks around [{b.y_cb0}, {b.y_cb0 + c.Cout // 16}))")
    return r, bad


def format_record(c: Case, kernel: str, ksplit: int, r: dict) -> str:
    return (f"[conv3 {c.cls}] {c.id:58s} {kernel:30s} ks {ksplit}  max|dev-ref|/tol {r['dev_over_tol']:5.2f} (model {r['mod_over_tol']:4.2f})  "
            f"rel_l2 dev {r['rel_dev']:.3e} mod {r['rel_mod']:.3e}")


# ---------------------------------------------------------------------------------------------------- simulated device
FAULTS = {
    "chunk": "the last channel chunk dropped",
    "split": "one split's partial slab not added",
    "x_cb0": "x_cb0 ignored",
    "y_cb0": "y_cb0 off by one block",
    "halo": "a halo column taken from the neighbouring row instead of zero",
    "image": "the last image of a multi-image tile skipped",
    "coutpad": "a partial cout block's padding channels written into the next blocks of the buffer",
    "ups": "ups reading pixel (y, x) instead of (y / 2, x / 2)",
    "finish_act": "the split-K finish applying the activation in front of the residual",
    "finish_noact": "the split-K finish skipping the activation",
}


def applies(fault: str, c: Case) -> bool:
    if fault == "split":
        return c.ksplit > 1
    if fault == "x_cb0":
        return c.view
    if fault == "halo":           # (stride 2 without a left pad reads the column behind the map only when W is even)
        return c.k == 3 and c.H * c.W > 1 and not (c.stride == 2 and not c.transposed and c.pad == 0 and c.W % 2)
    if fault == "image":
        return c.family == 0 and c.N > 1 and geometry(c)["NB"] > 1
    if fault == "coutpad":
        return c.family == 0 and c.Cout % (32 * c.NBT) != 0
    if fault == "ups":
        return c.ups == 1
    if fault == "finish_act":
        return c.ksplit > 1 and c.act > 0 and c.res
    if fault == "finish_noact":
        return c.ksplit > 1 and c.act > 0
    return True


def _halo(x: torch.Tensor, wrap: bool) -> torch.Tensor:
    """x [N, C, H, W] with a one-pixel frame: zeros; `wrap`: the left / right frame columns are what the flat address row * W + col holds
    (the neighbouring row's last / first pixel), as a patch copy without the column test reads them."""
    N, C, H, W = x.shape
    xp = F.pad(x, (1, 1, 1, 1))
    if wrap:
        flat = F.pad(x.reshape(N, C, H * W), (1, 1))          # flat index -1 .. H * W
        rows = torch.arange(H)
        xp[:, :, 1:H + 1, 0] = flat[:, :, rows * W]            # (row, -1) -> row * W - 1
        xp[:, :, 1:H + 1, W + 1] = flat[:, :, rows * W + W + 1]
    return xp


def sim_device(rf: Reference, fault: Optional[str] = None) -> np.ndarray:
    """The op as the conv3 family computes it, buffer to buffer, in fp32: the input view read from its channel blocks (through the
    nearest-upsample index where the kernel does that; rf.sim_x / sim_w / sim_scale: fp16 here, e4m3 codes in conv_fp8_cases), zero halo, one partial sum per channel chunk, the chunks of a split summed into
    its slab and the slabs in order, the affine + residual + activation on the fp32 sum, one rounding to fp16, the images of a tile stored
    one by one into the view's channel blocks of the pre-filled output buffer.  `fault`: one of FAULTS."""
    c, b = rf.c, rf.buf
    N = c.N
    geo = geometry(c)
    cb0 = 0 if fault == "x_cb0" else b.x_cb0
    x, w, scale = rf.sim_x(cb0, fault), rf.sim_w(fault), rf.sim_scale(fault)
    if c.ups == 1:
        if fault == "ups":
            yy, xx = torch.meshgrid(torch.arange(c.H), torch.arange(c.W), indexing="ij")
            x = x.reshape(N, c.Cin, c.Hs * c.Ws)[:, :, ((yy * c.Ws + xx) % (c.Hs * c.Ws)).reshape(-1)].reshape(N, c.Cin, c.H, c.W)
        else:
            x = F.interpolate(x, scale_factor=2, mode="nearest")
    wrap = fault == "halo"

    def part(xc, wc):
        if c.k == 1:
            return F.conv2d(xc, wc)
        xp = _halo(xc, wrap)
        if c.transposed:                                        # the row / column behind the map is the halo of the merged phases
            return F.conv_transpose2d(xp[:, :, 1:, 1:], wc, stride=2, padding=1, output_padding=1)[:, :, :c.Ho, :c.Wo]
        if c.ups == 2:                                          # the halo lives on the SOURCE map
            return F.conv2d(F.interpolate(xp, scale_factor=2, mode="nearest")[:, :, 1:-1, 1:-1], wc)
        if c.out_pad:
            xp = xp[:, :, 1:, 1:]
        return F.conv2d(xp, wc, stride=c.stride)

    per = rf.sim_chunk
    acc = None
    with torch.no_grad():
        for s in range(c.ksplit):
            slab = None
            for ch in range(s * c.cps, min(c.nchunks, (s + 1) * c.cps)):
                if fault == "chunk" and ch == c.nchunks - 1:
                    continue
                sl = slice(ch * per, (ch + 1) * per)
                p = part(x[:, sl], w[sl] if c.transposed else w[:, sl])
                slab = p if slab is None else slab + p
            if slab is None or (fault == "split" and s == 1):
                continue
            acc = slab if acc is None else acc + slab
        if acc is None:
            acc = torch.zeros(N, c.Cout, c.Ho, c.Wo)
        pre = acc * scale.view(1, -1, 1, 1) + rf.shift.view(1, -1, 1, 1)
        r = _nchw(b.res[:N, b.r_cb0:b.r_cb0 + c.Cout // 16]) if c.res else 0.0
        if fault == "finish_act":
            out = _cb(activate(c, pre) + r)
        elif fault == "finish_noact":
            out = _cb(pre + r)
        else:
            out = _cb(activate(c, pre + r))
    y = b.empty_y().view(np.float16)
    yb = y.reshape((N + 1) * b.y_cbt, c.Ho, c.Wo, 16)           # block (n, cb) at n * y_cbt + cb, as the kernels address it
    ncb = c.Cout // 16
    first = b.y_cb0 + (1 if fault == "y_cb0" else 0)
    pad_cb = -(-c.Cout // (32 * c.NBT)) * 2 * c.NBT
    for n in range(N):
        NB = geo["NB"]
        if fault == "image" and (n % NB == NB - 1 or n == N - 1) and n % NB != 0:
            continue
        if fault == "coutpad":
            for k in range(ncb, pad_cb):
                yb[n * b.y_cbt + b.y_cb0 + k] = 0
        for k in range(ncb):
            at = n * b.y_cbt + first + k
            if at < yb.shape[0]:
                yb[at] = out[n, k]
    return y.view(np.int16).reshape(b.y_shape)
