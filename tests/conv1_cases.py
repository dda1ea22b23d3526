"""What tests/test_conv1_host.py (CPU), tests/test_conv1_gpu.py and tests/test_w2l_head_gpu.py share: the cases at which the first-generation
conv kernel of csrc/conv_mfma.hip and the special-case kernels of csrc/conv7_mfma.hip change path, their inputs and buffers, the float64
reference, and simulated devices that compute each op as the kernels do and can be told to get it wrong.  Buffers, gates, the record and the
layout helpers are those of tests/conv_cases.py (Buffers, check, _cb, _nchw); nothing of them is restated here.

First generation.  A case names the instantiation it expects in the spelling of ltk_debug_conv1_variants, conv_mfma_kernel<NC8,NBT,TT9,MAXA>,
written by hand from conv_route (NC8, the widest NBT, TT9) and conv1_plan_launch (the effective NBT, MAXA from the staged items); the cases
an edge is named for also state their tile (l2w, l2h, NB, s2half) by hand.  geometry() restates conv1_plan_launch's arithmetic; the CPU
suite holds both to ltk_debug_conv_plan.  `v3` = knob CONV_V3 while the plan is built: 0 routes the 1x1 convs and the transposed convs here.

Inputs as in conv_cases: x, w, res drawn in fp32 and rounded to fp16, scale = U(0.5, 1.5), shift = 0.1 N(0, 1).  An input of <= 8 channels
is the plain [N + 1][H][W][8] tensor the kernel reads (channels past Cin zero, image N a guard).

Per element: |dev - ref| <= 2^-10 |ref| + slope n 2^-23 A + 2^-24 (conv_cases' derivation), n = the products per output as the device forms
them: taps x padded Cin; Tp x 8 on the 8-channel path (Tp = the taps padded to even); 4 Cin for the four-phase transposed conv; Cin for the
k x k transposed conv on a 1x1 map (one 1x1 GEMM).  Aggregate: rel_l2(dev, ref) <= 2 rel_l2(mod, ref) + 1e-4.

The head kernels (conv7 BANK / PACKED, audio0, audio3, convs2d): the same gates with n = 14 x 32 (conv7: 14 MFMAs of k = 32, the zero tap
and the zero channels included), 9 (audio0: nine fma), 9 Cin (audio3, convs2d).  Two operands are part of the op's definition: conv7 BANK
holds fp16(fp32(byte) * fp32(1 / 255)) with rows >= 128 of channels 0..2 and channels 6, 7 zero; audio0 holds fp16(mel).  They are formed
in numpy exactly so, and the float64 reference is taken on them."""
from __future__ import annotations

import functools
from typing import Dict, List, Optional

import numpy as np
import torch
import torch.nn.functional as F

import conv_cases as K
from oracle import op_replay as R

GUARD_GAIN, PATTERN = K.GUARD_GAIN, K.PATTERN
PATTERN_F16 = np.array([PATTERN], np.int16).view(np.float16)[0]
K_MIN_BLOCKS = 512          # conv1_plan_launch: 64-cout blocks only while the launch keeps this many
LDS_LIMIT = 160 * 1024


def vn(nc8, nbt, tt9, maxa) -> str:
    return f"conv_mfma_kernel<{nc8},{nbt},{'true' if tt9 else 'false'},{maxa}>"


def _pair(v):
    return (v, v) if isinstance(v, int) else tuple(v)


class Case:
    """H x W is the input map (the source map of a transposed conv)."""

    def __init__(self, cls, N, H, W, Cin, Cout, k=3, stride=1, pad=0, transposed=False, out_pad=0, res=False, act=0, view=False, v3=1, expect="",
                 tile=None):
        self.cls, self.N, self.H, self.W, self.Cin, self.Cout = cls, N, H, W, Cin, Cout
        self.k, self.stride, self.pad = k, stride, pad
        (self.kh, self.kw), (self.sh, self.sw), (self.ph, self.pw) = _pair(k), _pair(stride), _pair(pad)
        self.transposed, self.out_pad, self.res, self.act, self.view, self.v3, self.expect, self.tile = transposed, out_pad, res, act, view, v3, expect, tile
        self.expand = transposed and self.sh == 1                   # k x k transposed conv on a 1x1 map: a GEMM to k * k * Cout channels
        self.four = transposed and not self.expand                  # ConvTranspose2d(k3, s2, p1, op1) as four sub-pixel phases
        if self.expand:
            self.Ho, self.Wo = self.kh * H, self.kw * W
        elif self.four:
            self.Ho, self.Wo = 2 * H, 2 * W
        else:
            self.Ho, self.Wo = (H + 2 * self.ph - self.kh) // self.sh + 1, (W + 2 * self.pw - self.kw) // self.sw + 1
        nc8, nbt, tt9, maxa = expect[expect.index("<") + 1:-1].split(",")
        self.NC8, self.NBT, self.TT9, self.MAXA = int(nc8), int(nbt), tt9 == "true", int(maxa)
        self.CinP = 8 if Cin <= 8 else Cin
        self.taps = 1 if self.expand else 4 if self.four else self.kh * self.kw       # per chunk (the widest phase)
        self.Tp = (self.taps + 1) // 2 * 2 if self.NC8 == 1 else self.taps
        self.lCout = self.kh * self.kw * Cout if self.expand else Cout
        self.nphase = 4 if self.four else 1
        self.nchunks = -(-(self.CinP // 8) // self.NC8)
        self.n_prod = self.Tp * 8 if self.NC8 == 1 else 4 * Cin if self.four else Cin if self.expand else self.taps * self.CinP
        self.macs = N * self.Ho * self.Wo * Cout * Cin * (1 if self.expand else self.kh * self.kw / 4 if self.four else self.kh * self.kw)

    @property
    def id(self) -> str:
        j = lambda a, b: f"{a}" if a == b else f"{a}x{b}"
        kind = ("convT" if self.four else "expand" if self.expand else "") + f"k{j(self.kh, self.kw)}s{j(self.sh, self.sw)}p{j(self.ph, self.pw)}"
        s = f"{self.N}x{self.H}x{self.W}-{self.Cin}to{self.Cout}-{kind}" + ("" if self.v3 else "-v3off") + ("-res" if self.res else "")
        return s + (f"-{K.ACT_NAMES[self.act]}" if self.act else "") + ("-view" if self.view else "")

    def opts(self, b) -> dict:
        o = dict(act=self.act)
        if self.view:
            o.update(y_ld=b.y_cbt * 16, y_coff=b.y_cb0 * 16, res_ld=b.r_cbt * 16, res_coff=b.r_cb0 * 16)
            if self.NC8 > 1:                   # the 8-channel input is no channel-blocked tensor: no view of it (refused)
                o.update(x_ld=b.x_cbt * 16, x_coff=b.x_cb0 * 16)
        return o


# ---------------------------------------------------------------------------------------------------- geometry (conv1_plan_launch's)
def geometry(c: Case) -> dict:
    """The tile, the effective block width, the blocks, the LDS bytes and s2half of a launch, as conv1_plan_launch derives them."""
    if c.expand:
        Ho = Wo = 1
        sh = sw = 1
        ky = kx = 1
    elif c.four:
        Ho, Wo, sh, sw, ky, kx = c.H, c.W, 1, 1, 2, 2
    else:
        Ho, Wo, sh, sw, ky, kx = c.Ho, c.Wo, c.sh, c.sw, c.kh, c.kw
    l2w = min(5, K._clog2(Wo))
    l2h = min(8 - l2w, K._clog2(Ho))
    maxpix = {4: 6, 1: 5, 2: 10}[c.NC8] * 256 // c.NC8
    shrunk = False
    while True:
        PH, PW = ((1 << l2h) - 1) * sh + ky, ((1 << l2w) - 1) * sw + kx
        NB = min(256 >> (l2w + l2h), maxpix // (PH * PW))
        if NB >= 1:
            break
        shrunk = True
        if l2h > 0:
            l2h -= 1
        else:
            l2w -= 1
    NB = min(NB, c.N)
    npix = NB * PH * PW
    NPIXP = npix
    if c.NC8 > 1:
        while NPIXP & 7 != (2 if c.NC8 == 4 else 4):
            NPIXP += 1
    mtiles = c.nphase * -(-c.N // NB) * -(-Ho // (1 << l2h)) * -(-Wo // (1 << l2w))
    # conv_route: the widest block the staging registers allow, then at most 64 couts, then the 512-block rule
    NBT = 1 if c.NC8 == 1 else 4 if c.lCout >= 128 else 2 if c.lCout >= 64 else 1
    if c.NC8 > 1:
        while c.taps * c.NC8 * NBT * 32 > 9 * 256 and NBT > 1:
            NBT //= 2
        NBT = min(NBT, 2)
        while NBT > 1 and mtiles * -(-c.lCout // (32 * NBT)) < K_MIN_BLOCKS:
            NBT //= 2
    BN = 32 * NBT
    blocks = mtiles * -(-c.lCout // BN)
    lds = max(c.NC8 * NPIXP * 16 + c.Tp * c.NC8 * BN * 16, 4 * 64 * (BN * 2 + 16)) + 128
    lds = (lds + 255) // 256 * 256
    need = (npix * c.NC8 + 255) // 256
    s2half = (PW + 1) // 2 if (c.TT9 and sw == 2 and l2w >= 4) else 0
    return dict(l2w=l2w, l2h=l2h, NB=NB, PH=PH, PW=PW, NBT=NBT, blocks=blocks, lds=lds, need=need, s2half=s2half, shrunk=shrunk,
                fit=lds <= LDS_LIMIT and need <= c.MAXA and npix < 65536)


def report_mismatches(c: Case, g: dict, rep: dict) -> List[str]:
    """What a report (the planner's, or the launch's) says against the case and its geometry, one line per difference."""
    bad = []
    if rep["kernel"] != c.expect:
        bad.append(f"{c.id}: {rep['kernel']!r}, the case expects {c.expect!r}")
    if (rep["family"], rep["NC8"], rep["NBT"], rep["T"], rep["S"], rep["phases"]) != (0, c.NC8, c.NBT, c.Tp, 1 if c.transposed else c.sw, c.nphase):
        bad.append(f"{c.id}: the report's NC8 {rep['NC8']}, NBT {rep['NBT']}, T {rep['T']}, S {rep['S']}, phases {rep['phases']} are not the case's")
    got = (rep["l2w"], rep["l2h"], rep["NB"], rep["s2half"])
    if got != (g["l2w"], g["l2h"], g["NB"], g["s2half"]) or (c.tile and got != c.tile):
        bad.append(f"{c.id}: tile (l2w, l2h, NB, s2half) {got}; expected {(g['l2w'], g['l2h'], g['NB'], g['s2half'])}" + (f", by hand {c.tile}" if c.tile else ""))
    if (rep["items"], rep["grid"], rep["lds"]) != (g["blocks"], g["blocks"], g["lds"]):
        bad.append(f"{c.id}: {rep['items']} items on {rep['grid']} blocks with {rep['lds']} LDS bytes; expected {g['blocks']} blocks, {g['lds']} bytes")
    return bad


# ---------------------------------------------------------------------------------------------------- the cases
WIDE = 32768            # output channels that give a launch of one tile its 512 blocks of 64 (the NBT = 2 instantiations)


def _cases() -> List[Case]:
    o: List[Case] = []
    C = lambda *a, **kw: o.append(Case(*a, **kw))
    # ---- NC8 = 1: inputs of <= 8 channels, two taps per MFMA, an odd tap count padded with a zero tap
    e = vn(1, 1, False, 5)
    C("nc8_1", 3, 19, 37, 6, 16, k=7, pad=3, expect=e, tile=(5, 3, 1, 0))              # 49 taps -> 50; Cout 16: half a 32-cout block
    C("nc8_1", 5, 6, 5, 6, 16, k=7, pad=3, act=1, expect=e, tile=(3, 3, 4, 0))         # 4 images per tile, 5 images: a short last tile
    C("nc8_1", 5, 6, 5, 1, 32, pad=1, expect=e, tile=(3, 3, 4, 0))
    C("nc8_1", 2, 9, 16, 3, 32, pad=1, res=True, expect=e)
    C("nc8_1", 1, 1, 1, 8, 16, pad=1, expect=e, tile=(0, 0, 1, 0))
    C("nc8_1", 19, 1, 1, 8, 16, pad=1, act=2, expect=e, tile=(0, 0, 19, 0))            # 19 images in one tile
    C("nc8_1", 5, 6, 5, 3, 32, pad=1, res=True, view=True, expect=e)                   # views of y and res (x takes none)
    # ---- NC8 = 4, TT9: 3x3 without padding on >= 32 channels
    e = vn(4, 1, True, 6)
    C("nc8_4_tt9", 3, 19, 37, 32, 48, expect=e, tile=(5, 3, 1, 0))                     # Cout 48: one and a half blocks
    C("nc8_4_tt9", 5, 6, 5, 48, 32, act=1, expect=e, tile=(2, 2, 5, 0))                # Cin 48: the last chunk holds 2 of 4 planes
    C("nc8_4_tt9", 2, 9, 16, 96, 80, res=True, expect=e)                               # (64-cout blocks allowed, too few blocks for them)
    C("nc8_4_tt9", 19, 3, 3, 48, 32, act=3, expect=e, tile=(0, 0, 19, 0))              # 3x3 -> 1x1
    C("nc8_4_tt9", 1, 3, 3, 32, 16, expect=e, tile=(0, 0, 1, 0))
    C("nc8_4_tt9", 5, 6, 5, 48, 48, res=True, view=True, expect=e)
    C("nbt2", 384, 3, 35, 32, 96, res=True, expect=vn(4, 2, True, 6), tile=(5, 0, 3, 0))   # 2 x 128 tiles x 2 blocks of 64 (96: the second half valid)
    # ---- NC8 = 4, not TT9: the conv1d form; with CONV_V3 = 0 the 1x1 convs and the transposed convs on >= 32 channels
    e = vn(4, 1, False, 6)
    C("nc8_4", 3, 19, 37, 32, 48, k=(1, 3), pad=(0, 1), expect=e, tile=(5, 3, 1, 0))
    C("nc8_4", 5, 6, 5, 64, 32, k=(1, 3), pad=(0, 1), res=True, act=2, expect=e)
    C("nc8_4", 3, 3, 3, 32, 96, k=(1, 3), pad=(0, 1), expect=e)                        # the NBT = 1 twin of the wide layer below
    C("nbt2", 3, 3, 3, 32, WIDE, k=(1, 3), pad=(0, 1), expect=vn(4, 2, False, 6), tile=(2, 2, 3, 0))
    C("nc8_4", 19, 1, 1, 64, 48, k=1, v3=0, expect=e, tile=(0, 0, 19, 0))              # PHW == 1
    C("nc8_4", 2, 9, 1, 48, 32, k=1, v3=0, act=1, expect=e, tile=(0, 4, 2, 0))         # PW == 1; Cin 48: a partial last chunk
    C("nc8_4", 3, 5, 7, 64, 48, stride=2, pad=1, transposed=True, out_pad=1, v3=0, expect=e, tile=(3, 3, 3, 0))
    C("nc8_4", 2, 19, 21, 64, 32, stride=2, pad=1, transposed=True, out_pad=1, v3=0, act=1, expect=e)
    C("nc8_4", 3, 5, 7, 64, 48, stride=2, pad=1, transposed=True, out_pad=1, v3=0, res=True, view=True, expect=e)
    C("nc8_4", 3, 1, 1, 64, 32, k=4, transposed=True, v3=0, expect=e, tile=(0, 0, 3, 0))   # gemm_1x1_expand: 512 logical couts
    C("nc8_4", 5, 6, 5, 96, 48, k=(1, 3), pad=(0, 1), res=True, view=True, expect=e)
    # ---- NC8 = 2, TT9: 3x3 on 16 channels, and every strided 3x3; MAXA 3 up to 384 patch pixels, 10 above
    e3, e10 = vn(2, 1, True, 3), vn(2, 1, True, 10)
    C("nc8_2_tt9", 3, 19, 37, 16, 32, expect=e3, tile=(5, 3, 1, 0))
    C("nc8_2_tt9", 5, 6, 5, 16, 48, res=True, expect=e3)
    C("nc8_2_tt9", 3, 5, 5, 16, 96, expect=e3)                                          # the NBT = 1 twin
    C("nbt2", 3, 5, 5, 16, WIDE, expect=vn(2, 2, True, 3), tile=(2, 2, 3, 0))
    C("nc8_2_tt9", 3, 6, 5, 16, 32, stride=2, pad=1, expect=e3, tile=(2, 2, 3, 0))      # Wo 3: plain rows
    C("nc8_2_tt9", 5, 6, 5, 32, 48, stride=2, pad=1, act=1, expect=e10, tile=(2, 2, 5, 0))
    C("nc8_2_tt9", 2, 9, 20, 32, 32, stride=2, pad=1, expect=e10, tile=(4, 3, 2, 17))   # Wo 10: l2w 4, s2half
    C("nc8_2_tt9", 2, 9, 20, 16, 48, stride=2, pad=1, res=True, expect=e10, tile=(4, 3, 2, 17))
    C("nc8_2_tt9", 3, 19, 37, 48, 32, stride=2, pad=1, expect=e10, tile=(5, 3, 1, 33))  # Wo 19: l2w 5
    C("nc8_2_tt9", 3, 19, 37, 16, 80, stride=2, pad=1, act=3, expect=e10, tile=(5, 3, 1, 33))
    C("nc8_2_tt9", 2, 9, 20, 32, 64, stride=(3, 2), pad=1, expect=e10, tile=(4, 2, 2, 17))     # s2half under sh = 3
    C("nc8_2_tt9", 3, 19, 37, 32, 48, stride=(3, 1), pad=1, expect=e10, tile=(5, 3, 1, 0))
    C("nc8_2_tt9", 2, 16, 52, 32, 32, stride=3, pad=1, expect=e10, tile=(5, 2, 1, 0))   # a 24 x 96 patch does not fit: the loop lowers l2h to 2
    C("nc8_2_tt9", 2, 9, 20, 32, 48, stride=2, pad=1, res=True, view=True, expect=e10, tile=(4, 3, 2, 17))
    C("nbt2", 2, 1, 33, 16, WIDE, stride=2, pad=1, expect=vn(2, 2, True, 10), tile=(5, 0, 2, 33))
    # ---- NC8 = 2, not TT9: more than 9 taps, strided conv1d, the transposed conv on 16 channels
    e3, e10 = vn(2, 1, False, 3), vn(2, 1, False, 10)
    C("nc8_2", 5, 6, 5, 16, 32, k=4, expect=e3, tile=(1, 2, 5, 0))
    C("nc8_2", 3, 19, 37, 64, 80, k=4, res=True, expect=e10, tile=(5, 3, 1, 0))
    C("nc8_2", 3, 19, 37, 16, 48, k=(1, 3), stride=(1, 2), pad=(0, 1), act=2, expect=e10)
    C("nc8_2", 3, 3, 3, 16, 96, k=(1, 3), stride=(1, 2), pad=(0, 1), expect=e3)         # the NBT = 1 twin
    C("nbt2", 3, 3, 3, 16, WIDE, k=(1, 3), stride=(1, 2), pad=(0, 1), expect=vn(2, 2, False, 3), tile=(1, 2, 3, 0))
    C("nbt2", 6, 1, 33, 16, WIDE, k=(1, 3), stride=(1, 2), pad=(0, 1), expect=vn(2, 2, False, 10), tile=(5, 0, 6, 0))
    C("nc8_2", 2, 19, 21, 16, 32, stride=2, pad=1, transposed=True, out_pad=1, v3=0, expect=e3, tile=(5, 3, 1, 0))
    C("nc8_2", 3, 5, 7, 16, 48, stride=2, pad=1, transposed=True, out_pad=1, v3=0, res=True, act=1, expect=e3)
    C("nc8_2", 5, 6, 5, 32, 48, k=4, res=True, view=True, expect=e3)
    C("nc8_2", 3, 5, 7, 16, 48, stride=2, pad=1, transposed=True, out_pad=1, v3=0, res=True, view=True, expect=e3)
    return o


CASES = _cases()
CLASSES = ("nc8_1", "nc8_4_tt9", "nc8_4", "nc8_2_tt9", "nc8_2", "nbt2")

# (what conv_route or conv1_plan_launch says, plan arguments): refused before anything is enqueued.  The 7x7 on 16 channels is here and not
# among the cases: 49 taps x 2 planes x 32 couts = 3136 16-byte weight items against the 9 x 256 the staging registers hold.
REFUSALS = (
    ("Cout<=32", dict(N=2, H=9, W=16, Cin=6, Cout=48, k=3, stride=1, pad=1)),
    ("multiples of 16", dict(N=2, H=9, W=16, Cin=6, Cout=32, k=3, stride=1, pad=1, x_ld=16, x_coff=0)),
    ("must be contiguous", dict(N=3, H=1, W=1, Cin=64, Cout=32, k=4, stride=1, pad=0, transposed=True, v3=0, y_ld=80, y_coff=16)),
    ("only supported on 1x1 maps", dict(N=3, H=2, W=2, Cin=64, Cout=32, k=4, stride=1, pad=0, transposed=True, v3=0)),
    ("too large for 32-bit offsets", dict(N=128, H=1024, W=1024, Cin=16, Cout=32, k=3, stride=2, pad=1)),
    ("weight slab too large", dict(N=2, H=9, W=16, Cin=16, Cout=32, k=7, stride=1, pad=3)),
    ("conv3 feature", dict(N=2, H=10, W=16, Cin=32, Cout=64, k=3, stride=(3, 1), pad=1, ups=1)),
)


def groups() -> Dict[str, List[int]]:
    g: Dict[str, List[int]] = {}
    for i, c in enumerate(CASES):
        g.setdefault(f"{c.cls}:{c.expect}" if c.cls == "nbt2" else c.cls, []).append(i)
    return g


# ---------------------------------------------------------------------------------------------------- the op
def core(c: Case, x: torch.Tensor, w: torch.Tensor) -> torch.Tensor:
    if c.expand:
        return F.conv_transpose2d(x, w)
    if c.four:
        return F.conv_transpose2d(x, w, stride=2, padding=1, output_padding=1)
    return F.conv2d(x, w, stride=(c.sh, c.sw), padding=(c.ph, c.pw))


class Buffers(K.Buffers):
    """conv_cases.Buffers; an input of <= 8 channels is the plain [N + 1][H][W][8] tensor: channels past Cin zero, image N a guard."""

    def __init__(self, c: Case, x, res, seed):
        if c.NC8 > 1:
            super().__init__(c, x, res, seed)
            return
        super().__init__(c, F.pad(x, (0, 0, 0, 0, 0, 16 - c.Cin)), res, seed)
        rng = np.random.default_rng(seed + 1)
        x8 = np.zeros((c.N + 1, c.H, c.W, 8), np.float16)
        x8[:c.N, :, :, :c.Cin] = x.permute(0, 2, 3, 1).numpy().astype(np.float16)
        shape = x8[c.N].shape
        x8[c.N] = (rng.choice([-1.0, 1.0], shape) * rng.uniform(0.5, 1.0, shape) * GUARD_GAIN * float(x.abs().max())).astype(np.float16)
        self.x, self.x_cbt, self.x_cb0 = x8, 0, 0


class Reference:
    """Inputs, buffers, float64 reference, rounding model and bound of one case: computed once, read by every comparison."""

    def __init__(self, ci: int):
        c = self.c = CASES[ci]
        g = torch.Generator().manual_seed(9000 + ci)
        rn = lambda *s: torch.randn(*s, generator=g)
        self.x = R.f16(rn(c.N, c.Cin, c.H, c.W))
        fan = c.Cin * (1 if c.expand else c.kh * c.kw / 4 if c.four else c.kh * c.kw)
        self.w = R.f16(rn(*((c.Cin, c.Cout) if c.transposed else (c.Cout, c.Cin)), c.kh, c.kw) * (2.0 / fan) ** 0.5)
        self.scale = torch.rand(c.Cout, generator=g) + 0.5
        self.shift = rn(c.Cout) * 0.1
        self.r = R.f16(rn(c.N, c.Cout, c.Ho, c.Wo)) if c.res else None
        self.buf = Buffers(c, self.x, self.r, 11000 + ci)
        with torch.no_grad():
            d = lambda t: t.double()
            sc, sf = self.scale.view(1, -1, 1, 1), self.shift.view(1, -1, 1, 1)
            pre = core(c, d(self.x), d(self.w)) * d(sc) + d(sf)
            A = core(c, d(self.x).abs(), d(self.w).abs()) * d(sc).abs() + d(sf).abs()
            pm = core(c, self.x, self.w) * sc + sf
            if c.res:
                pre, A, pm = pre + d(self.r), A + d(self.r).abs(), pm + self.r
            self.ref = K.activate(c, pre)
            self.mod = K.activate(c, pm).half().float()
            slope = (1.0, 1.0, R.GELU_SLOPE, K.SILU_SLOPE)[c.act]
            self.tol = 2.0 ** -10 * self.ref.abs() + slope * c.n_prod * 2.0 ** -23 * A + R.F16_FLOOR


@functools.lru_cache(maxsize=8)
def reference(ci: int) -> Reference:
    return Reference(ci)


def format_record(tag: str, c, kernel: str, r: dict) -> str:
    return (f"[{tag} {c.cls}] {c.id:52s} {kernel:32s} max|dev-ref|/tol {r['dev_over_tol']:5.2f} (model {r['mod_over_tol']:4.2f})  "
            f"rel_l2 dev {r['rel_dev']:.3e} mod {r['rel_mod']:.3e}")


# ---------------------------------------------------------------------------------------------------- simulated device (first generation)
FAULTS = {
    "chunk": "the last chunk's partial planes dropped",
    "s2half": "the odd-column half of an s2half patch row taken from the even half",
    "halo": "a tile-edge halo column taken from the neighbouring row instead of zero",
    "image": "the last image of a multi-image tile skipped",
    "coutpad": "a partial cout block's padding channels written into the next blocks of the buffer",
    "x_cb0": "x_cb0 ignored",
    "phase_swap": "two phases of the transposed conv written at each other's offsets",
    "tap_pad": "the zero tap that pads an odd tap count (the 7x7's 50th) given a real weight",
}


def applies(fault: str, c: Case) -> bool:
    g = geometry(c)
    if fault == "chunk":
        return c.NC8 > 1 and (c.CinP // 8) % c.NC8 != 0
    if fault == "s2half":
        return g["s2half"] > 0
    if fault == "halo":
        return not c.transposed and c.pw >= 1 and c.H > 1 and c.W > 1
    if fault == "image":
        return c.N > 1 and g["NB"] > 1
    if fault == "coutpad":
        return not c.expand and c.Cout % (32 * c.NBT) != 0
    if fault == "x_cb0":
        return c.view and c.NC8 > 1
    if fault == "phase_swap":
        return c.four
    if fault == "tap_pad":        # (on a map whose every tap (0, 0) lies in the halo the pad tap reads zeros whatever its weight)
        return c.NC8 == 1 and c.taps % 2 == 1 and (c.Ho - 1) * c.sh >= c.ph and (c.Wo - 1) * c.sw >= c.pw
    raise KeyError(fault)


def _wrap_pad(x: torch.Tensor, ph: int, pw: int) -> torch.Tensor:
    """x zero-padded by (ph, pw), the pw columns left and right of a row holding what the flat address row * W + col holds (the neighbouring
    row's pixels, zero in front of the first and behind the last), as a patch copy without the column test reads them."""
    N, C, H, W = x.shape
    flat = F.pad(x.reshape(N, C, H * W), (pw, pw))
    idx = (torch.arange(H) * W).view(H, 1) + torch.arange(W + 2 * pw).view(1, -1)        # flat index (+ pw) of (row, col - pw)
    return F.pad(flat[:, :, idx], (0, 0, ph, ph))


def sim_device(rf: Reference, fault: Optional[str] = None) -> np.ndarray:
    """The op as the first-generation kernel computes it, buffer to buffer, in fp32: the input read from its channel blocks (or the 8-channel
    tensor), zero halo, one partial sum per chunk of 8 NC8 channels, the four phases of the transposed conv, the affine + residual +
    activation on the fp32 sum, one rounding to fp16, the images of a tile stored one by one into the view's channel blocks of the pre-filled
    output buffer.  `fault`: one of FAULTS."""
    c, b = rf.c, rf.buf
    N, geo = c.N, geometry(c)
    w = rf.w
    if c.NC8 == 1:
        x = torch.from_numpy(b.x[:N].astype(np.float32)).permute(0, 3, 1, 2).contiguous()
        w = F.pad(w, (0, 0, 0, 0, 0, 8 - c.Cin))
    else:
        cb0 = 0 if fault == "x_cb0" else b.x_cb0
        x = K._nchw(b.x[:N, cb0:cb0 + c.Cin // 16])
    if fault == "s2half":
        # patch column px = ix + 1 - 2 tx0 (pad 1, even tile origin): the odd px are the even ix; each reads the slot of px - 1
        x = x.clone()
        x[..., 2::2] = (x[..., 1:-1:2] if c.W % 2 else x[..., 1:-2:2]).clone()
        x[..., 0] = 0

    def part(xc, wc):
        if c.transposed:
            return core(c, xc, wc)
        if fault == "halo":
            return F.conv2d(_wrap_pad(xc, c.ph, c.pw), wc, stride=(c.sh, c.sw))
        return F.conv2d(xc, wc, stride=(c.sh, c.sw), padding=(c.ph, c.pw))

    per, Cp = 8 * c.NC8, x.shape[1]
    acc = torch.zeros(N, c.Cout, c.Ho, c.Wo)
    with torch.no_grad():
        for ch in range(c.nchunks):
            lo, hi = ch * per, min((ch + 1) * per, Cp)
            if fault == "chunk" and hi - lo < per:
                continue
            acc = acc + part(x[:, lo:hi], w[lo:hi] if c.transposed else w[:, lo:hi])
        if fault == "tap_pad":        # the pad tap reads patch offset (0, 0), as tap 0 does; its weight: the last tap's
            wf = torch.zeros_like(w)
            wf[:, :, 0, 0] = w[:, :, -1, -1]
            acc = acc + part(x, wf)
        if fault == "phase_swap":
            acc = acc.clone()
            a01, a10 = acc[:, :, 0::2, 1::2].clone(), acc[:, :, 1::2, 0::2].clone()
            acc[:, :, 0::2, 1::2], acc[:, :, 1::2, 0::2] = a10, a01
        pre = acc * rf.scale.view(1, -1, 1, 1) + rf.shift.view(1, -1, 1, 1)
        r = K._nchw(b.res[:N, b.r_cb0:b.r_cb0 + c.Cout // 16]) if c.res else 0.0
        out = K._cb(K.activate(c, pre + r))
    y = b.empty_y().view(np.float16)
    yb = y.reshape((N + 1) * b.y_cbt, c.Ho, c.Wo, 16)
    ncb = c.Cout // 16
    pad_cb = -(-c.Cout // (32 * c.NBT)) * 2 * c.NBT
    NB = geo["NB"]
    for n in range(N):
        if fault == "image" and (n % NB == NB - 1 or n == N - 1) and n % NB != 0:
            continue
        if fault == "coutpad":
            for k in range(ncb, pad_cb):
                if n * b.y_cbt + b.y_cb0 + k < yb.shape[0]:
                    yb[n * b.y_cbt + b.y_cb0 + k] = 0
        for k in range(ncb):
            yb[n * b.y_cbt + b.y_cb0 + k] = out[n, k]
    return y.view(np.int16).reshape(b.y_shape)


# ==================================================================================================== the head kernels (conv7_mfma.hip)
HEAD_OPS = ("conv7_bank", "conv7_packed", "audio0", "audio3", "convs2d")
CONV7_FRAMES = (1, 0, 2, 2, 1, 0, 0, 2, 1)          # frame i of a launch = distinct frame CONV7_FRAMES[i] (permuted, repeated)
MEL_FRAMES = (1, 0, 1)


class HeadCase:
    def __init__(self, op, N, H=0, W=0, Cin=0, Cout=0, view=False):
        self.op, self.N, self.view, self.cls = op, N, view, op
        if op.startswith("conv7"):
            H, W, Cin, Cout, self.k, self.sh, self.sw, self.pad, self.n_prod = 256, 256, 6, 16, 7, 1, 1, 3, 14 * 32
            self.frames = CONV7_FRAMES[:N]
        elif op == "audio0":
            H, W, Cin, Cout, self.k, self.sh, self.sw, self.pad, self.n_prod = 80, 16, 1, 32, 3, 1, 1, 1, 9
            self.frames = MEL_FRAMES[:N]
        elif op == "audio3":
            H, W, Cin, Cout, self.k, self.sh, self.sw, self.pad, self.n_prod = 80, 16, 32, 64, 3, 3, 1, 1, 9 * 32
            self.frames = tuple(range(N))
        else:
            self.k, self.sh, self.sw, self.pad, self.n_prod = 3, 2, 2, 1, 9 * Cin
            self.frames = tuple(range(N))
        self.H, self.W, self.Cin, self.Cout = H, W, Cin, Cout
        self.D = max(self.frames) + 1                   # distinct frames
        self.Ho, self.Wo = (H + 2 * self.pad - self.k) // self.sh + 1, (W + 2 * self.pad - self.k) // self.sw + 1
        self.x_view = view and op in ("audio3", "convs2d")
        self.act = 1
        self.macs = self.D * self.Ho * self.Wo * Cout * Cin * self.k * self.k

    @property
    def id(self) -> str:
        s = f"{self.op}-{self.N}"
        if self.op == "convs2d":
            s += f"x{self.H}x{self.W}-{self.Cin}to{self.Cout}"
        return s + ("-view" if self.view else "")

    def opts(self, b) -> dict:
        o = {}
        if self.view:
            o.update(y_ld=b.y_cbt * 16, y_coff=b.y_cb0 * 16)
            if self.x_view:
                o.update(x_ld=b.x_cbt * 16, x_coff=b.x_cb0 * 16)
        return o


def _head_cases() -> List[HeadCase]:
    o = [HeadCase(op, N, view=(N == 2)) for op in ("conv7_bank", "conv7_packed") for N in (1, 2, 9)]     # 9: 576 tiles > 512, the persistent walk
    o += [HeadCase("audio0", 1), HeadCase("audio0", 3, view=True)]
    o += [HeadCase("audio3", 1), HeadCase("audio3", 2, view=True), HeadCase("audio3", 3)]     # 432 N % 32 = 16 for odd N: a half-live last wave
    o += [HeadCase("convs2d", 3, 2, 64, 16, 32),                  # Ho = 1
          HeadCase("convs2d", 3, 6, 64, 16, 32, view=True),       # 9 tasks: a block with one live wave
          HeadCase("convs2d", 2, 6, 128, 32, 64),                 # two 32-pixel tiles per row, NT = 2
          HeadCase("convs2d", 2, 4, 64, 32, 96, view=True)]       # NT = 3
    return o


HEAD_CASES = _head_cases()

# (op, what the launcher or the plan says, arguments of Engine.w2l_head_f16 beside the buffers)
HEAD_REFUSALS = (
    ("conv7_bank", "conv7: bad arguments", dict(N=257)),
    ("conv7_packed", "conv7: bad arguments", dict(N=1, y_ld=24, y_coff=8)),
    ("audio0", "audio0: bad arguments", dict(N=257)),
    ("audio0", "audio0: bad arguments", dict(N=1, y_ld=40, y_coff=8)),
    ("audio3", "audio3: bad arguments", dict(N=257)),
    ("audio3", "audio3: bad arguments", dict(N=1, x_ld=40, x_coff=8)),
    ("convs2d", "convs2d: bad arguments", dict(N=1, H=3, W=64, Cin=16, Cout=32)),
    ("convs2d", "convs2d: bad arguments", dict(N=1, H=2, W=32, Cin=16, Cout=32)),
    ("convs2d", "convs2d: bad arguments", dict(N=1, H=2, W=64, Cin=16, Cout=32, y_ld=40, y_coff=8)),
    ("convs2d", "16 or 32 input channels", dict(N=1, H=2, W=64, Cin=48, Cout=32)),
    ("convs2d", "16 or 32 input channels", dict(N=1, H=2, W=64, Cin=16, Cout=48)),
    ("audio3", "outside its buffer", dict(N=1, y_ld=32, y_coff=0)),
    ("audio0", "no view of x", dict(N=1, x_ld=16, x_coff=0)),
)


def bank_operand(bgr: np.ndarray) -> np.ndarray:
    """uint8 [D][256][256][3] -> the fp16 [D][256][256][8] operand conv7 forms from a bank crop: fp16(fp32(byte) * fp32(1 / 255)) in
    channels 3..5, the same with rows >= 128 zero in channels 0..2, zero in 6 and 7."""
    v = (bgr.astype(np.float32) * np.float32(1.0 / 255.0)).astype(np.float16)
    x8 = np.zeros(bgr.shape[:3] + (8,), np.float16)
    x8[..., 3:6] = v
    x8[:, :128, :, 0:3] = v[:, :128]
    return x8


class HeadBuffers:
    """Device-side buffers of a head case: the per-frame inputs of the D distinct frames (bank crops uint8 / mel fp32), or the
    channel-blocked (packed [N + 1][256][256][8] for conv7 PACKED) input with guards as conv_cases lays them out; y pre-filled."""

    def __init__(self, c: HeadCase, x: torch.Tensor, seed, frames_u8=None, mel=None):
        rng = np.random.default_rng(seed)
        N = c.N
        self.frames_u8, self.mel = frames_u8, mel
        self.x, self.x_cbt, self.x_cb0 = None, c.Cin // 16, 0
        guard = lambda shape, mag: (rng.choice([-1.0, 1.0], shape) * rng.uniform(0.5, 1.0, shape) * mag).astype(np.float16)
        if c.op == "conv7_packed":
            x8 = bank_operand(frames_u8)[list(c.frames)]
            self.x = np.concatenate([x8, guard((1,) + x8.shape[1:], GUARD_GAIN)])
        elif c.op in ("audio3", "convs2d"):
            lead = 1 if c.x_view else 0
            self.x_cbt, self.x_cb0 = c.Cin // 16 + 2 * lead, lead
            self.x = guard((N + 1, self.x_cbt, c.H, c.W, 16), GUARD_GAIN * float(x.abs().max()))
            self.x[:N, lead:lead + c.Cin // 16] = K._cb(x)
        self.y_cb0 = 2 if c.view else 0
        self.y_cbt = c.Cout // 16 + (3 if c.view else 0)
        self.y_shape = (N + 1, self.y_cbt, c.Ho, c.Wo, 16)

    def empty_y(self) -> np.ndarray:
        return np.full(self.y_shape, PATTERN, np.int16)


@functools.lru_cache(maxsize=1)
def _conv7_shared():
    """The three distinct bank crops, the layer and its float64 reference / model / bound per distinct frame: one computation for all six
    conv7 cases."""
    g = torch.Generator().manual_seed(31000)
    rng = np.random.default_rng(31001)
    bgr = rng.integers(0, 256, (3, 256, 256, 3), dtype=np.uint8)
    bgr[0, :2, :128, :] = np.arange(256, dtype=np.uint8).reshape(2, 128, 1)         # every byte value is there
    w = R.f16(torch.randn(16, 6, 7, 7, generator=g) * (2.0 / (6 * 49)) ** 0.5)
    scale, shift = torch.rand(16, generator=g) + 0.5, torch.randn(16, generator=g) * 0.1
    x = torch.from_numpy(bank_operand(bgr)[..., :6].astype(np.float32)).permute(0, 3, 1, 2).contiguous()
    return (bgr, w, scale, shift) + _ref_parts(x, w, scale, shift, 1, 3, 14 * 32)


def _ref_parts(x, w, scale, shift, stride, pad, n_prod):
    with torch.no_grad():
        d = lambda t: t.double()
        sc, sf = scale.view(1, -1, 1, 1), shift.view(1, -1, 1, 1)
        ref = torch.relu(F.conv2d(d(x), d(w), stride=stride, padding=pad) * d(sc) + d(sf))
        A = F.conv2d(d(x).abs(), d(w).abs(), stride=stride, padding=pad) * d(sc).abs() + d(sf).abs()
        mod = torch.relu(F.conv2d(x, w, stride=stride, padding=pad) * sc + sf).half().float()
        return x, ref, mod, 2.0 ** -10 * ref.abs() + n_prod * 2.0 ** -23 * A + R.F16_FLOOR


class HeadReference:
    def __init__(self, hi: int):
        c = self.c = HEAD_CASES[hi]
        g = torch.Generator().manual_seed(30000 + hi)
        rn = lambda *s: torch.randn(*s, generator=g)
        frames_u8 = mel = None
        if c.op.startswith("conv7"):
            frames_u8, self.w, self.scale, self.shift, x, ref, mod, tol = _conv7_shared()
        else:
            self.w = R.f16(rn(c.Cout, c.Cin, 3, 3) * (2.0 / (9 * c.Cin)) ** 0.5)
            self.scale, self.shift = torch.rand(c.Cout, generator=g) + 0.5, rn(c.Cout) * 0.1
            if c.op == "audio0":
                mel = (rn(c.D, 80, 16) * 1.5).numpy()                              # float32, not fp16-exact
                x = torch.from_numpy(mel.astype(np.float16).astype(np.float32)).unsqueeze(1)
            else:
                x = R.f16(rn(c.D, c.Cin, c.H, c.W))
            x, ref, mod, tol = _ref_parts(x, self.w, self.scale, self.shift, (c.sh, c.sw), c.pad, c.n_prod)
        idx = list(c.frames)
        self.x, self.ref, self.mod, self.tol = x, ref[idx], mod[idx], tol[idx]      # x: the D distinct frames' operand, NCHW fp32
        self.buf = HeadBuffers(c, x, 32000 + hi, frames_u8, mel)


@functools.lru_cache(maxsize=4)
def head_reference(hi: int) -> HeadReference:
    return HeadReference(hi)


HEAD_FAULTS = {
    "maskrow": "the mask's row boundary off by one (rows >= 127 zeroed)",
    "ch67": "channels 6 and 7 of the operand non-zero, against the weights of channels 4 and 5",
    "replicate": "edge replication in place of zero padding",
    "frame_first": "audio3's frame index taken from the wave's first pixel",
    "tile2": "convs2d's second 32-pixel tile of a row skipped",
    "y_cb0": "y_cb0 off by one block",
}


def head_applies(fault: str, c: HeadCase) -> bool:
    if fault == "maskrow":
        return c.op == "conv7_bank"
    if fault == "ch67":
        return c.op.startswith("conv7")
    if fault == "replicate":
        return c.op == "audio0"
    if fault == "frame_first":
        return c.op == "audio3" and c.N >= 2
    if fault == "tile2":
        return c.op == "convs2d" and c.Wo > 32
    return True


def head_sim_device(rf: HeadReference, fault: Optional[str] = None) -> np.ndarray:
    """The op in fp32 from what the device is handed (bank bytes, mel windows, the packed or channel-blocked buffer), one rounding to fp16,
    stored frame by frame into the view's channel blocks of the pre-filled output buffer.  `fault`: one of HEAD_FAULTS."""
    c, b = rf.c, rf.buf
    N = c.N
    w = rf.w
    if c.op == "conv7_bank":
        x8 = bank_operand(b.frames_u8)
        if fault == "maskrow":
            x8[:, 127, :, 0:3] = 0
        x = torch.from_numpy(x8.astype(np.float32)).permute(0, 3, 1, 2)
    elif c.op == "conv7_packed":
        x = torch.from_numpy(b.x[:N].astype(np.float32)).permute(0, 3, 1, 2)
    elif c.op == "audio0":
        x = torch.from_numpy(b.mel.astype(np.float16).astype(np.float32)).unsqueeze(1)
    else:
        x = K._nchw(b.x[:N, b.x_cb0:b.x_cb0 + c.Cin // 16])
    if c.op.startswith("conv7"):
        w = F.pad(w, (0, 0, 0, 0, 0, 2))                # the packed weight's channels 6, 7: zero
        if fault == "ch67":
            x = x.clone()
            x[:, 6:8] = x[:, 3:5]
            w[:, 6:8] = w[:, 4:6]
    with torch.no_grad():
        if fault == "replicate":
            acc = F.conv2d(F.pad(x, (1, 1, 1, 1), mode="replicate"), w)
        else:
            acc = F.conv2d(x.contiguous(), w, stride=(c.sh, c.sw), padding=c.pad)
        out = K._cb(torch.relu(acc * rf.scale.view(1, -1, 1, 1) + rf.shift.view(1, -1, 1, 1)))
    if c.op in ("conv7_bank", "audio0"):                 # computed per distinct frame; frame i of the launch reads table entry i
        out = out[list(c.frames)]
    y = b.empty_y().view(np.float16)
    yb = y.reshape((N + 1) * b.y_cbt, c.Ho, c.Wo, 16)
    first = b.y_cb0 + (1 if fault == "y_cb0" else 0)
    P = c.Ho * c.Wo
    for n in range(N):
        for k in range(c.Cout // 16):
            at = n * b.y_cbt + first + k
            if at >= yb.shape[0]:
                continue
            blk = out[n, k].copy()
            if fault == "tile2":
                blk[:, 32:64] = PATTERN_F16
            if fault == "frame_first":      # pixels whose wave began in the frame before go to that frame's index: not stored here
                flat = blk.reshape(P, 16)
                gp = n * P + np.arange(P)
                flat[(gp // 32 * 32) // P != n] = PATTERN_F16
            yb[at] = blk
    return y.view(np.int16).reshape(b.y_shape)
