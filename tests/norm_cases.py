"""What tests/test_norm_host.py (CPU) and tests/test_norm_gpu.py share: the cases at which the non-matrix kernels of csrc/nn_kernels.hip
change path - the three GroupNorm implementations (gn_stats + gn_apply, gn_group_kernel, gn_coop_kernel; fp16 and e4m3 output), layernorm_kernel,
geglu_kernel, act_kernel, add_pos_kernel, nchw_to_cb16_kernel, tokens_to_cb16_kernel, vae_post_kernel -, their input families, the
channel-blocked buffers the kernels read and write, the float64 reference, the gates, a simulated device that computes the op as the kernels
do and can be told to get it wrong, and the launch rules of the GroupNorm kernels restated in Python.

A case names the implementation it forces (ltk_groupnorm_f16_ex's impl) and the instantiation, segment count, member count and grid it expects
the hook to report.

Input families of the normalisations (x is drawn in fp32 and rounded to fp16, so the device holds it exactly; a "set" is an (image, group) of
a GroupNorm or a token of a LayerNorm):
  gauss      N(0, 1)
  spread     per-channel gains U(0.5, 3.5) and offsets 2 N(0, 1), as tests/test_groupnorm_gpu.py has them
  offset16 / offset64 / offset256
             every set has mean = +-ratio x std with std 0.5 (means 8, 32, 128: well inside fp16), the sign alternating from set to set
  outlier    one value of 3e4 in a unit-variance set
  outlier0   the same with the 3e4 at the set's FIRST element (first channel, pixel 0; a token's channel 0): where a kernel that shifts its sums by one
             raw sample takes that sample
  flat       a set that is constant up to one fp16 ulp: c or c + ulp, c = 3 + the set's index / 64
gamma = U(0.5, 1.5), beta = 0.3 N(0, 1).  GEGLU and act: gates spread evenly over [-12, 12] (the negative tail is visited), a = 2 N(0, 1).

Reference: float64 of the same op on the fp16-rounded inputs.  Model (`mod`, the convention of oracle/op_replay.py): torch's float32 op, rounded
to fp16 once (to e4m3 through the loader's ltk_f32_to_e4m3 for an e4m3 output).

Per element, op_replay's own bounds (no constant is new):
  GroupNorm / LayerNorm  |dev - ref| <= 2^-10 |ref| + 2^-10 A + s + 2^-24,  A = |gamma| |x_hat| + |beta|,  s = 2^-24 ceil(log2 n) |gamma| rstd |mean|
                         with n the set's size.  (No variance term is needed: with sums of x - k, k inside the bulk of the set's values, the simulated
                         device stays inside half the bound on `offset256`, `flat` and `outlier0` too, tests/test_norm_host.py.)
  act                    the same form with A = |ref|; s = 0 for SiLU, and for GELU op_replay's own GELU term s = 2^-23 |x| (its conv1d_gelu and
                         GEGLU forms): Phi(x) = (1 + erf(x / sqrt 2)) / 2 in fp32 is off by 2^-25 absolute however small Phi is, so in the negative
                         tail, which the inputs visit, nothing relative to |ref| holds even the float32 model
  GEGLU                  2^-9 |ref| + 2^-23 |a| |g| + 2^-24
  add_pos, bridges       one rounding: 2^-10 |ref| + 2^-24; a bridge without `add` has to EQUAL f16(input); padding channels are exactly zero
  e4m3 output            no relative tolerance: the device's byte has to decode to a value between e4m3(lo) and e4m3(hi), lo / hi the ends of the
                         fp16-form bound on clamp(ref * scale, +-448), converted by ltk_f32_to_e4m3 (monotone, round-to-nearest-even, saturating)
Aggregate: rel_l2(dev, ref) <= 2 rel_l2(mod, ref) + 1e-4.

Buffers ([1 + N + 1] images of [cbt][P][16] halfs; the kernels get the address of image 1, the images in front of and behind the tensor belong
to nobody):
  x : the tensor's channel blocks at [cb0, cb0 + C / 16); every other block and both outer images hold min(GUARD_GAIN x the data's magnitude,
      6e4), finite, so a statistic that reads outside its view or past P leaves the bound.  View: x_coff 16 in x_ld C + 32.
  y : pre-filled with PATTERN; view: y_coff 32 in y_ld C + 48 (e4m3: y_coff 32 in y_ld C + 64, 32-channel blocks).  Every half (byte) outside
      the view has to hold PATTERN afterwards."""
from __future__ import annotations

import ctypes
import functools
import math
from typing import Dict, List, Optional, Tuple

import numpy as np
import torch
import torch.nn.functional as F

from oracle import op_replay as R

GUARD_GAIN = 1.0e3
GUARD_MAX = 6.0e4
PATTERN = 0x5A5A            # fp16 203.25; bytes 0x5A = e4m3 208
OUT_SCALE = 8.0             # the fp8 conv path's activation scale
GN_FAMILIES = ("gauss", "spread", "offset16", "offset64", "offset256", "outlier", "flat", "outlier0")
OFFSET_STD = 0.5
NORM_KINDS = ("gn", "ln")


# ---------------------------------------------------------------------------------------------------- launch rules (csrc/nn_kernels.hip)
def gn_segments(N: int, C: int, P: int) -> int:
    blocks, segs = N * (C // 16), 1
    while blocks * segs < 4096 and P // (segs * 2) >= 512 and segs < 256:
        segs *= 2
    return segs


def gn_group_log2L(cpg: int) -> int:
    l = 0
    while (1 << l) < cpg // 2:
        l += 1
    return l


def gn_group_fits(C: int, P: int, groups: int) -> bool:
    if groups <= 0 or C % groups:
        return False
    cpg = C // groups
    if cpg & 1 or cpg > 128:
        return False
    return (P << gn_group_log2L(cpg)) <= 16 * 1024


def gn_group_variant(C: int, P: int, groups: int) -> Tuple[int, int]:
    work = P << gn_group_log2L(C // groups)
    return (8, 256) if work <= 2048 else (8, 1024) if work <= 8192 else (16, 1024)


def gn_coop_members(C: int, P: int, groups: int) -> int:
    if groups <= 0 or C % groups:
        return 0
    cpg = C // groups
    if cpg not in (4, 8, 16) or C % 16 or P % 2048:
        return 0
    M = P // 2048
    return M if 2 <= M <= 32 else 0


def default_impl(C: int, P: int, groups: int) -> int:
    """What ltk_groupnorm_f16 resolves impl 0 to under the default knobs."""
    return 2 if gn_group_fits(C, P, groups) else 3 if gn_coop_members(C, P, groups) else 1


def _b(v: bool) -> str:
    return "true" if v else "false"


GN_KERNELS = tuple(f"gn_stats_kernel+gn_apply_kernel<{_b(f)}>" for f in (False, True)) + \
    tuple(f"gn_group_kernel<{k},{nt},{_b(f)}>" for (k, nt) in ((8, 256), (8, 1024), (16, 1024)) for f in (False, True)) + \
    tuple(f"gn_coop_kernel<{_b(f)}>" for f in (False, True))
POINTWISE_KERNELS = ("layernorm_kernel", "geglu_kernel", "act_kernel", "add_pos_kernel", "nchw_to_cb16_kernel", "tokens_to_cb16_kernel")


# ---------------------------------------------------------------------------------------------------- the cases
class Case:
    """kind: gn | ln | geglu | gelu | silu | add_pos | nchw | tokens | tokens_add.  For a GroupNorm: impl 1 / 2 / 3, fp8, silu, eps."""

    def __init__(self, cls, kind, N, C, P, groups=0, impl=0, fp8=False, silu=False, eps=1e-5, view=False):
        self.cls, self.kind, self.N, self.C, self.P, self.groups, self.impl = cls, kind, N, C, P, groups, impl
        self.fp8, self.silu, self.eps, self.view = fp8, silu, eps, view
        self.Cp = (C + 15) // 16 * 16
        self.CB = self.Cp // 16
        self.segs = self.members = self.grid = 0
        if kind == "gn":
            self.cpg = C // groups
            if impl == 1:
                self.expect = GN_KERNELS[int(fp8)]
                self.segs = gn_segments(N, C, P)
                self.grid = N * self.CB * -(-P // 1024)
            elif impl == 2:
                k, nt = gn_group_variant(C, P, groups)
                self.expect = f"gn_group_kernel<{k},{nt},{_b(fp8)}>"
                self.grid = N * groups
            else:
                self.expect = GN_KERNELS[8 + int(fp8)]
                self.members = gn_coop_members(C, P, groups)
                self.grid = N * self.CB * self.members
        else:
            self.expect = {"ln": "layernorm_kernel", "geglu": "geglu_kernel", "gelu": "act_kernel", "silu": "act_kernel", "add_pos": "add_pos_kernel",
                           "nchw": "nchw_to_cb16_kernel", "tokens": "tokens_to_cb16_kernel", "tokens_add": "tokens_to_cb16_kernel"}[kind]
        self.elems = N * self.Cp * P * (2 if kind == "geglu" else 1)

    @property
    def set_size(self) -> int:
        return self.cpg * self.P if self.kind == "gn" else self.C

    @property
    def id(self) -> str:
        s = f"{self.kind}-{self.N}x{self.C}x{self.P}"
        if self.kind == "gn":
            s += f"-g{self.groups}-impl{self.impl}" + ("-e4m3" if self.fp8 else "") + ("-silu" if self.silu else "") + f"-eps{self.eps:g}"
        elif self.kind == "ln":
            s += f"-eps{self.eps:g}"
        return s + ("-view" if self.view else "")


def _cases() -> List[Case]:
    out: List[Case] = []
    cnt: Dict[str, int] = {}

    def gn(cls, N, C, P, groups, impl, fp8=False, view=False):
        c = Case(cls, "gn", N, C, P, groups, impl, fp8, view=view)
        i = cnt.get(c.expect, 0)                 # SiLU and eps rotate per instantiation: each meets both of each
        cnt[c.expect] = i + 1
        c.silu, c.eps = bool(i & 1), 1e-6 if (i >> 1) & 1 else 1e-5
        out.append(c)

    # ---- the two-pass kernels: the 4-load main loop, the 128-stride tail, gn_apply's whole-segment path against its ragged one, 1 -> 8 segments
    for P in (1, 127, 128, 129, 511, 513, 1023, 1024, 1025, 3000, 4099):
        gn("two-pass", 2, 32, P, 2, 1)
    for P in (1, 129, 1023, 1025, 4099):
        gn("two-pass", 2, 32, P, 2, 1, fp8=True)
    gn("two-pass", 1, 16, 131075, 1, 1)                      # 256 segments of 513 pixels, the last one short
    # channels per group 1, 3, 10, 16, 40, 48: groups that straddle 16-channel blocks and groups over three blocks
    for C, groups in ((16, 16), (48, 16), (160, 16), (48, 3), (80, 2), (96, 2)):
        gn("two-pass", 2, C, 300, groups, 1)
    for C, groups in ((160, 16), (96, 2)):
        gn("two-pass", 2, C, 300, groups, 1, fp8=True)
    # ---- gn_group: L = 1 .. 64 with 5 / 10 / 20 / 40 live lanes of 8 / 16 / 32 / 64; the <8,256> / <8,1024> / <16,1024> switch and the 16384 limit
    GG = {2: (32, 16), 4: (32, 8), 10: (160, 16), 16: (32, 2), 20: (160, 8), 40: (160, 4), 80: (160, 2), 128: (128, 1)}
    for cpg in (4, 16, 20, 40, 80):
        gn("gn_group", 2, *GG[cpg][:1], 100, GG[cpg][1], 2)
    for cpg in (2, 10, 128):
        C, groups = GG[cpg]
        l2 = gn_group_log2L(cpg)
        for work in (2048, 8192, 16384):
            gn("gn_group", 2, C, work >> l2, groups, 2)
            gn("gn_group", 2, C, work >> l2, groups, 2, fp8=True)
            if work < 16384:
                gn("gn_group", 2, C, (work >> l2) + 1, groups, 2)
                gn("gn_group", 2, C, (work >> l2) + 1, groups, 2, fp8=True)
        for P in (1, 3):
            gn("gn_group", 2, C, P, groups, 2)
            gn("gn_group", 2, C, P, groups, 2, fp8=True)
    # ---- gn_coop: channels per group x members (3 and 5: no power of two) x channel blocks x images
    for cpg in (4, 8, 16):
        for M in (2, 3, 5, 32):
            for CB in (1, 3):
                for N in (1, 2):
                    gn("gn_coop", N, 16 * CB, 2048 * M, 16 * CB // cpg, 3)
    for cpg in (4, 8, 16):                                  # e4m3: whole 32-channel granules
        for M in (2, 3):
            gn("gn_coop", 2, 32, 2048 * M, 32 // cpg, 3, fp8=True)
    gn("gn_coop", 1, 32, 2048 * 32, 4, 3, fp8=True)
    # ---- one view per kernel and output type
    for fp8 in (False, True):
        gn("views", 2, 96, 1300, 2, 1, fp8=fp8, view=True)
        gn("views", 2, 160, 100, 16, 2, fp8=fp8, view=True)       # <8,256>
        gn("views", 2, 160, 300, 16, 2, fp8=fp8, view=True)       # <8,1024>
        gn("views", 2, 160, 1500, 16, 2, fp8=fp8, view=True)      # <16,1024>
        gn("views", 2, 32, 2048 * 3, 4, 3, fp8=fp8, view=True)
    # ---- LayerNorm: 16 tokens x 16 parts per block; C = 16 leaves 14 parts idle, P % 16 != 0 a ragged block
    i = 0
    for C in (16, 48, 320, 1280):
        for P in (1, 15, 16, 17, 50):
            for N in (1, 3):
                out.append(Case("ln", "ln", N, C, P, eps=1e-6 if i & 1 else 1e-5))
                i += 1
    out += [Case("views", "ln", 3, 48, 17, view=True), Case("views", "ln", 2, 320, 50, eps=1e-6, view=True)]
    # ---- GEGLU, act, add_pos: `total` = 2 N CB P just below, at and above a multiple of 256; P = 1; views; add_pos with a half-padded block
    for kind in ("geglu", "gelu", "silu", "add_pos"):
        for N, C, Ps in ((1, 32, (63, 64, 65)), (1, 16, (127, 128, 129)), (3, 32, (64,)), (2, 48, (1,))):
            out += [Case("pointwise", kind, N, C, P) for P in Ps]
        out.append(Case("views", kind, 2, 32, 65, view=True))
    out += [Case("pointwise", "add_pos", 2, 24, 50), Case("views", "add_pos", 2, 24, 50, view=True)]
    # ---- bridges
    for kind in ("nchw", "tokens", "tokens_add"):
        for C in (4, 8, 24, 384):
            for P in (1, 50, 1024):
                out.append(Case("bridges", kind, 2, C, P, view=(C == 24 and P == 50) or (C == 384 and P == 1)))
    return out


CASES = _cases()
CLASSES = ("two-pass", "gn_group", "gn_coop", "views", "ln", "pointwise", "bridges")
BIG = 1 << 20             # elements from which a case gets one family instead of two, and no planted fault

# (impl, N, C, P, groups, fp8, opts, what): shapes and views ltk_groupnorm_f16_ex has to refuse with LTK_E_INVALID
REFUSALS = (
    (2, 2, 32, 16385, 16, False, {}, "gn_group one step past 16384 thread slots (2 channels per group)"),
    (2, 2, 160, 2049, 16, False, {}, "gn_group one step past 16384 thread slots (10 channels per group)"),
    (2, 2, 128, 257, 1, True, {}, "gn_group one step past 16384 thread slots (128 channels per group)"),
    (2, 2, 48, 100, 16, False, {}, "gn_group: an odd channel count per group"),
    (3, 1, 32, 2048, 4, False, {}, "gn_coop: 1 member"),
    (3, 1, 16, 2048 * 33, 4, False, {}, "gn_coop: 33 members"),
    (3, 1, 32, 3000, 4, False, {}, "gn_coop: P % 2048 != 0"),
    (3, 1, 16, 4096, 8, False, {}, "gn_coop: 2 channels per group"),
    (3, 1, 32, 4096, 1, False, {}, "gn_coop: 32 channels per group"),
    (1, 1, 32, 100, 2, False, dict(x_ld=40, x_coff=8), "a view that is no multiple of 16 channels"),
    (1, 1, 32, 100, 2, False, dict(x_ld=32, x_coff=16), "a view outside its buffer"),
    (1, 1, 32, 100, 2, True, dict(y_ld=64, y_coff=16), "an e4m3 view that is no multiple of 32 channels"),
    (4, 1, 32, 100, 2, False, {}, "no such impl"),
)


def refusal_is_right(r) -> bool:
    """The refusal list against the launch rules restated above."""
    impl, N, C, P, groups, fp8, o, _ = r
    if impl == 2:
        return not gn_group_fits(C, P, groups)
    if impl == 3:
        return gn_coop_members(C, P, groups) == 0
    if impl < 1 or impl > 3:
        return True
    yb = 32 if fp8 else 16
    x_ld, y_ld = o.get("x_ld") or C, o.get("y_ld") or C
    xc, yc = o.get("x_coff", 0), o.get("y_coff", 0)
    return bool(x_ld % 16 or xc % 16 or y_ld % yb or yc % yb or xc + C > x_ld or yc + C > y_ld)


def _family_plan() -> List[Tuple[int, str]]:
    """(case index, family): a normalisation case gets "gauss" and one of the other six in rotation per expected kernel (a group of n cases
    hands family i mod 7 to its i-th case), so that every family meets every instantiation; a case of BIG elements or more gets the rotated
    one alone.  The other kinds have one input family."""
    seen: Dict[str, int] = {}
    plan = []
    rot = GN_FAMILIES[1:]
    for ci, c in enumerate(CASES):
        if c.kind not in NORM_KINDS:
            plan.append((ci, "data"))
            continue
        i = seen.get(c.expect, 0)
        seen[c.expect] = i + 1
        if c.elems < BIG:
            plan.append((ci, "gauss"))
        plan.append((ci, rot[i % len(rot)]))
        # `outlier0` also at a large set of the two-pass kernels and of gn_group, fp16 and e4m3, whatever the rotation hands them
        if c.kind == "gn" and not c.view and (c.impl, c.C, c.P) in ((1, 32, 4099), (2, 128, 256)) and plan[-1][1] != "outlier0":
            plan.append((ci, "outlier0"))
    return plan


PLAN = _family_plan()


def groups() -> Dict[str, List[int]]:
    """PLAN indices per test: a class, split by the expected kernel for the GroupNorm classes."""
    g: Dict[str, List[int]] = {}
    for pi, (ci, _) in enumerate(PLAN):
        c = CASES[ci]
        key = f"{c.cls}:{c.expect}" if c.cls in ("two-pass", "gn_group", "gn_coop") else f"{c.cls}:{c.kind}" if c.cls in ("pointwise", "bridges") else c.cls
        g.setdefault(key, []).append(pi)
    return g


# ---------------------------------------------------------------------------------------------------- e4m3 through the loader's converter
_E4M3_DEC = torch.arange(256, dtype=torch.uint8).view(torch.float8_e4m3fn).float().numpy()


def to_e4m3(a: np.ndarray) -> np.ndarray:
    from livetalking_amd import _lib
    a = np.ascontiguousarray(a, dtype=np.float32)
    out = np.empty(a.shape, np.uint8)
    rc = _lib.load().ltk_f32_to_e4m3(ctypes.c_void_p(a.ctypes.data), a.size, ctypes.c_void_p(out.ctypes.data))
    assert rc == 0
    return out


def from_e4m3(b: np.ndarray) -> np.ndarray:
    return _E4M3_DEC[b]


# ---------------------------------------------------------------------------------------------------- inputs
def _f16(t: torch.Tensor) -> torch.Tensor:
    return t.half().float()


def make_x(c: Case, family: str, g: torch.Generator) -> torch.Tensor:
    """-> float32 [N, C', P] holding fp16 values (C' = 2 C for a GEGLU)."""
    N, C, P = c.N, c.C, c.P
    rn = lambda *s: torch.randn(*s, generator=g)
    if c.kind in ("gelu", "silu"):
        n = N * C * P
        return _f16((torch.arange(n, dtype=torch.float32)[torch.randperm(n, generator=g)] / max(n - 1, 1) * 24 - 12).reshape(N, C, P))
    if c.kind == "geglu":
        n = N * C * P
        gate = (torch.arange(n, dtype=torch.float32)[torch.randperm(n, generator=g)] / max(n - 1, 1) * 24 - 12).reshape(N, C, P)
        return _f16(torch.cat([rn(N, C, P) * 2, gate], 1))
    if c.kind not in NORM_KINDS or family == "gauss":
        return _f16(rn(N, C, P))
    if family == "spread":
        return _f16(rn(N, C, P) * (0.5 + torch.rand(1, C, 1, generator=g) * 3.0) + rn(1, C, 1) * 2.0)
    # per set: view as [N, sets, members]
    if c.kind == "gn":
        sets, to_sets, back = c.groups, (lambda t: t.reshape(N, c.groups, c.cpg * P)), (lambda t: t.reshape(N, C, P))
    else:
        sets, to_sets, back = P, (lambda t: t.permute(0, 2, 1)), (lambda t: t.permute(0, 2, 1).contiguous())
    x = to_sets(rn(N, C, P)).clone()
    idx = torch.arange(N * sets).reshape(N, sets, 1)
    if family.startswith("offset"):
        ratio = float(family[6:])
        sign = 1.0 - 2.0 * (idx % 2)
        x = x * OFFSET_STD + sign * ratio * OFFSET_STD
    elif family == "outlier":
        pos = torch.randint(0, x.shape[-1], (N, sets, 1), generator=g)
        x.scatter_(2, pos, 3.0e4)
    elif family == "outlier0":
        x[:, :, 0] = 3.0e4
    elif family == "flat":
        base = _f16(3.0 + (idx % 48) / 64.0)                     # in [3, 3.75): one ulp is 2^-9
        x = base + (x > 0).float() * 2.0 ** -9
    return _f16(back(x))


def _cb(t: torch.Tensor) -> np.ndarray:
    """[N, C, P] -> fp16 [N, C / 16, P, 16]"""
    N, C, P = t.shape
    with np.errstate(over="ignore"):             # a planted fault may overflow fp16: inf, a violator
        return t.reshape(N, C // 16, 16, P).permute(0, 1, 3, 2).contiguous().numpy().astype(np.float16)


def _ncp(a: np.ndarray) -> torch.Tensor:
    """[N, cb, P, 16] -> float32 [N, cb * 16, P]"""
    N, cb, P, _ = a.shape
    return torch.from_numpy(a.astype(np.float32)).permute(0, 1, 3, 2).reshape(N, cb * 16, P)


class Buffers:
    """x: halfs [N + 2][x_cbt][P][16] (None for the bridges, whose input is fp32), the tensor in images [1, N + 1) at blocks [x_cb0, ..);
    y: [N + 2][y_cbt][P][yb] halfs (bytes for e4m3, yb = 32).  *_off: the element offset of image 1."""

    def __init__(self, c: Case, x: Optional[torch.Tensor], seed: int, inplace: Optional[torch.Tensor] = None):
        rng = np.random.default_rng(seed)
        N, P = c.N, c.P
        self.x = None
        self.inplace = inplace                 # add_pos works on y: the view starts out holding this tensor
        lead, tail = (1, 1) if c.view else (0, 0)
        if x is not None:
            cb = x.shape[1] // 16
            mag = min(GUARD_GAIN * max(float(x.abs().max()), 1e-3), GUARD_MAX)
            shape = (N + 2, lead + cb + tail, P, 16)
            self.x = (rng.choice([-1.0, 1.0], shape) * rng.uniform(0.5, 1.0, shape) * mag).astype(np.float16)
            self.x[1:N + 1, lead:lead + cb] = _cb(x)
            self.x_cbt, self.x_cb0, self.x_ncb = lead + cb + tail, lead, cb
            self.x_off = self.x_cbt * P * 16
        self.yb = 32 if c.fp8 else 16
        ycb = c.Cp // self.yb
        self.y_cb0 = (1 if c.fp8 else 2) if c.view else 0
        self.y_cbt = ycb + ((2 if c.fp8 else 3) if c.view else 0)
        self.y_ncb = ycb
        self.y_shape = (N + 2, self.y_cbt, P, self.yb)
        self.y_off = self.y_cbt * P * self.yb
        self.y_dtype = np.uint8 if c.fp8 else np.int16

    def empty_y(self) -> np.ndarray:
        return np.full(self.y_shape, PATTERN & (0xFF if self.y_dtype == np.uint8 else 0xFFFF), self.y_dtype)

    def initial_y(self) -> np.ndarray:
        y = self.empty_y()
        if self.inplace is not None:
            y.view(np.float16)[1:-1, self.y_cb0:self.y_cb0 + self.y_ncb] = _cb(self.inplace)
        return y

    def opts(self, c: Case) -> dict:
        if not c.view:
            return {}
        o = dict(y_ld=self.y_cbt * self.yb, y_coff=self.y_cb0 * self.yb)
        if self.x is not None:
            o.update(x_ld=self.x_cbt * 16, x_coff=self.x_cb0 * 16)
        return o


# ---------------------------------------------------------------------------------------------------- reference, model, bound
def _silu(t):
    return t * torch.sigmoid(t)


def _gelu32(t: torch.Tensor) -> torch.Tensor:
    """x Phi(x) in float32 around an erf that is correctly rounded to float32 (taken from float64), as a kernel with a 1-ulp erff forms it.
    torch's vectorised CPU erf leaves Phi off by up to 3 x 2^-24 near x = -4, more than the bound's 2^-25: no model of anything."""
    e = torch.erf(t.double() * math.sqrt(0.5)).float()
    return 0.5 * t * (1.0 + e)


def _stats64(c: Case, x: torch.Tensor):
    """mean, var of every element's set, broadcast to x's shape [N, C, P] (float64)."""
    N, C, P = x.shape
    if c.kind == "gn":
        xg = x.reshape(N, c.groups, -1)
        m, v = xg.mean(-1, keepdim=True), xg.var(-1, unbiased=False, keepdim=True)
        e = lambda t: t.expand(N, c.groups, c.cpg * P).reshape(N, C, P)
        return e(m), e(v)
    return x.mean(1, keepdim=True).expand(N, C, P), x.var(1, unbiased=False, keepdim=True).expand(N, C, P)


class Reference:
    """Inputs, buffers, float64 reference, rounding model and bound of one (case, family): computed once, read by every comparison.
    ref / mod / tol: [N, Cp, P]; for an e4m3 output in the scaled domain, clamp(. * OUT_SCALE, +-448), with lo8 / hi8 the byte bounds."""

    def __init__(self, pi: int):
        ci, family = PLAN[pi]
        c = self.c = CASES[ci]
        self.family, self.pi = family, pi
        g = torch.Generator().manual_seed(9000 + 16 * ci + (GN_FAMILIES.index(family) if family in GN_FAMILIES else 0))
        N, C, P, Cp = c.N, c.C, c.P, c.Cp
        self.gamma = self.beta = self.table = self.src = None
        d = lambda t: t.double()
        v = lambda t: t.view(1, -1, 1)
        self.exact = False
        if c.kind in NORM_KINDS:
            x = self.x = make_x(c, family, g)
            self.gamma = torch.rand(C, generator=g) + 0.5
            self.beta = torch.randn(C, generator=g) * 0.3
            mean, var = _stats64(c, d(x))
            rstd = torch.rsqrt(var + c.eps)
            xh = (d(x) - mean) * rstd
            ref = xh * v(d(self.gamma)) + v(d(self.beta))
            A = xh.abs() * v(d(self.gamma)).abs() + v(d(self.beta)).abs()
            n = c.set_size
            lg = math.ceil(math.log2(n)) if n > 1 else 0
            s = 2.0 ** -24 * lg * v(d(self.gamma)).abs() * rstd * mean.abs()
            if c.kind == "gn":
                mod = F.group_norm(x.reshape(N, C, P, 1), c.groups, self.gamma, self.beta, c.eps).reshape(N, C, P)
                if c.silu:
                    ref, mod = _silu(ref), _silu(mod)
            else:
                mod = F.layer_norm(x.permute(0, 2, 1), (C,), self.gamma, self.beta, c.eps).permute(0, 2, 1)
            self.tol = 2.0 ** -10 * ref.abs() + R.C_ACT * A + s + R.F16_FLOOR
        elif c.kind in ("gelu", "silu"):
            x = self.x = make_x(c, family, g)
            ref = F.gelu(d(x)) if c.kind == "gelu" else _silu(d(x))
            mod = _gelu32(x) if c.kind == "gelu" else _silu(x)
            self.tol = 2.0 ** -10 * ref.abs() + R.C_ACT * ref.abs() + R.F16_FLOOR
            if c.kind == "gelu":                 # s = op_replay's GELU term (its conv1d_gelu and GEGLU forms): Phi(x) in fp32 is off by 2^-25 absolute
                self.tol = self.tol + 2.0 ** -23 * d(x).abs()
        elif c.kind == "geglu":
            x = self.x = make_x(c, family, g)
            a, gt = x[:, :C], x[:, C:]
            ref = d(a) * F.gelu(d(gt))
            mod = a * _gelu32(gt)
            self.tol = 2.0 ** -9 * ref.abs() + 2.0 ** -23 * (d(a) * d(gt)).abs() + R.F16_FLOOR
        elif c.kind == "add_pos":
            x = self.x = _f16(torch.randn(N, Cp, P, generator=g))          # the padding channels hold data too: they have to stay as they are
            self.table = torch.randn(P, C, generator=g)
            ref = d(x).clone()
            ref[:, :C] += d(self.table).t()[None]
            mod = x.clone()
            mod[:, :C] += self.table.t()[None]
            self.tol = 2.0 ** -10 * ref.abs() + R.F16_FLOOR
            self.tol[:, C:] = 0.0
        else:                                                            # bridges: fp32 in
            x = None
            self.x = None
            src = torch.randn(N, C, P, generator=g) * 3.0
            if c.kind == "tokens_add":
                self.table = torch.randn(P, C, generator=g)
            self.src = src.contiguous() if c.kind == "nchw" else src.permute(0, 2, 1).contiguous()       # [N][C][P] | [N][P][C]
            ref = torch.zeros(N, Cp, P, dtype=torch.float64)
            mod = torch.zeros(N, Cp, P)
            ref[:, :C], mod[:, :C] = d(src), src
            if self.table is not None:
                ref[:, :C] += d(self.table).t()[None]
                mod[:, :C] += self.table.t()[None]
            self.tol = 2.0 ** -10 * ref.abs() + R.F16_FLOOR
            self.tol[:, C:] = 0.0
            self.exact = self.table is None
        self.buf = Buffers(c, None if c.kind == "add_pos" else self.x, 7000 + pi, inplace=self.x if c.kind == "add_pos" else None)
        if c.fp8:
            sc = OUT_SCALE
            clamp = lambda t: t.clamp(-448.0, 448.0)
            lo = np.nextafter(clamp((ref - self.tol) * sc).numpy().astype(np.float32), np.float32(-np.inf))
            hi = np.nextafter(clamp((ref + self.tol) * sc).numpy().astype(np.float32), np.float32(np.inf))
            self.lo8, self.hi8 = from_e4m3(to_e4m3(lo)), from_e4m3(to_e4m3(hi))
            self.ref = clamp(ref * sc)
            self.mod = torch.from_numpy(from_e4m3(to_e4m3(clamp(mod * sc).numpy())))
        else:
            self.ref, self.mod = ref, _f16(mod)


@functools.lru_cache(maxsize=4)
def reference(pi: int) -> Reference:
    return Reference(pi)


def view_of(rf: Reference, y: np.ndarray) -> np.ndarray:
    """The output buffer's view as float32 [N, Cp, P] (e4m3: decoded, in the scaled domain)."""
    c, b = rf.c, rf.buf
    blk = y[1:c.N + 1, b.y_cb0:b.y_cb0 + b.y_ncb]
    if c.fp8:
        N, cb, P, _ = blk.shape
        return np.ascontiguousarray(from_e4m3(blk).transpose(0, 1, 3, 2).reshape(N, cb * 32, P))
    return _ncp(blk.view(np.float16)).numpy()


def check(rf: Reference, y: np.ndarray, kernel: str = "") -> Tuple[dict, List[str]]:
    """Both gates on the view of output buffer `y` and the pattern outside it -> (op_replay's record, one line per failure)."""
    c, b = rf.c, rf.buf
    name = f"{c.id} {rf.family}"
    dev = torch.from_numpy(view_of(rf, y))
    rp = R.Replay({}, None)
    tol = rf.tol * (OUT_SCALE if c.fp8 else 1.0)
    rp.record(f"{name} {kernel}", dev, rf.ref, rf.mod, tol)
    r = rp.records[0]
    bad = []
    if c.fp8:
        inside = (torch.from_numpy(rf.lo8) <= dev) & (dev <= torch.from_numpy(rf.hi8))         # a NaN byte is outside
        r["violators"] = int((~inside).sum())
        r["elementwise"] = False
        if r["violators"]:
            bad.append(f"{name}: {r['violators']} of {r['n']} e4m3 bytes outside [e4m3(lo), e4m3(hi)]")
    else:
        r["violators"] = int((~((dev.double() - rf.ref).abs() <= tol)).sum())                   # a NaN is a violator
    bad += R.failures(rp.records)
    if not math.isfinite(r["rel_dev"]) and not bad:
        bad.append(f"{name}: rel_l2(dev, ref) is not finite")
    if rf.exact and not c.fp8:
        ne = int((dev != rf.mod).sum())
        if ne:
            bad.append(f"{name}: {ne} elements differ from f16(input)")
    if c.Cp != c.C and c.kind != "add_pos" and bool((dev[:, c.C:] != 0).any()):
        bad.append(f"{name}: padding channels are not zero")
    keep = np.ones(y.shape, bool)
    keep[1:c.N + 1, b.y_cb0:b.y_cb0 + b.y_ncb] = False
    touched = (y != b.empty_y()) & keep
    if touched.any():
        bad.append(f"{name}: {int(touched.sum())} elements outside the view were written ({int(touched[0].sum())} in front of the tensor, "
                   f"{int(touched[c.N + 1].sum())} behind it, {int(touched[1:c.N + 1].sum())} in the channel blocks around the view)")
    return r, bad


def format_record(rf: Reference, kernel: str, r: dict) -> str:
    c = rf.c
    gate = f"e4m3 bytes outside [lo, hi] {r['violators']:7d}          " if c.fp8 else f"max|dev-ref|/tol {r['dev_over_tol']:5.2f} (model {r['mod_over_tol']:4.2f})"
    return f"[norm {c.cls}] {c.id:52s} {rf.family:9s} {kernel:38s} {gate}  rel_l2 dev {r['rel_dev']:.3e} mod {r['rel_mod']:.3e}"


# ---------------------------------------------------------------------------------------------------- simulated device
FAULTS = {
    "unshifted": "var = Q / cnt - mean^2 from un-shifted fp32 sums",
    "first_sample": "GroupNorm sums shifted by the set's first element alone instead of the median of three samples",
    "count": "count taken as P instead of cpg x P",
    "group_edge": "group boundary off by one channel where groups straddle blocks",
    "last_seg": "the last partial segment left out of the statistics",
    "member": "one gn_coop member not summed",
    "eps": "eps dropped",
    "gamma_local": "gamma / beta indexed block-locally",
    "x_coff": "x_coff ignored",
    "y_coff": "y_coff ignored",
    "silu": "SiLU omitted",
    "e4m3_halves": "the two 16-byte halves of an e4m3 granule swapped",
    "ln_neighbour": "LayerNorm statistics taken from the neighbouring token",
    "ln_tail": "the tail tokens of a ragged LayerNorm block unnormalised",
}


def applies(fault: str, rf: Reference) -> bool:
    """Where a planted fault has to fail a gate.  Cases of BIG elements and more are left out (the CPU test's time)."""
    c, fam = rf.c, rf.family
    if c.elems >= BIG:
        return False
    gn, ln = c.kind == "gn", c.kind == "ln"
    if fault == "unshifted":            # (mean / std)^2 2^-24 = 4e-3 of var per rounding: sets large enough for the sums to carry roundings
        return (gn or ln) and fam == "offset256" and c.set_size >= 1024 and not c.fp8
    if fault == "first_sample":         # (mean - k) / std = sqrt(n) when k is the outlier: n 2^-24 of var per rounding
        return gn and fam == "outlier0" and c.set_size >= 24576 and not c.fp8
    if fault == "count":
        return gn and c.cpg > 1 and fam in ("gauss", "spread")
    if fault == "group_edge":           # the neighbouring channel has to differ in its statistics: per-channel or per-group offsets
        return gn and 16 % c.cpg != 0 and c.cpg % 16 != 0 and c.groups > 1 and fam in ("spread", "offset16", "offset64", "offset256")
    if fault == "last_seg":
        return gn and c.impl == 1 and c.segs > 1 and fam in ("gauss", "spread")
    if fault == "member":
        return gn and c.impl == 3 and fam in ("gauss", "spread")
    if fault == "eps":
        return (gn or ln) and fam == "flat" and c.set_size > 1
    if fault == "gamma_local":
        return (gn or ln) and c.C > 16
    if fault == "x_coff":
        return c.view and rf.buf.x is not None
    if fault == "y_coff":
        return c.view
    if fault == "silu":
        return gn and c.silu
    if fault == "e4m3_halves":
        return c.fp8
    if fault == "ln_neighbour":
        return ln and c.P > 1 and not fam.startswith("outlier")      # (a value of 3e4 gives every token the same statistics)
    if fault == "ln_tail":
        return ln and c.P % 16 != 0
    raise KeyError(fault)


def chain_tree(v: torch.Tensor) -> torch.Tensor:
    """fp32 sum over the last axis as a kernel forms it: 32 strided chains (a thread's own accumulator), then a pairwise tree (the lanes)."""
    n = v.shape[-1]
    m = -(-n // 32)
    m2 = 1 << max(0, (m - 1).bit_length())
    pad = torch.zeros(v.shape[:-1] + (32 * m2,), dtype=torch.float32)
    pad[..., :n] = v
    pad = pad.reshape(v.shape[:-1] + (m2, 32)).transpose(-1, -2)             # chain i takes elements i, i + 32, ..
    acc = torch.zeros(v.shape[:-1] + (m2,), dtype=torch.float32)
    for i in range(32):
        acc = acc + pad[..., i, :]
    while acc.shape[-1] > 1:
        h = acc.shape[-1] // 2
        acc = acc[..., :h] + acc[..., h:]
    return acc[..., 0]


def _sim_stats(c: Case, x: torch.Tensor, fault: Optional[str]):
    """-> mean, rstd broadcast to [N, C, P], float32, as the kernels form them: sums of (x - k), var = E[(x-k)^2] - E[x-k]^2, mean = k + E[x-k];
    k = a token's first channel (LayerNorm), the median of (first channel, pixel 0), (middle channel, pixel P / 2), (last channel, pixel P - 1) of
    the (image, group) (GroupNorm: gn_shift).  GroupNorm: two-pass sums per segment and channel, then over the group's channels and segments in order;
    gn_coop per member, then the members in order; gn_group over the whole set."""
    N, C, P = x.shape
    eps = 0.0 if fault == "eps" else c.eps
    if c.kind == "ln":
        xs = x.permute(0, 2, 1)                                         # [N, P, C]
        k = torch.zeros(N, P, 1) if fault == "unshifted" else xs[..., :1]
        dlt = xs - k
        S, Q = chain_tree(dlt), chain_tree(dlt * dlt)
        dm = S / C
        mean = k[..., 0] + dm
        rstd = torch.rsqrt(torch.clamp(Q / C - dm * dm, min=0.0) + eps)
        if fault == "ln_neighbour":
            mean, rstd = mean.roll(-1, 1), rstd.roll(-1, 1)
        e = lambda t: t[:, None, :].expand(N, C, P)
        return e(mean), e(rstd)
    G, cpg = c.groups, c.cpg
    xg = x
    if fault == "group_edge":                                           # every group's window starts one channel late
        xg = torch.cat([x[:, 1:], x[:, -1:]], 1)
    xg = xg.reshape(N, G, cpg, P)
    if fault == "unshifted":
        k = torch.zeros(N, G, 1, 1)
    elif fault == "first_sample":
        k = xg[:, :, :1, :1]
    else:
        k = torch.stack([xg[:, :, 0, 0], xg[:, :, cpg // 2, P // 2], xg[:, :, cpg - 1, P - 1]], -1).median(-1).values[:, :, None, None]
    dlt = xg - k
    sq = dlt * dlt
    if c.impl == 1:
        segs = c.segs
        seglen = -(-P // segs)
        S = torch.zeros(N, G)
        Q = torch.zeros(N, G)
        last = (P - 1) // seglen
        for ch in range(cpg):
            for sg in range(last + 1):
                if fault == "last_seg" and sg == last:
                    continue
                sl = slice(sg * seglen, min(P, (sg + 1) * seglen))
                S = S + chain_tree(dlt[:, :, ch, sl])
                Q = Q + chain_tree(sq[:, :, ch, sl])
    elif c.impl == 3:
        M = c.members
        S = torch.zeros(N, G)
        Q = torch.zeros(N, G)
        for m in range(M):
            if fault == "member" and m == M - 1:
                continue
            sl = slice(m * 2048, (m + 1) * 2048)
            S = S + chain_tree(dlt[..., sl].reshape(N, G, -1))
            Q = Q + chain_tree(sq[..., sl].reshape(N, G, -1))
    else:
        S, Q = chain_tree(dlt.permute(0, 1, 3, 2).reshape(N, G, -1)), chain_tree(sq.permute(0, 1, 3, 2).reshape(N, G, -1))
    cnt = float(P) if fault == "count" else float(cpg) * float(P)
    dm = S / cnt
    mean = k[:, :, 0, 0] + dm
    rstd = torch.rsqrt(torch.clamp(Q / cnt - dm * dm, min=0.0) + eps)
    e = lambda t: t[:, :, None].expand(N, G, cpg * P).reshape(N, C, P)
    return e(mean), e(rstd)


def sim_device(rf: Reference, fault: Optional[str] = None) -> np.ndarray:
    """The op as the kernels compute it, buffer to buffer, in fp32 with one rounding; `fault`: one of FAULTS."""
    c, b = rf.c, rf.buf
    N, C, P, Cp = c.N, c.C, c.P, c.Cp
    v = lambda t: t.view(1, -1, 1)
    if b.x is not None:
        cb0 = 0 if fault == "x_coff" else b.x_cb0
        x = _ncp(b.x[1:N + 1, cb0:cb0 + b.x_ncb])
    with torch.no_grad():
        if c.kind in NORM_KINDS:
            mean, rstd = _sim_stats(c, x, fault)
            gamma, beta = rf.gamma, rf.beta
            if fault == "gamma_local":
                idx = torch.arange(C) % 16
                gamma, beta = gamma[idx], beta[idx]
            if c.kind == "gn":                      # a = gamma rstd, b = beta - mean a, y = x a + b
                a = v(gamma) * rstd
                out = x * a + (v(beta) - mean * a)
                if c.silu and fault != "silu":
                    out = _silu(out)
            else:
                out = (x - mean) * rstd * v(gamma) + v(beta)
                if fault == "ln_tail" and P % 16:
                    out[:, :, P // 16 * 16:] = x[:, :, P // 16 * 16:]
        elif c.kind == "gelu":
            out = _gelu32(x)
        elif c.kind == "silu":
            out = _silu(x)
        elif c.kind == "geglu":
            out = x[:, :C] * _gelu32(x[:, C:])
        elif c.kind == "add_pos":
            out = rf.x.clone()
            out[:, :C] += rf.table.t()[None]
        else:
            src = rf.src if c.kind == "nchw" else rf.src.permute(0, 2, 1)
            out = torch.zeros(N, Cp, P)
            out[:, :C] = src
            if rf.table is not None:
                out[:, :C] += rf.table.t()[None]
    y = b.empty_y()
    first = 0 if fault == "y_coff" else b.y_cb0
    if c.fp8:
        q = to_e4m3((out * OUT_SCALE).clamp(-448.0, 448.0).numpy())                        # [N, C, P]
        q = q.reshape(N, C // 32, 32, P).transpose(0, 1, 3, 2)
        if fault == "e4m3_halves":
            q = np.concatenate([q[..., 16:], q[..., :16]], -1)
        y[1:N + 1, first:first + b.y_ncb] = q
    else:
        y.view(np.float16)[1:N + 1, first:first + b.y_ncb] = _cb(out)
    return y


# ---------------------------------------------------------------------------------------------------- vae_post
VAE_POST_P = (300, 512)          # a ragged last block of 44 pixels; whole blocks


def vae_post_case(P: int, N: int = 2):
    """-> (x halfs [N][1][P][16], the expected uint8 [N][P][3]): (x / 2 + 0.5) in fp16, clamp to [0, 1], x 255, round half even, RGB -> BGR."""
    rng = np.random.default_rng(40 + P)
    x = (rng.standard_normal((N, 1, P, 16)) * 0.8).astype(np.float16)
    t = (x[:, 0, :, :3].astype(np.float32) * np.float32(0.5) + np.float32(0.5)).astype(np.float16).astype(np.float32)
    u = np.rint(np.clip(t, 0.0, 1.0) * np.float32(255.0)).astype(np.uint8)
    return x, np.ascontiguousarray(u[:, :, ::-1])
