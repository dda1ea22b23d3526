"""CPU: what tests/test_conv3_gpu.py relies on, checked without a GPU (tests/conv_cases.py).

  * the cases claim every fp16 instantiation conv3's pickers can return (ltk_debug_conv3_variants, the pickers' own table) and none
    that is not there; every conv3 case's tile fits the staging budget as conv3_launch lays it out;
  * the rounding model sits inside the bound with op_replay's headroom at every case: max |mod - ref| / tol <= 0.5 - only then does a
    device inside the bound mean anything;
  * the library's own planners (conv_route and conv3_plan_launch, through the host-only hook ltk_debug_conv_plan) report for every case the
    instantiation, split, item count and grid the case expects, and refuse what tests/test_conv3_gpu.py sees refused before a launch;
  * the simulated device passes both gates and the pattern check at every case, and fails one of them under every planted fault at every
    case the fault applies to.

The same, in the test_fp8_* functions, for the fp8 family of tests/conv_fp8_cases.py (what tests/test_conv3_fp8_gpu.py relies on): the 12
instantiations of ltk_debug_conv3_fp8_variants, the planners through ltk_debug_conv_fp8_plan, exact e4m3 operands, the simulated device on
the byte buffers with the faults an fp8 operand path adds (`wscale`, `bytepair`, `mxhalf`), and the tile rule under knob CONV3_NC8 = 4."""
from __future__ import annotations

import pytest

import conv_cases as K
from oracle import op_replay as R

GROUPS = K.groups()


def test_cases_claim_every_conv3_instantiation_and_no_other():
    from livetalking_amd.engine import Engine
    listed = Engine.conv3_variants()
    assert len(listed) == len(set(listed)) == 22
    claimed = {c.expect for c in K.CASES if c.family == 0}
    assert claimed == set(listed), f"not claimed: {sorted(set(listed) - claimed)}; not listed: {sorted(claimed - set(listed))}"
    assert {c.expect for c in K.CASES if c.family} == set(K.ROW_KERNELS)
    # the finish kernel's own activation: every (T, S, G) split with each of ReLU, GELU, SiLU behind a residual
    for act in (1, 2, 3):
        assert {(c.T, c.S, c.G) for c in K.CASES if c.ksplit > 1 and c.act == act and c.res} == {(9, 1, 1), (1, 1, 1), (9, 2, 1), (9, 1, 4), (16, 1, 4)}
    assert {c.PXW for c in K.CASES if c.ups == 1 and c.view} == {1, 2, 4}
    ids = [c.id for c in K.CASES]
    assert len(ids) == len(set(ids))


def test_case_geometry():
    for c in K.CASES:
        g = K.geometry(c)
        assert g["fit"], c.id
        # about 0.5 GMAC per case (the float64 reference dominates).  One case is over: rowconv_kernel<4,4> is picked from
        # rows x J > 2^18 on, which at the 256 input channels the row layers have is 0.61 GMAC (65 x 4 x 4 rows to 256 channels)
        assert c.macs <= (0.62e9 if c.expect == K.ROW_KERNELS[3] else 0.5e9), (c.id, c.macs)
        assert c.Cin % (8 * c.NC8) == 0, c.id
        if c.fks > 1:
            assert c.nchunks == 7 and c.ksplit == {2: 2, 3: 3, 5: 4, 7: 7}[c.fks], c.id
    persistent = [c for c in K.CASES if K.geometry(c)["items"] > 512]
    assert persistent and persistent[0].expect == K.vname(1, 1, 1, 2, 9)
    assert any(K.geometry(c)["NB"] > 1 and c.N % K.geometry(c)["NB"] for c in K.CASES if c.family == 0)      # a short last tile
    assert {K.geometry(c)["l2w"] for c in K.CASES if c.family == 0} >= {0, 3, 4, 5}
    for cls in K.CLASSES:
        assert any(c.cls == cls for c in K.CASES), cls
    for f in K.FAULTS:
        assert sum(K.applies(f, c) for c in K.CASES) >= 4, f


@pytest.mark.parametrize("group", sorted(GROUPS), ids=sorted(GROUPS))
def test_model_headroom_and_planted_faults(group):
    bad = []
    for ci in GROUPS[group]:
        rf = K.reference(ci)
        c = rf.c
        rec, fails = K.check(rf, K.sim_device(rf), "sim")
        bad += [f"simulated device: {f}" for f in fails]
        if rec["mod_violators"] or rec["mod_over_tol"] > R.MODEL_HEADROOM:
            bad.append(f"{c.id}: the rounding model: max |mod - ref| / tol = {rec['mod_over_tol']:.3f}, {rec['mod_violators']} violators")
        for f in K.FAULTS:
            if K.applies(f, c) and not K.check(rf, K.sim_device(rf, f), f)[1]:
                bad.append(f"{c.id}: fault '{K.FAULTS[f]}' passes every gate")
    assert not bad, "\n".join(bad)


class _Views:
    """The channel views of conv_cases.Buffers (a guard block on either side of x and res, two in front of y and one behind) without the tensors."""

    def __init__(self, c):
        g = 1 if c.view else 0
        self.x_cbt, self.x_cb0 = c.Cin // 16 + 2 * g, g
        self.r_cbt, self.r_cb0 = (c.Cout // 16 + 2 * g, g) if c.res else (c.Cout // 16, 0)
        self.y_cbt, self.y_cb0 = c.Cout // 16 + 3 * g, 2 * g


def test_planner_reports_what_every_case_expects():
    """ltk_debug_conv_plan against the case table: what test_conv3_gpu._one demands of the device report, demanded of the planners."""
    from livetalking_amd.engine import Engine
    bad = []
    for c in K.CASES:
        try:
            if c.nc8:
                Engine.set_knob("CONV3_NC8", c.nc8)         # read when the plan is built
            rep = Engine.conv_plan(c.N, c.H, c.W, c.Cin, c.Cout, c.k, c.stride, c.pad, c.transposed, c.out_pad, c.res, **c.opts(_Views(c)))
        finally:
            if c.nc8:
                Engine.set_knob("CONV3_NC8", 0)
        if rep["kernel"] != c.expect:
            bad.append(f"{c.id}: planned {rep['kernel']!r}, the case expects {c.expect!r}")
        if rep["family"] != c.family:
            bad.append(f"{c.id}: family {rep['family']}")
        if c.family == 0:
            g = K.geometry(c)
            if (rep["ksplit"], rep["items"], rep["grid"]) != (c.ksplit, g["items"], g["grid"]):
                bad.append(f"{c.id}: reported ksplit {rep['ksplit']}, {rep['items']} items on {rep['grid']} blocks; expected {c.ksplit}, {g['items']} on {g['grid']}")
            if (rep["G"], rep["NBT"], rep["PXW"], rep["NC8"], rep["T"], rep["S"]) != (c.G, c.NBT, c.PXW, c.NC8, c.T, c.S):
                bad.append(f"{c.id}: the report's template arguments do not spell {c.expect}")
        elif f"<{rep['FT']}" not in rep["kernel"] or (c.family > 1 and f",{rep['UB']}>" not in rep["kernel"]):
            bad.append(f"{c.id}: the report's FT {rep['FT']} / UB {rep['UB']} do not spell {rep['kernel']}")
    assert not bad, "\n".join(bad)


def test_planner_refuses_what_it_cannot_serve():
    """The refusals of test_conv3_gpu.test_conv3_refuses_what_it_cannot_serve that are made before anything is enqueued, same arguments, same
    text, without a GPU.  ("rowconv: more rows" and rowgemm's 33 frames are refused by the launchers: GPU only.)"""
    from livetalking_amd._lib import LtkError
    from livetalking_amd.engine import Engine

    def refused(match, N=2, H=9, W=16, Cin=32, Cout=32, k=3, stride=1, pad=1, transposed=False, out_pad=0, **o):
        with pytest.raises(LtkError, match=match) as ex:
            Engine.conv_plan(N, H, W, Cin, Cout, k, stride, pad, transposed, out_pad, **o)
        assert ex.value.code == -1, (match, o)

    try:
        Engine.set_knob("CONV3_NC8", 4)
        refused("no kernel instantiation", force_pxw=4, force_nbt=1)                    # 512-pixel tiles: 16-channel chunks only
    finally:
        Engine.set_knob("CONV3_NC8", 0)
    refused("no kernel instantiation", force_pxw=2, force_nbt=2)                        # 64-cout blocks of a 32-cout layer
    refused("no kernel instantiation", Cout=128, force_pxw=2, force_nbt=4)              # 128-cout blocks: 1x1 only
    refused("no kernel instantiation", k=1, pad=0, force_pxw=1, force_nbt=1)            # 128-pixel tiles: 3x3 only
    refused("no kernel instantiation", Cin=64, stride=2, force_pxw=1, force_nbt=1)
    refused("no kernel instantiation", Cin=64, stride=2, transposed=True, out_pad=1, force_pxw=2, force_nbt=2)
    refused("patch does not fit the staging budget", N=1, H=256, W=1, force_pxw=2, force_nbt=1)
    refused("even H, W", ups=1)
    refused("even H, W", ups=2)
    refused("four-phase", H=10, k=1, pad=0, ups=2)
    refused("conv3 feature", H=10, Cout=64, stride=(3, 1), ups=1)                       # the first-generation kernel has no upsample read
    refused("multiples of 16", x_ld=40, x_coff=8)
    refused("outside its buffer", x_ld=32, x_coff=16)
    refused("outside its buffer", y_ld=48, y_coff=32)
    refused("bad options", act=4)
    refused("bad options", family=4)
    refused("rowgemm", N=2, H=2, W=1, Cin=512, Cout=512, k=1, pad=0, family=1)
    refused("rowconv", N=2, H=8, W=8, Cin=256, Cout=256, k=1, pad=0, family=2)
    refused("rowconvT", N=2, H=4, W=4, Cin=256, Cout=256, family=3)
    rep = Engine.conv_plan(2, 9, 16, 32, 32, 3, 1, 1, force_pxw=1, force_nbt=1, force_ksplit=1)     # and what is served is planned
    assert rep["kernel"] == K.vname(1, 1, 1, 2, 9)


# ---------------------------------------------------------------------------------------------------- the fp8 family (tests/conv_fp8_cases.py)
import conv_fp8_cases as F8  # noqa: E402

F8_GROUPS = F8.groups()


def test_fp8_cases_claim_every_fp8_instantiation_and_no_other():
    from livetalking_amd.engine import Engine
    listed = Engine.conv3_fp8_variants()
    assert len(listed) == len(set(listed)) == 12
    assert not set(listed) & set(Engine.conv3_variants())
    claimed = {c.expect for c in F8.CASES}
    assert claimed == set(listed), f"not claimed: {sorted(set(listed) - claimed)}; not listed: {sorted(claimed - set(listed))}"
    assert {c.expect for c in F8.CASES} == {F8.vname(*v) for v in F8.FV}
    # every instantiation at every map, 1, 3 and 7 chunks each; the finish kernel's own activation per Q; views per (Q, PXW)
    for v in F8.FV:
        mine = [c for c in F8.CASES if c.cls == "fp8-3x3" and c.expect == F8.vname(*v)]
        assert {(c.N, c.H, c.W) for c in mine} >= set(K.MAPS), v
        assert {c.nchunks for c in mine} == {1, 3, 7}, v
    for act in (1, 2, 3):
        assert {c.Q for c in F8.CASES if c.ksplit > 1 and c.act == act and c.res} == {1, 2}
        assert {c.Q for c in F8.CASES if c.ksplit == 1 and c.act == act} == {1, 2}
    assert {(c.Q, c.PXW) for c in F8.CASES if c.view} == {(1, 4), (1, 2), (1, 1), (2, 2), (2, 1)}
    assert {c.Q for c in F8.CASES if c.view and c.ksplit > 1} == {1, 2}
    assert {(c.Q, c.N, c.H, c.W) for c in F8.CASES if c.rng} == {(q, *m) for q in (1, 2) for m in ((2, 9, 16), (5, 6, 5))}
    ids = [c.id for c in F8.CASES]
    assert len(ids) == len(set(ids))


def test_fp8_case_geometry():
    for c in F8.CASES:
        g = F8.geometry(c)
        assert g["fit"], c.id
        assert c.macs <= 0.5e9, (c.id, c.macs)
        assert c.Cin % (16 * c.NC8) == 0 and c.nchunks == c.Cin // (16 * c.NC8), c.id
        assert c.NC8 == 4 or c.Q == 1, c.id
        if c.fks > 1:
            assert c.nchunks == 7 and c.ksplit == {2: 2, 3: 3, 5: 4, 7: 7}[c.fks], c.id
    assert {(c.Q, c.NC8) for c in F8.CASES if c.cls == "fp8-splitk"} == {(1, 2), (1, 4), (2, 4)}
    assert any(F8.geometry(c)["items"] > 512 for c in F8.CASES)                                         # the persistent walk
    assert any(F8.geometry(c)["NB"] > 1 and c.N % F8.geometry(c)["NB"] for c in F8.CASES)               # a short last tile
    for q in (1, 2):                                                                                    # 12-pixel pitch, row key, column key
        assert {F8.geometry(c)["l2w"] for c in F8.CASES if c.Q == q} >= {0, 3, 4, 5}
    for cls in F8.CLASSES:
        assert any(c.cls == cls for c in F8.CASES), cls
    for f in F8.FAULTS:
        assert sum(F8.applies(f, c) for c in F8.CASES) >= 4, f


def test_fp8_operands_are_exact():
    """What makes the fp8 cases' operands exact: the packer's own conversion (ltk_f32_to_e4m3) of w * (224 / max |w|) gives q's bytes, every
    output channel has max |q| = 224 and neighbouring channels differ in scale; x holds codes, subnormals and zeros among them, +-448 in the
    guards and in the range class, and never the NaN code."""
    import ctypes as C

    import numpy as np
    import torch
    from livetalking_amd import _lib
    lib = _lib.load()
    for ci in (0, 7, len(F8.CASES) - 1, next(i for i, c in enumerate(F8.CASES) if c.view)):
        rf = F8.reference(ci)
        c = rf.c
        w = rf.w.numpy()
        s = (np.float32(224.0) / np.abs(w).reshape(c.Cout, -1).max(1)).astype(np.float32)
        ws = np.ascontiguousarray(w * s[:, None, None, None], np.float32)
        out = np.empty(ws.size, np.uint8)
        assert lib.ltk_f32_to_e4m3(ws.ctypes.data, ws.size, out.ctypes.data) == 0
        qb = rf.q.to(torch.float8_e4m3fn).view(torch.uint8).numpy().reshape(-1)
        assert np.array_equal(out & 0x7F, qb & 0x7F) and np.array_equal((out >> 7)[(qb & 0x7F) != 0], (qb >> 7)[(qb & 0x7F) != 0]), c.id
        assert np.array_equal(rf.q.abs().reshape(c.Cout, -1).max(1).values.numpy(), np.full(c.Cout, 224.0, np.float32)), c.id
        assert np.array_equal(s, (1.0 / rf.g.numpy()).astype(np.float32)) and (rf.g[1:] != rf.g[:-1]).all(), c.id
        xb = rf.buf.x
        assert not ((xb & 0x7F) == 0x7F).any(), c.id
        data = xb[:c.N, rf.buf.x_cb0:rf.buf.x_cb0 + c.Cin // 32]
        assert np.array_equal(F8.bytes_to_codes(data).numpy(), rf.codes.numpy()), c.id
        mag = data & 0x7F
        assert ((mag > 0) & (mag < 8)).any() and (c.rng or (mag == 0).any()), c.id     # subnormals, and zeros among the ordinary codes
        assert ((xb[c.N] & 0x7F) == 0x7E).all(), c.id
        if c.rng:
            assert (mag == 0x7E).any() and float(rf.ref.abs().max()) < 2200.0, c.id
        else:
            assert float(rf.codes.abs().max()) <= 1.0, c.id
            if c.view:
                assert ((xb[:, 0] & 0x7F) == 0x7E).all() and ((xb[:, -1] & 0x7F) == 0x7E).all(), c.id


@pytest.mark.parametrize("group", sorted(F8_GROUPS), ids=sorted(F8_GROUPS))
def test_fp8_model_headroom_and_planted_faults(group):
    bad = []
    for ci in F8_GROUPS[group]:
        rf = F8.reference(ci)
        c = rf.c
        rec, fails = K.check(rf, F8.sim_device(rf), "sim")
        bad += [f"simulated device: {f}" for f in fails]
        if rec["mod_violators"] or rec["mod_over_tol"] > R.MODEL_HEADROOM:
            bad.append(f"{c.id}: the rounding model: max |mod - ref| / tol = {rec['mod_over_tol']:.3f}, {rec['mod_violators']} violators")
        for f in F8.FAULTS:
            if F8.applies(f, c) and not K.check(rf, F8.sim_device(rf, f), f)[1]:
                bad.append(f"{c.id}: fault '{F8.FAULTS[f]}' passes every gate")
    assert not bad, "\n".join(bad)


class _Fp8Views:
    """The channel views of conv_fp8_cases.Buffers without the tensors."""

    def __init__(self, c):
        g = 1 if c.view else 0
        self.x_cbt, self.x_cb0 = c.Cin // 32 + 2 * g, g
        self.r_cbt, self.r_cb0 = (c.Cout // 16 + 2 * g, g) if c.res else (c.Cout // 16, 0)
        self.y_cbt, self.y_cb0 = c.Cout // 16 + 3 * g, 2 * g


def _fp8_plan(c, **kw):
    from livetalking_amd.engine import Engine
    try:
        if c.nc8:
            Engine.set_knob("CONV3_NC8", c.nc8)         # read when the plan is built
        return Engine.conv_fp8_plan(c.N, c.H, c.W, c.Cin, c.Cout, c.Q, c.res, **c.opts(_Fp8Views(c)), **kw)
    finally:
        if c.nc8:
            Engine.set_knob("CONV3_NC8", 0)


def test_fp8_planner_reports_what_every_case_expects():
    """ltk_debug_conv_fp8_plan against the case table: what test_conv3_fp8_gpu._one demands of the device report, demanded of the planners."""
    bad = []
    for c in F8.CASES:
        rep = _fp8_plan(c)
        if rep["kernel"] != c.expect:
            bad.append(f"{c.id}: planned {rep['kernel']!r}, the case expects {c.expect!r}")
        g = F8.geometry(c)
        if (rep["family"], rep["ksplit"], rep["items"], rep["grid"]) != (0, c.ksplit, g["items"], g["grid"]):
            bad.append(f"{c.id}: reported ksplit {rep['ksplit']}, {rep['items']} items on {rep['grid']} blocks; expected {c.ksplit}, {g['items']} on {g['grid']}")
        if f"conv3_kernel<{rep['G']},{rep['NBT']},{rep['PXW']},{rep['NC8']},{rep['T']},{rep['S']},{c.Q}>" != c.expect or \
                (rep["NBT"], rep["PXW"], rep["NC8"]) != (c.NBT, c.PXW, c.NC8):
            bad.append(f"{c.id}: the report's template arguments do not spell {c.expect}")
    assert not bad, "\n".join(bad)


def test_fp8_planner_refuses_what_it_cannot_serve():
    from livetalking_amd._lib import LtkError
    from livetalking_amd.engine import Engine

    def refused(match, N=2, H=9, W=16, Cin=64, Cout=32, quant=1, nc8=0, **o):
        try:
            Engine.set_knob("CONV3_NC8", nc8)
            with pytest.raises(LtkError, match=match) as ex:
                Engine.conv_fp8_plan(N, H, W, Cin, Cout, quant, **o)
        finally:
            Engine.set_knob("CONV3_NC8", 0)
        assert ex.value.code == -1, (match, o)

    refused("Cin % 32 == 0", Cin=48)
    refused("Cin % 32 == 0", Cin=16)
    refused("Cin % 64 == 0", Cin=96, quant=2)
    for kw in (dict(k=1, pad=0), dict(stride=2), dict(pad=0), dict(k=(3, 1), pad=(1, 0)), dict(stride=2, transposed=True, out_pad=1), dict(out_pad=1)):
        refused("3x3 stride-1 pad-1", **kw)
    refused("no kernel instantiation", quant=2, force_pxw=4, force_nbt=1)               # MX: 64-channel chunks, no 512-pixel tile
    refused("no kernel instantiation", nc8=4, force_pxw=4, force_nbt=1)                 # ... nor the e4m3 kernels on 64-channel chunks
    refused("no kernel instantiation", nc8=4, force_pxw=1, force_nbt=1)                 # ... which have no 128-pixel tile either
    refused("no kernel instantiation", nc8=4, Cout=64, force_pxw=1, force_nbt=2)
    refused("no kernel instantiation", force_pxw=2, force_nbt=2)                        # 64-cout blocks of a 32-cout layer
    refused("multiples of 32", x_ld=112, x_coff=16)
    refused("outside its buffer", x_ld=64, x_coff=32)
    refused("outside its buffer", y_ld=48, y_coff=32)
    refused("multiples of 16", y_ld=56, y_coff=8)
    refused("bad options", act=4)
    refused("bad options", family=4)
    refused("bad options", ups=3)
    refused("fp8 operands", family=2)
    refused("fp8 operands", ups=1)
    refused("bad arguments", quant=3)
    # quant 0 = conv_fp8_quant: MX from 512 input channels on
    assert Engine.conv_fp8_plan(2, 9, 16, 448, 32)["kernel"].endswith(",1>")
    assert Engine.conv_fp8_plan(2, 9, 16, 512, 32)["kernel"].endswith(",2>")
    assert Engine.conv_fp8_plan(2, 9, 16, 544, 32)["kernel"].endswith(",1>")
    rep = Engine.conv_fp8_plan(2, 9, 16, 64, 32, 2, force_pxw=1, force_nbt=1, force_ksplit=1)        # and what is served is planned
    assert rep["kernel"] == F8.vname(1, 1, 4, 2)


def test_fp8_tile_rule_proposes_only_tiles_the_pickers_have():
    """k3_choose_tile walks its candidates to the smallest tile when a layer has few items; under sweep knob CONV3_NC8 = 4 the e4m3 kernels
    have no 128-pixel tile, and the rule used to settle on one ("no kernel instantiation" at launch; 2 x 32 x 32, 320 -> 320 is such a
    layer).  The unforced rule over a spread of layers, both chunk depths, e4m3 and MX: always a listed instantiation."""
    from livetalking_amd.engine import Engine
    listed = set(Engine.conv3_fp8_variants())
    shapes = [(2, 32, 32, 320, 320), (1, 8, 8, 64, 32), (1, 1, 1, 64, 64), (2, 16, 16, 128, 640), (16, 64, 64, 128, 128), (1, 256, 256, 128, 128), (3, 19, 37, 64, 96)]
    try:
        for nc8 in (0, 4):
            Engine.set_knob("CONV3_NC8", nc8)
            for quant in (1, 2):
                for N, H, W, Cin, Cout in shapes:
                    rep = Engine.conv_fp8_plan(N, H, W, Cin, Cout, quant)
                    assert rep["kernel"] in listed and rep["NC8"] == (4 if (nc8 == 4 or quant == 2) else 2), (nc8, quant, N, H, W, Cin, Cout, rep)
        Engine.set_knob("CONV3_NC8", 4)
        rep = Engine.conv_fp8_plan(2, 32, 32, 320, 320, 1)
        # the smallest tile the e4m3 kernels have at this depth: 8 tiles x 10 cout tiles, the 5 chunks split two ways
        assert (rep["kernel"], rep["ksplit"], rep["items"]) == (F8.vname(1, 2, 4, 1), 2, 160), rep
    finally:
        Engine.set_knob("CONV3_NC8", 0)


def test_fp8_default_rule_at_the_quantiser_test_shapes():
    """The tile-rule fix touches no default-knob plan: what the planner picks for the shapes of tests/test_fp8_gpu.py CASES (recorded from the
    library before the fix; the report then named only the family, so the template arguments are what is compared)."""
    from livetalking_amd.engine import Engine
    want = {   # (N, H, W, Cin, Cout, residual): (Q, NBT, PXW, NC8, ksplit, items)
        (2, 64, 64, 512, 512, True): (2, 1, 2, 4, 1, 512), (1, 256, 256, 128, 128, True): (1, 2, 2, 2, 1, 512),
        (2, 128, 128, 256, 128, False): (1, 1, 2, 2, 1, 512), (2, 32, 32, 320, 320, False): (1, 1, 1, 2, 1, 160),
        (3, 16, 16, 1280, 640, True): (2, 1, 1, 4, 3, 360), (2, 8, 8, 2560, 1280, False): (2, 1, 1, 4, 4, 160),
        (1, 37, 21, 64, 96, False): (1, 1, 1, 2, 1, 30), (5, 4, 4, 1280, 1280, True): (2, 1, 1, 4, 4, 160),
    }
    import test_fp8_gpu
    assert set(want) == {c[:6] for c in test_fp8_gpu.CASES}
    for (N, H, W, Cin, Cout, res), exp in want.items():
        rep = Engine.conv_fp8_plan(N, H, W, Cin, Cout, 0, res)
        got = (int(rep["kernel"][-2]), rep["NBT"], rep["PXW"], rep["NC8"], rep["ksplit"], rep["items"])
        assert got == exp, ((N, H, W, Cin, Cout), got)
