"""CPU: what tests/test_conv3_gpu.py relies on, checked without a GPU (tests/conv_cases.py).

  * the cases claim every fp16 instantiation conv3's pickers can return (ltk_debug_conv3_variants, the pickers' own table) and none
    that is not there; every conv3 case's tile fits the staging budget as conv3_launch lays it out;
  * the rounding model sits inside the bound with op_replay's headroom at every case: max |mod - ref| / tol <= 0.5 - only then does a
    device inside the bound mean anything;
  * the library's own planners (conv_route and conv3_plan_launch, through the host-only hook ltk_debug_conv_plan) report for every case the
    instantiation, split, item count and grid the case expects, and refuse what tests/test_conv3_gpu.py sees refused before a launch;
  * the simulated device passes both gates and the pattern check at every case, and fails one of them under every planted fault at every
    case the fault applies to."""
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
