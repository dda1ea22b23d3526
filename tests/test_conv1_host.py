"""CPU: what tests/test_conv1_gpu.py and tests/test_w2l_head_gpu.py rely on, checked without a GPU (tests/conv1_cases.py).

  * the cases claim every instantiation the first-generation picker can return (ltk_debug_conv1_variants, the picker's own table) and
    none that is not there, and reach the paths they are named for: s2half under both row strides, the tile-shrink loop, several images
    per tile with a short last tile, one-pixel and one-pixel-wide patches, partial chunks, partial cout blocks at both block widths, block
    counts that are no multiple of 8;
  * the library's own planners (conv_route and conv1_plan_launch, through ltk_debug_conv_plan) report for every case the instantiation,
    tile, images per tile, s2half, blocks and LDS bytes the case table and conv1_cases.geometry expect, and refuse what they have to;
  * the planner split changed no launch: for every geometry of tests/test_conv_gpu.py CASES under both values of knob CONV_V3 the planner
    reports the kernel, grid, LDS bytes, tile and the hash of the kernel's scalar arguments that the undivided conv1_launch formed
    (PARENT, recorded from it);
  * the rounding model sits inside the bound with op_replay's headroom; the simulated devices pass both gates and the pattern check at
    every case, and fail one of them under every planted fault at every case the fault applies to;
  * the byte operand of conv7's BANK mode, fp16(fp32(b) * fp32(1 / 255)), is b / 255 to 2^-11 relative for all 256 bytes."""
from __future__ import annotations

import numpy as np
import pytest

import conv1_cases as C1
import conv_cases as K
from oracle import op_replay as R

GROUPS = C1.groups()


class _Views:
    """The channel views of conv_cases.Buffers without the tensors."""

    def __init__(self, c):
        g = 1 if c.view else 0
        self.x_cbt, self.x_cb0 = c.CinP // 16 + 2 * g, g
        self.r_cbt, self.r_cb0 = (c.Cout // 16 + 2 * g, g) if c.res else (c.Cout // 16, 0)
        self.y_cbt, self.y_cb0 = c.Cout // 16 + 3 * g, 2 * g


def _plan(v3=1, **kw):
    from livetalking_amd.engine import Engine
    a = dict(transposed=False, out_pad=0, has_res=False)
    a.update(kw)
    try:
        Engine.set_knob("CONV_V3", v3)              # read when the plan is built
        return Engine.conv_plan(a.pop("N"), a.pop("H"), a.pop("W"), a.pop("Cin"), a.pop("Cout"), a.pop("k"), a.pop("stride"), a.pop("pad"), **a)
    finally:
        Engine.set_knob("CONV_V3", 1)


def test_cases_claim_every_conv1_instantiation_and_no_other():
    from livetalking_amd.engine import Engine
    listed = Engine.conv1_variants()
    assert len(listed) == len(set(listed)) == 13
    assert set(listed) == {C1.vn(1, 1, False, 5)} | {C1.vn(4, n, t, 6) for n in (1, 2) for t in (False, True)} | \
        {C1.vn(2, n, t, m) for n in (1, 2) for t in (False, True) for m in (3, 10)}
    claimed = {c.expect for c in C1.CASES}
    assert claimed == set(listed), f"not claimed: {sorted(set(listed) - claimed)}; not listed: {sorted(claimed - set(listed))}"
    assert not set(listed) & set(Engine.conv3_variants())
    ids = [c.id for c in C1.CASES]
    assert len(ids) == len(set(ids))


def test_case_geometry_reaches_every_named_path():
    geo = {c.id: C1.geometry(c) for c in C1.CASES}
    for c in C1.CASES:
        g = geo[c.id]
        assert g["fit"] and g["NBT"] == c.NBT, c.id
        assert c.MAXA == ({1: 5, 4: 6}.get(c.NC8) or (3 if g["need"] <= 3 else 10)), c.id
        assert c.macs <= 0.5e9, (c.id, c.macs)
        if c.tile:
            assert c.tile == (g["l2w"], g["l2h"], g["NB"], g["s2half"]), c.id
        if c.NBT == 2:
            assert g["blocks"] >= C1.K_MIN_BLOCKS, c.id
    tt9s2 = [c for c in C1.CASES if c.TT9 and c.sw == 2]
    assert {geo[c.id]["l2w"] for c in tt9s2} >= {2, 4, 5} and {c.Cin for c in tt9s2} >= {16, 32, 48}
    assert all((geo[c.id]["s2half"] > 0) == (geo[c.id]["l2w"] >= 4) for c in tt9s2)
    assert any(geo[c.id]["s2half"] and c.sh == 3 for c in C1.CASES)
    assert any(geo[c.id]["shrunk"] and c.sh == 3 and c.Wo > 16 for c in C1.CASES)
    assert any(c.NC8 == 1 and geo[c.id]["NB"] > 1 and c.N % geo[c.id]["NB"] for c in C1.CASES)                # a short last tile
    assert any(geo[c.id]["PH"] * geo[c.id]["PW"] == 1 for c in C1.CASES) and any(geo[c.id]["PW"] == 1 and geo[c.id]["PH"] > 1 for c in C1.CASES)
    assert any(c.NC8 == 1 and c.taps == 49 and c.Tp == 50 for c in C1.CASES)
    assert {c.Cin for c in C1.CASES if c.NC8 == 1} >= {1, 3, 6, 8}
    assert {c.Cin for c in C1.CASES if c.NC8 == 4 and c.TT9} >= {32, 48, 96}
    assert any(c.NC8 == 4 and c.TT9 and (c.Ho, c.Wo) == (1, 1) for c in C1.CASES)
    assert {c.Cout for c in C1.CASES if c.NBT == 1 and c.Cout % 32} >= {16, 48} and any(c.NBT == 2 and c.Cout in (80, 96) for c in C1.CASES)
    assert any(geo[c.id]["blocks"] % 8 for c in C1.CASES) and any(geo[c.id]["blocks"] > 8 and geo[c.id]["blocks"] % 8 for c in C1.CASES)
    assert any(c.expand for c in C1.CASES) and {c.Cin for c in C1.CASES if c.four} >= {16, 64}
    # views once per class that computes its own offsets; ReLU, GELU, SiLU, a residual
    assert {(c.NC8, c.four) for c in C1.CASES if c.view} >= {(1, False), (2, False), (4, False), (2, True), (4, True)}
    assert {c.act for c in C1.CASES} == {0, 1, 2, 3} and any(c.res for c in C1.CASES) and any(not c.res for c in C1.CASES)
    for cls in C1.CLASSES:
        assert any(c.cls == cls for c in C1.CASES), cls
    for f in C1.FAULTS:
        assert sum(C1.applies(f, c) for c in C1.CASES) >= 3, f
    for f in C1.HEAD_FAULTS:
        assert any(C1.head_applies(f, c) for c in C1.HEAD_CASES), f
    assert {c.op for c in C1.HEAD_CASES} == set(C1.HEAD_OPS)


def test_planner_reports_what_every_case_expects():
    """ltk_debug_conv_plan against the case table: what test_conv1_gpu._one demands of the device report, demanded of the planners."""
    bad = []
    for c in C1.CASES:
        g = C1.geometry(c)
        rep = _plan(c.v3, N=c.N, H=c.H, W=c.W, Cin=c.Cin, Cout=c.Cout, k=c.k, stride=c.stride, pad=c.pad, transposed=c.transposed, out_pad=c.out_pad,
                    has_res=c.res, **c.opts(_Views(c)))
        bad += C1.report_mismatches(c, g, rep)
    assert not bad, "\n".join(bad)


def test_planner_refuses_what_the_first_generation_cannot_serve():
    from livetalking_amd._lib import LtkError
    for match, kw in C1.REFUSALS:
        with pytest.raises(LtkError, match=match) as ex:
            _plan(**kw)
        assert ex.value.code == -1, (match, kw)
    rep = _plan(N=2, H=9, W=16, Cin=6, Cout=32, k=3, stride=1, pad=1)                 # and what is served is planned
    assert rep["kernel"] == C1.vn(1, 1, False, 5)


# (CONV_V3, index into test_conv_gpu.CASES): (kernel, grid, LDS bytes, l2w, l2h, NB, s2half, phases, args_hash) of the launch conv1_launch
# formed before it was split into conv1_plan_launch and the enqueue; the geometries that are not here are conv3's under that knob value
PARENT = {
    (1, 0): ("conv_mfma_kernel<1,1,false,5>", 15, 20736, 4, 4, 1, 0, 1, 893968579),
    (1, 2): ("conv_mfma_kernel<2,1,true,10>", 12, 37120, 4, 4, 1, 0, 1, 1319823997),
    (1, 4): ("conv_mfma_kernel<2,1,true,10>", 12, 46336, 3, 4, 1, 0, 1, 450713872),
    (1, 6): ("conv_mfma_kernel<2,1,true,3>", 8, 20736, 2, 2, 3, 0, 1, 239609781),
    (1, 8): ("conv_mfma_kernel<2,1,true,3>", 16, 20736, 0, 0, 3, 0, 1, 1910996871),
    (1, 11): ("conv_mfma_kernel<1,1,false,5>", 512, 34304, 5, 3, 1, 0, 1, 2017154641),
    (1, 12): ("conv_mfma_kernel<2,1,true,10>", 128, 44800, 5, 3, 1, 33, 1, 45994010),
    (1, 14): ("conv_mfma_kernel<2,1,true,10>", 64, 44800, 5, 3, 1, 33, 1, 248251285),
    (1, 24): ("conv_mfma_kernel<2,1,false,3>", 16, 20736, 0, 0, 5, 0, 1, 1254292572),
    (0, 0): ("conv_mfma_kernel<1,1,false,5>", 15, 20736, 4, 4, 1, 0, 1, 893968579),
    (0, 1): ("conv_mfma_kernel<4,1,true,6>", 15, 39680, 4, 4, 1, 0, 1, 2026897283),
    (0, 2): ("conv_mfma_kernel<2,1,true,10>", 12, 37120, 4, 4, 1, 0, 1, 1319823997),
    (0, 3): ("conv_mfma_kernel<4,1,true,6>", 12, 39680, 4, 4, 1, 0, 1, 1000880749),
    (0, 4): ("conv_mfma_kernel<2,1,true,10>", 12, 46336, 3, 4, 1, 0, 1, 450713872),
    (0, 5): ("conv_mfma_kernel<2,1,true,3>", 8, 20992, 3, 4, 2, 0, 1, 792439903),
    (0, 6): ("conv_mfma_kernel<2,1,true,3>", 8, 20736, 2, 2, 3, 0, 1, 239609781),
    (0, 7): ("conv_mfma_kernel<2,1,true,3>", 8, 20736, 2, 2, 3, 0, 1, 687328571),
    (0, 8): ("conv_mfma_kernel<2,1,true,3>", 16, 20736, 0, 0, 3, 0, 1, 1910996871),
    (0, 9): ("conv_mfma_kernel<4,1,false,6>", 16, 20736, 0, 0, 3, 0, 1, 913154931),
    (0, 10): ("conv_mfma_kernel<4,1,false,6>", 16, 20736, 0, 0, 19, 0, 1, 598632099),
    (0, 11): ("conv_mfma_kernel<1,1,false,5>", 512, 34304, 5, 3, 1, 0, 1, 2017154641),
    (0, 12): ("conv_mfma_kernel<2,1,true,10>", 128, 44800, 5, 3, 1, 33, 1, 45994010),
    (0, 13): ("conv_mfma_kernel<4,1,true,6>", 128, 40704, 5, 3, 1, 0, 1, 1201682650),
    (0, 14): ("conv_mfma_kernel<2,1,true,10>", 64, 44800, 5, 3, 1, 33, 1, 248251285),
    (0, 15): ("conv_mfma_kernel<4,1,true,6>", 64, 40704, 5, 3, 1, 0, 1, 698268098),
    (0, 16): ("conv_mfma_kernel<2,1,true,10>", 32, 44800, 5, 3, 1, 33, 1, 1592780668),
    (0, 17): ("conv_mfma_kernel<2,1,true,3>", 32, 20736, 5, 3, 1, 0, 1, 17430553),
    (0, 18): ("conv_mfma_kernel<2,1,true,10>", 16, 44288, 4, 4, 1, 17, 1, 530918134),
    (0, 19): ("conv_mfma_kernel<2,1,true,3>", 24, 20736, 4, 4, 1, 0, 1, 373565402),
    (0, 20): ("conv_mfma_kernel<2,1,true,10>", 16, 37120, 3, 3, 3, 0, 1, 909384730),
    (0, 21): ("conv_mfma_kernel<2,1,true,3>", 16, 20736, 3, 3, 3, 0, 1, 27236673),
    (0, 22): ("conv_mfma_kernel<2,1,true,3>", 16, 20736, 2, 2, 3, 0, 1, 92425598),
    (0, 23): ("conv_mfma_kernel<2,1,true,3>", 16, 20736, 2, 2, 5, 0, 1, 101142026),
    (0, 24): ("conv_mfma_kernel<2,1,false,3>", 16, 20736, 0, 0, 5, 0, 1, 1254292572),
    (0, 25): ("conv_mfma_kernel<4,1,false,6>", 256, 20736, 0, 0, 3, 0, 1, 1175028120),
    (0, 26): ("conv_mfma_kernel<4,1,false,6>", 64, 20736, 2, 2, 3, 0, 4, 1029091134),
    (0, 27): ("conv_mfma_kernel<4,1,false,6>", 64, 24320, 3, 3, 3, 0, 4, 1567282971),
    (0, 28): ("conv_mfma_kernel<4,1,false,6>", 96, 26880, 4, 4, 1, 0, 4, 1855618470),
    (0, 29): ("conv_mfma_kernel<2,1,true,3>", 96, 20736, 5, 3, 1, 0, 1, 309118178),
    (0, 30): ("conv_mfma_kernel<4,1,false,6>", 256, 27392, 5, 3, 1, 0, 4, 1610962822),
    (0, 31): ("conv_mfma_kernel<2,1,true,3>", 256, 20736, 5, 3, 1, 0, 1, 683227329),
    (0, 32): ("conv_mfma_kernel<4,1,false,6>", 512, 27392, 5, 3, 1, 0, 4, 318303796),
    (0, 33): ("conv_mfma_kernel<4,1,false,6>", 512, 27392, 5, 3, 1, 0, 4, 642947969),
    (0, 34): ("conv_mfma_kernel<4,1,true,6>", 512, 40704, 5, 3, 1, 0, 1, 345903596),
    (0, 35): ("conv_mfma_kernel<4,1,true,6>", 256, 40704, 5, 3, 1, 0, 1, 225673461),
    (0, 36): ("conv_mfma_kernel<4,1,true,6>", 10, 40704, 5, 3, 1, 0, 1, 1333172858),
    (0, 37): ("conv_mfma_kernel<2,1,true,10>", 24, 44800, 5, 3, 1, 33, 1, 1315093997),
}


def test_planner_split_changed_no_launch_of_the_wav2lip_geometries():
    """The same call ltk_conv2d_f16 makes for test_conv_gpu.run_case (contiguous tensors, ReLU, the input as residual), planned."""
    import test_conv_gpu
    assert len(test_conv_gpu.CASES) == 38 and {i for v, i in PARENT if v == 0} == set(range(38))
    bad = []
    for v3 in (1, 0):
        for i, (N, H, W, Cin, Cout, k, stride, pad, transposed, out_pad, residual) in enumerate(test_conv_gpu.CASES):
            rep = _plan(v3, N=N, H=H, W=W, Cin=Cin, Cout=Cout, k=k, stride=stride, pad=pad, transposed=transposed, out_pad=out_pad, has_res=residual, act=1)
            first_gen = rep["kernel"].startswith("conv_mfma_kernel<")
            if first_gen != ((v3, i) in PARENT):
                bad.append(f"CONV_V3 {v3} case {i}: served by {rep['kernel']!r}")
            elif first_gen:
                got = (rep["kernel"], rep["grid"], rep["lds"], rep["l2w"], rep["l2h"], rep["NB"], rep["s2half"], rep["phases"], rep["args_hash"])
                if got != PARENT[v3, i] or rep["items"] != rep["grid"]:
                    bad.append(f"CONV_V3 {v3} case {i}: planned {got}, the undivided launch was {PARENT[v3, i]}")
    assert not bad, "\n".join(bad)


@pytest.mark.parametrize("group", sorted(GROUPS), ids=sorted(GROUPS))
def test_model_headroom_and_planted_faults(group):
    bad = []
    for ci in GROUPS[group]:
        rf = C1.reference(ci)
        c = rf.c
        rec, fails = K.check(rf, C1.sim_device(rf), "sim")
        bad += [f"simulated device: {f}" for f in fails]
        if rec["mod_violators"] or rec["mod_over_tol"] > R.MODEL_HEADROOM:
            bad.append(f"{c.id}: the rounding model: max |mod - ref| / tol = {rec['mod_over_tol']:.3f}, {rec['mod_violators']} violators")
        for f in C1.FAULTS:
            if C1.applies(f, c) and not K.check(rf, C1.sim_device(rf, f), f)[1]:
                bad.append(f"{c.id}: fault '{C1.FAULTS[f]}' passes every gate")
    assert not bad, "\n".join(bad)


def test_bank_byte_operand_is_a_faithful_255th():
    """fp16(fp32(b) * fp32(1 / 255)), the operand conv7's BANK mode and pack_faces_kernel form, against b / 255 in float64: within the
    fp16 rounding, 2^-11 relative, for every byte - the stated rounding is a division by 255 and nothing else."""
    b = np.arange(256, dtype=np.uint8)
    op = (b.astype(np.float32) * np.float32(1.0 / 255.0)).astype(np.float16).astype(np.float64)
    exact = b.astype(np.float64) / 255.0
    assert op[0] == 0.0 and op[255] == 1.0
    assert (np.abs(op - exact) <= 2.0 ** -11 * exact).all()
    x8 = C1.bank_operand(np.broadcast_to(b.reshape(1, 256, 1, 1), (1, 256, 256, 3)).copy())
    assert np.array_equal(x8[0, :, 0, 3].astype(np.float64), op) and np.array_equal(x8[0, :128, 0, 0].astype(np.float64), op[:128])
    assert not x8[0, 128:, :, 0:3].any() and not x8[..., 6:8].any()


@pytest.mark.parametrize("hi", range(len(C1.HEAD_CASES)), ids=[c.id for c in C1.HEAD_CASES])
def test_head_model_headroom_and_planted_faults(hi):
    rf = C1.head_reference(hi)
    c = rf.c
    bad = []
    rec, fails = K.check(rf, C1.head_sim_device(rf), "sim")
    bad += [f"simulated device: {f}" for f in fails]
    if rec["mod_violators"] or rec["mod_over_tol"] > R.MODEL_HEADROOM:
        bad.append(f"{c.id}: the rounding model: max |mod - ref| / tol = {rec['mod_over_tol']:.3f}, {rec['mod_violators']} violators")
    for f in C1.HEAD_FAULTS:
        if C1.head_applies(f, c) and not K.check(rf, C1.head_sim_device(rf, f), f)[1]:
            bad.append(f"{c.id}: fault '{C1.HEAD_FAULTS[f]}' passes every gate")
    assert not bad, "\n".join(bad)


def test_head_inputs_are_what_the_ops_are_defined_on():
    """Bytes over the whole range, mel windows that are no fp16 values, frame tables that permute and repeat."""
    bgr = C1._conv7_shared()[0]
    assert set(np.unique(bgr)) == set(range(256))
    rf = C1.head_reference(next(i for i, c in enumerate(C1.HEAD_CASES) if c.op == "audio0" and c.N == 3))
    mel = rf.buf.mel
    assert mel.dtype == np.float32 and (mel.astype(np.float16).astype(np.float32) != mel).mean() > 0.9
    for c in C1.HEAD_CASES:
        if c.op in ("conv7_bank", "audio0") and c.N > 1:
            assert list(c.frames) != sorted(c.frames) and (c.N < 3 or len(set(c.frames)) < c.N), c.id
    assert {c.N for c in C1.HEAD_CASES if c.op == "conv7_bank"} == {1, 2, 9} == {c.N for c in C1.HEAD_CASES if c.op == "conv7_packed"}
    assert {c.N for c in C1.HEAD_CASES if c.op == "audio3"} == {1, 2, 3}
    assert {(c.N, c.H, c.W, c.Cin, c.Cout) for c in C1.HEAD_CASES if c.op == "convs2d"} == {(3, 2, 64, 16, 32), (3, 6, 64, 16, 32), (2, 6, 128, 32, 64), (2, 4, 64, 32, 96)}
    assert {c.Cin for c in C1.HEAD_CASES if c.op == "convs2d" and c.view} == {16, 32}
