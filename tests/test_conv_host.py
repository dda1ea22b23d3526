"""CPU: what tests/test_conv3_gpu.py relies on, checked without a GPU (tests/conv_cases.py).

  * the cases claim every fp16 instantiation conv3's pickers can return (ltk_debug_conv3_variants, the pickers' own table) and none
    that is not there; every conv3 case's tile fits the staging budget as conv3_launch lays it out;
  * the rounding model sits inside the bound with op_replay's headroom at every case: max |mod - ref| / tol <= 0.5 - only then does a
    device inside the bound mean anything;
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
