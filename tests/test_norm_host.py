"""CPU: what tests/test_norm_gpu.py relies on, checked without a GPU (tests/norm_cases.py).

  * every case names a kernel ltk_groupnorm_f16_ex can report or a pointwise kernel; the GroupNorm cases claim all ten instantiations and
    reach the edges the launch rules have (the <8,256> / <8,1024> / <16,1024> switch and the 16384 limit of gn_group, 1 .. 256 segments,
    2 .. 32 members); the refusal list agrees with gn_group_fits / gn_coop_members restated in Python;
  * the rounding model (torch float32, one rounding) AND the simulated device (shifted fp32 sums in a kernel's order) sit inside the bound
    with op_replay's headroom at every (case, family): max |. - ref| / tol <= 0.5; for an e4m3 output both lie inside the byte bounds;
  * the simulated device passes both gates and the pattern check everywhere, and fails one under every planted fault wherever the fault
    applies; the un-shifted variance formula, which the GroupNorm kernels had, fails the `offset256` family."""
from __future__ import annotations

import pytest
import torch

import norm_cases as K
from oracle import op_replay as R

GROUPS = K.groups()


def test_cases_claim_every_kernel_and_edge():
    gn = [c for c in K.CASES if c.kind == "gn"]
    assert {c.expect for c in gn} == set(K.GN_KERNELS) and len(K.GN_KERNELS) == 10
    assert {c.expect for c in K.CASES if c.kind != "gn"} == set(K.POINTWISE_KERNELS)
    ids = [c.id for c in K.CASES]
    assert len(ids) == len(set(ids))
    for c in gn:
        assert (c.impl == 1) or (c.impl == 2 and K.gn_group_fits(c.C, c.P, c.groups)) or (c.impl == 3 and K.gn_coop_members(c.C, c.P, c.groups)), c.id
        assert not c.fp8 or c.C % 32 == 0, c.id
    two = [c for c in gn if c.impl == 1]
    assert {c.segs for c in two} >= {1, 2, 4, 8, 256}
    assert any(c.segs == 256 and c.P % c.segs for c in two)
    assert {c.cpg for c in two} >= {1, 3, 10, 16, 40, 48}
    grp = [c for c in gn if c.impl == 2]
    assert {c.cpg for c in grp} == {2, 4, 10, 16, 20, 40, 80, 128}
    assert {K.gn_group_log2L(c.cpg) for c in grp} == {0, 1, 3, 4, 5, 6}
    for cpg in (2, 10, 128):
        works = {c.P << K.gn_group_log2L(cpg) for c in grp if c.cpg == cpg}
        l = 1 << K.gn_group_log2L(cpg)
        assert works >= {2048, 2048 + l, 8192, 8192 + l, 16384, l, 3 * l}, cpg
        for fp8 in (False, True):
            assert {c.expect for c in grp if c.cpg == cpg and c.fp8 == fp8} == {f"gn_group_kernel<{k},{fp8 and 'true' or 'false'}>" for k in ("8,256", "8,1024", "16,1024")}
    coop = [c for c in gn if c.impl == 3 and not c.fp8 and not c.view]
    assert {(c.cpg, c.members, c.CB, c.N) for c in coop} == {(a, b, d, e) for a in (4, 8, 16) for b in (2, 3, 5, 32) for d in (1, 3) for e in (1, 2)}
    for k in K.GN_KERNELS:                                   # SiLU on and off, both eps, per kernel
        mine = [c for c in gn if c.expect == k]
        assert {c.silu for c in mine} == {False, True} and {c.eps for c in mine} == {1e-5, 1e-6}, k
    assert {c.expect for c in gn if c.view} >= {K.GN_KERNELS[0], K.GN_KERNELS[1], K.GN_KERNELS[8], K.GN_KERNELS[9]} | {k for k in K.GN_KERNELS if "gn_group" in k}
    ln = [c for c in K.CASES if c.kind == "ln" and not c.view]
    assert {(c.C, c.P, c.N) for c in ln} == {(a, b, d) for a in (16, 48, 320, 1280) for b in (1, 15, 16, 17, 50) for d in (1, 3)}
    for kind in ("geglu", "gelu", "silu", "add_pos"):
        totals = {2 * c.N * c.CB * c.P for c in K.CASES if c.kind == kind}
        assert {t % 256 for t in totals} >= {0, 252, 254, 2, 4} and any(c.P == 1 for c in K.CASES if c.kind == kind), kind
        assert any(c.view for c in K.CASES if c.kind == kind)
    assert any(c.kind == "add_pos" and c.C == 24 for c in K.CASES)
    for kind in ("nchw", "tokens", "tokens_add"):
        assert {(c.C, c.P) for c in K.CASES if c.kind == kind} == {(a, b) for a in (4, 8, 24, 384) for b in (1, 50, 1024)}
        assert any(c.view for c in K.CASES if c.kind == kind)
    assert max(c.elems for c in K.CASES) * 2 <= 13 << 20      # the largest: 32 members x 3 channel blocks x 2 images, 12.6 MB; all others <= 8 MB
    assert sum(1 for c in K.CASES if c.elems * 2 > 8 << 20) == 3
    for cls in K.CLASSES:
        assert any(c.cls == cls for c in K.CASES), cls


def test_every_family_meets_every_normalisation_kernel():
    met = {}
    for ci, fam in K.PLAN:
        c = K.CASES[ci]
        if c.kind in K.NORM_KINDS:
            met.setdefault(c.expect, set()).add(fam)
    for k, fams in met.items():
        assert fams == set(K.GN_FAMILIES), (k, sorted(set(K.GN_FAMILIES) - fams))


def test_refusals_match_the_launch_rules():
    for r in K.REFUSALS:
        assert K.refusal_is_right(r), r[-1]
    # and the edges on the serving side
    assert K.gn_group_fits(32, 16384, 16) and K.gn_group_fits(160, 2048, 16) and K.gn_group_fits(128, 256, 1)
    assert K.gn_coop_members(32, 4096, 4) == 2 and K.gn_coop_members(16, 65536, 4) == 32
    assert K.gn_segments(1, 16, 131075) == 256 and K.gn_segments(2, 32, 1023) == 1 and K.gn_segments(2, 32, 1024) == 2
    assert K.gn_group_variant(32, 2048, 16) == (8, 256) and K.gn_group_variant(32, 2049, 16) == (8, 1024) and K.gn_group_variant(32, 8193, 16) == (16, 1024)


@pytest.mark.parametrize("group", sorted(GROUPS), ids=sorted(GROUPS))
def test_model_headroom_and_planted_faults(group):
    bad = []
    for pi in GROUPS[group]:
        rf = K.reference(pi)
        c = rf.c
        name = f"{c.id} {rf.family}"
        rec, fails = K.check(rf, K.sim_device(rf), "sim")
        bad += [f"simulated device: {f}" for f in fails]
        if c.fp8:
            mod = rf.mod
            if not bool(((torch.from_numpy(rf.lo8) <= mod) & (mod <= torch.from_numpy(rf.hi8))).all()):
                bad.append(f"{name}: the rounding model leaves the e4m3 byte bounds")
        else:
            if rec["mod_violators"] or rec["mod_over_tol"] > R.MODEL_HEADROOM:
                bad.append(f"{name}: the rounding model: max |mod - ref| / tol = {rec['mod_over_tol']:.3f}, {rec['mod_violators']} violators")
            if rec["dev_over_tol"] > R.MODEL_HEADROOM:
                bad.append(f"{name}: the simulated device (shifted sums): max |sim - ref| / tol = {rec['dev_over_tol']:.3f}")
        for f in K.FAULTS:
            if K.applies(f, rf) and not K.check(rf, K.sim_device(rf, f), f)[1]:
                bad.append(f"{name}: fault '{K.FAULTS[f]}' passes every gate")
    assert not bad, "\n".join(bad)


def test_every_fault_applies_somewhere():
    n = {f: 0 for f in K.FAULTS}
    for pi in range(len(K.PLAN)):
        ci, fam = K.PLAN[pi]
        c = K.CASES[ci]
        if c.elems >= K.BIG:
            continue
        rf = type("RF", (), dict(c=c, family=fam, buf=type("B", (), dict(x=None if c.kind in ("add_pos", "nchw", "tokens", "tokens_add") else 1))))
        for f in K.FAULTS:
            n[f] += K.applies(f, rf)
    assert all(v >= 3 for v in n.values()), n


def test_unshifted_variance_fails_offset256_and_shifted_holds():
    """Today's GroupNorm formula before this suite: Q / cnt - mean^2 from un-shifted fp32 sums.  On `offset256` it has to leave the bound for
    every implementation's summation structure; the shifted sums stay inside 0.5 of it."""
    seen = set()
    for pi, (ci, fam) in enumerate(K.PLAN):
        c = K.CASES[ci]
        if c.kind != "gn" or fam != "offset256" or c.fp8 or c.set_size < 1024 or c.elems >= K.BIG:
            continue
        rf = K.reference(pi)
        assert K.check(rf, K.sim_device(rf, "unshifted"), "unshifted")[1], c.id
        assert K.check(rf, K.sim_device(rf), "sim")[0]["dev_over_tol"] <= R.MODEL_HEADROOM, c.id
        seen.add(c.impl)
    assert seen == {1, 2, 3}


def test_first_sample_shift_fails_outlier0_and_the_median_holds():
    """A shift by the set's first element alone: with a 3e4 outlier there, (mean - k) / std = sqrt(n) and the variance cancels worse than
    un-shifted.  It has to leave a gate for every implementation's summation structure; the median of three samples stays inside 0.5."""
    seen = set()
    for pi, (ci, fam) in enumerate(K.PLAN):
        c = K.CASES[ci]
        if c.kind != "gn" or fam != "outlier0" or c.fp8 or c.set_size < 24576 or c.elems >= K.BIG:
            continue
        rf = K.reference(pi)
        assert K.check(rf, K.sim_device(rf, "first_sample"), "first_sample")[1], c.id
        assert K.check(rf, K.sim_device(rf), "sim")[0]["dev_over_tol"] <= R.MODEL_HEADROOM, c.id
        seen.add(c.impl)
    assert seen == {1, 2, 3}


def test_vae_post_case():
    x, want = K.vae_post_case(300)
    assert want.shape == (2, 300, 3) and want.min() == 0 and want.max() == 255 and 300 % 256
