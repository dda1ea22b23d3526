"""CPU: what keeps tests/test_attention_gpu.py honest.  For every case and input family of its list (tests/attention_cases.py) the
rounding model of oracle/op_replay.attention_model sits inside half its bound, so the device has the other half; the bound's
subnormal-probability term is needed; and a simulated device that computes the op as the kernels do passes every gate, while each
of nine planted faults, alone, fails one on a named case of the list."""
from __future__ import annotations

import functools

import pytest
import torch

import attention_cases as A
from oracle import op_replay as R

BY_ID = {c.id: c for c in A.CASES}


@functools.lru_cache(maxsize=None)
def _reference(case_id: str, family: str) -> A.Reference:
    return A.Reference(BY_ID[case_id], family)


def test_the_list_is_what_the_kernels_need():
    """Every kernel instantiation meets every family at a ragged and at a whole shape; ids are unique."""
    assert len(BY_ID) == len(A.CASES)
    seen = {}
    for c, f in A.PLAN:
        seen.setdefault((c.kernel, c.ragged), set()).add(f)
        if c.impl == 2:                     # the LDS cases run the per-wave kernel on the same inputs
            seen.setdefault((A.Case(c.heads, c.d, c.Tq, c.Tk, c.N, 1).kernel, False), set()).add(f)
    kernels = {c.kernel for c in A.CASES}
    assert len(kernels) == 7
    for kern in kernels:
        for ragged in (False, True):
            assert seen.get((kern, ragged)) == set(A.FAMILIES), (kern, ragged, seen.get((kern, ragged)))


@pytest.mark.parametrize("case", A.CASES, ids=lambda c: c.id)
def test_model_headroom_and_clean_device(case):
    """max |mod - ref| / tol <= MODEL_HEADROOM for each of the case's families, and the simulated device (fp32 online softmax over
    32-key tiles, p -> fp16, l in fp32) passes the per-element gate, the aggregate gate and the layout checks."""
    for c, family in A.PLAN:
        if c is not case:
            continue
        rf = _reference(c.id, family)
        over = float(((rf.mod.double() - rf.ref).abs() / rf.tol.double()).max())
        assert over <= R.MODEL_HEADROOM, f"{c.id} {family}: the rounding model is at {over:.2f} of the bound"
        rec, bad = A.check(rf, A.sim_device(rf))
        assert not bad, "\n".join(bad)
        assert rec["mod_over_tol"] == pytest.approx(over)


def test_subnormal_term_is_needed():
    """The "dominant key, heavy tail" family under the bound as the replays use it (2^-10 |ref| + 2^-10 softmax(S) |V| + 2^-24): the
    rounding model itself is outside it wherever the dominant key has a tail (Tk > 1), by a factor of 2 to 200 - the tail's
    probabilities round to fp16 subnormals or to zero, 2^-25 absolute each, times |V| ~ 1e3, against a result of 1e-3."""
    n = 0
    for c, family in A.PLAN:
        if family != "dominant" or c.Tk == 1:
            continue
        rf = _reference(c.id, family)
        without = rf.model_without_subnormal_term()
        assert without > 1.0, f"{c.id}: the model is inside the bound without the term ({without:.2f})"
        assert float(((rf.mod.double() - rf.ref).abs() / rf.tol.double()).max()) <= R.MODEL_HEADROOM
        n += 1
    assert n >= 14                          # two shapes and more of each of the seven instantiations


# fault -> the (case, family) of the GPU list on which it has to fail a gate
CAUGHT_ON = {
    "a": ("d64-h2-q33-k33-n1-impl1", "gauss"),               # one key in the second tile: key 33 is its second row
    "b": ("d64-h2-q33-k33-n1-impl1", "gauss"),
    "c": ("d64-h2-q40-k50-n1-impl1", "gauss"),               # 14 padded keys: K's own next blocks and, for the last, the guard
    "d": ("d64-h2-q127-k127-n3-impl1", "ascending"),         # the maximum moves at each of the four tiles
    "e": ("d64-h2-q127-k127-n3-impl1", "ascending"),
    "f": ("d64-h2-q33-k33-n1-impl1", "gauss"),
    "g": ("d40-h8-q16-k16-n1-impl1", "gauss"),
    "h": ("d64-h2-q33-k33-n1-impl1", "gauss"),               # 31 rows past Tq: the next block's first rows and, behind the last, the pattern
    "i": ("d160-h2-q16-k50-n1-impl1", "gauss"),
}


def test_every_fault_has_a_case():
    assert sorted(CAUGHT_ON) == sorted(A.FAULTS)
    plan = {(c.id, f) for c, f in A.PLAN}
    assert all(v in plan for v in CAUGHT_ON.values())


@pytest.mark.parametrize("fault", sorted(A.FAULTS))
def test_planted_fault_is_caught(fault):
    rf = _reference(*CAUGHT_ON[fault])
    _, clean = A.check(rf, A.sim_device(rf))
    assert not clean
    rec, bad = A.check(rf, A.sim_device(rf, fault))
    print(f"fault {fault} ({A.FAULTS[fault]}) on {rf.c.id} {rf.family}: max |dev - ref| / tol {rec['dev_over_tol']:.3g}; " + " | ".join(bad))
    assert bad, f"fault {fault} ({A.FAULTS[fault]}) passes every gate on {rf.c.id} {rf.family}"


def test_replay_attention_model_is_the_helper():
    """The replay's attention branch through the helper gives what it gave before the helper existed (the model and the bound as the
    replay stated them inline), with the subnormal term off."""
    g = torch.Generator().manual_seed(3)
    q, k, v = (R.f16(torch.randn(2, 8, 50, 40, generator=g)) for _ in range(3))
    S = (q @ k.transpose(-1, -2)) * (40 ** -0.5)
    pr = torch.exp(S - S.amax(-1, keepdim=True))
    l = pr.sum(-1, keepdim=True)
    ref, mod, tol = R.attention_model(q, k, v, scale=40 ** -0.5)
    assert torch.equal(mod, R.f16((R.f16(pr) @ v) / l))
    assert torch.equal(tol, R.C_ACT * (pr @ v.abs()) / l + 2.0 ** -10 * ref.abs().float())
    rp = R.Replay({}, None)
    mod2, tol2, _ = rp.model("x.attn", dict(kind="attn", q=q, k=k, v=v, hw=None), ref.transpose(1, 2).reshape(2, 50, 320, 1).permute(0, 2, 1, 3))
    assert torch.equal(mod2[..., 0].permute(0, 2, 1).reshape(2, 50, 8, 40).transpose(1, 2), mod)
