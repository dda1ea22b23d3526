"""CPU tests of the fused inverted residual (csrc/ul_ir.hip, knob UL_FUSE_IR): the check tests/test_ul_ir_gpu.py holds the device to
(tests/ul_ir_cases.py) held to itself - the float32 model inside half of every stage's bound, the fault-free simulated device through
`check`, every planted fault caught on every case its predicate names - and the pure planner (ltk_debug_ul_ir_plan, no GPU) held to
the block table of the Ultralight program."""
from __future__ import annotations

import ctypes as C
import functools

import numpy as np
import pytest

import ul_ir_cases as K
from oracle import op_replay as R


@functools.lru_cache(maxsize=None)
def _tile():
    return K.planner()


@functools.lru_cache(maxsize=None)
def _cases():
    return K.cases(*_tile())


@functools.lru_cache(maxsize=None)
def _setup(i):
    c = _cases()[i]
    inp = K.Inputs(c)
    return c, inp, K.Buffers(c, inp)


N_CASES = K.N_CASES


def test_case_count():
    assert len(_cases()) == N_CASES
    assert len({c.id for c in _cases()}) == N_CASES


def test_cases_reach_every_edge():
    TH, TW, MC = _tile()
    cs = _cases()
    for s in (1, 2):
        at = [c for c in cs if c.stride == s]
        assert any(c.Ho == TH + 1 and c.Wo == TW + 1 for c in at)
        assert any(c.Ho < TH and c.Wo < TW and (c.H, c.W) not in ((5, 7), (1, 1)) for c in at)
        assert any((c.H, c.W) == (5, 7) for c in at) and any((c.H, c.W) == (1, 1) for c in at)
    assert {(c.Cin, c.Cout) for c in cs} >= {(a, b) for a in (16, 32, 48) for b in (16, 32, 48)}
    assert any(c.mid % MC for c in cs) and any(c.mid == 2 * MC + 16 for c in cs)
    assert any(c.res and c.view for c in cs) and any(c.res and not c.view for c in cs) and any(c.view and not c.res for c in cs)
    assert any(c.N == 1 for c in cs) and any(c.big == "out" for c in cs) and any(c.big == "hid" for c in cs)
    for c in cs:
        assert not c.res or (c.Cin == c.Cout and c.stride == 1)


@pytest.mark.parametrize("i", range(N_CASES))
def test_model_and_simulated_device_pass(i):
    """The fault-free simulated device passes `check`, tapped and untapped runs leave the same y, and the float32 model sits inside
    half of every stage's bound."""
    c, inp, b = _setup(i)
    sim = K.SimDevice(c, inp, *_tile())
    y, e1, e2 = sim.run(b)
    figs = K.check(c, inp, b, y, e1, e2)
    for st, f in figs.items():
        assert f["model_worst"] <= R.MODEL_HEADROOM, f"{c.id} {st}: the model is at {f['model_worst']:.2f} of the bound"
    y2, e1u, e2u = sim.run(b, tap=False)
    assert np.array_equal(y, y2) and (e1u == K.PATTERN).all() and (e2u == K.PATTERN).all()


@pytest.mark.parametrize("fault", sorted(K.FAULTS))
def test_every_planted_fault_is_caught(fault):
    t = _tile()
    hit, missed = 0, []
    for i in range(N_CASES):
        c, inp, b = _setup(i)
        if not K.FAULTS[fault](t, c):
            continue
        hit += 1
        y, e1, e2 = K.SimDevice(c, inp, *t, fault=fault).run(b)
        try:
            K.check(c, inp, b, y, e1, e2)
        except AssertionError:
            continue
        missed.append(c.id)
    assert not missed, f"{fault} passes the check on {missed}"
    assert hit >= 2, f"{fault}: no case shows it"


# ---------------------------------------------------------------------------------------------------- the planner
# the 26 inverted residuals: (name, Cin, Cout, input map, stride, residual, must fuse)
BLOCKS = [("inc.inconv.0", 6, 32, 160, 1, False, False),
          ("down1.0", 32, 64, 160, 2, False, True), ("down1.1", 64, 64, 80, 1, True, True),
          ("down2.0", 64, 128, 80, 2, False, True), ("down2.1", 128, 128, 40, 1, True, True),
          ("down3.0", 128, 256, 40, 2, False, True), ("down3.1", 256, 256, 20, 1, True, False),
          ("down4.0", 256, 512, 20, 2, False, False), ("down4.1", 512, 512, 10, 1, True, False),
          ("audio.conv1", 16, 64, 32, 1, False, True), ("audio.conv2", 64, 128, 32, 1, False, True),
          ("audio.conv4", 256, 256, 16, 1, True, False), ("audio.conv6", 512, 512, 10, 1, True, False), ("audio.conv7", 512, 512, 10, 1, True, False),
          ("fuse_conv.0.0", 1024, 512, 10, 1, False, False), ("fuse_conv.0.1", 512, 512, 10, 1, True, False),
          ("fuse_conv.1.0", 512, 256, 10, 1, False, False), ("fuse_conv.1.1", 256, 256, 10, 1, True, False),
          ("up1.0", 512, 128, 20, 1, False, False), ("up1.1", 128, 128, 20, 1, True, False),
          ("up2.0", 256, 64, 40, 1, False, True), ("up2.1", 64, 64, 40, 1, True, True),
          ("up3.0", 128, 32, 80, 1, False, True), ("up3.1", 32, 32, 80, 1, True, True),
          ("up4.0", 64, 32, 160, 1, False, True), ("up4.1", 32, 32, 160, 1, True, True)]


def _plan(*a, **kw):
    from livetalking_amd.engine import Engine
    return Engine.ul_ir_plan(*a, **kw)


@pytest.mark.parametrize("N", [1, 16, 64, 256])
def test_planner_accepts_the_blocks_that_must_fuse(N):
    must = [b for b in BLOCKS if b[6]]
    assert len(must) == 13 and len(BLOCKS) == 26
    for name, cin, cout, hw, s, res, _ in must:
        p = _plan(N, hw, hw, cin, 2 * cin, cout, s, res)
        assert p["accepted"], f"{name} at N = {N}: {p['reason']}"
        assert p["lds_bytes"] <= p["lds_limit"] <= 160 * 1024
        TH, TW = p["tile"]
        ho = (hw - 1) // s + 1
        assert (p["Ho"], p["Wo"]) == (ho, ho)
        assert p["grid"] == (-(-ho // TW), -(-ho // TH), N) and p["blocks"] == p["grid"][0] * p["grid"][1] * N
        # the tiles cover every output pixel exactly once
        cover = np.zeros((ho, ho), int)
        for ty in range(p["grid"][1]):
            for tx in range(p["grid"][0]):
                cover[ty * TH:(ty + 1) * TH, tx * TW:(tx + 1) * TW] += 1
        assert (cover == 1).all()
        assert p["chunks"] * p["MC"] >= 2 * cin and (p["chunks"] - 1) * p["MC"] < 2 * cin
        assert p["hidden_px"] == (s * (TH - 1) + 3) * (s * (TW - 1) + 3)
        assert p["kernel"] == f"ul_ir_kernel<{cout // 16},false>" and p["threads"] == 256


def test_planner_reports_every_case():
    TH, TW, MC = _tile()
    for c in _cases():
        b = K.Buffers(c, K.Inputs(c))
        for tap in (False, True):
            p = _plan(c.N, c.H, c.W, c.Cin, c.mid, c.Cout, c.stride, c.res, tap, views=b.views() if c.view else None)
            want = c.geometry(TH, TW, MC, tap)
            assert {k: p[k] for k in want} == want, c.id


@pytest.mark.parametrize("word,args,kw", [
    ("multiples of 16", (1, 160, 160, 6, 12, 32, 1, False), {}),                      # inc.inconv.0: its expand reads the bank crop
    ("multiples of 16", (1, 8, 8, 24, 48, 16, 1, False), {}),
    ("multiples of 16", (1, 8, 8, 16, 40, 16, 1, False), {}),
    ("multiples of 16", (1, 8, 8, 16, 32, 24, 1, False), {}),
    ("stride", (1, 8, 8, 16, 32, 16, 3, False), {}),
    ("stride", (1, 8, 8, 16, 32, 16, 0, False), {}),
    ("256 images", (257, 8, 8, 16, 32, 16, 1, False), {}),
    ("residual", (1, 8, 8, 16, 32, 32, 1, True), {}),
    ("residual", (1, 8, 8, 16, 32, 16, 2, True), {}),
    ("view", (1, 8, 8, 16, 32, 16, 1, False), {"views": dict(x_ld=32, x_coff=32)}),
    ("view", (1, 8, 8, 16, 32, 16, 1, False), {"views": dict(y_ld=16, y_coff=16)}),
    ("view", (1, 8, 8, 16, 32, 16, 1, False), {"views": dict(x_ld=40)}),
    ("view", (1, 8, 8, 16, 32, 16, 1, True), {"views": dict(res_ld=32, res_coff=32)}),
    ("accumulators", (1, 10, 10, 256, 512, 512, 1, False), {}),
    ("accumulators", (1, 10, 10, 16, 32, 80, 1, False), {}),
    ("bad arguments", (0, 8, 8, 16, 32, 16, 1, False), {}),
    ("bad arguments", (1, 0, 8, 16, 32, 16, 1, False), {}),
    ("too large", (256, 1024, 1024, 16, 32, 16, 1, False), {}),
])
def test_planner_refuses_with_its_word(word, args, kw):
    p = _plan(*args, **kw)
    assert not p["accepted"] and word in p["reason"], p
    assert p["kernel"] == "" and p["blocks"] == 0


def test_entry_refuses_on_the_host_before_it_looks_at_the_engine():
    """What ltk_ul_ir_f16 refuses it refuses with the planner's text, also with no engine; an accepted plan without an engine is
    'bad arguments' behind the filled report."""
    from livetalking_amd import _lib
    lib = _lib.load()
    INVALID = -1          # include/ltk.h LTK_E_INVALID
    rep = _lib.UlIrReport()
    rc = lib.ltk_ul_ir_f16(None, None, 1, 8, 8, 16, 32, 16, 3, None, None, None, None, None, None, None, None, None, None, None, None, None, None, C.byref(rep))
    assert rc == INVALID and b"stride" in lib.ltk_last_error() and not rep.accepted and b"stride" in rep.reason
    rc2 = lib.ltk_ul_ir_f16(None, None, 1, 8, 8, 16, 32, 16, 1, None, None, None, None, None, None, None, None, None, None, None, None, None, None, C.byref(rep))
    assert rc2 == rc and rep.accepted and rep.kernel == b"ul_ir_kernel<1,false>" and b"bad arguments" in lib.ltk_last_error()


def test_knob_is_listed_and_defaults_to_zero():
    import os
    import re
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    with open(os.path.join(root, "livetalking_amd", "csrc", "tune.h")) as f:
        assert re.search(r"X\(UL_FUSE_IR, 0\)", f.read())
