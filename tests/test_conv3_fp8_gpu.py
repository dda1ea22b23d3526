"""The fp8 instantiations of the conv3 family (csrc/conv3_mfma.hip: conv3_kernel<1,NBT,PXW,NC8,9,1,Q>, Q = 1 the e4m3 MFMA behind
k3_pick_q8, Q = 2 the MX-scaled MFMA behind k3_pick_mx) on their own, through ltk_conv2d_fp8_ex, against float64: the cases, exact e4m3
operands, buffers and gates of tests/conv_fp8_cases.py (conv_cases' check), whose rounding model and planted faults tests/test_conv_host.py
holds on the CPU.  Every instantiation is forced by name at ragged tile columns (l2w 5: the column key), the 12-pixel pitch (l2w 3), the
row key (l2w 4), one-pixel maps, short last tiles, every split factor and channel views; tests/test_fp8_gpu.py keeps the
quantiser-in-the-loop path with off-grid weights at whatever tile the rule picks.

Every case asserts: the call succeeds; the hook reports the instantiation, the split factor and the item count the case expects; per
element |dev - ref| <= 2^-10 |ref| + slope 9 Cin 2^-23 A + 2^-24 with no violator; aggregate rel_l2(dev, ref) <= 2 rel_l2(mod, ref) + 1e-4;
every half of the output buffer outside the view still holds the pre-fill pattern.

LTK_CONV3_PARITY_OUT names a file the records are appended to."""
from __future__ import annotations

import os

import numpy as np
import pytest
import torch

import conv_cases as K
import conv_fp8_cases as F8

pytestmark = pytest.mark.gpu

GROUPS = F8.groups()


def _emit(lines):
    for ln in lines:
        print(ln)
    out = os.environ.get("LTK_CONV3_PARITY_OUT")
    if out:
        with open(out, "a") as f:
            f.write("\n".join(lines) + "\n")


def _run(engine, rf: F8.Reference):
    """-> (the hook's report, the output buffer as host int16)"""
    from livetalking_amd._lib import LtkError
    from livetalking_amd.engine import Engine
    c, b = rf.c, rf.buf
    d_x = torch.from_numpy(b.x).cuda()
    d_r = torch.from_numpy(b.res.view(np.int16)).cuda() if b.res is not None else None
    d_y = torch.from_numpy(b.empty_y()).cuda()
    try:
        if c.nc8:
            Engine.set_knob("CONV3_NC8", c.nc8)         # read when the plan is built
        rep = engine.conv2d_fp8_ex(d_x.data_ptr(), c.N, c.H, c.W, c.Cin, rf.w.numpy(), c.Cout, rf.scale.numpy(), rf.shift.numpy(), rf.act_scale,
                                   c.Q, d_r.data_ptr() if d_r is not None else 0, d_y.data_ptr(), **c.opts(b))
    except LtkError as ex:
        # a HIP error: the device context is gone.  Ending the SESSION is meant - the test files behind this one are not run either,
        # so that nothing more is started on a device that has just faulted
        if ex.code == -2:
            pytest.exit(f"{c.id}: {ex}", returncode=3)
        raise
    finally:
        if c.nc8:
            Engine.set_knob("CONV3_NC8", 0)
    return rep, d_y.cpu().numpy()


def _one(engine, ci: int):
    """One case -> (its line, its failures)."""
    rf = F8.reference(ci)
    c = rf.c
    rep, y = _run(engine, rf)
    rec, bad = K.check(rf, y, rep["kernel"])
    if rep["kernel"] != c.expect:
        bad.append(f"{c.id}: launched {rep['kernel']!r}, the case expects {c.expect!r}")
    g = F8.geometry(c)
    if (rep["family"], rep["ksplit"], rep["items"], rep["grid"]) != (0, c.ksplit, g["items"], g["grid"]):
        bad.append(f"{c.id}: reported ksplit {rep['ksplit']}, {rep['items']} items on {rep['grid']} blocks; expected {c.ksplit}, {g['items']} on {g['grid']}")
    if (rep["G"], rep["NBT"], rep["PXW"], rep["NC8"], rep["T"], rep["S"]) != (1, c.NBT, c.PXW, c.NC8, 9, 1):
        bad.append(f"{c.id}: the report's template arguments do not spell {c.expect}")
    return K.format_record(c, rep["kernel"], rep["ksplit"], rec), bad


@pytest.mark.parametrize("group", sorted(GROUPS), ids=sorted(GROUPS))
def test_conv3_fp8_against_float64(engine, group):
    lines, bad = [], []
    for ci in GROUPS[group]:
        ln, fails = _one(engine, ci)
        lines.append(ln)
        bad += fails
    _emit(lines)
    assert lines
    assert not bad, "\n".join(bad)


def test_every_listed_fp8_instantiation_is_launched(engine):
    """The union of what the hook reports over one (the smallest) case per expected kernel equals ltk_debug_conv3_fp8_variants."""
    first = {}
    for i, c in enumerate(F8.CASES):
        if c.expect not in first or c.macs < F8.CASES[first[c.expect]].macs:
            first[c.expect] = i
    seen = {_run(engine, F8.reference(i))[0]["kernel"] for i in first.values()}
    listed = engine.conv3_fp8_variants()
    assert len(listed) == 12 and seen == set(listed)


def test_conv3_fp8_refuses_what_it_cannot_serve(engine):
    """An operand format, a tile or a view the fp8 kernels have nothing for comes back as LTK_E_INVALID with its message, never as another
    tile - through the launching hook, with real buffers; and the engine still serves afterwards."""
    from livetalking_amd._lib import LtkError
    from livetalking_amd.engine import Engine
    x = torch.zeros(1 << 20, dtype=torch.uint8, device="cuda")
    y = torch.zeros(1 << 20, dtype=torch.int16, device="cuda")

    def call(N=2, H=9, W=16, Cin=64, Cout=32, quant=1, **o):
        return engine.conv2d_fp8_ex(x.data_ptr(), N, H, W, Cin, np.zeros((Cout, Cin, 3, 3), np.float32), Cout, None, None, 8.0, quant, 0, y.data_ptr(), **o)

    def refused(match, nc8=0, **kw):
        try:
            Engine.set_knob("CONV3_NC8", nc8)
            with pytest.raises(LtkError, match=match) as ex:
                call(**kw)
        finally:
            Engine.set_knob("CONV3_NC8", 0)
        assert ex.value.code == -1, kw

    refused("Cin % 32 == 0", Cin=48)
    refused("Cin % 64 == 0", Cin=96, quant=2)
    refused("no kernel instantiation", quant=2, force_pxw=4, force_nbt=1)               # MX: 64-channel chunks, no 512-pixel tile
    refused("no kernel instantiation", nc8=4, force_pxw=4, force_nbt=1)                 # ... nor the e4m3 kernels on 64-channel chunks
    refused("no kernel instantiation", nc8=4, force_pxw=1, force_nbt=1)                 # ... which have no 128-pixel tile either
    refused("no kernel instantiation", force_pxw=2, force_nbt=2)                        # 64-cout blocks of a 32-cout layer
    refused("patch does not fit the staging budget", N=1, H=256, W=1, force_pxw=2, force_nbt=1)
    refused("multiples of 32", x_ld=112, x_coff=16)
    refused("outside its buffer", x_ld=64, x_coff=32)
    refused("outside its buffer", y_ld=48, y_coff=32)
    refused("bad options", act=4)
    refused("bad options", family=4)
    refused("fp8 operands", ups=1)
    refused("bad arguments", quant=3)
    # the unforced rule under CONV3_NC8 = 4 on a layer with few items: a kernel that exists (it used to end in "no kernel instantiation")
    try:
        Engine.set_knob("CONV3_NC8", 4)
        rep = call(N=2, H=32, W=32, Cin=320, Cout=320)
    finally:
        Engine.set_knob("CONV3_NC8", 0)
    assert rep["kernel"] == F8.vname(1, 2, 4, 1)
    rep = call(force_pxw=1, force_nbt=1, force_ksplit=1)                                # and the engine still serves
    assert rep["kernel"] == F8.vname(1, 1, 2, 1)
