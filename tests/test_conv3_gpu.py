"""The conv3 family of csrc/conv3_mfma.hip (every fp16 instantiation of its pickers, the split-K finish, the persistent item walk, the
nearest-upsample read, the four-phase upsample-conv, the merged transposed conv, channel-block views) and the row kernels of
csrc/rowgemm.hip (rowgemm, rowconv, rowconvT) on their own, through ltk_conv2d_f16_ex, against float64: the cases, inputs, buffers and
gates of tests/conv_cases.py, whose rounding model and planted faults tests/test_conv_host.py holds on the CPU.

Every case asserts: the call succeeds; the hook reports the instantiation, the split factor (after the "no empty split" correction)
and the item count the case expects; per element |dev - ref| <= 2^-10 |ref| + slope n 2^-23 A + 2^-24 with no violator; aggregate
rel_l2(dev, ref) <= 2 rel_l2(mod, ref) + 1e-4; every half of the output buffer outside the view still holds the pre-fill pattern.

LTK_CONV3_PARITY_OUT names a file the records are appended to."""
from __future__ import annotations

import os

import numpy as np
import pytest
import torch

import conv_cases as K

pytestmark = pytest.mark.gpu

GROUPS = K.groups()


def _emit(lines):
    for ln in lines:
        print(ln)
    out = os.environ.get("LTK_CONV3_PARITY_OUT")
    if out:
        with open(out, "a") as f:
            f.write("\n".join(lines) + "\n")


def _run(engine, rf: K.Reference):
    """-> (the hook's report, the output buffer as host int16)"""
    from livetalking_amd.engine import Engine
    c, b = rf.c, rf.buf
    d_x = torch.from_numpy(b.x.view(np.int16)).cuda()
    d_r = torch.from_numpy(b.res.view(np.int16)).cuda() if b.res is not None else None
    d_y = torch.from_numpy(b.empty_y()).cuda()
    from livetalking_amd._lib import LtkError
    try:
        if c.nc8:
            Engine.set_knob("CONV3_NC8", c.nc8)         # read when the plan is built
        rep = engine.conv2d_f16_ex(d_x.data_ptr(), c.N, c.H, c.W, c.Cin, rf.w.numpy(), c.Cout, c.k, c.stride, c.pad, c.transposed, c.out_pad,
                                   rf.scale.numpy(), rf.shift.numpy(), d_r.data_ptr() if d_r is not None else 0, d_y.data_ptr(), **c.opts(b))
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
    rf = K.reference(ci)
    c = rf.c
    rep, y = _run(engine, rf)
    rec, bad = K.check(rf, y, rep["kernel"])
    if rep["kernel"] != c.expect:
        bad.append(f"{c.id}: launched {rep['kernel']!r}, the case expects {c.expect!r}")
    if c.family == 0:
        g = K.geometry(c)
        if (rep["ksplit"], rep["items"], rep["grid"]) != (c.ksplit, g["items"], g["grid"]):
            bad.append(f"{c.id}: reported ksplit {rep['ksplit']}, {rep['items']} items on {rep['grid']} blocks; expected {c.ksplit}, {g['items']} on {g['grid']}")
        if (rep["G"], rep["NBT"], rep["PXW"], rep["NC8"], rep["T"], rep["S"]) != (c.G, c.NBT, c.PXW, c.NC8, c.T, c.S):
            bad.append(f"{c.id}: the report's template arguments do not spell {c.expect}")
    elif f"<{rep['FT']}" not in rep["kernel"]:
        bad.append(f"{c.id}: the report's FT {rep['FT']} / UB {rep['UB']} do not spell {rep['kernel']}")
    return K.format_record(c, rep["kernel"], rep["ksplit"], rec), bad


@pytest.mark.parametrize("group", sorted(GROUPS), ids=sorted(GROUPS))
def test_conv3_against_float64(engine, group):
    lines, bad = [], []
    for ci in GROUPS[group]:
        ln, fails = _one(engine, ci)
        lines.append(ln)
        bad += fails
    _emit(lines)
    assert lines
    assert not bad, "\n".join(bad)


def test_every_listed_instantiation_is_launched(engine):
    """The union of what the hook reports over one (the smallest) case per expected kernel equals ltk_debug_conv3_variants."""
    first = {}
    for i, c in enumerate(K.CASES):
        if c.family == 0 and (c.expect not in first or c.macs < K.CASES[first[c.expect]].macs):
            first[c.expect] = i
    seen = {_run(engine, K.reference(i))[0]["kernel"] for i in first.values()}
    assert seen == set(engine.conv3_variants())


def test_conv3_refuses_what_it_cannot_serve(engine):
    """A tile, an upsample or a view conv3 has nothing for comes back as LTK_E_INVALID with its message, never as another tile."""
    from livetalking_amd._lib import LtkError
    x = torch.zeros(1 << 20, dtype=torch.int16, device="cuda")
    y = torch.zeros(1 << 20, dtype=torch.int16, device="cuda")

    def call(N=2, H=9, W=16, Cin=32, Cout=32, k=3, stride=1, pad=1, transposed=False, out_pad=0, **o):
        w = np.zeros((Cin, Cout, k, k) if transposed else (Cout, Cin, k, k), np.float32)
        return engine.conv2d_f16_ex(x.data_ptr(), N, H, W, Cin, w, Cout, k, stride, pad, transposed, out_pad, None, None, 0, y.data_ptr(), **o)

    def refused(match, **kw):
        with pytest.raises(LtkError, match=match) as ex:
            call(**kw)
        assert ex.value.code == -1, kw

    from livetalking_amd.engine import Engine
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
    # a tile that cannot be staged: a one-pixel-wide map makes the 256-pixel tile a 258 x 3 patch, 1600 slots against a budget of 1024
    refused("patch does not fit the staging budget", N=1, H=256, W=1, force_pxw=2, force_nbt=1)
    refused("even H, W", ups=1)
    refused("even H, W", ups=2)
    refused("four-phase", H=10, k=1, pad=0, ups=2)
    refused("conv3 feature", H=10, Cout=64, stride=(3, 1), ups=1)                                  # the first-generation kernel has no upsample read
    refused("multiples of 16", x_ld=40, x_coff=8)
    refused("outside its buffer", x_ld=32, x_coff=16)
    refused("outside its buffer", y_ld=48, y_coff=32)
    refused("bad options", act=4)
    refused("bad options", family=4)
    refused("rowgemm", N=33, H=1, W=1, Cin=512, Cout=512, k=1, pad=0, family=1)         # more frames than it is built for
    refused("rowgemm", N=2, H=2, W=1, Cin=512, Cout=512, k=1, pad=0, family=1)
    refused("rowconv", N=2, H=8, W=8, Cin=256, Cout=256, k=1, pad=0, family=2)
    refused("rowconv: more rows", N=33, H=8, W=8, Cin=32, Cout=32, family=2)
    refused("rowconvT", N=2, H=4, W=4, Cin=256, Cout=256, family=3)
    rep = call(force_pxw=1, force_nbt=1, force_ksplit=1)                                # and the engine still serves
    assert rep["kernel"] == K.vname(1, 1, 1, 2, 9)
