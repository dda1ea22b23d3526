"""CPU tests of the Ultralight launch program as the pure architecture table lists it (ltk_debug_ultralight_program: no GPU, no
avatar): the listing with the fused inverted residual off and on, every view against its buffer, and the dataflow - which launch reads
which launch's output - walked symbolically against the layer tables of tests/ultralight_ref.py."""
from __future__ import annotations

import copy
import ctypes as C

import pytest

import ultralight_ref as ref

INVALID = -1
U_P, U_Q = 4, 5            # csrc/ultralight.hip UlBuf: the two temporaries DoubleConvDW ping-pongs between


@pytest.fixture(scope="module")
def programs():
    from livetalking_amd.engine import Engine
    return {f: Engine.ul_program(f) for f in (0, 1)}


def test_listing_unfused_fused_and_following_the_knob(programs):
    from livetalking_amd.engine import Engine
    names0 = [o["name"] for o in programs[0]["ops"]]
    assert names0 == ref.op_names() and len(names0) == 86
    assert all(o["type"] != 15 for o in programs[0]["ops"])
    gone = {b + s for b in ref.FUSED for s in (".conv.0", ".conv.3")}
    ops1 = programs[1]["ops"]
    assert [o["name"] for o in ops1] == [n for n in names0 if n not in gone] and len(ops1) == 60
    assert [o["name"] for o in ops1 if o["type"] == 15] == [b + ".conv.6" for b in ref.FUSED]
    # every other launch is the unfused listing's, field for field; type codes as ltk_ultralight_op_name documents them
    by0 = {o["name"]: o for o in programs[0]["ops"]}
    assert all(o == by0[o["name"]] for o in ops1 if o["type"] != 15)
    assert {o["type"] for o in programs[0]["ops"]} == {0, 10, 11, 12, 13, 14}
    assert programs[0]["buf_halfs"] == programs[1]["buf_halfs"]
    try:
        for knob in (1, 0):
            Engine.set_knob("UL_FUSE_IR", knob)
            assert Engine.ul_program(-1) == programs[knob]
    finally:
        Engine.set_knob("UL_FUSE_IR", 0)


def _views(o):
    """(buffer, ld, coff, channels, H, W) of the input, output and residual view an op has."""
    v = {"in": (o["in_buf"], o["in_ld"], o["in_coff"], o["cin"], o["H"], o["W"]),
         "out": (o["out_buf"], o["out_ld"], o["out_coff"], o["C"], o["Ho"], o["Wo"]),
         "res": (o["res_buf"], o["res_ld"], o["res_coff"], o["C"], o["Ho"], o["Wo"])}
    return {k: t for k, t in v.items() if t[0] >= 0}


@pytest.mark.parametrize("fuse", [0, 1])
def test_every_view_fits_its_buffer(programs, fuse):
    ops, halfs = programs[fuse]["ops"], programs[fuse]["buf_halfs"]
    written = [0] * len(halfs)
    for o in ops:
        v = _views(o)
        for which, (buf, ld, coff, ch, H, W) in v.items():
            assert ld % 16 == 0 and coff % 16 == 0 and coff >= 0 and ch > 0, (o["name"], which)
            assert coff + ch <= ld, (o["name"], which)
            assert ld * H * W <= halfs[buf], (o["name"], which)
        if "out" in v:
            ob, old, ocoff, och, Ho, Wo = v["out"]
            written[ob] = max(written[ob], old * Ho * Wo)
            for which in ("in", "res"):
                if which in v and v[which][0] == ob:        # the same buffer: the same tensor shape, other channels
                    buf, ld, coff, ch, H, W = v[which]
                    assert (ld, H, W) == (old, Ho, Wo) and (coff + ch <= ocoff or ocoff + och <= coff), (o["name"], which)
    if fuse == 0:                   # (a fused program leaves U_E1 / U_E2 to its unfused blocks: the arena is sized for knob 0)
        assert written == halfs
    assert all(w <= h for w, h in zip(written, halfs))


@pytest.mark.parametrize("fuse", [0, 1])
def test_dataflow_is_the_layer_tables(programs, fuse):
    ops = programs[fuse]["ops"]
    ref.check_dataflow(ops, bool(fuse))
    reads = ref.program_reads(ops)
    # spot checks of what check_dataflow compared with: torch.cat order at an Up and at the fuse concat
    assert reads["up1.conv.double_conv.0.conv.0"][0] == [("up1.up", 256), ("down3.maxpool_conv.0.double_conv.1.conv.6", 256)]
    assert reads["fuse_conv.0.double_conv.0.conv.0"][0] == [("down4.maxpool_conv.0.double_conv.1.conv.6", 512), ("audio_model.conv7.conv.6", 512)]
    assert reads["outc.conv"][0] == [("up4.conv.double_conv.1.conv.6", 32)]


@pytest.mark.parametrize("fuse", [0, 1])
def test_dataflow_check_rejects_planted_faults(programs, fuse):
    by = {o["name"]: i for i, o in enumerate(programs[fuse]["ops"])}

    def planted(name, **change):
        ops = copy.deepcopy(programs[fuse]["ops"])
        ops[by[name]].update(change)
        return ops

    # two temporaries swapped: a DoubleConvDW's first block lands on the buffer its input lives in / its second block does not read
    first = "fuse_conv.1.double_conv.0.conv.6"
    tmp = programs[fuse]["ops"][by[first]]["out_buf"]
    assert tmp in (U_P, U_Q)
    with pytest.raises(AssertionError):
        ref.check_dataflow(planted(first, out_buf=U_P + U_Q - tmp), bool(fuse))
    # a concat half shifted by 16 channels: the encoder level's skip tensor inside up3's concat buffer
    skip = "down1.maxpool_conv.0.double_conv.1.conv.6"
    coff = programs[fuse]["ops"][by[skip]]["out_coff"]
    assert coff == 64
    with pytest.raises(AssertionError):
        ref.check_dataflow(planted(skip, out_coff=coff - 16), bool(fuse))
    # a skip tensor overwritten before its Up: the decoder's temporary pointed at the encoder's concat buffer
    with pytest.raises(AssertionError):
        ref.check_dataflow(planted("up1.conv.double_conv.1.conv.6", out_buf=programs[fuse]["ops"][by[skip]]["out_buf"], out_ld=128), bool(fuse))


def test_refusals_without_a_gpu():
    from livetalking_amd import _lib
    lib = _lib.load()
    ops = (_lib.UlOpInfo * 96)()
    halfs = (C.c_uint64 * 12)()
    n_ops, n_bufs = C.c_int(0), C.c_int(0)
    good = [0, ops, 96, C.byref(n_ops), halfs, 12, C.byref(n_bufs)]
    assert lib.ltk_debug_ultralight_program(*good) == 0 and n_ops.value == 86 and n_bufs.value == 11
    for at, bad in ((0, 2), (0, -2), (1, None), (2, 85), (2, 0), (3, None), (4, None), (5, 10), (5, 0), (6, None)):
        args = list(good)
        args[at] = bad
        assert lib.ltk_debug_ultralight_program(*args) == INVALID, (at, bad)
        assert lib.ltk_last_error()
    assert lib.ltk_debug_ultralight_program(1, ops, 60, C.byref(n_ops), halfs, 11, C.byref(n_bufs)) == 0 and n_ops.value == 60
    assert lib.ltk_debug_ultralight_program(1, ops, 59, C.byref(n_ops), halfs, 11, C.byref(n_bufs)) == INVALID
