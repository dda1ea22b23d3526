"""The first-generation conv kernel of csrc/conv_mfma.hip (all 13 instantiations of its picker: the two-taps-per-MFMA path on 8-channel
inputs with its padded odd tap, the compiled-in 3x3 taps with and without the s2half column-parity patch rows, the tap-table path, partial
chunks, multi-image tiles with a short last tile, the tile-shrink loop, the XCD block remap at uneven block counts, the four-phase
transposed conv, the 1x1-expand, the LDS-transposed epilogue with partial cout blocks, residual and every activation, channel views) on
its own, through ltk_conv2d_f16_ex, against float64: the cases, inputs, buffers and gates of tests/conv1_cases.py and tests/conv_cases.py,
whose rounding model and planted faults tests/test_conv1_host.py holds on the CPU.

Every case asserts: the call succeeds; the hook reports the instantiation, the tile (l2w, l2h, images per tile, s2half), the blocks and
the LDS bytes the case expects; per element |dev - ref| <= 2^-10 |ref| + slope n 2^-23 A + 2^-24 with no violator; aggregate
rel_l2(dev, ref) <= 2 rel_l2(mod, ref) + 1e-4; every half of the output buffer outside the view still holds the pre-fill pattern.

LTK_CONV1_PARITY_OUT names a file the records are appended to."""
from __future__ import annotations

import os

import numpy as np
import pytest
import torch

import conv1_cases as C1
import conv_cases as K

pytestmark = pytest.mark.gpu

GROUPS = C1.groups()


def _emit(lines):
    for ln in lines:
        print(ln)
    out = os.environ.get("LTK_CONV1_PARITY_OUT")
    if out:
        with open(out, "a") as f:
            f.write("\n".join(lines) + "\n")


def _run(engine, rf: C1.Reference):
    """-> (the hook's report, the output buffer as host int16)"""
    from livetalking_amd._lib import LtkError
    from livetalking_amd.engine import Engine
    c, b = rf.c, rf.buf
    d_x = torch.from_numpy(b.x.view(np.int16)).cuda()
    d_r = torch.from_numpy(b.res.view(np.int16)).cuda() if b.res is not None else None
    d_y = torch.from_numpy(b.empty_y()).cuda()
    try:
        Engine.set_knob("CONV_V3", c.v3)            # read when the plan is built
        rep = engine.conv2d_f16_ex(d_x.data_ptr(), c.N, c.H, c.W, c.Cin, rf.w.numpy(), c.Cout, c.k, c.stride, c.pad, c.transposed, c.out_pad,
                                   rf.scale.numpy(), rf.shift.numpy(), d_r.data_ptr() if d_r is not None else 0, d_y.data_ptr(), **c.opts(b))
    except LtkError as ex:
        # a HIP error: the device context is gone.  Ending the SESSION is meant - the test files behind this one are not run either,
        # so that nothing more is started on a device that has just faulted
        if ex.code == -2:
            pytest.exit(f"{c.id}: {ex}", returncode=3)
        raise
    finally:
        Engine.set_knob("CONV_V3", 1)
    return rep, d_y.cpu().numpy()


def _one(engine, ci: int):
    """One case -> (its line, its failures)."""
    rf = C1.reference(ci)
    c = rf.c
    rep, y = _run(engine, rf)
    rec, bad = K.check(rf, y, rep["kernel"])
    bad += C1.report_mismatches(c, C1.geometry(c), rep)
    return C1.format_record("conv1", c, rep["kernel"], rec), bad


@pytest.mark.parametrize("group", sorted(GROUPS), ids=sorted(GROUPS))
def test_conv1_against_float64(engine, group):
    lines, bad = [], []
    for ci in GROUPS[group]:
        ln, fails = _one(engine, ci)
        lines.append(ln)
        bad += fails
    _emit(lines)
    assert lines
    assert not bad, "\n".join(bad)


def test_every_listed_instantiation_is_launched(engine):
    """The union of what the hook reports over one (the smallest) case per expected kernel equals ltk_debug_conv1_variants."""
    first = {}
    for i, c in enumerate(C1.CASES):
        if c.expect not in first or c.macs < C1.CASES[first[c.expect]].macs:
            first[c.expect] = i
    seen = {_run(engine, C1.reference(i))[0]["kernel"] for i in first.values()}
    assert seen == set(engine.conv1_variants()) and len(seen) == 13


def test_conv1_refuses_what_it_cannot_serve(engine):
    """What the route and the first-generation planner refuse comes back as LTK_E_INVALID with its message, nothing enqueued; and the
    engine still serves."""
    from livetalking_amd._lib import LtkError
    from livetalking_amd.engine import Engine
    x = torch.zeros(1 << 16, dtype=torch.int16, device="cuda")
    y = torch.full((1 << 16,), K.PATTERN, dtype=torch.int16, device="cuda")

    def call(N, H, W, Cin, Cout, k, stride, pad, transposed=False, v3=1, **o):
        kh, kw = (k, k) if isinstance(k, int) else k
        w = np.zeros((Cin, Cout, kh, kw) if transposed else (Cout, Cin, kh, kw), np.float32)
        try:
            Engine.set_knob("CONV_V3", v3)
            return engine.conv2d_f16_ex(x.data_ptr(), N, H, W, Cin, w, Cout, k, stride, pad, transposed, 0, None, None, 0, y.data_ptr(), **o)
        finally:
            Engine.set_knob("CONV_V3", 1)

    for match, kw in C1.REFUSALS:
        with pytest.raises(LtkError, match=match) as ex:
            call(**kw)
        assert ex.value.code == -1, (match, kw)
    assert bool((y == K.PATTERN).all())
    rep = call(2, 9, 16, 6, 32, 3, 1, 1)
    assert rep["kernel"] == C1.vn(1, 1, False, 5) and (rep["l2w"], rep["l2h"], rep["NB"]) == (4, 4, 1)
    out = y.cpu().numpy()[:2 * 2 * 9 * 16 * 16]
    assert not out.any()                     # zero weights, scale 1, shift 0: the two images' 32 channels are zero, written
