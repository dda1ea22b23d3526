"""The special-case kernels at the head of the Wav2Lip program (csrc/conv7_mfma.hip: conv7_kernel<BANK> / <PACKED>, audio0_kernel,
audio3_kernel, convs2d_kernel<1|2>) on their own, through ltk_w2l_head_f16, against float64, away from the network's single geometry:
1, 2 and 9 frames through permuted and repeated frame tables (9: the persistent tile walk), waves that straddle frames and a half-live
last wave, one output row, blocks with one live wave, one, two and three cout tiles, two pixel tiles per row, channel views of x and y.
The cases, inputs, buffers and gates of tests/conv1_cases.py and tests/conv_cases.py, whose rounding model and planted faults
tests/test_conv1_host.py holds on the CPU.

Every case asserts: the call succeeds; per element |dev - ref| <= 2^-10 |ref| + n 2^-23 A + 2^-24 with no violator; aggregate
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


def _emit(lines):
    for ln in lines:
        print(ln)
    out = os.environ.get("LTK_CONV1_PARITY_OUT")
    if out:
        with open(out, "a") as f:
            f.write("\n".join(lines) + "\n")


def _call(engine, what, *a, **kw):
    from livetalking_amd._lib import LtkError
    try:
        return engine.w2l_head_f16(*a, **kw)
    except LtkError as ex:
        # a HIP error: the device context is gone.  Ending the SESSION is meant, so that nothing more is started on a device that has just faulted
        if ex.code == -2:
            pytest.exit(f"{what}: {ex}", returncode=3)
        raise


def _run(engine, rf: C1.HeadReference) -> np.ndarray:
    """-> the output buffer as host int16"""
    c, b = rf.c, rf.buf
    d_y = torch.from_numpy(b.empty_y()).cuda()
    kw = dict(H=c.H, W=c.W, Cin=c.Cin, Cout=c.Cout) if c.op == "convs2d" else {}
    kw.update(c.opts(b))
    if c.op in ("conv7_bank", "audio0"):
        d_in = torch.from_numpy(b.frames_u8 if c.op == "conv7_bank" else b.mel).cuda()
        stride = d_in[0].numel() * d_in.element_size()
        kw["frame_ptrs"] = [d_in.data_ptr() + f * stride for f in c.frames]
    else:
        d_in = torch.from_numpy(b.x.view(np.int16)).cuda()
        kw["d_x_ptr"] = d_in.data_ptr()
    _call(engine, c.id, c.op, rf.w.numpy(), rf.scale.numpy(), rf.shift.numpy(), d_y.data_ptr(), c.N, **kw)
    return d_y.cpu().numpy()


@pytest.mark.parametrize("hi", range(len(C1.HEAD_CASES)), ids=[c.id for c in C1.HEAD_CASES])
def test_head_kernel_against_float64(engine, hi):
    rf = C1.head_reference(hi)
    rec, bad = K.check(rf, _run(engine, rf), rf.c.op)
    _emit([C1.format_record("w2l-head", rf.c, rf.c.op, rec)])
    assert not bad, "\n".join(bad)


def test_conv7_bank_and_packed_are_byte_identical(engine):
    """The fused pack forms the operand the packed input holds: the same MFMAs on the same halfs, so the same bytes, at every frame count."""
    by = {(c.op, c.N): i for i, c in enumerate(C1.HEAD_CASES) if c.op.startswith("conv7")}
    for N in (1, 2, 9):
        yb = _run(engine, C1.head_reference(by["conv7_bank", N]))
        yp = _run(engine, C1.head_reference(by["conv7_packed", N]))
        assert yb.shape == yp.shape and np.array_equal(yb, yp), N


def test_head_hook_passes_the_launchers_refusals_back(engine):
    from livetalking_amd._lib import LtkError
    x = torch.zeros(1 << 20, dtype=torch.int16, device="cuda")
    y = torch.full((1 << 20,), K.PATTERN, dtype=torch.int16, device="cuda")
    shapes = {"conv7_bank": (16, 6, 7, 7), "conv7_packed": (16, 6, 7, 7), "audio0": (32, 1, 3, 3), "audio3": (64, 32, 3, 3)}

    def call(op, N, H=0, W=0, Cin=0, Cout=0, **o):
        w = np.zeros(shapes.get(op, (Cout, Cin, 3, 3)), np.float32)
        co = w.shape[0]
        kw = dict(frame_ptrs=[x.data_ptr()] * N) if op in ("conv7_bank", "audio0") else dict(d_x_ptr=x.data_ptr())
        return _call(engine, op, op, w, np.ones(co, np.float32), np.zeros(co, np.float32), y.data_ptr(), N, H=H, W=W, Cin=Cin, Cout=Cout, **kw, **o)

    for op, match, kw in C1.HEAD_REFUSALS:
        with pytest.raises(LtkError, match=match) as ex:
            call(op, **kw)
        assert ex.value.code == -1, (op, match, kw)
    assert bool((y == K.PATTERN).all())
    call("convs2d", 1, H=2, W=64, Cin=16, Cout=32)                      # and the engine still serves
    out = y.cpu().numpy()
    assert not out[:32 * 32].any() and (out[32 * 32:] == K.PATTERN).all()
