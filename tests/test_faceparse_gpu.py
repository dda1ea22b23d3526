"""GPU: the face parser's own kernels (csrc/parse_kernels.hip) through their stand-alone hooks, each against float64 on the device's
own inputs under the gates of tests/faceparse_cases.py (tests/test_faceparse_host.py holds a simulated device with planted faults to
the same gates): the stem at 10 x 14 (every tile partial), 64 x 64 and 512 x 512, N = 1 and 3; the max pool on negative input at odd
and even sizes; the global average at P = 4 .. 4096; the three forms of the channel gate inside a channel view between guard blocks;
the segmentation head at 2 x 2, 8 x 8 and 64 x 64 with the first-index tie rule; byte identity alone and in company; the refusals.
Engine of its own (module scope)."""
from __future__ import annotations

import numpy as np
import pytest

import faceparse_cases as FP

pytestmark = pytest.mark.gpu

GUARD = 0x5A5A          # what the channel blocks beside a view hold before and after a launch


@pytest.fixture(scope="module")
def eng():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from livetalking_amd.engine import Engine
    e = Engine(0)
    yield e
    e.close()


def _dev(a: np.ndarray):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a).view(np.int16 if a.dtype in (np.float16, np.uint16) else a.dtype)).cuda()


def _in_view(x_cb16: np.ndarray, view: bool) -> np.ndarray:
    """The tensor as blocks [1, 1 + CB) of a buffer of CB + 2 channel blocks (guards around it), or as it is."""
    if not view:
        return x_cb16
    n, cb = x_cb16.shape[:2]
    buf = np.full((n, cb + 2) + x_cb16.shape[2:], GUARD, np.uint16).view(np.float16)
    buf[:, 1:1 + cb] = x_cb16
    return buf


def _out_buf(n, cb, h, w, view: bool) -> np.ndarray:
    return np.full((n, cb + (2 if view else 0), h, w, 16), GUARD, np.uint16)


def _out_view(y, cb: int, view: bool) -> np.ndarray:
    """The device's output blocks as float16; the guard blocks must be as they were."""
    y = y.cpu().numpy().view(np.uint16)
    if not view:
        return y.view(np.float16)
    assert (y[:, 0] == GUARD).all() and (y[:, 1 + cb:] == GUARD).all(), "a guard block was written"
    return np.ascontiguousarray(y[:, 1:1 + cb]).view(np.float16)


# ------------------------------------------------------------------------------------------ stem
def _run_stem(eng, c, view=False):
    import torch
    rgb = torch.from_numpy(c.rgb).cuda()
    y = _dev(_out_buf(c.N, 4, c.H // 2, c.W // 2, view))
    eng.parse_stem_f16(rgb.data_ptr(), c.N, c.H, c.W, c.w, c.scale, c.shift, y.data_ptr(), dict(y_ld=96, y_coff=16) if view else None)
    torch.cuda.synchronize()
    return FP.from_cb16(_out_view(y, 4, view), 64)


@pytest.mark.parametrize("shape", FP.STEM_SHAPES + [(1, 512, 512)], ids=lambda s: "x".join(map(str, s)))
def test_stem_against_float64(eng, shape):
    c = FP.Stem(*shape)
    ref, tol = c.ref_tol()
    dev = _run_stem(eng, c, view=shape[1] == 10)
    fig = FP.check(dev, ref, c.model(), tol)
    print(f"stem {shape}: worst |dev - ref| / tol {fig['worst']:.3f}, rel dev {fig['rel_dev']:.3e} model {fig['rel_mod']:.3e}")


def test_stem_image_alone_and_in_company(eng):
    c3, c1 = FP.Stem(3, 64, 64), FP.Stem(1, 64, 64)
    c1.rgb, c1.w, c1.scale, c1.shift = c3.rgb[1:2].copy(), c3.w, c3.scale, c3.shift
    a, b = _run_stem(eng, c3), _run_stem(eng, c1)
    assert np.array_equal(a[1:2], b) and np.array_equal(_run_stem(eng, c3), a)


# ------------------------------------------------------------------------------------------ max pool
@pytest.mark.parametrize("shape", FP.POOL_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_maxpool_is_exact(eng, shape):
    import torch
    N, C, H, W = shape
    view = H == 7
    x = FP.pool_input(*shape)
    ref = FP.pool_ref(x)
    d_x = _dev(_in_view(FP.to_cb16(x), view))
    y = _dev(_out_buf(N, C // 16, ref.shape[2], ref.shape[3], view))
    ld = C + 32
    eng.maxpool3x3s2_f16(d_x.data_ptr(), N, H, W, C, y.data_ptr(), dict(x_ld=ld, x_coff=16, y_ld=ld, y_coff=16) if view else None)
    torch.cuda.synchronize()
    assert np.array_equal(FP.from_cb16(_out_view(y, C // 16, view), C), ref)


# ------------------------------------------------------------------------------------------ global average pool
def _run_gap(eng, x, view=False):
    import torch
    N, C, P, _ = x.shape
    d_x = _dev(_in_view(FP.to_cb16(x), view))
    y = _dev(_out_buf(N, C // 16, 1, 1, view))
    ld = C + 32
    eng.global_avgpool_f16(d_x.data_ptr(), N, P, C, y.data_ptr(), dict(x_ld=ld, x_coff=16, y_ld=ld, y_coff=16) if view else None)
    torch.cuda.synchronize()
    return FP.from_cb16(_out_view(y, C // 16, view), C)


@pytest.mark.parametrize("shape", FP.GAP_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_gap_against_float64(eng, shape):
    x = FP.gap_input(*shape)
    ref, tol = FP.gap_ref_tol(x)
    dev = _run_gap(eng, x, view=shape[2] == 9)
    fig = FP.check(dev, ref, FP.gap_model(x), tol)
    print(f"gap {shape}: worst |dev - ref| / tol {fig['worst']:.3f}, equals the tree model: {np.array_equal(dev, FP.gap_model(x))}")
    if shape[0] > 1:                 # the bytes of an image do not depend on the images beside it, nor on the run
        assert np.array_equal(_run_gap(eng, x[1:2]), dev[1:2]) and np.array_equal(_run_gap(eng, x, view=shape[2] == 9), dev)


# ------------------------------------------------------------------------------------------ channel gate
@pytest.mark.parametrize("form", list(FP.GATE_FORMS))
def test_gate_in_a_channel_view(eng, form):
    import torch
    c = FP.Gate(form)
    ref, tol = c.ref_tol()
    cb, ld = c.C // 16, c.C + 32
    d_x = _dev(_in_view(FP.to_cb16(c.x), True))
    d_a = _dev(FP.to_cb16(c.a))
    d_b = _dev(FP.to_cb16(c.b)) if c.b is not None else None
    d_r = _dev(_in_view(FP.to_cb16(c.r), True)) if c.r is not None else None
    y = _dev(_out_buf(c.N, cb, c.P, 1, True))
    eng.chan_gate_f16(d_x.data_ptr(), c.N, c.P, c.C, d_a.data_ptr(), y.data_ptr(), d_b.data_ptr() if d_b is not None else 0,
                      d_r.data_ptr() if d_r is not None else 0, c.plus1, dict(x_ld=ld, x_coff=16, y_ld=ld, y_coff=16, res_ld=ld, res_coff=16))
    torch.cuda.synchronize()
    dev = FP.from_cb16(_out_view(y, cb, True), c.C)
    fig = FP.check(dev, ref, c.model(), tol)
    print(f"gate {form}: worst |dev - ref| / tol {fig['worst']:.3f}, rel dev {fig['rel_dev']:.3e} model {fig['rel_mod']:.3e}")


# ------------------------------------------------------------------------------------------ segmentation head
def _run_seg(eng, x):
    import torch
    N, _, h, w = x.shape
    d_x = _dev(FP.to_cb16(x))
    lab = torch.full((N, 8 * h, 8 * w), 255, dtype=torch.uint8, device="cuda")
    eng.seg_argmax_f16(d_x.data_ptr(), N, h, w, lab.data_ptr())
    torch.cuda.synchronize()
    return lab.cpu().numpy()


@pytest.mark.parametrize("shape", FP.SEG_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_seg_labels_against_float64(eng, shape):
    x = FP.seg_input(*shape)
    dev = _run_seg(eng, x)
    fig = FP.seg_check(dev, x)
    print(f"seg {shape}: {fig['excluded']:.4%} of the pixels inside the margin, {fig['differ']} labels differ there")
    if shape[0] > 1:
        assert np.array_equal(_run_seg(eng, x[1:2]), dev[1:2]) and np.array_equal(_run_seg(eng, x), dev)


def test_seg_first_index_wins_a_tie(eng):
    x = FP.seg_input(2, 8, 8, ties=True)
    assert (_run_seg(eng, x) == 3).all()


# ------------------------------------------------------------------------------------------ refusals
def test_refusals(eng):
    import torch
    from livetalking_amd._lib import LtkError
    buf = torch.zeros(1 << 16, dtype=torch.int16, device="cuda")
    p = buf.data_ptr()
    w = np.zeros((64, 3, 7, 7), np.float32)
    calls = [
        (lambda: eng.parse_stem_f16(p, 1, 9, 8, w, d_y_ptr=p), "even"),
        (lambda: eng.parse_stem_f16(p, 1, 8, 8, w, d_y_ptr=p, views=dict(y_ld=64, y_coff=16)), "leaves its buffer"),
        (lambda: eng.parse_stem_f16(p, 1, 8, 8, w, d_y_ptr=p, views=dict(y_ld=72)), "multiples of 16"),
        (lambda: eng.parse_stem_f16(p, 1, 8, 8, w, d_y_ptr=p, views=dict(act=1)), "only the channel views"),
        (lambda: eng.maxpool3x3s2_f16(p, 1, 8, 8, 24, p), "C % 16"),
        (lambda: eng.maxpool3x3s2_f16(p, 1, 8, 8, 32, p, dict(x_ld=32, x_coff=16)), "leaves its buffer"),
        (lambda: eng.global_avgpool_f16(p, 1, 4097, 16, p), "4096"),
        (lambda: eng.global_avgpool_f16(p, 1, 0, 16, p), "bad arguments"),
        (lambda: eng.chan_gate_f16(p, 1, 4, 16, p, p, d_r_ptr=p, views=dict(res_ld=16, res_coff=16)), "leaves its buffer"),
        (lambda: eng.chan_gate_f16(p, 1, 4, 8, p, p), "C % 16"),
        (lambda: eng.seg_argmax_f16(p, 1, 0, 4, p), "bad arguments"),
    ]
    for call, word in calls:
        with pytest.raises(LtkError) as ex:
            call()
        assert ex.value.code == -1 and word in str(ex.value), (word, str(ex.value))
    torch.cuda.synchronize()
    assert int(buf.abs().max()) == 0                 # nothing was launched
    eng.maxpool3x3s2_f16(p, 1, 8, 8, 16, p + 8192)   # and the engine still works
    torch.cuda.synchronize()
