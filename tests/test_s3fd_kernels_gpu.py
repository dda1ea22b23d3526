"""GPU: the face detector's own kernels (csrc/s3fd_kernels.hip) through their stand-alone hooks, each against float64 on the
device's own inputs under the gates of tests/s3fd_cases.py (tests/test_face_detect_host.py holds a simulated device with planted
faults to the same gates): the stem at odd sizes, on a one-pixel-wide image and inside a channel view between guard blocks; the 2x2
pool at odd and even maps; L2Norm at C = 256 and 512 with values an fp16 square cannot hold and an all-zero pixel; the detect kernel at
every level with the max-out on and off, a score exactly at the threshold, a cap below the hits and two images' lists; the refusals.
Engine of its own (module scope)."""
from __future__ import annotations

import numpy as np
import pytest

import s3fd_cases as FD

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
    bgr = torch.from_numpy(c.bgr).cuda()
    y = _dev(_out_buf(c.N, 4, c.H, c.W, view))
    eng.s3fd_stem_f16(bgr.data_ptr(), c.N, c.H, c.W, c.w, c.bias, y.data_ptr(), dict(y_ld=96, y_coff=16) if view else None)
    torch.cuda.synchronize()
    return FD.from_cb16(_out_view(y, 4, view), 64)


@pytest.mark.parametrize("shape", FD.STEM_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_stem_against_float64(eng, shape):
    c = FD.Stem(*shape)
    ref, tol = c.ref_tol()
    dev = _run_stem(eng, c, view=shape[1] == 16)
    fig = FD.check(dev, ref, c.model(), tol)
    print(f"stem {shape}: worst |dev - ref| / tol {fig['worst']:.3f}, rel dev {fig['rel_dev']:.3e} model {fig['rel_mod']:.3e}, "
          f"equals the model: {np.array_equal(dev, c.model())}")


def test_stem_image_alone_and_in_company(eng):
    c3, c1 = FD.Stem(3, 16, 16), FD.Stem(1, 16, 16)
    c1.bgr, c1.w, c1.bias = c3.bgr[1:2].copy(), c3.w, c3.bias
    a, b = _run_stem(eng, c3), _run_stem(eng, c1)
    assert np.array_equal(a[1:2], b) and np.array_equal(_run_stem(eng, c3), a)


# ------------------------------------------------------------------------------------------ max pool
@pytest.mark.parametrize("shape", FD.POOL_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_maxpool_is_exact(eng, shape):
    import torch
    N, C, H, W = shape
    view = H == 7
    x = FD.pool_input(*shape)
    ref = FD.pool_ref(x)
    assert ref.shape[2:] == (H // 2, W // 2)
    d_x = _dev(_in_view(FD.to_cb16(x), view))
    y = _dev(_out_buf(N, C // 16, H // 2, W // 2, view))
    ld = C + 32
    eng.maxpool2x2s2_f16(d_x.data_ptr(), N, H, W, C, y.data_ptr(), dict(x_ld=ld, x_coff=16, y_ld=ld, y_coff=16) if view else None)
    torch.cuda.synchronize()
    assert np.array_equal(FD.from_cb16(_out_view(y, C // 16, view), C), ref)


# ------------------------------------------------------------------------------------------ L2Norm
@pytest.mark.parametrize("shape", FD.NORM_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_l2norm_against_float64(eng, shape):
    import torch
    N, C, P = shape
    view = C == 256
    x, w = FD.norm_input(*shape)
    ref, tol = FD.norm_ref_tol(x, w)
    d_x = _dev(_in_view(FD.to_cb16(x), view))
    y = _dev(_out_buf(N, C // 16, P, 1, view))
    ld = C + 32
    eng.l2norm_f16(d_x.data_ptr(), N, P, C, w, y.data_ptr(), dict(x_ld=ld, x_coff=16, y_ld=ld, y_coff=16) if view else None)
    torch.cuda.synchronize()
    dev = FD.from_cb16(_out_view(y, C // 16, view), C)
    fig = FD.check(dev, ref, FD.norm_model(x, w), tol)
    assert (dev[:, :, 0] == 0).all()                                   # the all-zero pixel: eps alone in the denominator, no NaN
    print(f"l2norm {shape}: worst |dev - ref| / tol {fig['worst']:.3f}, rel dev {fig['rel_dev']:.3e} model {fig['rel_mod']:.3e}")


# ------------------------------------------------------------------------------------------ detect
def _run_detect(eng, x, maxout, level, thresh, cap, view=False, counts0=None):
    import torch
    N, _, H, W = x.shape
    d_x = _dev(_in_view(FD.to_cb16(x), view))
    recs = torch.full((N + 1, cap, FD.REC_WORDS), 0x5A5A5A5A, dtype=torch.int32, device="cuda")       # a guard list behind the last image's
    counts = torch.zeros(N + 1, dtype=torch.int32, device="cuda") if counts0 is None else torch.tensor(counts0, dtype=torch.int32, device="cuda")
    eng.s3fd_detect_f16(d_x.data_ptr(), N, H, W, maxout, level, thresh, recs.data_ptr(), cap, counts.data_ptr(),
                        dict(x_ld=48, x_coff=16) if view else None)
    torch.cuda.synchronize()
    r, c = recs.cpu().numpy().view(np.uint32), counts.cpu().numpy().view(np.uint32)
    assert (r[N] == 0x5A5A5A5A).all() and c[N] == (0 if counts0 is None else counts0[N]), "the launch wrote behind its lists"
    return r[:N], c[:N]


@pytest.mark.parametrize("level,maxout", FD.DETECT_CASES, ids=lambda v: str(int(v)))
def test_detect_against_float64(eng, level, maxout):
    x = FD.detect_input(level, maxout)
    ref = FD.detect_ref(x, maxout, level, 0.05)
    assert all(len(rows) >= 8 for rows, _ in ref) and set(ref[0][0]) != set(ref[1][0])
    cap = 128
    recs, counts = _run_detect(eng, x, maxout, level, 0.05, cap, view=level == 1)
    got = FD.unpack_records(recs, counts, cap)
    fig = FD.detect_check(got, ref)
    for n, (rows, edge) in enumerate(ref):                               # unused slots of a list stay as they were
        assert abs(int(counts[n]) - len(rows)) <= len(edge) and (recs[n, counts[n]:] == 0x5A5A5A5A).all()
    print(f"detect level {level} maxout {maxout}: {[int(c) for c in counts]} records, score error {fig['worst_s']:.3f} of its bound, "
          f"box error {fig['worst_b']:.3f}")


def test_detect_score_at_the_threshold_is_not_a_candidate(eng):
    x = FD.detect_input(2, False)
    x[:, 0:2, 4, 5] = 1.25                               # equal logits: the score is 0.5 exactly, in fp32 as in float64
    x[0, 1, 4, 6] = x[0, 0, 4, 6] + 2.0 ** -6            # and the next one above it
    ref = FD.detect_ref(x, False, 2, 0.5)
    key = (2 << 28) | (4 << 14) | 5
    assert key not in ref[0][0] and key + 1 in ref[0][0]
    recs, counts = _run_detect(eng, x, False, 2, 0.5, 128)
    got = FD.unpack_records(recs, counts, 128)
    FD.detect_check(got, ref)
    assert all(key not in [k for k, _ in g] for g in got) and key + 1 in [k for k, _ in got[0]]


def test_detect_cap_below_the_hits_and_a_counter_that_is_not_reset(eng):
    x = FD.detect_input(1, False)
    ref = FD.detect_ref(x, False, 1, 0.05)
    hits = [len(rows) for rows, _ in ref]
    assert min(hits) > 8 and not any(edge for _, edge in ref)
    recs, counts = _run_detect(eng, x, False, 1, 0.05, 8)
    assert [int(c) for c in counts] == hits                      # the counter goes on past the cap: the host sees the overflow
    FD.detect_check(FD.unpack_records(recs, counts, 8), ref, cap=8)
    # a second level appends behind what the lists hold: image 0's starts at 3, image 1's is already full
    recs, counts = _run_detect(eng, x, False, 1, 0.05, 8, counts0=[3, 8, 0])
    assert [int(c) for c in counts] == [3 + hits[0], 8 + hits[1]]
    assert (recs[0, :3] == 0x5A5A5A5A).all() and (recs[1] == 0x5A5A5A5A).all()
    tail = [[(int(r[0]), np.ascontiguousarray(r[1:]).view(np.float32).astype(np.float64)) for r in recs[0, 3:]], []]
    FD.detect_check(tail, ref, cap=5)


# ------------------------------------------------------------------------------------------ refusals
def test_refusals(eng):
    import torch
    from livetalking_amd._lib import LtkError
    buf = torch.zeros(1 << 16, dtype=torch.int16, device="cuda")
    p = buf.data_ptr()
    w = np.zeros((64, 3, 3, 3), np.float32)
    w256 = np.ones(256, np.float32)
    calls = [
        (lambda: eng.s3fd_stem_f16(p, 1, 0, 8, w, d_y_ptr=p), "bad arguments"),
        (lambda: eng.s3fd_stem_f16(p, 1, 8, 8, w, d_y_ptr=p, views=dict(y_ld=64, y_coff=16)), "leaves its buffer"),
        (lambda: eng.s3fd_stem_f16(p, 1, 8, 8, w, d_y_ptr=p, views=dict(y_ld=72)), "multiples of 16"),
        (lambda: eng.s3fd_stem_f16(p, 1, 8, 8, w, d_y_ptr=p, views=dict(act=1)), "only the channel views"),
        (lambda: eng.maxpool2x2s2_f16(p, 1, 8, 8, 24, p), "C % 16"),
        (lambda: eng.maxpool2x2s2_f16(p, 1, 1, 8, 16, p), "smaller than the window"),
        (lambda: eng.maxpool2x2s2_f16(p, 1, 8, 8, 32, p, dict(x_ld=32, x_coff=16)), "leaves its buffer"),
        (lambda: eng.l2norm_f16(p, 1, 0, 256, w256, p), "bad arguments"),
        (lambda: eng.l2norm_f16(p, 1, 4, 256, w256, p, dict(y_ld=256, y_coff=16)), "leaves its buffer"),
        (lambda: eng.s3fd_detect_f16(p, 1, 4, 4, False, 6, 0.05, p, 8, p), "level"),
        (lambda: eng.s3fd_detect_f16(p, 1, 4, 4, False, 0, 1.0, p, 8, p), "thresh"),
        (lambda: eng.s3fd_detect_f16(p, 1, 4, 4, False, 0, 0.05, p, 0, p), "bad arguments"),
        (lambda: eng.s3fd_detect_f16(p, 1, 4, 4, False, 0, 0.05, p, 8, p, dict(x_ld=16, x_coff=16)), "leaves its buffer"),
    ]
    for call, word in calls:
        with pytest.raises(LtkError) as ex:
            call()
        assert ex.value.code == -1 and word in str(ex.value), (word, str(ex.value))
    torch.cuda.synchronize()
    assert int(buf.abs().max()) == 0                 # nothing was launched
    eng.maxpool2x2s2_f16(p, 1, 8, 8, 16, p + 8192)   # and the engine still works
    torch.cuda.synchronize()
