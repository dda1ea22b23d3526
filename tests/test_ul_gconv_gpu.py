"""GPU tests of ul_gconv_kernel (csrc/ul_gconv.hip), the dense conv of the Ultralight program with weights chosen per image, through
ltk_ul_gconv_f16: every case of tests/ul_gconv_cases.py against float64 under the check tests/test_ul_merge_host.py holds a
simulated device to - the bound, the aggregate gate, the guard blocks, images 0 and 2 (same input, same set) byte-identical and
image 1 different, the clamp - plus the report and the refusals.  Engine of its own (module scope)."""
from __future__ import annotations

import numpy as np
import pytest

import ul_gconv_cases as G

pytestmark = pytest.mark.gpu

_CASES = G.cases()


@pytest.fixture(scope="module")
def eng():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from livetalking_amd.engine import Engine
    e = Engine(0)
    yield e
    e.close()


def _run(eng, c, inp, b, sets=None):
    """-> (the y buffer the device left, the report)"""
    import torch
    x = torch.from_numpy(b.x.view(np.int16)).cuda()
    y = torch.from_numpy(b.y.view(np.int16).copy()).cuda()
    r = torch.from_numpy(b.res.view(np.int16)).cuda() if c.res else None
    rep = eng.ul_gconv_f16(x.data_ptr(), c.N, c.H, c.W, c.Cin, inp.w.numpy(), c.sets if sets is None else sets, c.k, c.stride, c.pad,
                           inp.scale.numpy(), inp.shift.numpy(), r.data_ptr() if c.res else 0, c.relu, y.data_ptr(),
                           b.views() if c.view else None)
    torch.cuda.synchronize()
    return y.cpu().numpy().view(np.uint16), rep


@pytest.mark.parametrize("c", _CASES, ids=lambda c: c.id)
def test_case_against_float64(eng, c):
    inp = G.Inputs(c)
    b = G.Buffers(c, inp)
    y, rep = _run(eng, c, inp, b)
    fig = G.check(c, inp, b, y)
    print(f"{c.id}: worst |dev - ref| / tol {fig['worst']:.3f}, rel dev {fig['rel_dev']:.3e} model {fig['rel_mod']:.3e}")
    g = c.geometry()
    assert rep == g, (rep, g)                        # the report names the kernel, tile, grid and blocks


def test_every_image_takes_its_own_set(eng):
    """The same input in all three images: sets [0, 1, 0] give images 0 and 2 byte-identical and image 1 different; [1, 1, 1] gives
    three identical images that equal the former image 1."""
    c = G.Case(3, 10, 10, 48, 32, res=True, relu=True, view=True)
    inp = G.Inputs(c)
    inp.x[1] = inp.x[0]
    inp.res[1] = inp.res[0]
    b = G.Buffers(c, inp)
    y, _ = _run(eng, c, inp, b)
    G.check(c, inp, b, y)
    v = y[:3, b.y_cb0:b.y_cb0 + c.Cout // 16]
    assert np.array_equal(v[0], v[2]) and not np.array_equal(v[0], v[1])
    y1, _ = _run(eng, c, inp, b, sets=[1, 1, 1])
    v1 = y1[:3, b.y_cb0:b.y_cb0 + c.Cout // 16]
    assert np.array_equal(v1[0], v[1]) and np.array_equal(v1[1], v[1]) and np.array_equal(v1[2], v[1])


def test_refusals(eng):
    import torch
    from livetalking_amd._lib import LtkError
    buf = torch.zeros(1 << 16, dtype=torch.int16, device="cuda")
    w = np.zeros((2, 32, 32, 3, 3), np.float32)

    def call(N=3, H=10, W=10, Cin=32, Cout=32, sets=(0, 1, 0), k=1, stride=1, pad=0, views=None):
        wt = np.zeros((2, Cout, Cin, k, k), np.float32) if (Cin % 16 == 0 and Cout % 16 == 0) else w
        return eng.ul_gconv_f16(buf.data_ptr(), N, H, W, Cin, wt, list(sets), k, stride, pad, d_y_ptr=buf.data_ptr(), views=views)

    for kw, word in ((dict(Cin=24), "Cin % 16"), (dict(sets=(0, 2, 0)), "weight set"), (dict(sets=(0, -1, 0)), "weight set"),
                     (dict(N=257, H=1, W=1, sets=[0] * 257), "256"), (dict(k=3, stride=1, pad=1), "3x3 stride 2"),
                     (dict(k=3, stride=2, pad=2), "3x3 stride 2"), (dict(k=1, stride=2), "1x1 stride 1"),
                     (dict(views=dict(x_ld=32, x_coff=16)), "outside the buffer")):
        with pytest.raises(LtkError) as ex:
            call(**kw)
        assert ex.value.code == -1 and word in str(ex.value), (kw, str(ex.value))
    torch.cuda.synchronize()
    assert int(buf.abs().max()) == 0                 # nothing was launched
    rep = call()                                     # and the engine still works
    assert rep["kernel"] == G.KERNEL and rep["grid"] == (4, 1, 3) and rep["blocks"] == 12
