"""GPU tests of the fused inverted residual (csrc/ul_ir.hip): ul_ir_kernel on its own through ltk_ul_ir_f16 - every case of
tests/ul_ir_cases.py stage by stage against float64 under the check tests/test_ul_ir_host.py holds a simulated device to, tapped
and untapped, each image alone against the same image inside the launch, the refusals - and inside the Ultralight program under
knob UL_FUSE_IR: the listing, every tap and the frames against float64, a frame's bytes whatever its company, the way back to knob 0
and the grouped path that ignores the knob.  Engines of their own (module scope)."""
from __future__ import annotations

import functools
import types

import numpy as np
import pytest

import synth_inputs as synth
import ul_ir_cases as K
import ultralight_ref as ref

pytestmark = pytest.mark.gpu

FULL_HW = (120, 200)


@pytest.fixture(scope="module")
def eng():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from livetalking_amd.engine import Engine
    e = Engine(0)
    yield e
    e.close()


@functools.lru_cache(maxsize=None)
def _tile():
    return K.planner()


@functools.lru_cache(maxsize=None)
def _cases():
    return K.cases(*_tile())


def _run(eng, c, inp, b, tap=True):
    """-> (y, e1, e2 as the device left them, the report)"""
    import torch
    dev = lambda a: torch.from_numpy(a.view(np.int16).copy()).cuda()
    x, y, e1, e2 = dev(b.x), dev(b.y), dev(b.e1), dev(b.e2)
    r = dev(b.res) if c.res else None
    rep = eng.ul_ir_f16(x.data_ptr(), c.N, c.H, c.W, c.Cin, c.stride, inp.w1.numpy(), inp.wd.numpy(), inp.w2.numpy(),
                        (inp.s1.numpy(), inp.b1.numpy()), (inp.sd.numpy(), inp.bd.numpy()), (inp.s2.numpy(), inp.b2.numpy()),
                        r.data_ptr() if c.res else 0, y.data_ptr(), b.views() if c.view else None,
                        e1.data_ptr() if tap else 0, e2.data_ptr() if tap else 0)
    torch.cuda.synchronize()
    back = lambda t: t.cpu().numpy().view(np.uint16)
    return back(y), back(e1), back(e2), rep


def _alone(c, inp, n):
    """Image n of a case as a case of its own."""
    c1 = K.Case(1, c.H, c.W, c.Cin, c.Cout, stride=c.stride, mid=c.mid, res=c.res, view=c.view, big=c.big)
    i1 = K.Inputs(c1)
    for name in ("w1", "wd", "w2", "s1", "b1", "sd", "bd", "s2", "b2"):
        setattr(i1, name, getattr(inp, name))
    i1.x = inp.x[n:n + 1].clone()
    i1.res = inp.res[n:n + 1].clone() if c.res else None
    return c1, i1


@pytest.mark.parametrize("i", range(K.N_CASES))
def test_case_against_float64(eng, i):
    c = _cases()[i]
    TH, TW, MC = _tile()
    inp = K.Inputs(c)
    b = K.Buffers(c, inp)
    y, e1, e2, rep = _run(eng, c, inp, b)
    figs = K.check(c, inp, b, y, e1, e2)
    for st, f in figs.items():
        print(f"{c.id} {st}: worst |dev - ref| / tol {f['worst']:.3f}, rel dev {f['rel_dev']:.3e} model {f['rel_mod']:.3e}")
    want = c.geometry(TH, TW, MC, True)
    assert {k: rep[k] for k in want} == want, (rep, want)
    from livetalking_amd.engine import Engine
    assert rep == Engine.ul_ir_plan(c.N, c.H, c.W, c.Cin, c.mid, c.Cout, c.stride, c.res, True, views=b.views() if c.view else None)
    # the untapped instantiation: the same y bytes, the tap buffers untouched
    y2, e1u, e2u, rep2 = _run(eng, c, inp, b, tap=False)
    assert np.array_equal(y, y2), f"{c.id}: tapped and untapped runs differ in y"
    assert (e1u == K.PATTERN).all() and (e2u == K.PATTERN).all() and rep2["kernel"] == c.geometry(TH, TW, MC, False)["kernel"]
    # batch independence: image 1 alone leaves the bytes it has inside the launch of three
    if c.N == 3:
        c1, i1 = _alone(c, inp, 1)
        b1 = K.Buffers(c1, i1)
        ya, e1a, e2a, _ = _run(eng, c1, i1, b1)
        cb = slice(b.y_cb0, b.y_cb0 + c.Cout // 16)
        assert np.array_equal(ya[0, cb], y[1, cb]) and np.array_equal(e1a[0], e1[1]) and np.array_equal(e2a[0], e2[1]), f"{c.id}: image 1 alone differs"


def test_refusals(eng):
    import torch
    from livetalking_amd._lib import LtkError
    buf = torch.zeros(1 << 18, dtype=torch.int16, device="cuda")

    def call(N=3, H=9, W=9, Cin=32, mid=64, Cout=32, stride=1, res=False, views=None, e1=False, e2=False):
        z = lambda *s: np.zeros(s, np.float32)
        p = buf.data_ptr()
        return eng.ul_ir_f16(p, N, H, W, Cin, stride, z(mid, Cin), z(mid, 3, 3), z(Cout, mid), d_res_ptr=p if res else 0, d_y_ptr=p, views=views,
                             d_e1_ptr=p if e1 else 0, d_e2_ptr=p if e2 else 0)

    for kw, word in ((dict(Cin=24), "multiples of 16"), (dict(mid=40), "multiples of 16"), (dict(Cout=24), "multiples of 16"),
                     (dict(stride=3), "stride"), (dict(N=257, H=1, W=1), "256 images"), (dict(res=True, Cout=16), "residual"),
                     (dict(res=True, stride=2), "residual"), (dict(views=dict(x_ld=32, x_coff=16)), "view"),
                     (dict(views=dict(y_ld=32, y_coff=16)), "view"), (dict(res=True, views=dict(res_ld=32, res_coff=16)), "view"),
                     (dict(Cout=512), "accumulators"), (dict(Cout=80), "accumulators"), (dict(e1=True), "both tap buffers")):
        with pytest.raises(LtkError) as ex:
            call(**kw)
        assert ex.value.code == -1 and word in str(ex.value), (kw, str(ex.value))
    torch.cuda.synchronize()
    assert int(buf.abs().max()) == 0                 # nothing was launched
    rep = call()                                     # and the engine still works
    assert rep["accepted"] and rep["kernel"] == "ul_ir_kernel<2,false>" and rep["grid"] == (2, 2, 3)


# ---------------------------------------------------------------------------------------------------- the program
class fused:
    """Knob UL_FUSE_IR for the block, restored on the way out."""

    def __init__(self, value=1):
        self.value = value

    def __enter__(self):
        from livetalking_amd.engine import Engine
        Engine.set_knob("UL_FUSE_IR", self.value)

    def __exit__(self, *exc):
        from livetalking_amd.engine import Engine
        Engine.set_knob("UL_FUSE_IR", 0)


class one_summation_order:
    """Knob SPLITK = 0 for the block (tests/test_ul_merge_gpu.py): the convs that stay unfused no longer split their channel loop by
    the launch's frame count."""

    def __enter__(self):
        from livetalking_amd.engine import Engine
        Engine.set_knob("SPLITK", 0)

    def __exit__(self, *exc):
        from livetalking_amd.engine import Engine
        Engine.set_knob("SPLITK", 1)


FUSED = ref.FUSED            # (tests/test_ul_program_host.py checks the same list without a GPU)


@pytest.fixture(scope="module")
def prog(eng):
    """Seed 1234 weights over the three-face golden bank, the float64 reference of its three frames, and the frames of a B = 2 call
    made BEFORE any test touches the knob."""
    sd = synth.ultralight_state_dict(1234)
    img6, feat = synth.ultralight_inputs(3, 1234)
    taps = {}
    pred = ref.forward(sd, img6, feat, taps=taps)
    model = ref.forward(sd, img6, feat, fp16_model=True)
    faces = synth.ultralight_faces(3, 1234)
    frames, _, coords = synth.ultralight_avatar(3, FULL_HW, seed=3)
    aid = eng.register_ultralight_avatar(sd, faces, frames, coords, max_frames=17)
    p = types.SimpleNamespace(aid=aid, img6=img6, feat=feat, taps=taps, frames=ref.frames_u8(pred), model_frames=ref.frames_u8(model))
    p.ops0 = eng.ultralight_ops(aid)
    p.before = [_infer(eng, p, 2) for _ in range(3)]          # eager, captured, replayed
    p.before_grouped = _merged(eng, p, [(0, 2)], mode=2)[0]
    return p


def _mirror(size, index):
    turn, res = divmod(index, size)
    return res if turn % 2 == 0 else size - res - 1


def _order(index, B):
    return [_mirror(3, index + i) for i in range(B)]


def _infer(eng, p, B, index=0):
    import torch
    d_feat = torch.from_numpy(np.ascontiguousarray(p.feat[_order(index, B)])).cuda()
    d_pred = torch.zeros(B, 160, 160, 3, dtype=torch.uint8, device="cuda")
    eng.ultralight_infer([(p.aid, index, B, d_feat.data_ptr(), d_pred.data_ptr())])
    return d_pred.cpu().numpy()


def _merged(eng, p, reqs, mode=1):
    """reqs: (index, batch); every frame takes the features of its bank frame.  -> frames per request"""
    import torch
    feats = [torch.from_numpy(np.ascontiguousarray(p.feat[_order(i, n)])).cuda() for i, n in reqs]
    preds = [torch.zeros(n, 160, 160, 3, dtype=torch.uint8, device="cuda") for _, n in reqs]
    eng.ultralight_infer_merged([(p.aid, i, n, f.data_ptr(), q.data_ptr()) for (i, n), f, q in zip(reqs, feats, preds)], mode=mode)
    return [q.cpu().numpy() for q in preds]


def test_knob_on_lists_60_ops_and_every_tap_matches_float64(eng, prog):
    assert len(prog.ops0) == 86 and all(t != 15 for _, t in prog.ops0)
    with fused():
        ops = eng.ultralight_ops(prog.aid)
        assert len(ops) == 60
        assert [n for n, t in ops if t == 15] == [b + ".conv.6" for b in FUSED]
        # the listing is the unfused one with each fused block's expand and depthwise conv taken out
        gone = {b + s for b in FUSED for s in (".conv.0", ".conv.3")}
        assert [n for n, _ in ops] == [n for n, _ in prog.ops0 if n not in gone]
        B = 2
        eng.debug_capture(True)
        try:
            eng.ultralight_forward_host(prog.aid, prog.img6[:B], prog.feat[:B])
            compared, worst = set(), (0.0, "")
            for name, _ in ops:
                if name not in prog.taps:
                    continue
                want = prog.taps[name][:B]
                got = eng.debug_get(name, want.shape)
                rel = float(np.linalg.norm(got - want) / np.linalg.norm(want))
                worst = max(worst, (rel, name))
                assert rel <= 1e-2, f"{name}: rel L2 {rel:.3e}"
                compared.add(name)
            print(f"worst tap {worst[1]}: rel L2 {worst[0]:.3e}; {len(compared)} compared")
            assert {b + ".conv.6" for b in FUSED} <= compared and len(compared) >= 55
            from livetalking_amd._lib import LtkError
            for name in sorted(gone):                       # absent, not zeros
                with pytest.raises(LtkError):
                    eng.debug_get(name, prog.taps[name][:B].shape)
        finally:
            eng.debug_capture(False)
    assert len(eng.ultralight_ops(prog.aid)) == 86


@pytest.mark.parametrize("B", [2, 17])
def test_fused_frames_against_float64(eng, prog, B):
    """The gates of tests/test_ultralight_gpu.py::test_infer_frames_against_float64 with the knob on."""
    with fused():
        got = _infer(eng, prog, B)
    order = _order(0, B)
    want = prog.frames[order]
    m_mx, m_psnr, m_share = ref.frame_stats(prog.model_frames[order], want)
    d_mx, d_psnr, d_share = ref.frame_stats(got, want)
    print(f"B {B}: model {m_mx} LSB {m_psnr:.2f} dB {m_share:.4f} | device {d_mx} LSB {d_psnr:.2f} dB {d_share:.4f}")
    assert d_mx <= m_mx + 1 and d_psnr >= m_psnr - 1.5 and d_share <= 1.5 * m_share
    assert d_mx <= 2 and d_psnr >= 57.5 and d_share < 0.12


def test_a_frames_bytes_do_not_depend_on_its_company(eng, prog):
    """Bank frame 1 with its features: alone, as the second frame of a 3-frame call, and inside a merged per-avatar pass of 1 + 2 + 3
    frames.  The fused blocks sum in one order at every frame count; the convs that stay unfused split their channel loop by the
    frame count of a frame's own call (ul_conv_as_own_calls), so the three-way equality is taken under SPLITK = 0, and with the
    default SPLITK the 1-frame request of the merged pass (a 6-frame launch of every fused block) has to equal the 1-frame call."""
    with fused():
        solo = _infer(eng, prog, 1, index=1)
        merged = _merged(eng, prog, [(1, 1), (0, 2), (0, 3)])
        assert np.array_equal(merged[0], solo), "the 1-frame request of a merged pass differs from its own call"
        with one_summation_order():
            solo0 = _infer(eng, prog, 1, index=1)[0]
            in3 = _infer(eng, prog, 3, index=0)[1]
            m = _merged(eng, prog, [(0, 1), (0, 2), (0, 3)])
            assert np.array_equal(in3, solo0), "frame 1 of a 3-frame call differs from the 1-frame call"
            assert np.array_equal(m[1][1], solo0), "frame 1 inside the merged 1 + 2 + 3 pass differs from the 1-frame call"
            assert np.array_equal(m[2][1], solo0)


def test_back_to_knob_0_is_the_parent_pass(eng, prog):
    """86 ops, frames byte-identical to the run made before the knob was first touched, and a graph captured under one knob value is
    not replayed under the other: the third call under each value equals the first (eager) call under that value."""
    assert all(np.array_equal(f, prog.before[0]) for f in prog.before)
    with fused():
        on = [_infer(eng, prog, 2) for _ in range(3)]           # eager, captured, replayed
        assert len(eng.ultralight_ops(prog.aid)) == 60
        assert eng.program_graph_count() >= 1
    off = [_infer(eng, prog, 2)]
    assert eng.program_graph_count() == 0                       # the knob changed: every captured pass went, this call ran eagerly
    off += [_infer(eng, prog, 2) for _ in range(2)]
    assert eng.program_graph_count() == 1
    with fused():
        on2 = _infer(eng, prog, 2)
    assert eng.ultralight_ops(prog.aid) == prog.ops0 and len(prog.ops0) == 86
    for f in off:
        assert np.array_equal(f, prog.before[0]), "knob 0 after knob 1 differs from the pass before the knob was touched"
    for f in on[1:] + [on2]:
        assert np.array_equal(f, on[0]), "knob 1: a replayed pass differs from the eager one"
    mx, _, share = ref.frame_stats(on[0], prog.before[0])
    print(f"knob 1 against knob 0 at B = 2: {mx} LSB on {share:.4f} of the bytes")


def test_grouped_path_ignores_the_knob(eng, prog):
    with fused():
        got = _merged(eng, prog, [(0, 2)], mode=2)[0]
    assert np.array_equal(got, prog.before_grouped)
