"""The non-matrix kernels of csrc/nn_kernels.hip on their own against float64: the three GroupNorm implementations at every instantiation
(ltk_groupnorm_f16_ex: fp16 and e4m3 output, channel views, the segment, member and thread-slot edges of their launch rules), and
layernorm_kernel, geglu_kernel, act_kernel, add_pos_kernel, nchw_to_cb16_kernel, tokens_to_cb16_kernel and vae_post_kernel
(ltk_pointwise_f16) - the cases, input families, buffers and gates of tests/norm_cases.py, whose rounding model, simulated device and planted
faults tests/test_norm_host.py holds on the CPU.

Every (case, family) asserts: the call succeeds; the hook reports the kernel, the segments, the members and the grid the case expects; per
element |dev - ref| inside op_replay's bound with no violator (an e4m3 byte between e4m3(lo) and e4m3(hi)); aggregate rel_l2(dev, ref) <=
2 rel_l2(mod, ref) + 1e-4; every half of the output buffer outside the view still holds the pre-fill pattern; a second call writes the same
bytes; impl 0 writes the same bytes where the case's implementation is the program's choice.

LTK_NORM_PARITY_OUT names a file the records are appended to (profiles/norm_parity.txt)."""
from __future__ import annotations

import os

import numpy as np
import pytest
import torch

import norm_cases as K

pytestmark = pytest.mark.gpu

GROUPS = K.groups()


def _emit(lines):
    for ln in lines:
        print(ln)
    out = os.environ.get("LTK_NORM_PARITY_OUT")
    if out:
        with open(out, "a") as f:
            f.write("\n".join(lines) + "\n")


def _call(engine, rf: K.Reference, d_x, d_y, impl=None):
    """One launch -> the hook's report (None for the pointwise family)."""
    c, b = rf.c, rf.buf
    esz = 1 if c.fp8 else 2
    y_ptr = d_y.data_ptr() + b.y_off * esz
    x_ptr = 0 if d_x is None else d_x.data_ptr() + (b.x_off * 2 if b.x is not None else 0)      # (a bridge's fp32 input has no outer images)
    o = b.opts(c)
    if c.kind == "gn":
        return engine.groupnorm_f16_ex(x_ptr, c.N, c.C, c.P, c.groups, c.eps, rf.gamma.numpy(), rf.beta.numpy(), c.silu, y_ptr,
                                       impl=c.impl if impl is None else impl, out_fp8=c.fp8, out_scale=K.OUT_SCALE, **o)
    op = {"ln": "layernorm", "nchw": "nchw_to_cb16", "tokens": "tokens_to_cb16", "tokens_add": "tokens_to_cb16"}.get(c.kind, c.kind)
    v0 = rf.gamma if c.kind == "ln" else rf.table
    engine.pointwise_f16(op, x_ptr, y_ptr, c.N, c.C, c.P, eps=c.eps, v0=v0.numpy() if v0 is not None else None,
                         v1=rf.beta.numpy() if c.kind == "ln" else None, **o)
    return None


def _run(engine, rf: K.Reference, impl=None):
    """-> (report, the output buffer on the host)"""
    from livetalking_amd._lib import LtkError
    c, b = rf.c, rf.buf
    if b.x is not None:
        d_x = torch.from_numpy(b.x.view(np.int16)).cuda()
    elif rf.src is not None:
        d_x = rf.src.cuda()
    else:
        d_x = None
    d_y = torch.from_numpy(b.initial_y()).cuda()
    try:
        rep = _call(engine, rf, d_x, d_y, impl)
    except LtkError as ex:
        # a HIP error: the device context is gone.  Ending the SESSION is meant, so that nothing more is started on a device that has faulted
        if ex.code == -2:
            pytest.exit(f"{c.id}: {ex}", returncode=3)
        raise
    return rep, d_y.cpu().numpy()


def _one(engine, pi: int):
    rf = K.reference(pi)
    c = rf.c
    name = f"{c.id} {rf.family}"
    rep, y = _run(engine, rf)
    kernel = rep["kernel"] if rep else c.expect
    rec, bad = K.check(rf, y, kernel)
    if rep:
        if (kernel, rep["impl"], rep["segs"], rep["members"], rep["grid"]) != (c.expect, c.impl, c.segs, c.members, c.grid):
            bad.append(f"{name}: launched {kernel!r} impl {rep['impl']} segs {rep['segs']} members {rep['members']} grid {rep['grid']}; the case expects "
                       f"{c.expect!r} impl {c.impl} segs {c.segs} members {c.members} grid {c.grid}")
    _, y2 = _run(engine, rf)
    if not np.array_equal(y, y2):
        bad.append(f"{name}: a second call wrote other bytes")
    if c.kind == "gn" and K.default_impl(c.C, c.P, c.groups) == c.impl:
        rep0, y0 = _run(engine, rf, impl=0)
        if rep0["kernel"] != kernel or not np.array_equal(y, y0):
            bad.append(f"{name}: impl 0 launched {rep0['kernel']!r} and its bytes {'equal' if np.array_equal(y, y0) else 'differ from'} impl {c.impl}'s")
    return K.format_record(rf, kernel, rec), bad


@pytest.mark.parametrize("group", sorted(GROUPS), ids=sorted(GROUPS))
def test_norm_against_float64(engine, group):
    lines, bad = [], []
    for pi in GROUPS[group]:
        ln, fails = _one(engine, pi)
        lines.append(ln)
        bad += fails
    _emit(lines)
    assert lines
    assert not bad, "\n".join(bad)


def test_every_groupnorm_instantiation_is_reported(engine):
    """2 gn_apply, 6 gn_group, 2 gn_coop: the union of what the hook reports over the smallest case per expected kernel."""
    first = {}
    for pi, (ci, _) in enumerate(K.PLAN):
        c = K.CASES[ci]
        if c.kind == "gn" and (c.expect not in first or c.elems < K.CASES[K.PLAN[first[c.expect]][0]].elems):
            first[c.expect] = pi
    seen = {_run(engine, K.reference(pi))[0]["kernel"] for pi in first.values()}
    assert seen == set(K.GN_KERNELS)


def test_groupnorm_refuses_what_it_cannot_serve(engine):
    """A forced impl that does not serve the shape, and a view that is none, come back as LTK_E_INVALID, never as another kernel."""
    from livetalking_amd._lib import LtkError
    x = torch.zeros(1 << 22, dtype=torch.int16, device="cuda")
    y = torch.zeros(1 << 22, dtype=torch.int16, device="cuda")
    for impl, N, C, P, groups, fp8, o, what in K.REFUSALS:
        assert N * (o.get("x_ld") or C) * P <= x.numel()
        with pytest.raises(LtkError) as ex:
            engine.groupnorm_f16_ex(x.data_ptr(), N, C, P, groups, 1e-5, np.ones(C, np.float32), np.zeros(C, np.float32), True, y.data_ptr(), impl=impl,
                                    out_fp8=fp8, out_scale=K.OUT_SCALE, **o)
        assert ex.value.code == -1, what
    rep = engine.groupnorm_f16_ex(x.data_ptr(), 2, 32, 100, 2, 1e-5, np.ones(32, np.float32), np.zeros(32, np.float32), True, y.data_ptr(), impl=2)
    assert rep["kernel"] == "gn_group_kernel<8,256,false>"          # and the engine still serves
    with pytest.raises(LtkError) as ex:
        engine.pointwise_f16("layernorm", x.data_ptr(), y.data_ptr(), 1, 24, 10, v0=np.ones(24, np.float32), v1=np.zeros(24, np.float32))
    assert ex.value.code == -1


@pytest.mark.parametrize("P", K.VAE_POST_P)
def test_vae_post_writes_a_ragged_last_block(engine, P):
    """vae_post_kernel wrote a block's 768 bytes only where all 256 pixels exist: with P % 256 != 0 a frame's last pixels stayed unwritten.
    Every pixel of every frame has to hold the reference's bytes, and nothing behind the last frame is touched."""
    x, want = K.vae_post_case(P)
    N = x.shape[0]
    d_x = torch.from_numpy(x.view(np.int16)).cuda()
    d_y = torch.full((N * P * 3 + 1024,), 0x5A, dtype=torch.uint8, device="cuda")
    engine.pointwise_f16("vae_post", d_x.data_ptr(), d_y.data_ptr(), N, 3, P)
    got = d_y.cpu().numpy()
    assert np.array_equal(got[:N * P * 3].reshape(N, P, 3), want)
    assert bool((got[N * P * 3:] == 0x5A).all())
