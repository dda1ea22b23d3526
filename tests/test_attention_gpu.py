"""The attention kernels of csrc/nn_kernels.hip on their own, through ltk_attention_f16 (v_transpose_kernel + attn_kernel<3,2,true>,
<4,2,true>, <5,3,true>, <10,5,false>, attn_lds_kernel<3,2>, <5,3>, attn_wide_kernel), against float64 at every tile edge: the cases,
input families, buffers and gates of tests/attention_cases.py, whose rounding model and planted faults tests/test_attention_host.py
holds on the CPU.

Reference and bound: oracle/op_replay.attention_model with the subnormal-probability term on; gates: the replay's two, unchanged -
per element |dev - ref| <= tol with no violator, aggregate rel_l2(dev) <= 2 rel_l2(mod) + 1e-4.  Inputs keep |S| <= 100
(attention_cases.S_CAP, asserted where they are made): the fp32 rounding of the exponent's argument, |S| 2^-23, then stays far below
the 2^-10 of the bound.

Layout, in every case: q, k, v are views into one allocation (one stacked tensor where Tq == Tk) at non-zero first channel blocks,
K's neighbouring channel blocks hold values 1e3 times K's, o goes to the middle of a wider buffer pre-filled with a bit pattern that
has to survive outside the heads' blocks, and the padded channels of a d < d16 head read back as zero.

Every LDS case: the same bytes as the per-wave kernel on the same inputs (what attn_lds_kernel's comment claims) and the same bytes on
a second call (its three-stage ring has raced before).  impl 0, the program's own choice, gives the bytes of the case's kernel.

LTK_ATTN_PARITY_OUT names a file the records are appended to (profiles/attention_parity.txt)."""
from __future__ import annotations

import functools
import os

import numpy as np
import pytest
import torch

import attention_cases as A

pytestmark = pytest.mark.gpu


def _emit(lines):
    for ln in lines:
        print(ln)
    out = os.environ.get("LTK_ATTN_PARITY_OUT")
    if out:
        with open(out, "a") as f:
            f.write("\n".join(lines) + "\n")


@functools.lru_cache(maxsize=4)
def _reference(case_index: int, family: str) -> A.Reference:
    return A.Reference(A.CASES[case_index], family)


def _run(engine, rf: A.Reference, d_in: torch.Tensor, impl: int) -> np.ndarray:
    c, b = rf.c, rf.buf
    d_o = torch.from_numpy(b.empty_o()).cuda()
    view = lambda t, spec: (t.data_ptr() + 2 * spec[0], spec[1], spec[2])
    engine.attention_f16(view(d_in, b.q), view(d_in, b.k), view(d_in, b.v), view(d_o, b.o), c.N, c.heads, c.d16, c.Tq, c.Tk, impl=impl)
    return d_o.cpu().numpy()


@pytest.mark.parametrize("ci", range(len(A.CASES)), ids=[c.id for c in A.CASES])
def test_attention_against_float64(engine, ci):
    case = A.CASES[ci]
    lines, bad = [], []
    for c, family in A.PLAN:
        if c is not case:
            continue
        rf = _reference(ci, family)
        d_in = torch.from_numpy(rf.buf.qkv).cuda()
        o = _run(engine, rf, d_in, c.impl)
        rec, fails = A.check(rf, o)
        bad += fails
        extra = ""
        same = lambda other: "same" if np.array_equal(o, other) else "DIFFERENT"
        if c.impl == 2:
            wave, again = _run(engine, rf, d_in, 1), _run(engine, rf, d_in, 2)
            extra = f"  bytes: per-wave {same(wave)}, second call {same(again)}"
            if not np.array_equal(o, wave):
                bad.append(f"{c.id} {family}: attn_lds_kernel and the per-wave kernel differ in {int((o != wave).sum())} halfs")
                bad += A.check(rf, wave, " (per-wave)")[1]
            if not np.array_equal(o, again):
                bad.append(f"{c.id} {family}: a second call of attn_lds_kernel differs in {int((o != again).sum())} halfs")
        auto = _run(engine, rf, d_in, 0)
        extra += f"{'' if extra else '  bytes:'}{',' if c.impl == 2 else ''} impl 0 {same(auto)}"
        if not np.array_equal(o, auto):
            bad.append(f"{c.id} {family}: impl 0 gives other bytes than {c.kernel}")
        lines.append(A.format_record(c, family, rec, extra))
    _emit(lines)
    assert lines
    assert not bad, "\n".join(bad)


def test_attention_refuses_what_no_kernel_serves(engine):
    from livetalking_amd._lib import LtkError
    t = torch.zeros(1 << 16, dtype=torch.int16, device="cuda")
    t_o = torch.zeros_like(t)
    p, po = t.data_ptr(), t_o.data_ptr()
    ok = dict(q=(p, 8, 0), k=(p, 8, 0), v=(p, 8, 0), o=(po, 8, 0), N=1, heads=2, d16=64, Tq=33, Tk=33, impl=1)

    def refused(**kw):
        a = dict(ok, **kw)
        with pytest.raises(LtkError) as ex:
            engine.attention_f16(a["q"], a["k"], a["v"], a["o"], a["N"], a["heads"], a["d16"], a["Tq"], a["Tk"], impl=a["impl"])
        assert ex.value.code == -1, kw

    for d16 in (0, 16, 32, 40, 96, 128, 256, 1024):
        refused(d16=d16)
    for name in ("N", "heads", "Tq", "Tk"):
        for bad in (0, -1):
            refused(**{name: bad})
    for name in ("q", "k", "v", "o"):
        refused(**{name: (0, 8, 0)})                        # a null pointer
        refused(**{name: (ok[name][0], 8, 1)})              # the heads run past the buffer's channel blocks
        refused(**{name: (ok[name][0], 8, -1)})
    refused(impl=3)
    refused(impl=-1)
    refused(impl=2)                                         # the LDS form: head dims 40 / 80 only,
    refused(impl=2, d16=48, heads=1, Tq=96, Tk=96)          # at least 128 keys,
    refused(impl=2, d16=80, heads=1, Tq=130, Tk=130)        # in whole 64-key tiles
    engine.attention_f16(ok["q"], ok["k"], ok["v"], ok["o"], 1, 2, 64, 33, 33, impl=1)       # and the engine still serves
