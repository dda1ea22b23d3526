"""CPU tests of the merged Ultralight pass: the call planner (ltk_debug_ul_merge_plan, no GPU) against a Python restatement, the ABI and
argument validation of the new entries, the scheduler kind "ultralight" over a fake engine, and the gates of tests/ul_gconv_cases.py and
tests/ul_merge_cases.py against simulated devices with one fault planted at a time - the gates the GPU files hold the device to."""
from __future__ import annotations

import ctypes as C
import os
import re
import threading

import numpy as np
import pytest

import ul_gconv_cases as G
import ul_merge_cases as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID = -1


# ------------------------------------------------------------------ planner
def _plan(reqs, cap, mode=0, grouped_ok=True, knob=0):
    from livetalking_amd.engine import Engine
    got = Engine.ul_merge_plan(reqs, cap, mode, grouped_ok, knob)
    want = M.expected_plan(reqs, cap, mode, grouped_ok, bool(knob))
    assert got == want, (reqs, cap, mode, got, want)
    # every frame of every request once, in order; a request's spans are contiguous; no pass past the arena
    seen = {r: [] for r in range(len(reqs))}
    for path, av, nf, spans in got:
        assert 0 < nf <= cap and sum(s[2] for s in spans) == nf
        at = 0
        for r, first, count, where in spans:
            assert where == at and count > 0
            at += count
            seen[r] += list(range(first, first + count))
            assert path == M.GROUPED or reqs[r][0] == av
        assert [s[0] for s in spans] == sorted(s[0] for s in spans)            # request order inside a pass
    assert all(seen[r] == list(range(reqs[r][1])) for r in seen)
    return got


def test_plan_of_one_request_is_the_single_request_plan():
    """ltk_ultralight_infer runs request r as passes of min(cap, rest) frames of its avatar: graph key (avatar, nf)."""
    for batch, cap in ((3, 17), (16, 16), (17, 16), (40, 16), (1, 1)):
        for mode, knob in ((0, 0), (0, 1), (1, 0)):
            got = _plan([(5, batch)], cap, mode, True, knob)
            assert [(p, a, nf) for p, a, nf, _ in got] == [(M.PER_AVATAR, 5, min(cap, batch - f0)) for f0 in range(0, batch, cap)]
            assert [s for _, _, _, s in got] == [[(0, f0, min(cap, batch - f0), 0)] for f0 in range(0, batch, cap)]


def test_plan_one_avatar_three_requests_is_one_pass():
    got = _plan([(2, 1), (2, 2), (2, 3)], 17)
    assert got == [(M.PER_AVATAR, 2, 6, [(0, 0, 1, 0), (1, 0, 2, 1), (2, 0, 3, 3)])]
    assert _plan([(2, 1), (2, 2), (2, 3)], 17, 0, True, 1) == got                  # the knob is about several avatars


def test_plan_splits_a_request_at_the_pass_boundary():
    got = _plan([(2, 3), (2, 2), (2, 1), (2, 1)], 4)
    assert got == [(M.PER_AVATAR, 2, 4, [(0, 0, 3, 0), (1, 0, 1, 3)]), (M.PER_AVATAR, 2, 3, [(1, 1, 1, 0), (2, 0, 1, 1), (3, 0, 1, 2)])]
    got = _plan([(2, 3), (9, 2), (2, 2)], 4, 2)
    assert got == [(M.GROUPED, -1, 4, [(0, 0, 3, 0), (1, 0, 1, 3)]), (M.GROUPED, -1, 3, [(1, 1, 1, 0), (2, 0, 2, 1)])]


def test_plan_two_avatars_interleaved():
    reqs = [(4, 2), (8, 1), (4, 1)]                                               # a, b, a
    per_avatar = [(M.PER_AVATAR, 4, 3, [(0, 0, 2, 0), (2, 0, 1, 2)]), (M.PER_AVATAR, 8, 1, [(1, 0, 1, 0)])]
    grouped = [(M.GROUPED, -1, 4, [(0, 0, 2, 0), (1, 0, 1, 2), (2, 0, 1, 3)])]
    assert _plan(reqs, 17, 0, True, 0) == per_avatar
    assert _plan(reqs, 17, 0, True, 1) == grouped
    assert _plan(reqs, 17, 0, False, 1) == per_avatar                             # knob on, no grouped path: the per-avatar form
    assert _plan(reqs, 17, 1, True, 1) == per_avatar
    assert _plan(reqs, 17, 2, True, 0) == grouped
    assert _plan([(8, 1), (4, 2), (8, 2)], 17, 1)[0][1] == 8                       # avatars in order of first appearance


def test_plan_256_and_257_frames():
    reqs = [(1 + r % 2, 16) for r in range(16)]
    assert [(p, nf) for p, _, nf, _ in _plan(reqs, 256, 2)] == [(M.GROUPED, 256)]
    assert [(p, a, nf) for p, a, nf, _ in _plan(reqs, 256, 1)] == [(M.PER_AVATAR, 1, 128), (M.PER_AVATAR, 2, 128)]
    got = _plan(reqs + [(1, 1)], 256, 2)
    assert [(p, nf) for p, _, nf, _ in got] == [(M.GROUPED, 256), (M.GROUPED, 1)] and got[1][3] == [(16, 0, 1, 0)]
    got = _plan([(3, 257)], 256)
    assert [(nf, s) for _, _, nf, s in got] == [(256, [(0, 0, 256, 0)]), (1, [(0, 256, 1, 0)])]


def test_plan_follows_the_process_knob():
    """grouped_knob = -1 reads knob UL_GROUPED, as ltk_ultralight_infer_merged does."""
    from livetalking_amd.engine import Engine
    reqs = [(4, 2), (8, 1)]
    try:
        Engine.set_knob("UL_GROUPED", 1)
        assert Engine.ul_merge_plan(reqs, 17, 0, True, -1) == M.expected_plan(reqs, 17, 0, True, True)
        Engine.set_knob("UL_GROUPED", 0)
        assert Engine.ul_merge_plan(reqs, 17, 0, True, -1) == M.expected_plan(reqs, 17, 0, True, False)
    finally:
        Engine.set_knob("UL_GROUPED", int(os.environ.get("LTK_UL_GROUPED", "0")))


# ------------------------------------------------------------------ ABI
def test_entries_and_report_struct():
    from livetalking_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "ltk.h")).read()
    lib = _lib.load()
    for name in ("ltk_ultralight_infer_merged", "ltk_ultralight_info", "ltk_debug_ul_merge_plan", "ltk_ul_gconv_f16"):
        assert re.search(r"\bint\s+" + name + r"\s*\(", hdr), f"{name} is not declared in include/ltk.h"
        assert name in _lib.SYMBOLS and getattr(lib, name) is not None
    body = re.search(r"typedef struct ltk_ul_merge_report \{(.*?)\} ltk_ul_merge_report;", hdr, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    names = [re.match(r"\s*int\s+(\w+)", d).group(1) for d in body.split(";") if d.strip()]
    assert names == [f[0] for f in _lib.UlMergeReport._fields_] == ["n_passes", "n_avatars", "grouped", "frames", "path", "nf", "avatar"]
    assert int(re.search(r"#define LTK_UL_MERGE_MAX_PASSES (\d+)", hdr).group(1)) == _lib.UL_MERGE_MAX_PASSES
    assert C.sizeof(_lib.UlMergeReport) == 4 * (4 + 3 * _lib.UL_MERGE_MAX_PASSES)
    assert "UL_GROUPED" in open(os.path.join(ROOT, "livetalking_amd", "csrc", "tune.h")).read()


def test_argument_validation_without_a_gpu():
    """Every request is checked before the engine is touched: a bad one is LTK_E_INVALID and named, also with no engine at all."""
    from livetalking_amd import _lib
    lib = _lib.load()
    buf = (C.c_float * 4)()

    def call(nreq, mode=0, **bad):
        reqs = (_lib.UlReq * max(nreq, 1))()
        for r in reqs:
            r.avatar, r.index, r.batch, r.d_feat, r.d_pred = 1, 0, 2, C.addressof(buf), C.addressof(buf)
        for k, v in bad.items():
            setattr(reqs[-1], k, v)
        return lib.ltk_ultralight_infer_merged(None, reqs, nreq, mode, None, None)

    assert lib.ltk_ultralight_infer_merged(None, None, 1, 0, None, None) == INVALID and b"bad arguments" in lib.ltk_last_error()
    assert call(0) == INVALID and call(-1) == INVALID and call(2, mode=3) == INVALID and call(2, mode=-1) == INVALID
    for bad in (dict(batch=0), dict(batch=-3), dict(index=-1), dict(d_feat=None), dict(d_pred=None)):
        assert call(3, **bad) == INVALID, bad
        assert b"bad request 2" in lib.ltk_last_error(), bad
    assert call(3) == INVALID and b"bad arguments" in lib.ltk_last_error()            # good requests, no engine
    assert lib.ltk_ultralight_info(None, None, None, None, None) == INVALID
    # the planner
    one = (C.c_int * 1)(1)
    out = [(C.c_int * 8)() for _ in range(8)]
    n1, n2 = C.c_int(), C.c_int()
    plan = lambda av, nb, nreq, cap, mode, ok=1, mp=8, ms=8: lib.ltk_debug_ul_merge_plan(
        av, nb, nreq, cap, mode, ok, 0, out[0], out[1], out[2], mp, C.byref(n1), out[3], out[4], out[5], out[6], out[7], ms, C.byref(n2))
    assert plan(one, one, 1, 4, 0) == 0 and n1.value == 1 and n2.value == 1
    assert plan(None, one, 1, 4, 0) == INVALID and plan(one, None, 1, 4, 0) == INVALID and plan(one, one, 0, 4, 0) == INVALID
    assert plan(one, one, 1, 0, 0) == INVALID and plan(one, one, 1, 4, 3) == INVALID
    assert plan(one, (C.c_int * 1)(0), 1, 4, 0) == INVALID
    assert plan(one, one, 1, 4, 2, ok=0) == INVALID and b"grouped" in lib.ltk_last_error()
    assert plan(one, (C.c_int * 1)(9), 1, 1, 0) == INVALID and b"more passes" in lib.ltk_last_error()       # 9 passes, 8 slots


def test_gconv_refusals_without_a_gpu():
    """What ltk_ul_gconv_f16 refuses it refuses on the host, before it looks at the engine."""
    from livetalking_amd import _lib
    lib = _lib.load()
    sets = (C.c_int32 * 300)()
    w = np.zeros(2 * 64 * 64 * 9, np.float32)

    def call(N=3, H=10, W=10, Cin=32, Cout=32, n_sets=2, k=1, stride=1, pad=0, opts=None, st=sets):
        return lib.ltk_ul_gconv_f16(None, None, N, H, W, Cin, w.ctypes.data, n_sets, st, Cout, k, stride, pad, None, None, None, 0, None, opts, None)

    assert call() == INVALID and b"bad arguments" in lib.ltk_last_error()              # a good shape, no engine
    for kw, word in ((dict(Cin=24), b"Cin % 16"), (dict(Cout=40), b"Cout % 16"), (dict(N=257), b"256"), (dict(N=0), b"bad arguments"),
                     (dict(k=3, stride=1, pad=1), b"3x3 stride 2"), (dict(k=3, stride=2, pad=2), b"3x3 stride 2"), (dict(k=1, stride=2), b"1x1 stride 1"),
                     (dict(k=5, stride=2, pad=1), b"1x1 stride 1"), (dict(k=1, pad=1), b"1x1 stride 1")):
        assert call(**kw) == INVALID and word in lib.ltk_last_error(), (kw, lib.ltk_last_error())
    bad = (C.c_int32 * 3)(0, 2, 0)
    assert call(st=bad) == INVALID and b"image 1" in lib.ltk_last_error()
    bad = (C.c_int32 * 3)(0, 1, -1)
    assert call(st=bad) == INVALID and b"image 2" in lib.ltk_last_error()
    o = _lib.ConvOpts()
    o.x_ld, o.x_coff = 32, 16
    assert call(opts=C.byref(o)) == INVALID and b"outside the buffer" in lib.ltk_last_error()
    o = _lib.ConvOpts()
    o.y_ld, o.y_coff = 56, 8
    assert call(opts=C.byref(o)) == INVALID and b"multiples of 16" in lib.ltk_last_error()
    o = _lib.ConvOpts()
    o.act = 2
    assert call(opts=C.byref(o)) == INVALID and b"channel views" in lib.ltk_last_error()


def test_gconv_report_geometry_without_a_gpu():
    """The report is filled from the host-side geometry before the engine is looked at: kernel, tile, grid and blocks of every case."""
    from livetalking_amd import _lib
    lib = _lib.load()
    for c in G.cases():
        rep = _lib.ConvReport()
        sets = (C.c_int32 * c.N)(*c.sets)
        rc = lib.ltk_ul_gconv_f16(None, None, c.N, c.H, c.W, c.Cin, None, c.n_sets, sets, c.Cout, c.k, c.stride, c.pad, None, None, None, 0, None,
                                  None, C.byref(rep))
        assert rc == INVALID and b"bad arguments" in lib.ltk_last_error()
        g = c.geometry()
        assert (rep.kernel.decode(), rep.PXW, rep.NBT, rep.T, rep.grid, (rep.items >> 16, rep.items & 0xFFFF, rep.NB)) == \
            (g["kernel"], g["tile_px"], g["tile_co"], g["ksteps"], g["blocks"], g["grid"]), c.id


# ------------------------------------------------------------------ scheduler kind "ultralight"
class _FakeUlEngine:
    """ultralight_infer_merged records its calls; the FIRST call waits for `gate` (so that later requests queue behind it), a request
    whose feature pointer is the string "poison" fails the call that carries it."""
    torch_device = "cpu"

    def __init__(self, hold_first=True, ul_max_frames=64):
        self.calls, self.direct = [], []
        self.lock = threading.Lock()
        self.gate = threading.Event()
        self.entered = threading.Event()
        self.ul_max_frames = ul_max_frames
        if not hold_first:
            self.gate.set()

    def ultralight_infer_merged(self, reqs, mode=0, stream=0, report=False):
        with self.lock:
            self.calls.append(list(reqs))
        self.entered.set()
        self.gate.wait(timeout=20)
        if any(r[3] == "poison" for r in reqs):
            raise RuntimeError("poisoned request")

    def ultralight_infer(self, reqs, stream=0):
        self.direct.append(list(reqs))


def _req(i, batch=16, feat=None):
    return (1 + i % 2, 16 * i, batch, 5000 + i if feat is None else feat, 9000 + i)


def _queue_behind_first(sch, eng, reqs):
    """One request goes down alone and is held inside the engine; `reqs` then queue behind it.  -> (threads, errors by request)"""
    errs = {}

    def run(i, rq):
        try:
            sch.infer(*rq)
        except Exception as ex:  # noqa: BLE001
            errs[i] = ex

    first = threading.Thread(target=run, args=(-1, _req(99)))
    first.start()
    assert eng.entered.wait(timeout=20)
    ts = [threading.Thread(target=run, args=(i, rq)) for i, rq in enumerate(reqs)]
    for t in ts:
        t.start()
    with sch._cv:
        assert sch._cv.wait_for(lambda: len(sch._pending) == len(reqs), timeout=20)
    return [first] + ts, errs


def _join(ts):
    for t in ts:
        t.join(timeout=20)
        assert not t.is_alive()


def test_the_frame_limit_follows_ul_max_frames():
    from livetalking_amd import scheduler
    eng = _FakeUlEngine(ul_max_frames=64)
    sch = scheduler.BatchingScheduler(eng, "ultralight")
    assert sch._limit() == 64
    eng.ul_max_frames = 32
    assert sch._limit() == 32
    eng.mt_max_frames, eng.max_frames = 7, 9                       # the other kinds' limits are not this kind's
    assert sch._limit() == 32
    ts, errs = _queue_behind_first(sch, eng, [_req(i) for i in range(5)])          # 5 x 16 frames behind the held call: 32 + 32 + 16
    eng.gate.set()
    _join(ts)
    sch.close()
    assert not errs
    assert sorted(len(c) for c in eng.calls) == [1, 1, 2, 2]
    assert sorted(r[4] for c in eng.calls for r in c) == [9000 + i for i in range(5)] + [9099]             # every request once
    assert sch.stats["requests"] == 6 and sch.stats["max_requests_per_call"] == 2 and sch.stats["frames"] == 96


def test_concurrent_callers_coalesce_under_a_fixed_window(monkeypatch):
    """CoalescingScheduler(window): the first caller holds its batch open, the others join it: one engine call.  The window is the
    scheduler's own time.sleep; here it ends when everyone has arrived instead of by the clock."""
    import time
    import types
    from livetalking_amd import scheduler
    eng = _FakeUlEngine(hold_first=False)
    arrived = threading.Event()
    slept = []

    def sleep(t):
        slept.append(t)
        assert arrived.wait(timeout=20)

    monkeypatch.setattr(scheduler, "time", types.SimpleNamespace(sleep=sleep, perf_counter=time.perf_counter))
    sch = scheduler.CoalescingScheduler(eng, 250.0, kind="ultralight")
    ts = [threading.Thread(target=lambda i=i: sch.infer(*_req(i, batch=2))) for i in range(4)]
    for t in ts:
        t.start()
    with sch._cv:
        assert sch._cv.wait_for(lambda: len(sch._pending) == 4, timeout=20)
    arrived.set()
    _join(ts)
    sch.close()
    assert slept == [0.25]
    assert [len(c) for c in eng.calls] == [4] and sch.stats["calls"] == 1 and sch.stats["requests"] == 4 and sch.stats["frames"] == 8


def test_a_lone_caller_takes_the_direct_path(monkeypatch):
    from livetalking_amd import scheduler
    eng = _FakeUlEngine(hold_first=False)
    sch = scheduler.BatchingScheduler(eng, "ultralight")
    solo = []
    orig = sch._run_solo
    monkeypatch.setattr(sch, "_run_solo", lambda args, units: (solo.append(threading.current_thread()), orig(args, units))[1])
    for i in range(3):
        sch.infer(*_req(i))
    assert solo == [threading.current_thread()] * 3 and [len(c) for c in eng.calls] == [1, 1, 1]
    assert eng.calls[0] == [_req(0)]
    assert sch.stats["calls"] == 3 and sch.stats["max_requests_per_call"] == 1 and not sch._workers
    sch.close()


def test_a_poisoned_request_fails_alone():
    from livetalking_amd import scheduler
    eng = _FakeUlEngine()
    sch = scheduler.BatchingScheduler(eng, "ultralight")
    reqs = [_req(0), _req(1, feat="poison"), _req(2)]
    ts, errs = _queue_behind_first(sch, eng, reqs)
    eng.gate.set()
    _join(ts)
    sch.close()
    assert list(errs) == [1] and "poisoned" in str(errs[1])
    assert [len(c) for c in eng.calls] == [1, 3, 1, 1, 1]                  # the batch, then its requests one by one


def test_the_knob_bypasses_the_scheduler(monkeypatch):
    """LTK_UL_SCHED is read once at import (as LTK_PASTE_BATCH); 0 keeps the direct ultralight_infer call."""
    torch = pytest.importorskip("torch")
    from livetalking_amd.avatars import ultralight_avatar as ul
    assert ul._UL_SCHED == (os.environ.get("LTK_UL_SCHED", ul._UL_SCHED_DEFAULT) != "0")
    monkeypatch.setattr(ul, "_PASTE_BATCH", False)
    B = 3
    for on in (False, True):
        eng = _FakeUlEngine(hold_first=False)
        sess = ul.LightReal.__new__(ul.LightReal)
        sess.engine, sess._aid, sess._frame_hw, sess.batch_size = eng, 9, (6, 10), B
        sess.face_list_cycle = [np.zeros((168, 168, 3), np.uint8)] * 3
        monkeypatch.setattr(ul, "_UL_SCHED", on)
        items = sess.inference_batch(2, torch.zeros(B, 16, 1024))
        assert len(items) == B
        if on:
            assert not eng.direct and len(eng.calls) == 1 and eng.calls[0][0][:3] == (9, 2, B)
            assert eng.calls[0][0][4] == items[0].data_ptr()
            eng.__dict__["_ltk_schedulers"]["ultralight"].close()
        else:
            assert len(eng.direct) == 1 and eng.direct[0][0][:3] == (9, 2, B) and not eng.calls and "_ltk_schedulers" not in eng.__dict__


# ------------------------------------------------------------------ ul_gconv: the gates against a simulated device
_CASES = G.cases()


@pytest.fixture(scope="module")
def refs():
    """case id -> (inputs, buffers, ref, tol, model), computed once for the module."""
    out = {}
    for c in _CASES:
        inp = G.Inputs(c)
        ref, tol = G.reference(c, inp)
        out[c.id] = (inp, G.Buffers(c, inp), ref, tol, G.model(c, inp))
    return out


def test_case_ids_are_unique_and_cover_the_edges():
    ids = [c.id for c in _CASES]
    assert len(set(ids)) == len(ids)
    one = [c for c in _CASES if c.k == 1]
    assert {(c.Cin, c.Cout) for c in one if (c.H, c.W) == (10, 10) and c.N == 3} >= {(ci, co) for ci in (16, 32, 48, 64) for co in (16, 32, 48)}
    assert {(c.H, c.W) for c in one} == {(10, 10), (5, 7), (1, 1)} and any(c.N == 1 for c in _CASES) and any(c.big for c in _CASES)
    assert {(c.H, c.W, c.Ho, c.Wo, c.pad) for c in _CASES if c.k == 3} == {(8, 8, 4, 4, 1), (16, 16, 10, 10, 3)}
    for flag in ("res", "relu", "view"):
        assert {getattr(c, flag) for c in _CASES} == {False, True}
    for fault, shows in G.FAULTS.items():
        assert any(shows(c) for c in _CASES), fault


@pytest.mark.parametrize("c", _CASES, ids=lambda c: c.id)
def test_the_rounding_model_sits_inside_half_the_bound(refs, c):
    import torch
    _, _, ref, tol, mod = refs[c.id]
    worst = float(((mod.double() - ref).abs() / tol).max())
    assert worst <= 0.5 and bool(torch.isfinite(mod).all()), f"{c.id}: max |mod - ref| / tol = {worst:.3f}"


@pytest.mark.parametrize("c", _CASES, ids=lambda c: c.id)
def test_the_unfaulted_simulation_passes_the_check(refs, c):
    inp, b, ref, tol, mod = refs[c.id]
    G.check(c, inp, b, G.SimDevice(c, inp).run(b), ref, tol, mod)


@pytest.mark.parametrize("fault", list(G.FAULTS))
def test_a_planted_fault_is_rejected(refs, fault):
    """... on every case the fault shows on."""
    shown = 0
    for c in _CASES:
        if not G.FAULTS[fault](c):
            continue
        inp, b, ref, tol, mod = refs[c.id]
        with pytest.raises(AssertionError):
            G.check(c, inp, b, G.SimDevice(c, inp, fault).run(b), ref, tol, mod)
        shown += 1
    assert shown


def test_a_read_outside_the_view_or_a_write_outside_it_is_rejected(refs):
    c = next(c for c in _CASES if c.view and c.res)
    inp, b, ref, tol, mod = refs[c.id]
    y = G.SimDevice(c, inp).run(b)
    y[c.N, 0, 0, 0, 0] ^= 1                                         # the image past N
    with pytest.raises(AssertionError):
        G.check(c, inp, b, y, ref, tol, mod)
    y = G.SimDevice(c, inp).run(b)
    y[0, b.y_cb0 - 1, 0, 0, 3] = 0                                  # the block in front of the view
    with pytest.raises(AssertionError):
        G.check(c, inp, b, y, ref, tol, mod)
    # the guard blocks of x dominate whatever reads them
    x = G._from_cb(b.x, c.N, 16, b.x_cb0 - 1)
    assert float(x.abs().min()) >= G.GUARD_GAIN


# ------------------------------------------------------------------ merged call: frames land in each request's own tensor
def test_a_merged_call_that_writes_in_avatar_sorted_order_is_rejected():
    names = ["a1", "b1", "a1b"]                                     # a, b, a
    good = M.SimMergedCall(names)
    for r, n in enumerate(names):
        M.gate_float64(n, good.out[r])
    bad = M.SimMergedCall(names, "avatar_sorted_outputs")
    M.gate_float64(names[0], bad.out[0])                            # the first request is where it would be anyway
    for r in (1, 2):
        with pytest.raises(AssertionError):
            M.gate_float64(names[r], bad.out[r])
