"""CPU tests of the batched HuBERT live step: the call planner (ltk_debug_hubert_batch_plan, no GPU), the ABI of
ltk_hubert_step_batch, the scheduler kind "hubert" over a fake engine, and the gates of tests/hubert_batch_cases.py against a
simulated device with one batching fault planted at a time - the gates the GPU file holds the device to."""
from __future__ import annotations

import ctypes as C
import os
import re
import threading

import numpy as np
import pytest

import hubert_batch_cases as B
import hubert_ref as H

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OVER_BUDGET = 60000              # 187 rows: 148.7 MB per clip at 24 layers, 2.38 GB at 16 clips


# ------------------------------------------------------------------ planner
def _check(lengths, layers=24):
    got, clip_bytes = B.device_plan(lengths, layers)
    by_len = dict(zip(lengths, clip_bytes))
    want = B.expected_plan(lengths, lambda n: by_len[n])
    assert got == want, (lengths, got, want)
    assert sorted(r for _, _, m in got for r in m) == list(range(len(lengths)))            # every request once
    for n, batched, members in got:
        assert members == sorted(members)                                                  # arrival order inside a run
        assert len(members) <= B.CAPACITY and (batched or len(members) == 1)
        assert all(lengths[r] == n for r in members)
    return got


def test_plan_edges_of_the_gpu_cases():
    got = _check([B.ROWS3] * 17)
    assert [(b, len(m)) for _, b, m in got] == [(True, 16), (False, 1)]
    got = _check(B.MIXED)
    assert got == [(B.ROWS3, True, [0, 2]), (B.LIVE, True, [1, 4]), (B.ROWS70, False, [3])]


@pytest.mark.parametrize("nreq,runs", [(1, [(False, 1)]), (2, [(True, 2)]), (16, [(True, 16)]), (17, [(True, 16), (False, 1)]),
                                       (33, [(True, 16), (True, 16), (False, 1)])])
def test_plan_cuts_a_group_into_runs_of_sixteen(nreq, runs):
    assert [(b, len(m)) for _, b, m in _check([B.LIVE] * nreq)] == runs


def test_plan_groups_of_one_and_lengths_over_the_budget():
    assert all(not b and len(m) == 1 for _, b, m in _check([400, 720, B.ROWS3, B.LIVE]))
    _, clip_bytes = B.device_plan([B.LIVE, OVER_BUDGET], 24)
    assert clip_bytes[0] == 40748032                       # 40.7 MB at the live length, 0.65 GB at 16 clips
    assert clip_bytes[0] * B.CAPACITY < B.BUDGET <= clip_bytes[1] * B.CAPACITY
    got = _check([OVER_BUDGET, B.LIVE, OVER_BUDGET, B.LIVE, OVER_BUDGET])
    assert got == [(OVER_BUDGET, False, [0]), (OVER_BUDGET, False, [2]), (OVER_BUDGET, False, [4]), (B.LIVE, True, [1, 3])]
    assert _check([OVER_BUDGET] * 3, layers=2) == [(OVER_BUDGET, True, [0, 1, 2])]       # the budget follows the depth
    # interleaved lengths: order within a group is arrival order, groups run in the order of their first request
    got = _check([B.LIVE, B.ROWS3, B.LIVE, B.ROWS3, B.ROWS3, B.LIVE])
    assert got == [(B.LIVE, True, [0, 2, 5]), (B.ROWS3, True, [1, 3, 4])]


# ------------------------------------------------------------------ ABI
def test_request_struct_and_entries():
    from livetalking_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "ltk.h")).read()
    lib = _lib.load()
    for name in ("ltk_hubert_step_batch", "ltk_hubert_debug_get_clip", "ltk_hubert_batch_info", "ltk_debug_hubert_batch_plan"):
        assert re.search(r"\bint\s+" + name + r"\s*\(", hdr), f"{name} is not declared in include/ltk.h"
        assert name in _lib.SYMBOLS and getattr(lib, name) is not None
    body = re.search(r"typedef struct ltk_hubert_req \{(.*?)\} ltk_hubert_req;", hdr, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    names = [n for decl in body.split(";") for n in re.findall(r"(\w+)\s*(?:,|$)", decl.strip())]
    assert names == ["pcm", "n_samples", "batch", "first_row", "row_step", "rows", "d_out"]
    R = _lib.HubertReq
    assert [f[0] for f in R._fields_] == names
    assert [getattr(R, n).offset for n in names] == [0, 8, 12, 16, 20, 24, 32] and C.sizeof(R) == 40


def test_argument_validation_without_a_gpu():
    """Every request is checked before the engine is touched: a bad one is LTK_E_INVALID and named, also with no engine at all."""
    from livetalking_amd import _lib
    lib = _lib.load()
    INVALID = -1
    pcm = np.zeros(1040, np.float32)
    out = (C.c_float * 16)()

    def call(nreq, **bad):
        reqs = (_lib.HubertReq * max(nreq, 1))()
        for r in reqs:
            r.pcm, r.n_samples, r.batch, r.first_row, r.row_step, r.rows = pcm.ctypes.data, 1040, 2, 0, 2, 16
            r.d_out = C.addressof(out)
        for k, v in bad.items():
            setattr(reqs[-1], k, v)
        return lib.ltk_hubert_step_batch(None, reqs, nreq)

    assert lib.ltk_hubert_step_batch(None, None, 1) == INVALID and b"bad arguments" in lib.ltk_last_error()
    assert call(0) == INVALID and call(-1) == INVALID
    for bad in (dict(pcm=None), dict(d_out=None), dict(n_samples=399), dict(n_samples=320000), dict(batch=0), dict(batch=-3), dict(rows=0)):
        assert call(3, **bad) == INVALID, bad
        assert b"bad request 2" in lib.ltk_last_error(), bad
    assert call(3) == INVALID and b"bad arguments" in lib.ltk_last_error()            # good requests, no engine
    assert lib.ltk_hubert_debug_get_clip(None, b"x", 0, out, 16) == INVALID
    assert lib.ltk_hubert_batch_info(None, None, None, None) == INVALID
    n = (C.c_int * 1)(1040)
    assert lib.ltk_debug_hubert_batch_plan(n, 0, 24, n, n, n, n, None) == INVALID
    assert lib.ltk_debug_hubert_batch_plan(None, 1, 24, n, n, n, n, None) == INVALID


# ------------------------------------------------------------------ scheduler kind "hubert"
class _FakeHubertEngine:
    """hubert_step_batch records its calls; the FIRST call waits for `gate` (so that later requests queue behind it), a request
    whose pcm is the string "poison" fails the call that carries it."""
    torch_device = "cpu"

    def __init__(self, hold_first=True):
        self.calls, self.single = [], []
        self.lock = threading.Lock()
        self.gate = threading.Event()
        self.entered = threading.Event()
        if not hold_first:
            self.gate.set()

    def hubert_step_batch(self, reqs):
        with self.lock:
            self.calls.append(list(reqs))
        self.entered.set()
        self.gate.wait(timeout=20)
        if any(isinstance(r[0], str) and r[0] == "poison" for r in reqs):
            raise RuntimeError("poisoned request")

    def hubert_step(self, pcm, batch, first_row, d_out_ptr, row_step=2, rows=16):
        self.single.append((batch, first_row, row_step, rows, d_out_ptr))


def _req(i, pcm=None):
    return (np.full(4, i, np.float32) if pcm is None else pcm, 4, 2, 2, 16, 1000 + i)


def _queue_behind_first(sch, eng, reqs):
    """One request goes down alone and is held inside the engine; `reqs` then queue behind it.  -> (threads, errors by request)"""
    errs = {}

    def run(i, rq):
        try:
            sch.submit(rq, 1)
        except Exception as ex:  # noqa: BLE001
            errs[i] = ex

    first = threading.Thread(target=run, args=(-1, _req(-1)))
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


def test_concurrent_sessions_coalesce_into_calls_of_at_most_sixteen_clips():
    from livetalking_amd import scheduler
    eng = _FakeHubertEngine()
    sch = scheduler.BatchingScheduler(eng, "hubert")
    assert sch._limit() == scheduler.HUBERT_BATCH_CLIPS == B.CAPACITY
    ts, errs = _queue_behind_first(sch, eng, [_req(i) for i in range(20)])
    eng.gate.set()
    _join(ts)
    sch.close()
    assert not errs
    assert sorted(len(c) for c in eng.calls) == [1, 4, 16]
    assert sorted(r[5] for c in eng.calls for r in c) == [999] + [1000 + i for i in range(20)]          # every request once
    assert sch.stats["requests"] == 21 and sch.stats["max_requests_per_call"] == 16 and sch.stats["frames"] == 21


def test_a_lone_caller_takes_the_direct_path(monkeypatch):
    from livetalking_amd import scheduler
    eng = _FakeHubertEngine(hold_first=False)
    sch = scheduler.BatchingScheduler(eng, "hubert")
    solo = []
    orig = sch._run_solo
    monkeypatch.setattr(sch, "_run_solo", lambda args, units: (solo.append(threading.current_thread()), orig(args, units))[1])
    for i in range(3):
        sch.submit(_req(i), 1)
    assert solo == [threading.current_thread()] * 3 and [len(c) for c in eng.calls] == [1, 1, 1]
    assert sch.stats["calls"] == 3 and sch.stats["max_requests_per_call"] == 1 and not sch._workers
    sch.close()


def test_a_poisoned_request_fails_alone():
    from livetalking_amd import scheduler
    eng = _FakeHubertEngine()
    sch = scheduler.BatchingScheduler(eng, "hubert")
    reqs = [_req(0), _req(1, "poison"), _req(2)]
    ts, errs = _queue_behind_first(sch, eng, reqs)
    eng.gate.set()
    _join(ts)
    sch.close()
    assert list(errs) == [1] and "poisoned" in str(errs[1])
    assert [len(c) for c in eng.calls] == [1, 3, 1, 1, 1]                  # the batch, then its requests one by one


def test_close_unblocks_waiters():
    from livetalking_amd import scheduler
    eng = _FakeHubertEngine()
    sch = scheduler.BatchingScheduler(eng, "hubert")
    ts, errs = _queue_behind_first(sch, eng, [_req(0), _req(1)])
    sch.close()
    _join(ts[1:])
    assert sorted(errs) == [0, 1] and all("scheduler closed" in str(e) for e in errs.values())
    eng.gate.set()
    _join(ts[:1])
    assert [len(c) for c in eng.calls] == [1]


def test_the_knob_bypasses_the_scheduler(monkeypatch):
    """LTK_HUBERT_BATCH is read once at import (as LTK_PASTE_BATCH); 0 keeps the direct hubert_step call."""
    pytest.importorskip("torch")
    from livetalking_amd.avatars.audio_features import hubert as hub
    assert hub._HUBERT_BATCH == (os.environ.get("LTK_HUBERT_BATCH", hub._HUBERT_BATCH_DEFAULT) != "0")
    pcm = np.zeros(1040, np.float32)
    for on in (False, True):
        eng = _FakeHubertEngine(hold_first=False)
        proc = object.__new__(hub.EngineAudio2Feature)
        proc.engine = eng
        monkeypatch.setattr(hub, "_HUBERT_BATCH", on)
        out = proc.step(pcm, 4, 2, row_step=2, rows=16)
        assert tuple(out.shape) == (4, 16, 1024)
        if on:
            assert not eng.single and len(eng.calls) == 1 and eng.calls[0][0][1:] == (4, 2, 2, 16, out.data_ptr())
            assert eng.calls[0][0][0] is pcm
            eng.__dict__["_ltk_schedulers"]["hubert"].close()
        else:
            assert eng.single == [(4, 2, 2, 16, out.data_ptr())] and not eng.calls and "_ltk_schedulers" not in eng.__dict__


def test_engines_without_hubert_methods_still_get_their_schedulers():
    from livetalking_amd import scheduler

    class W2l:
        max_frames = 64

        def __init__(self):
            self.calls = []

        def wav2lip_infer(self, reqs, stream=0):
            self.calls.append(list(reqs))

    class Mt:
        mt_max_frames = 16

        def __init__(self):
            self.calls = []

        def musetalk_infer(self, reqs, stream=0):
            self.calls.append(list(reqs))

    for eng, kind in ((W2l(), "wav2lip"), (Mt(), "musetalk")):
        sch = scheduler.BatchingScheduler(eng, kind)
        sch.infer(1, 0, 16, 10, 20)
        assert eng.calls == [[(1, 0, 16, 10, 20)]]
        sch.close()
    with pytest.raises(ValueError):
        scheduler.BatchingScheduler(W2l(), "hubert2")
    with pytest.raises(AttributeError):                       # a kind the engine cannot serve fails at the first request, loudly
        scheduler.BatchingScheduler(W2l(), "hubert").submit(_req(0), 1)


# ------------------------------------------------------------------ the gates against a simulated device
@pytest.fixture(scope="module")
def sd2():
    return H.state_dict(2, 20)


def _reqs(lengths):
    reqs = []
    for n in dict.fromkeys(lengths):
        members = [r for r, m in enumerate(lengths) if m == n]
        for pcm, r in zip(B.clips(len(members), n, seed=200 + n % 97), members):
            batch, first_row, _, _ = B.chunk_spec(r, n)
            reqs.append((r, (pcm, batch, first_row)))
    return [rq for _, rq in sorted(reqs, key=lambda t: t[0])]


def _hold(sd, sim, reqs):
    """Every gate of the GPU file on every request of the simulated call."""
    for r, (pcm, batch, first_row) in enumerate(reqs):
        label = f"req {r} ({len(pcm)} samples)"
        B.gate_input_values(sim.input_values(r), pcm, label)
        B.gate_replay(sd, sim.input_values(r), sim.get(r), B.sim_ops(2), label, model_too=True)
        own = H.forward(sd, H.normalise(pcm).astype(np.float32), fp16_model=True).numpy().astype(np.float32)
        B.gate_chunks(sim.out[r], own, batch, first_row, label)


@pytest.fixture(scope="module")
def sim_reqs():
    return _reqs([B.ROWS3, B.ROWS3, B.ROWS3])


def test_the_unfaulted_simulation_passes_every_gate(sd2, sim_reqs):
    """... with its rounding model inside R.MODEL_HEADROOM of every bound (failures(model_too=True))."""
    _hold(sd2, B.SimBatch(sd2, sim_reqs), sim_reqs)


@pytest.mark.parametrize("fault", [f for f in B.FAULTS if f != "outputs_in_grouped_order"])
def test_a_planted_batching_fault_is_rejected(sd2, sim_reqs, fault):
    with pytest.raises(AssertionError):
        _hold(sd2, B.SimBatch(sd2, sim_reqs, fault), sim_reqs)


def test_outputs_in_grouped_order_are_rejected(sd2):
    """Two lengths interleaved: grouped order is [0, 2, 1, 3], so requests 1 and 2 would receive each other's chunks."""
    reqs = _reqs([B.ROWS3, 720, B.ROWS3, 720])
    _hold(sd2, B.SimBatch(sd2, reqs), reqs)
    with pytest.raises(AssertionError):
        _hold(sd2, B.SimBatch(sd2, reqs, "outputs_in_grouped_order"), reqs)
