"""CPU tests of the batched Whisper live step: the call planner (ltk_debug_whisper_batch_plan, no GPU), the ABI of
ltk_whisper_step_batch, the scheduler kind "whisper" and WhisperASR.run_step over fake engines, and the clips the GPU file replays
against float64 (tests/whisper_batch_cases.py) on a simulated device: the reference alone stays inside the replay's bound on them."""
from __future__ import annotations

import ctypes as C
import os
import re
import threading
import types

import numpy as np
import pytest

import whisper_batch_cases as B

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID = -1


# ------------------------------------------------------------------ planner
def _device_plan(nreq):
    from livetalking_amd import _lib
    lib = _lib.load()
    n = max(nreq, 1)
    run_of, slot_of, batched, n_runs = (C.c_int * n)(), (C.c_int * n)(), (C.c_int * n)(), C.c_int()
    _lib.check(lib.ltk_debug_whisper_batch_plan(nreq, run_of, slot_of, batched, C.byref(n_runs)))
    runs = [(bool(batched[i]), []) for i in range(n_runs.value)]
    for r in range(nreq):
        assert slot_of[r] == len(runs[run_of[r]][1])                      # slots in request order
        runs[run_of[r]][1].append(r)
    return runs


@pytest.mark.parametrize("nreq,sizes", [(1, [(False, 1)]), (2, [(True, 2)]), (16, [(True, 16)]), (17, [(True, 16), (False, 1)]),
                                        (32, [(True, 16), (True, 16)]), (33, [(True, 16), (True, 16), (False, 1)])])
def test_plan_cuts_a_call_into_runs_of_sixteen(nreq, sizes):
    got = _device_plan(nreq)
    assert got == B.expected_plan(nreq)
    assert [(b, len(m)) for b, m in got] == sizes
    assert [r for _, m in got for r in m] == list(range(nreq))            # every request once, in request order


def test_plan_refuses_an_empty_call_and_the_engine_wrapper_agrees():
    from livetalking_amd import _lib
    from livetalking_amd.engine import Engine
    lib = _lib.load()
    n = (C.c_int * 1)()
    for nreq in (0, -1):
        assert lib.ltk_debug_whisper_batch_plan(nreq, n, n, n, n) == INVALID and b"bad arguments" in lib.ltk_last_error()
    assert lib.ltk_debug_whisper_batch_plan(1, None, n, n, n) == INVALID
    assert lib.ltk_debug_whisper_batch_plan(1, n, n, n, None) == INVALID
    eng = object.__new__(Engine)                                          # the planner needs no engine handle
    eng._lib, eng._h, eng._closed = lib, None, True
    assert eng.whisper_batch_plan(17) == B.expected_plan(17)
    with pytest.raises(_lib.LtkError):
        eng.whisper_batch_plan(0)


# ------------------------------------------------------------------ ABI
def test_request_struct_and_entries():
    from livetalking_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "ltk.h")).read()
    lib = _lib.load()
    for name in ("ltk_whisper_step_batch", "ltk_whisper_batch_info", "ltk_whisper_debug_get_clip", "ltk_debug_whisper_batch_plan"):
        assert re.search(r"\bint\s+" + name + r"\s*\(", hdr), f"{name} is not declared in include/ltk.h"
        assert name in _lib.SYMBOLS and getattr(lib, name) is not None
    body = re.search(r"typedef struct ltk_whisper_req \{(.*?)\} ltk_whisper_req;", hdr, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    names = [n for decl in body.split(";") for n in re.findall(r"(\w+)\s*(?:,|$)", decl.strip())]
    assert names == ["pcm", "n_samples", "batch", "first_row", "row_step", "rows", "d_out"]
    R = _lib.WhisperReq
    assert [f[0] for f in R._fields_] == names
    assert [getattr(R, n).offset for n in names] == [0, 8, 12, 16, 20, 24, 32] and C.sizeof(R) == 40


def test_argument_validation_without_a_gpu():
    """Every request is checked before the engine is touched: a bad one is LTK_E_INVALID and named, also with no engine at all; a
    null engine is refused by every entry."""
    from livetalking_amd import _lib
    lib = _lib.load()
    pcm = np.zeros(3200, np.float32)
    out = (C.c_float * 16)()

    def call(nreq, at=1, **bad):
        reqs = (_lib.WhisperReq * max(nreq, 1))()
        for r in reqs:
            r.pcm, r.n_samples, r.batch, r.first_row, r.row_step, r.rows = pcm.ctypes.data, 3200, 2, 0, 2, 10
            r.d_out = C.addressof(out)
        for k, v in bad.items():
            setattr(reqs[at], k, v)
        return lib.ltk_whisper_step_batch(None, reqs, nreq)

    assert lib.ltk_whisper_step_batch(None, None, 1) == INVALID and b"bad arguments" in lib.ltk_last_error()
    assert call(0, at=0) == INVALID and call(-1, at=0) == INVALID
    for bad in (dict(pcm=None), dict(d_out=None), dict(n_samples=0), dict(n_samples=479001), dict(batch=0), dict(batch=-3), dict(rows=0),
                dict(rows=65)):
        assert call(3, **bad) == INVALID, bad
        assert b"bad request 1" in lib.ltk_last_error(), bad
    assert call(3, n_samples=479000, rows=64) == INVALID and b"bad arguments" in lib.ltk_last_error()      # good requests, no engine
    assert lib.ltk_whisper_debug_get_clip(None, b"hidden_states.0", 0, out, 16) == INVALID
    assert lib.ltk_whisper_batch_info(None, None, None, None) == INVALID


# ------------------------------------------------------------------ scheduler kind "whisper"
class _FakeWhisperEngine:
    """whisper_step_batch records its calls; the FIRST call waits for `gate`, so that later requests queue behind it."""
    torch_device = "cpu"

    def __init__(self, hold_first=True):
        self.calls, self.single = [], []
        self.lock = threading.Lock()
        self.gate = threading.Event()
        self.entered = threading.Event()
        if not hold_first:
            self.gate.set()

    def whisper_step_batch(self, reqs):
        with self.lock:
            self.calls.append(list(reqs))
        self.entered.set()
        self.gate.wait(timeout=20)

    def whisper_step(self, pcm, batch, first_row, d_out_ptr, row_step=2, rows=10, stream=0):
        self.single.append((pcm, batch, first_row, d_out_ptr, row_step, rows))


def _req(i):
    return (np.full(4, i, np.float32), 16, 10 + i, 2, 10, 1000 + i)


def _submit_all(sch, reqs):
    errs = {}

    def run(i, rq):
        try:
            sch.submit(rq, 1)
        except Exception as ex:  # noqa: BLE001
            errs[i] = ex

    ts = [threading.Thread(target=run, args=(i, rq)) for i, rq in enumerate(reqs)]
    return ts, errs


def _join(ts):
    for t in ts:
        t.join(timeout=20)
        assert not t.is_alive()


def test_four_sessions_submitting_at_once_share_calls():
    from livetalking_amd import scheduler
    eng = _FakeWhisperEngine()
    sch = scheduler.BatchingScheduler(eng, "whisper")
    assert sch._limit() == scheduler.WHISPER_BATCH_CLIPS == B.CAPACITY
    reqs = [_req(i) for i in range(4)]
    ts, errs = _submit_all(sch, reqs)
    ts[0].start()
    assert eng.entered.wait(timeout=20)                    # the first one is inside the engine: the other three queue behind it
    for t in ts[1:]:
        t.start()
    with sch._cv:
        assert sch._cv.wait_for(lambda: len(sch._pending) == 3, timeout=20)
    eng.gate.set()
    _join(ts)
    sch.close()
    assert not errs
    assert [len(c) for c in eng.calls] == [1, 3] and sch.stats["max_requests_per_call"] == 3 and sch.stats["requests"] == 4
    seen = [r for c in eng.calls for r in c]
    assert sorted(r[5] for r in seen) == [1000, 1001, 1002, 1003]                       # every request once
    for r in seen:                                                                      # ... unchanged, in a slot of its own
        want = reqs[r[5] - 1000]
        assert r[0] is want[0] and r[1:] == want[1:]


def test_no_call_carries_more_than_sixteen_requests():
    from livetalking_amd import scheduler
    eng = _FakeWhisperEngine()
    sch = scheduler.BatchingScheduler(eng, "whisper")
    ts, errs = _submit_all(sch, [_req(i) for i in range(21)])
    ts[0].start()
    assert eng.entered.wait(timeout=20)
    for t in ts[1:]:
        t.start()
    with sch._cv:
        assert sch._cv.wait_for(lambda: len(sch._pending) == 20, timeout=20)
    eng.gate.set()
    _join(ts)
    sch.close()
    assert not errs and sorted(len(c) for c in eng.calls) == [1, 4, 16]
    assert sorted(r[5] for c in eng.calls for r in c) == [1000 + i for i in range(21)]


def test_a_lone_submitter_takes_the_direct_path(monkeypatch):
    from livetalking_amd import scheduler
    eng = _FakeWhisperEngine(hold_first=False)
    sch = scheduler.BatchingScheduler(eng, "whisper")
    solo = []
    orig = sch._run_solo
    monkeypatch.setattr(sch, "_run_solo", lambda args, units: (solo.append(threading.current_thread()), orig(args, units))[1])
    for i in range(3):
        sch.submit(_req(i), 1)
    assert solo == [threading.current_thread()] * 3 and [len(c) for c in eng.calls] == [1, 1, 1]
    assert sch.stats["calls"] == 3 and sch.stats["max_requests_per_call"] == 1 and not sch._workers
    sch.close()


def test_the_other_kinds_are_untouched():
    from livetalking_amd import scheduler
    assert scheduler._ENGINE_CALL == {"wav2lip": "wav2lip_infer", "musetalk": "musetalk_infer", "hubert": "hubert_step_batch",
                                      "ultralight": "ultralight_infer_merged", "whisper": "whisper_step_batch"}
    assert '"whisper" -> Engine.whisper_step_batch' in scheduler.__doc__
    with pytest.raises(AttributeError):                       # an engine that cannot serve the kind fails at the first request, loudly
        scheduler.BatchingScheduler(object(), "whisper").submit(_req(0), 1)


# ------------------------------------------------------------------ WhisperASR.run_step
def test_run_step_submits_to_the_whisper_scheduler_or_calls_whisper_step(monkeypatch):
    """LTK_WHISPER_BATCH is read once at import; on: (pcm, B, first_row, 2, 10, ptr) goes to the "whisper" scheduler as one clip;
    0: today's engine.whisper_step call, and no scheduler is made."""
    pytest.importorskip("torch")
    from livetalking_amd.avatars.audio_features import whisper as wh
    assert wh._WHISPER_BATCH == (os.environ.get("LTK_WHISPER_BATCH", wh._WHISPER_BATCH_DEFAULT) != "0")
    Bs, l, r = 4, 10, 10
    chunks = [np.full(320, i, np.float32) for i in range(l + r + 2 * Bs)]
    for on in (False, True):
        eng = _FakeWhisperEngine(hold_first=False)
        asr = object.__new__(wh.WhisperASR)
        asr.engine, asr._torch = eng, __import__("torch")
        asr.batch_size, asr.stride_left_size, asr.stride_right_size = Bs, l, r
        asr.frames = list(chunks[: l + r])
        it = iter(chunks[l + r:])
        asr.get_audio_frame = lambda: types.SimpleNamespace(data=next(it), type=0)
        sink = types.SimpleNamespace(put=lambda x: None)
        feats = []
        asr.output_queue, asr.feat_queue = sink, types.SimpleNamespace(put=feats.append)
        monkeypatch.setattr(wh, "_WHISPER_BATCH", on)
        asr.run_step()
        assert len(feats) == 1 and tuple(feats[0].shape) == (Bs, 50, 384) and len(asr.frames) == l + r
        pcm = np.concatenate(chunks)
        if on:
            assert not eng.single and len(eng.calls) == 1 and len(eng.calls[0]) == 1
            got = eng.calls[0][0]
            assert got[1:] == (Bs, int((l / 2) * 2), 2, 10, feats[0].data_ptr()) and np.array_equal(got[0], pcm)
            sch = eng.__dict__["_ltk_schedulers"]["whisper"]
            assert sch.stats["frames"] == 1                           # the unit is one clip
            sch.close()
        else:
            assert not eng.calls and "_ltk_schedulers" not in eng.__dict__ and len(eng.single) == 1
            got = eng.single[0]
            assert got[1:] == (Bs, int((l / 2) * 2), feats[0].data_ptr(), 2, 10) and np.array_equal(got[0], pcm)


# ------------------------------------------------------------------ the replay clips against a simulated device
@pytest.fixture(scope="module")
def whisper_layer():
    torch = pytest.importorskip("torch")
    pytest.importorskip("transformers")
    from oracle import op_replay as R
    from oracle import whisper_oracle as WO
    model = WO.tiny_whisper(0)
    sd = {k: v.detach().clone() for k, v in model.encoder.state_dict().items()}
    one = {k: v for k, v in sd.items() if not k.startswith("layers.") or k.startswith("layers.0.")}
    sim_sd = {k: (R.f16(v) if k.endswith(".weight") and v.dim() >= 2 and k != "embed_positions.weight" else v) for k, v in one.items()}
    return torch, R, WO, one, sim_sd


@pytest.mark.parametrize("i", B.REPLAY_CLIPS)
def test_the_replay_clips_pass_against_a_simulated_device(whisper_layer, i):
    """The form of tests/test_op_replay.py's Whisper test (one encoder layer has every op type): the float32 oracle with fp16 weights
    and fp16 op outputs stands in for the device on clip i's log-mel features; no op uncovered, no failure, the rounding model
    inside its headroom (model_too).  The quiet (x 1e-3) and the 21-frame clips put most of the window on the clamp floor."""
    torch, R, WO, one, sim_sd = whisper_layer
    x = R.f16(WO.input_features(B.clip(i)))
    sim = R.SimDevice(fused=("conv2",))
    with torch.no_grad():
        WO.encoder_ops(sim_sd, x, force=sim)
    rp, miss = B.replay(one, x, lambda name, shape: (sim.t[name] / (8.0 if name.endswith(".q_proj") else 1.0)).reshape(shape).numpy(), R, WO)
    assert not miss, miss
    bad = R.failures(rp.records, model_too=True)
    assert not bad, "\n".join(bad)
