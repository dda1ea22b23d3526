"""The batched Whisper live step (ltk_whisper_step_batch, scheduler kind "whisper") on the GPU: every op of every clip against float64
(oracle/op_replay.py, the project's own bound), the per-clip log-mel front end and chunk gather byte for byte, isolation between the
clips of a run, the library the reference calls (tests/test_whisper_gpu.py's tolerances), the 16 + 1 cut, graph replay, refusals and
the WhisperASR plugin path.  The program is fixed at 1500 tokens, so the small dimension is the clip count: 2 and 3 clips everywhere,
16 only where a test names it.  Clips: tests/whisper_batch_cases.py."""
from __future__ import annotations

import ctypes as C
import threading
import types

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytest.importorskip("transformers")

import synth_inputs as synth  # noqa: E402
import whisper_batch_cases as B  # noqa: E402
from oracle import op_replay as R  # noqa: E402
from oracle import whisper_oracle as WO  # noqa: E402

pytestmark = pytest.mark.gpu

BATCH, L = 16, 10                      # frames per step and the left context of the live session (first_row = 2 * (L / 2))
STATES = [f"hidden_states.{i}" for i in range(5)]


class _Ctx:
    def __init__(self):
        self.model = WO.tiny_whisper(0)
        self.sd = {k: v.detach().clone() for k, v in self.model.encoder.state_dict().items()}
        self.eng = self.new_engine()
        self._single = {}

    def new_engine(self):
        from livetalking_amd.engine import Engine
        eng = Engine(0)
        eng.load_whisper(dict(self.sd))
        return eng

    def single(self, i):
        """Clip i alone through whisper_step on the module's engine, once: its input_features and its (BATCH, 50, 384) chunks."""
        if i not in self._single:
            out = torch.zeros(BATCH, 50, 384, dtype=torch.float32, device="cuda")
            self.eng.whisper_step(B.clip(i), BATCH, L, out.data_ptr())
            self._single[i] = (self.eng.whisper_debug_get("input_features", (80, 3000)), out.cpu().numpy())
        return self._single[i]


@pytest.fixture(scope="module")
def ctx():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    c = _Ctx()
    yield c
    c.eng.close()


def _outs(specs, fill=0.0):
    return [torch.full((b, rows * 5, 384), fill, dtype=torch.float32, device="cuda") for b, _, _, rows in specs]


def _run(eng, pcms, specs=None, fill=0.0):
    """One whisper_step_batch call; specs = [(batch, first_row, row_step, rows)] (the live step's by default) -> host arrays"""
    specs = specs or [(BATCH, L, 2, 10)] * len(pcms)
    outs = _outs(specs, fill)
    eng.whisper_step_batch([(p, b, fr, st, rows, o.data_ptr()) for p, (b, fr, st, rows), o in zip(pcms, specs, outs)])
    return [o.cpu().numpy() for o in outs]


def _rel(a, b):
    return float(np.linalg.norm(a - b) / np.linalg.norm(b))


# ------------------------------------------------------------------ 1. every op of every clip against float64
@pytest.mark.parametrize("nclips,clip", [(2, 0), (2, 1), (16, 0), (16, 7), (16, 15)])
def test_every_op_of_a_clip_against_float64(ctx, nclips, clip):
    assert clip in B.REPLAY_CLIPS                      # the CPU file holds the reference to the bound on exactly these clips
    _run(ctx.eng, B.clips(nclips))
    feats = torch.from_numpy(ctx.eng.whisper_debug_get_clip("input_features", clip, (80, 3000)))[None]
    rp, miss = B.replay(ctx.sd, feats, lambda name, shape: ctx.eng.whisper_debug_get_clip(name, clip, shape), R, WO)
    for line in R.format_records(f"whisper x{nclips} clip {clip}", rp.records):
        print(line)
    assert not miss, miss
    bad = R.failures(rp.records)
    assert not bad, "\n".join(bad)


# ------------------------------------------------------------------ 2. log-mel per clip
def test_logmel_of_every_clip_is_the_single_steps(ctx):
    """Loud, x 1e-3 and all-zero in one run: a maximum word shared between clips would clamp the quiet clip at the loud one's
    maximum - 8 and lift the silent one off its constant."""
    pcms = [B.clip(0), B.clip(1), np.zeros(B.LIVE, np.float32)]
    assert np.abs(pcms[0]).max() > 100 * np.abs(pcms[1]).max() > 0
    want = [ctx.single(0)[0], ctx.single(1)[0]]
    out = torch.zeros(BATCH, 50, 384, dtype=torch.float32, device="cuda")
    ctx.eng.whisper_step(pcms[2], BATCH, L, out.data_ptr())
    want.append(ctx.eng.whisper_debug_get("input_features", (80, 3000)))
    _run(ctx.eng, pcms)
    for c in range(3):
        got = ctx.eng.whisper_debug_get_clip("input_features", c, (80, 3000))
        assert got.tobytes() == want[c].tobytes(), f"clip {c}: {int((got != want[c]).sum())} of 240000 features differ from the single step's"
    assert np.all(want[2] == np.float32(-1.5))
    assert not np.array_equal(want[0], want[1])


# ------------------------------------------------------------------ 3. isolation
def test_a_clip_does_not_see_its_neighbours(ctx):
    mid = B.clip(1)
    a = _run(ctx.eng, [B.clip(0), mid, B.clip(2)])
    sa = [ctx.eng.whisper_debug_get_clip(n, 1, (384, 1500)) for n in STATES]
    b = _run(ctx.eng, [B.clip(3), mid, B.clip(5)])
    sb = [ctx.eng.whisper_debug_get_clip(n, 1, (384, 1500)) for n in STATES]
    for n, x, y in zip(STATES, sa, sb):
        assert x.tobytes() == y.tobytes(), n
    assert a[1].tobytes() == b[1].tobytes()
    assert not np.array_equal(a[0], b[0]) and not np.array_equal(a[2], b[2])


# ------------------------------------------------------------------ 4. against the library
def test_every_request_against_transformers(ctx):
    pcms = B.clips(3)
    got = _run(ctx.eng, pcms)
    for c, pcm in enumerate(pcms):
        feat_arr, hs, feats = WO.audio2feat(ctx.model, pcm)
        e_in = float(np.abs(ctx.eng.whisper_debug_get_clip("input_features", c, (80, 3000)) - feats[0].numpy()).max())
        print(f"[whisper batch] clip {c} ({len(pcm)} samples): input_features max abs err {e_in:.3e}")
        assert e_in <= 2e-3
        for i in range(5):
            r = _rel(ctx.eng.whisper_debug_get_clip(STATES[i], c, (384, 1500)), hs[i].numpy().T)
            print(f"[whisper batch] clip {c} hidden_states.{i} rel_l2={r:.3e}")
            assert r <= 1e-2
        ref = np.stack(WO.feature2chunks(feat_arr, BATCH, L))
        r = _rel(got[c], ref)
        print(f"[whisper batch] clip {c} chunks rel_l2={r:.3e}")
        assert got[c].shape == ref.shape == (BATCH, 50, 384) and r <= 1e-2


# ------------------------------------------------------------------ 5. chunk gather per request
def test_every_request_gathers_its_own_rows_into_its_own_output(ctx):
    """Different batch / row_step / rows per request, a negative first row and windows past row 1499: every output equals the host
    gather of its own clip's hidden states exactly (fp16 -> fp32 is exact), and nothing is written outside it."""
    specs = [(16, -7, 2, 10), (3, 1490, 5, 64), (1, 10, 1, 1)]
    guard = 1024
    bufs, views = [], []
    for b, _, _, rows in specs:
        n = b * rows * 5 * 384
        t = torch.full((guard + n + guard,), float("nan"), dtype=torch.float32, device="cuda")
        t[guard: guard + n] = 0.0
        bufs.append(t)
        views.append(t[guard: guard + n])
    pcms = B.clips(3)
    ctx.eng.whisper_step_batch([(p, b, fr, st, rows, v.data_ptr()) for p, (b, fr, st, rows), v in zip(pcms, specs, views)])
    for c, ((b, fr, st, rows), t) in enumerate(zip(specs, bufs)):
        states = [ctx.eng.whisper_debug_get_clip(n, c, (384, 1500)) for n in STATES]
        want = B.host_chunks(states, b, fr, st, rows)
        h = t.cpu().numpy()
        got = h[guard: guard + want.size].reshape(want.shape)
        assert got.tobytes() == want.tobytes(), f"request {c}"
        assert np.isnan(h[:guard]).all() and np.isnan(h[guard + want.size:]).all(), f"request {c}: a guard block was written"


# ------------------------------------------------------------------ 6. one request is the single path
def test_one_request_is_whisper_step_and_builds_nothing(ctx):
    eng = ctx.new_engine()
    try:
        assert eng.whisper_batch_info() == {"capacity": 16, "built": 0, "activation_bytes": 0}
        got = _run(eng, [B.clip(1)])[0]
        assert eng.whisper_batch_info()["built"] == 0
        out = torch.zeros(BATCH, 50, 384, dtype=torch.float32, device="cuda")
        eng.whisper_step(B.clip(1), BATCH, L, out.data_ptr())
        assert got.tobytes() == out.cpu().numpy().tobytes()
        assert got.tobytes() == ctx.single(1)[1].tobytes()                 # ... and another engine's
        with pytest.raises(Exception, match="no batched Whisper run yet"):
            eng.whisper_debug_get_clip("input_features", 0, (80, 3000))
    finally:
        eng.close()


# ------------------------------------------------------------------ 7. 17 requests run as 16 + 1
def test_seventeen_requests_run_as_sixteen_and_one(ctx):
    assert ctx.eng.whisper_batch_plan(17) == [(True, list(range(16))), (False, [16])]
    pcms = [B.clip(i % 3) for i in range(17)]
    got = _run(ctx.eng, pcms, fill=float("nan"))
    info = ctx.eng.whisper_batch_info()
    assert info["capacity"] == 16 and info["built"] == 1 and info["activation_bytes"] > 0
    print(f"[whisper batch] activation_bytes {info['activation_bytes']} ({info['activation_bytes'] / 16 / 1e6:.1f} MB per clip)")
    for r, g in enumerate(got):
        assert np.isfinite(g).all(), f"request {r} is incomplete"
        want = ctx.single(r % 3)[1]
        assert _rel(g, want) <= 1e-2, f"request {r}"
    assert got[16].tobytes() == ctx.single(16 % 3)[1].tobytes()           # the run of one took the single-clip path
    assert ctx.eng.whisper_debug_get_clip("input_features", 15, (80, 3000)).tobytes() == ctx.single(0)[0].tobytes()
    with pytest.raises(Exception, match="carried 16 clips"):
        ctx.eng.whisper_debug_get_clip("input_features", 16, (80, 3000))


# ------------------------------------------------------------------ 8. graph replay
def test_a_repeated_call_replays_from_a_captured_graph(ctx):
    eng = ctx.new_engine()
    try:
        pcms = B.clips(2)
        n0 = eng.program_graph_count()
        runs = [_run(eng, pcms) for _ in range(3)]
        assert eng.program_graph_count() > n0
        for a, b in zip(runs[0], runs[2]):
            assert a.tobytes() == b.tobytes()
    finally:
        eng.close()


# ------------------------------------------------------------------ 9. refusals
@pytest.mark.parametrize("bad,code", [(dict(d_out=None), -1), (dict(n_samples=0), -1), (dict(n_samples=479001), -1), (dict(rows=65), -1),
                                      (dict(batch=0), -1)])
def test_a_bad_request_is_refused_before_anything_is_launched(ctx, bad, code):
    from livetalking_amd import _lib
    pcm = np.zeros(479001, np.float32)
    pcm[:B.LIVE] = B.clip(1)
    outs = _outs([(BATCH, L, 2, 10)] * 3)
    reqs = (_lib.WhisperReq * 3)()
    for r, o in zip(reqs, outs):
        r.pcm, r.n_samples, r.batch, r.first_row, r.row_step, r.rows, r.d_out = pcm.ctypes.data, B.LIVE, BATCH, L, 2, 10, o.data_ptr()
    for k, v in bad.items():
        setattr(reqs[1], k, v)
    assert ctx.eng._lib.ltk_whisper_step_batch(ctx.eng._h, reqs, 3) == code
    assert b"bad request 1" in ctx.eng._lib.ltk_last_error()
    ctx.eng.sync()
    for o in outs:
        assert not o.any().item()
    good = _run(ctx.eng, [pcm[:B.LIVE]] * 2)
    assert _rel(good[0], ctx.single(1)[1]) <= 1e-2 and good[0].tobytes() == good[1].tobytes()


def test_a_call_without_an_encoder_is_a_state_error():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from livetalking_amd.engine import Engine
    eng = Engine(0)
    try:
        out = torch.zeros(2, BATCH, 50, 384, dtype=torch.float32, device="cuda")
        with pytest.raises(Exception) as ei:
            eng.whisper_step_batch([(B.clip(0), BATCH, L, 2, 10, out[i].data_ptr()) for i in range(2)])
        assert getattr(ei.value, "code", None) == -3
        assert not out.any().item()
    finally:
        eng.close()


# ------------------------------------------------------------------ 10. plugin
def test_four_sessions_share_encoder_runs_through_the_plugin(ctx, monkeypatch):
    from livetalking_amd.avatars.audio_features import whisper as wh
    from livetalking_amd.scheduler import get_scheduler
    monkeypatch.setattr(wh, "_WHISPER_BATCH", True)
    Bs, steps, S = 4, 3, 4
    opt = types.SimpleNamespace(fps=25, batch_size=Bs, l=L, r=10)
    ap = types.SimpleNamespace(engine=ctx.eng)
    n_chunks = opt.l + opt.r + steps * 2 * Bs

    def session(s):
        asr = wh.WhisperASR(opt, None, ap)
        audio = synth.synthetic_audio(2.0, seed=300 + s)
        for k in range(n_chunks):
            asr.put_audio_frame(audio[k * 320: (k + 1) * 320], {})
        asr.warm_up()
        return asr

    def step(asr):
        asr.run_step()
        return asr.feat_queue.get(timeout=20)

    alone = [[step(asr).cpu().numpy() for _ in range(steps)] for asr in (session(s) for s in range(S))]
    sch = get_scheduler(ctx.eng, "whisper")
    sch.stats["max_requests_per_call"] = 0
    got, errs = [[] for _ in range(S)], []
    barrier = threading.Barrier(S)

    def run(s, asr):
        try:
            for _ in range(steps):
                barrier.wait(timeout=20)
                got[s].append(step(asr))
        except Exception as ex:  # noqa: BLE001
            errs.append(ex)
            barrier.abort()

    ts = [threading.Thread(target=run, args=(s, session(s))) for s in range(S)]
    for t in ts:
        t.start()
    for t in ts:
        t.join(timeout=60)
        assert not t.is_alive()
    assert not errs, errs
    assert sch.stats["max_requests_per_call"] > 1, sch.stats
    ptrs = set()
    for s in range(S):
        assert len(got[s]) == steps
        for k, t in enumerate(got[s]):
            assert tuple(t.shape) == (Bs, 50, 384) and t.is_cuda and t.dtype == torch.float32
            ptrs.add(t.data_ptr())
            assert _rel(t.cpu().numpy(), alone[s][k]) <= 1e-2, f"session {s} step {k}"
    assert len(ptrs) == S * steps                                           # every step's tensor is its own
