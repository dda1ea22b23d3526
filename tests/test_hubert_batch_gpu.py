"""GPU tests of the batched HuBERT live step (ltk_hubert_step_batch): every clip of every batch against the float64 reference of
THAT clip alone, through the gates of tests/hubert_batch_cases.py (the ones tests/test_hubert_batch_host.py shows to reject a
statistics, padding, stride, attention, clamp or routing fault across clips).  One engine with the seeded 2-layer model (module
scope); the 24-layer test brings its own."""
from __future__ import annotations

import threading
import types

import numpy as np
import pytest
import torch

import hubert_batch_cases as B
import hubert_ref as H
from oracle import op_replay as R

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def sd2():
    return H.state_dict(2, 20)


@pytest.fixture(scope="module")
def eng(sd2):
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from livetalking_amd.engine import Engine
    e = Engine(0)
    e.load_hubert(sd2)
    yield e
    e.close()


def _step_batch(eng, pcms, specs=None):
    """One hubert_step_batch call -> the device chunks of every request (host arrays) and the specs used."""
    specs = specs or [B.chunk_spec(i, len(p)) for i, p in enumerate(pcms)]
    outs = [torch.zeros(b, rows, 1024, dtype=torch.float32, device="cuda") for b, _, _, rows in specs]
    eng.hubert_step_batch([(p, b, fr, st, rows, o.data_ptr()) for p, (b, fr, st, rows), o in zip(pcms, specs, outs)])
    return [o.cpu().numpy() for o in outs], specs


def _get(eng, clip):
    return lambda name, shape: eng.hubert_debug_get_clip(name, clip, shape)


# ------------------------------------------------------------------ 1, 2: every op and the statistics of every clip
@pytest.mark.parametrize("nf,n", B.REPLAY_CASES)
def test_every_op_of_every_clip_against_float64(eng, sd2, nf, n):
    """Teacher-forced replay per clip on the device's own input_values of that clip: 3 rows (nearly every positional tap is padding:
    a neighbour's rows read instead show at full size), 51 (live: the row GEMM over nf x 51 rows), 70 (no row plan: conv3 over nf
    images), and 11 clips of 51 rows (561 rows: past kLinFkMinRows).  Also the first time the head-64 attention runs with nf > 1."""
    pcms = B.clips(nf, n)
    _step_batch(eng, pcms)
    ops = eng.hubert_ops()
    assert [nm for nm, _ in ops] == H.op_names(2)
    for i in range(nf):
        label = f"nf={nf} n={n} clip {i}"
        x_norm = eng.hubert_debug_get_clip("input_values", i, (n,))
        B.gate_input_values(x_norm, pcms[i], label)
        B.gate_replay(sd2, x_norm, _get(eng, i), ops, label)


@pytest.fixture(scope="module")
def normalised(eng):
    """Three clips at 3 rows and at the live length, clip 1 at a DC offset of 100 next to the zero-mean clip 0, gains 0.1 .. 3:
    [(label, clip index, pcm, input_values of the batched run, input_values of the single-clip path on that clip alone)]."""
    out = []
    for n in (B.ROWS3, B.LIVE):
        pcms = B.clips(3, n, seed=300)
        _step_batch(eng, pcms)
        got = [eng.hubert_debug_get_clip("input_values", i, (n,)) for i in range(3)]
        d_out = torch.zeros(2, 16, 1024, dtype=torch.float32, device="cuda")
        for i, pcm in enumerate(pcms):
            eng.hubert_step(pcm, 2, 0, d_out.data_ptr())
            out.append((f"n={n} clip {i}", i, pcm, got[i], eng.hubert_debug_get("input_values", (n,))))
    return out


def test_statistics_are_per_clip(normalised):
    """Every clip's normalised waveform equals, byte for byte, what the single-clip path (ltk_hubert_step) makes of that clip alone,
    and is held to H.normalise of that clip alone at rel L2 <= 1e-6, the gate of test_hubert_gpu - the clip at + 100 next to the
    zero-mean one included.  A mean of 100 is stored in fp32 to half an ulp of 7.6e-6, which x - mean alone would carry whole into
    a waveform whose deviation is a few tenths (2.1e-6 .. 8.1e-6 rel L2 were measured that way); both paths take the residual of the
    stored mean off the centred sample (hubert_kernels.h)."""
    for label, i, pcm, x_dev, alone in normalised:
        assert np.array_equal(x_dev, alone), f"{label}: not the bytes of the clip normalised alone"
        B.gate_input_values(x_dev, pcm, label)


# ------------------------------------------------------------------ 3, 4: isolation and the single path
@pytest.mark.parametrize("n", [B.ROWS3, B.LIVE])
def test_a_clip_does_not_see_its_neighbours(eng, n):
    """Clip 1 fixed, clips 0 and 2 replaced (another seed, gain and offset): clip 1's chunks are the same bytes."""
    a = B.clips(3, n, seed=400)
    b = B.clips(3, n, seed=500)
    b[1] = a[1]
    b[0], b[2] = (b[0] * 2.5 - 40.0).astype(np.float32), (b[2] * 0.3 + 7.0).astype(np.float32)
    out_a, specs = _step_batch(eng, a)
    out_b, _ = _step_batch(eng, b, specs)
    assert np.abs(out_a[1]).max() > 0.1 and not np.array_equal(out_a[0], out_b[0])
    assert np.array_equal(out_a[1], out_b[1])


def test_one_request_is_the_single_path(eng):
    pcm = B.clips(1, B.LIVE, seed=600)[0]
    (got,), ((b, fr, st, rows),) = _step_batch(eng, [pcm])
    want = torch.zeros(b, rows, 1024, dtype=torch.float32, device="cuda")
    eng.hubert_step(pcm, b, fr, want.data_ptr(), row_step=st, rows=rows)
    assert np.abs(got).max() > 0.1 and np.array_equal(got, want.cpu().numpy())


# ------------------------------------------------------------------ 5: plan edges
def _check_chunks(eng, pcms, label):
    outs, specs = _step_batch(eng, pcms)
    for r, (pcm, out, (b, fr, _, _)) in enumerate(zip(pcms, outs, specs)):
        T = H.rows(len(pcm))
        assert fr < 0, "the first window starts left of the clip"
        assert fr + 2 * (b - 1) + 16 > T, "the last window ends right of the clip"
        B.gate_chunks(out, eng.hubert_features(pcm), b, fr, f"{label} req {r} ({len(pcm)} samples)")


def test_seventeen_requests_run_as_sixteen_and_one(eng):
    pcms = B.clips(17, B.ROWS3, seed=700)
    _check_chunks(eng, pcms, "17 x 1040")
    assert eng.hubert_batch_info()["capacity"] == B.CAPACITY


def test_mixed_lengths_reach_their_own_requests(eng):
    """[1040, 16640, 1040, 22613, 16640]: two batched runs and a single one, every request with its own batch and first_row."""
    pcms = [None] * len(B.MIXED)
    for n in dict.fromkeys(B.MIXED):
        members = [r for r, m in enumerate(B.MIXED) if m == n]
        for pcm, r in zip(B.clips(len(members), n, seed=800 + n % 89), members):
            pcms[r] = pcm
    _check_chunks(eng, pcms, "mixed")


# ------------------------------------------------------------------ 6: end to end
def test_end_to_end_24_layers_two_live_clips():
    """24 layers, two live-length clips in one run: per clip, rel L2 against the float64 forward of that clip <= AGG_FACTOR x the
    fp16 rounding model's own (the gate of test_hubert_gpu._end_to_end)."""
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from livetalking_amd.engine import Engine
    sd = H.state_dict(24, 7)
    pcms = B.clips(2, B.LIVE, seed=12)
    T = H.rows(B.LIVE)
    e = Engine(0)
    try:
        e.load_hubert(sd)
        specs = [(1, 0, 0, T)] * 2                               # one frame of rows [0, T): the whole last_hidden_state
        outs, _ = _step_batch(e, pcms, specs)
        assert e.hubert_batch_info()["programs"] == 1 and e.hubert_info()["programs"] == 0
        for i, (pcm, out) in enumerate(zip(pcms, outs)):
            ref = H.features(sd, pcm)
            model = H.features(sd, pcm, fp16_model=True)
            r_dev = R.rel_l2(torch.from_numpy(out[0]), torch.from_numpy(ref))
            r_mod = R.rel_l2(torch.from_numpy(model), torch.from_numpy(ref))
            print(f"24 layers clip {i}: rel_l2 dev {r_dev:.3e}, fp16 model {r_mod:.3e} (gate {R.AGG_FACTOR * r_mod:.3e})")
            assert out[0].shape == ref.shape
            assert r_dev <= R.AGG_FACTOR * r_mod
    finally:
        e.close()


# ------------------------------------------------------------------ 7: refusals
def test_refusals_launch_nothing_and_leave_the_engine_usable(eng):
    from livetalking_amd._lib import LtkError
    from livetalking_amd.engine import Engine
    good = B.clips(3, B.ROWS3, seed=900)
    want, specs = _step_batch(eng, good)
    out = torch.zeros(4, 16, 1024, dtype=torch.float32, device="cuda")

    def refused(reqs, code=-1):
        with pytest.raises(LtkError) as ex:
            eng.hubert_step_batch(reqs)
        assert ex.value.code == code
        assert not out.any()                                 # nothing was launched into the good requests' buffer either
        got, _ = _step_batch(eng, good, specs)               # a following good call succeeds, same bytes
        assert all(np.array_equal(a, b) for a, b in zip(got, want))

    ok = (good[0], 4, 0, 2, 16, out.data_ptr())
    refused([ok, (good[1], 4, 0, 2, 16, 0)])                                      # null d_out
    refused([ok, (np.zeros(399, np.float32), 4, 0, 2, 16, out.data_ptr())])
    refused([ok, (np.zeros(320000, np.float32), 4, 0, 2, 16, out.data_ptr())])
    refused([ok, (good[1], 0, 0, 2, 16, out.data_ptr())])                          # batch <= 0
    refused([ok, (good[1], -1, 0, 2, 16, out.data_ptr())])
    with pytest.raises(LtkError) as ex:
        eng.hubert_step_batch([])                                                  # nreq <= 0
    assert ex.value.code == -1
    e = Engine(0)
    try:
        with pytest.raises(LtkError) as ex:                                        # no model loaded
            e.hubert_step_batch([ok, ok])
        assert ex.value.code == -3 and not out.any()
    finally:
        e.close()


# ------------------------------------------------------------------ 8: cache and accounting
def test_batched_programs_have_their_own_cache(eng):
    before = eng.hubert_info()["programs"]
    for n in (B.ROWS3, B.LIVE, B.ROWS70):
        _step_batch(eng, B.clips(2, n, seed=1000))
        info = eng.hubert_batch_info()
        assert 1 <= info["programs"] <= 2
        _, clip_bytes = B.device_plan([n], 2)
        assert info["activation_bytes"] == clip_bytes[0] * B.CAPACITY < B.BUDGET
    assert eng.hubert_batch_info()["programs"] == 2
    assert eng.hubert_info()["programs"] == before           # the single-clip programs are not touched, nor counted together


# ------------------------------------------------------------------ 9: plugin
def test_four_sessions_share_forwards_through_the_scheduler(eng, monkeypatch):
    """Four HubertASR instances over ONE EngineAudio2Feature step from four threads: the "hubert" scheduler carries more than one
    request in a call, and every session's chunks are its own host-side feature2chunks."""
    from livetalking_amd.avatars.audio_features import hubert as hub
    from livetalking_amd.scheduler import get_scheduler
    monkeypatch.setattr(hub, "_HUBERT_BATCH", True)
    proc = object.__new__(hub.EngineAudio2Feature)           # the engine already holds the model
    proc.engine = eng
    S, Bs, STEPS = 4, 4, 3
    opt = types.SimpleNamespace(fps=25, batch_size=Bs, l=10, r=10)
    asrs = [hub.HubertASR(opt, None, proc, audio_feat_length=[4, 4]) for _ in range(S)]
    seen = [[] for _ in range(S)]
    step = proc.step
    lock = threading.Lock()

    def spy(pcm, *a, **k):
        sid = int(round(float(pcm[0])))                      # the first sample of a session's audio carries its number
        with lock:
            seen[sid].append(np.array(pcm))
        return step(pcm, *a, **k)
    proc.step = spy
    for sid, asr in enumerate(asrs):
        audio = H.speech((20 + 2 * Bs * STEPS) * 320, 50 + sid) * (0.5 + sid)
        audio[::320] = sid                                   # every chunk starts with the session's number
        for f in np.split(audio.astype(np.float32), len(audio) // 320):
            asr.put_audio_frame(f, {})
        asr.warm_up()
    got = [[] for _ in range(S)]
    barrier = threading.Barrier(S)
    errs = []

    def session(sid):
        try:
            for _ in range(STEPS):
                barrier.wait(timeout=60)
                asrs[sid].run_step()
                got[sid].append(asrs[sid].feat_queue.get_nowait())
        except Exception as ex:  # noqa: BLE001
            errs.append(ex)
            barrier.abort()
    ts = [threading.Thread(target=session, args=(sid,)) for sid in range(S)]
    for t in ts:
        t.start()
    for t in ts:
        t.join(timeout=120)
        assert not t.is_alive()
    assert not errs, errs
    st = get_scheduler(eng, "hubert").stats
    print(f"hubert scheduler: {st}")
    assert st["requests"] == S * STEPS and st["max_requests_per_call"] > 1
    for sid in range(S):
        assert len(seen[sid]) == STEPS
        for pcm, chunks in zip(seen[sid], got[sid]):
            assert len(chunks) == Bs and all(c.is_cuda and c.shape == (16, 1024) for c in chunks)
            host = hub.feature2chunks(eng.hubert_features(pcm), Bs, [4, 4], opt.l / 2, 2)
            assert np.abs(host[0]).max() > 0.1
            assert all(np.array_equal(c.cpu().numpy(), h) for c, h in zip(chunks, host)), f"session {sid}"
