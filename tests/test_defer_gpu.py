"""Knob DEFER on the GPU (include/ltk.h ltk_wav2lip_infer_deferred): a lone session's call returns with its own pass in flight, once
the pass before it is complete.  Everything is compared byte for byte with the same calls under DEFER=0 (each call waits for its
own pass), at the smallest shapes at which it can go wrong: synthetic weights, a 5-frame bank with a 96 x 128 full frame,
max_frames = 4, calls of 1, 2 and 3 frames."""
import argparse
import ctypes as C

import numpy as np
import pytest
import synth_inputs as synth
import torch

pytestmark = pytest.mark.gpu

BANK, HW, BOX = 5, (96, 128), 48
WALK = 14
JUMP_AT, JUMP_BY = 11, 7          # calls 0..10 continue (slots 1 2 3 three times over: eager, captured, replayed), call 11 jumps


def _mels(n, B, seed):
    g = np.random.default_rng(seed)
    return [torch.from_numpy(g.standard_normal((B, 80, 16)).astype(np.float32)).cuda() for _ in range(n)]


def _preds(n, B):
    p = [torch.zeros(B, 256, 256, 3, dtype=torch.uint8, device="cuda") for _ in range(n)]
    torch.cuda.synchronize()      # the fills are done before any pass may write
    return p


def _read(eng, t):
    """The frames of `t` on the host, read on torch's current stream behind the pass that writes them: GPU-side order
    (Engine.order_frames), no host synchronisation."""
    eng.order_frames(t.data_ptr(), t.numel())
    return t.cpu()


def _walk_indices(B):
    idx, out = 0, []
    for k in range(WALK):
        if k == JUMP_AT:
            idx += JUMP_BY
        out.append(idx)
        idx += B
    return out


@pytest.fixture(scope="module")
def rig():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from livetalking_amd.engine import Engine
    eng = Engine(0)
    eng.load_wav2lip(synth.wav2lip_state_dict(1234), max_frames=4)
    eng.defer_handles = True          # every reader below goes through the engine or through order_frames
    frames, faces, coords = synth.wav2lip_avatar(n_frames=BANK, full_hw=HW, box=BOX, seed=3)
    aid = eng.register_avatar(faces, frames, coords)
    yield eng, aid, (frames, faces, coords)
    Engine.set_knob("DEFER", 1)
    eng.close()


def _run_walk(eng, aid, B, mels, defer, read_each):
    """The 14-call walk; read_each: every call's frames are read on torch's stream right behind the call, with no host synchronisation
    (else: all of them after ltk_engine_sync)."""
    from livetalking_amd.engine import Engine
    Engine.set_knob("DEFER", defer)
    preds = _preds(WALK, B)
    outs = []
    for k, index in enumerate(_walk_indices(B)):
        eng.wav2lip_infer([(aid, index, B, mels[k].data_ptr(), preds[k].data_ptr())])
        if read_each:
            outs.append(_read(eng, preds[k]))
    if not read_each:
        eng.sync()
        outs = [p.cpu() for p in preds]
    return outs


@pytest.mark.parametrize("B", [1, 2, 3])
def test_walk_equals_synchronous_calls(rig, B):
    """14 consecutive calls of one session: both mirror turns of the 5-frame bank, three times round the 3-slot rotation (every
    launch variant run eagerly, captured, replayed), one index jump (a miss that runs the whole pass).  Every call's frames equal
    the same walk with DEFER=0 - read after the walk, and read behind each call with no synchronisation - the counters show that
    the calls were deferred and that at most one pass was outstanding whenever one returned."""
    eng, aid, _ = rig
    mels = _mels(WALK, B, 10 + B)
    ref = _run_walk(eng, aid, B, mels, 0, False)
    st0 = eng.defer_stats()
    assert st0["outstanding"] == 0
    got = _run_walk(eng, aid, B, mels, 1, False)
    st1 = eng.defer_stats()
    got_each = _run_walk(eng, aid, B, mels, 1, True)
    print(f"[defer walk B={B}] {st0} -> {st1}")
    for k in range(WALK):
        assert torch.equal(got[k], ref[k]), f"call {k}: {int((got[k].to(torch.int16) - ref[k].to(torch.int16)).abs().max())} LSB"
        assert torch.equal(got_each[k], ref[k]), f"call {k}, read behind the call"
    assert not torch.equal(ref[0], ref[1]) and int(ref[0].max()) > 0
    assert st1["deferred"] - st0["deferred"] == WALK
    assert st1["max_outstanding"] == 1 and st1["outstanding"] == 0


def test_consumers_order_behind_the_pass(rig):
    """paste_back_batch / paste_back (the engine's own streams: they order themselves) and a torch read on torch's stream behind
    Engine.order_frames, right behind a deferred call with no host synchronisation, against the synchronous path.  (The plugin's
    handles issue that order themselves: test_plugin_loop_knob_on_equals_off reads torch.stack(pred).cpu() with nothing in front.)"""
    from livetalking_amd.engine import Engine
    eng, aid, _ = rig
    B = 3
    mels = _mels(4, B, 77)
    H, W = HW

    def run(defer):
        Engine.set_knob("DEFER", defer)
        preds = _preds(4, B)
        res = []
        for k in range(4):
            index = 20 + k * B
            eng.wav2lip_infer([(aid, index, B, mels[k].data_ptr(), preds[k].data_ptr())])
            idx = [((index + i) % BANK if ((index + i) // BANK) % 2 == 0 else BANK - (index + i) % BANK - 1) for i in range(B)]
            host = torch.empty((B, H, W, 3), dtype=torch.uint8, pin_memory=True)
            eng.paste_back_batch(aid, idx, preds[k].data_ptr(), host.data_ptr())
            one = np.empty((H, W, 3), dtype=np.uint8)
            eng.paste_back(aid, idx[1], preds[k][1].data_ptr(), one)
            eng.order_frames(preds[k].data_ptr(), preds[k].numel())
            res.append((host.clone(), one, torch.stack(list(preds[k].unbind(0))).cpu()))
        eng.sync()
        return res

    ref, got = run(0), run(1)
    for k in range(4):
        assert torch.equal(got[k][0], ref[k][0]) and np.array_equal(got[k][1], ref[k][1]) and torch.equal(got[k][2], ref[k][2]), k
        assert np.array_equal(ref[k][0][1].numpy(), ref[k][1])
    assert int(ref[0][2].max()) > 0


def test_release_knob_toggle_and_sync_drain_the_pass_in_flight(rig):
    from livetalking_amd.engine import Engine, LtkError
    eng, aid, (frames, faces, coords) = rig
    B = 2
    mels = _mels(6, B, 5)
    Engine.set_knob("DEFER", 0)
    ref = _preds(6, B)
    for k in range(6):
        eng.wav2lip_infer([(aid, 3 + 2 * k, B, mels[k].data_ptr(), ref[k].data_ptr())])
    ref = [r.cpu() for r in ref]
    Engine.set_knob("DEFER", 1)
    # release right behind a deferred call: the pass holds the bank; the id is gone afterwards
    aid2 = eng.register_avatar(faces, frames, coords)
    preds = _preds(6, B)
    eng.wav2lip_infer([(aid2, 3, B, mels[0].data_ptr(), preds[0].data_ptr())])
    assert eng.defer_stats()["outstanding"] == 1
    eng.release_avatar(aid2)
    assert eng.defer_stats()["outstanding"] == 0
    assert torch.equal(preds[0].cpu(), ref[0])
    with pytest.raises(LtkError) as ei:
        eng.wav2lip_infer([(aid2, 5, B, mels[1].data_ptr(), preds[1].data_ptr())])
    assert ei.value.code == -3
    # ltk_engine_sync drains
    eng.wav2lip_infer([(aid, 5, B, mels[1].data_ptr(), preds[1].data_ptr())])
    assert eng.defer_stats()["outstanding"] == 1
    eng.sync()
    assert eng.defer_stats()["outstanding"] == 0
    assert torch.equal(preds[1].cpu(), ref[1])
    # a knob toggle: the next call finds the engine drained and, with the knob off, waits for its own pass
    eng.wav2lip_infer([(aid, 7, B, mels[2].data_ptr(), preds[2].data_ptr())])
    assert eng.defer_stats()["outstanding"] == 1
    Engine.set_knob("DEFER", 0)
    eng.wav2lip_infer([(aid, 9, B, mels[3].data_ptr(), preds[3].data_ptr())])
    assert eng.defer_stats()["outstanding"] == 0
    Engine.set_knob("DEFER", 1)
    eng.wav2lip_infer([(aid, 11, B, mels[4].data_ptr(), preds[4].data_ptr())])
    eng.wav2lip_infer([(aid, 13, B, mels[5].data_ptr(), preds[5].data_ptr())])
    assert eng.defer_stats()["outstanding"] == 1
    for k in range(2, 6):
        assert torch.equal(_read(eng, preds[k]), ref[k]), k


def test_deferred_then_two_request_call_and_back(rig):
    from livetalking_amd.engine import Engine
    eng, aid, _ = rig
    B = 2
    mels = _mels(6, B, 21)

    def run(defer):
        Engine.set_knob("DEFER", defer)
        p = _preds(6, B)
        eng.wav2lip_infer([(aid, 0, B, mels[0].data_ptr(), p[0].data_ptr())])
        eng.wav2lip_infer([(aid, 2, B, mels[1].data_ptr(), p[1].data_ptr())])
        eng.wav2lip_infer([(aid, 4, B, mels[2].data_ptr(), p[2].data_ptr()), (aid, 1, B, mels[3].data_ptr(), p[3].data_ptr())])
        mid = eng.defer_stats()["outstanding"]
        eng.wav2lip_infer([(aid, 6, B, mels[4].data_ptr(), p[4].data_ptr())])
        eng.wav2lip_infer([(aid, 8, B, mels[5].data_ptr(), p[5].data_ptr())])
        out = [_read(eng, q) for q in p]
        eng.sync()
        return out, mid

    (ref, _), (got, mid) = run(0), run(1)
    assert mid == 0            # the synchronous call ran behind the pass in flight and retired it
    for k in range(6):
        assert torch.equal(got[k], ref[k]), k


def test_bad_request_while_a_pass_is_pending(rig):
    from livetalking_amd.engine import Engine, LtkError
    eng, aid, _ = rig
    B = 3
    mels = _mels(3, B, 31)
    Engine.set_knob("DEFER", 0)
    ref = _preds(3, B)
    for k in range(3):
        eng.wav2lip_infer([(aid, 1 + 3 * k, B, mels[k].data_ptr(), ref[k].data_ptr())])
    ref = [r.cpu() for r in ref]
    Engine.set_knob("DEFER", 1)
    p = _preds(3, B)
    eng.wav2lip_infer([(aid, 1, B, mels[0].data_ptr(), p[0].data_ptr())])
    assert eng.defer_stats()["outstanding"] == 1
    with pytest.raises(LtkError) as ei:
        eng.wav2lip_infer([(987654, 4, B, mels[1].data_ptr(), p[1].data_ptr())])
    assert ei.value.code == -3 and "unknown avatar" in str(ei.value)
    assert eng.defer_stats()["outstanding"] == 0            # nothing is in flight after an error return
    assert torch.equal(p[0].cpu(), ref[0])
    with pytest.raises(LtkError):
        eng.wav2lip_infer([(aid, 4, 5, mels[1].data_ptr(), p[1].data_ptr())])        # more frames than max_frames
    for k in (1, 2):
        eng.wav2lip_infer([(aid, 1 + 3 * k, B, mels[k].data_ptr(), p[k].data_ptr())])
        assert torch.equal(_read(eng, p[k]), ref[k]), k


def test_no_capture_after_the_rotation_has_been_walked():
    """A fresh engine, one session, back-to-back deferred calls: graph_count() stops growing at the call the slot rule says it must
    (ltk_debug_solo_walk: the same header the engine runs), and that call is within a benchmark's 8 priming + 5 warm-up calls."""
    from livetalking_amd import _lib
    from livetalking_amd.engine import Engine
    lib = _lib.load()
    used = C.c_int(0)
    last = lib.ltk_debug_solo_walk(1, WALK, -1, C.byref(used))
    assert 0 < last + 1 <= 13 and used.value == 3
    B = 2
    Engine.set_knob("DEFER", 1)
    eng = Engine(0)
    try:
        eng.load_wav2lip(synth.wav2lip_state_dict(1234), max_frames=4)
        eng.defer_handles = True
        frames, faces, coords = synth.wav2lip_avatar(n_frames=BANK, full_hw=HW, box=BOX, seed=3)
        aid = eng.register_avatar(faces, frames, coords)
        mels = _mels(WALK, B, 41)
        p = _preds(WALK, B)
        for k in range(last + 1):
            eng.wav2lip_infer([(aid, k * B, B, mels[k].data_ptr(), p[k].data_ptr())])
        after_rotation = eng.graph_count()
        for k in range(last + 1, WALK):
            eng.wav2lip_infer([(aid, k * B, B, mels[k].data_ptr(), p[k].data_ptr())])
        st = eng.prefetch_stats()
        print(f"[defer captures] last capture at call {last}, {after_rotation} graphs, {st}")
        assert eng.graph_count() == after_rotation == 1 + 2 * used.value      # the whole pass + per slot: decoder pass, prefetch
        assert st["hits"] == WALK - 2
    finally:
        eng.close()


def test_plugin_loop_knob_on_equals_off():
    """LipReal.inference_batch with device mel, 10 back-to-back calls; right behind each call, with nothing in front, the handles
    are read on torch's stream (torch.stack(pred).cpu(): the handles order that stream behind their pass) and composited through
    paste_back_frame."""
    import livetalking_amd.avatars.wav2lip_avatar as plugin
    from livetalking_amd.engine import Engine
    B = 2
    model = plugin.load_model(None, state_dict=synth.wav2lip_state_dict(1234), max_frames=4, device=0)
    try:
        avatar = synth.wav2lip_avatar(n_frames=BANK, full_hw=HW, box=BOX, seed=3)
        sess = plugin.LipReal(argparse.Namespace(fps=25, batch_size=B, l=10, r=10, sessionid=0), model, avatar)
        mels = _mels(10, B, 51)

        def run(defer):
            Engine.set_knob("DEFER", defer)
            res = []
            for k in range(10):
                pred = sess.inference_batch(k * B, mels[k])
                full = sess.paste_back_frame(pred[1], plugin.mirror_index(BANK, k * B + 1)).copy()
                res.append((torch.stack(pred).cpu(), full))
                assert isinstance(pred[0], torch.Tensor) and pred[0].dtype == torch.uint8 and tuple(pred[0].shape) == (256, 256, 3)
            model.engine.sync()
            return res

        ref = run(0)
        d0 = model.engine.defer_stats()["deferred"]
        got = run(1)
        assert model.engine.defer_stats()["deferred"] - d0 == 10
        for k in range(10):
            assert torch.equal(got[k][0], ref[k][0]) and np.array_equal(got[k][1], ref[k][1]), k
    finally:
        Engine.set_knob("DEFER", 1)
        for e in model.engines:
            e.close()


def test_dropped_handles_keep_their_block_until_the_pass_is_complete():
    """A caller that drops its handles at once (a benchmark loop does): the frame block must not go back to torch's allocator while
    the engine still writes it, or the next allocation on torch's stream - here a block of 7s of the same size - is handed the same
    memory and the pass scribbles over it."""
    import livetalking_amd.avatars.wav2lip_avatar as plugin
    from livetalking_amd.engine import Engine
    B = 3
    Engine.set_knob("DEFER", 1)
    model = plugin.load_model(None, state_dict=synth.wav2lip_state_dict(1234), max_frames=4, device=0)
    try:
        avatar = synth.wav2lip_avatar(n_frames=BANK, full_hw=HW, box=BOX, seed=3)
        sess = plugin.LipReal(argparse.Namespace(fps=25, batch_size=B, l=10, r=10, sessionid=0), model, avatar)
        mels = _mels(8, B, 61)
        sevens = []
        d0 = model.engine.defer_stats()["deferred"]
        for k in range(8):
            pred = sess.inference_batch(k * B, mels[k])
            del pred
            sevens.append(torch.full((B, 256, 256, 3), 7, dtype=torch.uint8, device="cuda"))
        assert model.engine.defer_stats()["deferred"] - d0 == 8
        model.engine.sync()
        torch.cuda.synchronize()
        for k, t in enumerate(sevens):
            assert bool((t == 7).all()), k
    finally:
        for e in model.engines:
            e.close()
