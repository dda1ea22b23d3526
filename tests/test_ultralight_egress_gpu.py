"""GPU tests of the Ultralight delivery path: ltk_ultralight_paste_back_batch, LTK_SRC_ULTRALIGHT through ltk_egress_frame and
ltk_egress_batch, and LightReal behind DeviceEgressMixin.  Every comparison is byte-exact: the composite is
oracle.paste_oracle.resize_linear_u8 of the 168x168 bank face with the prediction at [4:164, 4:164], pasted at (x1, y1, x2, y2)
(the construction of tests/test_ultralight_gpu.py::test_paste_back_is_byte_exact), followed by oracle.egress_oracle.  Engine of
its own (module scope); one bank of four frames per frame size, registered once."""
from __future__ import annotations

import threading
import time
import types

import numpy as np
import pytest

import synth_inputs as synth
from oracle import egress_oracle as eo
from oracle import paste_oracle

pytestmark = pytest.mark.gpu

N17 = 17
IDX17 = [2, 0, 3, 3, 1, 0, 2, 1, 3, 0, 0, 2, 1, 3, 2, 1, 0]        # unordered, repeats, crosses the 16-frame launch chunk


def _boxes(H, W):
    """The four boxes of the existing paste test: odd 71x93, touching the right and bottom edge, identity 168x168, 2x shrink 84x84."""
    return [(13, 9, 13 + 71, 9 + 93), (W - 100, H - 64, W, H), (20, 10, 20 + 168, 10 + 168), (20, 10, 20 + 84, 10 + 84)]


def _wm(seed=0):
    rng = np.random.default_rng(seed)
    return (rng.integers(0, 2, (9, 61), dtype=np.uint8) * 255).astype(np.uint8), 10, 12, (128, 128, 128)


def _composite(bank, idx, pred):
    x1, y1, x2, y2 = bank.boxes[idx]
    comp = bank.faces[idx].copy()
    comp[4:164, 4:164] = pred
    want = bank.frames[idx].copy()
    want[y1:y2, x1:x2] = paste_oracle.resize_linear_u8(comp, (x2 - x1, y2 - y1))
    return want


@pytest.fixture(scope="module")
def eng():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from livetalking_amd.engine import Engine
    e = Engine(0)
    yield e
    e.close()


@pytest.fixture(scope="module")
def sd():
    return synth.ultralight_state_dict(1234)


@pytest.fixture(scope="module")
def preds():
    """17 random predictions, host and device, shared and never written."""
    import torch
    p = np.random.default_rng(5).integers(0, 256, (N17, 160, 160, 3), dtype=np.uint8)
    return types.SimpleNamespace(host=p, dev=torch.from_numpy(p).cuda())


@pytest.fixture(scope="module")
def banks(eng, sd):
    """hw -> the four-frame bank of that frame size (registered on first use) and the oracle composites already computed for it."""
    made = {}

    def get(hw):
        if hw not in made:
            H, W = hw
            frames, faces, _ = synth.ultralight_avatar(4, hw, seed=21)
            boxes = _boxes(H, W)
            made[hw] = types.SimpleNamespace(H=H, W=W, frames=frames, faces=faces, boxes=boxes, composites={},
                                             aid=eng.register_ultralight_avatar(sd, faces, frames, boxes, max_frames=4))
        return made[hw]

    yield get
    for b in made.values():
        eng.release_avatar(b.aid)


def _want17(bank, preds):
    """The oracle composites of (IDX17[i], prediction i), computed once per bank."""
    for i in range(N17):
        if i not in bank.composites:
            bank.composites[i] = _composite(bank, IDX17[i], preds.host[i])
    return [bank.composites[i] for i in range(N17)]


# ------------------------------------------------------------------ batched paste-back
@pytest.mark.parametrize("hw", [(200, 260), (201, 263)])       # H*W*3 % 4 == 0: dword stores; odd: every second frame starts off a dword
def test_paste_back_batch_equals_oracle_and_per_frame(eng, banks, preds, hw):
    import torch
    bank = banks(hw)
    H, W = hw
    assert (H * W * 3) % 4 == 0 if hw == (200, 260) else (H * W * 3) % 2 == 1
    host = torch.zeros((N17, H, W, 3), dtype=torch.uint8, pin_memory=True)
    eng.ultralight_paste_back_batch(bank.aid, IDX17, preds.dev.data_ptr(), host.data_ptr())
    got = host.numpy()
    want = _want17(bank, preds)
    for i in range(N17):
        one = np.empty((H, W, 3), np.uint8)
        eng.ultralight_paste_back(bank.aid, IDX17[i], preds.dev[i].data_ptr(), one)
        assert np.array_equal(got[i], want[i]), f"frame {i} (bank {IDX17[i]}): {(got[i] != want[i]).sum()} bytes differ from the oracle"
        assert np.array_equal(got[i], one), f"frame {i} (bank {IDX17[i]}): differs from ltk_ultralight_paste_back"
    # n = 1
    single = torch.zeros((1, H, W, 3), dtype=torch.uint8, pin_memory=True)
    eng.ultralight_paste_back_batch(bank.aid, [IDX17[4]], preds.dev[4].data_ptr(), single.data_ptr())
    assert np.array_equal(single.numpy()[0], want[4])


def test_paste_back_batch_refusals_leave_the_engine_usable(eng, banks, preds):
    import torch
    from livetalking_amd._lib import LtkError
    bank = banks((200, 260))
    host = torch.zeros((2, 200, 260, 3), dtype=torch.uint8, pin_memory=True)
    for bad in ([0, 4], [-1, 0]):
        with pytest.raises(LtkError) as ex:
            eng.ultralight_paste_back_batch(bank.aid, bad, preds.dev.data_ptr(), host.data_ptr())
        assert ex.value.code == -1 and "index" in str(ex.value)
    with pytest.raises(LtkError) as ex:
        eng.ultralight_paste_back_batch(bank.aid, [], preds.dev.data_ptr(), host.data_ptr())
    assert ex.value.code == -1
    with pytest.raises(LtkError) as ex:
        eng.ultralight_paste_back_batch(bank.aid + 1000, [0, 1], preds.dev.data_ptr(), host.data_ptr())
    assert ex.value.code == -3
    assert not host.numpy().any()                                    # nothing was written by a refused call
    eng.ultralight_paste_back_batch(bank.aid, [1, 0], preds.dev.data_ptr(), host.data_ptr())
    assert np.array_equal(host.numpy()[0], _composite(bank, 1, preds.host[0]))
    assert np.array_equal(host.numpy()[1], _composite(bank, 0, preds.host[1]))


# ------------------------------------------------------------------ ltk_egress_frame
@pytest.mark.parametrize("hw", [(200, 260), (202, 262)])        # W % 4 == 0: dword kernels; 262: byte kernels (both even for I420)
def test_egress_frame_ultralight_formats_transition_watermark(eng, banks, preds, hw):
    """The seq of tests/test_egress_gpu.py::test_egress_wav2lip_sources_formats_transition with SRC_ULTRALIGHT: silent, switch to
    speaking with blends, back to silent, a custom host frame; oracle chain composite -> add_weighted_u8 -> egress_frame."""
    from livetalking_amd import egress
    bank = banks(hw)
    H, W = hw
    aid = bank.aid
    rng = np.random.default_rng(1)
    mask, wx, wy, col = _wm()
    comp = {idx: _composite(bank, idx, preds.host[idx]) for idx in range(4)}
    for fmt in ("bgr24", "i420"):
        for chroma in (0, 1):
            h = eng.egress_open(H, W)
            eng.egress_watermark(h, mask, wx, wy, col)
            fcode = egress.FMT_I420 if fmt == "i420" else egress.FMT_BGR24
            cache = {False: None, True: None}
            seq = [(False, 0, -1.0), (True, 1, 0.0), (True, 2, 0.37), (True, 3, 0.999), (True, 0, -1.0), (False, 1, 0.25),
                   (False, 2, 0.5), ("custom", 0, 0.75)]
            for speaking, idx, alpha in seq:
                out = np.empty((H * 3 // 2, W) if fmt == "i420" else (H, W, 3), dtype=np.uint8)
                if speaking == "custom":
                    custom = rng.integers(0, 256, (H, W, 3), dtype=np.uint8)
                    eng.egress_frame(h, out, egress.SRC_HOST, 0, 0, 0, custom, False, alpha, True, fcode, chroma)
                    frame, spk = custom, False
                elif speaking:
                    eng.egress_frame(h, out, egress.SRC_ULTRALIGHT, aid, idx, preds.dev[idx].data_ptr(), None, True, alpha, True, fcode, chroma)
                    frame, spk = comp[idx], True
                else:
                    eng.egress_frame(h, out, egress.SRC_ULTRALIGHT, aid, idx, 0, None, False, alpha, True, fcode, chroma)
                    frame, spk = bank.frames[idx], False
                other = cache[not spk]
                if 0 <= alpha < 1 and other is not None:
                    frame = eo.add_weighted_u8(other, 1 - alpha, frame, alpha)
                cache[spk] = frame.copy()
                ref = eo.egress_frame(frame, (mask, wx, wy, col), fmt, chroma)
                assert np.array_equal(out, ref), (fmt, chroma, speaking, idx, alpha, int((out != ref).sum()))
            eng.egress_close(h)


def test_egress_frame_ultralight_silent_path_and_errors(eng, banks, preds):
    from livetalking_amd import egress
    from livetalking_amd._lib import LtkError
    bank = banks((200, 260))
    H, W = 200, 260
    h = eng.egress_open(H, W)
    out = np.empty((H, W, 3), dtype=np.uint8)
    for idx in range(4):                                             # d_pred = 0: the bank frame itself
        eng.egress_frame(h, out, egress.SRC_ULTRALIGHT, bank.aid, idx, 0, None, False, -1.0, False, egress.FMT_BGR24, 1)
        assert np.array_equal(out, bank.frames[idx])
    with pytest.raises(LtkError) as ex:                              # a bad index
        eng.egress_frame(h, out, egress.SRC_ULTRALIGHT, bank.aid, 4, 0, None, False, -1.0, False, egress.FMT_BGR24, 1)
    assert ex.value.code == -1 and "index" in str(ex.value)
    # a Wav2Lip-registered id as an Ultralight source, and an Ultralight id as a Wav2Lip source
    frames, faces, coords = synth.wav2lip_avatar(n_frames=2, full_hw=(H, W), box=96, seed=3)
    wid = eng.register_avatar(faces, frames, coords)
    try:
        with pytest.raises(LtkError) as ex:
            eng.egress_frame(h, out, egress.SRC_ULTRALIGHT, wid, 0, preds.dev[0].data_ptr(), None, True, -1.0, False, egress.FMT_BGR24, 1)
        assert ex.value.code == -3
        with pytest.raises(LtkError) as ex:
            eng.egress_frame(h, out, egress.SRC_WAV2LIP, bank.aid, 0, 0, None, False, -1.0, False, egress.FMT_BGR24, 1)
        assert ex.value.code == -3
        host = np.empty((1, H, W, 3), np.uint8)
        with pytest.raises(LtkError):
            eng.egress_batch(h, egress.SRC_ULTRALIGHT, wid, [0], preds.dev.data_ptr(), host.ctypes.data, egress.FMT_BGR24, 1)
    finally:
        eng.release_avatar(wid)
    eng.egress_close(h)
    # a session of another frame size
    h2 = eng.egress_open(H + 2, W)
    big = np.empty((H + 2, W, 3), np.uint8)
    with pytest.raises(LtkError) as ex:
        eng.egress_frame(h2, big, egress.SRC_ULTRALIGHT, bank.aid, 0, 0, None, False, -1.0, False, egress.FMT_BGR24, 1)
    assert ex.value.code == -1 and "size" in str(ex.value)
    with pytest.raises(LtkError) as ex:
        eng.egress_batch(h2, egress.SRC_ULTRALIGHT, bank.aid, [0], preds.dev.data_ptr(), big.ctypes.data, egress.FMT_BGR24, 1)
    assert ex.value.code == -1 and "size" in str(ex.value)
    eng.egress_close(h2)
    # the engine still serves the source afterwards
    h3 = eng.egress_open(H, W)
    eng.egress_frame(h3, out, egress.SRC_ULTRALIGHT, bank.aid, 1, preds.dev[1].data_ptr(), None, True, -1.0, False, egress.FMT_BGR24, 1)
    assert np.array_equal(out, _composite(bank, 1, preds.host[1]))
    eng.egress_close(h3)


# ------------------------------------------------------------------ ltk_egress_batch
@pytest.mark.parametrize("fmt", ["bgr24", "i420"])
def test_egress_batch_ultralight_equals_per_frame_and_oracle(eng, banks, preds, fmt):
    import torch
    from livetalking_amd import egress
    H, W = 200, 260
    bank = banks((H, W))
    n, idx = N17, IDX17
    want = _want17(bank, preds)
    mask, wx, wy, col = _wm(2)
    fcode = egress.FMT_I420 if fmt == "i420" else egress.FMT_BGR24
    h = eng.egress_open(H, W)
    eng.egress_watermark(h, mask, wx, wy, col)
    shape = (n, H * 3 // 2, W) if fmt == "i420" else (n, H, W, 3)
    host = torch.zeros(shape, dtype=torch.uint8, pin_memory=True)
    eng.egress_batch(h, egress.SRC_ULTRALIGHT, bank.aid, idx, preds.dev.data_ptr(), host.data_ptr(), fcode, 1)
    got = host.numpy()
    for i in range(n):
        one = np.empty(shape[1:], dtype=np.uint8)
        eng.egress_frame(h, one, egress.SRC_ULTRALIGHT, bank.aid, idx[i], preds.dev[i].data_ptr(), None, True, -1.0, False, fcode, 1)
        ref = eo.egress_frame(want[i], (mask, wx, wy, col), fmt, 1)
        assert np.array_equal(got[i], ref), (fmt, i, int((got[i] != ref).sum()))
        assert np.array_equal(got[i], one), (fmt, i)
    eng.egress_close(h)
    # the plugin-side path: items of a batch carrying their FrameGroup
    eg = egress.DeviceEgress(eng, H, W, egress.SRC_ULTRALIGHT, bank.aid, fmt=fmt, watermark=(mask, wx, wy))
    try:
        items = [preds.dev[i] for i in range(n)]
        egress.FrameGroup.attach(items, preds.dev, idx)
        outs = [eg.speaking_frame_of(items[i], idx[i]) for i in range(n)]
        keep = outs[1].copy()
        more = [preds.dev[i] for i in range(n)]
        egress.FrameGroup.attach(more, preds.dev, idx)
        [eg.speaking_frame_of(more[i], idx[i]) for i in range(n)]
        for i in range(n):
            assert np.array_equal(np.asarray(outs[i]), got[i]), i
            if fmt == "i420":
                assert isinstance(outs[i], egress.I420Frame) and (outs[i].height, outs[i].width) == (H, W)
        assert np.array_equal(np.asarray(outs[1]), keep)              # a kept frame stays valid after the next batch
    finally:
        eg.close()


# ------------------------------------------------------------------ LightReal end to end
class _Proc:
    def get_hubert_from_16k_speech(self, pcm):
        return np.zeros(((len(pcm) - 80) // 320, 1024), np.float32)


class _Sink:
    def __init__(self):
        self.video, self.audio, self.started, self.stopped = [], [], False, False

    def start(self):
        self.started = True

    def push_video_frame(self, f):
        self.video.append(f)

    def push_audio_frame(self, pcm, userdata=None):
        self.audio.append(pcm)

    def stop(self):
        self.stopped = True


def _mirror(size, index):
    turn, res = divmod(index, size)
    return res if turn % 2 == 0 else size - res - 1


@pytest.fixture(scope="module")
def light_avatar(eng, sd):
    """An UltralightNet of its own (the plugin registers it) over a four-frame bank with the four boxes."""
    from livetalking_amd.avatars import ultralight_avatar as ul
    H, W = 200, 260
    frames, faces, _ = synth.ultralight_avatar(4, (H, W), seed=21)
    boxes = _boxes(H, W)
    net = ul.UltralightNet(sd, faces, frames, boxes, engine=eng, max_frames=4)
    yield types.SimpleNamespace(H=H, W=W, frames=frames, faces=faces, boxes=boxes, avatar=(net, frames, faces, boxes))
    net.release()


def test_lightreal_device_process_frames_loop(eng, light_avatar):
    """opt.egress = "i420": LightReal's process_frames is the mixin's; a silent item gives the bank frame, the B items of a real
    inference_batch the composites of the engine's own predictions, all as I420."""
    import torch
    from livetalking_amd import egress
    from livetalking_amd.avatars import ultralight_avatar as ul
    from livetalking_amd.hostshim import AudioFrameData
    la = light_avatar
    H, W, B = la.H, la.W, 4
    opt = types.SimpleNamespace(fps=25, batch_size=B, l=10, r=10, sessionid=2, egress="i420", enable_transition=False)
    sess = ul.LightReal(opt, (_Proc(), None), la.avatar)
    sess.output = _Sink()
    items = sess.inference_batch(1, list(synth.ultralight_feats(B, 40)))      # bank frames 1, 2, 3, 3
    order = [_mirror(4, 1 + i) for i in range(B)]
    assert order == [1, 2, 3, 3]
    pred = torch.stack(items).cpu().numpy()
    assert pred.any()
    quit_event = threading.Event()
    th = threading.Thread(target=sess.process_frames, args=(quit_event,))
    th.start()
    pcm = np.zeros(320, np.float32)
    speak = [AudioFrameData(pcm, 0, {}), AudioFrameData(pcm, 0, {})]
    quiet = [AudioFrameData(pcm, 1, {}), AudioFrameData(pcm, 1, {})]
    sess.res_frame_queue.put((None, quiet, 2))
    for i in range(B):
        sess.res_frame_queue.put((items[i], speak, order[i]))
    t0 = time.time()
    while len(sess.output.video) < B + 1 and time.time() - t0 < 30:
        time.sleep(0.01)
    quit_event.set()
    th.join(timeout=10)
    assert not th.is_alive() and sess.output.started and sess.output.stopped
    assert len(sess.output.video) == B + 1 and len(sess.output.audio) == 2 * (B + 1)
    m = egress.watermark_mask(H, W)                                     # None without OpenCV: then no watermark is drawn
    wm = None if m is None else (m[0], m[1], m[2], egress.WATERMARK_COLOR)
    bank = types.SimpleNamespace(frames=la.frames, faces=la.faces, boxes=la.boxes)
    assert np.array_equal(np.asarray(sess.output.video[0]), eo.egress_frame(la.frames[2], wm, "i420", 1))
    for i in range(B):
        got = sess.output.video[1 + i]
        assert isinstance(got, egress.I420Frame) and (got.width, got.height) == (W, H)
        assert np.array_equal(np.asarray(got), eo.egress_frame(_composite(bank, order[i], pred[i]), wm, "i420", 1)), i


def test_lightreal_paste_back_frame_serves_a_batch_from_one_block(eng, light_avatar, monkeypatch):
    """Without opt.egress: the items of one inference_batch come back as views of one pinned block, equal to ultralight_paste_back
    per frame; an item asked for with another idx than its group's takes the per-frame path and is still right."""
    import torch
    from livetalking_amd.avatars import ultralight_avatar as ul
    monkeypatch.setattr(ul, "_PASTE_BATCH", True)                      # whatever LTK_PASTE_BATCH says in this environment
    la = light_avatar
    H, W, B = la.H, la.W, 4
    opt = types.SimpleNamespace(fps=25, batch_size=B, l=10, r=10, sessionid=3)
    sess = ul.LightReal(opt, (_Proc(), None), la.avatar)
    assert sess.engine is eng
    items = sess.inference_batch(2, list(synth.ultralight_feats(B, 41)))      # bank frames 2, 3, 3, 2
    order = [_mirror(4, 2 + i) for i in range(B)]
    d_pred = torch.stack(items)
    out = [sess.paste_back_frame(items[i], order[i]) for i in range(B)]
    for i in range(B):
        want = np.empty((H, W, 3), np.uint8)
        eng.ultralight_paste_back(sess._aid, order[i], d_pred[i].data_ptr(), want)
        assert out[i].flags.c_contiguous and out[i].flags.writeable and np.array_equal(out[i], want), i
        assert out[i].base is out[0].base and out[i].base is not None
        assert not np.array_equal(out[i], la.frames[order[i]])
    block = items[0]._ltk_group.host
    assert block.shape == (B, H, W, 3) and all(np.shares_memory(o, block) for o in out)
    odd = sess.paste_back_frame(items[0], 0)                           # the group says bank frame 2
    want = np.empty((H, W, 3), np.uint8)
    eng.ultralight_paste_back(sess._aid, 0, d_pred[0].data_ptr(), want)
    assert np.array_equal(odd, want) and not np.shares_memory(odd, block) and odd.flags.writeable
