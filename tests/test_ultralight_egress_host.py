"""CPU tests of the Ultralight delivery path: the ABI surface of ltk_ultralight_paste_back_batch and LTK_SRC_ULTRALIGHT, argument
refusals that need no device, LightReal's wiring into DeviceEgressMixin, and paste_back_frame's grouping against an engine that
records its calls.

Pinned host memory needs a GPU runtime, so the grouping test patches `torch.empty` to drop `pin_memory=True` (and records that it
was asked for); everything else of the path runs as it is."""
from __future__ import annotations

import ctypes as C
import inspect
import os
import re
import types

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID = -1


# ------------------------------------------------------------------ ABI
def test_header_declares_and_library_exports_the_batch_entry_and_source():
    from livetalking_amd import _lib, egress
    hdr = open(os.path.join(ROOT, "include", "ltk.h")).read()
    name = "ltk_ultralight_paste_back_batch"
    assert re.search(r"\bint\s+" + name + r"\s*\(", hdr), f"{name} is not declared in include/ltk.h"
    assert re.search(r"^#define\s+LTK_SRC_ULTRALIGHT\s+3\b", hdr, re.M)
    assert name in _lib.SYMBOLS
    assert getattr(_lib.load(), name) is not None
    assert _lib.SYMBOLS[name] == _lib.SYMBOLS["ltk_paste_back_batch"]          # the twin: same argument list
    doc = hdr[:hdr.index("int " + name)].rsplit("/*", 1)[1]
    assert "ultralight_avatar.py:" in doc and "base_avatar.py:" in doc
    assert egress.SRC_ULTRALIGHT == 3
    assert (egress.SRC_WAV2LIP, egress.SRC_MUSETALK, egress.SRC_HOST) == (0, 1, 2)


def test_null_and_garbage_arguments_are_invalid_without_a_gpu():
    from livetalking_amd import _lib
    lib = _lib.load()
    fn = lib.ltk_ultralight_paste_back_batch
    buf = (C.c_uint8 * 16)()
    idx = (C.c_int32 * 2)(0, 1)
    assert fn(None, 1, idx, buf, 2, buf, None) == INVALID              # no engine
    assert lib.ltk_last_error()
    fake = C.cast(buf, C.c_void_p)                                       # never dereferenced: the pointer checks come first
    assert fn(fake, 1, None, buf, 2, buf, None) == INVALID
    assert fn(fake, 1, idx, None, 2, buf, None) == INVALID
    assert fn(fake, 1, idx, buf, 2, None, None) == INVALID
    assert fn(fake, 1, idx, buf, 0, buf, None) == INVALID
    assert fn(fake, 1, idx, buf, -3, buf, None) == INVALID
    assert b"bad arguments" in lib.ltk_last_error()
    assert lib.ltk_egress_batch(None, None, 3, 1, idx, buf, 2, 0, 1, buf, None) == INVALID
    assert lib.ltk_last_error()


# ------------------------------------------------------------------ plugin wiring
def test_lightreal_is_wired_into_the_egress_mixin():
    from livetalking_amd import egress, hostshim
    from livetalking_amd.avatars import ultralight_avatar as ul
    mro = ul.LightReal.__mro__
    assert mro.index(egress.DeviceEgressMixin) < mro.index(hostshim.BaseAvatar)
    assert ul.LightReal._egress_source == egress.SRC_ULTRALIGHT
    assert ul.LightReal.process_frames is egress.DeviceEgressMixin.process_frames
    # the reference module's names and parameter lists (tests/test_ultralight_host.py holds this table to the reference's source)
    want = {"load_model": ["opt"], "load_avatar": ["avatar_id"], "warm_up": ["batch_size", "avatar", "modelres"],
            "LightReal.__init__": ["self", "opt", "model", "avatar"], "LightReal.inference_batch": ["self", "index", "audiofeat_batch"],
            "LightReal.paste_back_frame": ["self", "pred_frame", "idx"]}
    for k, v in want.items():
        fn = getattr(ul.LightReal, k.split(".")[1]) if "." in k else getattr(ul, k)
        assert list(inspect.signature(fn).parameters) == v, k
    assert "LightReal" in inspect.getdoc(egress.DeviceEgressMixin)


# ------------------------------------------------------------------ paste_back_frame grouping
class _FakeEngine:
    """Records the paste-back calls; a batch call fills frame i of the host block with 100 + i, a per-frame call its array with
    idx."""
    torch_device = "cpu"

    def __init__(self):
        self.calls = []

    def ultralight_paste_back(self, aid, idx, d_pred_ptr, out, stream=0):
        self.calls.append(("one", aid, idx, d_pred_ptr))
        out[...] = idx

    def ultralight_paste_back_batch(self, aid, idx, d_pred_ptr, out_ptr, stream=0):
        idx = list(idx)
        self.calls.append(("batch", aid, idx, d_pred_ptr, out_ptr))
        H, W = 6, 10
        host = np.ctypeslib.as_array((C.c_uint8 * (len(idx) * H * W * 3)).from_address(out_ptr)).reshape(len(idx), H, W, 3)
        for i in range(len(idx)):
            host[i] = 100 + i

    def ultralight_infer(self, reqs, stream=0):
        self.calls.append(("infer", reqs[0][:3]))


def _session(ul, fe, B, n_bank=3):
    """A LightReal around the fake engine without its constructor (which starts HubertASR and registers a bank)."""
    sess = ul.LightReal.__new__(ul.LightReal)
    sess.engine, sess._aid, sess._frame_hw, sess.batch_size = fe, 9, (6, 10), B
    sess.face_list_cycle = [np.zeros((168, 168, 3), np.uint8)] * n_bank
    sess.frame_list_cycle = [np.zeros((6, 10, 3), np.uint8)] * n_bank
    return sess


@pytest.fixture()
def unpinned(monkeypatch):
    """No pinned allocator without a GPU runtime: torch.empty without pin_memory, and a note of who asked for it."""
    torch = pytest.importorskip("torch")
    asked = []
    real = torch.empty

    def empty(*a, pin_memory=False, **kw):
        asked.append(bool(pin_memory))
        return real(*a, **kw)

    monkeypatch.setattr(torch, "empty", empty)
    return asked


def test_paste_back_frame_groups_one_inference_batch(unpinned, monkeypatch):
    import torch
    from livetalking_amd import hostshim
    from livetalking_amd.avatars import ultralight_avatar as ul
    monkeypatch.setattr(ul, "_PASTE_BATCH", True)
    fe = _FakeEngine()
    B = 4
    sess = _session(ul, fe, B)
    feats = torch.zeros(B, 16, 1024)
    items = sess.inference_batch(2, feats)                              # bank frames 2, 2, 1, 0
    assert fe.calls == [("infer", (9, 2, B))] and len(items) == B
    grp = items[0]._ltk_group
    assert all(it._ltk_group is grp and it._ltk_i == i for i, it in enumerate(items))
    order = [hostshim.mirror_index(3, 2 + i) for i in range(B)]
    assert order == [2, 2, 1, 0] and grp.idx == order
    frames = [sess.paste_back_frame(items[i], order[i]) for i in range(B)]
    batch = [c for c in fe.calls if c[0] == "batch"]
    assert len(batch) == 1 and not [c for c in fe.calls if c[0] == "one"]
    assert batch[0][1:4] == (9, order, grp.pred.data_ptr())
    assert True in unpinned                                             # the block was asked for as pinned memory
    base = frames[0].base
    for i, f in enumerate(frames):
        assert f.shape == (6, 10, 3) and f.dtype == np.uint8 and f.flags.c_contiguous and f.flags.writeable
        assert f.base is base and (f == 100 + i).all()
    # a request whose idx is not the group's: the per-frame path, the group untouched
    odd = sess.paste_back_frame(items[1], 0)
    assert fe.calls[-1][:3] == ("one", 9, 0) and (odd == 0).all() and odd.base is None
    assert len([c for c in fe.calls if c[0] == "batch"]) == 1
    # a foreign float frame (numpy, no group): per-frame, converted to uint8 on the way
    n_before = len(fe.calls)
    foreign = sess.paste_back_frame(np.full((160, 160, 3), 7.9, np.float32), 1)
    assert len(fe.calls) == n_before + 1 and fe.calls[-1][:3] == ("one", 9, 1) and (foreign == 1).all()


def test_paste_batch_knob_off_gives_per_frame_calls(unpinned, monkeypatch):
    """LTK_PASTE_BATCH=0 (read once at import into _PASTE_BATCH, as in wav2lip_avatar): no group is attached, every frame takes
    ultralight_paste_back."""
    import torch
    from livetalking_amd.avatars import ultralight_avatar as ul
    from livetalking_amd.avatars import wav2lip_avatar as w2l
    assert ul._PASTE_BATCH == w2l._PASTE_BATCH == (os.environ.get("LTK_PASTE_BATCH", "1") != "0")
    monkeypatch.setattr(ul, "_PASTE_BATCH", False)
    fe = _FakeEngine()
    B = 3
    sess = _session(ul, fe, B)
    items = sess.inference_batch(0, torch.zeros(B, 16, 1024))
    assert not any(hasattr(it, "_ltk_group") for it in items)
    for i in range(B):
        f = sess.paste_back_frame(items[i], i)
        assert (f == i).all() and f.flags.writeable and f.flags.c_contiguous
    assert [c[0] for c in fe.calls] == ["infer", "one", "one", "one"] and True not in unpinned


def test_make_egress_finds_engine_and_avatar_id_on_lightreal():
    from livetalking_amd import egress
    from livetalking_amd.avatars import ultralight_avatar as ul
    opened = []

    class _Eg:
        def egress_open(self, H, W):
            opened.append((H, W))
            return 5

        def egress_watermark(self, *a):
            opened.append("wm")

    sess = _session(ul, _Eg(), 2)
    sess.opt = types.SimpleNamespace(egress="i420", enable_transition=False)
    eg = sess._make_egress()
    assert opened[0] == (6, 10) and eg.engine is sess.engine
    assert (eg.source, eg.avatar_id, eg.fmt) == (egress.SRC_ULTRALIGHT, 9, egress.FMT_I420)
