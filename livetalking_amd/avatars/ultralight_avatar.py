"""HIP-backed drop-in for avatars/ultralight_avatar.py.

Module contract the reference's app.py relies on (the plugin is picked by name):
  load_model(opt) -> (audio_processor, model)            (ultralight_avatar.py:58-61)
  load_avatar(avatar_id) -> avatar tuple                 (ultralight_avatar.py:63-81)
  warm_up(batch_size, avatar, modelres)                  (ultralight_avatar.py:84-90)
  @register("avatar", "ultralight") class LightReal(DeviceEgressMixin, BaseAvatar) with
  inference_batch(index, audiofeat_batch) and paste_back_frame(pred_frame, idx)   (ultralight_avatar.py:125-184)

What changes underneath: the U-Net is per avatar (`ultralight.pth`), so `load_avatar` returns an `UltralightNet` handle in the
model's place; it registers state_dict + bank with the engine (libltk_hip.so) on first use.  `inference_batch` returns device
handles (uint8 160x160x3, already truncated the way paste_back_frame's astype(uint8) does) instead of float numpy frames;
`paste_back_frame` composites on the GPU and returns a writable C-contiguous uint8 (H,W,3) BGR array; the B items of one
`inference_batch` result are composited and copied to the host together (LTK_PASTE_BATCH=0: one by one).  `inference_batch` goes
through the engine's "ultralight" scheduler, so that concurrent sessions' passes merge into one launch sequence
(Engine.ultralight_infer_merged; LTK_UL_SCHED=0: one ultralight_infer call per session).  With
`opt.egress` = "bgr24" | "i420" the frames leave through the device-side process_frames of egress.py.  HuBERT-large runs on
torch by default (audio_features/hubert.py Audio2Feature); with LTK_HUBERT_ENGINE=1 or opt.hubert_engine it runs on the engine
(EngineAudio2Feature) and its chunks reach inference_batch as device tensors.
"""
from __future__ import annotations

import glob
import os
import pickle
import threading

import numpy as np

from ..egress import SRC_ULTRALIGHT, DeviceEgressMixin, FrameGroup
from ..engine import Engine
from ..health import monitor_for
from ..hostshim import BaseAvatar, mirror_index, register  # noqa: F401  (mirror_index: part of the reference module's namespace)
from ..scheduler import get_scheduler
from .audio_features.hubert import HubertASR
from .audio_features import hubert as _hubert

_PASTE_BATCH = os.environ.get("LTK_PASTE_BATCH", "1") != "0"     # 0: one composite + one pageable copy per paste_back_frame call
_UL_SCHED_DEFAULT = "1"
_UL_SCHED = os.environ.get("LTK_UL_SCHED", _UL_SCHED_DEFAULT) != "0"    # 0: inference_batch calls ultralight_infer itself, no scheduler

_engines = {}
_engines_lock = threading.Lock()
_hubert_lock = threading.Lock()    # held across "look up, else build": two sessions' load_model calls must not both load the engine
_hubert_processors = {}            # engine -> its EngineAudio2Feature: an engine holds one HuBERT model, load_model may be called again


def _engine(device: int = 0) -> Engine:
    """One engine per GPU and process, shared by every Ultralight avatar and session."""
    with _engines_lock:
        eng = _engines.get(device)
        if eng is None or eng._h is None:
            eng = _engines[device] = Engine(device)
        return eng


class UltralightNet:
    """Stands where the reference's `Model(6, 'hubert')` stands in the avatar tuple: the state_dict plus, once a session
    or warm_up needs it, the engine-side avatar (weights folded and packed, bank in HBM)."""

    def __init__(self, state_dict, face_list, frame_list, coord_list, engine=None, max_frames=None):
        self.state_dict = state_dict
        self._bank = (face_list, frame_list, coord_list)
        self.engine = engine
        self.max_frames = int(max_frames or os.environ.get("LTK_UL_MAX_FRAMES", "32"))
        self._aid = None
        self._lock = threading.Lock()
        self.health_monitor = None       # LTK_HEALTH_WATCH=N: the avatar's first N calls are watched from its registration on

    def avatar_id(self, opt=None) -> int:
        """Registers the avatar on first use.  `opt`: a session's options - opt.health_watch arms the avatar's watch when
        LTK_HEALTH_WATCH did not at the registration."""
        with self._lock:
            if self._aid is None:
                if self.engine is None:
                    self.engine = _engine(0)
                faces, frames, coords = self._bank
                self._aid = self.engine.register_ultralight_avatar(self.state_dict, faces, frames, coords, max_frames=self.max_frames)
            if self.health_monitor is None:
                self.health_monitor = monitor_for(self.engine, "ultralight", opt, self._aid)
            return self._aid

    def health(self):
        """(ops, calls_seen, calls_left) of the headroom watch over this avatar's first calls (livetalking_amd/health.py); None when
        no watch was armed."""
        h = getattr(self, "health_monitor", None)
        return h.report() if h is not None else None

    def release(self):
        with self._lock:
            if self._aid is not None:
                self.engine.release_avatar(self._aid)
                self._aid = None
                self.health_monitor = None          # the table went with the avatar

    def eval(self):
        return self


def load_model(opt):
    """ultralight_avatar.py:58-61: (audio_processor, None) - the U-Net comes with the avatar."""
    _hubert.check_model_dir(_hubert.HUBERT_DIR)
    if os.environ.get("LTK_HUBERT_ENGINE", "0") == "1" or getattr(opt, "hubert_engine", False):
        eng = _engine(0)
        with _hubert_lock:
            audio_processor = _hubert_processors.get(eng)
            if audio_processor is None:
                for dead in [e for e in _hubert_processors if e._h is None]:
                    del _hubert_processors[dead]
                audio_processor = _hubert_processors[eng] = _hubert.EngineAudio2Feature(eng, _hubert.HUBERT_DIR, opt=opt)
    else:
        audio_processor = _hubert.load_model()
    model = None
    return audio_processor, model


def read_imgs(img_list):
    import cv2  # same third-party reader the reference uses (utils/image.py:14-24)
    return [cv2.imread(p) for p in img_list]


def load_avatar(avatar_id):
    import torch
    avatar_path = f"./data/avatars/{avatar_id}"
    sd = torch.load(f"{avatar_path}/ultralight.pth", map_location="cpu")
    with open(f"{avatar_path}/coords.pkl", "rb") as f:
        coord_list_cycle = pickle.load(f)

    def numbered(d):
        files = glob.glob(os.path.join(d, "*.[jpJP][pnPN]*[gG]"))
        return sorted(files, key=lambda x: int(os.path.splitext(os.path.basename(x))[0]))

    frame_list_cycle = read_imgs(numbered(f"{avatar_path}/full_imgs"))
    face_list_cycle = read_imgs(numbered(f"{avatar_path}/face_imgs"))
    model = UltralightNet(sd, face_list_cycle, frame_list_cycle, coord_list_cycle)
    return model.eval(), frame_list_cycle, face_list_cycle, coord_list_cycle


def warm_up(batch_size, avatar, modelres):
    """One forward on ones, as the reference does, to fault in kernels and arena."""
    model, _, _, _ = avatar
    aid = model.avatar_id()
    n = min(batch_size, model.max_frames)
    img = np.ones((n, 6, modelres, modelres), dtype=np.float32)
    feat = np.ones((n, 16, 32, 32), dtype=np.float32)
    model.engine.ultralight_forward_host(aid, img, feat)


@register("avatar", "ultralight")
class LightReal(DeviceEgressMixin, BaseAvatar):
    _egress_source = SRC_ULTRALIGHT   # opt.egress = "bgr24" | "i420": device-side process_frames (egress.py)
    _health = None                    # the avatar's headroom monitor while LTK_HEALTH_WATCH asks for one (health.py)

    def __init__(self, opt, model, avatar):
        super().__init__(opt)
        audio_processor, _ = model
        self.model, self.frame_list_cycle, self.face_list_cycle, self.coord_list_cycle = avatar
        self._aid = self.model.avatar_id(opt)
        self.engine = self.model.engine
        self._health = getattr(self.model, "health_monitor", None)
        h, w = self.frame_list_cycle[0].shape[:2]
        self._frame_hw = (int(h), int(w))
        self.asr = HubertASR(opt, self, audio_processor, audio_feat_length=[4, 4])
        self.asr.warm_up()

    def _feat_to_device(self, audiofeat_batch):
        import torch
        if isinstance(audiofeat_batch, torch.Tensor):
            return audiofeat_batch.to(self.engine.torch_device, torch.float32).reshape(-1, 16, 32, 32).contiguous()
        if len(audiofeat_batch) and isinstance(audiofeat_batch[0], torch.Tensor):     # HubertASR over a processor with step(): device views
            return torch.stack([a.to(self.engine.torch_device, torch.float32).reshape(16, 32, 32) for a in audiofeat_batch]).contiguous()
        arr = np.ascontiguousarray(np.stack([np.asarray(a, dtype=np.float32).reshape(16, 32, 32) for a in audiofeat_batch]))
        return torch.from_numpy(arr).to(self.engine.torch_device)

    def inference_batch(self, index, audiofeat_batch):
        """Returns batch_size device handles (uint8 [160][160][3] BGR), item i for bank index mirror_index(len, index+i)."""
        import torch
        feat = self._feat_to_device(audiofeat_batch)
        B = self.batch_size
        if feat.shape[0] != B:
            raise ValueError(f"expected {B} feature chunks, got {feat.shape[0]}")
        pred = torch.empty((B, 160, 160, 3), dtype=torch.uint8, device=feat.device)
        h = self._health
        if h is not None and h.pending:             # the first call behind the watched window logs its line
            h.tick()
        if _UL_SCHED and hasattr(self.engine, "ultralight_infer_merged"):
            # concurrent sessions' passes merge into one launch sequence (scheduler kind "ultralight"); a lone session takes the
            # scheduler's solo path: one request, the launches and bytes of the direct call
            get_scheduler(self.engine, "ultralight").infer(self._aid, int(index), B, feat.data_ptr(), pred.data_ptr())
        else:
            self.engine.ultralight_infer([(self._aid, int(index), B, feat.data_ptr(), pred.data_ptr())])
        items = list(pred.unbind(0))
        if _PASTE_BATCH and hasattr(self.engine, "ultralight_paste_back_batch"):
            # the process thread will ask for these B composites one by one, in order (base_avatar.py:429-433): remember
            # the batch so that the FIRST request composites all of them and moves them to the host in one copy
            FrameGroup.attach(items, pred, span=(len(self.face_list_cycle), int(index), B))
        return items

    def paste_back_frame(self, pred_frame, idx: int):
        import torch
        if not isinstance(pred_frame, torch.Tensor):   # a float frame from a foreign inference_batch
            pred_frame = torch.from_numpy(np.ascontiguousarray(pred_frame).astype(np.uint8)).to(self.engine.torch_device)
        h, w = self._frame_hw
        grp = getattr(pred_frame, "_ltk_group", None)
        if grp is not None and grp.idx[pred_frame._ltk_i] == int(idx):
            with grp.lock:
                if grp.host is None:
                    # one pinned host block per batch, as LipReal.paste_back_frame: n composites on the GPU, ONE device-to-host
                    # copy; the returned frames are views of the block, which lives as long as any of them does
                    host = torch.empty((len(grp.idx), h, w, 3), dtype=torch.uint8, pin_memory=True)
                    self.engine.ultralight_paste_back_batch(self._aid, grp.idx, grp.pred.data_ptr(), host.data_ptr())
                    grp.host = host.numpy()
            return grp.host[pred_frame._ltk_i]
        out = np.empty((h, w, 3), dtype=np.uint8)
        self.engine.ultralight_paste_back(self._aid, int(idx), pred_frame.contiguous().data_ptr(), out)
        return out
