"""Drop-in for avatars/audio_features/hubert.py (HubertASR), the audio front end of the Ultralight avatar.

Same class name, constructor `(opt, parent, audio_processor, audio_feat_length)`, queue protocol and step cadence as the
reference (hubert.py:13-49): every `run_step` pulls 2*batch_size 20-ms chunks, forwards them to `output_queue`, and - once
l+r chunks of context exist - puts ONE list of batch_size feature chunks on `feat_queue` and keeps the last l+r chunks.
With `audio_feat_length=[4, 4]` (ultralight_avatar.py:140), start = l/2 and multiplier 2, frame i takes HuBERT rows
[2*(i + l/2) - 8, 2*(i + l/2) + 8), index-clamped (base_asr.py:91-133): 16 rows of 1024 per frame.

`audio_processor` is any object with `get_hubert_from_16k_speech(pcm) -> (T, 1024)`: `load_model()` below (transformers'
HubertModel on torch, the default), a test stand-in, or `EngineAudio2Feature`: HuBERT-large as a device program of the engine
(csrc/hubert.hip), opt-in through ultralight_avatar.load_model.  A processor that also has `step(pcm, batch, first_row,
row_step, rows)` (EngineAudio2Feature does) hands back the chunks as ONE device tensor [batch][rows][1024]; run_step then puts
batch_size views of it on feat_queue and the features never visit the host (Engine.ultralight_infer takes them as float32
[batch][16][32][32]).

One deliberate difference: the reference's silent default is `batch_size * [zeros((10, 1024))]` (hubert.py:38), which
LightReal.inference_batch cannot reshape to (16, 32, 32); the silent chunks here are zeros((16, 1024)).
"""
from __future__ import annotations

import os

import numpy as np

from ...hostshim import BaseASR

HUBERT_DIR = "./models/hubert-large-ls960-ft"      # avatars/ultralight/audio2feature.py:9-10
# 1: the live steps of concurrent sessions go through the engine's "hubert" scheduler and share one forward per tick
# (Engine.hubert_step_batch); 0: every step is its own hubert_step call.  Read once.
_HUBERT_BATCH_DEFAULT = "1"
_HUBERT_BATCH = os.environ.get("LTK_HUBERT_BATCH", _HUBERT_BATCH_DEFAULT) != "0"


class Audio2Feature:
    """avatars/ultralight/audio2feature.py:6-53: transformers' HuBERT-large on torch (ROCm build: device "cuda")."""

    def __init__(self, model_dir: str = HUBERT_DIR):
        import torch
        from transformers import HubertModel, Wav2Vec2Processor
        self._torch = torch
        self.device = "cuda" if torch.cuda.is_available() else "cpu"
        self.processor = Wav2Vec2Processor.from_pretrained(model_dir)
        self.model = HubertModel.from_pretrained(model_dir).to(self.device)
        self.model.requires_grad_(False)

    def get_hubert_from_16k_speech(self, speech):
        torch = self._torch
        if speech.ndim == 2:
            speech = speech[:, 0]
        with torch.no_grad():
            x = self.processor(speech, return_tensors="pt", sampling_rate=16000).input_values.to(self.device)
            kernel, stride = 400, 320
            clip = stride * 1000
            expected = (x.shape[1] - (kernel - stride)) // stride
            parts = []
            n_iter = x.shape[1] // clip
            for i in range(n_iter):
                parts.append(self.model(x[:, clip * i: clip * i + clip - stride + kernel]).last_hidden_state[0])
            tail = x[:, clip * n_iter:]
            if tail.shape[1] >= kernel:
                parts.append(self.model(tail).last_hidden_state[0])
            ret = torch.cat(parts, dim=0).cpu()
            if abs(ret.shape[0] - expected) > 1:
                raise RuntimeError(f"HuBERT returned {ret.shape[0]} rows for {expected} expected")
            if ret.shape[0] < expected:
                ret = torch.nn.functional.pad(ret, (0, 0, 0, expected - ret.shape[0]))
            return ret[:expected]


class EngineAudio2Feature:
    """Audio2Feature on the engine: `source` is the checkpoint directory (HubertModel.from_pretrained; only the weights are read,
    the Wav2Vec2Processor's one job - zero mean, unit variance over the utterance - is part of the device program) or a
    HubertModel state dict."""

    def __init__(self, engine, source=HUBERT_DIR, opt=None):
        if isinstance(source, (str, os.PathLike)):
            from transformers import HubertModel
            source = HubertModel.from_pretrained(source).state_dict()
        self.engine = engine
        engine.load_hubert(source)
        from ...health import monitor_for
        self.health_monitor = monitor_for(engine, "hubert", opt)  # LTK_HEALTH_WATCH=N / opt.health_watch: the model's first N calls are watched

    def health(self):
        """(ops, calls_seen, calls_left) of the headroom watch over the model's first calls; None when no watch was armed."""
        h = getattr(self, "health_monitor", None)
        return h.report() if h is not None else None

    def _health_tick(self):
        h = getattr(self, "health_monitor", None)
        if h is not None and h.pending:             # the first call behind the watched window logs its line
            h.tick()

    def get_hubert_from_16k_speech(self, speech):
        speech = np.asarray(speech)
        if speech.ndim == 2:
            speech = speech[:, 0]
        self._health_tick()
        return self.engine.hubert_features(speech)

    def step(self, pcm, batch, first_row, row_step=2, rows=16):
        """One forward of the step's pcm -> device float32 (batch, rows, 1024): frame i = rows [first_row + i * row_step, + rows),
        index-clamped.  Steps of concurrent sessions on this engine share a forward (scheduler kind "hubert"); a lone session's
        call goes straight down in its own thread."""
        import torch
        out = torch.empty((batch, rows, 1024), dtype=torch.float32, device=self.engine.torch_device)
        self._health_tick()
        if _HUBERT_BATCH:
            from ...scheduler import get_scheduler
            get_scheduler(self.engine, "hubert").submit((pcm, batch, first_row, row_step, rows, out.data_ptr()), 1)
        else:
            self.engine.hubert_step(pcm, batch, first_row, out.data_ptr(), row_step=row_step, rows=rows)
        return out

    def zeros(self, batch, rows):
        import torch
        return torch.zeros((batch, rows, 1024), dtype=torch.float32, device=self.engine.torch_device)


def check_model_dir(model_dir: str = HUBERT_DIR) -> None:
    if not os.path.isdir(model_dir):
        raise FileNotFoundError(
            f"{model_dir} is missing: the Ultralight avatar needs the HuBERT-large checkpoint the reference uses "
            "(facebook/hubert-large-ls960-ft) there, or pass your own audio_processor with get_hubert_from_16k_speech()")


def load_model(model_dir: str = HUBERT_DIR) -> Audio2Feature:
    """The audio processor ultralight_avatar.load_model hands to every session (ultralight_avatar.py:58-61)."""
    check_model_dir(model_dir)
    return Audio2Feature(model_dir)


def feature2chunks(feature_array, batch_size, audio_feat_win, start, feature_idx_multiplier):
    """base_asr.py:91-156 (_get_sliced_feature + _feature2chunks): frame i takes rows
    [int((i + start) * m) - win[0] * m, int((i + start) * m) + win[1] * m), every index clamped into the array."""
    feature_array = np.asarray(feature_array)
    length = feature_array.shape[0]
    chunks = []
    for i in range(batch_size):
        center = int((i + start) * feature_idx_multiplier)
        left = int(center - audio_feat_win[0] * feature_idx_multiplier)
        right = int(center + audio_feat_win[1] * feature_idx_multiplier)
        idx = np.clip(np.arange(left, right), 0, length - 1)
        chunks.append(np.ascontiguousarray(feature_array[idx], dtype=np.float32))
    return chunks


class HubertASR(BaseASR):
    def __init__(self, opt, parent, audio_processor, audio_feat_length=[8, 8]):
        super().__init__(opt, parent)
        if not hasattr(audio_processor, "get_hubert_from_16k_speech"):
            raise TypeError("audio_processor must provide get_hubert_from_16k_speech(pcm)")
        self.audio_processor = audio_processor
        if getattr(audio_processor, "health_monitor", True) is None and hasattr(audio_processor, "engine"):
            # an engine-side processor loaded without the knob: opt.health_watch of the first session that brings it arms the watch
            from ...health import monitor_for
            audio_processor.health_monitor = monitor_for(audio_processor.engine, "hubert", opt)
        self.audio_feat_length = audio_feat_length
        self.last_is_silence = True

    def run_step(self):
        is_all_silence = True
        for _ in range(self.batch_size * 2):
            audio_frame = self.get_audio_frame()
            if audio_frame.type == 0:
                is_all_silence = False
            self.frames.append(audio_frame.data)
            self.output_queue.put(audio_frame)
        if len(self.frames) <= self.stride_left_size + self.stride_right_size:
            return
        rows = 2 * (self.audio_feat_length[0] + self.audio_feat_length[1])
        if hasattr(self.audio_processor, "step"):
            # the processor forwards and slices on the device: first_row = int(start * 2) - 2 * win[0] with start = l / 2
            if not is_all_silence or not self.last_is_silence:
                first_row = int(self.stride_left_size / 2 * 2) - 2 * self.audio_feat_length[0]
                dev = self.audio_processor.step(np.concatenate(self.frames), self.batch_size, first_row, 2, rows)
            elif hasattr(self.audio_processor, "zeros"):
                dev = self.audio_processor.zeros(self.batch_size, rows)           # the silent default, on the device as well
            else:
                dev = np.zeros((self.batch_size, rows, 1024), dtype=np.float32)
            self.feat_queue.put([dev[i] for i in range(self.batch_size)])
            self.frames = self.frames[-(self.stride_left_size + self.stride_right_size):]
            self.last_is_silence = is_all_silence
            return
        chunks = [np.zeros((rows, 1024), dtype=np.float32) for _ in range(self.batch_size)]
        if not is_all_silence or not self.last_is_silence:
            inputs = np.concatenate(self.frames)
            feat = self.audio_processor.get_hubert_from_16k_speech(inputs)
            if hasattr(feat, "detach"):
                feat = feat.detach().cpu().numpy()
            chunks = feature2chunks(feat, self.batch_size, self.audio_feat_length, self.stride_left_size / 2, 2)
        self.feat_queue.put(chunks)
        self.frames = self.frames[-(self.stride_left_size + self.stride_right_size):]
        self.last_is_silence = is_all_silence
