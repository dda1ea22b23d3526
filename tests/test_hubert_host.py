"""CPU tests of the HuBERT-large path: the C ABI's declarations and argument checks, the weight-norm fold, the float64
restatement (tests/hubert_ref.py) against transformers' HubertModel and against the reference's own clip loop, and HubertASR over
a processor that slices on the device."""
from __future__ import annotations

import ctypes as C
import importlib.util
import os
import re
import types

import numpy as np
import pytest
import torch

import hubert_ref as H

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REFERENCE = os.environ.get("LTK_REFERENCE", "/root/reference")
HAVE_REFERENCE = os.path.isfile(os.path.join(REFERENCE, "avatars", "ultralight", "audio2feature.py"))
ABI = ["ltk_hubert_load", "ltk_hubert_features", "ltk_hubert_step", "ltk_hubert_debug_get", "ltk_hubert_op_count", "ltk_hubert_op_name"]


def _gen():
    spec = importlib.util.spec_from_file_location("gen_golden_hubert", os.path.join(ROOT, "scripts", "gen_golden_hubert.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _rel(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.linalg.norm(a - b) / np.linalg.norm(b))


@pytest.fixture(scope="module")
def sd2():
    return H.state_dict(2, 20)


@pytest.fixture(scope="module")
def hf_model(sd2):
    from transformers import HubertModel
    m = HubertModel(H.config(2)).double().eval()
    m.load_state_dict({k: torch.as_tensor(v).double() for k, v in sd2.items()}, strict=True)
    return m


# ------------------------------------------------------------------ ABI
def test_abi_is_declared_and_exported():
    from livetalking_amd import _lib
    header = open(os.path.join(ROOT, "include", "ltk.h")).read()
    lib = _lib.load()
    for name in ABI:
        assert re.search(r"\bint\s+" + name + r"\s*\(", header), name + " is not declared in include/ltk.h"
        assert name in _lib.SYMBOLS and hasattr(lib, name), name


def test_argument_checks_need_no_gpu():
    """Null handles, null buffers and sizes out of range are refused before anything touches a device."""
    from livetalking_amd import _lib
    lib = _lib.load()
    buf = (C.c_float * 2048)()
    rows = C.c_int()
    assert lib.ltk_hubert_load(None, None, 0) == -1
    assert lib.ltk_hubert_features(None, buf, 400, buf, 1, C.byref(rows)) == -1
    assert lib.ltk_hubert_step(None, buf, 16640, 16, 2, 2, 16, buf) == -1
    assert lib.ltk_hubert_debug_get(None, b"encoder.layer_norm", buf, 1) == -1
    assert lib.ltk_hubert_op_count(None) == 0
    assert lib.ltk_hubert_op_name(None, 0, None, 0, None) == -1
    assert b"bad arguments" in lib.ltk_last_error()


# ------------------------------------------------------------------ weight norm
def test_weight_norm_fold_equals_torch_in_both_spellings(sd2):
    from torch.nn.utils.parametrizations import weight_norm
    from livetalking_amd.engine import Engine
    conv = weight_norm(torch.nn.Conv1d(H.D, H.D, H.POS_K, padding=H.POS_K // 2, groups=H.POS_GROUPS), name="weight", dim=2)
    with torch.no_grad():
        conv.parametrizations.weight.original0.copy_(torch.from_numpy(sd2[H.G_KEY]))
        conv.parametrizations.weight.original1.copy_(torch.from_numpy(sd2[H.V_KEY]))
        want = conv.weight.detach().numpy()
    for spelled in (sd2, H.weight_g_v_spelling(sd2)):
        out = Engine.fold_hubert_weight_norm(spelled)
        got = out[H.W_KEY]
        assert got.shape == (1024, 64, 128) and got.dtype == np.float32
        assert np.abs(got - want).max() <= 1e-6 * np.abs(want).max()
        assert not any("parametrizations" in k or k.endswith(("weight_g", "weight_v")) or k == "masked_spec_embed" for k in out)
    assert np.abs(H.fold_weight_norm(sd2)[H.W_KEY].numpy() - want).max() <= 1e-6 * np.abs(want).max()
    with pytest.raises(KeyError):
        Engine.fold_hubert_weight_norm({k: v for k, v in sd2.items() if k != H.G_KEY})


# ------------------------------------------------------------------ the restatement
@pytest.mark.parametrize("n", [1040, 16640])
def test_forward_equals_hubert_model_in_float64(sd2, hf_model, n):
    """Both sides are float64: rel L2 <= 1e-9."""
    x = H.normalise(H.speech(n, 3))
    with torch.no_grad():
        want = hf_model(torch.from_numpy(x)[None]).last_hidden_state[0].numpy()
    taps = {}
    got = H.forward(sd2, x, taps=taps).numpy()
    assert got.shape == want.shape == (H.rows(n), 1024)
    rel = _rel(got, want)
    print(f"n {n}: rel L2 {rel:.2e}")
    assert rel <= 1e-9
    assert list(taps) == [nm + ".attn" if nm.endswith(".attention") else nm for nm in H.op_names(2)]
    assert H.forward(H.weight_g_v_spelling(sd2), x).equal(torch.from_numpy(got))


def test_fp16_model_is_close_but_not_equal(sd2):
    x = H.normalise(H.speech(1040, 3))
    rel = _rel(H.forward(sd2, x, fp16_model=True).numpy(), H.forward(sd2, x).numpy())
    assert 1e-5 < rel < 1e-2, rel


def test_clip_ranges():
    assert H.clip_ranges(16640) == [(0, 16640)]
    assert H.clip_ranges(330000) == [(0, 320080), (320000, 330000)]
    assert H.clip_ranges(320000) == [(0, 320000)]                       # the slice is clamped; no tail
    assert H.clip_ranges(640300) == [(0, 320080), (320000, 640080)]                             # a tail under 400 samples is skipped
    assert [H.rows(b - a) for a, b in H.clip_ranges(330000)] == [1000, 31]


def test_clip_loop_is_the_reference_method(sd2, golden_dir):
    """hubert_ref.features against what the reference's get_hubert_from_16k_speech returned (tests/golden/hubert_golden.npz,
    regenerated and compared when the reference is present).  The recorded run normalises in float32 (Wav2Vec2FeatureExtractor,
    2^-24 per sample) and is stored as float32; everything else on both sides is float64: rel L2 <= 1e-5."""
    gen = _gen()
    fix = np.load(os.path.join(golden_dir, "hubert_golden.npz"))
    assert set(fix.files) == set(gen.CASES)
    assert os.path.getsize(os.path.join(golden_dir, "hubert_golden.npz")) < (1 << 20)
    for i, (name, (n, step)) in enumerate(gen.CASES.items()):
        got = H.features(sd2, H.speech(n, gen.SEED + i))
        assert got.shape == ((n - 80) // 320, 1024)
        want = fix[name]
        assert want.shape == got[:, ::step].shape, name
        rel = _rel(got[:, ::step], want)
        print(f"{name}: {got.shape[0]} rows, rel L2 {rel:.2e}")
        assert rel <= 1e-5, name
    if HAVE_REFERENCE:
        fresh = gen.generate(REFERENCE)
        for k, v in fresh.items():
            assert np.allclose(v, fix[k], rtol=1e-5, atol=1e-6), k


# ------------------------------------------------------------------ HubertASR over a processor with step()
class _StepProcessor:
    """get_hubert_from_16k_speech as tests/test_ultralight_host.py's stand-in, plus step(): the same rows, sliced by first_row /
    row_step / rows with clamped indices, handed back as ONE array."""

    def __init__(self, with_step):
        self.calls = []
        self.stepped = []          # what every step() call returned
        if with_step:
            self.step = self._step

    def get_hubert_from_16k_speech(self, pcm):
        rows = (len(pcm) - 80) // 320
        feat = (np.random.default_rng(len(self.calls)).integers(-128, 128, (rows, 1024)) / 16.0).astype(np.float32)
        self.calls.append(len(pcm))
        return feat

    def _step(self, pcm, batch, first_row, row_step, rows):
        feat = self.get_hubert_from_16k_speech(pcm)
        idx = np.clip(first_row + row_step * np.arange(batch)[:, None] + np.arange(rows)[None], 0, len(feat) - 1)
        self.stepped.append(feat[idx])
        return self.stepped[-1]


def test_hubert_asr_uses_step_with_the_same_cadence_and_chunks():
    from livetalking_amd.avatars.audio_features.hubert import HubertASR
    opt = types.SimpleNamespace(fps=25, batch_size=4, l=10, r=10)
    procs = [_StepProcessor(False), _StepProcessor(True)]
    asrs = [HubertASR(opt, None, p, audio_feat_length=[4, 4]) for p in procs]
    for a in asrs:
        a.warm_up()
    rng = np.random.default_rng(0)
    for step in range(5):                                  # three speaking steps, then silence: one more extraction, then zeros
        for _ in range(2 * opt.batch_size):
            frame = rng.standard_normal(320).astype(np.float32)
            for a in asrs:
                if step < 3:
                    a.put_audio_frame(frame, {})
        for a in asrs:
            a.run_step()
        plain, stepped = (a.feat_queue.get_nowait() for a in asrs)
        assert procs[0].calls == procs[1].calls
        # every extraction of the second processor went through step(), and feat_queue carries views of the ONE array it returned
        assert len(procs[1].stepped) == len(procs[1].calls) and not procs[0].stepped
        if step < 4:
            assert all(np.shares_memory(c, procs[1].stepped[-1]) for c in stepped)
            assert all(c.base is procs[1].stepped[-1] for c in stepped)
        assert len(stepped) == opt.batch_size and all(c.shape == (16, 1024) for c in stepped)
        assert all(np.array_equal(np.asarray(a), np.asarray(b)) for a, b in zip(plain, stepped))
        assert all(len(a.frames) == 20 for a in asrs) and asrs[0].output_queue.qsize() == asrs[1].output_queue.qsize()
    assert len(procs[1].calls) == 4 and not any(np.asarray(c).any() for c in stepped)


def test_load_model_stays_on_torch_unless_asked(tmp_path, monkeypatch):
    """No argument, no environment: the FileNotFoundError of the default path, from the plugin's load_model too, with or without
    the opt-in (the directory check comes first)."""
    from livetalking_amd.avatars import ultralight_avatar as ul
    monkeypatch.chdir(tmp_path)
    for env, opt in ((None, types.SimpleNamespace()), ("1", types.SimpleNamespace()), (None, types.SimpleNamespace(hubert_engine=True))):
        if env is None:
            monkeypatch.delenv("LTK_HUBERT_ENGINE", raising=False)
        else:
            monkeypatch.setenv("LTK_HUBERT_ENGINE", env)
        with pytest.raises(FileNotFoundError, match="hubert-large-ls960-ft"):
            ul.load_model(opt)
