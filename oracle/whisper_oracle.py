"""Oracle: MuseTalk audio features (Whisper-tiny encoder states + chunk slicing), CPU.

TEST INFRASTRUCTURE ONLY (see oracle/__init__.py).

Reference path:
  avatars/audio_features/whisper.py:58-76   WhisperASR.run_step (52 chunks -> audio2feat -> _feature2chunks)
  avatars/audio_features/whisper.py:35-56   _feature2chunks
  avatars/audio_features/base_asr.py:91-133 _get_sliced_feature (index clamping)
  avatars/musetalk/whisper/audio2feature.py:15-23,106-117  Audio2Feature: AutoFeatureExtractor + WhisperModel.encoder
      (output_hidden_states=True) -> torch.stack(hidden_states, dim=2) -> (1500, 5, 384)

Third-party arithmetic: `transformers` (WhisperFeatureExtractor, WhisperModel) IS installed in this image, so this
oracle CALLS it instead of restating it - the checker is the library the reference itself calls.  The model is a
whisper-tiny-shaped WhisperModel with seeded random weights (no checkpoint exists in the reference tree or here).
"""
from __future__ import annotations

import numpy as np
import torch


def tiny_whisper(seed: int = 0):
    from transformers import WhisperConfig, WhisperModel
    cfg = WhisperConfig(d_model=384, encoder_layers=4, encoder_attention_heads=6, encoder_ffn_dim=1536, decoder_layers=4,
                        decoder_attention_heads=6, decoder_ffn_dim=1536, num_mel_bins=80, max_source_positions=1500,
                        vocab_size=51865)
    torch.manual_seed(seed)
    return WhisperModel(cfg).eval()


def input_features(wav: np.ndarray) -> torch.Tensor:
    """audio2feature.py:107-111 -> (1, 80, 3000) float32."""
    from transformers import WhisperFeatureExtractor
    fe = WhisperFeatureExtractor()
    return fe(np.asarray(wav, dtype=np.float32), return_tensors="pt", sampling_rate=16000).input_features


def audio2feat(model, wav: np.ndarray):
    """audio2feature.py:106-117 on CPU/fp32 -> (1500, 5, 384) and the list of hidden states."""
    feats = input_features(wav)
    with torch.no_grad():
        hs = model.encoder(feats, output_hidden_states=True).hidden_states
    return torch.stack(hs, dim=2).squeeze(0).numpy(), [h.squeeze(0) for h in hs], feats


def encoder_op_names(layers: int = 4):
    """The ops of the device's Whisper program, under the names ltk_whisper_debug_get takes."""
    names = ["conv1", "conv2", "embed_positions"]
    for l in range(layers):
        p = f"layers.{l}."
        names += [p + n for n in ("self_attn_layer_norm", "self_attn.q_proj", "self_attn.k_proj", "self_attn.v_proj", "self_attn.attn",
                                  "self_attn.out_proj", "final_layer_norm", "fc1", "fc2")]
    return names + ["layer_norm"]


# the device adds the positions in place on conv2's output: that tensor is compared as the group's output
FUSED_INTO = {"conv2": "embed_positions"}


def encoder_ops(sd, feats: torch.Tensor, force=None, taps=None, heads: int = 6):
    """transformers' WhisperEncoder.forward restated op by op on the encoder's state dict (tests/test_op_replay.py holds it to the
    library's own hidden states), so that every op's output can be recorded and forced (see musetalk_oracle._tap) under the
    device's op names.  feats (1, 80, 3000) -> the five hidden states (embeddings, layers 0-2, final LayerNorm), each (1, 1500, 384).
    Tensors are recorded and forced as (1, C, T, 1)."""
    import torch.nn.functional as F
    from .musetalk_oracle import _tok_tap, _tap
    f = force is not None

    def conv(name, x, stride):
        return F.gelu(F.conv1d(x, sd[name + ".weight"], sd[name + ".bias"], stride=stride, padding=1))

    def lin(p, x):
        return F.linear(x, sd[p + ".weight"], sd.get(p + ".bias"))

    def ln(p, x):
        return F.layer_norm(x, (x.shape[-1],), sd[p + ".weight"], sd[p + ".bias"], 1e-5)

    c1 = _tap(taps, "conv1", conv("conv1", feats, 1)[..., None], force, f and dict(kind="conv1d_gelu", x=feats, p="conv1", stride=1))[..., 0]
    c2 = _tap(taps, "conv2", conv("conv2", c1, 2)[..., None], force, f and dict(kind="conv1d_gelu", x=c1, p="conv2", stride=2))[..., 0]
    pos = sd["embed_positions.weight"]
    h = _tok_tap(taps, "embed_positions", c2.permute(0, 2, 1) + pos, None, force, f and dict(kind="add_pos", x=c2, pos=pos))
    states = [h]
    n_layers = len({k.split(".")[1] for k in sd if k.startswith("layers.")})
    for l in range(n_layers):
        p = f"layers.{l}"
        B, T, C = h.shape
        d = C // heads
        n1 = _tok_tap(taps, p + ".self_attn_layer_norm", ln(p + ".self_attn_layer_norm", h), None, force, f and dict(kind="ln", x=h, p=p + ".self_attn_layer_norm"))
        a = p + ".self_attn"
        q = _tok_tap(taps, a + ".q_proj", lin(a + ".q_proj", n1), None, force, f and dict(kind="linear", x=n1, p=a + ".q_proj", scale=float(d) ** -0.5))
        k = _tok_tap(taps, a + ".k_proj", lin(a + ".k_proj", n1), None, force, f and dict(kind="linear", x=n1, p=a + ".k_proj"))
        v = _tok_tap(taps, a + ".v_proj", lin(a + ".v_proj", n1), None, force, f and dict(kind="linear", x=n1, p=a + ".v_proj"))
        qh, kh, vh = (t.view(B, T, heads, d).transpose(1, 2) for t in (q, k, v))
        o = F.scaled_dot_product_attention(qh, kh, vh).transpose(1, 2).reshape(B, T, C)
        o = _tok_tap(taps, a + ".attn", o, None, force, f and dict(kind="attn", q=qh, k=kh, v=vh))
        h1 = _tok_tap(taps, a + ".out_proj", lin(a + ".out_proj", o) + h, None, force, f and dict(kind="linear", x=o, p=a + ".out_proj", res=h))
        n2 = _tok_tap(taps, p + ".final_layer_norm", ln(p + ".final_layer_norm", h1), None, force, f and dict(kind="ln", x=h1, p=p + ".final_layer_norm"))
        f1 = _tok_tap(taps, p + ".fc1", F.gelu(lin(p + ".fc1", n2)), None, force, f and dict(kind="linear", x=n2, p=p + ".fc1", act="gelu"))
        h = _tok_tap(taps, p + ".fc2", lin(p + ".fc2", f1) + h1, None, force, f and dict(kind="linear", x=f1, p=p + ".fc2", res=h1))
        if l + 1 < n_layers:
            states.append(h)
    states.append(_tok_tap(taps, "layer_norm", ln("layer_norm", h), None, force, f and dict(kind="ln", x=h, p="layer_norm")))
    return states


def get_sliced_feature(feature_array, vid_idx, audio_feat_win, feature_idx_multiplier=1.0):
    """base_asr.py:91-133."""
    length = feature_array.shape[0]
    center_idx = int(vid_idx * feature_idx_multiplier)
    left = int(center_idx - audio_feat_win[0] * feature_idx_multiplier)
    right = int(center_idx + audio_feat_win[1] * feature_idx_multiplier)
    sel = []
    for idx in range(left, right):
        idx = min(length - 1, max(0, idx))
        sel.append(feature_array[idx])
    return np.asarray(sel)


def feature2chunks(feature_array, batch_size, l: int = 10):
    """whisper.py:35-56 as run_step calls it (whisper.py:71-73): win [0,5], start l/2, multiplier 2."""
    chunks = []
    for i in range(batch_size):
        sel = get_sliced_feature(feature_array, i + l / 2, [0, 5], 2)
        chunks.append(sel.reshape(-1, 384))
    return chunks
