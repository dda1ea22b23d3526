"""Float64 restatement of HuBERT-large for the tests (TEST INFRASTRUCTURE ONLY).

Restates transformers' HubertModel in the configuration of facebook/hubert-large-ls960-ft (feat_extract_norm "layer", conv_bias,
do_stable_layer_norm, feat_proj_layer_norm) as plain F.conv1d / F.linear / F.layer_norm calls over its state dict, called the way
avatars/ultralight/audio2feature.py:35,45 calls it (no attention mask, last_hidden_state), and that file's clip loop
(get_hubert_from_16k_speech, :15-54).  tests/test_hubert_host.py holds forward() to HubertModel(cfg).double() and features() to the
reference's own method; tests/golden/hubert_golden.npz (scripts/gen_golden_hubert.py) records the latter.

Every op is recorded / forced (oracle.musetalk_oracle._tap) under the name the device program gives it, as a (1, C, T, 1) tensor:
  feature_extractor.conv_layers.0.layer_norm      conv + LayerNorm + GELU of layer 0 (one kernel on the device)
  feature_extractor.conv_layers.i.conv / .layer_norm   (i = 1..6; the second one is LayerNorm + GELU)
  feature_projection.layer_norm / .projection, encoder.pos_conv_embed (h + GELU(conv)),
  encoder.layers.l.{layer_norm, attention.q_proj, .k_proj, .v_proj, attention.attn, attention.out_proj, final_layer_norm,
                    feed_forward.intermediate_dense, feed_forward.output_dense}, encoder.layer_norm

`fp16_model=True` is the rounding model of an fp16 implementation that the end-to-end tests measure against: matrix weights
rounded to fp16 (layer 0's ten-tap weights, biases and LayerNorm affines stay fp32, as on the device), every op output above
rounded to fp16, everything else float64.
"""
from __future__ import annotations

import math
from typing import Dict, Optional

import numpy as np
import torch
import torch.nn.functional as F

from oracle import op_replay as R
from oracle.musetalk_oracle import _tap, _tok_tap

CONV_K = (10, 3, 3, 3, 3, 2, 2)
CONV_S = (5, 2, 2, 2, 2, 2, 2)
D, HEADS, FF, C = 1024, 16, 4096, 512
POS_K, POS_GROUPS = 128, 16
EPS = 1e-5
KERNEL, STRIDE, CLIP = 400, 320, 320 * 1000          # audio2feature.py:21-23
G_KEY = "encoder.pos_conv_embed.conv.parametrizations.weight.original0"
V_KEY = "encoder.pos_conv_embed.conv.parametrizations.weight.original1"
W_KEY = "encoder.pos_conv_embed.conv.weight"


def config(layers: int):
    from transformers import HubertConfig
    return HubertConfig(hidden_size=D, num_hidden_layers=layers, num_attention_heads=HEADS, intermediate_size=FF, feat_extract_norm="layer",
                        conv_bias=True, conv_dim=(C,) * 7, conv_kernel=CONV_K, conv_stride=CONV_S, do_stable_layer_norm=True,
                        feat_proj_layer_norm=True, num_conv_pos_embeddings=POS_K, num_conv_pos_embedding_groups=POS_GROUPS,
                        layer_norm_eps=EPS, hidden_act="gelu", hidden_dropout=0.0, attention_dropout=0.0, activation_dropout=0.0,
                        feat_proj_dropout=0.0, final_dropout=0.0, layerdrop=0.0, mask_time_prob=0.05)


def rows(n_samples: int) -> int:
    t = n_samples
    for k, s in zip(CONV_K, CONV_S):
        t = (t - k) // s + 1
    return t


def state_dict(layers: int = 2, seed: int = 0) -> Dict[str, np.ndarray]:
    """HubertModel.state_dict() names (weight norm as parametrizations.weight.original0 / original1), float32, drawn from numpy:
    weights N(0, gain^2 / fan_in), biases 0.1 N, LayerNorm gains 1 + 0.2 N and biases 0.1 N, so that no activation is degenerate."""
    rng = np.random.default_rng(seed)
    sd: Dict[str, np.ndarray] = {}

    def w(shape, fan_in, gain=1.0):
        return (rng.standard_normal(shape, dtype=np.float32) * np.float32(gain / math.sqrt(fan_in)))

    def bias(n):
        return rng.standard_normal(n, dtype=np.float32) * np.float32(0.1)

    def norm(p, n):
        sd[p + ".weight"] = (1.0 + 0.2 * rng.standard_normal(n)).astype(np.float32)
        sd[p + ".bias"] = bias(n)

    def lin(p, cin, cout, gain=1.0):
        sd[p + ".weight"] = w((cout, cin), cin, gain)
        sd[p + ".bias"] = bias(cout)

    sd["masked_spec_embed"] = rng.uniform(0, 1, D).astype(np.float32)
    for i, k in enumerate(CONV_K):
        cin = 1 if i == 0 else C
        p = f"feature_extractor.conv_layers.{i}"
        sd[p + ".conv.weight"] = w((C, cin, k), cin * k, 1.4)
        sd[p + ".conv.bias"] = bias(C)
        norm(p + ".layer_norm", C)
    norm("feature_projection.layer_norm", C)
    lin("feature_projection.projection", C, D)
    sd["encoder.pos_conv_embed.conv.bias"] = bias(D)
    sd[G_KEY] = (2.8 * (1.0 + 0.1 * rng.standard_normal((1, 1, POS_K)))).astype(np.float32)
    sd[V_KEY] = rng.standard_normal((D, D // POS_GROUPS, POS_K), dtype=np.float32)
    norm("encoder.layer_norm", D)
    for l in range(layers):
        p = f"encoder.layers.{l}"
        for n in ("q_proj", "k_proj", "v_proj"):
            lin(f"{p}.attention.{n}", D, D, 1.5)
        lin(p + ".attention.out_proj", D, D, 0.5)
        norm(p + ".layer_norm", D)
        lin(p + ".feed_forward.intermediate_dense", D, FF, 1.4)
        lin(p + ".feed_forward.output_dense", FF, D, 0.5)
        norm(p + ".final_layer_norm", D)
    return sd


def weight_g_v_spelling(sd: Dict[str, np.ndarray]) -> Dict[str, np.ndarray]:
    """The same state dict under torch.nn.utils.weight_norm's older names."""
    out = {k: v for k, v in sd.items() if k not in (G_KEY, V_KEY)}
    out["encoder.pos_conv_embed.conv.weight_g"] = sd[G_KEY]
    out["encoder.pos_conv_embed.conv.weight_v"] = sd[V_KEY]
    return out


def fold_weight_norm(sd) -> Dict[str, torch.Tensor]:
    """float64 tensors with the positional conv's effective weight g * v / ||v|| (norm over dims 0, 1) under W_KEY."""
    out = {k: torch.as_tensor(np.asarray(v)).double() for k, v in sd.items()}
    if W_KEY not in out:
        old = G_KEY not in out
        g = out.pop("encoder.pos_conv_embed.conv.weight_g" if old else G_KEY)
        v = out.pop("encoder.pos_conv_embed.conv.weight_v" if old else V_KEY)
        out[W_KEY] = g * v / v.pow(2).sum(dim=(0, 1), keepdim=True).sqrt()
    return out


def normalise(pcm: np.ndarray) -> np.ndarray:
    """Wav2Vec2FeatureExtractor.zero_mean_unit_var_norm in float64."""
    x = np.asarray(pcm, dtype=np.float64)
    return (x - x.mean()) / np.sqrt(x.var() + 1e-7)


def speech(n: int, seed: int = 0) -> np.ndarray:
    """n samples of a seeded speech-like signal in [-1, 1]: a few drifting tones under an envelope, plus noise."""
    rng = np.random.default_rng(seed)
    t = np.arange(n) / 16000.0
    x = sum(a * np.sin(2 * np.pi * f * t + p) for a, f, p in zip((0.3, 0.2, 0.1), (140.0, 410.0, 2300.0), rng.uniform(0, 6.28, 3)))
    env = 0.55 + 0.45 * np.sin(2 * np.pi * 3.1 * t)
    return (env * x + 0.02 * rng.standard_normal(n)).astype(np.float32)


def forward(sd, x_norm, fp16_model: bool = False, taps: Optional[dict] = None, force=None) -> torch.Tensor:
    """x_norm: the normalised waveform (n,) -> last_hidden_state (T, 1024), float64.  sd: state_dict() (either spelling of the weight
    norm, or folded)."""
    sd = fold_weight_norm(sd)
    f = force is not None

    def r16(t):
        return t.half().double() if fp16_model else t

    def w(name):
        t = sd[name]
        return t.float().half().double() if fp16_model else t

    def ln(p, x):
        return F.layer_norm(x, (x.shape[-1],), sd[p + ".weight"], sd[p + ".bias"], EPS)

    def lin(p, x):
        return F.linear(x, w(p + ".weight"), sd[p + ".bias"])

    with torch.no_grad():
        x = torch.as_tensor(np.asarray(x_norm)).double().reshape(1, 1, -1)
        # layer 0: its weights stay fp32 on the device
        p = "feature_extractor.conv_layers.0"
        z = F.conv1d(x, sd[p + ".conv.weight"], sd[p + ".conv.bias"], stride=CONV_S[0]).transpose(1, 2)
        h = _tok_tap(taps, p + ".layer_norm", r16(F.gelu(ln(p + ".layer_norm", z))), None, force,
                     f and dict(kind="l0", x=x, p=p))
        for i in range(1, 7):
            p = f"feature_extractor.conv_layers.{i}"
            xin = h.transpose(1, 2)
            c = r16(F.conv1d(xin, w(p + ".conv.weight"), sd[p + ".conv.bias"], stride=CONV_S[i]))
            c = _tap(taps, p + ".conv", c[..., None], force, f and dict(kind="conv1d", x=xin, p=p + ".conv", stride=CONV_S[i]))[..., 0]
            c = c.transpose(1, 2)
            h = _tok_tap(taps, p + ".layer_norm", r16(F.gelu(ln(p + ".layer_norm", c))), None, force,
                         f and dict(kind="ln_gelu", x=c, p=p + ".layer_norm"))
        p = "feature_projection"
        n0 = _tok_tap(taps, p + ".layer_norm", r16(ln(p + ".layer_norm", h)), None, force, f and dict(kind="ln", x=h, p=p + ".layer_norm"))
        h = _tok_tap(taps, p + ".projection", r16(lin(p + ".projection", n0)), None, force, f and dict(kind="linear", x=n0, p=p + ".projection"))
        p = "encoder.pos_conv_embed"
        pc = F.conv1d(h.transpose(1, 2), w(W_KEY), sd[p + ".conv.bias"], padding=POS_K // 2, groups=POS_GROUPS)[:, :, :-1]
        h = _tok_tap(taps, p, r16(h + F.gelu(pc.transpose(1, 2))), None, force, f and dict(kind="posconv", x=h, p=p + ".conv"))
        n_layers = len({k.split(".")[2] for k in sd if k.startswith("encoder.layers.")})
        d = D // HEADS
        for l in range(n_layers):
            p = f"encoder.layers.{l}"
            a = p + ".attention"
            B, T, _ = h.shape
            n1 = _tok_tap(taps, p + ".layer_norm", r16(ln(p + ".layer_norm", h)), None, force, f and dict(kind="ln", x=h, p=p + ".layer_norm"))
            q = _tok_tap(taps, a + ".q_proj", r16(lin(a + ".q_proj", n1)), None, force, f and dict(kind="linear", x=n1, p=a + ".q_proj", scale=float(d) ** -0.5))
            k = _tok_tap(taps, a + ".k_proj", r16(lin(a + ".k_proj", n1)), None, force, f and dict(kind="linear", x=n1, p=a + ".k_proj"))
            v = _tok_tap(taps, a + ".v_proj", r16(lin(a + ".v_proj", n1)), None, force, f and dict(kind="linear", x=n1, p=a + ".v_proj"))
            qh, kh, vh = (t.view(B, T, HEADS, d).transpose(1, 2) for t in (q, k, v))
            o = torch.softmax(qh @ kh.transpose(-1, -2) * d ** -0.5, dim=-1) @ vh
            o = _tok_tap(taps, a + ".attn", r16(o.transpose(1, 2).reshape(B, T, D)), None, force, f and dict(kind="attn", q=qh, k=kh, v=vh))
            h1 = _tok_tap(taps, a + ".out_proj", r16(lin(a + ".out_proj", o) + h), None, force, f and dict(kind="linear", x=o, p=a + ".out_proj", res=h))
            n2 = _tok_tap(taps, p + ".final_layer_norm", r16(ln(p + ".final_layer_norm", h1)), None, force,
                          f and dict(kind="ln", x=h1, p=p + ".final_layer_norm"))
            ff = p + ".feed_forward"
            f1 = _tok_tap(taps, ff + ".intermediate_dense", r16(F.gelu(lin(ff + ".intermediate_dense", n2))), None, force,
                          f and dict(kind="linear", x=n2, p=ff + ".intermediate_dense", act="gelu"))
            h = _tok_tap(taps, ff + ".output_dense", r16(lin(ff + ".output_dense", f1) + h1), None, force,
                         f and dict(kind="linear", x=f1, p=ff + ".output_dense", res=h1))
        out = _tok_tap(taps, "encoder.layer_norm", r16(ln("encoder.layer_norm", h)), None, force, f and dict(kind="ln", x=h, p="encoder.layer_norm"))
        return out[0]


def op_names(layers: int):
    """The ops of the device program in execution order, as Engine.hubert_ops() names them."""
    out = ["feature_extractor.conv_layers.0.layer_norm"]
    for i in range(1, 7):
        out += [f"feature_extractor.conv_layers.{i}.conv", f"feature_extractor.conv_layers.{i}.layer_norm"]
    out += ["feature_projection.layer_norm", "feature_projection.projection", "encoder.pos_conv_embed"]
    for l in range(layers):
        p = f"encoder.layers.{l}."
        out += [p + n for n in ("layer_norm", "attention.q_proj", "attention.k_proj", "attention.v_proj", "attention", "attention.out_proj",
                                "final_layer_norm", "feed_forward.intermediate_dense", "feed_forward.output_dense")]
    return out + ["encoder.layer_norm"]


def clip_ranges(n: int):
    """audio2feature.py:24-47: [start, end) of every forward of an n-sample utterance."""
    out = []
    n_iter = n // CLIP
    for i in range(n_iter):
        out.append((CLIP * i, min(n, CLIP * i + CLIP - STRIDE + KERNEL)))
    if n - CLIP * n_iter >= KERNEL:
        out.append((CLIP * n_iter, n))
    return out


def features(sd, pcm, fp16_model: bool = False, fwd=None) -> np.ndarray:
    """get_hubert_from_16k_speech restated: normalise over the whole input, forward the clips and the tail, concatenate, pad with
    zero rows or trim to (n - 80) // 320 rows.  fwd(x_norm_clip) -> (T, 1024) replaces forward() (tests)."""
    pcm = np.asarray(pcm)
    if pcm.ndim == 2:
        pcm = pcm[:, 0]
    x = normalise(pcm)
    expected = (len(x) - (KERNEL - STRIDE)) // STRIDE
    run = fwd or (lambda c: forward(sd, c, fp16_model=fp16_model).numpy())
    ret = np.concatenate([np.asarray(run(x[a:b])) for a, b in clip_ranges(len(x))], axis=0)
    assert abs(ret.shape[0] - expected) <= 1
    if ret.shape[0] < expected:
        ret = np.concatenate([ret, np.zeros((expected - ret.shape[0], ret.shape[1]), ret.dtype)])
    return ret[:expected]


# ---------------------------------------------------------------------------------------------------- op replay
def posconv_parts(x: torch.Tensor, W: torch.Tensor, b: torch.Tensor):
    """x (1, T, 1024) float32 -> (acc, lin_tol) of the grouped conv before the GELU, token-major: op_replay's conv / linear bound
    with K = 64 x 128 = 8192 products (short_sum(8192) = 1)."""
    xt = x.transpose(1, 2)
    K = W.shape[1] * W.shape[2]
    acc = F.conv1d(xt, R.f16(W), b, padding=POS_K // 2, groups=POS_GROUPS)[:, :, :-1]
    A = R.short_sum(K) * F.conv1d(xt.abs(), W.abs(), None, padding=POS_K // 2, groups=POS_GROUPS)[:, :, :-1] + 4 * b.abs()[None, :, None]
    gs = xt.abs().reshape(1, POS_GROUPS, -1, xt.shape[-1]).sum(2)                                   # sum |x| over a group's channels
    s = 2.0 ** -24 * F.conv1d(gs, torch.ones(POS_GROUPS, 1, POS_K), None, padding=POS_K // 2, groups=POS_GROUPS)[:, :, :-1]
    s = s.repeat_interleave(W.shape[0] // POS_GROUPS, dim=1)
    return acc.transpose(1, 2), (R.C_LIN * A + s).transpose(1, 2)


def posconv_model(x: torch.Tensor, W: torch.Tensor, b: torch.Tensor, ref_tok: torch.Tensor):
    """-> (mod, tol), token-major: GELU bound of op_replay's linear layers (slope 1.13, 2^-23 |acc| for the fp32 erf term), the
    residual added in fp32, one rounding to fp16."""
    acc, lin_tol = posconv_parts(x, W, b)
    tol = 2.0 ** -10 * ref_tok.abs() + R.GELU_SLOPE * lin_tol + 2.0 ** -23 * acc.abs()
    return R.f16(x + F.gelu(acc)), tol


def ln_gelu_model(x: torch.Tensor, gamma: torch.Tensor, beta: torch.Tensor, ref_tok: torch.Tensor, extra: Optional[torch.Tensor] = None):
    """LayerNorm + GELU, token-major x (1, T, C) float32 -> (mod, tol): op_replay's LayerNorm bound (A = |gamma| |x_hat| + |beta|,
    c = 2^-10, and the mean's tree-sum term) through the GELU (slope 1.13, 2^-23 |z|).  extra: a bound on the error x itself carries
    (layer 0's fp32 conv), which reaches x_hat as rstd (extra + its mean over the channels)."""
    n = x.shape[-1]
    xh = F.layer_norm(x, (n,), None, None, EPS)
    z = xh * gamma + beta
    rstd = torch.rsqrt(x.var(-1, unbiased=False, keepdim=True) + EPS)
    A = xh.abs() * gamma.abs() + beta.abs()
    sm = 2.0 ** -24 * math.ceil(math.log2(n)) * gamma.abs() * x.mean(-1, keepdim=True).abs() * rstd
    t = R.C_ACT * A + sm
    if extra is not None:
        t = t + gamma.abs() * rstd * (extra + extra.mean(-1, keepdim=True))
    tol = 2.0 ** -10 * ref_tok.abs() + R.GELU_SLOPE * t + 2.0 ** -23 * z.abs()
    return R.f16(F.gelu(z)), tol


def layer0_model(x: torch.Tensor, W: torch.Tensor, b: torch.Tensor, gamma, beta, ref_tok):
    """x (1, 1, n) float32.  The conv is 10 fp32 fmas on fp32 weights: each output within 11 * 2^-24 (|w| (*) |x| + |b|)."""
    z = F.conv1d(x, W, b, stride=CONV_S[0]).transpose(1, 2)
    e0 = 11 * 2.0 ** -24 * (F.conv1d(x.abs(), W.abs(), b.abs(), stride=CONV_S[0])).transpose(1, 2)
    return ln_gelu_model(z, gamma, beta, ref_tok, extra=e0)


class HubertReplay(R.Replay):
    """op_replay.Replay with the models of the ops only HuBERT has."""

    def model(self, name, op, ref):
        kind = op["kind"]
        nchw = lambda t: R._tok_to_nchw(t, None)
        ref_tok = ref[..., 0].transpose(1, 2).float()
        if kind == "conv1d":
            x = op["x"].float()
            W, b = self._w(op["p"])
            st = op["stride"]
            acc = F.conv1d(x, R.f16(W), b, stride=st)
            A = R.short_sum(W.shape[1] * W.shape[2]) * F.conv1d(x.abs(), W.abs(), None, stride=st) + 4 * b.abs()[None, :, None]
            s = 2.0 ** -24 * F.conv1d(x.abs().sum(1, keepdim=True), torch.ones(1, 1, W.shape[2]), None, stride=st)
            return R.f16(acc)[..., None], (2.0 ** -10 * ref.abs() + (R.C_LIN * A + s)[..., None]), True
        if kind == "ln_gelu":
            gamma, beta = self._w(op["p"])
            mod, tol = ln_gelu_model(op["x"].float(), gamma, beta, ref_tok)
            return nchw(mod), nchw(tol), True
        if kind == "l0":
            p = op["p"]
            W, b = self._w(p + ".conv")
            gamma, beta = self._w(p + ".layer_norm")
            mod, tol = layer0_model(op["x"].float(), W, b, gamma, beta, ref_tok)
            return nchw(mod), nchw(tol), True
        if kind == "posconv":
            W, b = self._w(op["p"])
            mod, tol = posconv_model(op["x"].float(), W, b, ref_tok)
            return nchw(mod), nchw(tol), True
        return super().model(name, op, ref)


def replay(sd, x_norm, fetch) -> HubertReplay:
    """sd: state dict (any spelling); x_norm: the device's own "input_values"; fetch(name, ref) -> the device's tensor."""
    folded = fold_weight_norm(sd)
    rp = HubertReplay({k: v.float() for k, v in folded.items()}, fetch)
    rp.may_fuse = {}
    forward(folded, x_norm, force=rp)
    return rp
