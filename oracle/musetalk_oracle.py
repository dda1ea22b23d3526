"""Oracle: MuseTalk per-frame generator (conditional U-Net + VAE decoder), plain torch on CPU.

TEST INFRASTRUCTURE ONLY (see oracle/__init__.py).

What the reference runs for this path (paths relative to the upstream checkout):
  avatars/musetalk_avatar.py:130-152   MuseReal.inference_batch
      latents (B,8,32,32) gathered by mirror_index; PE on the whisper features;
      unet.model(latent, timesteps=[0], encoder_hidden_states=feat).sample; vae.decode_latents
  avatars/musetalk/models/unet.py:12-27   PositionalEncoding (sinusoidal, d_model 384)
  avatars/musetalk/models/unet.py:36-46   diffusers.UNet2DConditionModel(**musetalk.json)
  avatars/musetalk/models/vae.py:96-108   decode_latents: latents/scaling_factor -> AutoencoderKL.decode
      -> (x/2+0.5).clamp(0,1) -> NHWC -> (x*255).round().astype(uint8) -> RGB->BGR

THIRD-PARTY ARITHMETIC, ABSENT HERE: `diffusers` is an unpinned requirement of the reference
(requirements.txt:41), is not vendored under the checkout and is not installed in this
container; the model config `models/musetalkV15/musetalk.json` and every checkpoint are not in
the tree either.  This module therefore RESTATES the published diffusers
algorithm for
  * UNet2DConditionModel with the MuseTalk-1.5 configuration (SD-1.x topology: in 8 / out 4,
    block_out_channels (320,640,1280,1280), layers_per_block 2, CrossAttnDown x3 + Down,
    Up + CrossAttnUp x3, 8 attention heads, cross_attention_dim 384, GroupNorm 32, SiLU,
    conv (not linear) proj_in/proj_out, GEGLU feed-forward, flip_sin_to_cos timestep embedding),
  * AutoencoderKL (sd-vae-ft-mse) decoder: post_quant_conv, conv_in, mid (resnet, 1-head
    attention, resnet), 4 up blocks x 3 resnets with nearest-2x upsample + conv, GN-SiLU-conv_out,
under diffusers' own state_dict key names, so a real checkpoint would load unchanged.

PARITY UNPINNED for the graph as a whole: no diffusers build, config file, checkpoint or golden tensor
exists in this container or in the reference tree to check this restatement against.  What IS pinned:
the ResnetBlock2D building block (GN -> SiLU -> conv -> GN -> SiLU -> conv + 1x1 shortcut) and the
asymmetric-pad stride-2 downsample, against the reference's own in-tree implementation
(avatars/musetalk/models/syncnet.py:71-139, imported with `diffusers` stubbed; golden tensors in
tests/golden/musetalk_blocks_golden.npz), the positional encoding (unet.py:12-27) and the Whisper side
(oracle/whisper_oracle.py calls the installed transformers); the Transformer2D composition (GN, 1x1 in, LN, attention +
residual, LN, GEGLU feed-forward + residual, 1x1 out + residual) against the reference's in-tree AttentionBlock2D
(syncnet.py:142-181, its two diffusers leaf classes replaced by the pinned multi-head attention and a literal GEGLU);
and the WHOLE VAE decoder / encoder graph against an independent implementation of the same network that is installed
here (transformers' Janus VQ-VAE = the taming / latent-diffusion autoencoder AutoencoderKL ports; tests/test_vae_pin.py,
2.7e-6).  Still unpinned: the U-Net's block wiring (down / mid / up order, skip concatenation, timestep embedding) and
diffusers' key names / config values.  The HIP path is required to match THIS statement within the fp16 tolerance
written in tests/test_musetalk_gpu.py.
"""
from __future__ import annotations

import math
from typing import Dict, List, Optional

import torch
import torch.nn.functional as F

Tensor = torch.Tensor
SD = Dict[str, Tensor]

# ---------------------------------------------------------------------------------------------
# configuration (MuseTalk 1.5 musetalk.json as published upstream; sd-vae-ft-mse config.json)
# ---------------------------------------------------------------------------------------------
UNET_IN, UNET_OUT = 8, 4
UNET_CH = (320, 640, 1280, 1280)
UNET_HEADS = 8
UNET_CTX_DIM = 384
UNET_GROUPS = 32
UNET_EPS = 1e-5            # norm_eps (resnets, conv_norm_out)
ATTN_GN_EPS = 1e-6         # Transformer2DModel.norm
LN_EPS = 1e-5
TIME_DIM = 1280
DOWN_HAS_ATTN = (True, True, True, False)
UP_HAS_ATTN = (False, True, True, True)

VAE_CH = (128, 256, 512, 512)
VAE_LATENT = 4
VAE_GROUPS = 32
VAE_EPS = 1e-6
VAE_SCALING = 0.18215


# ---------------------------------------------------------------------------------------------
# building blocks
# ---------------------------------------------------------------------------------------------
def conv2d_f64(x: Tensor, w: Tensor, b: Optional[Tensor], stride=1, pad=1) -> Tensor:
    """F.conv2d for float64 operands as unfold + one matrix product per image: the same sums, four to five times faster than
    torch's float64 convolution (which does not reach the threaded dgemm); only the float64 replay of oracle/op_replay.py comes here."""
    Co, Ci, kh, kw = w.shape
    Ho = (x.shape[2] + 2 * pad - kh) // stride + 1
    Wo = (x.shape[3] + 2 * pad - kw) // stride + 1
    wm = w.reshape(Co, -1)
    out = []
    for i in range(x.shape[0]):
        cols = x[i:i + 1].reshape(1, Ci, -1) if (kh == 1 and kw == 1 and stride == 1 and pad == 0) else F.unfold(x[i:i + 1], (kh, kw), padding=pad, stride=stride)
        out.append((wm @ cols[0]).reshape(Co, Ho, Wo))
    y = torch.stack(out)
    return y if b is None else y + b[None, :, None, None]


def _conv(sd: SD, p: str, x: Tensor, stride=1, pad=1) -> Tensor:
    if x.dtype == torch.float64:
        return conv2d_f64(x, sd[p + ".weight"], sd[p + ".bias"], stride, pad)
    return F.conv2d(x, sd[p + ".weight"], sd[p + ".bias"], stride=stride, padding=pad)


# fp8 conv path (BASELINE.json configs[4]; include/ltk.h ltk_musetalk_set_fp8): emulation of what the engine does when it
# is enabled -- the SiLU(GroupNorm(x)) in front of every ResnetBlock2D 3x3 conv is multiplied by `ascale`, saturated to
# +-448 and rounded to OCP e4m3 (round to nearest even); the conv weights are rounded to e4m3 after a per-output-channel
# scale 224 / max|w|; products and sums are fp32.  Off by default: the reference has no fp8 mode, this is OUR statement
# of the quantised path, used to check the kernels, and its distance to the unquantised oracle is what the fp8 test reports.
FP8 = {"on": False, "ascale": 8.0}


def fp8_round(x: Tensor) -> Tensor:
    return x.clamp(-448.0, 448.0).to(torch.float8_e4m3fn).float()


def fp8_weight(w: Tensor):
    """-> (dequantised weight, per-output-channel scale)"""
    m = w.abs().amax(dim=(1, 2, 3))
    # tensor / tensor: correctly rounded fp32 division like the engine's 224.f / m (torch evaluates `224.0 / m` as
    # 224 * reciprocal(m), one ulp off for some m, which flips the e4m3 rounding of weights that sit on a tie)
    sw = torch.where(m > 0, torch.full_like(m, 224.0) / m, torch.ones_like(m))
    return fp8_round(w * sw[:, None, None, None]) / sw[:, None, None, None], sw


def _conv3_q(sd: SD, p: str, x: Tensor) -> Tensor:
    """3x3 s1 p1 conv of a GroupNorm+SiLU output: fp8 operands when FP8 is on and the channel count allows it."""
    if not FP8["on"] or x.shape[1] % 32 != 0:
        return _conv(sd, p, x)
    a = float(FP8["ascale"])
    wq, _ = fp8_weight(sd[p + ".weight"])
    return F.conv2d(fp8_round(x * a) / a, wq, sd[p + ".bias"], padding=1)


def _linear(sd: SD, p: str, x: Tensor) -> Tensor:
    return F.linear(x, sd[p + ".weight"], sd.get(p + ".bias"))


def _gn(sd: SD, p: str, x: Tensor, groups: int, eps: float) -> Tensor:
    return F.group_norm(x, groups, sd[p + ".weight"], sd[p + ".bias"], eps)


def _ln(sd: SD, p: str, x: Tensor) -> Tensor:
    return F.layer_norm(x, (x.shape[-1],), sd[p + ".weight"], sd[p + ".bias"], LN_EPS)


def timestep_embedding(timesteps: Tensor, dim: int = 320) -> Tensor:
    """diffusers get_timestep_embedding(flip_sin_to_cos=True, downscale_freq_shift=0)."""
    half = dim // 2
    exponent = -math.log(10000.0) * torch.arange(half, dtype=torch.float32) / half
    emb = timesteps[:, None].float() * torch.exp(exponent)[None, :]
    emb = torch.cat([torch.sin(emb), torch.cos(emb)], dim=-1)
    return torch.cat([emb[:, half:], emb[:, :half]], dim=-1)   # cos first


def time_embed(sd: SD, timesteps: Tensor) -> Tensor:
    """UNet2DConditionModel.time_proj + time_embedding (linear -> SiLU -> linear) -> (1,1280)."""
    t = timestep_embedding(timesteps, UNET_CH[0]).to(sd["time_embedding.linear_1.weight"].dtype)     # (a float64 replay)
    t = _linear(sd, "time_embedding.linear_1", t)
    t = F.silu(t)
    return _linear(sd, "time_embedding.linear_2", t)


class OpTaps(dict):
    """A taps dict that asks for EVERY op-level tensor (mid_block, the VAE decoder, q / k / v): a plain dict keeps getting the
    taps it always got (block outputs, plus the ops of the blocks `detail` names)."""


def _ops(taps):
    return taps if isinstance(taps, OpTaps) else None


def _tap(taps, name, t, force=None, op=None):
    """Record `t` under `name`; with `force`, continue with what force(name, t) returns (None: with t).  `op` describes the op
    that produced t (kind, input tensors, parameters); a force object with a `describe` method is told first (oracle/op_replay.py
    builds its rounding model and its bound from that)."""
    if taps is not None:
        taps[name] = t.detach().clone()
    if force is not None:
        if op is not None and hasattr(force, "describe"):
            force.describe(name, op)
        r = force(name, t)
        if r is not None:
            t = r
    return t


def _tok_tap(taps, name, t, hw, force=None, op=None):
    """_tap for a token-major tensor (B, T, c): recorded, and forced, as (B, c, H, W) (hw = None: as (B, c, T, 1))."""
    if taps is None and force is None:
        return t
    B, T, c = t.shape
    H, W = hw if hw is not None else (T, 1)
    r = _tap(taps, name, t.reshape(B, H, W, c).permute(0, 3, 1, 2), force, op)
    return r.permute(0, 2, 3, 1).reshape(B, T, c)


def resnet(sd: SD, p: str, x: Tensor, temb: Optional[Tensor], groups: int, eps: float, taps=None, force=None) -> Tensor:
    """diffusers ResnetBlock2D (output_scale_factor 1, no up/down).  Without temb this is the reference's in-tree
    ResnetBlock2D (avatars/musetalk/models/syncnet.py:71-139): pinned against it by oracle/gen_golden_musetalk.py ->
    tests/golden/musetalk_blocks_golden.npz (tests/test_musetalk_host.py)."""
    f = force is not None
    n1 = _tap(taps, p + ".norm1", F.silu(_gn(sd, p + ".norm1", x, groups, eps)), force,
              f and dict(kind="gn", x=x, p=p + ".norm1", groups=groups, eps=eps, silu=True))
    h = _conv3_q(sd, p + ".conv1", n1)
    tb = None
    if temb is not None:
        tb = _linear(sd, p + ".time_emb_proj", F.silu(temb))
        h = h + tb[:, :, None, None]
    h = _tap(taps, p + ".conv1", h, force, f and dict(kind="conv", x=n1, p=p + ".conv1", stride=1, pad=1, q8=True, bias2=tb))
    n2 = _tap(taps, p + ".norm2", F.silu(_gn(sd, p + ".norm2", h, groups, eps)), force,
              f and dict(kind="gn", x=h, p=p + ".norm2", groups=groups, eps=eps, silu=True))
    h = _conv3_q(sd, p + ".conv2", n2)
    if (p + ".conv_shortcut.weight") in sd:
        x = _tap(taps, p + ".conv_shortcut", _conv(sd, p + ".conv_shortcut", x, pad=0), force,
                 f and dict(kind="conv", x=x, p=p + ".conv_shortcut", stride=1, pad=0))
    return _tap(taps, p + ".conv2", x + h, force, f and dict(kind="conv", x=n2, p=p + ".conv2", stride=1, pad=1, q8=True, res=x))


def downsample_asym(sd: SD, p: str, x: Tensor) -> Tensor:
    """diffusers Downsample2D(padding=0): one zero row / column at the bottom / right, then Conv2d(k3, s2, p0).
    Pinned (tests/golden/musetalk_blocks_golden.npz) against the in-tree equivalent, syncnet.py:112-121,136-138."""
    return _conv(sd, p, F.pad(x, (0, 1, 0, 1)), stride=2, pad=0)


def attention(sd: SD, p: str, x: Tensor, ctx: Tensor, heads: int, taps=None, force=None, hw=None, res: Optional[Tensor] = None) -> Tensor:
    """diffusers Attention (AttnProcessor2_0): q/k/v projections, scaled dot-product, to_out.0.
    `taps` gets ".attn" token-major (B, T, C) as before; an OpTaps also the projections.  `hw`: the query map's (H, W), the shape
    q / .attn / to_out.0 are forced in (the keys and values of a cross-attention as (B, C, Tk, 1)).  `res`: the residual that the
    caller adds to the result, so that a forced "to_out.0" is the device's `to_out.0(o) + res`; the sum is returned then."""
    B, T, C = x.shape
    f = force is not None
    ot = _ops(taps)
    self_attn = ctx is x
    q = _tok_tap(ot, p + ".to_q", _linear(sd, p + ".to_q", x), hw, force, f and dict(kind="linear", x=x, p=p + ".to_q", hw=hw, scale=float(C // heads) ** -0.5))
    khw = hw if self_attn else None
    k = _tok_tap(ot, p + ".to_k", _linear(sd, p + ".to_k", ctx), khw, force, f and dict(kind="linear", x=ctx, p=p + ".to_k", hw=khw))
    v = _tok_tap(ot, p + ".to_v", _linear(sd, p + ".to_v", ctx), khw, force, f and dict(kind="linear", x=ctx, p=p + ".to_v", hw=khw))
    d = C // heads
    qh = q.view(B, T, heads, d).transpose(1, 2)
    kh = k.view(B, -1, heads, d).transpose(1, 2)
    vh = v.view(B, -1, heads, d).transpose(1, 2)
    o = F.scaled_dot_product_attention(qh, kh, vh)            # scale = d ** -0.5
    o = o.transpose(1, 2).reshape(B, T, C)
    if taps is not None:
        taps[p + ".attn"] = o.detach().clone()            # (B, T, C) token-major
    if f:
        o = _tok_tap(None, p + ".attn", o, hw, force, dict(kind="attn", q=qh, k=kh, v=vh, hw=hw))
    out = _linear(sd, p + ".to_out.0", o)
    if res is None:
        return out
    return _tok_tap(None, p + ".to_out.0", out + res, hw, force, f and dict(kind="linear", x=o, p=p + ".to_out.0", res=res, hw=hw))


def transformer2d(sd: SD, p: str, x: Tensor, ctx: Optional[Tensor], taps=None, cross: bool = True, heads: int = UNET_HEADS,
                  groups: int = UNET_GROUPS, gn_eps: float = ATTN_GN_EPS, force=None) -> Tensor:
    """diffusers Transformer2DModel (use_linear_projection False) with one BasicTransformerBlock: GroupNorm -> 1x1 proj_in ->
    [LN -> self-attention + x; LN -> cross-attention + x; LN -> GEGLU feed-forward + x] -> 1x1 proj_out -> + input.
    `cross=False` drops the cross-attention sub-block: that is the reference's in-tree AttentionBlock2D
    (avatars/musetalk/models/syncnet.py:142-181), against which this function is pinned
    (oracle/gen_golden_musetalk.py, tests/golden/musetalk_blocks_golden.npz: same code path, one sub-block fewer).
    Token-major taps (B, T, C) are stored as (B, C, H, W) so they compare directly with the device tensors."""
    B, C, H, W = x.shape
    hw = (H, W)
    f = force is not None

    def tk(name, t, op=None):      # (B, T, c) -> (B, c, H, W)
        return _tok_tap(taps, name, t, hw, force, op)

    res = x
    h = _tap(taps, p + ".norm", _gn(sd, p + ".norm", x, groups, gn_eps), force,
             f and dict(kind="gn", x=x, p=p + ".norm", groups=groups, eps=gn_eps, silu=False))
    h = _tap(taps, p + ".proj_in", _conv(sd, p + ".proj_in", h, pad=0), force, f and dict(kind="conv", x=h, p=p + ".proj_in", stride=1, pad=0))
    h = h.permute(0, 2, 3, 1).reshape(B, H * W, C)
    b = p + ".transformer_blocks.0"
    n = tk(b + ".norm1", _ln(sd, b + ".norm1", h), f and dict(kind="ln", x=h, p=b + ".norm1", hw=hw))
    at = {} if taps is not None else None
    if isinstance(taps, OpTaps):
        at = OpTaps()
    h = _tok_tap(taps, b + ".attn1.to_out.0", attention(sd, b + ".attn1", n, n, heads, at, force, hw, res=h), hw)
    if cross:
        n = tk(b + ".norm2", _ln(sd, b + ".norm2", h), f and dict(kind="ln", x=h, p=b + ".norm2", hw=hw))
        h = _tok_tap(taps, b + ".attn2.to_out.0", attention(sd, b + ".attn2", n, ctx, heads, at, force, hw, res=h), hw)
    if at:
        for k, v in at.items():
            if k.endswith(".attn"):
                taps[k] = v.detach().reshape(B, H, W, -1).permute(0, 3, 1, 2).clone()
            else:
                taps[k] = v
    n = tk(b + ".norm3", _ln(sd, b + ".norm3", h), f and dict(kind="ln", x=h, p=b + ".norm3", hw=hw))
    g = tk(b + ".ff.net.0.proj", _linear(sd, b + ".ff.net.0.proj", n), f and dict(kind="linear", x=n, p=b + ".ff.net.0.proj", hw=hw))               # GEGLU
    a, gate = g.chunk(2, dim=-1)
    gg = tk(b + ".ff.geglu", a * F.gelu(gate), f and dict(kind="geglu", x=g, hw=hw))
    h = tk(b + ".ff.net.2", _linear(sd, b + ".ff.net.2", gg) + h, f and dict(kind="linear", x=gg, p=b + ".ff.net.2", res=h, hw=hw))
    h = h.reshape(B, H, W, C).permute(0, 3, 1, 2)
    hin = h
    h = _conv(sd, p + ".proj_out", h, pad=0)
    return _tap(taps, p + ".proj_out", h + res, force, f and dict(kind="conv", x=hin, p=p + ".proj_out", stride=1, pad=0, res=res))


def positional_encoding(x: Tensor) -> Tensor:
    """avatars/musetalk/models/unet.py:12-27 (d_model 384)."""
    b, t, d = x.shape
    pe = torch.zeros(t, d)
    position = torch.arange(0, t, dtype=torch.float).unsqueeze(1)
    div_term = torch.exp(torch.arange(0, d, 2).float() * (-math.log(10000.0) / d))
    pe[:, 0::2] = torch.sin(position * div_term)
    pe[:, 1::2] = torch.cos(position * div_term)
    return x + pe[None].to(x.dtype)


# ---------------------------------------------------------------------------------------------
# UNet2DConditionModel.forward
# ---------------------------------------------------------------------------------------------
def upsample_conv(sd: SD, p: str, x: Tensor, taps=None, force=None) -> Tensor:
    """diffusers Upsample2D: nearest 2x, then Conv2d(k3, p1)."""
    h = F.interpolate(x, scale_factor=2.0, mode="nearest")
    return _tap(taps, p, _conv(sd, p, h), force, force is not None and dict(kind="conv", x=h, p=p, stride=1, pad=1))


def unet_forward(sd: SD, latent: Tensor, ctx: Tensor, timestep: int = 0,
                 taps: Optional[Dict[str, Tensor]] = None, detail: Optional[str] = None, force=None) -> Tensor:
    """latent (B,8,32,32), ctx (B,50,384) (already position-encoded) -> (B,4,32,32).
    `force` (see _tap): every op's output, under the device's op name, may be replaced by the device's own tensor."""
    f = force is not None
    ot = _ops(taps)

    def tap(name, t):
        if taps is not None:
            taps[name] = t.detach().clone()
        return t

    def dt(prefix):       # op-level taps only for blocks whose name starts with `detail` (an OpTaps: for every block)
        return taps if (ot is not None or (taps is not None and detail is not None and prefix.startswith(detail))) else None

    temb = time_embed(sd, torch.tensor([timestep])).to(latent.dtype).expand(latent.shape[0], -1)
    h = tap("conv_in", _tap(None, "conv_in", _conv(sd, "conv_in", latent), force, f and dict(kind="conv", x=latent, p="conv_in", stride=1, pad=1)))
    skips: List[Tensor] = [h]
    for i in range(4):
        for j in range(2):
            h = resnet(sd, f"down_blocks.{i}.resnets.{j}", h, temb, UNET_GROUPS, UNET_EPS, dt(f"down_blocks.{i}.resnets.{j}"), force)
            if DOWN_HAS_ATTN[i]:
                h = transformer2d(sd, f"down_blocks.{i}.attentions.{j}", h, ctx, dt(f"down_blocks.{i}.attentions.{j}"), force=force)
            skips.append(tap(f"down_blocks.{i}.{j}", h))
        if i < 3:
            dp = f"down_blocks.{i}.downsamplers.0.conv"
            h = _tap(ot, dp, _conv(sd, dp, h, stride=2, pad=1), force, f and dict(kind="conv", x=h, p=dp, stride=2, pad=1))
            skips.append(tap(f"down_blocks.{i}.down", h))
    h = resnet(sd, "mid_block.resnets.0", h, temb, UNET_GROUPS, UNET_EPS, ot, force)
    h = transformer2d(sd, "mid_block.attentions.0", h, ctx, ot, force=force)
    h = tap("mid_block", resnet(sd, "mid_block.resnets.1", h, temb, UNET_GROUPS, UNET_EPS, ot, force))
    for i in range(4):
        for j in range(3):
            h = torch.cat([h, skips.pop()], dim=1)
            h = resnet(sd, f"up_blocks.{i}.resnets.{j}", h, temb, UNET_GROUPS, UNET_EPS, dt(f"up_blocks.{i}.resnets.{j}"), force)
            if UP_HAS_ATTN[i]:
                h = transformer2d(sd, f"up_blocks.{i}.attentions.{j}", h, ctx, dt(f"up_blocks.{i}.attentions.{j}"), force=force)
            tap(f"up_blocks.{i}.{j}", h)
        if i < 3:
            h = tap(f"up_blocks.{i}.up", upsample_conv(sd, f"up_blocks.{i}.upsamplers.0.conv", h, ot, force))
    hn = _tap(ot, "conv_norm_out", F.silu(_gn(sd, "conv_norm_out", h, UNET_GROUPS, UNET_EPS)), force,
              f and dict(kind="gn", x=h, p="conv_norm_out", groups=UNET_GROUPS, eps=UNET_EPS, silu=True))
    return tap("conv_out", _tap(None, "conv_out", _conv(sd, "conv_out", hn), force, f and dict(kind="conv", x=hn, p="conv_out", stride=1, pad=1)))


# ---------------------------------------------------------------------------------------------
# AutoencoderKL.decode (sd-vae-ft-mse)
# ---------------------------------------------------------------------------------------------
def vae_attention(sd: SD, p: str, x: Tensor, taps=None, force=None) -> Tensor:
    """diffusers Attention inside UNetMidBlock2D of the VAE: GroupNorm, 1 head, residual."""
    B, C, H, W = x.shape
    f = force is not None
    h = _tap(taps, p + ".group_norm", _gn(sd, p + ".group_norm", x, VAE_GROUPS, VAE_EPS), force,
             f and dict(kind="gn", x=x, p=p + ".group_norm", groups=VAE_GROUPS, eps=VAE_EPS, silu=False))
    h = h.view(B, C, H * W).transpose(1, 2)
    if not f and taps is None:
        h = attention(sd, p, h, h, 1)
        return h.transpose(1, 2).reshape(B, C, H, W) + x
    at = OpTaps() if taps is not None else None
    h = attention(sd, p, h, h, 1, at, force, (H, W), res=x.view(B, C, H * W).transpose(1, 2))
    h = h.transpose(1, 2).reshape(B, C, H, W)
    if taps is not None:
        for k, v in at.items():
            taps[k] = v.transpose(1, 2).reshape(B, C, H, W).clone() if k.endswith(".attn") else v
        taps[p + ".to_out.0"] = h.detach().clone()
    return h


def vae_decode(sd: SD, z: Tensor, taps: Optional[Dict[str, Tensor]] = None, force=None) -> Tensor:
    """AutoencoderKL.decode(z).sample: z (B,4,32,32) -> (B,3,256,256) RGB in ~[-1,1]."""
    f = force is not None
    ot = _ops(taps)

    def tap(name, t):
        if taps is not None:
            taps[name] = t.detach().clone()
        return t

    h = _tap(ot, "post_quant_conv", _conv(sd, "post_quant_conv", z, pad=0), force, f and dict(kind="conv", x=z, p="post_quant_conv", stride=1, pad=0))
    h = tap("decoder.conv_in", _tap(None, "decoder.conv_in", _conv(sd, "decoder.conv_in", h), force,
                                    f and dict(kind="conv", x=h, p="decoder.conv_in", stride=1, pad=1)))
    h = resnet(sd, "decoder.mid_block.resnets.0", h, None, VAE_GROUPS, VAE_EPS, ot, force)
    h = vae_attention(sd, "decoder.mid_block.attentions.0", h, ot, force)
    h = tap("decoder.mid_block", resnet(sd, "decoder.mid_block.resnets.1", h, None, VAE_GROUPS, VAE_EPS, ot, force))
    for i in range(4):
        for j in range(3):
            h = resnet(sd, f"decoder.up_blocks.{i}.resnets.{j}", h, None, VAE_GROUPS, VAE_EPS, ot, force)
        tap(f"decoder.up_blocks.{i}", h)
        if i < 3:
            h = upsample_conv(sd, f"decoder.up_blocks.{i}.upsamplers.0.conv", h, ot, force)
    hn = _tap(ot, "decoder.conv_norm_out", F.silu(_gn(sd, "decoder.conv_norm_out", h, VAE_GROUPS, VAE_EPS)), force,
              f and dict(kind="gn", x=h, p="decoder.conv_norm_out", groups=VAE_GROUPS, eps=VAE_EPS, silu=True))
    return tap("decoder.conv_out", _tap(None, "decoder.conv_out", _conv(sd, "decoder.conv_out", hn), force,
                                        f and dict(kind="conv", x=hn, p="decoder.conv_out", stride=1, pad=1)))


def vae_encode_moments(sd: SD, x: Tensor, taps: Optional[Dict[str, Tensor]] = None) -> Tensor:
    """AutoencoderKL.encode(x) up to the moments (mean | logvar): x (B,3,256,256) in [-1,1] -> (B,8,32,32).
    diffusers Encoder: conv_in, DownEncoderBlock2D x4 (2 resnets; Downsample2D(padding=0) = F.pad(0,1,0,1) + conv s2),
    UNetMidBlock2D, GN-SiLU-conv_out, then quant_conv."""
    h = _conv(sd, "encoder.conv_in", x)
    for i in range(4):
        for j in range(2):
            h = resnet(sd, f"encoder.down_blocks.{i}.resnets.{j}", h, None, VAE_GROUPS, VAE_EPS)
        if i < 3:
            h = downsample_asym(sd, f"encoder.down_blocks.{i}.downsamplers.0.conv", h)
        if taps is not None:
            taps[f"encoder.down_blocks.{i}"] = h.detach().clone()
    h = resnet(sd, "encoder.mid_block.resnets.0", h, None, VAE_GROUPS, VAE_EPS)
    h = vae_attention(sd, "encoder.mid_block.attentions.0", h)
    h = resnet(sd, "encoder.mid_block.resnets.1", h, None, VAE_GROUPS, VAE_EPS)
    if taps is not None:
        taps["encoder.mid_block"] = h.detach().clone()
    h = F.silu(_gn(sd, "encoder.conv_norm_out", h, VAE_GROUPS, VAE_EPS))
    h = _conv(sd, "encoder.conv_out", h)
    return _conv(sd, "quant_conv", h, pad=0)


def get_latents_for_unet(vae_sd: SD, face_bgr, noise: Optional[Tensor] = None) -> Tensor:
    """avatars/musetalk/models/vae.py:55-94,110-122 for one 256x256 BGR array -> (1,8,32,32).
    noise (2,4,32,32): the standard-normal draws of latent_dist.sample() for (masked, reference); None -> the mean."""
    import numpy as np
    img = np.asarray(face_bgr)[..., ::-1]                             # cv2.cvtColor(BGR2RGB)
    x = np.asarray([img]) / 255.
    x = torch.squeeze(torch.FloatTensor(np.transpose(x, (3, 0, 1, 2))))
    mask = torch.zeros((256, 256))
    mask[:128, :] = 1
    outs = []
    for k, half_mask in enumerate((True, False)):
        xi = x * (mask > 0.5) if half_mask else x
        xi = ((xi - 0.5) / 0.5).unsqueeze(0)
        mom = vae_encode_moments(vae_sd, xi)
        mean, logvar = mom[:, :4], torch.clamp(mom[:, 4:], -30.0, 20.0)
        z = mean if noise is None else mean + torch.exp(0.5 * logvar) * noise[k][None]
        outs.append(VAE_SCALING * z)
    return torch.cat(outs, dim=1)


def decode_latents(vae_sd: SD, latents: Tensor):
    """avatars/musetalk/models/vae.py:96-108 -> uint8 (B,256,256,3) BGR."""
    image = vae_decode(vae_sd, (1 / VAE_SCALING) * latents)       # vae.py:102: the reciprocal, then a product
    image = (image / 2 + 0.5).clamp(0, 1)
    image = image.detach().cpu().permute(0, 2, 3, 1).float().numpy()
    image = (image * 255).round().astype("uint8")
    return image[..., ::-1]


def inference_batch(unet_sd: SD, vae_sd: SD, latent_list_cycle, index: int, batch_size: int, whisper_batch):
    """avatars/musetalk_avatar.py:130-152 on explicit weights: uint8 (B,256,256,3) BGR."""
    from .paste_oracle import mirror_index
    length = len(latent_list_cycle)
    latent = torch.cat([latent_list_cycle[mirror_index(length, index + i)] for i in range(batch_size)], dim=0)
    feat = positional_encoding(torch.as_tensor(whisper_batch, dtype=torch.float32))
    pred = unet_forward(unet_sd, latent.float(), feat)
    return decode_latents(vae_sd, pred)
