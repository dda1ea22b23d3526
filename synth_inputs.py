"""Seeded synthetic inputs for parity tests and the bench.

Input generators only - no reference arithmetic lives here, and nothing under
oracle/ is imported.  There are no trained
weights, avatar banks or audio clips in the reference tree, so every parity
claim is made on these seeded stand-ins:

* weights  - He-scaled conv kernels + randomised BatchNorm affine/running stats
             under the reference state_dict names
             (avatars/wav2lip/models/wav2lip_v2.py:12-91, conv.py:5-44);
* audio    - the tone+noise formula of benchmark_asr.py:44-59;
* avatar   - smooth low-pass-noise face crops / full frames and (y1,y2,x1,x2)
             boxes in the layout `load_avatar` returns
             (avatars/wav2lip_avatar.py:72-88, avatars/wav2lip/genavatar.py:130).

Generators use numpy's PCG64 (`default_rng`) only, which is bit-stable across
platforms, so the GPU box regenerates the exact tensors the golden fixtures
were made from.
"""
from __future__ import annotations

from typing import Dict, List, Tuple

import numpy as np


# (state_dict prefix, kind, cin, cout, k, stride_product, residual) for the 54 Conv2d/Conv2dTranspose
# blocks of avatars/wav2lip/models/wav2lip_v2.py:12-89, in state_dict order: only what the
# generator needs (shapes + fan-in).  The engine's own table lives in csrc/w2l_program.hip.
def _layers():
    L = []
    def c(p, cin, cout, k, s=1, res=False): L.append((p, "conv", cin, cout, k, s, res))
    def t(p, cin, cout, k, s): L.append((p, "convT", cin, cout, k, s, False))
    a = "audio_encoder."
    c(a + "0", 1, 32, 3); c(a + "1", 32, 32, 3, 1, True); c(a + "2", 32, 32, 3, 1, True)
    c(a + "3", 32, 64, 3, 3); c(a + "4", 64, 64, 3, 1, True); c(a + "5", 64, 64, 3, 1, True)
    c(a + "6", 64, 128, 3, 9); c(a + "7", 128, 128, 3, 1, True); c(a + "8", 128, 128, 3, 1, True)
    c(a + "9", 128, 256, 3, 6); c(a + "10", 256, 256, 3, 1, True); c(a + "11", 256, 512, 3); c(a + "12", 512, 512, 1)
    e = "face_encoder_blocks."
    c(e + "0.0", 6, 16, 7)
    for b, (ci, co, n) in enumerate([(16, 32, 2), (32, 64, 3), (64, 128, 2), (128, 256, 2), (256, 512, 1), (512, 512, 1)], start=1):
        c(e + f"{b}.0", ci, co, 3, 4)
        for j in range(1, n + 1): c(e + f"{b}.{j}", co, co, 3, 1, True)
    c(e + "7.0", 512, 512, 4); c(e + "7.1", 512, 512, 1)
    d = "face_decoder_blocks."
    c(d + "0.0", 512, 512, 1)
    t(d + "1.0", 1024, 512, 4, 1); c(d + "1.1", 512, 512, 3, 1, True)
    for b, (ci, co, n) in enumerate([(1024, 512, 1), (1024, 512, 2), (768, 384, 2), (512, 256, 2), (320, 128, 2), (160, 64, 2)], start=2):
        t(d + f"{b}.0", ci, co, 3, 4)
        for j in range(1, n + 1): c(d + f"{b}.{j}", co, co, 3, 1, True)
    c("output_block.0", 80, 32, 3)
    return L

OUTPUT_HEAD_PREFIX = "output_block.1"


def wav2lip_state_dict(seed: int = 1234, gain: float = 1.0) -> Dict[str, np.ndarray]:
    """Reference-named fp32 state_dict as numpy arrays (380 tensors).

    `gain` (parity-stress family, tests/test_parity_stress_gpu.py): the BatchNorm affine of the two input layers
    (face_encoder_blocks.0.0, audio_encoder.0) is multiplied by it, so every activation behind them grows about
    linearly with it (peak |activation| of the fp32 forward: ~70 at gain 1, ~1.2e3 at 16, ~1.9e4 at 256, past the
    fp16 limit 65 504 from ~1024 on), and the output head's weights are divided by it so that the sigmoid keeps
    working across its range.  gain = 1 is the draw every other test uses."""
    rng = np.random.default_rng(seed)
    sd: Dict[str, np.ndarray] = {}
    for prefix, kind, cin, cout, k, sprod, residual in _layers():
        if kind == "conv":
            shape = (cout, cin, k, k)            # nn.Conv2d layout
            fan_in = cin * k * k
        else:
            shape = (cin, cout, k, k)            # nn.ConvTranspose2d layout
            # each output pixel of the s2 transposed conv sees ~k*k/s*s taps
            fan_in = cin * k * k / sprod
        std = np.sqrt(2.0 / fan_in)
        sd[prefix + ".conv_block.0.weight"] = (rng.standard_normal(shape) * std).astype(np.float32)
        sd[prefix + ".conv_block.0.bias"] = (rng.standard_normal(cout) * 0.05).astype(np.float32)
        # residual layers: damp the conv branch so y = relu(bn(conv(x)) + x) stays bounded
        g_lo, g_hi = (0.3, 0.7) if residual else (0.7, 1.3)
        sd[prefix + ".conv_block.1.weight"] = rng.uniform(g_lo, g_hi, cout).astype(np.float32)
        sd[prefix + ".conv_block.1.bias"] = (rng.standard_normal(cout) * 0.1).astype(np.float32)
        sd[prefix + ".conv_block.1.running_mean"] = (rng.standard_normal(cout) * 0.2).astype(np.float32)
        sd[prefix + ".conv_block.1.running_var"] = rng.uniform(0.6, 1.6, cout).astype(np.float32)
        sd[prefix + ".conv_block.1.num_batches_tracked"] = np.asarray(1000, dtype=np.int64)
    # output head: plain conv 32->3; scaled so the sigmoid is used across its range
    sd[OUTPUT_HEAD_PREFIX + ".weight"] = (rng.standard_normal((3, 32, 1, 1)) * 0.04).astype(np.float32)
    sd[OUTPUT_HEAD_PREFIX + ".bias"] = (rng.standard_normal(3) * 0.2).astype(np.float32)
    if gain != 1.0:
        g = np.float32(gain)
        for p in ("face_encoder_blocks.0.0", "audio_encoder.0"):
            sd[p + ".conv_block.1.weight"] = sd[p + ".conv_block.1.weight"] * g
            sd[p + ".conv_block.1.bias"] = sd[p + ".conv_block.1.bias"] * g
        sd[OUTPUT_HEAD_PREFIX + ".weight"] = sd[OUTPUT_HEAD_PREFIX + ".weight"] / g
    return sd


def synthetic_audio(duration_s: float, sample_rate: int = 16000, seed: int = 42) -> np.ndarray:
    """benchmark_asr.py:44-59 (same constants, same seed by default)."""
    rng = np.random.default_rng(seed)
    t = np.linspace(0, duration_s, int(sample_rate * duration_s), dtype=np.float32)
    audio = (
        0.3 * np.sin(2 * np.pi * 200 * t)
        + 0.2 * np.sin(2 * np.pi * 500 * t)
        + 0.1 * np.sin(2 * np.pi * 1200 * t)
        + 0.15 * rng.standard_normal(len(t)).astype(np.float32)
    )
    fade = int(0.05 * sample_rate)
    audio[:fade] *= np.linspace(0, 1, fade)
    audio[-fade:] *= np.linspace(1, 0, fade)
    return audio.astype(np.float32)


def _smooth_image(rng: np.random.Generator, h: int, w: int, cells: int = 12) -> np.ndarray:
    """Low-pass noise image uint8 (h,w,3): bilinear upsample of a coarse random
    grid plus a little fine grain, so bilinear resize / PSNR are meaningful."""
    gh, gw = cells + 1, cells * w // h + 2
    coarse = rng.uniform(0, 255, (gh, gw, 3))
    ys = np.linspace(0, gh - 1.001, h)
    xs = np.linspace(0, gw - 1.001, w)
    y0 = ys.astype(np.int64)
    x0 = xs.astype(np.int64)
    fy = (ys - y0)[:, None, None]
    fx = (xs - x0)[None, :, None]
    a = coarse[y0][:, x0]
    b = coarse[y0][:, x0 + 1]
    c = coarse[y0 + 1][:, x0]
    d = coarse[y0 + 1][:, x0 + 1]
    img = (a * (1 - fy) * (1 - fx) + b * (1 - fy) * fx + c * fy * (1 - fx) + d * fy * fx)
    img += rng.normal(0, 3.0, img.shape)
    return np.clip(np.rint(img), 0, 255).astype(np.uint8)


def wav2lip_avatar(n_frames: int = 8, full_hw: Tuple[int, int] = (720, 1280),
                   box: int = 320, seed: int = 0
                   ) -> Tuple[List[np.ndarray], List[np.ndarray], List[Tuple[int, int, int, int]]]:
    """(frame_list_cycle, face_list_cycle, coord_list_cycle) as `load_avatar`
    returns them (avatars/wav2lip_avatar.py:72-88): BGR uint8 full frames,
    BGR uint8 256x256 face crops, (y1,y2,x1,x2) int boxes that differ per frame
    (avatars/wav2lip/genavatar.py:118-130)."""
    rng = np.random.default_rng(seed)
    H, W_ = full_hw
    frames, faces, coords = [], [], []
    cy, cx = H // 2, W_ // 2
    for _ in range(n_frames):
        frames.append(_smooth_image(rng, H, W_))
        faces.append(_smooth_image(rng, 256, 256, cells=10))
        j = rng.integers(-4, 5, 4)
        y1 = int(cy - box // 2 + j[0]); y2 = int(cy + box // 2 + j[1])
        x1 = int(cx - box // 2 + j[2]); x2 = int(cx + box // 2 + j[3])
        coords.append((y1, y2, x1, x2))
    return frames, faces, coords


def _lerp_axis(a: np.ndarray, n_out: int, axis: int) -> np.ndarray:
    """Linear interpolation of fp32 `a` along `axis` at the sample positions `_smooth_image` uses: elementwise IEEE
    products and sums only (no BLAS), so the bytes are the same on every host."""
    n_in = a.shape[axis]
    pos = np.linspace(0, n_in - 1.001, n_out)
    i0 = pos.astype(np.int64)
    shape = [1] * a.ndim
    shape[axis] = n_out
    f = (pos - i0).astype(np.float32).reshape(shape)
    return np.take(a, i0, axis=axis) * (np.float32(1) - f) + np.take(a, i0 + 1, axis=axis) * f


def _smooth_image_fast(rng: np.random.Generator, h: int, w: int, grain: np.ndarray, cells: int = 12) -> np.ndarray:
    """`_smooth_image` for LARGE banks (the 250-frame 720p bench bank): the same coarse-grid bilinear
    field in fp32, separable, plus a fixed fine-grain field rolled by a per-frame offset (~10x faster per 720p frame).  A
    different pixel stream than `_smooth_image`: fixtures name the generator they used."""
    gh, gw = cells + 1, cells * w // h + 2
    coarse = rng.uniform(0, 255, (gh, gw, 3)).astype(np.float32)
    img = _lerp_axis(_lerp_axis(coarse, h, 0), w, 1)
    dy, dx = (int(v) for v in rng.integers(0, 64, 2))
    img += grain[dy:dy + h, dx:dx + w]
    return np.clip(np.rint(img), 0, 255).astype(np.uint8)


def wav2lip_bank(n_frames: int = 250, full_hw: Tuple[int, int] = (720, 1280), box: int = 320, seed: int = 0
                 ) -> Tuple[List[np.ndarray], List[np.ndarray], List[Tuple[int, int, int, int]]]:
    """The SURVEY.md 8d bench bank: `n_frames` smooth full frames + 256^2 face crops + jittered (y1,y2,x1,x2) boxes of
    about box^2 pixels (box 320: the paste-back upscales the 256^2 prediction, box 200: it shrinks it), in the layout
    `load_avatar` returns (avatars/wav2lip_avatar.py:72-88).  Same contract as `wav2lip_avatar`, ~15x faster per frame."""
    rng = np.random.default_rng([seed, n_frames, box])
    H, W_ = full_hw
    grain = rng.normal(0, 3.0, (H + 64, W_ + 64, 3)).astype(np.float32)
    frames, faces, coords = [], [], []
    cy, cx = H // 2, W_ // 2
    for _ in range(n_frames):
        frames.append(_smooth_image_fast(rng, H, W_, grain))
        faces.append(_smooth_image_fast(rng, 256, 256, grain, cells=10))
        j = rng.integers(-4, 5, 4)
        coords.append((int(cy - box // 2 + j[0]), int(cy + box // 2 + j[1]), int(cx - box // 2 + j[2]), int(cx + box // 2 + j[3])))
    return frames, faces, coords


# ---------------------------------------------------------------------------------------------------------
# MuseTalk: seeded state dicts under diffusers' key names (UNet2DConditionModel with the MuseTalk-1.5 config,
# AutoencoderKL decoder of sd-vae-ft-mse).  No checkpoint or config exists in the reference tree
# (avatars/musetalk/utils/utils.py:16-18 loads models/musetalkV15/{unet.pth,musetalk.json} at run time).
# ---------------------------------------------------------------------------------------------------------
UNET_CH = (320, 640, 1280, 1280)
UNET_CTX = 384
VAE_CH = (128, 256, 512, 512)


class _Shape:
    """Stand-in array for `shapes_only=True`: carries a shape through the generators' arithmetic without allocating."""

    def __init__(self, shape):
        self.shape = tuple(shape) if isinstance(shape, (tuple, list)) else (int(shape),)

    def __mul__(self, other):
        return self

    def astype(self, dtype):
        return self


class _ShapeRng:
    def standard_normal(self, shape, dtype=None):
        return _Shape(shape)

    def uniform(self, lo, hi, shape):
        return _Shape(shape)


def _finish(sd, shapes_only):
    return {k: tuple(v.shape) for k, v in sd.items()} if shapes_only else sd


def _w(rng, shape, fan_in, gain=1.0):
    return (rng.standard_normal(shape, dtype=np.float32) * np.float32(gain / np.sqrt(fan_in))).astype(np.float32)


def _norm(rng, sd, p, c):
    sd[p + ".weight"] = rng.uniform(0.8, 1.2, c).astype(np.float32)
    sd[p + ".bias"] = (rng.standard_normal(c) * 0.05).astype(np.float32)


def _conv(rng, sd, p, cin, cout, k, gain=1.0):
    sd[p + ".weight"] = _w(rng, (cout, cin, k, k), cin * k * k, gain)
    sd[p + ".bias"] = (rng.standard_normal(cout) * 0.02).astype(np.float32)


def _lin(rng, sd, p, cin, cout, bias=True, gain=1.0):
    sd[p + ".weight"] = _w(rng, (cout, cin), cin, gain)
    if bias:
        sd[p + ".bias"] = (rng.standard_normal(cout) * 0.02).astype(np.float32)


def _resnet(rng, sd, p, cin, cout, temb):
    _norm(rng, sd, p + ".norm1", cin)
    _conv(rng, sd, p + ".conv1", cin, cout, 3)
    if temb:
        _lin(rng, sd, p + ".time_emb_proj", temb, cout, gain=0.3)
    _norm(rng, sd, p + ".norm2", cout)
    _conv(rng, sd, p + ".conv2", cout, cout, 3, gain=0.5)
    if cin != cout:
        _conv(rng, sd, p + ".conv_shortcut", cin, cout, 1)


def _transformer(rng, sd, p, c, ctx):
    _norm(rng, sd, p + ".norm", c)
    _conv(rng, sd, p + ".proj_in", c, c, 1)
    b = p + ".transformer_blocks.0"
    for i, kv in ((1, c), (2, ctx)):
        _norm(rng, sd, b + f".norm{i}", c)
        _lin(rng, sd, b + f".attn{i}.to_q", c, c, bias=False, gain=1.5)
        _lin(rng, sd, b + f".attn{i}.to_k", kv, c, bias=False, gain=1.5)
        _lin(rng, sd, b + f".attn{i}.to_v", kv, c, bias=False)
        _lin(rng, sd, b + f".attn{i}.to_out.0", c, c, gain=0.5)
    _norm(rng, sd, b + ".norm3", c)
    _lin(rng, sd, b + ".ff.net.0.proj", c, 8 * c)
    _lin(rng, sd, b + ".ff.net.2", 4 * c, c, gain=0.5)
    _conv(rng, sd, p + ".proj_out", c, c, 1, gain=0.5)


def _gn_gain(sd, gain):
    """Parity-stress family: the affine of every ResnetBlock2D GroupNorm (norm1 / norm2) times `gain`.  GroupNorm renormalises
    whatever reaches it, so the network does not blow up: the tensors BETWEEN a norm and the next one (norm outputs, conv
    outputs, the residual stream) grow about linearly with the gain - fp32 peak |activation| U-Net / VAE decoder: 13 / 14 at gain 1,
    92 / 122 at 16, 1.5e3 / 1.9e3 at 256, 1.2e4 / 1.5e4 at 2048, past the fp16 limit at 16 384."""
    if gain == 1.0:
        return sd
    import re
    g = np.float32(gain)
    for k in list(sd):
        if re.search(r"resnets\.\d+\.norm[12]\.(weight|bias)$", k):
            sd[k] = sd[k] * g
    return sd


def musetalk_unet_state_dict(seed: int = 4321, shapes_only: bool = False, gn_gain: float = 1.0) -> Dict[str, np.ndarray]:
    rng = _ShapeRng() if shapes_only else np.random.default_rng(seed)
    sd: Dict[str, np.ndarray] = {}
    ch = UNET_CH
    _conv(rng, sd, "conv_in", 8, ch[0], 3)
    _lin(rng, sd, "time_embedding.linear_1", ch[0], 1280)
    _lin(rng, sd, "time_embedding.linear_2", 1280, 1280)
    cin = ch[0]
    skip_ch = [ch[0]]
    for i in range(4):
        for j in range(2):
            _resnet(rng, sd, f"down_blocks.{i}.resnets.{j}", cin, ch[i], 1280)
            cin = ch[i]
            if i < 3:
                _transformer(rng, sd, f"down_blocks.{i}.attentions.{j}", ch[i], UNET_CTX)
            skip_ch.append(cin)
        if i < 3:
            _conv(rng, sd, f"down_blocks.{i}.downsamplers.0.conv", cin, cin, 3)
            skip_ch.append(cin)
    _resnet(rng, sd, "mid_block.resnets.0", cin, cin, 1280)
    _transformer(rng, sd, "mid_block.attentions.0", cin, UNET_CTX)
    _resnet(rng, sd, "mid_block.resnets.1", cin, cin, 1280)
    rev = ch[::-1]
    for i in range(4):
        for j in range(3):
            sk = skip_ch.pop()
            _resnet(rng, sd, f"up_blocks.{i}.resnets.{j}", cin + sk, rev[i], 1280)
            cin = rev[i]
            if i > 0:
                _transformer(rng, sd, f"up_blocks.{i}.attentions.{j}", cin, UNET_CTX)
        if i < 3:
            _conv(rng, sd, f"up_blocks.{i}.upsamplers.0.conv", cin, cin, 3)
    _norm(rng, sd, "conv_norm_out", cin)
    _conv(rng, sd, "conv_out", cin, 4, 3, gain=0.5)
    if not shapes_only:
        _gn_gain(sd, gn_gain)
    return _finish(sd, shapes_only)


def vae_decoder_state_dict(seed: int = 987, shapes_only: bool = False, gn_gain: float = 1.0) -> Dict[str, np.ndarray]:
    rng = _ShapeRng() if shapes_only else np.random.default_rng(seed)
    sd: Dict[str, np.ndarray] = {}
    _conv(rng, sd, "post_quant_conv", 4, 4, 1)
    top = VAE_CH[-1]
    _conv(rng, sd, "decoder.conv_in", 4, top, 3)
    _resnet(rng, sd, "decoder.mid_block.resnets.0", top, top, 0)
    a = "decoder.mid_block.attentions.0"
    _norm(rng, sd, a + ".group_norm", top)
    for nme in ("to_q", "to_k", "to_v"):
        _lin(rng, sd, a + "." + nme, top, top, gain=1.5 if nme != "to_v" else 1.0)
    _lin(rng, sd, a + ".to_out.0", top, top, gain=0.5)
    _resnet(rng, sd, "decoder.mid_block.resnets.1", top, top, 0)
    cin = top
    for i, c in enumerate(VAE_CH[::-1]):
        for j in range(3):
            _resnet(rng, sd, f"decoder.up_blocks.{i}.resnets.{j}", cin, c, 0)
            cin = c
        if i < 3:
            _conv(rng, sd, f"decoder.up_blocks.{i}.upsamplers.0.conv", cin, cin, 3)
    _norm(rng, sd, "decoder.conv_norm_out", cin)
    _conv(rng, sd, "decoder.conv_out", cin, 3, 3, gain=0.7)
    if not shapes_only:
        _gn_gain(sd, gn_gain)
    return _finish(sd, shapes_only)


def vae_encoder_state_dict(seed: int = 654, shapes_only: bool = False) -> Dict[str, np.ndarray]:
    """AutoencoderKL (sd-vae) encoder + quant_conv under diffusers' key names."""
    rng = _ShapeRng() if shapes_only else np.random.default_rng(seed)
    sd: Dict[str, np.ndarray] = {}
    _conv(rng, sd, "encoder.conv_in", 3, VAE_CH[0], 3)
    cin = VAE_CH[0]
    for i, c in enumerate(VAE_CH):
        for j in range(2):
            _resnet(rng, sd, f"encoder.down_blocks.{i}.resnets.{j}", cin, c, 0)
            cin = c
        if i < 3:
            _conv(rng, sd, f"encoder.down_blocks.{i}.downsamplers.0.conv", cin, cin, 3)
    _resnet(rng, sd, "encoder.mid_block.resnets.0", cin, cin, 0)
    a = "encoder.mid_block.attentions.0"
    _norm(rng, sd, a + ".group_norm", cin)
    for nme in ("to_q", "to_k", "to_v"):
        _lin(rng, sd, a + "." + nme, cin, cin, gain=1.5 if nme != "to_v" else 1.0)
    _lin(rng, sd, a + ".to_out.0", cin, cin, gain=0.5)
    _resnet(rng, sd, "encoder.mid_block.resnets.1", cin, cin, 0)
    _norm(rng, sd, "encoder.conv_norm_out", cin)
    _conv(rng, sd, "encoder.conv_out", cin, 8, 3, gain=0.7)
    _conv(rng, sd, "quant_conv", 8, 8, 1)
    return _finish(sd, shapes_only)


def musetalk_latents(n_frames: int = 4, seed: int = 5) -> List[np.ndarray]:
    """input_latent_list_cycle stand-in: per frame fp32 (1,8,32,32) = cat(masked, reference) VAE latents scaled by
    0.18215 (avatars/musetalk/models/vae.py:110-122)."""
    rng = np.random.default_rng(seed)
    return [(rng.standard_normal((1, 8, 32, 32)) * 0.18215 * 4).astype(np.float32) for _ in range(n_frames)]


def _soft_mask(h: int, w: int, blur: int) -> np.ndarray:
    """A lower-half box, box-blurred twice (the shape of the Gaussian-blurred masks genavatar writes,
    avatars/musetalk/utils/blending.py:129-135), stored grey as cv2.imread returns a grey PNG: (h,w,3) uint8, B = G = R."""
    m = np.zeros((h, w), np.float64)
    m[h // 2:, w // 8: w - w // 8] = 255.0
    k = np.ones(blur) / blur
    for _ in range(2):
        m = np.apply_along_axis(lambda r: np.convolve(r, k, mode="same"), 1, m)
        m = np.apply_along_axis(lambda c: np.convolve(c, k, mode="same"), 0, m)
    m8 = np.clip(np.rint(m), 0, 255).astype(np.uint8)
    return np.repeat(m8[:, :, None], 3, axis=2)


def musetalk_blend_avatar(full_hw: Tuple[int, int] = (360, 640), seed: int = 9):
    """Four frames for the MuseTalk composite (avatars/musetalk_avatar.py:154-164, myutil.py:4-25), one per case the
    composite has: 0 soft mask on a growing face box (300 px wide > 256), 1 a crop box touching the frame's left and
    bottom edges, 2 a shrinking face box (150 x 170 < 256), 3 a growing, non-square box with a hard-edged (0 / 255) mask.
    Returns (frames, masks, face_boxes (x1,y1,x2,y2), crop_boxes (x_s,y_s,x_e,y_e), preds uint8 (4,256,256,3))."""
    H, W = full_hw
    rng = np.random.default_rng(seed)
    frames = [np.ascontiguousarray(_smooth_image(rng, H, W)) for _ in range(4)]
    face_boxes = [(170, 30, 470, 330), (20, H - 230, 200, H - 30), (250, 100, 400, 270), (180, 20, 460, 340)]
    crop_boxes = [(140, 10, 500, H - 5), (0, H - 260, 230, H), (220, 60, 440, 320), (150, 5, 490, H - 2)]
    masks = []
    for i, (xs, ys, xe, ye) in enumerate(crop_boxes):
        m = _soft_mask(ye - ys, xe - xs, 15 if i != 1 else 9)
        if i == 3:
            m = np.where(m >= 128, 255, 0).astype(np.uint8)
        masks.append(m)
    preds = np.ascontiguousarray(np.stack([_smooth_image(rng, 256, 256, cells=6) for _ in range(4)]))     # C order: the device reads raw bytes
    return frames, masks, face_boxes, crop_boxes, preds


def musetalk_whisper_feats(batch: int, seed: int = 11) -> np.ndarray:
    """(B,50,384) audio feature stand-in with the value range of Whisper encoder states."""
    rng = np.random.default_rng(seed)
    return rng.standard_normal((batch, 50, 384)).astype(np.float32)


def whisper_encoder_state_dict(seed: int = 2468) -> Dict[str, np.ndarray]:
    """whisper-tiny ENCODER stand-in under transformers' key names (WhisperModel(...).encoder.state_dict()): d_model 384,
    6 heads, 4 layers, ffn 1536, 1500 positions (avatars/musetalk/whisper/audio2feature.py:15-23 loads the real one)."""
    rng = np.random.default_rng(seed)
    sd: Dict[str, np.ndarray] = {}
    D, FF = 384, 1536
    sd["conv1.weight"] = _w(rng, (D, 80, 3), 80 * 3)
    sd["conv1.bias"] = (rng.standard_normal(D) * 0.02).astype(np.float32)
    sd["conv2.weight"] = _w(rng, (D, D, 3), D * 3)
    sd["conv2.bias"] = (rng.standard_normal(D) * 0.02).astype(np.float32)
    pos = np.arange(1500)[:, None] * np.exp(-np.log(10000.0) / (D // 2 - 1) * np.arange(D // 2))[None, :]
    sd["embed_positions.weight"] = np.concatenate([np.sin(pos), np.cos(pos)], axis=1).astype(np.float32)
    for l in range(4):
        p = f"layers.{l}"
        for name in ("q_proj", "k_proj", "v_proj", "out_proj"):
            sd[f"{p}.self_attn.{name}.weight"] = _w(rng, (D, D), D, gain=0.7)
            if name != "k_proj":
                sd[f"{p}.self_attn.{name}.bias"] = (rng.standard_normal(D) * 0.02).astype(np.float32)
        for ln in ("self_attn_layer_norm", "final_layer_norm"):
            sd[f"{p}.{ln}.weight"] = (1.0 + 0.1 * rng.standard_normal(D)).astype(np.float32)
            sd[f"{p}.{ln}.bias"] = (0.05 * rng.standard_normal(D)).astype(np.float32)
        sd[f"{p}.fc1.weight"] = _w(rng, (FF, D), D)
        sd[f"{p}.fc1.bias"] = (rng.standard_normal(FF) * 0.02).astype(np.float32)
        sd[f"{p}.fc2.weight"] = _w(rng, (D, FF), FF, gain=0.7)
        sd[f"{p}.fc2.bias"] = (rng.standard_normal(D) * 0.02).astype(np.float32)
    sd["layer_norm.weight"] = (1.0 + 0.1 * rng.standard_normal(D)).astype(np.float32)
    sd["layer_norm.bias"] = (0.05 * rng.standard_normal(D)).astype(np.float32)
    return sd


# ------------------------------------------------------------------------------------------------ Ultralight
def _ul_blocks():
    """(prefix, kind, cin, cout, residual) in the registration order of avatars/ultralight/unet.py Model(6, 'hubert')
    (unet.py:168-196): kind "ir" = InvertedResidual with expand_ratio 2 (unet.py:7-36), "conv" = biased dense 3x3 conv +
    BatchNorm of the audio tower (prefix = (conv name, bn name))."""
    out = []

    def dconv(p, cin, cout):                     # DoubleConvDW, unet.py:38-49
        out.append((p + ".double_conv.0", "ir", cin, cout, False))
        out.append((p + ".double_conv.1", "ir", cout, cout, True))

    a = "audio_model."                           # AudioConvHubert, unet.py:132-150
    out.append((a + "conv1", "ir", 16, 64, False))
    out.append((a + "conv2", "ir", 64, 128, False))
    out.append(((a + "conv3", a + "bn3"), "conv", 128, 256, False))
    out.append((a + "conv4", "ir", 256, 256, True))
    out.append(((a + "conv5", a + "bn5"), "conv", 256, 512, False))
    out.append((a + "conv6", "ir", 512, 512, True))
    out.append((a + "conv7", "ir", 512, 512, True))
    dconv("fuse_conv.0", 1024, 512)
    dconv("fuse_conv.1", 512, 256)
    out.append(("inc.inconv.0", "ir", 6, 32, False))
    for i, (ci, co) in enumerate(((32, 64), (64, 128), (128, 256), (256, 512)), 1):
        dconv(f"down{i}.maxpool_conv.0", ci, co)
    for i, (ci, co) in enumerate(((512, 128), (256, 64), (128, 32), (64, 32)), 1):
        dconv(f"up{i}.conv", ci, co)
    return out


def ultralight_state_dict(seed: int = 1234) -> Dict[str, np.ndarray]:
    """Reference-named fp32 state_dict of avatars/ultralight/unet.py Model(6, 'hubert') as numpy arrays (484 tensors).

    Fixed BatchNorm statistics, as wav2lip_state_dict draws them (a data-calibrated draw gives dead channels a gain of
    1/sqrt(eps) and makes the random network amplify rounding ~1000x): conv std sqrt(2/fan_in) where a ReLU follows,
    sqrt(1/fan_in) for the linear project conv (depthwise fan_in = 9); gamma U(0.7, 1.3), U(0.3, 0.7) on the last
    BatchNorm of a residual block; beta 0.1 N, running_mean 0.2 N, running_var U(0.6, 1.6); audio conv biases 0.05 N;
    outc weight 0.4 N, bias 0.2 N."""
    rng = np.random.default_rng(seed)
    sd: Dict[str, np.ndarray] = {}

    def bn(p, c, damp=False):
        lo, hi = (0.3, 0.7) if damp else (0.7, 1.3)
        sd[p + ".weight"] = rng.uniform(lo, hi, c).astype(np.float32)
        sd[p + ".bias"] = (rng.standard_normal(c) * 0.1).astype(np.float32)
        sd[p + ".running_mean"] = (rng.standard_normal(c) * 0.2).astype(np.float32)
        sd[p + ".running_var"] = rng.uniform(0.6, 1.6, c).astype(np.float32)
        sd[p + ".num_batches_tracked"] = np.asarray(1000, dtype=np.int64)

    def w(shape, fan_in, relu):
        return (rng.standard_normal(shape) * np.sqrt((2.0 if relu else 1.0) / fan_in)).astype(np.float32)

    for prefix, kind, cin, cout, residual in _ul_blocks():
        if kind == "ir":
            mid = 2 * cin
            sd[prefix + ".conv.0.weight"] = w((mid, cin, 1, 1), cin, True)
            bn(prefix + ".conv.1", mid)
            sd[prefix + ".conv.3.weight"] = w((mid, 1, 3, 3), 9, True)
            bn(prefix + ".conv.4", mid)
            sd[prefix + ".conv.6.weight"] = w((cout, mid, 1, 1), mid, False)
            bn(prefix + ".conv.7", cout, damp=residual)
        else:
            conv, norm = prefix
            sd[conv + ".weight"] = w((cout, cin, 3, 3), cin * 9, True)
            sd[conv + ".bias"] = (rng.standard_normal(cout) * 0.05).astype(np.float32)
            bn(norm, cout)
    sd["outc.conv.weight"] = (rng.standard_normal((3, 32, 1, 1)) * 0.4).astype(np.float32)
    sd["outc.conv.bias"] = (rng.standard_normal(3) * 0.2).astype(np.float32)
    return sd


def ultralight_avatar(n_frames: int = 4, full_hw: Tuple[int, int] = (360, 640), seed: int = 3
                      ) -> Tuple[List[np.ndarray], List[np.ndarray], List[Tuple[int, int, int, int]]]:
    """(frame_list_cycle, face_list_cycle, coord_list_cycle) as avatars/ultralight_avatar.py:63-81 load_avatar returns them:
    BGR uint8 full frames, BGR uint8 168x168 face crops, (x1, y1, x2, y2) boxes that differ per frame."""
    rng = np.random.default_rng(seed)
    H, W_ = full_hw
    frames, faces, coords = [], [], []
    cy, cx = H // 2, W_ // 2
    box = min(H, W_) // 2
    for _ in range(n_frames):
        frames.append(_smooth_image(rng, H, W_))
        faces.append(_smooth_image(rng, 168, 168, cells=8))
        j = rng.integers(-4, 5, 4)
        x1 = int(cx - box // 2 + j[0]); x2 = int(cx + box // 2 + j[1])
        y1 = int(cy - box // 2 + j[2]); y2 = int(cy + box // 2 + j[3])
        coords.append((x1, y1, x2, y2))
    return frames, faces, coords


def ultralight_feats(batch: int, seed: int = 21) -> np.ndarray:
    """Stand-in HuBERT chunks: float32 (batch, 16, 1024), unit variance (layer-normed hidden states)."""
    return np.random.default_rng(seed).standard_normal((batch, 16, 1024)).astype(np.float32)


def ultralight_faces(batch: int, seed: int = 1234) -> List[np.ndarray]:
    """The 168x168 BGR uint8 bank faces ultralight_inputs builds its images from."""
    rng = np.random.default_rng(seed + 77)
    return [_smooth_image(rng, 168, 168, cells=8) for _ in range(batch)]


def ultralight_inputs(batch: int, seed: int = 1234):
    """(img6 float32 (batch, 6, 160, 160), feat float32 (batch, 16, 32, 32)) as LightReal.inference_batch builds them
    (avatars/ultralight_avatar.py:150-166) from ultralight_faces(batch, seed): reference crop, masked crop, / 255, BGR.
    The first k items of a longer draw equal the draw of k items."""
    imgs = []
    for face in ultralight_faces(batch, seed):
        real = face[4:164, 4:164].copy()
        masked = real.copy()
        masked[5:150, 5:155] = 0                    # cv2.rectangle(img, (5, 5, 150, 145), 0, -1): x 5..154, y 5..149
        imgs.append(np.concatenate([real.transpose(2, 0, 1), masked.transpose(2, 0, 1)]).astype(np.float32) / np.float32(255.0))
    return np.stack(imgs), ultralight_feats(batch, seed + 78).reshape(batch, 16, 32, 32)


# ---------------------------------------------------------------------------------------------- BiSeNet face parser
def _fp_convs():
    """(conv key, BatchNorm key or None, cin, cout, k, a ReLU follows, last BatchNorm of a residual block) of BiSeNet's main output path
    (avatars/musetalk/utils/face_parsing/model.py, resnet.py), in state_dict order."""
    out = [("cp.resnet.conv1", "cp.resnet.bn1", 3, 64, 7, True, False)]
    cin = 64
    for l, c in enumerate((64, 128, 256, 512)):
        for b in range(2):
            p = f"cp.resnet.layer{l + 1}.{b}"
            out.append((p + ".conv1", p + ".bn1", cin if b == 0 else c, c, 3, True, False))
            out.append((p + ".conv2", p + ".bn2", c, c, 3, False, True))
            if b == 0 and l > 0:
                out.append((p + ".downsample.0", p + ".downsample.1", cin, c, 1, False, False))
        cin = c
    for p, ci in (("cp.arm16", 256), ("cp.arm32", 512)):
        out.append((p + ".conv.conv", p + ".conv.bn", ci, 128, 3, True, False))
        out.append((p + ".conv_atten", p + ".bn_atten", 128, 128, 1, False, False))
    out += [("cp.conv_head32.conv", "cp.conv_head32.bn", 128, 128, 3, True, False), ("cp.conv_head16.conv", "cp.conv_head16.bn", 128, 128, 3, True, False),
            ("cp.conv_avg.conv", "cp.conv_avg.bn", 512, 128, 1, True, False), ("ffm.convblk.conv", "ffm.convblk.bn", 256, 256, 1, True, False),
            ("ffm.conv1", None, 256, 64, 1, True, False), ("ffm.conv2", None, 64, 256, 1, False, False),
            ("conv_out.conv.conv", "conv_out.conv.bn", 256, 256, 3, True, False), ("conv_out.conv_out", None, 256, 19, 1, False, False)]
    return out


FACEPARSE_CLASS_GAIN = (1.0, 1.0, 1.0, 1.5, 1.562, 1.562, 1.0, 1.562, 0.64, 1.562, 1.103, 1.562, 1.562, 0.809, 1.278, 1.562, 1.562, 1.562, 1.562)


def faceparse_state_dict(seed: int = 83, shapes_only: bool = False, heads: bool = True) -> Dict[str, np.ndarray]:
    """Reference-named fp32 state_dict of face_parsing's BiSeNet(n_classes=19) as numpy arrays: He-scaled convs (std sqrt(2 / fan_in) in
    front of a ReLU, sqrt(1 / fan_in) otherwise), BatchNorm as ultralight_state_dict draws it (gamma damped on the last BatchNorm of a
    residual block), conv_out.conv_out with zero-sum rows and per-class gains so that the classes the mask modes use win.  `heads`: also the conv_out16 / conv_out32
    heads, which net(img)[0] does not use."""
    rng = np.random.default_rng(seed)
    sd: Dict[str, np.ndarray] = {}

    def bn(p, c, damp):
        lo, hi = (0.3, 0.7) if damp else (0.7, 1.3)
        sd[p + ".weight"] = rng.uniform(lo, hi, c).astype(np.float32)
        sd[p + ".bias"] = (rng.standard_normal(c) * 0.1).astype(np.float32)
        sd[p + ".running_mean"] = (rng.standard_normal(c) * 0.2).astype(np.float32)
        sd[p + ".running_var"] = rng.uniform(0.6, 1.6, c).astype(np.float32)
        sd[p + ".num_batches_tracked"] = np.asarray(1000, dtype=np.int64)

    for conv, norm, cin, cout, k, relu, damp in _fp_convs():
        sd[conv + ".weight"] = (rng.standard_normal((cout, cin, k, k)) * np.sqrt((2.0 if relu else 1.0) / (cin * k * k))).astype(np.float32)
        if norm:
            bn(norm, cout, damp)
    # every class's weights sum to zero: the features behind a ReLU are all positive, and their common mean times a row's sum would
    # decide the argmax for the whole image (one class won 98 % of the pixels).  Then the per-class gains FACEPARSE_CLASS_GAIN, fitted
    # once on seed 83 / faceparse_image(512, 0) so that no row takes the image, and rows 1 <-> 4 and 12 <-> 8 change places: classes
    # 1, 10, 11, 12 and 13 - the ones the mask modes keep - each win 10 % or more of that image (scripts/gen_golden_faceparse.py asserts 2 %).
    w = sd["conv_out.conv_out.weight"]
    w = (w - w.mean(1, keepdims=True)) * np.asarray(FACEPARSE_CLASS_GAIN, np.float32).reshape(19, 1, 1, 1)
    w[[1, 4, 12, 8]] = w[[4, 1, 8, 12]]
    sd["conv_out.conv_out.weight"] = np.ascontiguousarray(w, dtype=np.float32)
    if heads:
        for p in ("conv_out16", "conv_out32"):
            sd[p + ".conv.conv.weight"] = (rng.standard_normal((64, 128, 3, 3)) * np.sqrt(2.0 / 1152)).astype(np.float32)
            bn(p + ".conv.bn", 64, False)
            sd[p + ".conv_out.weight"] = (rng.standard_normal((19, 64, 1, 1)) * np.sqrt(1.0 / 64)).astype(np.float32)
    return _finish(sd, shapes_only)


def faceparse_image(size: int = 512, seed: int = 0) -> np.ndarray:
    """A smooth low-pass RGB uint8 image (size, size, 3)."""
    rng = np.random.default_rng(9000 + seed)
    return _smooth_image(rng, size, size)


# ---------------------------------------------------------------------------------------------- S3FD face detector
S3FD_TRUNK = (("conv1_1", 3, 64, 3), ("conv1_2", 64, 64, 3), ("conv2_1", 64, 128, 3), ("conv2_2", 128, 128, 3), ("conv3_1", 128, 256, 3),
              ("conv3_2", 256, 256, 3), ("conv3_3", 256, 256, 3), ("conv4_1", 256, 512, 3), ("conv4_2", 512, 512, 3), ("conv4_3", 512, 512, 3),
              ("conv5_1", 512, 512, 3), ("conv5_2", 512, 512, 3), ("conv5_3", 512, 512, 3), ("fc6", 512, 1024, 3), ("fc7", 1024, 1024, 1),
              ("conv6_1", 1024, 256, 1), ("conv6_2", 256, 512, 3), ("conv7_1", 512, 128, 1), ("conv7_2", 128, 256, 3))
S3FD_NORMS = (("conv3_3_norm", 256, 10.0), ("conv4_3_norm", 512, 8.0), ("conv5_3_norm", 512, 5.0))
S3FD_HEADS = (("conv3_3_norm_mbox", 256, 4), ("conv4_3_norm_mbox", 512, 2), ("conv5_3_norm_mbox", 512, 2), ("fc7_mbox", 1024, 2),
              ("conv6_2_mbox", 512, 2), ("conv7_2_mbox", 256, 2))
# per level, fitted once on seed 29 / s3fd_frame(64, 64, 0..7): the gain on the head's conf rows sets the spread of the (face - background)
# logit over a map, the shift (half on the face bias, half against the background's) its mean: 1.2 around -5.0 at level 0, 0.7 around
# -1.1 at the others.  Almost every position of levels 1..5 then scores above the 0.05 threshold, far from it (a score's fp16 error
# cannot move it across), a few percent of them above 0.5, and level 0 with its 16 x more positions adds a handful
S3FD_CONF_GAIN = (3.0, 1.6, 3.4, 1.3, 2.3, 3.4)
S3FD_FACE_BIAS = (-6.2, -1.3, -0.5, -0.8, -0.7, -1.2)


def s3fd_state_dict(seed: int = 29, shapes_only: bool = False) -> Dict[str, np.ndarray]:
    """Reference-named fp32 state_dict of face_detection's s3fd() (detection/sfd/net_s3fd.py) as numpy arrays, in the module's key
    order: fan-in scaled convs like `_conv` (gain sqrt 2 in the trunk, where a ReLU follows every conv), L2Norm weights around their
    scales (10, 8, 5), and heads whose conf rows carry S3FD_CONF_GAIN and whose face logit carries S3FD_FACE_BIAS, so that the float64
    network on s3fd_frame gives a usable score distribution (scripts/gen_golden_s3fd.py asserts it)."""
    rng = np.random.default_rng(seed)
    sd: Dict[str, np.ndarray] = {}
    for name, cin, cout, k in S3FD_TRUNK:
        # conv1_1 sees mean-subtracted bytes (rms about 64): its gain brings the trunk to unit scale
        _conv(rng, sd, name, cin, cout, k, gain=float(np.sqrt(2.0)) / (64.0 if name == "conv1_1" else 1.0))
    for name, c, scale in S3FD_NORMS:
        sd[name + ".weight"] = (scale * rng.uniform(0.9, 1.1, c)).astype(np.float32)
    for (name, cin, nconf), gain, bias in zip(S3FD_HEADS, S3FD_CONF_GAIN, S3FD_FACE_BIAS):
        _conv(rng, sd, name + "_conf", cin, nconf, 3, gain=gain)
        # zero-sum rows: the features are all positive, and their common mean times a row's sum would move every logit of the map by
        # the same large amount - fp16 would then round the logits more coarsely than their difference, which is all the softmax reads
        w = sd[name + "_conf.weight"]
        sd[name + "_conf.weight"] = np.ascontiguousarray(w - w.mean(axis=(1, 2, 3), keepdims=True), dtype=np.float32)
        sd[name + "_conf.bias"][:-1] -= np.float32(bias / 2)
        sd[name + "_conf.bias"][-1] += np.float32(bias / 2)
        _conv(rng, sd, name + "_loc", cin, 4, 3)
    return _finish(sd, shapes_only)


def s3fd_frame(H: int = 64, W: int = 64, seed: int = 0) -> np.ndarray:
    """A smooth low-pass BGR uint8 frame (H, W, 3), as cv2.imread would hand it over."""
    rng = np.random.default_rng(9500 + seed)
    return np.ascontiguousarray(_smooth_image(rng, H, W, cells=6)[..., ::-1])
