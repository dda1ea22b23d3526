"""The op-by-op replay (oracle/op_replay.py) shown to bite, without a GPU.

A SIMULATED device - the float32 oracle with fp16 weights whose every op output is rounded to fp16 - stands in for the program:
  * it passes every gate, U-Net + VAE decoder at B = 1 with the default program's fusions (LayerNorms, GEGLU projection not
    materialised), and the rounding model alone stays inside half the bound for every op (0 violators, max |mod - ref| / tol <= 0.5);
  * six faults planted into it are each found, and the failure names the faulty op and no other;
  * the coverage walk fails when a name is missing from the compared set;
  * the Ultralight program (tests/ultralight_ref.py, 86 ops) the same way at B = 1 and B = 2, with eight planted faults (bottom of the file).
Measured (synthetic draw of synth_inputs): largest |mod - ref| / tol over the 422 ops of the full pass 0.42 (gate 0.5), the bound is
0.3 % of the output's rms (median over ops).  The tanh-GELU fault (e), the subtle one, passes the aggregate gate (rel_l2 2.9e-4
against the model's 2.1e-4) and is caught per element: 40 259 of 655 360 elements outside the bound, worst |dev - ref| / tol 102.
"""
import math

import numpy as np
import pytest

torch = pytest.importorskip("torch")
import torch.nn.functional as F  # noqa: E402

import synth_inputs as synth  # noqa: E402
from oracle import musetalk_oracle as M  # noqa: E402
from oracle import op_replay as R  # noqa: E402


@pytest.fixture(scope="module")
def weights():
    usd = {k: torch.from_numpy(v) for k, v in synth.musetalk_unet_state_dict().items()}
    vsd = {k: torch.from_numpy(v) for k, v in synth.vae_decoder_state_dict().items()}
    return usd, vsd


def _ctx(B):
    return R.f16(M.positional_encoding(torch.from_numpy(synth.musetalk_whisper_feats(B))))


def _ops_of(names, fused):
    """An op list as Engine.musetalk_ops() gives it, from the tensors of a (simulated) pass."""
    ops = [(n[:-len(".attn")], 3) if n.endswith(".attn") else (n, 0) for n in names]
    return ops + [(n, 2) for n in fused]


def test_simulated_device_passes_every_gate_and_the_model_sits_inside_the_bound(weights):
    usd, vsd = weights
    fused = [k for k in R.fused_into() if k != "attn2.v_transpose_all"]
    lat = R.f16(torch.from_numpy(np.concatenate(synth.musetalk_latents(1))))
    ctx = _ctx(1)
    sim = R.SimDevice(fused)
    sim.t["latent_in"] = lat
    sim.t["encoder_hidden_states"] = ctx.transpose(1, 2)[..., None].contiguous()
    with torch.no_grad():
        out = M.unet_forward(R.half_weights(usd), lat, ctx, force=sim)
        M.vae_decode(R.half_weights(vsd), out / M.VAE_SCALING, force=sim)
    rp = R.replay_musetalk(usd, vsd, sim.fetch)
    worst = max(rp.records, key=lambda r: r["mod_over_tol"])
    print(f"[op replay] {len(rp.records)} ops compared; largest |mod - ref| / tol {worst['mod_over_tol']:.2f} ({worst['name']}); "
          f"bound / rms of the output, median over ops {np.median([r['tol_over_rms'] for r in rp.records]):.4f}")
    assert len(rp.records) >= 400
    bad = R.failures(rp.records, model_too=True)
    assert not bad, "\n".join(bad)
    # coverage: everything the pass produced is covered; one name less in the compared set and the walk says which
    compared = [r["name"] for r in rp.records]
    ops = _ops_of([n for n in sim.t if n not in ("latent_in", "encoder_hidden_states")], fused)
    assert R.uncovered(ops, compared, R.fused_into()) == []
    for gone in ("decoder.up_blocks.1.upsamplers.0.conv", "mid_block.attentions.0.transformer_blocks.0.attn1.attn",
                 "down_blocks.2.attentions.1.transformer_blocks.0.ff.geglu"):
        miss = R.uncovered(ops, [n for n in compared if n != gone], R.fused_into())
        want = {gone[:-len(".attn")] if gone.endswith(".attn") else gone}
        if gone.endswith(".ff.geglu"):          # the group output stands for the ops fused into it
            want |= {gone[:-len(".ff.geglu")] + s for s in (".norm3", ".ff.net.0.proj")}
        assert set(miss) == want, (gone, miss)
    # a fused op that FUSED_INTO does not list is an error, not a silent skip
    with pytest.raises(KeyError):
        R.Replay({}, lambda name, ref: None)("down_blocks.0.resnets.0.conv1", torch.zeros(1))


# ------------------------------------------------------------------------------------------------ planted faults
TB = "down_blocks.0.attentions.0"          # C = 320: heads of 40 channels (padded to 48 on the device)
BLK = TB + ".transformer_blocks.0"


def _transformer_failures(usd, mutate):
    sd = {k: v for k, v in usd.items() if k.startswith(TB + ".")}
    g = torch.Generator().manual_seed(5)
    x = R.f16(torch.randn(2, 320, 16, 16, generator=g))
    ctx = _ctx(2)
    sim = R.SimDevice(mutate=mutate)
    with torch.no_grad():
        M.transformer2d(R.half_weights(sd), TB, x, ctx, force=sim)
        rp = R.Replay(sd, sim.fetch)
        M.transformer2d({k: v.double() for k, v in sd.items()}, TB, x.double(), ctx.double(), force=rp)
    assert len(rp.records) == 19
    return R.failures(rp.records, model_too=True), {r["name"]: r for r in rp.records}


def _only(bad, name):
    assert len(bad) == 1 and bad[0].startswith(name + ": "), "\n".join(bad) or "nothing failed"


def test_unmutated_block_passes(weights):
    bad, _ = _transformer_failures(weights[0], None)
    assert not bad, "\n".join(bad)


def test_fault_a_last_query_tile_taken_from_the_previous_one(weights):
    def f(t, op):                          # (B, C, H, W), tokens row-major: the last 32 queries = the last two rows of 16
        t = t.clone()
        t[:, :, 14:16] = t[:, :, 12:14]
        return t
    bad, _ = _transformer_failures(weights[0], {BLK + ".attn1.attn": f})
    _only(bad, BLK + ".attn1.attn")


def test_fault_c_one_heads_channel_block_shifted_by_one_head(weights):
    def f(t, op):
        t = t.clone()
        t[:, 120:160] = t[:, 80:120]
        return t
    bad, _ = _transformer_failures(weights[0], {BLK + ".attn2.attn": f})
    _only(bad, BLK + ".attn2.attn")


def test_fault_d_layernorm_mean_over_c_plus_one(weights):
    usd = weights[0]

    def f(t, op):
        x = op["x"]
        C = x.shape[-1]
        mean = x.sum(-1, keepdim=True) / (C + 1)
        y = (x - mean) * torch.rsqrt(x.var(-1, unbiased=False, keepdim=True) + M.LN_EPS) * usd[BLK + ".norm2.weight"] + usd[BLK + ".norm2.bias"]
        return y.reshape(t.shape[0], t.shape[2], t.shape[3], C).permute(0, 3, 1, 2)
    bad, _ = _transformer_failures(usd, {BLK + ".norm2": f})
    _only(bad, BLK + ".norm2")


def test_fault_e_geglu_with_the_tanh_gelu(weights):
    def f(t, op):
        a, g = op["x"].chunk(2, dim=-1)
        y = a * F.gelu(g, approximate="tanh")
        return y.reshape(t.shape[0], t.shape[2], t.shape[3], -1).permute(0, 3, 1, 2)
    bad, rec = _transformer_failures(weights[0], {BLK + ".ff.geglu": f})
    r = rec[BLK + ".ff.geglu"]
    print(f"[op replay] tanh-GELU in the GEGLU: {r['violators']} of {r['n']} elements outside the bound, worst |dev - ref| / tol "
          f"{r['dev_over_tol']:.1f}; rel_l2 {r['rel_dev']:.3e} against the model's {r['rel_mod']:.3e}")
    _only(bad, BLK + ".ff.geglu")


def _vae_failures(vsd, sd_sim, mutate):
    """decoder.up_blocks.3.resnets.1 (128 -> 128, 3x3 convs) on a 32 x 32 map, then decoder.up_blocks.2.upsamplers.0.conv (256) 16 -> 32."""
    rn, up = "decoder.up_blocks.3.resnets.1", "decoder.up_blocks.2.upsamplers.0.conv"
    sd = {k: v for k, v in vsd.items() if k.startswith(rn + ".") or k.startswith(up + ".")}
    g = torch.Generator().manual_seed(6)
    x = R.f16(torch.randn(2, 128, 32, 32, generator=g))
    u = R.f16(torch.randn(2, 256, 16, 16, generator=g))
    sim = R.SimDevice(mutate=mutate)
    sd16 = R.half_weights(sd)
    sd16.update(sd_sim or {})
    with torch.no_grad():
        M.resnet(sd16, rn, x, None, M.VAE_GROUPS, M.VAE_EPS, force=sim)
        M.upsample_conv(sd16, up, u, force=sim)
        rp = R.Replay(sd, sim.fetch)
        sd64 = {k: v.double() for k, v in sd.items()}
        M.resnet(sd64, rn, x.double(), None, M.VAE_GROUPS, M.VAE_EPS, force=rp)
        M.upsample_conv(sd64, up, u.double(), force=rp)
    assert len(rp.records) == 5
    return R.failures(rp.records, model_too=True)


def test_fault_b_one_of_nine_taps_of_a_vae_conv_dropped(weights):
    vsd = weights[1]
    assert not _vae_failures(vsd, None, None)
    w = R.f16(vsd["decoder.up_blocks.3.resnets.1.conv1.weight"]).clone()
    w[:, :, 0, 2] = 0
    _only(_vae_failures(vsd, {"decoder.up_blocks.3.resnets.1.conv1.weight": w}, None), "decoder.up_blocks.3.resnets.1.conv1")


def test_fault_f_last_column_of_an_upsampler_output_zeroed_on_one_image(weights):
    def f(t, op):
        t = t.clone()
        t[1, :, :, -1] = 0
        return t
    up = "decoder.up_blocks.2.upsamplers.0.conv"
    _only(_vae_failures(weights[1], None, {up: f}), up)


def test_float64_conv_path_equals_torch():
    g = torch.Generator().manual_seed(1)
    x = torch.randn(2, 5, 9, 8, generator=g, dtype=torch.float64)
    for k, st, pad in ((3, 1, 1), (3, 2, 1), (1, 1, 0), (3, 2, 0)):
        w = torch.randn(7, 5, k, k, generator=g, dtype=torch.float64)
        b = torch.randn(7, generator=g, dtype=torch.float64)
        a = M.conv2d_f64(x, w, b, st, pad)
        r = F.conv2d(x, w, b, stride=st, padding=pad)
        assert a.shape == r.shape and float((a - r).abs().max()) <= 1e-12 * math.sqrt(5 * k * k) * float(r.abs().max())


# ------------------------------------------------------------------------------------------------ Wav2Lip
class _SimW2L:
    """The float32 Wav2Lip oracle with every layer rounded to fp16 (the head stays fp32, as on the device)."""

    def __init__(self, mutate=None):
        self.t, self.ops, self.mutate = {}, {}, mutate or {}

    def describe(self, name, op):
        self.ops[name] = op

    def __call__(self, name, t):
        op = self.ops.pop(name, None)
        if name in self.mutate:
            t = self.mutate[name](t, op)
        t = t if name == "output_block.1" else R.f16(t)
        self.t[name] = t.clone()
        return t


def _w2l_failures(mutate):
    from oracle import wav2lip_oracle as W
    sd = {k: torch.from_numpy(v) for k, v in synth.wav2lip_state_dict(1234).items()}
    g = torch.Generator().manual_seed(0)
    mel = R.f16(torch.randn(1, 1, 80, 16, generator=g))
    face = R.f16(torch.rand(1, 6, 256, 256, generator=g))
    sim = _SimW2L(mutate)
    W.forward(sd, mel, face, force=sim)
    rp = R.replay_wav2lip(sd, mel, face, lambda name, ref: sim.t[name].to(ref.dtype))
    assert [r["name"] for r in rp.records] == [l.prefix for l in W.all_block_layers()] + [W.OUTPUT_HEAD_PREFIX]
    return R.failures(rp.records, model_too=True)


def test_wav2lip_simulated_device_and_a_residual_added_twice():
    """54 layers + head of a simulated pass sit inside the bound (the model folds the residual into the centre tap as the loader
    does); a residual block that adds its input a second time on the last row only is found, and only it."""
    assert not _w2l_failures(None)

    def f(t, op):
        t = t.clone()
        t[:, :, -1] += op["x"][:, :, -1]
        return t
    _only(_w2l_failures({"face_decoder_blocks.6.2": f}), "face_decoder_blocks.6.2")


# ------------------------------------------------------------------------------------------------ Whisper
def test_whisper_restatement_equals_transformers_and_one_simulated_layer():
    """oracle.whisper_oracle.encoder_ops is the library's encoder (hidden states equal to 1e-6); a simulated device - one encoder
    layer is enough for every op type - passes every gate; an attention that drops the 12 keys behind the last whole tile of 16
    (1500 = 93 x 16 + 12) is found.  The tanh-GELU in fc1's epilogue is NOT: there the GELU shares one fp16 rounding with a
    384-term sum, and the weight-rounding term c A of that sum (2^-12 * 1.13 * sum |w| |x|) is larger than the tanh form's error
    (at most 5e-4 absolute): measured worst |dev - ref| / tol 0.32, rel_l2 3.3e-4 against the model's 3.0e-4.  As its own op
    (the GEGLU of the MuseTalk program with MT_FUSE=0, fault (e) above) the same fault is 102 x outside the bound."""
    from oracle import whisper_oracle as WO
    model = WO.tiny_whisper(0)
    sd = {k: v.detach().clone() for k, v in model.encoder.state_dict().items()}
    wav = synth.synthetic_audio(2.0)[: 52 * 320]
    _, hs, feats = WO.audio2feat(model, wav)
    with torch.no_grad():
        st = WO.encoder_ops(sd, feats)
    assert len(st) == 5 and all(float((a[0] - b).abs().max()) <= 1e-6 for a, b in zip(st, hs))

    one = {k: v for k, v in sd.items() if not k.startswith("layers.") or k.startswith("layers.0.")}
    sim_sd = {k: (R.f16(v) if k.endswith(".weight") and v.dim() >= 2 and k != "embed_positions.weight" else v) for k, v in one.items()}
    x = R.f16(feats)

    def run(mutate):
        sim = R.SimDevice(fused=("conv2",), mutate=mutate)
        with torch.no_grad():
            WO.encoder_ops(sim_sd, x, force=sim)
        rp = R.replay_whisper(one, x, sim.fetch)
        names = [r["name"] for r in rp.records]
        assert R.uncovered([(n, 0) for n in WO.encoder_op_names(1)], names, WO.FUSED_INTO) == []
        assert R.uncovered([(n, 0) for n in WO.encoder_op_names(1)], [n for n in names if n != "embed_positions"], WO.FUSED_INTO) == ["conv2", "embed_positions"]
        return R.failures(rp.records, model_too=True), {r["name"]: r for r in rp.records}

    assert not run(None)[0]

    def ragged(t, op):
        q, k, v = op["q"], op["k"][:, :, :1488], op["v"][:, :, :1488]
        o = F.scaled_dot_product_attention(q, k, v).transpose(1, 2).reshape(1, 1500, 384)
        return o.permute(0, 2, 1)[..., None]
    _only(run({"layers.0.self_attn.attn": ragged})[0], "layers.0.self_attn.attn")

    def tanh_gelu(t, op):
        z = F.linear(op["x"], sim_sd["layers.0.fc1.weight"], sim_sd["layers.0.fc1.bias"])
        return F.gelu(z, approximate="tanh").permute(0, 2, 1)[..., None]
    bad, rec = run({"layers.0.fc1": tanh_gelu})
    r = rec["layers.0.fc1"]
    print(f"[op replay] tanh-GELU in fc1's epilogue: worst |dev - ref| / tol {r['dev_over_tol']:.2f}, rel_l2 {r['rel_dev']:.3e} against the model's {r['rel_mod']:.3e}")
    assert not [b for b in bad if not b.startswith("layers.0.fc1: ")]


# ------------------------------------------------------------------------------------------------ Ultralight
import ultralight_ref as U  # noqa: E402

UL_DW = "down1.maxpool_conv.0.double_conv.0.conv.3"


class _SimUL(R.SimDevice):
    """The float32 restatement as the device computes it: fp16 weights for the dense convs (the state dict it is run on), fp32 for
    the depthwise convs, inc.inconv.0.conv.0 and outc.conv, the upsample evaluated in float64 (upsample2x_kernel), every output
    rounded to fp16 but outc.conv's."""

    def __init__(self, mutate=None):
        super().__init__(mutate=mutate, fp32=("outc.conv",))

    def __call__(self, name, t):
        if name.endswith(".up") and name not in self.mutate:
            t = F.interpolate(self.ops[name]["x"].double(), scale_factor=2, mode="bilinear", align_corners=True).float()
        return super().__call__(name, t)


@pytest.fixture(scope="module")
def ul():
    sd = synth.ultralight_state_dict(1234)
    dense = lambda k, v: k.endswith(".weight") and v.ndim == 4 and v.shape[1] > 1 and k not in ("inc.inconv.0.conv.0.weight", "outc.conv.weight")
    sim_sd = {k: (v.astype(np.float16).astype(np.float32) if dense(k, v) else v) for k, v in sd.items()}
    assert sum(dense(k, v) for k, v in sd.items()) == 81 - 26 - 2          # 26 depthwise convs, the input conv and the head stay fp32
    return sd, sim_sd


def _ul_records(ul, B, mutate=None):
    sd, sim_sd = ul
    img6, feat = synth.ultralight_inputs(B, 1234)
    sim = _SimUL(mutate)
    U.forward(sim_sd, img6, feat, dtype=torch.float32, force=sim)
    rp = U.replay_ultralight(sd, img6, feat, sim.fetch)
    assert [r["name"] for r in rp.records] == U.op_names() and len(rp.records) == 86          # 81 convs, 4 upsamples, audio_feat
    return rp.records


@pytest.mark.parametrize("B", [1, 2])
def test_ultralight_simulated_device_passes_every_gate(ul, B):
    """Measured: largest |mod - ref| / tol 0.4997 (the upsamples and audio_feat: one fp16 rounding, 2^-11, against 2^-10 |ref|),
    0.43 over the dense convs (down4.maxpool_conv.0.double_conv.0.conv.6)."""
    rec = _ul_records(ul, B)
    worst = max(rec, key=lambda r: r["mod_over_tol"])
    dense = max((r for r in rec if r["name"].endswith((".conv.0", ".conv.6", "conv3", "conv5")) and r["name"] != "inc.inconv.0.conv.0"),
                key=lambda r: r["mod_over_tol"])
    print(f"[op replay] ultralight B={B}: {len(rec)} ops; largest |mod - ref| / tol {worst['mod_over_tol']:.4f} ({worst['name']}), "
          f"dense convs {dense['mod_over_tol']:.2f} ({dense['name']})")
    bad = R.failures(rec, model_too=True)
    assert not bad, "\n".join(bad)
    names = [r["name"] for r in rec]
    ops = [(n, 0) for n in U.op_names()]
    assert R.uncovered(ops, names, {}) == []
    assert R.uncovered(ops, [n for n in names if n != "up3.up"], {}) == ["up3.up"]


def _bn(sd, bn, y):
    v = lambda k: torch.from_numpy(sd[bn + k])[None, :, None, None]
    return (y - v(".running_mean")) / torch.sqrt(v(".running_var") + U.BN_EPS) * v(".weight") + v(".bias")


def _ul_only(ul, B, name, fn):
    _only(R.failures(_ul_records(ul, B, {name: fn}), model_too=True), name)


def test_ultralight_fault_1_depthwise_pads_with_the_clamped_edge(ul):
    sd = ul[1]

    def f(t, op):
        w = torch.from_numpy(sd[UL_DW + ".weight"])
        y = F.conv2d(F.pad(op["x"], (1, 1, 1, 1), mode="replicate"), w, stride=2, groups=w.shape[0])
        return F.relu(_bn(sd, op["bn"], y))
    _ul_only(ul, 1, UL_DW, f)


def test_ultralight_fault_2_depthwise_stride_2_sampled_without_the_padding_offset(ul):
    sd = ul[1]

    def f(t, op):                              # ix = 2 ox + kx: padding 0, the map padded at the far edge to keep the size
        w = torch.from_numpy(sd[UL_DW + ".weight"])
        y = F.conv2d(F.pad(op["x"], (0, 2, 0, 2)), w, stride=2, groups=w.shape[0])
        assert y.shape == t.shape
        return F.relu(_bn(sd, op["bn"], y))
    _ul_only(ul, 1, UL_DW, f)


def test_ultralight_fault_3_upsample_without_align_corners(ul):
    _ul_only(ul, 1, "up2.up", lambda t, op: F.interpolate(op["x"], scale_factor=2, mode="bilinear", align_corners=False))


def test_ultralight_fault_4_project_conv_loses_its_residual(ul):
    _ul_only(ul, 1, "fuse_conv.0.double_conv.1.conv.6", lambda t, op: t - op["res"])


def test_ultralight_fault_5_residual_from_the_neighbouring_channel_block(ul):
    _ul_only(ul, 1, "down2.maxpool_conv.0.double_conv.1.conv.6", lambda t, op: t - op["res"] + torch.roll(op["res"], 16, dims=1))


def test_ultralight_fault_6_conv5_outer_ring_as_if_the_padding_were_1(ul):
    sd = ul[1]

    def f(t, op):                              # iy = 2 oy - 1 + ky on the ring (zeros beyond the 16 x 16 map), 2 oy - 3 + ky inside
        w, b = torch.from_numpy(sd["audio_model.conv5.weight"]), torch.from_numpy(sd["audio_model.conv5.bias"])
        y = F.relu(_bn(sd, op["bn"], F.conv2d(F.pad(op["x"], (1, 5, 1, 5)), w, b, stride=2)))
        assert y.shape == t.shape == (1, 512, 10, 10)
        y[:, :, 1:-1, 1:-1] = t[:, :, 1:-1, 1:-1]
        return y
    _ul_only(ul, 1, "audio_model.conv5", f)


def test_ultralight_fault_7_stale_ragged_last_tile_at_b2(ul):
    """200 rows (2 frames x 100 pixels) in tiles of 128: rows 128..199 - frame 1, pixels 28..99 - keep frame 0's values."""
    def f(t, op):
        t = t.clone()
        t[1].reshape(t.shape[1], 100)[:, 28:] = t[0].reshape(t.shape[1], 100)[:, 28:]
        return t
    _ul_only(ul, 2, "down4.maxpool_conv.0.double_conv.0.conv.6", f)


def test_ultralight_fault_8_mask_rectangle_one_row_short(ul):
    sd = ul[1]

    def f(t, op):                              # y = 149, the last masked row, keeps the image
        x = op["x"].clone()
        x[:, 3:, 149, 5:155] = x[:, :3, 149, 5:155]
        y = F.conv2d(x, torch.from_numpy(sd["inc.inconv.0.conv.0.weight"]))
        return F.relu(_bn(sd, op["bn"], y))
    _ul_only(ul, 1, "inc.inconv.0.conv.0", f)
