"""Op-by-op replay of the MuseTalk device program (U-Net + VAE decoder), the Wav2Lip program, the Whisper encoder and the Ultralight
program against float64: oracle/op_replay.py.

The program runs once; every named tensor is read back (Engine.musetalk_debug_get); the float64 oracle then recomputes every op on
the DEVICE's own inputs, so each comparison measures one op (or one fused group) and nothing upstream.  Gates, per op (bound and
rounding model: header of oracle/op_replay.py):
  * per element, no violator: |dev - ref| <= 2^-10 |ref| + c A + s;
  * aggregate: rel_l2(dev, ref) <= 2 * rel_l2(mod, ref) + 1e-4  (the fp8 convs: this gate only);
  * coverage: every op of Engine.musetalk_ops() compared on its own, through its named views, or through the group output that
    oracle.op_replay.fused_into() names - 0 uncovered ops.
Ops are independent per frame: of a 16-frame pass the replay takes the first and last frame and the pair (7, 8), the fp8 16-frame
pass the first and the last.  Every line "<configuration> <op> dev mod ratio max|dev-ref|/tol" is printed; with LTK_OP_REPLAY_OUT
set the same figures are written to that file as one table per program (profiles/op_replay.txt is such a run).

Measured (profiles/op_replay.txt): the whole file 250 s on the GPU box (float64 replay 15 s per frame on 16 CPU threads); 0 uncovered
ops in every configuration; largest |dev - ref| / tol 0.49.  The five largest ratios rel_l2(dev, ref) / rel_l2(mod, ref):
  1.55  ff.geglu of down_blocks.0.attentions.0, token mean at 64 standard deviations (folded LayerNorm: E[x^2] - E[x]^2)
  1.29  attn1.to_q | to_k | to_v of the same case;  1.28  attn2.to_q of the same case
  1.02  decoder.up_blocks.0.upsamplers.0.conv (every configuration);  1.01  decoder.up_blocks.1.upsamplers.0.conv
everything else between 0.99 and 1.00.  Before its sums were shifted, layernorm_kernel (MT_FUSE=0) stood at 1.73 with 4-14 elements per
tensor outside the bound in the 64-standard-deviation case; 1.00 now.
Wav2Lip (54 layers + head, golden batch and 16 frames): every ratio 1.00 (the fp32 head 1.06 at rel_l2 4.7e-8), largest |dev - ref| / tol 0.39.
Whisper encoder (40 ops, the 52-chunk step): every ratio 1.00, largest |dev - ref| / tol 0.85 (layers.2.final_layer_norm).
Ultralight (86 ops of Engine.ultralight_ops(): 81 convs, 4 upsamples, audio_feat; profiles/ultralight_op_replay.txt): host path at
B = 1, 2, 6 (B = 6: lin_fk on the 10 x 10 Cin = 512 expand convs) and the bank path (ultralight_infer, B = 3 from index 1: gather, crop
and mask inside ul_in_kernel, uint8 frames in place of outc.conv), every frame replayed: 0 uncovered ops in every configuration, every
ratio 1.00, largest |dev - ref| / tol 0.50 (the ops that are one fp16 rounding of an exact or fp32 result, where the model itself
sits: upsamples, audio_feat, depthwise and input conv), 0.46 over the dense convs (down4.maxpool_conv.0.double_conv.0.conv.6, B = 6);
audio_feat equals f16(input); uint8 head: 0 of 230 400 bytes outside floor(v) / floor(v +- d), 1 byte not floor(v), 0.28 % of the
bytes within d of an integer.  The four tests 18 s on the GPU box (float64 replay 1 - 1.5 s per frame).
"""
import os
import time
import types

import numpy as np
import pytest

torch = pytest.importorskip("torch")

import synth_inputs as synth  # noqa: E402
from oracle import musetalk_oracle as M  # noqa: E402
from oracle import op_replay as R  # noqa: E402

MT_FUSE_DEFAULT = 7          # csrc/tune.hip


@pytest.fixture(scope="module")
def weights():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    unet_sd = synth.musetalk_unet_state_dict()
    vae_sd = synth.vae_decoder_state_dict()
    return unet_sd, vae_sd, {k: torch.from_numpy(v) for k, v in unet_sd.items()}, {k: torch.from_numpy(v) for k, v in vae_sd.items()}


_TABLES, _NOTES = {}, []          # section -> {configuration: records}; the "#" lines


def _emit(lines):
    for l in lines:
        print(l)
    _NOTES.extend(lines)


def _table(section, config, records):
    for l in R.format_records(config, records):
        print(l)
    _TABLES.setdefault(section, {})[config] = records


@pytest.fixture(scope="module", autouse=True)
def _record_file():
    """LTK_OP_REPLAY_OUT: the figures of the run as one table per program, an op per line, a configuration per column."""
    yield
    path = os.environ.get("LTK_OP_REPLAY_OUT")
    if path and _TABLES:
        with open(path, "a") as f:
            f.write("\n".join(R.format_tables(_TABLES) + _NOTES) + "\n")


def _run_and_replay(config, unet_sd, vae_sd, usd, vsd, B, frames, fp8=False, knobs=None):
    """Build the program under `knobs`, run B frames, replay `frames` of them; -> the Replay.  Knobs are restored by the caller."""
    from livetalking_amd.engine import Engine
    for k, v in (knobs or {}).items():
        Engine.set_knob(k, v)
    eng = Engine(0)
    try:
        eng.load_musetalk(unet_sd, vae_sd, max_frames=B, fp8=fp8)
        lat = np.concatenate(synth.musetalk_latents(5) * 4)[:B]
        feat = synth.musetalk_whisper_feats(B, seed=11 + B)
        eng.musetalk_forward_host(lat, feat, want_image=False, want_frames=False)
        ops = eng.musetalk_ops()
        t0 = time.time()
        rp = R.replay_musetalk(usd, vsd, R.engine_fetch(eng, B, frames), fp8=fp8)
        dt = time.time() - t0
    finally:
        eng.close()
    _table("musetalk", config, rp.records)
    miss = R.uncovered(ops, [r["name"] for r in rp.records], R.fused_into(fp8))
    top = sorted(rp.records, key=lambda r: -r["ratio"])[:5]
    _emit([f"# {config}: {len(ops)} ops, {len(rp.records)} compared, {len(miss)} uncovered, replay of {len(frames)} frames {dt:.0f} s; largest ratios: "
           + ", ".join(f"{r['name']} {r['ratio']:.2f}" for r in top)])
    assert not miss, f"{config}: ops neither compared nor listed in FUSED_INTO: {miss}"
    bad = R.failures(rp.records)
    assert not bad, f"{config}:\n" + "\n".join(bad)
    return rp


@pytest.mark.gpu
def test_fp16_default_program_b2(weights):
    _run_and_replay("fp16 B=2", *weights, B=2, frames=[0, 1])


@pytest.mark.gpu
def test_fp16_unfused_program_b2(weights):
    """MT_FUSE=0, MT_GN1=0, GN_COOP=0: every LayerNorm, the GEGLU projection and the GEGLU are ops with tensors of their own, the
    GroupNorms are the two-pass kernels."""
    from livetalking_amd.engine import Engine
    try:
        _run_and_replay("fp16 B=2 plain", *weights, B=2, frames=[1], knobs={"MT_FUSE": 0, "MT_GN1": 0, "GN_COOP": 0})
    finally:
        Engine.set_knob("MT_FUSE", MT_FUSE_DEFAULT)
        Engine.set_knob("MT_GN1", 1)
        Engine.set_knob("GN_COOP", 1)


@pytest.mark.gpu
def test_fp16_default_program_b16(weights):
    """The benched size: row counts of 16 x pixels select other kernels than B = 2 does (lin_fk / lin_mp instead of rowconv at the
    8^2 level, the tile table, split-K)."""
    _run_and_replay("fp16 B=16", *weights, B=16, frames=[0, 7, 8, 15])


@pytest.mark.gpu
def test_fp8_program_b2(weights):
    _run_and_replay("fp8 B=2", *weights, B=2, frames=[0, 1], fp8=True)


@pytest.mark.gpu
def test_fp8_program_b16(weights):
    _run_and_replay("fp8 B=16", *weights, B=16, frames=[0, 15], fp8=True)


@pytest.mark.gpu
@pytest.mark.parametrize("ratio", [16, 64])
def test_layernorm_fold_with_a_large_token_mean(weights, ratio):
    """down_blocks.0.attentions.0.proj_in.bias raised so that the tokens entering the folded LayerNorm have mean / std of about
    `ratio` (var = E[x^2] - E[x]^2 in the fold's epilogue loses log2(ratio^2) bits).  The block's ops pass the same gates, and the
    folded group (norm1 -> to_q | to_k | to_v) is no more than 1.5 x as far from float64 as the LayerNorm kernel + linear of the
    MT_FUSE=0 program on the same input (a numpy emulation of both gives 0.7 x at ratio 16 and 0.9 x at 64)."""
    from livetalking_amd.engine import Engine
    unet_sd, vae_sd, usd, vsd = weights
    p = "down_blocks.0.attentions.0"
    B = 2
    lat = np.concatenate(synth.musetalk_latents(B))
    feat = synth.musetalk_whisper_feats(B)
    taps = {}
    with torch.no_grad():
        M.unet_forward(usd, torch.from_numpy(lat), M.positional_encoding(torch.from_numpy(feat)), taps=taps, detail=p)
    h0 = taps[p + ".proj_in"]                                            # (B, C, H, W)
    std = float(h0.std(dim=1, unbiased=False).mean())
    mean = float(h0.mean(dim=1).abs().mean())
    sd_np = dict(unet_sd)
    sd_np[p + ".proj_in.bias"] = (unet_sd[p + ".proj_in.bias"] + np.float32(ratio * std)).astype(np.float32)
    sd_t = dict(usd)
    sd_t[p + ".proj_in.bias"] = torch.from_numpy(sd_np[p + ".proj_in.bias"])
    print(f"[op replay] fold case: token std {std:.3f}, token |mean| {mean:.3f} -> {ratio * std:.1f} added to proj_in.bias")

    def run(config, knobs, hide):
        for k, v in knobs.items():
            Engine.set_knob(k, v)
        eng = Engine(0)
        try:
            eng.load_musetalk(sd_np, vae_sd, max_frames=B)
            eng.musetalk_forward_host(lat, feat, want_image=False, want_frames=False)
            inner = R.engine_fetch(eng, B)
            fetch = (lambda name, ref: None if name.endswith(hide) else inner(name, ref)) if hide else inner
            rp = R.replay_transformer(sd_t, p, fetch, "down_blocks.0.resnets.0.conv2")
        finally:
            eng.close()
        _table("musetalk, token mean raised", config, rp.records)
        return rp

    try:
        folded = run(f"fold x{ratio}", {}, None)
        plain = run(f"fold x{ratio} plain", {"MT_FUSE": 0}, None)
        # the LayerNorm kernel + linear of the plain program as ONE group on the raw input: its norm1 hidden from the replay
        group = run(f"fold x{ratio} LN+lin", {"MT_FUSE": 0}, (".norm1",))
    finally:
        Engine.set_knob("MT_FUSE", MT_FUSE_DEFAULT)
    bad = R.failures(folded.records) + R.failures(plain.records)
    assert not bad, "\n".join(bad)
    f = {r["name"]: r for r in folded.records}
    g = {r["name"]: r for r in group.records}
    worse = []
    for n in ("to_q", "to_k", "to_v"):
        name = p + ".transformer_blocks.0.attn1." + n
        _emit([f"# fold x{ratio}: {name} folded {f[name]['rel_dev']:.3e}, LayerNorm kernel + linear {g[name]['rel_dev']:.3e}, "
               f"ratio {f[name]['rel_dev'] / g[name]['rel_dev']:.2f}"])
        if not f[name]["rel_dev"] <= 1.5 * g[name]["rel_dev"]:
            worse.append(name)
    assert not worse, worse


# ------------------------------------------------------------------------------------------------ Wav2Lip: 54 layers + head
def _wav2lip_replay(config, engine, sd_np, mel, face, frames):
    """One pass with the layer capture on; the float64 replay of `frames` of it, layer by layer (a captured layer is read, sliced
    and dropped).  mel (B,1,80,16), face (B,6,256,256) float32 tensors."""
    from oracle import wav2lip_oracle
    B = face.shape[0]
    sd = {k: torch.from_numpy(v) for k, v in sd_np.items()}
    idx = np.asarray(frames)
    engine.debug_capture(True)
    try:
        got = engine.wav2lip_forward_host(mel.numpy().reshape(B, 80, 16), face.numpy())

        def fetch(name, ref):
            if name == wav2lip_oracle.OUTPUT_HEAD_PREFIX:
                return torch.from_numpy(got[idx]).to(ref.dtype)
            return torch.from_numpy(engine.debug_get(name, (B,) + tuple(ref.shape[1:]))[idx]).to(ref.dtype)

        # the pass takes its inputs in as fp16
        rp = R.replay_wav2lip(sd, R.f16(mel[idx]), R.f16(face[idx]), fetch)
    finally:
        engine.debug_capture(False)
    _table("wav2lip", config, rp.records)
    compared = {r["name"] for r in rp.records}
    miss = [n for n in engine.layer_names() + [wav2lip_oracle.OUTPUT_HEAD_PREFIX] if n not in compared]
    top = sorted(rp.records, key=lambda r: -r["ratio"])[:5]
    _emit([f"# {config}: {len(engine.layer_names())} layers + head, {len(rp.records)} compared, {len(miss)} uncovered; largest ratios: "
           + ", ".join(f"{r['name']} {r['ratio']:.2f}" for r in top)])
    assert not miss, f"{config}: layers not compared: {miss}"
    bad = R.failures(rp.records)
    assert not bad, f"{config}:\n" + "\n".join(bad)


@pytest.mark.gpu
def test_wav2lip_golden_batch(engine, golden_dir):
    import zlib
    from oracle import plugin_oracle
    g = np.load(os.path.join(golden_dir, "wav2lip_golden.npz"))
    gm = np.load(os.path.join(golden_dir, "mel_golden.npz"))
    _, faces, _ = synth.wav2lip_avatar(n_frames=int(g["avatar_frames"]), full_hw=tuple(int(v) for v in g["avatar_hw"]),
                                       box=int(g["avatar_box"]), seed=int(g["avatar_seed"]))
    assert zlib.crc32(b"".join(f.tobytes() for f in faces)) == int(g["face_crc"]), "synthetic bank drifted"
    B = int(g["batch"])
    feats = [gm["ref_chunks"][int(g["mel_step"])][i] for i in range(B)]
    mel, face = plugin_oracle.pack_inputs(faces, int(g["index"]), B, feats)
    _wav2lip_replay(f"w2l B={B}", engine, synth.wav2lip_state_dict(int(g["weight_seed"])), mel, face, list(range(B)))


@pytest.mark.gpu
def test_wav2lip_16_frames(engine, golden_dir):
    """The benched batch: the 16-frame pass picks other tiles and kernels (rowconv / rowgemm thresholds follow the row count)."""
    from oracle import mel_oracle, plugin_oracle
    B = 16
    _, faces, _ = synth.wav2lip_avatar(n_frames=5, full_hw=(360, 640), box=160, seed=3)
    audio = synth.synthetic_audio(3.0)
    feats = list(mel_oracle.mel_chunks(audio[: (20 + 2 * B) * 320], 20 + 2 * B))[:B]
    mel, face = plugin_oracle.pack_inputs(faces, 1, B, feats)
    _wav2lip_replay("w2l B=16", engine, synth.wav2lip_state_dict(1234), mel, face, [0, 7, 8, 15])


# ------------------------------------------------------------------------------------------------ Whisper encoder
@pytest.mark.gpu
def test_whisper_encoder_step():
    """The 52-chunk step of tests/test_whisper_gpu.py: conv1 / conv2 + positions (added in place: one group), and per layer the
    LayerNorms, q / k / v, attention (d = 64 over 1500 keys), out_proj, fc1 + GELU, fc2, then the final LayerNorm, each on the
    device's own input, the log-mel "input_features" included."""
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from livetalking_amd.engine import Engine
    from oracle import whisper_oracle as WO
    model = WO.tiny_whisper(0)
    sd = {k: v.detach().clone() for k, v in model.encoder.state_dict().items()}
    B, l = 16, 10
    eng = Engine(0)
    try:
        eng.load_whisper(dict(sd))
        wav = synth.synthetic_audio(2.0)[: (20 + 2 * B) * 320]
        d_out = torch.zeros(B, 50, 384, dtype=torch.float32, device="cuda")
        eng.whisper_step(wav, B, first_row=int((0 + l / 2) * 2), d_out_ptr=d_out.data_ptr())
        feats = torch.from_numpy(eng.whisper_debug_get("input_features", (80, 3000)))[None]

        def fetch(name, ref):
            if name in WO.FUSED_INTO:
                return None
            _, C, T, _ = ref.shape
            t = torch.from_numpy(eng.whisper_debug_get(name, (C, T))).reshape(1, C, T, 1).to(ref.dtype)
            return t * 8.0 if name.endswith(".q_proj") else t          # d^-0.5 = 1 / 8 is folded into q_proj

        rp = R.replay_whisper(sd, feats, fetch)
    finally:
        eng.close()
    _table("whisper", "whisper", rp.records)
    miss = R.uncovered([(n, 0) for n in WO.encoder_op_names()], [r["name"] for r in rp.records], WO.FUSED_INTO)
    top = sorted(rp.records, key=lambda r: -r["ratio"])[:5]
    _emit([f"# whisper: {len(WO.encoder_op_names())} ops, {len(rp.records)} compared, {len(miss)} uncovered; largest ratios: "
           + ", ".join(f"{r['name']} {r['ratio']:.2f}" for r in top)])
    assert not miss, miss
    bad = R.failures(rp.records)
    assert not bad, "\n".join(bad)


# ------------------------------------------------------------------------------------------------ Ultralight: 86 ops
@pytest.fixture(scope="module")
def ul():
    """An engine of its own with the golden's weights over the three-face bank of synth.ultralight_faces."""
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import ultralight_ref as U
    from livetalking_amd.engine import Engine
    sd = synth.ultralight_state_dict(1234)
    faces = synth.ultralight_faces(3, 1234)
    frames, _, coords = synth.ultralight_avatar(3, (120, 200), seed=3)
    eng = Engine(0)
    try:
        aid = eng.register_ultralight_avatar(sd, faces, frames, coords, max_frames=6)
        yield types.SimpleNamespace(eng=eng, aid=aid, sd=sd, faces=faces, U=U)
    finally:
        eng.close()


def _ul_replay(config, ul, B, img6, feat, run, fused=None):
    """run() executes one pass of B frames with the capture on; every frame of it is replayed and every op of
    Engine.ultralight_ops() has to be compared (fused: {op: what the caller checks in its place}).  -> the Replay."""
    eng = ul.eng
    eng.debug_capture(True)
    try:
        run()

        def fetch(name, ref):
            if fused and name in fused:
                return None
            return torch.from_numpy(eng.debug_get(name, (B,) + tuple(ref.shape[1:]))).to(ref.dtype)

        t0 = time.time()
        rp = ul.U.replay_ultralight(ul.sd, img6, feat, fetch, fused=fused)
        dt = time.time() - t0
    finally:
        eng.debug_capture(False)
    _table("ultralight", config, rp.records)
    ops = eng.ultralight_ops(ul.aid)
    assert [n for n, _ in ops] == ul.U.op_names()
    miss = R.uncovered(ops, [r["name"] for r in rp.records] + list((fused or {}).values()), fused or {})
    top = sorted(rp.records, key=lambda r: -r["ratio"])[:5]
    _emit([f"# {config}: {len(ops)} ops, {len(rp.records)} compared, {len(miss)} uncovered, largest |dev - ref| / tol {max(r['dev_over_tol'] for r in rp.records):.2f}, "
           f"replay of {B} frames {dt:.0f} s; largest ratios: " + ", ".join(f"{r['name']} {r['ratio']:.2f}" for r in top)])
    assert not miss, f"{config}: ops not compared: {miss}"
    bad = R.failures(rp.records)
    assert not bad, f"{config}:\n" + "\n".join(bad)
    return rp


@pytest.mark.gpu
@pytest.mark.parametrize("B", [1, 2, 6])
def test_ultralight_host_path(ul, B):
    """ultralight_forward_host on the golden's weights and inputs, every frame replayed, every op of Engine.ultralight_ops()
    compared.  B = 1: the 10 x 10 maps are one ragged 100-row tile; B = 2: lin_fk takes up1's Cin = 512 expand conv (800 rows);
    B = 6: the smallest count at which it takes the 10 x 10 Cin = 512 expand convs (600 rows >= kLinFkMinRows)."""
    img6, feat = synth.ultralight_inputs(B, 1234)
    rp = _ul_replay(f"ul host B={B}", ul, B, img6, feat, lambda: ul.eng.ultralight_forward_host(ul.aid, img6, feat))
    assert len(rp.records) == 86


def _mirror(size, index):
    turn, res = divmod(index, size)
    return res if turn % 2 == 0 else size - res - 1


@pytest.mark.gpu
def test_ultralight_bank_path_and_uint8_head(ul):
    """One ultralight_infer call with the capture on (eager: the capture disables the graph), B = 3 from index 1 over the
    three-face bank: bank order 1, 2, 2.  inc.inconv.0.conv.0 is held to the float64 op on img6_from_faces of those faces in that
    order (gather order, crop offset and mask rectangle per element), audio_feat to the request's features.

    outc.conv has no float tap here; the uint8 frames stand for it.  On the device's own up4.conv.double_conv.1.conv.6 tensor,
    v = 255 sigmoid(conv) in float64; a byte has to be floor(v), or, where v lies within d of an integer, floor(v - d) or
    floor(v + d); more than 1 % of the bytes inside that zone fails the test (it would then say too little).
    d = 255 x the head's bound.  The bound of the w2l_head kind (2^-10 |ref| + 2^-12 A s (1 - s), made for every program's table)
    gives d = 0.25 LSB (median) and puts 41.9 % of these bytes into the zone - computed on the CPU from the float64 forward of
    these inputs alone - so it cannot meet the 1 % condition whatever the device does.  ul_head_kernel is fp32 throughout: 32 FMAs
    and the bias (33 roundings of 2^-24 of at most A = |W| (*) |x| + |b|: 2^-18 A, through the sigmoid's slope s (1 - s)), expf,
    the sum, the division, the product with 255 (2^-21 s together).  The test uses that bound, asserts that it is nowhere above
    the w2l_head bound (what it accepts the other accepts too), and gets d = 1.5e-3 LSB (median), 0.29 % of the bytes in the
    zone on the CPU."""
    import torch.nn.functional as F
    U, eng = ul.U, ul.eng
    B, index = 3, 1
    order = [_mirror(3, index + i) for i in range(B)]
    assert order == [1, 2, 2]
    img6 = U.img6_from_faces([ul.faces[i] for i in order])
    feat = synth.ultralight_inputs(B, 1234)[1]
    d_feat = torch.from_numpy(np.ascontiguousarray(feat)).cuda()
    d_pred = torch.zeros(B, 160, 160, 3, dtype=torch.uint8, device="cuda")
    rp = _ul_replay("ul bank B=3", ul, B, img6, feat, lambda: eng.ultralight_infer([(ul.aid, index, B, d_feat.data_ptr(), d_pred.data_ptr())]),
                         fused={"outc.conv": "frames"})
    compared = [r["name"] for r in rp.records]
    assert "outc.conv" not in compared and "inc.inconv.0.conv.0" in compared and "audio_feat" in compared

    x = rp.fused["outc.conv"]["x"]                                       # the device's own tensor, float64
    W, b = (torch.from_numpy(ul.sd["outc.conv." + k]).double() for k in ("weight", "bias"))
    sg = torch.sigmoid(F.conv2d(x, W, b))
    v = 255.0 * sg
    wide = rp.head(x.float(), "outc.conv", sg)[1].double() + R.F16_FLOOR
    tol = 2.0 ** -18 * F.conv2d(x.abs(), W.abs(), b.abs()) * sg * (1 - sg) + 2.0 ** -21 * sg
    assert bool((tol <= wide).all())
    d = 255.0 * tol
    lo, hi = torch.floor(v - d), torch.floor(v + d)
    zone = float((lo != hi).double().mean())
    got = d_pred.cpu().permute(0, 3, 1, 2).double()
    wrong = int(((got != torch.floor(v)) & ~((lo != hi) & ((got == lo) | (got == hi)))).sum())
    off = int((got != torch.floor(v)).sum())
    _emit([f"# ul bank B=3 uint8 head: {got.numel()} bytes, {wrong} outside floor(v) / floor(v +- d), {off} not floor(v); d median {float(d.median()):.2e} LSB, "
           f"{100 * zone:.2f} % of the bytes within d of an integer"])
    assert zone <= 0.01, f"{100 * zone:.2f} % of the bytes lie within d of an integer"
    assert wrong == 0, f"{wrong} bytes are neither floor(v) nor inside the rounding zone"
