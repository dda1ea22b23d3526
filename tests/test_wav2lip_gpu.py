"""Parity of the HIP Wav2Lip path against the oracle (oracle/wav2lip_oracle.py,
pinned to the reference by oracle/gen_golden.py) and the committed golden
fixtures produced by the reference's own LipReal.inference_batch.

Tolerances (fp16 activations / fp32 accumulate vs the reference's fp32):
  per layer : relative L2 error <= 1e-2, |mean| drift small
  frames    : PSNR >= 40 dB and max-abs <= 6 LSB on the uint8 face crop,
              >= 99% of bytes within +-2 LSB
"""
import os
import zlib

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from oracle import mel_oracle, plugin_oracle, wav2lip_oracle  # noqa: E402
import synth_inputs as synth


def _golden_inputs(golden_dir):
    g = np.load(os.path.join(golden_dir, "wav2lip_golden.npz"))
    gm = np.load(os.path.join(golden_dir, "mel_golden.npz"))
    hw = tuple(int(v) for v in g["avatar_hw"])
    frames, faces, coords = synth.wav2lip_avatar(n_frames=int(g["avatar_frames"]), full_hw=hw,
                                                 box=int(g["avatar_box"]), seed=int(g["avatar_seed"]))
    assert zlib.crc32(b"".join(f.tobytes() for f in faces)) == int(g["face_crc"]), "synthetic bank drifted"
    feats = [gm["ref_chunks"][int(g["mel_step"])][i] for i in range(int(g["batch"]))]
    return g, frames, faces, coords, feats


def psnr_u8(a, b):
    d = a.astype(np.float64) - b.astype(np.float64)
    mse = float((d * d).mean())
    return 99.0 if mse == 0 else 10 * np.log10(255.0 ** 2 / mse)


@pytest.mark.gpu
def test_layers_vs_oracle(engine, golden_dir):
    g, frames, faces, coords, feats = _golden_inputs(golden_dir)
    B, index = int(g["batch"]), int(g["index"])
    sd = {k: torch.from_numpy(v) for k, v in synth.wav2lip_state_dict(int(g["weight_seed"])).items()}
    mel_t, img_t = plugin_oracle.pack_inputs(faces, index, B, feats)
    taps = {}
    ref = wav2lip_oracle.forward(sd, mel_t, img_t, taps).numpy()
    engine.debug_capture(True)
    try:
        got = engine.wav2lip_forward_host(mel_t.numpy().reshape(B, 80, 16), img_t.numpy())
        report = []
        for name in [l.prefix for l in wav2lip_oracle.all_block_layers()]:
            r = taps[name].numpy()
            o = engine.debug_get(name, r.shape)
            rel = float(np.linalg.norm(o - r) / max(np.linalg.norm(r), 1e-9))
            mx = float(np.abs(o - r).max())
            print(f"[layer] {name:28s} rel_l2={rel:.3e} maxabs={mx:.3e} refmax={np.abs(r).max():.3g}")
            if not (rel <= 1e-2):
                report.append(f"{name}: rel L2 {rel:.3e} (max abs {mx:.3e})")
    finally:
        engine.debug_capture(False)
    assert not report, "\n".join(report)
    err = np.abs(got - ref)
    print(f"[forward] sigmoid max abs err {err.max():.3e} mean {err.mean():.3e}")
    assert err.max() < 2.5e-2 and err.mean() < 2e-3


@pytest.mark.gpu
def test_infer_vs_reference_golden(engine, golden_dir):
    """ltk_wav2lip_infer (bank gather + mask + pack + 55 layers + head) against
    the frames the reference's LipReal.inference_batch produced."""
    g, frames, faces, coords, feats = _golden_inputs(golden_dir)
    B, index = int(g["batch"]), int(g["index"])
    aid = engine.register_avatar(faces, frames, coords)
    mel = torch.from_numpy(np.stack(feats).astype(np.float32)).cuda()
    pred = torch.zeros(B, 256, 256, 3, dtype=torch.uint8, device="cuda")
    engine.wav2lip_infer([(aid, index, B, mel.data_ptr(), pred.data_ptr())])
    got = pred.cpu().numpy()
    ref = g["ref_pred_u8"]
    d = np.abs(got.astype(np.int32) - ref.astype(np.int32))
    p = psnr_u8(got, ref)
    frac2 = float((d <= 2).mean())
    print(f"[infer] PSNR {p:.2f} dB, max abs {d.max()} LSB, within+-2: {frac2:.5f}, within+-1: {float((d <= 1).mean()):.5f}")
    assert p >= 40.0 and d.max() <= 6 and frac2 >= 0.99
    engine.release_avatar(aid)


@pytest.mark.gpu
@pytest.mark.parametrize("B", [1, 2])
def test_infer_one_and_two_frames(engine, golden_dir, B):
    """--batch_size 1 (config.py:65) and a 2-frame call through ltk_wav2lip_infer with the fused head (the default): the
    output conv must pick a tile the fused epilogue exists for also when a launch has a single frame.  Frames against the
    reference's LipReal.inference_batch golden (frame i of the B=4 golden depends on bank index and window i only)."""
    g, frames, faces, coords, feats = _golden_inputs(golden_dir)
    index = int(g["index"])
    aid = engine.register_avatar(faces, frames, coords)
    mel = torch.from_numpy(np.stack(feats[:B]).astype(np.float32)).cuda()
    pred = torch.zeros(B, 256, 256, 3, dtype=torch.uint8, device="cuda")
    engine.wav2lip_infer([(aid, index, B, mel.data_ptr(), pred.data_ptr())])
    got = pred.cpu().numpy()
    ref = g["ref_pred_u8"][:B]
    d = np.abs(got.astype(np.int32) - ref.astype(np.int32))
    p = psnr_u8(got, ref)
    print(f"[infer B={B}] PSNR {p:.2f} dB, max abs {d.max()} LSB")
    assert p >= 40.0 and d.max() <= 6
    engine.release_avatar(aid)


@pytest.mark.gpu
def test_infer_batching_invariance(engine, golden_dir):
    """Two sessions coalesced into one launch vs the same sessions run one by one: cross-session batching
    must not change a session's frames.  Tiling never changes an output element's summation order; the
    split-K factor of the small-map layers does depend on the launch's frame count (fp32 partial sums are
    then added in a different order; one fp16 ulp in the 1x1 bottleneck reaches every output pixel), so the
    default mode is held to <= 2 LSB / PSNR >= 55 dB and the LTK_SPLITK=0 mode to bit equality."""
    g, frames, faces, coords, feats = _golden_inputs(golden_dir)
    aid = engine.register_avatar(faces, frames, coords)
    mel = torch.from_numpy(np.stack(feats).astype(np.float32)).cuda()
    a = torch.zeros(4, 256, 256, 3, dtype=torch.uint8, device="cuda")
    b = torch.zeros(3, 256, 256, 3, dtype=torch.uint8, device="cuda")
    engine.wav2lip_infer([(aid, 3, 4, mel.data_ptr(), a.data_ptr())])
    engine.wav2lip_infer([(aid, 7, 3, mel.data_ptr(), b.data_ptr())])
    a2, b2 = torch.zeros_like(a), torch.zeros_like(b)
    engine.wav2lip_infer([(aid, 3, 4, mel.data_ptr(), a2.data_ptr()), (aid, 7, 3, mel.data_ptr(), b2.data_ptr())])
    for got, ref in ((a2, a), (b2, b)):
        d = (got.to(torch.int16) - ref.to(torch.int16)).abs()
        neq = float((d != 0).float().mean())
        print(f"[batching] max diff {int(d.max())} LSB, differing bytes {neq:.2e}")
        assert int(d.max()) <= 2 and psnr_u8(got.cpu().numpy(), ref.cpu().numpy()) >= 55.0
    # LTK_SPLITK=0: no split-K anywhere -> every output element has ONE summation order whatever the
    # launch's frame count, and coalescing is bit-exact
    from livetalking_amd.engine import Engine
    Engine.set_knob("SPLITK", 0)
    try:
        engine.wav2lip_infer([(aid, 3, 4, mel.data_ptr(), a.data_ptr())])
        engine.wav2lip_infer([(aid, 7, 3, mel.data_ptr(), b.data_ptr())])
        engine.wav2lip_infer([(aid, 3, 4, mel.data_ptr(), a2.data_ptr()), (aid, 7, 3, mel.data_ptr(), b2.data_ptr())])
    finally:
        Engine.set_knob("SPLITK", 1)
    assert torch.equal(a2, a) and torch.equal(b2, b)
    engine.release_avatar(aid)


@pytest.mark.gpu
def test_audio_first_layers_vs_generic_path(engine, golden_dir):
    """Knob AUDIO0 (default 3, conv7_mfma.hip).  Bit 0: audio_encoder.0 (Conv2d(1, 32, 3, 1, 1) + BN + ReLU, wav2lip_v2.py:42) as the VALU kernel
    that reads the float32 mel windows itself; bit 1: the stride-(3, 1) layer audio_encoder.3 (wav2lip_v2.py:46) as one-wave blocks whose MFMA operands come straight from global memory.  Against
    pack_mel + the generic MFMA launches: same fp16 operands, fp32 sums in another order - each layer's tap holds the oracle's to the
    per-layer tolerance either way, and the frames of a call differ by at most 1 LSB (1-, 7- and 16-frame calls)."""
    from livetalking_amd.engine import Engine
    g, frames, faces, coords, feats = _golden_inputs(golden_dir)
    B, index = int(g["batch"]), int(g["index"])
    sd = {k: torch.from_numpy(v) for k, v in synth.wav2lip_state_dict(int(g["weight_seed"])).items()}
    mel_t, img_t = plugin_oracle.pack_inputs(faces, index, B, feats)
    taps = {}
    wav2lip_oracle.forward(sd, mel_t, img_t, taps)
    rel = {}
    try:
        for on in (3, 0):
            Engine.set_knob("AUDIO0", on)
            engine.debug_capture(True)
            engine.wav2lip_forward_host(mel_t.numpy().reshape(B, 80, 16), img_t.numpy())
            for name in ("audio_encoder.0", "audio_encoder.3", "audio_encoder.12"):
                r = taps[name].numpy()
                o = engine.debug_get(name, r.shape)
                rel[on, name] = float(np.linalg.norm(o - r) / np.linalg.norm(r))
                print(f"[audio0={on}] {name} rel_l2={rel[on, name]:.3e} maxabs={float(np.abs(o - r).max()):.3e}")
            engine.debug_capture(False)
    finally:
        engine.debug_capture(False)
        Engine.set_knob("AUDIO0", 3)
    for name in ("audio_encoder.0", "audio_encoder.3", "audio_encoder.12"):
        assert rel[3, name] <= 2e-3 and rel[3, name] <= rel[0, name] * 1.5 + 1e-5, name
    aid = engine.register_avatar(faces, frames, coords)
    rng = np.random.default_rng(7)
    try:
        for n in (1, 7, 16):
            mel = torch.from_numpy((np.stack([feats[i % len(feats)] for i in range(n)]) +
                                    0.05 * rng.standard_normal((n, 80, 16))).astype(np.float32)).cuda()
            out = {}
            for on in (3, 1, 0):
                Engine.set_knob("AUDIO0", on)
                pred = torch.zeros(n, 256, 256, 3, dtype=torch.uint8, device="cuda")
                engine.wav2lip_infer([(aid, index, n, mel.data_ptr(), pred.data_ptr())])
                out[on] = pred.cpu().numpy()
            for on in (3, 1):
                d = np.abs(out[on].astype(np.int32) - out[0].astype(np.int32))
                print(f"[audio0={on} vs 0, {n} frames] max diff {d.max()} LSB, differing bytes {float((d != 0).mean()):.2e}")
                # (a last-bit change in the first layers reaches every pixel through the audio embedding: as many truncation flips as the
                # rowconv / rowgemm-vs-conv3 comparison below sees)
                assert d.max() <= 1 and float((d != 0).mean()) < 0.10
    finally:
        Engine.set_knob("AUDIO0", 3)
        engine.release_avatar(aid)


@pytest.mark.gpu
def test_convs2d_kernel_vs_first_generation_kernel(engine, golden_dir):
    """Knob CONV_S2D (default 1, conv7_mfma.hip convs2d_kernel): the face encoder's shallow stride-2 layers face_encoder_blocks.1.0 / 2.0
    (wav2lip_v2.py:15,19) with the pixel operands of their MFMAs straight from global memory, against the first-generation kernel: each
    layer's tap holds the oracle's to the per-layer tolerance either way; frames of 1-, 5- and 16-frame calls differ by <= 1 LSB."""
    from livetalking_amd.engine import Engine
    g, frames, faces, coords, feats = _golden_inputs(golden_dir)
    B, index = int(g["batch"]), int(g["index"])
    sd = {k: torch.from_numpy(v) for k, v in synth.wav2lip_state_dict(int(g["weight_seed"])).items()}
    mel_t, img_t = plugin_oracle.pack_inputs(faces, index, B, feats)
    taps = {}
    wav2lip_oracle.forward(sd, mel_t, img_t, taps)
    names = ("face_encoder_blocks.1.0", "face_encoder_blocks.2.0", "face_encoder_blocks.2.3")
    rel = {}
    try:
        for on in (1, 0):
            Engine.set_knob("CONV_S2D", on)
            engine.debug_capture(True)
            engine.wav2lip_forward_host(mel_t.numpy().reshape(B, 80, 16), img_t.numpy())
            for name in names:
                r = taps[name].numpy()
                o = engine.debug_get(name, r.shape)
                rel[on, name] = float(np.linalg.norm(o - r) / np.linalg.norm(r))
                print(f"[convs2d={on}] {name} rel_l2={rel[on, name]:.3e} maxabs={float(np.abs(o - r).max()):.3e}")
            engine.debug_capture(False)
    finally:
        engine.debug_capture(False)
        Engine.set_knob("CONV_S2D", 1)
    for name in names:
        assert rel[1, name] <= 2e-3 and rel[1, name] <= rel[0, name] * 1.5 + 1e-5, name
    aid = engine.register_avatar(faces, frames, coords)
    try:
        for n in (1, 5, 16):
            mel = torch.from_numpy(np.stack([feats[i % len(feats)] for i in range(n)]).astype(np.float32)).cuda()
            out = {}
            for on in (1, 0):
                Engine.set_knob("CONV_S2D", on)
                pred = torch.zeros(n, 256, 256, 3, dtype=torch.uint8, device="cuda")
                engine.wav2lip_infer([(aid, index + 3, n, mel.data_ptr(), pred.data_ptr())])
                out[on] = pred.cpu().numpy()
            d = np.abs(out[1].astype(np.int32) - out[0].astype(np.int32))
            print(f"[convs2d 1 vs 0, {n} frames] max diff {d.max()} LSB, differing bytes {float((d != 0).mean()):.2e}")
            assert d.max() <= 1 and float((d != 0).mean()) < 0.10
    finally:
        Engine.set_knob("CONV_S2D", 1)
        engine.release_avatar(aid)


@pytest.mark.gpu
def test_fused_head_vs_separate_head(engine, golden_dir):
    """output_block conv 80->32 + 1x1 head + sigmoid in ONE launch (knob HEAD_FUSED, the default) against the two-launch
    path (32-channel map rounded to fp16 in between): the fused epilogue keeps fp32, so frames may differ by the
    truncation of a value that sat within one fp16 ulp of an integer -- at most 1 LSB, rarely."""
    from livetalking_amd.engine import Engine
    g, frames, faces, coords, feats = _golden_inputs(golden_dir)
    B, index = int(g["batch"]), int(g["index"])
    aid = engine.register_avatar(faces, frames, coords)
    mel = torch.from_numpy(np.stack(feats).astype(np.float32)).cuda()
    out = {}
    try:
        for fused in (1, 0):
            Engine.set_knob("HEAD_FUSED", fused)
            pred = torch.zeros(B, 256, 256, 3, dtype=torch.uint8, device="cuda")
            engine.wav2lip_infer([(aid, index, B, mel.data_ptr(), pred.data_ptr())])
            out[fused] = pred.cpu().numpy()
    finally:
        Engine.set_knob("HEAD_FUSED", 1)
    d = np.abs(out[1].astype(np.int32) - out[0].astype(np.int32))
    print(f"[fused head] max diff {d.max()} LSB, differing bytes {float((d != 0).mean()):.2e}")
    assert d.max() <= 1 and float((d != 0).mean()) < 0.02
    ref = g["ref_pred_u8"]
    assert psnr_u8(out[1], ref) >= psnr_u8(out[0], ref) - 0.2      # and it is not further from the reference's frames
    engine.release_avatar(aid)


@pytest.mark.gpu
def test_rowconv_and_rowgemm_vs_conv3(golden_dir):
    """The small-map layers as weight-streaming GEMMs (csrc/rowgemm.hip: rowgemm for the one-pixel maps, rowconv for the 3x3 convs
    on the 4x4 / 8x8 maps - knobs ROWGEMM / ROWCONV, both on by default) against the same layers on conv3 + split-K finish: another
    summation order of the same fp16 products, so frames differ by at most 1 LSB, rarely, and are no further from the
    reference's golden frames.  Launch sizes 1, 5, 17, 32 and 64 frames: rowgemm_kernel<1> (<= 16 frames), <2> (17..32), the
    live[] masking of an odd remainder, rowconv on 16 / 80 / 272 / 512 / 1024 rows of the 4x4 maps and the conv3 hand-over
    above 32 frames / 1024 rows."""
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from livetalking_amd.engine import Engine
    g, frames, faces, coords, feats = _golden_inputs(golden_dir)
    B0, index = int(g["batch"]), int(g["index"])
    eng = Engine(0)
    try:
        eng.load_wav2lip(synth.wav2lip_state_dict(int(g["weight_seed"])), max_frames=64)
        aid = eng.register_avatar(faces, frames, coords)
        for nf in (B0, 1, 5, 17, 32, 64):
            # requests of at most 16 frames each (a session's batch), the last one carries the odd remainder
            sizes = [16] * (nf // 16) + ([nf % 16] if nf % 16 else [])
            mels = [torch.from_numpy(np.stack([feats[(i + 3 * r) % len(feats)] for i in range(b)]).astype(np.float32)).cuda()
                    for r, b in enumerate(sizes)]
            out = {}
            try:
                for on in (1, 0):
                    Engine.set_knob("ROWCONV", 1024 if on else 0)
                    Engine.set_knob("ROWGEMM", on)
                    preds = [torch.zeros(b, 256, 256, 3, dtype=torch.uint8, device="cuda") for b in sizes]
                    eng.wav2lip_infer([(aid, index + 2 * r, b, mels[r].data_ptr(), preds[r].data_ptr()) for r, b in enumerate(sizes)])
                    out[on] = np.concatenate([p.cpu().numpy() for p in preds])
            finally:
                Engine.set_knob("ROWCONV", 1024)
                Engine.set_knob("ROWGEMM", 1)
            d = np.abs(out[1].astype(np.int32) - out[0].astype(np.int32))
            print(f"[rowconv/rowgemm vs conv3] {nf} frames: max diff {d.max()} LSB, differing bytes {float((d != 0).mean()):.2e}")
            assert d.max() <= 1 and float((d != 0).mean()) < 0.10, nf
            if nf == B0:
                ref = g["ref_pred_u8"]
                assert psnr_u8(out[1], ref) >= psnr_u8(out[0], ref) - 0.2
        eng.release_avatar(aid)
    finally:
        eng.close()


@pytest.mark.gpu
def test_forward_host_runs_as_arena_passes(golden_dir):
    """warm_up(batch_size) with an arena (LTK_MICROBATCH) smaller than the session batch: ltk_wav2lip_forward_host runs as
    several passes and returns what one pass returns (frames are independent; split-K off so the summation order is too)."""
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from livetalking_amd.engine import Engine
    g, frames, faces, coords, feats = _golden_inputs(golden_dir)
    B, index = int(g["batch"]), int(g["index"])
    mel_t, img_t = plugin_oracle.pack_inputs(faces, index, B, feats)
    mel, img = mel_t.numpy().reshape(B, 80, 16), img_t.numpy()
    weights = synth.wav2lip_state_dict(int(g["weight_seed"]))
    outs = []
    Engine.set_knob("SPLITK", 0)
    try:
        for mb in (0, 3):
            Engine.set_knob("MICROBATCH", mb)
            eng = Engine(0)
            try:
                eng.load_wav2lip(weights, max_frames=B)
                outs.append(eng.wav2lip_forward_host(mel, img))
            finally:
                eng.close()
    finally:
        Engine.set_knob("MICROBATCH", 0)
        Engine.set_knob("SPLITK", 1)
    assert outs[0].shape == outs[1].shape == (B, 3, 256, 256)
    np.testing.assert_array_equal(outs[0], outs[1])


@pytest.mark.gpu
def test_full_size_batching_properties(golden_dir):
    """BASELINE.json configs[3]'s per-GPU share at full size - 16 sessions x 16 frames in ONE call (256 frames), and a
    512-frame call that runs as two arena passes - checked through size-independent properties: a session's frames do
    not depend on what it was batched with (bit-exact with LTK_SPLITK=0, <= 2 LSB with the default per-launch split-K), two
    sessions asking for the same bank frames with the same audio get the same bytes, and the ping-pong index wraps."""
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from livetalking_amd.engine import Engine
    g, frames, faces, coords, feats = _golden_inputs(golden_dir)
    n_bank = len(faces)
    B, S = 16, 32
    mel = torch.from_numpy(np.stack([feats[i % len(feats)] for i in range(B)]).astype(np.float32)).cuda()      # B windows (the golden step has 4)
    assert mel.shape == (B, 80, 16)
    Engine.set_knob("MICROBATCH", 256)
    eng = Engine(0)
    try:
        eng.load_wav2lip(synth.wav2lip_state_dict(int(g["weight_seed"])), max_frames=S * B)
        aid = eng.register_avatar(faces, frames, coords)
        index = [(5 * s) % (2 * n_bank) for s in range(S)]
        index[7] = index[3]                                   # same bank frames, same audio -> same bytes
        index[9] = index[3] + 2 * n_bank                      # one full ping-pong period later (mirror_index, utils/image.py:26-32)
        single = torch.zeros(S, B, 256, 256, 3, dtype=torch.uint8, device="cuda")
        for mode in (1, 0):                                   # default split-K, then LTK_SPLITK=0
            Engine.set_knob("SPLITK", mode)
            for s in range(S):
                eng.wav2lip_infer([(aid, index[s], B, mel.data_ptr(), single[s].data_ptr())])
            assert torch.equal(single[7], single[3]) and torch.equal(single[9], single[3])
            both = torch.zeros_like(single)
            eng.wav2lip_infer([(aid, index[s], B, mel.data_ptr(), both[s].data_ptr()) for s in range(16)])        # 256 frames
            whole = torch.zeros_like(single)
            eng.wav2lip_infer([(aid, index[s], B, mel.data_ptr(), whole[s].data_ptr()) for s in range(S)])        # 512 = 2 passes
            for name, got, n in (("256-frame call", both, 16), ("512-frame call", whole, S)):
                d = (got[:n].to(torch.int16) - single[:n].to(torch.int16)).abs()
                print(f"[full size] {name}, SPLITK={mode}: max diff {int(d.max())} LSB, differing bytes {float((d != 0).float().mean()):.2e}")
                if mode == 0:
                    assert int(d.max()) == 0
                else:
                    assert int(d.max()) <= 2
            assert torch.equal(whole[:16], both[:16]) or mode == 1
    finally:
        Engine.set_knob("SPLITK", 1)
        Engine.set_knob("MICROBATCH", 0)
        eng.close()


# ---------------------------------------------------------------------------------------------------------------
# the BENCHMARKED configuration (BASELINE.json configs[1] / configs[3] share): B = 16 on the 250-frame 720p bank
# ---------------------------------------------------------------------------------------------------------------
def _bench_inputs(golden_dir):
    g = np.load(os.path.join(golden_dir, "wav2lip_bench_golden.npz"))
    gm = np.load(os.path.join(golden_dir, "mel_golden.npz"))
    hw = tuple(int(v) for v in g["bank_hw"])
    frames, faces, coords = synth.wav2lip_bank(int(g["bank_frames"]), hw, int(g["bank_box"]), int(g["bank_seed"]))
    assert zlib.crc32(b"".join(f.tobytes() for f in faces)) == int(g["face_crc"]), "synthetic bank drifted"
    return g, gm, frames, faces, coords


def _frame_report(tag, got, ref_f32):
    """got uint8 (B,256,256,3) from the HIP path, ref_f32 the oracle's float frames (truncated like paste_back does)."""
    ref = ref_f32.astype(np.uint8)
    worst_p, worst_d = 99.0, 0
    for i in range(got.shape[0]):
        d = np.abs(got[i].astype(np.int32) - ref[i].astype(np.int32))
        worst_p, worst_d = min(worst_p, psnr_u8(got[i], ref[i])), max(worst_d, int(d.max()))
    frac2 = float((np.abs(got.astype(np.int32) - ref.astype(np.int32)) <= 2).mean())
    print(f"[{tag}] worst frame PSNR {worst_p:.2f} dB, max abs {worst_d} LSB, within+-2: {frac2:.5f}")
    return worst_p, worst_d, frac2


@pytest.mark.gpu
def test_bench_config_b16_vs_oracle(engine, golden_dir):
    """One bench step (bench.py: 1 session x 16 frames, 250-frame 720p bank, ~320-px boxes) through ltk_wav2lip_infer +
    ltk_paste_back against the oracle run live on the same inputs, every one of the 16 frames; the oracle itself is held to
    the reference's own LipReal output at this configuration (tests/golden/wav2lip_bench_golden.npz).  The composite is
    bit-exact given the prediction bytes, on the upscaling (320-px) and on the shrinking (200-px) bank."""
    g, gm, frames, faces, coords = _bench_inputs(golden_dir)
    B, index = int(g["batch"]), int(g["index"])
    feats = [gm["ref_chunks"][int(g["mel_step"])][i] for i in range(B)]
    sd = {k: torch.from_numpy(v) for k, v in synth.wav2lip_state_dict(int(g["weight_seed"])).items()}
    ref = plugin_oracle.inference_batch(sd, faces, index, B, feats)                       # float32 (16,256,256,3)
    assert np.abs(ref[:, ::8, ::8] - g["ref_pred_sub"]).max() < 2e-3                      # the oracle's pin at this configuration
    aid = engine.register_avatar(faces, frames, coords)
    mel = torch.from_numpy(np.stack(feats).astype(np.float32)).cuda()
    pred = torch.zeros(B, 256, 256, 3, dtype=torch.uint8, device="cuda")
    engine.wav2lip_infer([(aid, index, B, mel.data_ptr(), pred.data_ptr())])
    got = pred.cpu().numpy()
    p, dmax, frac2 = _frame_report("bench B=16", got, ref)
    assert p >= 40.0 and dmax <= 6 and frac2 >= 0.99
    from oracle import paste_oracle
    out = np.empty_like(frames[0])
    for i in range(B):
        idx = int(g["bank_idx"][i])
        engine.paste_back(aid, idx, pred[i].data_ptr(), out)
        assert np.array_equal(out, paste_oracle.paste_back_frame(got[i].astype(np.float32), frames[idx], coords[idx])), i
        y1, y2, x1, x2 = coords[idx]          # and the composited box stays within the frame tolerance of the reference's composite
        dd = np.abs(out[y1:y2:8, x1:x2:8][:39, :39].astype(np.int32) - g["bbox_sub"][i].astype(np.int32))
        assert dd.max() <= 6, (i, int(dd.max()))
    engine.release_avatar(aid)
    hw = tuple(int(v) for v in g["bank_hw"])
    fr_s, fa_s, co_s = synth.wav2lip_bank(int(g["shrink_frames"]), hw, int(g["shrink_box"]), int(g["shrink_seed"]))
    aid2 = engine.register_avatar(fa_s, fr_s, co_s)
    for i in range(B):
        k = i % len(fr_s)
        engine.paste_back(aid2, k, pred[i].data_ptr(), out)
        assert np.array_equal(out, paste_oracle.paste_back_frame(got[i].astype(np.float32), fr_s[k], co_s[k])), i
        y1, y2, x1, x2 = co_s[k]
        dd = np.abs(out[y1:y2:8, x1:x2:8][:24, :24].astype(np.int32) - g["shrink_sub"][i].astype(np.int32))
        assert dd.max() <= 6, (i, int(dd.max()))
    engine.release_avatar(aid2)


@pytest.mark.gpu
def test_coalesced_256_frames_vs_oracle(golden_dir):
    """BASELINE.json configs[3]'s per-GPU share: 16 sessions x 16 frames coalesced into ONE 256-frame call on the bench bank,
    every session with its own bank position and its own audio windows; the first and the last session's frames are checked
    against the ORACLE (not against the engine's own 16-frame calls)."""
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from livetalking_amd.engine import Engine
    g, gm, frames, faces, coords = _bench_inputs(golden_dir)
    B, S = 16, 16
    chunks = gm["ref_chunks"]                                             # (3,16,80,16): three MelASR steps of the reference
    sess_feats = [[chunks[(s + i) % 3][(i + 5 * s) % 16] for i in range(B)] for s in range(S)]
    index = [(243 + 37 * s) % (2 * len(frames)) for s in range(S)]
    sd = {k: torch.from_numpy(v) for k, v in synth.wav2lip_state_dict(int(g["weight_seed"])).items()}
    Engine.set_knob("MICROBATCH", 256)
    eng = Engine(0)
    try:
        eng.load_wav2lip(synth.wav2lip_state_dict(int(g["weight_seed"])), max_frames=S * B)
        aid = eng.register_avatar(faces, frames, coords)
        mel = torch.from_numpy(np.asarray(sess_feats, dtype=np.float32)).cuda()              # (S,B,80,16)
        pred = torch.zeros(S, B, 256, 256, 3, dtype=torch.uint8, device="cuda")
        eng.wav2lip_infer([(aid, index[s], B, mel[s].data_ptr(), pred[s].data_ptr()) for s in range(S)])
        for s in (0, S - 1):
            ref = plugin_oracle.inference_batch(sd, faces, index[s], B, sess_feats[s])
            p, dmax, frac2 = _frame_report(f"256-frame call, session {s}", pred[s].cpu().numpy(), ref)
            assert p >= 40.0 and dmax <= 6 and frac2 >= 0.99
    finally:
        Engine.set_knob("MICROBATCH", 0)
        eng.close()


@pytest.mark.gpu
def test_coalesced_32_and_24_frames_vs_oracle(golden_dir):
    """Two sessions coalesced into one call - what the default scheduler produces whenever two sessions' inference threads meet
    (livetalking_amd/scheduler.py) - on the bench bank: ONE 32-frame call (2 x 16 frames: rowgemm_kernel<2>, rowconv on the 512
    rows of the 4x4 maps, conv3 + split-K on the 8x8 maps) and ONE 24-frame call (16 + 8: the odd-remainder masking of the
    two-frame-tile rowgemm), each session at its own bank position with its own audio windows, BOTH sessions of both calls against
    the ORACLE (reference semantics: wav2lip_avatar.py:116-139 per session; wav2lip_v2.py:36-39,60-66 are the layers that change
    kernel with the launch size)."""
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from livetalking_amd.engine import Engine
    g, gm, frames, faces, coords = _bench_inputs(golden_dir)
    chunks = gm["ref_chunks"]                                             # (3,16,80,16): three MelASR steps of the reference
    sd = {k: torch.from_numpy(v) for k, v in synth.wav2lip_state_dict(int(g["weight_seed"])).items()}
    eng = Engine(0)
    try:
        eng.load_wav2lip(synth.wav2lip_state_dict(int(g["weight_seed"])), max_frames=32)
        aid = eng.register_avatar(faces, frames, coords)
        for sizes in ((16, 16), (16, 8)):
            index = [243, 61]                                            # session 0 walks over the ping-pong turn of the bank
            sess_feats = [[chunks[(s + 1) % 3][(i + 7 * s) % 16] for i in range(b)] for s, b in enumerate(sizes)]
            mels = [torch.from_numpy(np.asarray(f, dtype=np.float32)).cuda() for f in sess_feats]
            preds = [torch.zeros(b, 256, 256, 3, dtype=torch.uint8, device="cuda") for b in sizes]
            eng.wav2lip_infer([(aid, index[s], b, mels[s].data_ptr(), preds[s].data_ptr()) for s, b in enumerate(sizes)])
            for s, b in enumerate(sizes):
                ref = plugin_oracle.inference_batch(sd, faces, index[s], b, sess_feats[s])
                p, dmax, frac2 = _frame_report(f"{sum(sizes)}-frame call, session {s} ({b} frames)", preds[s].cpu().numpy(), ref)
                assert p >= 40.0 and dmax <= 6 and frac2 >= 0.99
    finally:
        eng.close()


@pytest.mark.gpu
def test_graph_replay_equals_eager_launches(engine, golden_dir):
    """Knob GRAPH (default on): a pass of a given frame count is captured as a hipGraph the second time it is seen and replayed from
    then on; the per-call pointers (bank crops, mel windows, output frames) travel through the device-resident tables, not through
    captured kernel arguments.  Five calls with DIFFERENT bank positions, mel buffers and output tensors each - eager, capture,
    three replays - must give byte for byte what the same calls give launch by launch (GRAPH=0): same kernels, same order, same
    fixed-order split-K sums.  Also through the depth-first sub-batch schedule of the 128^2 / 256^2 level (knob DF_FRAMES), which
    changes launch sizes only."""
    from livetalking_amd.engine import Engine
    g, frames, faces, coords, feats = _golden_inputs(golden_dir)
    B = 16
    aid = engine.register_avatar(faces, frames, coords)
    mels = [torch.from_numpy(np.stack([feats[(i + k) % len(feats)] for i in range(B)]).astype(np.float32) * (1.0 - 0.05 * k)).cuda()
            for k in range(5)]

    def run_all():
        outs = []
        for k in range(5):
            pred = torch.zeros(B, 256, 256, 3, dtype=torch.uint8, device="cuda")
            engine.wav2lip_infer([(aid, 3 * k, B, mels[k].data_ptr(), pred.data_ptr())])
            outs.append(pred)
        return outs

    try:
        Engine.set_knob("GRAPH", 0)
        eager = run_all()
        assert engine.graph_count() == 0
        Engine.set_knob("GRAPH", 1)
        replay = run_all()
        assert engine.graph_count() >= 1, "the 16-frame pass was not captured"
        for k in range(5):
            assert torch.equal(eager[k], replay[k]), f"call {k}: graph replay differs from the eager launches"
        assert not torch.equal(eager[0], eager[1])                 # the calls really are different frames
        Engine.set_knob("DF_FRAMES", 4)
        Engine.set_knob("DF_MIN", 1)
        df = run_all()
        d = max(int((a.to(torch.int16) - b.to(torch.int16)).abs().max()) for a, b in zip(eager, df))
        print(f"[depth-first 4-frame sub-batches vs layer by layer] max diff {d} LSB")
        assert d == 0                                              # no split-K in that region: same sums in the same order
    finally:
        Engine.set_knob("GRAPH", 1)
        Engine.set_knob("DF_FRAMES", 0)
        Engine.set_knob("DF_MIN", 32)
    engine.release_avatar(aid)


@pytest.mark.gpu
def test_tile_table_off_equals_table_on_within_one_lsb(engine, golden_dir):
    """The measured per-layer tile table (csrc/w2l_program.hip kTileTable, knob TILE_TABLE) only moves work between tile shapes and
    split factors: with it disabled (conv3's rule alone) a 16-frame and a 64-frame call must give the same frames - tiles never
    change a sum's order, the few split-factor entries do (fixed-order split-K: <= 1 LSB on a small share of the bytes)."""
    from livetalking_amd.engine import Engine
    from livetalking_amd import _lib
    g, frames, faces, coords, feats = _golden_inputs(golden_dir)
    eng = Engine(0)
    try:
        eng.load_wav2lip(synth.wav2lip_state_dict(1234), max_frames=64)
        aid = eng.register_avatar(faces, frames, coords)
        for nf in (16, 64):
            mel = torch.from_numpy(np.stack([feats[i % len(feats)] for i in range(nf)]).astype(np.float32)).cuda()

            def run():
                pred = torch.zeros(nf, 256, 256, 3, dtype=torch.uint8, device="cuda")
                eng.wav2lip_infer([(aid, 1, nf, mel.data_ptr(), pred.data_ptr())])
                return pred.cpu().numpy().astype(np.int16)

            try:
                Engine.set_knob("TILE_TABLE", 1)
                on = run()
                Engine.set_knob("TILE_TABLE", 0)
                off = run()
            finally:
                Engine.set_knob("TILE_TABLE", 1)
            d = np.abs(on - off)
            print(f"[tile table off vs on, {nf} frames] max {int(d.max())} LSB, differing bytes {float((d != 0).mean()):.5f}")
            assert d.max() <= 1 and float((d != 0).mean()) < 0.05
    finally:
        eng.close()


@pytest.mark.gpu
def test_face_cache_mode_equals_mode_off(golden_dir):
    """Knob FACE_CACHE (opt-in deployment mode, include/ltk.h ltk_avatar_face_cache_bytes): the face encoder's skip tensors of
    every bank frame are computed once per avatar and copied into the decoder's concat buffers instead of running conv7 + 20
    encoder layers (wav2lip_v2.py:132-140: `feats` depend on the bank frame only).  A 16-frame call across the bank's ping-pong
    turn must give byte for byte the frames of the mode off (the cache is built by 16-frame launches of the same kernels); a
    64-frame call of four sessions stays within 1 LSB (other split factors on the small-map encoder layers, as between any two
    call sizes) and is byte-identical under LTK_SPLITK=0; the cached pass replays from its own captured graph."""
    from livetalking_amd.engine import Engine
    frames, faces, coords = synth.wav2lip_avatar(n_frames=20, full_hw=(180, 320), box=96, seed=4)
    gm = np.load(os.path.join(golden_dir, "mel_golden.npz"))
    feats = gm["ref_chunks"].reshape(-1, 80, 16).astype(np.float32)          # 48 real mel windows
    eng = Engine(0)
    try:
        eng.load_wav2lip(synth.wav2lip_state_dict(1234), max_frames=64)
        aid = eng.register_avatar(faces, frames, coords)
        mel16 = torch.from_numpy(feats[:16].copy()).cuda()
        mel64 = torch.from_numpy(np.concatenate([feats, feats[:16]]).copy()).cuda()

        def run16():
            pred = torch.zeros(16, 256, 256, 3, dtype=torch.uint8, device="cuda")
            for _ in range(3):                                          # eager, capture, replay
                eng.wav2lip_infer([(aid, 13, 16, mel16.data_ptr(), pred.data_ptr())])       # bank frames 13..19, 19..11
            return pred.cpu().numpy().astype(np.int16)

        def run64():
            pred = torch.zeros(64, 256, 256, 3, dtype=torch.uint8, device="cuda")
            reqs = [(aid, 5 + 9 * s, 16, mel64[16 * s:].data_ptr(), pred[16 * s:].data_ptr()) for s in range(4)]
            for _ in range(2):
                eng.wav2lip_infer(reqs)
            return pred.cpu().numpy().astype(np.int16)

        try:
            off16, off64 = run16(), run64()
            assert eng.face_cache_bytes(aid) == 0
            Engine.set_knob("FACE_CACHE", 1)
            on16, on64 = run16(), run64()          # (the knob change dropped the graphs of the mode off: what is counted below is new)
            per_frame = sum(c * hw * hw * 2 for c, hw in zip((16, 32, 64, 128, 256, 512, 512, 512), (256, 128, 64, 32, 16, 8, 4, 1)))
            assert eng.face_cache_bytes(aid) == 20 * per_frame and per_frame == 4_146_176
            assert eng.graph_count() == 2, "the cached 16- and 64-frame passes were not captured as their own graphs"
            assert np.array_equal(on16, off16), f"16-frame call: max diff {np.abs(on16 - off16).max()} LSB"
            d = np.abs(on64 - off64)
            print(f"[face cache, 64-frame call] max {int(d.max())} LSB, differing bytes {float((d != 0).mean()):.5f}")
            assert d.max() <= 1 and float((d != 0).mean()) < 0.05
            Engine.set_knob("SPLITK", 0)
            Engine.set_knob("FACE_CACHE", 0)
            off64_s = run64()
            assert eng.face_cache_bytes(aid) == 0, "a call with the mode switched off gives the avatar's records back"
            Engine.set_knob("FACE_CACHE", 1)
            Engine.set_knob("FACE_CACHE_MAX_MB", 8)          # 20 frames need 79 MB: refused, loudly, nothing allocated
            with pytest.raises(RuntimeError, match="LTK_FACE_CACHE_MAX_MB"):
                run64()
            assert eng.face_cache_bytes(aid) == 0
            Engine.set_knob("FACE_CACHE_MAX_MB", 16384)
            on64_s = run64()
            assert eng.face_cache_bytes(aid) == 20 * per_frame
            assert np.array_equal(on64_s, off64_s), "LTK_SPLITK=0: the cache must be exact at every call size"
        finally:
            Engine.set_knob("FACE_CACHE", 0)
            Engine.set_knob("FACE_CACHE_MAX_MB", 16384)
            Engine.set_knob("SPLITK", 1)
    finally:
        eng.close()


@pytest.mark.gpu
def test_prefetch_slots_serve_interleaved_sessions(golden_dir):
    """Round 6: the prefetched face-encoder outputs live in an LRU of slots keyed by (avatar, next bank index, frame count)
    (csrc/engine_internal.h PfSlot; round 5 kept ONE engine-wide slot, which interleaved sessions never hit).  Three paced sessions call
    round-robin - two of them on the SAME avatar at different bank positions, one on another avatar - then one session jumps, one
    avatar is released and a new session starts on a new avatar.  Every call's frames equal the knob off byte for byte, and every
    call except the first two of each sequence (the one that starts it, the one that proves it continues) starts at the decoder."""
    from livetalking_amd.engine import Engine
    banks = [synth.wav2lip_avatar(n_frames=20, full_hw=(180, 320), box=96, seed=4), synth.wav2lip_avatar(n_frames=7, full_hw=(180, 320), box=96, seed=6),
             synth.wav2lip_avatar(n_frames=11, full_hw=(180, 320), box=96, seed=8)]
    gm = np.load(os.path.join(golden_dir, "mel_golden.npz"))
    feats = gm["ref_chunks"].reshape(-1, 80, 16).astype(np.float32)
    B = 16
    # script: ("call", session) | ("jump", session, new index) | ("release", bank) | ("start", session, bank, index)
    script = [("start", "a", 0, 0), ("start", "b", 0, 5), ("start", "c", 1, 2)]
    script += [("call", s) for _ in range(6) for s in "abc"]
    script += [("jump", "b", 3)] + [("call", s) for _ in range(4) for s in "abc"]
    script += [("release", 1), ("start", "d", 2, 1)] + [("call", s) for _ in range(5) for s in "abd"]
    n_calls = sum(1 for st in script if st[0] == "call")
    starts = 3 + 1 + 1          # three sessions, the jump, the new session: two misses each
    mels = [torch.from_numpy(np.roll(feats, 3 * k, axis=0)[:B].copy() * (1.0 - 0.004 * k)).cuda() for k in range(n_calls)]
    eng = Engine(0)
    try:
        eng.load_wav2lip(synth.wav2lip_state_dict(1234), max_frames=32)

        def run_all():
            aids = {}
            sess = {}
            outs = []
            k = 0
            for st in script:
                if st[0] == "start":
                    _, name, bank, index = st
                    if bank not in aids:
                        fr, fa, co = banks[bank]
                        aids[bank] = eng.register_avatar(fa, fr, co)
                    sess[name] = [bank, index]
                elif st[0] == "jump":
                    sess[st[1]][1] = st[2]
                elif st[0] == "release":
                    eng.release_avatar(aids.pop(st[1]))
                    for name in [n for n, v in sess.items() if v[0] == st[1]]:
                        del sess[name]
                else:
                    bank, index = sess[st[1]]
                    pred = torch.zeros(B, 256, 256, 3, dtype=torch.uint8, device="cuda")
                    eng.wav2lip_infer([(aids[bank], index, B, mels[k].data_ptr(), pred.data_ptr())])
                    outs.append(pred.cpu())
                    sess[st[1]][1] = index + B
                    k += 1
            for a in aids.values():
                eng.release_avatar(a)
            return outs

        try:
            Engine.set_knob("PREFETCH", 0)
            whole = run_all()
            st0 = eng.prefetch_stats()
            Engine.set_knob("PREFETCH", 1)
            piped = run_all()
            st = eng.prefetch_stats()
            hits, misses = st["hits"] - st0["hits"], st["misses"] - st0["misses"]
            print(f"[prefetch slots] {n_calls} calls of 3 interleaved sessions: hits {hits}, misses {misses} ({100.0 * hits / n_calls:.1f} % of all calls)")
            for k in range(n_calls):
                assert torch.equal(piped[k], whole[k]), f"call {k}: max diff {int((piped[k].to(torch.int16) - whole[k].to(torch.int16)).abs().max())} LSB"
            assert misses == 2 * starts and hits == n_calls - 2 * starts, (hits, misses)
        finally:
            Engine.set_knob("PREFETCH", 1)
    finally:
        eng.close()


@pytest.mark.gpu
@pytest.mark.parametrize("graph", [1, 0])
def test_prefetched_face_encoder_equals_whole_pass(golden_dir, graph):
    """Knob PREFETCH (default on): a session's consecutive single-request calls are pipelined across calls - the face encoder of
    the frames call N+1 will ask for runs beside call N's decoder on a third stream into the other set of concat buffers
    (include/ltk.h ltk_wav2lip_prefetch_stats).  A sequence of calls as a session issues them (index += batch, across the bank's
    ping-pong turn), then a jump of the index (the prefetch is dropped), then the sequence resumed, with another avatar's call
    interleaved once: every call's frames must equal byte for byte the frames of the knob off, the counters must show that calls
    really started at the decoder, and the same with the pass replayed from graphs and launched eagerly."""
    from livetalking_amd.engine import Engine
    frames, faces, coords = synth.wav2lip_avatar(n_frames=20, full_hw=(180, 320), box=96, seed=4)
    frames2, faces2, coords2 = synth.wav2lip_avatar(n_frames=7, full_hw=(180, 320), box=96, seed=6)
    gm = np.load(os.path.join(golden_dir, "mel_golden.npz"))
    feats = gm["ref_chunks"].reshape(-1, 80, 16).astype(np.float32)
    B = 16
    # (avatar, index): nine consecutive steps of avatar 0 (20 bank frames: several ping-pong turns), a jump, three more, the other
    # avatar once, then avatar 0 continuing where it was
    seq = [(0, B * k) for k in range(9)] + [(0, 7), (0, 7 + B), (0, 7 + 2 * B), (1, 3), (0, 7 + 3 * B), (0, 7 + 4 * B), (0, 7 + 5 * B)]
    eng = Engine(0)
    try:
        Engine.set_knob("GRAPH", graph)
        eng.load_wav2lip(synth.wav2lip_state_dict(1234), max_frames=32)
        aids = [eng.register_avatar(faces, frames, coords), eng.register_avatar(faces2, frames2, coords2)]
        mels = [torch.from_numpy(np.roll(feats, 3 * k, axis=0)[:B].copy() * (1.0 - 0.01 * k)).cuda() for k in range(len(seq))]

        def run_all():
            outs = []
            for k, (av, index) in enumerate(seq):
                pred = torch.zeros(B, 256, 256, 3, dtype=torch.uint8, device="cuda")
                eng.wav2lip_infer([(aids[av], index, B, mels[k].data_ptr(), pred.data_ptr())])
                outs.append(pred.cpu())
            return outs

        try:
            Engine.set_knob("PREFETCH", 0)
            whole = run_all()
            st0 = eng.prefetch_stats()
            assert st0["hits"] == 0 and st0["issued"] == 0
            Engine.set_knob("PREFETCH", 1)
            piped = run_all()
            st = eng.prefetch_stats()
            print(f"[prefetch, graph={graph}] {st}")
            # hits: steps 2..8 of the first run (7), steps 2 and 3 after the jump... the call after the foreign avatar misses, then two hits
            assert st["hits"] >= 9 and st["issued"] >= st["hits"] and st["misses"] >= 4
            for k in range(len(seq)):
                assert torch.equal(piped[k], whole[k]), f"call {k} {seq[k]}: max diff {int((piped[k].to(torch.int16) - whole[k].to(torch.int16)).abs().max())} LSB"
            assert not torch.equal(whole[0], whole[1])
        finally:
            Engine.set_knob("PREFETCH", 1)
            Engine.set_knob("GRAPH", 1)
    finally:
        eng.close()
