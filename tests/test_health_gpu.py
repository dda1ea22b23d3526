"""GPU: the fp16 headroom watch (include/ltk.h: ltk_health_watch / ltk_health_report / ltk_health_scan).

1. the scan kernel alone against the numpy model of tests/health_cases.py: integers equal, max_abs bit-equal;
2. Wav2Lip: one layer's BatchNorm affine scaled past the fp16 range (asserted on the oracle first), two watched calls of five: the
   planted layer is named, the layers before it are clean, max_abs is the tap's, the frames are byte-identical to an unwatched
   engine's, and the graph / prefetch counters behind the window move as a fresh session's do; output_block.0 is observed with the
   head unfused (HEAD_FUSED = 0) and only then;
3. MuseTalk (B = 1), fp16 and fp8; 4. Ultralight with UL_FUSE_IR off and on, two avatars; 5. Whisper and HuBERT, single and batched;
6. refusals and lifetime.
"""
import numpy as np
import pytest

torch = pytest.importorskip("torch")

import health_cases as HC  # noqa: E402
import synth_inputs as synth  # noqa: E402

pytestmark = pytest.mark.gpu

INT_FIELDS = ("elements", "at_limit", "near_limit", "nonfinite")


@pytest.fixture(scope="module")
def eng():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from livetalking_amd.engine import Engine
    e = Engine(0)
    yield e
    e.close()


def _bits(x):
    return np.array([x], dtype=np.float32).view(np.uint32)[0]


# ------------------------------------------------------------------ 1. the kernel alone
@pytest.mark.parametrize("q8", [False, True], ids=["fp16", "e4m3"])
@pytest.mark.parametrize("shape", HC.KERNEL_SHAPES, ids=lambda s: "N%d-cbt%d-cb%d+%d-P%d" % s)
def test_scan_kernel_against_the_numpy_model(eng, shape, q8):
    N, cbt, cb0, CB, P = shape
    codes = HC.build_tensor(N, cbt, cb0, CB, P, q8, seed=7 + P)
    want = HC.scan_model(codes, cb0, CB, q8)
    assert want["at_limit"] >= 1 and want["nonfinite"] >= 1                      # the planted values are in the view
    d = torch.from_numpy(codes.view(np.int16) if not q8 else codes).cuda()
    torch.cuda.synchronize()
    got = eng.health_scan(d.data_ptr(), N, cbt, cb0, CB, P, q8)
    print(f"[health scan] {shape} q8={int(q8)}: got {got}  want {want}")
    for k in INT_FIELDS:
        assert got[k] == want[k], (k, got[k], want[k])
    assert _bits(got["max_abs"]) == _bits(want["max_abs"]), (got["max_abs"], want["max_abs"])
    assert got["limit"] == want["limit"] and got["q8"] == want["q8"] and got["observed"] == 1


def test_scan_of_a_clean_tensor_and_subnormals(eng):
    x = np.zeros((1, 1, 3, 16), dtype=np.uint16)
    x[0, 0, 1, 4] = 0x8003                                   # a negative fp16 subnormal is the largest magnitude
    got = eng.health_scan(torch.from_numpy(x.view(np.int16)).cuda().data_ptr(), 1, 1, 0, 1, 3, False)
    assert [got[k] for k in INT_FIELDS] == [48, 0, 0, 0]
    assert _bits(got["max_abs"]) == _bits(HC.decode_f16(0x0003))


# ------------------------------------------------------------------ 2. Wav2Lip
def _w2l_inputs(B, calls):
    from oracle import mel_oracle
    frames, faces, coords = synth.wav2lip_avatar(n_frames=5, full_hw=(360, 640), box=160, seed=0)
    audio = synth.synthetic_audio(2.0)
    n_chunks = 20 + 2 * B * calls
    mel = np.stack(mel_oracle.mel_chunks(audio[: n_chunks * 320], n_chunks))[: B * calls].astype(np.float32)
    return frames, faces, coords, mel.reshape(calls, B, 80, 16)


def test_wav2lip_watch_names_the_planted_layer_and_leaves_the_frames_alone():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from livetalking_amd.engine import Engine
    from oracle import plugin_oracle, wav2lip_oracle as W
    B, CALLS, WATCHED = 2, 5, 2
    frames, faces, coords, mel = _w2l_inputs(B, CALLS)
    sd_np = synth.wav2lip_state_dict(1234)
    # the oracle first: the affine of ONE layer times PLANT_SCALE (its output is linear in it: a non-residual layer, ReLU behind)
    taps, shapes = {}, {}
    with torch.no_grad():
        for c in range(WATCHED):
            t = {}
            mel_t, img_t = plugin_oracle.pack_inputs(faces, c * B, B, list(mel[c]))
            W.forward({k: torch.from_numpy(np.asarray(v)) for k, v in sd_np.items()}, mel_t, img_t, t)
            for k, v in t.items():
                taps[k] = max(taps.get(k, 0.0), float(v.abs().max()))
                shapes[k] = tuple(v.shape)
    order = list(taps)
    at = order.index(HC.W2L_PLANTED)
    assert taps[HC.W2L_PLANTED] * HC.PLANT_SCALE >= 4 * 65504.0, taps[HC.W2L_PLANTED]
    assert max(taps[k] for k in order[:at]) <= 65504.0 / 4
    for leaf in ("weight", "bias"):
        k = f"{HC.W2L_PLANTED}.conv_block.1.{leaf}"
        sd_np[k] = (sd_np[k] * np.float32(HC.PLANT_SCALE)).astype(np.float32)

    def session(watch):
        e = Engine(0)
        out, ctr = [], []
        try:
            e.load_wav2lip(sd_np, max_frames=4)
            aid = e.register_avatar(faces, frames, coords)
            if watch:
                e.health_watch("wav2lip", WATCHED)
            for c in range(CALLS):
                d_mel = torch.from_numpy(mel[c]).cuda()
                d_pred = torch.zeros(B, 256, 256, 3, dtype=torch.uint8, device="cuda")
                torch.cuda.synchronize()
                e.wav2lip_infer([(aid, c * B, B, d_mel.data_ptr(), d_pred.data_ptr())])
                out.append(d_pred.cpu().numpy())
                ctr.append((e.graph_count(), tuple(sorted(e.prefetch_stats().items()))))
            rep = e.health_report("wav2lip") if watch else None
            tap_max = {}
            if not watch:                                   # the same two calls once more with every layer captured
                e.debug_capture(True)
                for c in range(WATCHED):
                    d_mel = torch.from_numpy(mel[c]).cuda()
                    d_pred = torch.zeros(B, 256, 256, 3, dtype=torch.uint8, device="cuda")
                    torch.cuda.synchronize()
                    e.wav2lip_infer([(aid, c * B, B, d_mel.data_ptr(), d_pred.data_ptr())])
                    for name in HC.W2L_EARLIER:
                        tap = e.debug_get(name, shapes[name])
                        tap_max[name] = max(tap_max.get(name, 0.0), float(np.abs(tap).max()))
                e.debug_capture(False)
            return out, ctr, rep, tap_max
        finally:
            e.close()

    got, ctr_w, (ops, seen, left), _ = session(True)
    ref, ctr_u, _, tap_max = session(False)
    names = [o["name"] for o in ops]
    print(f"[health w2l] seen {seen} left {left}; counters watched {ctr_w}; unwatched {ctr_u}")
    for o in ops:
        print(f"[health w2l] {o}")
    assert seen == WATCHED and left == 0
    assert names[-1] == "output_block.0" and ops[-1]["observed"] == 0 and ops[-1]["elements"] == 0      # inside the fused head
    assert set(order) == set(names)
    planted = ops[names.index(HC.W2L_PLANTED)]
    assert planted["observed"] == 1 and planted["at_limit"] > 0 and planted["max_abs"] == 65504.0
    for k in order[:at]:
        o = ops[names.index(k)]
        assert o["observed"] == 1 and o["at_limit"] == 0 and o["nonfinite"] == 0 and o["elements"] > 0, o
    for name, m in tap_max.items():
        assert ops[names.index(name)]["max_abs"] == m, (name, ops[names.index(name)]["max_abs"], m)
    assert set(tap_max) == set(HC.W2L_EARLIER)
    for c in range(CALLS):
        assert np.array_equal(got[c], ref[c]), f"call {c}: a watched session's frames differ from the unwatched session's"
    # behind the window the graph cache and the prefetch slots are where a fresh session's are: call WATCHED + k against call k
    base = ctr_w[WATCHED - 1]
    assert base[0] == 0 and all(v == 0 for _, v in base[1]), base
    for k in range(CALLS - WATCHED):
        assert ctr_w[WATCHED + k] == ctr_u[k], (k, ctr_w[WATCHED + k], ctr_u[k])
    assert ctr_u[CALLS - WATCHED - 1][0] >= 1 and dict(ctr_u[CALLS - WATCHED - 1][1])["hits"] >= 1      # ... and that is a session that captures and hits


def test_wav2lip_watch_sees_output_block_0_only_with_the_head_unfused():
    """The one layer whose coverage depends on a knob: under HEAD_FUSED = 0 the 32-channel map of output_block.0 is in memory and
    scanned (B x 32 x 256 x 256 values); in the fused head it never is, and the report says so.  Every other layer is observed on
    both routes.  tests/test_parity_stress_gpu.py relies on the first to scan every layer."""
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from livetalking_amd.engine import Engine
    frames, faces, coords, mel = _w2l_inputs(1, 1)
    e = Engine(0)
    try:
        e.load_wav2lip(synth.wav2lip_state_dict(1234), max_frames=2)
        aid = e.register_avatar(faces, frames, coords)
        d_mel = torch.from_numpy(mel[0]).cuda()
        d_pred = torch.zeros(1, 256, 256, 3, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        for fused in (0, 1):
            e.health_watch("wav2lip", 1)
            Engine.set_knob("HEAD_FUSED", fused)
            try:
                e.wav2lip_infer([(aid, 0, 1, d_mel.data_ptr(), d_pred.data_ptr())])
            finally:
                Engine.set_knob("HEAD_FUSED", 1)
            ops, seen, left = e.health_report("wav2lip")
            assert (seen, left) == (1, 0) and ops[-1]["name"] == "output_block.0"
            assert all(o["observed"] == 1 and o["elements"] > 0 for o in ops[:-1]), [o["name"] for o in ops[:-1] if o["observed"] != 1]
            if fused:
                assert ops[-1]["observed"] == 0 and ops[-1]["elements"] == 0
            else:
                assert ops[-1]["observed"] == 1 and ops[-1]["elements"] == 32 * 65536
    finally:
        e.close()


# ------------------------------------------------------------------ 6. refusals and lifetime
def test_refusals_and_rearming(eng):
    from livetalking_amd._lib import LtkError
    for prog in ("wav2lip", "musetalk", "whisper", "hubert"):
        with pytest.raises(LtkError) as ei:
            eng.health_watch(prog, 1)
        assert ei.value.code == -3, prog
    with pytest.raises(LtkError) as ei:
        eng.health_watch("ultralight", 1, avatar_id=12345)
    assert ei.value.code == -3
    with pytest.raises(LtkError) as ei:
        eng.health_report("wav2lip")
    assert ei.value.code == -3
    x = torch.zeros(1, 2, 4, 16, dtype=torch.float16, device="cuda")
    # a live engine: the program and the call count are refused on their own, before the "not loaded" state is looked at
    for prog, calls in ((99, 1), (-1, 1), (5, 1), (0, -1), (3, -7)):
        with pytest.raises(LtkError) as ei:
            eng.health_watch(prog, calls)
        assert ei.value.code == -1, (prog, calls)
    with pytest.raises(LtkError) as ei:
        eng.health_report(99)
    assert ei.value.code == -1
    for bad in ((1, 2, 1, 2, 4), (1, 2, 0, 0, 4), (0, 2, 0, 1, 4), (1, 2, -1, 1, 4), (1, 2, 0, 1, 0)):
        with pytest.raises(LtkError) as ei:
            eng.health_scan(x.data_ptr(), *bad)
        assert ei.value.code == -1, bad


def test_rearming_zeroes_and_a_small_buffer_is_refused():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import ctypes as C
    from livetalking_amd import _lib
    from livetalking_amd.engine import Engine
    enc = synth.whisper_encoder_state_dict()
    pcm = synth.synthetic_audio(1.0)[:9600]
    e = Engine(0)
    try:
        e.load_whisper(enc)
        out = torch.zeros(2, 50, 384, device="cuda")
        e.health_watch("whisper", 1)
        e.whisper_step(pcm, 2, 2, out.data_ptr())
        e.whisper_step(pcm, 2, 2, out.data_ptr())               # behind the window: not counted
        ops, seen, left = e.health_report("whisper")
        assert (seen, left) == (1, 0) and sum(o["elements"] for o in ops) > 0
        first = [o["elements"] for o in ops]
        ops2 = (_lib.HealthOp * 2)()
        n = C.c_int()
        rc = e._lib.ltk_health_report(e._h, _lib.HEALTH_WHISPER, -1, ops2, 2, C.byref(n), None, None)
        assert rc == -1 and n.value == len(ops) > 2
        e.health_watch("whisper", 3)                            # armed again: the counters start from zero
        ops, seen, left = e.health_report("whisper")
        assert (seen, left) == (0, 3) and all(o["elements"] == 0 and o["observed"] == 0 and o["max_abs"] == 0.0 for o in ops)
        e.whisper_step(pcm, 2, 2, out.data_ptr())
        e.health_watch("whisper", 0)                            # disarmed: what was counted stays
        e.whisper_step(pcm, 2, 2, out.data_ptr())
        ops, seen, left = e.health_report("whisper")
        assert (seen, left) == (1, 0) and [o["elements"] for o in ops] == first
    finally:
        e.close()


# ------------------------------------------------------------------ 5. Whisper and HuBERT
def _dirty(ops):
    return [o["name"] for o in ops if o["at_limit"] or o["nonfinite"]]


def test_whisper_watch_single_and_batched_and_a_planted_layer():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from livetalking_amd.engine import Engine
    enc = synth.whisper_encoder_state_dict()
    pcm = synth.synthetic_audio(1.0)[:9600]
    e = Engine(0)
    try:
        e.load_whisper(enc)
        out = torch.zeros(2, 2, 50, 384, device="cuda")
        g0 = e.program_graph_count()
        e.health_watch("whisper", 1)
        e.whisper_step(pcm, 2, 2, out[0].data_ptr())
        single, seen, _ = e.health_report("whisper")
        assert seen == 1 and e.program_graph_count() == g0
        print("[health whisper]", [(o["name"], o["observed"], o["elements"], o["max_abs"]) for o in single])
        assert all(o["at_limit"] == 0 and o["near_limit"] == 0 and o["nonfinite"] == 0 for o in single)
        assert all(o["elements"] > 0 for o in single if o["observed"]) and sum(o["observed"] for o in single) >= len(single) - 1
        by = {o["name"]: o for o in single}
        for name, shape in (("conv1", (384, 3000)), ("layers.0.self_attn.out_proj", (384, 1500))):
            tap = e.whisper_debug_get(name, shape)
            assert by[name]["max_abs"] == float(np.abs(tap).max()), name
        e.health_watch("whisper", 1)
        e.whisper_step_batch([(pcm, 2, 2, 2, 10, out[0].data_ptr()), (pcm, 2, 2, 2, 10, out[1].data_ptr())])
        both, seen, left = e.health_report("whisper")
        assert (seen, left) == (1, 0)                           # one engine call, whatever it carries
        for a, b in zip(single, both):          # (the 16-clip program takes other kernel routes: its values may differ in the last bits)
            assert b["elements"] == 2 * a["elements"] and b["observed"] == a["observed"], (a, b)
            assert b["at_limit"] == 0 and b["nonfinite"] == 0
        assert torch.equal(out[0], out[1])
    finally:
        e.close()
    bad = dict(enc)
    bad["conv1.weight"] = (bad["conv1.weight"] * np.float32(1e6)).astype(np.float32)
    bad["conv1.bias"] = (bad["conv1.bias"] * np.float32(1e6)).astype(np.float32)
    e = Engine(0)
    try:
        e.load_whisper(bad)
        out = torch.zeros(2, 50, 384, device="cuda")
        e.health_watch("whisper", 1)
        e.whisper_step(pcm, 2, 2, out.data_ptr())
        ops, _, _ = e.health_report("whisper")
        assert _dirty(ops)[0] == "conv1", _dirty(ops)[:4]
    finally:
        e.close()


def test_hubert_watch_single_and_batched_and_a_planted_layer():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import hubert_ref as H
    from livetalking_amd.engine import Engine
    sd = H.state_dict(2, 20)
    n = 16640
    pcm = H.speech(n, 9)
    T = H.rows(n)
    e = Engine(0)
    try:
        e.load_hubert(sd)
        out = torch.zeros(2, 2, 16, 1024, device="cuda")
        e.health_watch("hubert", 1)
        e.hubert_step(pcm, 2, 0, out[0].data_ptr())
        single, seen, _ = e.health_report("hubert")
        print("[health hubert]", [(o["name"], o["observed"], o["elements"], o["max_abs"]) for o in single])
        assert seen == 1 and [o["name"] for o in single] == H.op_names(2)
        assert all(o["at_limit"] == 0 and o["nonfinite"] == 0 for o in single)
        by = {o["name"]: o for o in single}
        for name, C_ in (("feature_projection.projection", 1024), ("feature_extractor.conv_layers.6.conv", 512), ("encoder.layer_norm", 1024)):
            tap = e.hubert_debug_get(name, (C_, T))
            assert by[name]["observed"] == 1 and by[name]["max_abs"] == float(np.abs(tap).max()), name
        e.health_watch("hubert", 1)
        e.hubert_step_batch([(pcm, 2, 0, 2, 16, out[0].data_ptr()), (pcm, 2, 0, 2, 16, out[1].data_ptr())])
        both, seen, left = e.health_report("hubert")
        assert (seen, left) == (1, 0) and e.hubert_batch_info()["programs"] == 1      # the batched program counted into the same table
        for a, b in zip(single, both):
            assert b["elements"] == 2 * a["elements"] and b["observed"] == a["observed"], (a, b)
    finally:
        e.close()
    bad = dict(sd)
    p = "feature_extractor.conv_layers.2.conv"
    bad[p + ".weight"] = (np.asarray(bad[p + ".weight"]) * np.float32(1e6)).astype(np.float32)
    e = Engine(0)
    try:
        e.load_hubert(bad)
        out = torch.zeros(2, 16, 1024, device="cuda")
        e.health_watch("hubert", 1)
        e.hubert_step(pcm, 2, 0, out.data_ptr())
        ops, _, _ = e.health_report("hubert")
        assert _dirty(ops)[0] == p, _dirty(ops)[:4]
    finally:
        e.close()


# ------------------------------------------------------------------ 4. Ultralight
UL_BLOCK = "down1.maxpool_conv.0.double_conv.1"          # an inverted residual that ul_ir_kernel takes under knob UL_FUSE_IR


def test_ultralight_watch_per_avatar_fused_and_unfused():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from livetalking_amd._lib import LtkError
    from livetalking_amd.engine import Engine
    sd = synth.ultralight_state_dict(1234)
    bad = dict(sd)
    for leaf in ("weight", "bias"):                          # the expand conv's BatchNorm affine
        bad[f"{UL_BLOCK}.conv.1.{leaf}"] = (bad[f"{UL_BLOCK}.conv.1.{leaf}"] * np.float32(1e5)).astype(np.float32)
    frames, faces, coords = synth.ultralight_avatar(3, (96, 128), seed=11)
    feat = torch.from_numpy(synth.ultralight_feats(1, 30).reshape(1, 16, 32, 32)).cuda()
    e = Engine(0)
    try:
        a = e.register_ultralight_avatar(bad, faces, frames, coords, max_frames=2)
        b = e.register_ultralight_avatar(sd, faces, frames, coords, max_frames=2)
        frames_by_knob = {}
        for knob in (0, 1):
            Engine.set_knob("UL_FUSE_IR", knob)
            try:
                ref = torch.zeros(1, 160, 160, 3, dtype=torch.uint8, device="cuda")
                e.ultralight_infer([(a, 0, 1, feat.data_ptr(), ref.data_ptr())])          # unwatched
                g0 = e.program_graph_count()
                e.health_watch("ultralight", 1, avatar_id=a)
                got = torch.zeros_like(ref)
                e.ultralight_infer([(a, 0, 1, feat.data_ptr(), got.data_ptr()), (b, 0, 1, feat.data_ptr(), torch.zeros_like(ref).data_ptr())])
                assert torch.equal(got, ref) and e.program_graph_count() >= g0
                ops, seen, left = e.health_report("ultralight", a)
                names = [o["name"] for o in ops]
                assert (seen, left) == (1, 0) and len(ops) == e._lib.ltk_ultralight_op_count(e._h, a) == (60 if knob else 86)
                assert names == [nm for nm, _ in e.ultralight_ops(a)]
                dirty = _dirty(ops)
                print(f"[health ul] knob {knob}: dirty {dirty[:4]}")
                if knob == 0:
                    assert dirty[0] == UL_BLOCK + ".conv.0"
                    assert all(o["observed"] == 1 for o in ops if o["type"] != 14) and ops[-1]["observed"] == 0      # the head writes bytes
                else:
                    assert UL_BLOCK + ".conv.0" not in names and UL_BLOCK + ".conv.3" not in names
                    blk = ops[names.index(UL_BLOCK + ".conv.6")]
                    assert blk["type"] == 15 and blk["observed"] == 1 and blk["elements"] > 0
                    # the hidden tensors that overflow stay inside the kernel: the watch sees what the block lets out, and the first
                    # op it names is the block or one behind it
                    assert dirty and names.index(dirty[0]) >= names.index(UL_BLOCK + ".conv.6")
                ops_b, seen_b, _ = e.health_report("ultralight", b)
                assert seen_b == 0 and all(o["elements"] == 0 and o["observed"] == 0 for o in ops_b)
                frames_by_knob[knob] = got.cpu().numpy()
            finally:
                Engine.set_knob("UL_FUSE_IR", 0)
        # a released avatar takes its table with it: its id is unknown to the watch from then on
        e.release_avatar(a)
        with pytest.raises(LtkError) as ei:
            e.health_report("ultralight", a)
        assert ei.value.code == -3
        ops_b, _, _ = e.health_report("ultralight", b)
        assert len(ops_b) == 86
        e.release_avatar(b)
    finally:
        e.close()


# ------------------------------------------------------------------ 3. MuseTalk
MT_PLANTED = "decoder.conv_in"          # the VAE decoder's first conv: its output is a tap of the oracle (peak 5.5 at gain 1)
MT_EARLIER = "conv_in"                  # the U-Net's first conv


def _mt_avatar(eng):
    lats = synth.musetalk_latents(1)
    frames, _, _ = synth.wav2lip_avatar(n_frames=1, full_hw=(360, 640), box=160, seed=2)
    x1, y1, x2, y2 = 240, 100, 390, 270
    xs, ys, xe, ye = x1 - 30, y1 - 40, x2 + 30, y2 + 35
    mask = np.full((ye - ys, xe - xs, 3), 255, np.uint8)
    return lats, eng.register_musetalk_avatar(lats, frames, [(x1, y1, x2, y2)], [mask], [(xs, ys, xe, ye)])


def test_musetalk_watch_names_the_planted_vae_conv():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from livetalking_amd.engine import Engine
    from oracle import musetalk_oracle as M
    unet_sd = synth.musetalk_unet_state_dict(4321)
    vae_sd = synth.vae_decoder_state_dict(987)
    lat = np.concatenate(synth.musetalk_latents(1))
    feat = synth.musetalk_whisper_feats(1, seed=21)
    taps, vtaps = {}, {}
    with torch.no_grad():
        ref_lat = M.unet_forward({k: torch.from_numpy(v) for k, v in unet_sd.items()}, torch.from_numpy(lat),
                                 M.positional_encoding(torch.from_numpy(feat)), taps=taps, detail="")
        M.vae_decode({k: torch.from_numpy(v) for k, v in vae_sd.items()}, ref_lat / M.VAE_SCALING, vtaps)
    vorder = list(vtaps)
    at = vorder.index(MT_PLANTED)
    # the conv's output is linear in its weight and bias: the oracle at scale 1 times the scale
    assert float(vtaps[MT_PLANTED].abs().max()) * 1e5 >= 4 * 65504.0
    before = [float(t.abs().max()) for t in taps.values()] + [float(vtaps[k].abs().max()) for k in vorder[:at]]
    assert max(before) <= 65504.0 / 4
    for leaf in ("weight", "bias"):
        vae_sd[f"{MT_PLANTED}.{leaf}"] = (vae_sd[f"{MT_PLANTED}.{leaf}"] * np.float32(1e5)).astype(np.float32)
    d_feat = torch.from_numpy(feat).cuda()

    # one engine (a MuseTalk load is seconds): two unwatched calls (eager, then captured), two watched, two unwatched, all on the same
    # inputs - every call's frames must be the same bytes, and the graph cache must not move inside the window
    e = Engine(0)
    try:
        e.load_musetalk(unet_sd, vae_sd, max_frames=1)
        _, aid = _mt_avatar(e)
        out, ctr = [], []
        for c in range(6):
            if c == 2:
                e.health_watch("musetalk", 2)
            d_pred = torch.zeros(1, 256, 256, 3, dtype=torch.uint8, device="cuda")
            torch.cuda.synchronize()
            e.musetalk_infer([(aid, 0, 1, d_feat.data_ptr(), d_pred.data_ptr())])
            out.append(d_pred.cpu().numpy())
            ctr.append(e.program_graph_count())
        tap = float(np.abs(e.musetalk_debug_get(MT_EARLIER, tuple(taps[MT_EARLIER].shape))).max())
        ops, seen, left = e.health_report("musetalk")
    finally:
        e.close()
    names = [o["name"] for o in ops]
    print(f"[health mt] graphs {ctr}; dirty {_dirty(ops)[:3]}")
    assert (seen, left) == (2, 0)
    p = names.index(MT_PLANTED)
    assert ops[p]["at_limit"] > 0 and ops[p]["observed"] == 1
    assert all(o["at_limit"] == 0 and o["nonfinite"] == 0 for o in ops[:p]) and _dirty(ops)[0] == MT_PLANTED
    assert ops[names.index(MT_EARLIER)]["max_abs"] == tap
    for c in range(1, 6):
        assert np.array_equal(out[c], out[0]), c
    assert ctr == [0, 1, 1, 1, 1, 1]                        # captured at its second sight; the window neither drops nor adds a graph


def test_musetalk_fp8_ops_report_the_e4m3_limit_and_match_the_tensor():
    """The fp8 conv path at an activation scale that puts values into e4m3's top binade (GroupNorm + SiLU outputs of a few units
    times 64).  Every e4m3 op reports limit 448; the LAST one of the program (no later op writes its buffer) is read back as raw codes
    through ltk_musetalk_debug_get_q8 - a host-side walk of the view, nothing of the scan's - and the numpy model of those codes
    must give the record: elements, near_limit, at_limit, nonfinite equal, max_abs bit-equal."""
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from livetalking_amd.engine import Engine
    e = Engine(0)
    try:
        e.load_musetalk(synth.musetalk_unet_state_dict(11), synth.vae_decoder_state_dict(12), max_frames=1, fp8=True, fp8_act_scale=64.0)
        _, aid = _mt_avatar(e)
        d_feat = torch.from_numpy(synth.musetalk_whisper_feats(1, seed=21)).cuda()
        d_pred = torch.zeros(1, 256, 256, 3, dtype=torch.uint8, device="cuda")
        e.health_watch("musetalk", 1)
        e.musetalk_infer([(aid, 0, 1, d_feat.data_ptr(), d_pred.data_ptr())])
        ops, seen, _ = e.health_report("musetalk")
        q8 = [o for o in ops if o["q8"]]
        assert seen == 1 and len(q8) > 10 and any(not o["q8"] for o in ops)
        codes = {float(HC.decode_e4m3(c)) for c in range(0x7F)}
        for o in q8:
            assert o["limit"] == 448.0 and o["type"] == 1 and o["observed"] == 1 and o["elements"] > 0, o      # GroupNorm + SiLU writes the e4m3 tensors
            assert o["nonfinite"] == 0 and o["at_limit"] <= o["near_limit"] <= o["elements"] and o["max_abs"] in codes, o
        last = q8[-1]
        raw = e.musetalk_debug_get_q8(last["name"], (1, last["elements"]))
        want = HC.scan_model(raw.reshape(1, 1, -1, 32), 0, 1, True)
        print(f"[health fp8] {last}  tensor: {want}")
        assert want["near_limit"] > 0 and want["at_limit"] > 0, "the act scale no longer reaches e4m3's top binade: raise it"
        for k in INT_FIELDS:
            assert last[k] == want[k], (k, last[k], want[k])
        assert _bits(last["max_abs"]) == _bits(want["max_abs"])
    finally:
        e.close()
