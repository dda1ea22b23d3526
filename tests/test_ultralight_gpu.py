"""GPU tests of the Ultralight avatar: the depthwise and upsample kernels against torch float64, every layer of the launch
program against tests/ultralight_ref.py, frames against float64 with the fp16 rounding model of the reference as the
yardstick, the bank gather path, paste-back, the plugin and avatar release.  Engine of its own (module scope)."""
from __future__ import annotations

import os
import pickle
import sys
import types

import numpy as np
import pytest

import synth_inputs as synth
import ultralight_ref as ref

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FULL_HW = (120, 200)


@pytest.fixture(scope="module")
def eng():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from livetalking_amd.engine import Engine
    e = Engine(0)
    yield e
    e.close()


@pytest.fixture(scope="module")
def sd():
    return synth.ultralight_state_dict(1234)


@pytest.fixture(scope="module")
def cpu_ref(sd):
    """ONE float64 forward (with taps) and ONE fp16-rounding-model forward of three frames, shared by the tests; the first two
    frames are the golden's inputs."""
    img6, feat = synth.ultralight_inputs(3, 1234)
    taps = {}
    pred = ref.forward(sd, img6, feat, taps=taps)
    model = ref.forward(sd, img6, feat, fp16_model=True)
    return types.SimpleNamespace(img6=img6, feat=feat, pred=pred, taps=taps, frames=ref.frames_u8(pred), model_frames=ref.frames_u8(model))


@pytest.fixture(scope="module")
def golden_avatar(eng, sd):
    """The golden's weights over a bank of the three faces the shared reference was computed from."""
    faces = synth.ultralight_faces(3, 1234)
    frames, _, coords = synth.ultralight_avatar(3, FULL_HW, seed=3)
    return eng.register_ultralight_avatar(sd, faces, frames, coords, max_frames=17)


# ------------------------------------------------------------------ depthwise kernel
@pytest.mark.parametrize("C", [16, 64])
@pytest.mark.parametrize("hw", [(5, 7), (10, 10), (33, 20)])
def test_dwconv3x3_against_float64(eng, C, hw):
    """Per element: one fp16 rounding of the result plus fp32 accumulation of 9 products and the affine:
    |d| <= 2^-10 |ref| + 2^-20 (sum |w x| |scale| + |shift|) + 2^-24.  Reference: torch float64 on the device's own fp16 inputs."""
    import torch
    import torch.nn.functional as F
    from livetalking_amd.layout import empty_cb16, from_cb16, to_cb16
    H, W = hw
    g = torch.Generator().manual_seed(C * 1000 + H * 10 + W)
    w = torch.randn(C, 1, 3, 3, generator=g) * 0.5
    scale = torch.rand(C, generator=g) * 1.5 + 0.2
    shift = torch.randn(C, generator=g) * 0.3
    for N in (1, 3):
        x = torch.randn(N, C, H, W, generator=g)
        x_cb = to_cb16(x.cuda())
        x16 = from_cb16(x_cb, C).double().cpu()            # what the kernel reads (border pixels are ordinary non-zero values)
        for stride in (1, 2):
            conv = F.conv2d(x16, w.double(), stride=stride, padding=1, groups=C)
            mag = F.conv2d(x16.abs(), w.double().abs(), stride=stride, padding=1, groups=C)
            lin = conv * scale.double()[None, :, None, None] + shift.double()[None, :, None, None]
            slack = 2.0 ** -20 * (mag * scale.double()[None, :, None, None] + shift.double().abs()[None, :, None, None]) + 2.0 ** -24
            Ho, Wo = conv.shape[2:]
            assert (Ho, Wo) == ((H - 1) // stride + 1, (W - 1) // stride + 1)
            for relu in (False, True):
                want = lin.clamp_min(0) if relu else lin
                y = empty_cb16(N, C, Ho, Wo, fill=7.0)
                eng.dwconv3x3_f16(x_cb.data_ptr(), N, H, W, C, w.numpy(), stride, scale.numpy(), shift.numpy(), relu, y.data_ptr())
                got = from_cb16(y, C).double().cpu()
                excess = ((got - want).abs() - (2.0 ** -10 * want.abs() + slack)).max().item()
                assert excess <= 0, f"N {N} stride {stride} relu {relu}: {excess:.3e} over the bound"


def test_dwconv3x3_pads_with_zeros_not_with_the_edge(eng):
    """Ones in, ones as weights: a pixel's value is the number of taps inside the map (4 in a corner, 6 on an edge, 9 inside); a
    clamped edge would give 9 everywhere."""
    import torch
    from livetalking_amd.layout import empty_cb16, from_cb16, to_cb16
    C, H, W = 16, 6, 9
    x_cb = to_cb16(torch.ones(2, C, H, W).cuda())
    for stride in (1, 2):
        Ho, Wo = (H - 1) // stride + 1, (W - 1) // stride + 1
        y = empty_cb16(2, C, Ho, Wo, fill=-1.0)
        eng.dwconv3x3_f16(x_cb.data_ptr(), 2, H, W, C, np.ones((C, 1, 3, 3), np.float32), stride, None, None, False, y.data_ptr())
        got = from_cb16(y, C).cpu().numpy()
        cnt = np.zeros((H, W))
        for yy in range(H):
            for xx in range(W):
                cnt[yy, xx] = (min(yy + 1, H - 1) - max(yy - 1, 0) + 1) * (min(xx + 1, W - 1) - max(xx - 1, 0) + 1)
        assert np.array_equal(got, np.broadcast_to(cnt[::stride, ::stride], got.shape)), f"stride {stride}"


# ------------------------------------------------------------------ upsample + concat
@pytest.mark.parametrize("C_up", [16, 48])
@pytest.mark.parametrize("hw", [(5, 3), (10, 10)])
def test_upsample2x_cat_against_float64(eng, C_up, hw):
    """|d| <= 2^-10 |ref| + 2^-24 against F.interpolate(align_corners=True) in float64 on the device's fp16 input; the skip half is
    a byte copy."""
    import torch
    import torch.nn.functional as F
    from livetalking_amd.layout import empty_cb16, from_cb16, to_cb16
    h, w = hw
    N, C_skip = 2, 16
    g = torch.Generator().manual_seed(C_up + h)
    x_cb = to_cb16(torch.randn(N, C_up, h, w, generator=g).cuda())
    s_cb = to_cb16(torch.randn(N, C_skip, 2 * h, 2 * w, generator=g).cuda())
    y = empty_cb16(N, C_up + C_skip, 2 * h, 2 * w, fill=3.0)
    eng.upsample2x_cat_f16(x_cb.data_ptr(), N, h, w, C_up, s_cb.data_ptr(), 2 * h, 2 * w, C_skip, y.data_ptr())
    want = F.interpolate(from_cb16(x_cb, C_up).double().cpu(), scale_factor=2, mode="bilinear", align_corners=True)
    got = from_cb16(y, C_up + C_skip).cpu()
    excess = ((got[:, :C_up].double() - want).abs() - (2.0 ** -10 * want.abs() + 2.0 ** -24)).max().item()
    assert excess <= 0, f"{excess:.3e} over the bound"
    assert torch.equal(y[:, C_up // 16:].cpu(), s_cb.cpu())


def test_upsample2x_cat_refuses_a_size_mismatch(eng):
    import torch
    from livetalking_amd._lib import LtkError
    from livetalking_amd.layout import empty_cb16
    x, s, y = empty_cb16(1, 16, 5, 3, fill=0.0), empty_cb16(1, 16, 10, 7, fill=0.0), empty_cb16(1, 32, 10, 7, fill=0.0)
    with pytest.raises(LtkError) as ex:
        eng.upsample2x_cat_f16(x.data_ptr(), 1, 5, 3, 16, s.data_ptr(), 10, 7, 16, y.data_ptr())
    assert ex.value.code == -1
    torch.cuda.synchronize()


# ------------------------------------------------------------------ every layer
def test_every_layer_tap_against_float64(eng, golden_avatar, cpu_ref):
    """B = 2 forward_host on the launch program, every launch's output against the float64 restatement: rel L2 <= 1e-2, the
    project's per-layer tolerance (tests/test_wav2lip_gpu.py)."""
    B = 2
    eng.debug_capture(True)
    try:
        pred = eng.ultralight_forward_host(golden_avatar, cpu_ref.img6[:B], cpu_ref.feat[:B])
        compared, worst = set(), (0.0, "")
        for name, t in cpu_ref.taps.items():
            want = t[:B]
            got = eng.debug_get(name, want.shape)
            rel = float(np.linalg.norm(got - want) / np.linalg.norm(want))
            worst = max(worst, (rel, name))
            assert rel <= 1e-2, f"{name}: rel L2 {rel:.3e}"
            compared.add(name)
    finally:
        eng.debug_capture(False)
    print(f"worst layer {worst[1]}: rel L2 {worst[0]:.3e}")
    assert np.abs(pred - cpu_ref.pred[:B]).max() <= 2e-2
    # coverage walk: every state_dict prefix that holds a conv was compared
    sd = synth.ultralight_state_dict(1234)
    convs = {k[:-len(".weight")] for k, v in sd.items() if k.endswith(".weight") and v.ndim == 4}
    assert len(convs) == 81 and convs <= compared, sorted(convs - compared)


# ------------------------------------------------------------------ frames
def _bank_order(n_bank, index, B):
    return [ref_mirror(n_bank, index + i) for i in range(B)]


def ref_mirror(size, index):
    turn, res = divmod(index, size)
    return res if turn % 2 == 0 else size - res - 1


@pytest.mark.parametrize("B", [1, 2, 3, 17])
def test_infer_frames_against_float64(eng, golden_avatar, cpu_ref, golden_dir, B):
    """ultralight_infer against float64.  Yardstick: the fp16 rounding model of the reference (weights and every BatchNorm /
    biased conv / upsample output rounded to fp16), computed on the CPU against the same float64 frames; the device may be at
    most 1 LSB worse in max error, 1.5 dB lower in PSNR and 1.5x the share of differing bytes, and never past the absolute floor
    2 LSB / 57.5 dB / 12 %.  B = 17 walks the three-face bank back and forth (frames repeat; the reference is per frame)."""
    import torch
    order = _bank_order(3, 0, B)
    d_feat = torch.from_numpy(np.ascontiguousarray(cpu_ref.feat[order])).cuda()
    d_pred = torch.zeros(B, 160, 160, 3, dtype=torch.uint8, device="cuda")
    eng.ultralight_infer([(golden_avatar, 0, B, d_feat.data_ptr(), d_pred.data_ptr())])
    got = d_pred.cpu().numpy()
    want = cpu_ref.frames[order]
    m_mx, m_psnr, m_share = ref.frame_stats(cpu_ref.model_frames[order], want)
    d_mx, d_psnr, d_share = ref.frame_stats(got, want)
    print(f"B {B}: model {m_mx} LSB {m_psnr:.2f} dB {m_share:.4f} | device {d_mx} LSB {d_psnr:.2f} dB {d_share:.4f}")
    assert d_mx <= m_mx + 1 and d_psnr >= m_psnr - 1.5 and d_share <= 1.5 * m_share
    assert d_mx <= 2 and d_psnr >= 57.5 and d_share < 0.12
    if B == 2:
        gold = np.load(os.path.join(golden_dir, "ultralight_golden.npz"))["frames"]
        g_mx, g_psnr, g_share = ref.frame_stats(got, gold)
        print(f"B 2 vs the reference's float32 frames: {g_mx} LSB {g_psnr:.2f} dB {g_share:.4f}")
        assert g_mx <= 2 and g_psnr >= 57.5 and g_share < 0.12


# ------------------------------------------------------------------ gather path
def test_infer_gathers_crops_masks_and_replays(eng, sd):
    """Two requests of different avatars (different weights) in one call, both crossing their bank's ping-pong boundary, against
    forward_host fed with host-built [4:164, 4:164] crops and the rectangle mask: <= 1 LSB on < 2 % of the bytes (two launch
    shapes of the same kernels).  The third call of a frame count replays a captured graph: byte-identical to the first."""
    import torch
    fa, faces_a, ca = synth.ultralight_avatar(5, FULL_HW, seed=11)
    fb, faces_b, cb = synth.ultralight_avatar(4, (96, 128), seed=12)
    a = eng.register_ultralight_avatar(sd, faces_a, fa, ca, max_frames=17)
    b = eng.register_ultralight_avatar(synth.ultralight_state_dict(7), faces_b, fb, cb, max_frames=8)
    try:
        reqs = [(a, 3, 4, faces_a), (b, 2, 3, faces_b)]            # bank frames 3, 4, 4, 3 and 2, 3, 3
        feats = [torch.from_numpy(synth.ultralight_feats(n, 30 + i).reshape(n, 16, 32, 32)).cuda() for i, (_, _, n, _) in enumerate(reqs)]
        preds = [torch.zeros(n, 160, 160, 3, dtype=torch.uint8, device="cuda") for _, _, n, _ in reqs]
        runs = []
        g0 = eng.program_graph_count()
        for _ in range(3):
            for p in preds:
                p.zero_()
            eng.ultralight_infer([(aid, idx, n, f.data_ptr(), p.data_ptr()) for (aid, idx, n, _), f, p in zip(reqs, feats, preds)])
            runs.append([p.cpu().numpy().copy() for p in preds])
        assert eng.program_graph_count() == g0 + 2                  # one captured pass per (avatar, frame count)
        for first, third in zip(runs[0], runs[2]):
            assert np.array_equal(first, third)
        for (aid, idx, n, faces), f, got in zip(reqs, feats, runs[0]):
            order = _bank_order(len(faces), idx, n)
            host = eng.ultralight_forward_host(aid, ref.img6_from_faces([faces[i] for i in order]), f.cpu().numpy())
            mx, _, share = ref.frame_stats(got, ref.frames_u8(host))
            assert mx <= 1 and share < 0.02, (mx, share)
        assert not np.array_equal(runs[0][0][0], runs[0][1][0])
        # the arena and an avatar's listing are the pure architecture's (Engine.ul_program: no GPU, no avatar)
        from livetalking_amd.engine import Engine
        assert eng.ultralight_info()["bytes_per_frame"] == 2 * sum(Engine.ul_program(0)["buf_halfs"])
        try:
            for knob in (0, 1):
                Engine.set_knob("UL_FUSE_IR", knob)
                assert eng.ultralight_ops(b) == [(o["name"], o["type"]) for o in Engine.ul_program(knob)["ops"]]
        finally:
            Engine.set_knob("UL_FUSE_IR", 0)
    finally:
        eng.release_avatar(a)
        eng.release_avatar(b)


# ------------------------------------------------------------------ paste-back
def test_paste_back_is_byte_exact(eng, sd):
    """Byte-exact against oracle.paste_oracle.resize_linear_u8 of the 168x168 composite (bank face, prediction at [4:164, 4:164])
    pasted at (x1, y1, x2, y2).  The cv2.resize leaf stays a RESTATEMENT of OpenCV's 8-bit bilinear path, as for Wav2Lip
    (oracle/paste_oracle.py: no OpenCV build here to pin it against).  Boxes: an odd size, one touching the frame's right and
    bottom edge, the identity size and the exact 2x shrink."""
    import torch
    from oracle import paste_oracle
    H, W = 200, 260
    frames, faces, _ = synth.ultralight_avatar(4, (H, W), seed=21)
    boxes = [(13, 9, 13 + 71, 9 + 93), (W - 100, H - 64, W, H), (20, 10, 20 + 168, 10 + 168), (20, 10, 20 + 84, 10 + 84)]
    aid = eng.register_ultralight_avatar(sd, faces, frames, boxes, max_frames=1)
    try:
        rng = np.random.default_rng(5)
        for idx, (x1, y1, x2, y2) in enumerate(boxes):
            pred = rng.integers(0, 256, (160, 160, 3), dtype=np.uint8)
            d_pred = torch.from_numpy(pred).cuda()
            out = np.empty((H, W, 3), np.uint8)
            eng.ultralight_paste_back(aid, idx, d_pred.data_ptr(), out)
            comp = faces[idx].copy()
            comp[4:164, 4:164] = pred
            want = frames[idx].copy()
            want[y1:y2, x1:x2] = paste_oracle.resize_linear_u8(comp, (x2 - x1, y2 - y1))
            assert np.array_equal(out, want), f"box {idx}: {(out != want).sum()} bytes differ"
    finally:
        eng.release_avatar(aid)


def test_register_refuses_bad_input(eng, sd):
    from livetalking_amd._lib import LtkError
    frames, faces, coords = synth.ultralight_avatar(2, FULL_HW, seed=1)
    with pytest.raises(LtkError) as ex:
        eng.register_ultralight_avatar(sd, faces, frames, [(0, 0, FULL_HW[1] + 1, 50), coords[1]])
    assert ex.value.code == -1 and "box" in str(ex.value)
    missing = {k: v for k, v in sd.items() if k != "audio_model.conv5.bias"}
    with pytest.raises(LtkError) as ex:
        eng.register_ultralight_avatar(missing, faces, frames, coords)
    assert ex.value.code == -1 and "audio_model.conv5" in str(ex.value)
    wrong = dict(sd)
    wrong["up3.conv.double_conv.0.conv.3.weight"] = np.zeros((128, 1, 3, 3), np.float32)
    with pytest.raises(LtkError) as ex:
        eng.register_ultralight_avatar(wrong, faces, frames, coords)
    assert ex.value.code == -1 and "up3.conv.double_conv.0.conv.3" in str(ex.value)


# ------------------------------------------------------------------ plugin
def test_plugin_runs_from_an_avatar_directory(eng, sd, tmp_path, monkeypatch):
    """LightReal behind load_avatar from a directory in the reference's format (ultralight.pth via torch.save, face_imgs/,
    full_imgs/, coords.pkl); inference_batch + paste_back_frame equal the engine-level path."""
    import torch
    from PIL import Image
    from livetalking_amd import bank
    from livetalking_amd.avatars import ultralight_avatar as ul
    frames, faces, coords = synth.ultralight_avatar(3, FULL_HW, seed=31)
    adir = tmp_path / "data" / "avatars" / "ul1"
    os.makedirs(adir / "full_imgs"); os.makedirs(adir / "face_imgs")
    for i in range(3):                                   # cv2.imwrite stores BGR arrays as RGB files
        Image.fromarray(np.ascontiguousarray(frames[i][..., ::-1])).save(adir / "full_imgs" / f"{i:08d}.png")
        Image.fromarray(np.ascontiguousarray(faces[i][..., ::-1])).save(adir / "face_imgs" / f"{i:08d}.png")
    with open(adir / "coords.pkl", "wb") as f:
        pickle.dump(coords, f)
    torch.save({k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()}, adir / "ultralight.pth")
    monkeypatch.chdir(tmp_path)
    # cv2 is not installed in this image: a stand-in whose imread has cv2.imread's semantics for 8-bit PNGs (BGR, 3 channels)
    monkeypatch.setitem(sys.modules, "cv2", types.SimpleNamespace(imread=bank._imread_bgr))
    avatar = ul.load_avatar("ul1")
    model, frame_list, face_list, coord_list = avatar
    assert all(np.array_equal(a, b) for a, b in zip(face_list, faces)) and list(map(tuple, coord_list)) == coords
    model.engine, model.max_frames = eng, 4                 # this module's engine instead of the process-wide one
    ul.warm_up(2, avatar, 160)

    class _Proc:
        def get_hubert_from_16k_speech(self, pcm):
            return np.zeros(((len(pcm) - 80) // 320, 1024), np.float32)

    B = 4
    opt = types.SimpleNamespace(fps=25, batch_size=B, l=10, r=10, sessionid=1)
    sess = ul.LightReal(opt, (_Proc(), None), avatar)
    try:
        chunks = list(synth.ultralight_feats(B, 40))             # (16, 1024) each, as HubertASR hands them over
        items = sess.inference_batch(2, chunks)                   # bank frames 2, 2, 1, 0
        assert len(items) == B and all(t.shape == (160, 160, 3) and t.dtype == torch.uint8 and t.is_cuda for t in items)
        d_feat = torch.from_numpy(np.stack(chunks).reshape(B, 16, 32, 32)).cuda()
        d_pred = torch.zeros(B, 160, 160, 3, dtype=torch.uint8, device="cuda")
        eng.ultralight_infer([(sess._aid, 2, B, d_feat.data_ptr(), d_pred.data_ptr())])
        assert torch.equal(torch.stack(items), d_pred)
        for i, idx in enumerate(_bank_order(3, 2, B)):
            frame = sess.paste_back_frame(items[i], idx)
            want = np.empty(FULL_HW + (3,), np.uint8)
            eng.ultralight_paste_back(sess._aid, idx, d_pred[i].data_ptr(), want)
            assert frame.flags.c_contiguous and frame.flags.writeable and np.array_equal(frame, want)
            assert not np.array_equal(frame, frames[idx])
    finally:
        model.release()


# ------------------------------------------------------------------ release
def test_release_then_register_again(eng, sd):
    import torch
    from livetalking_amd._lib import LtkError
    frames, faces, coords = synth.ultralight_avatar(2, FULL_HW, seed=41)
    d_feat = torch.from_numpy(synth.ultralight_feats(2, 42).reshape(2, 16, 32, 32)).cuda()
    d_pred = torch.zeros(2, 160, 160, 3, dtype=torch.uint8, device="cuda")
    a = eng.register_ultralight_avatar(sd, faces, frames, coords, max_frames=2)
    for _ in range(3):                                       # eager, captured, replayed
        eng.ultralight_infer([(a, 0, 2, d_feat.data_ptr(), d_pred.data_ptr())])
    first = d_pred.cpu().numpy().copy()
    eng.release_avatar(a)
    with pytest.raises(LtkError) as ex:
        eng.ultralight_infer([(a, 0, 2, d_feat.data_ptr(), d_pred.data_ptr())])
    assert ex.value.code == -3
    b = eng.register_ultralight_avatar(synth.ultralight_state_dict(99), faces, frames, coords, max_frames=2)
    try:
        assert b != a
        d_pred.zero_()
        for _ in range(3):
            eng.ultralight_infer([(b, 0, 2, d_feat.data_ptr(), d_pred.data_ptr())])
        second = d_pred.cpu().numpy()
        assert second.any() and not np.array_equal(first, second)      # the new avatar's weights, not a stale captured pass
        host = ref.frames_u8(eng.ultralight_forward_host(b, ref.img6_from_faces(faces), d_feat.cpu().numpy()))
        mx, _, share = ref.frame_stats(second, host)
        assert mx <= 1 and share < 0.02
    finally:
        eng.release_avatar(b)
