"""The delivery kernels on the device against tests/delivery_cases.py: paste_kernel / paste_batch_kernel (Wav2Lip), ul_paste_kernel /
ul_paste_batch_kernel (Ultralight), paste_blend_kernel (MuseTalk), egress_kernel / egress_batch_kernel (transition blend, watermark,
BGR24 -> I420) and mel_kernel.

Byte kernels, every case: byte-equal to oracle/paste_oracle.py / oracle/egress_oracle.py, and strictly under 1 LSB from the float64
reference of the stage (delivery_cases.py explains why the float64 references are per stage).  A miss names the case, the count of
differing bytes, the first differing (y, x, c) and the device / restatement / float64 values there.

Mel: |dev - mel_oracle| <= max(2e-5, 4 x the CPU-measured gap between the two float64 statements on the same signal) - not MEL_TOL of
tests/test_mel_paste_gpu.py, which stays where it is.  Kernel and oracle both run the chain in fp64 on the float32 basis; the one float32
rounding is the store (2.4e-7 at +-4).  Columns 0 and n_cols - 1 are held to the CONSTANT-padding oracle: that is the project's stated
convention (oracle/mel_oracle.py's docstring: librosa's padding mode differs across versions, and the render loop never consumes a
column the padding reaches), so the kernel's zero padding is the definition here, not an approximation.

The module builds its own engine and avatars.  LTK_DELIVERY_PARITY_OUT names a file the records are appended to
(profiles/delivery_parity.txt)."""
from __future__ import annotations

import ctypes as C
import os

import numpy as np
import pytest

import delivery_cases as K
import synth_inputs as synth
from oracle import egress_oracle as eo
from oracle import mel_oracle
from oracle import paste_oracle as po

pytestmark = pytest.mark.gpu

WM_COLOUR = (7, 130, 251)
SENTINEL = 0xA5


def _emit(line):
    print(line)
    out = os.environ.get("LTK_DELIVERY_PARITY_OUT")
    if out:
        with open(out, "a") as f:
            f.write(line + "\n")


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
def ul_sd():
    return synth.ultralight_state_dict(1234)


def _gate(case, dev, orc, f64=None, region=None):
    """Both gates on one frame; returns (bytes differing from the restatement, worst distance to float64).  f64 covers `region`
    (y1, y2, x1, x2) of the frame, or all of it."""
    dev, orc = np.asarray(dev), np.asarray(orc)
    assert dev.shape == orc.shape, (case, dev.shape, orc.shape)
    ndiff = int((dev != orc).sum())
    worst = 0.0
    d3, o3 = np.atleast_3d(dev), np.atleast_3d(orc)
    if f64 is not None:
        sub = d3 if region is None else d3[region[0]:region[1], region[2]:region[3]]
        dist = np.abs(sub.astype(np.float64) - np.atleast_3d(f64))
        worst = float(dist.max()) if dist.size else 0.0
    if ndiff or worst >= 1.0:
        where = np.argwhere(d3 != o3)
        y, x, c = (int(v) for v in (where[0] if len(where) else np.unravel_index(int(dist.argmax()), dist.shape)))
        if not len(where) and region is not None:
            y, x = y + region[0], x + region[2]
        fv = None
        if f64 is not None:
            f3 = np.atleast_3d(f64)
            ry, rx = (y, x) if region is None else (y - region[0], x - region[2])
            if 0 <= ry < f3.shape[0] and 0 <= rx < f3.shape[1]:
                fv = float(f3[ry, rx, c])
        pytest.fail(f"{case}: {ndiff} bytes differ from the restatement, worst distance to float64 {worst:.3f} LSB; first at (y, x, c) = "
                    f"({y}, {x}, {c}): device {int(d3[y, x, c])}, restatement {int(o3[y, x, c])}, float64 {fv}")
    return ndiff, worst


# ----------------------------------------------------------------------------------------------------------------- paste-back
def _register(eng, ul_sd, g, inp):
    if g.S == K.W2L_S:
        return eng.register_avatar(list(inp.preds), list(inp.frames), [K.w2l_coords(b) for b in g.boxes])
    return eng.register_ultralight_avatar(ul_sd, list(inp.faces), list(inp.frames), list(g.boxes), max_frames=4)


def _paste_one(eng, g, aid, i, pred_ptr, out):
    (eng.paste_back if g.S == K.W2L_S else eng.ultralight_paste_back)(aid, i, pred_ptr, out)


def _paste_device(eng, g, aid, i, pred_ptr, out_ptr):
    if g.S == K.W2L_S:
        eng.paste_back_device(aid, i, pred_ptr, out_ptr)
    else:
        from livetalking_amd import _lib
        _lib.check(eng._lib.ltk_ultralight_paste_back(eng._h, int(aid), int(i), C.c_void_p(pred_ptr), C.c_void_p(out_ptr), 1, C.c_void_p(0)))


def _paste_want(g, inp, i):
    """(restatement composite, float64 of the box, region) of bank frame i."""
    x1, y1, x2, y2 = g.boxes[i]
    src = K.paste_source(g, inp, i)
    want = inp.frames[i].copy()
    want[y1:y2, x1:x2] = po.resize_linear_u8(src, (x2 - x1, y2 - y1))
    return want, K.resize_f64(src, x2 - x1, y2 - y1), (y1, y2, x1, x2)


FAMILY = {K.W2L_S: "wav2lip_paste", K.UL_S: "ultralight_paste"}
PASTE_IDS = [(S, cls) for S in (K.W2L_S, K.UL_S) for cls in K.CLASS_BOUNDS[S]]


@pytest.mark.parametrize("S,cls", PASTE_IDS, ids=[f"{FAMILY[S]}-le{cls}" for S, cls in PASTE_IDS])
def test_paste_every_box_batched_and_per_frame(eng, ul_sd, S, cls):
    """Every box of the size class: the whole avatar in one batched launch, then frame by frame through the per-frame entry."""
    import torch
    for g in (g for g in K.paste_groups(S) if g.cls == cls):
        inp = K.paste_inputs(g)
        n = len(g.boxes)
        aid = _register(eng, ul_sd, g, inp)
        try:
            d_preds = torch.from_numpy(inp.preds).cuda()
            batch = np.full((n, g.H, g.W, 3), SENTINEL, np.uint8)
            (eng.paste_back_batch if S == K.W2L_S else eng.ultralight_paste_back_batch)(aid, list(range(n)), d_preds.data_ptr(), batch.ctypes.data)
            worst, at = 0.0, None
            for i in range(n):
                want, f64, region = _paste_want(g, inp, i)
                case = f"{FAMILY[S]} {g.name} frame {i} box {g.boxes[i]} in {g.H}x{g.W}"
                _, w = _gate(case + " (batched)", batch[i], want, f64, region)
                one = np.full((g.H, g.W, 3), SENTINEL, np.uint8)
                _paste_one(eng, g, aid, i, d_preds[i].data_ptr(), one)
                assert np.array_equal(one, batch[i]), f"{case}: the per-frame entry differs from the batched launch in {(one != batch[i]).sum()} bytes"
                if w >= worst:
                    worst, at = w, (g.boxes[i][2] - g.boxes[i][0], g.boxes[i][3] - g.boxes[i][1])
            mod4 = g.H * g.W * 3 % 4
            _emit(f"{FAMILY[S]} {g.name} frame {g.H}x{g.W} (H*W*3 % 4 = {mod4}: {'dword stores' if mod4 == 0 else 'dword and byte stores by frame'}) "
                  f"boxes {n} bytes_differing 0 per_frame_equal yes worst_f64 {worst:.3f} LSB at {at[0]}x{at[1]}")
        finally:
            eng.release_avatar(aid)


@pytest.mark.parametrize("S", [K.W2L_S, K.UL_S], ids=[FAMILY[K.W2L_S], FAMILY[K.UL_S]])
def test_paste_device_output_at_byte_offsets(eng, ul_sd, S):
    """The device-output entry with the output 1, 2 and 3 bytes into a larger buffer: the frame is right and nothing outside it is written."""
    import torch
    g = next(g for g in K.paste_groups(S) if g.name == f"box{S}x{S - 1}")
    inp = K.paste_inputs(g)
    aid = _register(eng, ul_sd, g, inp)
    try:
        d_preds = torch.from_numpy(inp.preds).cuda()
        i = 4
        want, f64, region = _paste_want(g, inp, i)
        nbytes = g.H * g.W * 3
        for off in (0, 1, 2, 3):
            buf = torch.full((nbytes + 16,), SENTINEL, dtype=torch.uint8, device="cuda")
            _paste_device(eng, g, aid, i, d_preds[i].data_ptr(), buf.data_ptr() + off)
            got = buf.cpu().numpy()
            _gate(f"{FAMILY[S]} {g.name} device output at +{off}", got[off:off + nbytes].reshape(g.H, g.W, 3), want, f64, region)
            assert (got[:off] == SENTINEL).all() and (got[off + nbytes:] == SENTINEL).all(), f"+{off}: bytes outside the frame were written"
            _emit(f"{FAMILY[S]} {g.name} device_output +{off} ({'dword' if off == 0 else 'byte'} stores) bytes_differing 0 outside_untouched yes")
    finally:
        eng.release_avatar(aid)


# ----------------------------------------------------------------------------------------------------------------- MuseTalk blend
@pytest.mark.parametrize("hw", K.MT_FRAMES, ids=[f"{h}x{w}" for h, w in K.MT_FRAMES])
def test_musetalk_blend_per_frame_and_batched_egress(eng, hw):
    import torch
    from livetalking_amd import egress
    H, W = hw
    cases = K.blend_cases(H, W)
    n = len(cases)
    lat = [np.zeros((1, 8, 32, 32), np.float32) for _ in range(n)]
    aid = eng.register_musetalk_avatar(lat, [c.frame for c in cases], [c.face for c in cases], [c.mask for c in cases], [c.crop for c in cases])
    h = eng.egress_open(H, W)
    try:
        d_preds = torch.from_numpy(np.stack([c.pred for c in cases])).cuda()
        wants = []
        for i, c in enumerate(cases):
            want = po.paste_blend_frame(c.pred, c.frame, c.face, c.mask, c.crop)
            wants.append(want)
            out = np.full((H, W, 3), SENTINEL, np.uint8)
            eng.paste_blend(aid, i, d_preds[i].data_ptr(), out)
            _, w = _gate(f"musetalk_blend {c.name} in {H}x{W}", out, want, K.blend_stage_f64(c))
            if c.name == "mask_all255":         # weight 1: the blend hands the resized bytes through, so the resize stage shows
                x1, y1, x2, y2 = c.face
                _gate(f"musetalk_blend {c.name} resize stage", out, want, K.resize_f64(c.pred, x2 - x1, y2 - y1), (y1, y2, x1, x2))
            _emit(f"musetalk_blend {c.name} frame {H}x{W} ({'dword' if H * W * 3 % 4 == 0 else 'dword, byte tail'} stores) bytes_differing 0 worst_f64 {w:.3f} LSB")
        fmts = [("bgr24", 1)] + ([("i420", 0), ("i420", 1)] if H % 2 == 0 and W % 2 == 0 else [])
        for fmt, chroma in fmts:
            shape = (n, H * 3 // 2, W) if fmt == "i420" else (n, H, W, 3)
            got = np.full(shape, SENTINEL, np.uint8)
            eng.egress_batch(h, egress.SRC_MUSETALK, aid, list(range(n)), d_preds.data_ptr(), got.ctypes.data,
                             egress.FMT_I420 if fmt == "i420" else egress.FMT_BGR24, chroma)
            worst = 0.0
            for i, c in enumerate(cases):
                ref = eo.egress_frame(wants[i], None, fmt, chroma)
                f64 = K.i420_f64(wants[i], chroma) if fmt == "i420" else K.blend_stage_f64(c)
                worst = max(worst, _gate(f"musetalk egress_batch {fmt} chroma {chroma} {c.name}", got[i], ref, f64)[1])
            _emit(f"musetalk_egress_batch {fmt} chroma {chroma} frame {H}x{W} n {n} ({'VEC' if W % 4 == 0 and H * W * 3 % 4 == 0 else 'byte'} kernel) "
                  f"bytes_differing 0 worst_f64 {worst:.3f} LSB")
    finally:
        eng.egress_close(h)
        eng.release_avatar(aid)


# ----------------------------------------------------------------------------------------------------------------- egress
def _is_vec(H, W, i420):
    return W % 4 == 0 and (not i420 or ((H * W) % 4 == 0 and ((H // 2) * (W // 2)) % 2 == 0))


def _egress_f64(blend_f64, blend_u8, wm, fmt, chroma):
    """Float64 reference of the delivered frame: BGR24: the float64 weighted sum with the watermark colour set; I420: the float64 matrix of
    the restatement's watermarked BGR bytes (the previous stage's output)."""
    if fmt == "i420":
        return K.i420_f64(eo.egress_frame(blend_u8, wm, "bgr24", 1), chroma)
    ref = blend_f64.copy()
    if wm is not None:
        mask, x, y, col = wm
        tmp = np.zeros(ref.shape[:2] + (3,), np.uint8)
        cover = eo.apply_watermark(tmp, mask, x, y, (1, 1, 1))[:, :, 0].astype(bool)
        ref[cover] = np.asarray(col, np.float64)
    return ref


ALL_SHAPES = [(hw, False) for hw in K.EGRESS_BGR] + [(hw, True) for hw in K.EGRESS_I420]


@pytest.mark.parametrize("hw,even", ALL_SHAPES, ids=[f"{h}x{w}" for (h, w), _ in ALL_SHAPES])
def test_egress_host_frames_every_tail_watermark_and_alpha(eng, hw, even):
    from livetalking_amd import egress
    H, W = hw
    fmts = [("bgr24", 1)] + ([("i420", 0), ("i420", 1)] if even else [])
    h = eng.egress_open(H, W)
    try:
        stats = {f: [0, 0.0] for f in fmts}
        for wm_name, mask, x, y in [("none", None, 0, 0)] + K.watermarks(H, W):
            eng.egress_watermark(h, mask, x, y, WM_COLOUR)
            wm = None if mask is None else (mask, x, y, WM_COLOUR)
            for img, prev, src in K.egress_frames(H, W):
                # the silent frame `prev` goes into the session's cache (before the watermark); every speaking frame then blends with it
                first = np.full((H, W, 3), SENTINEL, np.uint8)
                eng.egress_frame(h, first, egress.SRC_HOST, 0, 0, 0, prev, False, -1.0, True, egress.FMT_BGR24, 1)
                _gate(f"egress {H}x{W} wm {wm_name} {img} silent", first, eo.egress_frame(prev, wm, "bgr24", 1), _egress_f64(prev.astype(np.float64), prev, wm, "bgr24", 1))
                for alpha in K.ALPHAS:
                    blend_u8 = eo.add_weighted_u8(prev, 1 - alpha, src, alpha)
                    blend_f = K.weighted_f64(prev, src, alpha)
                    for fmt, chroma in fmts:
                        out = np.full((H * 3 // 2, W) if fmt == "i420" else (H, W, 3), SENTINEL, np.uint8)
                        eng.egress_frame(h, out, egress.SRC_HOST, 0, 0, 0, src, True, alpha, False,
                                         egress.FMT_I420 if fmt == "i420" else egress.FMT_BGR24, chroma)
                        _, w = _gate(f"egress {H}x{W} {fmt} chroma {chroma} wm {wm_name} {img} alpha {alpha!r}", out, eo.egress_frame(blend_u8, wm, fmt, chroma),
                                     _egress_f64(blend_f, blend_u8, wm, fmt, chroma))
                        stats[(fmt, chroma)][0] += 1
                        stats[(fmt, chroma)][1] = max(stats[(fmt, chroma)][1], w)
        for (fmt, chroma), (calls, w) in stats.items():
            _emit(f"egress_frame host {H}x{W} {fmt} chroma {chroma} ({'VEC' if _is_vec(H, W, fmt == 'i420') else 'byte'} kernel) cases {calls} "
                  f"(9 watermarks x 2 images x {len(K.ALPHAS)} alphas) bytes_differing 0 worst_f64 {w:.3f} LSB")
    finally:
        eng.egress_close(h)


def test_egress_colours(eng):
    """The 8 cube corners, the 256 greys and 65 536 random colours through the device matrix, both chroma modes."""
    from livetalking_amd import egress
    H, W = K.COLOUR_HW
    col = K.colour_frame()
    h = eng.egress_open(H, W)
    try:
        for chroma in (0, 1):
            out = np.full((H * 3 // 2, W), SENTINEL, np.uint8)
            eng.egress_frame(h, out, egress.SRC_HOST, 0, 0, 0, col, False, -1.0, False, egress.FMT_I420, chroma)
            _, w = _gate(f"egress colours chroma {chroma}", out, eo.bgr_to_i420(col, chroma), K.i420_f64(col, chroma))
            _emit(f"egress_frame colours {H}x{W} i420 chroma {chroma} (VEC kernel) bytes_differing 0 worst_f64 {w:.3f} LSB")
    finally:
        eng.egress_close(h)


@pytest.mark.parametrize("hw", K.BATCH_SHAPES, ids=[f"{h}x{w}" for h, w in K.BATCH_SHAPES])
def test_egress_batch_wav2lip_sourced(eng, hw):
    """ltk_egress_batch with n = 1, 2 and 17 (crosses the 16-frame launch chunk) on a Wav2Lip bank, per format: each frame equals the
    per-frame entry and the restatement."""
    import torch
    from livetalking_amd import egress
    H, W = hw
    rng = np.random.default_rng(H * W)
    boxes = [(1, 1, 8, 7), (0, 0, W, H), (W - 5, H - 3, W, H), (2, 3, 3, 4)]
    frames = rng.integers(0, 256, (4, H, W, 3), dtype=np.uint8)
    preds = rng.integers(0, 256, (max(K.BATCH_NS), 256, 256, 3), dtype=np.uint8)
    aid = eng.register_avatar(list(preds[:4]), list(frames), [K.w2l_coords(b) for b in boxes])
    h = eng.egress_open(H, W)
    try:
        d_preds = torch.from_numpy(preds).cuda()
        _, mask, x, y = next(w for w in K.watermarks(H, W) if w[0] == "odd_start")
        eng.egress_watermark(h, mask, x, y, WM_COLOUR)
        wm = (mask, x, y, WM_COLOUR)
        for fmt, chroma in (("bgr24", 1), ("i420", 0), ("i420", 1)):
            fcode = egress.FMT_I420 if fmt == "i420" else egress.FMT_BGR24
            shape = (H * 3 // 2, W) if fmt == "i420" else (H, W, 3)
            for n in K.BATCH_NS:
                idx = [(3 * i + 1) % 4 for i in range(n)]
                got = np.full((n,) + shape, SENTINEL, np.uint8)
                eng.egress_batch(h, egress.SRC_WAV2LIP, aid, idx, d_preds.data_ptr(), got.ctypes.data, fcode, chroma)
                worst = 0.0
                for i in range(n):
                    comp = po.paste_back_frame(preds[i].astype(np.float32), frames[idx[i]], K.w2l_coords(boxes[idx[i]]))
                    ref = eo.egress_frame(comp, wm, fmt, chroma)
                    f64 = K.i420_f64(eo.egress_frame(comp, wm, "bgr24", 1), chroma) if fmt == "i420" else None
                    worst = max(worst, _gate(f"egress_batch wav2lip {H}x{W} {fmt} chroma {chroma} n {n} frame {i}", got[i], ref, f64)[1])
                    one = np.full(shape, SENTINEL, np.uint8)
                    eng.egress_frame(h, one, egress.SRC_WAV2LIP, aid, idx[i], d_preds[i].data_ptr(), None, True, -1.0, False, fcode, chroma)
                    assert np.array_equal(one, got[i]), (fmt, chroma, n, i)
                _emit(f"egress_batch wav2lip {H}x{W} {fmt} chroma {chroma} n {n} ({'VEC' if _is_vec(H, W, fmt == 'i420') else 'byte'} kernel) "
                      f"bytes_differing 0 per_frame_equal yes worst_f64 {worst:.3f} LSB")
    finally:
        eng.egress_close(h)
        eng.release_avatar(aid)


# ----------------------------------------------------------------------------------------------------------------- mel
def _mel_tol(signal):
    """(tolerance, CPU gap, which applied): the larger of the floor and 4 x the gap of the two float64 statements on this signal."""
    gap = K.mel_statement_gap(signal)
    tol = max(K.MEL_FLOOR_TOL, 4 * gap)
    return tol, gap, "floor 2e-5" if tol == K.MEL_FLOOR_TOL else "4 x CPU gap"


@pytest.mark.parametrize("signal", K.MEL_SIGNALS)
def test_mel_every_window_list_and_length(eng, signal):
    import torch
    from livetalking_amd._lib import LtkError
    tol, gap, which = _mel_tol(signal)
    for n in K.MEL_SAMPLES:
        wav = K.mel_signal(signal, n)
        ref = mel_oracle.melspectrogram(wav)            # constant padding: columns 0 and n_cols - 1 included (module docstring)
        raw = K.mel_unclipped_f64(wav)
        worst, clipped = 0.0, 0
        for name, starts in K.mel_windows(n):
            nw = len(starts)
            out = torch.full((nw + 1, 80, 16), 777.0, dtype=torch.float32, device="cuda")
            eng.mel_step(wav, starts, out.data_ptr())
            got = out.cpu().numpy()
            want = np.stack([ref[:, s:s + 16] for s in starts])
            err = float(np.abs(got[:nw] - want).max())
            worst = max(worst, err)
            assert err <= tol, f"mel {signal} n_samples {n} windows {name}: max |dev - oracle| {err:.3e} > {tol:.3e} ({which})"
            assert (got[nw] == 777.0).all(), f"mel {signal} n_samples {n} windows {name}: wrote past window {nw - 1}"
            if signal in K.MEL_EXACT_CLIP:
                rw = np.stack([raw[:, s:s + 16] for s in starts])
                hi, lo = rw > 4.0 + tol, rw < -4.0 - tol
                assert (got[:nw][hi] == 4.0).all() and (got[:nw][lo] == -4.0).all(), f"mel {signal} n_samples {n} windows {name}: clip value missed"
                clipped += int(hi.sum() + lo.sum())
        _emit(f"mel {signal} n_samples {n} window_lists {len(K.mel_windows(n))} max|dev-ref|/tol {worst / tol:.3f} (tol {tol:.1e}: {which}, CPU gap {gap:.1e})"
              + (f" exact_clip_values {clipped}" if signal in K.MEL_EXACT_CLIP else ""))
    # refusals: the error comes back, nothing is written, and the next valid call still matches
    n = 16640
    wav = K.mel_signal(signal, n)
    ref = mel_oracle.melspectrogram(wav)
    out = torch.full((1026, 80, 16), 777.0, dtype=torch.float32, device="cuda")
    for name, starts in K.mel_refusals(n):
        with pytest.raises(LtkError) as ex:
            eng.mel_step(wav, starts, out.data_ptr())
        assert ex.value.code == -1, name
    assert (out.cpu().numpy() == 777.0).all()
    eng.mel_step(wav, [0, 68], out.data_ptr())
    assert float(np.abs(out.cpu().numpy()[:2] - np.stack([ref[:, 0:16], ref[:, 68:84]])).max()) <= tol
