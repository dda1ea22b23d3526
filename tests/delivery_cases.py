"""Case tables, seeded inputs and float64 references for the delivery kernels: the Wav2Lip / Ultralight paste-back, the MuseTalk blend,
frame egress (transition blend, watermark, BGR24 -> I420) and the mel front end.  Pure numpy, no GPU; tests/test_delivery_host.py proves
the tables and the gates on the CPU, tests/test_delivery_gpu.py runs them on the device.

Two gates per byte kernel.  (1) byte-equal to the integer restatement (oracle/paste_oracle.py, oracle/egress_oracle.py).  (2) strictly
less than 1 LSB from the plain float64 definition of the operation.  Kernel and restatement were written from one reading of OpenCV and
swscale, so (1) alone cannot see a mistake they share; (2) is independent of that reading.

The float64 references are per STAGE: each takes the bytes the previous stage delivered.  The stages' rounding errors do not compose
under 1 LSB (a 0.82 LSB resize under a 0.50 LSB blend may end 1.3 LSB from the float64 of the chain), so a chained reference could not
hold the gate even for a correct kernel; per stage every figure is the stage's own rounding.

All boxes here are (x1, y1, x2, y2); the Wav2Lip bank wants (y1, y2, x1, x2) (`w2l_coords`)."""
from __future__ import annotations

import types

import numpy as np

from oracle import mel_oracle
from oracle import paste_oracle

W2L_S, UL_S, UL_PRED, UL_OFF = 256, 168, 160, 4
W_MAX = {W2L_S: 520, UL_S: 350}
AVATAR_FRAMES = 16                      # one avatar = one batched launch (misc_kernels.h kPasteBatch)
CLASS_BOUNDS = {W2L_S: (128, 256, 320, 384, 448, 520), UL_S: (84, 168, 232, 296, 350)}
LONG_SIDE = 97                          # the N of the (1, N) and (N, 1) boxes


# ----------------------------------------------------------------------------------------------------------------- float64 references
def resize_f64(src: np.ndarray, dw: int, dh: int) -> np.ndarray:
    """Bilinear resize, half-pixel centres, replicated borders: float64 (dh, dw, C)."""
    sh, sw = src.shape[:2]

    def axis(dst, s):
        c = (np.arange(dst, dtype=np.float64) + 0.5) * (s / dst) - 0.5
        i0 = np.floor(c)
        f = c - i0
        i0 = i0.astype(np.int64)
        return np.clip(i0, 0, s - 1), np.clip(i0 + 1, 0, s - 1), f

    x0, x1, fx = axis(dw, sw)
    y0, y1, fy = axis(dh, sh)
    s = src.astype(np.float64)
    r = s[:, x0] * (1 - fx)[None, :, None] + s[:, x1] * fx[None, :, None]
    return r[y0] * (1 - fy)[:, None, None] + r[y1] * fy[:, None, None]


def blend_f64(s1: np.ndarray, s2: np.ndarray, mask_u8: np.ndarray) -> np.ndarray:
    """The convex mix s1 * m + s2 * (1 - m), m = mask / 255; s1, s2 (h, w, 3), mask (h, w)."""
    m = mask_u8.astype(np.float64)[..., None] / 255.0
    return s1.astype(np.float64) * m + s2.astype(np.float64) * (1.0 - m)


def weighted_f64(prev: np.ndarray, src: np.ndarray, alpha: float) -> np.ndarray:
    """prev * (1 - alpha) + src * alpha with the weights the engine is handed: float32(alpha) and float32(1 - alpha), exactly."""
    return prev.astype(np.float64) * float(np.float32(1.0 - alpha)) + src.astype(np.float64) * float(np.float32(alpha))


def yuv_f64(bgr: np.ndarray):
    """BT.601 limited range on (..., 3) BGR: float64 Y, U, V."""
    f = bgr.astype(np.float64)
    b, g, r = f[..., 0], f[..., 1], f[..., 2]
    y = 16 + 219 * (0.299 * r + 0.587 * g + 0.114 * b) / 255
    u = 128 + 224 * (-0.168736 * r - 0.331264 * g + 0.5 * b) / 255
    v = 128 + 224 * (0.5 * r - 0.418688 * g - 0.081312 * b) / 255
    return y, u, v


def quad_mean_f64(bgr: np.ndarray) -> np.ndarray:
    f = bgr.astype(np.float64)
    return (f[0::2, 0::2] + f[0::2, 1::2] + f[1::2, 0::2] + f[1::2, 1::2]) / 4.0


def i420_f64(frame: np.ndarray, chroma: int) -> np.ndarray:
    """Float64 I420 planes of a BGR frame, laid out as egress_oracle.bgr_to_i420.  With chroma = 1 the chroma sample is the matrix of the
    ROUNDED quad mean (the mean is a stage of its own, `quad_mean_f64` is its reference)."""
    H, W = frame.shape[:2]
    y = yuv_f64(frame)[0]
    q = ((frame.astype(np.int64)[0::2, 0::2] + frame[0::2, 1::2] + frame[1::2, 0::2] + frame[1::2, 1::2] + 2) >> 2) if chroma else frame[0::2, 0::2]
    _, u, v = yuv_f64(q)
    return np.concatenate([y.reshape(-1), u.reshape(-1), v.reshape(-1)]).reshape(H * 3 // 2, W)


def mel_unclipped_f64(wav: np.ndarray) -> np.ndarray:
    """oracle/mel_oracle.py's chain (constant centre padding) without the final clip: float64 (80, 1 + len // 200)."""
    D = mel_oracle.stft(mel_oracle.preemphasis(wav))
    S = mel_oracle.amp_to_db(np.dot(mel_oracle.mel_basis(), np.abs(D))) - mel_oracle.REF_LEVEL_DB
    return (2 * mel_oracle.MAX_ABS) * ((S - mel_oracle.MIN_LEVEL_DB) / (-mel_oracle.MIN_LEVEL_DB)) - mel_oracle.MAX_ABS


def mel_direct_f64(wav: np.ndarray) -> np.ndarray:
    """A second float64 statement of the mel chain, independent of numpy's FFT: the 800-point DFT with an explicit twiddle table, every
    bin summed over n in order (what mel_kernel does).  Clipped, float64 (80, n_cols)."""
    x = np.asarray(wav, dtype=np.float64)
    y = x.copy()
    y[1:] = x[1:] - 0.97 * x[:-1]
    n_cols = 1 + len(x) // 200
    ypad = np.concatenate([np.zeros(400), y, np.zeros(400)])
    n = np.arange(800)
    ang = 2.0 * n / 800.0
    tw_c, tw_s = np.cos(np.pi * ang), np.sin(np.pi * ang)
    frames = np.stack([ypad[200 * t: 200 * t + 800] for t in range(n_cols)]) * (0.5 - 0.5 * tw_c)[None, :]
    k = np.arange(401)
    re = np.zeros((n_cols, 401))
    im = np.zeros((n_cols, 401))
    for i in range(800):
        idx = (i * k) % 800
        re += frames[:, i, None] * tw_c[idx][None, :]
        im -= frames[:, i, None] * tw_s[idx][None, :]
    mag = np.sqrt(re * re + im * im)
    basis = mel_oracle.mel_basis().astype(np.float64)
    acc = np.zeros((n_cols, 80))
    for kk in range(401):                                   # ascending k, as the kernel's lo..hi loop
        acc += mag[:, kk, None] * basis[None, :, kk]
    S = 20.0 * np.log10(np.maximum(1e-5, acc)) - 20.0
    return np.clip(8.0 * ((S + 100.0) / 100.0) - 4.0, -4.0, 4.0).T


# ----------------------------------------------------------------------------------------------------------------- resize boxes
def sweep_boxes(S: int):
    """(dw, dh): every width 1..W_max with a height from a fixed permutation, so every length occurs once on each axis."""
    n = W_MAX[S]
    perm = np.random.default_rng(7000 + S).permutation(np.arange(1, n + 1))
    return [(dw, int(perm[dw - 1])) for dw in range(1, n + 1)]


def mixed_boxes(S: int):
    """One axis at a shortcut length, the other not: these must take the general path."""
    h = S // 2
    return [(S, S - 1), (S - 1, S), (h, h - 1), (h - 1, h), (h, S)]


def explicit_boxes(S: int):
    h = S // 2
    return [(S, S), (h, h)] + mixed_boxes(S) + [(2 * S, 2 * S), (2 * S + 1, 2 * S - 1), (1, 1), (1, LONG_SIDE), (LONG_SIDE, 1), (2, 2), (3, 3)]


def _frame_hw(h0: int, w0: int, k: int):
    """The smallest (H, W) with H > h0, W > w0 and H * W * 3 % 4 == k."""
    for dh in range(1, 6):
        for dw in range(1, 6):
            if ((h0 + dh) * (w0 + dw) * 3) % 4 == k:
                return h0 + dh, w0 + dw
    raise AssertionError


def size_class(S: int, dw: int, dh: int) -> int:
    return next(b for b in CLASS_BOUNDS[S] if max(dw, dh) <= b)


def paste_groups(S: int):
    """The avatars of one family (S = 256 Wav2Lip, 168 Ultralight).  Each group: name, size class, frame (H, W), up to 16 boxes
    (x1, y1, x2, y2), one per bank frame, and a seed.  Sweep boxes are sorted by their longer side and cut into avatars of 16, so a
    frame is only as large as its boxes need; an explicit box is one avatar of five frames: the four corners and the interior."""
    groups = []
    rng = np.random.default_rng(9000 + S)
    boxes = sorted(sweep_boxes(S), key=lambda b: (max(b), b))
    for g0 in range(0, len(boxes), AVATAR_FRAMES):
        chunk = boxes[g0: g0 + AVATAR_FRAMES]
        H, W = _frame_hw(max(b[1] for b in chunk), max(b[0] for b in chunk), (g0 // AVATAR_FRAMES) % 4)
        placed = []
        for dw, dh in chunk:
            x1, y1 = int(rng.integers(0, W - dw + 1)), int(rng.integers(0, H - dh + 1))
            placed.append((x1, y1, x1 + dw, y1 + dh))
        groups.append(types.SimpleNamespace(name=f"sweep{g0 // AVATAR_FRAMES:02d}", cls=size_class(S, *chunk[-1]), H=H, W=W, boxes=placed,
                                            seed=100 * S + g0, S=S))
    for i, (dw, dh) in enumerate(explicit_boxes(S)):
        H, W = _frame_hw(dh + 2, dw + 2, i % 4)
        placed = [(0, 0, dw, dh), (W - dw, 0, W, dh), (0, H - dh, dw, H), (W - dw, H - dh, W, H), (2, 1, 2 + dw, 1 + dh)]
        groups.append(types.SimpleNamespace(name=f"box{dw}x{dh}", cls=size_class(S, dw, dh), H=H, W=W, boxes=placed, seed=100 * S + 50000 + i, S=S))
    return groups


def checkerboard(h: int, w: int, phase: int = 0) -> np.ndarray:
    yy, xx = np.mgrid[0:h, 0:w]
    return np.repeat((((yy + xx + phase) & 1) * 255).astype(np.uint8)[:, :, None], 3, axis=2)


def paste_inputs(g):
    """Seeded bytes of one group: bank frames (n, H, W, 3), predictions (n, P, P, 3) (P = 256, or 160 for Ultralight) and, for Ultralight,
    the bank faces (n, 168, 168, 3), an independent draw.  Prediction 0 of every group is the 0 / 255 checkerboard (for Ultralight the
    bank face 0 carries the opposite phase, so the seam at rows / columns 4 and 164 is a full-swing edge)."""
    rng = np.random.default_rng(g.seed)
    n = len(g.boxes)
    P = W2L_S if g.S == W2L_S else UL_PRED
    frames = rng.integers(0, 256, (n, g.H, g.W, 3), dtype=np.uint8)
    preds = rng.integers(0, 256, (n, P, P, 3), dtype=np.uint8)
    preds[0] = checkerboard(P, P)
    faces = None
    if g.S == UL_S:
        faces = rng.integers(0, 256, (n, UL_S, UL_S, 3), dtype=np.uint8)
        faces[0] = checkerboard(UL_S, UL_S, 1)
    return types.SimpleNamespace(frames=frames, preds=preds, faces=faces)


def paste_source(g, inp, i: int) -> np.ndarray:
    """The image the resize reads for bank frame i: the prediction, or the Ultralight bank face with the prediction at [4:164, 4:164]."""
    if g.S == W2L_S:
        return inp.preds[i]
    comp = inp.faces[i].copy()
    comp[UL_OFF:UL_OFF + UL_PRED, UL_OFF:UL_OFF + UL_PRED] = inp.preds[i]
    return comp


def w2l_coords(box):
    x1, y1, x2, y2 = box
    return (y1, y2, x1, x2)


# ----------------------------------------------------------------------------------------------------------------- MuseTalk blend
MT_FRAMES = ((141, 151), (140, 152))        # odd: H*W*3 % 4 == 1, byte stores and the byte egress kernel; even, W % 4 == 0: dword, I420


def blend_cases(H: int, W: int):
    """One MuseTalk avatar of frame size (H, W): per bank frame a face box, a crop box, a mask (h, w, 3) and a prediction."""
    rng = np.random.default_rng(31 * H + W)
    spec = [  # name, face (x1, y1, x2, y2), crop (xs, ys, xe, ye), mask kind
        ("odd_crop_first", (21, 11, 60, 48), (10, 5, 83, 72), "all256"),           # 73 x 67 crop: the next mask offset is odd
        ("face_is_crop", (30, 20, 90, 99), (30, 20, 90, 99), "random"),
        ("crop_is_frame", (5, 6, W - 9, H - 4), (0, 0, W, H), "all256"),
        ("crop_left", (3, 40, 50, 90), (0, 31, 61, 100), "random"),
        ("crop_top", (40, 2, 90, 60), (33, 0, 99, 71), "hard"),
        ("crop_right", (W - 50, 30, W - 1, 80), (W - 61, 22, W, 91), "random"),
        ("crop_bottom", (30, H - 70, 100, H - 3), (21, H - 77, 110, H), "nongrey"),
        ("face_1x1", (70, 70, 71, 71), (60, 61, 81, 80), "all256"),
        ("mixed_128x127", (10, 5, 138, 132), (4, 2, 145, 137), "all256"),
        ("identity_like_127x128", (12, 6, 139, 134), (7, 0, 144, 139), "random"),
        ("mask_all0", (20, 20, 80, 90), (10, 10, 95, 101), "zero"),
        ("mask_all255", (20, 20, 80, 90), (10, 10, 95, 101), "full"),
        ("checker_pred", (25, 15, 125, 126), (20, 10, 131, 133), "all256"),
    ]
    cases = []
    for name, face, crop, kind in spec:
        h, w = crop[3] - crop[1], crop[2] - crop[0]
        if kind == "all256":                    # every mask value, many times, in an order unrelated to the pixel grid
            g = rng.permutation(np.arange(h * w) % 256).astype(np.uint8).reshape(h, w)
        elif kind == "random" or kind == "nongrey":
            g = rng.integers(0, 256, (h, w), dtype=np.uint8)
        elif kind == "hard":
            g = (rng.integers(0, 2, (h, w)) * 255).astype(np.uint8)
        else:
            g = np.full((h, w), 0 if kind == "zero" else 255, dtype=np.uint8)
        mask = np.repeat(g[:, :, None], 3, axis=2)
        if kind == "nongrey":                   # B != G: the kernel and the oracle read channel 0 (B), as the reference's saved masks allow
            mask[:, :, 1] = rng.integers(0, 256, (h, w), dtype=np.uint8)
            mask[:, :, 2] = rng.integers(0, 256, (h, w), dtype=np.uint8)
        frame = rng.integers(0, 256, (H, W, 3), dtype=np.uint8)
        pred = checkerboard(256, 256) if name == "checker_pred" else rng.integers(0, 256, (256, 256, 3), dtype=np.uint8)
        cases.append(types.SimpleNamespace(name=name, face=face, crop=crop, mask=mask, frame=frame, pred=pred))
    return cases


def blend_stage_f64(c) -> np.ndarray:
    """Float64 reference of the blend STAGE of a case: the exact mix of the restatement's resized bytes and the frame."""
    x1, y1, x2, y2 = c.face
    xs, ys, xe, ye = c.crop
    ref = c.frame.astype(np.float64)
    fl = c.frame[ys:ye, xs:xe].copy()
    fl[y1 - ys:y2 - ys, x1 - xs:x2 - xs] = paste_oracle.resize_linear_u8(c.pred, (x2 - x1, y2 - y1))
    ref[ys:ye, xs:xe] = blend_f64(fl, c.frame[ys:ye, xs:xe], c.mask[:, :, 0])
    return ref


# ----------------------------------------------------------------------------------------------------------------- egress
EGRESS_BGR = ((1, 1), (1, 5), (2, 3), (3, 4), (5, 8), (7, 9), (8, 10), (9, 11))
EGRESS_I420 = ((2, 2), (2, 4), (4, 2), (6, 10), (10, 12), (12, 18))
ALPHAS = (0.0, 0.5, 0.25, 0.999, 1.0 - 2.0 ** -24)
BATCH_SHAPES = ((10, 12), (12, 18))     # W % 4 == 0 and W % 4 == 2
BATCH_NS = (1, 2, 17)
COLOUR_HW = (258, 256)


def watermarks(H: int, W: int):
    """(name, mask (h, w) of 0 / 255, x, y) rectangles for an (H, W) frame: inside, over each edge, over the whole frame, odd starts."""
    rng = np.random.default_rng(17 * H + W)

    def bits(h, w):
        m = (rng.random((h, w)) < 0.7).astype(np.uint8) * 255
        m[0, 0] = m[-1, -1] = 255
        return m

    out = [("inside", bits(max(1, H - 2), max(1, W - 2)), min(1, W - 1), min(1, H - 1)),
           ("over_left", bits(max(1, H // 2), 3), -2, 0),
           ("over_top", bits(3, max(1, W // 2)), 0, -2),
           ("over_right", bits(H, 4), W - 2, 0),
           ("over_bottom", bits(4, W), 0, H - 2),
           ("covers_all", np.full((H + 2, W + 3), 255, np.uint8), -1, -1),
           ("odd_start", bits(3, 5), 3, 1),          # x 3..7 straddles the 4-pixel patch at x = 4, y 1..3 the row pair at y = 2
           ("odd_start_11", bits(2, 2), 1, 1)]       # straddles the chroma quads at (0, 0), (0, 2), (2, 0), (2, 2)
    return out


def egress_frames(H: int, W: int):
    """(prev, src) pairs of one shape: the two checkerboard phases (with alpha = 0.5 every sum lands on .5) and a random pair."""
    rng = np.random.default_rng(1000 * H + W)
    return [("checker", checkerboard(H, W, 0), checkerboard(H, W, 1)),
            ("random", rng.integers(0, 256, (H, W, 3), dtype=np.uint8), rng.integers(0, 256, (H, W, 3), dtype=np.uint8))]


def colour_frame() -> np.ndarray:
    """The 8 cube corners, the 256 greys and 65 536 seeded random colours (the rest random too) in one (258, 256) BGR frame."""
    H, W = COLOUR_HW
    rng = np.random.default_rng(601)
    px = rng.integers(0, 256, (H * W, 3), dtype=np.uint8)
    px[:8] = [[255 * ((i >> k) & 1) for k in range(3)] for i in range(8)]
    px[8:264] = np.arange(256, dtype=np.uint8)[:, None]
    return px.reshape(H, W, 3)


# ----------------------------------------------------------------------------------------------------------------- mel
MEL_SAMPLES = (3000, 3001, 3199, 3200, 16640, 16641)
MEL_SIGNALS = ("noise", "noise_tone", "square", "tiny", "dc", "silence")
MEL_EXACT_CLIP = ("square", "tiny", "silence")
MEL_FLOOR_TOL = 2e-5     # the float32 store is 2.4e-7 (half an ulp at +-4); the rest is the relative error r of an fp64 mel sum, 0.695 r in the
#                          output (8 * 20 / 100 / ln 10): libm's cos / sin / log10 against the device's, summation order of equal length


def mel_signal(name: str, n: int) -> np.ndarray:
    rng = np.random.default_rng(4242)
    t = np.arange(n)
    if name == "noise":
        w = 0.3 * rng.standard_normal(n)
    elif name == "noise_tone":
        w = 0.05 * rng.standard_normal(n) + 0.5 * np.sin(2 * np.pi * 440 * t / 16000)
    elif name == "square":                      # full scale, 500 Hz: the upper clip
        w = np.where((t // 16) % 2 == 0, 1.0, -1.0)
    elif name == "tiny":                        # mel sums around the 1e-5 floor: the lower clip boundary
        w = 1e-7 * rng.standard_normal(n)
    elif name == "dc":                          # y[0] = x[0] = 0.5, y[n] = 0.015 afterwards
        w = np.full(n, 0.5)
    else:
        w = np.zeros(n)
    return w.astype(np.float32)


def mel_windows(n_samples: int):
    """(name, starts) lists for a buffer of n_samples (n_cols = 1 + n_samples // 200 columns)."""
    n_cols = 1 + n_samples // 200
    last = n_cols - 16
    out = [("first", [0]), ("last", [last]), ("both", [0, last]), ("thrice", [last // 2] * 3), ("descending", list(range(last, -1, -3))),
           ("every", list(range(0, last + 1))), ("n1024", [(7 * i) % (last + 1) for i in range(1024)])]
    if last >= 40:
        out.append(("far_apart", [1, last - 1]))         # the columns between belong to no window
    return out


def mel_refusals(n_samples: int):
    n_cols = 1 + n_samples // 200
    return [("past_end", [0, n_cols - 15]), ("negative", [-1]), ("n_win_0", []), ("n_win_1025", [0] * 1025)]


def mel_statement_gap(signal: str) -> float:
    """max |direct DFT statement - mel_oracle.melspectrogram| over the table's buffer lengths: what two float64 statements of the same
    chain differ by on this signal (both clipped, the difference taken as it stands).  Four times this, or MEL_FLOOR_TOL if larger, is
    the device tolerance."""
    worst = 0.0
    for n in MEL_SAMPLES:
        wav = mel_signal(signal, n)
        worst = max(worst, float(np.abs(mel_direct_f64(wav) - mel_oracle.melspectrogram(wav)).max()))
    return worst
