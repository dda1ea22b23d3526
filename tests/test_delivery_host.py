"""CPU proof of tests/delivery_cases.py: the tables meet their own conditions, the repository's integer restatements stay strictly under
1 LSB from the plain float64 definition of each stage on every case (figures printed), and the two gates of tests/test_delivery_gpu.py
have power: numpy mutants of the restatements are caught by the byte-equal gate, the gross ones also by the float64 gate, and the ones
that escape the float64 gate are named (that is why the byte gate stays).  No GPU."""
from __future__ import annotations

import numpy as np
import pytest

import delivery_cases as K
from oracle import egress_oracle as eo
from oracle import mel_oracle
from oracle import paste_oracle as po


# ----------------------------------------------------------------------------------------------------------------- the tables
@pytest.mark.parametrize("S", [K.W2L_S, K.UL_S])
def test_resize_table_meets_its_conditions(S):
    n = K.W_MAX[S]
    sweep = K.sweep_boxes(S)
    assert sorted(b[0] for b in sweep) == list(range(1, n + 1)) and sorted(b[1] for b in sweep) == list(range(1, n + 1))
    h = S // 2
    want = {(S, S), (h, h), (S, S - 1), (S - 1, S), (h, h - 1), (h - 1, h), (h, S), (2 * S, 2 * S), (2 * S + 1, 2 * S - 1), (1, 1), (2, 2), (3, 3),
            (1, K.LONG_SIDE), (K.LONG_SIDE, 1)}
    assert set(K.explicit_boxes(S)) == want and set(K.mixed_boxes(S)) <= want
    groups = K.paste_groups(S)
    seen, mod4, resident = [], set(), 0
    for g in groups:
        assert 1 <= len(g.boxes) <= K.AVATAR_FRAMES
        for x1, y1, x2, y2 in g.boxes:
            assert 0 <= x1 < x2 <= g.W and 0 <= y1 < y2 <= g.H
            assert max(x2 - x1, y2 - y1) <= g.cls
            seen.append((x2 - x1, y2 - y1))
        mod4.add(g.H * g.W * 3 % 4)
        resident = max(resident, len(g.boxes) * (g.H * g.W * 3 + 256 * 256 * 3 * 2))
        if g.name.startswith("box"):            # four corners and the interior
            (dw, dh), b = seen[-1], g.boxes
            assert (b[0][0], b[0][1]) == (0, 0) and (b[1][2], b[1][1]) == (g.W, 0) and (b[2][0], b[2][3]) == (0, g.H)
            assert (b[3][2], b[3][3]) == (g.W, g.H) and b[4][0] > 0 and b[4][1] > 0 and b[4][2] < g.W and b[4][3] < g.H
    assert mod4 == {0, 1, 2, 3}
    assert sorted(seen) == sorted(sweep + 5 * K.explicit_boxes(S))
    assert {g.cls for g in groups} == set(K.CLASS_BOUNDS[S])
    assert resident < 32 << 20                   # one avatar at a time: well under 64 MB of bank
    inp = K.paste_inputs(groups[0])
    assert set(np.unique(inp.preds[0])) == {0, 255}
    if S == K.UL_S:
        assert not np.array_equal(inp.faces[1][4:164, 4:164], inp.preds[1])


def test_blend_table_meets_its_conditions():
    for H, W in K.MT_FRAMES:
        cases = K.blend_cases(H, W)
        names = {c.name for c in cases}
        assert {"face_is_crop", "crop_is_frame", "crop_left", "crop_top", "crop_right", "crop_bottom", "face_1x1"} <= names
        offs = np.cumsum([0] + [c.mask.size for c in cases])
        assert any(o % 2 for o in offs[:-1]), "no odd mask offset"
        pairs, kinds = set(), set()
        for c in cases:
            x1, y1, x2, y2 = c.face
            xs, ys, xe, ye = c.crop
            assert 0 <= xs <= x1 < x2 <= xe <= W and 0 <= ys <= y1 < y2 <= ye <= H
            assert c.mask.shape == (ye - ys, xe - xs, 3)
            m = c.mask[:, :, 0]
            fl = c.frame[ys:ye, xs:xe].copy()
            fl[y1 - ys:y2 - ys, x1 - xs:x2 - xs] = po.resize_linear_u8(c.pred, (x2 - x1, y2 - y1))
            par = (fl.astype(int) - c.frame[ys:ye, xs:xe]) & 1
            pairs |= set(zip(np.repeat(m[:, :, None], 3, 2).ravel().tolist(), par.ravel().tolist()))
            u = set(np.unique(m).tolist())
            kinds.add("all256" if len(u) == 256 else "zero" if u == {0} else "full" if u == {255} else "hard" if u == {0, 255} else "other")
        by = {c.name: c for c in cases}
        assert by["face_is_crop"].face == by["face_is_crop"].crop and by["crop_is_frame"].crop == (0, 0, W, H)
        assert by["crop_left"].crop[0] == 0 and by["crop_top"].crop[1] == 0 and by["crop_right"].crop[2] == W and by["crop_bottom"].crop[3] == H
        f = by["mixed_128x127"].face
        assert (f[2] - f[0], f[3] - f[1]) in K.mixed_boxes(K.W2L_S)
        assert any((c.crop[2] - c.crop[0]) % 2 for c in cases)
        assert {"all256", "zero", "full", "hard"} <= kinds
        assert len(pairs) == 512, f"{512 - len(pairs)} (mask, parity) pairs never occur"


def test_egress_and_mel_tables_meet_their_conditions():
    assert {W % 4 for _, W in K.EGRESS_BGR} == {0, 1, 2, 3} and {H % 2 for H, _ in K.EGRESS_BGR} == {0, 1}
    assert any(H < 2 for H, _ in K.EGRESS_BGR) and any(W < 4 for _, W in K.EGRESS_BGR)          # frames smaller than a patch
    assert all(H % 2 == 0 and W % 2 == 0 for H, W in K.EGRESS_I420) and {W % 4 for _, W in K.EGRESS_I420} == {0, 2}
    assert {W % 4 for _, W in K.BATCH_SHAPES} == {0, 2} and 17 in K.BATCH_NS
    for H, W in K.EGRESS_BGR + K.EGRESS_I420:
        wm = {n: (m, x, y) for n, m, x, y in K.watermarks(H, W)}
        assert wm["over_left"][1] < 0 and wm["over_top"][2] < 0
        assert wm["over_right"][1] + wm["over_right"][0].shape[1] > W and wm["over_bottom"][2] + wm["over_bottom"][0].shape[0] > H
        m, x, y = wm["covers_all"]
        assert x < 0 and y < 0 and x + m.shape[1] > W and y + m.shape[0] > H and m.all()
        assert wm["odd_start"][1] % 2 == 1 and wm["odd_start"][2] % 2 == 1
    col = K.colour_frame().reshape(-1, 3)
    assert {tuple(c) for c in col[:8].tolist()} == {(b, g, r) for b in (0, 255) for g in (0, 255) for r in (0, 255)}
    assert all((col[8 + v] == v).all() for v in range(256)) and len(col) >= 8 + 256 + 65536
    _, prev, src = K.egress_frames(6, 10)[0]
    s = K.weighted_f64(prev, src, 0.5)
    assert np.all(s == 127.5)
    for n in K.MEL_SAMPLES:
        names = {w[0] for w in K.mel_windows(n)}
        assert {"first", "last", "both", "thrice", "descending", "every", "n1024"} <= names
        n_cols = 1 + n // 200
        for name, st in K.mel_windows(n):
            assert st and len(st) <= 1024 and min(st) >= 0 and max(st) + 16 <= n_cols, name
        assert len(dict(K.mel_windows(n))["n1024"]) == 1024
    d = dict(K.mel_windows(16640))
    assert d["descending"] == sorted(d["descending"], reverse=True) and d["far_apart"][1] - d["far_apart"][0] > 16


# ----------------------------------------------------------------------------------------------------------------- restatement vs float64
def _each_resize(S, every: int = 1):
    """(source image, dw, dh) of every distinct (box, kind of image) of the family, explicit boxes first; sources are the table's own.  every > 1: the
    explicit boxes and every n-th avatar of the sweep (the power checks need a catching case, not all of them)."""
    groups = K.paste_groups(S)
    groups = [g for i, g in enumerate(groups) if g.name.startswith("box") or i % every == 0]
    for g in sorted(groups, key=lambda g: not g.name.startswith("box")):
        inp = K.paste_inputs(g)
        done = set()
        for i, (x1, y1, x2, y2) in enumerate(g.boxes):
            key = (x2 - x1, y2 - y1, i == 0)       # prediction 0 is the checkerboard: an explicit box is tried on it and on a random one
            if key in done:
                continue
            done.add(key)
            yield K.paste_source(g, inp, i), x2 - x1, y2 - y1


@pytest.mark.parametrize("S", [K.W2L_S, K.UL_S])
def test_resize_restatement_under_one_lsb_of_float64(S):
    worst, at, n = 0.0, None, 0
    for src, dw, dh in _each_resize(S):
        d = float(np.abs(po.resize_linear_u8(src, (dw, dh)).astype(np.float64) - K.resize_f64(src, dw, dh)).max())
        n += 1
        if d > worst:
            worst, at = d, (dw, dh)
    print(f"[delivery] resize S={S}: {n} boxes, worst |restatement - float64| = {worst:.3f} LSB at {at}")
    assert worst < 1.0


def test_blend_restatement_under_one_lsb_of_float64():
    """All (s1, s2, mask) triples, then every case of the table through paste_blend_frame's own stages."""
    s1, s2 = np.meshgrid(np.arange(256, dtype=np.uint8), np.arange(256, dtype=np.uint8), indexing="ij")
    s1, s2 = s1[:, :, None], s2[:, :, None]
    worst = 0.0
    for m in range(256):
        mk = np.full((256, 256), m, np.uint8)
        w1 = (mk / 255).astype(np.float32)
        o = po.blend_linear_u8(s1, s2, w1, 1 - w1).astype(np.float64)
        worst = max(worst, float(np.abs(o - K.blend_f64(s1, s2, mk)).max()))
    print(f"[delivery] blendLinear float32 vs the exact convex mix, all triples: worst {worst:.3f} LSB")
    assert worst < 1.0
    for H, W in K.MT_FRAMES:
        for c in K.blend_cases(H, W):
            got = po.paste_blend_frame(c.pred, c.frame, c.face, c.mask, c.crop)
            d = float(np.abs(got.astype(np.float64) - K.blend_stage_f64(c)).max())
            assert d < 1.0, (c.name, d)


def test_weighted_sum_restatement_under_one_lsb_of_float64():
    a, b = np.meshgrid(np.arange(256, dtype=np.uint8), np.arange(256, dtype=np.uint8), indexing="ij")
    worst = 0.0
    for alpha in K.ALPHAS + (0.37, 0.75):
        o = eo.add_weighted_u8(a, 1 - alpha, b, alpha).astype(np.float64)
        worst = max(worst, float(np.abs(o - K.weighted_f64(a, b, alpha)).max()))
    print(f"[delivery] addWeighted float32 vs float64, all byte pairs: worst {worst:.3f} LSB")
    assert worst < 1.0
    for H, W in K.EGRESS_BGR + K.EGRESS_I420:
        for _, prev, src in K.egress_frames(H, W):
            for alpha in K.ALPHAS:
                assert np.abs(eo.add_weighted_u8(prev, 1 - alpha, src, alpha) - K.weighted_f64(prev, src, alpha)).max() < 1.0


def test_yuv_restatement_under_one_lsb_of_float64():
    """All 2^24 colours through the integer matrix; the quad mean as its own stage; every I420 case of the table."""
    g, b = np.meshgrid(np.arange(256), np.arange(256), indexing="ij")
    worst = np.zeros(3)
    for r in range(256):
        bgr = np.stack([b, g, np.full_like(g, r)], axis=-1).astype(np.uint8)
        f = bgr.astype(np.int64)
        Y = ((eo.RY * f[..., 2] + eo.GY * f[..., 1] + eo.BY * f[..., 0] + 16384) >> 15) + 16
        U = ((eo.RU * f[..., 2] + eo.GU * f[..., 1] + eo.BU * f[..., 0] + 16384) >> 15) + 128
        V = ((eo.RV * f[..., 2] + eo.GV * f[..., 1] + eo.BV * f[..., 0] + 16384) >> 15) + 128
        for k, (a, ref) in enumerate(zip((Y, U, V), K.yuv_f64(bgr))):
            worst[k] = max(worst[k], float(np.abs(a - ref).max()))
    print(f"[delivery] swscale integer matrix vs float64 BT.601, all 2^24 colours: worst Y/U/V {worst[0]:.3f} / {worst[1]:.3f} / {worst[2]:.3f} LSB")
    assert worst.max() < 1.0
    col = K.colour_frame()
    q = (col.astype(np.int64)[0::2, 0::2] + col[0::2, 1::2] + col[1::2, 0::2] + col[1::2, 1::2] + 2) >> 2
    assert np.abs(q - K.quad_mean_f64(col)).max() <= 0.5
    for chroma in (0, 1):
        assert np.abs(eo.bgr_to_i420(col, chroma).astype(np.float64) - K.i420_f64(col, chroma)).max() < 1.0
        for H, W in K.EGRESS_I420:
            for _, prev, src in K.egress_frames(H, W):
                assert np.abs(eo.bgr_to_i420(src, chroma).astype(np.float64) - K.i420_f64(src, chroma)).max() < 1.0


# ----------------------------------------------------------------------------------------------------------------- power: resize mutants
def resize_mutant(src: np.ndarray, dw: int, dh: int, m: str) -> np.ndarray:
    """oracle/paste_oracle.py resize_linear_u8 with one planted fault `m` ("" = none: must equal the restatement everywhere)."""
    sh, sw, _ = src.shape
    f32 = np.float32
    if dw == sw and dh == sh:
        return src.copy()
    half = (sw == 2 * dw or sh == 2 * dh) if m == "avg_on_one_axis" else (sw == 2 * dw and sh == 2 * dh)
    if half and m != "no_avg":
        s = src.astype(np.int32)
        yy = np.minimum(2 * np.arange(dh), sh - 2)[:, None]         # the kernel's fixed (2 dy, 2 dx) reads, kept inside the image
        xx = np.minimum(2 * np.arange(dw), sw - 2)[None, :]
        return ((s[yy, xx] + s[yy, xx + 1] + s[yy + 1, xx] + s[yy + 1, xx + 1] + 2) >> 2).astype(np.uint8)

    def table(dst, s_):
        scale = np.float64(f32(s_) / f32(dst)) if m == "f32_scale" else np.float64(s_) / np.float64(dst)
        d = np.arange(dst, dtype=np.float64)
        f = ((d * scale) if m == "no_centre" else ((d + 0.5) * scale - 0.5)).astype(f32)
        s = np.floor(f).astype(np.int64)
        return s, (f - s.astype(f32)).astype(f32)

    def coefs(f):
        c0 = (f32(1.0) - f).astype(f32)
        if m == "trunc_coef":
            return np.floor(c0 * f32(2048)).astype(np.int64), np.floor(f * f32(2048)).astype(np.int64)
        return np.rint(c0 * f32(2048)).astype(np.int64), np.rint(f * f32(2048)).astype(np.int64)

    def clamp(s, f, n):
        lo = s < 0
        f = np.where(lo, f32(0), f); s = np.where(lo, 0, s)
        hi = s >= n - 1
        return np.where(hi, n - 1, s), np.where(hi, f32(0), f).astype(f32)

    sx, fx = table(dw, sw)
    sx, fx = clamp(sx, fx, sw)
    ax0, ax1 = coefs(fx)
    sx1 = np.minimum(sx + 1, sw - 1)
    sy, fy = table(dh, sh)
    if m == "clamp_fy":
        sy, fy = clamp(sy, fy, sh)
    by0, by1 = coefs(fy)
    s = src.astype(np.int64)
    rows = s[:, sx, :] * ax0[None, :, None] + s[:, sx1, :] * ax1[None, :, None]
    sy0 = np.clip(sy, 0, sh - 1)
    if m == "no_last_row_clamp":                # row sh is whatever lies behind the image: zeros here
        rows = np.concatenate([rows, np.zeros_like(rows[:1])])
        sy1 = np.clip(sy + 1, 0, sh)
    else:
        sy1 = np.clip(sy + 1, 0, sh - 1)
    out = (((by0[:, None, None] * (rows[sy0] >> 4)) >> 16) + ((by1[:, None, None] * (rows[sy1] >> 4)) >> 16) + 2) >> 2
    return np.clip(out, 0, 255).astype(np.uint8)


RESIZE_MUTANTS = ("clamp_fy", "f32_scale", "trunc_coef", "avg_on_one_axis", "no_last_row_clamp", "no_centre")
# a planted fault the float64 gate must see (it moves a pixel by more than a rounding) / one it cannot see (it IS a rounding)
F64_MUST_CATCH = ("no_centre", "avg_on_one_axis", "no_last_row_clamp")
F64_ESCAPES = ("f32_scale", "trunc_coef", "clamp_fy")


def test_resize_mutant_none_is_the_restatement():
    for S in (K.W2L_S, K.UL_S):
        for src, dw, dh in _each_resize(S, every=4):
            assert np.array_equal(resize_mutant(src, dw, dh, ""), po.resize_linear_u8(src, (dw, dh))), (S, dw, dh)


def test_missing_2x2_average_is_not_a_fault():
    """"The 2x2 average missing" cannot be caught, by either gate: at an exact 2x shrink the general path IS the average, byte for byte.
    Source coordinate 2 d + 0.5 gives taps (2 d, 2 d + 1) with coefficients 1024 / 1024 on both axes (no clamp applies: 2 d + 1 <= S - 1),
    so S0 = 1024 (p00 + p01), (1024 * (S0 >> 4)) >> 16 = p00 + p01 exactly, and the result is (p00 + p01 + p10 + p11 + 2) >> 2.  The
    shortcut is an optimisation with no arithmetic of its own; what CAN go wrong with it is taking it for the wrong box (next mutant)."""
    for S in (K.W2L_S, K.UL_S):
        rng = np.random.default_rng(S)
        for src in (rng.integers(0, 256, (S, S, 3), dtype=np.uint8), K.checkerboard(S, S)):
            assert np.array_equal(resize_mutant(src, S // 2, S // 2, "no_avg"), po.resize_linear_u8(src, (S // 2, S // 2)))


@pytest.mark.parametrize("m", RESIZE_MUTANTS)
def test_resize_gates_catch_the_mutant(m):
    """The byte gate catches every mutant on some case of the table; the float64 gate those it should; the escapes stay under 1 LSB on
    every case they were tried on, which is what the byte gate is for."""
    exact_at = f64_at = None
    worst = 0.0
    for src, dw, dh in _each_resize(K.W2L_S, every=4):
        got = resize_mutant(src, dw, dh, m)
        if exact_at is None and not np.array_equal(got, po.resize_linear_u8(src, (dw, dh))):
            exact_at = (dw, dh)
        d = float(np.abs(got.astype(np.float64) - K.resize_f64(src, dw, dh)).max())
        worst = max(worst, d)
        if f64_at is None and d >= 1.0:
            f64_at = (dw, dh, d)
        if exact_at and (f64_at or m not in F64_MUST_CATCH) and m not in F64_ESCAPES:
            break
    print(f"[delivery] resize mutant {m}: byte gate caught at {exact_at}, float64 gate {('caught at %s' % (f64_at,)) if f64_at else 'escaped, worst %.3f LSB' % worst}")
    assert exact_at is not None, f"the byte gate never catches {m}"
    if m in F64_MUST_CATCH:
        assert f64_at is not None, f"the float64 gate never catches {m}"
    if m in F64_ESCAPES:
        assert f64_at is None and worst < 1.0


# ----------------------------------------------------------------------------------------------------------------- power: blend, YUV, chroma
def _blend_mutant(c, m: str) -> np.ndarray:
    x1, y1, x2, y2 = c.face
    xs, ys, xe, ye = c.crop
    body = c.frame.copy()
    fl = body[ys:ye, xs:xe].copy()
    fl[y1 - ys:y2 - ys, x1 - xs:x2 - xs] = po.resize_linear_u8(c.pred, (x2 - x1, y2 - y1))
    gray = c.mask[:, :, 1 if m == "mask_channel_1" else 0]
    w1 = (gray / 255).astype(np.float32)
    w2 = np.float32(1) - w1
    s1, s2 = fl.astype(np.float32), body[ys:ye, xs:xe].astype(np.float32)
    den = (w1 + w2) + (np.float32(0) if m == "no_eps" else np.float32(1e-5))
    if m == "fma":          # fma(s1, w1, s2 * w2): the first product unrounded, one rounding of the sum
        num = (s1.astype(np.float64) * w1[..., None].astype(np.float64) + (s2 * w2[..., None]).astype(np.float64)).astype(np.float32)
    else:
        num = s1 * w1[..., None] + s2 * w2[..., None]
    body[ys:ye, xs:xe] = np.clip(np.rint(num / den[..., None]), 0, 255).astype(np.uint8)
    return body


@pytest.mark.parametrize("m", ["fma", "no_eps", "mask_channel_1"])
def test_blend_gates_catch_the_mutant(m):
    caught, f64 = [], []
    for H, W in K.MT_FRAMES:
        for c in K.blend_cases(H, W):
            assert np.array_equal(_blend_mutant(c, ""), po.paste_blend_frame(c.pred, c.frame, c.face, c.mask, c.crop))
            got = _blend_mutant(c, m)
            if not np.array_equal(got, po.paste_blend_frame(c.pred, c.frame, c.face, c.mask, c.crop)):
                caught.append(c.name)
            if np.abs(got.astype(np.float64) - K.blend_stage_f64(c)).max() >= 1.0:
                f64.append(c.name)
    print(f"[delivery] blend mutant {m}: byte gate caught on {sorted(set(caught))}, float64 gate on {sorted(set(f64))}")
    assert caught, f"the byte gate never catches {m}"
    if m == "mask_channel_1":
        assert "crop_bottom" in f64            # a wrong mask is not a rounding
    else:
        assert not f64                          # a rounding-level fault: only the byte gate sees it


def _i420_mutant(frame, chroma, m):
    f = frame.astype(np.int64)
    rnd = 0 if m == "trunc" else 16384
    gy = eo.GY + (1 if m == "coef" else 0)
    b, g, r = f[..., 0], f[..., 1], f[..., 2]
    Y = ((eo.RY * r + gy * g + eo.BY * b + rnd) >> 15) + 16
    q = ((f[0::2, 0::2] + f[0::2, 1::2] + f[1::2, 0::2] + f[1::2, 1::2] + (0 if m == "mean_no_round" else 2)) >> 2) if chroma else f[0::2, 0::2]
    U = ((eo.RU * q[..., 2] + eo.GU * q[..., 1] + eo.BU * q[..., 0] + rnd) >> 15) + 128
    V = ((eo.RV * q[..., 2] + eo.GV * q[..., 1] + eo.BV * q[..., 0] + rnd) >> 15) + 128
    return np.concatenate([Y.reshape(-1), U.reshape(-1), V.reshape(-1)]).astype(np.uint8).reshape(frame.shape[0] * 3 // 2, frame.shape[1])


@pytest.mark.parametrize("m", ["trunc", "coef", "mean_no_round"])
def test_yuv_gates_catch_the_mutant(m):
    col = K.colour_frame()
    assert np.array_equal(_i420_mutant(col, 1, ""), eo.bgr_to_i420(col, 1)) and np.array_equal(_i420_mutant(col, 0, ""), eo.bgr_to_i420(col, 0))
    got = _i420_mutant(col, 1, m)
    assert not np.array_equal(got, eo.bgr_to_i420(col, 1)), f"the byte gate never catches {m}"
    d = float(np.abs(got.astype(np.float64) - K.i420_f64(col, 1)).max())
    print(f"[delivery] yuv mutant {m}: byte gate caught, worst distance to float64 {d:.3f} LSB")
    if m == "mean_no_round":                    # the matrix of a truncated mean against the matrix of the rounded one: up to a whole chroma step
        q = (col.astype(np.int64)[0::2, 0::2] + col[0::2, 1::2] + col[1::2, 0::2] + col[1::2, 1::2]) >> 2
        assert np.abs(q - K.quad_mean_f64(col)).max() == 0.75      # a correct mean is within 0.5
    if m == "coef":                             # a coefficient off by one moves a sample by 255 / 2^15: only the byte gate sees it
        assert d < 1.0


# ----------------------------------------------------------------------------------------------------------------- mel
@pytest.mark.parametrize("signal", K.MEL_SIGNALS)
def test_mel_two_float64_statements_agree(signal):
    gap = K.mel_statement_gap(signal)
    tol = max(K.MEL_FLOOR_TOL, 4 * gap)
    print(f"[delivery] mel {signal}: direct DFT vs rFFT statement, worst {gap:.3e}; device tolerance {tol:.3e} "
          f"({'floor' if tol == K.MEL_FLOOR_TOL else '4 x gap'})")
    assert gap < 1e-6, "two float64 statements of one chain should agree far below the float32 store"
    wav = K.mel_signal(signal, 3200)
    assert np.array_equal(np.clip(K.mel_unclipped_f64(wav), -4, 4), mel_oracle.melspectrogram(wav))
