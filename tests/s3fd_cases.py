"""Cases, float64 references, float32 rounding models and bounds of the face detector's own kernels (csrc/s3fd_kernels.hip through
include/ltk.h ltk_s3fd_stem_f16, ltk_maxpool2x2s2_f16, ltk_l2norm_f16, ltk_s3fd_detect_f16), and the network-level cases of the
detector (sizes, seeded weights and frames, the fp16 rounding model of the whole launch list and the end-to-end bounds tau_s / tau_b).
CPU code; tests/test_face_detect_host.py holds the models and a simulated device with planted faults to the gates,
tests/test_s3fd_kernels_gpu.py holds the device to the same gates.

Every op is compared on the DEVICE's own inputs (what the test uploaded), so `dev - ref` is that op's error alone.  Per op:

  ref : float64, the reference's arithmetic (torch CPU), unrounded weights;
  mod : the kernel's arithmetic restated in float32 - fp16 weights where the kernel rounds them, fp32 sums, one fp16 rounding;
  tol : per element, in the forms of oracle/op_replay.py:
        stem     2^-10 |ref| + (2^-12 short_sum(27) + 2^-19) |W| (*) |x| + 2^-22 |bias| + 2^-24, x the reversed, mean-subtracted frame
                 (integers: exact in fp16, so only the weights are rounded), zero outside it.  2^-19: 32 fp32 accumulation steps of
                 2^-24 each, whatever order the MFMA sums its 32 products in.
        maxpool  exact: dev == ref.
        l2norm   2^-10 |ref| + 2^-14 |ref| + 2^-24.  The sum of C <= 512 non-negative squares in fp32, one after the other, is good to
                 C 2^-24 <= 2^-15 relative, its root to 2^-16; the reciprocal and the two products add 4 x 2^-24: 2^-14 has room.
        detect   score: 2^-20 absolute (two expf good to 2^-22 relative, a sum, a quotient, all at most 1);
                 box: 2^-19 M, M = |prior centre| + 0.1 size |loc| + size exp(0.2 loc): 8 fp32 roundings and an expf good to 2^-22 stay
                 below 16 x 2^-24 = 2^-20 of the largest intermediate, with a factor 2 of room.
                 Candidate set: a position whose float64 score is within 2^-20 of the threshold may be on either side; every other
                 one has to agree.  A score EXACTLY at the threshold (equal logits, threshold 0.5) is exact on both sides: no record.
Gates (check()): no element beyond tol; rel_l2(dev, ref) <= 2 rel_l2(mod, ref) + 1e-4; the model itself within 0.5 tol.
"""
from __future__ import annotations

import math

import numpy as np
import torch
import torch.nn.functional as F

import s3fd_ref as R
from faceparse_cases import check, f16, from_cb16, model_inside, to_cb16  # noqa: F401  (the layout and the gates are the parser's)
from oracle.op_replay import C_LIN, F16_FLOOR, short_sum

REC_WORDS = 6


# ------------------------------------------------------------------------------------------ stem
# 37 x 53: odd, 3 x 4 blocks, every edge tile partial; 20 x 1 and 1 x 1: a one-pixel-wide image (padding on both sides of every tap row)
STEM_SHAPES = [(2, 37, 53), (1, 20, 1), (1, 1, 1), (3, 16, 16)]


class Stem:
    """Seeded inputs of one conv1_1 call: a smooth BGR frame plus noise (both saturate), fan-in scaled weights, a bias."""

    def __init__(self, N, H, W, seed=0):
        g = np.random.default_rng(2000 + seed + 7 * N + H)
        yy, xx = np.mgrid[0:H, 0:W]
        base = 128 + 100 * np.sin(yy[None, :, :, None] / 5.0 + np.arange(N)[:, None, None, None]) * np.cos(xx[None, :, :, None] / 7.0 + np.arange(3))
        self.bgr = np.clip(base + g.normal(0, 40, (N, H, W, 3)), 0, 255).astype(np.uint8)
        self.bgr[:, 0, 0] = 0                                        # the extremes of the input range at the corners
        self.bgr[:, -1, -1] = 255
        self.w = g.normal(0, math.sqrt(2.0 / 27) / 64, (64, 3, 3, 3)).astype(np.float32)
        self.bias = g.normal(0, 0.3, 64).astype(np.float32)
        self.N, self.H, self.W = N, H, W

    def ref_tol(self):
        x, W, b = R.preprocess(self.bgr), torch.from_numpy(self.w).double(), torch.from_numpy(self.bias).double()
        ref = F.relu(F.conv2d(x, W, b, padding=1))
        A = F.conv2d(x.abs(), W.abs(), None, padding=1)
        tol = 2.0 ** -10 * ref.abs() + (C_LIN * short_sum(27) + 2.0 ** -19) * A + 2.0 ** -22 * b.abs().view(1, -1, 1, 1) + F16_FLOOR
        return ref.numpy(), tol.numpy()

    def model(self, fault: str = "") -> np.ndarray:
        """The kernel in float32 (NCHW, float16-representable).  `fault`: "not_reversed" (the bytes are taken as they come),
        "means_unreversed" (reversed, but the means go with the bytes' own channels), "zero_byte_pad" (the BYTE is padded)."""
        x = R.preprocess(self.bgr, torch.float32)
        m = torch.tensor(R.MEANS).view(1, 3, 1, 1)
        if fault == "not_reversed":
            x = torch.from_numpy(self.bgr.copy()).float().permute(0, 3, 1, 2) - m
        elif fault == "means_unreversed":
            x = x + m - m.flip(1)
        W, b = f16(torch.from_numpy(self.w)), torch.from_numpy(self.bias)
        if fault == "zero_byte_pad":
            y = F.conv2d(F.pad(x + m, (1, 1, 1, 1)) - m, W, b)
        else:
            y = F.conv2d(x, W, b, padding=1)
        return f16(F.relu(y)).double().numpy()


# ------------------------------------------------------------------------------------------ max pool
POOL_SHAPES = [(2, 32, 7, 9), (1, 16, 8, 12), (1, 16, 2, 3), (1, 64, 33, 64)]      # odd: a row and a column dropped; 33 x 64: several blocks


def pool_input(N, C, H, W) -> np.ndarray:
    g = np.random.default_rng(2100 + H)
    return g.normal(-1.0, 2.0, (N, C, H, W)).astype(np.float16).astype(np.float64)     # negative maxima too


def pool_ref(x: np.ndarray, ceil_mode: bool = False) -> np.ndarray:
    return F.max_pool2d(torch.from_numpy(x), 2, 2, ceil_mode=ceil_mode).numpy()


# ------------------------------------------------------------------------------------------ L2Norm
NORM_SHAPES = [(2, 256, 300), (1, 512, 77)]                                           # (N, C, P): 300 pixels = two blocks


def norm_input(N, C, P):
    """x (N, C, P, 1) float16-representable: unit-scale post-ReLU features; pixel 0 all zeros (only eps is left in the denominator),
    pixel 1 values up to 4096 (an fp16 square would overflow), pixel 2 one non-zero channel.  weight (C,) around 10."""
    g = np.random.default_rng(2200 + C)
    x = np.maximum(g.normal(0.2, 1.0, (N, C, P, 1)), 0)
    x[:, :, 0] = 0
    x[:, :, 1] = g.uniform(0, 4096, (N, C, 1))
    x[:, 0, 1] = 4096
    x[:, :, 2] = 0
    x[:, C // 2, 2] = 3.0
    return x.astype(np.float16).astype(np.float64), (10.0 * g.uniform(0.9, 1.1, C)).astype(np.float32)


def norm_ref_tol(x: np.ndarray, w: np.ndarray):
    ref = R.l2norm(torch.from_numpy(x), torch.from_numpy(w).double())
    tol = (2.0 ** -10 + 2.0 ** -14) * ref.abs() + F16_FLOOR
    return ref.numpy(), tol.numpy()


def norm_model(x: np.ndarray, w: np.ndarray, fault: str = "") -> np.ndarray:
    """fp32: squares summed channel after channel, 1 / (sqrt + eps), two products, one rounding.  `fault`: "f16_sum" (squares in fp16)."""
    xt = torch.from_numpy(x).float()
    ss = torch.zeros_like(xt[:, 0])
    for c in range(xt.shape[1]):
        sq = xt[:, c].double() * xt[:, c].double()
        if fault == "f16_sum":
            ss = (ss.half() + sq.half()).float()
        else:
            ss = (ss.double() + sq).float()                       # an FMA: the product is not rounded
    inv = (1.0 / (ss.sqrt() + torch.tensor(1e-10))).unsqueeze(1)
    return f16(xt * inv * torch.from_numpy(w).view(1, -1, 1, 1)).double().numpy()


# ------------------------------------------------------------------------------------------ detect
DETECT_CASES = [(0, True), (1, False), (2, False), (3, False), (4, False), (5, False), (0, False), (2, True)]     # (level, maxout)
DETECT_MAP = (9, 13)


def detect_input(level: int, maxout: bool, N: int = 2, hw=DETECT_MAP, seed: int = 0) -> np.ndarray:
    """A merged head map (N, 16, H, W), float16-representable: conf logits whose face score passes 0.05 at about a third of the
    positions (another third per image, so that two images' lists differ), loc at unit scale, channels 8..15 zero."""
    g = np.random.default_rng(2300 + 10 * level + int(maxout) + seed)
    H, W = hw
    x = np.zeros((N, 16, H, W))
    nconf = 4 if maxout else 2
    x[:, :nconf] = g.normal(0, 1.5, (N, nconf, H, W))
    x[:, nconf - 1] -= 2.5 + 0.5 * np.arange(N).reshape(N, 1, 1)
    if not maxout:
        x[:, 2:4] = g.normal(0, 5, (N, 2, H, W))                 # what a kernel that always applied the max-out would pick up
    x[:, 4:8] = g.normal(0, 1.0, (N, 4, H, W))
    return x.astype(np.float16).astype(np.float64)


def detect_ref(x: np.ndarray, maxout: bool, level: int, thresh: float):
    """Per image: dict key -> (row float64 (5,), box bound (4,)) of the positions above thresh, and the set of keys whose score is
    within 2^-20 of thresh."""
    t = torch.from_numpy(x)
    conf = torch.cat([t[:, 0:3].max(1, keepdim=True).values, t[:, 3:4]], 1) if maxout else t[:, 0:2]
    score = F.softmax(conf, dim=1)[:, 1]
    loc = t[:, 4:8].permute(0, 2, 3, 1)
    N, H, W = score.shape
    hh, ww = torch.meshgrid(torch.arange(H), torch.arange(W), indexing="ij")
    box = R.decode(loc, level, hh.double(), ww.double())
    stride = 2 ** (level + 2)
    size = 4.0 * stride
    M = (stride / 2 + torch.maximum(hh, ww) * stride).double() + 0.1 * size * loc[..., :2].abs().max(-1).values + \
        size * torch.exp(0.2 * loc[..., 2:]).max(-1).values
    res = []
    for n in range(N):
        rows, edge = {}, set()
        for h in range(H):
            for w in range(W):
                key = (level << 28) | (h << R.KEY_BITS) | w
                s = float(score[n, h, w])
                if abs(s - thresh) <= 2.0 ** -20 and s != thresh:
                    edge.add(key)
                if s > thresh:
                    rows[key] = (np.concatenate([box[n, h, w].numpy(), [s]]), float(2.0 ** -19 * M[n, h, w]))
        res.append((rows, edge))
    return res


def detect_model(x: np.ndarray, maxout: bool, level: int, thresh: float, fault: str = ""):
    """The kernel in float32: per image a list of (key, row (5,)) in row-major order.  `fault`: "no_maxout", "swapped" (conf and loc
    channels change places), "stride" (the next level's stride), "ge" (score >= thresh)."""
    t = torch.from_numpy(x).float()
    if fault == "swapped":
        t = torch.cat([t[:, 4:8], t[:, 0:4], t[:, 8:]], 1)
    if maxout and fault != "no_maxout":
        conf = torch.cat([t[:, 0:3].max(1, keepdim=True).values, t[:, 3:4]], 1)
    else:
        conf = t[:, 0:2]
    score = F.softmax(conf, dim=1)[:, 1]
    loc = t[:, 4:8].permute(0, 2, 3, 1)
    N, H, W = score.shape
    hh, ww = torch.meshgrid(torch.arange(H), torch.arange(W), indexing="ij")
    box = R.decode(loc, level + (1 if fault == "stride" else 0), hh.float(), ww.float())
    out = []
    for n in range(N):
        hit = (score[n] >= thresh) if fault == "ge" else (score[n] > thresh)
        out.append([((level << 28) | (int(h) << R.KEY_BITS) | int(w), np.concatenate([box[n, h, w].double().numpy(), [float(score[n, h, w])]]))
                    for h, w in zip(*np.where(hit.numpy()))])
    return out


def detect_check(records, ref, cap=None) -> dict:
    """records: per image a list of (key, row); ref: detect_ref's.  The gates of the docstring; with `cap`, records may be any `cap`
    of the float64 candidates.  -> figures."""
    worst_s = worst_b = 0.0
    for n, (recs, (rows, edge)) in enumerate(zip(records, ref)):
        keys = [k for k, _ in recs]
        assert len(set(keys)) == len(keys), f"image {n}: a position is listed twice"
        extra = set(keys) - set(rows) - edge
        assert not extra, f"image {n}: {len(extra)} records at positions float64 does not list (first key {sorted(extra)[0]:#x})"
        if cap is None:
            missing = set(rows) - set(keys) - edge
            assert not missing, f"image {n}: {len(missing)} float64 candidates are missing (first key {sorted(missing)[0]:#x})"
        else:
            assert len(keys) == min(cap, len(keys)) and len(keys) <= cap
        for k, row in recs:
            if k not in rows:
                continue
            r, tb = rows[k]
            assert np.isfinite(row).all()
            worst_s = max(worst_s, abs(row[4] - r[4]) / 2.0 ** -20)
            worst_b = max(worst_b, float(np.abs(row[:4] - r[:4]).max()) / tb)
    assert worst_s <= 1.0 and worst_b <= 1.0, f"score error reaches {worst_s:.3f} of its bound, box error {worst_b:.3f}"
    return dict(worst_s=worst_s, worst_b=worst_b)


def unpack_records(recs_u32: np.ndarray, counts: np.ndarray, cap: int):
    """Device buffers (N, cap, 6) uint32 + counts (N,) -> per image a list of (key, row float64 (5,)) sorted by key."""
    out = []
    for n in range(recs_u32.shape[0]):
        k = min(int(counts[n]), cap)
        r = recs_u32[n, :k]
        order = np.argsort(r[:, 0], kind="stable")
        vals = np.ascontiguousarray(r[:, 1:]).view(np.float32).astype(np.float64)
        out.append([(int(r[i, 0]), vals[i]) for i in order])
    return out


# ========================================================================================== the whole detector
# (H, W) -> the frame seeds of the case (synth_inputs.s3fd_frame), run as one call with max_images = 2: a 2-image chunk and a short tail.
#   64 x 64   maps 64 .. 2 x 2, then 6 x 6 (fc7), 3 x 3, 2 x 2; frame 0 has no score above 0.5 (the frame without a face)
#   72 x 104  pooled maps 9 x 13 -> 4 x 6 -> 2 x 3: floor pooling drops a row and a column, every conv tile is partial
#   180 x 320 45 x 80 -> 22 x 40; once, against the stored results
SEED = 29
NET_CASES = {(64, 64): (0, 1, 3), (72, 104): (0, 1, 2), (180, 320): (0, 1)}
THRESH = 0.05
NEAR_CAP = 0.05          # at most this share of an image's candidates within tau_s of the threshold (the cap the face parser's gate uses)


def state_dict(dtype=torch.float64):
    import synth_inputs as synth
    return {k: torch.from_numpy(v).to(dtype) for k, v in synth.s3fd_state_dict(SEED).items()}


def frames(hw):
    import synth_inputs as synth
    return np.stack([synth.s3fd_frame(hw[0], hw[1], s) for s in NET_CASES[tuple(hw)]])


def model_op(name: str, sd32, x: torch.Tensor, op: dict) -> torch.Tensor:
    """One launch of the list in the device's arithmetic, float32 on a float16-representable input: fp16 weights, fp32 sums, fp32 bias,
    one fp16 rounding (the stem sees the integer frame; pools are exact; L2Norm as norm_model)."""
    t = op["type"]
    if t in (0, 20):
        if op["level"] >= 0:
            w, b = R.merged_head(sd32, op["level"])
        else:
            w, b = sd32[name + ".weight"], sd32[name + ".bias"]
        y = F.conv2d(x, f16(w), b, stride=op["stride"], padding=op["pad"])
        return f16(F.relu(y) if op["relu"] else y)
    if t == 21:
        return F.max_pool2d(x, 2, 2)
    if t == 22:
        n, c, h, w_ = x.shape
        return torch.from_numpy(norm_model(x.reshape(n, c, h * w_, 1).double().numpy(), sd32[name + ".weight"].numpy())).float().reshape(n, c, h, w_)
    raise ValueError(name)


def model_walk(sd32, bgr: np.ndarray, program) -> dict:
    """The fp16 rounding chain through the launch list (program = Engine.face_detect_program's dicts): name -> float32 tensor."""
    out, src = {}, R.preprocess(bgr, torch.float32)
    cur = src
    for op in program:
        n = op["name"]
        if op["type"] == 23:
            continue
        if op["type"] == 22 or op["level"] >= 0:
            x = out[n[:-5]]                                   # "<source>_norm", "<source>[_norm]_mbox"
        else:
            x = cur
        out[n] = model_op(n, sd32, x, op)
        if op["type"] != 22 and op["level"] < 0:
            cur = out[n]
    return out


def dense(heads):
    """The six merged head maps -> per level (score (N, H, W), box (N, H, W, 4)) at EVERY position, in the maps' dtype."""
    ol = R.olist_from_heads(heads)
    res = []
    for i in range(6):
        score = F.softmax(ol[2 * i], dim=1)[:, 1]
        N, H, W = score.shape
        hh, ww = torch.meshgrid(torch.arange(H), torch.arange(W), indexing="ij")
        res.append((score, R.decode(ol[2 * i + 1].permute(0, 2, 3, 1), i, hh.to(score.dtype), ww.to(score.dtype))))
    return res


def taus(ref_heads, mod_heads, thresh=THRESH):
    """tau_s = 2 max |score_mod - score_ref| over every position; tau_b = 2 max |box_mod - box_ref| over the positions either lists."""
    ts = tb = 0.0
    for (sr, br), (sm, bm) in zip(dense(ref_heads), dense([m.double() for m in mod_heads])):
        ts = max(ts, float((sm - sr).abs().max()))
        either = (sr > thresh) | (sm > thresh)
        if bool(either.any()):
            tb = max(tb, float((bm - br).abs()[either].max()))
    return 2 * ts, 2 * tb


def dense_scores(heads):
    """The six merged head maps (or the twelve tensors of s3fd.forward) -> per level the float64 score at EVERY position, (N, H, W)."""
    ol = R.olist_from_heads(heads) if len(heads) == 6 else heads
    return [F.softmax(ol[2 * i].double(), dim=1)[:, 1] for i in range(6)]


def check_candidates(dev, ref, dense_ref, tau_s: float, tau_b: float, thresh=THRESH) -> dict:
    """dev, ref: per image (keys, rows (k, 5)); dense_ref: dense_scores() of the float64 heads.  The device's set holds every float64
    candidate above thresh + tau_s; EVERY device record, listed by float64 or not, sits at a position whose float64 score is at least
    thresh - tau_s and within tau_s of the device's; common candidates agree within tau_b."""
    worst_s = worst_b = 0.0
    for n, ((dk, dr), (rk, rr)) in enumerate(zip(dev, ref)):
        for k, row in zip(dk, dr):
            level, h, w = int(k) >> 28, (int(k) >> R.KEY_BITS) & ((1 << R.KEY_BITS) - 1), int(k) & ((1 << R.KEY_BITS) - 1)
            assert level < 6 and h < dense_ref[level].shape[1] and w < dense_ref[level].shape[2], f"image {n}: key {int(k):#x} names no position"
            s = float(dense_ref[level][n, h, w])
            assert s >= thresh - tau_s, f"image {n}: a record at key {int(k):#x}, where float64 scores {s:.5f}, below thresh - tau_s"
            assert abs(float(row[4]) - s) <= tau_s, f"image {n}: key {int(k):#x} scores {float(row[4]):.5f}, float64 {s:.5f} (tau_s {tau_s:.2e})"
            worst_s = max(worst_s, abs(float(row[4]) - s))
        d = {int(k): r for k, r in zip(dk, dr)}
        r_ = {int(k): r for k, r in zip(rk, rr)}
        assert len(d) == len(dk), f"image {n}: a position is listed twice"
        assert list(dk) == sorted(dk), f"image {n}: the records are not in key order"
        missing = [k for k, r in r_.items() if r[4] > thresh + tau_s and k not in d]
        assert not missing, f"image {n}: {len(missing)} float64 candidates above thresh + tau_s are missing"
        for k in set(d) & set(r_):
            worst_b = max(worst_b, float(np.abs(np.asarray(d[k][:4], np.float64) - r_[k][:4]).max()))
    assert worst_s <= tau_s and worst_b <= tau_b, f"common candidates: score {worst_s:.3e} (tau_s {tau_s:.3e}), box {worst_b:.3e} (tau_b {tau_b:.3e})"
    return dict(worst_s=worst_s, worst_b=worst_b)


def check_boxes(dev_boxes, ref_faces, tau_b: float):
    """Final integer boxes: equal to float64's wherever no float64 coordinate lies within tau_b of an integer, within 1 otherwise.
    ref_faces: per image the float64 kept rows (first one is the box), or an empty list."""
    for n, (db, faces) in enumerate(zip(dev_boxes, ref_faces)):
        if len(faces) == 0:
            assert db is None, f"image {n}: a face where float64 has none"
            continue
        assert db is not None, f"image {n}: no face"
        f = np.clip(np.asarray(faces[0][:4], np.float64), 0, None)
        for c in range(4):
            near = abs(f[c] - np.rint(f[c])) <= tau_b
            assert abs(db[c] - int(f[c])) <= (1 if near else 0), f"image {n}: coordinate {c} is {db[c]}, float64 {f[c]:.4f}"


class SimEngine:
    """A stand-in engine whose face_detect is the float64 restatement (or any callable olist = net(bgr))."""

    def __init__(self, sd=None, net=None):
        self.sd = sd if sd is not None else state_dict()
        self.net = net or (lambda bgr: R.net(self.sd, R.preprocess(bgr)))
        self.calls = []

    def face_detect(self, frames_bgr, thresh=THRESH, cap=4096):
        self.calls.append(len(frames_bgr))
        return [rows.astype(np.float32) for _, rows in R.candidates(self.net(np.asarray(frames_bgr)), thresh)]


# ------------------------------------------------------------------------------------------ the binding table, replayed
def producer(name: str, op: dict, prev: str) -> str:
    """The launch whose output `name` reads: the trunk is a chain; "<source>_norm" and "<source>[_norm]_mbox" read their source;
    detect i reads level i's head."""
    if op["type"] == 23:
        return R.head_prefix(op["level"])
    if op["type"] == 22 or op["level"] >= 0:
        return name[:-5]
    return prev


def replay_through_views(plan, prog, sd32, bgr):
    """The six merged head maps (float32) after every launch has run as model_op runs it, on inputs taken from - and with its output
    stored into - buffers addressed by the plan's views alone.  A buffer remembers what its last writer made of it: reading it with
    another geometry, or after a later launch has written it, is a wiring fault of the plan."""
    arena, heads, prev = {}, {}, None

    def read(v, cin):
        if v["buf"] == plan["image_buf"]:
            return R.preprocess(bgr, torch.float32)
        a = arena[v["buf"]]
        assert (a["ld"], a["H"], a["W"]) == (v["ld"], v["H"], v["W"]), "a view reads a buffer its last writer shaped otherwise"
        return a["data"][:, v["coff"]:v["coff"] + cin]

    for o, p in zip(plan["ops"], prog):
        n = p["name"]
        if p["type"] == 23:
            assert o["y"] is None
            heads[p["level"]] = read(o["x"], 16)
            continue
        out = model_op(n, sd32, read(o["x"], p["cin"]), p)
        y = o["y"]
        assert y["buf"] != o["x"]["buf"], f"{n}: writes the buffer it reads"
        assert tuple(out.shape[1:]) == (p["cout"], y["H"], y["W"]) and y["C"] == p["cout"] and y["coff"] == 0, f"{n}: the output does not fit its view"
        arena[y["buf"]] = dict(ld=y["ld"], H=y["H"], W=y["W"], data=out)
    return [heads[i] for i in range(6)]


# ------------------------------------------------------------------------------------------ op by op on the device's own inputs
def conv_ref_tol(x, W, b, stride, pad, relu):
    """float64 tensors; -> (ref, tol): oracle/op_replay.py's dense conv form with the bias as the epilogue's shift,
    2^-10 |ref| + 2^-12 (short_sum(n) |W| (*) |x| + 4 |b|) + 2^-24 sum |x| + 2^-24.  A merged head's zero rows are exact zeros."""
    k = W.shape[-1]
    kw = dict(stride=stride, padding=pad)
    ref = F.conv2d(x, W, b, **kw)
    A = short_sum(W.shape[1] * k * k) * F.conv2d(x.abs(), W.abs(), None, **kw) + 4 * b.abs().view(1, -1, 1, 1)
    s = 2.0 ** -24 * F.conv2d(x.abs().sum(1, keepdim=True), torch.ones(1, 1, k, k, dtype=torch.float64), None, **kw)
    if relu:
        ref = F.relu(ref)
    return ref, 2.0 ** -10 * ref.abs() + C_LIN * A + s + F16_FLOOR


def check_ops(fetch, plan, prog, sd, bgr, records, thresh=THRESH):
    """fetch(name, shape) -> the device's float32 output of launch `name`; bgr: the frames of the run that is read back; records: per
    image (keys, rows) as the call returned them.  Every launch of the list against float64 on the device's own input, the detect
    launches through the records of their level.  -> {name: figures}; raises AssertionError naming the launch."""
    sd32 = {k: v.float() for k, v in sd.items()}
    N = bgr.shape[0]
    cache, figs, prev = {}, {}, None
    ybind = {o["name"]: o["y"] for o in plan["ops"]}

    def dev_of(p):
        n = p["name"]
        if n not in cache:
            shape = (N, p["cout"], p["Ho"], p["Wo"])
            got = np.asarray(fetch(n, shape), np.float32)
            assert got.shape == shape and np.isfinite(got).all(), n
            assert np.array_equal(got.astype(np.float16).astype(np.float32), got), f"{n}: not fp16 values"
            cache[n] = got
        return cache[n]

    by_name = {p["name"]: p for p in prog}
    for o, p in zip(plan["ops"], prog):
        n, t = p["name"], p["type"]
        try:
            if t == 20:
                assert o["x"]["buf"] == plan["image_buf"]
                c = object.__new__(Stem)
                c.bgr, c.w, c.bias = np.ascontiguousarray(bgr), sd32[n + ".weight"].numpy(), sd32[n + ".bias"].numpy()
                ref, tol = c.ref_tol()
                figs[n] = check(dev_of(p).astype(np.float64), ref, c.model(), tol)
                prev = n
                continue
            src = producer(n, p, prev)
            assert o["x"] == ybind[src], f"the plan binds the input to something else than {src}'s output"
            x = torch.from_numpy(dev_of(by_name[src]).astype(np.float64))
            if t == 23:
                ref = detect_ref(x.numpy(), bool(p["maxout"]), p["level"], thresh)
                got = [[(int(k), np.asarray(r, np.float64)) for k, r in zip(keys, rows) if int(k) >> 28 == p["level"]] for keys, rows in records]
                figs[n] = detect_check(got, ref)
                continue
            dev = dev_of(p).astype(np.float64)
            if t == 21:
                assert np.array_equal(dev, pool_ref(x.numpy())), "max pool is not exact"
                figs[n] = dict(worst=0.0)
            elif t == 22:
                w = sd32[n + ".weight"].numpy()
                xs = x.numpy().reshape(N, p["cin"], -1, 1)
                ref, tol = norm_ref_tol(xs, w)
                figs[n] = check(dev.reshape(ref.shape), ref, norm_model(xs, w), tol)
            else:
                W, b = R.merged_head(sd, p["level"]) if p["level"] >= 0 else (sd[n + ".weight"], sd[n + ".bias"])
                ref, tol = conv_ref_tol(x, W, b, p["stride"], p["pad"], p["relu"])
                figs[n] = check(dev, ref.numpy(), model_op(n, sd32, x.float(), p).double().numpy(), tol.numpy())
            if t != 22 and p["level"] < 0:
                prev = n
        except AssertionError as e:
            raise AssertionError(f"{n} (type {t}): {e}") from e
    return figs


class SimDevice:
    """A simulated device: the fp16 rounding chain of the launch list with, optionally, one planted wiring fault - "swapped" (conf and
    loc channels change places in detect), "no_maxout", "stride" (detect takes the next level's stride), "fc6_pad1", "ceil_pool",
    "not_reversed" (the stem takes the bytes as they come).  fetch / records as check_ops takes them."""

    def __init__(self, sd, bgr, prog, fault: str = "", thresh=THRESH):
        sd32 = {k: v.float() for k, v in sd.items()}
        self.out, cur = {}, R.preprocess(bgr, torch.float32)
        for p in prog:
            n, t = p["name"], p["type"]
            if t == 23:
                continue
            if t == 20 and fault == "not_reversed":
                c = object.__new__(Stem)
                c.bgr, c.w, c.bias = bgr, sd32[n + ".weight"].numpy(), sd32[n + ".bias"].numpy()
                y = torch.from_numpy(c.model("not_reversed")).float()
            elif t == 21 and fault == "ceil_pool":
                y = F.max_pool2d(cur, 2, 2, ceil_mode=True)
            else:
                q = dict(p, pad=1) if n == "fc6" and fault == "fc6_pad1" else p
                y = model_op(n, sd32, self.out[n[:-5]] if (t == 22 or p["level"] >= 0) else cur, q)
            self.out[n] = y
            if t != 22 and p["level"] < 0:
                cur = y
        self.records = None
        per_level = [detect_model(self.out[R.head_prefix(p["level"])].double().numpy(), bool(p["maxout"]), p["level"], thresh,
                                  fault if fault in ("swapped", "no_maxout", "stride") and (fault != "no_maxout" or p["maxout"]) else "")
                     for p in prog if p["type"] == 23]
        self.records = []
        for n in range(bgr.shape[0]):
            recs = sorted((kr for lv in per_level for kr in lv[n]), key=lambda kr: kr[0])
            self.records.append((np.asarray([k for k, _ in recs], np.uint32), np.asarray([r for _, r in recs], np.float64).reshape(-1, 5)))

    def fetch(self, name, shape):
        return self.out[name].numpy()
