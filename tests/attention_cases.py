"""What tests/test_attention_host.py (CPU) and tests/test_attention_gpu.py share: the shapes at which the attention kernels of
csrc/nn_kernels.hip change path, the input families, the CB16 buffers the kernels read and write, the gates, and a simulated device
that computes the op as the kernels do and can be told to get it wrong.

A case is (heads, d, Tq, Tk, N, impl); d is the real head dimension, d16 its padding to whole channel blocks (zero channels),
impl 1 = attn_kernel / attn_wide_kernel, impl 2 = attn_lds_kernel (ltk_attention_f16).  Logits are the plain q . k: the 1 / sqrt(d)
is folded into q, as the programs do.  Every family keeps |S| <= S_CAP = 100: the kernels form exp(S - max) from an fp32 S, whose
own rounding (|S| 2^-23 = 1.2e-5 relative on the probability) then stays far below the 2^-10 the bound allows.

Buffers (halfs, channel-blocked [N][cbt][T][16]), one allocation per case:
  Tq == Tk : [guard | q | guard | k | guard | v | guard]   one stacked tensor, as the to_qkv projections write it;
  Tq != Tk : [guard | q | guard] of Tq rows, then [guard | k | guard | v | guard] of Tk rows (the to_q / to_kv pair).
  A guard is one channel block of GUARD_GAIN x the magnitude of K, finite: a key row read past Tk lands in the next channel block
  (the address is (block * Tk + row) * 16), and with the guard behind K's last block such a leak dominates the softmax instead of
  hiding in it.
  o : [N][O_CB0 + heads * d16 / 16 + O_TAIL][Tq][16], pre-filled with PATTERN; the heads go to blocks [O_CB0, O_CB0 + heads * d16 / 16)."""
from __future__ import annotations

import math
from typing import Dict, List, Optional, Tuple

import numpy as np
import torch

from oracle import op_replay as R

S_CAP = 100.0
GUARD_GAIN = 1.0e3
PATTERN = 0x5A5A            # fp16 203.25
O_CB0, O_TAIL = 2, 3
FAMILIES = ("gauss", "sharp", "offset", "ascending", "descending", "dominant")
SLOT = (0, 1, 2, 3, 8, 9, 10, 11, 4, 5, 6, 7, 12, 13, 14, 15)     # MFMA B-operand slot order of a 16-key group (v_transpose_body)


class Case:
    def __init__(self, heads, d, Tq, Tk, N, impl):
        self.heads, self.d, self.Tq, self.Tk, self.N, self.impl = heads, d, Tq, Tk, N, impl
        self.d16 = (d + 15) // 16 * 16
        self.hcb = heads * self.d16 // 16

    @property
    def kernel(self) -> str:
        if self.impl == 2:
            return {48: "attn_lds_kernel<3,2>", 80: "attn_lds_kernel<5,3>"}[self.d16]
        return {48: "attn_kernel<3,2,true>", 64: "attn_kernel<4,2,true>", 80: "attn_kernel<5,3,true>", 160: "attn_kernel<10,5,false>",
                512: "attn_wide_kernel"}[self.d16]

    @property
    def ragged(self) -> bool:
        """A partial 32-row tile of keys or queries; for the LDS form, whose key tiles are whole by construction, a last block with
        fewer than its four query tiles."""
        return bool(self.Tq % 128) if self.impl == 2 else bool(self.Tq % 32 or self.Tk % 32)

    @property
    def id(self) -> str:
        return f"d{self.d}-h{self.heads}-q{self.Tq}-k{self.Tk}-n{self.N}-impl{self.impl}"


def _cases() -> List[Case]:
    out = []
    both = (1, 3)
    # HuBERT, Whisper: every parity of the two-tile prefetch loop, the ragged last tile in its first and in its second slot, one to
    # five blocks of four query tiles, the last block partly empty
    for T in (1, 3, 31, 32, 33, 63, 64, 65, 95, 96, 97, 127, 128, 129, 160, 500):
        out += [Case(2, 64, T, T, n, 1) for n in both]
    for Tq, Tk in ((1, 129), (129, 1), (40, 50)):
        out += [Case(2, 64, Tq, Tk, n, 1) for n in both]
    # MuseTalk: head dims 40 and 80
    for d in (40, 80):
        for T in (16, 64):
            out += [Case(8, d, T, T, n, 1) for n in both]
        out += [Case(8, d, 64, 50, 1, 1), Case(8, d, 1024, 50, 1, 1)]
        # the LDS ring: two tiles (no third stage), three (exactly full), four and five (wrap), the model's own 1024; 192 and 320
        # leave the last block with two of its four waves past Tq; (50, 128): fewer queries than one tile
        for T in (128, 192, 256, 320, 1024):
            out += [Case(8, d, T, T, n, 2) for n in both]
        out += [Case(8, d, 50, 128, n, 2) for n in both]
    for T in (16, 33, 64):
        out += [Case(2, 160, T, T, n, 1) for n in both]
    out += [Case(2, 160, 16, 50, n, 1) for n in both]
    for T in (1, 32, 33, 100):
        out += [Case(1, 512, T, T, n, 1) for n in both]
    out.append(Case(1, 512, 1024, 1024, 1, 1))
    return out


CASES = _cases()


def _family_plan() -> List[Tuple[Case, str]]:
    """Every case with "gauss" and with the other families in rotation, per (kernel instantiation, ragged or whole): a group of n
    cases hands out families i, i + n, .. to its i-th case, so that each family meets each instantiation at a ragged and at a whole
    shape also where a group has fewer than five cases.  The per-wave kernels' whole shapes include those of the LDS cases, which
    run impl 1 on the same inputs for the byte comparison."""
    groups: Dict[Tuple[str, bool], List[Case]] = {}
    for c in CASES:
        groups.setdefault((c.kernel, c.ragged), []).append(c)
    plan = []
    rot = FAMILIES[1:]
    for c in CASES:
        g = groups[(c.kernel, c.ragged)]
        i, n = g.index(c), len(g)
        fams = ["gauss"] + [rot[j % 5] for j in range(i, max(5, i + 1), n)]
        plan += [(c, f) for f in fams]
    return plan


PLAN = _family_plan()


# ---------------------------------------------------------------------------------------------------- inputs
def make_inputs(c: Case, family: str):
    """-> q [N, h, Tq, d16], k, v [N, h, Tk, d16] float32 holding fp16 values, channels >= d zero."""
    g = torch.Generator().manual_seed(1000 * CASES.index(c) + FAMILIES.index(family))
    N, h, d, Tq, Tk = c.N, c.heads, c.d, c.Tq, c.Tk
    rn = lambda *s: torch.randn(*s, generator=g)
    q, k, v = rn(N, h, Tq, d) * d ** -0.25, rn(N, h, Tk, d) * d ** -0.25, rn(N, h, Tk, d)
    u = torch.zeros(d)
    u[0] = 1.0
    if family == "sharp":                       # a few keys take all the weight: |S| up to 90
        smax = float((q.double() @ k.double().transpose(-1, -2)).abs().max())
        q = q * (90.0 / smax)
    elif family == "offset":                    # a common direction lifts every logit by +48: lost without the max subtraction
        q, k = q + u * math.sqrt(48.0), k + u * math.sqrt(48.0)
    elif family in ("ascending", "descending"):
        # S = 40 ramp(key) + noise of about 1: the running maximum moves at every tile / never after the first
        ramp = torch.linspace(0.0, 1.0, Tk).view(1, 1, Tk, 1)
        if family == "descending":
            ramp = ramp.flip(-2)
        q[..., 0] = math.sqrt(40.0)
        k[..., 0] = 0.0
        k = k + ramp * math.sqrt(40.0) * u
    elif family == "dominant":
        # The last key leads every other by 20.25 - a probability of 1.6e-9 +- a factor e (the noise q . k has a standard deviation of
        # 0.2), below half of fp16's smallest subnormal, so it rounds to zero - and, from 64 keys on, every other key of the tail by
        # 13 (2e-6: 38 subnormal steps, rounded to a whole one).  The last key's value row is 1e-3, the tail's 1e3: what the model
        # loses is then up to 2^-25 |V| per key, against a result of 1e-3.  With fewer than 64 keys all of the tail rounds to zero, and
        # the model's error is at most 0.2 of the subnormal term by construction; from 64 keys on the errors of the rounded half add
        # up like a random walk, 2.9 sqrt(Tk / 2) / Tk <= 0.26 of it at four standard deviations.
        q = q * 0.2
        q[..., 0] = 4.5
        k[..., 0] = 0.0
        if Tk >= 64:
            k[..., 0:Tk - 1:2, 0] = 4.5 - 13.0 / 4.5
        k[..., Tk - 1, :] = 4.5 * u
        v = v * 1.0e3
        v[..., Tk - 1, :] = v[..., Tk - 1, :] * 1.0e-6
    pad = lambda t: torch.nn.functional.pad(R.f16(t), (0, c.d16 - d))
    q, k, v = pad(q), pad(k), pad(v)
    assert float((q.double() @ k.double().transpose(-1, -2)).abs().max()) <= S_CAP
    return q, k, v


# ---------------------------------------------------------------------------------------------------- buffers
class Buffers:
    """The case's device buffers as host int16 arrays (fp16 bits): `qkv` the one input allocation, `o` the pre-filled output; for each
    of q, k, v, o its (offset in halfs into its allocation, cbt, cb0)."""

    def __init__(self, c: Case, q, k, v):
        self.c = c
        N, hcb, Tq, Tk = c.N, c.hcb, c.Tq, c.Tk
        rng = np.random.default_rng(7)
        kmag = float(k.abs().max())

        def region(T, parts):
            cbt = 1 + sum(hcb + 1 for _ in parts)
            guard = (rng.choice([-1.0, 1.0], (N, cbt, T, 16)) * rng.uniform(0.5, 1.0, (N, cbt, T, 16)) * GUARD_GAIN * kmag).astype(np.float16)
            cb0 = []
            for i, t in enumerate(parts):
                b = 1 + i * (hcb + 1)
                guard[:, b:b + hcb] = self._to_cb(t)
                cb0.append(b)
            return guard, cbt, cb0

        if Tq == Tk:
            buf, cbt, (qb, kb, vb) = region(Tq, [q, k, v])
            self.qkv = buf.reshape(-1).view(np.int16)
            self.q, self.k, self.v = (0, cbt, qb), (0, cbt, kb), (0, cbt, vb)
        else:
            bq, qcbt, (qb,) = region(Tq, [q])
            bkv, kcbt, (kb, vb) = region(Tk, [k, v])
            self.qkv = np.concatenate([bq.reshape(-1), bkv.reshape(-1)]).view(np.int16)
            self.q, self.k, self.v = (0, qcbt, qb), (bq.size, kcbt, kb), (bq.size, kcbt, vb)
        self.o_cbt = O_CB0 + hcb + O_TAIL
        self.o = (0, self.o_cbt, O_CB0)

    def _to_cb(self, t):
        """[N, h, T, d16] -> [N, h * d16 / 16, T, 16] fp16"""
        N, h, T, D = t.shape
        return t.reshape(N, h, T, D // 16, 16).permute(0, 1, 3, 2, 4).reshape(N, h * D // 16, T, 16).numpy().astype(np.float16)

    def empty_o(self) -> np.ndarray:
        return np.full(self.c.N * self.o_cbt * self.c.Tq * 16, PATTERN, np.int16)

    def k_rows(self) -> np.ndarray:
        """K as the kernels address it: float32 [N, h, d16 / 16, rows, 16] with `rows` = the 32-row tiles covering Tk, row r of channel
        block b at (b * Tk + r) of the image's buffer - past Tk that is the next block's first rows (clamped to the buffer here)."""
        c = self.c
        off, cbt, cb0 = self.k
        img = self.qkv.view(np.float16)[off:off + c.N * cbt * c.Tk * 16].reshape(c.N, cbt * c.Tk, 16).astype(np.float32)
        rows = (c.Tk + 31) // 32 * 32
        blocks = cb0 + np.arange(c.hcb).reshape(c.heads, c.d16 // 16, 1)
        idx = np.minimum(blocks * c.Tk + np.arange(rows).reshape(1, 1, rows), cbt * c.Tk - 1)
        return img[:, idx]

    def unpack_o(self, o: np.ndarray) -> torch.Tensor:
        """The heads' blocks of an output buffer -> float32 [N, h, Tq, d16]."""
        c = self.c
        t = torch.from_numpy(o.view(np.float16).reshape(c.N, self.o_cbt, c.Tq, 16)[:, O_CB0:O_CB0 + c.hcb].astype(np.float32))
        return t.reshape(c.N, c.heads, c.d16 // 16, c.Tq, 16).permute(0, 1, 3, 2, 4).reshape(c.N, c.heads, c.Tq, c.d16)


# ---------------------------------------------------------------------------------------------------- reference and gates
class Reference:
    """float64 reference, rounding model and bound of one (case, family): computed once, read by every comparison."""

    def __init__(self, c: Case, family: str):
        self.c, self.family = c, family
        self.q, self.k, self.v = make_inputs(c, family)
        self.buf = Buffers(c, self.q, self.k, self.v)
        parts = [R.attention_model(self.q[n:n + 1], self.k[n:n + 1], self.v[n:n + 1], subnormal_p=True) for n in range(c.N)]
        self.ref, self.mod, self.tol = (torch.cat([p[i] for p in parts]) for i in range(3))
        self.tol = self.tol + R.F16_FLOOR

    def model_without_subnormal_term(self) -> float:
        """max |mod - ref| / tol under the replay's bound as it was: 2^-10 |ref| + 2^-10 softmax(S) |V| + 2^-24."""
        _, mod, tol = R.attention_model(self.q, self.k, self.v)
        return float(((mod.double() - self.ref).abs() / (tol.double() + R.F16_FLOOR)).max())


def check(rf: Reference, o: np.ndarray, label: str = "") -> Tuple[dict, List[str]]:
    """The replay's two gates on the heads' blocks of output buffer `o`, and the layout checks: nothing outside those blocks
    written, the padded channels of a d < d16 head zero.  -> (the replay's record, one line per failure)."""
    c = rf.c
    dev = rf.buf.unpack_o(o)
    rp = R.Replay({}, None)
    rp.record(f"{c.id} {rf.family}{label}", dev, rf.ref, rf.mod, rf.tol)
    bad = R.failures(rp.records)
    ob = o.reshape(c.N, rf.buf.o_cbt, c.Tq, 16)
    outside = int((ob[:, :O_CB0] != np.int16(PATTERN)).sum() + (ob[:, O_CB0 + c.hcb:] != np.int16(PATTERN)).sum())
    if outside:
        bad.append(f"{c.id}: {outside} halfs outside channel blocks [{O_CB0}, {O_CB0 + c.hcb}) of the output buffer were written")
    if c.d < c.d16 and bool((dev[..., c.d:] != 0).any()):
        bad.append(f"{c.id}: the zero-padded channels {c.d}..{c.d16 - 1} of a head are not zero")
    return rp.records[0], bad


def format_record(c: Case, family: str, r: dict, extra: str = "") -> str:
    return (f"{c.id:28s} {family:10s} {c.kernel:24s} max|dev-ref|/tol {r['dev_over_tol']:5.2f} (model {r['mod_over_tol']:4.2f})  "
            f"rel_l2 dev {r['rel_dev']:.3e} mod {r['rel_mod']:.3e}{extra}")


# ---------------------------------------------------------------------------------------------------- simulated device
FAULTS = {
    "a": "key Tk admitted as a copy of key Tk-1 (the clamped load, the mask off by one)",
    "b": "the last key dropped",
    "c": "padded keys read from the next channel block's first rows instead of being masked",
    "d": "accumulator not rescaled when the maximum moves",
    "e": "l not rescaled when the maximum moves",
    "f": "two heads' outputs swapped",
    "g": "the two 8-channel halves of a channel block swapped (the permlane transpose)",
    "h": "query rows >= Tq of the last tile written",
    "i": "a V^T row-group in natural instead of MFMA slot order",
}
LOG2E = 1.4426950408889634


def sim_device(rf: Reference, fault: Optional[str] = None) -> np.ndarray:
    """The op as attn_kernel computes it, buffer to buffer: 32-key tiles, fp32 logits, a running maximum with the accumulator and l
    rescaled by exp(m - m_new), exp2((S - m_new) log2 e) rounded to fp16 in front of P V, l summed in fp32, keys >= Tk of the last
    tile masked to -1e30 (their K rows are the clamped load's copy of row Tk-1, their V^T columns zero), the result acc / l rounded to
    fp16 once and written to the heads' blocks of the pre-filled output buffer.  `fault`: one of FAULTS."""
    c = rf.c
    N, h, Tq, Tk, D = c.N, c.heads, c.Tq, c.Tk, c.d16
    rows = (Tk + 31) // 32 * 32
    q = rf.q
    K = torch.cat([rf.k, rf.k[:, :, -1:].expand(N, h, rows - Tk, D)], 2)
    V = torch.cat([rf.v, torch.zeros(N, h, rows - Tk, D)], 2)
    valid = torch.arange(rows) < Tk
    if fault == "a" and Tk < rows:
        valid[Tk] = True
    if fault == "b":
        valid[Tk - 1] = False
    if fault == "c":
        valid[:] = True
        kr = torch.from_numpy(rf.buf.k_rows())                          # [N, h, d16 / 16, rows, 16]
        K = kr.permute(0, 1, 3, 2, 4).reshape(N, h, rows, D)
    if fault == "i":                                                    # the P fragment is in slot order, this V^T group is not
        V = V.clone()
        V[:, :, :16] = V[:, :, list(SLOT)]
    m = torch.full((N, h, Tq, 1), -1e30)
    l = torch.zeros(N, h, Tq, 1)
    acc = torch.zeros(N, h, Tq, D)
    for k0 in range(0, rows, 32):
        S = q @ K[:, :, k0:k0 + 32].transpose(-1, -2)
        S = torch.where(valid[k0:k0 + 32], S, torch.full_like(S, -1e30))
        m_new = torch.maximum(m, S.amax(-1, keepdim=True))
        p = torch.exp2(S * LOG2E - m_new * LOG2E)
        alpha = torch.exp(m - m_new)
        l = (l if fault == "e" else l * alpha) + p.sum(-1, keepdim=True)
        acc = (acc if fault == "d" else acc * alpha) + R.f16(p) @ V[:, :, k0:k0 + 32]
        m = m_new
    out = (acc * (1.0 / l)).half()
    if fault == "f":
        out = out[:, [1, 0] + list(range(2, h))] if h > 1 else out
    if fault == "g":
        out = out.reshape(N, h, Tq, D // 16, 2, 8).flip(-2).reshape(N, h, Tq, D)
    ob = rf.buf.empty_o().view(np.float16).reshape(N, rf.buf.o_cbt * Tq, 16)
    blocks = rf.buf._to_cb(out.float())                                 # [N, hcb, Tq, 16]
    for b in range(c.hcb):
        r0 = (O_CB0 + b) * Tq
        ob[:, r0:r0 + Tq] = blocks[:, b]
    if fault == "h":                                                    # the clamped query's result, at the rows the tile runs past Tq
        over = (Tq + 31) // 32 * 32 - Tq
        for b in range(c.hcb):
            r0 = (O_CB0 + b) * Tq + Tq
            n_over = min(over, ob.shape[1] - r0)
            ob[:, r0:r0 + n_over] = blocks[:, b, Tq - 1:Tq]
    return ob.reshape(-1).view(np.int16)
