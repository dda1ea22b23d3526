"""Teacher-forced, op-by-op replay of the MuseTalk program (U-Net + VAE decoder) of the Wav2Lip program, of the Whisper encoder and of the
Ultralight program (its restatement and replay_ultralight live in tests/ultralight_ref.py) against float64.

TEST INFRASTRUCTURE ONLY (see oracle/__init__.py); CPU code.

The device program runs once and every named tensor is read back.  The oracle (oracle/musetalk_oracle.py) then runs in float64 with
a `force` hook: at every op, under the device's op name, the forward continues with the DEVICE's tensor.  What the oracle computed at
that point, `ref`, is therefore the exact result of ONE op (or one fused group) on the device's own inputs, and `dev - ref` is that
op's error and nothing upstream.  Beside `ref` the replay evaluates, in float32 on the same inputs,

  mod : a rounding model of the op - weights rounded as the loader packs them (fp16; fp16(W * d^-0.5) for to_q; fp16(W * gamma) for
        the consumer of a folded LayerNorm; e4m3 per output channel and e4m3 activations at `ascale` for the fp8 convs), attention
        probabilities rounded to fp16 before P V, fp32 sums, the result rounded to fp16 once;
  tol : the per-element bound  2^-10 |ref| + c A + s  with
        conv / linear     A = |W| (*) |x| + 4 (|b| + |res|),  c = 2^-12,  s = 2^-24 sum |x| over the receptive field
                          (each weight within 2^-11 relative of its value, fp16-subnormal weights within 2^-25 absolute; the factor 4
                          leaves room for a residual folded into a weight).  c = 2^-12 is half the worst case 2^-11 |W| |x|: it counts
                          on the rounding errors of a long sum not all pointing the same way.  A sum of n < 576 products gets
                          min(4, 24 / sqrt n) |W| (*) |x| (short_sum(): conv_in, post_quant_conv, decoder.conv_in with 72, 4 and 36
                          products, the 320- and 384-channel linear layers, Wav2Lip's shallow layers);
        folded LayerNorm  A = rstd (|W'| |x_raw| + |mean| |sum W'|) + |shift|  on the RAW input: that is what the MFMAs sum before
                          the mean term is taken off (ln_fold in csrc/musetalk.hip);
        attention         A = softmax(S) |V|,  c = 2^-10;
        Group/LayerNorm   A = |gamma| |x_hat| + |beta|,  c = 2^-10  (the SiLU behind a GroupNorm has slope <= 1.1),
                          s = 2^-24 ceil(log2 n) |gamma| rstd |mean|: x - mean is taken in fp32 from a mean that is a tree sum of n
                          fp32 terms (n = C, or the group's channels x pixels), one rounding of 2^-24 |mean| per level; it
                          matters where x_hat is near 0 and |mean| / std is large, and nothing relative to |x_hat| covers it;
                          no term for the variance: a device that sums x - k (k an element of the set) loses ((mean - k) / std)^2 2^-24 per
                          rounding, inside the terms above also at |mean| = 256 std (tests/test_norm_host.py); un-shifted sums lose
                          (mean / std)^2 2^-24 and are a fault the bound is there to catch (tests/norm_cases.py, `unshifted`);
        GEGLU             A = |ref|,  c = 2^-10,  s = 2^-23 |a| |g|: Phi(g) = (1 + erf(g / sqrt 2)) / 2 evaluated in fp32 carries an absolute
                          error of 2^-25 and more however small Phi is (the sum cancels in the negative tail), so a gelu(g) has
                          |a| |g| 2^-25 that no bound relative to |ref| covers;  in the projection's epilogue (the projection is never rounded): first-order
                          propagation of the projection's own bound, A = A_a |gelu(g)| + |a| |gelu'(g)| A_g with c = 2^-12, plus 2^-10 |ref|.
        Ultralight (csrc/ultralight.hip, csrc/dw_kernels.hip; the ops of tests/ultralight_ref.py):
        dense conv        the Wav2Lip layer's form (fp16 weights, BatchNorm + conv bias as an fp32 scale / shift in the epilogue) with the
                          residual added BEHIND the affine, never folded into a tap, and a ReLU only where the op has one:
                          A = short_sum(n) |W| (*) |x| |scale| + 4 |shift| + 4 |res|,  c = 2^-12,  s = 2^-24 sum |x| |scale|;
        depthwise 3x3     weights, scale and shift stay fp32: no weight rounding in the model; 9 fp32 FMAs, the affine, one rounding:
                          A = |w| (*) |x| |scale| + |shift|,  c = 2^-20,  s = 2^-24;  the same form for inc.inconv.0.conv.0 (ul_in_kernel:
                          6 fp32 products on the float32 input);
        upsample          evaluated in float64 on the device, one rounding: 2^-10 |ref| + 2^-24;
        audio_feat        one fp32 -> fp16 rounding; beyond the bound the device's tensor has to EQUAL f16(input) (record "inexact");
        outc.conv         fp32 throughout: the Wav2Lip head's bound.
        The leading 2^-10 |ref| is the output's own rounding to fp16 (2^-11) with a factor 2 of room; every bound also gets 2^-24
        absolute, the same for an output in fp16's subnormal range (spacing 2^-24).

Gates (failures()):
  per element : |dev - ref| <= tol, no violator allowed (not for the fp8 convs: e4m3 operands make c = 2^-3, which says nothing);
  exact       : an op whose model is exact (audio_feat) has to equal it;
  aggregate   : rel_l2(dev, ref) <= 2 * rel_l2(mod, ref) + 1e-4.
  The model itself has to sit inside the bound: max |mod - ref| / tol <= 0.5 (tests/test_op_replay.py).

Coverage (uncovered()): every op of Engine.musetalk_ops() is compared on its own, through its named views (the stacked q|k|v and
k|v projections), or through the output of the group FUSED_INTO names.
"""
from __future__ import annotations

import math
from typing import Callable, Dict, List, Optional

import torch
import torch.nn.functional as F

from . import musetalk_oracle as M

Tensor = torch.Tensor

C_LIN = 2.0 ** -12
C_ACT = 2.0 ** -10
AGG_FACTOR = 2.0
AGG_FLOOR = 1e-4
MODEL_HEADROOM = 0.5
GELU_SLOPE = 1.13           # max |gelu'(x)| = 1.129 (at x = sqrt 2)
C_F32 = 2.0 ** -20          # a short fp32 sum (<= 9 FMAs and an affine): 16 roundings of 2^-24
EXACT_KINDS = ("ul_feat",)  # ops whose rounding model the device has to equal
F16_FLOOR = 2.0 ** -24      # fp16 output below 2^-14 is subnormal: its rounding error is up to 2^-25 absolute, whatever |ref| is


def short_sum(n: int) -> float:
    """The factor on |W| (*) |x| for a sum of n products.  c = 2^-12 is half the worst case 2^-11 |W| |x|: it counts on n independent
    weight roundings not all pointing one way.  Their sum has a standard deviation of about 2^-12 A / sqrt(n); over the millions of
    elements of a tensor it reaches six of those, and that is to stay within a quarter of the bound (the other quarter of the 0.5
    the model is held to belongs to the output rounding): 24 / sqrt(n), no less than 1 (n >= 576) and no more than 4 (the worst case
    with a factor 2 of room, as for the output rounding)."""
    return max(1.0, min(4.0, 24.0 / math.sqrt(n)))


def f16(t: Tensor) -> Tensor:
    return t.half().to(t.dtype)


def rel_l2(a: Tensor, b: Tensor) -> float:
    return float((a.double() - b.double()).norm() / max(float(b.double().norm()), 1e-30))


def _blocks():
    out = []
    for i in range(3):
        for j in range(2):
            out.append(f"down_blocks.{i}.attentions.{j}")
    out.append("mid_block.attentions.0")
    for i in range(1, 4):
        for j in range(3):
            out.append(f"up_blocks.{i}.attentions.{j}")
    return out


def fused_into(fp8: bool = False) -> Dict[str, str]:
    """op -> the group output it is compared through, for the intermediates a program may not materialise: the LayerNorms folded
    into their consumers, the GEGLU projection that lives in its epilogue's accumulators, the value transpose (consumed by every
    cross-attention kernel) and, in the fp8 program, the e4m3 GroupNorm outputs of the resnets."""
    m = {}
    for p in _blocks():
        b = p + ".transformer_blocks.0"
        m[b + ".norm1"] = b + ".attn1.to_q"
        m[b + ".norm2"] = b + ".attn2.to_q"
        m[b + ".norm3"] = b + ".ff.geglu"
        m[b + ".ff.net.0.proj"] = b + ".ff.geglu"
    m["attn2.v_transpose_all"] = "mid_block.attentions.0.transformer_blocks.0.attn2.attn"
    if fp8:
        res = [f"down_blocks.{i}.resnets.{j}" for i in range(4) for j in range(2)] + ["mid_block.resnets.0", "mid_block.resnets.1"]
        res += [f"up_blocks.{i}.resnets.{j}" for i in range(4) for j in range(3)]
        res += ["decoder.mid_block.resnets.0", "decoder.mid_block.resnets.1"] + [f"decoder.up_blocks.{i}.resnets.{j}" for i in range(4) for j in range(3)]
        for r in res:
            m[r + ".norm1"] = r + ".conv1"
            m[r + ".norm2"] = r + ".conv2"
    return m


# consumer -> the op in front of it that a program may have fused into it
PRODUCER = {}
for _p in _blocks():
    _b = _p + ".transformer_blocks.0"
    for _n in ("to_q", "to_k", "to_v"):
        PRODUCER[_b + ".attn1." + _n] = _b + ".norm1"
    PRODUCER[_b + ".attn2.to_q"] = _b + ".norm2"
    PRODUCER[_b + ".ff.net.0.proj"] = _b + ".norm3"
    PRODUCER[_b + ".ff.geglu"] = _b + ".ff.net.0.proj"


def uncovered(ops, compared, fused: Dict[str, str]) -> List[str]:
    """The ops of Engine.musetalk_ops() ([(name, type)]) whose output was neither compared nor reached through FUSED_INTO."""
    compared = set(compared)
    miss = []
    for name, typ in ops:
        if typ == 3:                                    # attention: its output is named "<op>.attn"
            ok = name + ".attn" in compared
        elif name.endswith(".to_qkv"):                  # stacked projections: compared through their three views
            ok = all(name[:-len("to_qkv")] + n in compared for n in ("to_q", "to_k", "to_v"))
        elif name.endswith(".to_kv"):
            ok = all(name[:-len("to_kv")] + n in compared for n in ("to_k", "to_v"))
        elif name == "attn2.to_kv_all":
            ok = all(p + ".transformer_blocks.0.attn2." + n in compared for p in _blocks() for n in ("to_k", "to_v"))
        else:
            ok = name in compared or (name in fused and fused[name] in compared)
        if not ok:
            miss.append(name)
    return miss


# ---------------------------------------------------------------------------------------------------- per-op models
def _tok_to_nchw(t: Tensor, hw) -> Tensor:
    B, T, c = t.shape
    H, W = hw if hw is not None else (T, 1)
    return t.reshape(B, H, W, c).permute(0, 3, 1, 2)


def _gelu_grad(g: Tensor) -> Tensor:
    return 0.5 * (1 + torch.erf(g / math.sqrt(2.0))) + g * torch.exp(-0.5 * g * g) / math.sqrt(2.0 * math.pi)


def attention_model(q: Tensor, k: Tensor, v: Tensor, subnormal_p: bool = False, scale: float = 1.0, want_ref: bool = True):
    """softmax(scale q k^T) v per (image, head): q [B, h, Tq, d], k / v [B, h, Tk, d] (fp16 values in any float dtype; Tq != Tk is
    fine).  q is taken as it stands - the programs fold d^-0.5 into the q projection - and `scale` multiplies the logits for a caller
    whose q is not scaled (the replay).  -> (ref, mod, tol):
      ref : float64 (None with want_ref=False: the replay has the oracle's own);
      mod : the rounding model, float32 - fp32 logits and exp, probabilities rounded to fp16 in front of P V, their sum l kept in
            fp32, the result rounded to fp16 once;
      tol : 2^-10 |ref| + 2^-10 softmax(S) |V| (with want_ref=False only the second term: the caller adds 2^-10 |ref|), without
            F16_FLOOR, which the gates add to every bound.
    subnormal_p adds 2^-25 sum_k |V_k| / l.  The kernels round exp(S - max) to fp16 before the P V MFMA; below 2^-14 that is fp16's
    subnormal range, where a probability is off by up to 2^-25 ABSOLUTE whatever its size, and a key with p ~ 1e-6 and |V| ~ 1e3
    behind a dominant key with a small value row puts the model itself two orders of magnitude outside the relative terms
    (tests/test_attention_host.py).  Off by default: the replays' constants stay as they are."""
    qf, kf, vf = q.float(), k.float(), v.float()
    S = (qf @ kf.transpose(-1, -2)) * scale
    pr = torch.exp(S - S.amax(-1, keepdim=True))
    l = pr.sum(-1, keepdim=True)
    mod = f16((f16(pr) @ vf) / l)                       # probabilities go to the MFMA as fp16, their sum stays fp32
    tol = C_ACT * (pr @ vf.abs()) / l
    if subnormal_p:
        tol = tol + 2.0 ** -25 * vf.abs().sum(-2, keepdim=True) / l
    ref = None
    if want_ref:
        ref = torch.softmax((q.double() @ k.double().transpose(-1, -2)) * scale, -1) @ v.double()
        tol = tol + 2.0 ** -10 * ref.abs().float()
    return ref, mod, tol


class Replay:
    """The `force` object of one replay.  sd: float32 state dict (U-Net and VAE keys together); fetch(name, ref) -> the device's
    tensor in ref's shape and dtype, or None when the program does not materialise it."""

    def __init__(self, sd: Dict[str, Tensor], fetch: Callable[[str, Tensor], Optional[Tensor]], fp8: bool = False, ascale: float = 8.0,
                 only: Optional[Callable[[str], bool]] = None):
        self.sd = sd
        self.fetch = fetch
        self.fp8 = fp8
        self.ascale = ascale
        self.may_fuse = fused_into(fp8)
        self.fold_residual = True                  # Wav2Lip: the engine folds the residual into the centre tap
        self.only = only
        self.ops: Dict[str, dict] = {}
        self.fused: Dict[str, dict] = {}           # ops the device did not materialise: name -> description
        self.records: List[dict] = []

    # -- the hook protocol of musetalk_oracle._tap
    def describe(self, name: str, op: dict):
        self.ops[name] = op

    def __call__(self, name: str, ref: Tensor) -> Optional[Tensor]:
        op = self.ops.pop(name, None)
        dev = self.fetch(name, ref)
        if dev is None:
            if op is None or name not in self.may_fuse:
                raise KeyError(f"the program has no tensor named {name} and FUSED_INTO does not list it")
            self.fused[name] = op
            return None
        if op is not None and (self.only is None or self.only(name)):
            with torch.no_grad():
                mod, tol, elementwise = self.model(name, op, ref)
                tol = tol + F16_FLOOR
            self.record(name, dev, ref, mod, tol, elementwise)
            if op["kind"] in EXACT_KINDS:
                self.records[-1]["inexact"] = int((dev.double() != mod.double()).sum())
        return dev

    # -- bookkeeping
    def record(self, name, dev, ref, mod, tol, elementwise=True):
        ref = ref.double()
        mod = mod.double()
        tol = tol.double()
        e_dev = (dev.double() - ref).abs()
        e_mod = (mod - ref).abs()
        tiny = 1e-300
        r_dev, r_mod = rel_l2(dev, ref), rel_l2(mod, ref)
        q = e_dev / (tol + tiny)
        worst = int(q.argmax())
        rms = float(ref.pow(2).mean().sqrt())
        self.records.append(dict(
            name=name, elementwise=elementwise, rel_dev=r_dev, rel_mod=r_mod, ratio=r_dev / max(r_mod, 1e-30),
            dev_over_tol=float(q.max()), violators=int((e_dev > tol).sum()), worst_index=worst,
            mod_over_tol=float((e_mod / (tol + tiny)).max()), mod_violators=int((e_mod > tol).sum()),
            tol_over_rms=float(tol.median()) / max(rms, 1e-30), n=ref.numel()))

    # -- models
    def _w(self, p):
        return self.sd[p + ".weight"].float(), (self.sd[p + ".bias"].float() if (p + ".bias") in self.sd else None)

    def _linear_parts(self, name, op, round_w=True):
        """-> (acc, A, s) of a linear layer on token-major x, before the output rounding; acc already carries bias and residual and
        is in the oracle's scale (a folded d^-0.5 is taken out again, as the fetch does for the device's tensor)."""
        W, b = self._w(op["p"])
        sc = float(op.get("scale") or 1.0)
        prod = self.fused.get(PRODUCER.get(name, ""))
        if b is None:
            b = torch.zeros(W.shape[0])
        if prod is not None and prod["kind"] == "ln":
            # the LayerNorm in front was folded in: W' = W gamma (x d^-0.5), scale = sum fp16(W'), shift = W beta + b
            x = prod["x"].float()
            gamma, beta = self._w(prod["p"])
            Wf = W * gamma[None, :] * sc
            W16 = f16(Wf)
            scale = W16.double().sum(1).float()
            shift = ((W.double() @ beta.double()).float() + b) * sc
            mean = x.mean(-1, keepdim=True)
            rstd = torch.rsqrt(x.var(-1, unbiased=False, keepdim=True) + M.LN_EPS)
            acc = rstd * (F.linear(x, W16) - mean * scale) + shift
            A = rstd * (short_sum(x.shape[-1]) * F.linear(x.abs(), Wf.abs()) + mean.abs() * scale.abs()) + shift.abs()
            s = 2.0 ** -24 * rstd * x.abs().sum(-1, keepdim=True)
        else:
            x = op["x"].float()
            Ws = W * sc
            acc = F.linear(x, f16(Ws) if round_w else Ws) + b * sc
            A = short_sum(x.shape[-1]) * F.linear(x.abs(), Ws.abs()) + 4 * (b * sc).abs()
            s = 2.0 ** -24 * x.abs().sum(-1, keepdim=True)
        if op.get("res") is not None:
            r = op["res"].float()
            acc = acc + r * sc
            A = A + 4 * r.abs() * sc
        return acc, A, s, sc

    def model(self, name: str, op: dict, ref: Tensor):
        kind = op["kind"]
        elementwise = True
        if kind == "conv":
            p = op["p"]
            W, b = self._w(p)
            x = op["x"].float()
            if p == "post_quant_conv":              # 1 / scaling_factor is folded into the weights; the device's input is the raw latent
                W = W / M.VAE_SCALING
                x = x * M.VAE_SCALING
            b2 = op.get("bias2")
            if b2 is not None:                      # the timestep term, folded into the bias at load time
                b = b + b2[0].float()
            st, pad = op["stride"], op["pad"]
            if self.fp8 and op.get("q8") and x.shape[1] % 32 == 0:
                a = self.ascale
                wq, _ = M.fp8_weight(W)
                acc = F.conv2d(M.fp8_round(x * a) / a, wq, b, stride=st, padding=pad)
                elementwise = False
            else:
                acc = F.conv2d(x, f16(W), b, stride=st, padding=pad)
            k = W.shape[-1]
            short = short_sum(W.shape[1] * k * k)
            A = short * F.conv2d(x.abs(), W.abs(), None, stride=st, padding=pad) + 4 * b.abs()[None, :, None, None]
            s = 2.0 ** -24 * F.conv2d(x.abs().sum(1, keepdim=True), torch.ones(1, 1, k, k), None, stride=st, padding=pad)
            if op.get("res") is not None:
                r = op["res"].float()
                acc = acc + r
                A = A + 4 * r.abs()
            mod = f16(acc)
            tol = 2.0 ** -10 * ref.abs() + C_LIN * A + s
        elif kind == "linear":
            acc, A, s, sc = self._linear_parts(name, op)
            lin_tol = (C_LIN * A + s) / sc
            if op.get("act") == "gelu":             # GELU in the epilogue: slope <= 1.13, and the fp32 (1 + erf) term of the GEGLU
                lin_tol = GELU_SLOPE * lin_tol + 2.0 ** -23 * acc.abs()
                acc = F.gelu(acc)
            mod = _tok_to_nchw(f16(acc) / sc, op.get("hw"))
            tol = 2.0 ** -10 * ref.abs() + _tok_to_nchw(lin_tol, op.get("hw"))
        elif kind in ("conv1d_gelu", "add_pos"):
            # Whisper's Conv1d(k 3, padding 1) + GELU over a (1, C, T) map; "add_pos": the device adds the positions IN PLACE on
            # conv2's fp16 output, so that tensor is compared as the group conv2 -> GELU -> fp16 -> + positions -> fp16
            c = self.fused["conv2"] if kind == "add_pos" else op
            x = c["x"].float()
            W, b = self._w(c["p"])
            st = c["stride"]
            z = F.conv1d(x, f16(W), b, stride=st, padding=1)
            A = short_sum(W.shape[1] * 3) * F.conv1d(x.abs(), W.abs(), None, stride=st, padding=1) + 4 * b.abs()[None, :, None]
            s = 2.0 ** -24 * F.conv1d(x.abs().sum(1, keepdim=True), torch.ones(1, 1, 3), None, stride=st, padding=1)
            g = F.gelu(z)
            t = GELU_SLOPE * (C_LIN * A + s) + 2.0 ** -23 * z.abs()
            if kind == "add_pos":
                mod = f16(f16(g) + op["pos"].float().t()[None])[..., None]
                t = t + 2.0 ** -10 * g.abs() + F16_FLOOR
            else:
                mod = f16(g)[..., None]
            tol = 2.0 ** -10 * ref.abs() + t[..., None]
        elif kind in ("gn", "ln"):
            x = op["x"].float()
            gamma, beta = self._w(op["p"])
            if kind == "gn":
                xh = F.group_norm(x, op["groups"], None, None, op["eps"])
                y = xh * gamma[None, :, None, None] + beta[None, :, None, None]
                A = xh.abs() * gamma.abs()[None, :, None, None] + beta.abs()[None, :, None, None]
                B_, C_ = x.shape[:2]
                xg = x.reshape(B_, op["groups"], -1)
                ms = xg.mean(-1).abs() * torch.rsqrt(xg.var(-1, unbiased=False) + op["eps"])           # |mean| rstd per (image, group)
                ms = ms.repeat_interleave(C_ // op["groups"], dim=1)[:, :, None, None]
                sm = 2.0 ** -24 * math.ceil(math.log2(xg.shape[-1])) * gamma.abs()[None, :, None, None] * ms
                if op["silu"]:
                    y = F.silu(y)
            else:
                xh = F.layer_norm(x, (x.shape[-1],), None, None, M.LN_EPS)
                y = _tok_to_nchw(xh * gamma + beta, op.get("hw"))
                A = _tok_to_nchw(xh.abs() * gamma.abs() + beta.abs(), op.get("hw"))
                ms = x.mean(-1, keepdim=True).abs() * torch.rsqrt(x.var(-1, unbiased=False, keepdim=True) + M.LN_EPS)
                sm = _tok_to_nchw(2.0 ** -24 * math.ceil(math.log2(x.shape[-1])) * gamma.abs() * ms, op.get("hw"))
            mod = f16(y)
            tol = 2.0 ** -10 * ref.abs() + C_ACT * A + sm
        elif kind == "attn":
            q, k, v = op["q"], op["k"], op["v"]
            B, h, T, d = q.shape
            _, o, A = attention_model(q, k, v, scale=d ** -0.5, want_ref=False)
            mod = _tok_to_nchw(o.transpose(1, 2).reshape(B, T, h * d), op.get("hw"))
            tol = 2.0 ** -10 * ref.abs() + _tok_to_nchw(A.transpose(1, 2).reshape(B, T, h * d), op.get("hw"))
        elif kind == "geglu":
            prod = self.fused.get(PRODUCER.get(name, ""))
            if prod is not None:                        # GEGLU in the epilogue of its projection
                acc, A, s, _ = self._linear_parts(PRODUCER[name], prod)
                a, g = acc.chunk(2, dim=-1)
                Aa, Ag = (C_LIN * A + s).chunk(2, dim=-1)
                mod = _tok_to_nchw(f16(a * F.gelu(g)), op.get("hw"))
                tol = 2.0 ** -9 * ref.abs() + _tok_to_nchw(Aa * F.gelu(g).abs() + a.abs() * _gelu_grad(g).abs() * Ag + 2.0 ** -23 * (a * g).abs(), op.get("hw"))
            else:
                a, g = op["x"].float().chunk(2, dim=-1)
                mod = _tok_to_nchw(f16(a * F.gelu(g)), op.get("hw"))
                tol = 2.0 ** -9 * ref.abs() + _tok_to_nchw(2.0 ** -23 * (a * g).abs(), op.get("hw"))
        elif kind == "w2l":
            mod, tol = self._w2l_layer(op, ref)
        elif kind in ("w2l_head", "ul_head"):
            # fp32 weights, fp32 sigmoid, fp32 result: no fp16 rounding anywhere; the bound is the conv's own through the slope of the sigmoid
            mod, tol = self.head(op["x"].float(), op.get("p", "output_block.1"), ref)
        elif kind == "ul_conv":
            mod, tol = self._ul_conv(op, ref)
        elif kind in ("ul_dw", "ul_in"):
            # fp32 weights and fp32 affine (ul_in: on the float32 input): FMAs in fp32, ReLU, one rounding to fp16
            x = op["x"].float()
            W = self.sd[op["p"] + ".weight"].float()
            sc, sf = self._bn_fold(op["bn"], None)
            kw = dict(stride=op["stride"], padding=1, groups=W.shape[0]) if kind == "ul_dw" else {}
            v = lambda t: t[None, :, None, None]
            mod = f16(F.relu(F.conv2d(x, W, None, **kw) * v(sc) + v(sf)))
            tol = 2.0 ** -10 * ref.abs() + C_F32 * (F.conv2d(x.abs(), W.abs(), None, **kw) * v(sc.abs()) + v(sf.abs())) + 2.0 ** -24
        elif kind == "ul_up":
            # the kernel interpolates in float64 from exact integer quotients: the result is float64's, rounded once
            mod = f16(F.interpolate(op["x"].double(), scale_factor=2, mode="bilinear", align_corners=True))
            tol = 2.0 ** -10 * ref.abs() + 2.0 ** -24
        elif kind == "ul_feat":
            mod = f16(op["x"].float())
            tol = 2.0 ** -10 * ref.abs()
        else:
            raise ValueError(kind)
        return mod, tol, elementwise

    def head(self, x, p, ref):
        """-> (mod, tol) of a 1x1 conv + sigmoid that stays fp32 (Wav2Lip's output_block.1, Ultralight's outc.conv); tol without F16_FLOOR."""
        W, b = self.sd[p + ".weight"].float(), self.sd[p + ".bias"].float()
        mod = torch.sigmoid(F.conv2d(x, W, b))
        A = F.conv2d(x.abs(), W.abs()) + 4 * b.abs()[None, :, None, None]
        return mod, 2.0 ** -10 * ref.abs() + C_LIN * A * (mod * (1 - mod))

    def _bn_fold(self, bn, bias):
        """BatchNorm2d (eval, eps 1e-5) and the conv's bias as the fp32 scale / shift csrc/ultralight.hip fold_bn computes."""
        sd = self.sd
        sc = sd[bn + ".weight"].float() / torch.sqrt(sd[bn + ".running_var"].float() + 1e-5)
        b = bias.float() if bias is not None else 0.0
        return sc, (b - sd[bn + ".running_mean"].float()) * sc + sd[bn + ".bias"].float()

    def _ul_conv(self, op, ref):
        """A dense conv of the Ultralight program (1x1 expand / project, the two biased 3x3 audio convs) as conv_plan_create packs it:
        fp16 weights, fp32 scale / shift, the residual added behind them, ReLU where the op has one, one rounding to fp16."""
        p = op["p"]
        x = op["x"].float()
        W = self.sd[p + ".weight"].float()
        sc, sf = self._bn_fold(op["bn"], self.sd.get(p + ".bias"))
        k = W.shape[-1]
        kw = dict(stride=op["stride"], padding=op["pad"])
        v = lambda t: t[None, :, None, None]
        acc = F.conv2d(x, f16(W), None, **kw) * v(sc) + v(sf)
        A = short_sum(W.shape[1] * k * k) * F.conv2d(x.abs(), W.abs(), None, **kw) * v(sc.abs()) + 4 * v(sf.abs())
        s = F.conv2d(x.abs().sum(1, keepdim=True), torch.ones(1, 1, k, k), None, **kw) * v(sc.abs())
        if op.get("res") is not None:
            r = op["res"].float()
            acc = acc + r
            A = A + 4 * r.abs()
        mod = f16(F.relu(acc) if op["relu"] else acc)
        return mod, 2.0 ** -10 * ref.abs() + C_LIN * A + 2.0 ** -24 * s

    def _w2l_layer(self, op, ref):
        """A Wav2Lip Conv2d / ConvTranspose2d block as csrc/w2l_program.hip packs it: fp16 weights, BatchNorm (eval) as an fp32
        scale / shift in the epilogue, the residual of a stride-1 same-size block folded into the centre tap (w += 1 / scale;
        not when a scale is below 1e-3), ReLU, one rounding to fp16."""
        l, sd = op["layer"], self.sd
        x = op["x"].float()
        pre = l.prefix + ".conv_block."
        W, b = sd[pre + "0.weight"].float(), sd[pre + "0.bias"].float()
        sc = sd[pre + "1.weight"].float() / torch.sqrt(sd[pre + "1.running_var"].float() + 1e-5)
        sf = (b - sd[pre + "1.running_mean"].float()) * sc + sd[pre + "1.bias"].float()
        kh, kw = l.k
        fold = (self.fold_residual and l.residual and l.kind == "conv" and l.cin == l.cout and kh == kw and kh % 2 == 1
                and tuple(l.stride) == (1, 1) and tuple(l.pad) == (kh // 2, kh // 2) and bool((sc.abs() >= 1e-3).all()))
        if fold:
            W = W.clone()
            i = torch.arange(l.cout)
            W[i, i, kh // 2, kw // 2] += 1.0 / sc
        ones = torch.ones(1, 1, kh, kw)
        xs = x.abs().sum(1, keepdim=True)
        if l.kind == "conv":
            conv = F.conv2d(x, f16(W), None, stride=l.stride, padding=l.pad)
            A = F.conv2d(x.abs(), W.abs(), None, stride=l.stride, padding=l.pad)
            s = F.conv2d(xs, ones, None, stride=l.stride, padding=l.pad)
        else:
            conv = F.conv_transpose2d(x, f16(W), None, stride=l.stride, padding=l.pad, output_padding=l.out_pad)
            A = F.conv_transpose2d(x.abs(), W.abs(), None, stride=l.stride, padding=l.pad, output_padding=l.out_pad)
            s = F.conv_transpose2d(xs, ones, None, stride=l.stride, padding=l.pad, output_padding=l.out_pad)
        v = lambda t: t[None, :, None, None]
        acc = conv * v(sc) + v(sf)
        # a stride-s transposed conv reaches an output through (k // s)^2 of its k^2 taps at the least
        short = short_sum(l.cin * kh * kw if l.kind == "conv" else l.cin * max(1, kh // l.stride[0]) * max(1, kw // l.stride[1]))
        A = short * A * v(sc.abs()) + 4 * v(sf.abs())
        if l.residual:
            A = A + 4 * x.abs()
            if not fold:
                acc = acc + x
        mod = f16(F.relu(acc))
        tol = 2.0 ** -10 * ref.abs() + C_LIN * A + 2.0 ** -24 * s * v(sc.abs())
        return mod, tol


def failures(records: List[dict], model_too: bool = False) -> List[str]:
    """One line per op that misses a gate (the line starts with the op's name)."""
    out = []
    for r in records:
        why = []
        if r["elementwise"] and r["violators"]:
            why.append(f"{r['violators']} of {r['n']} elements outside the bound, worst |dev - ref| / tol = {r['dev_over_tol']:.2f} at flat index {r['worst_index']}")
        if r.get("inexact"):
            why.append(f"{r['inexact']} of {r['n']} elements differ from the op's exact model")
        if not (r["rel_dev"] <= AGG_FACTOR * r["rel_mod"] + AGG_FLOOR):
            why.append(f"rel_l2(dev, ref) = {r['rel_dev']:.3e} > 2 * rel_l2(mod, ref) + 1e-4 = {AGG_FACTOR * r['rel_mod'] + AGG_FLOOR:.3e}")
        if model_too and r["elementwise"] and (r["mod_violators"] or r["mod_over_tol"] > MODEL_HEADROOM):
            why.append(f"the rounding model itself: max |mod - ref| / tol = {r['mod_over_tol']:.2f}, {r['mod_violators']} violators")
        if why:
            out.append(r["name"] + ": " + "; ".join(why))
    return out


def format_records(config: str, records: List[dict]) -> List[str]:
    return [f"{config:14s} {r['name']:72s} dev {r['rel_dev']:.3e}  mod {r['rel_mod']:.3e}  ratio {r['ratio']:5.2f}  "
            f"max|dev-ref|/tol {r['dev_over_tol']:5.2f}{'' if r['elementwise'] else ' (aggregate only)'}" for r in records]


def format_tables(tables: Dict[str, Dict[str, List[dict]]]) -> List[str]:
    """section -> {configuration: records} as text: an op per line, per configuration "rel_l2(dev, ref) rel_l2(mod, ref) ratio
    max |dev - ref| / tol" ("a" behind it: held by the aggregate gate only; "-": the configuration has no such tensor)."""
    out = []
    for section, cfgs in tables.items():
        names = []
        for recs in cfgs.values():
            names += [r["name"] for r in recs if r["name"] not in names]
        by = {c: {r["name"]: r for r in recs} for c, recs in cfgs.items()}
        w = max(len(n) for n in names)
        out.append(f"== {section}: dev mod ratio max|dev-ref|/tol per configuration")
        out.append(" " * w + "".join(f" | {c:27s}" for c in cfgs))
        for n in names:
            cells = []
            for c in cfgs:
                r = by[c].get(n)
                cells.append(f"{r['rel_dev']:.2e} {r['rel_mod']:.2e} {r['ratio']:.2f} {r['dev_over_tol']:.2f}{' ' if r['elementwise'] else 'a'}" if r else "-")
            out.append(f"{n:{w}s}" + "".join(f" | {c:27s}" for c in cells))
    return out


# ---------------------------------------------------------------------------------------------------- whole-program replay
def replay_musetalk(usd: Dict[str, Tensor], vsd: Dict[str, Tensor], fetch, fp8: bool = False, ascale: float = 8.0, vae: bool = True,
                    only=None) -> Replay:
    """usd / vsd: float32 state dicts.  The inputs are the device's own: "latent_in", "encoder_hidden_states" (the position-encoded
    audio context as the pass wrote it) and, for the decoder, its "conv_out"."""
    sd = dict(usd)
    sd.update(vsd)
    rp = Replay(sd, fetch, fp8, ascale, only)
    lat = fetch("latent_in", torch.zeros(0, 8, 32, 32, dtype=torch.float64))
    ctx = fetch("encoder_hidden_states", torch.zeros(0, 384, 50, 1, dtype=torch.float64))
    ctx = ctx[:, :, :, 0].transpose(1, 2).contiguous()
    usd64 = {k: v.double() for k, v in usd.items()}
    assert not M.FP8["on"], "the reference side of the replay is the unquantised oracle"
    with torch.no_grad():
        out = M.unet_forward(usd64, lat, ctx, force=rp)
        del usd64
        if vae:
            M.vae_decode({k: v.double() for k, v in vsd.items()}, out / M.VAE_SCALING, force=rp)
    return rp


def replay_transformer(sd: Dict[str, Tensor], p: str, fetch, x_name: str, hw=(32, 32)) -> Replay:
    """The replay of ONE Transformer2D block `p` of the U-Net: its input is the device's tensor `x_name`."""
    rp = Replay(sd, fetch)
    C = sd[p + ".norm.weight"].shape[0]
    x = fetch(x_name, torch.zeros(0, C, hw[0], hw[1], dtype=torch.float64))
    ctx = fetch("encoder_hidden_states", torch.zeros(0, 384, 50, 1, dtype=torch.float64))
    ctx = ctx[:, :, :, 0].transpose(1, 2).contiguous()
    with torch.no_grad():
        M.transformer2d({k: v.double() for k, v in sd.items() if k.startswith(p + ".")}, p, x, ctx, force=rp)
    return rp


def replay_wav2lip(sd: Dict[str, Tensor], mel: Tensor, face: Tensor, fetch) -> Replay:
    """sd float32; mel (B,1,80,16) and face (B,6,256,256) as the device takes them in (fp16).  fetch(name, ref): the captured layer
    (Engine.debug_get), "output_block.1" = the sigmoid output of the pass."""
    from . import wav2lip_oracle as W
    rp = Replay(sd, fetch)
    W.forward({k: v.double() for k, v in sd.items()}, mel.double(), face.double(), force=rp)
    return rp


def replay_whisper(sd: Dict[str, Tensor], feats: Tensor, fetch) -> Replay:
    """sd: the encoder's float32 state dict; feats (1, 80, 3000): the device's own "input_features"."""
    from . import whisper_oracle as WO
    rp = Replay(sd, fetch)
    rp.may_fuse = WO.FUSED_INTO
    with torch.no_grad():
        WO.encoder_ops({k: v.double() for k, v in sd.items()}, feats.double(), force=rp)
    return rp


def engine_fetch(eng, frames_total: int, frames: Optional[List[int]] = None):
    """fetch() over Engine.musetalk_debug_get: channel blocks of 16 and heads padded to multiples of 16 taken out, d^-0.5 out of
    to_q, frames `frames` of the `frames_total` the pass ran."""
    import numpy as np
    idx = list(range(frames_total)) if frames is None else list(frames)

    def fetch(name: str, ref: Tensor) -> Optional[Tensor]:
        _, C, H, W = ref.shape
        heads = 0
        if name.endswith((".to_q", ".to_k", ".to_v", ".attn")):
            heads = 1 if name.startswith("decoder.") else M.UNET_HEADS
        Cd = heads * ((C // heads + 15) // 16 * 16) if heads else (C + 15) // 16 * 16
        try:
            dev = eng.musetalk_debug_get(name, (frames_total, Cd, H, W))
        except Exception as e:          # the program has no such tensor (a size mismatch is an error of the test, not a fused op)
            if "no MuseTalk tensor named" in str(e):
                return None
            raise
        dev = dev[np.asarray(idx)]
        if heads:
            d = C // heads
            dev = dev.reshape(len(idx), heads, Cd // heads, H, W)[:, :, :d].reshape(len(idx), C, H, W)
        else:
            dev = dev[:, :C]
        t = torch.from_numpy(np.ascontiguousarray(dev)).to(ref.dtype)
        if name.endswith(".to_q"):
            t = t * math.sqrt(C // heads)
        return t

    return fetch


# ---------------------------------------------------------------------------------------------------- simulated device (CPU tests)
class SimDevice:
    """A stand-in for the device that the CPU tests replay against: the float32 oracle with fp16 weights whose every op output is
    rounded to fp16 and kept under the op's name.  `fused`: the names a fused program would not materialise (not rounded, not
    kept).  `mutate`: name -> fn(t, op) applied to that op's output before the rounding - the faults the replay has to find.
    `fp32`: the names whose output the device keeps in fp32 (not rounded)."""

    def __init__(self, fused=(), mutate=None, fp32=()):
        self.t: Dict[str, Tensor] = {}
        self.fused = set(fused)
        self.fp32 = set(fp32)
        self.mutate = mutate or {}
        self.ops = {}

    def describe(self, name, op):
        self.ops[name] = op

    def __call__(self, name, t):
        op = self.ops.pop(name, None)
        if name in self.fused:
            return None
        if name in self.mutate:
            t = self.mutate[name](t, op)
        t = t if name in self.fp32 else f16(t)
        self.t[name] = t.clone()
        return t

    def fetch(self, name, ref):
        if name not in self.t:
            return None
        return self.t[name].to(ref.dtype)


def half_weights(sd: Dict[str, Tensor]) -> Dict[str, Tensor]:
    return {k: (f16(v) if k.endswith(".weight") and v.dim() >= 2 else v) for k, v in sd.items()}
