"""Cases, float64 reference, gates and a simulated device for the batched HuBERT live step (TEST INFRASTRUCTURE ONLY).

Shared by tests/test_hubert_batch_gpu.py (the device behind Engine.hubert_step_batch) and tests/test_hubert_batch_host.py (SimBatch
below, with and without planted faults): both hold every clip of a batch to the SAME functions here, so a gate that cannot see a
batching fault on the CPU cannot be trusted to see it on the GPU.

The reference is per clip, never per batch: tests/hubert_ref.py's float64 forward / replay of ONE clip, called clip by clip.  The
gates are oracle.op_replay's, constants unchanged (per element |dev - ref| <= tol, aggregate rel L2 <= AGG_FACTOR x the rounding
model's + AGG_FLOOR, the rounding model inside MODEL_HEADROOM of the bound), the 1e-6 rel L2 of tests/test_hubert_gpu.py for the
normalised waveform, and byte equality for the chunk gather (fp16 rows as float32 on both sides).
"""
from __future__ import annotations

from typing import Callable, Dict, List, Optional, Sequence

import numpy as np
import torch
import torch.nn.functional as F

import hubert_ref as H
from oracle import op_replay as R

CAPACITY = 16                      # kHubertBatchClips
BUDGET = 2 << 30                   # activation bytes of a batched program at full capacity stay under this
ROWS3, LIVE, ROWS70 = 1040, 16640, 22613          # 3 rows (nearly every positional tap is padding), 51 (live, row GEMM), 70 (conv3 over N images)

# (clips, samples) of the op replay: nf = 2 and 3 at every length; 11 x 51 = 561 rows cross kLinFkMinRows = 512
REPLAY_CASES = [(2, ROWS3), (3, ROWS3), (2, LIVE), (3, LIVE), (2, ROWS70), (3, ROWS70), (11, LIVE)]
MIXED = [ROWS3, LIVE, ROWS3, ROWS70, LIVE]        # plan edges: lengths of one call, in arrival order


def clips(nf: int, n: int, seed: int = 100) -> List[np.ndarray]:
    """nf clips of n samples that differ in seed, gain (0.1 .. 3) and DC offset: clip 1 sits at +100 next to the zero-mean clip 0,
    so statistics taken over more than one clip, or a neighbour's rows read as padding, are errors at full size."""
    gains = np.linspace(0.1, 3.0, nf) if nf > 1 else np.array([1.0])
    return [(gains[i] * H.speech(n, seed + i) + (100.0 if i == 1 else 0.0)).astype(np.float32) for i in range(nf)]


def chunk_spec(i: int, n: int):
    """(batch, first_row, row_step, rows) of request i of a call: windows that leave the clip on the left (first_row < 0) and on the
    right (the last frame ends past row T - 1), different per request."""
    T = H.rows(n)
    batch = 2 + i % 3
    first_row = -7 + 2 * (i % 4)
    while first_row + 2 * (batch - 1) + 16 <= T:            # the last window must pass the clip's end
        batch += 1
    return batch, first_row, 2, 16


def host_chunks(feat: np.ndarray, batch: int, first_row: int) -> np.ndarray:
    """feature2chunks (rows 16, step 2) of one request on its own features: start such that frame i begins at first_row + 2 i."""
    from livetalking_amd.avatars.audio_features.hubert import feature2chunks
    return np.stack(feature2chunks(feat, batch, [4, 4], (first_row + 8) / 2, 2))


# ---------------------------------------------------------------------------------------------------- the plan, restated
def expected_plan(lengths: Sequence[int], clip_bytes: Callable[[int], int]):
    """-> [(n_samples, batched, [request indices])] in execution order: groups by length in arrival order, runs of at most CAPACITY, a
    run of one or a length over the budget one request at a time on the single-clip path."""
    runs, seen = [], []
    for n in lengths:
        if n not in seen:
            seen.append(n)
    for n in seen:
        group = [r for r, m in enumerate(lengths) if m == n]
        fits = clip_bytes(n) * CAPACITY < BUDGET
        for i0 in range(0, len(group), CAPACITY):
            part = group[i0:i0 + CAPACITY]
            if fits and len(part) > 1:
                runs.append((n, True, part))
            else:
                runs += [(n, False, [r]) for r in part]
    return runs


def device_plan(lengths: Sequence[int], layers: int):
    """ltk_debug_hubert_batch_plan (no GPU) in expected_plan's form, and the bytes of one clip per request."""
    import ctypes as C
    from livetalking_amd import _lib
    lib = _lib.load()
    n = len(lengths)
    ns = (C.c_int * n)(*lengths)
    run_of, slot_of, batched, n_runs, cb = (C.c_int * n)(), (C.c_int * n)(), (C.c_int * n)(), C.c_int(), (C.c_size_t * n)()
    _lib.check(lib.ltk_debug_hubert_batch_plan(ns, n, layers, run_of, slot_of, batched, C.byref(n_runs), cb))
    runs = [[None, bool(batched[i]), {}] for i in range(n_runs.value)]
    for r in range(n):
        runs[run_of[r]][0] = lengths[r]
        assert slot_of[r] not in runs[run_of[r]][2]
        runs[run_of[r]][2][slot_of[r]] = r
    return [(nn, b, [slots[j] for j in range(len(slots))]) for nn, b, slots in runs], list(cb)


# ---------------------------------------------------------------------------------------------------- gates
def gate_input_values(x_dev: np.ndarray, pcm: np.ndarray, label: str = "") -> float:
    """The device's normalised waveform of ONE clip against hubert_ref.normalise of that clip alone: rel L2 <= 1e-6."""
    rel = R.rel_l2(torch.from_numpy(np.asarray(x_dev, dtype=np.float32)), torch.from_numpy(H.normalise(pcm)))
    print(f"{label} input_values rel_l2 {rel:.3e}")
    assert rel <= 1e-6, f"{label}: input_values rel L2 {rel:.3e} > 1e-6 (statistics of another clip, or of the batch?)"
    return rel


def gate_replay(sd, x_norm: np.ndarray, get: Callable[[str, tuple], np.ndarray], ops, label: str = "", model_too: bool = False):
    """hubert_ref.replay of ONE clip on the device's own input_values of that clip.  get(name, (C, T)) -> the device's tensor of
    the clip as Engine.hubert_debug_get returns it (q_proj carries the folded d^-0.5).  Every op of `ops` compared, none outside
    op_replay's gates."""
    def fetch(name, ref):
        _, C, T, _ = ref.shape
        t = torch.from_numpy(np.ascontiguousarray(get(name, (C, T)), dtype=np.float32)).reshape(1, C, T, 1).to(ref.dtype)
        return t * 8.0 if name.endswith(".q_proj") else t

    rp = H.replay(sd, x_norm, fetch)
    for ln in R.format_records(label, rp.records):
        print(ln)
    miss = R.uncovered(ops, [r["name"] for r in rp.records], {})
    assert not miss, f"{label}: ops not compared: {miss}"
    bad = R.failures(rp.records, model_too=model_too)
    assert not bad, label + "\n" + "\n".join(bad)
    return rp.records


def gate_chunks(got: np.ndarray, feat: np.ndarray, batch: int, first_row: int, label: str = ""):
    """A request's device chunks against feature2chunks of ITS OWN features: byte for byte."""
    want = host_chunks(feat, batch, first_row)
    got = np.asarray(got)
    assert got.shape == want.shape, f"{label}: {got.shape} for {want.shape}"
    diff = int((got != want).sum())
    print(f"{label} chunks: {diff} of {want.size} values differ, max |d| {float(np.abs(got - want).max()):.3e}")
    assert np.array_equal(got, want), f"{label}: {diff} of {want.size} chunk values differ from the request's own feature2chunks"


def sim_ops(layers: int):
    """[(name, type)] as Engine.hubert_ops() gives it (type 3 = attention)."""
    return [(nm, 3 if nm.endswith(".attention") else 0) for nm in H.op_names(layers)]


# ---------------------------------------------------------------------------------------------------- simulated device
FAULTS = ("stats_over_batch", "posconv_reads_neighbour", "conv_crosses_clip", "attention_over_all_keys", "chunks_clamped_to_batch",
          "outputs_in_grouped_order")


class _Hook:
    """force object of hubert_ref.forward: keeps every op's output (after `mutate[name](t, op)`) and every op's description."""

    def __init__(self, mutate: Optional[Dict[str, Callable]] = None):
        self.t: Dict[str, torch.Tensor] = {}
        self.ops: Dict[str, dict] = {}
        self.mutate = mutate or {}
        self._op = None

    def describe(self, name, op):
        self.ops[name] = op
        self._op = op

    def __call__(self, name, t):
        if name in self.mutate:
            t = self.mutate[name](t, self.ops.get(name)).half().double()
        self.t[name] = t.clone()
        return t


class SimBatch:
    """The batched step as a device would run it, in float64 with the fp16 rounding model (hubert_ref.forward(fp16_model=True)):
    per clip statistics, per clip forward, per request chunk gather in request order.  `fault` plants ONE batching fault:
      stats_over_batch         mean and variance taken over all clips of a run
      posconv_reads_neighbour  the positional conv runs over the run's rows as one sequence: taps that leave a clip read the neighbour
      conv_crosses_clip        conv layer 1 runs over the run's layer-0 maps as one sequence (207 = 2 x 103 + 1 rows: clip i's outputs
                               start one row inside clip i - 1)
      attention_over_all_keys  layer 0's softmax runs over the keys and values of every clip of the run
      chunks_clamped_to_batch  the chunk gather clamps into [0, nf T) of the run instead of the clip's own [0, T)
      outputs_in_grouped_order request r receives the chunks of the r-th clip in run order instead of its own
    reqs: [(pcm, batch, first_row)] (row_step 2, rows 16); the call is cut by expected_plan."""

    def __init__(self, sd, reqs, fault: Optional[str] = None):
        assert fault is None or fault in FAULTS
        self.sd, self.reqs, self.fault = H.fold_weight_norm(sd), reqs, fault
        lengths = [len(p) for p, _, _ in reqs]
        self.runs = expected_plan(lengths, lambda n: 0)
        self.x: Dict[int, np.ndarray] = {}              # request -> input_values (float32)
        self.t: Dict[int, Dict[str, torch.Tensor]] = {}
        self.out: Dict[int, np.ndarray] = {}
        order = []
        for n, _, members in self.runs:
            self._run(members)
            order += members
        if fault == "outputs_in_grouped_order":
            self.out = {r: self._own_shape(self.out[order[r]], r) for r in range(len(reqs))}

    def _own_shape(self, a, r):
        b = self.reqs[r][1]
        return np.resize(a, (b, 16, 1024)) if a.shape[0] != b else a

    def _run(self, members):
        pcm = [np.asarray(self.reqs[r][0], dtype=np.float64) for r in members]
        if self.fault == "stats_over_batch":
            allx = np.concatenate(pcm)
            xs = [((p - allx.mean()) / np.sqrt(allx.var() + 1e-7)).astype(np.float32) for p in pcm]
        else:
            xs = [H.normalise(p).astype(np.float32) for p in pcm]
        clean = []
        for x in xs:                                    # what every clip's ops see when nothing crosses a clip
            hk = _Hook()
            H.forward(self.sd, x, fp16_model=True, force=hk)
            clean.append(hk)
        w16 = lambda name: self.sd[name].float().half().double()
        for i, r in enumerate(members):
            mutate = {}
            if self.fault == "posconv_reads_neighbour":
                def pos(t, op, i=i):
                    X = torch.cat([c.ops["encoder.pos_conv_embed"]["x"] for c in clean], dim=1)
                    pc = F.conv1d(X.transpose(1, 2), w16(H.W_KEY), self.sd["encoder.pos_conv_embed.conv.bias"], padding=H.POS_K // 2,
                                  groups=H.POS_GROUPS)[:, :, :-1]
                    y = (X + F.gelu(pc.transpose(1, 2)))[:, i * t.shape[2]:(i + 1) * t.shape[2]]
                    return y.transpose(1, 2)[..., None]
                mutate["encoder.pos_conv_embed"] = pos
            if self.fault == "conv_crosses_clip":
                p = "feature_extractor.conv_layers.1.conv"

                def conv(t, op, i=i, p=p):
                    X = torch.cat([c.ops[p]["x"] for c in clean] + [torch.zeros_like(clean[0].ops[p]["x"])], dim=2)
                    y = F.conv1d(X, w16(p + ".weight"), self.sd[p + ".bias"], stride=H.CONV_S[1])
                    return y[:, :, i * t.shape[2]:(i + 1) * t.shape[2], None]
                mutate[p] = conv
            if self.fault == "attention_over_all_keys":
                a = "encoder.layers.0.attention.attn"

                def attn(t, op, a=a):
                    K = torch.cat([c.ops[a]["k"] for c in clean], dim=2)
                    V = torch.cat([c.ops[a]["v"] for c in clean], dim=2)
                    q = op["q"]
                    o = torch.softmax(q @ K.transpose(-1, -2) * q.shape[-1] ** -0.5, dim=-1) @ V
                    return o.transpose(1, 2).reshape(1, q.shape[2], -1).transpose(1, 2)[..., None]
                mutate[a] = attn
            hk = clean[i]
            if mutate:
                hk = _Hook(mutate)
                H.forward(self.sd, xs[i], fp16_model=True, force=hk)
            self.x[r], self.t[r] = xs[i], hk.t
        feats = [self.features(r) for r in members]
        T = feats[0].shape[0]
        for i, r in enumerate(members):
            _, batch, first_row = self.reqs[r]
            idx = first_row + 2 * np.arange(batch)[:, None] + np.arange(16)[None]
            if self.fault == "chunks_clamped_to_batch":
                self.out[r] = np.concatenate(feats)[np.clip(i * T + idx, 0, len(members) * T - 1)]
            else:
                self.out[r] = feats[i][np.clip(idx, 0, T - 1)]

    # -- what the tests read, per request
    def features(self, r) -> np.ndarray:
        return self.t[r]["encoder.layer_norm"][0, :, :, 0].T.numpy().astype(np.float32)

    def input_values(self, r) -> np.ndarray:
        return self.x[r]

    def get(self, r):
        def get(name, shape):
            t = self.t[r][name][0, :, :, 0].numpy().astype(np.float32)
            assert t.shape == tuple(shape), (name, t.shape, shape)
            return t / 8.0 if name.endswith(".q_proj") else t
        return get
