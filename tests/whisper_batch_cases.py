"""What tests/test_whisper_batch_host.py (CPU) and tests/test_whisper_batch_gpu.py share: the clips of a batched Whisper run, the
float64 replay of one clip and the host restatement of the chunk gather.

Clip i of a run is synth.synthetic_audio under seed 42 + i, cut to one of three lengths - 3 200 samples (21 log-mel frames), the
16 640-sample live step of a 16-frame session, 80 000 samples - and scaled by 1 (even i) or 1e-3 (odd i), so that no two clips of a
run share a spectral maximum.  The length index is (i + i // 3) % 3: the clips the GPU file replays against float64 - 0 and 1 of a
2-clip run, 0, 7 and 15 of a 16-clip run - then cover the three lengths and both amplitudes."""
from __future__ import annotations

import numpy as np

import synth_inputs as synth

CAPACITY = 16                                   # csrc/nn_kernels.h kWhisperBatchClips
LIVE = (20 + 2 * 16) * 320                      # the 52-chunk buffer of one step at batch_size 16
LENGTHS = (3200, LIVE, 80000)
REPLAY_CLIPS = (0, 1, 7, 15)                    # every clip index the GPU file replays


def clip(i: int) -> np.ndarray:
    n = LENGTHS[(i + i // 3) % 3]
    amp = 1.0 if i % 2 == 0 else 1e-3
    return (synth.synthetic_audio(5.0, seed=42 + i)[:n] * np.float32(amp)).astype(np.float32)


def clips(n: int):
    return [clip(i) for i in range(n)]


def expected_plan(nreq: int):
    """[(batched, [requests])]: runs of at most CAPACITY in request order, a run of one on the single-clip path."""
    runs = []
    for r0 in range(0, nreq, CAPACITY):
        members = list(range(r0, min(r0 + CAPACITY, nreq)))
        runs.append((len(members) > 1, members))
    return runs


def replay(sd, feats, get, R, WO):
    """oracle.op_replay.replay_whisper over `get(name, (C, T)) -> float32 array`, the fetch of
    tests/test_op_replay_gpu.py::test_whisper_encoder_step: d^-0.5 = 1 / 8 taken out of q_proj, conv2 compared through the positions
    added in place.  -> (replay, uncovered op names)"""
    import torch

    def fetch(name, ref):
        if name in WO.FUSED_INTO:
            return None
        _, C, T, _ = ref.shape
        t = torch.from_numpy(get(name, (C, T))).reshape(1, C, T, 1).to(ref.dtype)
        return t * 8.0 if name.endswith(".q_proj") else t

    rp = R.replay_whisper(sd, feats, fetch)
    layers = len({k.split(".")[1] for k in sd if k.startswith("layers.")})
    miss = R.uncovered([(n, 0) for n in WO.encoder_op_names(layers)], [r["name"] for r in rp.records], WO.FUSED_INTO)
    return rp, miss


def host_chunks(states, batch: int, first_row: int, row_step: int, rows: int) -> np.ndarray:
    """whisper_chunks_kernel on the host: states = the five hidden states of ONE clip, each float32 [384][1500] (as the debug
    read-back hands them over) -> float32 [batch][rows * 5][384]; frame f takes rows [first_row + f * row_step, + rows), clamped."""
    st = np.stack([np.asarray(s).T for s in states], axis=1)                 # [1500][5][384]
    T = st.shape[0]
    out = np.empty((batch, rows * 5, 384), np.float32)
    for f in range(batch):
        idx = np.clip(first_row + f * row_step + np.arange(rows), 0, T - 1)
        out[f] = st[idx].reshape(rows * 5, 384)
    return out
