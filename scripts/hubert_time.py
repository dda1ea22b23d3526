#!/usr/bin/env python3
"""Times HuBERT-large on the engine against what the Ultralight plugin does by default (transformers' HubertModel in torch fp32
on the same GPU; a torch fp16 leg for information) and writes profiles/hubert_step.txt.  Needs an MI355X.

    python scripts/hubert_time.py [--out profiles/hubert_step.txt] [--layers 24]

Legs, each a child process under its own time limit, chained (a leg that fails ends the run):
  live   the live step: 16 640 samples (l + 2 x 16 + r chunks of 20 ms), the forward plus the chunk gather into device memory
  clip   the 320 080-sample clip of an offline call (one forward, 1 000 rows, features to the host)
Weights are seeded (tests/hubert_ref.py), the depth is the real one (24).  Per leg: warm-up calls (the engine captures its program
on the second one), then the median and the spread of `--iters` calls, each timed on the host around a call that ends in a device
synchronise: that is what a session's audio thread waits for.  Per-kernel shares are NOT part of this record: they want a
`rocprofv3 --kernel-trace --stats` run of their own, which has not been made (DESIGN.md §3.8 says so).
"""
import argparse
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

os.environ.setdefault("LTK_ALLOW_STANDIN", "1")      # the plugin module's host classes, outside a LiveTalking checkout

LEGS = {"live": 16640, "clip": 320080}


def _time(fn, warmup, iters):
    import torch
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(iters):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e3)
    ts.sort()
    return statistics.median(ts), ts[0], ts[int(0.9 * (len(ts) - 1))]


def run_leg(leg, layers, warmup, iters):
    import numpy as np
    import torch
    import hubert_ref as H
    from transformers import HubertModel
    from livetalking_amd.engine import Engine
    from livetalking_amd.avatars.audio_features.hubert import feature2chunks
    n = LEGS[leg]
    sd = H.state_dict(layers, 7)
    pcm = H.speech(n, 12)
    lines = []

    def line(what, r):
        lines.append(f"{leg:5s} {n:7d} samples  {what:44s} median {r[0]:8.3f} ms   min {r[1]:8.3f}   p90 {r[2]:8.3f}")
        print(lines[-1], flush=True)

    eng = Engine(0)
    eng.load_hubert(sd)
    if leg == "live":
        d_out = torch.zeros(16, 16, 1024, dtype=torch.float32, device="cuda")
        line("engine: hubert_step (forward + device chunks)", _time(lambda: eng.hubert_step(pcm, 16, 2, d_out.data_ptr()), warmup, iters))
    line("engine: hubert_features (forward + rows to host)", _time(lambda: eng.hubert_features(pcm), warmup, iters))
    dev = eng.hubert_features(pcm)
    lines.append(f"{leg:5s} activation memory of the {dev.shape[0]}-row program: {eng.hubert_info()['activation_bytes'] / 1e6:.1f} MB")
    eng.close()

    model = HubertModel(H.config(layers)).eval()
    model.load_state_dict({k: torch.as_tensor(v) for k, v in sd.items()}, strict=True)
    model = model.cuda()
    x = torch.from_numpy(H.normalise(pcm).astype(np.float32))[None]

    def torch_call(m, dtype):
        with torch.no_grad():
            feat = m(x.cuda().to(dtype)).last_hidden_state[0].float().cpu().numpy()       # as Audio2Feature: input up, rows down
        return feature2chunks(feat, 16, [4, 4], 5, 2) if leg == "live" else feat

    line("torch fp32: HubertModel, rows to host" + (" + chunks" if leg == "live" else ""), _time(lambda: torch_call(model, torch.float32), warmup, iters))
    ref = torch_call(model, torch.float32)
    ref = np.stack(ref) if leg == "live" else ref
    half = model.half()
    line("torch fp16 (information)", _time(lambda: torch_call(half, torch.float16), warmup, iters))
    if leg == "clip":
        rel = float(np.linalg.norm(dev.astype(np.float64) - ref) / np.linalg.norm(ref))
        lines.append(f"{leg:5s} engine vs torch fp32 on the same input: rel L2 {rel:.3e}")
        print(lines[-1], flush=True)
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "hubert_step.txt"))
    ap.add_argument("--layers", type=int, default=24)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--iters", type=int, default=40)
    ap.add_argument("--leg", choices=list(LEGS))
    ap.add_argument("--limit", type=int, default=280, help="seconds per leg")
    args = ap.parse_args()
    if args.leg:
        import torch
        if not torch.cuda.is_available():
            sys.exit("hubert_time.py measures on a GPU; none found")
        with open(args.out, "a") as f:
            f.write("\n".join(run_leg(args.leg, args.layers, args.warmup, args.iters)) + "\n")
        return
    with open(args.out, "w") as f:
        f.write(f"# scripts/hubert_time.py: HuBERT-large, {args.layers} layers, seeded weights; host time around a call that ends in a device synchronise;\n"
                f"# {args.warmup} warm-up calls, {args.iters} timed ones per line\n")
    for leg in LEGS:
        cmd = ["timeout", "-k", "10", str(args.limit), sys.executable, os.path.abspath(__file__), "--leg", leg, "--out", args.out,
               "--layers", str(args.layers), "--warmup", str(args.warmup), "--iters", str(args.iters)]
        rc = subprocess.run(cmd).returncode
        if rc:
            sys.exit(f"leg {leg} ended with status {rc}; stopping")


if __name__ == "__main__":
    main()
