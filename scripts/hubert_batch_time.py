#!/usr/bin/env python3
"""Times K live HuBERT steps as K sequential ltk_hubert_step calls against ONE ltk_hubert_step_batch call of K requests and writes
profiles/hubert_batch_step.txt.  Needs an MI355X.

    python scripts/hubert_batch_time.py [--out profiles/hubert_batch_step.txt] [--layers 24]

scripts/hubert_time.py's protocol: one job (a child process under its own time limit), 24 layers, seeded weights (tests/hubert_ref.py),
live length (16 640 samples: l + 2 x 16 + r chunks of 20 ms, 16 frames of chunks per session), per K in 1, 2, 4, 8, 16 five warm-up
calls per leg (the engine captures a program on the second run of a (program, clip count)), then `--iters` timed rounds; in a
round the two legs run back to back (sequential, then batched: interleaved, so that drift of the clock or the box hits both), each
timed on the host around calls that end synchronised.  The sequential leg is what K sessions cost without this entry.  Written: the
medians of both legs, their ratio, and the activation bytes of the batched program.  The default of LTK_HUBERT_BATCH follows from
the K = 8 line by the rule the record states.
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

os.environ.setdefault("LTK_ALLOW_STANDIN", "1")

N_LIVE = 16640
KS = (1, 2, 4, 8, 16)
RULE = 0.92          # on by default only if the batched call at K = 8 takes at most this share of eight sequential steps


def run(layers, warmup, iters):
    import torch
    import hubert_ref as H
    from livetalking_amd.engine import Engine
    sd = H.state_dict(layers, 7)
    eng = Engine(0)
    eng.load_hubert(sd)
    pcms = [(0.3 + 0.15 * i) * H.speech(N_LIVE, 12 + i) for i in range(max(KS))]
    outs = [torch.zeros(16, 16, 1024, dtype=torch.float32, device="cuda") for _ in range(max(KS))]
    lines = []
    for K in KS:
        reqs = [(pcms[i], 16, 2, 2, 16, outs[i].data_ptr()) for i in range(K)]

        def seq():
            for i in range(K):
                eng.hubert_step(pcms[i], 16, 2, outs[i].data_ptr())

        def bat():
            eng.hubert_step_batch(reqs)

        for _ in range(warmup):
            seq()
            bat()
        torch.cuda.synchronize()
        ts, tb = [], []
        for _ in range(iters):
            t0 = time.perf_counter()
            seq()
            t1 = time.perf_counter()
            bat()
            t2 = time.perf_counter()
            ts.append((t1 - t0) * 1e3)
            tb.append((t2 - t1) * 1e3)
        ms, mb = statistics.median(ts), statistics.median(tb)
        act = eng.hubert_batch_info()["activation_bytes"]
        lines.append(f"K {K:2d}  sequential hubert_step x K: median {ms:8.3f} ms (min {min(ts):8.3f})   one hubert_step_batch: median {mb:8.3f} ms "
                     f"(min {min(tb):8.3f})   batched / sequential {mb / ms:5.3f}   per clip {mb / K:6.3f} ms"
                     + (f"   batched program: {act / 1e6:.1f} MB of activations at 16 clips" if act else "   (one request: the single-clip path)"))
        print(lines[-1], flush=True)
        if K == 8:
            ratio8 = mb / ms
    lines.append(f"rule: LTK_HUBERT_BATCH defaults on only if batched / sequential at K = 8 is at most {RULE}: measured {ratio8:.3f} -> "
                 f"default {'on' if ratio8 <= RULE else 'off'}")
    print(lines[-1], flush=True)
    eng.close()
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "hubert_batch_step.txt"))
    ap.add_argument("--layers", type=int, default=24)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--child", action="store_true")
    ap.add_argument("--limit", type=int, default=280, help="seconds for the job")
    args = ap.parse_args()
    if args.child:
        import torch
        if not torch.cuda.is_available():
            sys.exit("hubert_batch_time.py measures on a GPU; none found")
        lines = run(args.layers, args.warmup, args.iters)
        with open(args.out, "a") as f:
            f.write("\n".join(lines) + "\n")
        return
    with open(args.out, "w") as f:
        f.write(f"# scripts/hubert_batch_time.py: HuBERT-large, {args.layers} layers, seeded weights, {N_LIVE} samples per clip; K sequential\n"
                f"# hubert_step calls against one hubert_step_batch call of K requests, interleaved in one job; host time around calls that end\n"
                f"# synchronised; {args.warmup} warm-up rounds, medians of {args.iters} timed ones\n")
    cmd = ["timeout", "-k", "10", str(args.limit), sys.executable, os.path.abspath(__file__), "--child", "--out", args.out,
           "--layers", str(args.layers), "--warmup", str(args.warmup), "--iters", str(args.iters)]
    rc = subprocess.run(cmd).returncode
    if rc:
        sys.exit(f"the job ended with status {rc}")


if __name__ == "__main__":
    main()
