#!/usr/bin/env python3
"""Times K live Whisper steps as K separate ltk_whisper_step calls against ONE ltk_whisper_step_batch call of K requests and writes
profiles/whisper_batch_step.txt.  Needs an MI355X.

    python scripts/whisper_batch_time.py [--out profiles/whisper_batch_step.txt]

scripts/hubert_batch_time.py's protocol: one job (a child process under its own time limit), the whisper-tiny-shaped encoder with
seeded weights (oracle.whisper_oracle.tiny_whisper(0)), the 52-chunk live clip (16 640 samples: l + 2 x 16 + r chunks of 20 ms) of
K sessions, each with its own audio; per K in 1, 2, 4, 8, 16 five warm-up rounds per leg (the engine captures a program on the
second run of a (program, clip count)), then `--iters` timed rounds; in a round the two legs run back to back (separate, then batched:
interleaved, so that drift of the clock or the box hits both), each timed on the host around calls that end synchronised.  The
separate leg is what K sessions cost without this entry.  Written: the medians of both legs, their ratio, and the activation bytes of
the batched program.  bench.py calls Engine.whisper_step directly, so this record is the only timing of the batched path.  The default
of LTK_WHISPER_BATCH follows from the record by the rule its last line states.
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

N_LIVE = (20 + 2 * 16) * 320
KS = (1, 2, 4, 8, 16)


def run(warmup, iters):
    import torch
    import synth_inputs as synth
    from livetalking_amd.engine import Engine
    from oracle import whisper_oracle as WO
    eng = Engine(0)
    eng.load_whisper({k: v for k, v in WO.tiny_whisper(0).encoder.state_dict().items()})
    import numpy as np
    pcms = [((0.4 + 0.1 * i) * synth.synthetic_audio(2.0, seed=42 + i)[:N_LIVE]).astype(np.float32) for i in range(max(KS))]
    outs = [torch.zeros(16, 50, 384, dtype=torch.float32, device="cuda") for _ in range(max(KS))]
    lines, ratios = [], {}
    for K in KS:
        reqs = [(pcms[i], 16, 10, 2, 10, outs[i].data_ptr()) for i in range(K)]

        def sep():
            for i in range(K):
                eng.whisper_step(pcms[i], 16, 10, outs[i].data_ptr())

        def bat():
            eng.whisper_step_batch(reqs)

        for _ in range(warmup):
            sep()
            bat()
        torch.cuda.synchronize()
        ts, tb = [], []
        for _ in range(iters):
            t0 = time.perf_counter()
            sep()
            t1 = time.perf_counter()
            bat()
            t2 = time.perf_counter()
            ts.append((t1 - t0) * 1e3)
            tb.append((t2 - t1) * 1e3)
        ms, mb = statistics.median(ts), statistics.median(tb)
        ratios[K] = mb / ms
        act = eng.whisper_batch_info()["activation_bytes"]
        lines.append(f"K {K:2d}  separate whisper_step x K: median {ms:8.3f} ms (min {min(ts):8.3f})   one whisper_step_batch: median {mb:8.3f} ms "
                     f"(min {min(tb):8.3f})   batched / separate {mb / ms:5.3f}   per clip {mb / K:6.3f} ms"
                     + (f"   batched program: activation_bytes {act} ({act / 1e6:.1f} MB at 16 clips)" if act
                        else "   (one request: the single-clip path, nothing built)"))
        print(lines[-1], flush=True)
    worst = max(ratios[K] for K in KS if K >= 2)
    lines.append(f"rule: LTK_WHISPER_BATCH defaults on only if the batched call is no slower than the separate calls at K = 2 and at every larger K "
                 f"measured: largest batched / separate over K >= 2 is {worst:.3f} -> default {'on' if worst <= 1.0 else 'off'}")
    print(lines[-1], flush=True)
    eng.close()
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "whisper_batch_step.txt"))
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--child", action="store_true")
    ap.add_argument("--limit", type=int, default=280, help="seconds for the job")
    args = ap.parse_args()
    if args.child:
        import torch
        if not torch.cuda.is_available():
            sys.exit("whisper_batch_time.py measures on a GPU; none found")
        lines = run(args.warmup, args.iters)
        with open(args.out, "a") as f:
            f.write("\n".join(lines) + "\n")
        return
    with open(args.out, "w") as f:
        f.write(f"# scripts/whisper_batch_time.py: Whisper-tiny encoder, seeded weights, {N_LIVE} samples per clip (the 52-chunk live step); K separate\n"
                f"# whisper_step calls against one whisper_step_batch call of K requests, interleaved in one job; host time around calls that end\n"
                f"# synchronised; {args.warmup} warm-up rounds, medians of {args.iters} timed ones\n")
    # one GPU step, under its own time limit; a failure stops the script
    cmd = ["timeout", "-k", "10", str(args.limit), sys.executable, os.path.abspath(__file__), "--child", "--out", args.out,
           "--warmup", str(args.warmup), "--iters", str(args.iters)]
    rc = subprocess.run(cmd).returncode
    if rc:
        sys.exit(f"the job ended with status {rc}")


if __name__ == "__main__":
    main()
