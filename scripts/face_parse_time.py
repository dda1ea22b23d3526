#!/usr/bin/env python3
"""The face parser on the engine at 512 x 512 on seeded weights (synth_inputs.faceparse_state_dict(83)): the record profiles/face_parse.txt.

    python scripts/face_parse_time.py [--out profiles/face_parse.txt] [--images 8] [--repeats 5] [--iters 50]

One MI355X job.  Every GPU step is a child process of its own under `timeout -k 10`, the steps are chained and the first one that
fails ends the job (nothing further is started on the GPU); the record is written when all of them have passed.

  call 1 / call 4   ltk_face_parse with max_images 1 and 4: milliseconds per image of a call over `--images` images - upload, the
                    replayed program and the copy-back of every chunk included, a host clock around the call (it returns synchronised),
                    the median and the extremes of `--repeats` calls behind a warm-up that has seen every chunk size - and the device
                    pass alone (HIP events around `--iters` replays of the captured program, no upload or copy-back), and per-launch
                    times from events between eager launches (they do not add up to the replayed pass: every event costs a gap);
  gates 512         the three end-to-end figures of tests/test_face_parse_gpu.py at 512 on the stored float64 results
                    (tests/golden/faceparse_golden.npz): the share of pixels inside tau, max |device logits - float64|, label
                    disagreement against the rounding model's own.

There is no earlier build to compare with and the reference's PyTorch network does not run on this machine: a record, nothing gates
on it.
"""
from __future__ import annotations

import argparse
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

SIZE = 512
STEPS = [("call", 1, 240), ("call", 4, 240), ("gates", 1, 240)]          # (step, max_images, seconds)


def step_call(max_images: int, images: int, repeats: int, iters: int) -> None:
    import numpy as np
    import torch
    import synth_inputs as synth
    from livetalking_amd.engine import Engine
    if not torch.cuda.is_available():
        sys.exit("needs a GPU: a CPU run measures nothing")
    sd = synth.faceparse_state_dict(83)
    rgb = np.stack([synth.faceparse_image(SIZE, seed=i % 3) for i in range(images)])
    eng = Engine(0)
    eng.load_face_parser(sd, size=SIZE, max_images=max_images)
    for _ in range(3):                                   # eager, captured, replayed - for the full and for the short chunk
        eng.face_parse(rgb)
    ms = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        eng.face_parse(rgb)
        ms.append((time.perf_counter() - t0) * 1e3 / images)
    ms.sort()
    dev, per_op = eng.face_parse_time(max_images, iters, per_op=True)
    prog = Engine.face_parse_program(SIZE)
    print(f"max_images {max_images}: ltk_face_parse over {images} images, upload and copy-back included: "
          f"{ms[len(ms) // 2]:.3f} ms / image (median of {repeats} calls, {ms[0]:.3f} .. {ms[-1]:.3f})")
    print(f"max_images {max_images}: the device pass alone, {max_images} image(s) per replay: {dev:.3f} ms / pass, {dev / max_images:.3f} ms / image "
          f"(events around {iters} replays)")
    print(f"max_images {max_images}: per launch, eager with an event between launches (sum {per_op.sum():.3f} ms), the ten longest:")
    for i in np.argsort(-per_op)[:10]:
        print(f"    {prog[i]['name']:<34} type {prog[i]['type']:>2}  {per_op[i] * 1e3:8.1f} us")
    by_type = {}
    for p, t in zip(prog, per_op):
        by_type[p["type"]] = by_type.get(p["type"], 0.0) + float(t)
    print("    by type: " + ", ".join(f"{k}: {v * 1e3:.0f} us" for k, v in sorted(by_type.items())) + "  (0 conv, 10 stem, 11 max pool, 12 average pool, 13 gate, 14 labels)")
    eng.close()


def step_gates() -> None:
    import numpy as np
    import torch
    import face_parse_cases as C
    import synth_inputs as synth
    from livetalking_amd.engine import Engine
    if not torch.cuda.is_available():
        sys.exit("needs a GPU")
    g = np.load(os.path.join(ROOT, "tests", "golden", "faceparse_golden.npz"))
    sd = synth.faceparse_state_dict(int(g["seed"]))
    rgb = synth.faceparse_image(SIZE, seed=0)[None]
    ref = C.E2E(sd, rgb, g["logits_512"][:1], g["labels_512"][:1])
    eng = Engine(0)
    eng.load_face_parser(sd, size=SIZE, max_images=1)
    labels = eng.face_parse(rgb)
    logits = eng.face_parse_debug_get("conv_out.conv_out", (1, 19, SIZE // 8, SIZE // 8))
    eng.close()
    gated = ref.excluded <= C.EXCLUDED_CAP
    sys.stdout.write(C.record_512(ref, labels, logits, gated))         # the lines tests/test_face_parse_gpu.py appends under LTK_FACE_PARSE_OUT
    ref.gates(labels, logits, label_gate=gated)                         # a failed gate fails the step: no record of a wrong parser


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "face_parse.txt"))
    ap.add_argument("--images", type=int, default=8)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--step", default="", help="(internal) run one step in this process")
    ap.add_argument("--max-images", type=int, default=1)
    args = ap.parse_args()
    if args.step == "call":
        return step_call(args.max_images, args.images, args.repeats, args.iters)
    if args.step == "gates":
        return step_gates()
    lines = [f"# scripts/face_parse_time.py: the BiSeNet face parser on the engine, {SIZE} x {SIZE}, seeded weights; one MI355X job, a record that gates nothing"]
    for step, max_images, seconds in STEPS:
        cmd = ["timeout", "-k", "10", str(seconds), sys.executable, os.path.abspath(__file__), "--step", step, "--max-images", str(max_images),
               "--images", str(args.images), "--repeats", str(args.repeats), "--iters", str(args.iters)]
        r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
        sys.stdout.write(r.stdout)
        if r.returncode:                                 # a failed, faulted or timed-out step: nothing more is started
            sys.exit(f"step {step} (max_images {max_images}) ended with status {r.returncode}: no record written")
        lines += [ln for ln in r.stdout.splitlines() if ln.startswith(("max_images", "512 x 512", "    "))]
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print(f"wrote {args.out}")


if __name__ == "__main__":
    main()
