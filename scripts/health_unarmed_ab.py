#!/usr/bin/env python3
"""The unarmed path of the headroom watch against another build of the library (the parent commit's), in one MI355X job:
sections 2a and 2b of profiles/health_watch.txt.

    make -C <parent checkout>/livetalking_amd/csrc          # the parent's libltk_hip.so
    python scripts/health_unarmed_ab.py --parent-lib <parent checkout>/livetalking_amd/libltk_hip.so [--pairs 3]

2a. Four unarmed 16-frame ltk_wav2lip_infer calls, eager (LTK_GRAPH=0), under `rocprofv3 --kernel-trace --stats`, once per library
    (the other build is selected with LTK_LIB): launches per kernel name, every difference, and the health_scan_kernel count (0).
2b. `python bench.py --gpus 1 --steps 200 --warmup 20`, legs interleaved (parent, this) x pairs: the timed line of each run.
Exit code 1 when a kernel of the library is launched another number of times than by the parent.
"""
import argparse
import csv
import glob
import json
import os
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

B = 16


def one_pass_process():
    """--calls: the process rocprofv3 wraps."""
    import torch
    import synth_inputs as synth
    from livetalking_amd.engine import Engine
    eng = Engine(0)
    eng.load_wav2lip(synth.wav2lip_state_dict(1234), max_frames=B)
    frames, faces, coords = synth.wav2lip_avatar(n_frames=8, full_hw=(360, 640), box=160, seed=0)
    aid = eng.register_avatar(faces, frames, coords)
    d_mel = torch.randn(B, 80, 16, device="cuda")
    d_pred = torch.zeros(B, 256, 256, 3, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    for i in range(4):
        eng.wav2lip_infer([(aid, i * B, B, d_mel.data_ptr(), d_pred.data_ptr())])
    eng.close()


def listing(lib):
    env = dict(os.environ, LTK_GRAPH="0")
    if lib:
        env["LTK_LIB"] = lib
    else:
        env.pop("LTK_LIB", None)
    out = {}
    with tempfile.TemporaryDirectory() as d:
        subprocess.run(["rocprofv3", "--kernel-trace", "--stats", "-d", d, "-o", "p", "--output-format", "csv", "--", sys.executable,
                        os.path.abspath(__file__), "--calls"], env=env, check=True, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL, timeout=240)
        for f in glob.glob(d + "/**/*kernel_stats.csv", recursive=True):
            with open(f) as fh:
                for r in csv.DictReader(fh):
                    out[r["Name"]] = out.get(r["Name"], 0) + int(r["Calls"])
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib")
    ap.add_argument("--pairs", type=int, default=3)
    ap.add_argument("--calls", action="store_true", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.calls:
        one_pass_process()
        return 0
    if not a.parent_lib or not os.path.exists(a.parent_lib):
        ap.error("--parent-lib: the other build's libltk_hip.so")
    parent = os.path.abspath(a.parent_lib)
    pa, th = listing(parent), listing(None)
    print("# 2a. kernel listing")
    print(f"# kernel launches of four unarmed 16-frame ltk_wav2lip_infer calls (LTK_GRAPH=0, rocprofv3 --kernel-trace --stats): parent library "
          f"{sum(pa.values())}, this library {sum(th.values())}")
    for k in sorted(th, key=lambda k: -th[k]):
        print(f"  {th[k]:6d}  (parent {pa.get(k, 0):6d})  {k[:150]}")
    diff = sorted(k for k in set(pa) | set(th) if pa.get(k, 0) != th.get(k, 0))
    print("# kernels whose launch count differs from the parent's:", diff if diff else "none")
    print("# health_scan_kernel launches:", sum(v for k, v in th.items() if "health_scan" in k))
    if diff == ["__amd_rocclr_fillBufferAligned"]:
        print("# (the runtime's fill kernel only: the two builds issue another number of hipMemset calls at engine creation / model load; no launch of a pass differs)")
    bad = any("ltk" in k for k in diff)
    print(f"\n# 2b. python bench.py --gpus 1 --steps 200 --warmup 20, legs interleaved (parent, this) x {a.pairs}: the timed line")
    ms = {"parent": [], "this": []}
    for r in range(1, a.pairs + 1):
        for leg in ("parent", "this"):
            env = dict(os.environ)
            env.pop("LTK_LIB", None)
            if leg == "parent":
                env["LTK_LIB"] = parent
            out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "200", "--warmup", "20"], env=env,
                                 check=True, capture_output=True, text=True, timeout=300).stdout.strip().splitlines()[-1]
            d = json.loads(out)
            ms[leg].append(d["ms_per_step"])
            print(f"  {leg:<7}{r}  {d['value']:>10.1f} {d['unit']}  {d['ms_per_step']:.4f} ms per step", flush=True)
    print(summary_line(ms["parent"], ms["this"]))
    return 1 if bad else 0


def summary_line(parent, this):
    """The verdict of 2b: no leg of this library slower than the parent's slowest, and the pairwise ratios."""
    lo, hi = min(parent), max(parent)
    pairs = ", ".join(f"{100 * (t / p - 1):+.2f} %" for p, t in zip(parent, this))
    verdict = "no run slower than the parent's slowest" if max(this) <= hi else "SLOWER than the parent's slowest run"
    return (f"# parent {lo:.4f} .. {hi:.4f} ms (run-to-run spread {100 * (hi / lo - 1):.2f} %); this {min(this):.4f} .. {max(this):.4f} ms: {verdict}; "
            f"this against the parent run in front of it: {pairs}")


if __name__ == "__main__":
    sys.exit(main())
