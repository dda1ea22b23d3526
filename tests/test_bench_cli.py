"""bench.py's command line: `--dump-outputs` (the frames of the last timed step, whole or as a fixed seeded sample) and the plain
run against `--full` (a plain run times the steps only; what else the bench measures is behind --full)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BENCH = os.path.join(ROOT, "bench.py")


def _frames(S, B, seed):
    import torch
    g = torch.Generator().manual_seed(seed)
    return [list(torch.randint(0, 256, (B, 256, 256, 3), generator=g, dtype=torch.uint8).unbind(0)) for _ in range(S)]


def test_dump_outputs_writes_every_frame_as_float32(tmp_path):
    pytest.importorskip("torch")
    sys.path.insert(0, ROOT)
    import bench
    last = _frames(2, 3, 0)
    bench.dump_outputs(str(tmp_path / "out"), last)
    got = np.load(tmp_path / "out" / "frames.npy")
    assert got.dtype == np.float32 and got.shape == (2, 3, 256, 256, 3)
    assert np.array_equal(got, np.stack([np.stack([f.numpy() for f in s]) for s in last]).astype(np.float32))
    assert not (tmp_path / "out" / "frames_index.npy").exists()


def test_dump_outputs_samples_large_outputs_within_budget(tmp_path):
    pytest.importorskip("torch")
    sys.path.insert(0, ROOT)
    import bench
    last = _frames(8, 16, 1)                          # 128 frames, 100 MB as float32: above the budget
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), last)
    total = sum(os.path.getsize(tmp_path / "a" / f) for f in os.listdir(tmp_path / "a"))
    assert total <= bench.DUMP_BYTES
    frames, idx = np.load(tmp_path / "a" / "frames.npy"), np.load(tmp_path / "a" / "frames_index.npy")
    assert frames.dtype == np.float32 and idx.dtype == np.float64 and len(frames) == len(idx) > 64
    assert np.all(np.diff(idx) > 0) and idx[-1] < 8 * 16
    for f, i in zip(frames, idx.astype(int)):
        assert np.array_equal(f, last[i // 16][i % 16].numpy().astype(np.float32))
    # the sample is fixed: the same frames every run
    assert np.array_equal(idx, np.load(tmp_path / "b" / "frames_index.npy"))


@pytest.mark.gpu
def test_plain_bench_run_is_lean_and_dumps_its_last_step(tmp_path):
    """The plain line times its steps and nothing else (no roofline, sustained twin, PCIe figure, other configs or CPU baseline)
    and --dump-outputs writes the 16 frames of the last timed step; the same arguments twice give the same frames."""
    torch = pytest.importorskip("torch")
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    outs = []
    for k in range(2):
        d = tmp_path / f"dump{k}"
        r = subprocess.run([sys.executable, BENCH, "--gpus", "1", "--steps", "3", "--warmup", "1", "--dump-outputs", str(d)],
                           capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stderr[-3000:]
        line = json.loads([l for l in r.stdout.strip().splitlines() if l.startswith("{")][-1])
        assert line["metric"] == "inferfps" and line["unit"] == "frames/s" and line["higher_is_better"] is True
        assert line["dtype"] == "f16" and line["steps"] == 3 and line["warmup"] == 1
        assert abs(line["value"] - 3 * 16 / (line["ms_per_step"] * 3e-3)) <= 0.01 * line["value"]
        assert line["roofline"] is None
        for key in ("sustained", "pcie_inclusive", "also", "paced", "delivered", "cpu_baseline"):
            assert key not in line, key
        frames = np.load(d / "frames.npy")
        assert frames.dtype == np.float32 and frames.shape == (1, 16, 256, 256, 3)
        assert frames.min() >= 0 and frames.max() <= 255 and frames.std() > 0
        outs.append(frames)
    assert np.array_equal(outs[0], outs[1])
