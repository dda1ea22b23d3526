"""Knob DEFER on the CPU: the window of deferred Wav2Lip passes and the prefetch-slot choice (csrc/defer_window.h, HIP-free) are
driven with fake events by a stand-alone program (tests/native/defer_window_main.cpp) built with AddressSanitizer and
UndefinedBehaviorSanitizer, once per host compiler.  Sequences: steady walk, jump, release while pending, error while pending,
drain, destroy with a pass pending.  The sanitizers are in the stand-alone program only, never in anything Python loads."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "native", "defer_window_main.cpp")
COMPILERS = ["g++", "/opt/rocm/llvm/bin/clang++"]


@pytest.mark.parametrize("cxx", COMPILERS)
def test_defer_window_sequences_under_sanitizers(cxx, tmp_path):
    exe = shutil.which(cxx)
    assert exe, f"{cxx} is not on this machine"
    out = tmp_path / "defer_window"
    b = subprocess.run([exe, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-pthread", SRC, "-o", str(out)],
                       capture_output=True, text=True, timeout=300)
    assert b.returncode == 0, b.stderr
    r = subprocess.run([str(out)], capture_output=True, text=True, timeout=60)
    print(r.stdout)
    assert r.returncode == 0, r.stdout + r.stderr
    for name in ("steady walk", "slot rotation", "jump", "release while pending", "error while pending", "destroy with a pass pending"):
        assert f"{name}: ok" in r.stdout, name
    assert r.stdout.rstrip().endswith("all ok")


def test_solo_walk_captures_within_the_benchmarks_untimed_calls():
    """The lone session's slot walk as the library computes it (ltk_debug_solo_walk, the same header): synchronous calls rotate over
    two slots, deferred calls over three, and every launch variant of the deferred walk has been run eagerly and captured by the
    eighth call - inside bench.py's 8 priming + 5 warm-up calls, so no capture falls into its timed region."""
    import ctypes as C
    from livetalking_amd import _lib
    lib = _lib.load()
    used = C.c_int(0)
    assert lib.ltk_debug_solo_walk(0, 40, -1, C.byref(used)) == 5 and used.value == 2
    last = lib.ltk_debug_solo_walk(1, 40, -1, C.byref(used))
    assert used.value == 3
    assert last + 1 <= 13, last
    assert lib.ltk_debug_solo_walk(2, 40, -1, C.byref(used)) == -1
