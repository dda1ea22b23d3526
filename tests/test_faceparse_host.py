"""CPU: the face parser's own ops (include/ltk.h ltk_parse_stem_f16 ... ltk_seg_argmax_f16; tests/faceparse_cases.py).

  * the ABI declares, binds and exports the five hooks, and each refuses a call without an engine;
  * the float32 rounding model of every op sits inside half its bound, at every shape the GPU suite runs (the 512 x 512 stem aside);
  * a simulated device - the model with one planted fault - is caught by the gates the GPU suite applies: zero-byte padding of the
    stem (normalisation behind the padding is the same tensor), a BGR / RGB swap, a max pool padded with 0 on negative input, a global
    average divided by a padded pixel count, the FFM gate without its + 1, and in the head align_corners=False, a last-index tie rule
    and an argmax over the 32 layout channels;
  * the whole network as tests/faceparse_ref.py restates it (41 named launches) equals what the reference's own BiSeNet computed on the
    seeded weights (tests/golden/faceparse_golden.npz, scripts/gen_golden_faceparse.py), reads exactly the reference's keys minus the
    unused heads, and leaves few pixels inside the fp16 chain's margin on the chosen seed."""
from __future__ import annotations

import ctypes
import os
import re

import numpy as np
import pytest

import faceparse_cases as FP

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOOKS = ["ltk_parse_stem_f16", "ltk_maxpool3x3s2_f16", "ltk_global_avgpool_f16", "ltk_chan_gate_f16", "ltk_seg_argmax_f16"]


def test_abi_declares_binds_and_exports_the_hooks():
    from livetalking_amd import _lib
    lib = _lib.load()
    hdr = open(os.path.join(ROOT, "include", "ltk.h")).read()
    for name in HOOKS:
        assert re.search(r"\bint\s+" + name + r"\s*\(", hdr), f"{name} is not declared in include/ltk.h"
        assert name in _lib.SYMBOLS and getattr(lib, name) is not None


def test_hooks_refuse_a_call_without_an_engine():
    from livetalking_amd import _lib
    lib = _lib.load()
    INVALID = -1          # include/ltk.h LTK_E_INVALID
    buf = ctypes.create_string_buffer(64 * 3 * 49 * 4)
    p = ctypes.cast(buf, ctypes.c_void_p)
    assert lib.ltk_parse_stem_f16(None, p, 1, 8, 8, p, None, None, p, None) == INVALID
    assert lib.ltk_maxpool3x3s2_f16(None, p, 1, 8, 8, 16, p, None) == INVALID
    assert lib.ltk_global_avgpool_f16(None, p, 1, 4, 16, p, None) == INVALID
    assert lib.ltk_chan_gate_f16(None, p, 1, 4, 16, p, None, None, 0, p, None) == INVALID
    assert lib.ltk_seg_argmax_f16(None, p, 1, 2, 2, p) == INVALID
    assert b"bad arguments" in lib.ltk_last_error()


# ------------------------------------------------------------------------------------------ stem
@pytest.mark.parametrize("shape", FP.STEM_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_stem_model_inside_half_the_bound(shape):
    c = FP.Stem(*shape)
    ref, tol = c.ref_tol()
    w = FP.model_inside(ref, c.model(), tol)
    fig = FP.check(c.model(), ref, c.model(), tol)
    print(f"stem {shape}: model at {w:.3f} of the bound, rel_l2 {fig['rel_mod']:.3e}")
    assert ref.shape == (shape[0], 64, shape[1] // 2, shape[2] // 2) and (ref > 0).mean() > 0.2


@pytest.mark.parametrize("fault", ["zero_byte_pad", "bgr"])
@pytest.mark.parametrize("shape", [FP.STEM_SHAPES[0], FP.STEM_SHAPES[2]], ids=lambda s: "x".join(map(str, s)))
def test_stem_planted_faults_are_caught(shape, fault):
    c = FP.Stem(*shape)
    ref, tol = c.ref_tol()
    bad = c.model(fault)
    with pytest.raises(AssertionError):
        FP.check(bad, ref, c.model(), tol)
    if fault != "bgr":            # a padding fault shows within three output pixels of the border and nowhere else
        inner = (slice(None), slice(None), slice(2, -2), slice(2, -2))
        if ref[inner].size:
            assert np.array_equal(bad[inner], c.model()[inner])


# ------------------------------------------------------------------------------------------ max pool
@pytest.mark.parametrize("shape", FP.POOL_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_maxpool_reference_and_zero_padding_fault(shape):
    x = FP.pool_input(*shape)
    ref = FP.pool_ref(x)
    N, C, H, W = shape
    assert ref.shape == (N, C, (H - 1) // 2 + 1, (W - 1) // 2 + 1)
    assert np.array_equal(ref.astype(np.float16).astype(np.float64), ref)       # a maximum of fp16 values: exact
    bad = FP.pool_ref(x, "zero_pad")
    assert not np.array_equal(bad[0], ref[0]) and (bad[0, :, 0] == 0).all()      # image 0 is negative: the padding wins the border
    assert np.array_equal(bad[:, :, 1:-1, 1:-1], ref[:, :, 1:-1, 1:-1])      # and nothing else


# ------------------------------------------------------------------------------------------ global average pool
@pytest.mark.parametrize("shape", FP.GAP_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_gap_model_inside_half_the_bound(shape):
    x = FP.gap_input(*shape)
    ref, tol = FP.gap_ref_tol(x)
    mod = FP.gap_model(x)
    w = FP.model_inside(ref, mod, tol)
    print(f"gap {shape}: model at {w:.3f} of the bound")
    # the tree does not depend on the images beside it: image 0 alone gives the same bytes
    assert np.array_equal(FP.gap_model(x[:1]), mod[:1])


@pytest.mark.parametrize("P", [4, 9])
def test_gap_padded_divisor_is_caught(P):
    x = FP.gap_input(1, 128, P)
    ref, tol = FP.gap_ref_tol(x)
    with pytest.raises(AssertionError):
        FP.check(FP.gap_model(x, "padded_p"), ref, FP.gap_model(x), tol)


def test_gap_padded_divisor_is_invisible_at_a_multiple_of_128():
    """Why P = 4 and 9 are among the GPU shapes: at P = 256 and 4096 a divisor rounded up to the pass width is the right one."""
    x = FP.gap_input(1, 128, 4096)
    assert np.array_equal(FP.gap_model(x, "padded_p"), FP.gap_model(x))


# ------------------------------------------------------------------------------------------ channel gate
@pytest.mark.parametrize("form", list(FP.GATE_FORMS))
def test_gate_model_inside_half_the_bound(form):
    c = FP.Gate(form)
    ref, tol = c.ref_tol()
    w = FP.model_inside(ref, c.model(), tol)
    print(f"gate {form}: model at {w:.3f} of the bound")


def test_gate_without_plus_one_is_caught():
    c = FP.Gate("ffm")
    ref, tol = c.ref_tol()
    with pytest.raises(AssertionError):
        FP.check(c.model("no_plus1"), ref, c.model(), tol)


# ------------------------------------------------------------------------------------------ segmentation head
@pytest.mark.parametrize("shape", FP.SEG_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_seg_model_agrees_outside_the_margin(shape):
    x = FP.seg_input(*shape)
    fig = FP.seg_check(FP.seg_model(x), x)
    print(f"seg {shape}: {fig['excluded']:.4%} excluded, {fig['differ']} labels differ inside the margin")
    ref, _ = FP.seg_ref(x)
    assert len(np.unique(ref)) >= 4                                   # several classes win: the comparison says something


@pytest.mark.parametrize("fault", ["half_pixel", "all32"])
@pytest.mark.parametrize("shape", FP.SEG_SHAPES[:2], ids=lambda s: "x".join(map(str, s)))
def test_seg_planted_faults_are_caught(shape, fault):
    x = FP.seg_input(*shape)
    with pytest.raises(AssertionError):
        FP.seg_check(FP.seg_model(x, fault), x)


def test_seg_tie_rule():
    x = FP.seg_input(2, 8, 8, ties=True)
    assert (FP.seg_model(x) == 3).all()
    assert (FP.seg_model(x, "last_tie") == 12).all()


# ------------------------------------------------------------------------------------------ the whole network: restatement and seeded weights
def test_seeded_state_dict_has_the_reference_key_set():
    """BiSeNet(n_classes=19).state_dict(): 191 keys, 13.3 M parameters; without the two unused heads and the BatchNorm counters, what the
    network's main output reads."""
    import synth_inputs as synth
    shapes = synth.faceparse_state_dict(shapes_only=True)
    assert len(shapes) == 191
    assert sum(int(np.prod(s)) for k, s in shapes.items() if not k.endswith("num_batches_tracked")) == 13313088
    assert shapes["cp.resnet.conv1.weight"] == (64, 3, 7, 7) and shapes["conv_out.conv_out.weight"] == (19, 256, 1, 1)
    assert shapes["cp.resnet.layer2.0.downsample.0.weight"] == (128, 64, 1, 1) and "cp.resnet.layer1.0.downsample.0.weight" not in shapes
    assert shapes["ffm.conv1.weight"] == (64, 256, 1, 1) and shapes["conv_out32.conv_out.weight"] == (19, 64, 1, 1)


def test_restatement_walk_and_end_to_end_margin():
    """The op walk of the restatement (the launch list a program over these kernels has to follow), and the margin figure of the seeded net:
    the share of the pixels inside tau = 2 max |mod - ref| (the unforced fp16-rounded chain against float64), and several
    classes winning."""
    import faceparse_ref as R
    import synth_inputs as synth
    names = R.op_names()
    assert len(names) == 41 and names[0] == ("cp.resnet.conv1", 10) and names[1] == ("cp.resnet.maxpool", 11) and names[-1] == ("labels", 14)
    assert [n for n, t in names if t == 12] == ["cp.avg", "cp.arm32.avg", "cp.arm16.avg", "ffm.avg"]
    assert [n for n, t in names if t == 13] == ["cp.feat32_sum", "cp.feat16_sum", "ffm"]
    assert sum(t == 0 for _, t in names) == 31 and len({n for n, _ in names}) == 41
    sd = synth.faceparse_state_dict(83)
    rgb = np.stack([synth.faceparse_image(64, seed=i) for i in range(3)])
    labels, decided, tau = R.end_to_end(sd, rgb)
    excluded = 1.0 - float(decided.mean())
    big = [int(c) for c in np.unique(labels) if (labels == c).mean() >= 0.02]
    print(f"seed 83, 64 x 64, 3 images: tau {tau:.4f}, {excluded:.3%} inside tau, classes with >= 2 % of the pixels {big}")
    assert excluded <= 0.05 and len(big) >= 4          # 3.3 % here with the balanced head (tau moves with the CPU's fp32 summation order)


# ------------------------------------------------------------------------------------------ the restatement against the reference's own BiSeNet
GOLDEN = os.path.join(ROOT, "tests", "golden", "faceparse_golden.npz")
MANIFEST = os.path.join(ROOT, "tests", "golden", "faceparse_key_manifest.json")
IGNORED = ("conv_out16.", "conv_out32.")          # the heads net(img)[0] does not use; and every num_batches_tracked


def test_key_manifest_of_the_reference_equals_the_seeded_state_dict():
    """tests/golden/faceparse_key_manifest.json: BiSeNet.state_dict() of the reference (scripts/gen_golden_faceparse.py loaded the seeded
    state dict into it strictly).  What net(img)[0] needs = the manifest minus the ignored keys = what tests/faceparse_ref.py reads."""
    import json
    import synth_inputs as synth
    manifest = {k: tuple(v) for k, v in json.load(open(MANIFEST)).items()}
    assert manifest == synth.faceparse_state_dict(shapes_only=True)
    used = {k for k in manifest if not k.startswith(IGNORED) and not k.endswith("num_batches_tracked")}

    class Spy(dict):
        def __init__(self, d):
            super().__init__(d)
            self.seen = set()

        def __getitem__(self, k):
            self.seen.add(k)
            return super().__getitem__(k)

    import faceparse_ref as R
    spy = Spy(synth.faceparse_state_dict(83))
    R.Chain(spy, "ref").run(np.stack([synth.faceparse_image(64, seed=0)]))
    assert spy.seen == used


@pytest.mark.parametrize("size", [64, 96, 512])
def test_restatement_equals_the_reference_golden(size):
    """The float64 chain of tests/faceparse_ref.py against what the reference's own BiSeNet computed in float64 on the same seeded weights
    and images: logits within float32 noise of their scale, labels (bilinear x8, argmax) equal."""
    import faceparse_ref as R
    import synth_inputs as synth
    g = np.load(GOLDEN)
    seed = int(g["seed"])
    n = int(g["counts"][list(g["sizes"]).index(size)])
    sd = synth.faceparse_state_dict(seed)
    rgb = np.stack([synth.faceparse_image(size, seed=i) for i in range(n)])
    logits = R.Chain(sd, "ref").run(rgb)
    gold = g[f"logits_{size}"].astype(np.float64)
    err = float(np.abs(logits.numpy() - gold).max())
    scale = float(np.abs(gold).max())
    print(f"size {size}: max |restatement - reference| {err:.3e} at max |logit| {scale:.2f}")
    # the file keeps float64 logits (float32 at 512 x 512: one rounding of 2^-24 relative, and a different summation order in float64)
    assert err <= (1e-9 if g[f"logits_{size}"].dtype == np.float64 else 2.0 ** -22 * scale)
    labels = R.upsampled(logits).argmax(1).numpy().astype(np.uint8)
    assert np.array_equal(labels, g[f"labels_{size}"])
    reference = os.environ.get("LTK_REFERENCE", "/root/reference")
    if size == 64 and os.path.isdir(os.path.join(reference, "avatars", "musetalk", "utils", "face_parsing")):      # re-derive it from the checkout
        import sys
        sys.path.insert(0, os.path.join(ROOT, "scripts"))
        import gen_golden_faceparse as G
        ref_logits, ref_labels, _ = G.reference_outputs(reference, sd, rgb)
        assert np.array_equal(ref_logits, gold) and np.array_equal(ref_labels, g["labels_64"])


# ------------------------------------------------------------------------------------------ the launch list (csrc/faceparse.hip fp_program)
@pytest.mark.parametrize("size", [64, 96, 512])
def test_program_listing_equals_the_op_walk_and_the_planner_takes_every_conv(size):
    """ltk_debug_face_parse_program against the restatement's walk - names, types, every output map, a conv's channels, kernel, stride,
    ReLU, upsample read and residual - and every conv of it against the host-only conv planner at 1 and 4 images (the stem, which the
    planner refuses, is parse_stem_kernel's)."""
    import faceparse_ref as R
    import synth_inputs as synth
    from livetalking_amd.engine import Engine
    from livetalking_amd._lib import LtkError
    prog = Engine.face_parse_program(size)
    assert [(o["name"], o["type"]) for o in prog] == R.op_names() and len(prog) == 41
    chain = R.Chain(synth.faceparse_state_dict(83), "ref")
    chain.run(np.stack([synth.faceparse_image(size, seed=0)]))
    assert len(chain.ops) == len(prog)
    for o, w in zip(prog, chain.ops):
        assert (o["name"], o["type"]) == (w["name"], w["type"])
        if o["type"] == 14:
            assert (o["Ho"], o["Wo"]) == w["shape"][1:] == (size, size) and (o["H"], o["W"]) == (size // 8, size // 8)
            continue
        assert (o["cout"], o["Ho"], o["Wo"]) == w["shape"][1:], o["name"]
        if o["type"] == 0:
            want = (w["cin"], w["k"], w["stride"], w["k"] // 2, w["relu"], w["ups"], w["has_res"], w["hw"])
            assert (o["cin"], o["k"], o["stride"], o["pad"], o["relu"], o["ups"], o["has_res"], (o["H"], o["W"])) == want, o["name"]
            for n in (1, 4):
                rep = Engine.conv_plan(n, o["H"], o["W"], o["cin"], (o["cout"] + 15) // 16 * 16, o["k"], o["stride"], o["pad"],
                                       has_res=bool(o["has_res"]), ups=o["ups"])
                assert rep["kernel"], o["name"]
        elif o["type"] == 13:
            assert (o["has_res"], o["plus1"]) == (w["has_res"], w["plus1"])
    stem = prog[0]
    assert (stem["cin"], stem["cout"], stem["k"], stem["stride"], stem["pad"], stem["H"], stem["Ho"]) == (3, 64, 7, 2, 3, size, size // 2)
    with pytest.raises(LtkError, match="Cout<=32"):
        Engine.conv_plan(1, size, size, 3, 64, 7, 2, 3)


def test_program_listing_refusals():
    from livetalking_amd import _lib
    lib = _lib.load()
    ops = (_lib.FpOpInfo * 64)()
    n = ctypes.c_int()
    for size in (48, 80, 32, 544):
        assert lib.ltk_debug_face_parse_program(size, ops, 64, ctypes.byref(n)) == -1 and b"multiple of 32" in lib.ltk_last_error()
    assert lib.ltk_debug_face_parse_program(64, ops, 40, ctypes.byref(n)) == -1 and b"41 ops" in lib.ltk_last_error()
    assert lib.ltk_debug_face_parse_program(64, None, 64, ctypes.byref(n)) == -1
    assert lib.ltk_debug_face_parse_program(64, ops, 64, ctypes.byref(n)) == 0 and n.value == 41
