"""CPU: the face parser's binding table (csrc/faceparse.h fp_plan through ltk_debug_face_parse_plan / Engine.face_parse_plan) - where
every launch of the 41-launch list reads and writes - which is what the device program of ltk_face_parse_load is built from.

  * one entry per launch of Engine.face_parse_program(size), same names, same order; every view inside its buffer, its channels and
    map those of the op; every buffer's byte size what its views say; no launch writes where it reads;
  * the wiring itself: the float32 rounding chain of tests/faceparse_ref.py, Chain(sd, "mod"), run launch by launch through numpy
    buffers that are addressed by the plan's views and by nothing else, ends in bit-for-bit the logits of a plain Chain(sd, "mod").run -
    residuals, the broadcast of cp.conv_avg, the two halves of the concat buffer;
  * five planted wiring faults, each caught by that comparison (a view whose shape the op cannot take counts as caught too: the
    comparison never gets its logits);
  * the op-by-op check the GPU suite applies (tests/face_parse_cases.py check_ops) on a simulated device that computes the rounding
    model: every launch passes inside half its bound, and a dropped residual is named;
  * the refusals."""
from __future__ import annotations

import copy

import numpy as np
import pytest

import faceparse_ref as R
import synth_inputs as synth
from face_parse_cases import SEED, replay_through_views, up16


def _plan(size, max_images):
    from livetalking_amd.engine import Engine
    return Engine.face_parse_plan(size, max_images), Engine.face_parse_program(size)


# ------------------------------------------------------------------------------------------ the table against the launch list
@pytest.mark.parametrize("size,max_images", [(64, 1), (96, 3), (512, 4)])
def test_one_entry_per_launch_and_every_view_fits(size, max_images):
    plan, prog = _plan(size, max_images)
    ops, nbytes = plan["ops"], plan["buf_bytes"]
    assert [o["name"] for o in ops] == [p["name"] for p in prog] and len(ops) == 41
    img, lab = plan["image_buf"], plan["label_buf"]
    assert img != lab and nbytes[img] == max_images * size * size * 3 and nbytes[lab] == max_images * size * size
    geom = {}                                    # buffer -> (ld, H, W): every view of a buffer says the same

    def fits(v, what):
        assert 0 <= v["buf"] < len(nbytes) and v["C"] > 0 and v["coff"] >= 0 and v["coff"] + v["C"] <= v["ld"], what
        assert geom.setdefault(v["buf"], (v["ld"], v["H"], v["W"])) == (v["ld"], v["H"], v["W"]), what
        unit = 1 if v["buf"] in (img, lab) else 2
        assert v["ld"] * v["H"] * v["W"] * unit * max_images == nbytes[v["buf"]], what
        if unit == 2:
            assert v["C"] % 16 == 0 and v["ld"] % 16 == 0 and v["coff"] % 16 == 0, what

    for o, p in zip(ops, prog):
        n, t = p["name"], p["type"]
        for k in "xyrab":
            if o[k] is not None:
                fits(o[k], (n, k))
        x, y = o["x"], o["y"]
        if t == 14:
            assert (y["buf"], y["C"], y["H"], y["W"]) == (lab, 1, size, size) and (x["C"], x["ld"], x["H"], x["W"]) == (32, 32, p["H"], p["W"]), n
        else:
            assert (y["C"], y["H"], y["W"]) == (up16(p["cout"]), p["Ho"], p["Wo"]), n
        if t == 10:
            assert (x["buf"], x["C"], x["H"], x["W"]) == (img, 3, size, size), n
        elif t != 14:
            f = 2 if p["ups"] else 1             # a conv behind a nearest x2 upsample reads the stored, half-size map
            assert (x["C"], x["H"] * f, x["W"] * f) == (up16(p["cin"]), p["H"], p["W"]), n
        assert (o["r"] is not None) == bool(p["has_res"]), n
        if o["r"] is not None:
            assert (o["r"]["C"], o["r"]["H"], o["r"]["W"]) == (y["C"], y["H"], y["W"]), n
        assert (o["a"] is not None) == (t == 13) and (o["b"] is not None) == (n == "cp.feat32_sum"), n
        for k in "ab":                           # what the gate kernel reads as dense [N][C/16][1][16] tensors
            if o[k] is not None:
                assert (o[k]["C"], o[k]["ld"], o[k]["coff"], o[k]["H"], o[k]["W"]) == (x["C"], x["C"], 0, 1, 1), (n, k)
        for k in "xrab":                         # no launch writes the channels it reads
            v = o[k]
            if v is not None and v["buf"] == y["buf"]:
                assert v["coff"] + v["C"] <= y["coff"] or y["coff"] + y["C"] <= v["coff"], (n, k)
    # the concat of ffm.convblk is two channel views of ONE 256-channel buffer, no copy
    by = {o["name"]: o for o in ops}
    cat = by["ffm.convblk"]["x"]
    f8, cp8 = by["cp.resnet.layer2.1.conv2"]["y"], by["cp.conv_head16"]["y"]
    assert (cat["ld"], cat["coff"], cat["C"]) == (256, 0, 256)
    assert (f8["buf"], f8["coff"], f8["C"]) == (cat["buf"], 0, 128) and (cp8["buf"], cp8["coff"], cp8["C"]) == (cat["buf"], 128, 128)
    assert by["labels"]["x"] == by["conv_out.conv_out"]["y"]


# ------------------------------------------------------------------------------------------ the wiring: Chain("mod") through the views
@pytest.fixture(scope="module")
def plain():
    """size -> (rgb, the plain chain's logits): computed once, left unchanged"""
    sd = synth.faceparse_state_dict(SEED)
    out = {}
    for size in (64, 96):
        rgb = np.stack([synth.faceparse_image(size, seed=i) for i in range(2)])
        out[size] = (rgb, R.Chain(sd, "mod").run(rgb).numpy())
    return sd, out


def wired_right(plan, prog, sd, rgb, want) -> bool:
    try:
        got = replay_through_views(plan, prog, sd, rgb)
    except (AssertionError, RuntimeError, ValueError) as e:             # an operand the op cannot take: no logits to compare
        print(f"  replay stopped: {str(e).splitlines()[0][:120]}")
        return False
    return got.shape == want.shape and np.array_equal(got, want)


@pytest.mark.parametrize("size", [64, 96])
def test_chain_through_the_views_equals_the_plain_chain(plain, size):
    sd, runs = plain
    rgb, want = runs[size]
    plan, prog = _plan(size, 2)
    got = replay_through_views(plan, prog, sd, rgb)
    assert got.shape == want.shape == (2, 19, size // 8, size // 8)
    assert np.array_equal(got, want), f"max |through the views - plain| {np.abs(got - want).max():.3e}"


def _swap_concat_halves(by):
    by["cp.resnet.layer2.1.conv2"]["y"], by["cp.conv_head16"]["y"] = by["cp.conv_head16"]["y"], by["cp.resnet.layer2.1.conv2"]["y"]


def _residual_is_block_input(by):
    by["cp.resnet.layer2.0.conv2"]["r"] = copy.deepcopy(by["cp.resnet.layer2.0.conv1"]["x"])


def _feat16_adds_conv_avg(by):
    by["cp.feat16_sum"]["r"] = copy.deepcopy(by["cp.conv_avg"]["y"])


def _ffm_gate_is_conv1(by):
    by["ffm"]["a"] = copy.deepcopy(by["ffm.conv1"]["y"])


def _labels_read_16_channels(by):
    by["labels"]["x"]["C"] = 16


FAULTS = {"concat_halves_swapped": _swap_concat_halves, "downsample_residual_is_block_input": _residual_is_block_input,
          "feat16_sum_adds_conv_avg": _feat16_adds_conv_avg, "ffm_gate_is_conv1": _ffm_gate_is_conv1,
          "labels_read_16_channels": _labels_read_16_channels}


@pytest.mark.parametrize("fault", list(FAULTS))
def test_planted_wiring_faults_are_caught(plain, fault):
    sd, runs = plain
    rgb, want = runs[64]
    plan, prog = _plan(64, 2)
    assert wired_right(plan, prog, sd, rgb, want)
    bad = copy.deepcopy(plan)
    FAULTS[fault]({o["name"]: o for o in bad["ops"]})
    assert bad != plan and not wired_right(bad, prog, sd, rgb, want)


# ------------------------------------------------------------------------------------------ the GPU suite's op-by-op check on a simulated device
class _Sim(R.Chain):
    """Chain(sd, "mod") that keeps every launch's output: a device that computes exactly the rounding model."""

    def __init__(self, sd):
        super().__init__(sd, "mod")
        self.outs = {}

    def _done(self, name, kind, ref, mod, **info):
        out = super()._done(name, kind, ref, mod, **info)
        self.outs[name] = out.numpy().astype(np.float32)
        return out


def test_op_by_op_check_takes_the_rounding_model_and_catches_a_dropped_residual(plain):
    """check_ops (tests/face_parse_cases.py) as tests/test_face_parse_gpu.py applies it, on the model as the device: every launch is
    checked and passes; with layer1.0.conv2's residual left out of the simulated device's output, that launch is named."""
    from face_parse_cases import check_ops
    sd, runs = plain
    rgb, _ = runs[64]
    plan, prog = _plan(64, 2)
    sim = _Sim(sd)
    labels = R.upsampled(sim.run(rgb)).argmax(1).numpy().astype(np.uint8)
    figs = check_ops(lambda name, shape: sim.outs[name], plan, prog, sd, rgb, labels)
    assert set(figs) == {p["name"] for p in prog} and len(figs) == 41
    assert max(f.get("worst", 0.0) for f in figs.values()) <= 0.5          # the model sits inside half of every bound
    bad = dict(sim.outs)
    n = "cp.resnet.layer1.0.conv2"
    bad[n] = np.maximum(bad[n] - sim.outs["cp.resnet.maxpool"], 0).astype(np.float16).astype(np.float32)
    with pytest.raises(AssertionError, match=n.replace(".", r"\.")):
        check_ops(lambda name, shape: bad[name], plan, prog, sd, rgb, labels)


# ------------------------------------------------------------------------------------------ refusals
def test_refusals():
    from livetalking_amd._lib import LtkError
    from livetalking_amd.engine import Engine
    for size, n, word in ((0, 1, "multiple of 32"), (48, 1, "multiple of 32"), (544, 1, "multiple of 32"), (64, 0, "max_images"), (64, 9, "max_images")):
        with pytest.raises(LtkError) as ei:
            Engine.face_parse_plan(size, n)
        assert ei.value.code == -1 and word in str(ei.value), (size, n, str(ei.value))
    assert len(Engine.face_parse_plan(64, 8)["ops"]) == 41
