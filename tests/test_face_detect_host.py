"""CPU: the S3FD face detector without a device.  The float64 restatement (tests/s3fd_ref.py) equals what the reference's own s3fd,
batch_detect, nms and get_smoothened_boxes gave on seeded weights (tests/golden/s3fd_golden.npz, scripts/gen_golden_s3fd.py), and is
re-derived from the checkout where that is present; the launch list (csrc/facedet.h) equals the restatement's op walk and every
library conv of it is accepted by the conv planner; the binding table is replayed through the fp16 rounding chain bit for bit; a
simulated device with planted wiring faults is caught by the gates the GPU suite applies; livetalking_amd/face_detect.py - nms, the
batch quirk, the smoothing, the coords.pkl order - equals the stored reference outputs; the rounding models stay inside half of every
bound they are used for."""
from __future__ import annotations

import ctypes
import json
import os
import pickle
import re

import numpy as np
import pytest
import torch

import s3fd_cases as FD
import s3fd_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOOKS = ("ltk_s3fd_stem_f16", "ltk_maxpool2x2s2_f16", "ltk_l2norm_f16", "ltk_s3fd_detect_f16", "ltk_debug_face_detect_program",
         "ltk_debug_face_detect_plan", "ltk_face_detect_load", "ltk_face_detect", "ltk_face_detect_debug_get", "ltk_debug_face_detect_time")
SMALL = ((64, 64), (72, 104))


@pytest.fixture(scope="module")
def gold():
    return np.load(os.path.join(ROOT, "tests", "golden", "s3fd_golden.npz"))


@pytest.fixture(scope="module")
def sd():
    return FD.state_dict()


@pytest.fixture(scope="module")
def walks(sd):
    """per small case: frames, the float64 walk, the fp16 model walk, the launch list - computed once"""
    from livetalking_amd.engine import Engine
    out = {}
    sd32 = {k: v.float() for k, v in sd.items()}
    for hw in SMALL:
        frames = FD.frames(hw)
        prog = Engine.face_detect_program(*hw)
        out[hw] = dict(frames=frames, prog=prog, ref=R.walk(sd, R.preprocess(frames)), mod=FD.model_walk(sd32, frames, prog))
    return out


def _key(hw):
    return f"{hw[0]}x{hw[1]}"


# ------------------------------------------------------------------------------------------ ABI
def test_abi_declares_binds_and_exports_the_entries():
    from livetalking_amd import _lib
    lib = _lib.load()
    hdr = open(os.path.join(ROOT, "include", "ltk.h")).read()
    for name in HOOKS:
        assert re.search(r"\bint\s+" + name + r"\s*\(", hdr), f"{name} is not declared in include/ltk.h"
        assert name in _lib.SYMBOLS and getattr(lib, name) is not None
    assert ctypes.sizeof(_lib.FdOpInfo) == 64 + 13 * 4 and ctypes.sizeof(_lib.FdBind) == 64 + 2 * 24
    assert _lib.HEALTH_PROGRAMS["facedet"] == 7 and re.search(r"LTK_HEALTH_FACEDET\s*=\s*7", hdr)
    assert lib.ltk_face_detect_load(None, None, 0, 1) == -1 and lib.ltk_face_detect(None, None, 0, 64, 64, 0.05, None, 1, None) == -1


# ------------------------------------------------------------------------------------------ the restatement against the reference
def test_restatement_equals_the_stored_reference_outputs(gold, sd, walks):
    man = json.load(open(os.path.join(ROOT, "tests", "golden", "s3fd_key_manifest.json")))
    assert {k: list(v.shape) for k, v in sd.items()} == man and int(gold["seed"]) == FD.SEED
    for hw in SMALL:
        ol = R.olist_from_heads([walks[hw]["ref"][R.head_prefix(i)] for i in range(6)])
        for i in range(12):
            ref = gold[f"heads_{_key(hw)}_{i}"]
            assert ol[i].shape == ref.shape and float((ol[i] - torch.from_numpy(ref)).abs().max()) <= 1e-11 * max(1.0, float(np.abs(ref).max())), (hw, i)
        # batch_detect itself, chunk by chunk (a pair and a short tail), rows in its own order
        for c, sl in enumerate((slice(0, 2), slice(2, 3))):
            bd = R.batch_detect([o[sl] for o in ol])
            ref = gold[f"bd_{_key(hw)}_{c}"]
            assert bd.shape == ref.shape and np.abs(bd - ref).max() <= 1e-9 * max(1.0, np.abs(ref).max()), (hw, c)


def test_180x320_restatement_against_the_stored_float32_heads(gold, sd):
    hw = (180, 320)
    ol = R.net(sd, R.preprocess(FD.frames(hw)))
    for i in range(12):
        ref = gold[f"heads_180x320_{i}"]
        assert ref.dtype == np.float32 and np.abs(ol[i].numpy() - ref).max() <= 2.0 ** -23 * max(1.0, np.abs(ref).max()), i


def test_golden_file_is_rederived_from_the_checkout():
    ref = os.environ.get("LTK_REFERENCE", "/root/reference")
    if not os.path.exists(os.path.join(ref, "avatars", "wav2lip", "face_detection", "detection", "sfd", "net_s3fd.py")):
        pytest.skip("no reference checkout")
    import importlib.util
    import synth_inputs as synth
    spec = importlib.util.spec_from_file_location("gen_golden_s3fd", os.path.join(ROOT, "scripts", "gen_golden_s3fd.py"))
    gen = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gen)
    net_s3fd, bbox, detect, ga = gen.load_reference(ref)
    net, manifest = gen.reference_net(net_s3fd, synth.s3fd_state_dict(FD.SEED))
    g = np.load(os.path.join(ROOT, "tests", "golden", "s3fd_golden.npz"))
    case = gen.reference_case(net, bbox, detect, FD.frames((64, 64)))
    for k, v in case.items():
        parts = k.split("_")
        stored = g[f"{parts[0]}_64x64" + (f"_{parts[1]}" if len(parts) > 1 else "")]
        assert stored.shape == v.shape and np.array_equal(stored, v), k
    ex = gen.smoothing_example(ga, case["boxes"], (64, 64))
    for k, v in ex.items():
        assert np.array_equal(g[k], v), k
    assert manifest == json.load(open(os.path.join(ROOT, "tests", "golden", "s3fd_key_manifest.json")))


# ------------------------------------------------------------------------------------------ the launch list and the plan
def test_launch_list_equals_the_op_walk(walks):
    from livetalking_amd.engine import Engine
    for hw in SMALL:
        prog, ref = walks[hw]["prog"], walks[hw]["ref"]
        assert len(prog) == 39 and [p["type"] for p in prog].count(0) == 24          # 18 trunk convs + 6 merged heads
        assert [p["name"] for p in prog if p["type"] != 23] == list(ref.keys())
        for p in prog:
            if p["type"] != 23:
                assert tuple(ref[p["name"]].shape[1:]) == (p["cout"], p["Ho"], p["Wo"]), p
        det = [p for p in prog if p["type"] == 23]
        assert [(p["level"], p["maxout"]) for p in det] == [(i, int(i == 0)) for i in range(6)]
        fc7 = next(p for p in prog if p["name"] == "fc7")
        assert (fc7["Ho"], fc7["Wo"]) == (hw[0] // 32 + 4, hw[1] // 32 + 4) and (det[3]["H"], det[3]["W"]) == (fc7["Ho"], fc7["Wo"])
    for bad in ((31, 64), (64, 20000)):
        with pytest.raises(Exception, match="32, 16384"):
            Engine.face_detect_program(*bad)


def test_every_library_conv_is_accepted_by_the_conv_planner():
    from livetalking_amd.engine import Engine
    seen = {}
    for hw, n in (((64, 64), 2), ((72, 104), 3), ((720, 1280), 4)):
        for p in Engine.face_detect_program(*hw):
            if p["type"] != 0:
                continue
            rep = Engine.conv_plan(n, p["H"], p["W"], p["cin"], p["cout"], k=p["k"], stride=p["stride"], pad=p["pad"])
            kernel = rep["kernel"] if isinstance(rep, dict) else rep.kernel
            kernel = kernel.decode() if isinstance(kernel, bytes) else kernel
            assert kernel, (hw, p["name"])
            seen.setdefault(p["name"], set()).add(kernel.split("<")[0])
    assert seen["fc6"] == {"conv_mfma_kernel"}                    # pad 3: the first-generation kernel; no conv3 instantiation was added
    print({k: sorted(v) for k, v in seen.items()})


def test_which_convs_leave_the_one_image_summation_order_to_the_fallback():
    """mt_graph.hip gives every conv of this program the split-K factor of a ONE-image launch and runs it image by image where the
    planner, at the run's image count, changes kernel family or refuses that factor.  On the host: no conv does at the sizes the GPU
    suite holds to byte identity with two images up to 180 x 320; conv7_1 (512 -> 128, 1x1: conv3 split 8 for one image, lin_fk_kernel
    from kLinFkMinRows rows on) is the only one that ever does, from 180 x 320 x 16 and 720 x 1280 x 2 on
    (tests/test_face_detect_gpu.py runs that case)."""
    from livetalking_amd.engine import Engine
    fam = lambda r: r["kernel"].split("<")[0]
    taken = {}
    for hw in ((64, 64), (72, 104), (180, 320), (360, 640), (720, 1280)):
        for nf in (2, 16):
            for p in Engine.face_detect_program(*hw):
                if p["type"] != 0:
                    continue
                a = dict(k=p["k"], stride=p["stride"], pad=p["pad"])
                r1 = Engine.conv_plan(1, p["H"], p["W"], p["cin"], p["cout"], **a)
                ks = max(1, r1["ksplit"])
                rn = Engine.conv_plan(nf, p["H"], p["W"], p["cin"], p["cout"], force_ksplit=ks, **a)
                if fam(rn) != fam(r1) or max(1, rn["ksplit"]) != ks:
                    taken.setdefault((hw, nf), []).append(p["name"])
    assert set(taken) == {((180, 320), 16), ((360, 640), 16), ((720, 1280), 2), ((720, 1280), 16)}
    assert all(v == ["conv7_1"] for v in taken.values())


def test_plan_sizes_and_refusals():
    from livetalking_amd.engine import Engine
    pl = Engine.face_detect_plan(720, 1280, 16)
    assert pl["total_bytes"] == sum(pl["buf_bytes"]) < 8 << 30 and pl["buf_bytes"][pl["image_buf"]] == 16 * 720 * 1280 * 3
    assert pl["buf_bytes"][-1] == 16 * (4096 * 24 + 256)              # the record buffer is the plan's last, and counted
    assert Engine.face_detect_plan(360, 640, 16)["total_bytes"] < pl["total_bytes"]
    with pytest.raises(Exception) as ex:
        Engine.face_detect_plan(1440, 2560, 16)
    assert re.search(r"needs \d+ bytes", str(ex.value)) and str(8 << 30) in str(ex.value)
    for n in (0, 17):
        with pytest.raises(Exception, match="max_images"):
            Engine.face_detect_plan(64, 64, n)


def test_binding_table_replays_the_rounding_chain_bit_for_bit(sd, walks):
    from livetalking_amd.engine import Engine
    sd32 = {k: v.float() for k, v in sd.items()}
    for hw in SMALL:
        w = walks[hw]
        heads = FD.replay_through_views(Engine.face_detect_plan(*hw, 2), w["prog"], sd32, w["frames"])
        for i in range(6):
            assert torch.equal(heads[i], w["mod"][R.head_prefix(i)]), (hw, i)
    # a plan whose trunk wrote ONE buffer in turn with itself would hand conv1_2 its own output: the replay notices
    plan = Engine.face_detect_plan(64, 64, 2)
    a, b = plan["ops"][0]["y"]["buf"], plan["ops"][1]["y"]["buf"]
    assert a != b
    for o in plan["ops"]:
        for v in (o["x"], o["y"]):
            if v is not None and v["buf"] == b:
                v["buf"] = a
    with pytest.raises(AssertionError, match="writes the buffer it reads"):
        FD.replay_through_views(plan, walks[(64, 64)]["prog"], sd32, walks[(64, 64)]["frames"])
    # ... and one whose conv3_3 (a tapped map: its norm reads it after the trunk has moved on) sat in a trunk buffer
    plan = Engine.face_detect_plan(64, 64, 2)
    tap = next(o for o in plan["ops"] if o["name"] == "conv3_3")["y"]["buf"]
    for o in plan["ops"]:
        for v in (o["x"], o["y"]):
            if v is not None and v["buf"] == tap:
                v["buf"] = a if next(q for q in plan["ops"] if q["name"] == "conv3_3")["x"]["buf"] != a else b
    with pytest.raises(AssertionError, match="writes the buffer it reads|shaped otherwise"):
        FD.replay_through_views(plan, walks[(64, 64)]["prog"], sd32, walks[(64, 64)]["frames"])


# ------------------------------------------------------------------------------------------ the gates catch planted faults
def test_simulated_device_passes_and_planted_faults_are_caught(sd, walks):
    from livetalking_amd.engine import Engine
    hw = (72, 104)
    prog, plan, frames = walks[hw]["prog"], Engine.face_detect_plan(*hw, 2), walks[hw]["frames"][:2]
    sim = FD.SimDevice(sd, frames, prog)
    figs = FD.check_ops(sim.fetch, plan, prog, sd, frames, sim.records)
    assert len(figs) == 39
    worst = max(f.get("worst_mod", 0.0) for f in figs.values())
    assert worst <= 0.5, f"a rounding model reaches {worst:.3f} of its bound"
    where = {"swapped": "detect", "no_maxout": "detect0", "stride": "detect", "fc6_pad1": "fc6", "ceil_pool": "pool", "not_reversed": "conv1_1"}
    for fault, op in where.items():
        bad = FD.SimDevice(sd, frames, prog, fault)
        with pytest.raises(AssertionError, match=op):
            FD.check_ops(bad.fetch, plan, prog, sd, frames, bad.records)


def test_kernel_models_stay_inside_half_of_their_bounds_and_faults_do_not():
    for shape in FD.STEM_SHAPES:
        c = FD.Stem(*shape)
        ref, tol = c.ref_tol()
        FD.model_inside(ref, c.model(), tol)
        if shape[1] > 1:
            for fault in ("not_reversed", "means_unreversed", "zero_byte_pad"):
                with pytest.raises(AssertionError):
                    FD.check(c.model(fault), ref, c.model(), tol)
    for shape in FD.NORM_SHAPES:
        x, w = FD.norm_input(*shape)
        ref, tol = FD.norm_ref_tol(x, w)
        FD.model_inside(ref, FD.norm_model(x, w), tol)
        bad = FD.norm_model(x, w, "f16_sum")
        with pytest.raises(AssertionError):
            FD.check(np.nan_to_num(bad, nan=0.0, posinf=65504.0), ref, FD.norm_model(x, w), tol)
    x = FD.pool_input(2, 32, 7, 9)
    assert FD.pool_ref(x).shape[2:] == (3, 4) and FD.pool_ref(x, ceil_mode=True).shape[2:] == (4, 5)
    for level, maxout in FD.DETECT_CASES:
        x = FD.detect_input(level, maxout)
        ref = FD.detect_ref(x, maxout, level, 0.05)
        fig = FD.detect_check(FD.detect_model(x, maxout, level, 0.05), ref)
        assert fig["worst_s"] <= 0.5 and fig["worst_b"] <= 0.5
        for fault in ("swapped", "stride") + (("no_maxout",) if maxout else ()):
            with pytest.raises(AssertionError):
                FD.detect_check(FD.detect_model(x, maxout, level, 0.05, fault), ref)
    x = FD.detect_input(2, False)
    x[:, 0:2, 4, 5] = 1.25
    with pytest.raises(AssertionError):                            # a score exactly at the threshold is not a candidate
        FD.detect_check(FD.detect_model(x, False, 2, 0.5, "ge"), FD.detect_ref(x, False, 2, 0.5))


def test_end_to_end_model_is_inside_the_gates_it_defines(sd, walks):
    for hw in SMALL:
        w = walks[hw]
        rh = [w["ref"][R.head_prefix(i)] for i in range(6)]
        mh = [w["mod"][R.head_prefix(i)] for i in range(6)]
        tau_s, tau_b = FD.taus(rh, mh)
        ref = R.candidates(R.olist_from_heads(rh), FD.THRESH)
        mod = R.candidates(R.olist_from_heads([m.double() for m in mh]), FD.THRESH)
        fig = FD.check_candidates(mod, ref, FD.dense_scores(rh), tau_s, tau_b)
        # a record where float64 scores nothing is refused even when its own score sits just above the threshold
        # (level 0, row 0, column 0 = key 0, in front of every list; no case's image is a candidate there)
        assert all(0 not in k for k, _ in mod)
        ghost = [(np.concatenate([[0], k]).astype(np.uint32), np.concatenate([[[0, 0, 1, 1, FD.THRESH + 0.5 * tau_s]], r])) for k, r in mod]
        flat = [s.clone() for s in FD.dense_scores(rh)]
        flat[0][:, 0, 0] = 0.0
        with pytest.raises(AssertionError, match="below thresh - tau_s"):
            FD.check_candidates(ghost, ref, flat, tau_s, tau_b)
        assert fig["worst_s"] <= 0.5 * tau_s + 1e-12 and fig["worst_b"] <= 0.5 * tau_b + 1e-9
        for keys, rows in ref:
            assert len(keys) >= 40 and len(np.unique(keys >> 28)) >= 3
            assert (np.abs(rows[:, 4] - FD.THRESH) <= tau_s).sum() <= FD.NEAR_CAP * len(keys)


# ------------------------------------------------------------------------------------------ the host side against the reference
def test_nms_and_the_batch_quirk_against_the_stored_reference_outputs(gold, sd, walks):
    from livetalking_amd import face_detect as H
    kept_counts = []
    for hw in SMALL:
        eng = FD.SimEngine(sd)
        det = H.FaceDetector(eng)
        frames = walks[hw]["frames"]
        own = det.candidates(frames)
        for c, sl in enumerate((slice(0, 2), slice(2, 3))):
            bd = gold[f"bd_{_key(hw)}_{c}"]                                 # (K, B, 5): every image's row at every position ANY image lists
            for j, n in enumerate(range(sl.start, min(sl.stop, 3))):
                theirs = bd[:, j, :]
                assert len(theirs) >= len(own[n])
                if bd.shape[1] > 1:
                    assert (theirs[:, 4] <= H.DET_THRESH).any() or len(theirs) > len(own[n])    # the quirk is there: extra rows
                kept = gold[f"kept_{_key(hw)}_{n}"]
                # the reference's own nms on its own list, restated; then the image's OWN candidates give the same kept rows
                assert np.array_equal(np.asarray(H.keep_faces(theirs)).reshape(-1, 5), kept)
                mine = np.asarray(H.keep_faces(own[n])).reshape(-1, 5)
                assert mine.shape == kept.shape and np.abs(mine - kept).max(initial=0.0) <= 1e-4 * max(1.0, np.abs(kept).max(initial=0.0))
                kept_counts.append(len(kept))
        boxes = det.get_detections_for_batch(frames)
        stored = gold[f"boxes_{_key(hw)}"]
        assert [(-1,) * 4 if b is None else b for b in boxes] == [tuple(int(v) for v in r) for r in stored]
        assert [len(f) for f in det.detect_from_batch(frames[..., ::-1])] == [len(gold[f"kept_{_key(hw)}_{n}"]) for n in range(3)]
    assert max(kept_counts) >= 3 and min(kept_counts) == 0
    assert H.nms(np.zeros((0, 5)), 0.3) == []


def test_smoothing_and_avatar_boxes_against_the_stored_reference_outputs(gold):
    from livetalking_amd import face_detect as H
    out = H.get_smoothened_boxes(gold["smooth_in"].copy(), T=5)
    assert out.dtype.kind == "i" and np.array_equal(out, gold["smooth_out"])
    preds = [None if p[0] < 0 else tuple(int(v) for v in p) for p in gold["avatar_pred"]]
    frames = [np.zeros((64, 64, 3), np.uint8)] * len(preds)
    assert np.array_equal(H.avatar_boxes(preds, frames), gold["avatar_boxes"])
    assert any(p is None for p in preds)                                     # the whole-frame fallback is part of the example
    plain = H.avatar_boxes(preds, frames, nosmooth=True)
    assert plain[0].tolist() == [0, 0, 64, 64] and int(plain[:, 3].max()) <= 64   # the pad is clipped to the frame


def test_prepare_wav2lip_avatar_writes_the_directory_load_avatar_reads(gold, sd, walks, tmp_path, monkeypatch):
    from PIL import Image
    from livetalking_amd import face_detect as H
    import livetalking_amd.avatars.wav2lip_avatar as Wv
    base = walks[(64, 64)]["frames"]
    frames = [base[i % 3] for i in range(7)]                                 # the golden example's predictions: frames 0, 3, 6 without a face
    eng = FD.SimEngine(sd)
    out = H.prepare_wav2lip_avatar(frames, str(tmp_path / "data" / "avatars" / "av1"), eng, img_size=48, batch=2)
    assert eng.calls == [2, 2, 2, 1]
    with open(os.path.join(out, "coords.pkl"), "rb") as f:
        coords = pickle.load(f)
    assert coords == [(int(b[1]), int(b[3]), int(b[0]), int(b[2])) for b in gold["avatar_boxes"]]      # (y1, y2, x1, x2)

    def read_imgs(paths):                      # what cv2.imread returns: 3-channel BGR
        return [np.ascontiguousarray(np.asarray(Image.open(p).convert("RGB"))[:, :, ::-1]) for p in paths]

    monkeypatch.setattr(Wv, "read_imgs", read_imgs)
    monkeypatch.chdir(tmp_path)
    full, faces, coords2 = Wv.load_avatar("av1")
    assert coords2 == coords and len(full) == len(faces) == 7
    assert all(np.array_equal(a, b) for a, b in zip(full, frames)) and all(f.shape == (48, 48, 3) for f in faces)
    from oracle.paste_oracle import resize_linear_u8
    y1, y2, x1, x2 = coords[1]
    assert np.array_equal(faces[1], resize_linear_u8(np.ascontiguousarray(frames[1][y1:y2, x1:x2]), (48, 48)))
