"""GPU: the S3FD face detector as a device program (ltk_face_detect_load / ltk_face_detect; csrc/facedet.h, musetalk.hip
mt_build_face_detect_graph) on seeded weights: every listed launch against float64 on the device's own inputs at 64 x 64 and 72 x 104
with max_images = 2, on the 2-image chunk and on the short tail; the candidate lists end to end against float64 under tau_s / tau_b
(tests/s3fd_cases.py); 180 x 320 once against the stored reference results; an image alone, as the second of two and as the tail; the
cache of two programs and its drop; FaceDetector's boxes; a prepared Wav2Lip directory read back by load_avatar; loader refusals and
call order; a watched call.  Engine of its own (module scope); float64 references are computed once per size and shared."""
from __future__ import annotations

import os
import pickle

import numpy as np
import pytest
import torch

import s3fd_cases as FD
import s3fd_ref as R

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_REF = {}


def ref_of(hw):
    """float64 and fp16-model results of a case, once: dict(frames, cands, tau_s, tau_b, faces)."""
    hw = tuple(hw)
    if hw not in _REF:
        from livetalking_amd import face_detect as H
        from livetalking_amd.engine import Engine
        sd = FD.state_dict()
        frames = FD.frames(hw)
        w = R.walk(sd, R.preprocess(frames))
        m = FD.model_walk({k: v.float() for k, v in sd.items()}, frames, Engine.face_detect_program(*hw))
        heads = [w[R.head_prefix(i)] for i in range(6)]
        tau_s, tau_b = FD.taus(heads, [m[R.head_prefix(i)] for i in range(6)])
        cands = R.candidates(R.olist_from_heads(heads), FD.THRESH)
        _REF[hw] = dict(frames=frames, cands=cands, dense=FD.dense_scores(heads), tau_s=tau_s, tau_b=tau_b, faces=[H.keep_faces(rows) for _, rows in cands])
    return _REF[hw]


@pytest.fixture(scope="module")
def eng():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from livetalking_amd.engine import Engine
    import synth_inputs as synth
    e = Engine(0)
    e.load_face_detector(synth.s3fd_state_dict(FD.SEED), max_images=2)
    yield e
    e.close()


def detect(eng, frames, **kw):
    rows, keys = eng.face_detect(frames, return_keys=True, **kw)
    return list(zip(keys, rows))


# ------------------------------------------------------------------------------------------ op by op, end to end
@pytest.mark.parametrize("hw", [(64, 64), (72, 104)], ids=lambda s: "x".join(map(str, s)))
def test_every_launch_and_the_lists_against_float64(eng, hw):
    from livetalking_amd.engine import Engine
    ref = ref_of(hw)
    sd, frames = FD.state_dict(), ref["frames"]
    prog, plan = Engine.face_detect_program(*hw), Engine.face_detect_plan(*hw, 2)
    got = detect(eng, frames)                               # a 2-image chunk, then the short tail: the tail's run is the one read back
    fig = FD.check_candidates(got, ref["cands"], ref["dense"], ref["tau_s"], ref["tau_b"])
    print(f"{hw}: {[len(k) for k, _ in got]} candidates, score error {fig['worst_s']:.2e} (tau_s {ref['tau_s']:.2e}), box error {fig['worst_b']:.2e} "
          f"(tau_b {ref['tau_b']:.2e})")
    figs = FD.check_ops(eng.face_detect_debug_get, plan, prog, sd, frames[2:], got[2:])
    assert len(figs) == len(prog) == 39
    pair = detect(eng, frames[:2])
    figs2 = FD.check_ops(eng.face_detect_debug_get, plan, prog, sd, frames[:2], pair)
    worst = max(figs2, key=lambda n: figs2[n].get("worst", 0.0))
    print(f"{hw}: 39 launches on the tail and on the pair; worst |dev - ref| / tol {figs2[worst]['worst']:.3f} at {worst}")
    # the same image alone, as the second of two, and as the tail of three: byte-identical records
    alone = detect(eng, frames[1:2])
    for other in (pair[1], got[1]):
        assert np.array_equal(alone[0][0], other[0]) and np.array_equal(alone[0][1].view(np.uint32), other[1].view(np.uint32))
    tail = detect(eng, np.concatenate([frames[:2], frames[1:2]]))[2]
    assert np.array_equal(alone[0][0], tail[0]) and np.array_equal(alone[0][1].view(np.uint32), tail[1].view(np.uint32))


def test_180x320_against_the_stored_reference_results(eng):
    from livetalking_amd import face_detect as H
    g = np.load(os.path.join(ROOT, "tests", "golden", "s3fd_golden.npz"))
    hw = (180, 320)
    ref = ref_of(hw)
    heads = [torch.from_numpy(g[f"heads_180x320_{i}"].astype(np.float64)) for i in range(12)]
    stored = R.candidates(heads, FD.THRESH)
    got = detect(eng, ref["frames"])
    # the stored heads are float32: their own rounding (2^-24 relative on logits below 16: 1e-6 on a score, 1e-4 on a box) joins tau
    fig = FD.check_candidates(got, stored, FD.dense_scores(heads), ref["tau_s"] + 2e-6, ref["tau_b"] + 2e-4)
    boxes = [H.first_box(H.keep_faces(np.asarray(rows, np.float64))) for _, rows in got]
    FD.check_boxes(boxes, [g[f"kept_180x320_{n}"] for n in range(2)], ref["tau_b"])
    print(f"180 x 320: {[len(k) for k, _ in got]} candidates, score error {fig['worst_s']:.2e} (tau_s {ref['tau_s']:.2e}), box error "
          f"{fig['worst_b']:.2e} (tau_b {ref['tau_b']:.2e}); boxes {boxes}, stored {g['boxes_180x320'].tolist()}")


# ------------------------------------------------------------------------------------------ the cache of two programs
def test_two_sizes_alternate_and_a_third_drops_one(eng):
    a, b = ref_of((64, 64)), ref_of((72, 104))
    first = {hw: detect(eng, r["frames"][:2]) for hw, r in (((64, 64), a), ((72, 104), b))}
    for _ in range(2):
        for hw, r in (((64, 64), a), ((72, 104), b)):
            again = detect(eng, r["frames"][:2])
            assert all(np.array_equal(x[0], y[0]) and np.array_equal(x[1], y[1]) for x, y in zip(again, first[hw]))
    third = np.ascontiguousarray(b["frames"][:1, :40, :48])              # 40 x 48: a third size, the least recently used program goes
    assert len(detect(eng, third)[0][0]) > 0
    for hw, r in (((64, 64), a), ((72, 104), b)):                        # both come back (one of them rebuilt) with the same bytes
        again = detect(eng, r["frames"][:2])
        assert all(np.array_equal(x[0], y[0]) and np.array_equal(x[1], y[1]) for x, y in zip(again, first[hw]))


def test_image_by_image_fallback_keeps_an_images_bytes(eng):
    """720 x 1280 x 2: conv7_1 changes kernel family between one image and two (tests/test_face_detect_host.py), so the pair runs it
    image by image; the second image's records equal its records alone.  Threshold 0.45: the seeded weights put more positions above
    0.05 than the lists hold at this size."""
    import synth_inputs as synth
    frames = np.stack([synth.s3fd_frame(720, 1280, s) for s in (1, 2)])
    pair = detect(eng, frames, thresh=0.45)
    alone = detect(eng, frames[1:2], thresh=0.45)
    assert len(alone[0][0]) > 0
    assert np.array_equal(alone[0][0], pair[1][0]) and np.array_equal(alone[0][1].view(np.uint32), pair[1][1].view(np.uint32))


# ------------------------------------------------------------------------------------------ host side on the engine
def test_face_detector_boxes(eng):
    from livetalking_amd import face_detect as H
    for hw in ((64, 64), (72, 104)):
        ref = ref_of(hw)
        det = H.FaceDetector(eng)
        boxes = det.get_detections_for_batch(ref["frames"])
        FD.check_boxes(boxes, ref["faces"], ref["tau_b"])
        faces = det.detect_from_batch(ref["frames"][..., ::-1])
        assert [len(f) for f in faces] == [len(f) for f in ref["faces"]]
    assert boxes is not None and ref_of((64, 64))["faces"][0] == []      # the 64 x 64 case's first frame has no face


def test_prepared_wav2lip_directory_reads_back(eng, tmp_path, monkeypatch):
    from PIL import Image
    from livetalking_amd import face_detect as H
    import livetalking_amd.avatars.wav2lip_avatar as Wv
    ref = ref_of((64, 64))
    frames = [ref["frames"][i % 3] for i in range(7)]                    # frames 0, 3 and 6 have no face: the whole frame is their box
    out = H.prepare_wav2lip_avatar(frames, str(tmp_path / "data" / "avatars" / "av1"), eng, img_size=96, batch=2)
    boxes = H.avatar_boxes(H.FaceDetector(eng).get_detections_for_batch(np.array(frames)), frames)
    with open(os.path.join(out, "coords.pkl"), "rb") as f:
        coords = pickle.load(f)
    assert coords == [(int(b[1]), int(b[3]), int(b[0]), int(b[2])) for b in boxes]

    def read_imgs(paths):                      # what cv2.imread returns: 3-channel BGR
        return [np.ascontiguousarray(np.asarray(Image.open(p).convert("RGB"))[:, :, ::-1]) for p in paths]

    monkeypatch.setattr(Wv, "read_imgs", read_imgs)
    monkeypatch.chdir(tmp_path)
    full, faces, coords2 = Wv.load_avatar("av1")
    assert coords2 == coords and len(full) == len(faces) == 7
    assert all(np.array_equal(a, b) for a, b in zip(full, frames)) and all(f.shape == (96, 96, 3) for f in faces)


# ------------------------------------------------------------------------------------------ refusals, call order, the watch
def test_loader_refusals_and_call_order():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from livetalking_amd._lib import LtkError
    from livetalking_amd.engine import Engine
    import synth_inputs as synth
    sd = synth.s3fd_state_dict(FD.SEED)
    frame = FD.frames((64, 64))[:1]
    e = Engine(0)
    try:
        with pytest.raises(LtkError) as ex:
            e.face_detect(frame)
        assert ex.value.code == -3 and "ltk_face_detect_load" in str(ex.value)
        short = {k: v for k, v in sd.items() if k != "conv6_2_mbox_loc.bias"}
        with pytest.raises(LtkError) as ex:
            e.load_face_detector(short)
        assert ex.value.code == -1 and "conv6_2_mbox_loc.bias" in str(ex.value)
        with pytest.raises(LtkError) as ex:
            e.load_face_detector(sd, max_images=17)
        assert ex.value.code == -1 and "max_images" in str(ex.value)
        e.load_face_detector(sd, max_images=1)                        # the refused loads left nothing behind
        with pytest.raises(LtkError) as ex:
            e.load_face_detector(sd)
        assert ex.value.code == -3
        with pytest.raises(LtkError) as ex:
            e.face_detect(np.zeros((1, 31, 64, 3), np.uint8))
        assert ex.value.code == -1 and "[32, 16384]" in str(ex.value)
        with pytest.raises(LtkError) as ex:
            e.face_detect(frame, cap=4097)
        assert ex.value.code == -1 and "cap" in str(ex.value)
        rows = e.face_detect(frame)
        assert len(rows[0]) >= 40
        with pytest.raises(RuntimeError, match="candidates"):          # a list shorter than the hits: the call reports it
            e.face_detect(frame, cap=16)
        strict = e.face_detect(frame, thresh=0.3)                      # the threshold is the call's, not the captured program's
        assert 0 < len(strict[0]) < len(rows[0]) and float(strict[0][:, 4].min()) > 0.3
        assert np.array_equal(e.face_detect(frame)[0], rows[0])
    finally:
        e.close()


def test_a_watched_call_lists_every_launch_and_changes_no_record(eng):
    ref = ref_of((64, 64))
    plain = detect(eng, ref["frames"])
    eng.health_watch("facedet", 1)
    watched = detect(eng, ref["frames"])
    assert all(np.array_equal(x[0], y[0]) and np.array_equal(x[1], y[1]) for x, y in zip(watched, plain))
    ops, seen, left = eng.health_report("facedet")                     # 2 + 1 images: one call, whatever its chunks
    assert (seen, left) == (1, 0) and len(ops) == 39
    from livetalking_amd.engine import Engine
    prog = Engine.face_detect_program(64, 64)
    assert [o["name"] for o in ops] == [p["name"] for p in prog] and [o["type"] for o in ops] == [p["type"] for p in prog]
    for o, p in zip(ops, prog):
        assert bool(o["observed"]) == (p["type"] != 23), o["name"]
        assert o["nonfinite"] == 0 and o["at_limit"] == 0
    assert all(np.array_equal(x[0], y[0]) and np.array_equal(x[1], y[1]) for x, y in zip(detect(eng, ref["frames"]), plain))    # disarmed: replayed again
