"""CPU tests of the Ultralight avatar: ABI surface, argument checks without a GPU, the plugin module's contract, HubertASR's
cadence and slicing, and the float64 restatement (tests/ultralight_ref.py) against the reference's own Model
(tests/golden/ultralight_golden.npz, scripts/gen_golden_ultralight.py)."""
from __future__ import annotations

import ctypes as C
import importlib.util
import inspect
import os
import re
import types

import numpy as np
import pytest

import synth_inputs as synth
import ultralight_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REFERENCE = os.environ.get("LTK_REFERENCE", "/root/reference")
HAVE_REFERENCE = os.path.isfile(os.path.join(REFERENCE, "avatars", "ultralight_avatar.py"))

NEW_ENTRIES = ["ltk_ultralight_avatar_register", "ltk_ultralight_infer", "ltk_ultralight_paste_back", "ltk_ultralight_forward_host",
               "ltk_ultralight_time", "ltk_dwconv3x3_f16", "ltk_upsample2x_cat_f16", "ltk_ultralight_op_count", "ltk_ultralight_op_name"]


def _gen():
    spec = importlib.util.spec_from_file_location("gen_golden_ultralight", os.path.join(ROOT, "scripts", "gen_golden_ultralight.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.fixture(scope="module")
def golden(golden_dir):
    return dict(np.load(os.path.join(golden_dir, "ultralight_golden.npz")))


@pytest.fixture(scope="module")
def f64_run():
    """ONE float64 forward of the golden's inputs, shared."""
    sd = synth.ultralight_state_dict(1234)
    img6, feat = synth.ultralight_inputs(2, 1234)
    taps = {}
    pred = ref.forward(sd, img6, feat, taps=taps)
    return pred, taps


# ------------------------------------------------------------------ ABI
def test_header_declares_and_library_exports_the_ultralight_entries():
    from livetalking_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "ltk.h")).read()
    lib = _lib.load()
    for name in NEW_ENTRIES:
        assert re.search(r"\bint\s+" + name + r"\s*\(", hdr), f"{name} is not declared in include/ltk.h"
        assert name in _lib.SYMBOLS
        assert getattr(lib, name) is not None
    assert "typedef struct ltk_ul_req" in hdr
    fields = [f[0] for f in _lib.UlReq._fields_]
    assert fields == ["avatar", "index", "batch", "d_feat", "d_pred"]
    # every entry names the reference lines it replaces
    for name in ("ltk_ultralight_avatar_register", "ltk_ultralight_infer", "ltk_ultralight_paste_back"):
        doc = hdr[:hdr.index("int " + name)].rsplit("/*", 1)[1]
        assert "ultralight_avatar.py:" in doc, name


def test_null_and_garbage_arguments_are_invalid_without_a_gpu():
    from livetalking_amd import _lib
    lib = _lib.load()
    INVALID = -1
    aid = C.c_int(0)
    buf = (C.c_uint8 * 16)()
    assert lib.ltk_ultralight_avatar_register(None, None, 0, None, None, None, 0, 0, 0, 0, C.byref(aid)) == INVALID
    assert lib.ltk_last_error()
    assert lib.ltk_ultralight_infer(None, None, 0, None) == INVALID
    req = (_lib.UlReq * 1)()
    assert lib.ltk_ultralight_infer(None, req, 1, None) == INVALID
    assert lib.ltk_ultralight_paste_back(None, 1, 0, buf, buf, 0, None) == INVALID
    assert lib.ltk_ultralight_forward_host(None, 1, buf, buf, 1, buf) == INVALID
    ms, macs = C.c_float(), C.c_double()
    assert lib.ltk_ultralight_time(None, 1, 1, 1, C.byref(ms), C.byref(macs)) == INVALID
    assert lib.ltk_ultralight_op_count(None, 1) == 0
    assert lib.ltk_ultralight_op_name(None, 1, 0, None, 0, None) == INVALID
    assert lib.ltk_dwconv3x3_f16(None, buf, 1, 4, 4, 16, buf, 1, None, None, 1, buf) == INVALID
    assert lib.ltk_upsample2x_cat_f16(None, buf, 1, 4, 4, 16, buf, 8, 8, 16, buf) == INVALID


# ------------------------------------------------------------------ plugin contract
def _ref_signatures():
    """Parameter names of the reference module's functions and LightReal's methods, from its source (the module itself imports
    cv2 / av / transformers)."""
    import ast
    tree = ast.parse(open(os.path.join(REFERENCE, "avatars", "ultralight_avatar.py"), encoding="utf-8").read())
    out = {}
    for node in tree.body:
        if isinstance(node, ast.FunctionDef):
            out[node.name] = [a.arg for a in node.args.args]
        if isinstance(node, ast.ClassDef) and node.name == "LightReal":
            for m in node.body:
                if isinstance(m, ast.FunctionDef):
                    out["LightReal." + m.name] = [a.arg for a in m.args.args]
            out["@register"] = [[getattr(a, "value", None) for a in d.args] for d in node.decorator_list if isinstance(d, ast.Call)]
    return out


def test_plugin_module_has_the_reference_names_and_signatures():
    from livetalking_amd import hostshim
    from livetalking_amd.avatars import ultralight_avatar as ul
    want = {"load_model": ["opt"], "load_avatar": ["avatar_id"], "warm_up": ["batch_size", "avatar", "modelres"],
            "LightReal.__init__": ["self", "opt", "model", "avatar"], "LightReal.inference_batch": ["self", "index", "audiofeat_batch"],
            "LightReal.paste_back_frame": ["self", "pred_frame", "idx"]}
    if HAVE_REFERENCE:
        got_ref = _ref_signatures()
        for k, v in want.items():
            assert got_ref[k] == v, f"the reference's {k} takes {got_ref[k]}"
        assert got_ref["@register"] == [["avatar", "ultralight"]]
    for k, v in want.items():
        fn = getattr(ul.LightReal, k.split(".")[1]) if "." in k else getattr(ul, k)
        assert list(inspect.signature(fn).parameters) == v, k
    if not hostshim.USING_REFERENCE_HOST:
        assert hostshim._REGISTRY["avatar"]["ultralight"] is ul.LightReal
    assert issubclass(ul.LightReal, hostshim.BaseAvatar)


# ------------------------------------------------------------------ HubertASR
class _StandInProcessor:
    """get_hubert_from_16k_speech: one row of 1024 per 320 samples (kernel 400), values a function of the row and the call."""

    def __init__(self):
        self.calls = []

    def get_hubert_from_16k_speech(self, pcm):
        rows = (len(pcm) - 80) // 320
        feat = (np.random.default_rng(len(self.calls)).integers(-128, 128, (rows, 1024)) / 16.0).astype(np.float32)
        self.calls.append((len(pcm), feat))
        return feat


def test_hubert_asr_run_step_cadence_and_chunks(golden_dir):
    from livetalking_amd.avatars.audio_features.hubert import HubertASR, feature2chunks
    gen = _gen()
    opt = types.SimpleNamespace(fps=25, batch_size=4, l=10, r=10)
    proc = _StandInProcessor()
    asr = HubertASR(opt, None, proc, audio_feat_length=[4, 4])
    asr.warm_up()
    assert len(asr.frames) == 20
    f2c_ref = gen.reference_feature2chunks(REFERENCE) if HAVE_REFERENCE else None
    rng = np.random.default_rng(0)
    for step in range(3):
        for _ in range(2 * opt.batch_size):
            asr.put_audio_frame(rng.standard_normal(320).astype(np.float32), {})
        asr.run_step()
        chunks = asr.feat_queue.get_nowait()
        n_pcm, feat = proc.calls[-1]
        assert n_pcm == (20 + 2 * opt.batch_size) * 320            # l + 2B + r chunks of 20 ms
        assert len(chunks) == opt.batch_size and all(c.shape == (16, 1024) and c.dtype == np.float32 for c in chunks)
        for i, c in enumerate(chunks):                                # rows [2 * (i + l/2) - 8, + 16)
            assert np.array_equal(c, feat[2 * i + 2: 2 * i + 18])
        if f2c_ref is not None:
            want = f2c_ref(feature_array=feat, batch_size=opt.batch_size, audio_feat_win=[4, 4], start=opt.l / 2, feature_idx_multiplier=2)
            assert all(np.array_equal(a, b) for a, b in zip(chunks, want))
        assert len(asr.frames) == 20 and asr.output_queue.qsize() == 10 + (step + 1) * 2 * opt.batch_size
    # all-silent steps: the first one after speech still extracts features, the next ones hand out zero chunks
    asr.run_step()
    n_calls = len(proc.calls)
    asr.feat_queue.get_nowait()
    asr.run_step()
    silent = asr.feat_queue.get_nowait()
    assert len(proc.calls) == n_calls and all(c.shape == (16, 1024) and not c.any() for c in silent)
    # the slicing itself, windows leaving the array at either end included, against the reference's recorded output
    fix = np.load(os.path.join(golden_dir, "hubert_chunks_golden.npz"))
    for i, (name, (rows, batch, left)) in enumerate(gen.HUBERT_CASES.items()):
        feat = gen.hubert_features(rows, gen.SEED + i)
        got = np.stack(feature2chunks(feat, batch, [4, 4], left / 2, 2))
        assert got.shape == (batch, 16, 1024)
        assert np.array_equal(got, fix[name]), name
    if HAVE_REFERENCE:
        fresh = gen.generate_hubert(REFERENCE)
        assert all(np.array_equal(fresh[k], fix[k]) for k in gen.HUBERT_CASES)


def test_hubert_load_model_needs_the_checkpoint(tmp_path, monkeypatch):
    from livetalking_amd.avatars.audio_features import hubert
    monkeypatch.chdir(tmp_path)
    with pytest.raises(FileNotFoundError, match="hubert-large-ls960-ft"):
        hubert.load_model()
    with pytest.raises(TypeError):
        hubert.HubertASR(types.SimpleNamespace(fps=25, batch_size=2, l=10, r=10), None, object())


# ------------------------------------------------------------------ synthetic weights and the float64 restatement
def test_synthetic_state_dict_has_the_reference_names():
    sd = synth.ultralight_state_dict(1234)
    assert len(sd) == 484
    assert sum(int(np.prod(v.shape)) for k, v in sd.items() if not k.endswith("num_batches_tracked") and "running" not in k) == 12_159_591      # the 12.2 M parameters of Model(6, "hubert")
    convs = sorted(k[:-len(".weight")] for k, v in sd.items() if k.endswith(".weight") and v.ndim == 4)
    assert convs == sorted(ref.conv_prefixes())
    assert sd["audio_model.conv5.weight"].shape == (512, 256, 3, 3) and sd["inc.inconv.0.conv.0.weight"].shape == (12, 6, 1, 1)
    frames, faces, coords = synth.ultralight_avatar(3, (120, 200), seed=1)
    assert faces[0].shape == (168, 168, 3) and frames[0].shape == (120, 200, 3)
    assert all(0 <= x1 < x2 <= 200 and 0 <= y1 < y2 <= 120 for x1, y1, x2, y2 in coords)


def test_float64_restatement_equals_the_reference_golden(golden, f64_run):
    """Bound = the fp32-vs-fp64 gap of this network (the golden is the reference's float32 run): frames differ by at most 1 LSB on
    fewer than 1e-3 of the bytes, taps agree to rel L2 1e-5."""
    gen = _gen()
    pred, taps = f64_run
    assert int(golden["seed"]) == 1234 and int(golden["batch"]) == 2
    mx, psnr, share = ref.frame_stats(ref.frames_u8(pred), golden["frames"])
    print(f"frames vs golden: max {mx} LSB, {psnr:.1f} dB, {share:.2e} of the bytes differ")
    assert mx <= 1 and share < 1e-3
    for key, (_, tap_name) in gen.TAPS.items():
        t = taps[tap_name]
        assert tuple(golden["shape_" + key]) == t.shape, key
        assert np.array_equal(golden["pos_" + key], gen.sample_positions(key, t.size))
        got = t.reshape(-1)[golden["pos_" + key]]
        want = golden["tap_" + key].astype(np.float64)
        rel = np.linalg.norm(got - want) / np.linalg.norm(want)
        print(f"{key}: rel L2 {rel:.2e}")
        assert rel <= 1e-5, key
    inside = ((pred > 0.02) & (pred < 0.98)).mean()
    assert inside > 0.99            # the sigmoid is used across its range, not saturated


@pytest.mark.skipif(not HAVE_REFERENCE, reason="needs the LiveTalking checkout")
def test_golden_is_what_the_reference_model_computes(golden):
    fresh = _gen().generate(REFERENCE)
    assert set(fresh) == set(golden)
    assert np.array_equal(fresh["frames"], golden["frames"])
    for k in fresh:
        if k.startswith("tap_"):
            assert np.allclose(fresh[k], golden[k], rtol=1e-5, atol=1e-6), k


def test_fp16_rounding_model_sits_where_the_recipe_puts_it(f64_run):
    """The yardstick of the GPU frame tests: with the fixed-statistics recipe an fp16 implementation of the reference is within
    1 LSB of float64, >= 59 dB, < 8 % of the bytes."""
    pred, _ = f64_run
    sd = synth.ultralight_state_dict(1234)
    img6, feat = synth.ultralight_inputs(2, 1234)
    m16 = ref.forward(sd, img6, feat, fp16_model=True)
    mx, psnr, share = ref.frame_stats(ref.frames_u8(m16), ref.frames_u8(pred))
    print(f"fp16 model vs float64: max {mx} LSB, {psnr:.2f} dB, {share:.4f}")
    assert mx <= 1 and psnr >= 59.0 and share < 0.08


def test_input_pack_restates_the_mask_rectangle():
    frames, faces, _ = synth.ultralight_avatar(1, (64, 64), seed=2)
    x = ref.img6_from_faces(faces)
    assert x.shape == (1, 6, 160, 160)
    real, masked = x[0, :3], x[0, 3:]
    assert np.array_equal(real, faces[0][4:164, 4:164].transpose(2, 0, 1).astype(np.float32) / 255.0)
    assert not masked[:, 5:150, 5:155].any()
    keep = np.ones((160, 160), bool)
    keep[5:150, 5:155] = False
    assert np.array_equal(masked[:, keep], real[:, keep])
