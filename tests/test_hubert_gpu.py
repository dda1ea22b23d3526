"""GPU tests of HuBERT-large on the engine: its own kernels against torch float64 on the device's inputs, the whole program op by
op (teacher-forced, tests/hubert_ref.py + oracle/op_replay.py) and end to end against float64 with the fp16 rounding model as the
yardstick, the clip path, the live step into ltk_ultralight_infer, and the plugin behind LTK_HUBERT_ENGINE=1.  One engine with the
seeded 2-layer model (module scope); the 24-layer test brings its own."""
from __future__ import annotations

import importlib.util
import math
import os
import types

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import hubert_ref as H
import synth_inputs as synth
from oracle import op_replay as R

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U = 2.0 ** -24


def _emit(lines):
    """What the parity record (profiles/hubert_parity.txt) is made of: LTK_HUBERT_PARITY_OUT names a file to append to."""
    for ln in lines:
        print(ln)
    out = os.environ.get("LTK_HUBERT_PARITY_OUT")
    if out:
        with open(out, "a") as f:
            f.write("\n".join(lines) + "\n")


def _gate(name, dev, ref, mod, tol):
    """op_replay's two gates on token-major tensors: per element |dev - ref| <= tol (+ 2^-24), aggregate rel_l2(dev, ref) <=
    2 rel_l2(mod, ref) + 1e-4; the rounding model itself has to sit inside half the bound."""
    dev, ref, mod, tol = (torch.as_tensor(np.asarray(t)).double() for t in (dev, ref, mod, tol))
    tol = tol + R.F16_FLOOR
    e = (dev - ref).abs()
    r_dev, r_mod = R.rel_l2(dev, ref), R.rel_l2(mod, ref)
    worst = float((e / tol).max())
    _emit([f"{name}: rel_l2 dev {r_dev:.3e} mod {r_mod:.3e}, max |dev - ref| / tol {worst:.2f}, model {float(((mod - ref).abs() / tol).max()):.2f}"])
    assert float(((mod - ref).abs() / tol).max()) <= R.MODEL_HEADROOM, name
    assert int((e > tol).sum()) == 0, f"{name}: {int((e > tol).sum())} elements outside the bound, worst {worst:.2f}"
    assert r_dev <= R.AGG_FACTOR * r_mod + R.AGG_FLOOR, name


@pytest.fixture(scope="module")
def sd2():
    return H.state_dict(2, 20)


@pytest.fixture(scope="module")
def eng(sd2):
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from livetalking_amd.engine import Engine
    e = Engine(0)
    e.load_hubert(sd2)
    yield e
    e.close()


# ------------------------------------------------------------------ kernels on their own
@pytest.mark.parametrize("n,dc", [(400, 0.0), (16640, 0.0), (100003, 0.0), (100003, 100.0)])
def test_stats_against_float64(eng, n, dc):
    """Mean and population variance of n fp32 samples; dc = 100 on unit-variance noise is where E[x^2] - E[x]^2 loses the variance
    (1e4 - 1e4 in fp32: 1e-3 and more of what is left).  The kernel sums in fp32: a thread adds m = ceil(n / 1024) terms in turn, a
    wave tree of 6 levels and 16 wave sums follow, so no term passes through more than m + 22 additions; with u = 2^-24, centred
    sums (mean = mean0 + sum(x - mean0) / n, var = sum (x - mean0)^2 / n - (mean - mean0)^2) and a few roundings for the
    subtraction, the square and the final division
        |mean - mean64| <= u ((m + 25) mad + 2 |mean64|),  mad = mean |x - mean64| + (m + 23) u mean |x|   (mean0's own error)
        |var  - var64 | <= 1.01 u (m + 30) var64.
    At n = 100 003 that is 7.8e-6 of the variance; the uncentred form misses it by three orders of magnitude at dc = 100."""
    x = (np.random.default_rng(n).standard_normal(n) + dc).astype(np.float32)
    mean, var = eng.hubert_stats(x)
    x64 = x.astype(np.float64)
    m = math.ceil(n / 1024)
    mad = np.abs(x64 - x64.mean()).mean() + (m + 23) * U * np.abs(x64).mean()
    b_mean = U * ((m + 25) * mad + 2 * abs(x64.mean()))
    b_var = 1.01 * U * (m + 30) * x64.var()
    print(f"n {n} dc {dc}: mean err {abs(mean - x64.mean()):.3e} (bound {b_mean:.3e}), var err {abs(var - x64.var()):.3e} (bound {b_var:.3e})")
    assert abs(mean - x64.mean()) <= b_mean
    assert abs(var - x64.var()) <= b_var


@pytest.mark.parametrize("n", [400, 1043, 16640])
def test_layer0_against_float64(eng, sd2, n):
    """Conv1d(1, 512, 10, 5) + LayerNorm + GELU in one kernel on an fp32 waveform: 79, 207 and 3 327 time steps (a block is 32 of
    them, a wave 8: partial waves and partial blocks).  Bound: hubert_ref.layer0_model."""
    p = "feature_extractor.conv_layers.0"
    w, b, g, be = (sd2[p + s] for s in (".conv.weight", ".conv.bias", ".layer_norm.weight", ".layer_norm.bias"))
    x = H.normalise(H.speech(n, 5)).astype(np.float32)
    dev = eng.hubert_layer0(x, w.reshape(512, 10), b, g, be)
    assert dev.shape == ((n - 10) // 5 + 1, 512)
    xt = torch.from_numpy(x).double().reshape(1, 1, -1)
    t64 = lambda a: torch.from_numpy(a).double()
    z = F.conv1d(xt, t64(w), t64(b), stride=5).transpose(1, 2)
    ref = F.gelu(F.layer_norm(z, (512,), t64(g), t64(be), 1e-5))
    mod, tol = H.layer0_model(xt.float(), torch.from_numpy(w), torch.from_numpy(b), torch.from_numpy(g), torch.from_numpy(be), ref.float())
    _gate(f"layer0 n={n}", dev[None], ref, mod, tol)


@pytest.mark.parametrize("T", [1, 17, 79])
def test_ln_gelu_against_float64(eng, sd2, T):
    """LayerNorm(512) + GELU on CB16: one row, one block and a row (16 rows per block), five blocks less a row; rows with a mean
    of several standard deviations included.  Bound: hubert_ref.ln_gelu_model (op_replay's LayerNorm bound through the GELU)."""
    p = "feature_extractor.conv_layers.3.layer_norm"
    g, be = sd2[p + ".weight"], sd2[p + ".bias"]
    rng = np.random.default_rng(T)
    x = (rng.standard_normal((T, 512)) * rng.uniform(0.2, 3.0, (T, 1)) + rng.standard_normal((T, 1)) * 4.0).astype(np.float16).astype(np.float32)
    dev = eng.hubert_ln_gelu(x, g, be)
    xt = torch.from_numpy(x)[None]
    ref = F.gelu(F.layer_norm(xt.double(), (512,), torch.from_numpy(g).double(), torch.from_numpy(be).double(), 1e-5))
    mod, tol = H.ln_gelu_model(xt, torch.from_numpy(g), torch.from_numpy(be), ref.float())
    _gate(f"ln_gelu T={T}", dev[None], ref, mod, tol)


@pytest.fixture(scope="module")
def pos_weights(sd2):
    w = H.fold_weight_norm(sd2)[H.W_KEY].float().numpy()
    return w, sd2["encoder.pos_conv_embed.conv.bias"]


@pytest.mark.parametrize("T", [1, 3, 51, 70, 130])
def test_posconv_against_float64(eng, pos_weights, T):
    """x + GELU(grouped Conv1d k 128 pad 64 (x)[:T]): T = 1 (every tap but one in the padding), 3, 51 (the live length: two row
    tiles of 32, the second one partial), 70 (a tile's edge + 6), 130 (five tiles, taps cut at both ends).  Bound:
    hubert_ref.posconv_model = op_replay's conv / linear bound at K = 8192 through its GELU bound.  The same call twice gives the
    same bytes (the tap split is summed in a fixed order)."""
    w, b = pos_weights
    x = np.random.default_rng(100 + T).standard_normal((T, 1024)).astype(np.float16).astype(np.float32)
    dev = eng.hubert_posconv(x, w, b)
    assert np.array_equal(dev, eng.hubert_posconv(x, w, b))
    xt = torch.from_numpy(x)[None]
    conv = F.conv1d(xt.double().transpose(1, 2), torch.from_numpy(w).double(), torch.from_numpy(b).double(), padding=64, groups=16)[:, :, :-1]
    ref = xt.double() + F.gelu(conv.transpose(1, 2))
    mod, tol = H.posconv_model(xt, torch.from_numpy(w), torch.from_numpy(b), ref.float())
    _gate(f"posconv T={T}", dev[None], ref, mod, tol)


def test_chunk_gather_is_bit_exact(eng, golden_dir):
    """The cases of tests/golden/hubert_chunks_golden.npz (the reference's own _feature2chunks: a step, windows leaving the array
    on the left and on the right); their values are multiples of 1/16, exact in fp16."""
    spec = importlib.util.spec_from_file_location("gen_golden_ultralight", os.path.join(ROOT, "scripts", "gen_golden_ultralight.py"))
    gen = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gen)
    fix = np.load(os.path.join(golden_dir, "hubert_chunks_golden.npz"))
    for i, (name, (rows, batch, left)) in enumerate(gen.HUBERT_CASES.items()):
        feat = gen.hubert_features(rows, gen.SEED + i)
        got = eng.hubert_chunks(feat, batch, first_row=int(left / 2 * 2) - 8, row_step=2, rows=16)
        assert np.array_equal(got, fix[name]), name


# ------------------------------------------------------------------ the whole program
def _fetch(eng):
    def fetch(name, ref):
        _, C, T, _ = ref.shape
        t = torch.from_numpy(eng.hubert_debug_get(name, (C, T))).reshape(1, C, T, 1).to(ref.dtype)
        return t * 8.0 if name.endswith(".q_proj") else t          # d^-0.5 = 1 / 8 is folded into q_proj
    return fetch


# rows at which the kernel choice of a program changes with the clip's length (n = 320 T + 80 samples give T rows)
EDGE_ROWS = (1, 31, 32, 33, 51, 64, 65, 128, 129, 513)


@pytest.mark.parametrize("n", [1040, 22613] + [320 * T + 80 for T in EDGE_ROWS])
def test_every_op_against_float64(eng, sd2, n):
    """2 layers, every op on the device's own input, op_replay's gates, and no op of hubert_ops() left uncompared.  3 rows and 70
    rows (layers 5 and 6 are the two-tap convs; 70 rows take conv3 for the linear layers, 3 rows the row GEMM), then the lengths
    where a program built for another clip length takes another kernel: 1 row; 31 / 32 / 33 and 64 / 65, 128 / 129 (the attention's
    32-key tiles and blocks of four query tiles; the linear layers leave the row GEMM for conv3 from 65 rows on); 51, the live step's
    length; 513 (feature_projection.projection goes to lin_fk_kernel from 512 rows on, conv3's split-K choice moves with the row
    count).  At most three programs stay alive over the sweep."""
    pcm = H.speech(n, 9)
    feat = eng.hubert_features(pcm)
    assert feat.shape == ((n - 80) // 320, 1024)
    assert eng.hubert_info()["programs"] <= 3
    x_norm = eng.hubert_debug_get("input_values", (n,))
    assert R.rel_l2(torch.from_numpy(x_norm), torch.from_numpy(H.normalise(pcm))) <= 1e-6
    rp = H.replay(sd2, x_norm, _fetch(eng))
    ops = eng.hubert_ops()
    assert [nm for nm, _ in ops] == H.op_names(2)
    _emit([f"# hubert op replay, {n} samples ({H.rows(n)} rows)"] + R.format_records(f"n={n}", rp.records))
    miss = R.uncovered(ops, [r["name"] for r in rp.records], {})
    assert not miss, miss
    bad = R.failures(rp.records)
    assert not bad, "\n".join(bad)


def _end_to_end(eng, sd, n, label):
    pcm = H.speech(n, 12)
    dev = eng.hubert_features(pcm)
    ref = H.features(sd, pcm)
    model = H.features(sd, pcm, fp16_model=True)
    r_dev, r_mod = R.rel_l2(torch.from_numpy(dev), torch.from_numpy(ref)), R.rel_l2(torch.from_numpy(model), torch.from_numpy(ref))
    info = eng.hubert_info()
    _emit([f"# hubert end to end, {label}: {dev.shape[0]} rows, rel_l2 dev {r_dev:.3e}, fp16 model {r_mod:.3e} (gate {R.AGG_FACTOR * r_mod:.3e}); "
           f"{info['programs']} programs, activations of the last one {info['activation_bytes'] / 1e6:.1f} MB"])
    assert dev.shape == ref.shape
    assert r_dev <= R.AGG_FACTOR * r_mod
    return info


def test_end_to_end_24_layers_live_length():
    """24 layers, 16 640 samples (51 rows) against the float64 forward.  Yardstick: hubert_ref.forward(fp16_model=True), whose own
    rel L2 against float64 on these weights and this input is 1.45e-3 (computed on the CPU; profiles/hubert_parity.txt); gate:
    rel L2 <= 2x that, op_replay's aggregate factor."""
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from livetalking_amd.engine import Engine
    sd = H.state_dict(24, 7)
    e = Engine(0)
    try:
        e.load_hubert(sd)
        assert e.hubert_info()["layers"] == 24
        _end_to_end(e, sd, 16640, "24 layers, 16 640 samples")
    finally:
        e.close()


def test_end_to_end_clip_path(eng, sd2):
    """2 layers, 330 000 samples: the 320 080-sample clip (1 000 rows) and the 10 000-sample tail (31 rows), normalised over the
    whole input, against the float64 restatement of the loop.  The fp16 model's own rel L2 here is 1.19e-3 (CPU;
    profiles/hubert_parity.txt).  Then a third and a fourth length: at most three programs stay."""
    _end_to_end(eng, sd2, 330000, "2 layers, 330 000 samples")
    for n in (1040, 16640, 22613):
        eng.hubert_features(H.speech(n, 1))
    assert eng.hubert_info()["programs"] == 3


def test_load_refuses_bad_input(eng, sd2):
    from livetalking_amd._lib import LtkError
    from livetalking_amd.engine import Engine
    with pytest.raises(LtkError) as ex:
        eng.load_hubert(sd2)
    assert ex.value.code == -3
    e = Engine(0)
    try:
        with pytest.raises(LtkError) as ex:
            e.hubert_features(H.speech(1040))
        assert ex.value.code == -3
        missing = {k: v for k, v in sd2.items() if k != "encoder.layers.1.attention.k_proj.bias"}
        with pytest.raises(LtkError) as ex:
            e.load_hubert(missing)
        assert ex.value.code == -1 and "encoder.layers.1.attention.k_proj.bias" in str(ex.value)
        wrong = dict(sd2)
        wrong["feature_extractor.conv_layers.5.conv.weight"] = np.zeros((512, 512, 3), np.float32)
        with pytest.raises(LtkError) as ex:
            e.load_hubert(wrong)
        assert ex.value.code == -1 and "feature_extractor.conv_layers.5.conv.weight" in str(ex.value)
        e.load_hubert(sd2)                                   # a failed load leaves nothing behind
        with pytest.raises(LtkError) as ex:
            e.hubert_features(H.speech(399))
        assert ex.value.code == -1
    finally:
        e.close()


# ------------------------------------------------------------------ into the U-Net
FULL_HW = (120, 200)


def test_step_chunks_reach_ultralight_infer_on_the_device(eng):
    """ltk_hubert_step's device chunks into ltk_ultralight_infer against the same chunks taken through hubert_features +
    feature2chunks on the host: byte for byte (both are the fp16 rows as float32).  Twice: the second step replays."""
    from livetalking_amd.avatars.audio_features.hubert import feature2chunks
    B, l = 16, 10
    frames, faces, coords = synth.ultralight_avatar(3, FULL_HW, seed=3)
    aid = eng.register_ultralight_avatar(synth.ultralight_state_dict(1234), faces, frames, coords, max_frames=B)
    try:
        for rep in range(3):
            pcm = H.speech((l + 2 * B + l) * 320, 30 + rep)
            d_chunks = torch.zeros(B, 16, 1024, dtype=torch.float32, device="cuda")
            eng.hubert_step(pcm, B, int(l / 2 * 2) - 8, d_chunks.data_ptr())
            host = np.stack(feature2chunks(eng.hubert_features(pcm), B, [4, 4], l / 2, 2))
            assert np.array_equal(d_chunks.cpu().numpy(), host)
            assert np.abs(host).max() > 0.1
            preds = []
            for feat in (d_chunks, torch.from_numpy(host).cuda()):
                pred = torch.zeros(B, 160, 160, 3, dtype=torch.uint8, device="cuda")
                eng.ultralight_infer([(aid, 1, B, feat.data_ptr(), pred.data_ptr())])
                preds.append(pred.cpu().numpy())
            assert np.array_equal(preds[0], preds[1])
    finally:
        eng.release_avatar(aid)


def test_plugin_behind_the_opt_in(sd2, tmp_path, monkeypatch):
    """LightReal with LTK_HUBERT_ENGINE=1 over a checkpoint directory written by save_pretrained from the seeded 2-layer model.  The
    engine-backed processor reads only the weights (its normalisation is part of the device program), so no tokenizer files are
    needed.  A speaking step puts batch_size device views on feat_queue; inference_batch on them equals inference_batch on the
    host chunks of the same audio; a silent step hands out device zeros."""
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from transformers import HubertModel
    from livetalking_amd.avatars import ultralight_avatar as ul
    from livetalking_amd.avatars.audio_features import hubert as hub
    model = HubertModel(H.config(2)).eval()
    model.load_state_dict({k: torch.as_tensor(v) for k, v in sd2.items()}, strict=True)
    model.save_pretrained(tmp_path / "models" / "hubert-large-ls960-ft")
    monkeypatch.chdir(tmp_path)
    monkeypatch.setenv("LTK_HUBERT_ENGINE", "1")
    B = 4
    opt = types.SimpleNamespace(fps=25, batch_size=B, l=10, r=10, sessionid=1)
    try:
        proc, none = ul.load_model(opt)
        assert isinstance(proc, hub.EngineAudio2Feature) and none is None and proc.engine is ul._engine(0)
        assert ul.load_model(opt)[0] is proc                 # an engine holds one model: a second load_model hands out the same processor
        frames, faces, coords = synth.ultralight_avatar(3, FULL_HW, seed=31)
        net = ul.UltralightNet(synth.ultralight_state_dict(1234), faces, frames, coords, max_frames=B)
        sess = ul.LightReal(opt, (proc, None), (net, frames, faces, coords))
        assert sess.engine is proc.engine
        rng = np.random.default_rng(2)
        seen = []
        step = proc.step
        proc.step = lambda pcm, *a, **k: (seen.append(np.array(pcm)), step(pcm, *a, **k))[1]
        for f in np.split(H.speech(2 * B * 320, 40), 2 * B):
            sess.asr.put_audio_frame(f.astype(np.float32), {})
        sess.asr.run_step()
        chunks = sess.asr.feat_queue.get_nowait()
        assert len(chunks) == B and all(isinstance(c, torch.Tensor) and c.is_cuda and c.shape == (16, 1024) for c in chunks)
        assert len(seen) == 1 and len(seen[0]) == (20 + 2 * B) * 320
        host = hub.feature2chunks(proc.get_hubert_from_16k_speech(seen[0]), B, [4, 4], opt.l / 2, 2)
        assert all(np.array_equal(c.cpu().numpy(), h) for c, h in zip(chunks, host)) and np.abs(host[0]).max() > 0.1
        a = torch.stack(sess.inference_batch(1, chunks)).cpu().numpy()
        b = torch.stack(sess.inference_batch(1, host)).cpu().numpy()
        assert a.shape == (B, 160, 160, 3) and np.array_equal(a, b)
        sess.asr.run_step()                                  # silent, but the step before it spoke: still extracted
        sess.asr.feat_queue.get_nowait()
        sess.asr.run_step()
        silent = sess.asr.feat_queue.get_nowait()
        assert len(seen) == 2 and all(c.is_cuda and not c.any() for c in silent)
        net.release()
    finally:
        with ul._engines_lock:
            e = ul._engines.pop(0, None)
        if e is not None:
            e.close()
