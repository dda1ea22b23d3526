"""CPU: the headroom watch without a GPU - the numpy model of the scan held to hand-built tensors, the ABI rows and the refusals that
need no device, the plugin-side window logic over a stand-in engine, and the report's formatting."""
import ctypes as C
import logging

import numpy as np
import pytest

import health_cases as HC
import health_fake as HF


def _f16(vals):
    return np.asarray(vals, dtype=np.float16).view(np.uint16)


def _tensor16(codes):
    x = np.zeros((1, 1, 2, 16), dtype=np.uint16)
    x.reshape(-1)[: len(codes)] = np.asarray(codes, dtype=np.uint16)
    return x


# ------------------------------------------------------------------ the model against hand-built tensors
def test_model_counts_both_signs_of_the_limit_and_infinities():
    x = _tensor16([0x7BFF, 0xFBFF, 0x7C00, 0xFC00, 0x3C00])          # +-65504, +-inf, 1.0
    m = HC.scan_model(x, 0, 1, False)
    assert (m["elements"], m["at_limit"], m["near_limit"], m["nonfinite"]) == (32, 2, 2, 2)
    assert m["max_abs"] == np.float32(65504.0) and m["limit"] == 65504.0


def test_model_counts_nans_with_payloads_as_nonfinite_only():
    x = _tensor16([0x7C01, 0xFFFF, 0x7E00, 0xFD55, 0x4000])          # signalling / quiet NaNs of both signs, 2.0
    m = HC.scan_model(x, 0, 1, False)
    assert (m["at_limit"], m["near_limit"], m["nonfinite"]) == (0, 0, 4)
    assert m["max_abs"] == np.float32(2.0)


def test_model_takes_a_negative_maximum_and_subnormals():
    x = _tensor16(list(_f16([1.5, -40000.0, 3.0])) + [0x0001, 0x83FF])      # -40000 rounds to -40000 (top binade); two subnormals
    m = HC.scan_model(x, 0, 1, False)
    assert (m["at_limit"], m["near_limit"], m["nonfinite"]) == (0, 1, 0)
    assert m["max_abs"] == np.float32(np.float16(-40000.0)) * -1
    sub = HC.scan_model(_tensor16([0x0001, 0x83FF]), 0, 1, False)
    assert sub["max_abs"] == np.float32(1023 * 2.0 ** -24) and sub["near_limit"] == 0
    assert HC.scan_model(_tensor16([]), 0, 1, False)["max_abs"] == 0.0


def test_model_top_binade_boundaries():
    x = _tensor16([0x77FF, 0x7800, 0xF800, 0x7BFE])                  # 32752 (below), +-32768 (first of the binade), 65472
    m = HC.scan_model(x, 0, 1, False)
    assert (m["at_limit"], m["near_limit"], m["nonfinite"]) == (0, 3, 0)
    assert m["max_abs"] == np.float32(65472.0)


def test_model_e4m3_special_codes():
    x = np.zeros((1, 1, 1, 32), dtype=np.uint8)
    x.reshape(-1)[:7] = [0x7E, 0xFE, 0x7F, 0xFF, 0x78, 0x77, 0x01]   # +-448, the two NaNs, 256, 240, the smallest subnormal
    m = HC.scan_model(x, 0, 1, True)
    assert (m["elements"], m["at_limit"], m["near_limit"], m["nonfinite"]) == (32, 2, 3, 2)
    assert m["max_abs"] == np.float32(448.0) and m["limit"] == 448.0
    assert HC.decode_e4m3(0x77) == 240.0 and HC.decode_e4m3(0x78) == 256.0 and HC.decode_e4m3(0x01) == np.float32(2.0 ** -9)
    assert HC.decode_e4m3(0x38) == 1.0 and HC.decode_e4m3(0xB8) == 1.0
    torch = pytest.importorskip("torch")
    if hasattr(torch, "float8_e4m3fn"):                              # every finite code against torch's decoder
        codes = np.arange(0, 0x7F, dtype=np.uint8)
        want = torch.from_numpy(codes).view(torch.float8_e4m3fn).to(torch.float32).numpy()
        assert all(HC.decode_e4m3(int(c)) == w for c, w in zip(codes, want))


def test_model_ignores_blocks_outside_the_view():
    for q8 in (False, True):
        codes = HC.build_tensor(2, 5, 2, 2, 63, q8, seed=3)
        m = HC.scan_model(codes, 2, 2, q8)
        assert m["elements"] == 2 * 2 * 63 * (32 if q8 else 16)
        assert (m["at_limit"], m["near_limit"], m["nonfinite"]) == (2, 3, 2)      # the five planted values and nothing of the neighbours


# ------------------------------------------------------------------ ABI rows, refusals without a device
def test_abi_rows_and_struct_layout():
    from livetalking_amd import _lib
    for name in ("ltk_health_watch", "ltk_health_report", "ltk_health_scan"):
        assert name in _lib.SYMBOLS
    assert C.sizeof(_lib.HealthOp) == 64 + 3 * 4 + 4 + 4 * 8 + 2 * 4      # char[64], 3 ints, padding, 4 counters, 2 floats
    assert _lib.HealthOp.elements.offset == 80 and _lib.HealthOp.max_abs.offset == 112
    assert [_lib.HEALTH_PROGRAMS[k] for k in ("wav2lip", "musetalk", "ultralight", "whisper", "hubert")] == [0, 1, 2, 3, 4]


def test_entries_refuse_bad_arguments_before_anything_else():
    from livetalking_amd import _lib
    lib = _lib.load()
    rec = _lib.HealthOp()
    ops = (_lib.HealthOp * 4)()
    n = C.c_int()
    assert lib.ltk_health_watch(None, 0, -1, 1) == -1
    assert lib.ltk_health_watch(None, 99, -1, 1) == -1
    assert lib.ltk_health_watch(None, 0, -1, -1) == -1
    assert lib.ltk_health_report(None, 0, -1, ops, 4, C.byref(n), None, None) == -1
    assert lib.ltk_health_scan(None, None, 1, 1, 0, 1, 1, 0, C.byref(rec)) == -1
    assert b"null" in lib.ltk_last_error() or b"bad" in lib.ltk_last_error()


def test_engine_wrapper_refuses_an_unknown_program_name():
    from livetalking_amd.engine import Engine
    with pytest.raises(ValueError):
        Engine._health_program("wav2lips")
    assert Engine._health_program("hubert") == 4 and Engine._health_program(2) == 2


# ------------------------------------------------------------------ the plugin side over a stand-in engine
CLEAN = [HF.op("a", 3.0), HF.op("b", 900.0), HF.op("fused", 0.0, observed=0), HF.op("c", 20.0, q8=1), HF.op("d", 70.0)]
DIRTY = [HF.op("a", 3.0), HF.op("b", 65504.0, at_limit=7), HF.op("c", 5.0), HF.op("d", 65504.0, nonfinite=2), HF.op("e", 448.0, at_limit=1, q8=1)]


def _drive(mon, eng, calls):
    for _ in range(calls):
        if mon is not None and mon.pending:
            mon.tick()
        eng.infer()


def test_window_counts_calls_and_the_report_is_read_once():
    from livetalking_amd.health import HealthMonitor
    eng, log = HF.StandInEngine(CLEAN), HF.Log()
    mon = HealthMonitor(eng, "wav2lip", 3, log=log)
    assert eng.watches == [("wav2lip", 3, -1)] and mon.pending
    _drive(mon, eng, 3)
    assert eng.reports == 0 and log.lines == [] and mon.pending          # the window is open for exactly its three calls
    _drive(mon, eng, 5)
    assert eng.reports == 1 and not mon.pending and mon.clean is True
    assert len(log.lines) == 1 and log.lines[0][0] == "info"
    text = log.lines[0][1]
    assert "wav2lip" in text and "3 calls" in text
    assert "at c:" in text and "4.46 %" in text and "448" in text         # least headroom: 20 / 448, not 900 / 65504


def test_window_follows_engine_calls_when_requests_are_coalesced():
    from livetalking_amd.health import HealthMonitor
    eng, log = HF.StandInEngine(CLEAN), HF.Log()
    mon = HealthMonitor(eng, "musetalk", 4, log=log)
    for _ in range(2):                       # four inference_batch calls of two sessions travel as two engine calls
        mon.tick(); mon.tick()
        eng.infer(nreq=2)
    assert eng.seen == 2 and eng.left == 2
    mon.tick()                               # the fifth looks: the engine's window is still open for two calls
    assert eng.reports == 1 and mon.pending and log.lines == []
    eng.infer(); mon.tick(); eng.infer(); mon.tick()
    assert eng.reports == 2 and not mon.pending and len(log.lines) == 1 and "4 calls" in log.lines[0][1]


def test_dirty_report_warns_and_lists_ops_in_program_order():
    from livetalking_amd.health import HealthMonitor
    eng, log = HF.StandInEngine(DIRTY), HF.Log()
    mon = HealthMonitor(eng, "ultralight", 1, avatar_id=7, log=log)
    assert eng.watches == [("ultralight", 1, 7)]
    _drive(mon, eng, 3)
    assert eng.reports == 1 and mon.clean is False
    (level, text), = log.lines
    assert level == "warning" and "ultralight" in text and text == text.replace("\n", "")
    assert text.index("b: 7 at the limit") < text.index("d: 0 at the limit, 2 non-finite") < text.index("e: 1 at the limit")
    assert " a:" not in text and " c:" not in text and "3 op(s)" in text


def test_unset_knob_arms_nothing_and_calls_nothing(monkeypatch):
    from livetalking_amd import health
    monkeypatch.delenv("LTK_HEALTH_WATCH", raising=False)
    eng = HF.StandInEngine(CLEAN)
    assert health.watch_calls() == 0 and health.watch_calls(object()) == 0
    assert health.monitor_for(eng, "wav2lip") is None and health.arm(eng, "whisper") is None
    _drive(health.monitor_for(eng, "wav2lip"), eng, 4)
    assert eng.watches == [] and eng.reports == 0


def test_knob_and_opt_arm_once_per_engine_and_program(monkeypatch):
    from livetalking_amd import health
    monkeypatch.setenv("LTK_HEALTH_WATCH", "2")
    eng = HF.StandInEngine(CLEAN)
    m = health.monitor_for(eng, "hubert")
    assert m is health.monitor_for(eng, "hubert") and eng.watches == [("hubert", 2, -1)]
    monkeypatch.setenv("LTK_HEALTH_WATCH", "junk")
    assert health.watch_calls() == 0

    class Opt:
        health_watch = 5
    assert health.watch_calls(Opt()) == 5
    eng2 = HF.StandInEngine(CLEAN)
    assert health.monitor_for(eng2, "wav2lip", Opt()).calls == 5
    assert health.monitor_for(object.__new__(type("NoEntry", (), {})), "wav2lip", Opt()) is None      # an engine without the entry


def test_opt_arms_after_a_load_without_the_knob(monkeypatch):
    """The plugins' order: load_model asks without an opt (knob unset: nothing armed, nothing remembered), the session's __init__ asks
    again with its opt - that call must arm.  An armed monitor is then the one every later caller gets."""
    from livetalking_amd import health
    monkeypatch.delenv("LTK_HEALTH_WATCH", raising=False)

    class Opt:
        health_watch = 3
    for program, aid in (("wav2lip", -1), ("musetalk", -1), ("whisper", -1), ("hubert", -1), ("ultralight", 5)):
        eng = HF.StandInEngine(CLEAN)
        assert health.monitor_for(eng, program, None, aid) is None and eng.watches == []
        assert health.lookup(eng, program, aid) is None
        m = health.monitor_for(eng, program, Opt(), aid)
        assert m is not None and m.pending and eng.watches == [(program, 3, aid)]
        assert health.monitor_for(eng, program, None, aid) is m and health.monitor_for(eng, program, Opt(), aid) is m
        assert health.lookup(eng, program, aid) is m and eng.watches == [(program, 3, aid)]


def test_opt_reaches_the_audio_front_ends_and_the_ultralight_avatar(monkeypatch):
    monkeypatch.delenv("LTK_HEALTH_WATCH", raising=False)
    from livetalking_amd.avatars.audio_features.hubert import EngineAudio2Feature, HubertASR
    from livetalking_amd.avatars.audio_features.whisper import Audio2Feature, WhisperASR
    from livetalking_amd.avatars.ultralight_avatar import UltralightNet

    class Opt:
        health_watch = 2
        batch_size = 2
        fps = 50
        l = 10
        r = 10

    class Eng(HF.StandInEngine):
        torch_device = "cpu"

        def load_whisper(self, sd):
            pass

        def load_hubert(self, sd):
            pass

        def register_ultralight_avatar(self, *a, **k):
            return 9
    eng = Eng(CLEAN)
    ap = Audio2Feature(eng, {"w": 0})
    assert ap.health_monitor is None and ap.health() is None and eng.watches == []
    asr = WhisperASR(Opt(), None, ap)
    assert asr._health is ap.health_monitor is not None and eng.watches == [("whisper", 2, -1)]
    hp = EngineAudio2Feature(eng, {"w": 0})
    assert hp.health_monitor is None
    HubertASR(Opt(), None, hp)
    assert hp.health_monitor is not None and eng.watches[-1] == ("hubert", 2, -1)
    assert EngineAudio2Feature(Eng(CLEAN), {"w": 0}, opt=Opt()).health_monitor is not None      # ultralight's load_model(opt)
    net = UltralightNet({}, [], [], [], engine=eng, max_frames=2)
    assert net.avatar_id() == 9 and net.health_monitor is None and net.health() is None
    assert net.avatar_id(Opt()) == 9 and net.health_monitor is not None and eng.watches[-1] == ("ultralight", 2, 9)


def test_plugin_model_objects_expose_the_report_and_arm_nothing(monkeypatch):
    monkeypatch.setenv("LTK_HEALTH_WATCH", "1")
    from livetalking_amd import health
    from livetalking_amd.avatars.wav2lip_avatar import Wav2LipModel
    eng = HF.StandInEngine(CLEAN)
    eng.device = 0
    model = Wav2LipModel(eng)
    assert model.health() == [None] and eng.watches == []              # a getter: it arms nothing, knob or not
    health.monitor_for(eng, "wav2lip")                                 # what load_model does
    (ops, seen, left), = model.health()
    assert [o["name"] for o in ops] == [o["name"] for o in CLEAN] and (seen, left) == (0, 1) and len(eng.watches) == 1


# ------------------------------------------------------------------ formatting
def test_format_line_and_table():
    from livetalking_amd import health
    clean, text = health.format_line("whisper", CLEAN, 2)
    assert clean and text.startswith("health watch [whisper]: 2 calls clean; least headroom at c: max |x| 20 = 4.46 % of 448")
    clean, text = health.format_line("whisper", [HF.op("x", observed=0)], 2)
    assert clean and "no op output was observed" in text
    clean, text = health.format_line("hubert", DIRTY, 1)
    assert not clean and text.startswith("HEALTH WATCH [hubert]:")
    table = health.format_table("wav2lip", DIRTY).splitlines()
    assert table[0] == "[wav2lip]" and len(table) == 2 + len(DIRTY)
    assert table[1].split()[:3] == ["op", "obs", "fmt"]
    row = table[3].split()
    assert row[0] == "b" and row[2] == "fp16" and row[5] == "7" and row[-2:] == ["100", "%"]
    assert "-" == health.format_table("x", [HF.op("u", observed=0)]).splitlines()[2].split()[-1]
    assert logging.getLogger("livetalking_amd.health") is health.logger
