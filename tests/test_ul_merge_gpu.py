"""GPU tests of ltk_ultralight_infer_merged (csrc/ultralight.hip): the requests of one tick as one launch sequence per pass of the
merge plan - per avatar over the union of its requests' frames, or grouped over the frames of several avatars with the weights
chosen per image (csrc/ul_gconv.hip, the grouped kernels of csrc/dw_kernels.hip).  Avatars, requests, references and gates:
tests/ul_merge_cases.py.  Engines of their own (module scope)."""
from __future__ import annotations

import threading
import types

import numpy as np
import pytest

import ul_merge_cases as M
import ultralight_ref as U
from oracle import op_replay as R

pytestmark = pytest.mark.gpu

ARENA = 17


def _register(eng, av, max_frames):
    frames, faces, coords = M.bank(av)
    return eng.register_ultralight_avatar(M.state_dict(av), faces, frames, coords, max_frames=max_frames)


@pytest.fixture(scope="module")
def ul():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from livetalking_amd.engine import Engine
    eng = Engine(0)
    try:
        yield types.SimpleNamespace(eng=eng, aid={"a": _register(eng, "a", ARENA), "b": _register(eng, "b", 4)})
    finally:
        eng.close()


class Call:
    """The device side of a list of named requests: features up, a zeroed frame tensor per request."""

    def __init__(self, aid, names):
        import torch
        self.names = list(names)
        self.feat = [torch.from_numpy(M.feats(n)).cuda() for n in names]
        self.pred = [torch.zeros(M.REQUESTS[n][2], 160, 160, 3, dtype=torch.uint8, device="cuda") for n in names]
        self.reqs = [(aid[M.REQUESTS[n][0]], M.REQUESTS[n][1], M.REQUESTS[n][2], f.data_ptr(), p.data_ptr()) for n, f, p in zip(names, self.feat, self.pred)]

    def frames(self):
        return [p.cpu().numpy() for p in self.pred]


def _solo(eng, aid, name):
    c = Call(aid, [name])
    eng.ultralight_infer(c.reqs)
    return c.frames()[0]


class one_summation_order:
    """Knob SPLITK = 0 for the block: conv3 never splits the channel loop, so a conv's fp32 summation order no longer depends on the
    launch's frame count and a frame's bytes must not depend on which pass carried it."""

    def __enter__(self):
        from livetalking_amd.engine import Engine
        Engine.set_knob("SPLITK", 0)

    def __exit__(self, *exc):
        from livetalking_amd.engine import Engine
        Engine.set_knob("SPLITK", 1)


def _same_bytes_under_one_order(eng, aid, names, **kw):
    """Under SPLITK = 0 every request's frames in the merged call are byte-identical to its own call's."""
    with one_summation_order():
        c = Call(aid, names)
        eng.ultralight_infer_merged(c.reqs, **kw)
        for n, got in zip(names, c.frames()):
            assert np.array_equal(got, _solo(eng, aid, n)), f"{n}: merged and solo frames differ under SPLITK = 0"


def _solo_gates(eng, aid, names, frames, label):
    """The 'two launch shapes of the same kernels' gate for every request, every figure printed before the first assertion."""
    solos = [_solo(eng, aid, n) for n in names]
    figs = [U.frame_stats(got, solo) for got, solo in zip(frames, solos)]
    for n, (mx, _, share) in zip(names, figs):
        print(f"{label}{n} against its own call: {mx} LSB on {share:.4f} of the bytes")
    for n, got, solo in zip(names, frames, solos):
        M.gate_solo(n, got, solo, label)
    for n, got, solo in zip(names, frames, solos):                  # the same kernels in the same summation order
        assert np.array_equal(got, solo), f"{label}{n}: a per-avatar pass's frames differ from the request's own call"


def test_one_request_is_the_single_call(ul):
    """Bytes equal ltk_ultralight_infer's and no graph is added: the merged call replays the graph the plain call captured."""
    eng = ul.eng
    plain = Call(ul.aid, ["a2"])
    for _ in range(3):                                              # eager, captured, replayed
        eng.ultralight_infer(plain.reqs)
    g0 = eng.program_graph_count()
    for mode in (0, 1):
        merged = Call(ul.aid, ["a2"])
        rep = eng.ultralight_infer_merged(merged.reqs, mode=mode, report=True)
        assert rep["passes"] == [(M.PER_AVATAR, 2, ul.aid["a"])] and rep["avatars"] == 1 and rep["grouped"] == 0 and rep["frames"] == 2
        assert np.array_equal(merged.frames()[0], plain.frames()[0])
    assert eng.program_graph_count() == g0
    M.gate_float64("a2", plain.frames()[0])
    info = eng.ultralight_info()
    assert info["frames"] == ARENA == eng.ul_max_frames and info["grouped"] and info["bytes"] == ARENA * info["bytes_per_frame"] > 0


def test_one_avatar_three_requests_share_one_pass(ul):
    """Requests of 1, 2 and 3 frames of one avatar: one PER_AVATAR pass of 6 frames; every request's frames against float64, then
    against its own ltk_ultralight_infer call at <= 1 LSB on < 2 % of the bytes - and, since every conv of the pass sums a frame's
    channels in the order of that frame's own call (ul_conv_as_own_calls: conv3's split-K factor follows a launch's frame count, the
    1-, 2- and 3-frame calls and a plain 6-frame pass take different ones), byte for byte."""
    eng = ul.eng
    names = ["a1", "a2", "a3"]
    c = Call(ul.aid, names)
    rep = eng.ultralight_infer_merged(c.reqs, report=True)
    assert rep["passes"] == [(M.PER_AVATAR, 6, ul.aid["a"])] and rep["n_passes"] == 1 and rep["avatars"] == 1
    for n, got in zip(names, c.frames()):
        M.gate_float64(n, got)
    _same_bytes_under_one_order(eng, ul.aid, names)
    _solo_gates(eng, ul.aid, names, c.frames(), "one pass ")


def test_a_composition_of_call_sizes_is_captured_once(ul):
    """A per-avatar pass whose frames come from own calls of other sizes launches by the run lengths of those sizes: one captured graph
    per composition, whichever requests make it up; eager, captured and replayed frames are the same bytes."""
    eng = ul.eng
    g0 = eng.program_graph_count()
    runs = []
    for names in (["a1", "a2", "a3"], ["a1", "a2", "a3"], ["a1b", "a2", "a3"]):     # eager, captured, replayed
        c = Call(ul.aid, names)
        rep = eng.ultralight_infer_merged(c.reqs, report=True)
        assert rep["passes"] == [(M.PER_AVATAR, 6, ul.aid["a"])]
        runs.append(c.frames())
    assert eng.program_graph_count() == g0 + 1
    for got, first in zip(runs[1], runs[0]):
        assert np.array_equal(got, first)
    for n, got in zip(["a1b", "a2", "a3"], runs[2]):
        M.gate_float64(n, got, "replayed ")
    for names in (["a3", "a2", "a1"],) * 2:                         # another order is another composition
        c = Call(ul.aid, names)
        eng.ultralight_infer_merged(c.reqs)
    assert eng.program_graph_count() == g0 + 2
    _solo_gates(eng, ul.aid, ["a1b", "a2", "a3"], runs[2], "replayed ")
    _solo_gates(eng, ul.aid, ["a3", "a2", "a1"], c.frames(), "replayed ")


def test_two_avatars_share_one_grouped_pass(ul):
    eng = ul.eng
    names = ["a2", "b1", "a1"]                                      # a, b, a
    c = Call(ul.aid, names)
    rep = eng.ultralight_infer_merged(c.reqs, mode=2, report=True)
    assert rep["passes"] == [(M.GROUPED, 4, -1)] and rep["avatars"] == 2 and rep["grouped"] == 1
    for n, got in zip(names, c.frames()):
        M.gate_float64(n, got, "grouped ")
    assert not np.array_equal(c.frames()[1][0], c.frames()[2][0])
    # mode 1 on the same requests: one pass per avatar, the same frames by the gates of the per-avatar path
    c1 = Call(ul.aid, names)
    rep = eng.ultralight_infer_merged(c1.reqs, mode=1, report=True)
    assert rep["passes"] == [(M.PER_AVATAR, 3, ul.aid["a"]), (M.PER_AVATAR, 1, ul.aid["b"])]
    for n, got in zip(names, c1.frames()):
        M.gate_float64(n, got, "mode 1 ")
    # two compositions of three frames share one captured graph (the pass holds no avatar's address)
    g0 = eng.program_graph_count()
    x, y = Call(ul.aid, ["a2", "b1"]), Call(ul.aid, ["a1", "b2"])
    eng.ultralight_infer_merged(x.reqs, mode=2)                    # eager
    eng.ultralight_infer_merged(y.reqs, mode=2)                    # captured
    assert eng.program_graph_count() == g0 + 1
    x2, y2 = Call(ul.aid, ["a2", "b1"]), Call(ul.aid, ["a1", "b2"])
    eng.ultralight_infer_merged(x2.reqs, mode=2)                   # replayed, twice
    eng.ultralight_infer_merged(y2.reqs, mode=2)
    assert eng.program_graph_count() == g0 + 1
    for a, b in ((x, x2), (y, y2)):
        for n, f0, f1 in zip(a.names, a.frames(), b.frames()):
            assert np.array_equal(f0, f1), n                        # eager / captured and replayed: the same bytes
            M.gate_float64(n, f1, "replayed ")
    _same_bytes_under_one_order(eng, ul.aid, names, mode=1)        # (last: a knob change drops every captured graph)


def test_release_then_register_leaves_no_stale_entry(ul):
    """b is released after grouped calls and c registered over b's bank: the same composition gives c's frames - no stale table entry,
    no stale graph (the grouped graph survives the release: it holds no avatar's address)."""
    eng = ul.eng
    for _ in range(3):
        before = Call(ul.aid, ["a1", "b1"])
        eng.ultralight_infer_merged(before.reqs, mode=2)
    M.gate_float64("b1", before.frames()[1])
    eng.release_avatar(ul.aid["b"])                                # (drops b's own per-avatar graphs)
    g0 = eng.program_graph_count()
    from livetalking_amd._lib import LtkError
    with pytest.raises(LtkError) as ex:
        eng.ultralight_infer_merged(before.reqs, mode=2)
    assert ex.value.code == -3 and "request 1" in str(ex.value)
    ul.aid["c"] = _register(eng, "c", 4)
    ul.aid["b"] = _register(eng, "b", 4)                           # (b again, for the tests behind this one)
    after = Call(ul.aid, ["a1", "c1"])
    rep = eng.ultralight_infer_merged(after.reqs, mode=2, report=True)
    assert rep["passes"] == [(M.GROUPED, 2, -1)]
    assert eng.program_graph_count() == g0                          # the two-frame grouped graph is still the one captured above
    M.gate_float64("a1", after.frames()[0])
    M.gate_float64("c1", after.frames()[1])
    with pytest.raises(AssertionError):
        M.gate_float64("b1", after.frames()[1])                     # not b's frames any more


def test_op_by_op_replay_of_a_grouped_pass(ul):
    """replay_ultralight over a captured grouped pass of two avatars, B = 2 + 1, per avatar on that avatar's frames: 0 failures and
    0 uncovered ops under the gates of oracle/op_replay.py.  outc.conv has no float tap on the bank path; the frames stand for it
    (tests/test_op_replay_gpu.py), held here by the float64 frame gate."""
    import torch
    eng = ul.eng
    names = ["a2", "b1"]
    c = Call(ul.aid, names)
    eng.debug_capture(True)
    try:
        rep = eng.ultralight_infer_merged(c.reqs, mode=2, report=True)
        assert rep["passes"] == [(M.GROUPED, 3, -1)]
        at = 0
        for n, got in zip(names, c.frames()):
            av, _, k, _ = M.REQUESTS[n]
            lo, hi = at, at + k
            at = hi

            def fetch(name, ref, lo=lo, hi=hi):
                if name == "outc.conv":
                    return None
                return torch.from_numpy(eng.debug_get(name, (3,) + tuple(ref.shape[1:]))[lo:hi]).to(ref.dtype)

            rp = U.replay_ultralight(M.state_dict(av), M.img6_of(n), M.feats(n), fetch, fused={"outc.conv": "frames"})
            ops = eng.ultralight_ops(ul.aid[av])
            assert [o for o, _ in ops] == U.op_names()
            miss = R.uncovered(ops, [r["name"] for r in rp.records] + ["frames"], {"outc.conv": "frames"})
            assert not miss, f"{n}: ops not compared: {miss}"
            bad = R.failures(rp.records)
            assert not bad, f"{n}:\n" + "\n".join(bad)
            M.gate_float64(n, got, "captured ")
    finally:
        eng.debug_capture(False)


@pytest.mark.parametrize("knob", [0, 1])
def test_scheduler_end_to_end(ul, knob):
    """Four threads, two avatars, one fixed window: the merge is certain.  UL_GROUPED off: each avatar's requests share a per-avatar
    pass and are held to float64 and then to their solo results; on: one grouped pass, held to float64."""
    from livetalking_amd import scheduler
    from livetalking_amd.engine import Engine
    eng = ul.eng
    names = ["a2", "a3", "b1", "b2"]
    solo = {n: _solo(eng, ul.aid, n) for n in names}
    reports = []
    real = eng.ultralight_infer_merged
    eng.ultralight_infer_merged = lambda reqs, **kw: reports.append(real(reqs, report=True))
    Engine.set_knob("UL_GROUPED", knob)
    sch = scheduler.CoalescingScheduler(eng, 400.0, kind="ultralight")
    try:
        calls = {n: Call(ul.aid, [n]) for n in names}
        errs = []

        def run(n):
            try:
                sch.infer(*calls[n].reqs[0])
            except Exception as ex:  # noqa: BLE001
                errs.append(ex)

        ts = [threading.Thread(target=run, args=(n,)) for n in names]
        for t in ts:
            t.start()
        for t in ts:
            t.join(timeout=60)
            assert not t.is_alive()
    finally:
        sch.close()
        Engine.set_knob("UL_GROUPED", 0)
        del eng.ultralight_infer_merged
    assert not errs, errs
    assert sch.stats["requests"] == 4 and sch.stats["calls"] < sch.stats["requests"], sch.stats
    paths = {p for rep in reports for p, _, _ in rep["passes"]}
    if sch.stats["calls"] == 1:
        assert paths == ({M.GROUPED} if knob else {M.PER_AVATAR}) and reports[0]["frames"] == 8
    for n in names:
        M.gate_float64(n, calls[n].frames()[0], "scheduler grouped " if knob else "scheduler ")
    if not (knob and sch.stats["calls"] == 1):
        for n in names:
            mx, _, share = U.frame_stats(calls[n].frames()[0], solo[n])
            print(f"scheduler {n} against its own call: {mx} LSB on {share:.4f} of the bytes")
        for n in names:
            M.gate_solo(n, calls[n].frames()[0], solo[n], "scheduler ")


# ------------------------------------------------------------------ chunking: an engine whose arena holds four frames
@pytest.fixture(scope="module")
def small():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from livetalking_amd.engine import Engine
    eng = Engine(0)
    try:
        yield types.SimpleNamespace(eng=eng, aid={"a": _register(eng, "a", 4), "b": _register(eng, "b", 2)})
    finally:
        eng.close()


def test_seven_frames_through_an_arena_of_four(small):
    """Both paths cut 7 frames into passes of 4 + 3, a request split across them; the frames are held as in the unchunked tests (a2's
    two frames ride in different passes and still equal its own 2-frame call's)."""
    eng = small.eng
    assert eng.ul_max_frames == 4
    names = ["a3", "a2", "a1", "a1b"]                               # per avatar: 3 + 1 | 1 + 1 + 1
    c = Call(small.aid, names)
    rep = eng.ultralight_infer_merged(c.reqs, report=True)
    assert rep["passes"] == [(M.PER_AVATAR, 4, small.aid["a"]), (M.PER_AVATAR, 3, small.aid["a"])]
    per_avatar = (names, c.frames())
    for n, got in zip(names, c.frames()):
        M.gate_float64(n, got, "chunked ")
    _same_bytes_under_one_order(eng, small.aid, names)
    names = ["a3", "b2", "a2"]                                      # grouped: 3 + 1 | 1 + 2
    c = Call(small.aid, names)
    rep = eng.ultralight_infer_merged(c.reqs, mode=2, report=True)
    assert rep["passes"] == [(M.GROUPED, 4, -1), (M.GROUPED, 3, -1)] and rep["n_passes"] == 2 and rep["frames"] == 7
    for n, got in zip(names, c.frames()):
        M.gate_float64(n, got, "chunked grouped ")
    _solo_gates(eng, small.aid, per_avatar[0], per_avatar[1], "chunked ")
