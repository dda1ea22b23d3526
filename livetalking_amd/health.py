"""First calls on a real checkpoint: the plugin side of the fp16 headroom watch (include/ltk.h: ltk_health_watch).

`LTK_HEALTH_WATCH=N` arms the engine's watch for the first N inference calls of every program a plugin loads, at the load;
`opt.health_watch = N` arms it when the first session (or, for the Ultralight family, load_model(opt)) brings the opt, for the N calls
from then on; default 0: nothing is armed, nothing is called.  A `HealthMonitor` owns one (engine, program[, avatar]) watch.  The plugin's hot
call checks one attribute (`monitor.pending`); the first call after the window has closed reads the report once and logs one line:

  * clean: the op with the least headroom and its max |x| / limit;
  * otherwise a loud warning that lists, in program order, every op with values at the limit of its type or non-finite values - a
    checkpoint whose activations reach the fp16 limit renders wrong frames and nothing else reports it.

The report stays available (`monitor.report()`, the plugins' `.health()`).
"""
from __future__ import annotations

import logging
import os
import threading

logger = logging.getLogger("livetalking_amd.health")


def watch_calls(opt=None) -> int:
    """Calls to watch after a load: opt.health_watch, else LTK_HEALTH_WATCH, else 0 (off)."""
    v = getattr(opt, "health_watch", None) if opt is not None else None
    if v is None:
        v = os.environ.get("LTK_HEALTH_WATCH", "0")
    try:
        return max(0, int(v))
    except (TypeError, ValueError):
        return 0


def dirty_ops(ops):
    """The ops of a report with values at the limit of their type or non-finite values, in program order."""
    return [o for o in ops if o["at_limit"] > 0 or o["nonfinite"] > 0]


def least_headroom(ops):
    """The observed op whose largest |x| is closest to its type's limit (None: nothing was observed)."""
    seen = [o for o in ops if o["observed"] and o["elements"] > 0]
    return max(seen, key=lambda o: o["max_abs"] / o["limit"]) if seen else None


def format_line(program: str, ops, calls_seen: int):
    """(clean, text): the one log line of a closed window."""
    bad = dirty_ops(ops)
    if not bad:
        o = least_headroom(ops)
        if o is None:
            return True, f"health watch [{program}]: {calls_seen} calls watched, no op output was observed"
        return True, (f"health watch [{program}]: {calls_seen} calls clean; least headroom at {o['name']}: max |x| {o['max_abs']:.6g} = "
                      f"{100.0 * o['max_abs'] / o['limit']:.3g} % of {o['limit']:g}")
    rows = "; ".join(f"{o['name']}: {o['at_limit']} at the limit, {o['nonfinite']} non-finite of {o['elements']}" for o in bad)
    return False, (f"HEALTH WATCH [{program}]: ACTIVATIONS REACH THE LIMIT OF THEIR NUMBER FORMAT in {len(bad)} op(s) over {calls_seen} watched calls "
                   f"- the frames are not the checkpoint's: {rows}")


def format_table(program: str, ops) -> str:
    """The whole report as a table (scripts/checkpoint_health.py)."""
    head = f"{'op':<58}{'obs':>4}{'fmt':>6}{'elements':>13}{'near':>10}{'at limit':>10}{'nonfinite':>10}{'max |x|':>12}{'of limit':>10}"
    lines = [f"[{program}]", head]
    for o in ops:
        frac = f"{100.0 * o['max_abs'] / o['limit']:.3g} %" if o["observed"] else "-"
        lines.append(f"{o['name'][:57]:<58}{o['observed']:>4}{'e4m3' if o['q8'] else 'fp16':>6}{o['elements']:>13}{o['near_limit']:>10}{o['at_limit']:>10}"
                     f"{o['nonfinite']:>10}{o['max_abs']:>12.6g}{frac:>10}")
    return "\n".join(lines)


class HealthMonitor:
    """One armed watch.  `pending` is the cheap flag of the hot call: `if mon.pending: mon.tick()` in front of every engine call."""

    def __init__(self, engine, program: str, calls: int, avatar_id: int = -1, log=None):
        self.engine, self.program, self.calls, self.avatar_id = engine, program, int(calls), int(avatar_id)
        self.log = log or logger
        self.pending = False
        self.clean = None            # True / False once the window's line has been logged
        self._issued = 0             # calls of ours since the watch was armed
        self._recheck_at = 0
        self._lock = threading.Lock()
        if self.calls > 0:
            engine.health_watch(program, self.calls, avatar_id)
            self._recheck_at = self.calls
            self.pending = True

    def tick(self):
        """In front of an engine call.  The first one behind the window reads the report and logs its line; when engine calls carried
        several of ours (a scheduler coalescing sessions) the window is still open: looked at again after what is left of it."""
        with self._lock:
            if not self.pending:
                return
            if self._issued < self._recheck_at:
                self._issued += 1
                return
            ops, seen, left = self.engine.health_report(self.program, self.avatar_id)
            if left > 0:
                self._recheck_at = self._issued + left
                self._issued += 1
                return
            self.pending = False
            self.clean, text = format_line(self.program, ops, seen)
            (self.log.info if self.clean else self.log.warning)(text)

    def report(self):
        """(ops, calls_seen, calls_left) as Engine.health_report returns them."""
        return self.engine.health_report(self.program, self.avatar_id)


_monitors_lock = threading.Lock()


def lookup(engine, program: str, avatar_id: int = -1):
    """The engine's monitor of (program, avatar) if one was armed, else None.  Arms nothing (the plugins' .health())."""
    return getattr(engine, "__dict__", {}).get("_health_monitors", {}).get((program, int(avatar_id)))


def monitor_for(engine, program: str, opt=None, avatar_id: int = -1):
    """The engine's monitor of (program, avatar).  The first caller that asks for a watch - LTK_HEALTH_WATCH at load_model, or a
    session's opt.health_watch later - arms it; until then nothing is remembered, so a load without the knob does not keep a later
    session's opt from arming.  An armed monitor is returned as it is (one window per engine and program).  None: no watch."""
    with _monitors_lock:
        mons = engine.__dict__.setdefault("_health_monitors", {})
        key = (program, int(avatar_id))
        mon = mons.get(key)
        if mon is None:
            mon = arm(engine, program, opt, avatar_id)
            if mon is not None:
                mons[key] = mon
        return mon


def arm(engine, program: str, opt=None, avatar_id: int = -1, log=None):
    """A monitor for `program` when watching is asked for (watch_calls) and the engine has the entry, else None."""
    n = watch_calls(opt)
    if n <= 0 or not hasattr(engine, "health_watch"):
        return None
    return HealthMonitor(engine, program, n, avatar_id, log)
