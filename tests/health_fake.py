"""A stand-in engine for the plugin side of the headroom watch (livetalking_amd/health.py): it keeps the window the way the engine
does - armed for N engine calls, one engine call counts once whatever it carries - and counts how often it is asked."""


def op(name, max_abs=1.0, at_limit=0, nonfinite=0, observed=1, q8=0, elements=1000, near_limit=None, type=0):
    return {"name": name, "type": type, "observed": observed, "q8": q8, "elements": elements if observed else 0, "at_limit": at_limit,
            "near_limit": at_limit if near_limit is None else near_limit, "nonfinite": nonfinite, "max_abs": float(max_abs),
            "limit": 448.0 if q8 else 65504.0}


class StandInEngine:
    def __init__(self, ops):
        self.ops = ops
        self.left = self.seen = 0
        self.watches = []           # (program, calls, avatar_id) of every health_watch
        self.reports = 0            # health_report calls
        self.calls = 0              # engine calls

    def health_watch(self, program, calls, avatar_id=-1):
        self.watches.append((program, calls, avatar_id))
        self.left, self.seen = calls, 0

    def health_report(self, program, avatar_id=-1):
        self.reports += 1
        return list(self.ops), self.seen, self.left

    def infer(self, nreq=1):
        """One engine call carrying nreq sessions' requests."""
        self.calls += 1
        if self.left > 0:
            self.left -= 1
            self.seen += 1


class Log:
    def __init__(self):
        self.lines = []

    def info(self, text):
        self.lines.append(("info", text))

    def warning(self, text):
        self.lines.append(("warning", text))
