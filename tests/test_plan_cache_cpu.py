"""The plan cache behind BA_rgbd_droid (batrack_amd/backend/ba.py: PlanCache) as a policy, on CPU int64 tensors: `Plan`, `Stepper`
and the waits for the index tensors are replaced by fakes that answer as scripted and record a trace of
(operation, fixedp, outcome); `Driver.call` makes the cache's calls in the order BA_rgbd_droid makes them.  No GPU, no built library.

The expected traces and observations (tests/golden/plan_cache_traces.json) were recorded by running these same scenarios through
the functions this class replaced (`_plan_for`, `_confirm`, `_preshift`, `prefetch_plan` over the module's globals), not through
PlanCache: a scenario passes when the cache decides, builds, binds, settles and destroys exactly as they did.  What a
scenario is there to show is asserted beside that in words of its own."""
import contextlib
import json
import os

import pytest
import torch

from batrack_amd.backend import ba

N_BUF, P_TOT, E = 16, 64, 8
DEV = torch.device("cuda:0")                 # (a name for the keys only: nothing here touches a device)
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "plan_cache_traces.json")


def lst(k):
    """A list of 8 edges, distinct per k."""
    return tuple(torch.arange(E, dtype=torch.int64) + k + d for d in (0, 1, 2))


class World:
    """The trace, and the scripted answers: script[op] is a list consumed from the front, one answer per call of `op`; where it is
    empty the operation succeeds."""

    def __init__(self):
        self.trace, self.script = [], {}

    def log(self, op, fixedp, outcome):
        self.trace.append((op, fixedp, outcome))

    def answer(self, op, default=True):
        q = self.script.get(op)
        a = q.pop(0) if q else default
        if isinstance(a, BaseException):
            raise a
        return a

    def ops(self, start=0):
        return [t[0] for t in self.trace[start:]]


def fakes(w):
    class FakePlan:
        speculative = unbound = False

        def __init__(self, ii, jj, kk, n_buf, p_tot, fixedp, sync=True, made="Plan"):
            if made == "Plan":
                assert sync is False                                   # (the cache has waited itself, once)
                w.answer("Plan")
            self.info = dict(E=ii.numel() if ii is not None else E, n_buf=int(n_buf), p_tot=int(p_tot), fixedp=int(fixedp))
            self.made, self.uploaded = made, True
            if made == "Plan":
                w.log("Plan", self.info["fixedp"], "built")

        @classmethod
        def shifted_any(cls, srcs, ii, jj, kk, n_buf, p_tot, fixedp, sync=True):
            assert sync is False and 1 <= len(srcs) <= 3
            src = srcs[0] if w.answer("shifted_any") else None
            w.log("shifted_any", int(fixedp), [[s.info["fixedp"] for s in srcs], src.info["fixedp"] if src else None])
            return (cls(ii, jj, kk, n_buf, p_tot, fixedp, made="shifted_any"), src) if src else (None, None)

        @classmethod
        def shifted_spec(cls, src, ii, jj, kk, n_buf, p_tot, fixedp):
            ok = w.answer("shifted_spec")
            w.log("shifted_spec", int(fixedp), src.info["fixedp"] if ok else "declined")
            if not ok:
                return None
            pl = cls(ii, jj, kk, n_buf, p_tot, fixedp, made="shifted_spec")
            pl.speculative = True
            return pl

        @classmethod
        def preshift(cls, src, df):
            assert not src.speculative
            ok = w.answer("preshift")
            w.log("preshift", src.info["fixedp"] + df, src.info["fixedp"] if ok else "declined")
            if not ok:
                return None
            pl = cls(None, None, None, src.info["n_buf"], src.info["p_tot"], src.info["fixedp"] + df, made="preshift")
            pl.speculative = pl.unbound = True
            return pl

        def bind(self, ii, jj, kk, n_buf, p_tot, fixedp):
            ok = bool(self.unbound and w.answer("bind"))
            w.log("bind", self.info["fixedp"], ok)
            if ok:
                self.unbound = False
            return ok

        def confirm(self):
            try:
                ok = bool(w.answer("confirm"))
            except BaseException:
                w.log("confirm", self.info["fixedp"], "raised")
                raise
            w.log("confirm", self.info["fixedp"], ok)
            if ok:
                self.speculative = False
            return ok

        def __del__(self):
            if "made" in self.__dict__:
                w.log("destroy", self.info["fixedp"], self.made)

    class FakeStepper:
        def __init__(self, plan, device, ws=None):
            self.plan, self.device = plan, device
            self.ws = ws if ws is not None else object()
            w.log("Stepper", plan.info["fixedp"], "shared workspace" if ws is not None else "own workspace")

    return FakePlan, FakeStepper


class Driver:
    """One fresh cache over fakes, called as BA_rgbd_droid calls it."""

    def __init__(self, setenv, patch):
        self.w, self.setenv, self.patch = World(), setenv, patch
        self.cache = ba.PlanCache()
        self.install(*fakes(self.w))

    def install(self, plan, stepper):
        w = self.w

        class Waited:                                  # a stream or an event of the caller's
            def __init__(self, what):
                self.what = what

            def record(self, stream):
                pass

            def synchronize(self):
                w.log("wait", None, self.what)

        class FakeCuda:
            Event = staticmethod(lambda: Waited("event"))
            current_stream = staticmethod(lambda dev=None: Waited("stream"))
            device = stream = staticmethod(lambda x: contextlib.nullcontext())
        self.patch(ba, "Plan", plan)
        self.patch(ba, "Stepper", stepper)
        self.patch(ba, "_cuda", FakeCuda)

    # -- what differs between this cache and the functions it replaced
    def get(self, ii, jj, kk, fixedp):
        return self.cache.get(ii, jj, kk, N_BUF, P_TOT, fixedp, DEV)

    def settle(self, stepper):
        return self.cache.settle(stepper)

    def after_step(self, stepper):
        self.cache.after_step()

    def prefetch(self, lst_, fixedp, background):
        self.cache.prefetch(*lst_, N_BUF, P_TOT, fixedp, DEV, background)
        for fut, _, _ in list(self.cache.pending.values()):   # (the worker's part of the trace is complete before the caller's goes on)
            fut.result()

    def clear(self):
        self.cache.clear()

    def sizes(self):
        return [len(self.cache.plans), len(self.cache.ahead), len(self.cache.pending)]

    def has_last(self):
        return self.cache.last is not None

    @property
    def last_shift(self):
        return self.cache.last_shift

    @last_shift.setter
    def last_shift(self, v):
        self.cache.last_shift = v

    def rekey(self, table, old, new, fixedp):
        """Files the entry of list `old` under the key of list `new`, as a recycled id() / address would."""
        t = getattr(self.cache, table)
        t[ba._key(*new, N_BUF, P_TOT, fixedp, DEV)] = t.pop(ba._key(*old, N_BUF, P_TOT, fixedp, DEV))

    # -- BA_rgbd_droid's order of calls
    def call(self, lst_, fixedp, per_track=False):
        ii, jj, kk = lst_
        stepper, in_place = self.get(ii, jj, kk, fixedp)
        if per_track and stepper.plan.speculative and not self.settle(stepper):
            stepper, in_place = self.get(ii, jj, kk, fixedp)
        self.w.log("step", stepper.plan.info["fixedp"], stepper.plan.made)
        if stepper.plan.speculative and not self.settle(stepper):
            return self.call(lst_, fixedp, per_track)
        if in_place:
            self.after_step(stepper)
        return in_place

    def calls(self, lst_, fixedp, n):
        return [self.call(lst_, fixedp) for _ in range(n)]


# ---- the scenarios: each takes a factory of fresh drivers and returns (trace, observations) per driver it used

def s01_same_list_four_times(new):
    d = new()
    obs = dict(in_place=d.calls(lst(0), 3, 4), sizes=d.sizes())
    return [(list(d.w.trace), obs)]


def s02_stale_hits(new):
    d = new()
    a = lst(0)
    d.call(a, 3)
    a[0].add_(0)                                       # an in-place edit: the version moves, the plan is another
    obs = dict(after_edit=d.call(a, 3), sizes=d.sizes())
    b = lst(10)
    d.rekey("plans", a, b, 3)                          # a hit whose weak references point at other tensors
    obs["other_tensors"] = d.call(b, 3)
    c, gone = lst(20), lst(30)
    d.call(gone, 3)
    d.rekey("plans", gone, c, 3)
    d.call(b, 3)                                       # (the last call holds its list)
    del gone                                           # ... and one whose weak references are dead
    obs["dead"] = d.call(c, 3)
    obs["sizes_end"] = d.sizes()
    return [(list(d.w.trace), obs)]


def s03_eviction(new):
    d = new()
    d.last_shift = 1
    lists = [lst(10 * k) for k in range(9)]
    d.calls(lists[0], 3, 3)                            # the first plan, with a clone made ahead
    obs = dict(with_clone=d.sizes())
    for l in lists[1:8]:
        d.call(l, 3)
    obs["full"] = d.sizes()
    mark = len(d.w.trace)
    d.call(lists[8], 3)                                # the ninth: the first plan leaves, its clone with it
    obs["ninth"] = d.sizes()
    obs["ninth_ops"] = d.w.trace[mark:]
    d.calls(lists[1], 3, 3)                            # the oldest plan is the one being stepped: spared behind its preshift
    obs["oldest_stepped"] = d.sizes()
    mark = len(d.w.trace)
    d.calls(lists[2], 3, 3)                            # ... the next preshift evicts it early (not the plan being stepped)
    obs["early"] = d.sizes()
    obs["early_ops"] = d.w.trace[mark:]
    return [(list(d.w.trace), obs)]


def s04_steady_state(new):
    d = new()
    f = 3
    a, b, c, dd = lst(0), lst(1), lst(2), lst(3)
    d.w.script["preshift"] = [False]                   # (the clone from B is declined: C is served by shifted_spec, D by bind)
    obs = dict(a=d.calls(a, f, 6), shift_a=d.last_shift)
    obs.update(b=d.calls(b, f + 1, 6), shift_b=d.last_shift)
    obs.update(c=d.calls(c, f + 2, 6), shift_c=d.last_shift, sizes_c=d.sizes())
    mark = len(d.w.trace)
    d.prefetch(dd, f + 3, False)                       # the probe finds the clone: nothing is built
    obs.update(probe_ops=d.w.trace[mark:], sizes_probe=d.sizes())
    mark = len(d.w.trace)
    obs.update(d=d.calls(dd, f + 3, 6), d_ops=d.w.ops(mark), sizes_d=d.sizes())
    return [(list(d.w.trace), obs)]


def s05_behind_which_call(new):
    out = []
    for before, at in ((2, None), (4, None), (6, None), (6, "4"), (2, "6")):
        d = new()
        d.setenv("BT_PLAN_PRESHIFT_AT", at)
        d.last_shift = 1
        d.calls(lst(0), 3, before)
        mark = len(d.w.trace)
        d.calls(lst(50), 3, 6)
        ops = d.w.ops(mark)
        out.append((list(d.w.trace), dict(before=before, at=at, steps_before_preshift=ops[:ops.index("preshift")].count("step"),
                                    preshifts=ops.count("preshift"))))
    return out


def s06_bind_and_spec_decline(new):
    d = new()
    d.last_shift = 1
    a, b, c = lst(0), lst(1), lst(2)
    d.calls(a, 3, 3)
    d.w.script["bind"] = [False]
    mark = len(d.w.trace)
    d.calls(b, 4, 3)                                   # bind says no: shifted_spec from the same source
    obs = dict(b_ops=d.w.trace[mark:])
    d.w.script.update(bind=[False], shifted_spec=[False])
    mark = len(d.w.trace)
    d.call(c, 5)                                       # both say no: the synchronous path, one wait
    obs.update(c_ops=d.w.trace[mark:], shift=d.last_shift, sizes=d.sizes())
    return [(list(d.w.trace), obs)]


def _before_wrong_guess(d):
    """A list with a clone made ahead for the next one, and an older list with a clone of its own; shifted_any never matches."""
    d.last_shift = 1
    d.w.script["shifted_any"] = [False] * 4
    d.calls(lst(40), 3, 3)
    d.calls(lst(0), 5, 3)
    return d.sizes()


def s07_failed_speculation(new):
    out = []
    for confirm, per_track in ((False, False), (RuntimeError("index out of range"), False), (False, True)):
        d = new()
        obs = dict(before=_before_wrong_guess(d))
        d.w.script["confirm"] = [confirm]
        mark = len(d.w.trace)
        try:
            obs["in_place"] = d.call(lst(1), 6, per_track)
        except RuntimeError as e:
            obs["raised"] = str(e)
        obs.update(ops=d.w.trace[mark:], sizes=d.sizes(), shift=d.last_shift, has_last=d.has_last())
        out.append((list(d.w.trace), obs))
    return out


def s08_switches(new):
    out = []
    for name in ("BT_PLAN_SHIFT", "BT_PLAN_SPECULATE", "BT_PLAN_PRESHIFT"):
        d = new()
        d.setenv(name, "0")
        for k in range(5):
            d.calls(lst(k), 3 + k, 3)
        d.setenv(name, None)
        out.append((list(d.w.trace), dict(off=name, ops=sorted(set(d.w.ops())))))
    d = new()                                          # flipped between two calls
    obs = {}
    for k in range(3):
        d.calls(lst(k), 3 + k, 3)
    d.setenv("BT_PLAN_SPECULATE", "0")
    mark = len(d.w.trace)
    d.calls(lst(3), 6, 3)
    obs["speculate_off"] = d.w.ops(mark)
    d.setenv("BT_PLAN_SPECULATE", None)
    d.setenv("BT_PLAN_SHIFT", "0")
    mark = len(d.w.trace)
    d.calls(lst(4), 7, 3)
    obs["shift_off"] = d.w.ops(mark)
    d.setenv("BT_PLAN_SHIFT", None)
    mark = len(d.w.trace)
    d.calls(lst(5), 8, 3)
    obs["on_again"] = d.w.ops(mark)
    out.append((list(d.w.trace), obs))
    return out


def s09_prefetch(new):
    out = []
    d = new()
    a, b, c, other = lst(0), lst(10), lst(20), lst(30)
    d.prefetch(a, 3, False)                            # in the open: stored, and the next get hits it
    obs = dict(stored=d.sizes())
    mark = len(d.w.trace)
    obs.update(hit=d.call(a, 3), hit_ops=d.w.ops(mark))
    d.prefetch(b, 3, True)                             # in the background: picked up through the pending entry
    obs["pending"] = d.sizes()
    mark = len(d.w.trace)
    obs.update(picked_up=d.call(b, 3), picked_ops=d.w.ops(mark), sizes=d.sizes())
    d.prefetch(other, 3, True)                         # a pending entry whose held tensors are not the caller's is not used
    d.rekey("pending", other, c, 3)
    mark = len(d.w.trace)
    obs.update(not_held=d.call(c, 3), not_held_ops=d.w.trace[mark:], sizes_end=d.sizes())
    out.append((list(d.w.trace), obs))
    d = new()                                          # a fifth pending prefetch waits for the oldest and drops it
    for k in range(4):
        d.prefetch(lst(10 * k), 3 + k, True)
    obs = dict(four=d.sizes())
    mark = len(d.w.trace)
    d.prefetch(lst(40), 7, True)
    obs.update(five=d.sizes(), fifth_ops=d.w.trace[mark:])
    out.append((list(d.w.trace), obs))
    d = new()                                          # the worker's ordinary error: rebuilt in the open
    d.w.script["Plan"] = [RuntimeError("boom")]
    d.prefetch(a, 3, True)
    mark = len(d.w.trace)
    obs = dict(rebuilt=d.call(a, 3), ops=d.w.ops(mark), sizes=d.sizes())
    d.w.script["Plan"] = [KeyboardInterrupt()]         # ... any other is raised again
    d.prefetch(b, 3, True)
    try:
        d.call(b, 3)
    except KeyboardInterrupt:
        obs["interrupt"] = "raised again"
    obs["sizes_end"] = d.sizes()
    out.append((list(d.w.trace), obs))
    return out


def s10_clear(new):
    d = new()
    d.last_shift = 1
    d.calls(lst(0), 3, 3)
    d.prefetch(lst(10), 3, True)
    obs = dict(before=d.sizes())
    d.clear()
    obs.update(after=d.sizes(), shift=d.last_shift, has_last=d.has_last())
    mark = len(d.w.trace)
    d.calls(lst(0), 3, 3)                              # (the last shift is still there: the clone is made again)
    obs["ops_after"] = d.w.ops(mark)
    return [(list(d.w.trace), obs)]


SCENARIOS = {f.__name__: f for f in (s01_same_list_four_times, s02_stale_hits, s03_eviction, s04_steady_state, s05_behind_which_call,
                                     s06_bind_and_spec_decline, s07_failed_speculation, s08_switches, s09_prefetch, s10_clear)}


def run(name, new):
    """The scenario's traces and observations, as JSON holds them."""
    alive = []                                         # (the end of a driver's cache is not part of its scenario)

    def keep():
        alive.append(new())
        return alive[-1]
    return json.loads(json.dumps([dict(trace=t, obs=o) for t, o in SCENARIOS[name](keep)]))


@pytest.fixture
def results(monkeypatch):
    for name in ("BT_PLAN_SHIFT", "BT_PLAN_SPECULATE", "BT_PLAN_PRESHIFT", "BT_PLAN_PRESHIFT_AT"):
        monkeypatch.delenv(name, raising=False)

    def setenv(name, value):
        monkeypatch.delenv(name, raising=False) if value is None else monkeypatch.setenv(name, value)

    with open(GOLDEN) as f:
        golden = json.load(f)

    def results(name):
        got = run(name, lambda: Driver(setenv, monkeypatch.setattr))
        assert got == golden[name]
        return [r["obs"] for r in got], [r["trace"] for r in got]
    return results


def ops_of(trace):
    return [t[0] for t in trace]


def test_same_list_four_times(results):
    (obs,), (trace,) = results("s01_same_list_four_times")
    assert obs["in_place"] == [False, True, True, True]
    assert ops_of(trace) == ["wait", "Plan", "Stepper", "step", "step", "step", "step"]


def test_stale_hits_are_rebuilt(results):
    (obs,), (trace,) = results("s02_stale_hits")
    assert obs["after_edit"] is False and obs["other_tensors"] is False and obs["dead"] is False
    assert ops_of(trace).count("Plan") == 5                        # the first, the edited, the two stale hits, the list that died


def test_eviction_takes_the_clone_and_spares_the_plan_being_stepped(results):
    (obs,), _ = results("s03_eviction")
    assert obs["with_clone"] == [1, 1, 0] and obs["full"] == [8, 1, 0] and obs["ninth"] == [8, 0, 0]
    gone = [t for t in obs["ninth_ops"] if t[0] == "destroy"]
    assert gone == [["destroy", 4, "preshift"], ["destroy", 3, "Plan"]]
    assert obs["oldest_stepped"] == [8, 1, 0]                      # 8 plans and a preshift: the oldest is being stepped, and stays
    assert obs["early"] == [7, 1, 0] and [t for t in obs["early_ops"] if t[0] == "destroy"] == [["destroy", 4, "preshift"], ["destroy", 3, "Plan"]]


def test_steady_state(results):
    (obs,), (trace,) = results("s04_steady_state")
    assert obs["shift_a"] is None and obs["shift_b"] == 1 and obs["shift_c"] == 1
    for k in "abcd":
        assert obs[k] == [False] + [True] * 5
    ops = ops_of(trace)
    assert ops.count("Plan") == 1 and ops.count("shifted_any") == 1 and ops.count("shifted_spec") == 1 and ops.count("bind") == 1
    assert ["shifted_spec", 5, 4] in trace and ["bind", 6, True] in trace and ops.count("confirm") == 2
    assert [t[1:] for t in trace if t[0] == "preshift"] == [[5, "declined"], [6, 5], [7, 6]]        # once per plan that has a shift to go by
    for fp in (4, 5, 6):                                           # ... behind call 5: the list before got six
        i = trace.index([t for t in trace if t[0] == "preshift" and t[1] == fp + 1][0])
        assert [t[1] for t in trace[:i] if t[0] == "step"].count(fp) == 5
    assert obs["probe_ops"] == [] and obs["sizes_probe"] == obs["sizes_c"]
    assert "shifted_spec" not in obs["d_ops"] and obs["d_ops"][:2] == ["bind", "step"]


def test_the_call_the_clone_is_made_behind(results):
    obs, _ = results("s05_behind_which_call")
    assert [(o["before"], o["at"], o["steps_before_preshift"]) for o in obs] == [(2, None, 2), (4, None, 3), (6, None, 5), (6, "4", 4), (2, "6", 6)]
    assert all(o["preshifts"] == 1 for o in obs)


def test_bind_declines_then_shifted_spec_declines(results):
    (obs,), _ = results("s06_bind_and_spec_decline")
    assert [t[:2] for t in obs["b_ops"][:2]] == [["bind", 4], ["shifted_spec", 4]] and obs["b_ops"][1][2] == 3
    ops = [op for op in ops_of(obs["c_ops"]) if op != "destroy"]
    assert ops[:4] == ["bind", "shifted_spec", "wait", "shifted_any"] and ops.count("wait") == 1
    assert ["shifted_any", 5, [[4, 3], 4]] in obs["c_ops"]                 # the last shift's plan first


def test_failed_speculation(results):
    (wrong, raised, per_track), _ = results("s07_failed_speculation")
    for o in (wrong, per_track):
        assert o["before"] == [2, 2, 0] and o["sizes"] == [3, 0, 0] and o["shift"] is None and o["in_place"] is False
        assert ops_of(o["ops"]).count("Plan") == 1 and ops_of(o["ops"]).count("destroy") == 2      # the wrong guess and the other clone
    ops = ops_of(wrong["ops"])
    assert ops.index("step") < ops.index("confirm") and ops.count("step") == 2
    ops = ops_of(per_track["ops"])
    assert ops.index("confirm") < ops.index("step") and ops.count("step") == 1                       # settled BEFORE the step
    assert raised["raised"] == "index out of range" and raised["sizes"] == [2, 0, 0] and raised["shift"] is None and raised["has_last"] is False


def test_switches(results):
    (shift, spec, pre, flipped), _ = results("s08_switches")
    assert shift["ops"] == ["Plan", "Stepper", "step", "wait"]
    assert "shifted_any" in spec["ops"] and not {"shifted_spec", "preshift", "bind"} & set(spec["ops"])
    assert "shifted_spec" in pre["ops"] and not {"preshift", "bind"} & set(pre["ops"])
    assert "shifted_any" in flipped["speculate_off"] and not {"shifted_spec", "preshift", "bind"} & set(flipped["speculate_off"])
    assert "Plan" in flipped["shift_off"] and not {"shifted_any", "shifted_spec", "preshift", "bind"} & set(flipped["shift_off"])
    assert {"preshift"} <= set(flipped["on_again"])


def test_prefetch(results):
    (one, five, errors), _ = results("s09_prefetch")
    assert one["stored"] == [1, 0, 0] and one["hit"] is False and one["hit_ops"] == ["step"]
    assert one["pending"] == [1, 0, 1] and one["picked_ops"] == ["step"] and one["sizes"] == [2, 0, 0]
    assert "Plan" in ops_of(one["not_held_ops"]) and one["sizes_end"] == [3, 0, 0]
    assert five["four"] == [0, 0, 4] and five["five"] == [0, 0, 4] and five["fifth_ops"][0] == ["destroy", 3, "Plan"]
    assert errors["ops"] == ["wait", "Plan", "Stepper", "step"] and errors["interrupt"] == "raised again"


def test_clear_keeps_the_last_shift(results):
    (obs,), _ = results("s10_clear")
    assert obs["before"] == [1, 1, 1] and obs["after"] == [0, 0, 0] and obs["shift"] == 1 and obs["has_last"] is False
    assert "preshift" in obs["ops_after"]
