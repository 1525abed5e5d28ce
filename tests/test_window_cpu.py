"""CPU: the one sampling window (gfv/window.py) and the one follower protocol (gfv/follow.py) that `FieldStats`, `WallForces`, `TimeBC`
and `TimeScheme` share: the window's argument checks, its unattached state, the record's word order, that both samplers reach the
one `Window`, the order in which an owner refuses a follower, and that a failed attach leaves a follower free.  Nothing here
touches a GPU.
"""
import types

import pytest
import torch

import cases
import fieldstats_ref
import wallforce_ref
import window_ref as R


def test_the_window_checks_its_arguments_and_needs_no_device():
    from gfv.window import NO_STOP, Window, check_window_args
    assert check_window_args() == (1, 1, NO_STOP, 1)
    assert check_window_args(1, 3, 10, False) == (1, 3, 10, 0)
    # the cases of test_fieldstats_cpu.py::test_argument_refusals_need_no_device
    for bad in (dict(start=-1), dict(start=0), dict(start=1.5), dict(start=True), dict(stride=0), dict(stride=-2), dict(stride=2.0),
                dict(stop=-1), dict(stop=3.5), dict(stop=False), dict(start=2 ** 31), dict(stop=2 ** 31), dict(enabled="yes"),
                dict(start=None)):
        with pytest.raises(ValueError):
            check_window_args(**bad)
        if "enabled" not in bad:
            with pytest.raises(ValueError):
                Window(**bad)
    # the cases of test_wallforce_cpu.py::test_refusals_and_window_arguments: the message names the argument
    for kw, what in ((dict(start=0), "start"), (dict(start=1.5), "start"), (dict(start=True), "start"), (dict(stride=0), "stride"),
                     (dict(stop=-1), "stop"), (dict(start=2 ** 31), "start"), (dict(stride="2"), "stride")):
        with pytest.raises(ValueError, match=what):
            Window(**kw)
    # unattached: set() changes the host words alone, and checks before anything changes
    w = Window(start=3, stride=2, stop=9)
    assert (w.start, w.stride, w.stop, w.enabled) == (3, 2, 9, True) and w.rec is None
    w.set(stride=4)
    assert (w.start, w.stride, w.stop, w.enabled) == (3, 4, 9, True)
    w.set(stop=None, enabled=False)
    assert (w.start, w.stride, w.stop, w.enabled) == (3, 4, None, False) and w.rec is None
    with pytest.raises(ValueError, match="stride"):
        w.set(start=5, stride=0)
    assert w.start == 3
    # attached (a CPU tensor stands in for the device record): the host words are written, the device's start over
    rec = w.attach(torch.device("cpu"))
    assert rec is w.rec and rec.dtype == torch.int32 and rec.tolist() == [3, 4, -1, -1, 0, 0, 0, 0] and w.count() == 0
    rec[R.N], rec[R.LAST] = 5, 12                                           # (what launches leave)
    w.set(start=7, enabled=True)
    assert rec.tolist() == [7, 4, -1, 12, 5, 0, 1, 0] and w.count() == 5    # the device's words stay
    w.reset()
    assert rec.tolist() == [7, 4, -1, -1, 0, 0, 1, 0]


def test_the_words_of_the_record_are_stated_once():
    from gfv import fieldstats as F
    from gfv import lib as L
    from gfv import window as W
    names = ("START", "STRIDE", "STOP", "LAST", "N_SAMPLES", "COUNTER", "ENABLED")
    assert [getattr(W, n) for n in names] == list(range(7)) == [R.START, R.STRIDE, R.STOP, R.LAST, R.N, R.COUNTER, R.ENABLED]
    assert [getattr(F, n) for n in names] == list(range(7))                 # re-exported
    assert F.NO_STOP is W.NO_STOP and F.UNCHANGED is W.UNCHANGED and F.check_field_stats_args is W.check_window_args
    assert L.WINDOW_RECORD == L.FIELD_STATS_RECORD == L.WALL_FORCE_RECORD == R.RECORD == 8
    # the float64 references share one statement of the rule, too
    assert fieldstats_ref.take is R.take is wallforce_ref.take and fieldstats_ref.RECORD == wallforce_ref.RECORD == R.RECORD


def test_both_samplers_reach_the_one_window(monkeypatch):
    from gfv.fieldstats import FieldStats
    from gfv.wallforce import WallForces
    from gfv.window import Window
    calls = []
    real = Window.set
    monkeypatch.setattr(Window, "set", lambda self, *a, **k: (calls.append((self, a, k)), real(self, *a, **k))[1])
    for obj in (FieldStats(start=2), WallForces(start=2)):
        assert isinstance(obj._window, Window)
        obj.set_window(stride=3, stop=11)
        obj.set_window(5, None, None, False)
        assert [c[0] for c in calls] == [obj._window] * 2
        assert (obj.start, obj.stride, obj.stop, obj.enabled) == (5, 3, None, False)
        calls.clear()


def test_the_four_followers_share_one_base():
    from gfv import timebc as T
    from gfv.fieldstats import FieldStats
    from gfv.follow import Follower
    from gfv.timescheme import TimeScheme
    from gfv.wallforce import WallForces
    made = (FieldStats(), WallForces(), T.TimeBC(velocity=T.Const()), TimeScheme("bdf2"))
    for obj, keyword in zip(made, ("field_stats", "wall_forces", "time_bc", "time_scheme")):
        cls = type(obj)
        assert issubclass(cls, Follower) and cls.KEYWORD == keyword
        assert "check_free" not in vars(cls) and "_need" not in vars(cls) and "_claim" not in vars(cls)
        obj.check_free()
        with pytest.raises(RuntimeError, match=rf"this {cls.__name__} is not attached.*{keyword}="):
            obj._need()
        obj._claim(types.SimpleNamespace())                                 # an owner object: its class name is kept, not the object
        assert obj._owner == "SimpleNamespace"
        with pytest.raises(ValueError, match=f"this {cls.__name__} is already attached to a SimpleNamespace"):
            obj.check_free()
        obj._claim("evaluate")                                              # or a plain name
        assert obj._owner == "evaluate"


def test_check_followers_refuses_in_the_documented_order():
    from gfv import timebc as T
    from gfv.fieldstats import FieldStats
    from gfv.follow import check_followers
    from gfv.timescheme import TimeScheme
    from gfv.wallforce import WallForces
    graphs = cases.make_graphs("cyl_cavity_b2")                             # CPU graphs, B = 2
    pooled = (types.SimpleNamespace(_gfv_pool_plan=object()),) + tuple(graphs[1:])
    check_followers("Rollout", graphs, 2)                                   # nothing handed: nothing refused
    check_followers("MarchStep", graphs, 0, field_stats=FieldStats(), wall_forces=WallForces(), time_bc=T.TimeBC(velocity=T.Const()),
                    time_scheme=TimeScheme())
    check_followers("MarchStep", graphs, 2, time_scheme=TimeScheme())       # (no reason to refuse anderson: not refused)

    def taken(obj):
        obj._owner = "Rollout"
        return obj
    three = lambda: T.TimeBC(velocity=[T.Const()] * 3)
    for keyword, make, has_graph_check in (("field_stats", FieldStats, False), ("wall_forces", WallForces, True),
                                           ("time_bc", lambda: T.TimeBC(velocity=T.Const()), True)):
        # 1. the type, whatever else is wrong
        with pytest.raises(ValueError, match=f"Rollout: {keyword} must be a gfv.*or None"):
            check_followers("Rollout", pooled, 2, **{keyword: dict(start=1)})
        # 2. then a follower that is taken
        with pytest.raises(ValueError, match="already attached to a Rollout"):
            check_followers("Rollout", pooled, 2, **{keyword: taken(make())})
        # 3. then anderson
        with pytest.raises(ValueError, match=f"Rollout: anderson > 0 together with {keyword}"):
            check_followers("Rollout", pooled, 2, **{keyword: make()})
        # 4. then the class's own check of the graphs
        if has_graph_check:
            with pytest.raises(ValueError, match="DevicePool"):
                check_followers("Rollout", pooled, 0, **{keyword: make()})
        else:
            check_followers("Rollout", pooled, 0, **{keyword: make()})
    with pytest.raises(ValueError, match="3 waveforms for a batch of 2"):
        check_followers("MarchStep", graphs, 0, time_bc=three())
    with pytest.raises(ValueError, match="anderson"):
        check_followers("Rollout", graphs, 1, time_bc=three())              # anderson in front of the graphs
    with pytest.raises(ValueError, match="MarchStep: time_scheme must be a gfv.timescheme.TimeScheme or None"):
        check_followers("MarchStep", None, 0, time_scheme="bdf2")
    with pytest.raises(ValueError, match="already attached"):
        check_followers("MarchStep", None, 0, time_scheme=taken(TimeScheme()))
    # among several, the launch order decides: field_stats, wall_forces, time_bc, time_scheme
    with pytest.raises(ValueError, match="wall_forces must be"):
        check_followers("MarchStep", graphs, 0, field_stats=FieldStats(), wall_forces=1, time_bc=2, time_scheme=3)


def test_an_attach_that_raised_leaves_the_follower_free():
    from gfv import timebc as T
    from gfv.fieldstats import FieldStats
    from gfv.plan import build_plan
    from gfv.timescheme import TimeScheme
    from gfv.wallforce import WallForces
    graphs = cases.make_graphs("cyl_cavity_b2")
    plan = build_plan(*graphs)
    xb, clock, owner = torch.zeros(plan.N, 12), torch.zeros(2, dtype=torch.int32), types.SimpleNamespace()
    attempts = ((FieldStats(), lambda f: f.attach(owner, xb, clock, 0)),
                (WallForces(), lambda f: f.attach(owner, graphs, plan, xb, clock, 0)),
                (T.TimeBC(velocity=T.Const()), lambda f: f.attach(owner, graphs, plan, xb, xb.clone(), clock, 0, 4)),
                (TimeScheme("bdf2"), lambda f: f.attach(owner, plan, xb, clock, 0)))
    for follower, attach in attempts:
        with pytest.raises(ValueError, match="GPU"):
            attach(follower)                                                # a CPU node state: there is no CPU path
        follower.check_free()
        assert follower.rec is None and follower._owner is None
        with pytest.raises(RuntimeError, match="not attached"):
            follower.reset()
