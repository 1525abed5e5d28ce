"""CPU: the launch sequence of one optimiser step (gfv/optstep.py) - for every combination of accumulation (A),
active guard (G), averaged weights (E) and parameter groups (P) `optimizer_launches` calls the entries of the table, in its
order, and hands the Adam entry exactly the records that are on.  The library is a recorder: nothing is launched."""
import ast
import itertools
import os
import types

import pytest

import cases

GFV = os.path.join(cases.ROOT, "gen-fvgn-steady_amd", "gfv")


class Buf:
    """Stand-in for a device tensor: an address."""
    _next = 0x1000

    def __init__(self):
        Buf._next += 0x100
        self.addr = Buf._next

    def data_ptr(self):
        return self.addr


class Recorder:
    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        def entry(*args):
            self.calls.append((name, args))
            return 0
        return entry


@pytest.fixture
def recorder(monkeypatch):
    from gfv import lib
    rec = Recorder()
    monkeypatch.setattr(lib, "load", lambda raw=False: rec)
    monkeypatch.setattr(lib, "stream_ptr", lambda: "stream")     # (the current stream needs a device)
    return rec


def owners(active=True):
    guard = types.SimpleNamespace(active=active, guard=Buf(), segs=Buf(), ws=Buf(), n_seg=3, n_elems=40)
    accum = types.SimpleNamespace(acc=Buf(), rec=Buf())
    ema = types.SimpleNamespace(e=Buf(), rec=Buf())
    groups = types.SimpleNamespace(run_start=Buf(), run_group=Buf(), table=Buf(), n_runs=3)
    return guard, accum, ema, groups


def expected(A, G, E, P, t, guard, accum, ema, groups):
    """The table of DESIGN.md 5f, written out: [(entry, args)]."""
    p, g, m, v, state, hyper, loss = (t[k].addr for k in ("p", "g", "m", "v", "state", "hyper", "loss"))
    n, B, st = 44, 5, "stream"
    arec = accum.rec.addr if A else None
    grec = guard.guard.addr if G else None
    e, erec = (ema.e.addr, ema.rec.addr) if E else (None, None)
    out = []
    if A:
        out.append(("gfv_grad_accum_dev", (g, accum.acc.addr, n, B, loss, arec, st)))
    if G:
        norm = (g, guard.segs.addr, guard.n_seg, guard.n_elems, hyper, grec, guard.ws.addr)
        out.append(("gfv_grad_guard_accum_dev", norm + (arec, st)) if A else ("gfv_grad_guard_dev", norm + (st,)))
    if P:
        out.append(("gfv_adam_step_groups_dev", (p, g, m, v, e, n, state, hyper, grec, arec, erec, groups.run_start.addr,
                                                 groups.run_group.addr, groups.n_runs, groups.table.addr, st)))
    elif E:
        out.append(("gfv_adam_step_ema_dev", (p, g, m, v, e, n, state, hyper, grec, arec, erec, st)))
    elif A:
        out.append(("gfv_adam_step_accum_dev", (p, g, m, v, n, state, hyper, grec, arec, st)))
    elif G:
        out.append(("gfv_adam_step_guarded_dev", (p, g, m, v, n, state, hyper, grec, st)))
    else:
        out.append(("gfv_adam_step_dev", (p, g, m, v, n, state, hyper, st)))
    return out


def run(recorder, A, G, E, P, guard_given=True, active=True):
    from gfv.optstep import optimizer_launches
    t = {k: Buf() for k in ("p", "g", "m", "v", "state", "hyper", "loss")}
    guard, accum, ema, groups = owners(active)
    optimizer_launches(t["p"], t["g"], t["m"], t["v"], 44, t["state"], t["hyper"], guard=guard if guard_given else None,
                       accum=accum if A else None, ema=ema if E else None, groups=groups if P else None, B=5,
                       loss=t["loss"] if A else None)
    return recorder.calls, expected(A, G, E, P, t, guard, accum, ema, groups)


@pytest.mark.parametrize("A,G,E,P", list(itertools.product((False, True), repeat=4)))
def test_every_form_issues_the_entries_of_the_table_in_order(recorder, A, G, E, P):
    got, want = run(recorder, A, G, E, P, active=G)
    assert [name for name, _ in got] == [name for name, _ in want]
    assert got == want
    # which records the Adam entry is handed: guard iff G, accum iff A, e and ema iff E
    name, args = got[-1]
    assert name.startswith("gfv_adam_step")
    assert len(got) == 1 + int(A) + int(G)
    if name in ("gfv_adam_step_groups_dev", "gfv_adam_step_ema_dev"):
        e, grec, arec, erec = args[4], args[8], args[9], args[10]
        assert (e is not None) == E and (erec is not None) == E
        assert (grec is not None) == G and (arec is not None) == A
    elif name == "gfv_adam_step_accum_dev":
        assert (args[7] is not None) == G and args[8] is not None
    elif name == "gfv_adam_step_guarded_dev":
        assert args[7] is not None


@pytest.mark.parametrize("A,E,P", list(itertools.product((False, True), repeat=3)))
@pytest.mark.parametrize("guard_given", [True, False])
def test_a_guard_that_is_not_active_issues_no_norm_launch_and_a_null_record(recorder, A, E, P, guard_given):
    got, want = run(recorder, A, False, E, P, guard_given=guard_given, active=False)
    assert got == want
    assert not any("grad_guard" in name for name, _ in got)
    name, args = got[-1]
    if name in ("gfv_adam_step_groups_dev", "gfv_adam_step_ema_dev"):
        assert args[8] is None
    elif name == "gfv_adam_step_accum_dev":
        assert args[7] is None
    else:
        assert name == "gfv_adam_step_dev"


def test_a_failing_entry_raises_with_its_label(recorder, monkeypatch):
    from gfv.optstep import optimizer_launches
    labels = {"gfv_grad_accum_dev": "grad_accum", "gfv_grad_guard_accum_dev": "grad_guard_accum", "gfv_grad_guard_dev": "grad_guard",
              "gfv_adam_step_groups_dev": "adam_step_groups", "gfv_adam_step_ema_dev": "adam_step_ema",
              "gfv_adam_step_accum_dev": "adam_step_accum", "gfv_adam_step_guarded_dev": "adam_step_guarded",
              "gfv_adam_step_dev": "adam_step"}
    forms = {"gfv_grad_accum_dev": (1, 1, 0, 0), "gfv_grad_guard_accum_dev": (1, 1, 0, 0), "gfv_grad_guard_dev": (0, 1, 0, 0),
             "gfv_adam_step_groups_dev": (0, 0, 0, 1), "gfv_adam_step_ema_dev": (0, 0, 1, 0), "gfv_adam_step_accum_dev": (1, 0, 0, 0),
             "gfv_adam_step_guarded_dev": (0, 1, 0, 0), "gfv_adam_step_dev": (0, 0, 0, 0)}
    for entry, label in labels.items():
        A, G, E, P = forms[entry]
        monkeypatch.setattr(recorder, entry, lambda *a: -1, raising=False)
        t = {k: Buf() for k in ("p", "g", "m", "v", "state", "hyper", "loss")}
        guard, accum, ema, groups = owners(bool(G))
        with pytest.raises(RuntimeError, match=rf"libgfv: {label} failed with code -1"):
            optimizer_launches(t["p"], t["g"], t["m"], t["v"], 44, t["state"], t["hyper"], guard=guard, accum=accum if A else None,
                               ema=ema if E else None, groups=groups if P else None, B=5, loss=t["loss"])
        monkeypatch.delattr(recorder, entry)


def imported_modules(path):
    """Names of the gfv modules a source imports (import check only: `from . import x`, `from .x import y`, `import gfv.x`)."""
    found = set()
    for node in ast.walk(ast.parse(open(path).read())):
        if isinstance(node, ast.ImportFrom):
            if node.module:
                found.add(node.module.split(".")[-1])
            if node.level > 0 and not node.module or node.module in ("gfv",):
                found.update(a.name for a in node.names)
        elif isinstance(node, ast.Import):
            found.update(a.name.split(".")[-1] for a in node.names)
    return found


@pytest.mark.parametrize("module", ["guard", "accum", "ema"])
def test_the_record_owners_do_not_import_one_another(module):
    others = {"guard", "accum", "ema", "groups", "optstep"} - {module}
    assert not imported_modules(os.path.join(GFV, module + ".py")) & others


def test_the_record_owners_have_no_launch_method():
    from gfv.accum import GradAccum
    from gfv.ema import WeightEMA
    from gfv.groups import ParamGroups
    from gfv.guard import GradGuard
    for owner in (GradGuard, GradAccum, WeightEMA, ParamGroups):
        assert not hasattr(owner, "launch"), owner.__name__
