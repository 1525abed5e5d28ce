"""The adaptive time step on the device (gfv/timescheme.py `StepControl`, csrc/stepcontrol.hip; include/gfv.h
gfv_step_control_rate, gfv_step_control_rows).

1. the two launches alone against the float64 rule of tests/stepcontrol_ref.py: B = 1, B = 3 with wavefronts and a workgroup that
   hold cells of two graphs, the polygon fixture, a graph at rest; every clamp hit by construction of the fields;
2. repeatability bit for bit, and the history ring's wrap;   3. `adapt` at unit ratio is the fixed-step scheme;
4. the device-decided march equals a host-driven loop that applies the rule (in float32, the order include/gfv.h writes down);
5. run-ahead and held steps;   6. resume;   7. the controller grows the step of a cavity started from rest.

Tolerances.  1: relative 1e-5 against float64 - a cell sums at most a dozen non-negative float32 terms, a few 1e-6 at the most;
`ustar` is normalised by its largest magnitude over the graph (its elements cancel).  3: 1e-6 on `ustar` - measured against the
larger of |ustar| and |u_n - u_{n-1}| - and on `dt_eff`; the loss history within tests/test_timescheme_gpu.py's tolerance of the
`losses` stage (4 x the float32 oracle's own error on the polygon mesh, floor 2^-22: 2.9e-6 ... 6.2e-5 per column).  The launches
apply the variable-step weights as divisions by (1 + 2 w) / w^2 and (1 + 2 w) / (1 + w), which are exactly 3 and 1.5 at w = 1, so
both differences are in fact zero; with the weights applied as products (a rounding apart from 1/3 and 1/1.5) `ustar` was 1.6e-7
and `dt_eff` 6.3e-8 off and the loss history of level 1 up to 2.0e-4 (the pressure term; Adam amplifies the last bit), 3.2 x that
tolerance.  4 to 6: bit for bit.

Measured on the MI355X (1: largest over the six clocks of every batch): rate 1.2e-7, dt_next 1.3e-7, omega 1.3e-7, dt_eff 1.5e-7,
time 3.5e-8, ustar 2.4e-7; every launch also had the bits of the float32 rule.  7: dt / plan.dt = 1.5, 2.25, 3.375, 5.0625, 7.594,
9.186, 9.199, 9.200, 9.201 with the Courant number at 0.10, 0.17, 0.25, 0.37, 0.55, 0.83, 0.9986, 0.9999, 0.9999 of the target."""
import functools

import numpy as np
import pytest
import torch

import fvm_float64 as F
import stepcontrol_ref as R
from test_march_gpu import LR, _assert_same, _cpu_graphs, _graphs, _model
from test_timescheme_gpu import MAX_INNER, _carry_over, _march, _named_state, _reference

pytestmark = pytest.mark.gpu

f32, f64 = np.float32, np.float64
RTOL = 1e-5


def _control(**kw):
    from gfv.timescheme import StepControl
    return StepControl(**kw)


def _scheme(scheme="bdf2", **kw):
    from gfv.timescheme import TimeScheme
    return TimeScheme(scheme, adapt=_control(**kw))


class _Owner:
    pass


# ---- 1. the launches alone -------------------------------------------------------------------------------------------------------
def _cavities(ns):
    from gfv import meshgen
    from gfv.graph import build_batch
    meshes = [meshgen.finish_mesh(meshgen.raw_quad_cavity(n=n, jitter=0.1, tri_fraction=0.0, seed=30 + n), U=0.5 + 0.25 * i)
              for i, n in enumerate(ns)]
    return build_batch(meshes, [meshgen.random_fields(m, seed=40 + i) for i, m in enumerate(meshes)])


@functools.lru_cache(maxsize=None)
def _batch(which):
    if which == "B1":
        g = _cavities((6,))
    elif which == "B3":
        g = _cavities((9, 14, 11))            # 81, 196 and 121 cells: the graphs meet inside wavefronts 1 and 4 and workgroup 1
    elif which == "rest":
        g = _cavities((7, 5))
    else:
        g = _cpu_graphs("poly")               # the committed polygon mesh: cells of four to eight incidences
    return F.distinct_coefficients(g, 7)


class _Alone:
    """A TimeScheme on a field and a clock word of the test's own, beside the float64 rule (and the float32 one, for figures)."""

    def __init__(self, which, ctl_kw, scheme="bdf2", plain=False):
        from gfv import plan as P
        from gfv.timescheme import TimeScheme
        self.graphs = tuple(g.clone().to("cuda") for g in _batch(which))
        self.plan = P.build_plan(*self.graphs)
        self.N, self.B = int(self.plan.N), int(self.plan.B)
        self.xb = torch.zeros((self.N, 12), dtype=torch.float32, device="cuda")
        self.clock = torch.zeros(1, dtype=torch.int32, device="cuda")
        self.ctl = _control(**ctl_kw)
        self.sch = TimeScheme(scheme, adapt=self.ctl).attach(_Owner(), self.plan, self.xb, self.clock, 0)
        self.plain = TimeScheme(scheme).attach(_Owner(), self.plan, self.xb, self.clock, 0) if plain else None
        self.arr = R.plan_arrays(self.plan)
        word = R.BDF2 if scheme == "bdf2" else R.BDF1
        self.rule, self.rule32 = R.StepRule(self.arr, self.ctl, word), R.StepRule(self.arr, self.ctl, word, f32)
        self.rule.reset(0)
        self.rule32.reset(0)
        self.dt_plan = self.plan.dt.cpu().clone()

    def put(self, field, clock):
        self.xb.copy_(torch.from_numpy(np.ascontiguousarray(field, dtype=f32)))
        self.clock.fill_(int(clock))

    def launch(self, field=None, clock=None):
        if field is not None:
            self.put(field, clock)
        self.sch.launch()
        torch.cuda.synchronize()

    def buffers(self):
        torch.cuda.synchronize()
        out = {"ring": self.sch.ring, "ustar": self.sch.ustar, "dt_eff": self.sch.dt_eff, "rec": self.sch.rec}
        out.update(self.sch._ctl)
        return {k: v.cpu().clone() for k, v in out.items()}


def _fields_for(arr, gains, seed, rest=()):
    """One random field per clock whose Courant number UNDER THE PLAN'S dt is gains[clock] in every graph (float64): the velocity
    columns of graph b are scaled by gains[c] / (rate_b dt_b).  Graphs in `rest` are at rest."""
    g = np.random.default_rng(seed)
    batch, dt = np.asarray(arr["batch"], np.int64), np.asarray(arr["dt"], f64)
    out = []
    for gain in gains:
        x = (g.standard_normal((batch.shape[0], 12)) + np.arange(12)[None, :]).astype(f32)
        rates = R.cell_rates(x, arr["uvp_dim"], arr["crow"], arr["knode"], arr["kS"], arr["area"], arr["cbatch"])
        top, _ = R.graph_rates(rates, arr["cbatch"], dt.shape[0])
        scale = gain / (top * dt)
        scale[list(rest)] = 0.0
        x[:, 0:2] = (x[:, 0:2] * scale[batch][:, None]).astype(f32)
        out.append(x)
    return out


def _close(got, want, what):
    got, want = np.asarray(got, f64), np.asarray(want, f64)
    err = np.abs(got - want) / np.where(want != 0, np.abs(want), 1.0)
    assert bool(np.all(err <= RTOL)), (what, got.tolist(), want.tolist())
    return float(err.max())


# courant 1, ratio in [0.5, 1.5], step in [0.4, 2] plan.dt.  The Courant number under the plan's dt, clock by clock:
GAINS = (1e-3, 1e-3, 1e3, 1e3, 1e3, 1.0 / 0.48)
# clock 0: Co = 1e-3, grow: 1.5 dt      clock 1: grow: 2.25 dt, max_factor: 2 dt      clock 2: Co = 2e3, shrink: dt
# clock 3: shrink: 0.5 dt               clock 4: shrink: 0.25 dt, min_factor: 0.4 dt  clock 5: Co = 0.4 / 0.48: fac = 1.2, no clamp
CTL = dict(courant=1.0, grow=1.5, shrink=0.5, min_factor=0.4, max_factor=2.0, keep=8)


@pytest.mark.parametrize("which,scheme", [("B1", "bdf2"), ("B3", "bdf2"), ("poly", "bdf2"), ("rest", "bdf2"), ("B3", "bdf1")])
def test_the_launches_alone_against_the_numpy_rule(which, scheme):
    k = _Alone(which, CTL, scheme)
    cb = k.arr["cbatch"]
    counts = np.bincount(cb, minlength=k.B)
    assert not np.any(counts % 64 == 0), counts
    if which == "B3":
        assert k.B == 3 and len(set(counts.tolist())) == 3
        assert any(cb[w] != cb[min(w + 63, len(cb) - 1)] for w in range(0, len(cb), 64))         # a wavefront of two graphs
        assert any(cb[w] != cb[min(w + 255, len(cb) - 1)] for w in range(256, len(cb), 256))     # a second workgroup of two
    if which == "poly":
        n = np.diff(k.arr["crow"])
        assert len(set(n.tolist())) >= 3, set(n.tolist())
    rest = (1,) if which == "rest" else ()
    fields = _fields_for(k.arr, GAINS, seed=5, rest=rest)
    hits = {"grow": 0, "shrink": 0, "min_factor": 0, "max_factor": 0, "none": 0, "rest": 0}
    worst = {}
    for c, x in enumerate(fields):
        k.launch(x, c)
        want, want32 = k.rule.launch(x, c), k.rule32.launch(x, c)
        got = k.sch.read()
        assert got["clock"] == c and got["order"] == (2 if want["active"] else 1) and want["active"] == (scheme == "bdf2" and c > 0)
        # the maximum must pick the right cell: the runner-up lies further below than the tolerance
        top, second = R.graph_rates(want["rates"], cb, k.B)
        for b in range(k.B):
            assert top[b] == 0.0 if b in rest else (top[b] - second[b]) > 10 * RTOL * top[b], (b, top[b], second[b])
        figs = {"rate": _close(got["rate"], want["rate"], "rate"), "courant": _close(got["courant"], want["courant"], "Co"),
                "dt": _close(got["dt"], want["dt"], "dt_next"), "omega": _close(got["omega"], want["omega"], "omega"),
                "dt_eff": _close(got["dt_eff"], want["dt_eff"], "dt_eff"), "time": _close(got["time"], want["time"], "time")}
        us, batch = got["ustar"].numpy().astype(f64), np.asarray(k.arr["batch"], np.int64)
        for b in range(k.B):
            m = batch == b
            scale = np.abs(want["ustar"][m]).max()
            e = np.abs(us[m] - want["ustar"][m]).max() / scale if scale > 0 else np.abs(us[m]).max()
            assert e <= RTOL, ("ustar", c, b, e)
            figs["ustar"] = max(figs.get("ustar", 0.0), float(e))
        same32 = {n: bool(np.array_equal(got[n].numpy(), want32[n])) for n in ("rate", "dt", "omega", "dt_eff", "ustar")}
        print(f"{which} {scheme} clock {c}: " + ", ".join(f"{n} {v:.1e}" for n, v in figs.items()) + f"; float32 rule bits {same32}")
        for n, v in figs.items():
            worst[n] = max(worst.get(n, 0.0), v)
        # which clamp this launch hit, from the float64 rule
        dt_plan = np.asarray(k.arr["dt"], f64)
        for b in range(k.B):
            co, last = want["courant"][b], want["dt_last"][b]
            if co == 0.0:
                hits["rest"] += 1
                assert b in rest and want["dt"][b] == min(last * k.ctl.grow, k.ctl.max_factor * dt_plan[b])
                continue
            fac = k.ctl.courant / co
            hit = "grow" if fac > k.ctl.grow else "shrink" if fac < k.ctl.shrink else None
            stepped = last * min(max(fac, k.ctl.shrink), k.ctl.grow)
            bound = ("max_factor" if stepped > k.ctl.max_factor * dt_plan[b] else
                     "min_factor" if stepped < k.ctl.min_factor * dt_plan[b] else None)
            for h in (hit, bound):
                if h:
                    hits[h] += 1
            if not hit and not bound:
                hits["none"] += 1
                assert abs(co * want["omega"][b] - k.ctl.courant) < 1e-12         # the target is met in one step
    print(f"{which} {scheme}: clamps hit {hits}, largest errors {worst}")
    for h in ("grow", "shrink", "min_factor", "max_factor", "none"):
        assert hits[h] >= 1, hits
    assert (hits["rest"] > 0) == (which == "rest")
    assert torch.equal(k.plan.dt.cpu(), k.dt_plan)                          # plan.dt is never written
    rows = k.sch.step_history()
    assert [r["clock"] for r in rows] == list(range(len(GAINS)))
    for r in rows:
        _close(r["dt"], k.rule.history[r["clock"]]["dt"], "history dt")
        _close(r["time"], k.rule.history[r["clock"]]["time"], "history time")


# ---- 2. repeatability ------------------------------------------------------------------------------------------------------------
def test_a_launch_that_finds_the_same_clock_writes_the_same_bits():
    ctl = dict(courant=1.0, grow=1.5, shrink=0.5, min_factor=0.4, max_factor=2.0, keep=64)
    k = _Alone("B3", ctl)
    fields = _fields_for(k.arr, (0.7, 1.3, 0.9), seed=9)
    states = []
    for c in range(3):
        k.launch(fields[c], c)
        first = k.buffers()
        k.launch()
        _assert_same(k.buffers(), first, f"clock {c}, again")
        k.sch.launch()
        k.sch.launch()                                                     # back to back, nothing in between
        _assert_same(k.buffers(), first, f"clock {c}, back to back")
        assert int(first["crec"][1]) == 0                                  # the arrival counter is back at zero
        states.append(first)
    assert not torch.equal(states[0]["dts"], states[1]["dts"]) and not torch.equal(states[1]["state"], states[2]["state"])
    assert torch.equal(k.plan.dt.cpu(), k.dt_plan)
    # sixty-six clocks with keep = 64: the history ring wraps; the rows are what read() showed at each clock
    base = fields[0]
    seen = {}
    for c in range(3, 66):
        x = base.copy()
        x[:, 0:2] *= f32(1.0 + 0.3 * np.sin(1.7 * c))
        k.launch(x, c)
        r = k.sch.read()
        seen[c] = (r["dt"], r["courant"], r["time"])
    rows = k.sch.step_history()
    assert [r["clock"] for r in rows] == list(range(2, 66))
    for r in rows[1:]:
        dt, co, tm = seen[r["clock"]]
        _assert_same({"dt": r["dt"], "courant": r["courant"], "time": r["time"]}, {"dt": dt, "courant": co, "time": tm}, r["clock"])
    _assert_same({"dt": rows[0]["dt"]}, {"dt": states[2]["state"][0]}, "row of clock 2")
    # the time of a row is the float64 sum of the steps in front of it
    for a, b in zip(rows[:-1], rows[1:]):
        assert torch.equal(b["time"], a["time"] + a["dt"].double()), b["clock"]


# ---- 3. unit ratio ---------------------------------------------------------------------------------------------------------------
def test_at_unit_ratio_the_launches_write_the_fixed_step_scheme():
    k = _Alone("B3", dict(courant=0.7, grow=1, shrink=1), plain=True)
    g = np.random.default_rng(21)
    fields = [(g.standard_normal((k.N, 12)) + np.arange(12)[None, :]).astype(f32) for _ in range(3)]
    batch = np.asarray(k.arr["batch"], np.int64)
    dim = np.asarray(k.arr["uvp_dim"], f64)[batch][:, 0:2]
    for c in range(3):
        k.put(fields[c], c)
        k.plain.launch()
        k.sch.launch()
        torch.cuda.synchronize()
        a, b = k.sch.read(), k.plain.read()
        assert a["order"] == b["order"] == (2 if c else 1)
        assert torch.equal(a["omega"], torch.ones(k.B)) and torch.equal(a["dt"], k.dt_plan)
        assert torch.equal(k.sch.ring.cpu(), k.plain.ring.cpu())
        d = (a["ustar"].double() - b["ustar"].double()).abs().numpy()
        diff = np.abs(fields[c][:, 0:2].astype(f64) - fields[c - 1][:, 0:2].astype(f64)) / dim if c else np.zeros_like(d)
        scale = np.maximum(b["ustar"].double().abs().numpy(), diff)
        e_u = float((d / scale).max())
        e_dt = float(((a["dt_eff"].double() - b["dt_eff"].double()).abs() / b["dt_eff"].double()).max())
        print(f"clock {c}: ustar {e_u:.1e}, dt_eff {e_dt:.1e}")
        assert e_u <= 1e-6 and e_dt <= 1e-6
        assert e_u == 0.0 and e_dt == 0.0                                 # the divisors are exactly 3 and 1.5: the plain scheme's bits


def test_a_march_at_unit_ratio_matches_the_fixed_step_march():
    fixed = _march("list", "bdf2", tol=None)
    want = fixed.run(levels=4)
    ms = _march("list", _scheme(courant=0.7, grow=1, shrink=1), tol=None)
    got = ms.run(levels=4)
    _, yard = _reference("poly", True, "imex")
    tol = F.tolerance(yard)["losses"]
    assert [r["inner"] for r in got] == [r["inner"] for r in want] == [MAX_INNER] * 4
    worst = 0.0
    for a, b in zip(got, want):
        err = torch.stack([F.col_err(a["losses"][g:g + 1], b["losses"][g:g + 1]) for g in range(ms.plan.B)])
        worst = max(worst, float((err / tol).max()))
        assert bool((err <= tol).all()), (a["level"], err.tolist(), tol.tolist())
    print(f"loss history: at most {worst:.2e} of the tolerance {tol.tolist()}")
    read = ms.time_scheme.read()
    assert torch.equal(read["omega"], torch.ones(ms.plan.B)) and torch.equal(read["dt"], ms.plan.dt.cpu())
    assert torch.equal(read["time"], 4.0 * ms.plan.dt.cpu().double())


# ---- 4. device-decided equals host-driven ------------------------------------------------------------------------------------------
MARCH_CTL = dict(courant=2.0, grow=1.5, shrink=0.5, min_factor=0.1, max_factor=4.0, keep=16)
LEVELS = 3


def _control_state(sch):
    """What the controller shows, free of the clock's parity (two objects may count their clocks from different fields)."""
    r = sch.read()
    return {k: r[k].clone() for k in ("ustar", "dt_eff", "dt", "omega", "courant", "time", "dt_last")}


@functools.lru_cache(maxsize=None)
def _host_driven():
    """TrainStep with a fixed-step scheme whose two tensors the HOST overwrites after every level, with a synchronisation: the
    numpy rule in float32 on the field as the device holds it."""
    from gfv.timescheme import TimeScheme
    from gfv.trainer import TrainStep
    ts = TrainStep(_model(), _graphs(), lr=LR, use_graph=False, time_scheme=TimeScheme("bdf2"))
    rule = R.StepRule(R.plan_arrays(ts.plan), _control(**MARCH_CTL), R.BDF2, f32)
    rule.reset(0)
    outs = []

    def apply(clock):
        torch.cuda.synchronize()
        out = rule.launch(ts.x_backup.cpu().numpy(), clock)
        ts.time_scheme.ustar.copy_(torch.from_numpy(out["ustar"]))
        ts.time_scheme.dt_eff.copy_(torch.from_numpy(out["dt_eff"]))
        outs.append(out)

    apply(0)
    for level in range(LEVELS):
        for _ in range(MAX_INNER):
            ts.step()
        ts.advance_time()
        apply(level + 1)
    last = outs[-1]
    ctl = {k: torch.from_numpy(np.ascontiguousarray(last[k])) for k in ("ustar", "dt_eff", "dt", "omega", "courant", "time", "dt_last")}
    print("host-driven steps:", [o["dt"].tolist() for o in outs], "Courant numbers:", [o["courant"].tolist() for o in outs])
    assert any(float(o["omega"][0]) != 1.0 for o in outs)                  # the step did change
    return _named_state(ts), ctl


@pytest.mark.parametrize("owner,mode", [("march", False), ("march", "list"), ("train", False), ("train", "list"), ("train", True)],
                         ids=["march-eager", "march-list", "train-eager", "train-list", "train-hipgraph"])
def test_the_device_decided_march_equals_the_host_driven_loop(owner, mode):
    from gfv.trainer import TrainStep
    want, want_ctl = _host_driven()
    sch = _scheme(**MARCH_CTL)
    if owner == "march":
        ms = _march(mode, sch, tol=None)
        rows = ms.run(levels=LEVELS)
        assert [r["inner"] for r in rows] == [MAX_INNER] * LEVELS
    else:
        ms = TrainStep(_model(), _graphs(), lr=LR, use_graph=mode, time_scheme=sch)
        for _ in range(LEVELS):
            for _ in range(MAX_INNER):
                ms.step()
            ms.advance_time()
    _assert_same(_named_state(ms), want, f"{owner} {mode}")
    _assert_same(_control_state(sch), want_ctl, f"{owner} {mode} controller")
    assert sch.read()["clock"] == LEVELS and [r["clock"] for r in sch.step_history()] == list(range(LEVELS + 1))


# ---- 5. run-ahead and held steps ---------------------------------------------------------------------------------------------------
def _history_state(sch):
    rows = sch.step_history()
    return {f"{k}{r['clock']}": r[k] for r in rows for k in ("dt", "courant", "time")}


def test_run_ahead_and_held_steps_leave_the_same_bits():
    outs = []
    for ahead in (0, 32):
        ms = _march("list", _scheme(**MARCH_CTL))
        ms.run(levels=3, max_ahead=ahead)
        outs.append((_named_state(ms), _control_state(ms.time_scheme), _history_state(ms.time_scheme), ms.stats()))
    assert outs[0][3]["held"] == 0
    for i, what in enumerate(("state", "controller", "history")):
        _assert_same(outs[0][i], outs[1][i], f"run-ahead {what}")
    print("held with max_ahead=32:", outs[1][3]["held"])
    held = ms.stats()["held"]
    for _ in range(3):
        ms.step()
    assert ms.stats()["held"] == held + 3
    _assert_same(_named_state(ms), outs[1][0], "held")
    _assert_same(_control_state(ms.time_scheme), outs[1][1], "held controller")
    _assert_same(_history_state(ms.time_scheme), outs[1][2], "held history")


# ---- 6. resume ---------------------------------------------------------------------------------------------------------------------
def test_a_resumed_march_continues_with_the_step_and_the_time_it_had():
    whole = _march("list", _scheme(**MARCH_CTL))
    whole.run(levels=5, max_ahead=8)
    first = _march("list", _scheme(**MARCH_CTL))
    first.run(levels=3, max_ahead=8)
    sd = first.state_dict()
    saved = sd["gfv_time_scheme"]
    assert saved["has_previous"] and tuple(saved["dt_last"].shape) == tuple(saved["time"].shape) == (first.plan.B,)
    assert saved["time"].dtype == torch.float64 and float(saved["time"][0]) > 0 and not saved["time"].is_cuda
    second = _carry_over(first, _scheme(**MARCH_CTL))
    second.load_state_dict(sd)
    _assert_same(_control_state(second.time_scheme), _control_state(first.time_scheme), "installed")
    second.run(levels=2, max_ahead=8)
    _assert_same(_named_state(second), _named_state(whole), "resumed")
    _assert_same(_control_state(second.time_scheme), _control_state(whole.time_scheme), "resumed controller")
    # a dict without the step and the time loads as before: the plan's dt, time 0
    third = _carry_over(first, _scheme(**MARCH_CTL))
    old = dict(sd, gfv_time_scheme={k: v for k, v in saved.items() if k not in ("dt_last", "time")})
    third.load_state_dict(old)
    r = third.time_scheme.read()
    assert r["order"] == 2 and torch.equal(r["dt_last"], third.plan.dt.cpu()) and torch.equal(r["time"], torch.zeros(third.plan.B).double())


# ---- 7. the controller does something -----------------------------------------------------------------------------------------------
def test_the_step_of_a_cavity_started_from_rest_grows_to_the_target():
    """Measured on the MI355X: see the printed history (DESIGN.md 5x quotes it)."""
    from gfv import meshgen
    from gfv.graph import build_batch
    from gfv.march import MarchStep
    from gfv.plan import get_plan
    m = meshgen.finish_mesh(meshgen.raw_quad_cavity(n=6, jitter=0.1, tri_fraction=0.0, seed=13), U=1.0)
    start = m["init_uvp"].astype(f32).copy()
    start[m["node|node_type"] == meshgen.NORMAL] = 0.0                     # at rest; the lid moves
    graphs = build_batch([m], [start], device="cuda")
    arr = R.plan_arrays(get_plan(graphs))
    rates = R.cell_rates(graphs[0].x.cpu().numpy(), arr["uvp_dim"], arr["crow"], arr["knode"], arr["kS"], arr["area"], arr["cbatch"])
    co0 = float(rates.max() * f64(arr["dt"][0]))
    assert co0 > 0
    grow, max_factor, levels = 1.5, 20.0, 8
    sch = _scheme(courant=10.0 * co0, grow=grow, shrink=0.25, min_factor=0.05, max_factor=max_factor, keep=32)
    ms = MarchStep(_model(), graphs, lr=LR, use_graph="list", tol=None, max_inner=2, max_levels=levels + 1, time_scheme=sch)
    ms.run(levels=levels)
    rows = sch.step_history()
    assert [r["clock"] for r in rows] == list(range(levels + 1))
    dt_plan = f32(arr["dt"][0])
    target = f32(10.0 * co0)
    last = dt_plan
    grown = 0
    print("clock, dt / plan.dt, Courant number / target, time:")
    for r in rows:
        dt, co = f32(r["dt"][0]), f32(r["courant"][0])
        print(f"  {r['clock']}  {dt / dt_plan:.4f}  {co / target:.4f}  {float(r['time'][0]):.6f}")
        assert dt <= f32(max_factor) * dt_plan
        if 0 < co * f32(grow) < target:                                    # below the band: the ratio is clamped at grow
            assert dt == min(f32(last * f32(grow)), f32(max_factor) * dt_plan), r["clock"]
            grown += 1
        last = dt
    assert f32(rows[0]["dt"][0]) == f32(dt_plan * f32(grow)) and grown >= 1      # by construction: Co of the start is target / 10
    total = torch.zeros(1, dtype=torch.float64)
    for r in rows[:-1]:
        total = total + r["dt"].double()
    assert torch.equal(rows[-1]["time"], total) and torch.equal(sch.read()["time"], total)
    assert torch.equal(ms.plan.dt.cpu(), torch.from_numpy(np.asarray(arr["dt"])))
