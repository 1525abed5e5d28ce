"""Unsteady boundary data: the inflow (or lid) velocity and the body force as functions of time, rewritten on the device.

`Rollout` and `MarchStep` run unsteady cases with no synchronisation per step, but what drives the case - the Dirichlet targets
`plan.y` and the PDE coefficients `plan.theta` - was frozen when the plan was built.  The reference re-evaluates a time-dependent
source every time step (Load_mesh/Graph_loader.py:323-362 `update_env`) and forms `sin(f pi dt k)` from the step index
(Load_mesh/Set_BC.py:68-113).  `TimeBC` is one small launch behind the launch that advances the field (`gfv_time_bc_update`,
csrc/timebc.hip, include/gfv.h), following the owner's clock - `Rollout`'s step counter, `MarchStep`'s level count - the way
`FieldStats` does:

    tbc = TimeBC(velocity=Sine(mean=1.0, amp=0.3, freq=0.2), source=None, nodes=("inflow",))
    r = Rollout(model, graphs, max_steps=1000, time_bc=tbc)
    ms = MarchStep(model, graphs, max_inner=20, tol=1e-2, time_bc=TimeBC(velocity=Ramp(0.0, 1.0, 0.0, 5.0, "smooth")))
    tbc.read()                      # {"clock" [k], "t" [k,B], "velocity" [k,B], "source" [k,B]}: what was applied (synchronises)
    tbc.set(velocity=..., graph=b)  # a new waveform under a recorded list (device record: nothing is recorded again)
    tbc.evaluate(clock)             # stand-alone: (y [N,2], theta5 [B]) for that clock from scratch tensors, owner state untouched
    tbc.rebase()                    # re-read the base targets after the caller edited graph_node.y / theta_PDE in place

The clock counts fields: the field the first step (the first completed level) computes has clock 1, and the launch behind the
advance that has written field c writes the data for field c + 1.  `attach()`, the owner's `reset()` and `set()` issue the launch
once themselves, so the data of the next field are always in place.  Waveforms g(t) are evaluated in float64 at
t = clock * (double)plan.dt[b]:

    Const(value)                              g = value
    Ramp(g0, g1, t0, t1, shape)               s = clamp((t - t0) / (t1 - t0), 0, 1); "linear": g0 + (g1 - g0) s; "smooth": g0 + (g1 - g0) s s (3 - 2 s)
    Sine(mean, amp, freq, phase, start)       g = mean + amp sin(2 pi freq max(t - start, 0) + phase)
    Table(times, values, periodic)            piecewise linear through at most 1024 points, clamped outside; periodic: t wrapped
                                              into [times[0], times[-1]) by fmod

What a launch writes, for graph b and node i of b: `plan.y[i, 0:2] = float32(g_v * y0[i, 0:2])` where `node_type[i]` is one of
`nodes` (every other row stays bit for bit); `plan.theta[b, 5] = float32(g_s * theta0[b, 5])` and the same float in node-feature
column 8 of every node of b, in `x_backup` (what the next forward's input preparation reads) and in `x` (the advance launches keep
x == x_backup between steps; nothing of the forward reads it); one history row (t, g_v, g_s) in float64.  A channel given as None
is not written at all (its history column holds 1).  `y0` and `theta0` are this object's own copies taken at `attach()`; the kernel
never reads what it writes, so a launch that finds the same clock - an inner iteration or a held step of a march - writes the same
bits again.

`plan.y` MAY ALIAS THE CALLER'S `graph_node.y` (a contiguous float32 [N, 2] tensor is used as it is), and `plan.theta` the caller's
`theta_PDE`: the launch then writes into the caller's tensors.  After an in-place edit of either, call `rebase()`: whatever the
masked rows hold then becomes the new base.

Who owns what a recorded list points at: DESIGN.md 5l.  Particular to this object, allocated once when its owner attaches it and
never reallocated: the records, the table slots, the control words, the base copies and the history.  One owner per object.
"""
from __future__ import annotations

import math
import numbers
import weakref

import torch

from . import lib as L
from .follow import Follower

NODE_TYPES = {"inflow": 1, "wall": 3, "in_wall": 5}      # utils/utilities.py NodeType
DEFAULT_NODES = ("inflow", "in_wall")
SOURCE_COLUMN = 5                                         # of theta_PDE; node-feature column 3 + 5
UNCHANGED = object()


def _num(name, v):
    if isinstance(v, bool) or not isinstance(v, numbers.Real):
        raise ValueError(f"{name} must be a number, got {v!r}")
    v = float(v)
    if not math.isfinite(v):
        raise ValueError(f"{name} must be finite, got {v!r}")
    return v


class Waveform:
    """g(t); `pack()` -> (the record's GFV_TIME_BC_RECORD doubles, times or None, values or None)."""
    _fields = ()

    def __eq__(self, other):
        return type(self) is type(other) and all(getattr(self, f) == getattr(other, f) for f in self._fields)

    def __repr__(self):
        return f"{type(self).__name__}({', '.join(f'{f}={getattr(self, f)!r}' for f in self._fields)})"

    def _rec(self, kind, *params):
        return [float(kind)] + list(params) + [0.0] * (L.TIME_BC_RECORD - 1 - len(params))


class Const(Waveform):
    _fields = ("value",)

    def __init__(self, value=1.0):
        self.value = _num("value", value)

    def pack(self):
        return self._rec(L.TIME_BC_CONST, self.value), None, None


class Ramp(Waveform):
    _fields = ("g0", "g1", "t0", "t1", "shape")

    def __init__(self, g0, g1, t0, t1, shape="linear"):
        self.g0, self.g1, self.t0, self.t1 = _num("g0", g0), _num("g1", g1), _num("t0", t0), _num("t1", t1)
        if shape not in ("linear", "smooth"):
            raise ValueError(f'shape must be "linear" or "smooth", got {shape!r}')
        if not self.t1 > self.t0:
            raise ValueError(f"Ramp needs t1 > t0, got t0 = {self.t0}, t1 = {self.t1}")
        if not math.isfinite(self.t1 - self.t0) or not math.isfinite(self.g1 - self.g0):
            raise ValueError("Ramp: t1 - t0 and g1 - g0 must be finite")
        self.shape = shape

    def pack(self):
        kind = L.TIME_BC_RAMP_SMOOTH if self.shape == "smooth" else L.TIME_BC_RAMP_LINEAR
        return self._rec(kind, self.g0, self.g1, self.t0, self.t1), None, None


class Sine(Waveform):
    _fields = ("mean", "amp", "freq", "phase", "start")

    def __init__(self, mean, amp, freq, phase=0.0, start=0.0):
        self.mean, self.amp, self.freq = _num("mean", mean), _num("amp", amp), _num("freq", freq)
        self.phase, self.start = _num("phase", phase), _num("start", start)
        if self.freq < 0:
            raise ValueError(f"freq must be at least 0, got {self.freq}")

    def pack(self):
        return self._rec(L.TIME_BC_SINE, self.mean, self.amp, self.freq, self.phase, self.start), None, None


class Table(Waveform):
    _fields = ("times", "values", "periodic")

    def __init__(self, times, values, periodic=False):
        times, values = list(times), list(values)
        if len(times) != len(values):
            raise ValueError(f"Table: {len(times)} times for {len(values)} values")
        if not 1 <= len(times) <= L.TIME_BC_TABLE_MAX:
            raise ValueError(f"Table: 1 .. {L.TIME_BC_TABLE_MAX} points, got {len(times)}")
        self.times = tuple(_num("times", t) for t in times)
        self.values = tuple(_num("values", v) for v in values)
        if any(not b > a for a, b in zip(self.times, self.times[1:])):
            raise ValueError("Table: times must be strictly increasing")
        if not math.isfinite(self.times[-1] - self.times[0]):
            raise ValueError("Table: the span of the times must be finite")
        self.periodic = bool(periodic)
        if self.periodic and len(self.times) < 2:
            raise ValueError("Table: a periodic table needs at least 2 points")

    def pack(self):
        kind = L.TIME_BC_TABLE_PERIODIC if self.periodic else L.TIME_BC_TABLE
        return self._rec(kind, float(len(self.times))), list(self.times), list(self.values)


def unpack(rec, times=None, values=None):
    """The waveform of a packed record (and, for a table, its slot's times and values) - pack()'s inverse."""
    rec = [float(v) for v in rec]
    kind = int(rec[0])
    if kind == L.TIME_BC_CONST:
        return Const(rec[1])
    if kind in (L.TIME_BC_RAMP_LINEAR, L.TIME_BC_RAMP_SMOOTH):
        return Ramp(rec[1], rec[2], rec[3], rec[4], "smooth" if kind == L.TIME_BC_RAMP_SMOOTH else "linear")
    if kind == L.TIME_BC_SINE:
        return Sine(rec[1], rec[2], rec[3], rec[4], rec[5])
    if kind in (L.TIME_BC_TABLE, L.TIME_BC_TABLE_PERIODIC):
        n = int(rec[1])
        return Table([float(t) for t in times[:n]], [float(v) for v in values[:n]], kind == L.TIME_BC_TABLE_PERIODIC)
    raise ValueError(f"not a waveform record: kind {rec[0]!r}")


def _check_channel(name, spec):
    if spec is None or isinstance(spec, Waveform):
        return spec
    if isinstance(spec, (list, tuple)):
        if not spec or any(not isinstance(w, Waveform) for w in spec):
            raise ValueError(f"{name}: a list must hold one waveform per graph (Const, Ramp, Sine or Table)")
        return list(spec)
    raise ValueError(f"{name} must be a waveform (Const, Ramp, Sine, Table), a list of one per graph or None, got {spec!r}")


def check_time_bc_args(velocity, source, nodes):
    """The constructor's checks; needs no GPU.  -> (velocity, source, type_mask)."""
    velocity, source = _check_channel("velocity", velocity), _check_channel("source", source)
    if velocity is None and source is None:
        raise ValueError("TimeBC: velocity=None together with source=None drives nothing")
    if isinstance(nodes, str):
        nodes = (nodes,)
    nodes = tuple(nodes)
    unknown = [n for n in nodes if n not in NODE_TYPES]
    if unknown:
        raise ValueError(f"unknown node names {unknown}: nodes is a subset of {tuple(NODE_TYPES)}")
    if velocity is not None and not nodes:
        raise ValueError("TimeBC: a velocity waveform needs at least one node name")
    mask = 0
    for n in nodes:
        mask |= 1 << NODE_TYPES[n]
    return velocity, source, mask


def per_graph(name, spec, B):
    """One waveform per graph from a channel's spec; a list whose length is not B is refused.  Needs no GPU."""
    if spec is None:
        return None
    if isinstance(spec, Waveform):
        return [spec] * B
    if len(spec) != B:
        raise ValueError(f"{name}: {len(spec)} waveforms for a batch of {B} graphs")
    return list(spec)


def check_graphs(graphs):
    """Batches of a DevicePool are refused (their plan's tensors ARE the pool's state: `reset_env` and the renewal launches own
    them).  Needs no GPU."""
    if getattr(graphs[0], "_gfv_pool_plan", None) is not None:
        raise ValueError("TimeBC: graphs of a DevicePool are not supported (the pool owns their boundary targets and coefficients; "
                         "Sweep and PoolTrainStep are out of scope)")


def check_owner(time_bc, graphs=None, anderson=0):
    """What an owner refuses of `time_bc=`; needs no GPU."""
    TimeBC.check_handed(None, time_bc, graphs, anderson)


class TimeBC(Follower):
    KEYWORD = "time_bc"
    NO_ANDERSON = "a boundary condition that follows the step count has no meaning for them"

    def __init__(self, velocity=None, source=None, nodes=DEFAULT_NODES):
        self._velocity, self._source, self.type_mask = check_time_bc_args(velocity, source, nodes)
        self.nodes = (nodes,) if isinstance(nodes, str) else tuple(nodes)
        self.channels = (1 if self._velocity is not None else 0) | (2 if self._source is not None else 0)
        self._owner_ref = None
        self.rec = self.tab = self.ctl = self.hist = self.y0 = self.theta0 = None    # device state: allocated by attach(), never
        self._scratch = None                                                         # reallocated (evaluate()'s scratch: on first use)
        self._waves = None          # [B][2] waveforms (None for a channel that is off)
        self._offset = 0

    # ---- the owner's side (gfv/follow.py) -------------------------------------------------------------------------------------
    def _check_graphs(self, graphs):
        check_graphs(graphs)
        self.resolve(int(graphs[4].theta_PDE.shape[0]))

    def resolve(self, B):
        """-> (velocity, source) as one waveform per graph (or None); refuses a list whose length is not B.  Needs no GPU."""
        return per_graph("velocity", self._velocity, B), per_graph("source", self._source, B)

    def attach(self, owner, graphs, plan, x_backup, x, clock, clock_word, k_max):
        """Called by the owner's constructor: `clock` is the owner's int32 record, `clock_word` the word of it that counts the
        fields written, `k_max` the fields it can write.  Allocates the device state (once), takes the base copies and issues the
        launch for the first field.  -> self"""
        self.check_free()
        check_graphs(graphs)
        B, N = int(plan.B), int(plan.N)
        vel, src = self.resolve(B)
        if not x_backup.is_cuda:
            raise ValueError("TimeBC: the node state must live on the GPU (the boundary data are written by a HIP kernel; there is "
                             "no CPU path)")
        dev = x_backup.device
        self._graphs, self._plan, self._xb, self._x = graphs, plan, x_backup, x
        self._clock, self._clock_ptr = clock, clock.data_ptr() + 4 * int(clock_word)
        self.B, self.N, self.k_max = B, N, int(k_max) + 1            # (+ 1: the data of the field behind the last one are written too)
        self.rec = torch.zeros((B, 2, L.TIME_BC_RECORD), dtype=torch.float64, device=dev)
        self.tab = torch.zeros((B, 2, 2, L.TIME_BC_TABLE_MAX), dtype=torch.float64, device=dev)
        self.ctl = torch.zeros(L.TIME_BC_CTL, dtype=torch.int32, device=dev)
        self.hist = torch.zeros((self.k_max, B, L.TIME_BC_HIST), dtype=torch.float64, device=dev)
        self.y0 = plan.y.detach().clone()
        self.theta0 = plan.theta[:, SOURCE_COLUMN].detach().clone().contiguous()
        self._scratch = None
        self._offset = 0
        self._waves = [[None, None] for _ in range(B)]
        for b in range(B):
            for ch, ws in enumerate((vel, src)):
                if ws is not None:
                    self._write_wave(b, ch, ws[b])
        self.launch()
        self._owner_ref = weakref.ref(owner)        # (weak: rebase() tells a TrainStep that the plan is fresh)
        self._claim(owner)
        return self

    def launch(self):
        """The one launch, behind the owner's advance: part of the step body (eager steps and recorded lists carry it alike)."""
        pl = self._plan
        L.check(L.load().gfv_time_bc_update(
            self._clock_ptr, self.ctl.data_ptr(), self.rec.data_ptr(), self.tab.data_ptr(), pl.dt.data_ptr(), pl.batch.data_ptr(),
            pl.node_type.data_ptr(), self.N, self.B, self.y0.data_ptr(), pl.y.data_ptr(), self.theta0.data_ptr(),
            pl.theta.data_ptr() + 4 * SOURCE_COLUMN, int(pl.theta.shape[1]), self._xb.data_ptr(), self._x.data_ptr(),
            self.hist.data_ptr(), self.k_max, self.type_mask, self.channels, L.stream_ptr()), "gfv_time_bc_update")

    def reset(self):
        """The owner's reset() calls it behind clearing its clock: the history is cleared, the clock offset dropped and the data of
        field 1 written."""
        self._need()
        self.hist.zero_()
        self._set_offset(0)
        self.launch()

    def set_clock_offset(self, offset):
        """Fields that came before this owner's clock started (a resumed run): the launch evaluates clock + offset.  Writes the
        data of the next field.  `MarchStep.load_state_dict` calls it."""
        self._need()
        offset = int(offset)
        if offset < 0:
            raise ValueError(f"the clock offset must be at least 0, got {offset}")
        self._set_offset(offset)
        self.launch()

    clock_offset = property(lambda self: self._offset)

    def _set_offset(self, offset):
        self._offset = offset
        self.ctl[0:1].copy_(torch.tensor([offset], dtype=torch.int32))

    # ---- the records ---------------------------------------------------------------------------------------------------------------
    def _write_wave(self, b, ch, w):
        rec, times, values = w.pack()
        self.rec[b, ch].copy_(torch.tensor(rec, dtype=torch.float64))
        if times is not None:
            n = len(times)
            self.tab[b, ch, 0, :n].copy_(torch.tensor(times, dtype=torch.float64))
            self.tab[b, ch, 1, :n].copy_(torch.tensor(values, dtype=torch.float64))
        self._waves[b][ch] = w

    def waveforms(self, graph):
        """(velocity, source) of one graph as set (None for a channel that is off)."""
        self._need()
        return tuple(self._waves[int(graph)])

    def set(self, velocity=UNCHANGED, source=UNCHANGED, graph=None):
        """A new waveform for one graph (`graph=b`) or for all of them (one waveform, or a list of B), checked before anything
        changes.  It reaches recorded lists through the device record: nothing is recorded again.  The data of the next field are
        written again with it: it holds from the next step issued.  A channel that was built as None stays off."""
        self._need()
        todo = []
        for ch, (name, spec) in enumerate((("velocity", velocity), ("source", source))):
            if spec is UNCHANGED:
                continue
            if not self.channels & (1 << ch):
                raise ValueError(f"TimeBC.set: the {name} channel was built as None (its rows are never written)")
            spec = _check_channel(name, spec)
            if spec is None:
                raise ValueError(f"TimeBC.set: {name}=None would switch a channel off; use Const(1.0)")
            if graph is None:
                todo += [(b, ch, w) for b, w in enumerate(per_graph(name, spec, self.B))]
            else:
                b = int(graph)
                if not 0 <= b < self.B:
                    raise IndexError(f"graph {graph} of a batch of {self.B}")
                if not isinstance(spec, Waveform):
                    raise ValueError(f"TimeBC.set: graph={graph} takes one waveform")
                todo.append((b, ch, spec))
        for b, ch, w in todo:
            self._write_wave(b, ch, w)
        if todo:
            self.launch()

    def rebase(self):
        """Re-read the base targets after the caller edited `graph_node.y` / `theta_PDE` in place: the plan's copies are refreshed
        the way the owner's next step would, `y0` and `theta0` are taken again from what the plan holds, and the data of the next
        field are written from them."""
        self._need()
        from .plan import _live_key, get_plan
        get_plan(self._graphs)
        owner = self._owner_ref() if self._owner_ref is not None else None
        if owner is not None and hasattr(owner, "_live"):
            owner._live = _live_key(self._graphs)      # (TrainStep.step would otherwise refresh once more, over the launch's rows)
        self.y0.copy_(self._plan.y)
        self.theta0.copy_(self._plan.theta[:, SOURCE_COLUMN])
        if self._scratch is not None:
            self._scratch[0].copy_(self.y0)
            self._scratch[1].copy_(self.theta0)
        self.launch()

    # ---- reading ---------------------------------------------------------------------------------------------------------------------
    def evaluate(self, clock):
        """(y [N, 2] float32, theta5 [B] float32) as the launch would write them for field `clock` (rows outside the mask, and a
        channel that is off, hold the base values), from scratch tensors of this object: the owner's state, the plan and the
        history are untouched.  Device tensors (copies); no synchronisation."""
        self._need()
        clock = int(clock)
        if not 1 <= clock < 2 ** 31:
            raise ValueError(f"clock must be at least 1 (the first field computed), got {clock}")
        if self._scratch is None:
            dev = self.rec.device
            self._scratch = (self.y0.clone(), self.theta0.clone(), torch.zeros(1, dtype=torch.int32, device=dev),
                             torch.zeros(L.TIME_BC_CTL, dtype=torch.int32, device=dev))
        y, th, ck, ctl = self._scratch
        pl = self._plan
        ck.copy_(torch.tensor([clock - 1], dtype=torch.int32))
        L.check(L.load().gfv_time_bc_update(
            ck.data_ptr(), ctl.data_ptr(), self.rec.data_ptr(), self.tab.data_ptr(), pl.dt.data_ptr(), pl.batch.data_ptr(),
            pl.node_type.data_ptr(), self.N, self.B, self.y0.data_ptr(), y.data_ptr(), self.theta0.data_ptr(), th.data_ptr(), 1,
            None, None, None, 0, self.type_mask, self.channels, L.stream_ptr()), "gfv_time_bc_update")
        return y.clone(), th.clone()

    def read(self):
        """{"clock" [k] int64, "t" [k, B], "velocity" [k, B], "source" [k, B]} float64 CPU tensors: the time and the two factors
        applied for every field whose data have been written so far - clocks 1 .. k with k = fields computed + 1 (the data of the
        next field are already in place), from the clock offset on for a resumed run.  A channel that is off reads 1.
        Synchronises."""
        self._need()
        done = int(self._clock.cpu()[(self._clock_ptr - self._clock.data_ptr()) // 4])
        first, last = self._offset, min(done + 1 + self._offset, self.k_max)
        h = self.hist[first:last].cpu()
        return {"clock": torch.arange(first + 1, last + 1, dtype=torch.int64), "t": h[:, :, 0].clone(),
                "velocity": h[:, :, 1].clone(), "source": h[:, :, 2].clone()}
