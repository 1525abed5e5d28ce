"""Time differencing of a march: second-order BDF2, its history kept on the device.

What `TrainStep.step()` x k + `advance_time()` and `MarchStep` march with is first order in time: the momentum residual's time term
is `theta0 * (u_new - u_old) / dt * area` (csrc/fvm.hip `cell_fwd_kernel`) with `u_old` the one previous level - backward Euler,
whichever of explicit / implicit / imex chooses the velocity of the fluxes.  The term is linear in `u_old` and it is the only place
`dt` enters the finite-volume section, so the second-order backward difference is the same term with two substitutions:

    u_old -> u* = u_n + (u_n - u_{n-1}) / 3        dt -> dt / 1.5        (u - u*) / (dt / 1.5) = (3 u - 4 u_n + u_{n-1}) / (2 dt)

What is missing is the history: only the device knows which step of a `MarchStep` ends a level, so only the device can rotate
u_{n-1} <- u_n at the right moment.  `TimeScheme` is one small launch behind the launch that advances the field
(`gfv_time_scheme_update`, csrc/timescheme.hip, include/gfv.h), following the owner's clock the way `FieldStats` and `TimeBC` do:

    ms = MarchStep(model, graphs, ..., time_scheme=TimeScheme("bdf2"))
    ts = TrainStep(model, graphs, ..., time_scheme=TimeScheme("bdf2"))      # ts.step() x k; ts.advance_time()
    sch = TimeScheme("bdf2", previous=u_minus_1)   # field -1 [N, 2] (or [N, >= 2]: columns 0:2), dimensional: second order at once
    sch.read()       # {"clock", "order", "ustar", "previous" or None, "dt_eff"} (synchronises)
    sch.reset()      # history forgotten: the level that comes next is first order again (the owner's reset() calls it)
    sch.state_dict() / sch.load_state_dict()

The clock counts fields written: `x_backup` holds field `clock`, field 0 is the initial state.  For a `MarchStep` it is the level
count of the march record, for a `TrainStep` a word of this object's own that `advance_time()` bumps in stream order.  The launch
keeps the velocity columns of the last two fields in a ring, one slot per clock parity, and writes the two tensors the
finite-volume section reads with `Engine.forward(..., time_state=(ustar, dt_eff))`: `ustar` [N, 2], the dimensionless baseline of
the time difference in the form the input preparation's `uv_old` has, and `dt_eff` [B].  The scheme is second order from the first
level that has two fields behind it (clock > base); until then - the start-up level, and always with "bdf1" - `ustar` has the bits
of `uv_old` and `dt_eff` the bits of the plan's dt, and the step is bit-identical to a step without a scheme.  A launch that finds
the clock it found before (an inner iteration, a held step) writes the same bits again.  `plan.dt` is never written.

Second order in time is "bdf2" TOGETHER WITH `integrator="implicit"`: the fluxes are then evaluated at the new level.  With imex /
explicit the scheme is accepted and only the time term changes - the fluxes keep their u_n-based `uv_hat`.  `Rollout`, `Sweep` and
`PoolTrainStep` take no scheme.

Adaptive step.  Without `adapt=` the step is the plan's dt, a constant of the mesh file.  With it the device sizes
every level's step to a Courant-number target, and "bdf2" takes its variable-step form:

    ctl = StepControl(courant=2.0, grow=1.5, shrink=0.25, min_factor=0.05, max_factor=20.0, keep=1024)
    ms  = MarchStep(model, graphs, ..., time_scheme=TimeScheme("bdf2", adapt=ctl))     # also "bdf1", also TrainStep
    sch.read()          # gains "dt" [B] (the step of the level being computed), "time" [B] float64 (the time of field `clock`),
                        # "courant" [B] (the Courant number field `clock` had under the step that produced it), "omega" [B]
    sch.step_history()  # rows {"clock", "dt" [B], "courant" [B], "time" [B]} of the last `keep` fields, oldest first; synchronises

Two launches take the place of the one (`gfv_step_control_rate`, `gfv_step_control_rows`, csrc/stepcontrol.hip), per graph b:

    rate    = max over the cells j of  sum_k |u_j . kS[k]| / (2 area[j]),  u_j the mean dimensionless velocity of the cell's nodes
    dt_last = the step that produced field `clock` (the plan's dt at clock == base);   Co = rate * dt_last
    fac     = Co > 0 ? courant / Co : grow, clamped to [shrink, grow]
    dt_next = clamp(dt_last * fac, min_factor * plan.dt, max_factor * plan.dt);   omega = dt_next / dt_last
    second order active:  ustar = u_n + omega^2 / (1 + 2 omega) (u_n - u_{n-1}),  dt_eff = dt_next (1 + omega) / (1 + 2 omega)
    otherwise:            ustar = u_n,  dt_eff = dt_next
    time[clock] = time[clock - 1] + dt_last  in float64;  time[base] = 0, or what install_previous / load_state_dict were given

The two weights are applied as divisions by (1 + 2 omega) / omega^2 and (1 + 2 omega) / (1 + omega): at omega = 1 these are exactly
3 and 1.5, so `StepControl(grow=1, shrink=1)` marches with the bits of the scheme without `adapt=`.

A row of the history is what `read()` shows at that clock: the time of row k + 1 is the time of row k plus the "dt" of row k.  The
per-graph state is kept by clock parity like the ring, so an inner iteration or a held step - a launch that finds the clock it
found before - writes the same bits everywhere, the history row included.  `state_dict()` gains "dt_last" [B] and "time" [B];
`load_state_dict()` installs them, a dict without them loads as before.  `adapt=` is refused together with `time_bc=` (it forms
t = clock * plan.dt) and `field_stats=` (its means are unweighted in time).  `adapt=None` (the default): the one launch, the same
bits, nothing allocated.

Who owns what a recorded list points at: DESIGN.md 5l.  Particular to this object, allocated once when its owner attaches it and
never reallocated: the ring, `ustar`, `dt_eff`, the record and its own clock word.  One owner per object.  `MarchStep.state_dict()`
carries the scheme's state (`gfv_time_scheme`); `TrainStep.state_dict()` stays the optimiser's: save `sch.state_dict()` beside it.
"""
from __future__ import annotations

import math
import numbers

import torch

from . import lib as L
from .follow import Follower

SCHEMES = {"bdf1": L.TIME_SCHEME_BDF1, "bdf2": L.TIME_SCHEME_BDF2}
SCHEME, BASE = 0, 1        # words of the record (include/gfv.h gfv_time_scheme_update)
TBASE = 0                  # word of the control record (include/gfv.h gfv_step_control_rate)
ST_DT, ST_OMEGA, ST_COURANT, ST_RATE = range(4)     # rows of the per-graph state
BDF2_MAX_GROW = 2.4        # variable-step BDF2 is zero-stable for step ratios below 1 + sqrt(2) = 2.414...


class StepControl:
    """The controller of an adaptive step (`TimeScheme(..., adapt=)`): the Courant-number target, the bounds of the step ratio
    per level (`shrink` <= dt_next / dt_last <= `grow`), the bounds of the step as multiples of the plan's dt, and the number of
    history rows kept on the device.  The constructor's checks need no GPU."""

    def __init__(self, courant=2.0, grow=1.5, shrink=0.25, min_factor=0.05, max_factor=20.0, keep=1024):
        vals = {}
        for name, v in (("courant", courant), ("grow", grow), ("shrink", shrink), ("min_factor", min_factor),
                        ("max_factor", max_factor)):
            if isinstance(v, bool) or not isinstance(v, numbers.Real) or not math.isfinite(v):
                raise ValueError(f"StepControl: {name} must be a finite number, got {v!r}")
            vals[name] = float(v)
        if not vals["courant"] > 0:
            raise ValueError(f"StepControl: courant must be > 0, got {courant!r}")
        if not 0 < vals["shrink"] <= 1 <= vals["grow"]:
            raise ValueError(f"StepControl: 0 < shrink <= 1 <= grow is required, got shrink = {shrink!r}, grow = {grow!r}")
        if not 0 < vals["min_factor"] <= 1 <= vals["max_factor"]:
            raise ValueError("StepControl: 0 < min_factor <= 1 <= max_factor is required, got min_factor = "
                             f"{min_factor!r}, max_factor = {max_factor!r}")
        if isinstance(keep, bool) or not isinstance(keep, numbers.Integral) or keep < 1:
            raise ValueError(f"StepControl: keep must be an integer >= 1, got {keep!r}")
        self.courant, self.grow, self.shrink = vals["courant"], vals["grow"], vals["shrink"]
        self.min_factor, self.max_factor, self.keep = vals["min_factor"], vals["max_factor"], int(keep)

    def check_scheme(self, scheme):
        if scheme == "bdf2" and self.grow > BDF2_MAX_GROW:
            raise ValueError(f'StepControl: with "bdf2" grow must be at most {BDF2_MAX_GROW}, got {self.grow!r}: variable-step BDF2 '
                             "is zero-stable only for step ratios below 1 + sqrt(2)")

    def params(self):
        return [self.courant, self.grow, self.shrink, self.min_factor, self.max_factor, 0.0, 0.0, 0.0]


def check_time_scheme_args(scheme, previous, adapt=None):
    """The constructor's checks; needs no GPU.  -> (the record's scheme word, previous)."""
    if not isinstance(scheme, str) or scheme not in SCHEMES:
        raise ValueError(f'scheme must be one of {tuple(SCHEMES)}, got {scheme!r}')
    if adapt is not None:
        if not isinstance(adapt, StepControl):
            raise ValueError(f"adapt must be a gfv.timescheme.StepControl or None, got {adapt!r}")
        adapt.check_scheme(scheme)
    if previous is not None:
        if not isinstance(previous, torch.Tensor) or previous.dim() != 2 or previous.shape[1] < 2 or previous.shape[0] < 1:
            raise ValueError("previous must be a [N, 2] (or [N, >= 2]: columns 0:2 are read) tensor, got "
                             f"{tuple(previous.shape) if isinstance(previous, torch.Tensor) else previous!r}")
        if not previous.dtype.is_floating_point:
            raise ValueError(f"previous must be a floating-point tensor, got {previous.dtype}")
        if not previous.is_cuda:
            raise ValueError("previous must live on the GPU (it becomes one slot of the device ring; there is no CPU path)")
    return SCHEMES[scheme], previous


def check_owner(time_scheme):
    """What an owner refuses of `time_scheme=`; needs no GPU."""
    TimeScheme.check_handed(None, time_scheme)


def check_adapt_owner(who, time_scheme, time_bc=None, field_stats=None):
    """What an owner refuses of an adaptive scheme beside its other followers of the clock; needs no GPU."""
    if not isinstance(time_scheme, TimeScheme) or time_scheme.adapt is None:
        return
    if time_bc is not None:
        raise ValueError(f"{who}: time_scheme adapt= together with time_bc= is not supported (TimeBC forms t = clock * plan.dt, "
                         "which is wrong once the steps vary)")
    if field_stats is not None:
        raise ValueError(f"{who}: time_scheme adapt= together with field_stats= is not supported (its means are unweighted in "
                         "time, which is wrong once the steps vary)")


def check_field(x_backup, N):
    """The node state an owner attaches: a contiguous float32 [N, 12] device tensor."""
    if not isinstance(x_backup, torch.Tensor) or tuple(x_backup.shape) != (N, 12):
        raise ValueError(f"TimeScheme: the node state must be a [{N}, 12] tensor")
    if x_backup.dtype != torch.float32 or not x_backup.is_contiguous():
        raise ValueError("TimeScheme: the node state must be contiguous float32")
    if not x_backup.is_cuda:
        raise ValueError("TimeScheme: the node state must live on the GPU (the history is kept by a HIP kernel; there is no CPU "
                         "path)")


class TimeScheme(Follower):
    KEYWORD = "time_scheme"
    OWNERS = ("MarchStep", "TrainStep")

    def __init__(self, scheme="bdf2", previous=None, adapt=None):
        self._word, self._previous = check_time_scheme_args(scheme, previous, adapt)
        self.scheme = scheme
        self.adapt = adapt                                        # a StepControl, or None: the plan's dt, the one launch
        self._ctl = None                                          # the controller's device state (attach(), with adapt only)
        self.ring = self.ustar = self.dt_eff = self.rec = None    # device state: allocated by attach(), never reallocated
        self._own_clock = None
        self._tbase = 0
        self._base = 0

    # ---- the owner's side (gfv/follow.py) -------------------------------------------------------------------------------------
    def attach(self, owner, plan, x_backup, clock=None, clock_word=0):
        """Called by the owner's constructor, last: `clock` is the owner's int32 record and `clock_word` the word of it that counts
        the fields written (None: a word of this object's own, bumped by `tick()`).  Allocates the device state (once), installs
        `previous` if one was given and issues the launch, so `ustar` / `dt_eff` are in place for the first forward.  -> self"""
        self.check_free()
        N, B = int(plan.N), int(plan.B)
        check_field(x_backup, N)
        dev = x_backup.device
        prev = self._previous
        if prev is not None and (prev.shape[0] != N or prev.device != dev):
            raise ValueError(f"previous must be a [{N}, >= 2] tensor on {dev}, got {tuple(prev.shape)} on {prev.device}")
        self._plan, self._xb, self.N, self.B = plan, x_backup, N, B
        self.ring = torch.zeros((2, N, 2), dtype=torch.float32, device=dev)
        self.ustar = torch.zeros((N, 2), dtype=torch.float32, device=dev)
        self.dt_eff = torch.zeros(B, dtype=torch.float32, device=dev)
        self.rec = torch.zeros(L.TIME_SCHEME_RECORD, dtype=torch.int32, device=dev)
        if clock is None:
            self._own_clock = clock = torch.zeros(1, dtype=torch.int32, device=dev)
        self._clock, self._clock_word = clock, int(clock_word)
        self._clock_ptr = clock.data_ptr() + 4 * self._clock_word
        if self.adapt is not None:
            self._ctl = self._alloc_control(plan, dev)
        if prev is None:
            self.reset()
        else:
            self.install_previous(prev)
        self._previous = None                   # (the ring holds it now)
        self._claim(owner)
        return self

    def _alloc_control(self, plan, dev):
        """The controller's device state: allocated once, never reallocated (recorded lists hold these addresses)."""
        B, keep = self.B, self.adapt.keep
        for name in ("crow", "knode", "kS", "area", "cbatch"):
            if getattr(plan, name, None) is None:
                raise ValueError(f"TimeScheme adapt=: the plan has no {name} (the Courant rate is a reduction over its cells)")
        z = lambda shape, dtype: torch.zeros(shape, dtype=dtype, device=dev)
        ctl = {"crec": z(L.STEP_CONTROL_RECORD, torch.int32),
               "par": torch.tensor(self.adapt.params(), dtype=torch.float32, device=dev),
               "dt0": z(B, torch.float32), "time0": z(B, torch.float64), "rate": z((2, B), torch.int32),
               "dts": z((2, B), torch.float32), "times": z((2, B), torch.float64),
               "state": z((L.STEP_CONTROL_STATE, B), torch.float32), "hist_clock": torch.full((keep,), -1, dtype=torch.int32, device=dev),
               "hist": z((keep, 2, B), torch.float32), "hist_time": z((keep, B), torch.float64)}
        assert len(self.adapt.params()) == L.STEP_CONTROL_PARAMS
        return ctl

    def launch(self):
        """The one launch (with `adapt=`: the two), behind the owner's advance: part of the step body (eager steps and recorded
        lists carry it alike)."""
        self._need()
        pl = self._plan
        if self._ctl is not None:
            c, lib, st = self._ctl, L.load(), L.stream_ptr()
            L.check(lib.gfv_step_control_rate(
                self._xb.data_ptr(), pl.uvp_dim.data_ptr(), pl.dt.data_ptr(), pl.crow.data_ptr(), pl.knode.data_ptr(),
                pl.kS.data_ptr(), pl.area.data_ptr(), pl.cbatch.data_ptr(), int(pl.C), self.B, self._clock_ptr, self.rec.data_ptr(),
                c["crec"].data_ptr(), c["par"].data_ptr(), c["dt0"].data_ptr(), c["time0"].data_ptr(), c["rate"].data_ptr(),
                c["dts"].data_ptr(), c["times"].data_ptr(), c["state"].data_ptr(), self.dt_eff.data_ptr(),
                c["hist_clock"].data_ptr(), c["hist"].data_ptr(), c["hist_time"].data_ptr(), self.adapt.keep, st),
                "gfv_step_control_rate")
            L.check(lib.gfv_step_control_rows(
                self._xb.data_ptr(), pl.batch.data_ptr(), pl.uvp_dim.data_ptr(), self.N, self.B, self._clock_ptr,
                self.rec.data_ptr(), c["state"].data_ptr(), self.ring.data_ptr(), self.ustar.data_ptr(), st),
                "gfv_step_control_rows")
            return
        L.check(L.load().gfv_time_scheme_update(
            self._xb.data_ptr(), pl.batch.data_ptr(), pl.uvp_dim.data_ptr(), pl.dt.data_ptr(), self.N, self.B, self._clock_ptr,
            self.rec.data_ptr(), self.ring.data_ptr(), self.ustar.data_ptr(), self.dt_eff.data_ptr(), L.stream_ptr()),
            "gfv_time_scheme_update")

    def tick(self):
        """`TrainStep.advance_time()` calls it behind its two copies: this object's own clock word + 1 in stream order, then the
        launch - the rotation, and the baseline of the level that comes next."""
        self._need()
        if self._own_clock is None:
            raise RuntimeError(f"the clock of this TimeScheme is the {self._owner}'s: the device advances it")
        self._own_clock.add_(1)
        self.launch()

    time_state = property(lambda self: (self.ustar, self.dt_eff))

    def _read_clock(self):
        """(synchronises) the clock as the device holds it."""
        return int(self._clock[self._clock_word:self._clock_word + 1].cpu()[0])

    def _write_rec(self, base):
        self._base = int(base)
        self.rec[SCHEME:BASE + 1].copy_(torch.tensor([self._word, self._base], dtype=torch.int32))

    def _write_control(self, clock, dt_last, time):
        """The controller starts over at `clock`: its step and time there are the host's (dt_last [B], None: the plan's dt; time
        [B] float64, None: 0), both rate slots are cleared and the history forgotten.  In stream order, in front of the launch."""
        c = self._ctl
        if c is None:
            if dt_last is not None or time is not None:
                raise ValueError("dt_last= / time= need a TimeScheme with adapt=")
            return
        for name, v, dtype in (("dt_last", dt_last, torch.float32), ("time", time, torch.float64)):
            if v is None:
                continue
            if not isinstance(v, torch.Tensor) or tuple(v.shape) != (self.B,) or not v.dtype.is_floating_point:
                raise ValueError(f"{name} must be a floating-point [{self.B}] tensor, got {v!r}")
            if name == "dt_last" and not bool((v > 0).all()):
                raise ValueError(f"dt_last must be > 0 for every graph, got {v.tolist()}")
        self._tbase = int(clock)
        c["crec"][TBASE:TBASE + 1].copy_(torch.tensor([self._tbase], dtype=torch.int32))     # (word [1], the counter, is the device's)
        c["dt0"].copy_(self._plan.dt if dt_last is None else dt_last.to(torch.float32))
        if time is None:
            c["time0"].zero_()
        else:
            c["time0"].copy_(time.to(torch.float64))
        c["rate"].zero_()
        c["hist_clock"].fill_(-1)

    # ---- the history ----------------------------------------------------------------------------------------------------------------
    def reset(self, dt_last=None, time=None):
        """History forgotten: base = the current clock, so the level that comes next is first order (the usual start-up), then the
        launch.  The owner's reset() calls it behind clearing its clock.  With `adapt=` the controller starts over too: the step
        behind the current field is the plan's dt (or `dt_last` [B]) and its time 0 (or `time` [B]).  Synchronises (the clock is
        the device's)."""
        self._need()
        c = self._read_clock()
        self._write_control(c, dt_last, time)
        self._write_rec(c)
        self.launch()

    def install_previous(self, previous, dt_last=None, time=None):
        """`previous` [N, >= 2] (dimensional, columns 0:2) becomes the field in front of the current one: it is copied into the
        ring slot the next launch reads and base = clock - 1, so the level that comes next is already second order - what the
        constructor's `previous=` does, and how a resumed run continues.  With `adapt=`: `dt_last` [B] is the step that lay
        between `previous` and the current field (None: the plan's dt) and `time` [B] the current field's time (None: 0).
        Synchronises."""
        self._need()
        check_time_scheme_args(self.scheme, previous)
        if previous.shape[0] != self.N or previous.device != self.ring.device:
            raise ValueError(f"previous must be a [{self.N}, >= 2] tensor on {self.ring.device}, got {tuple(previous.shape)} on "
                             f"{previous.device}")
        c = self._read_clock()
        self._write_control(c, dt_last, time)
        self.ring[(c & 1) ^ 1].copy_(previous[:, 0:2])
        self._write_rec(c - 1)
        self.launch()

    # ---- reading (each of these synchronises) ---------------------------------------------------------------------------------------
    def read(self):
        """{"clock", "order", "ustar" [N,2], "previous" [N,2] or None, "dt_eff" [B]}: the clock as the device holds it, the order
        in time of the field being computed (2: "bdf2" with two fields behind it), the baseline and the step the finite-volume
        section reads, and field clock - 1 (dimensional) where the ring is known to hold it.  CPU tensors.  Synchronises."""
        self._need()
        c = self._read_clock()
        active = self._word == L.TIME_SCHEME_BDF2 and c > self._base
        out = {"clock": c, "order": 2 if active else 1, "ustar": self.ustar.cpu(),
               "previous": self.ring[(c & 1) ^ 1].cpu() if c > self._base else None, "dt_eff": self.dt_eff.cpu()}
        if self._ctl is not None:
            # with adapt=: the step of the level being computed, the time of field `clock`, its Courant number under the step that
            # produced it, the step ratio, and that step itself
            st = self._ctl["state"].cpu()
            out.update(dt=st[ST_DT].clone(), omega=st[ST_OMEGA].clone(), courant=st[ST_COURANT].clone(), rate=st[ST_RATE].clone(),
                       time=self._ctl["times"][c & 1].cpu(),
                       dt_last=(self._ctl["dt0"] if c <= self._tbase else self._ctl["dts"][c & 1]).cpu())
        return out

    def step_history(self):
        """With `adapt=`: one row {"clock", "dt" [B], "courant" [B], "time" [B] float64} per field among the last `keep` (what
        `read()` showed at that clock), oldest first, from the field the controller last started over at.  Synchronises."""
        self._need()
        if self._ctl is None:
            raise RuntimeError("step_history() needs a TimeScheme with adapt=")
        c, keep = self._read_clock(), self.adapt.keep
        clocks, hist, times = self._ctl["hist_clock"].cpu(), self._ctl["hist"].cpu(), self._ctl["hist_time"].cpu()
        rows = []
        for k in range(max(self._tbase, c - keep + 1, 0), c + 1):
            s = k % keep
            if int(clocks[s]) != k:
                continue
            rows.append({"clock": k, "dt": hist[s, 0].clone(), "courant": hist[s, 1].clone(), "time": times[s].clone()})
        return rows

    def state_dict(self):
        """{"scheme", "has_previous", "previous" [N,2] CPU tensor or None}: field clock - 1, what a resumed run needs beside the
        current field (which is the caller's to carry over).  With `adapt=` also "dt_last" [B] (the step that produced the current
        field) and "time" [B] float64 (its time), CPU tensors.  Synchronises."""
        read = self.read()
        prev = read["previous"]
        sd = {"scheme": self.scheme, "has_previous": prev is not None, "previous": prev}
        if self._ctl is not None:
            sd.update(dt_last=read["dt_last"], time=read["time"])
        return sd

    def load_state_dict(self, sd):
        """Installs the saved field as `previous=` would (a dict without one: `reset()`), and with `adapt=` the saved step and
        time (a dict without them: the plan's dt and 0)."""
        self._need()
        if sd.get("scheme") != self.scheme:
            raise ValueError(f"the state of a {sd.get('scheme')!r} time scheme does not load into a {self.scheme!r} one")
        dev = self.ring.device
        more = {}
        if self._ctl is not None:
            more = {k: sd[k].to(dev) for k in ("dt_last", "time") if sd.get(k) is not None}
        if sd.get("has_previous"):
            self.install_previous(sd["previous"].to(dev), **more)
        else:
            self.reset(**more)
