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
explicit the scheme is accepted and only the time term changes - the fluxes keep their u_n-based `uv_hat`.  Variable step ratios
are not supported (a march cannot change dt between levels).  `Rollout`, `Sweep` and `PoolTrainStep` take no scheme.

Who owns what a recorded list points at: DESIGN.md 5l.  Particular to this object, allocated once when its owner attaches it and
never reallocated: the ring, `ustar`, `dt_eff`, the record and its own clock word.  One owner per object.  `MarchStep.state_dict()`
carries the scheme's state (`gfv_time_scheme`); `TrainStep.state_dict()` stays the optimiser's: save `sch.state_dict()` beside it.
"""
from __future__ import annotations

import torch

from . import lib as L

SCHEMES = {"bdf1": L.TIME_SCHEME_BDF1, "bdf2": L.TIME_SCHEME_BDF2}
SCHEME, BASE = 0, 1        # words of the record (include/gfv.h gfv_time_scheme_update)


def check_time_scheme_args(scheme, previous):
    """The constructor's checks; needs no GPU.  -> (the record's scheme word, previous)."""
    if not isinstance(scheme, str) or scheme not in SCHEMES:
        raise ValueError(f'scheme must be one of {tuple(SCHEMES)}, got {scheme!r}')
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
    if time_scheme is None:
        return
    if not isinstance(time_scheme, TimeScheme):
        raise ValueError(f"time_scheme must be a gfv.timescheme.TimeScheme or None, got {time_scheme!r}")
    time_scheme.check_free()


def check_field(x_backup, N):
    """The node state an owner attaches: a contiguous float32 [N, 12] device tensor."""
    if not isinstance(x_backup, torch.Tensor) or tuple(x_backup.shape) != (N, 12):
        raise ValueError(f"TimeScheme: the node state must be a [{N}, 12] tensor")
    if x_backup.dtype != torch.float32 or not x_backup.is_contiguous():
        raise ValueError("TimeScheme: the node state must be contiguous float32")
    if not x_backup.is_cuda:
        raise ValueError("TimeScheme: the node state must live on the GPU (the history is kept by a HIP kernel; there is no CPU "
                         "path)")


class TimeScheme:
    def __init__(self, scheme="bdf2", previous=None):
        self._word, self._previous = check_time_scheme_args(scheme, previous)
        self.scheme = scheme
        self.ring = self.ustar = self.dt_eff = self.rec = None    # device state: allocated by attach(), never reallocated
        self._own_clock = None
        self._owner = None                                        # the owner's class name once attached (FieldStats' rule)
        self._base = 0

    # ---- the owner's side -------------------------------------------------------------------------------------------------------
    def check_free(self):
        """Needs no GPU: an owner's constructor calls it before it looks at anything else."""
        if self._owner is not None:
            raise ValueError(f"this TimeScheme is already attached to a {self._owner} (one owner per object: it follows one clock "
                             "and holds one batch's history)")

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
        if prev is None:
            self.reset()
        else:
            self.install_previous(prev)
        self._previous = None                   # (the ring holds it now)
        self._owner = type(owner).__name__      # (last: an attach that raised leaves the object free)
        return self

    def launch(self):
        """The one launch, behind the owner's advance: part of the step body (eager steps and recorded lists carry it alike)."""
        self._need()
        pl = self._plan
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

    def _need(self):
        if self.rec is None:
            raise RuntimeError("this TimeScheme is not attached yet: hand it to MarchStep(..., time_scheme=) or "
                               "TrainStep(..., time_scheme=)")

    def _read_clock(self):
        """(synchronises) the clock as the device holds it."""
        return int(self._clock[self._clock_word:self._clock_word + 1].cpu()[0])

    def _write_rec(self, base):
        self._base = int(base)
        self.rec[SCHEME:BASE + 1].copy_(torch.tensor([self._word, self._base], dtype=torch.int32))

    # ---- the history ----------------------------------------------------------------------------------------------------------------
    def reset(self):
        """History forgotten: base = the current clock, so the level that comes next is first order (the usual start-up), then the
        launch.  The owner's reset() calls it behind clearing its clock.  Synchronises (the clock is the device's)."""
        self._need()
        self._write_rec(self._read_clock())
        self.launch()

    def install_previous(self, previous):
        """`previous` [N, >= 2] (dimensional, columns 0:2) becomes the field in front of the current one: it is copied into the
        ring slot the next launch reads and base = clock - 1, so the level that comes next is already second order - what the
        constructor's `previous=` does, and how a resumed run continues.  Synchronises."""
        self._need()
        check_time_scheme_args(self.scheme, previous)
        if previous.shape[0] != self.N or previous.device != self.ring.device:
            raise ValueError(f"previous must be a [{self.N}, >= 2] tensor on {self.ring.device}, got {tuple(previous.shape)} on "
                             f"{previous.device}")
        c = self._read_clock()
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
        return {"clock": c, "order": 2 if active else 1, "ustar": self.ustar.cpu(),
                "previous": self.ring[(c & 1) ^ 1].cpu() if c > self._base else None, "dt_eff": self.dt_eff.cpu()}

    def state_dict(self):
        """{"scheme", "has_previous", "previous" [N,2] CPU tensor or None}: field clock - 1, what a resumed run needs beside the
        current field (which is the caller's to carry over).  Synchronises."""
        prev = self.read()["previous"]
        return {"scheme": self.scheme, "has_previous": prev is not None, "previous": prev}

    def load_state_dict(self, sd):
        """Installs the saved field as `previous=` would (a dict without one: `reset()`)."""
        self._need()
        if sd.get("scheme") != self.scheme:
            raise ValueError(f"the state of a {sd.get('scheme')!r} time scheme does not load into a {self.scheme!r} one")
        if sd.get("has_previous"):
            self.install_previous(sd["previous"].to(self.ring.device))
        else:
            self.reset()
