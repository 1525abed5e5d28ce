"""Time march: the reference's "Inference With Adam (PINN-style)" loop that advances in time only after the inner iterations
of a time level have converged - decided on the device.

The reference (solve_with_grad_GPU.py:133-209) runs `max_inner_steps` Adam iterations per time level and then writes the
prediction back as the next level's state; it declares `--residual_tolerance` and `Data_Pool.init_loss` "to calculate the
relative residual" and never wires them up.  `TrainStep.step()` x N + `advance_time()` is that loop with a fixed count: the host
cannot know that a level has converged without a synchronisation per step.  `MarchStep` moves the decision into one launch per
step (`gfv_march_advance`, csrc/march.hip, include/gfv.h) between the backward and the optimiser's launches:

    ms = MarchStep(model, graphs, max_inner=20, min_inner=1, tol=1e-2, abs_tol=None, max_levels=1000, keep=0)
    rows = ms.run(levels=50, max_ahead=32)   # one dict per completed level (decode_history)
    ms.step()                                 # one inner iteration; the device decides whether it ends the level
    ms.level; ms.stats(); ms.snapshot(level); ms.reset()

The rule (per step, with the device record as the launch finds it): r[b] = the weighted residual of graph b - the argument of the
training loss's logarithm; at the first inner iteration of a level r0[b] = r[b]; the level ends when every graph has
r <= tol * r0 or r <= abs_tol and at least `min_inner` iterations were taken, or at `max_inner` iterations.  Ending a level is
`advance_time()` - x_backup[:, 0:3] = prediction; x = x_backup - plus one history row.  The step whose launch ends a level is
still applied: the level's last Adam step, as in the reference's loop.

Held steps.  Once `levels` levels are complete the record says `done`: every later step is HELD - its march launch writes
apply = 0, and the guard, Adam and log launches behind it read that word where they read the accumulation's (`hold=` of
gfv/optstep.py).  No parameter, moment, step count, averaged weight, guard count, field or history row moves, so the result does
not depend on how far the host ran ahead (`max_ahead`).  What a held step does touch: the recorded step's own outputs (`loss`,
`losses`, `uvp_node`: a forward of the current state), the log's ring (one row with apply = 0) and - while the model's Normalizer
is still accumulating (fewer than `dataset_size` forwards so far) - its statistics, which the forward updates in front of the
march launch.  March a model whose Normalizer has finished accumulating, or use `max_ahead=0`.

`run()` issues steps until the pinned mirror says done, `levels * max_inner` steps are out (a bound the host knows: the loop ends
without the mirror), keeping at most `max_ahead` steps queued beyond what is known to have completed; then it synchronises once
and decodes the history.  A later `run()` raises the target and clears `done`, after a synchronisation.

Who owns what a recorded list points at: DESIGN.md 5l.  Particular to this object, created in the constructor and held for its
lifetime, never reallocated: the march record, r0, the history, the snapshot ring, the reduction workspace, the pinned mirror.
One batch per object: `set_batch()` is refused.  The march state is not part of `state_dict()`.

`schedule=` (gfv/schedule.py): the reference steps its scheduler once per time level (solve_with_grad_GPU.py:197).
With a schedule attached every step issues one more launch in front of the march launch (`gfv_lr_schedule`, mode FOLLOW): the
schedule's epoch becomes the level count, capped at the last level that runs, and that level's rate is written where Adam reads it.
The step that ends a level runs at that level's rate; held steps change neither the rate nor the schedule's record.

`field_stats=FieldStats(start=, stride=, stop=)` (gfv/fieldstats.py): one more launch behind the march launch keeps the
time mean, the variances, u'v' and the extremes of the LEVELS' fields on the device, following the level count: exactly one sample
per completed level (the field level 0 leaves has clock 1), whatever its inner count; steps that do not end a level, and held
steps, sample nothing.  `ms.field_stats.read()` reads them; `stats()` keeps its meaning (the march record).  Not part of
`state_dict()`.  `field_stats=None` (the default) issues no new launch and allocates nothing.

`wall_forces=WallForces(faces=, box=, origin=, start=, stride=, stop=, keep=)` (gfv/wallforce.py): two more launches behind
the march launch, where `field_stats` launches, sum the pressure and the viscous force on the selected wall faces, and their moments,
per graph, for every COMPLETED level - one row of a device ring per level, whatever its inner count; held steps add nothing.
`ms.wall_forces.read()` reads them.  Allowed beside `field_stats`, `time_bc` and `time_scheme` (`StepControl` included: the time of a
sample is joined through its clock with `step_history()`); refused for graphs of a DevicePool.  Not part of `state_dict()`.
`wall_forces=None` (the default) issues no new launch and allocates nothing.

`probes=Probes(points, graph=, start=, stride=, stop=, keep=, tolerance=)` (gfv/probes.py): one more launch behind the
march launch, after the wall-force pair, interpolates (u, v, p) and their gradients at fixed points of the mesh for every COMPLETED
level - one row of a device ring per level, whatever its inner count; held steps add nothing.  `ms.probes.read()` reads them.
Allowed beside every other follower (`StepControl` included: the time of a sample is joined through its clock with
`step_history()`); refused for graphs of a DevicePool.  Not part of `state_dict()`.  `probes=None` (the default) issues no new
launch and allocates nothing.

`integrals=FlowIntegrals(start=, stride=, stop=, keep=, fields=)` (gfv/integrals.py): one more launch behind the march
launch, after the wall-force pair and before the probes, sums per graph the kinetic energy, the enstrophy, the norms of the discrete
divergence and the flux through the inflow, outflow and other boundary faces for every COMPLETED level - one row of a device ring
per level, whatever its inner count; held steps add nothing.  `ms.integrals.read()` reads them.  Allowed beside every other follower
(`StepControl` included: the time of a sample is joined through its clock with `step_history()`); refused for graphs of a DevicePool.
Not part of `state_dict()`.  `integrals=None` (the default) issues no new launch and allocates nothing.

`time_bc=TimeBC(velocity=, source=, nodes=)` (gfv/timebc.py): one more launch behind the march launch rewrites the
Dirichlet velocity targets and the source coefficient for the level about to be computed (level count + 1), from per-graph waveform
records on the device.  The host cannot do this: only the device knows which step starts a new level.  Inner iterations and held
steps find the level count they found before and write the same values again.  With it `state_dict()` carries the level count
(`gfv_time_bc`: one synchronisation) and `load_state_dict()` puts the boundary data of the level that comes next in place, so a
march that resumes in a new object is driven as the uninterrupted one.  `time_bc=None` (the default) issues no new launch and
allocates nothing.

`time_scheme=TimeScheme("bdf2")` (gfv/timescheme.py): one more launch behind the march launch keeps the velocity of
the last two levels in a ring and writes the baseline and the step of a second-order backward difference where the finite-volume
section reads them - from the second level on (the first runs backward Euler, the usual start-up; `TimeScheme("bdf2", previous=)`
starts at second order).  Second order in time needs `integrator="implicit"`.  Inner iterations and held steps find the level count
they found before and write the same bits again.  With it `state_dict()` carries the previous level's velocity
(`gfv_time_scheme`: one synchronisation) and `load_state_dict()` installs it, so a march that resumes in a new object on the
carried-over field continues at second order.  `time_scheme=None` (the default) issues no new launch and allocates nothing.

`time_scheme=TimeScheme("bdf2", adapt=StepControl(courant=2.0, ...))`: the step of every level is sized on the
device to a Courant-number target - two launches behind the march launch in place of the one: the Courant rate of the level's
field (a maximum over its cells) with the controller, then the baseline with the variable-step coefficients.  The host cannot do
this: it does not know which step ends a level.  Inner iterations and held steps write the same bits again, the step, the time
and the history row included; `ms.time_scheme.read()` shows the step, the time and the Courant number, `step_history()` the last
levels'.  `gfv_time_scheme` of `state_dict()` then also carries the last step and the time, and a resumed march continues with
them.  Refused together with `time_bc=` (it forms t = level * plan.dt) and `field_stats=` (its means are unweighted in time).
"""
from __future__ import annotations

import collections
import ctypes as C
import math
import numbers
import struct

import torch

from . import lib as L
from .follow import check_followers
from .schedule import Plateau
from .timescheme import check_adapt_owner
from .trainer import TrainStep

# words of the march record (include/gfv.h gfv_march_advance)
MAX_INNER, MIN_INNER, INNER, APPLY, TOL, ABS_TOL, LEVEL, COUNTER, TARGET, DONE, SEEN, HELD, KEEP = range(13)
NEVER = -1.0    # a negative tolerance never fires


def _f2w(v):
    """The 32-bit word that holds the fp32 value v (as a signed int, for an int32 tensor)."""
    return struct.unpack("i", struct.pack("f", float(v)))[0]


def check_march_args(max_inner, min_inner, tol, abs_tol, max_levels, keep):
    """The constructor checks; needs no GPU.  -> (max_inner, min_inner, tol, abs_tol, max_levels, keep), None tolerances as NEVER."""
    for name, v in (("max_inner", max_inner), ("min_inner", min_inner), ("max_levels", max_levels), ("keep", keep)):
        if isinstance(v, bool) or not isinstance(v, numbers.Integral):
            raise ValueError(f"{name} must be an integer, got {v!r}")
    if max_inner < 1:
        raise ValueError(f"max_inner must be at least 1, got {max_inner}")
    if not 1 <= min_inner <= max_inner:
        raise ValueError(f"min_inner must lie in [1, max_inner = {max_inner}], got {min_inner}")
    if max_levels < 1:
        raise ValueError(f"max_levels must be at least 1, got {max_levels}")
    if keep < 0:
        raise ValueError(f"keep must be 0 (no snapshots) or the number of levels to keep, got {keep}")
    out = []
    for name, v in (("tol", tol), ("abs_tol", abs_tol)):
        v = NEVER if v is None else float(v)
        if math.isnan(v) or math.isinf(v):
            raise ValueError(f"{name} must be a finite number or None, got {v!r}")
        out.append(v)
    return int(max_inner), int(min_inner), out[0], out[1], int(max_levels), int(keep)


def check_step_args(use_graph, kw):
    """What a MarchStep refuses of TrainStep's arguments; needs no GPU."""
    if use_graph not in (False, "list"):
        raise ValueError('MarchStep: use_graph must be False or "list" (a captured hipGraph is not supported)')
    if kw.get("accum_steps", 1) != 1:
        raise ValueError("MarchStep: accum_steps > 1 is not supported (the march record takes the accumulation record's place "
                         "in the optimiser's launches)")
    if kw.get("world_size", 1) != 1 or kw.get("distributed"):
        raise ValueError("MarchStep: data parallelism is not supported (the ranks would have to agree on every level's end)")
    if not kw.get("want_outputs", True):
        raise ValueError("MarchStep: want_outputs=False leaves no prediction to advance to")
    if kw.get("balance") is not None:
        raise ValueError("MarchStep: balance= is not supported (the convergence test compares r with r0 under ONE set of weights; "
                         "a balancer would move them within a level)")
    if kw.get("observations") is not None:
        raise ValueError("MarchStep: observations= is not supported (the convergence rule is on the PDE residual alone; a data "
                         "term inside the objective would not be seen by it)")
    if isinstance(kw.get("schedule"), Plateau):
        raise ValueError("MarchStep: a Plateau schedule is not supported (the per-level launch follows the level count: it has no "
                         "metric to observe)")


def decode_history(words, B):
    """History rows [n, MARCH_HEAD + MARCH_GRAPH * B] of 32-bit words (an int32 CPU tensor) -> one dict per row: level, inner
    (iterations taken), converged, capped, seen (launches that found `done` clear, this one included), and per graph the tensors
    losses [B,4] (cont, mom_x, mom_y, press), r0 [B], r [B], update_norm [B] = || uvp - uvp_prev ||_2, field_norm [B]."""
    words = torch.as_tensor(words, dtype=torch.int32).contiguous()
    width = L.MARCH_HEAD + L.MARCH_GRAPH * int(B)
    if words.dim() != 2 or words.shape[1] != width:
        raise ValueError(f"history rows of B = {B} graphs are {width} words, got shape {tuple(words.shape)}")
    per = words[:, L.MARCH_HEAD:].contiguous().view(torch.float32).reshape(-1, int(B), L.MARCH_GRAPH)
    rows = []
    for k in range(words.shape[0]):
        flags = int(words[k, 2])
        rows.append({"level": int(words[k, 0]), "inner": int(words[k, 1]), "converged": bool(flags & L.MARCH_CONVERGED),
                     "capped": bool(flags & L.MARCH_CAPPED), "seen": int(words[k, 3]), "losses": per[k, :, 0:4].clone(),
                     "r0": per[k, :, 4].clone(), "r": per[k, :, 5].clone(), "update_norm": per[k, :, 6].clone(),
                     "field_norm": per[k, :, 7].clone()})
    return rows


class MarchStep(TrainStep):
    def __init__(self, model, graphs, *, max_inner=20, min_inner=1, tol=1e-2, abs_tol=None, max_levels=1000, keep=0,
                 use_graph="list", field_stats=None, time_bc=None, time_scheme=None, wall_forces=None, probes=None,
                 integrals=None, **trainstep_kwargs):
        args = check_march_args(max_inner, min_inner, tol, abs_tol, max_levels, keep)
        check_step_args(use_graph, trainstep_kwargs)
        check_adapt_owner("MarchStep", time_scheme, time_bc, field_stats)
        check_followers("MarchStep", graphs, 0, field_stats=field_stats, wall_forces=wall_forces, time_bc=time_bc,
                        time_scheme=time_scheme, integrals=integrals, probes=probes)
        self._march = None
        self.field_stats = self.wall_forces = self.integrals = self.probes = self.time_bc = None
        self._followers = []
        super().__init__(model, graphs, use_graph=use_graph, **trainstep_kwargs)
        self._max_inner, self._min_inner, self._tol, self._abs_tol, self.max_levels, self.keep = args
        dev, pl = self.dev, self.plan
        if not (self.x.dtype == torch.float32 and self.x.is_contiguous() and tuple(self.x.shape) == (pl.N, 12)):
            raise ValueError("MarchStep: graphs[0].x must be a contiguous float32 [N, 12] tensor")
        # device state of the march: created once, never reallocated (recorded lists hold these addresses)
        self._march = torch.zeros(L.MARCH_RECORD, dtype=torch.int32, device=dev)
        self._r0 = torch.zeros(pl.B, dtype=torch.float32, device=dev)
        self._hist = torch.zeros((self.max_levels, L.MARCH_HEAD + L.MARCH_GRAPH * pl.B), dtype=torch.int32, device=dev)
        self._snap = torch.zeros((self.keep, pl.N, 3), dtype=torch.float32, device=dev) if self.keep else None
        self._partial = torch.zeros((pl.n_chunks, 2), dtype=torch.float64, device=dev)
        self._x0 = self.x_backup.clone()
        host, devp = C.POINTER(C.c_int32)(), C.c_void_p()
        L.check(L.load(raw=True).gfv_sweep_mirror_create(3, C.byref(host), C.byref(devp)), "gfv_sweep_mirror_create")
        self._mirror, self._mirror_dev = host, devp.value
        self._write_control()
        self._put(TARGET, [self.max_levels])     # (step() on its own marches until the history is full)
        # The followers of the level count (gfv/follow.py), attached last: the constructor above issues no step, so no list has been
        # recorded without their launches.  The clock is word LEVEL of the march record: it moves on the launch that ends a level and
        # on no other, so each acts once per level, whatever its inner count: behind an inner iteration or a held step the samplers
        # sample nothing, and time_bc (the targets of level count + 1) and time_scheme (the ring's rotation, the next level's baseline)
        # write the same bits again (an early-out would need the blocks to agree on a "last" word: DESIGN.md 5u); the attach of each
        # of those two issues its launch for level 0 (the level count is 0; second order with `previous=`).  They touch disjoint data
        # (wall_forces, integrals and probes read x_backup and the plan) and none reads what another writes: their order among themselves does
        # not matter.
        self.field_stats = field_stats and field_stats.attach(self, self.x_backup, self._march, LEVEL)
        self.wall_forces = wall_forces and wall_forces.attach(self, graphs, pl, self.x_backup, self._march, LEVEL)
        self.integrals = integrals and integrals.attach(self, graphs, pl, self.x_backup, self._march, LEVEL)
        self.probes = probes and probes.attach(self, graphs, pl, self.x_backup, self._march, LEVEL)
        self.time_bc = time_bc and time_bc.attach(self, graphs, pl, self.x_backup, self.x, self._march, LEVEL, self.max_levels)
        self.time_scheme = time_scheme and time_scheme.attach(self, pl, self.x_backup, self._march, LEVEL)
        self._followers = [f for f in (self.field_stats, self.wall_forces, self.integrals, self.probes, self.time_bc,
                                       self.time_scheme) if f is not None]

    def __del__(self):
        host = getattr(self, "_mirror", None)
        if host:
            try:
                self._drop_recorded()
                torch.cuda.synchronize(self.dev)     # (nothing queued may still publish into the mirror)
                L.load(raw=True).gfv_sweep_mirror_free(host)
            except Exception:
                pass
            self._mirror = None

    # ---- the record's host-written words ---------------------------------------------------------------------------------------
    def _put(self, word, ints):
        """Host words into the record, in stream order (the other words are the device's and stay)."""
        self._march[word:word + len(ints)].copy_(torch.tensor(ints, dtype=torch.int32))
        if word == TARGET and self.schedule is not None:
            # the schedule follows the level count up to the last level that runs: a step issued past the target (held) finds
            # level == target and must leave the rate and the schedule's record as they are
            self.schedule.set_follow_cap(int(ints[0]) - 1)

    def _write_control(self):
        self._put(MAX_INNER, [self._max_inner, self._min_inner])
        self._put(TOL, [_f2w(self._tol), _f2w(self._abs_tol)])
        self._put(KEEP, [self.keep])

    max_inner = property(lambda self: self._max_inner)
    min_inner = property(lambda self: self._min_inner)
    tol = property(lambda self: self._tol)
    abs_tol = property(lambda self: self._abs_tol)

    def set_control(self, max_inner=None, min_inner=None, tol=None, abs_tol=None):
        """New iteration bounds / tolerances (None: unchanged; a negative tolerance never fires), checked before anything changes.
        They reach recorded lists through the device record: nothing is recorded again.  They hold from the next step issued."""
        new = check_march_args(self._max_inner if max_inner is None else max_inner,
                               self._min_inner if min_inner is None else min_inner, self._tol if tol is None else tol,
                               self._abs_tol if abs_tol is None else abs_tol, self.max_levels, self.keep)
        self._max_inner, self._min_inner, self._tol, self._abs_tol = new[0:4]
        self._write_control()

    # ---- what TrainStep offers and a march cannot take ----------------------------------------------------------------------
    accum_steps = property(lambda self: 1)

    @accum_steps.setter
    def accum_steps(self, v):
        if v != 1:
            raise ValueError("MarchStep: accum_steps > 1 is not supported")

    def advance_time(self):
        raise RuntimeError("MarchStep: the device owns the time advance (the march launch of the step that ends a level performs "
                           "it); advance_time() would advance a second time")

    def set_batch(self, graphs):
        raise RuntimeError("MarchStep: one batch per object (the march record, history and snapshots belong to it)")

    # ---- the step ------------------------------------------------------------------------------------------------------------
    def _after_backward(self):
        pl = self.plan
        if self.schedule is not None:
            # one scheduler step per time level (solve_with_grad_GPU.py:197), in front of the march launch: the level word shows
            # every latch up to the previous step, so the step that ends a level still runs at that level's rate
            self.schedule.follow(self._march.data_ptr() + 4 * LEVEL)
        L.check(L.load().gfv_march_advance(
            self.uvp_node.data_ptr(), self.x_backup.data_ptr(), self.x.data_ptr(), pl.N, pl.chunk_beg.data_ptr(),
            pl.chunk_end.data_ptr(), pl.gchunk_ptr.data_ptr(), pl.n_chunks, pl.B, self.losses.data_ptr(), self._partial.data_ptr(),
            self.hyper.data_ptr(), self._march.data_ptr(), self._r0.data_ptr(), self._hist.data_ptr(), self.max_levels,
            self._max_inner, self._min_inner, None if self._snap is None else self._snap.data_ptr(), self.keep, self._mirror_dev,
            L.stream_ptr()), "gfv_march_advance")
        self._follow_level()

    def _follow_level(self):
        """The launches that follow the level count, behind the march launch (which, and why there: the constructor)."""
        for f in self._followers:
            f.launch()

    def _hold_record(self):
        return self._march       # (word [3] = APPLY: the march launch of this step wrote it; the guard, Adam and the log read it)

    # ---- the run -------------------------------------------------------------------------------------------------------------
    def _read_record(self):
        """(synchronises) the record as the device holds it, a list of 16 ints."""
        torch.cuda.current_stream().synchronize()
        return [int(v) for v in self._march.cpu()]

    def run(self, levels, max_ahead=32):
        """Complete `levels` more time levels -> their decoded history rows (decode_history), oldest first.  max_ahead: steps the
        host may have queued beyond what is known to have completed (0: a synchronisation per step)."""
        levels, max_ahead = int(levels), int(max_ahead)
        if levels < 1 or max_ahead < 0:
            raise ValueError("MarchStep.run: levels >= 1 and max_ahead >= 0 are required")
        L.raise_on_status("MarchStep.run")
        stream = torch.cuda.current_stream()
        rec = self._read_record()
        level0, seen0 = rec[LEVEL], rec[SEEN]
        if level0 + levels > self.max_levels:
            raise IndexError(f"MarchStep: {level0} levels done + {levels} asked for exceeds max_levels={self.max_levels} (the "
                             "device history has one row per level); reset() or build the MarchStep with a larger max_levels")
        self._put(TARGET, [level0 + levels, 0])                       # target, done
        self._mirror[0], self._mirror[1], self._mirror[2] = seen0, level0, 0
        budget = levels * self._max_inner - rec[INNER]                # (the open level has taken rec[INNER] of its iterations)
        issued = known = 0
        events = collections.deque()
        stride = max(1, max_ahead // 2)                               # (an event every so many steps: what a wait can fall back on)
        while issued < budget and self._mirror[2] == 0:
            self.step()
            issued += 1
            if max_ahead == 0:
                stream.synchronize()
                known = issued
                continue
            if issued % stride == 0:
                ev = torch.cuda.Event()
                ev.record(stream)
                events.append((issued, ev))
            known = max(known, min(int(self._mirror[0]) - seen0, issued))
            while issued - known > max_ahead and events:
                n, ev = events.popleft()
                ev.synchronize()
                known = max(known, n)
            while events and events[0][0] <= known:
                events.popleft()
        rec = self._read_record()
        L.raise_on_status("MarchStep.run")
        return decode_history(self._hist[level0:rec[LEVEL]].cpu(), self.plan.B)

    # ---- reading the state (each of these synchronises) ----------------------------------------------------------------------
    @property
    def level(self):
        """Levels completed (synchronises)."""
        return self._read_record()[LEVEL]

    def stats(self):
        """{"level", "inner", "target", "done", "seen", "held", "apply"} of the device record: levels completed, inner iterations
        taken in the open level, the level count at which steps are held, whether they are, the march launches that found `done`
        clear / set so far, and the last launch's apply flag.  Synchronises."""
        rec = self._read_record()
        return {"level": rec[LEVEL], "inner": rec[INNER], "target": rec[TARGET], "done": bool(rec[DONE]), "seen": rec[SEEN],
                "held": rec[HELD], "apply": rec[APPLY]}

    def history(self):
        """The decoded rows of every completed level (synchronises)."""
        rec = self._read_record()
        return decode_history(self._hist[:min(rec[LEVEL], self.max_levels)].cpu(), self.plan.B)

    def snapshot(self, level):
        """The node field [N, 3] that completed level `level` left (a copy), one of the last `keep` levels.  Synchronises."""
        if not self.keep:
            raise RuntimeError("this MarchStep was built with keep=0")
        done = self._read_record()[LEVEL]
        level = int(level)
        if not max(0, done - self.keep) <= level < done:
            raise IndexError(f"level {level} is not among the last {self.keep} of {done} completed levels")
        return self._snap[level % self.keep].clone()

    def reset(self, x=None):
        """Back to level 0 from the initial node state (or from `x` [N, 12], un-normalised): record, r0, history and snapshots
        are cleared, the field statistics (if any) start over.  Parameters and optimiser state stay as they are."""
        src = self._x0 if x is None else x
        if tuple(src.shape) != tuple(self.x_backup.shape) or not src.is_cuda:
            raise ValueError(f"x must be a device tensor of shape {tuple(self.x_backup.shape)}")
        torch.cuda.current_stream().synchronize()
        self.x_backup.copy_(src)
        self.x.copy_(src)
        self._march.zero_()
        self._r0.zero_()
        self._hist.zero_()
        if self._snap is not None:
            self._snap.zero_()
        for i in range(3):
            self._mirror[i] = 0
        self._write_control()
        self._put(TARGET, [self.max_levels])
        for f in self._followers:
            f.reset()                                 # (behind the record's zero: the data of level 0's field; base = 0)

    # ---- checkpoints -----------------------------------------------------------------------------------------------------------
    def state_dict(self):
        """TrainStep's; with `time_bc` also the time the boundary data have reached: `gfv_time_bc` = {"clock": levels completed,
        this object's clock offset included} (one synchronisation); with `time_scheme` also `gfv_time_scheme` = {"scheme",
        "has_previous", "previous" [N, 2] CPU tensor}: the velocity of level count - 1 (one synchronisation), and with an adaptive
        scheme its "dt_last" [B] and "time" [B].  The march record itself is not part of it."""
        sd = super().state_dict()
        if self.time_scheme is not None:
            sd["gfv_time_scheme"] = self.time_scheme.state_dict()
        if self.time_bc is not None:
            sd["gfv_time_bc"] = {"clock": self._read_record()[LEVEL] + self.time_bc.clock_offset}
        return sd

    def load_state_dict(self, sd):
        """TrainStep's; with `time_bc` the boundary data of the level that comes next are put in place: clock = the saved count + 1
        (a dict without `gfv_time_bc`: this object's own level count + 1); with `time_scheme` the saved previous level is
        installed as the constructor's `previous=` would (a dict without `gfv_time_scheme`: the history is forgotten).  The field
        itself is the caller's to carry over (`graphs[0].x` of the new object, or `reset(x=)` before loading)."""
        saved_ts = sd.get("gfv_time_scheme") if self.time_scheme is not None else None
        if saved_ts is not None and saved_ts.get("scheme") != self.time_scheme.scheme:
            raise ValueError(f"the state of a {saved_ts.get('scheme')!r} time scheme does not load into a "
                             f"{self.time_scheme.scheme!r} one")
        super().load_state_dict(sd)
        if self.time_scheme is not None:
            self.time_scheme.load_state_dict(saved_ts if saved_ts is not None else {"scheme": self.time_scheme.scheme})
        if self.time_bc is not None:
            saved = sd.get("gfv_time_bc")
            level = self._read_record()[LEVEL]
            clock = level if saved is None else int(saved["clock"])
            if clock < level:
                raise ValueError(f"the saved boundary-data clock {clock} lies before this object's level count {level}")
            self.time_bc.set_clock_offset(clock - level)
