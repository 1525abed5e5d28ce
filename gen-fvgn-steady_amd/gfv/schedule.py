"""Learning-rate schedules evaluated on the device (include/gfv.h gfv_lr_schedule, csrc/sched.hip).

Both training drivers of the reference attach a `StepexpLRScheduler` to Adam and call `lr_scheduler.step()` - once per epoch
(pre_train_Adam.py:203), once per TIME LEVEL (solve_with_grad_GPU.py:197); utils/scheduler.py also ships `ExpLR` and
`GradualStepExplrScheduler`, which can hand over to torch's `ReduceLROnPlateau`.  Here the rate lives in device memory
(`hyper[0]`, one `lr` word per parameter-group row) and the host no longer knows where training stands: a march ends its levels
on the device, the loss of a step reaches the host once per epoch at best.  So the schedule is a device record plus one small
launch that writes the rate where the Adam launches already read it:

    ts = TrainStep(model, graphs, lr=1e-3, schedule=StepExp(1e-3, 10, 1.0, 50, 1e-1, 100, 1e-6))
    ts.schedule.tick()                       # lr_scheduler.step(): one launch, no copy
    ms = MarchStep(model, graphs, schedule=StepExp(...))    # one scheduler step per time level, decided on the device
    ts = TrainStep(model, graphs, schedule=Plateau(factor=0.5, patience=5)); ts.schedule.tick()   # observes ts.loss
    Table.from_torch(lambda opt: torch.optim.lr_scheduler.CosineAnnealingLR(opt, 100), base_lr=1e-3, n=101)

The classes and their argument names are the reference's and torch's: `StepExp` (StepexpLRScheduler), `Exp` (ExpLR),
`GradualStepExp` (the non-plateau branch of GradualStepExplrScheduler), `Plateau` (ReduceLROnPlateau, mode "min", threshold mode
"rel", with the optional linear warm-up of GradualStepExplrScheduler.step_ReduceLROnPlateau) and `Table` (any host scheduler,
evaluated once in advance).  `base_lr` is the optimiser's initial rate there; here it is the owner's `lr` unless given.

Argument checks need no GPU.  Each object owns its device record, allocated once (`to(device)`; a step object does it when the
schedule is attached), never reallocated: recorded lists hold its address.  A schedule belongs to one step object.

What the record holds and what each mode does: include/gfv.h.  Host-written words are written here, in stream order."""
from __future__ import annotations

import math
import numbers
import struct

import torch

from . import lib as L

# 32-bit words / doubles of the record (include/gfv.h gfv_lr_schedule)
W_KIND, W_EPOCH, W_N_MILESTONES, W_NUM_BAD, W_COOLDOWN_LEFT, W_PATIENCE, W_COOLDOWN, W_WARMUP = range(8)
W_STEP_MILESTONE, W_EXP_MILESTONE, W_TOTAL_EPOCH, W_FOLLOW_CAP = 8, 9, 10, 11
W_MILESTONES = 40
D_LR, D_BASE_LR, D_MIN_LR, D_GAMMA, D_EXPGAMMA, D_DECAY_STEPS, D_START_LR, D_BEST, D_FACTOR, D_THRESHOLD, D_EPS, D_MULTIPLIER = range(8, 20)


def _real(name, v, lo=None, lo_open=False):
    if isinstance(v, bool) or not isinstance(v, numbers.Real) or math.isnan(v) or math.isinf(v):
        raise ValueError(f"{name} must be a finite number, got {v!r}")
    if lo is not None and (v <= lo if lo_open else v < lo):
        raise ValueError(f"{name} must be {'>' if lo_open else '>='} {lo}, got {v!r}")
    return float(v)


def _int(name, v, lo=0):
    if isinstance(v, bool) or not isinstance(v, numbers.Integral):
        raise ValueError(f"{name} must be an integer, got {v!r}")
    if v < lo or v >= 2 ** 31:
        raise ValueError(f"{name} must lie in [{lo}, 2^31), got {v!r}")
    return int(v)


class Schedule:
    """What the five kinds share: the device record, the launches, the state."""
    KIND = 0

    def __init__(self, base_lr=None):
        self.base_lr = None if base_lr is None else _real("base_lr", base_lr, 0.0)
        self.rec = None           # device record: GFV_SCHED_RECORD doubles
        self._scales = None       # device: one double per parameter group of the owner
        self._n_scales = 0
        self._own_hyper = None    # hyper[8] of a schedule without an owner
        self._owner = None
        self._table_dev = None
        self.follow_cap = -1

    # ---- the record on the host (needs no GPU) ------------------------------------------------------------------------------------
    def _fill(self, w, d):
        """The kind's host-written words into the int32 view `w` and the float64 view `d` of a record."""
        raise NotImplementedError

    def _start(self):
        """(epoch, rate) of a new object."""
        return 0, self._need_base()

    def _need_base(self):
        if self.base_lr is None:
            raise ValueError(f"{type(self).__name__}: base_lr is not known yet (give base_lr=, or attach the schedule to a step object: "
                             "its lr is the base rate)")
        return self.base_lr

    def pack(self):
        """The record of a new object: a CPU float64 tensor of GFV_SCHED_RECORD doubles."""
        d = torch.zeros(L.SCHED_RECORD, dtype=torch.float64)
        w = d.view(torch.int32)
        epoch, lr = self._start()
        w[W_KIND], w[W_EPOCH], w[W_FOLLOW_CAP] = self.KIND, epoch, self.follow_cap
        d[D_LR], d[D_BEST] = lr, math.inf
        d[D_BASE_LR] = self._need_base()
        self._fill(w, d)
        return d

    # ---- the device side ---------------------------------------------------------------------------------------------------------
    def to(self, device):
        """Allocate the record on `device` (once) and write the new object's words.  -> self"""
        if self.rec is not None:
            if torch.device(device) != self.rec.device:
                raise RuntimeError("a schedule's device record is allocated once and stays where it is")
            return self
        host = self.pack()
        self.rec = torch.zeros(L.SCHED_RECORD, dtype=torch.float64, device=device)
        self._scales = torch.ones(L.MAX_PARAM_GROUPS, dtype=torch.float64, device=device)
        self._own_hyper = torch.zeros(8, dtype=torch.float32, device=device)
        self._make_table(device)
        self.rec.copy_(host)
        return self

    def _make_table(self, device):
        pass

    def _attach(self, owner):
        """Called by a step object's constructor: the owner's lr is the base rate unless one was given; one EVAL."""
        if self._owner is not None and self._owner is not owner:
            raise ValueError("this schedule is already attached to another step object (it owns one rate)")
        if self.base_lr is None:
            self.base_lr = _real("lr", owner.lr, 0.0)
        self._owner = owner
        self.to(owner.dev)
        self._sync_scales()
        self.eval()

    def _sync_scales(self):
        gs = self._owner._gs
        scales = [float(g["lr_scale"]) for g in gs.groups]
        self._n_scales = len(scales)
        self._scales[:len(scales)].copy_(torch.tensor(scales, dtype=torch.float64))

    def _target(self):
        """(hyper, group table or None, number of groups) the launch writes to."""
        o = self._owner
        if o is None:
            return self._own_hyper, None, 0
        pg = o._pg
        return o.hyper, (None if pg is None else pg.table), (0 if pg is None else self._n_scales)

    def _launch(self, mode, metric=None, counter=None):
        if self.rec is None:
            raise RuntimeError("the schedule has no device record yet: to(device), or attach it to a step object")
        hyper, table, n = self._target()
        tab = self._table_dev
        L.check(L.load().gfv_lr_schedule(self.rec.data_ptr(), mode, hyper.data_ptr(), None if table is None else table.data_ptr(),
                                         self._scales.data_ptr(), n, None if tab is None else tab.data_ptr(),
                                         0 if tab is None else tab.numel(), metric, counter, L.stream_ptr()), "gfv_lr_schedule")

    def eval(self):
        """Recompute the rate from the record and write it out (idempotent)."""
        self._launch(L.SCHED_EVAL)

    def tick(self, metric=None):
        """The host's lr_scheduler.step(): epoch += 1 and the new rate, in one launch.  `metric` is for Plateau."""
        if metric is not None:
            raise ValueError(f"{type(self).__name__}.tick takes no metric (only Plateau observes one)")
        self._launch(L.SCHED_TICK)

    def follow(self, counter_ptr):
        """epoch = the 32-bit device word at `counter_ptr` (capped by follow_cap), then as eval(): part of a step body."""
        self._launch(L.SCHED_FOLLOW, counter=counter_ptr)

    def set_follow_cap(self, cap):
        """The largest epoch a FOLLOW launch sets (negative: none); written in stream order."""
        self.follow_cap = int(cap)
        if self.rec is not None:
            self.rec.view(torch.int32)[W_FOLLOW_CAP:W_FOLLOW_CAP + 1].copy_(torch.tensor([self.follow_cap], dtype=torch.int32))

    # ---- reading and restoring (each synchronises once) -----------------------------------------------------------------------
    def _read(self):
        if self.rec is None:
            raise RuntimeError("the schedule has no device record yet")
        d = self.rec.cpu()
        return d.view(torch.int32), d

    def current_lr(self):
        """The unrounded rate of the record, a Python float (synchronises)."""
        return float(self._read()[1][D_LR])

    @property
    def epoch(self):
        return int(self._read()[0][W_EPOCH])

    def state_dict(self):
        w, d = self._read()
        return {"kind": type(self).__name__, "epoch": int(w[W_EPOCH]), "lr": float(d[D_LR]), "best": float(d[D_BEST]),
                "num_bad": int(w[W_NUM_BAD]), "cooldown_left": int(w[W_COOLDOWN_LEFT])}

    def load_state_dict(self, sd):
        if sd.get("kind") != type(self).__name__:
            raise ValueError(f"the state of a {sd.get('kind')} schedule does not load into a {type(self).__name__}")
        if self.rec is None:
            raise RuntimeError("the schedule has no device record yet")
        ints = torch.tensor([int(sd["epoch"])], dtype=torch.int32)
        bad = torch.tensor([int(sd["num_bad"]), int(sd["cooldown_left"])], dtype=torch.int32)
        w = self.rec.view(torch.int32)
        w[W_EPOCH:W_EPOCH + 1].copy_(ints)
        w[W_NUM_BAD:W_NUM_BAD + 2].copy_(bad)
        self.rec[D_LR:D_LR + 1].copy_(torch.tensor([float(sd["lr"])], dtype=torch.float64))
        self.rec[D_BEST:D_BEST + 1].copy_(torch.tensor([float(sd["best"])], dtype=torch.float64))
        self.eval()


def check_schedule(schedule):
    """The constructor check of the step objects' `schedule=`; needs no GPU."""
    if schedule is None:
        return
    if not isinstance(schedule, Schedule):
        raise TypeError(f"schedule must be a gfv.schedule object (StepExp, Exp, GradualStepExp, Table, Plateau), got {schedule!r}")
    if schedule._owner is not None:
        raise ValueError("this schedule is already attached to a step object (it owns one rate)")


class StepExp(Schedule):
    """The reference's StepexpLRScheduler: startlr, then startlr * steplr_gamma from steplr_milestone, then from explr_milestone
    min_lr + max(base_lr * steplr_gamma - min_lr, 0) * explr_gamma ** ((epoch - explr_milestone) / (total_epoch - explr_milestone))
    - continued past total_epoch."""
    KIND = L.SCHED_STEPEXP

    def __init__(self, startlr, steplr_milestone, steplr_gamma, explr_milestone, explr_gamma, total_epoch, min_lr, base_lr=None):
        super().__init__(base_lr)
        self.startlr = _real("startlr", startlr, 0.0)
        self.steplr_milestone = _int("steplr_milestone", steplr_milestone)
        self.steplr_gamma = _real("steplr_gamma", steplr_gamma, 0.0)
        self.explr_milestone = _int("explr_milestone", explr_milestone)
        self.explr_gamma = _real("explr_gamma", explr_gamma, 0.0, lo_open=True)
        self.total_epoch = _int("total_epoch", total_epoch)
        self.min_lr = _real("min_lr", min_lr, 0.0)
        if self.total_epoch <= self.explr_milestone:
            raise ValueError(f"total_epoch = {total_epoch} must exceed explr_milestone = {explr_milestone}: the decay runs over their "
                             "difference (the reference divides by it)")

    def _need_base(self):
        return self.startlr if self.base_lr is None else self.base_lr     # (without an owner: the drivers' startlr = lr)

    def _fill(self, w, d):
        w[W_STEP_MILESTONE], w[W_EXP_MILESTONE], w[W_TOTAL_EPOCH] = self.steplr_milestone, self.explr_milestone, self.total_epoch
        d[D_MIN_LR], d[D_GAMMA], d[D_EXPGAMMA], d[D_START_LR] = self.min_lr, self.steplr_gamma, self.explr_gamma, self.startlr
        d[D_DECAY_STEPS] = float(self.total_epoch - self.explr_milestone)


class Exp(Schedule):
    """The reference's ExpLR: min_lr + max(base_lr - min_lr, 0) * gamma ** (epoch / decay_steps)."""
    KIND = L.SCHED_EXP

    def __init__(self, decay_steps=10000, gamma=0.4, min_lr=1e-7, base_lr=None):
        super().__init__(base_lr)
        self.decay_steps = _real("decay_steps", decay_steps, 0.0, lo_open=True)
        self.gamma = _real("gamma", gamma, 0.0, lo_open=True)
        self.min_lr = _real("min_lr", min_lr, 0.0)

    def _fill(self, w, d):
        d[D_MIN_LR], d[D_GAMMA], d[D_DECAY_STEPS] = self.min_lr, self.gamma, self.decay_steps


class GradualStepExp(Schedule):
    """The non-plateau branch of the reference's GradualStepExplrScheduler: base_lr * gamma ** (milestones reached) up to
    total_epoch, then min_lr + max(that - min_lr, 0) * expgamma ** ((epoch - total_epoch) / decay_steps).  Its refusals: a milestone
    above total_epoch, multiplier < 1 (the multiplier acts in the plateau branch only: see Plateau)."""
    KIND = L.SCHED_GRADUAL

    def __init__(self, multiplier, milestone, gamma, expgamma, total_epoch, decay_steps, min_lr=1e-6, base_lr=None):
        super().__init__(base_lr)
        self.total_epoch = _int("total_epoch", total_epoch)
        ms = [_int("milestone", m) for m in milestone]
        for m in ms:
            if m > self.total_epoch:
                raise ValueError("steps in milestone should be smaller than total_epoch")
        self.multiplier = _real("multiplier", multiplier)
        if self.multiplier < 1.0:
            raise ValueError("multiplier should be greater than or equal to 1.")
        self.milestone = sorted(set(ms))          # (the reference tests `epoch in milestone`: a repeated entry counts once)
        if len(self.milestone) > L.SCHED_MAX_MILESTONES:
            raise ValueError(f"{len(self.milestone)} milestones: at most {L.SCHED_MAX_MILESTONES}")
        self.gamma = _real("gamma", gamma, 0.0)
        self.expgamma = _real("expgamma", expgamma, 0.0, lo_open=True)
        self.decay_steps = _real("decay_steps", decay_steps, 0.0, lo_open=True)
        self.min_lr = _real("min_lr", min_lr, 0.0)

    def _fill(self, w, d):
        w[W_N_MILESTONES], w[W_TOTAL_EPOCH] = len(self.milestone), self.total_epoch
        for i, m in enumerate(self.milestone):
            w[W_MILESTONES + i] = m
        d[D_MIN_LR], d[D_GAMMA], d[D_EXPGAMMA], d[D_DECAY_STEPS] = self.min_lr, self.gamma, self.expgamma, self.decay_steps


class Table(Schedule):
    """lr = values[min(epoch, len(values) - 1)]: any host scheduler, evaluated once in advance (doubles, on the device)."""
    KIND = L.SCHED_TABLE

    def __init__(self, values):
        vals = [_real("a table entry", v, 0.0) for v in values]
        if not vals:
            raise ValueError("Table: at least one rate")
        super().__init__(vals[0])
        self.values = vals

    @classmethod
    def from_torch(cls, make_scheduler, base_lr, n):
        """The first n rates of `make_scheduler(optimizer)` - a torch scheduler - on a throw-away CPU optimiser of rate base_lr,
        driven as the drivers drive theirs: optimizer.step(); scheduler.step()."""
        n = _int("n", n, 1)
        p = torch.nn.Parameter(torch.zeros(1))
        opt = torch.optim.SGD([p], lr=_real("base_lr", base_lr, 0.0))
        sch = make_scheduler(opt)
        vals = []
        for _ in range(n):
            vals.append(float(opt.param_groups[0]["lr"]))
            opt.step()
            sch.step()
        return cls(vals)

    def _start(self):
        return 0, self.values[0]

    def _fill(self, w, d):
        pass

    def _make_table(self, device):
        self._table_dev = torch.tensor(self.values, dtype=torch.float64).to(device)


class Plateau(Schedule):
    """torch.optim.lr_scheduler.ReduceLROnPlateau with mode "min" and threshold_mode "rel", its state in the device record; with
    warmup_epochs > 0 the linear warm-up of the reference's GradualStepExplrScheduler.step_ReduceLROnPlateau in front of it
    (warmup_epochs is its total_epoch): base_lr * epoch / warmup_epochs with multiplier 1, else
    base_lr * ((multiplier - 1) * epoch / warmup_epochs + 1), the plateau rule observing nothing until epoch > warmup_epochs.  As the
    reference's constructor leaves its object, a warming schedule starts at epoch 1.

    tick(metric=None) observes the owner's `loss` (the last step's); any 1-element fp32 device tensor may be given instead."""
    KIND = L.SCHED_PLATEAU

    def __init__(self, factor=0.1, patience=10, threshold=1e-4, cooldown=0, min_lr=0.0, eps=1e-8, warmup_epochs=0, multiplier=1.0,
                 base_lr=None):
        super().__init__(base_lr)
        self.factor = _real("factor", factor)
        if self.factor >= 1.0:
            raise ValueError("Factor should be < 1.0.")
        self.patience = _int("patience", patience)
        self.threshold = _real("threshold", threshold)
        self.cooldown = _int("cooldown", cooldown)
        self.min_lr = _real("min_lr", min_lr, 0.0)
        self.eps = _real("eps", eps)
        self.warmup_epochs = _int("warmup_epochs", warmup_epochs)
        self.multiplier = _real("multiplier", multiplier)
        if self.multiplier < 1.0:
            raise ValueError("multiplier should be greater than or equal to 1.")

    def _start(self):
        base = self._need_base()
        if self.warmup_epochs > 0:
            return 1, warmup_rate(base, self.multiplier, 1, self.warmup_epochs)
        return 0, base

    def _fill(self, w, d):
        w[W_PATIENCE], w[W_COOLDOWN], w[W_WARMUP] = self.patience, self.cooldown, self.warmup_epochs
        d[D_MIN_LR], d[D_FACTOR], d[D_THRESHOLD], d[D_EPS], d[D_MULTIPLIER] = (self.min_lr, self.factor, self.threshold, self.eps,
                                                                              self.multiplier)

    def tick(self, metric=None):
        o = self._owner
        if metric is None:
            if o is None:
                raise ValueError("Plateau.tick: a schedule without a step object needs metric= (a 1-element fp32 device tensor)")
            if o.dist_on:
                raise ValueError("Plateau.tick(metric=None) under data parallelism: the step's loss is rank-local and the ranks' "
                                 "rates would part; give a metric every rank holds alike")
            metric = o.loss
        if not (isinstance(metric, torch.Tensor) and metric.is_cuda and metric.dtype == torch.float32 and metric.numel() == 1):
            raise ValueError("Plateau.tick: metric must be a 1-element float32 device tensor")
        self._launch(L.SCHED_TICK, metric=metric.data_ptr())

    def follow(self, counter_ptr):
        raise ValueError("Plateau cannot follow a device counter: there is no metric to observe")


def warmup_rate(base_lr, multiplier, epoch, warmup_epochs):
    """The warm-up of GradualStepExplrScheduler.step_ReduceLROnPlateau at `epoch` <= warmup_epochs."""
    if multiplier == 1.0:
        return base_lr * (float(epoch) / warmup_epochs)
    return base_lr * ((multiplier - 1.0) * epoch / warmup_epochs + 1.0)


def f32(x):
    """float32(x) as a Python float."""
    return struct.unpack("f", struct.pack("f", float(x)))[0]
