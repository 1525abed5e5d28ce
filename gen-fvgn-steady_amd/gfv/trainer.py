"""Training-step driver: forward + loss + backward (+ RCCL gradient all-reduce) + fused Adam on the HIP engine.

Reproduces the call sequence of the reference's drivers for ONE batch kept on the device
(solve_with_grad_GPU.py:133-181: restore `x` from a backup and re-arm the norm flags every inner step;
pre_train_Adam.py:158-191: zero_grad, forward, `mean(log(weighted residuals))`, backward, Adam), without the autograd
tape: parameters, gradients and Adam moments live in flat fp32 buffers, so the optimiser is one kernel and the
data-parallel exchange is ONE all-reduce of 4.7 MB.  The fixed launch sequence can be captured into
a hipGraph (torch.cuda.CUDAGraph, kept in `_captures`) or recorded as a command list (gfv/cmdlist.py, kept in `_lists`: a
`gfv.listcache.ListCache`, the policy of every recorded path) to remove host launch overhead.

One step skeleton serves `TrainStep`, `gfv.pool_trainer.PoolTrainStep` and `gfv.march.MarchStep`: `_step_head`, a launch path (`_issue`:
eager, recorded or replayed; `_capture_step`: hipGraph), `_step_tail`.  A subclass adds through hooks: `_after_backward` (launches in
the body), `_hold_record` (whose apply flag the optimiser reads), `_list_stamp` / `_list_valid` (what a list must find unmoved).
"""
from __future__ import annotations

import contextlib

import torch

from . import cmdlist
from . import lib as L
from . import listcache
from .accum import GradAccum, check_accum_steps
from .balance import check_balance
from .ema import WeightEMA, check_ema
from .engine import GradStore
from .functions import unused_param_names
from .groups import ParamGroups, check_groups, check_weight_decay
from .guard import GradGuard, check_policy
from .observe import Observations, check_observe
from .optstep import optimizer_launches
from .plan import _live_key, _refresh_live, get_plan
from .schedule import check_schedule
from .timescheme import check_owner as check_time_scheme
from .trainlog import make_log


def _gather(src, index, out):
    torch.index_select(src, 0, index, out=out)


def check_train_args(who, obs_kind, model, *, world_size=1, distributed=None, max_grad_norm=None, skip_on_flag=False,
                     accum_steps=1, ema_decay=None, ema_warmup=True, weight_decay=0.0, decoupled_weight_decay=True,
                     param_groups=None, schedule=None, balance=None, observations=None, time_scheme=None, **unchecked):
    """The constructor checks of the step objects, in the order they have always been made; needs no GPU.  who: the class name the
    messages carry; obs_kind: what its `observations=` takes; the keywords are TrainStep's (`unchecked`: those nothing is checked
    of).  -> (dist_on, accum_steps, ema_decay, the GroupSpec)"""
    # distributed=True with world_size 1 sends the step through the same collectives (identity all-reduce): the
    # RCCL path can then be exercised on a single GPU (tests/test_rccl_gpu.py)
    dist_on = (world_size > 1) if distributed is None else bool(distributed)
    check_policy(max_grad_norm, skip_on_flag, dist_on)
    accum_steps = check_accum_steps(accum_steps, dist_on)
    ema_decay = check_ema(ema_decay, ema_warmup)
    spec = check_groups(*model.param_names_tensors(), weight_decay, decoupled_weight_decay, param_groups)
    check_schedule(schedule)
    check_balance(balance, dist_on, world_size, who)
    check_observe(observations, balance, who, obs_kind)
    check_time_scheme(time_scheme)
    return dist_on, accum_steps, ema_decay, spec


class TrainStep:
    _OBS_KIND = Observations          # what `observations=` takes (PoolTrainStep: PoolObservations)
    max_list_bytes = None             # the byte budget of the recorded lists: unbounded (PoolTrainStep: its argument)

    def __init__(self, model, graphs, *, lr=None, betas=(0.9, 0.999), eps=1e-8, loss_weights=None, world_size=1,
                 process_group=None, use_graph=False, want_outputs=True, distributed=None, max_grad_norm=None,
                 skip_nonfinite=False, skip_on_flag=False, accum_steps=1, ema_decay=None, ema_warmup=True, weight_decay=0.0,
                 decoupled_weight_decay=True, param_groups=None, log=None, schedule=None, balance=None, observations=None,
                 time_scheme=None):
        dist_on, accum_steps, ema_decay, spec = check_train_args(
            type(self).__name__, self._OBS_KIND, model, world_size=world_size, distributed=distributed, max_grad_norm=max_grad_norm,
            skip_on_flag=skip_on_flag, accum_steps=accum_steps, ema_decay=ema_decay, ema_warmup=ema_warmup, weight_decay=weight_decay,
            decoupled_weight_decay=decoupled_weight_decay, param_groups=param_groups, schedule=schedule, balance=balance,
            observations=observations, time_scheme=time_scheme)
        self.time_scheme = None
        self.schedule = None
        self.balance = None
        self.observations = None
        self.model = model
        self.graphs = graphs
        self.plan = get_plan(graphs)
        self._live = _live_key(graphs)
        self.engine = model.engine()
        p = model.params
        self._hyper_host = None
        self._gs, self._pg, self._stateful = spec, None, None
        self._lr = p.lr if lr is None else lr
        self._betas, self._eps = tuple(betas), eps
        self._lw = tuple(loss_weights or (p.loss_cont, p.loss_mom, p.loss_press))
        self.world_size, self.pg = world_size, process_group
        self.dist_on = dist_on
        self.engine.dist_world, self.engine.dist_group = world_size, process_group
        self.engine.dist_force = self.dist_on
        self.use_graph = use_graph
        self._split, self._comm, self._early = None, None, False
        self.want_outputs = want_outputs
        dev = graphs[0].x.device
        self.dev = dev

        # flat parameter / gradient / moment buffers; the module's parameters become views of the flat buffer
        names, tensors = model.param_names_tensors()
        skip = unused_param_names(names)
        self.flat_g = None
        self.G = GradStore(names, [t.shape for t in tensors], dev, skip=skip)
        self.flat_g = self.G.flat
        total = self.G.total
        self.flat_p = torch.zeros(total + 4, dtype=torch.float32, device=dev)[:total + 1]   # (+ one zero the padding maps read)
        self.flat_m = torch.zeros(total, dtype=torch.float32, device=dev)
        self.flat_v = torch.zeros(total, dtype=torch.float32, device=dev)
        # Adam step counter + derived bias corrections, and the hyper-parameters: device resident (include/gfv.h,
        # gfv_adam_step_dev), so a captured step follows `ts.lr = ...` (lr_scheduler.step() in the reference drivers)
        # (adam_state[16] = {completed steps, the NEXT step's bias corrections, arrival counter, 1 - betas, running powers}: include/gfv.h)
        self.adam_state = torch.zeros(16, dtype=torch.float32, device=dev)
        self.hyper = torch.zeros(8, dtype=torch.float32, device=dev)
        self._sync_hyper()
        L.status_mirror()   # the fused Adam publishes the device status word from now on; step() reads it without a sync
        self.P = {}
        for n, t in zip(names, tensors):
            off, k = self.G.off[n], t.numel()
            view = self.flat_p[off:off + k].view(t.shape)
            view.copy_(t.data)
            t.data = view
            self.P[n] = view
        assert all(v.data_ptr() % 16 == 0 for v in self.P.values())
        self._setup_padding(names, tensors, skip)
        self._probes = [(names[i], tensors[i]) for i in sorted({0, len(names) // 2, len(names) - 1})]
        self.n_params = total
        # training guard (gfv/guard.py): the device record the two guarded launches of _adam() read.  Its policy -
        # max_grad_norm, skip_nonfinite, skip_on_flag - is mirrored into it on change; with all three off _adam() is one launch
        self._guard = GradGuard(self.G, dev, max_grad_norm, skip_nonfinite, skip_on_flag)
        # gradient accumulation (gfv/accum.py): None with accum_steps == 1 - no second buffer, _adam() as it was
        self._accum = GradAccum(total, dev, accum_steps) if accum_steps > 1 else None
        # averaged weights (gfv/ema.py): None with ema_decay None - no third buffer, _adam() as it was
        self._ema_warmup = bool(ema_warmup)
        self._ema = WeightEMA(self.flat_p, total, ema_decay, self._ema_warmup) if ema_decay is not None else None
        # what has been recorded of the step: command lists per (accumulate, distributed) under the one list policy (gfv/listcache.py:
        # warm up, record once, replay, never issue a stale list); hipGraph captures as (CUDAGraph, engine signature) per the same key
        self._lists = listcache.ListCache(self.max_list_bytes, dev=dev)
        self._captures = {}
        # parameter groups (gfv/groups.py): None with everything at its default - no table, _adam() as it was
        self.log = None
        spec.skip = set(self.G.skip)
        spec.check_some_live([g["frozen"] for g in spec.groups])
        self._groups_changed(frozen_changed=bool(spec.frozen_names()))
        # learning-rate schedule (gfv/schedule.py): None - no launch, no allocation, `ts.lr = v` as it was.  Attached,
        # it owns hyper[0] and the lr word of every group row: one EVAL launch here, `ts.schedule.tick()` per epoch
        if schedule is not None:
            self.schedule = schedule
            schedule._attach(self)
            self._lr = schedule.base_lr                             # (ts.lr reads back the base rate)
        # loss balancing (gfv/balance.py): None - no launch, no allocation, `ts.loss_weights = v` as it was.  Attached,
        # it owns hyper[5:8]: the constructor's loss_weights are its base weights, one launch follows every step (_balance_step)
        if balance is not None:
            self.balance = balance
            balance._attach(self)
        # observation term (gfv/observe.py): None - no launch, no allocation, the step body as it was.  Attached, two
        # launches join the step body (_body): the loss launch's `loss` / `gloss` are overwritten, the decoder gradient added to
        if observations is not None:
            observations._attach(self)
            self.observations = observations
        # training log (gfv/trainlog.py): None with log=None - no launch, no allocation.  An int capacity, a
        # TrainLog or a dict of its arguments; its two launches follow every step eagerly (_log_step), outside lists and graphs
        self.log = make_log(log, self.plan.B)
        if self.log is not None:
            self.log.bind(self.G, dev, spec.frozen_names(), owner=self)
        self.x = graphs[0].x
        self.x_backup = self.x.clone()
        B = self.plan.B
        self.loss = torch.zeros(1, dtype=torch.float32, device=dev)
        self.gloss = torch.zeros((B, 4), dtype=torch.float32, device=dev)
        self.losses = None
        self.uvp_node = None
        # time differencing (gfv/timescheme.py): None - no launch, no allocation, the forward as it was.  Attached
        # (last: nothing has been recorded yet), the finite-volume section reads its two tensors and advance_time() issues its launch
        if time_scheme is not None:
            self.time_scheme = time_scheme.attach(self, self.plan, self.x_backup)

    # hidden_size below 128 (FVMmodel/padding.py): parameters, moments and gradients of the TRUE shapes stay the state
    # (flat_p / flat_m / flat_v / flat_g, what Adam and the checkpoints see); every step gathers the parameters into the
    # kernels' 128-column shapes with one index_select, runs forward / backward on those, and gathers the gradients back
    # with another.  The two index maps come from padding the flat offsets themselves.
    def _setup_padding(self, names, tensors, skip):
        from FVMmodel.padding import pad_parameters
        h = int(getattr(self.model, "hidden_size", 128))
        self.padded = h != 128
        if not self.padded:
            self.P_run, self.G_run = self.P, self.G
            return
        dev, total = self.dev, self.G.total
        offs = [torch.arange(t.numel(), device=dev, dtype=torch.int64).view(t.shape) + (self.G.off[n] + 1)
                for n, t in zip(names, tensors)]                       # flat offset + 1 of every true element (0 = padding)
        padded = pad_parameters(names, offs, h)
        self.G_run = GradStore(names, [t.shape for t in padded], dev, skip=skip)
        fwd = torch.full((self.G_run.total,), total, dtype=torch.int64, device=dev)   # -> the zero behind flat_p
        back = torch.zeros(total, dtype=torch.int64, device=dev)
        for n, t in zip(names, padded):
            o = self.G_run.off[n]
            flat = t.reshape(-1)
            real = flat > 0
            fwd[o:o + flat.numel()] = torch.where(real, flat - 1, torch.full_like(flat, total))
            back[(flat[real] - 1)] = o + torch.nonzero(real).reshape(-1)
        self._pad_map, self._unpad_map = fwd, back
        self.flat_pp = torch.zeros(self.G_run.total, dtype=torch.float32, device=dev)
        self.P_run = {n: self.flat_pp[self.G_run.off[n]:self.G_run.off[n] + self.G_run.numel(n)].view(self.G_run.shape[n])
                      for n in names}

    # hyper-parameters: plain attributes on the host, mirrored into `self.hyper` on change --------------------------
    def _sync_hyper(self):
        vals = (self._lr, self._betas[0], self._betas[1], self._eps, 1.0 / self.world_size, *self._lw)
        if vals != self._hyper_host:
            betas_moved = self._hyper_host is None or vals[1:3] != self._hyper_host[1:3]
            if self.schedule is None and self.balance is None:
                self.hyper.copy_(torch.tensor(vals, dtype=torch.float32))
            else:
                # (word 0 is the schedule's, words 5 .. 7 are the balancer's)
                lo, hi = (0 if self.schedule is None else 1), (8 if self.balance is None else 5)
                self.hyper[lo:hi].copy_(torch.tensor(vals[lo:hi], dtype=torch.float32))
            self._hyper_host = vals
            if betas_moved:
                self._init_adam_state()
        if self._pg is not None:
            self._pg.sync(self._gs.values(self._lr), self._gs.decoupled)   # (every group's rate is lr * lr_scale)
            self._sched_eval()

    def _sched_eval(self):
        """Behind every host write of the group table: the schedule's scales follow the groups and one EVAL launch puts the
        scheduled rate back into the rows (in stream order: no step runs in between)."""
        if self.schedule is not None:
            self.schedule._sync_scales()
            self.schedule.eval()

    def _init_adam_state(self, steps_done=None):
        """The device-side bias corrections of the next step, from the step count (a new object, a loaded checkpoint, new betas)."""
        t = float(self.adam_state[0]) if steps_done is None else float(steps_done)
        L.check(L.load().gfv_adam_state_init(self.adam_state.data_ptr(), float(self._betas[0]), float(self._betas[1]), t,
                                             L.stream_ptr()), "adam_state_init")

    lr = property(lambda self: self._lr)
    betas = property(lambda self: self._betas)
    eps = property(lambda self: self._eps)
    loss_weights = property(lambda self: self._lw)
    w_cont = property(lambda self: self._lw[0])
    w_mom = property(lambda self: self._lw[1])
    w_press = property(lambda self: self._lw[2])

    @lr.setter
    def lr(self, v):
        if self.schedule is not None:
            raise RuntimeError("the attached schedule owns the learning rate (ts.schedule.tick(); ts.lr reads the base rate)")
        self._lr = float(v)
        self._sync_hyper()

    @betas.setter
    def betas(self, v):
        self._betas = (float(v[0]), float(v[1]))
        self._sync_hyper()

    @eps.setter
    def eps(self, v):
        self._eps = float(v)
        self._sync_hyper()

    @loss_weights.setter
    def loss_weights(self, v):
        if self.balance is not None:
            raise RuntimeError("the attached balancer owns the loss weights (ts.balance.set_base(weights) gives it new base "
                               "weights; ts.loss_weights reads the base weights)")
        self._lw = tuple(float(x) for x in v)
        self._sync_hyper()

    # the guard's policy: attributes like lr.  A new VALUE reaches recorded lists and captured graphs through the device record;
    # only switching the guard as a whole on or off changes the launch sequence (one launch <-> two) and drops them.
    max_grad_norm = property(lambda self: self._guard.max_grad_norm)
    skip_nonfinite = property(lambda self: self._guard.skip_nonfinite)
    skip_on_flag = property(lambda self: self._guard.skip_on_flag)

    def _drop_recorded(self):
        """Recorded lists and captured graphs hold the launch sequence and the addresses of the moment they were made.  Every key
        warms up again before it is recorded again."""
        self._lists.clear()
        self._captures.clear()

    def stats(self):
        """{"replayed", "recorded", "eager", "lists", "list_bytes"}: steps per path of `_issue` (a hipGraph step counts nowhere),
        lists kept, the bytes of their private pools.  Host counts: no synchronisation."""
        return self._lists.stats()

    def _set_guard(self, **kw):
        g = self._guard
        new = dict(max_grad_norm=g.max_grad_norm, skip_nonfinite=g.skip_nonfinite, skip_on_flag=g.skip_on_flag)
        new.update(kw)
        check_policy(new["max_grad_norm"], new["skip_on_flag"], self.dist_on)
        was = g.active
        g.set(**new)
        if g.active != was:
            self._drop_recorded()

    @max_grad_norm.setter
    def max_grad_norm(self, v):
        self._set_guard(max_grad_norm=v)

    @skip_nonfinite.setter
    def skip_nonfinite(self, v):
        self._set_guard(skip_nonfinite=v)

    @skip_on_flag.setter
    def skip_on_flag(self, v):
        self._set_guard(skip_on_flag=v)

    # parameter groups: per-group rate (lr * lr_scale), weight decay and freezing inside the Adam launch
    def _groups_changed(self, frozen_changed=False):
        gs = self._gs
        if self._pg is None:
            if gs.trivial:
                return
            self._pg = ParamGroups(self.G, self.dev, gs.group_of, gs.values(self._lr), gs.decoupled)
            self._stateful = self._live_names()
            self._drop_recorded()
        self._pg.sync(gs.values(self._lr), gs.decoupled)
        self._sched_eval()
        if frozen_changed:
            frozen = gs.frozen_names()
            self._stateful |= self._live_names()
            self._guard.set_segments(self.G, frozen)
            if self.log is not None:
                self.log.set_buckets(self.G, frozen)     # (its launches are in no list: nothing more to drop)
            self._drop_recorded()

    def _live_names(self):
        """Parameters that move now: with a gradient and in no frozen group."""
        frozen = self._gs.frozen_names()
        return {n for n in self.G.off if n not in self.G.skip and n not in frozen}

    @property
    def param_groups(self):
        """[{"params": names, "lr", "lr_scale", "weight_decay", "frozen"}] per group: the caller's groups in their order, then the
        implicit default group of the parameters no group selected (lr_scale 1, the object's weight_decay, not frozen).  A group's
        rate is `ts.lr * lr_scale`; its decay is decoupled (AdamW) or an L2 term (`decoupled_weight_decay=False`) for all groups
        alike.  Read-only: change values with set_group().  betas, eps and the STEP COUNT are shared by all groups - see
        set_group() for what that means for a group that is unfrozen later."""
        return self._gs.public(self._lr)

    def set_group(self, i, lr_scale=None, weight_decay=None, frozen=None):
        """New values for group `i` of `param_groups` (None: unchanged); checked before anything changes.

        A new lr_scale or weight_decay goes through the device table the Adam launch reads: recorded lists and captured graphs
        follow it, nothing is recorded again.  A change of `frozen` also gives the guard a new segment table (its norm covers what
        clip_grad_norm_ would see: no frozen group, no parameter without a gradient) and drops lists and graphs - a rare event,
        like switching the guard on.  Freezing the last group that still moves raises ValueError.

        A frozen group keeps its bits - parameters, moments, averaged weights - whatever the decay, and has no entry in
        state_dict()["state"] until it has moved.  It is still differentiated by the backward (its gradient is computed, not used).

        One deviation from torch.optim: the step count is shared.  torch counts steps per parameter, so a group unfrozen after k
        steps starts its bias correction at 1 there; here its next step carries the shared count k + 1 with the moments it has
        (zero if it never moved): a first update of 0.58 lr instead of lr at k = 3, up to 3.2 lr for large k, until the moments
        have filled (about ten steps)."""
        self._groups_changed(self._gs.set_group(int(i), lr_scale, weight_decay, frozen))

    weight_decay = property(lambda self: self._gs.weight_decay)
    decoupled_weight_decay = property(lambda self: self._gs.decoupled)

    @weight_decay.setter
    def weight_decay(self, v):
        self._gs.weight_decay = check_weight_decay(v)
        self._groups_changed()

    # gradient accumulation: `accum_steps` is an attribute like lr.  A new value is mirrored into the device record and drops the
    # open accumulation; only a change between 1 and more than 1 changes the launch sequence and drops lists and graphs.
    @property
    def accum_steps(self):
        return 1 if self._accum is None else self._accum.steps

    @accum_steps.setter
    def accum_steps(self, v):
        v = check_accum_steps(v, self.dist_on)
        if v == self.accum_steps:
            return
        if (v > 1) != (self._accum is not None):
            self._accum = GradAccum(self.n_params, self.dev, v) if v > 1 else None
            self._drop_recorded()
        else:
            self._accum.set_steps(v)

    @property
    def accum_pending(self):
        """Micro-steps taken in the open accumulation (host count; the device count depends on nothing but the steps issued)."""
        return 0 if self._accum is None else self._accum.pending

    def accum_reset(self):
        """Drop an open accumulation: the next step is the first micro-step of a new one."""
        if self._accum is not None:
            self._accum.reset()

    def accum_stats(self):
        """{"micro", "graphs", "loss_mean", "closed"} of the device record: micro-steps and graphs of the open accumulation, the
        mean loss over the graphs of the last closed one, the number closed.  Synchronises: for logging, like guard_stats().
        Not part of state_dict(): an open accumulation is not state."""
        if self._accum is None:
            return {"micro": 0, "graphs": 0, "loss_mean": float("nan"), "closed": 0}
        return self._accum.stats()

    # averaged weights: `ema_decay` and `ema_warmup` are attributes like lr.  A new value goes to the device record through
    # gfv_ema_init and keeps the update count; only a change between None and a value changes the launch sequence and drops lists
    # and graphs (and starts the average from the current parameters).
    @property
    def ema_decay(self):
        return None if self._ema is None else self._ema.decay

    @ema_decay.setter
    def ema_decay(self, v):
        v = check_ema(v, self._ema_warmup)
        if v == self.ema_decay:
            return
        self._not_swapped("ema_decay")
        if (v is None) != (self._ema is None):
            self._ema = WeightEMA(self.flat_p, self.n_params, v, self._ema_warmup) if v is not None else None
            self._drop_recorded()
        else:
            self._ema.set(v, self._ema_warmup)

    @property
    def ema_warmup(self):
        return self._ema_warmup

    @ema_warmup.setter
    def ema_warmup(self, v):
        v = bool(v)
        if v != self._ema_warmup and self._ema is not None:
            self._ema.set(self._ema.decay, v)
        self._ema_warmup = v

    def _need_ema(self, what):
        if self._ema is None:
            raise RuntimeError(f"{what} needs the averaged weights (ema_decay=...)")
        return self._ema

    def _not_swapped(self, what):
        if self._ema is not None and self._ema.swapped:
            raise RuntimeError(f"{what} inside `with ema_weights():` - the model holds the averaged weights, not the iterate")

    def ema_reset(self):
        """The average restarts from the current parameters, the update count (and with it the warmup) from zero."""
        self._not_swapped("ema_reset()")
        if self._ema is not None:
            self._ema.reset(self.flat_p)

    def ema_stats(self):
        """{"decay", "warmup", "updates", "w"} of the device record: `updates` counts the optimiser steps that were applied (not
        the skipped ones, not the hold micro-steps), `w` is the weight of the next update.  Synchronises."""
        if self._ema is None:
            return {"decay": None, "warmup": self._ema_warmup, "updates": 0, "w": float("nan")}
        return self._ema.stats()

    def ema_parameters(self):
        """{name: CPU tensor} of the averaged weights, named and shaped as `model.param_names_tensors()` (no alignment padding)."""
        ema = self._need_ema("ema_parameters()")
        src = (self.flat_p if ema.swapped else ema.e).detach().cpu()
        return {n: self.G.view_of(src, n).clone() for n in self.G.off}

    @contextlib.contextmanager
    def ema_weights(self):
        """Inside the block the model holds the averaged weights: the CONTENTS of the parameters - views of flat_p - and of the
        average change places, so the model carries them at the addresses every recorded list and every Rollout / Sweep points
        at (their WeightGuard sees the in-place change: `refresh_weights()` first).  Swapped back on exit; no step() inside."""
        ema = self._need_ema("ema_weights()")
        self._not_swapped("ema_weights()")
        self._check_aliasing()
        names, tensors = self.model.param_names_tensors()
        offsets = [self.G.off[n] for n in names]
        ema.swap(tensors, offsets)
        try:
            yield self
        finally:
            ema.swap(tensors, offsets)

    def guard_stats(self):
        """{"norm", "coef", "decision", "clipped", "skipped_nonfinite", "skipped_flag"} of the guard: the last guarded step's
        gradient norm (after the all-reduce and the 1 / world scale), clip coefficient and decision bits (gfv.lib.GUARD_*), and
        the running counts.  Synchronises: for logging every so often, not every step.  Not part of state_dict()."""
        return self._guard.stats()

    def set_lr(self, lr):
        """What `lr_scheduler.step()` does to the reference's optimizer; eager and hipGraph steps both follow it."""
        self.lr = lr

    @property
    def step_t(self):
        return self.adam_state[0:1]

    # optimizer state in the reference's checkpoint slot (importer.py:292-313 saves `optimizer{i}`) -------------------
    def state_dict(self):
        """Same nesting as torch.optim.Adam.state_dict(): per-parameter step / exp_avg / exp_avg_sq keyed by position in
        `model.parameters()` order, one param group.  `NNmodel.save_checkpoint(path, optimizer=ts)` stores it under
        `optimizer0`, `load_checkpoint(optimizer=ts, ...)` restores it."""
        names = list(self.G.off)
        t = self.adam_state[0:1].detach().cpu().clone().reshape(())
        state = {}
        for i, n in enumerate(names):
            if n in self.G.skip or (self._stateful is not None and n not in self._stateful):
                continue   # parameters without a gradient (or frozen since construction / load) have no Adam state in torch either
            state[i] = {"step": t.clone(), "exp_avg": self.G.view_of(self.flat_m, n).detach().cpu().clone(),
                        "exp_avg_sq": self.G.view_of(self.flat_v, n).detach().cpu().clone()}
        group = {"lr": self._lr, "betas": self._betas, "eps": self._eps, "weight_decay": 0, "amsgrad": False,
                 "maximize": False, "params": list(range(len(names)))}
        sd = {"state": state, "param_groups": [group], "gfv_param_names": names, "gfv_loss_weights": self._lw}
        if self._pg is not None:
            # one entry per group in torch's nesting ("params": positions in model.parameters() order); a torch.optim.AdamW built
            # with the same grouping loads it.  lr_scale, frozen: keys torch keeps and ignores
            pos = {n: i for i, n in enumerate(names)}
            sd["param_groups"] = [dict(group, lr=g["lr"], weight_decay=g["weight_decay"], lr_scale=g["lr_scale"], frozen=g["frozen"],
                                       params=[pos[n] for n in g["params"]]) for g in self._gs.public(self._lr)]
            sd["gfv_groups"] = {"lr": self._lr, "weight_decay": self._gs.weight_decay, "decoupled": self._gs.decoupled}
        if self._ema is not None:
            # (a top-level key torch.optim.Adam.load_state_dict ignores, as it does the two above)
            avg = self.ema_parameters()
            sd["gfv_ema"] = {"decay": self._ema.decay, "warmup": self._ema.warmup, "updates": self._ema.stats()["updates"],
                             "params": [avg[n] for n in names]}
        if self.schedule is not None:
            sd["gfv_schedule"] = self.schedule.state_dict()       # (epoch, rate, plateau state: one synchronisation)
        if self.balance is not None:
            sd["gfv_balance"] = self.balance.state_dict()         # (the record's device-written words: one synchronisation)
        return sd

    def load_state_dict(self, sd):
        self._not_swapped("load_state_dict()")
        names = list(self.G.off)
        if "gfv_param_names" in sd and list(sd["gfv_param_names"]) != names:
            raise ValueError("optimizer state belongs to a different parameter set")
        # everything is checked before a buffer or a group is touched
        steps = {float(st["step"]) for st in sd["state"].values()}
        if len(steps) > 1:
            raise ValueError("per-parameter step counts differ: not a state this fused Adam can resume")
        step = steps.pop() if steps else None
        plan = self._plan_groups(sd, names)
        sched = sd.get("gfv_schedule") if self.schedule is not None else None
        if sched is not None and sched.get("kind") != type(self.schedule).__name__:
            raise ValueError(f"the state of a {sched.get('kind')} schedule does not load into a {type(self.schedule).__name__}")
        bal = sd.get("gfv_balance") if self.balance is not None else None
        if bal is not None and bal.get("kind") != type(self.balance).__name__:
            raise ValueError(f"the state of a {bal.get('kind')} balancer does not load into a {type(self.balance).__name__}")
        self.flat_m.zero_()
        self.flat_v.zero_()
        for i, st in sd["state"].items():
            n = names[int(i)]
            self.G.view_of(self.flat_m, n).copy_(st["exp_avg"].reshape(self.G.shape[n]))
            self.G.view_of(self.flat_v, n).copy_(st["exp_avg_sq"].reshape(self.G.shape[n]))
        g = sd["param_groups"][0]
        self._betas, self._eps = (float(g["betas"][0]), float(g["betas"][1])), float(g["eps"])
        frozen_moved = False
        if plan is None:
            # a dict without groups (a pre-training checkpoint, torch.optim.Adam): an object without groups takes its rate, as it
            # always did; a grouped object keeps its own rate and group values - the dict says nothing about them
            if self._pg is None:
                self._lr = float(g["lr"])
        else:
            gs = self._gs
            self._lr, gs.weight_decay, gs.decoupled = plan["lr"], plan["weight_decay"], plan["decoupled"]
            for i, (scale, wd, fr) in enumerate(plan["groups"]):
                frozen_moved |= gs.set_group(i, scale, wd, None)
                if fr is not None and fr != gs.groups[i]["frozen"]:
                    gs.groups[i]["frozen"], frozen_moved = fr, True      # (checked as a whole in _plan_groups)
        if "gfv_loss_weights" in sd:
            self._lw = tuple(float(x) for x in sd["gfv_loss_weights"])
        self._sync_hyper()
        self._groups_changed(frozen_moved)
        if self._pg is not None:
            # what has state: what the dict had state for, and what moves now (its moments are live from the next step on)
            self._stateful = {names[int(i)] for i in sd["state"]} | self._live_names()
        self._init_adam_state(0.0 if step is None else step)
        self.accum_reset()
        if self._ema is not None:
            # (the model was loaded before the optimiser: without an average in the dict it restarts from the loaded weights)
            self._ema.reset(self.flat_p)
            avg = sd.get("gfv_ema")
            if avg is not None:
                for n, t in zip(names, avg["params"]):
                    self.G.view_of(self._ema.e, n).copy_(t.reshape(self.G.shape[n]))
                self._ema_warmup = bool(avg["warmup"])
                self._ema.set(check_ema(avg["decay"]), self._ema_warmup, int(avg["updates"]))
        if self.schedule is not None:
            self._lr = self.schedule.base_lr
            if sched is not None:
                self.schedule.load_state_dict(sched)
        if self.balance is not None:
            if bal is not None:
                self.balance.load_state_dict(bal)                 # (the record and hyper[5:8]; ts.loss_weights = its base weights)
            else:
                # a dict without a balancer's state: a new record over the loaded base weights
                self.balance.set_base(self._lw)
                self.balance.reset()

    def _plan_groups(self, sd, names):
        """What a state_dict says about the groups, checked and nothing changed: None for a dict without groups (one group over
        all parameters and no `gfv_groups` key: a pre-training checkpoint loads into a grouped fine-tuning object, which keeps its
        own groups), else {"lr", "weight_decay", "decoupled", "groups": [(lr_scale, weight_decay, frozen)]} - for which the
        grouping (which parameter is in which group) must be the one this object was built with."""
        groups, gs = sd["param_groups"], self._gs
        extra = sd.get("gfv_groups")
        if len(groups) == 1 and extra is None and sorted(groups[0]["params"]) == list(range(len(names))):
            return None
        pos = {n: i for i, n in enumerate(names)}
        if [list(g["params"]) for g in groups] != [[pos[n] for n in g["names"]] for g in gs.groups]:
            raise ValueError("optimizer state belongs to a different parameter grouping")
        if extra is not None:
            lr, wd, dec = float(extra["lr"]), check_weight_decay(extra["weight_decay"]), bool(extra["decoupled"])
        else:
            # (a torch.optim.AdamW dict: the object's rate is the one its first group's lr_scale leads back to)
            s0 = gs.groups[0]["lr_scale"]
            lr = float(groups[0]["lr"]) / s0 if s0 > 0 else self._lr
            wd, dec = gs.weight_decay, bool(groups[0].get("decoupled_weight_decay", gs.decoupled))
        out = []
        for g, mine in zip(groups, gs.groups):
            scale = g.get("lr_scale")
            if scale is None:
                scale = float(g["lr"]) / lr if lr > 0 else mine["lr_scale"]
            fr = g.get("frozen")
            out.append((float(scale), check_weight_decay(g.get("weight_decay", wd)), None if fr is None else bool(fr)))
        gs.check_some_live([mine["frozen"] if fr is None else fr for (_, _, fr), mine in zip(out, gs.groups)])
        for scale, _, _ in out:
            if not scale >= 0:
                raise ValueError(f"lr_scale must be a finite number >= 0, got {scale!r}")
        return {"lr": lr, "weight_decay": wd, "decoupled": dec, "groups": out}

    def named_state(self):
        """{name: (parameter, exp_avg, exp_avg_sq)} views of the flat buffers.  (The alignment padding between tensors is not
        state: its gradient slots take whatever the shared slab workspace held, see gfv_dw_multi in include/gfv.h.)"""
        return {n: tuple(self.G.view_of(b, n) for b in (self.flat_p, self.flat_m, self.flat_v)) for n in self.G.off}

    def advance_time(self):
        """Time advance of the reference's solve loop (solve_with_grad_GPU.py:180-197): after the inner iterations of a time
        step the predicted node field becomes the next step's input state, the conditioning columns stay -
        `graph_node.x = cat(uvp_node_new.detach(), backup[:, 3:])`.  In place on the persistent backup (captured steps keep
        reading the same tensor)."""
        if self.uvp_node is None:
            raise RuntimeError("advance_time() needs the prediction of a step (want_outputs=True)")
        self.x_backup[:, 0:3].copy_(self.uvp_node)
        self.x.copy_(self.x_backup)
        if self.time_scheme is not None:
            # the scheme's own clock word counts the fields written: bumped in stream order behind the two copies, then the launch
            # that rotates the history and writes the next level's baseline where eager steps, lists and graphs read it
            self.time_scheme.tick()

    def sync_from_model(self):
        """Call after loading a checkpoint into the model: `load_state_dict` copies into the parameter views of the flat
        buffer in place, so the values are already there; this re-checks the aliasing and drops captured steps (their
        weight images belong to the old values' step, the next step rebuilds them anyway)."""
        for n, t in zip(*self.model.param_names_tensors()):
            off = self.G.off[n]
            if t.data_ptr() != self.flat_p.data_ptr() + 4 * off:
                view = self.flat_p[off:off + t.numel()].view(t.shape)
                view.copy_(t.data)
                t.data = view
                self.P[n] = view
        self.model.node_norm._host_num_acc = None

    def set_batch(self, graphs):
        """Switch to another batch (dataset training: a new batch every step, pre_train_Adam.py:146-156).  Captured
        hipGraphs belong to the tensors of one batch and are dropped; with a gfv.pool.DevicePool the switch costs one
        small launch."""
        if self.observations is not None:
            raise ValueError("set_batch() with observations attached: they belong to the nodes of ONE batch (changing batches are "
                             "PoolTrainStep's and gfv.observe.PoolObservations' job)")
        if self.time_scheme is not None:
            raise ValueError("set_batch() with a time scheme attached: its history belongs to the nodes of ONE batch")
        self.graphs = graphs
        self.plan = get_plan(graphs)
        self._live = _live_key(graphs)
        self.x = graphs[0].x
        self.x_backup = self.x.clone()
        if self.gloss.shape[0] != self.plan.B:
            self.gloss = torch.zeros((self.plan.B, 4), dtype=torch.float32, device=self.dev)
        self._drop_recorded()

    # one un-captured step body ------------------------------------------------------------------------------
    def _body(self, accumulate, with_adam=True):
        lib = L.load()
        st = L.stream_ptr()
        if self.padded:
            cmdlist.call(_gather, self.flat_p, self._pad_map, self.flat_pp)
        # solve_with_grad_GPU.py:143: fresh, un-normalised node state every step.  Round 6: no restore copy - the input
        # preparation reads the raw rows from the persistent backup and writes the normalised ones into `x` (Engine.prep_fwd)
        with self.engine.model_width():
            losses, uvp_node, uvp_cell, _, ctx = self.engine.forward(
                self.P_run, self.model.node_norm.buffers_dict(), self.x, self.plan, norm_global=True, accumulate=accumulate,
                want_outputs=self.want_outputs, want_edge_attr15=False, x_raw=self.x_backup,
                train_loss=(self.hyper, self.loss, self.gloss),   # loss + its gradient behind the residual norms, same launch
                time_state=None if self.time_scheme is None else self.time_scheme.time_state)
            obs, hook = self.observations, None
            if obs is not None:
                # the data term (gfv/observe.py): loss and gloss re-formed with it behind the forward, its own gradient added to
                # the decoder-output gradient inside the backward
                fv, pl = ctx["fvm"], self.plan
                obs.fwd(fv["phi"], pl, losses, self.hyper, self.loss, self.gloss)
                hook = lambda g_dec: obs.bwd(fv["dec"], fv["phi"], pl, g_dec)
            self.engine.backward(self.P_run, ctx, self.gloss, self.G_run, self.plan, g_dec_hook=hook)
        if self.padded:
            cmdlist.call(_gather, self.G_run.flat, self._unpad_map, self.flat_g)
        self.losses, self.uvp_node, self.uvp_cell = losses, uvp_node, uvp_cell
        self._after_backward()
        if with_adam:
            self._adam()

    def _after_backward(self):
        """Launches of a subclass between the backward and the optimiser's (gfv.march.MarchStep: the march launch): part of the
        step body, so eager steps, recorded lists and captures carry them alike.  Nothing here."""

    def _hold_record(self):
        """A device record whose word [3] a launch of `_after_backward` wrote as this step's apply flag (`hold=` of gfv/optstep.py),
        or None.  The optimiser and the log read it where they read the accumulation's record: an owner has one or the other."""
        return None

    def _adam(self):
        """The optimiser step's one to three launches (gfv/optstep.py): eager, list and hipGraph mode all go through here."""
        optimizer_launches(self.flat_p, self.flat_g, self.flat_m, self.flat_v, self.n_params, self.adam_state, self.hyper,
                           guard=self._guard, accum=self._accum, ema=self._ema, groups=self._pg, B=self.plan.B, loss=self.loss,
                           hold=self._hold_record())

    # data-parallel exchange: the flat gradient is reduced in two buckets.  The upper one (last processor + decoder:
    # their backward runs first) goes out on a communication stream as soon as its last gradient kernel is launched and
    # overlaps the backward of the first processor and the encoders; the lower one follows the backward.  The fork to the
    # communication stream and the early all-reduce go through cmdlist.call: a RECORDED step replays them at the same
    # point of the backward (round 4: the command list is the default launch mode - the exchange of its first bucket used
    # to be exposed behind the replay).  A hipGraph capture keeps the exchange outside the graph, in one piece.
    def _bucket_split(self):
        if self._split is None:
            names = [n for n in self.G.off if ".processpr_list." in n]
            last = max((int(n.split(".processpr_list.")[1].split(".")[0]) for n in names), default=-1)
            offs = [self.G.off[n] for n in names if f".processpr_list.{last}." in n]
            self._split = min(offs) if (last > 0 and offs) else 0
        return self._split

    def _allreduce_upper(self):
        import torch.distributed as dist
        # (the blocking form: under `torch.cuda.stream(comm)` it is the communication STREAM that waits for the collective and
        # nothing has to be kept alive for a replay.  The overlap with the rest of the backward is an RCCL property: under gloo,
        # or with TORCH_NCCL_BLOCKING_WAIT set, the HOST waits here and the early bucket is merely correct, not overlapped -
        # the gloo tests assert numerics only)
        dist.all_reduce(self.flat_g[self._split:], op=dist.ReduceOp.SUM, group=self.pg)

    def _bucket_ready(self):
        split = self._bucket_split()
        if split <= 0 or torch.cuda.is_current_stream_capturing():
            return
        if self._comm is None:
            self._comm = torch.cuda.Stream()
        L.stream_wait(self._comm, torch.cuda.current_stream())
        for sd in self.engine._sides:
            L.stream_wait(self._comm, sd)        # the weight-gradient kernels run there
        with torch.cuda.stream(self._comm):
            cmdlist.call(self._allreduce_upper)
        self._early = True

    def _allreduce(self, early=None):
        """The rest of the exchange, behind the backward: the lower bucket + the join with the communication stream when the
        upper one went out early (`early`: default = what the step that just ran did), else the whole buffer."""
        import torch.distributed as dist
        early = self._early if early is None else early
        self._early = False
        if early:
            dist.all_reduce(self.flat_g[:self._split], op=dist.ReduceOp.SUM, group=self.pg)
            torch.cuda.current_stream().wait_stream(self._comm)
        else:
            dist.all_reduce(self.flat_g, op=dist.ReduceOp.SUM, group=self.pg)

    def _hooked_body(self, acc, dist_on):
        # (a padded model's true-shape gradient exists only after the gather at the end of the backward: one all-reduce)
        self._early = False
        self.engine.bucket_hook = self._bucket_ready if (dist_on and not self.padded) else None
        try:
            self._body(acc, with_adam=not dist_on)
        finally:
            self.engine.bucket_hook = None
        return self._early

    def _list_stamp(self):
        """What a recorded list points at and does not own, as it is now: kept in the list's entry when it is recorded and compared
        before every replay.  Here the engine's weight-image set and product form."""
        return {"engine_sig": self.engine.capture_signature()}

    def _list_valid(self, ent):
        """Whether everything `_list_stamp` named when the list of `ent` was recorded is still where it was."""
        return ent.engine_sig == self.engine.capture_signature()

    def _issue(self, key, acc, dist_on, listed):
        """The step body on the launch path of `key` (gfv/listcache.py): replayed from its list, eager (not `listed`, or a warm-up:
        the first steps settle the weight-image set and the persistent workspaces), or recorded - the eager launch sequence taken
        down at the C ABI and replayed with one ctypes call per launch: same two streams, same event edges, no per-launch Python
        work.  A list that finds something it points at moved is dropped, and the step is the first of a new warm-up: a stale list
        is never issued.  Under `dist_on` the rest of the exchange and the optimiser follow on every path, outside the list (the
        early bucket's fork + all-reduce are inside).  -> the Entry of a list recorded just now, for the caller to store, or None."""
        ent = self._lists.get(key)
        if ent is not None and not self._list_valid(ent):
            self._lists.invalidate(key)
        what = self._lists.decide(key, listed)
        new = None
        if what == "replay":
            ent.cl.replay()
            self.losses, self.uvp_node, self.uvp_cell = ent.outs      # (the recorded step's own tensors: every replay rewrites them)
            early = ent.early
        elif what == "eager":
            early = self._hooked_body(acc, dist_on)
        else:
            before = torch.cuda.memory_reserved(self.dev)
            with cmdlist.record() as cl:
                early = self._hooked_body(acc, dist_on)
            nbytes = max(torch.cuda.memory_reserved(self.dev) - before, 0)   # the segments of the list's private pool
            new = listcache.Entry(cl, nbytes, (self.losses, self.uvp_node, self.uvp_cell), early=early, **self._list_stamp())
        if dist_on:
            self._allreduce(early)
            self._adam()
        return new

    def _log_step(self, entries=None, n_entries=0):
        """The training log's two launches (gfv/trainlog.py), eagerly on the current stream behind the optimiser launches of the
        step - whichever way those were issued: eager, replayed from a list, replayed from a hipGraph, or behind the all-reduce.
        Never recorded: `losses` differs per recorded list and the pool entries per step (the rule of Evaluate's collect
        launch).  Under data parallelism the log is rank-local: this rank's loss and terms, the REDUCED gradient."""
        if self.log is None:
            return
        self.log.append(self.flat_g, self.flat_p, self.adam_state, self.hyper, self.loss, self.losses, self.plan.B,
                        guard=self._guard.guard if self._guard.active else None,
                        accum=self._hold_record() if self._accum is None else self._accum.rec, entries=entries,
                        n_entries=n_entries)

    def _balance_step(self):
        """The balancer's launch (gfv/balance.py), eagerly on the current stream behind the optimiser launches of the step and
        behind the log's (a row shows the weights its step used) - whichever way the step was issued: `_log_step`'s rule.  It
        observes this step's terms and may write hyper[5:8] for the NEXT step.  Under accumulation the record's apply word is its
        hold word: every micro-step is observed, the weights move only behind an applied step.  A step the guard skipped is
        observed too (an observation is about losses, not gradients); non-finite terms reject themselves."""
        if self.balance is None:
            return
        self.balance.observe(self.losses, self.plan.B, self.hyper, None if self._accum is None else self._accum.rec_i[3:4])

    def _check_aliasing(self):
        """The module's parameters must still be the views of the flat buffer this object made them (a `model.to()`, a
        `load_state_dict(assign=True)` or a second TrainStep on the same model re-points them): captured steps hold raw
        pointers, and a replay does not run the host code that would notice.  Three probes per step; on a mismatch the
        views are re-established from the module's current values and every capture is dropped."""
        for n, t in self._probes:
            if t.data_ptr() != self.flat_p.data_ptr() + 4 * self.G.off[n]:
                self.sync_from_model()
                self._drop_recorded()
                return

    def _step_head(self, who):
        """What every step does first.  who: the name the status error carries."""
        self._not_swapped("step()")
        self._check_aliasing()
        # what the kernels of the steps BEFORE the last one raised in the device status word (a hidden activation outside the
        # fixed-scale fp16 window, a weight-gradient operand beyond fp16): read from the pinned mirror the fused Adam publishes
        # into - no synchronisation; the step that overflowed has long finished when its successor is issued
        L.raise_on_status(who)
        # caller-owned data the plan holds copies of (Dirichlet targets, node / face types, theta_PDE, sigma, uvp_dim, dt_graph):
        # an in-place edit between two steps reaches the plan's tensors here - copied in place, so the pointers a captured step
        # holds stay valid (the reference re-reads graph_node.y / graph_Index on every forward, importer.py:141-154,168).
        # Batches of a DevicePool carry their plan with them: nothing to refresh.
        live = _live_key(self.graphs)
        if live != self._live:
            _refresh_live(self.plan, self.graphs)
            self._live = live

    def _step_tail(self, acc, entries=None, n_entries=0):
        """What every step does last, behind the optimiser's launches however they were issued -> the (device) loss."""
        if acc:
            self.model.node_norm.note_accumulated()
        if self._accum is not None:
            self._accum.note_step()
        self._log_step(entries, n_entries)
        self._balance_step()
        return self.loss

    def _listed(self, acc):
        """Whether this step goes through its recorded list.  (An accumulating data-parallel step exchanges the Normalizer
        statistics inside the forward: neither recorded nor captured.)"""
        return self.use_graph == "list" and not (acc and self.dist_on)

    def step(self):
        """One training iteration.  Returns the (device) scalar loss tensor of this rank's batch.
        `use_graph`: False = eager launches, True = hipGraph replay, "list" = command-list replay.
        With `log=...` the step also appends one row to `self.log` (gfv/trainlog.py): read it with `ts.log.read()` when
        convenient - nothing in step() waits for the device.  Under data parallelism the log is rank-local (this rank's loss,
        the reduced gradient)."""
        self._step_head("TrainStep.step")
        acc = self.model.node_norm.should_accumulate()
        dist_on = self.dist_on
        key = (acc, dist_on)
        if self.use_graph and self.use_graph != "list" and not (acc and dist_on):
            self._capture_step(key, acc, dist_on)
        else:
            ent = self._issue(key, acc, dist_on, self._listed(acc))
            if ent is not None:
                self._lists.store(key, ent)
        return self._step_tail(acc)

    def _capture_step(self, key, acc, dist_on):
        """The step as a hipGraph replay; captured on the first visit of `key` and after the engine's signature moved."""
        g = self._captures.get(key)
        if g is not None and g[1] != self.engine.capture_signature():
            # the captured launches hold raw pointers into the weight-image set / descriptor tables of the engine:
            # a changed set (model.to(), re-flattened parameters, a new weight block) makes every capture stale
            self._drop_recorded()   # (command lists too: they re-record only after new warm-up steps)
            g = None
        if g is None:
            # warm the allocator on a side stream, then capture (PyTorch CUDA-graph recipe)
            s = torch.cuda.Stream()
            s.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(s):
                self._snapshot()
                # twice: the first pass notes the weight blocks of the chain launches, the second allocates and
                # builds their split-fp16 images - the capture then records the launch sequence of a steady step
                for _ in range(2 if self.engine.f16split else 1):
                    self._body(acc, with_adam=not dist_on)
                    self._restore()
            torch.cuda.current_stream().wait_stream(s)
            torch.cuda.synchronize()
            g = torch.cuda.CUDAGraph()
            # (thread_local: the RCCL watchdog thread of a process group polls events while this thread captures; under
            # the default global mode that poll invalidates the capture and aborts the process)
            with torch.cuda.graph(g, capture_error_mode="thread_local"):
                self._body(acc, with_adam=not dist_on)
            g = (g, self.engine.capture_signature())
            self._captures[key] = g
            self._restore()  # capture does not execute; state is as before this step
        g[0].replay()
        if dist_on:
            self._allreduce()
            self._adam()

    # state snapshot so the capture warm-up does not advance training ---------------------------------------
    def _state_tensors(self):
        nb = self.model.node_norm
        return ((self.flat_p, self.flat_m, self.flat_v, self.adam_state, self._guard.guard, nb.acc_count, nb.num_accumulations,
                 nb.acc_sum, nb.acc_sum_squared)
                + (() if self._accum is None else (self._accum.acc, self._accum.rec))
                + (() if self._ema is None else (self._ema.e, self._ema.rec)))

    def _snapshot(self):
        self._capture_state = tuple(t.clone() for t in self._state_tensors())

    def _restore(self):
        for dst, src in zip(self._state_tensors(), self._capture_state):
            dst.copy_(src)
