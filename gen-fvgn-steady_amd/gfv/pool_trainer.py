"""Pool training: a different batch of the device-resident pool every step, on the recorded launch path.

The reference's training loop (pre_train_Adam.py:112-198) sends a DIFFERENT batch of its dataset pool through forward, loss,
backward and Adam at every inner step and writes the prediction back into the pool on the last one (`Data_Pool.payback`,
Graph_loader.py:370-396).  `TrainStep` is bound to one batch: `set_batch` drops its recorded list, so with a new batch per step
nothing is ever replayed.  `PoolTrainStep` is that loop with replay:

    ts = PoolTrainStep(model, pool, max_graphs=8, lr=1e-3)          # use_graph="list"
    loss = ts.step(indices)                  # assemble + forward + loss + backward + Adam for THIS batch
    loss = ts.step(indices, payback=True)    # ... and the prediction goes back into the pool entries
    ts.stats()                               # {"replayed", "recorded", "eager", "lists", "list_bytes"}

Why a list recorded for one batch is valid for another.  A recorded list holds pointers, sizes and grids, nothing else.  Every
batch is assembled into the SAME memory (`gfv.pool.BatchArena`, one launch of gfv_pool_assemble), so every batch with the same
ordered size signature (per mesh: nodes, faces, cells, incidences, stencil entries, slice chunks) issues exactly the launches
that were recorded - no host-side decision of `Engine.forward / backward` reads table CONTENTS, only sizes, limits and flags
(DESIGN.md 5c).  Lists are kept per (signature, accumulate, distributed) in a `gfv.listcache.ListCache` bounded by
`max_list_bytes`.  The recorded list contains only the step; assembly and payback are issued around the replay.

Gradient accumulation (`accum_steps=k`, gfv/accum.py): k consecutive `step()` calls are one optimiser step over the
mean gradient of all their graphs.  The key of a list is unchanged: the launches behind the backward are the same on every
micro-step and read their phase from a device record, so the list of a signature is replayed in every phase.  With micro-batches
of one or two meshes a pool of N sizes has N or N^2 ordered signatures instead of N^8, and every list is small.

Observations (`observations=gfv.observe.PoolObservations(pool)`): measured fields per pool entry enter the objective
as a data term.  One launch behind `arena.load` and in front of the replay gathers the batch's entries into the observations'
staging buffers (eager in every mode, never recorded); the two launches of the term are part of the recorded body and read those
buffers, so the key of a list is unchanged.

Who owns what a recorded list points at: DESIGN.md 5l.  Particular to this object, for its lifetime: the flat parameter /
gradient / moment buffers, `loss`, the per-B `gloss`, the Adam state.  The weight-image set is checked through
`Engine.capture_signature()`.  The engine scratch of a training step - `_zero_e`, `_dw_ws`, `_dw_ws_main`, `_prep_ws`,
`_fvm_cnt` - is owned by THIS object and swapped into the engine for the duration of a step.  `_prep_ws`, `_fvm_cnt` and `_zero_e` (one capacity-sized buffer viewed to E rows) are sized once for the arena's capacity and must not be
re-allocated inside a step (asserted).  The two weight-gradient workspaces follow the engine's own grow-only rule - they are
allocated and, for a batch larger than any before, re-allocated INSIDE a step by the engine, on exactly the steps where a plain
`TrainStep` over the same batches would do it (the padding slots of the flat gradient take whatever that workspace held, so its
history is part of the bit-identity with the eager path) - and when that happens the new tensor is adopted and EVERY list is
dropped (the old tensor dies with them; the keys keep their warm-up counts and record again on their next visit).  Before a
replay the engine signature and the pointers of all five pieces (`_list_stamp`) are compared with what the list was recorded
against; on any mismatch the list is dropped and the step runs eager.  A stale list is never issued.

The step itself is `TrainStep`'s (gfv/trainer.py: `_step_head`, `_issue`, `_step_tail`); what is the pool's lies between them:
the load, the per-B `gloss`, the observations' gather, the scratch swap around `_issue`, and the payback.
"""
from __future__ import annotations

import contextlib

import torch

from . import listcache
from .observe import PoolObservations
from .static_forward import prep_scratch
from .trainer import TrainStep, check_train_args
from .trainlog import make_log

_SCRATCH = ("_zero_e", "_dw_ws", "_dw_ws_main", "_prep_ws", "_fvm_cnt")
_FIXED = ("_zero_e", "_prep_ws", "_fvm_cnt")       # sized once for the arena's capacity


class PoolTrainStep(TrainStep):
    WARM, EVICT_MAX = listcache.WARM, listcache.EVICT_MAX
    _OBS_KIND = PoolObservations

    def __init__(self, model, pool, max_graphs=8, *, max_sizes=None, lr=None, betas=(0.9, 0.999), eps=1e-8, loss_weights=None,
                 use_graph="list", max_list_bytes=16 << 30, want_outputs=True, distributed=None, max_grad_norm=None,
                 skip_nonfinite=False, skip_on_flag=False, accum_steps=1, ema_decay=None, ema_warmup=True, weight_decay=0.0,
                 decoupled_weight_decay=True, param_groups=None, log=None, schedule=None, balance=None, observations=None,
                 time_scheme=None):
        if use_graph not in (False, "list"):
            raise ValueError('PoolTrainStep: use_graph must be False or "list" (the hipGraph mode is bound to one batch)')
        if time_scheme is not None:
            raise ValueError("PoolTrainStep: time_scheme= is not supported (the pool owns the fields and keeps one level per entry: "
                             "there is no previous level to difference against)")
        step_kw = dict(lr=lr, betas=betas, eps=eps, loss_weights=loss_weights, want_outputs=want_outputs, distributed=distributed,
                       max_grad_norm=max_grad_norm, skip_nonfinite=skip_nonfinite, skip_on_flag=skip_on_flag, accum_steps=accum_steps,
                       ema_decay=ema_decay, ema_warmup=ema_warmup, weight_decay=weight_decay, param_groups=param_groups,
                       decoupled_weight_decay=decoupled_weight_decay, schedule=schedule, balance=balance, observations=observations)
        check_train_args("PoolTrainStep", PoolObservations, model, **step_kw)      # (TrainStep's, before the arena is allocated)
        if observations is not None and observations.pool is not pool:
            raise ValueError("PoolTrainStep: the PoolObservations were built on another pool than the one to train on")
        self.pool = pool
        self.arena = pool.arena(max_graphs, max_sizes)
        self.max_list_bytes = int(max_list_bytes)                   # (TrainStep builds `_lists` with it: key -> Entry with scratch)
        log = make_log(log, self.arena.max_graphs)                  # (before anything is built: its arguments are checked here)
        graphs, _ = self.arena.load([0])
        super().__init__(model, graphs, use_graph=use_graph, log=log, **step_kw)
        self.x_backup = graphs[0]._gfv_x_raw                      # the arena's raw state, not a per-batch clone
        self._gloss = {self.plan.B: self.gloss}                     # one per batch size, kept: recorded lists point at them
        dev, cap = self.dev, self.arena.capacity
        self._zero_e_cap = torch.zeros((max(cap["e"], 1), 128), dtype=torch.float32, device=dev)
        self._zero_views = {}
        prep_ws, fvm_cnt = prep_scratch(self.arena.max_graphs, dev)
        self._scratch = dict(_zero_e=None, _dw_ws=None, _dw_ws_main=None, _prep_ws=prep_ws, _fvm_cnt=fvm_cnt)

    # ---- bookkeeping ---------------------------------------------------------------------------------------------------
    def set_batch(self, graphs):
        raise TypeError("PoolTrainStep takes its batch per step: step(indices)")

    def _scratch_ptrs(self):
        return tuple(None if self._scratch[n] is None else self._scratch[n].data_ptr() for n in _SCRATCH)

    @contextlib.contextmanager
    def _own_scratch(self, E):
        """The engine works on this object's scratch for the duration of a step.  -> a one-element list, set to True when the
        engine re-allocated a weight-gradient workspace inside the step (adopted; every list dropped)."""
        eng = self.engine
        view = self._zero_views.get(E)
        if view is None or view.data_ptr() != self._zero_e_cap.data_ptr():
            view = self._zero_views[E] = self._zero_e_cap[:E]
        self._scratch["_zero_e"] = view
        mine = dict(self._scratch)
        saved = {n: getattr(eng, n) for n in _SCRATCH}
        for n in _SCRATCH:
            setattr(eng, n, mine[n])
        grown = [False]
        try:
            yield grown
        finally:
            for n in _SCRATCH:
                cur = getattr(eng, n)
                if cur is not mine[n]:
                    assert n not in _FIXED, f"engine scratch {n} was reallocated inside a step"
                    self._scratch[n] = cur          # grow-only workspace of the weight gradients: adopt it ...
                    grown[0] = True
                setattr(eng, n, saved[n])
            if grown[0]:
                # ... and no list recorded against the old one survives.  The warm-up counts stay: what a key needs of the
                # workspace depends on its sizes alone, and the new one is at least as large
                self._lists.clear(keep_warm=True)

    def _list_stamp(self):
        return dict(super()._list_stamp(), scratch=self._scratch_ptrs())      # (the engine works on this object's scratch now)

    def _list_valid(self, ent):
        return super()._list_valid(ent) and ent.scratch == self._scratch_ptrs()

    # ---- one step ------------------------------------------------------------------------------------------------------
    def step(self, indices, payback=False, advance=False):
        """One training iteration over the pool entries `indices` -> the (device) scalar loss tensor.
        With `log=...` every call - every micro-step of an accumulation too, `apply` 0 on the hold ones - appends a row carrying
        `indices` to `self.log` and updates its per-entry table; under data parallelism the log is rank-local (this rank's
        loss and entries, the reduced gradient).
        payback: write the predicted (u, v, p) back into the entries' own `x` (one launch); advance: also into the arena's raw
        state, so that the next inner step over the SAME batch starts from it (`TrainStep.advance_time`)."""
        self._step_head("PoolTrainStep.step")
        idx = [int(i) for i in indices]
        graphs, plan = self.arena.load(idx)
        sig = self.arena._last[1]
        self.graphs, self.plan = graphs, plan
        self.x, self.x_backup = graphs[0].x, graphs[0]._gfv_x_raw
        gl = self._gloss.get(plan.B)
        if gl is None:
            gl = self._gloss[plan.B] = torch.zeros((plan.B, 4), dtype=torch.float32, device=self.dev)
        self.gloss = gl
        if self.observations is not None:
            # the batch's measured values and weights into the observations' staging buffers (gfv/observe.py): eager, in front of
            # the step in every launch mode - the recorded body reads the buffers, never the entries
            self.observations.gather(idx, plan)
        acc = self.model.node_norm.should_accumulate()
        key = (sig, acc, self.dist_on)
        with self._own_scratch(plan.E) as grown:
            ent = self._issue(key, acc, self.dist_on, self._listed(acc))
        if ent is not None and not grown[0]:         # (a workspace that moved while the list was recorded: the list is not kept)
            self._lists.store(key, ent)
        # (the log and the balancer: eager, behind Adam, outside the list - the row carries this step's entries, B differs per batch)
        self._step_tail(acc, idx, self.pool.n)
        if payback or advance:
            if self.uvp_node is None:
                raise RuntimeError("payback needs the prediction of the step (want_outputs=True)")
            self.arena.payback(idx, self.uvp_node.contiguous(), advance=advance)
        return self.loss
