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
(DESIGN.md 5c).  Lists are kept per (signature, accumulate, distributed): the third step of a key records (two eager warm-up
steps first, as `TrainStep` does), later ones replay; the cache is bounded by the bytes of the lists' private memory pools,
least recently used out (a key evicted EVICT_MAX times stays eager: it would otherwise record on every visit).  The recorded list contains only the step; assembly and payback are issued around the replay.

Gradient accumulation (`accum_steps=k`, gfv/accum.py): k consecutive `step()` calls are one optimiser step over the
mean gradient of all their graphs.  The key of a list is unchanged: the launches behind the backward are the same on every
micro-step and read their phase from a device record, so the list of a signature is replayed in every phase.  With micro-batches
of one or two meshes a pool of N sizes has N or N^2 ordered signatures instead of N^8, and every list is small.

Who owns what a recorded list points at.  (1) The list's own private memory pool: activations and outputs.  (2) The arena: every
plan tensor, the normalised `x` and the un-normalised state the input preparation reads (`x_raw=`).  (3) The flat parameter /
gradient / moment buffers, `loss`, the per-B `gloss`, the Adam state: this object, for its lifetime.  (4) The engine's
weight-image set (checked through `Engine.capture_signature()`).  (5) Engine scratch - `_zero_e`, `_dw_ws`, `_dw_ws_main`,
`_prep_ws`, `_fvm_cnt` - owned by THIS object and swapped into the engine for the duration of a step (as `Rollout._own_scratch`
does), so that another batch run through the same engine by someone else cannot replace it under a list.  `_prep_ws`,
`_fvm_cnt` and `_zero_e` (one capacity-sized buffer viewed to E rows) are sized once for the arena's capacity and must not be
re-allocated inside a step (asserted).  The two weight-gradient workspaces follow the engine's own grow-only rule - they are
allocated and, for a batch larger than any before, re-allocated INSIDE a step by the engine, on exactly the steps where a plain
`TrainStep` over the same batches would do it (the padding slots of the flat gradient take whatever that workspace held, so its
history is part of the bit-identity with the eager path) - and when that happens the new tensor is adopted and EVERY list is
dropped (the old tensor dies with them; the keys keep their warm-up counts and record again on their next visit).  Before a replay the engine signature and the pointers of all five pieces are compared with what the list was recorded
against; on any mismatch the list is dropped and the step runs eager.  A stale list is never issued.
"""
from __future__ import annotations

import collections
import contextlib

import torch

from . import cmdlist
from . import lib as L
from .accum import check_accum_steps
from .ema import check_ema
from .groups import check_groups
from .guard import check_policy
from .trainer import TrainStep

_SCRATCH = ("_zero_e", "_dw_ws", "_dw_ws_main", "_prep_ws", "_fvm_cnt")
_FIXED = ("_zero_e", "_prep_ws", "_fvm_cnt")       # sized once for the arena's capacity


class _Recorded:
    __slots__ = ("cl", "engine_sig", "early", "scratch", "bytes", "outs")

    def __init__(self, cl, engine_sig, early, scratch, nbytes, outs):
        self.cl, self.engine_sig, self.early, self.scratch, self.bytes, self.outs = cl, engine_sig, early, scratch, nbytes, outs


class PoolTrainStep(TrainStep):
    WARM = 2   # eager steps of a key before its list is recorded (they are training steps like any other)
    EVICT_MAX = 2

    def __init__(self, model, pool, max_graphs=8, *, max_sizes=None, lr=None, betas=(0.9, 0.999), eps=1e-8, loss_weights=None,
                 use_graph="list", max_list_bytes=16 << 30, want_outputs=True, distributed=None, max_grad_norm=None,
                 skip_nonfinite=False, skip_on_flag=False, accum_steps=1, ema_decay=None, ema_warmup=True, weight_decay=0.0,
                 decoupled_weight_decay=True, param_groups=None):
        if use_graph not in (False, "list"):
            raise ValueError('PoolTrainStep: use_graph must be False or "list" (the hipGraph mode is bound to one batch)')
        check_policy(max_grad_norm, skip_on_flag, bool(distributed))
        check_accum_steps(accum_steps, bool(distributed))
        check_ema(ema_decay, ema_warmup)
        check_groups(*model.param_names_tensors(), weight_decay, decoupled_weight_decay, param_groups)
        self.pool = pool
        self.arena = pool.arena(max_graphs, max_sizes)
        self.max_list_bytes = int(max_list_bytes)
        graphs, _ = self.arena.load([0])
        super().__init__(model, graphs, lr=lr, betas=betas, eps=eps, loss_weights=loss_weights, world_size=1, use_graph=use_graph,
                         want_outputs=want_outputs, distributed=distributed, max_grad_norm=max_grad_norm,
                         skip_nonfinite=skip_nonfinite, skip_on_flag=skip_on_flag, accum_steps=accum_steps,
                         ema_decay=ema_decay, ema_warmup=ema_warmup, weight_decay=weight_decay,
                         decoupled_weight_decay=decoupled_weight_decay, param_groups=param_groups)
        self.x_backup = graphs[0]._gfv_x_raw                      # the arena's raw state, not a per-batch clone
        self._gloss = {self.plan.B: self.gloss}                     # one per batch size, kept: recorded lists point at them
        self._graphs = collections.OrderedDict()                    # key -> _Recorded, least recently used first
        self._list_warm = {}
        self._oversize = set()                                      # keys the byte budget has no room for: eager for good
        self._evicted = {}
        self._counts = dict(replayed=0, recorded=0, eager=0)
        dev, cap = self.dev, self.arena.capacity
        lib = L.load()
        self._zero_e_cap = torch.zeros((max(cap["e"], 1), 128), dtype=torch.float32, device=dev)
        self._zero_views = {}
        self._scratch = dict(
            _zero_e=None, _dw_ws=None, _dw_ws_main=None,
            _prep_ws=torch.zeros(max(lib.gfv_prep_workspace_bytes(self.arena.max_graphs) // 4, 1), dtype=torch.float32, device=dev),
            _fvm_cnt=torch.zeros(4, dtype=torch.int32, device=dev))

    # ---- bookkeeping ---------------------------------------------------------------------------------------------------
    def stats(self):
        return dict(self._counts, lists=len(self._graphs), list_bytes=sum(e.bytes for e in self._graphs.values()))

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
                self._graphs.clear()

    def _valid(self, ent):
        return ent.engine_sig == self.engine.capture_signature() and ent.scratch == self._scratch_ptrs()

    # ---- one step ------------------------------------------------------------------------------------------------------
    def step(self, indices, payback=False, advance=False):
        """One training iteration over the pool entries `indices` -> the (device) scalar loss tensor.
        payback: write the predicted (u, v, p) back into the entries' own `x` (one launch); advance: also into the arena's raw
        state, so that the next inner step over the SAME batch starts from it (`TrainStep.advance_time`)."""
        self._not_swapped("step()")
        self._check_aliasing()
        L.raise_on_status("PoolTrainStep.step")
        idx = [int(i) for i in indices]
        graphs, plan = self.arena.load(idx)
        sig = self.arena._last[1]
        self.graphs, self.plan = graphs, plan
        self.x, self.x_backup = graphs[0].x, graphs[0]._gfv_x_raw
        gl = self._gloss.get(plan.B)
        if gl is None:
            gl = self._gloss[plan.B] = torch.zeros((plan.B, 4), dtype=torch.float32, device=self.dev)
        self.gloss = gl
        acc = self.model.node_norm.should_accumulate()
        dist_on = self.dist_on
        key = (sig, acc, dist_on)
        listed = self.use_graph == "list" and self.max_list_bytes > 0 and not (acc and dist_on) and key not in self._oversize
        recorded = None
        with self._own_scratch(plan.E) as grown:
            ent = self._graphs.get(key) if listed else None
            if ent is not None and not self._valid(ent):
                # something a recorded launch points at moved (weight-image set, product form, a piece of scratch): the list is
                # dropped and this step runs eager - a stale list is never issued
                del self._graphs[key]
                self._list_warm[key] = 0            # (this eager step is the first of the key's new warm-up)
                ent = None
            if ent is not None:
                self._graphs.move_to_end(key)
                ent.cl.replay()
                self.losses, self.uvp_node, self.uvp_cell = ent.outs
                if dist_on:
                    self._allreduce(ent.early)
                    self._adam()
                self._counts["replayed"] += 1
            elif not listed or self._list_warm.get(key, 0) < PoolTrainStep.WARM:
                if listed:
                    self._list_warm[key] = self._list_warm.get(key, 0) + 1
                self._eager(acc, dist_on)
                self._counts["eager"] += 1
            else:
                before = torch.cuda.memory_reserved(self.dev)
                with cmdlist.record() as cl:
                    early = self._hooked_body(acc, dist_on)
                nbytes = max(torch.cuda.memory_reserved(self.dev) - before, 0)   # the segments of the list's private pool
                if dist_on:
                    self._allreduce(early)
                    self._adam()
                self._counts["recorded"] += 1
                recorded = (cl, early, nbytes)
        if recorded is not None and not grown[0]:    # (a workspace that moved while the list was recorded: the list is not kept)
            cl, early, nbytes = recorded
            if nbytes > self.max_list_bytes:
                self._oversize.add(key)
            else:
                self._graphs[key] = _Recorded(cl, self.engine.capture_signature(), early, self._scratch_ptrs(), nbytes,
                                              (self.losses, self.uvp_node, self.uvp_cell))
                while sum(e.bytes for e in self._graphs.values()) > self.max_list_bytes and len(self._graphs) > 1:
                    old, _ = self._graphs.popitem(last=False)
                    # a key that keeps losing its list to the byte budget would record on every visit (a recording allocates a
                    # whole step's activations afresh): after EVICT_MAX evictions it stays eager
                    self._evicted[old] = self._evicted.get(old, 0) + 1
                    if self._evicted[old] >= PoolTrainStep.EVICT_MAX:
                        self._oversize.add(old)
        if acc:
            self.model.node_norm.note_accumulated()
        if self._accum is not None:
            self._accum.note_step()
        if payback or advance:
            if self.uvp_node is None:
                raise RuntimeError("payback needs the prediction of the step (want_outputs=True)")
            self.arena.payback(idx, self.uvp_node.contiguous(), advance=advance)
        return self.loss
