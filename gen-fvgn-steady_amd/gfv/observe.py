"""Observation term: train on measured fields beside the PDE residual (include/gfv.h gfv_obs_*, csrc/obs.hip).

`gfv.evaluate.Evaluate.set_target` scores a model against a measured or CFD field; this module fits it.  With observations
attached the training objective is

    mean_b log(w_press * press_b + w_cont * cont_b + w_mom * (mom_x_b + mom_y_b) + weight * obs_b)
    obs_b = sum_ic w_ic * (pred_ic - t_ic)^2 / sum_ic w_ic          over the nodes i of graph b and the channels c = u, v, p

    obs = Observations(values, weights, weight=10.0)            # [N, 3] fp32 device tensors of ONE fixed batch
    ts = TrainStep(model, graphs, observations=obs)             # eager, "list" and hipGraph modes alike
    obs.weight = 3.0; obs.set_values(v)                         # reach recorded lists and captured graphs as they are
    obs.read()                                                  # [B, 4]: obs_b, W_b, gobs_b, tot_b of the last step (synchronises)

    pobs = PoolObservations(pool, weight=10.0)                  # a new batch every step
    pobs.set(i, values_i, weights_i); pobs.clear(j)             # per pool entry, exactly pool.sizes[i]["n"] rows
    ts = PoolTrainStep(model, pool, observations=pobs)

**What is fitted** is the network's OWN nodal prediction `BC(10 tanh(dec / 10))` - channels 0..2 of `phi`, what the finite-volume
section differentiates - re-dimensionalised like the returned field (`(phi * uvp_dim) * sigma`): the values are in the units of
`uvp_node`, the units `Evaluate.set_target` takes.  It is NOT the smoothed `uvp_node` the step returns (that passes through the
cell-to-node interpolation; fitting it would need that interpolation's adjoint).  At Dirichlet nodes the prediction is the boundary
value: such elements count in `obs_b` and pass no gradient.

`weights` >= 0 per node and channel; 0 means "not observed": such an element's value is never read into any arithmetic and may be
anything, NaN included.  A graph without any observed element has `obs_b = 0`.

Two launches per step, both part of the step body (eager steps, recorded lists and captured graphs carry them alike):
`gfv_obs_fwd` behind the forward - it OVERWRITES the step's `loss` and `gloss` with the extended objective's - and `gfv_obs_bwd`
between the finite-volume adjoint and the decoder's backward (`Engine.backward(g_dec_hook=)`).  `ts.losses` stays the four PDE
residuals.  The pool path issues one more, `gfv_obs_gather`, eagerly in front of the step: it fills the batch-sized buffers from the
entries' tensors and is never part of a recorded list (the rule of `gfv_eval_collect`).

Ownership: the value / weight buffers, the record, the weight word, the reduction workspace and its counter belong
to the observations object, are created once (for the batch; for the arena's capacity) and never reallocated - recorded lists point
at them.  Observations are data, not state: they are not in `state_dict()`.  Host-only checks need no GPU (`check_observations`,
`check_observe`).  The term is rank-local like the loss, so data parallelism needs nothing new - no test exercises it.  Not with
`MarchStep` (its convergence rule is on the PDE residual alone) and not with `balance=` (its shares are of the PDE residual)."""
from __future__ import annotations

import ctypes as C
import math
import numbers

import torch

from . import lib as L


def check_weight(weight):
    """The term's weight: a finite number >= 0 -> float."""
    if isinstance(weight, bool) or not isinstance(weight, numbers.Real):
        raise ValueError(f"observations: weight must be a number, got {weight!r}")
    w = float(weight)
    if math.isnan(w) or math.isinf(w) or w < 0.0:
        raise ValueError(f"observations: weight must be finite and >= 0, got {weight!r}")
    return w


def _check_field(name, t, n=None):
    if not isinstance(t, torch.Tensor):
        raise ValueError(f"observations: {name} must be a torch tensor, got {type(t).__name__}")
    if t.dtype != torch.float32:
        raise ValueError(f"observations: {name} must be float32, got {t.dtype}")
    if t.dim() != 2 or t.shape[1] != 3:
        raise ValueError(f"observations: {name} must be [N, 3] (u, v, p per node), got {list(t.shape)}")
    if n is not None and t.shape[0] != int(n):
        raise ValueError(f"observations: {name} must have {int(n)} rows (one per node), got {t.shape[0]}")


def _check_weights(weights):
    if weights.numel() and not bool((torch.isfinite(weights) & (weights >= 0)).all()):
        raise ValueError("observations: every weight must be finite and >= 0 (0 = not observed)")


def check_observations(values, weights, weight=1.0, n=None):
    """Host-only checks of an observed field; needs no GPU.  values, weights: [N, 3] float32 tensors (N == n when given); every
    weight finite and >= 0 (values under a zero weight may be anything); weight: a finite number >= 0.  -> float(weight)"""
    _check_field("values", values, n)
    _check_field("weights", weights, n)
    if values.shape != weights.shape:
        raise ValueError(f"observations: values {list(values.shape)} and weights {list(weights.shape)} differ in shape")
    if values.device != weights.device:
        raise ValueError("observations: values and weights live on different devices")
    _check_weights(weights)
    return check_weight(weight)


def check_observe(observations, balance=None, what="TrainStep", kind=None):
    """The constructor check of the step objects' `observations=`; needs no GPU."""
    if observations is None:
        return
    kind = ObservationTerm if kind is None else kind
    if not isinstance(observations, kind):
        raise TypeError(f"{what}: observations must be a gfv.observe.{kind.__name__}, got {observations!r}")
    if balance is not None:
        raise ValueError(f"{what}: balance= together with observations= is not supported (the balancer's shares are of the PDE "
                         "residual; it knows nothing of the data term)")
    if observations._owner is not None:
        raise ValueError("these observations are already attached to a step object (its recorded lists point at their buffers)")


class ObservationTerm:
    """What the two kinds share: the device buffers, the weight word, the two launches of the step body."""

    def __init__(self, weight):
        self._weight = check_weight(weight)
        self._owner = None
        self.values = self.weights = None      # [rows, 3] fp32: what the launches read
        self.rec = None                        # [graphs, GFV_OBS_RECORD] fp32
        self._w = self._partial = self._counter = None
        self._B = 0

    def _alloc(self, dev, rows, graphs, chunks):
        """Created once, never reallocated: recorded lists and captured graphs point at all of it."""
        self.rec = torch.zeros((graphs, L.OBS_RECORD), dtype=torch.float32, device=dev)
        self._partial = torch.zeros((max(chunks, 1), 2), dtype=torch.float64, device=dev)
        self._counter = torch.zeros(4, dtype=torch.int32, device=dev)       # (arrival counter: zero between launches)
        self._w = torch.full((4,), self._weight, dtype=torch.float32, device=dev)
        if self.values is None:
            self.values = torch.zeros((max(rows, 1), 3), dtype=torch.float32, device=dev)
            self.weights = torch.zeros((max(rows, 1), 3), dtype=torch.float32, device=dev)

    # ---- the weight of the term: a device word ----------------------------------------------------------------------------------
    @property
    def weight(self):
        return self._weight

    @weight.setter
    def weight(self, v):
        self._weight = check_weight(v)
        if self._w is not None:
            self._w.fill_(self._weight)       # (in stream order; recorded lists and graphs read the word)

    # ---- the two launches of the step body ----------------------------------------------------------------------------------------
    def fwd(self, phi, pl, losses, hyper, loss, gloss):
        """gfv_obs_fwd behind the forward: the record of the batch, `loss` and `gloss` overwritten."""
        L.check(L.load().gfv_obs_fwd(phi.data_ptr(), self.values.data_ptr(), self.weights.data_ptr(), pl.N, pl.chunk_beg.data_ptr(),
                                     pl.chunk_end.data_ptr(), pl.gchunk_ptr.data_ptr(), pl.n_chunks, pl.B, pl.uvp_dim.data_ptr(),
                                     pl.sigma.data_ptr(), losses.data_ptr(), hyper.data_ptr(), self._w.data_ptr(),
                                     self._partial.data_ptr(), self._counter.data_ptr(), self.rec.data_ptr(), loss.data_ptr(),
                                     gloss.data_ptr(), L.stream_ptr()), "gfv_obs_fwd")

    def bwd(self, dec, phi, pl, g_dec):
        """gfv_obs_bwd: the term's gradient added into the decoder-output gradient."""
        L.check(L.load().gfv_obs_bwd(self.rec.data_ptr(), dec.data_ptr(), phi.data_ptr(), self.values.data_ptr(),
                                     self.weights.data_ptr(), pl.batch.data_ptr(), pl.node_type.data_ptr(), pl.uvp_dim.data_ptr(),
                                     pl.sigma.data_ptr(), pl.N, pl.B, g_dec.data_ptr(), L.stream_ptr()), "gfv_obs_bwd")

    def read(self):
        """The last step's record as a CPU tensor [B, 4]: obs_b, W_b, gobs_b = d loss / d obs_b, tot_b.  Synchronises."""
        if self.rec is None or not self._B:
            raise RuntimeError("observations: not attached to a step object yet (or no batch loaded): there is no record")
        return self.rec[:self._B].cpu()       # (_B: the graphs of the batch, noted on the host - a replayed step runs no host code)


def _need_gpu(*tensors):
    for t in tensors:
        if not t.is_cuda:
            raise RuntimeError("observations: tensors must live on the GPU (HIP kernels only, no CPU fallback)")


class Observations(ObservationTerm):
    """Measured values of ONE fixed batch: `values`, `weights` [N, 3] fp32 on the device, N the batch's node count; `weight` the
    term's weight inside the logarithm.  Both tensors are cloned into buffers this object owns for its lifetime."""

    def __init__(self, values, weights, weight=1.0):
        super().__init__(check_observations(values, weights, weight))
        _need_gpu(values, weights)
        self.values = values.detach().contiguous().clone()
        self.weights = weights.detach().contiguous().clone()

    def _attach(self, owner):
        pl = owner.plan
        if self.values.shape[0] != pl.N:
            raise ValueError(f"observations: the batch has {pl.N} nodes, the observed field {self.values.shape[0]} rows")
        if self.values.device != owner.dev:
            raise ValueError("observations: the observed field lives on another device than the batch")
        if not 1 <= pl.B <= L.POOL_MAX_GRAPHS:
            raise ValueError(f"observations: a batch of {pl.B} graphs (at most {L.POOL_MAX_GRAPHS})")
        self._alloc(owner.dev, pl.N, pl.B, pl.n_chunks)
        self._owner, self._B = owner, pl.B

    def set_values(self, values):
        """New measured values, copied in place (stream order): recorded lists and captured graphs follow."""
        _check_field("values", values, self.values.shape[0])
        _need_gpu(values)
        self.values.copy_(values)

    def set_weights(self, weights):
        """New per-element weights, copied in place."""
        _check_field("weights", weights, self.weights.shape[0])
        _check_weights(weights)
        _need_gpu(weights)
        self.weights.copy_(weights)


class PoolObservations(ObservationTerm):
    """Measured values per entry of a `gfv.pool.DevicePool`, for `PoolTrainStep(..., observations=)`.  Entries without
    observations take part with zero weights.  Bound to the step's arena: staging buffers of the arena's node capacity and a record
    of `max_graphs` rows, filled per batch by one eager launch in front of the step."""

    def __init__(self, pool, weight=1.0):
        super().__init__(weight)
        self.pool = pool
        self._entries = {}          # entry -> (values, weights) [n_i, 3] fp32 on the pool's device

    def set(self, i, values, weights):
        """The observed field of entry `i`: tensors of exactly pool.sizes[i]["n"] rows, cloned."""
        i = int(i)
        if not 0 <= i < self.pool.n:
            raise ValueError(f"observations: pool entry {i} does not exist (the pool holds {self.pool.n})")
        check_observations(values, weights, self._weight, n=int(self.pool.sizes[i]["n"]))
        _need_gpu(values, weights)
        self._entries[i] = (values.detach().contiguous().clone(), weights.detach().contiguous().clone())

    def clear(self, i=None):
        """Entry `i` (None: every entry) is no longer observed."""
        if i is None:
            self._entries = {}
        else:
            self._entries.pop(int(i), None)

    def _attach(self, owner):
        if getattr(owner, "pool", None) is not self.pool:
            raise ValueError("observations: these PoolObservations were built on another pool than the step trains on")
        cap, B = owner.arena.capacity, owner.arena.max_graphs
        self._alloc(owner.dev, cap["n"], B, cap["nchunk"])
        self._owner = owner

    def gather(self, batch, pl):
        """gfv_obs_gather: the batch's values and weights into the staging buffers, in the order of `batch`.  Eager, on the
        current stream, in front of the step - the entries' addresses travel in the launch's argument block."""
        B = len(batch)
        vals, wts, rows = (C.c_void_p * B)(), (C.c_void_p * B)(), (C.c_int32 * B)()
        for b, i in enumerate(batch):
            rows[b] = int(self.pool.sizes[i]["n"])
            ent = self._entries.get(i)
            if ent is not None:
                vals[b], wts[b] = ent[0].data_ptr(), ent[1].data_ptr()
        assert sum(rows) == pl.N
        self._B = B
        L.check(L.load().gfv_obs_gather(C.addressof(vals), C.addressof(wts), C.addressof(rows), B, self.values.data_ptr(),
                                        self.weights.data_ptr(), self.values.shape[0], L.stream_ptr()), "gfv_obs_gather")
