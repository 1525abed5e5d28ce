"""Evaluate: held-out losses and field errors of a model over the entries of a device pool.

The reference has no evaluation loop; what a user who keeps some of the pool's entries (`utils/get_param.py:41`: 100 of them) aside
wants once per epoch is the training objective (`pre_train_Adam.py:177-184`) on those entries, with the iterate or the averaged
weights, without training on them and without moving them.  `Rollout` is bound to one batch, `Sweep` advances every entry to its
own convergence and writes the fields back, `PoolTrainStep.step` trains.  `Evaluate` is the forward-only step over batch after
batch of a `BatchArena` with one launch behind it (`gfv_eval_collect`, csrc/eval.hip) and ONE synchronisation at the end:

    ev  = Evaluate(model, pool, max_graphs=8)
    ev.set_target(i, uvp)               # optional: a field [n_i, 3] entry i's prediction is compared with
    rep = ev.run(held_out)              # rep.losses [n, 4], rep.loss_batch, rep.objective, rep.rel_update, rep.rel_error, ...
    with ts.ema_weights():              # the averaged weights of a TrainStep / PoolTrainStep
        ev.refresh_weights()
        rep = ev.run(held_out)
    ev.refresh_weights()                # (the iterate is back)

The pool is NOT written: no payback, no advance - every entry's `x` is bit for bit what it was.

The objective is formed with this object's own fixed `loss_weights` (the model's constants unless given), also when the training
step carries a balancer (`balance=`, gfv/balance.py) that moves ITS weights from step to step: a held-out objective stays comparable
across epochs.  Pass `loss_weights=ts.loss_weights` to evaluate under the training step's base weights.

Per batch: `arena.load(batch)`; the targets of its entries copied into the staging buffer at the host-known node offsets; the
body - `Sweep._body` without the advance: `StaticForward.forward` and nothing behind it - eager, recorded or replayed; then
`gfv_eval_collect`, which writes a 16-float record per graph into row `entry` of a device table `[n_entries, 16]` (the layout is in
include/gfv.h).  The entry indices and the target flags travel by value in that launch's argument block, so it is issued eagerly
behind the body and is not part of the recorded list: one list serves every batch of a size signature.

Recorded lists are kept per ordered batch signature in a `gfv.listcache.ListCache` bounded by `max_list_bytes`.  Warm-up counts
and lists live across `run()` calls: the second epoch's evaluation replays.  A list the byte budget refuses is parked until the
collect launch behind its body has been issued: its private pool holds the outputs that launch reads.

Who owns what a recorded list points at: DESIGN.md 5l.  The arena may be this object's own or a shared one of the same pool
(`PoolTrainStep.arena`: it is assembled afresh for every batch by whoever uses it).  The table, the partial sums, the arrival
counter and the target staging buffer `[capacity n, 3]` are this object's and are read and written by the collect launch only.

`refresh_weights()` rebuilds the weight images and a narrow model's padded copies IN PLACE (gfv/static_forward.py), on the
calling stream, behind every replay issued before it - so a recorded list stays valid: the lists are dropped only when something
they point at moved (`.to()`, another parameter set through the same engine, another product form).
"""
from __future__ import annotations

import collections
import ctypes as C
import math

import torch

from . import lib as L
from . import listcache
from .functions import require_gpu
from .pool import batch_totals, check_fits
from .static_forward import StaticForward, check_normalizer

EvalReport = collections.namedtuple("EvalReport", "entries losses loss_batch objective rel_update rel_error nonfinite table")


# ---- host-side checks and the report: no GPU -----------------------------------------------------------------------------------
def check_indices(indices, n):
    """-> the indices as a list of ints (None: every entry); ValueError for none at all, a repeat or an entry outside the pool."""
    out = list(range(n)) if indices is None else [int(i) for i in indices]
    if not out:
        raise ValueError("Evaluate: no entries to evaluate (the objective is a mean over them)")
    for i in out:
        if not 0 <= i < n:
            raise ValueError(f"Evaluate: pool entry {i} does not exist (the pool holds {n})")
    if len(set(out)) != len(out):
        raise ValueError("Evaluate: an entry appears more than once (each entry has one row of the table)")
    return out


def split_batches(indices, max_graphs):
    """Consecutive runs of `max_graphs` of `indices`, in the order given; the last one may be shorter."""
    B = int(max_graphs)
    if B < 1:
        raise ValueError("max_graphs must be at least 1")
    idx = list(indices)
    return [idx[k:k + B] for k in range(0, len(idx), B)]


def _log(v):
    return math.log(v) if v > 0.0 else (-math.inf if v == 0.0 else math.nan)      # (torch.log's values for 0, negatives and NaN)


def make_report(entries, table, loss_weights):
    """The report of `entries` from their rows of the table (`table` [n, 16] fp32 on the host, row k = entries[k]).
    loss_weights = (w_cont, w_mom, w_press).  Everything beyond `losses` is float64 arithmetic on the stored fp32 values:
    loss_batch = w_press * press + w_cont * cont + w_mom * (mom_x + mom_y); objective = the mean of log(loss_batch), summed in the
    order asked; rel_update = columns 4-6 / 7-9, rel_error = 10-12 / 13-15 (NaN without a target)."""
    w_cont, w_mom, w_press = (float(w) for w in loss_weights)
    table = table.detach().to(torch.float32).reshape(-1, L.EVAL_RECORD).clone()
    assert table.shape[0] == len(entries)
    t = table.double()
    cont, mom_x, mom_y, press = t[:, 0], t[:, 1], t[:, 2], t[:, 3]
    loss_batch = w_press * press + w_cont * cont + w_mom * (mom_x + mom_y)
    total = 0.0
    for v in loss_batch.tolist():
        total += _log(v)
    objective = total / len(entries)
    nonfinite = int((~torch.isfinite(loss_batch)).sum())
    return EvalReport(list(entries), table[:, 0:4].clone(), loss_batch, objective, t[:, 4:7] / t[:, 7:10], t[:, 10:13] / t[:, 13:16],
                      nonfinite, table)


class Evaluate:
    WARM, EVICT_MAX = listcache.WARM, listcache.EVICT_MAX

    def __init__(self, model, pool, max_graphs=8, loss_weights=None, launch_mode="cmd_list", max_list_bytes=16 << 30,
                 max_sizes=None, arena=None):
        if launch_mode not in ("cmd_list", "eager"):
            raise ValueError('launch_mode must be "cmd_list" or "eager"')
        self.launch_mode, self.max_list_bytes = launch_mode, int(max_list_bytes)
        self.max_graphs = int(max_graphs)
        if not 1 <= self.max_graphs <= L.POOL_MAX_GRAPHS:
            raise ValueError(f"max_graphs must be in [1, {L.POOL_MAX_GRAPHS}]")
        self.model, self.pool = model, pool
        p = model.params
        self.loss_weights = tuple(float(w) for w in (loss_weights or (p.loss_cont, p.loss_mom, p.loss_press)))
        check_normalizer(model)
        require_gpu(pool.x[0])
        if arena is not None and arena.pool is not pool:
            raise ValueError("Evaluate: the arena belongs to another pool")
        self.arena = pool.arena(self.max_graphs, max_sizes) if arena is None else arena
        self.engine = model.engine()
        dev = self.dev = pool.device
        cap, B = self.arena.capacity, self.arena.max_graphs
        self.norm_global = True        # (what the graphs of a pool carry: gfv.pool.BatchArena._make_views)
        # created once, never reallocated
        self.n_entries = pool.n
        self._table = torch.full((pool.n, L.EVAL_RECORD), float("nan"), dtype=torch.float32, device=dev)
        self._partial = torch.zeros((max(cap["nchunk"], 1), L.EVAL_RECORD - 4), dtype=torch.float64, device=dev)
        self._counter = torch.zeros(1, dtype=torch.int32, device=dev)
        self._target3 = torch.zeros((max(cap["n"], 1), 3), dtype=torch.float32, device=dev)
        L.status_mirror()
        self._targets = {}                           # entry -> [n_i, 3] fp32 on the device
        self._lists = listcache.ListCache(self.max_list_bytes, dev=dev)      # batch signature -> the recorded body
        self._batches = 0
        self._fwd = StaticForward(model, B, dev)

    # ---- weights -------------------------------------------------------------------------------------------------------
    def refresh_weights(self):
        """(Re)build what depends on the parameter VALUES, in place.  The recorded lists are kept when nothing they point at
        moved, dropped otherwise."""
        if self._fwd.refresh():
            self._lists.clear()

    P = property(lambda self: self._fwd.P)

    def stats(self):
        return dict(self._lists.stats(), batches=self._batches)

    # ---- targets -------------------------------------------------------------------------------------------------------
    def set_target(self, i, uvp):
        """The field entry `i`'s prediction is compared with: [n_i, 3] fp32, copied to the device."""
        i = int(i)
        if not 0 <= i < self.n_entries:
            raise ValueError(f"Evaluate: pool entry {i} does not exist (the table holds {self.n_entries})")
        n = int(self.pool.sizes[i]["n"])
        t = torch.as_tensor(uvp, dtype=torch.float32)
        if tuple(t.shape) != (n, 3):
            raise ValueError(f"Evaluate: the target of entry {i} must be [{n}, 3], not {list(t.shape)}")
        self._targets[i] = t.detach().to(self.dev).contiguous().clone()

    def clear_targets(self):
        self._targets = {}

    # ---- one batch -----------------------------------------------------------------------------------------------------
    def _body(self, graphs, pl):
        losses, uvp_node, _ = self._fwd.forward(graphs[0].x, graphs[0]._gfv_x_raw, pl, False, self.norm_global)
        L.status_publish()
        return losses, uvp_node

    def _step(self, key, graphs, pl):
        """The body over the batch the arena holds, on the launch path of its signature -> (losses [B,4], uvp_node [N,3])."""
        self._batches += 1
        return self._lists.run(key, lambda: self._body(graphs, pl), self.launch_mode == "cmd_list")

    def _collect(self, batch, pl, x_raw, losses, uvp_node):
        """Targets into the staging buffer (device-to-device, at the host-known node offsets), then the collect launch."""
        B = len(batch)
        flags, off = [0] * B, 0
        for b, i in enumerate(batch):
            n = int(self.pool.sizes[i]["n"])
            t = self._targets.get(i)
            if t is not None:
                self._target3[off:off + n].copy_(t)
                flags[b] = 1
            off += n
        assert off == pl.N
        ent, flg = (C.c_int32 * B)(*batch), (C.c_int32 * B)(*flags)
        rc = L.load().gfv_eval_collect(
            uvp_node.data_ptr(), x_raw.data_ptr(), self._target3.data_ptr() if any(flags) else None, pl.N, pl.chunk_beg.data_ptr(),
            pl.chunk_end.data_ptr(), pl.gchunk_ptr.data_ptr(), pl.n_chunks, B, losses.data_ptr(), C.addressof(ent), C.addressof(flg),
            self._table.data_ptr(), self.n_entries, self._partial.data_ptr(), self._counter.data_ptr(), L.stream_ptr())
        L.check(rc, "gfv_eval_collect")

    # ---- the run -------------------------------------------------------------------------------------------------------
    def run(self, indices=None):
        """Evaluate the pool entries `indices` (None: all of them), `max_graphs` at a time in the order given -> EvalReport, rows
        in the order asked.  One synchronisation, at the end.  The pool is not written."""
        L.raise_on_status("Evaluate.run")
        idx = check_indices(indices, min(self.pool.n, self.n_entries))
        check_normalizer(self.model)
        self._fwd.check("Evaluate", "evaluation")
        batches = split_batches(idx, self.max_graphs)
        for batch in batches:           # every batch has to fit before anything is launched
            check_fits(batch_totals(self.pool.sizes, batch), len(batch), self.arena.capacity, self.arena.max_graphs)
        for batch in batches:
            graphs, pl = self.arena.load(batch)
            losses, uvp_node = self._step(self.arena.signature(batch), graphs, pl)
            self._collect(batch, pl, graphs[0]._gfv_x_raw, losses, uvp_node)
            self._lists.parked = None   # (a list the byte budget refused: its pool held the outputs up to here)
        table = self._table.cpu()[idx]  # (the one synchronisation)
        L.raise_on_status("Evaluate.run")
        return make_report(idx, table, self.loss_weights)
