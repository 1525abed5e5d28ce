"""Training log: per-step losses, norms and guard decisions kept on the device (include/gfv.h gfv_train_log_norms /
gfv_train_log_append, csrc/trainlog.hip).

A training run that wants its own loss curve no longer drains the queue every step: with `log=...` a `TrainStep` /
`PoolTrainStep` issues two short launches behind the optimiser launches of every step - eagerly, in every launch mode, never
inside a recorded list or a captured graph - and the host reads the ring when it likes, once per epoch say:

    ts = PoolTrainStep(model, pool, max_graphs=8, log=4096)               # or log=TrainLog(...), log={"buckets": [...]}
    for idx in batches: ts.step(idx)                                      # nothing here waits for the device
    rows = ts.log.read()                                                  # ONE copy, ONE synchronisation
    rows.loss, rows.norm, rows.decision, rows.entries, rows.grad_sumsq    # arrays in append order; rows.dropped
    trainlog.derive(rows, ts.loss_weights)                                # loss_batch, objective: float64, on the host
    ts.log.entry_stats()                                                  # visits, last ordinal, last terms per pool entry

`TrainLog` owns the ring (one allocation: a 64-byte header with the 64-bit cursor, then `capacity` rows), the bucket tables, the
norm launch's sums and workspace, and the per-entry table.  It is diagnostics, not state: no checkpoint holds it.

Buckets: `buckets=["encoder", "processor"]` names parameter-name prefixes; a live parameter (one with a gradient, not frozen)
belongs to the FIRST prefix it starts with, the unmatched ones form a last bucket "rest" (dropped if empty); None is one bucket
"all" over every live parameter.  Per bucket a row carries sum g^2, sum p^2 and the count of non-finite g, in double, g as
stored (apply `grad_scale` and the clip coefficient on the host if wanted).  The buckets are rebuilt when the set of frozen
parameters changes (the event on which the guard rebuilds its segments); if that changes their NUMBER - "rest" appears or
vanishes - the row layout changes and the ring starts again from empty.

The host-only pieces - `ring_window`, `bucket_segments`, `bucket_tables`, `check_args`, `parse_rows` - need no GPU."""
from __future__ import annotations

import collections
import ctypes as C
import math
import numbers

import numpy as np
import torch

from . import lib as L

FIELDS = ("ordinal", "adam_t", "loss", "lr", "B", "norm", "coef", "decision", "apply", "applied", "terms", "entries",
          "grad_sumsq", "param_sumsq", "grad_nonfinite", "dropped")
TrainLogRows = collections.namedtuple("TrainLogRows", FIELDS)
EntryStats = collections.namedtuple("EntryStats", "visits last_ordinal last_terms")
HEADER_WORDS = 16            # the ring allocation's own header: the cursor (int64) in words 0-1, the rest zero
SKIP_BITS = L.GUARD_SKIP_NONFINITE | L.GUARD_SKIP_FLAG


# ---- host-side pieces: no GPU ------------------------------------------------------------------------------------------------------
def check_args(capacity, max_graphs, buckets=None):
    """-> (capacity, max_graphs, prefixes or None), or ValueError."""
    for what, v in (("capacity", capacity), ("max_graphs", max_graphs)):
        if isinstance(v, bool) or not isinstance(v, numbers.Integral) or v < 1:
            raise ValueError(f"TrainLog: {what} must be an integer >= 1, got {v!r}")
    if max_graphs > L.POOL_MAX_GRAPHS:
        raise ValueError(f"TrainLog: max_graphs must be at most {L.POOL_MAX_GRAPHS}, got {max_graphs}")
    if buckets is not None:
        if isinstance(buckets, str):
            raise ValueError("TrainLog: buckets is a list of parameter-name prefixes, not one string")
        buckets = list(buckets)
        for b in buckets:
            if not isinstance(b, str) or not b:
                raise ValueError(f"TrainLog: a bucket is a non-empty parameter-name prefix, got {b!r}")
        if len(set(buckets)) != len(buckets):
            raise ValueError("TrainLog: a bucket prefix appears twice")
        if "rest" in buckets:
            raise ValueError('TrainLog: "rest" names the bucket of the unmatched parameters')
        if not buckets:
            raise ValueError("TrainLog: an empty list of buckets (None = one bucket over every live parameter)")
        if len(buckets) + 1 > L.TRAIN_LOG_MAX_BUCKETS:
            raise ValueError(f"TrainLog: at most {L.TRAIN_LOG_MAX_BUCKETS - 1} named buckets")
    return int(capacity), int(max_graphs), buckets


def row_words(max_graphs, K):
    """32-bit words of a ring row (gfv_train_log_row_words of include/gfv.h, restated)."""
    return L.TRAIN_LOG_HEAD + ((5 * max_graphs + 1) & ~1) + 6 * K


def ring_window(count, capacity):
    """After `count` appends into a ring of `capacity` rows -> (first ordinal still held, rows held, dropped, the ring row of
    each held ordinal in append order)."""
    count, capacity = int(count), int(capacity)
    n = min(count, capacity)
    first = count - n
    return first, n, first, [(first + i) % capacity for i in range(n)]


def bucket_segments(store, prefixes=None, exclude=()):
    """[(name, [(offset, count), ...])]: the buckets of `store` (a gfv.engine.GradStore).  Live parameters only - none of
    `store.skip` (no gradient), of `exclude` (frozen), of zero size; no alignment padding.  A parameter belongs to the first
    prefix its name starts with, the unmatched ones to a last bucket "rest" (dropped if empty); prefixes None: one bucket "all".
    Within a bucket the segments keep the store's order and neighbours without a gap are merged (the guard's rule).  ValueError
    for a named bucket that is empty, or when nothing is live at all."""
    names = ["all"] if prefixes is None else list(prefixes) + ["rest"]
    segs = [[] for _ in names]
    for n, off in store.off.items():
        k = store.numel(n)
        if n in store.skip or n in exclude or k == 0:
            continue
        b = 0 if prefixes is None else next((i for i, p in enumerate(prefixes) if n.startswith(p)), len(names) - 1)
        if segs[b] and segs[b][-1][0] + segs[b][-1][1] == off:
            segs[b][-1][1] += k
        else:
            segs[b].append([off, k])
    out = []
    for name, sg in zip(names, segs):
        if not sg:
            if name == "rest" and prefixes is not None:
                continue
            raise ValueError("TrainLog: no live parameter at all" if prefixes is None else
                             f"TrainLog: bucket {name!r} matches no live parameter")
        out.append((name, [(int(o), int(k)) for o, k in sg]))
    return out


def bucket_tables(buckets):
    """The two device tables of gfv_train_log_norms from bucket_segments' result, as int64 lists: segs [n_seg, 2] and
    bucket_tab [K, 4] = {first segment, one past the last, first chunk, elements}; and the chunk total."""
    segs, tab, chunk = [], [], 0
    for _, sg in buckets:
        n = sum(k for _, k in sg)
        tab.append([len(segs), len(segs) + len(sg), chunk, n])
        segs.extend([o, k] for o, k in sg)
        chunk += (n + L.TRAIN_LOG_CHUNK - 1) // L.TRAIN_LOG_CHUNK
    return segs, tab, chunk


def parse_rows(words, capacity, max_graphs, K):
    """The ring allocation as the host sees it (`words`: int32 numpy array, header + capacity rows) -> TrainLogRows in append
    order."""
    words = np.ascontiguousarray(words, dtype=np.int32)
    rw = row_words(max_graphs, K)
    assert words.size == HEADER_WORDS + capacity * rw, (words.size, capacity, rw)
    count = int(words[0:2].view(np.int64)[0])
    _, n, dropped, order = ring_window(count, capacity)
    rows = words[HEADER_WORDS:].reshape(capacity, rw)[np.asarray(order, dtype=np.int64)].copy() if n else \
        np.zeros((0, rw), dtype=np.int32)
    f32 = rows.view(np.float32)
    t0 = L.TRAIN_LOG_HEAD
    e0 = t0 + 4 * max_graphs
    s0 = L.TRAIN_LOG_HEAD + ((5 * max_graphs + 1) & ~1)
    sums = np.ascontiguousarray(rows[:, s0:s0 + 6 * K]).view(np.float64).reshape(n, K, 3)
    return TrainLogRows(
        ordinal=np.ascontiguousarray(rows[:, 0:2]).view(np.int64).reshape(n), adam_t=f32[:, 2].copy(), loss=f32[:, 3].copy(),
        lr=f32[:, 4].copy(), B=rows[:, 5].copy(), norm=f32[:, 6].copy(), coef=f32[:, 7].copy(), decision=rows[:, 8].copy(),
        apply=rows[:, 9].copy(), applied=rows[:, 10].copy(), terms=f32[:, t0:e0].reshape(n, max_graphs, 4).copy(),
        entries=rows[:, e0:e0 + max_graphs].copy(), grad_sumsq=sums[:, :, 0].copy(), param_sumsq=sums[:, :, 1].copy(),
        grad_nonfinite=sums[:, :, 2].astype(np.int64), dropped=dropped)


def _log(v):
    return math.log(v) if v > 0.0 else (-math.inf if v == 0.0 else math.nan)      # (torch.log's values for 0, negatives and NaN)


def derive(rows, loss_weights):
    """(loss_batch [n, max_graphs] float64, objective [n] float64) of the logged steps, float64 arithmetic on the stored fp32
    terms as gfv.evaluate.make_report does it: loss_batch = w_press * press + w_cont * cont + w_mom * (mom_x + mom_y) per slot
    (NaN beyond B), objective = the mean of log(loss_batch) over the step's B graphs, summed in slot order.  loss_weights =
    (w_cont, w_mom, w_press).  Nothing of this is computed on the device."""
    w_cont, w_mom, w_press = (float(w) for w in loss_weights)
    t = rows.terms.astype(np.float64)
    lb = w_press * t[:, :, 3] + w_cont * t[:, :, 0] + w_mom * (t[:, :, 1] + t[:, :, 2])
    obj = np.zeros(lb.shape[0], dtype=np.float64)
    for i, B in enumerate(rows.B.tolist()):
        lb[i, B:] = np.nan
        total = 0.0
        for v in lb[i, :B].tolist():
            total += _log(v)
        obj[i] = total / B if B else np.nan
    return lb, obj


def make_log(log, max_graphs):
    """The `log=` keyword of the step objects -> a TrainLog or None: an int capacity, a TrainLog, or a dict of its arguments."""
    if log is None:
        return None
    if isinstance(log, TrainLog):
        return log
    if isinstance(log, dict):
        kw = dict(log)
        kw.setdefault("max_graphs", max_graphs)
        return TrainLog(**kw)
    if isinstance(log, bool) or not isinstance(log, numbers.Integral):
        raise ValueError(f"log must be None, an int capacity, a TrainLog or a dict of its arguments, got {log!r}")
    return TrainLog(capacity=int(log), max_graphs=max_graphs)


# ---- the device side ---------------------------------------------------------------------------------------------------------------
class TrainLog:
    def __init__(self, capacity=4096, max_graphs=8, buckets=None):
        self.capacity, self.max_graphs, self.prefixes = check_args(capacity, max_graphs, buckets)
        self.device = None
        self.names, self.K = None, None
        self.buf = self.table = None
        self._owner = None

    # binding to the step object that feeds it: the flat buffers' layout and the device
    def bind(self, store, device, exclude=(), owner=None):
        if self._owner is not None and owner is not None and self._owner != id(owner):
            raise ValueError("TrainLog: already bound to another step object")
        self._owner = None if owner is None else id(owner)
        self.device = device
        self.set_buckets(store, exclude)

    def set_buckets(self, store, exclude=()):
        """(Re)build the bucket tables of `store` without the parameters of `exclude`.  New tables, sums and workspace; the ring
        is kept unless the number of buckets changed."""
        buckets = bucket_segments(store, self.prefixes, exclude)
        segs, tab, n_chunks = bucket_tables(buckets)
        dev = self.device
        self.names = [n for n, _ in buckets]
        self.segs = torch.tensor(segs, dtype=torch.int64).reshape(-1).to(dev)
        self.bucket_tab = torch.tensor(tab, dtype=torch.int64).reshape(-1).to(dev)
        self.n_chunks = n_chunks
        K = len(buckets)
        self.sums = torch.zeros(3 * K, dtype=torch.float64, device=dev)
        ws = int(L.load(raw=True).gfv_train_log_workspace_bytes(n_chunks))
        self.ws = torch.zeros((ws + 7) // 8, dtype=torch.float64, device=dev)
        if K != self.K:
            self.K = K
            self.row_words = row_words(self.max_graphs, K)
            assert self.row_words == L.load(raw=True).gfv_train_log_row_words(self.max_graphs, K)
            self.buf = torch.zeros(HEADER_WORDS + self.capacity * self.row_words, dtype=torch.int32, device=dev)

    def _grow_table(self, n_entries):
        if n_entries <= 0:
            return
        old = self.table
        if old is not None and old.shape[0] >= n_entries:
            return
        self.table = torch.zeros((n_entries, L.TRAIN_LOG_ENTRY_RECORD), dtype=torch.int32, device=self.device)
        if old is not None:
            self.table[:old.shape[0]].copy_(old)      # (on the stream of the appends: behind every one that wrote `old`)

    def append(self, flat_g, flat_p, state, hyper, loss, losses, B, guard=None, accum=None, entries=None, n_entries=0):
        """The two launches of one step, on the current stream: the caller has issued the optimiser launches before.  guard,
        accum: the device records or None; entries: the pool entry of every graph (host ints) or None; n_entries: the pool's size
        now (the table grows with it, old rows kept)."""
        if not 1 <= int(B) <= self.max_graphs:
            raise ValueError(f"TrainLog: a step over {B} graphs, the rows hold {self.max_graphs} (max_graphs)")
        lib, st = L.load(), L.stream_ptr()
        L.check(lib.gfv_train_log_norms(flat_g.data_ptr(), flat_p.data_ptr(), self.segs.data_ptr(), self.bucket_tab.data_ptr(),
                                        self.K, self.n_chunks, self.sums.data_ptr(), self.ws.data_ptr(), st), "train_log_norms")
        ent = None
        if entries is not None:
            self._grow_table(int(n_entries))
            ent = (C.c_int32 * len(entries))(*entries)
        table, rows = (None, 0) if self.table is None else (self.table.data_ptr(), self.table.shape[0])
        base = self.buf.data_ptr()
        L.check(lib.gfv_train_log_append(base + 4 * HEADER_WORDS, self.capacity, self.max_graphs, self.K, base, state.data_ptr(),
                                         hyper.data_ptr(), loss.data_ptr(), losses.data_ptr(), int(B),
                                         None if guard is None else guard.data_ptr(), None if accum is None else accum.data_ptr(),
                                         ent, self.sums.data_ptr(), table, rows, st), "train_log_append")

    def _need(self):
        if self.buf is None:
            raise RuntimeError("TrainLog: not attached to a step object yet (pass it as log=...)")

    def read(self):
        """-> TrainLogRows: arrays in append order - ordinal, adam_t, loss, lr, B, norm, coef, decision, apply, applied, terms
        [n, max_graphs, 4], entries [n, max_graphs], grad_sumsq / param_sumsq / grad_nonfinite [n, K] (bucket k = self.names[k]) -
        and `dropped`, the appends the ring has overwritten.  One device-to-host copy, one synchronisation."""
        self._need()
        return parse_rows(self.buf.cpu().numpy(), self.capacity, self.max_graphs, self.K)

    def entry_stats(self):
        """-> EntryStats(visits [n_entries], last_ordinal [n_entries], last_terms [n_entries, 4]) of the per-entry table (empty
        arrays before the first step over pool entries).  Synchronises."""
        self._need()
        if self.table is None:
            return EntryStats(np.zeros(0, np.int32), np.zeros(0, np.int32), np.zeros((0, 4), np.float32))
        t = self.table.cpu().numpy()
        return EntryStats(t[:, 0].copy(), t[:, 1].copy(), np.ascontiguousarray(t[:, 2:6]).view(np.float32).copy())

    def clear(self):
        """Zero the cursor, the ring and the tables."""
        self._need()
        self.buf.zero_()
        self.sums.zero_()
        if self.table is not None:
            self.table.zero_()
