"""Anderson acceleration AA(m) of the steady-state rollout, decided on the device (include/gfv.h gfv_anderson_gram /
gfv_anderson_mix, csrc/anderson.hip).

`Rollout` is the fixed-point iteration x_{k+1} = G(x_k) of a trained model G.  With `anderson=m` it keeps the last m differences
of the residual f_k = G(x_k) - x_k and of G(x_k) per graph, solves the m x m least-squares problem  min || f_k - dF gamma ||  and
advances to  G(x_k) - (1-beta) f_k - sum_j gamma_j (dG_j - (1-beta) dF_j)  instead of G(x_k).  `AndersonState` owns the device
state of that: allocated once, never reallocated (a recorded launch list points at it), zeroed by `reset()`; its two launches go
between the forward and `gfv_rollout_advance` and read nothing from the host, so one recorded list serves every step.

For the STEADY iteration only: the accelerated iterates are not the model's time steps.  A time-accurate unsteady rollout must
leave it off (`anderson=0`, the default: no launch, no allocation).

`SlotAndersonState` is the same for the slots of a `gfv.sweep.Sweep` (gfv_sweep_anderson_gram / gfv_sweep_anderson_mix, one kernel
body with the rollout form: csrc/anderson_kernel.h): rings per slot at a fixed stride, the slot's own age as the step index,
frozen slots skipped, a record per slot instead of a table, and a plain step whenever the residual is below the sweep's `tol`.

The defaults `reg=1e-10` and `restart=10` are the values of a CPU experiment on linear contractions (tests/anderson_ref.py); they
have not been tuned on a trained model.
"""
from __future__ import annotations

import math

import torch

from . import lib as L

MAX_DEPTH = 8                               # GFV_AA_MAX_DEPTH of include/gfv.h
PARTIALS = 46                               # GFV_AA_PARTIALS
NONFINITE, GROWTH, SINGULAR = 1, 2, 4       # GFV_AA_* flags: column 3 of the table
TABLE_WIDTH = 4                             # (|| f ||_2, || g ||_2, depth used, flags) per step and graph
FLAG_NAMES = {NONFINITE: "NONFINITE", GROWTH: "GROWTH", SINGULAR: "SINGULAR"}


def check_args(anderson=0, beta=1.0, reg=1e-10, restart=10.0, start=0):
    """The constructor checks of every owner of an AndersonState; needs no GPU.  -> (m, beta, reg, restart, start)."""
    if isinstance(anderson, bool) or int(anderson) != anderson:
        raise ValueError(f"anderson must be an integer depth 0 .. {MAX_DEPTH}, got {anderson!r}")
    m = int(anderson)
    if not 0 <= m <= MAX_DEPTH:
        raise ValueError(f"anderson must be 0 (off) or a depth 1 .. {MAX_DEPTH}, got {anderson!r}")
    beta, reg, restart = float(beta), float(reg), float(restart)
    if math.isnan(beta) or not 0.0 < beta <= 1.0:
        raise ValueError(f"anderson_beta must be in (0, 1], got {beta!r}")
    if math.isnan(reg) or reg < 0.0:
        raise ValueError(f"anderson_reg must be a non-negative number, got {reg!r}")
    if math.isnan(restart) or restart < 0.0 or 0.0 < restart <= 1.0:
        raise ValueError(f"anderson_restart must be 0 (no growth test) or a factor above 1, got {restart!r}")
    if isinstance(start, bool) or int(start) != start or int(start) < 0:
        raise ValueError(f"anderson_start must be a non-negative step index, got {start!r}")
    return m, beta, reg, restart, int(start)


class AndersonState:
    def __init__(self, plan, device, max_steps, m, beta=1.0, reg=1e-10, restart=10.0, start=0):
        self.m, self.beta, self.reg, self.restart, self.start = check_args(m, beta, reg, restart, start)
        if self.m < 1:
            raise ValueError("AndersonState needs a depth of at least 1")
        self.plan, self.max_steps = plan, int(max_steps)
        N, B = plan.N, plan.B
        f32 = dict(dtype=torch.float32, device=device)
        self.f_prev, self.g_prev = torch.zeros((N, 3), **f32), torch.zeros((N, 3), **f32)
        self.dF, self.dG = torch.zeros((self.m, N, 3), **f32), torch.zeros((self.m, N, 3), **f32)
        self.state = torch.zeros((B, 4), dtype=torch.int32, device=device)       # cnt, head, has_prev, restarts
        self.r_prev = torch.zeros(B, dtype=torch.float64, device=device)
        self.gamma = torch.zeros((B, MAX_DEPTH), dtype=torch.float64, device=device)
        self.partial = torch.zeros((plan.n_chunks, PARTIALS), dtype=torch.float64, device=device)
        self.counter = torch.zeros(1, dtype=torch.int32, device=device)
        self.table = torch.zeros((self.max_steps, B, TABLE_WIDTH), **f32)

    def launch(self, uvp_node, x_backup, step_state):
        """The two launches of one step, on the current stream: `uvp_node` [N,3] (the model's output) becomes the iterate to
        advance to; `step_state` is the rollout's step counter, which gfv_rollout_advance increments afterwards."""
        pl, lib, st = self.plan, L.load(), L.stream_ptr()
        tabs = (pl.chunk_beg.data_ptr(), pl.chunk_end.data_ptr(), pl.gchunk_ptr.data_ptr(), pl.n_chunks, pl.B, self.m)
        L.check(lib.gfv_anderson_gram(
            uvp_node.data_ptr(), x_backup.data_ptr(), pl.N, *tabs, self.reg, self.restart, self.start, self.f_prev.data_ptr(),
            self.g_prev.data_ptr(), self.dF.data_ptr(), self.dG.data_ptr(), self.state.data_ptr(), self.r_prev.data_ptr(),
            self.gamma.data_ptr(), self.partial.data_ptr(), self.counter.data_ptr(), self.table.data_ptr(), self.max_steps,
            step_state.data_ptr(), st), "gfv_anderson_gram")
        L.check(lib.gfv_anderson_mix(
            uvp_node.data_ptr(), self.f_prev.data_ptr(), pl.N, *tabs, self.beta, self.dF.data_ptr(), self.dG.data_ptr(),
            self.gamma.data_ptr(), self.table.data_ptr(), self.max_steps, step_state.data_ptr(), st), "gfv_anderson_mix")

    def reset(self):
        for t in (self.f_prev, self.g_prev, self.dF, self.dG, self.state, self.r_prev, self.gamma, self.partial, self.counter,
                  self.table):
            t.zero_()

    def stats(self):
        """Restarts per graph and the other state words (synchronises)."""
        s = self.state.cpu()
        return {"restarts": s[:, 3].tolist(), "columns": s[:, 0].tolist(), "head": s[:, 1].tolist(), "has_prev": s[:, 2].tolist()}


# ---- the slot form: Anderson acceleration per slot of a Sweep ----------------------------------------------------------------
def check_ring_stride(node_counts, ring_stride):
    """Every entry that runs in a slot must fit the slot's ring region of `ring_stride` rows; needs no GPU.
    `node_counts`: {entry: nodes} or a sequence (entry = position).  ValueError names the first entry that does not fit."""
    stride = int(ring_stride)
    if stride < 1:
        raise ValueError(f"the ring stride must be at least 1, got {ring_stride!r}")
    items = node_counts.items() if hasattr(node_counts, "items") else enumerate(node_counts)
    for e, n in items:
        if int(n) > stride:
            raise ValueError(f"Sweep: pool entry {e} has {int(n)} nodes, more than the Anderson ring stride of {stride} (the "
                             "largest node count of the pool when the Sweep was built); build a new Sweep for this pool")
    return stride


def ring_bytes(n_slots, ring_stride, m):
    """Device memory of the rings of the slot form: f_prev, g_prev and m columns each of dF, dG, fp32 x 3 channels."""
    return int(n_slots) * int(ring_stride) * (2 * int(m) + 2) * 12


def count_dict(count_row, slot_row):
    """One entry of `Sweep.anderson_stats()` from its rows of aa_count [4] and aa_slot [4]."""
    return {"accelerated": int(count_row[0]),
            "restarts": {"NONFINITE": int(count_row[1]), "GROWTH": int(count_row[2]), "SINGULAR": int(count_row[3])},
            "last_depth": int(slot_row[2])}


class SlotAndersonState:
    """The device state of AA(m) per slot of a `Sweep` (include/gfv.h gfv_sweep_anderson_gram / gfv_sweep_anderson_mix): rings per
    slot at a fixed stride, so that a neighbour's swap to an entry of another size moves nothing under a live slot's columns.
    Created once for `n_slots` x `ring_stride` rows, never reallocated (recorded lists point at it).  The step index is the slot's
    own age, frozen slots are skipped on the device, and the record of a step is `aa_slot[b]` / `aa_count[b]`."""

    def __init__(self, n_slots, ring_stride, max_chunks, device, m, beta=1.0, reg=1e-10, restart=10.0, start=0):
        self.m, self.beta, self.reg, self.restart, self.start = check_args(m, beta, reg, restart, start)
        if self.m < 1:
            raise ValueError("SlotAndersonState needs a depth of at least 1")
        self.n_slots, self.ring_stride = int(n_slots), check_ring_stride((), ring_stride)
        B, R = self.n_slots, self.n_slots * self.ring_stride
        f32 = dict(dtype=torch.float32, device=device)
        self.f_prev, self.g_prev = torch.zeros((R, 3), **f32), torch.zeros((R, 3), **f32)
        self.dF, self.dG = torch.zeros((self.m, R, 3), **f32), torch.zeros((self.m, R, 3), **f32)
        self.state = torch.zeros((B, 4), dtype=torch.int32, device=device)       # cnt, head, has_prev, restarts
        self.r_prev = torch.zeros(B, dtype=torch.float64, device=device)
        self.gamma = torch.zeros((B, MAX_DEPTH), dtype=torch.float64, device=device)
        self.partial = torch.zeros((max(int(max_chunks), 1), PARTIALS), dtype=torch.float64, device=device)
        self.counter = torch.zeros(1, dtype=torch.int32, device=device)
        self.aa_slot = torch.zeros((B, TABLE_WIDTH), **f32)                      # (|| f ||, || g ||, depth, flags) per slot
        self.aa_count = torch.zeros((B, 4), dtype=torch.int32, device=device)    # accelerated, NONFINITE, GROWTH, SINGULAR

    def launch(self, uvp_node, x_backup, pl, ctl, slots):
        """The two launches of one step over the batch of plan `pl` (at most `n_slots` graphs), on the current stream; `ctl` and
        `slots` are the sweep's control words and per-slot state, which the advance behind them updates."""
        if pl.B > self.n_slots or pl.n_chunks > self.partial.shape[0]:
            raise ValueError(f"SlotAndersonState: a batch of {pl.B} graphs / {pl.n_chunks} chunks exceeds what it was built for")
        lib, st = L.load(), L.stream_ptr()
        tabs = (pl.chunk_beg.data_ptr(), pl.chunk_end.data_ptr(), pl.gchunk_ptr.data_ptr(), pl.n_chunks, pl.B, self.m)
        L.check(lib.gfv_sweep_anderson_gram(
            uvp_node.data_ptr(), x_backup.data_ptr(), pl.N, *tabs, self.reg, self.restart, self.start, self.ring_stride,
            self.f_prev.data_ptr(), self.g_prev.data_ptr(), self.dF.data_ptr(), self.dG.data_ptr(), self.state.data_ptr(),
            self.r_prev.data_ptr(), self.gamma.data_ptr(), self.partial.data_ptr(), self.counter.data_ptr(), ctl.data_ptr(),
            slots.data_ptr(), self.aa_slot.data_ptr(), self.aa_count.data_ptr(), st), "gfv_sweep_anderson_gram")
        L.check(lib.gfv_sweep_anderson_mix(
            uvp_node.data_ptr(), self.f_prev.data_ptr(), pl.N, *tabs, self.beta, self.ring_stride, self.dF.data_ptr(),
            self.dG.data_ptr(), self.gamma.data_ptr(), slots.data_ptr(), self.aa_slot.data_ptr(), st), "gfv_sweep_anderson_mix")

    def reset_slot(self, b):
        """Slot b takes a new entry: its state words, r_prev and counts go to zero.  The rings need no clearing: cnt = 0 and
        has_prev = 0 mask them, and stale values, NaN included, are never read."""
        self.state[b].zero_()
        self.r_prev[b].zero_()
        self.aa_count[b].zero_()

    def reset(self):
        """Every slot as new (the start of a run); the rings are left as they are (see reset_slot)."""
        for t in (self.state, self.r_prev, self.gamma, self.counter, self.aa_slot, self.aa_count):
            t.zero_()
