"""Anderson acceleration AA(m) of the steady-state rollout, decided on the device (include/gfv.h gfv_anderson_gram /
gfv_anderson_mix, csrc/anderson.hip).

`Rollout` is the fixed-point iteration x_{k+1} = G(x_k) of a trained model G.  With `anderson=m` it keeps the last m differences
of the residual f_k = G(x_k) - x_k and of G(x_k) per graph, solves the m x m least-squares problem  min || f_k - dF gamma ||  and
advances to  G(x_k) - (1-beta) f_k - sum_j gamma_j (dG_j - (1-beta) dF_j)  instead of G(x_k).  `AndersonState` owns the device
state of that: allocated once, never reallocated (a recorded launch list points at it), zeroed by `reset()`; its two launches go
between the forward and `gfv_rollout_advance` and read nothing from the host, so one recorded list serves every step.

For the STEADY iteration only: the accelerated iterates are not the model's time steps.  A time-accurate unsteady rollout must
leave it off (`anderson=0`, the default: no launch, no allocation).

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
