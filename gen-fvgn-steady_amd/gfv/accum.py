"""Gradient accumulation: k micro-batches, one optimiser step, decided on the device (include/gfv.h gfv_grad_accum_dev,
DESIGN.md 5g).  `GradAccum` owns the second flat gradient buffer `acc` and the device record `accum[8]`; the launches that read
them are issued by `gfv.optstep.optimizer_launches`, the same ones on every micro-step: which of them does what follows from the
record's own count, so one recorded launch list or captured graph per batch signature serves the first, the middle and the
closing micro-step alike.  The host writes `steps` into word [0] and zeroes the open accumulation on a reset; it never tells a
launch its phase."""
from __future__ import annotations

import numbers

import torch


def check_accum_steps(accum_steps, dist_on=False):
    """The constructor check shared by the step objects; needs no GPU."""
    if isinstance(accum_steps, bool) or not isinstance(accum_steps, numbers.Integral) or accum_steps < 1:
        raise ValueError(f"accum_steps must be an integer >= 1, got {accum_steps!r}")
    if accum_steps > 1 and dist_on:
        raise ValueError("accum_steps > 1 with a data-parallel step: ranks whose micro-batches hold different graph counts would "
                         "need a weighted exchange of the accumulated gradient, which is not implemented")
    return int(accum_steps)


class GradAccum:
    def __init__(self, n, device, steps):
        self.n = int(n)
        self.acc = torch.zeros(self.n, dtype=torch.float32, device=device)
        self.rec = torch.zeros(8, dtype=torch.float32, device=device)
        self.rec_i = self.rec.view(torch.int32)
        self.steps = 0
        self.pending = 0            # micro-steps of the open accumulation, counted by the owner per step issued
        self.set_steps(steps)

    def set_steps(self, steps):
        """A new k: mirrored into word [0]; the open accumulation is dropped."""
        self.steps = int(steps)
        self.rec_i[0:1].fill_(self.steps)
        self.reset()

    def reset(self):
        """Drop the open accumulation (words [1], [2], [4]).  `acc` stays as it is: a first micro-step does not read it."""
        self.rec_i[1:3].zero_()
        self.rec[4:5].zero_()
        self.pending = 0

    def note_step(self):
        self.pending = (self.pending + 1) % self.steps

    def stats(self):
        """The device record (synchronises: for logging every so often)."""
        rec = self.rec.detach().cpu()
        ints = rec.view(torch.int32)
        return {"micro": int(ints[1]), "graphs": int(ints[2]), "loss_mean": float(rec[5]), "closed": int(ints[6])}
