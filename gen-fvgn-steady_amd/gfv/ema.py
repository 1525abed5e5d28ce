"""Averaged weights: an exponential moving average of the parameters, advanced inside the fused Adam launch (include/gfv.h
gfv_adam_step_ema_dev).  `WeightEMA` owns the flat average `e` and the device record `ema[8]`; the Adam launch
that reads them is issued by `gfv.optstep.optimizer_launches`.  Whether an update happens is decided where the step is decided:
a step that is left out or held back leaves `e`, the update count and the next weight as they were.  The host writes decay and
warmup through `gfv_ema_init` (the weight's formula is evaluated on the device only); `ema_weight` below states the same formula
for documentation and tests."""
from __future__ import annotations

import math
import numbers
import struct

import torch

from . import lib as L


def check_ema(decay, warmup=True):
    """The constructor check shared by the step objects; needs no GPU.  -> None (off) or the decay as a float."""
    if decay is None:
        return None
    if isinstance(decay, bool) or not isinstance(decay, numbers.Real) or math.isnan(decay) or not 0.0 <= decay < 1.0:
        raise ValueError(f"ema_decay must be None or a real number in [0, 1), got {decay!r}")
    if struct.unpack("f", struct.pack("f", float(decay)))[0] >= 1.0:
        raise ValueError(f"ema_decay must be below 1 as an fp32 value (the device record holds it as one), got {decay!r}")
    return float(decay)


def ema_weight(decay, warmup, k):
    """Weight of the update that follows `k` applied ones: e <- e + w (p - e).  w = 1 - decay, or with warmup
    1 - min(decay, (1 + k) / (10 + k)): a young average follows the parameters closely (w = 0.9 at k = 0) and reaches the
    requested decay at k = (10 decay - 1) / (1 - decay)."""
    d = float(decay)
    if warmup:
        d = min(d, (1.0 + k) / (10.0 + k))
    return 1.0 - d


class WeightEMA:
    def __init__(self, flat_p, n, decay, warmup):
        self.n = int(n)
        self.e = torch.empty(self.n, dtype=torch.float32, device=flat_p.device)
        self.rec = torch.zeros(8, dtype=torch.float32, device=flat_p.device)
        self.decay, self.warmup = float(decay), bool(warmup)
        self.swapped = False        # inside `TrainStep.ema_weights()`: e holds the iterate, flat_p the average
        self.reset(flat_p)

    def set(self, decay, warmup, updates=None):
        """decay, warmup (and the update count; default: as the device has it) through the one-thread launch that also writes
        the next weight."""
        if updates is None:
            updates = int(self.rec.view(torch.int32)[2])
        self.decay, self.warmup = float(decay), bool(warmup)
        L.check(L.load().gfv_ema_init(self.rec.data_ptr(), self.decay, int(self.warmup), int(updates), L.stream_ptr()), "ema_init")

    def reset(self, flat_p):
        """The average restarts from the current parameters: e <- flat_p[:n], updates <- 0."""
        self.e.copy_(flat_p[:self.n])
        self.set(self.decay, self.warmup, 0)

    def swap(self, tensors, offsets):
        """Exchange the contents of the parameters `tensors` (views of the flat parameter buffer) and of the average at their
        flat `offsets` (plain copies: an evaluation, not a step).  The copies are in-place operations on the parameters
        themselves, so their version counters move and a gfv.rollout.WeightGuard notices."""
        avg = [self.e[o:o + t.numel()].view(t.shape) for t, o in zip(tensors, offsets)]
        with torch.no_grad():
            tmp = [t.detach().clone() for t in tensors]
            torch._foreach_copy_(list(tensors), avg)
            torch._foreach_copy_(avg, tmp)
        self.swapped = not self.swapped

    def stats(self):
        """The device record (synchronises: for logging every so often)."""
        rec = self.rec.detach().cpu()
        ints = rec.view(torch.int32)
        return {"decay": float(rec[0]), "warmup": bool(int(ints[1])), "updates": int(ints[2]), "w": float(rec[3])}
