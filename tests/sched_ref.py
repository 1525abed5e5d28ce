"""The rules of the schedule launch (include/gfv.h gfv_lr_schedule) restated in plain Python.

Written from the header's paragraph, not from the kernel: tests/test_schedule_cpu.py holds it to the reference's classes (recorded
doubles, tests/golden/lr_schedules.json) and to torch's ReduceLROnPlateau exactly; tests/test_schedule_gpu.py compares the kernel
with it.  Python floats are IEEE doubles and `**` / math.pow is libm's pow: every statement is one rounding, in the order the
header writes it.  Nothing here touches a GPU.
"""
import math
import struct

EVAL, TICK, FOLLOW = 0, 1, 2


def f32(x):
    """float32(x) (round to nearest even) as a Python float."""
    return struct.unpack("f", struct.pack("f", x))[0]


def hexd(x):
    return float(x).hex()


def stepexp(e, startlr, steplr_milestone, steplr_gamma, explr_milestone, explr_gamma, total_epoch, min_lr, base_lr=None):
    base_lr = startlr if base_lr is None else base_lr
    if e < steplr_milestone:
        return startlr
    if e < explr_milestone:
        return startlr * steplr_gamma
    decay_steps = total_epoch - explr_milestone
    return min_lr + max(base_lr * steplr_gamma - min_lr, 0) * math.pow(explr_gamma, (e - explr_milestone) / decay_steps)


def exp(e, base_lr, decay_steps, gamma, min_lr):
    return min_lr + max(base_lr - min_lr, 0) * math.pow(gamma, e / decay_steps)


def gradual(e, base_lr, milestone, gamma, expgamma, total_epoch, decay_steps, min_lr):
    hit = sum(1 for m in sorted(set(milestone)) if m <= min(e, total_epoch))
    s = base_lr * gamma ** hit
    if e <= total_epoch:
        return s
    return min_lr + max(s - min_lr, 0) * math.pow(expgamma, (e - total_epoch) / decay_steps)


def table(e, values):
    return values[min(max(e, 0), len(values) - 1)]


def warmup(e, base_lr, multiplier, warmup_epochs):
    if multiplier == 1.0:
        return base_lr * (float(e) / warmup_epochs)
    return base_lr * ((multiplier - 1.0) * e / warmup_epochs + 1.0)


class Plateau:
    """ReduceLROnPlateau (mode "min", threshold mode "rel") with the optional warm-up, state as the record holds it."""

    def __init__(self, base_lr, factor=0.1, patience=10, threshold=1e-4, cooldown=0, min_lr=0.0, eps=1e-8, warmup_epochs=0,
                 multiplier=1.0):
        self.base_lr, self.factor, self.patience, self.threshold = base_lr, factor, patience, threshold
        self.cooldown, self.min_lr, self.eps, self.warmup_epochs, self.multiplier = cooldown, min_lr, eps, warmup_epochs, multiplier
        self.best, self.num_bad, self.cooldown_left = math.inf, 0, 0
        if warmup_epochs > 0:
            self.epoch, self.lr = 1, warmup(1, base_lr, multiplier, warmup_epochs)
        else:
            self.epoch, self.lr = 0, base_lr

    def tick(self, metric):
        """metric: the fp32 value the device word holds (None: nothing to observe).  -> the rate"""
        self.epoch += 1
        if self.warmup_epochs > 0 and self.epoch <= self.warmup_epochs:
            self.lr = warmup(self.epoch, self.base_lr, self.multiplier, self.warmup_epochs)
            return self.lr
        if metric is None:
            return self.lr
        a = float(metric)
        if a < self.best * (1.0 - self.threshold):
            self.best, self.num_bad = a, 0
        else:
            self.num_bad += 1
        if self.cooldown_left > 0:
            self.cooldown_left -= 1
            self.num_bad = 0
        if self.num_bad > self.patience:
            new = max(self.lr * self.factor, self.min_lr)
            if self.lr - new > self.eps:
                self.lr = new
            self.cooldown_left = self.cooldown
            self.num_bad = 0
        return self.lr


def rate(kind, args, e):
    """The closed forms by the fixture's kind name."""
    return {"stepexp": stepexp, "exp": exp, "gradual": gradual}[kind](e, **args)


def follow_epoch(epoch, counter, cap):
    """The epoch a FOLLOW launch leaves."""
    c = min(counter, cap) if cap >= 0 else counter
    return c if c != epoch else epoch


def group_word(lr, scale):
    """The lr word of a group row: the product in double from the unrounded rate, one rounding to fp32."""
    return f32(lr * scale)
