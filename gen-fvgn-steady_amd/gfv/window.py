"""The sampling window: which fields of a run a sampler (`FieldStats`, `WallForces`, `FlowIntegrals`, `Probes`; gfv/follow.py) takes.

The clock counts fields written: the field the first step (the first completed level) leaves has clock 1; clock 0 is the initial
state, which is never sampled (`start` is at least 1).  A clock value is sampled when `start <= clock < stop` and
`(clock - start) % stride == 0`, once.  The decision is the device's (csrc/gfv_window.h), from the 8-word record of include/gfv.h
(GFV_WINDOW_RECORD) as the launch finds it.  `Window` owns the host words and, once attached, the device record.
"""
from __future__ import annotations

import numbers

import torch

from . import lib as L

# words of the record (include/gfv.h GFV_WINDOW_RECORD)
START, STRIDE, STOP, LAST, N_SAMPLES, COUNTER, ENABLED = range(7)
NO_STOP = -1    # a negative stop is no stop
UNCHANGED = object()    # set(stop=): None already means "no end"


def check_window_args(start=1, stride=1, stop=None, enabled=True):
    """The window's checks; needs no GPU.  -> (start, stride, stop, enabled) as the record's words, stop None as NO_STOP."""
    for name, v in (("start", start), ("stride", stride)) + ((("stop", stop),) if stop is not None else ()):
        if isinstance(v, bool) or not isinstance(v, numbers.Integral):
            raise ValueError(f"{name} must be an integer, got {v!r}")
        if v >= 2 ** 31:
            raise ValueError(f"{name} must be below 2^31, got {v!r}")
    if start < 1:
        # clock 0 is the INITIAL state: a MarchStep's level word is 0 until its first level ends, so start = 0 would sample the
        # field nobody has advanced yet (a Rollout's launch never sees clock 0)
        raise ValueError(f"start must be at least 1 (the first field written has clock 1; clock 0 is the initial state), got {start}")
    if stride < 1:
        raise ValueError(f"stride must be at least 1, got {stride}")
    if stop is not None and stop < 0:
        raise ValueError(f"stop must be None (no end) or at least 0 (exclusive), got {stop}")
    if not isinstance(enabled, (bool, numbers.Integral)):
        raise ValueError(f"enabled must be a bool, got {enabled!r}")
    return int(start), int(stride), NO_STOP if stop is None else int(stop), 1 if enabled else 0


class Window:
    def __init__(self, start=1, stride=1, stop=None):
        self._words = check_window_args(start, stride, stop, True)
        self.rec = None                               # the device record: allocated by attach(), never reallocated

    start = property(lambda self: self._words[0])
    stride = property(lambda self: self._words[1])
    stop = property(lambda self: None if self._words[2] < 0 else self._words[2])
    enabled = property(lambda self: bool(self._words[3]))

    def attach(self, dev):
        """Allocates the record on `dev` (once), writes the host words and starts over.  -> the record"""
        self.rec = torch.zeros(L.WINDOW_RECORD, dtype=torch.int32, device=dev)
        self.write()
        self.reset()
        return self.rec

    def write(self):
        """The host-written words into the record, in stream order (the other words are the device's and stay)."""
        w = self._words
        self.rec[START:STOP + 1].copy_(torch.tensor(w[0:3], dtype=torch.int32))
        self.rec[ENABLED:ENABLED + 1].copy_(torch.tensor(w[3:4], dtype=torch.int32))

    def set(self, start=None, stride=None, stop=UNCHANGED, enabled=None):
        """A new window (None: unchanged; `stop=None` removes the end, leaving `stop` out keeps it), checked before anything
        changes.  It reaches recorded lists through the device record, from the next step issued: nothing is recorded again."""
        w = self._words
        self._words = check_window_args(w[0] if start is None else start, w[1] if stride is None else stride,
                                        self.stop if stop is UNCHANGED else stop, bool(w[3]) if enabled is None else enabled)
        if self.rec is not None:
            self.write()

    def reset(self):
        """Start over: last = -1, n = 0, in stream order (the next launch finds a clock it has not seen)."""
        self.rec[LAST:N_SAMPLES + 1].copy_(torch.tensor([-1, 0], dtype=torch.int32))

    def count(self):
        """Samples taken so far (one synchronisation)."""
        return int(self.rec[N_SAMPLES:N_SAMPLES + 1].cpu()[0])
