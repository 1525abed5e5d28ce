"""Field statistics: the time mean and the fluctuations of a run, kept on the device.

For an unsteady case the step history is not what the user wants: they want the time-averaged field, the variances, the Reynolds
shear stress u'v' and the extremes, over a window that starts after the transient.  `Rollout` and `MarchStep` exist so that the
host never synchronises per step; `FieldStats` is one small launch behind the launch that advances the field
(`gfv_field_stats_update`, csrc/fieldstats.hip, include/gfv.h), following the owner's clock - `Rollout`'s step counter,
`MarchStep`'s level count - the way a FOLLOW schedule does:

    fs = FieldStats(start=200, stride=2)                   # sample the fields of steps 200, 202, ... (the first step is 1)
    r = Rollout(model, graphs, max_steps=1000, field_stats=fs)
    r.run(steps=1000)
    s = fs.read()                                          # n, mean [N,3], var [N,3], cov_uv [N], min [N,3], max [N,3]
    fs.set_window(stride=1)                                # recorded lists follow it: nothing is recorded again
    ms = MarchStep(model, graphs, ..., field_stats=FieldStats(start=1))   # one sample per completed level (the first is 1)

Which fields are sampled: gfv/window.py (a `MarchStep` step that does not end a level, or is held, leaves the clock as it is and
samples nothing).  How the object is handed over, attached and launched: gfv/follow.py.

What is kept, per node and channel: the shift K (the first sample), S1 = sum (x - K), S2 = sum (x - K)^2 and sum (u - Ku)(v - Kv)
in float64, the minimum and the maximum.  Shifted by the first sample the sums are of the size of the fluctuation, so a mean a
thousand times the fluctuation costs no digits.  No floating-point atomics, no sum across nodes: the same run gives the same
bits.

Who owns what a recorded list points at: DESIGN.md 5l.  Particular to this object, allocated once when its owner attaches it and
never reallocated: the record, the sums and the shift / extremes.  One owner per object.  The statistics are not part of any
`state_dict()`.
"""
from __future__ import annotations

import torch

from . import lib as L
from .follow import Follower
from .window import (COUNTER, ENABLED, LAST, N_SAMPLES, NO_STOP, START, STOP, STRIDE, UNCHANGED, Window,  # noqa: F401  (re-exports)
                     check_window_args as check_field_stats_args)


def check_field(x_backup):
    """The field tensor an owner attaches: a contiguous float32 [N, 12] device tensor.  -> N"""
    if not isinstance(x_backup, torch.Tensor) or x_backup.dim() != 2 or x_backup.shape[1] != 12 or x_backup.shape[0] < 1:
        raise ValueError("FieldStats: the node state must be a [N, 12] tensor")
    if x_backup.dtype != torch.float32 or not x_backup.is_contiguous():
        raise ValueError("FieldStats: the node state must be contiguous float32")
    if not x_backup.is_cuda:
        raise ValueError("FieldStats: the node state must live on the GPU (the statistics are kept by a HIP kernel; there is no "
                         "CPU path)")
    return int(x_backup.shape[0])


def moments(n, sums, aux):
    """The statistics from the raw state (CPU tensors: sums float64 [7, N], aux float32 [9, N]) in float64 -> a dict."""
    if n < 1:
        raise RuntimeError("FieldStats: no sample has been taken yet (n == 0): nothing to read")
    s, a = sums.to(torch.float64), aux.to(torch.float64)
    m1 = s[0:3] / n                                              # [3, N]: the mean of x - K
    mean = a[0:3] + m1
    var = s[3:6] / n - m1 * m1
    cov_uv = s[6] / n - m1[0] * m1[1]
    return {"n": int(n), "mean": mean.t().contiguous(), "var": var.t().contiguous(), "cov_uv": cov_uv.contiguous(),
            "min": aux[3:6].t().contiguous(), "max": aux[6:9].t().contiguous()}


class FieldStats(Follower):
    KEYWORD = "field_stats"
    NO_ANDERSON = "their mean and variance are not the flow's"

    def __init__(self, start=1, stride=1, stop=None):
        self._window = Window(start, stride, stop)
        self.rec = self.sums = self.aux = None        # device state: allocated by attach(), never reallocated
        self.N = 0

    start = property(lambda self: self._window.start)
    stride = property(lambda self: self._window.stride)
    stop = property(lambda self: self._window.stop)
    enabled = property(lambda self: self._window.enabled)

    # ---- the owner's side (gfv/follow.py) -------------------------------------------------------------------------------------
    def attach(self, owner, x_backup, clock, clock_word=0):
        """Called by the owner's constructor with the tensor it advances, its int32 record `clock` and the word of it that counts
        the fields written: allocates the record and the state (once).  -> self"""
        self.check_free()
        n = check_field(x_backup)
        dev = x_backup.device
        sums = torch.zeros((L.FIELD_STATS_SUMS, n), dtype=torch.float64, device=dev)
        aux = torch.zeros((L.FIELD_STATS_AUX, n), dtype=torch.float32, device=dev)
        self._xb, self._clock, self._clock_ptr = x_backup, clock, clock.data_ptr() + 4 * int(clock_word)
        self.N, self.rec, self.sums, self.aux = n, self._window.attach(dev), sums, aux
        self._claim(owner)
        return self

    def launch(self):
        """The one launch, behind the owner's advance: part of the step body (eager steps and recorded lists carry it alike)."""
        L.check(L.load().gfv_field_stats_update(self._xb.data_ptr(), self.N, self._clock_ptr, self.rec.data_ptr(),
                                                self.sums.data_ptr(), self.aux.data_ptr(), L.stream_ptr()), "gfv_field_stats_update")

    def set_window(self, start=None, stride=None, stop=UNCHANGED, enabled=None):
        """`Window.set`: a new window under recorded lists.  The statistics so far stay: reset() starts over."""
        self._window.set(start, stride, stop, enabled)

    def reset(self):
        """`Window.reset`; the owner's reset() calls it.  The sums need no clearing (the first sample writes every element)."""
        self._need()
        self._window.reset()

    # ---- reading (each of these is one synchronisation) ----------------------------------------------------------------------
    def count(self):
        """Samples taken so far."""
        self._need()
        return self._window.count()

    def read(self):
        """{"n", "mean" [N,3], "var" [N,3], "cov_uv" [N], "min" [N,3], "max" [N,3]} as CPU tensors; raises with n == 0.
        mean = K + S1 / n; var = S2 / n - (S1 / n)^2 is the POPULATION variance (divide by n, not n - 1: multiply by n / (n - 1) for
        the sample variance); cov_uv = S2uv / n - (S1u / n)(S1v / n) is the Reynolds shear stress u'v' (population form).  Means and
        moments float64, the extremes float32.  A node that met a NaN has NaN moments; its extremes ignore the NaN."""
        self._need()
        n_words = L.FIELD_STATS_RECORD
        # one device-to-host copy of everything (one synchronisation): the three tensors packed as bytes
        packed = torch.cat([self.rec.view(torch.uint8), self.sums.view(torch.uint8).reshape(-1),
                            self.aux.view(torch.uint8).reshape(-1)]).cpu()
        rec = packed[:4 * n_words].view(torch.int32)
        nb = 8 * L.FIELD_STATS_SUMS * self.N
        sums = packed[4 * n_words:4 * n_words + nb].view(torch.float64).reshape(L.FIELD_STATS_SUMS, self.N)
        aux = packed[4 * n_words + nb:].view(torch.float32).reshape(L.FIELD_STATS_AUX, self.N)
        return moments(int(rec[N_SAMPLES]), sums, aux)

    def raw(self):
        """(record [8] int32, sums [7, N] float64, aux [9, N] float32) as CPU copies, as the device holds them (synchronises)."""
        self._need()
        return self.rec.cpu(), self.sums.cpu(), self.aux.cpu()
