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

The clock counts fields written: the field the first step (the first completed level) leaves has clock 1; clock 0 is the initial
state, which is never sampled (`start` is at least 1).  A clock value is
sampled when `start <= clock < stop` and `(clock - start) % stride == 0`, once (a `MarchStep` step that does not end a level, or
is held, leaves the clock as it is and samples nothing).

What is kept, per node and channel: the shift K (the first sample), S1 = sum (x - K), S2 = sum (x - K)^2 and sum (u - Ku)(v - Kv)
in float64, the minimum and the maximum.  Shifted by the first sample the sums are of the size of the fluctuation, so a mean a
thousand times the fluctuation costs no digits.  No floating-point atomics, no sum across nodes: the same run gives the same
bits.

Who owns what a recorded list points at: DESIGN.md 5l.  Particular to this object, allocated once when its owner attaches it and
never reallocated: the record, the sums and the shift / extremes.  One owner per object.  The statistics are not part of any
`state_dict()`.
"""
from __future__ import annotations

import numbers

import torch

from . import lib as L

# words of the record (include/gfv.h gfv_field_stats_update)
START, STRIDE, STOP, LAST, N_SAMPLES, COUNTER, ENABLED = range(7)
NO_STOP = -1    # a negative stop is no stop
UNCHANGED = object()    # set_window(stop=): None already means "no end"


def check_field_stats_args(start=1, stride=1, stop=None, enabled=True):
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


class FieldStats:
    def __init__(self, start=1, stride=1, stop=None):
        self._window = check_field_stats_args(start, stride, stop, True)
        self.rec = self.sums = self.aux = None        # device state: allocated by attach(), never reallocated
        self._owner = None                            # the owner's class name once attached - NOT the owner: a reference back
        self.N = 0                                    # would tie the two into a cycle and keep the owner's recorded lists (and
                                                      # a MarchStep's pinned mirror) alive until a garbage collection

    start = property(lambda self: self._window[0])
    stride = property(lambda self: self._window[1])
    stop = property(lambda self: None if self._window[2] < 0 else self._window[2])
    enabled = property(lambda self: bool(self._window[3]))

    # ---- the owner's side -------------------------------------------------------------------------------------------------------
    def check_free(self):
        """Needs no GPU: an owner's constructor calls it before it looks at anything else."""
        if self._owner is not None:
            raise ValueError(f"this FieldStats is already attached to a {self._owner} (one owner per object: it follows one "
                             "clock)")

    def attach(self, owner, x_backup):
        """Called by the owner's constructor with the tensor it advances: allocates the record and the state (once).  -> self"""
        self.check_free()
        n = check_field(x_backup)
        dev = x_backup.device
        rec = torch.zeros(L.FIELD_STATS_RECORD, dtype=torch.int32, device=dev)
        sums = torch.zeros((L.FIELD_STATS_SUMS, n), dtype=torch.float64, device=dev)
        aux = torch.zeros((L.FIELD_STATS_AUX, n), dtype=torch.float32, device=dev)
        self.N, self.rec, self.sums, self.aux = n, rec, sums, aux
        self._write_window()
        self.reset()
        self._owner = type(owner).__name__       # (last: an attach that raised leaves the object free)
        return self

    def launch(self, x_backup, clock_ptr):
        """The one launch, behind the owner's advance: part of the step body (eager steps and recorded lists carry it alike)."""
        L.check(L.load().gfv_field_stats_update(x_backup.data_ptr(), self.N, clock_ptr, self.rec.data_ptr(), self.sums.data_ptr(),
                                                self.aux.data_ptr(), L.stream_ptr()), "gfv_field_stats_update")

    def _need(self):
        if self.rec is None:
            raise RuntimeError("this FieldStats is not attached yet: hand it to Rollout(..., field_stats=) or "
                               "MarchStep(..., field_stats=)")

    # ---- the record's host-written words ---------------------------------------------------------------------------------------
    def _write_window(self):
        w = self._window
        self.rec[START:STOP + 1].copy_(torch.tensor(w[0:3], dtype=torch.int32))
        self.rec[ENABLED:ENABLED + 1].copy_(torch.tensor(w[3:4], dtype=torch.int32))

    def set_window(self, start=None, stride=None, stop=UNCHANGED, enabled=None):
        """A new window (None: unchanged; `stop=None` removes the end, leaving `stop` out keeps it), checked before anything
        changes.  It reaches recorded lists through the device record: nothing is recorded again.  It holds from the next step
        issued.  The statistics so far stay: reset() starts over."""
        w = self._window
        self._window = check_field_stats_args(w[0] if start is None else start, w[1] if stride is None else stride,
                                              self.stop if stop is UNCHANGED else stop, bool(w[3]) if enabled is None else enabled)
        if self.rec is not None:
            self._write_window()

    def reset(self):
        """Start over: last = -1, n = 0, in stream order.  The sums need no clearing (the first sample writes every element).  The
        owner's reset() calls it; called alone, the next launch finds a clock it has not seen and samples it if the window holds."""
        self._need()
        self.rec[LAST:N_SAMPLES + 1].copy_(torch.tensor([-1, 0], dtype=torch.int32))

    # ---- reading (each of these is one synchronisation) ----------------------------------------------------------------------
    def count(self):
        """Samples taken so far."""
        self._need()
        return int(self.rec[N_SAMPLES:N_SAMPLES + 1].cpu()[0])

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
