"""Training guard: clip by global norm and leave bad steps out, decided on the device (include/gfv.h gfv_grad_guard_dev,
DESIGN.md 5f).  `GradGuard` owns the device record `guard[8]`, the segment table of the gradient elements torch would see and
the norm launch's workspace; the launches that read them are issued by `gfv.optstep.optimizer_launches`.  The policy is three
plain host values mirrored into `guard` on change (as `lr` is into `hyper`): nothing a recorded launch list or a captured graph
holds depends on them."""
from __future__ import annotations

import math
import struct

import torch

from . import lib as L


def check_policy(max_grad_norm, skip_on_flag=False, dist_on=False):
    """The constructor checks shared by every owner of a guard; needs no GPU."""
    if max_grad_norm is not None:
        v = float(max_grad_norm)
        if math.isnan(v) or v <= 0.0:
            raise ValueError(f"max_grad_norm must be a positive number or None, got {max_grad_norm!r}")
    if skip_on_flag and dist_on:
        raise ValueError("skip_on_flag with a data-parallel step: the device status word is rank-local, the ranks would "
                         "disagree on whether the step is applied")


def segments(store, exclude=()):
    """(offset, count) of every run of gradient elements of `store` (a gfv.engine.GradStore) that belongs to a used parameter:
    no alignment padding, no parameter of `store.skip` or of `exclude` (frozen parameters: torch's clip_grad_norm_ would not see
    them); neighbours without a gap are merged."""
    segs = []
    for n, off in store.off.items():
        k = store.numel(n)
        if n in store.skip or n in exclude or k == 0:
            continue
        if segs and segs[-1][0] + segs[-1][1] == off:
            segs[-1][1] += k
        else:
            segs.append([off, k])
    return [(int(o), int(k)) for o, k in segs]


class GradGuard:
    FIELDS = ("norm", "coef", "decision", "clipped", "skipped_nonfinite", "skipped_flag")

    def __init__(self, store, device, max_grad_norm=None, skip_nonfinite=False, skip_on_flag=False):
        self.device = device
        self.set_segments(store)
        self.guard = torch.zeros(8, dtype=torch.float32, device=device)
        ws = int(L.load(raw=True).gfv_grad_guard_workspace_bytes())
        self.ws = torch.zeros((ws + 7) // 8, dtype=torch.float64, device=device)
        self._host = None
        self.set(max_grad_norm, skip_nonfinite, skip_on_flag)

    def set_segments(self, store, exclude=()):
        """The segment table of `store` without the parameters of `exclude`.  A NEW table: the owner drops its recorded lists and
        captured graphs (they hold the old one's address and length)."""
        segs = segments(store, exclude)
        if not segs:
            raise ValueError("no parameter with a gradient: nothing to guard")
        self.n_seg, self.n_elems = len(segs), sum(k for _, k in segs)
        self.segs = torch.tensor(segs, dtype=torch.int64).reshape(-1).to(self.device)

    def set(self, max_grad_norm, skip_nonfinite, skip_on_flag):
        self.max_grad_norm = None if max_grad_norm is None else float(max_grad_norm)
        self.skip_nonfinite, self.skip_on_flag = bool(skip_nonfinite), bool(skip_on_flag)
        policy = ((L.GUARD_CLIP if self.max_grad_norm is not None else 0) | (L.GUARD_SKIP_NONFINITE if self.skip_nonfinite else 0)
                  | (L.GUARD_SKIP_FLAG if self.skip_on_flag else 0))
        vals = (self.max_grad_norm or 0.0, policy)
        if vals != self._host:
            bits = struct.unpack("i", struct.pack("f", vals[0]))[0]
            self.guard.view(torch.int32)[0:2].copy_(torch.tensor([bits, policy], dtype=torch.int32))
            self._host = vals
        self.active = policy != 0

    def stats(self):
        """What the last guarded step decided and the running counts (synchronises: for logging every so often)."""
        rec = self.guard.detach().cpu()
        ints = rec.view(torch.int32)
        return {"norm": float(rec[2]), "coef": float(rec[3]), "decision": int(ints[4]), "clipped": int(ints[5]),
                "skipped_nonfinite": int(ints[6]), "skipped_flag": int(ints[7])}
