"""Loss balancing: the weights of the three residual terms adapted on the device (include/gfv.h gfv_loss_balance,
csrc/balance.hip).

The training objective is `mean_b log(w_press * press_b + w_cont * cont_b + w_mom * (mom_x_b + mom_y_b))`.  The reference ships
the three weights as hand-tuned constants (`loss_cont 6e4`, `loss_mom 5e4`, `loss_press 1`, utils/get_param.py:59-61), right
for the meshes and the Reynolds range they were tuned on.  Here the weights live in device memory (`hyper[5:8]`, read by the loss
launch, its gradient and the march) and the host no longer sees a step's terms, so balancing them is a device record plus one
small launch per step, behind the step's optimiser launches, that writes the weights where they are read:

    ts = TrainStep(model, graphs, balance=Inverse())                      # every class an equal share of the base residual
    ts = PoolTrainStep(model, pool, balance=Inverse(shares=(2, 1, 1)))    # continuity twice the share of the others
    ts = TrainStep(model, graphs, balance=Progress(alpha=0.9, tau=1.0))   # weight follows the terms that fall most slowly
    ts.balance.stats()                                                    # n, n_applied, n_updates, n_skipped, weights, ema, last

`Inverse` is magnitude normalisation: after a publish class k contributes the share `g_k / sum(g)` of the residual the base
weights would give, so the level of the objective stays comparable with an unbalanced run.  `Progress` is the deterministic form of
ReLoBRaLo (Bischof and Kraus) without its random look-back: `w_k = w0_k * lam_k` with `sum(lam) == 3`.  The base weights `w0` are
the owner's `loss_weights`.  What the record holds and the rule, operation by operation: include/gfv.h.

Argument checks need no GPU.  Each object owns its device record, allocated once (`to(device)`; a step object does it when the
balancer is attached), never reallocated.  A balancer belongs to one step object.  Host-written words are written here, in stream
order.  The launch is issued eagerly behind every step and is never part of a recorded list or a captured graph (`losses` differs
per recorded list, B per pool batch: the rule of the training log's launches)."""
from __future__ import annotations

import torch

from . import lib as L
from .schedule import _int, _real

# 32-bit words / doubles of the record (include/gfv.h gfv_loss_balance)
W_KIND, W_WARMUP, W_EVERY, W_N, W_N_APPLIED, W_N_UPDATES, W_N_SKIPPED = range(7)
D_DECAY, D_FLOOR, D_ALPHA, D_TAU = 4, 5, 6, 7
D_G, D_W0, D_POWER, D_M, D_S, D_SREF, D_LAM, D_W = 8, 11, 14, 15, 18, 21, 24, 27
CLASSES = ("cont", "mom", "press")          # the order of hyper[5], hyper[6], hyper[7]

_STATE_WORDS = (("n", W_N), ("n_applied", W_N_APPLIED), ("n_updates", W_N_UPDATES), ("n_skipped", W_N_SKIPPED))
_STATE_TRIPLES = (("w0", D_W0), ("ema", D_M), ("last", D_S), ("s_ref", D_SREF), ("lam", D_LAM), ("weights", D_W))


def _triple(name, v, lo_open=True):
    v = tuple(v)
    if len(v) != 3:
        raise ValueError(f"{name} must hold three numbers (cont, mom, press), got {v!r}")
    return tuple(_real(f"{name}[{i}]", x, 0.0, lo_open=lo_open) for i, x in enumerate(v))


def _unit(name, v):
    v = _real(name, v, 0.0)
    if v >= 1.0:
        raise ValueError(f"{name} must lie in [0, 1), got {v!r}")
    return v


def state_of(d):
    """The device-written part of a record (and its base weights) as plain Python numbers; `d` a CPU float64 record."""
    w = d.view(torch.int32)
    sd = {k: int(w[i]) for k, i in _STATE_WORDS}
    sd["power"] = float(d[D_POWER])
    sd.update({k: [float(d[i + j]) for j in range(3)] for k, i in _STATE_TRIPLES})
    return sd


def state_into(sd, d):
    """The inverse of state_of: the state's words into the CPU float64 record `d`."""
    w = d.view(torch.int32)
    for k, i in _STATE_WORDS:
        w[i] = int(sd[k])
    d[D_POWER] = float(sd["power"])
    for k, i in _STATE_TRIPLES:
        for j in range(3):
            d[i + j] = float(sd[k][j])
    return d


class Balancer:
    """What the two kinds share: the device record, the launch, the state."""
    KIND = 0

    def __init__(self, decay, warmup, every, floor):
        self.decay = _unit("decay", decay)
        self.warmup = _int("warmup", warmup)
        self.every = _int("every", every, 1)
        self.floor = _real("floor", floor, 0.0, lo_open=True)
        self.base = None          # w0: the owner's loss_weights, or set_base()
        self.rec = None           # device record: GFV_BALANCE_RECORD doubles
        self._own_hyper = None    # hyper[8] of a balancer without an owner
        self._owner = None

    # ---- the record on the host (needs no GPU) ------------------------------------------------------------------------------------
    def _fill(self, d):
        """The kind's host-written doubles into the float64 view `d` of a record."""

    def _need_base(self):
        if self.base is None:
            raise ValueError(f"{type(self).__name__}: the base weights are not known yet (set_base(), or attach the balancer to a "
                             "step object: its loss_weights are the base weights)")
        return self.base

    def pack(self):
        """The record of a new object: a CPU float64 tensor of GFV_BALANCE_RECORD doubles."""
        base = self._need_base()
        d = torch.zeros(L.BALANCE_RECORD, dtype=torch.float64)
        w = d.view(torch.int32)
        w[W_KIND], w[W_WARMUP], w[W_EVERY] = self.KIND, self.warmup, self.every
        d[D_DECAY], d[D_FLOOR], d[D_POWER] = self.decay, self.floor, 1.0
        for k in range(3):
            d[D_G + k], d[D_W0 + k], d[D_LAM + k], d[D_W + k] = 1.0, base[k], 1.0, base[k]
        self._fill(d)
        return d

    # ---- the device side ---------------------------------------------------------------------------------------------------------
    def to(self, device):
        """Allocate the record on `device` (once) and write the new object's words.  -> self"""
        if self.rec is not None:
            dev, mine = torch.device(device), self.rec.device
            if dev.type != mine.type or (dev.index is not None and dev.index != mine.index):
                raise RuntimeError("a balancer's device record is allocated once and stays where it is")
            return self
        host = self.pack()
        self.rec = torch.zeros(L.BALANCE_RECORD, dtype=torch.float64, device=device)
        self._own_hyper = torch.zeros(8, dtype=torch.float32, device=device)
        self.rec.copy_(host)
        self._own_hyper[5:8].copy_(host[D_W:D_W + 3].to(torch.float32))
        return self

    def _attach(self, owner):
        """Called by a step object's constructor: the owner's loss_weights are the base weights."""
        if self._owner is not None and self._owner is not owner:
            raise ValueError("this balancer is already attached to another step object (it owns one set of weights)")
        self.base = _triple("loss_weights", owner.loss_weights, lo_open=False)
        self._owner = owner
        self.to(owner.dev)

    def _hyper(self):
        return self._own_hyper if self._owner is None else self._owner.hyper

    def _need_rec(self):
        if self.rec is None:
            raise RuntimeError("the balancer has no device record yet: to(device), or attach it to a step object")
        return self.rec

    def observe(self, losses, B, hyper=None, hold=None):
        """The launch on its own: observe the terms `losses` [B, 4] (fp32, on the device) of a step and, on a publish, write the
        weights into `hyper[5:8]` (default: the owner's, or this object's own 8 words).  `hold`: a 1-element int32 device tensor
        - the `apply` word of an accumulation record - or None (every step is an applied step)."""
        rec = self._need_rec()
        B = _int("B", B, 1)
        if not (isinstance(losses, torch.Tensor) and losses.is_cuda and losses.dtype == torch.float32 and losses.is_contiguous()
                and losses.numel() >= 4 * B):
            raise ValueError(f"observe: losses must be a contiguous float32 device tensor of at least [B = {B}, 4]")
        hyper = self._hyper() if hyper is None else hyper
        if not (hyper.is_cuda and hyper.dtype == torch.float32 and hyper.is_contiguous() and hyper.numel() >= 8):
            raise ValueError("observe: hyper must be a contiguous float32 device tensor of 8 words")
        if hold is not None and not (isinstance(hold, torch.Tensor) and hold.is_cuda and hold.dtype == torch.int32
                                     and hold.numel() >= 1):
            raise ValueError("observe: hold must be an int32 device tensor (its first word is read)")
        L.check(L.load().gfv_loss_balance(losses.data_ptr(), B, rec.data_ptr(), hyper.data_ptr(),
                                          None if hold is None else hold.data_ptr(), L.stream_ptr()), "gfv_loss_balance")

    def set_base(self, weights):
        """New base weights w0 (host words, written in stream order).  The current weights follow with the next publish."""
        self.base = _triple("weights", weights, lo_open=False)
        if self.rec is not None:
            self.rec[D_W0:D_W0 + 3].copy_(torch.tensor(self.base, dtype=torch.float64))
        if self._owner is not None:
            self._owner._lw = self.base

    def reset(self):
        """Back to a new object's record - counts, average, multipliers - and to the base weights in hyper[5:8]."""
        self._load_record(self.pack())

    def _load_record(self, host):
        self._need_rec().copy_(host)
        self._hyper()[5:8].copy_(host[D_W:D_W + 3].to(torch.float32))

    # ---- reading and restoring (each synchronises once) -----------------------------------------------------------------------
    def stats(self):
        """{"n", "n_applied", "n_updates", "n_skipped", "weights", "ema", "last"} of the device record: accepted observations,
        those behind an applied step, publishes, rejected observations, the current weights (doubles; hyper[5:8] holds them rounded
        to fp32), the moving average and the last accepted statistic per class (cont, mom, press).  Synchronises."""
        sd = state_of(self._need_rec().cpu())
        return {k: sd[k] for k in ("n", "n_applied", "n_updates", "n_skipped", "weights", "ema", "last")}

    def state_dict(self):
        return dict(state_of(self._need_rec().cpu()), kind=type(self).__name__)

    def load_state_dict(self, sd):
        if sd.get("kind") != type(self).__name__:
            raise ValueError(f"the state of a {sd.get('kind')} balancer does not load into a {type(self).__name__}")
        self._need_rec()
        self.base = _triple("w0", sd["w0"], lo_open=False)
        if self._owner is not None:
            self._owner._lw = self.base
        self._load_record(state_into(sd, self.pack()))


def check_balance(balance, dist_on=False, world_size=1, what="TrainStep"):
    """The constructor check of the step objects' `balance=`; needs no GPU."""
    if balance is None:
        return
    if not isinstance(balance, Balancer):
        raise TypeError(f"balance must be a gfv.balance object (Inverse, Progress), got {balance!r}")
    if dist_on or world_size != 1:
        raise ValueError(f"{what}: balance= under data parallelism is not supported (every rank would derive its own weights from "
                         "its own shard)")
    if balance._owner is not None:
        raise ValueError("this balancer is already attached to a step object (it owns one set of weights)")


class Inverse(Balancer):
    """Magnitude normalisation.  On a publish, with mh the bias-corrected moving average of the batch-mean terms:
    `R0 = sum_j w0_j * mh_j`, `w_k = (shares_k / sum(shares)) * R0 / max(mh_k, floor)` - class k then contributes its share of the
    residual the base weights would give.  decay: of the moving average; warmup: observations before the first publish; every:
    publish behind every `every`-th applied step; floor: the smallest average a weight is computed from."""
    KIND = L.BALANCE_INVERSE

    def __init__(self, shares=(1, 1, 1), decay=0.9, warmup=10, every=1, floor=1e-30):
        super().__init__(decay, warmup, every, floor)
        self.shares = _triple("shares", shares)

    def _fill(self, d):
        for k in range(3):
            d[D_G + k] = self.shares[k]


class Progress(Balancer):
    """The deterministic form of ReLoBRaLo (Bischof and Kraus), without its random look-back.  On a publish:
    `rho_k = mh_k / max(s_ref_k, floor)` (the term now against the term at the last publish), `lh = 3 * softmax(rho / tau)`,
    `lam_k = alpha * lam_k + (1 - alpha) * lh_k`, `w_k = w0_k * lam_k`, `s_ref = mh`.  A term that falls more slowly than the others
    gains weight; `sum(lam) == 3` is kept.  alpha: memory of the multipliers; tau: temperature of the softmax."""
    KIND = L.BALANCE_PROGRESS

    def __init__(self, alpha=0.9, tau=1.0, decay=0.9, warmup=10, every=1, floor=1e-30):
        super().__init__(decay, warmup, every, floor)
        self.alpha = _unit("alpha", alpha)
        self.tau = _real("tau", tau, 0.0, lo_open=True)

    def _fill(self, d):
        d[D_ALPHA], d[D_TAU] = self.alpha, self.tau
