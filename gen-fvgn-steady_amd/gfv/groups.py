"""Parameter groups of the fused Adam: a learning rate, a weight decay and a "leave this alone" per group of parameter tensors,
inside the one Adam launch (include/gfv.h gfv_adam_step_groups_dev).

Host side, most of it without a GPU: the selectors that say which parameter belongs to which group (`assign`), the checks every
owner runs at construction (`check_groups` -> a `GroupSpec`), the run table of a flat layout (`build_runs`) and `ParamGroups`,
the owner of the two device tables - run table and group table - which mirrors host values into them on change, as `_sync_hyper`
does for `hyper`.  `gfv.trainer.TrainStep`, `gfv.pool_trainer.PoolTrainStep` and `gfv.optim.Adam` / `AdamW` hand it to
`gfv.optstep.optimizer_launches` once a group feature is in use; with everything at its default none of this is touched.

One deviation from torch: the step count is shared.  torch counts steps per parameter, so a group unfrozen after k steps starts
its bias correction at 1 there; here it continues with the shared count k + 1 and the moments it has (zero if it never moved)."""
from __future__ import annotations

import math
import numbers
import struct

import torch

from . import lib as L

MAX_GROUPS = L.MAX_PARAM_GROUPS   # rows a caller may use; row MAX_GROUPS of the device table is reserved and always frozen
RESERVED = MAX_GROUPS
FROZEN = L.GROUP_FROZEN
GROUP_KEYS = ("params", "lr_scale", "weight_decay", "frozen")


def _f32(x):
    return struct.unpack("f", struct.pack("f", float(x)))[0]


def _check_number(what, v, allow_none=False):
    if v is None and allow_none:
        return None
    if isinstance(v, bool) or not isinstance(v, numbers.Real) or math.isnan(v) or math.isinf(v) or v < 0:
        raise ValueError(f"{what} must be a finite number >= 0, got {v!r}")
    return float(v)


def check_weight_decay(v):
    return _check_number("weight_decay", v)


def select(names, tensors, selector):
    """The names a group's `"params"` selects: a list of strings - each selects the parameter of that name and every parameter
    whose name starts with it plus "." - or a callable (name, tensor) -> bool.  A string that selects nothing is an error."""
    if callable(selector):
        return [n for n, t in zip(names, tensors) if selector(n, t)]
    if isinstance(selector, str):
        selector = [selector]
    chosen = set()
    for s in selector:
        if not isinstance(s, str):
            raise TypeError(f'a group\'s "params" is a list of names / prefixes or a callable, got an entry {s!r}')
        hit = [n for n in names if n == s or n.startswith(s + ".")]
        if not hit:
            raise ValueError(f"parameter group selector {s!r} selects no parameter")
        chosen.update(hit)
    return [n for n in names if n in chosen]


def no_decay_names(model):
    """Every bias and every 1-D tensor of `model` - LayerNorm weight / bias, and the attention temperatures, which are vectors
    stored with broadcast axes of length 1 ((1, heads, 1, 1): at most one axis longer than 1 counts as 1-D).  What the usual recipe
    keeps out of the weight decay: `param_groups=[{"params": no_decay_names(model), "weight_decay": 0.0}]`."""
    return [n for n, p in model.named_parameters()
            if sum(1 for d in p.shape if d > 1) <= 1 or n == "bias" or n.endswith(".bias")]


class GroupSpec:
    """The groups of one owner on the host: per group its parameter names, lr_scale, weight_decay (None: the owner's) and frozen;
    `group_of[name]` -> index.  Groups given by the caller come first, in their order; the parameters no group selects form an
    implicit default group behind them (lr_scale 1, the owner's weight_decay, not frozen)."""

    def __init__(self, names, groups, weight_decay, decoupled):
        self.names = list(names)
        self.groups = groups
        self.weight_decay = weight_decay
        self.decoupled = bool(decoupled)
        self.group_of = {n: i for i, g in enumerate(groups) for n in g["names"]}
        self.skip = set()   # names that never receive a gradient (the owner's GradStore.skip): they do not count as live

    def check_some_live(self, frozen):
        """`frozen`: a flag per group.  Raises if no parameter with a gradient would be left to move."""
        if not any(n not in self.skip for g, fr in zip(self.groups, frozen) if not fr for n in g["names"]):
            raise ValueError("every parameter group with a gradient would be frozen: nothing left to optimise")

    @property
    def trivial(self):
        """One group, no decay, nothing frozen, the owner's own rate: the plain Adam launch computes it."""
        return (len(self.groups) == 1 and self.wd(0) == 0.0 and not self.groups[0]["frozen"]
                and self.groups[0]["lr_scale"] == 1.0)

    def wd(self, i):
        w = self.groups[i]["weight_decay"]
        return self.weight_decay if w is None else w

    def values(self, lr):
        """[(lr, weight_decay, frozen)] per group for the owner's rate `lr`."""
        return [(float(lr) * g["lr_scale"], self.wd(i), g["frozen"]) for i, g in enumerate(self.groups)]

    def frozen_names(self):
        return {n for g in self.groups if g["frozen"] for n in g["names"]}

    def public(self, lr):
        return [{"params": list(g["names"]), "lr": float(lr) * g["lr_scale"], "lr_scale": g["lr_scale"], "weight_decay": self.wd(i),
                 "frozen": g["frozen"]} for i, g in enumerate(self.groups)]

    def set_group(self, i, lr_scale=None, weight_decay=None, frozen=None):
        """New values for group i (None: unchanged).  Everything is checked before anything is changed.  -> True if `frozen`
        changed."""
        g = self.groups[i]
        lr_scale = _check_number("lr_scale", lr_scale, allow_none=True)
        weight_decay = _check_number("weight_decay", weight_decay, allow_none=True)
        moved = frozen is not None and bool(frozen) != g["frozen"]
        if moved:
            self.check_some_live([bool(frozen) if k == i else h["frozen"] for k, h in enumerate(self.groups)])
        if lr_scale is not None:
            g["lr_scale"] = lr_scale
        if weight_decay is not None:
            g["weight_decay"] = weight_decay
        if moved:
            g["frozen"] = bool(frozen)
        return moved


def check_groups(names, tensors, weight_decay=0.0, decoupled_weight_decay=True, param_groups=None):
    """The constructor check shared by the step objects; needs no GPU.  -> GroupSpec.
    Refused: a negative / non-finite weight_decay or lr_scale, an unknown group key, a parameter selected by two groups, a string
    that selects nothing, more than MAX_GROUPS groups (the implicit default group included)."""
    weight_decay = _check_number("weight_decay", weight_decay)
    groups, taken = [], {}
    for gi, pg in enumerate(param_groups or []):
        if not isinstance(pg, dict) or "params" not in pg:
            raise TypeError(f'parameter group {gi}: a dict with a "params" selector')
        unknown = set(pg) - set(GROUP_KEYS)
        if unknown:
            raise ValueError(f"parameter group {gi}: unknown keys {sorted(unknown)} (known: {list(GROUP_KEYS)})")
        chosen = select(names, tensors, pg["params"])
        for n in chosen:
            if n in taken:
                raise ValueError(f"parameter {n!r} is selected by groups {taken[n]} and {gi}")
            taken[n] = gi
        groups.append({"names": chosen, "lr_scale": _check_number("lr_scale", pg.get("lr_scale", 1.0)),
                       "weight_decay": _check_number("weight_decay", pg.get("weight_decay"), allow_none=True),
                       "frozen": bool(pg.get("frozen", False))})
    rest = [n for n in names if n not in taken]
    if rest or not groups:
        groups.append({"names": rest, "lr_scale": 1.0, "weight_decay": None, "frozen": False})
    if len(groups) > MAX_GROUPS:
        raise ValueError(f"{len(groups)} parameter groups (the implicit default group included): at most {MAX_GROUPS}")
    return GroupSpec(names, groups, weight_decay, decoupled_weight_decay)


def build_runs(store, assignment):
    """The run table of `store` (a gfv.engine.GradStore): (starts, rows) - one run per tensor in layout order, starts ascending
    and closed by store.total (a tensor's alignment padding belongs to its run), rows[r] = assignment[name], or RESERVED for a
    parameter of store.skip (it never receives a gradient)."""
    starts, rows = [], []
    for n, off in store.off.items():
        starts.append(int(off))
        rows.append(RESERVED if n in store.skip else int(assignment[n]))
    if not starts or starts[0] != 0:
        raise ValueError("the flat layout does not start at 0")
    if any(not 0 <= r <= RESERVED for r in rows):
        raise ValueError("group index outside the table")
    starts.append(int(store.total))
    return starts, rows


class ParamGroups:
    """Owner of the device tables of gfv_adam_step_groups_dev: `run_start` (int64, runs + 1), `run_group` (int32, runs) and `table`
    ((MAX_GROUPS + 2) rows of 8 words: header, the groups, the reserved frozen row).  The number of runs is fixed; `set_rows`
    rewrites group indices in place, `sync` the group rows and the header - nothing a recorded list holds depends on either."""

    def __init__(self, store, device, assignment, values, decoupled):
        starts, rows = build_runs(store, assignment)
        if len(rows) > L.MAX_PARAM_RUNS:
            raise ValueError(f"{len(rows)} parameter tensors: the grouped Adam launch takes at most {L.MAX_PARAM_RUNS} runs "
                             "(GFV_MAX_PARAM_RUNS, include/gfv.h)")
        self.n_runs = len(rows)
        self.names = list(store.off)
        self._home = list(rows)                      # the group of every run when it has a gradient
        self._rows = list(rows)
        self.run_start = torch.tensor(starts, dtype=torch.int64).to(device)
        self.run_group = torch.tensor(rows, dtype=torch.int32).to(device)
        self.table = torch.zeros((MAX_GROUPS + 2) * 8, dtype=torch.float32, device=device)
        self._host = None
        self.sync(values, decoupled)

    def sync(self, values, decoupled):
        """values: [(lr, weight_decay, frozen)] per group.  Written on change."""
        vals = (tuple((_f32(lr), _f32(wd), bool(fr)) for lr, wd, fr in values), bool(decoupled))
        if vals == self._host:
            return
        if len(vals[0]) > MAX_GROUPS:
            raise ValueError(f"{len(vals[0])} parameter groups: at most {MAX_GROUPS}")
        host = torch.zeros((MAX_GROUPS + 2) * 8, dtype=torch.float32)
        ints = host.view(torch.int32)
        ints[0], ints[1] = len(vals[0]), int(vals[1])
        for k, (lr, wd, fr) in enumerate(vals[0]):
            host[8 * (1 + k)], host[8 * (1 + k) + 1] = lr, wd
            ints[8 * (1 + k) + 2] = FROZEN if fr else 0
        ints[8 * (1 + RESERVED) + 2] = FROZEN
        self.table.copy_(host)
        self._host = vals

    def set_rows(self, without_gradient=()):
        """Point the runs at positions `without_gradient` at the reserved frozen row, every other one at its own group."""
        gone = set(without_gradient)
        rows = [RESERVED if i in gone else h for i, h in enumerate(self._home)]
        if rows != self._rows:
            self.run_group.copy_(torch.tensor(rows, dtype=torch.int32))
            self._rows = rows
