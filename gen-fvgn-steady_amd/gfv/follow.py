"""Followers of a run's clock: what the five followers - `FieldStats`, `WallForces`, `Probes`, `TimeBC` and `TimeScheme` - share
(DESIGN.md 5l), and a sixth, `FlowIntegrals` (keyword `integrals`), with them.

A follower is handed to an owner (`Rollout`, `MarchStep`; `TrainStep` for a `TimeScheme`) by keyword; its launches sit behind the
owner's advance launch, in the step body, and read a clock word that launch writes.  The protocol: the owner's constructor calls
`check_followers` before it touches a device and each follower's own `attach(owner, ...)` LAST; `attach` binds the clock (the
owner's int32 record and the word of it that counts the fields written: the tensor is kept alive, the word's address stored), so
`launch()` and `reset()` take no argument; the owner keeps its followers in `_followers`, in the order field_stats, wall_forces, integrals,
probes, time_bc, time_scheme, and loops over it in its step body and in its `reset()`.  One owner per follower.  A follower holds NO strong
reference to its owner, only the owner's class name (a reference back would tie the two into a cycle and keep the owner's recorded
lists, and a MarchStep's pinned mirror, alive until a garbage collection), and the claim is `attach`'s last statement: an attach
that raised leaves the follower free.  `keyword=None` issues no launch and allocates nothing.
"""
from __future__ import annotations


class Follower:
    KEYWORD = None                       # the keyword an owner is handed it by
    OWNERS = ("Rollout", "MarchStep")    # who takes one: named by the "not attached" message
    NO_ANDERSON = None                   # why an owner with anderson > 0 refuses it (None: it does not)
    rec = None                           # every follower has a device record, allocated by attach()
    _owner = None                        # the owner's class name once attached

    def check_free(self):
        """Needs no GPU: an owner's constructor calls it before it looks at anything else."""
        if self._owner is not None:
            raise ValueError(f"this {type(self).__name__} is already attached to a {self._owner} (one owner per object)")

    def _need(self):
        if self.rec is None:
            hand = " or ".join(f"{o}(..., {self.KEYWORD}=)" for o in self.OWNERS)
            raise RuntimeError(f"this {type(self).__name__} is not attached yet: hand it to {hand}")

    def _claim(self, owner):                # attach()'s last statement; owner: the owning object, or a plain name
        self._owner = owner if isinstance(owner, str) else type(owner).__name__

    def _check_graphs(self, graphs):        # what the class refuses of an owner's graphs; needs no GPU
        pass

    @classmethod
    def check_handed(cls, who, obj, graphs=None, anderson=0):
        """What an owner `who` refuses of `KEYWORD=obj`, in this order: the type, a follower that is taken, `anderson` > 0, the
        class's own check of the graphs.  Needs no GPU."""
        if obj is None:
            return
        at = f"{who}: " if who else ""
        if not isinstance(obj, cls):
            raise ValueError(f"{at}{cls.KEYWORD} must be a {cls.__module__}.{cls.__name__} or None, got {obj!r}")
        obj.check_free()
        if anderson and cls.NO_ANDERSON:
            raise ValueError(f"{at}anderson > 0 together with {cls.KEYWORD} is not supported (accelerated iterates are not time "
                             f"steps of the model: {cls.NO_ANDERSON})")
        if graphs is not None:
            obj._check_graphs(graphs)


def check_followers(who, graphs, anderson, field_stats=None, wall_forces=None, time_bc=None, time_scheme=None, integrals=None,
                    probes=None):
    """An owner's one check of the followers it is handed, before any device is touched; the order is the launch order."""
    from . import fieldstats as F, integrals as I, probes as P, timebc as B, timescheme as S, wallforce as W
    for cls, obj in ((F.FieldStats, field_stats), (W.WallForces, wall_forces), (I.FlowIntegrals, integrals), (P.Probes, probes),
                     (B.TimeBC, time_bc), (S.TimeScheme, time_scheme)):
        cls.check_handed(who, obj, graphs, anderson)
