"""The recorded-list cache: which launch path a key takes, and which lists are kept.

A key (a batch signature, an `accumulate` value) is issued eagerly `warm` times - steps like any other, which settle the
weight-image set and the persistent workspaces - then recorded once with `gfv.cmdlist.record` and replayed from then on.  The
lists are bounded by the bytes of their private memory pools, least recently used out; a key that lost its list `evict_max`
times, or whose list alone is larger than the budget, stays eager for good (it would otherwise record on every visit, and a
recording allocates a whole step's activations afresh).

`decide` / `store` / `invalidate` / `clear` are host code with no GPU in them; `run` is the step of the forward-only users
(`Rollout`, `Sweep`, `Evaluate`) on top of them.  The training step (`TrainStep._issue`, shared by `PoolTrainStep` and `MarchStep`)
has an all-reduce and the optimiser behind each path and a validity check in front, and calls the policy directly.
"""
from __future__ import annotations

import collections
import collections.abc

WARM = 2        # eager steps of a key before its list is recorded
EVICT_MAX = 2   # a key that lost its list to the byte budget this often stays eager
_COUNTED = {"replay": "replayed", "record": "recorded", "eager": "eager"}


class Entry:
    """One recorded list: the `CommandList`, the bytes of its private pool, the outputs of the recorded step (they live in that
    pool and are overwritten by every replay) and whatever the caller keeps beside them."""

    def __init__(self, cl, nbytes, outs=None, **own):
        self.cl, self.bytes, self.outs = cl, nbytes, outs
        self.__dict__.update(own)


class ListCache(collections.abc.Mapping):
    """key -> Entry, least recently used first.  max_bytes=None: unbounded; max_bytes <= 0: nothing is ever listed."""

    def __init__(self, max_bytes, warm=WARM, evict_max=EVICT_MAX, dev=None):
        self.max_bytes, self.warm_steps, self.evict_max, self.dev = max_bytes, int(warm), int(evict_max), dev
        self._entries = collections.OrderedDict()
        self.warm, self.oversize, self.evicted = {}, set(), {}      # eager visits per key; keys eager for good; evictions per key
        self.counts = dict(replayed=0, recorded=0, eager=0)
        self.parked = None              # the list `run` recorded last, if the budget refused it: the caller releases it

    # ---- the mapping view --------------------------------------------------------------------------------------------------
    def __getitem__(self, key):
        return self._entries[key]

    def get(self, key, default=None):      # (the mixin's, in one dictionary look-up: it is on every step's path)
        return self._entries.get(key, default)

    def __iter__(self):
        return iter(self._entries)

    def __len__(self):
        return len(self._entries)

    def stats(self):
        return dict(self.counts, lists=len(self._entries), list_bytes=sum(e.bytes for e in self._entries.values()))

    # ---- the policy --------------------------------------------------------------------------------------------------------
    def decide(self, key, listed=True):
        """-> "replay" (the key moves to the recent end), "eager" (a warm-up of the key when `listed`) or "record"."""
        listed = listed and key not in self.oversize and (self.max_bytes is None or self.max_bytes > 0)
        if listed and key in self._entries:
            self._entries.move_to_end(key)
            what = "replay"
        elif not listed or self.warm.get(key, 0) < self.warm_steps:
            if listed:
                self.warm[key] = self.warm.get(key, 0) + 1
            what = "eager"
        else:
            what = "record"
        self.counts[_COUNTED[what]] += 1
        return what

    def store(self, key, entry):
        """Keep the list just recorded for `key` -> whether it was kept.  Larger than the budget: not kept, the key stays eager.
        Otherwise the oldest lists go while the sum exceeds the budget and more than one list remains."""
        if self.max_bytes is not None and entry.bytes > self.max_bytes:
            self.oversize.add(key)
            return False
        self._entries[key] = entry
        while (self.max_bytes is not None and len(self._entries) > 1
               and sum(e.bytes for e in self._entries.values()) > self.max_bytes):
            old, _ = self._entries.popitem(last=False)
            self.evicted[old] = self.evicted.get(old, 0) + 1
            if self.evicted[old] >= self.evict_max:
                self.oversize.add(old)
        return True

    def invalidate(self, key):
        """Something the list of `key` points at moved: it is dropped, and the eager step that follows is the first of the key's
        new warm-up."""
        del self._entries[key]
        self.warm[key] = 0

    def clear(self, keep_warm=False):
        """Drop every list.  keep_warm: the keys record again on their next visit (what they need has not changed, only where it
        is); otherwise they warm up again.  What the byte budget has decided about a key stays either way."""
        self._entries.clear()
        if not keep_warm:
            self.warm.clear()

    # ---- the forward-only step ---------------------------------------------------------------------------------------------
    def run(self, key, body, listed=True):
        """`body()` on the launch path of `key` -> its outputs (on a replay: the recorded step's own tensors)."""
        what = self.decide(key, listed)
        if what == "replay":
            ent = self._entries[key]
            ent.cl.replay()
            return ent.outs
        if what == "eager":
            return body()
        import torch
        from . import cmdlist
        before = torch.cuda.memory_reserved(self.dev)
        with cmdlist.record() as cl:
            outs = body()
        ent = Entry(cl, max(torch.cuda.memory_reserved(self.dev) - before, 0), outs)     # the segments of the list's private pool
        if not self.store(key, ent):
            self.parked = ent           # (its pool holds `outs`: it has to outlive the launches issued behind this step)
        return outs
