"""The reference's pool-renewal schedule as a host object (pre_train_Adam.py:116-118, Graph_loader.py:154-229,389-396).

Every ``ceil(average_sequence_length / dataset_size)`` epochs the reference arms its pool; at the next ``payback`` the pool then
retires its ``rst_time = ceil(dataset_size / average_sequence_length)`` OLDEST entries (``meta_pool.pop(0)``) and appends each
re-made with a freshly chosen boundary condition - so a renewed entry is the youngest.  Here the entries stay where they are in
the `DevicePool`; their age is kept as a first-in first-out order of indices, and the retired ones are re-drawn by ONE
``pool.renew`` call (one launch, no host synchronisation).  The draw itself stays with the caller, as for
``DevicePool.reset_env``: ``draw(i) -> dict`` of sampled values for entry ``i`` (the reference's: ``random.choice(theta_PDE_list)``).

Pure host logic: no torch, no device."""
from __future__ import annotations

from collections import deque
from math import ceil


class PoolRenewal:
    def __init__(self, pool, draw, dataset_size=None, average_sequence_length=1):
        self.pool, self.draw = pool, draw
        self.dataset_size = int(pool.n if dataset_size is None else dataset_size)
        self.average_sequence_length = int(average_sequence_length)
        if self.dataset_size < 1 or self.average_sequence_length < 1:
            raise ValueError("dataset_size and average_sequence_length must be at least 1")
        self.period = ceil(self.average_sequence_length / self.dataset_size)      # epochs between two renewals
        self.rst_time = ceil(self.dataset_size / self.average_sequence_length)    # entries retired by one renewal
        self.age = deque(range(int(pool.n)))                                      # oldest first
        self.armed = False
        self.renewed = 0                                                          # entries re-drawn so far

    def arm(self, epoch):
        """Call at the start of every epoch -> whether the flag is now set (the reference sets it on the epochs that are multiples
        of the period and leaves a flag that is still set alone)."""
        if int(epoch) % self.period == 0:
            self.armed = True
        return self.armed

    def after_payback(self):
        """Call after every payback -> the indices renewed ([] while the flag is not set).  Entries added to the pool since the
        last call (add_variant) join as the youngest."""
        self.age.extend(range(len(self.age), int(self.pool.n)))
        if not self.armed:
            return []
        if self.rst_time > len(self.age):
            raise ValueError(f"a renewal retires {self.rst_time} entries, the pool holds {len(self.age)}")
        retired = [self.age[k] for k in range(self.rst_time)]
        self.pool.renew(retired, [self.draw(i) for i in retired])
        self.age.rotate(-self.rst_time)                                           # the renewed entries are now the youngest
        self.armed = False
        self.renewed += len(retired)
        return retired
