"""Sweep: run a trained model over the entries of a device pool, slot by slot (continuous batching of a parameter sweep).

The reference solves one case at a time (`solve_without_grad_GPU.py:117-173`); `gfv.rollout.Rollout` is that loop for ONE batch,
bound to the graphs it was built with, and its `run(tol=...)` stops a batch only when its slowest member is below the tolerance.
`Sweep` is the inference twin of `gfv.pool_trainer.PoolTrainStep`: a fixed number of slots in a `BatchArena`, every slot advances
its own pool entry until THAT entry meets the criterion and is frozen on the device at that step; a retired slot takes the next
pending entry.

    sw = Sweep(model, pool, max_graphs=8, tol=1e-6, max_steps=40000)
    results = sw.run()                  # results[i]: entry, steps, converged, losses (4 floats), rel_update
    sw.stats()                          # {"steps", "swaps", "replayed", "recorded", "eager", "lists", "list_bytes"}

The fields themselves are in the pool afterwards (entry `x[:, 0:3]`), as after `PoolTrainStep.step(payback=True)`.

The step is `Rollout._body` over the arena's plan and `x` / `x_raw` - the forward-only engine path on static weight images - with
`gfv_sweep_advance` (csrc/sweep.hip) in place of `gfv_rollout_advance`: per-slot `age / streak / done` live on the device, the
criterion is evaluated there, and a slot whose `done` is set keeps its state whatever is queued behind it.  That is what lets the
host run ahead without synchronising (`max_ahead`) and makes an entry's result independent of its neighbours.

Recorded lists are kept per ordered batch signature (variants of one mesh share it: one list serves the whole sweep) in a
`gfv.listcache.ListCache` bounded by `max_list_bytes`.  Who owns what a list points at: DESIGN.md 5l.  Particular to this object,
for its lifetime, never reallocated: `ctl`, `slots`, `last`, `state3`, the reduction workspace, the counters, the pinned mirror.

A swap (the mirror shows a retired slot and something is pending): synchronise; read `slots` / `last` from device memory; pay
`state3` back into ALL current entries; record the retired entries' results; load the new index list; zero the swapped slots.
The mirror is only a hint that a synchronisation is worth it - every value acted on is read from device memory after it.

Anderson acceleration per slot (`anderson=m`, 1 .. 8; gfv/anderson.py SlotAndersonState): for STEADY cases.
Two more launches between the forward and the advance mix each live slot's model output with that slot's last m residual
differences, decided on the device; the rings are per slot at a fixed stride (the largest node count of the pool at
construction), the step index is the slot's own age, and a swap zeroes the swapped slots' state words.  The criterion is then the
true fixed-point residual || G(x) - x || / || G(x) || (`rel_update` of a result is that of the latching step), and a step whose
residual is below `tol` is a plain step: a converged entry's field is the model's own output G(x_k) with a measured residual
below `tol`, the same guarantee as without it.  `anderson_stats()` reports, per entry of the last run, the accelerated steps, the
restarts by kind and the depth of the last step.  `anderson=0` (the default) issues no new launch and allocates nothing.
"""
from __future__ import annotations

import collections
import ctypes as C
import math
import struct

import torch

from . import anderson as AA
from . import lib as L
from . import listcache
from .functions import require_gpu
from .static_forward import StaticForward, check_normalizer

SweepResult = collections.namedtuple("SweepResult", "entry steps converged losses rel_update")

DONE_LIVE, DONE_CONVERGED, DONE_MAX_STEPS = 0, 1, 2


# ---- host-side checks and the scheduler: no GPU ------------------------------------------------------------------------------
def check_max_steps(max_steps):
    """Termination is enforced on the device by `max_steps`: it has to be a finite positive whole number."""
    try:
        ok = math.isfinite(max_steps) and max_steps >= 1 and int(max_steps) == max_steps and max_steps < 2 ** 31
    except (TypeError, ValueError, OverflowError):
        ok = False
    if not ok:
        raise ValueError(f"Sweep: max_steps must be a finite positive integer, not {max_steps!r} (it is what ends a slot that "
                         "never converges)")
    return int(max_steps)


def check_entries(entries, n):
    """-> the entries as a list of ints; ValueError for a duplicate or an entry outside the pool of `n`."""
    out = list(range(n)) if entries is None else [int(e) for e in entries]
    for e in out:
        if not 0 <= e < n:
            raise ValueError(f"Sweep: pool entry {e} does not exist (the pool holds {n})")
    if len(set(out)) != len(out):
        raise ValueError("Sweep: an entry appears more than once (each entry is solved once and written back once)")
    return out


class SlotScheduler:
    """Which entry runs in which slot.  Slots are filled from the pending queue in order; a retired slot takes the first pending
    entry with the SAME entry signature (the batch signature - and with it the recorded list - stays), else the first pending
    entry of any signature; with nothing pending it keeps its (frozen) entry.  A live entry never changes slot."""

    def __init__(self, entries, signature_of, n_slots):
        if int(n_slots) < 1:
            raise ValueError("a sweep needs at least one slot")
        self.pending = collections.deque(entries)
        self.sig = {e: signature_of(e) for e in entries}
        self.n_slots = int(n_slots)
        self.slots = []

    def start(self):
        """-> the entries of the first batch, slot by slot."""
        while self.pending and len(self.slots) < self.n_slots:
            self.slots.append(self.pending.popleft())
        return list(self.slots)

    def replace(self, retired):
        """`retired`: slot numbers whose entries are finished -> {slot: new entry} for those that got one."""
        new = {}
        for b in sorted(retired):
            if not self.pending:
                break
            want = self.sig[self.slots[b]]
            pick = next((e for e in self.pending if self.sig[e] == want), self.pending[0])
            self.pending.remove(pick)
            self.slots[b] = pick
            new[b] = pick
        return new

    def batch_signature(self):
        return tuple(self.sig[e] for e in self.slots)


class Sweep:
    WARM, EVICT_MAX = listcache.WARM, listcache.EVICT_MAX

    def __init__(self, model, pool, max_graphs=8, tol=1e-6, max_steps=40000, min_steps=1, patience=1, max_ahead=64,
                 launch_mode="cmd_list", max_list_bytes=16 << 30, max_sizes=None, anderson=0, anderson_beta=1.0,
                 anderson_reg=1e-10, anderson_restart=10.0, anderson_start=0):
        if launch_mode not in ("cmd_list", "eager"):
            raise ValueError('launch_mode must be "cmd_list" or "eager"')
        aa_args = AA.check_args(anderson, anderson_beta, anderson_reg, anderson_restart, anderson_start)
        self.max_steps = check_max_steps(max_steps)
        if int(min_steps) < 0 or int(patience) < 1 or int(max_ahead) < 0:
            raise ValueError("Sweep: min_steps >= 0, patience >= 1 and max_ahead >= 0 are required")
        self.tol, self.min_steps, self.patience = float(tol), int(min_steps), int(patience)
        if math.isnan(self.tol):
            raise ValueError("Sweep: tol is NaN (a negative tol means: never converge)")
        self.max_ahead = int(max_ahead)
        self.launch_mode, self.max_list_bytes = launch_mode, int(max_list_bytes)
        self.model, self.pool = model, pool
        check_normalizer(model)
        require_gpu(pool.x[0])
        self.arena = pool.arena(max_graphs, max_sizes)
        self.engine = model.engine()
        dev = self.dev = pool.device
        cap, B = self.arena.capacity, self.arena.max_graphs
        self.norm_global = True        # (what the graphs of a pool carry: gfv.pool.BatchArena._make_views)
        # device-resident state of the slots and what the advance launch works on: created once, never reallocated
        self._ctl = torch.zeros(4, dtype=torch.int32, device=dev)
        self._slots = torch.zeros((B, 4), dtype=torch.int32, device=dev)
        self._last = torch.zeros((B, 6), dtype=torch.float32, device=dev)
        self._state3 = torch.zeros((max(cap["n"], 1), 3), dtype=torch.float32, device=dev)
        self._partial = torch.zeros((max(cap["nchunk"], 1), 2), dtype=torch.float64, device=dev)
        self._state = torch.zeros(2, dtype=torch.int32, device=dev)          # (step sequence number, arrival counter)
        self._mirror_words = 1 + 2 * B
        host, devp = C.POINTER(C.c_int32)(), C.c_void_p()
        L.check(L.load(raw=True).gfv_sweep_mirror_create(self._mirror_words, C.byref(host), C.byref(devp)), "gfv_sweep_mirror_create")
        self._mirror, self._mirror_dev = host, devp.value
        L.status_mirror()
        self._lists = listcache.ListCache(self.max_list_bytes, dev=dev)      # batch signature -> the recorded step
        self._counts = dict(steps=0, swaps=0)
        self._fwd = StaticForward(model, B, dev)
        # Anderson acceleration per slot: rings at a fixed stride per slot, created once (recorded lists point at them)
        self.anderson = aa_args[0]
        self._aa, self._aa_stats = None, None
        if self.anderson:
            stride = max(int(sz["n"]) for sz in pool.sizes)
            self._aa = AA.SlotAndersonState(B, stride, max(cap["nchunk"], 1), dev, *aa_args)

    def __del__(self):
        host = getattr(self, "_mirror", None)
        if host:
            try:
                self._lists.clear()
                torch.cuda.synchronize(self.dev)     # (nothing queued may still publish into the mirror)
                L.load(raw=True).gfv_sweep_mirror_free(host)
            except Exception:
                pass
            self._mirror = None

    # ---- weights, one step ---------------------------------------------------------------------------------------------
    def refresh_weights(self):
        """(Re)build what depends on the parameter VALUES: padded copies (hidden_size < 128) and the forward weight images.
        Recorded lists are dropped (the next steps warm up and record again)."""
        self._fwd.refresh()
        self._lists.clear()

    P = property(lambda self: self._fwd.P)

    def stats(self):
        return dict(self._counts, **self._lists.stats())

    def _body(self, graphs, pl):
        x, x_raw = graphs[0].x, graphs[0]._gfv_x_raw
        losses, uvp_node, _ = self._fwd.forward(x, x_raw, pl, False, self.norm_global)
        args = (uvp_node.data_ptr(), x_raw.data_ptr(), x.data_ptr(), pl.N, pl.chunk_beg.data_ptr(), pl.chunk_end.data_ptr(),
                pl.gchunk_ptr.data_ptr(), pl.n_chunks, pl.B, losses.data_ptr(), self._partial.data_ptr(), self._ctl.data_ptr(),
                self._slots.data_ptr(), self._last.data_ptr(), self._state3.data_ptr(), self._mirror_dev, self._state.data_ptr())
        if self._aa is None:
            L.check(L.load().gfv_sweep_advance(*args, L.stream_ptr()), "gfv_sweep_advance")
        else:
            self._aa.launch(uvp_node, x_raw, pl, self._ctl, self._slots)
            L.check(L.load().gfv_sweep_advance_aa(*args, self._aa.aa_slot.data_ptr(), L.stream_ptr()), "gfv_sweep_advance_aa")
        L.status_publish()
        return losses, uvp_node

    def _step(self, key, graphs, pl):
        self._counts["steps"] += 1
        self._lists.run(key, lambda: self._body(graphs, pl), self.launch_mode == "cmd_list")
        self._lists.parked = None       # (a list the byte budget refused goes at once: nothing behind the step reads its outputs)

    # ---- the run -------------------------------------------------------------------------------------------------------
    def _write_ctl(self):
        words = struct.unpack("4i", struct.pack("f3i", self.tol, self.min_steps, self.max_steps, self.patience))
        self._ctl.copy_(torch.tensor(words, dtype=torch.int32))

    def _read_slots(self):
        """(synchronises) -> slots [B,4] and last [B,6] as the device holds them; with Anderson acceleration the per-slot counts
        and records are copied at the same synchronisation."""
        torch.cuda.current_stream().synchronize()
        if self._aa is not None:
            self._aa_rows = (self._aa.aa_count.cpu(), self._aa.aa_slot.cpu())
        return self._slots.cpu(), self._last.cpu()

    def anderson_stats(self):
        """One dict per entry of the last `run`, in the order of its `entries`: {"accelerated": steps that were mixed,
        "restarts": {"NONFINITE", "GROWTH", "SINGULAR"}, "last_depth": the depth of the entry's last step}.  Harvested where the
        results are: no synchronisation of its own."""
        if self._aa is None:
            raise RuntimeError("this Sweep was built with anderson=0")
        if self._aa_stats is None:
            raise RuntimeError("anderson_stats() reports the last run(): nothing has run")
        return list(self._aa_stats)

    @staticmethod
    def _result(entry, slot_row, last_row):
        d, n = float(last_row[4]), float(last_row[5])
        rel = d / n if n != 0.0 else float("nan")
        return SweepResult(entry, int(slot_row[0]), int(slot_row[2]) == DONE_CONVERGED, tuple(float(v) for v in last_row[0:4]), rel)

    def run(self, entries=None):
        """Solve the pool entries `entries` (None: all of them) -> a list of SweepResult in the order of `entries`; the fields are
        written back into the pool entries' `x[:, 0:3]`."""
        L.raise_on_status("Sweep.run")
        ents = check_entries(entries, self.pool.n)
        check_normalizer(self.model)
        self._fwd.check("Sweep", "sweep")
        if self._aa is not None:
            AA.check_ring_stride({e: self.pool.sizes[e]["n"] for e in ents}, self._aa.ring_stride)
            self._aa_stats = []
        if not ents:
            return []
        sched = SlotScheduler(ents, lambda e: self.arena.signature([e])[0], self.arena.max_graphs)
        cur = sched.start()
        B = len(cur)
        stream = torch.cuda.current_stream()
        stream.synchronize()
        for i in range(self._mirror_words):
            self._mirror[i] = 0
        self._write_ctl()
        self._slots.zero_()
        self._last.zero_()
        self._state.zero_()
        if self._aa is not None:
            self._aa.reset()
        aa_stats = {}
        graphs, pl = self.arena.load(cur)
        key = sched.batch_signature()
        state3 = self._state3[:pl.N]
        results, harvested = {}, set()        # entry -> SweepResult; slots whose current entry's result has been recorded
        issued = known = 0                    # steps issued since the counters were zeroed; of those, known to have completed
        taken = [0] * B                       # steps issued since the slot was loaded: at max_steps it is done, mirror or not
        events = collections.deque()
        while True:
            self._step(key, graphs, pl)
            issued += 1
            taken = [t + 1 for t in taken]
            if self.max_ahead == 0:
                stream.synchronize()
                known = issued
            else:
                if issued % self.max_ahead == 0:
                    ev = torch.cuda.Event()
                    ev.record(stream)
                    events.append((issued, ev))
                known = max(known, min(int(self._mirror[0]), issued))
                while issued - known >= self.max_ahead and events:
                    n, ev = events.popleft()
                    ev.synchronize()
                    known = max(known, n)
            # the mirror: a hint that a synchronisation is worth it (a slot that has been issued max_steps steps needs none)
            retired = [b for b in range(B) if b not in harvested
                       and (self._mirror[1 + 2 * b] != DONE_LIVE or taken[b] >= self.max_steps)]
            if not retired:
                continue
            if not sched.pending and len(retired) + len(harvested) < B:
                continue                      # (nothing to hand out, and live slots remain: keep going)
            slots, last = self._read_slots()  # (synchronises: from here on, what the device holds)
            events.clear()
            known = issued
            done = [b for b in range(B) if int(slots[b, 2]) != DONE_LIVE]
            self.arena.payback(cur, state3)
            for b in done:
                if b not in harvested:
                    results[cur[b]] = self._result(cur[b], slots[b], last[b])
                    if self._aa is not None:
                        aa_stats[cur[b]] = AA.count_dict(self._aa_rows[0][b], self._aa_rows[1][b])
                    harvested.add(b)
            new = sched.replace(done)
            if not new:
                if len(harvested) == B:
                    break                     # every slot done, nothing pending: the payback above was the final one
                continue
            self._counts["swaps"] += 1
            cur = list(sched.slots)
            graphs, pl = self.arena.load(cur)
            key = sched.batch_signature()
            state3 = self._state3[:pl.N]
            for b in new:
                self._slots[b].zero_()
                if self._aa is not None:
                    self._aa.reset_slot(b)
                self._mirror[1 + 2 * b] = 0
                self._mirror[2 + 2 * b] = 0
                harvested.discard(b)
                taken[b] = 0
        stream.synchronize()
        L.raise_on_status("Sweep.run")
        self._current = (key, graphs, pl)     # (what the arena holds: every slot frozen)
        if self._aa is not None:
            self._aa_stats = [aa_stats[e] for e in ents]
        return [results[e] for e in ents]
