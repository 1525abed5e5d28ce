"""GPU: Anderson acceleration per slot of a `Sweep` (csrc/anderson_kernel.h, csrc/sweep_anderson.hip, gfv_sweep_advance_aa in
csrc/sweep.hip, gfv/anderson.py SlotAndersonState, gfv/sweep.py).

Tests 1 - 3 drive the slot launches stand-alone through ctypes on the rank-3 contraction of tests/anderson_ref.py, G evaluated on
the host.  The reference is each entry run ALONE (B = 1) through the merged `gfv_anderson_gram` / `gfv_anderson_mix` /
`gfv_rollout_advance` (`Device` of tests/test_anderson_gpu.py), not the code under test:

1. offsets move under a live ring: two slots, entries of 133, 4161, 37 and 133 nodes with their own seeds, `tol = -1`; slot 0 is
   swapped from the 133-node entry to the 37-node one (and later to the second 133-node one) while slot 1, the 4161-node entry,
   is mid-run with a full ring, so that slot 1's first row moves from 133 to 37 and back.  Every step of every entry has the
   solo run's bits at the same age: record, gamma, advanced iterate.  AA(4), and AA(8) with beta = 0.5;
2. criterion, latch and freeze at `tol = 1e-5`: a slot latches at the first step whose fp32 ratio in the solo table is below tol,
   with depth 0, the host's g as its field, the table's norms in `last`, and nothing of it changes afterwards; `patience = 2`;
   the same entries without acceleration have not latched by then;
3. decisions per slot: a NaN restarts that slot only; a zero Gram matrix gives SINGULAR and no NaN.

Tests 4 - 8 go through `Sweep` on the fixture model, against `Rollout(..., anderson=4)` of the same batch composition (bit for
bit) - and, for mixed topologies, against the solo rollout, where the difference is printed and not asserted:

4. `anderson=0` is today's `Sweep`;  5. no swap, no latch, both launch modes;  6. continuous batching on one signature (the
   reset at a swap);  7. a latching tolerance: the field of a converged entry is the PLAIN model output of its latching step;
8. mixed topologies, a zero byte budget.

Measured on the MI355X, test 8 (the field of each of the four meshes after 6 steps of AA(4) in a sweep of two slots against its
solo `Rollout(anderson=4)`, relative to the field's largest value): see DESIGN.md 5e.
"""
import ctypes as C
import struct
import types

import numpy as np
import pytest
import torch

import anderson_ref as R
from test_anderson_gpu import _run, _same_bits
from test_sweep_gpu import _choose_tol, _cyl_pool_with_variants, _expect, _fields, _mesh_pool, _model, rel_err

pytestmark = pytest.mark.gpu
STRIDE = max(R.SIZES)


# ---- the stand-alone harness -----------------------------------------------------------------------------------------------
class SlotDevice:
    """`n_slots` slots of at most `stride` nodes on buffers of its own: the two slot launches + gfv_sweep_advance_aa (or, with
    m = 0, gfv_sweep_advance alone), G on the host.  `load` / `swap` do what Sweep's arena does: lay the slots' rows out one after
    the other, whatever their sizes."""

    def __init__(self, n_slots, m, beta=1.0, reg=1e-10, restart=10.0, start=0, tol=-1.0, min_steps=1, max_steps=1000, patience=1,
                 stride=STRIDE):
        from gfv import lib as L
        from gfv.anderson import SlotAndersonState
        dev = self.dev = torch.device("cuda")
        self.B, self.stride, self.m = n_slots, stride, m
        cap_n, cap_c = n_slots * stride, n_slots * ((stride + R.CHUNK - 1) // R.CHUNK)
        self.aa = SlotAndersonState(n_slots, stride, cap_c, dev, m, beta, reg, restart, start) if m else None
        f32 = dict(dtype=torch.float32, device=dev)
        self.x_backup, self.x = torch.zeros((cap_n, 12), **f32), torch.zeros((cap_n, 12), **f32)
        self.uvp, self.state3 = torch.zeros((cap_n, 3), **f32), torch.zeros((cap_n, 3), **f32)
        self.losses = torch.zeros((n_slots, 4), **f32)
        self.partial = torch.zeros((cap_c, 2), dtype=torch.float64, device=dev)
        words = struct.unpack("4i", struct.pack("f3i", tol, min_steps, max_steps, patience))
        self.ctl = torch.tensor(words, dtype=torch.int32).to(dev)
        self.slots = torch.zeros((n_slots, 4), dtype=torch.int32, device=dev)
        self.last = torch.zeros((n_slots, 6), **f32)
        self.state = torch.zeros(2, dtype=torch.int32, device=dev)
        host, devp = C.POINTER(C.c_int32)(), C.c_void_p()
        L.check(L.load(raw=True).gfv_sweep_mirror_create(1 + 2 * n_slots, C.byref(host), C.byref(devp)), "gfv_sweep_mirror_create")
        self._mirror, self._mirror_dev = host, devp.value
        self.sizes, self.plan, self.steps = None, None, 0

    def __del__(self):
        from gfv import lib as L
        if getattr(self, "_mirror", None):
            torch.cuda.synchronize()
            L.load(raw=True).gfv_sweep_mirror_free(self._mirror)
            self._mirror = None

    def _compose(self, sizes, xs):
        assert len(sizes) == self.B and all(1 <= n <= self.stride for n in sizes)
        cb, ce, gcp = R.chunk_tables(sizes)
        N = int(sum(sizes))
        assert int(ce.max()) <= N <= self.x_backup.shape[0] and int(cb.min()) >= 0 and int(gcp[-1]) == len(cb) <= self.partial.shape[0]
        t = lambda a: torch.from_numpy(a).to(self.dev)
        self.plan = types.SimpleNamespace(N=N, B=self.B, n_chunks=len(cb), chunk_beg=t(cb), chunk_end=t(ce), gchunk_ptr=t(gcp))
        self.sizes = list(sizes)
        self.ptr = np.concatenate(([0], np.cumsum(sizes))).tolist()
        self.x_backup[:N, 0:3] = torch.from_numpy(np.ascontiguousarray(np.concatenate(xs))).to(self.dev)

    def load(self, sizes, xs):
        self._compose(sizes, xs)

    def get_x(self):
        torch.cuda.synchronize()
        x = self.x_backup[:self.plan.N, 0:3].cpu().numpy()
        return [x[self.ptr[b]:self.ptr[b + 1]].copy() for b in range(self.B)]

    def swap(self, b, n, x0):
        """Slot b takes a new entry of n nodes: the other slots' rows move to where the new layout puts them, slot b's per-slot
        words go to zero (what Sweep.run does at a swap); the rings are NOT cleared."""
        xs = self.get_x()
        xs[b] = x0
        sizes = list(self.sizes)
        sizes[b] = n
        self._compose(sizes, xs)
        self.slots[b].zero_()
        if self.aa is not None:
            self.aa.reset_slot(b)

    def snapshot(self, b):
        """Everything slot b owns, as bytes: ring regions, state words, records, slots, last, its rows of x_backup."""
        torch.cuda.synchronize()
        s, rows = self.stride, slice(self.ptr[b], self.ptr[b + 1])
        parts = [self.slots[b], self.last[b], self.x_backup[rows]]
        if self.aa is not None:
            a = self.aa
            parts += [a.f_prev[b * s:(b + 1) * s], a.g_prev[b * s:(b + 1) * s], a.dF[:, b * s:(b + 1) * s], a.dG[:, b * s:(b + 1) * s],
                      a.state[b], a.r_prev[b], a.gamma[b], a.aa_slot[b], a.aa_count[b]]
        return [p.cpu().numpy().tobytes() for p in parts]

    def step(self, gs):
        """One step with the model's outputs `gs` (one [n_b, 3] array per slot) -> per slot the iterate the step left in uvp_node,
        and copies of aa_slot [B,4], gamma [B,8], aa_count [B,4], slots [B,4], last [B,6]."""
        from gfv import lib as L
        pl = self.plan
        self.uvp[:pl.N] = torch.from_numpy(np.ascontiguousarray(np.concatenate(gs))).to(self.dev)
        args = (self.uvp.data_ptr(), self.x_backup.data_ptr(), self.x.data_ptr(), pl.N, pl.chunk_beg.data_ptr(), pl.chunk_end.data_ptr(),
                pl.gchunk_ptr.data_ptr(), pl.n_chunks, pl.B, self.losses.data_ptr(), self.partial.data_ptr(), self.ctl.data_ptr(),
                self.slots.data_ptr(), self.last.data_ptr(), self.state3.data_ptr(), self._mirror_dev, self.state.data_ptr())
        if self.aa is None:
            L.check(L.load().gfv_sweep_advance(*args, L.stream_ptr()), "gfv_sweep_advance")
        else:
            self.aa.launch(self.uvp, self.x_backup, pl, self.ctl, self.slots)
            L.check(L.load().gfv_sweep_advance_aa(*args, self.aa.aa_slot.data_ptr(), L.stream_ptr()), "gfv_sweep_advance_aa")
        torch.cuda.synchronize()
        self.steps += 1
        assert self.state.tolist() == [self.steps, 0]
        out = self.uvp[:pl.N].cpu().numpy()
        rec = types.SimpleNamespace(out=[out[self.ptr[b]:self.ptr[b + 1]].copy() for b in range(self.B)],
                                    slots=self.slots.cpu().numpy().copy(), last=self.last.cpu().numpy().copy())
        if self.aa is not None:
            assert int(self.aa.counter) == 0
            rec.aa_slot, rec.gamma = self.aa.aa_slot.cpu().numpy().copy(), self.aa.gamma.cpu().numpy().copy()
            rec.count = self.aa.aa_count.cpu().numpy().copy()
        return rec


_SOLO = {}


def _solo(n, seed, m, beta, steps):
    """The entry (n nodes, seed) run alone for `steps` steps through the merged rollout-form launches -> the map and per step
    (x_k, g_k, iterate, table row [1,4], gamma [1,8]).  Computed once per key and left unchanged."""
    key = (n, seed, m, beta)
    if key not in _SOLO or len(_SOLO[key][1]) < steps:
        mp = R.Rank3Map(n, seed)
        rec, _ = _run(mp, mp.x0, [n], m, steps=steps, beta=beta, max_steps=steps)
        _SOLO[key] = (mp, rec)
    return _SOLO[key]


def _ratio32(row):
    return np.float32(row[0]) / np.float32(row[1])          # the fp32 quotient of the two fp32 norms


# 1 ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("m,beta", [(4, 1.0), (8, 0.5)])
def test_offsets_move_under_a_live_ring(m, beta):
    first, second, third = m + 2, 4, 3            # steps before the first swap (slot 1's ring is full), between, after
    total = first + second + third
    e133, e4161, e37, e133b = ((133, 12), (4161, 13), (37, 11), (133, 34))      # (R.SEEDS, and one more)
    solo = {e: _solo(*e, m, beta, total if e == e4161 else max(first, second, third)) for e in (e133, e4161, e37, e133b)}
    d = SlotDevice(2, m, beta=beta)
    cur, age = [e133, e4161], [0, 0]
    d.load([133, 4161], [solo[e133][0].x0, solo[e4161][0].x0])
    assert d.ptr[1] == 133
    depths = []
    for k in range(total):
        if k == first:
            d.swap(0, 37, solo[e37][0].x0)
            cur[0], age[0] = e37, 0
            assert d.ptr[1] == 37                 # slot 1's first row has moved under its live, full ring
            assert int(d.aa.state[1, 0]) == m
        if k == first + second:
            d.swap(0, 133, solo[e133b][0].x0)
            cur[0], age[0] = e133b, 0
            assert d.ptr[1] == 133
        xs = d.get_x()
        gs = [solo[cur[b]][0](xs[b]) for b in range(2)]
        rec = d.step(gs)
        for b in range(2):
            x_ref, g_ref, out_ref, row_ref, gamma_ref = solo[cur[b]][1][age[b]]
            where = (m, beta, k, b, cur[b], age[b])
            assert _same_bits(xs[b], x_ref) and _same_bits(gs[b], g_ref), (where, "the inputs")
            assert _same_bits(rec.aa_slot[b], row_ref[0]), (where, "record", rec.aa_slot[b], row_ref[0])
            assert _same_bits(rec.gamma[b], gamma_ref[0]), (where, "gamma", rec.gamma[b], gamma_ref[0])
            assert _same_bits(rec.out[b], out_ref), (where, "iterate")
            age[b] += 1
            assert rec.slots[b].tolist() == [age[b], 0, 0, 0], (where, rec.slots[b])
        depths.append(rec.aa_slot[:, 2].astype(int).tolist())
    print(f"m={m} beta={beta}: depths per step (slot 0, slot 1) {depths}")
    assert max(dp[1] for dp in depths) == m and depths[first][0] == 0 and depths[first + 1][0] == 1
    for b in range(2):
        assert _same_bits(d.get_x()[b], solo[cur[b]][1][age[b] - 1][2])


# 2 ---------------------------------------------------------------------------------------------------------------------
TOL = 1e-5
ENTRIES = list(zip(R.SIZES, R.SEEDS))


def _latch_index(rec):
    below = [k for k, r in enumerate(rec) if _ratio32(r[3][0]) < np.float32(TOL)]
    assert below, "the solo reference never goes below tol"
    return below[0]


@pytest.fixture(scope="module")
def solo_tol():
    return {e: _solo(*e, 4, 1.0, 12) for e in ENTRIES}


def test_criterion_latch_and_freeze(solo_tol):
    latch = {e: _latch_index(solo_tol[e][1]) for e in ENTRIES}
    print("expected latch step index per entry", latch)
    assert all(L <= 8 for L in latch.values()), latch          # step index 8 or earlier for all three sizes
    d = SlotDevice(3, 4, tol=TOL, patience=1)
    d.load(list(R.SIZES), [solo_tol[e][0].x0 for e in ENTRIES])
    frozen = {}
    for k in range(max(latch.values()) + 4):                   # (three more steps after the last slot has latched)
        xs = d.get_x()
        gs = [solo_tol[e][0](xs[b]) if b not in frozen else np.full((e[0], 3), np.nan, np.float32) for b, e in enumerate(ENTRIES)]
        rec = d.step(gs)
        for b, e in enumerate(ENTRIES):
            if b in frozen:
                assert d.snapshot(b) == frozen[b], (k, b, "a frozen slot changed")
                continue
            x_ref, g_ref, out_ref, row_ref, gamma_ref = solo_tol[e][1][k]
            assert _same_bits(rec.aa_slot[b, 0:2], row_ref[0, 0:2]) and _same_bits(rec.last[b, 4:6], row_ref[0, 0:2]), (k, b)
            if k < latch[e]:
                assert _same_bits(rec.aa_slot[b], row_ref[0]) and _same_bits(rec.gamma[b], gamma_ref[0]), (k, b)
                assert _same_bits(rec.out[b], out_ref) and rec.slots[b].tolist() == [k + 1, 0, 0, 0], (k, b, rec.slots[b])
            else:
                assert k == latch[e]
                assert rec.aa_slot[b, 2] == 0 and rec.aa_slot[b, 3] == 0 and not rec.gamma[b].any(), (k, b, rec.aa_slot[b])
                assert _same_bits(rec.out[b], gs[b]) and _same_bits(d.get_x()[b], gs[b]), (k, b, "the field is the host's g")
                assert rec.slots[b].tolist() == [k + 1, 1, 1, 0], (k, b, rec.slots[b])
                assert int(rec.count[b, 0]) == sum(int(r[3][0, 2] > 0) for r in solo_tol[e][1][:k])
                frozen[b] = d.snapshot(b)
    assert sorted(frozen) == [0, 1, 2]
    assert [int(d._mirror[1 + 2 * b]) for b in range(3)] == [1, 1, 1]


def test_patience_two_takes_two_plain_steps(solo_tol):
    latch = {e: _latch_index(solo_tol[e][1]) for e in ENTRIES}
    d = SlotDevice(3, 4, tol=TOL, patience=2)
    d.load(list(R.SIZES), [solo_tol[e][0].x0 for e in ENTRIES])
    done = set()
    for k in range(max(latch.values()) + 2):
        xs = d.get_x()
        gs = [solo_tol[e][0](xs[b]) if b not in done else np.full((e[0], 3), np.nan, np.float32) for b, e in enumerate(ENTRIES)]
        rec = d.step(gs)
        for b, e in enumerate(ENTRIES):
            if b in done or k < latch[e]:
                continue
            assert k in (latch[e], latch[e] + 1)
            assert _ratio32(rec.aa_slot[b]) < np.float32(TOL), (k, b, rec.aa_slot[b])
            assert rec.aa_slot[b, 2] == 0 and _same_bits(rec.out[b], gs[b]), (k, b, "a below-tol step is a plain step")
            if k == latch[e]:
                assert rec.slots[b].tolist() == [k + 1, 1, 0, 0], (k, b, rec.slots[b])
            else:
                assert rec.slots[b].tolist() == [k + 1, 2, 1, 0], (k, b, rec.slots[b])
                assert _same_bits(d.get_x()[b], gs[b])                 # the latched field: the host's g of the SECOND step
                done.add(b)
    assert done == {0, 1, 2}


def test_without_acceleration_nothing_has_latched_by_then(solo_tol):
    steps = max(_latch_index(solo_tol[e][1]) for e in ENTRIES) + 1
    d = SlotDevice(3, 0, tol=TOL, patience=1)
    d.load(list(R.SIZES), [solo_tol[e][0].x0 for e in ENTRIES])
    for k in range(steps):
        xs = d.get_x()
        rec = d.step([solo_tol[e][0](xs[b]) for b, e in enumerate(ENTRIES)])
    rel = rec.last[:, 4] / rec.last[:, 5]
    print(f"plain iteration after {steps} steps: rel {rel.tolist()}")
    assert rec.slots[:, 2].tolist() == [0, 0, 0] and rec.slots[:, 0].tolist() == [steps] * 3 and bool((rel > TOL).all())


# 3 ---------------------------------------------------------------------------------------------------------------------
def test_a_nan_restarts_its_slot_only(solo_tol):
    maps = [solo_tol[e][0] for e in ENTRIES]
    d, twin = SlotDevice(3, 4), SlotDevice(3, 4)
    for dev in (d, twin):
        dev.load(list(R.SIZES), [mp.x0 for mp in maps])
    for k in range(3):
        xs = d.get_x()
        gs = [mp(x) for mp, x in zip(maps, xs)]
        rec, rec_t = d.step(gs), twin.step(gs)
    assert rec.aa_slot[:, 2].tolist() == [2, 2, 2]
    xs = d.get_x()
    gs = [mp(x) for mp, x in zip(maps, xs)]
    bad = [g.copy() for g in gs]
    bad[1][70, 1] = np.nan
    rec, rec_t = d.step(bad), twin.step(gs)
    assert rec.aa_slot[:, 3].tolist() == [0, R.NONFINITE, 0] and rec.aa_slot[:, 2].tolist() == [3, 0, 3], rec.aa_slot
    assert rec.count.tolist() == [[3, 0, 0, 0], [2, 1, 0, 0], [3, 0, 0, 0]], rec.count
    assert not np.isnan(rec.gamma).any() and not rec.gamma[1].any()
    for b in (0, 2):
        assert _same_bits(rec.aa_slot[b], rec_t.aa_slot[b]) and _same_bits(rec.gamma[b], rec_t.gamma[b]), b
        assert _same_bits(rec.out[b], rec_t.out[b]), b
    assert _same_bits(rec.out[1], bad[1])                                   # depth 0: the model's output as it is
    st = d.aa.state.cpu().numpy()
    assert st[:, 3].tolist() == [0, 1, 0] and st[:, 0].tolist() == [3, 0, 3] and st[:, 2].tolist() == [1, 0, 1]


def test_zero_gram_matrix_gives_singular_and_no_nan(solo_tol):
    maps = [solo_tol[e][0] for e in ENTRIES]
    gs = [mp(mp.x0) for mp in maps]
    d = SlotDevice(3, 4)
    d.load(list(R.SIZES), gs)
    seen = set()
    for k in range(6):                                   # x = g every step: f = 0, every column 0
        rec = d.step(gs)
        assert all(_same_bits(o, g) for o, g in zip(rec.out, gs)), k
        assert not np.isnan(rec.aa_slot).any() and not np.isnan(rec.gamma).any() and not rec.gamma.any()
        assert all(rec.aa_slot[b, 2] == 0 and rec.aa_slot[b, 3] in (0, R.SINGULAR) for b in range(3)), (k, rec.aa_slot)
        assert rec.aa_slot[:, 0].tolist() == [0, 0, 0]
        seen |= set(rec.aa_slot[:, 3].astype(int).tolist())
    assert R.SINGULAR in seen
    assert rec.count.tolist() == [[0, 0, 0, 5]] * 3 and d.aa.state[:, 3].tolist() == [5, 5, 5]


# ---- through Sweep on the fixture model ------------------------------------------------------------------------------------
K = 6
_REF = {}


def _shared(kind):
    if ("pool", kind) not in _REF:
        _REF[("pool", kind)] = {"cyl": _cyl_pool_with_variants, "mesh": _mesh_pool}[kind]()
    if "model" not in _REF:
        _REF["model"] = _model()
    return _REF["pool", kind], _REF["model"]


def _aa_reference(kind, idx, steps=K):
    """`Rollout(model, pool.batch(idx), anderson=4)` over a pool nothing has been written into -> x_backup [N,12] BEFORE every
    step, x_backup[:, 0:3] after every step, the table [steps, B, 4], the history, the node offsets.  Computed once, left
    unchanged."""
    from gfv.rollout import Rollout
    key = (kind, tuple(idx), steps)
    if key not in _REF:
        pool, model = _shared(kind)
        g, _ = pool.batch(idx)
        r = Rollout(model, g, max_steps=steps, launch_mode="eager", anderson=4)
        before, after = [], []
        for _ in range(steps):
            before.append(r.x_backup.clone())
            r.step()
            after.append(r.x_backup[:, 0:3].clone())
        offs = np.concatenate(([0], np.cumsum([pool.sizes[i]["n"] for i in idx])))
        _REF[key] = (before, after, r.anderson_history().clone(), r.history.cpu().clone(), offs)
    return _REF[key]


def _check_fields(kind, idx, pool, results, steps):
    before, after, table, hist, offs = _aa_reference(kind, idx, steps)
    for b, (i, r) in enumerate(zip(idx, results)):
        assert (r.entry, r.steps, r.converged) == (i, steps, False), (b, r)
        want = after[steps - 1][offs[b]:offs[b + 1]]
        assert torch.equal(pool.x[i][:, 0:3], want), (kind, idx, b, rel_err(pool.x[i][:, 0:3], want))
        assert torch.equal(torch.tensor(r.losses, dtype=torch.float32), hist[steps - 1, b, 0:4]), (b, r.losses)
        assert r.rel_update == float(table[steps - 1, b, 0]) / float(table[steps - 1, b, 1])


# 4 ---------------------------------------------------------------------------------------------------------------------
def test_anderson_zero_is_the_sweep_of_today():
    from gfv.sweep import Sweep
    runs = []
    for kw in ({}, {"anderson": 0}):
        pool = _cyl_pool_with_variants()
        sw = Sweep(_shared("cyl")[1], pool, max_graphs=2, tol=-1, max_steps=4, max_ahead=0, **kw)
        res = sw.run()
        runs.append((res, _fields(pool, range(6)), sw.stats()))
        assert sw._aa is None and sw.anderson == 0
        with pytest.raises(RuntimeError, match="anderson=0"):
            sw.anderson_stats()
    assert runs[0][0] == runs[1][0] and runs[0][2] == runs[1][2], (runs[0][2], runs[1][2])
    assert all(torch.equal(a, b) for a, b in zip(runs[0][1], runs[1][1]))


# 5 ---------------------------------------------------------------------------------------------------------------------
def test_no_swap_no_latch_equals_the_accelerated_rollout():
    from gfv.sweep import Sweep
    idx = [0, 1, 2]
    _, _, table, _, _ = _aa_reference("cyl", idx)
    assert float(table[:, :, 2].max()) > 0, "the reference never accelerated a step"
    fields = {}
    for mode in ("cmd_list", "eager"):
        pool = _cyl_pool_with_variants()
        sw = Sweep(_shared("cyl")[1], pool, max_graphs=4, tol=-1, max_steps=K, launch_mode=mode, anderson=4)
        assert sw._aa.ring_stride == max(s["n"] for s in pool.sizes)
        res = sw.run(idx)
        _check_fields("cyl", idx, pool, res, K)
        torch.cuda.synchronize()
        assert torch.equal(sw._last[:3, 4:6].cpu(), table[K - 1, :, 0:2]) and torch.equal(sw._aa.aa_slot[:3].cpu(), table[K - 1])
        st, aa = sw.stats(), sw.anderson_stats()
        assert [a["accelerated"] for a in aa] == [int((table[:, b, 2] > 0).sum()) for b in range(3)], aa
        assert [a["last_depth"] for a in aa] == table[K - 1, :, 2].int().tolist()
        assert all(sum(a["restarts"].values()) == int((table[:, b, 3] != 0).sum()) for b, a in enumerate(aa))
        if mode == "cmd_list":
            assert (st["eager"], st["recorded"], st["replayed"], st["lists"]) == (2, 1, 3, 1), st
        else:
            assert (st["eager"], st["recorded"], st["lists"]) == (K, 0, 0), st
        fields[mode] = (_fields(pool, idx), res)
    assert fields["cmd_list"][1] == fields["eager"][1]
    assert all(torch.equal(a, b) for a, b in zip(fields["cmd_list"][0], fields["eager"][0]))


# 6 ---------------------------------------------------------------------------------------------------------------------
def test_continuous_batching_resets_a_swapped_slot():
    from gfv.sweep import Sweep
    pool = _cyl_pool_with_variants()
    sw = Sweep(_shared("cyl")[1], pool, max_graphs=2, tol=-1, max_steps=5, max_ahead=0, anderson=4)
    res = sw.run()
    assert [r.entry for r in res] == list(range(6))
    for pair in ([0, 1], [2, 3], [4, 5]):
        _check_fields("cyl", pair, pool, [res[i] for i in pair], 5)
    st, aa = sw.stats(), sw.anderson_stats()
    assert st["lists"] == 1 and st["recorded"] == 1 and st["swaps"] == 2 and st["steps"] == 15, st
    assert len(aa) == 6 and all(set(a) == {"accelerated", "restarts", "last_depth"} for a in aa), aa
    for pair in ([0, 1], [2, 3], [4, 5]):
        table = _aa_reference("cyl", pair, 5)[2]
        assert [aa[i]["accelerated"] for i in pair] == [int((table[:, b, 2] > 0).sum()) for b in range(2)], (pair, aa)


# 7 ---------------------------------------------------------------------------------------------------------------------
def test_a_latching_tolerance_latches_the_plain_model_output():
    from gfv.rollout import Rollout
    from gfv.sweep import Sweep
    idx = [0, 1, 2]
    before, after, aa_table, hist, offs = _aa_reference("cyl", idx)
    table = aa_table[:, :, 0] / aa_table[:, :, 1]              # fp32 quotient of the two fp32 norms
    tol, expect = _choose_tol(table)
    print(f"AA(4) residual table\n{table}\ntol {tol:.6e} -> expected (steps, converged) {expect}")
    assert any(c for _, c in expect)
    pool0, model = _shared("cyl")
    plain = Rollout(model, pool0.batch(idx)[0], max_steps=1, launch_mode="eager")
    runs = []
    for ahead in (0, 4):
        pool = _cyl_pool_with_variants()
        sw = Sweep(model, pool, max_graphs=3, tol=tol, max_steps=K, max_ahead=ahead, anderson=4)
        res = sw.run(idx)
        for b, (i, r, (steps, conv)) in enumerate(zip(idx, res, expect)):
            assert (r.entry, r.steps, r.converged) == (i, steps, conv), (b, r, steps, conv)
            assert r.rel_update == float(aa_table[steps - 1, b, 0]) / float(aa_table[steps - 1, b, 1])
            if conv:
                assert r.rel_update < tol and sw.anderson_stats()[b]["last_depth"] == 0
                plain.reset(before[steps - 1])                 # the state the latching step started from
                want = plain.step()[1][offs[b]:offs[b + 1]]    # G(x_k): the reference forward's uvp_node, unmixed
            else:
                want = after[steps - 1][offs[b]:offs[b + 1]]
            assert torch.equal(pool.x[i][:, 0:3], want), (ahead, b, conv, rel_err(pool.x[i][:, 0:3], want))
        runs.append((res, _fields(pool, idx), sw.anderson_stats()))
    assert runs[0][0] == runs[1][0] and runs[0][2] == runs[1][2]
    assert all(torch.equal(a, b) for a, b in zip(runs[0][1], runs[1][1]))


# 8 ---------------------------------------------------------------------------------------------------------------------
def test_mixed_topologies():
    from gfv.sweep import Sweep
    runs = {}
    for budget in (16 << 30, 0):
        pool = _mesh_pool()
        sw = Sweep(_shared("mesh")[1], pool, max_graphs=2, tol=-1, max_steps=K, max_ahead=0, max_list_bytes=budget, anderson=4)
        res = sw.run()
        runs[budget] = (res, _fields(pool, range(4)), sw.stats(), sw.anderson_stats())
    res, fields, st, aa = runs[16 << 30]
    assert [r.entry for r in res] == [0, 1, 2, 3] and all((r.steps, r.converged) == (K, False) for r in res)
    assert len(aa) == 4 and st["swaps"] == 1 and st["lists"] >= 2, (st, aa)
    for i in range(4):
        _, after, table, _, _ = _aa_reference("mesh", [i])
        e = rel_err(fields[i], after[K - 1])
        print(f"mesh {i}: field after {K} steps of AA(4) in the sweep against the solo Rollout(anderson=4): rel {e:.2e} "
              f"(bitwise {bool(torch.equal(fields[i], after[K - 1]))}); depths solo {table[:, 0, 2].int().tolist()} "
              f"accelerated in the sweep {aa[i]['accelerated']}")
        assert bool(torch.isfinite(fields[i]).all())
    res0, fields0, st0, aa0 = runs[0]
    assert res0 == res and aa0 == aa and all(torch.equal(a, b) for a, b in zip(fields0, fields))
    assert st0["eager"] == st0["steps"] == st["steps"] and st0["recorded"] == 0 and st0["lists"] == 0, st0
