"""Training log on the device (gfv/trainlog.py, csrc/trainlog.hip; include/gfv.h gfv_train_log_norms / gfv_train_log_append).
The log copies values and sums in a fixed order, so every comparison is exact: `==`, `torch.equal`, bit patterns for the doubles
(tests/trainlog_ref.py restates the order of summation).  Run as a script this file is the one-rank RCCL worker of the last test."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

if __name__ == "__main__":
    ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    for p in (ROOT, os.path.join(ROOT, "gen-fvgn-steady_amd"), os.path.join(ROOT, "tests", "golden"), os.path.join(ROOT, "tests")):
        sys.path.insert(0, p)

import cases
import trainlog_ref as R
from oracle import fvgn_oracle as O

pytestmark = pytest.mark.gpu

LR = 1e-3
NAN32, ONE32 = 0x7fc00000, 0x3f800000


# ---- the tiny meshes of tests/test_pool_train_gpu.py (copies) ----------------------------------------------------------------------
def _meshes():
    from gfv import meshgen
    ms, fs = [], []
    for fac, kw, U, seed in (("raw_tri_channel_cylinder", dict(nx=30, ny=6, quad_fraction=0.0, seed=21), 0.15, 5),
                             ("raw_quad_cavity", dict(n=7, jitter=0.1, tri_fraction=0.3, seed=13), 1.0, 3),
                             ("raw_tri_channel_cylinder", dict(nx=36, ny=7, quad_fraction=0.3, seed=22), 0.25, 6),
                             ("raw_poisson_cavity", dict(n=6, seed=14), None, 4)):
        m = meshgen.finish_mesh(getattr(meshgen, fac)(**kw), U=U)
        ms.append(m)
        fs.append(meshgen.random_fields(m, seed=seed))
    return ms, fs


def _model(dataset_size=1):
    from FVMmodel.importer import NNmodel
    from gfv.params import default_params
    P = O.init_parameters(cases.WEIGHT_SEED)
    m = NNmodel(default_params(dataset_size=dataset_size))
    sd = m.state_dict()
    for k, v in P.items():
        sd[k].copy_(v)
    m.load_state_dict(sd)
    return m.cuda()


def _cyl_pool_with_variants():
    from gfv import meshgen
    from gfv.pool import DevicePool
    raw = meshgen.raw_tri_channel_cylinder(nx=30, ny=6, quad_fraction=0.0, seed=21)
    m = meshgen.finish_mesh(raw, U=0.15)
    pool = DevicePool([m], [meshgen.random_fields(m, seed=5)])
    for j in range(5):
        v = pool.add_variant(0, fields=meshgen.random_fields(m, seed=11 + j), U=0.12 + 0.04 * j, mu=1e-3 * (1 + j), dt=0.01 * (2 + j))
        assert v == j + 1
    return pool, m


def _mesh_pool():
    from gfv.pool import DevicePool
    ms, fs = _meshes()
    return DevicePool(ms, fs)


def _graphs():
    from gfv.graph import build_batch
    ms, fs = _meshes()
    return build_batch(ms[:2], fs[:2], device="cuda")


def _bits32(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.int32)


def _bits64(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def _rows_equal(a, b):
    """Two TrainLogRows, field by field and bit for bit (NaN norms included)."""
    for name in a._fields:
        x, y = getattr(a, name), getattr(b, name)
        if name == "dropped":
            assert x == y
        elif x.dtype == np.float32:
            assert np.array_equal(_bits32(x), _bits32(y)), name
        elif x.dtype == np.float64:
            assert np.array_equal(_bits64(x), _bits64(y)), name
        else:
            assert np.array_equal(x, y), name


# ---- 1: the norms launch alone -----------------------------------------------------------------------------------------------------
def _spread(n, seed):
    rng = np.random.default_rng(seed)
    return (rng.standard_normal(n) * 10.0 ** rng.uniform(-2.0, 2.0, n)).astype(np.float32)


class _Norms:
    """gfv_train_log_norms over hand-made buckets [(name, [(offset, count), ...])]: one workspace, kept across launches."""

    def __init__(self, buckets):
        from gfv import lib as L
        from gfv.trainlog import bucket_tables
        self.buckets, self.K = buckets, len(buckets)
        segs, tab, self.n_chunks = bucket_tables(buckets)
        self.segs = torch.tensor(segs, dtype=torch.int64).reshape(-1).cuda()
        self.tab = torch.tensor(tab, dtype=torch.int64).reshape(-1).cuda()
        nbytes = int(L.load().gfv_train_log_workspace_bytes(self.n_chunks))
        assert nbytes == 8 + 24 * self.n_chunks
        self.ws = torch.zeros(nbytes // 8, dtype=torch.float64, device="cuda")

    def run(self, g, p, fill=-7.0):
        from gfv import lib as L
        sums = torch.full((max(self.K, 1), 3), fill, dtype=torch.float64, device="cuda")
        rc = L.load().gfv_train_log_norms(g.data_ptr(), p.data_ptr(), self.segs.data_ptr() if self.K else None,
                                          self.tab.data_ptr() if self.K else None, self.K, self.n_chunks, sums.data_ptr(),
                                          self.ws.data_ptr(), L.stream_ptr())
        assert rc == 0, rc
        torch.cuda.synchronize()
        assert int(self.ws.view(torch.int32)[0]) == 0          # the arrival counter is left at zero
        return sums.cpu().numpy()

    def check(self, g, p):
        got = self.run(g, p)
        gh, ph = g.cpu().numpy(), p.cpu().numpy()
        for k, (name, segs) in enumerate(self.buckets):
            gs, ps, bad = R.bucket_sums(gh, ph, segs)
            assert np.isfinite(gs) and np.isfinite(ps), name
            assert R.same_bits(got[k, 0], gs), (name, got[k, 0], gs)
            assert R.same_bits(got[k, 1], ps), (name, got[k, 1], ps)
            assert got[k, 2] == bad == 0.0, name
        assert np.array_equal(_bits64(self.run(g, p)), _bits64(got))          # the same workspace again: the same bits
        return got


FIVE = [("one", [(5, 1)]),                                                     # one element
        ("chunk", [(1024, 1024)]),                                             # exactly one chunk
        ("chunk+1", [(4096, 1025)]),                                           # ... and one more element
        ("odd", [(6001, 700), (7002, 333), (8003, 1500)]),                     # offsets 1, 2, 3 mod 4: no 16-byte aligned segment
        ("long", [(12000, 40000), (52004, 66 * 1024 + 5 - 40000)])]            # 67 chunks: the fold's second round
N_FLAT = 12000 + 66 * 1024 + 5 + 64


def test_norms_launch_bit_for_bit():
    assert [o % 4 for o, _ in FIVE[3][1]] == [1, 2, 3] and sum(k for _, k in FIVE[4][1]) > 64 * 1024
    g, p = torch.from_numpy(_spread(N_FLAT, 1)).cuda(), torch.from_numpy(_spread(N_FLAT, 2)).cuda()
    five = _Norms(FIVE)
    assert five.n_chunks == 1 + 1 + 2 + 3 + 67
    got5 = five.check(g, p)
    # K = 1: aligned segments with counts that are no multiple of 4, so 16-byte and element loads alternate inside one bucket
    one = _Norms([("mixed", [(0, 1030), (2000, 7), (3000, 4096), (9001, 2)])])
    one.check(g, p)
    # the order is defined over the logical index: the same elements at other places in memory give the same bits
    g2, p2 = torch.zeros_like(g), torch.zeros_like(p)
    moved = [(17, 700), (2000, 333), (5006, 1500)]
    for (o, k), (o2, _) in zip(FIVE[3][1], moved):
        g2[o2:o2 + k], p2[o2:o2 + k] = g[o:o + k], p[o:o + k]
    got = _Norms([("moved", moved)]).run(g2, p2)
    assert np.array_equal(_bits64(got[0]), _bits64(got5[3]))
    # buffers that are not 16-byte aligned themselves: element loads throughout, the same bits
    gs, ps = torch.zeros(N_FLAT + 1, device="cuda"), torch.zeros(N_FLAT + 1, device="cuda")
    gs[1:], ps[1:] = g, p
    assert np.array_equal(_bits64(five.run(gs[1:], ps[1:])), _bits64(got5))
    # K = 0: nothing is launched, nothing written
    none = _Norms([])
    assert np.array_equal(none.run(g, p, fill=-7.0), np.full((1, 3), -7.0))


def test_norms_launch_counts_nonfinite():
    g, p = torch.from_numpy(_spread(N_FLAT, 1)).cuda(), torch.from_numpy(_spread(N_FLAT, 2)).cuda()
    five = _Norms(FIVE)
    clean = five.run(g, p)
    g[7002 + 5], g[8003 + 1499], g[6001] = float("nan"), float("inf"), float("nan")      # all in bucket "odd"
    g[7001], g[0] = float("nan"), float("inf")                                            # outside every segment: never read
    got = five.run(g, p)
    assert got[3, 2] == 3.0 and not np.isfinite(got[3, 0])
    assert np.array_equal(_bits64(got[:, 1]), _bits64(clean[:, 1]))                        # the parameter sums are untouched
    keep = [0, 1, 2, 4]
    assert np.array_equal(_bits64(got[keep]), _bits64(clean[keep]))
    assert R.bucket_sums(g.cpu().numpy(), p.cpu().numpy(), FIVE[3][1])[2] == 3


# ---- 2: the append launch alone, hand-made records ---------------------------------------------------------------------------------
class _Ring:
    def __init__(self, capacity, max_graphs, K=0, n_entries=0):
        from gfv.trainlog import HEADER_WORDS, row_words
        self.cap, self.MG, self.K = capacity, max_graphs, K
        self.buf = torch.zeros(HEADER_WORDS + capacity * row_words(max_graphs, K), dtype=torch.int32, device="cuda")
        self.table = torch.zeros((n_entries, 8), dtype=torch.int32, device="cuda") if n_entries else None
        self.head = 4 * HEADER_WORDS

    def append(self, t, loss, lr, losses, guard=None, accum=None, entries=None, sums=None):
        """guard = (norm, coef, decision), accum = apply: hand-made device records around them."""
        from gfv import lib as L
        dev = "cuda"
        state = torch.zeros(16, device=dev)
        state[0] = t
        hyper = torch.zeros(8, device=dev)
        hyper[0] = lr
        lo = torch.tensor([loss], dtype=torch.float32, device=dev)
        ls = torch.tensor(losses, dtype=torch.float32, device=dev).reshape(-1, 4)
        grec = arec = None
        if guard is not None:
            grec = torch.zeros(8, device=dev)
            grec[0], grec[2], grec[3] = 123.0, guard[0], guard[1]
            grec.view(torch.int32)[1], grec.view(torch.int32)[4] = 7, guard[2]
        if accum is not None:
            arec = torch.zeros(8, dtype=torch.int32, device=dev)
            arec[0], arec[3] = 3, accum
        ent = None if entries is None else (C.c_int32 * len(entries))(*entries)
        sm = None if sums is None else torch.tensor(sums, dtype=torch.float64, device=dev)
        rc = L.load().gfv_train_log_append(self.buf.data_ptr() + self.head, self.cap, self.MG, self.K, self.buf.data_ptr(),
                                           state.data_ptr(), hyper.data_ptr(), lo.data_ptr(), ls.data_ptr(), ls.shape[0],
                                           None if grec is None else grec.data_ptr(), None if arec is None else arec.data_ptr(), ent,
                                           None if sm is None else sm.data_ptr(), None if self.table is None else self.table.data_ptr(),
                                           0 if self.table is None else self.table.shape[0], L.stream_ptr())
        torch.cuda.synchronize()
        return rc

    def read(self):
        from gfv.trainlog import parse_rows
        return parse_rows(self.buf.cpu().numpy(), self.cap, self.MG, self.K)


def test_append_skip_hold_and_no_guard():
    from gfv import lib as L
    ring = _Ring(8, 2, K=2)
    t4 = [[1.5, 2.5, 3.5, 4.5]]
    sums = [[1.0, 2.0, 0.0], [3.0, 4.0, 2.0]]
    assert ring.append(1.0, 0.25, 1e-3, t4, sums=sums) == 0                                                   # no guard, no accum
    assert ring.append(2.0, 0.5, 1e-3, t4, guard=(3.0, 0.5, L.GUARD_CLIP), sums=sums) == 0                    # clipped: applied
    assert ring.append(2.0, float("inf"), 2e-3, t4, guard=(float("inf"), 1.0, L.GUARD_SKIP_NONFINITE), sums=sums) == 0
    assert ring.append(2.0, 0.5, 2e-3, t4, guard=(3.0, 1.0, L.GUARD_SKIP_FLAG), accum=1, sums=sums) == 0
    assert ring.append(2.0, 0.5, 2e-3, t4, guard=(3.0, 1.0, 0), accum=0, sums=sums) == 0                      # a hold micro-step
    assert ring.append(3.0, 0.5, 2e-3, t4, guard=(3.0, 1.0, 0), accum=1, sums=sums) == 0
    r = ring.read()
    assert r.dropped == 0 and r.ordinal.tolist() == [0, 1, 2, 3, 4, 5] and r.adam_t.tolist() == [1, 2, 2, 2, 2, 3]
    assert _bits32(r.norm)[0] == NAN32 and _bits32(r.coef)[0] == ONE32 and r.decision[0] == 0
    assert r.norm[1:].tolist() == [3.0, float("inf"), 3.0, 3.0, 3.0] and r.coef.tolist() == [1.0, 0.5, 1.0, 1.0, 1.0, 1.0]
    assert r.decision.tolist() == [0, L.GUARD_CLIP, L.GUARD_SKIP_NONFINITE, L.GUARD_SKIP_FLAG, 0, 0]
    assert r.apply.tolist() == [1, 1, 1, 1, 0, 1] and r.applied.tolist() == [1, 1, 0, 0, 0, 1]
    assert r.loss.tolist() == [0.25, 0.5, float("inf"), 0.5, 0.5, 0.5]
    assert np.array_equal(r.lr, np.array([1e-3, 1e-3, 2e-3, 2e-3, 2e-3, 2e-3], dtype=np.float32)) and r.B.tolist() == [1] * 6
    assert (r.terms[:, 0] == np.array(t4[0], dtype=np.float32)).all() and (r.terms[:, 1] == 0).all() and (r.entries == -1).all()
    assert (r.grad_sumsq == [1.0, 3.0]).all() and (r.param_sumsq == [2.0, 4.0]).all() and (r.grad_nonfinite == [0, 2]).all()


def test_append_wraps():
    """Capacity 4, 11 appends - through a TrainLog, so read() is the reader under test."""
    from gfv.engine import GradStore
    from gfv.trainlog import TrainLog
    store = GradStore(["a", "b"], [(5,), (3, 2)], "cuda")
    log = TrainLog(capacity=4, max_graphs=1)
    log.bind(store, "cuda")
    g = torch.arange(store.total, dtype=torch.float32, device="cuda")
    state, hyper = torch.zeros(16, device="cuda"), torch.full((8,), 0.5, device="cuda")
    loss, losses = torch.zeros(1, device="cuda"), torch.zeros((1, 4), device="cuda")
    assert log.read().ordinal.size == 0 and log.read().dropped == 0
    for k in range(11):
        state[0], loss[0], losses[0, 0] = k + 1, 10.0 + k, 100.0 + k
        log.append(g, g, state, hyper, loss, losses, 1)
    r = log.read()
    assert r.dropped == 7 and r.ordinal.tolist() == [7, 8, 9, 10] and r.adam_t.tolist() == [8, 9, 10, 11]
    assert r.loss.tolist() == [17.0, 18.0, 19.0, 20.0] and r.terms[:, 0, 0].tolist() == [107.0, 108.0, 109.0, 110.0]
    want = float(sum(v * v for v in [0, 1, 2, 3, 4, 8, 9, 10, 11, 12, 13]))         # (a: 0..4, three words padding, b: 8..13)
    assert log.names == ["all"] and (r.grad_sumsq == want).all() and (r.param_sumsq == want).all()
    log.clear()
    r = log.read()
    assert r.ordinal.size == 0 and r.dropped == 0
    log.append(g, g, state, hyper, loss, losses, 1)
    assert log.read().ordinal.tolist() == [0]


def test_append_slots_and_duplicate_entries():
    ring = _Ring(4, 3, n_entries=5)
    a, b, c = [1.0, 2.0, 3.0, 4.0], [5.0, 6.0, 7.0, 8.0], [9.0, 10.0, 11.0, 12.0]
    assert ring.append(1.0, 0.5, 1e-3, [a], entries=[4]) == 0
    assert ring.append(2.0, 0.5, 1e-3, [a, b, c], entries=[2, 0, 3]) == 0
    assert ring.append(3.0, 0.5, 1e-3, [b, c], entries=[0, 0]) == 0                  # the same entry twice: the later slot wins
    assert ring.append(4.0, 0.5, 1e-3, [c, a], entries=[-1, 3]) == 0                 # a slot without an entry
    assert ring.append(5.0, 0.5, 1e-3, [c, a], entries=[5, 3]) == -1                 # outside the table: refused, nothing appended
    assert ring.append(5.0, 0.5, 1e-3, [a, a, a, a], entries=[0, 1, 2, 3]) == -1     # B above max_graphs
    r = ring.read()
    assert r.ordinal.tolist() == [0, 1, 2, 3] and r.B.tolist() == [1, 3, 2, 2]
    assert r.entries.tolist() == [[4, -1, -1], [2, 0, 3], [0, 0, -1], [-1, 3, -1]]
    z = [0.0] * 4
    assert r.terms.tolist() == [[a, z, z], [a, b, c], [b, c, z], [c, a, z]]
    t = ring.table.cpu().numpy()
    assert t[:, 0].tolist() == [3, 0, 1, 2, 1] and t[:, 1].tolist() == [2, 0, 1, 3, 0] and (t[:, 6:] == 0).all()
    terms = np.ascontiguousarray(t[:, 2:6]).view(np.float32)
    assert terms.tolist() == [c, z, a, a, a]


# ---- 3: TrainStep in every launch mode ---------------------------------------------------------------------------------------------
def _train_run(use_graph, log, steps=8, **kw):
    from gfv.trainer import TrainStep
    ts = TrainStep(_model(), _graphs(), lr=LR, use_graph=use_graph, max_grad_norm=2.0, log=log, **kw)
    seen = []
    for k in range(steps):
        if k == 4:
            ts.lr = 0.5 * LR
        loss = ts.step()
        if log is None:                     # the run without a log drains the queue after every step to learn the same things
            st = ts.guard_stats()
            seen.append(dict(loss=float(loss), terms=ts.losses.cpu().numpy().copy(), norm=st["norm"], coef=st["coef"],
                             decision=st["decision"], adam_t=float(ts.adam_state[0]), lr=ts.lr))
    return ts, seen


@pytest.mark.parametrize("use_graph", [False, "list", True])
def test_trainstep_rows_equal_per_step_readings(use_graph):
    ta, _ = _train_run(use_graph, 16)
    rows = ta.log.read()
    tb, seen = _train_run(use_graph, None)
    assert tb.log is None
    n, B = len(seen), ta.plan.B
    assert B == 2 and ta.log.max_graphs == 2 and ta.log.names == ["all"]
    assert rows.dropped == 0 and rows.ordinal.tolist() == list(range(n)) and rows.B.tolist() == [B] * n
    for k, s in enumerate(seen):
        assert _bits32(rows.loss[k]) == _bits32(np.float32(s["loss"])), k
        assert np.array_equal(_bits32(rows.terms[k]), _bits32(s["terms"])), k
        assert _bits32(rows.norm[k]) == _bits32(np.float32(s["norm"])) and rows.coef[k] == np.float32(s["coef"]), k
        assert rows.decision[k] == s["decision"] and rows.adam_t[k] == s["adam_t"] == k + 1, k
        assert rows.lr[k] == np.float32(s["lr"]), k
    assert rows.lr[3] == np.float32(LR) and rows.lr[4] == np.float32(0.5 * LR)
    assert (rows.apply == 1).all() and (rows.applied == 1).all() and (rows.entries == -1).all()
    assert np.isfinite(rows.norm).all() and (rows.grad_nonfinite == 0).all() and (rows.grad_sumsq > 0).all()
    for name in ("flat_p", "flat_m", "flat_v"):
        assert torch.equal(getattr(ta, name), getattr(tb, name)), name
    assert "log" not in ta.state_dict() and set(ta.state_dict()) == set(tb.state_dict())


# ---- 4: PoolTrainStep on the recorded path -----------------------------------------------------------------------------------------
POOL_SEQ = [[0], [1], [0, 2], [0], [0], [0], [0, 2], [1], [0, 2], [0, 2], [3, 0], [0], [1, 1], [0, 2]]


def _pool_run(log, seq=POOL_SEQ, pool=None, **kw):
    from gfv.pool_trainer import PoolTrainStep
    pool = _mesh_pool() if pool is None else pool
    ts = PoolTrainStep(_model(), pool, max_graphs=2, lr=LR, use_graph="list", log=log, **kw)
    for idx in seq:
        ts.step(idx, payback=True)
    return ts


def test_pool_training_rows_carry_the_entries():
    ta = _pool_run(32)
    rows, es = ta.log.read(), ta.log.entry_stats()
    tb = _pool_run(None)
    n = len(POOL_SEQ)
    assert rows.ordinal.tolist() == list(range(n)) and rows.B.tolist() == [len(i) for i in POOL_SEQ]
    assert rows.entries.tolist() == [(i + [-1])[:2] for i in POOL_SEQ]
    assert rows.adam_t.tolist() == list(range(1, n + 1)) and _bits32(rows.norm).tolist() == [NAN32] * n      # (no guard)
    visits = [sum(i.count(e) for i in POOL_SEQ) for e in range(4)]
    assert es.visits.tolist() == visits == [11, 4, 5, 1]
    for e in range(4):
        k = max(j for j, i in enumerate(POOL_SEQ) if e in i)
        slot = max(s for s, v in enumerate(POOL_SEQ[k]) if v == e)
        assert es.last_ordinal[e] == k
        assert np.array_equal(_bits32(es.last_terms[e]), _bits32(rows.terms[k, slot])), e
    assert (rows.terms[np.array(rows.B) == 1, 1] == 0).all()
    sa, sb = ta.stats(), tb.stats()
    for key in ("replayed", "recorded", "eager", "lists", "list_bytes"):
        assert sa[key] == sb[key], (key, sa, sb)
    assert sa["replayed"] > 0 and sa["lists"] >= 2
    assert torch.equal(ta.flat_p, tb.flat_p) and torch.equal(ta.flat_m, tb.flat_m) and torch.equal(ta.flat_v, tb.flat_v)
    assert _bits32(rows.loss[-1]) == _bits32(np.float32(float(tb.loss)))


# ---- 5: accumulation ---------------------------------------------------------------------------------------------------------------
def test_accumulation_logs_every_micro_step():
    seq = [[0], [1], [0, 2], [0], [0], [1], [0]]
    ts = _pool_run(16, seq=seq, accum_steps=3, max_grad_norm=1e30)
    rows = ts.log.read()
    assert rows.apply.tolist() == [0, 0, 1, 0, 0, 1, 0] == rows.applied.tolist()
    assert rows.adam_t.tolist() == [0, 0, 1, 1, 1, 2, 2]
    assert rows.entries.tolist() == [(i + [-1])[:2] for i in seq]
    tb = _pool_run(None, seq=seq, accum_steps=3, max_grad_norm=1e30)
    assert torch.equal(ts.flat_p, tb.flat_p)


# ---- 7: the pool grows -------------------------------------------------------------------------------------------------------------
def test_entry_table_grows_with_the_pool():
    from gfv import meshgen
    pool, m = _cyl_pool_with_variants()
    ts = _pool_run(8, seq=[[0], [1], [2, 3]], pool=pool)
    before = ts.log.entry_stats()
    assert before.visits.tolist() == [1, 1, 1, 1, 0, 0]
    v = pool.add_variant(0, fields=meshgen.random_fields(m, seed=40), U=0.3, mu=2e-3, dt=0.02)
    assert v == 6
    ts.step([1])
    mid = ts.log.entry_stats()
    assert mid.visits.tolist() == [1, 2, 1, 1, 0, 0, 0] and mid.last_ordinal[6] == 0 and (mid.last_terms[6] == 0).all()
    keep = [0, 2, 3, 4, 5]
    assert np.array_equal(mid.last_ordinal[keep], before.last_ordinal[keep])
    assert np.array_equal(_bits32(mid.last_terms[keep]), _bits32(before.last_terms[keep]))
    ts.step([v])
    after, rows = ts.log.entry_stats(), ts.log.read()
    assert after.visits.tolist() == [1, 2, 1, 1, 0, 0, 1] and after.last_ordinal[6] == 4
    assert rows.entries[-1].tolist() == [6, -1] and np.array_equal(_bits32(after.last_terms[6]), _bits32(rows.terms[-1, 0]))
    assert (after.last_terms[6] != 0).any()


# ---- 8: bucket norms at trainer level ----------------------------------------------------------------------------------------------
def test_bucket_norms_of_the_last_step():
    from gfv.trainlog import bucket_segments
    prefixes = ["simulator.encoder.", "simulator.processpr_list.0.", "simulator.decoder."]
    ts, _ = _train_run("list", dict(capacity=4, buckets=prefixes), steps=5)
    rows = ts.log.read()
    torch.cuda.synchronize()
    assert ts.log.names == prefixes + ["rest"] and rows.grad_sumsq.shape == (4, 4) and rows.dropped == 1
    g, p = ts.flat_g.cpu().numpy(), ts.flat_p.cpu().numpy()
    buckets = bucket_segments(ts.G, prefixes)
    assert [n for n, _ in buckets] == ts.log.names
    for k, (name, segs) in enumerate(buckets):
        gs, ps, bad = R.bucket_sums(g, p, segs)
        assert R.same_bits(rows.grad_sumsq[-1, k], gs), name
        assert R.same_bits(rows.param_sumsq[-1, k], ps), name
        assert rows.grad_nonfinite[-1, k] == bad == 0
    # the buckets partition what the guard's norm covers: their sum is its square up to the rounding of two orders of summation
    # (the guard rounds its norm to fp32: 2^-24 relative, squared 2^-23; the double sums differ by n 2^-53, far below)
    total = float(rows.grad_sumsq[-1].sum())
    assert abs(float(rows.norm[-1]) ** 2 - total) <= 2.0 ** -22 * total
    # freezing a group rebuilds the buckets (the event on which the guard rebuilds its segments); a new count of buckets starts
    # the ring again
    from gfv.trainer import TrainStep
    groups = [dict(params=["simulator.decoder"], frozen=False)]
    ts = TrainStep(_model(), _graphs(), lr=LR, use_graph=False, param_groups=groups, log=dict(capacity=4, buckets=prefixes[:2]))
    ts.step()
    assert ts.log.names == prefixes[:2] + ["rest"]
    n_rest = int(ts.log.bucket_tab.cpu()[4 * 2 + 3])
    ts.set_group(0, frozen=True)
    ts.step()
    rows = ts.log.read()
    frozen = sum(ts.G.numel(n) for n in ts.G.off if n.startswith("simulator.decoder."))
    assert frozen > 0 and int(ts.log.bucket_tab.cpu()[4 * 2 + 3]) == n_rest - frozen
    assert rows.ordinal.tolist() == [0, 1]
    rest = dict(bucket_segments(ts.G, prefixes[:2], exclude=ts._gs.frozen_names()))["rest"]
    gs, ps, _ = R.bucket_sums(ts.flat_g.cpu().numpy(), ts.flat_p.cpu().numpy(), rest)
    assert R.same_bits(rows.grad_sumsq[1, 2], gs) and R.same_bits(rows.param_sumsq[1, 2], ps)


# ---- 6: through the one-rank collectives -------------------------------------------------------------------------------------------
def test_rows_through_rccl_one_rank_equal_the_plain_run():
    """distributed=True, world_size=1 (tests/test_rccl_gpu.py): the log's launches sit behind the all-reduce and Adam of the
    data-parallel tail; a one-rank all-reduce is the identity, so the rows are those of the plain run.  A child process: this
    file run as a script under torch.distributed.run."""
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", HSA_ENABLE_IPC_MODE_LEGACY="0")
    port = 29500 + (os.getpid() % 90)
    r = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "1", "--master-addr",
                        "127.0.0.1", "--master-port", str(port), os.path.abspath(__file__)], capture_output=True, text=True,
                       timeout=600, env=env)
    lines = re.findall(r"TRAINLOGRESULT mode=(\S+) same=(\d) rows=(\d+) backend=(\S+) world=(\d+)", r.stdout)
    assert r.returncode == 0 and len(lines) == 3 and "TRAINLOGOK 1" in r.stdout, r.stdout[-2000:] + r.stderr[-6000:]
    for mode, same, n, backend, world in lines:
        assert same == "1" and n == "6" and backend == "nccl" and world == "1", (mode, same, n, backend, world)


def _worker():
    import torch.distributed as dist
    torch.cuda.set_device(0)
    dist.init_process_group("nccl", device_id=torch.device("cuda", 0))
    ok = True
    for mode in (False, "list", True):
        plain, _ = _train_run(mode, 8, steps=6)
        through, _ = _train_run(mode, 8, steps=6, distributed=True, world_size=1)
        a, b = plain.log.read(), through.log.read()
        try:
            _rows_equal(a, b)
            same = torch.equal(plain.flat_p, through.flat_p) and through.dist_on and not plain.dist_on
        except AssertionError as e:
            print("TRAINLOGDIFF", mode, e)
            same = False
        ok = ok and same
        print(f"TRAINLOGRESULT mode={mode} same={int(same)} rows={len(b.ordinal)} backend={dist.get_backend()} "
              f"world={dist.get_world_size()}")
    print(f"TRAINLOGOK {int(ok)}")
    dist.destroy_process_group()


if __name__ == "__main__":
    _worker()
