"""Training log, host side (gfv/trainlog.py; include/gfv.h gfv_train_log_norms / gfv_train_log_append): the ring window
arithmetic, the bucket construction, the argument checks, the numpy restatement of the summation order against math.fsum, and the
refusals of the two entry points - all without a GPU."""
import ctypes as C
import math

import numpy as np
import pytest

import trainlog_ref as R


class FakeStore:
    """What bucket_segments reads of a gfv.engine.GradStore: off, numel(), skip - offsets 16-byte aligned like the real one."""

    def __init__(self, sizes, skip=()):
        self.off, self._n, off = {}, dict(sizes), 0
        for n, k in sizes:
            self.off[n] = off
            off += (k + 3) // 4 * 4
        self.total, self.skip = off, set(skip)

    def numel(self, n):
        return self._n[n]


# ---- ring window -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,c", [(0, 5), (3, 5), (5, 5), (13, 5), (11, 4), (1, 1), (7, 1)])
def test_ring_window(n, c):
    from gfv.trainlog import ring_window
    first, held, dropped, order = ring_window(n, c)
    ring = [None] * c
    for o in range(n):                      # what the device does: row = ordinal mod capacity
        ring[o % c] = o
    assert held == min(n, c) and dropped == n - held == first
    assert [ring[r] for r in order] == list(range(first, n))


def test_parse_rows_of_a_wrapped_ring():
    from gfv import lib as L
    from gfv.trainlog import HEADER_WORDS, parse_rows, row_words
    cap, MG, K = 4, 3, 2
    rw = row_words(MG, K)
    assert rw == 16 + 16 + 12 and row_words(2, 0) == 16 + 10 and row_words(8, 1) == 16 + 40 + 6
    words = np.zeros(HEADER_WORDS + cap * rw, dtype=np.int32)
    n = 2 * cap + 3
    words[0:2] = np.array([n], dtype=np.int64).view(np.int32)
    rows = words[HEADER_WORDS:].reshape(cap, rw)
    for o in range(n):
        r = rows[o % cap]
        r[:] = 0
        r[0:2] = np.array([o], dtype=np.int64).view(np.int32)
        r[2:5] = np.array([o + 1, 0.5 * o, 1e-3], dtype=np.float32).view(np.int32)
        r[5] = 2
        r[6:8] = np.array([np.nan, 1.0], dtype=np.float32).view(np.int32)
        r[9], r[10] = 1, 1
        r[16:16 + 8] = np.arange(8, dtype=np.float32).view(np.int32) + o
        r[16 + 12:16 + 15] = [o, o + 1, -1]
        r[32:32 + 12] = (np.arange(6, dtype=np.float64) + 10 * o).view(np.int32)
    got = parse_rows(words, cap, MG, K)
    assert got.dropped == n - cap and got.ordinal.tolist() == list(range(n - cap, n))
    assert got.adam_t.tolist() == [o + 1 for o in range(n - cap, n)] and got.B.tolist() == [2] * cap
    assert np.isnan(got.norm).all() and got.coef.tolist() == [1.0] * cap and got.applied.tolist() == [1] * cap
    assert got.terms.shape == (cap, MG, 4) and (got.terms[:, 2] == 0).all()
    assert got.entries[-1].tolist() == [n - 1, n, -1]
    assert got.grad_sumsq[-1].tolist() == [10.0 * (n - 1), 10.0 * (n - 1) + 3] and got.param_sumsq[0, 1] == 10.0 * (n - cap) + 4
    assert got.grad_nonfinite.dtype == np.int64 and got.grad_nonfinite[-1].tolist() == [10 * (n - 1) + 2, 10 * (n - 1) + 5]
    assert L.TRAIN_LOG_HEAD == 16


def test_derive_is_float64_host_arithmetic():
    from gfv.trainlog import TrainLogRows, derive
    terms = np.zeros((2, 3, 4), dtype=np.float32)
    terms[0, 0] = [1e-3, 2e-3, 3e-3, 4e-3]
    terms[1, :2] = [[1e-3, 2e-3, 3e-3, 4e-3], [0.0, 0.0, 0.0, 0.0]]
    blank = np.zeros(2)
    rows = TrainLogRows(blank, blank, blank, blank, np.array([1, 2], dtype=np.int32), blank, blank, blank, blank, blank, terms,
                        np.zeros((2, 3), np.int32), blank, blank, blank, 0)
    lb, obj = derive(rows, (6e4, 5e4, 5e4))
    t = terms[0, 0].astype(np.float64)
    want = 5e4 * t[3] + 6e4 * t[0] + 5e4 * (t[1] + t[2])
    assert lb[0, 0] == want and np.isnan(lb[0, 1:]).all() and np.isnan(lb[1, 2])
    assert obj[0] == math.log(want) and obj[1] == -math.inf


# ---- buckets -----------------------------------------------------------------------------------------------------------------------
def _store():
    return FakeStore([("enc.a.w", 8), ("enc.a.b", 3), ("enc.b.w", 4), ("proc.0.w", 16), ("unused.w", 8), ("proc.0.b", 4),
                      ("dec.w", 12), ("dec.b", 3), ("enc_late", 5), ("empty", 0)], skip={"unused.w"})


def test_bucket_construction():
    from gfv.trainlog import bucket_segments, bucket_tables
    st = _store()
    # offsets: enc.a.w 0, enc.a.b 8 (3 + 1 pad), enc.b.w 12, proc.0.w 16, unused.w 32, proc.0.b 40, dec.w 44, dec.b 56, enc_late 60
    got = dict(bucket_segments(st, ["enc.", "proc.", "enc"]))
    assert list(got) == ["enc.", "proc.", "enc", "rest"]
    assert got["enc."] == [(0, 11), (12, 4)]                  # adjacent merged (0..8 + 8..11), the padding word 11 left out
    assert got["proc."] == [(16, 16), (40, 4)]                # the skipped parameter between them is left out
    assert got["enc"] == [(60, 5)]                            # "enc.a.w" went to the FIRST prefix it matches
    assert got["rest"] == [(44, 15)]                          # dec.w and dec.b lie back to back: one segment
    # frozen names are left out; a rest that is empty is dropped
    got = dict(bucket_segments(st, ["enc", "proc.", "dec"], exclude={"enc.a.b", "dec.b"}))
    assert list(got) == ["enc", "proc.", "dec"]
    assert got["enc"] == [(0, 8), (12, 4), (60, 5)] and got["dec"] == [(44, 12)]
    # None: one bucket over every live parameter, the guard's segments
    from gfv.guard import segments
    assert bucket_segments(st, None) == [("all", segments(st))]
    with pytest.raises(ValueError, match="matches no live parameter"):
        bucket_segments(st, ["enc.", "nothing"])
    with pytest.raises(ValueError, match="matches no live parameter"):
        bucket_segments(st, ["dec."], exclude={"dec.w", "dec.b"})
    with pytest.raises(ValueError, match="no live parameter"):
        bucket_segments(FakeStore([("a", 4)], skip={"a"}), None)
    segs, tab, n_chunks = bucket_tables([("a", [(0, 1024), (2048, 1)]), ("b", [(4096, 5)]), ("c", [(8192, 2048)])])
    assert segs == [[0, 1024], [2048, 1], [4096, 5], [8192, 2048]]
    assert tab == [[0, 2, 0, 1025], [2, 3, 2, 5], [3, 4, 3, 2048]] and n_chunks == 5


def test_argument_checks():
    from gfv.trainlog import TrainLog, check_args, make_log
    assert check_args(16, 3, None) == (16, 3, None) and check_args(1, 64, ("a", "b")) == (1, 64, ["a", "b"])
    for bad in (dict(capacity=0), dict(capacity=-4), dict(capacity=2.5), dict(capacity=True), dict(max_graphs=0),
                dict(max_graphs=65), dict(buckets=[]), dict(buckets="encoder"), dict(buckets=["a", ""]), dict(buckets=["a", "a"]),
                dict(buckets=["a", 3]), dict(buckets=["rest"]), dict(buckets=[f"p{i}." for i in range(32)])):
        kw = dict(capacity=8, max_graphs=2, buckets=None)
        kw.update(bad)
        with pytest.raises(ValueError):
            check_args(**kw)
        with pytest.raises(ValueError):
            TrainLog(**kw)
    assert make_log(None, 4) is None
    lg = make_log(32, 4)
    assert (lg.capacity, lg.max_graphs, lg.prefixes) == (32, 4, None) and make_log(lg, 9) is lg
    lg = make_log({"capacity": 7, "buckets": ["x."]}, 5)
    assert (lg.capacity, lg.max_graphs, lg.prefixes) == (7, 5, ["x."])
    for bad in (True, 2.0, "16", [16]):
        with pytest.raises(ValueError):
            make_log(bad, 4)
    with pytest.raises(ValueError):
        make_log(0, 4)
    with pytest.raises(RuntimeError, match="not attached"):
        TrainLog().read()


# ---- the restated order ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 63, 1024, 1025, 5000, 70 * 1024 + 17])
def test_ref_order_against_fsum(n):
    """Any order of a double sum of n non-negative terms lies within n * 2^-53 relative of the exact sum."""
    rng = np.random.default_rng(n)
    x = (rng.standard_normal(n) * 10.0 ** rng.uniform(-3, 3, n)).astype(np.float32)
    sq = x.astype(np.float64) ** 2
    exact = math.fsum(sq.tolist())
    got = R.ordered_sum(sq)
    assert abs(got - exact) <= n * 2.0 ** -53 * exact
    # segments only say where the elements lie: the sum is a function of the logical order
    flat = np.zeros(n + 40, dtype=np.float32)
    cut = n // 3
    flat[3:3 + cut] = x[:cut]
    flat[3 + cut + 7:n + 10] = x[cut:]
    segs = [(3, cut), (3 + cut + 7, n - cut)] if cut else [(10, n)]
    gs, ps, bad = R.bucket_sums(flat, flat[::-1].copy(), segs)
    assert R.same_bits(gs, got) and bad == 0
    assert ps == R.ordered_sum(R.gather(flat[::-1].copy(), segs).astype(np.float64) ** 2)


def test_ref_counts_nonfinite():
    g = np.ones(3000, dtype=np.float32)
    g[[5, 1030, 2999]] = [np.inf, np.nan, -np.inf]
    gs, ps, bad = R.bucket_sums(g, np.ones_like(g), [(0, 3000)])
    assert bad == 3 and not np.isfinite(gs) and ps == 3000.0


# ---- the entry points refuse bad arguments before anything is launched -------------------------------------------------------------
def test_entry_points_refuse_bad_arguments_without_a_gpu():
    from gfv import lib
    h = lib.load()
    ERR = -1
    buf = (C.c_int64 * 64)()                      # host memory standing in for every pointer: nothing is launched
    p = C.addressof(buf)
    ent = (C.c_int32 * 4)(0, 1, -1, 2)

    def append(ring=p, capacity=4, max_graphs=4, K=1, cursor=p, state=p, hyper=p, loss=p, losses=p, B=3, guard=None, accum=None,
               entry=ent, sums=p, table=p, n_entries=3):
        return h.gfv_train_log_append(ring, capacity, max_graphs, K, cursor, state, hyper, loss, losses, B, guard, accum, entry,
                                      sums, table, n_entries, None)
    assert append(ring=None) == ERR
    assert append(capacity=0) == ERR and append(capacity=-1) == ERR
    assert append(B=0) == ERR and append(B=5) == ERR
    assert append(max_graphs=lib.POOL_MAX_GRAPHS + 1, B=1) == ERR and append(max_graphs=0) == ERR
    assert append(entry=(C.c_int32 * 3)(0, 3, 1)) == ERR                 # an entry at n_entries
    assert append(entry=(C.c_int32 * 3)(0, -2, 1)) == ERR                # ... and below -1
    assert append(entry=(C.c_int32 * 3)(0, -2, 1), table=None) == ERR
    assert append(K=-1) == ERR and append(K=lib.TRAIN_LOG_MAX_BUCKETS + 1) == ERR
    assert append(K=2, sums=None) == ERR                                 # a NULL bucket table with K above 0
    assert append(cursor=None) == ERR and append(state=None) == ERR and append(hyper=None) == ERR
    assert append(loss=None) == ERR and append(losses=None) == ERR
    assert append(n_entries=0) == ERR and append(ring=p + 4) == ERR

    def norms(g=p, pp=p, segs=p, tab=p, K=2, n_chunks=3, sums=p, ws=p):
        return h.gfv_train_log_norms(g, pp, segs, tab, K, n_chunks, sums, ws, None)
    assert norms(K=-1) == ERR and norms(K=lib.TRAIN_LOG_MAX_BUCKETS + 1) == ERR
    assert norms(segs=None) == ERR and norms(tab=None) == ERR and norms(g=None) == ERR and norms(pp=None) == ERR
    assert norms(sums=None) == ERR and norms(ws=None) == ERR and norms(ws=p + 4) == ERR and norms(n_chunks=0) == ERR
    assert norms(K=0, segs=None, tab=None, sums=None, ws=None, n_chunks=0) == 0       # K = 0: nothing to do, nothing launched
    assert h.gfv_train_log_row_words(0, 1) == ERR and h.gfv_train_log_row_words(65, 1) == ERR and h.gfv_train_log_row_words(4, -1) == ERR
    from gfv.trainlog import row_words
    for mg, k in ((1, 0), (2, 1), (3, 5), (8, 4), (64, 32)):
        assert h.gfv_train_log_row_words(mg, k) == row_words(mg, k)
    for n in (0, 1, 1024, 1025, 10 ** 7):
        assert h.gfv_train_log_chunks(n) == (n + lib.TRAIN_LOG_CHUNK - 1) // lib.TRAIN_LOG_CHUNK
        assert h.gfv_train_log_workspace_bytes(h.gfv_train_log_chunks(n)) == 8 + 24 * h.gfv_train_log_chunks(n)


def test_log_none_is_the_default_and_keywords_exist():
    import inspect
    from gfv.pool_trainer import PoolTrainStep
    from gfv.trainer import TrainStep
    for cls in (TrainStep, PoolTrainStep):
        prm = inspect.signature(cls.__init__).parameters["log"]
        assert prm.default is None and prm.kind is inspect.Parameter.KEYWORD_ONLY
