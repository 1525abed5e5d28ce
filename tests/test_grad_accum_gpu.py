"""Gradient accumulation on the GPU (include/gfv.h gfv_grad_accum_dev / gfv_grad_guard_accum_dev / gfv_adam_step_accum_dev,
gfv/accum.py).  The kernel alone on random vectors - exact where the arithmetic is exact, against float64 with the
rounding count of the stated arithmetic where it is not, the device record after every launch, a stale accumulator, hold
launches that leave no trace and apply launches that are the existing entry points bit for bit - and through `TrainStep` and
`PoolTrainStep`: twins started from ONE state_dict taken after the Normalizer stopped accumulating, so that a graph's loss does
not depend on the batch it travels in."""
import struct

import numpy as np
import pytest
import torch

import cases
from oracle import fvgn_oracle as O

pytestmark = pytest.mark.gpu

ACC_PASS = 512 * 256 * 4          # floats one pass of the full accumulate grid covers (csrc/misc.hip ACC_MAX_WGS * ACC_TPB * 4)
N_BIG = 2 * ACC_PASS + 1203       # more than a pass of the full grid, n % 4 == 3
CLIP, SKIP_NONFINITE = 1, 2
EPS = 2.0 ** -24


# ---- the C ABI on flat buffers ---------------------------------------------------------------------------------------------
def _lib():
    from gfv import lib as L
    return L, L.load()


def _new_record(steps):
    rec = torch.zeros(8, dtype=torch.int32)
    rec[0] = steps
    return rec.cuda().view(torch.float32)


def _read(rec):
    torch.cuda.synchronize()
    f = rec.detach().cpu().clone()
    i = f.view(torch.int32)
    return dict(steps=int(i[0]), micro=int(i[1]), graphs=int(i[2]), apply=int(i[3]), loss_sum=f[4].clone(), loss_mean=f[5].clone(),
                closed=int(i[6]), counter=int(i[7]))


def _accum(g, acc, n, B, loss, rec):
    L, lib = _lib()
    L.check(lib.gfv_grad_accum_dev(g.data_ptr(), acc.data_ptr(), n, B, loss.data_ptr(), rec.data_ptr(), L.stream_ptr()), "grad_accum")


def _vectors(n, k, seed=7):
    gen = torch.Generator().manual_seed(seed)
    return [torch.randn(n, generator=gen) * (0.5 + j) for j in range(k)]


def _f32(x):
    return torch.tensor(x, dtype=torch.float32)


def _exact_run(n, acc, offset=0):
    """k = 4, B = 2 each -> (finished g, the record after every launch).  `offset`: g and acc start that many floats into their
    allocations (1: neither is 16-byte aligned, every element takes the by-element path)."""
    gs = _vectors(n, 4)
    losses = [_f32(0.75), _f32(1.5), _f32(-0.25), _f32(3.0)]
    rec = _new_record(4)
    buf = torch.zeros(n + offset, device="cuda")
    g = buf[offset:]
    records = []
    for j in range(4):
        g.copy_(gs[j])
        _accum(g, acc, n, 2, losses[j].cuda(), rec)
        records.append(_read(rec))
    return g.cpu(), gs, losses, records


@pytest.mark.parametrize("n,offset", [(1, 0), (3, 0), (1027, 0), (1027, 1), (N_BIG, 0)],
                         ids=["1", "3", "1027", "1027_misaligned", "beyond_one_grid_pass"])
def test_exact_accumulation_and_the_record_after_every_launch(n, offset):
    acc = torch.zeros(n + offset, device="cuda")[offset:]
    got, gs, losses, records = _exact_run(n, acc, offset)
    want = (((2 * gs[0] + 2 * gs[1]) + 2 * gs[2]) + 2 * gs[3]) / 8      # torch fp32: every product and the final scale are exact
    assert want.dtype == torch.float32
    assert torch.equal(got, want)
    s = _f32(0.0)
    for j, r in enumerate(records):
        s = s + 2 * losses[j]
        assert r["steps"] == 4 and r["counter"] == 0, (j, r)
        if j < 3:
            assert (r["micro"], r["graphs"], r["apply"], r["closed"]) == (j + 1, 2 * (j + 1), 0, 0), (j, r)
            assert torch.equal(r["loss_sum"], s), (j, r)
        else:
            assert (r["micro"], r["graphs"], r["apply"], r["closed"]) == (0, 0, 1, 1), r
            assert float(r["loss_sum"]) == 0.0 and torch.equal(r["loss_mean"], s / 8), r
    # the accumulator after the close is the sum of the first three: the closing launch does not write it
    torch.cuda.synchronize()
    assert torch.equal(acc.cpu(), (2 * gs[0] + 2 * gs[1]) + 2 * gs[2])


@pytest.mark.parametrize("n", [1027, N_BIG])
def test_uneven_graph_counts_against_float64(n):
    """B = 3, 1, 2.  Per element: k products and k - 1 sums of the accumulation, one division - at most 2k roundings, each at most
    2^-24 of a partial sum that is itself at most sum_i B_i |g_i| (1 + small); the bound (2k + 2) 2^-24 sum_i B_i |g_i| / n_graphs
    leaves the second-order terms their room.  loss_mean: the same count on positive losses (no cancellation), 4 2^-24 relative."""
    Bs, k = (3, 1, 2), 3
    gs = _vectors(n, k, seed=19)
    losses = [_f32(0.3), _f32(1.7), _f32(0.9)]
    rec = _new_record(k)
    g, acc = torch.zeros(n, device="cuda"), torch.zeros(n, device="cuda")
    for j in range(k):
        g.copy_(gs[j])
        _accum(g, acc, n, Bs[j], losses[j].cuda(), rec)
    r = _read(rec)
    assert (r["micro"], r["graphs"], r["apply"], r["closed"]) == (0, 0, 1, 1)
    want = sum(B * x.double() for B, x in zip(Bs, gs)) / sum(Bs)
    bound = (2 * k + 2) * EPS * sum(B * x.double().abs() for B, x in zip(Bs, gs)) / sum(Bs)
    err = (g.cpu().double() - want).abs()
    print(f"uneven n={n}: worst error / bound {float((err / bound.clamp_min(1e-300)).max()):.3f}")
    assert bool((err <= bound).all())
    mean64 = sum(B * float(l) for B, l in zip(Bs, losses)) / sum(Bs)
    rel = abs(float(r["loss_mean"]) - mean64) / abs(mean64)
    print(f"uneven n={n}: loss_mean relative error {rel:.3e} (bound {4 * EPS:.3e})")
    assert rel <= 4 * EPS


def test_a_stale_accumulator_does_not_leak_and_a_nan_gradient_does_arrive():
    n = 1027
    acc = torch.full((n,), float("nan"), device="cuda")
    got, gs, _, records = _exact_run(n, acc)
    assert bool(torch.isfinite(got).all())
    assert torch.equal(got, (((2 * gs[0] + 2 * gs[1]) + 2 * gs[2]) + 2 * gs[3]) / 8)
    # a NaN in the MIDDLE micro-gradient reaches the finished g (and only its own slot)
    rec, g, loss = _new_record(3), torch.zeros(n, device="cuda"), _f32(1.0).cuda()
    gs = _vectors(n, 3, seed=5)
    gs[1][5] = float("nan")
    for j in range(3):
        g.copy_(gs[j])
        _accum(g, acc, n, 1, loss, rec)
    out = g.cpu()
    assert bool(torch.isnan(out[5])) and int(torch.isnan(out).sum()) == 1
    assert _read(rec)["closed"] == 1


N_ADAM = 70001     # 137 workgroups of the Adam launch, 69 of the norm launch, 69 of the accumulate launch


def _hyper(lr=1e-3):
    return torch.tensor([lr, 0.9, 0.999, 1e-8, 1.0, 0.0, 0.0, 0.0], dtype=torch.float32, device="cuda")


def _guard_record(max_norm, policy):
    rec = torch.zeros(8, dtype=torch.int32)
    rec[0] = struct.unpack("i", struct.pack("f", max_norm))[0]
    rec[1] = policy
    return rec.cuda().view(torch.float32)


class _Flat:
    """p, m, v, state and guard record of one Adam run over n slots; `twin()` is a bit copy."""

    def __init__(self, n, seed=3):
        L, lib = _lib()
        gen = torch.Generator().manual_seed(seed)
        self.n = n
        self.p = torch.randn(n, generator=gen).cuda()
        self.m, self.v = torch.zeros(n, device="cuda"), torch.zeros(n, device="cuda")
        self.state = torch.zeros(16, device="cuda")
        L.check(lib.gfv_adam_state_init(self.state.data_ptr(), 0.9, 0.999, 0.0, L.stream_ptr()), "state_init")
        self.guard = _guard_record(3.0, CLIP | SKIP_NONFINITE)
        self.ws = torch.zeros(lib.gfv_grad_guard_workspace_bytes() // 8, dtype=torch.float64, device="cuda")
        self.table = torch.tensor([0, n], dtype=torch.int64).cuda()

    def twin(self):
        t = object.__new__(_Flat)
        t.n, t.table = self.n, self.table
        for name in ("p", "m", "v", "state", "guard", "ws"):
            setattr(t, name, getattr(self, name).clone())
        return t

    def bits(self):
        torch.cuda.synchronize()
        return [t.detach().cpu().view(torch.int32).clone() for t in (self.p, self.m, self.v, self.state, self.guard)]

    # the existing entry points
    def plain(self, g, hyper):
        L, lib = _lib()
        L.check(lib.gfv_adam_step_dev(self.p.data_ptr(), g.data_ptr(), self.m.data_ptr(), self.v.data_ptr(), self.n,
                                      self.state.data_ptr(), hyper.data_ptr(), L.stream_ptr()), "adam")

    def guarded(self, g, hyper):
        L, lib = _lib()
        L.check(lib.gfv_grad_guard_dev(g.data_ptr(), self.table.data_ptr(), 1, self.n, hyper.data_ptr(), self.guard.data_ptr(),
                                       self.ws.data_ptr(), L.stream_ptr()), "grad_guard")
        L.check(lib.gfv_adam_step_guarded_dev(self.p.data_ptr(), g.data_ptr(), self.m.data_ptr(), self.v.data_ptr(), self.n,
                                              self.state.data_ptr(), hyper.data_ptr(), self.guard.data_ptr(), L.stream_ptr()),
                "adam_guarded")

    # the hold-aware forms
    def accum_forms(self, g, hyper, rec, with_guard):
        L, lib = _lib()
        if with_guard:
            L.check(lib.gfv_grad_guard_accum_dev(g.data_ptr(), self.table.data_ptr(), 1, self.n, hyper.data_ptr(),
                                                 self.guard.data_ptr(), self.ws.data_ptr(), rec.data_ptr(), L.stream_ptr()),
                    "grad_guard_accum")
        L.check(lib.gfv_adam_step_accum_dev(self.p.data_ptr(), g.data_ptr(), self.m.data_ptr(), self.v.data_ptr(), self.n,
                                            self.state.data_ptr(), hyper.data_ptr(), self.guard.data_ptr() if with_guard else None,
                                            rec.data_ptr(), L.stream_ptr()), "adam_accum")


def _same(a, b):
    return len(a) == len(b) and all(torch.equal(x, y) for x, y in zip(a, b))


@pytest.mark.parametrize("with_guard", [True, False], ids=["guarded", "unguarded"])
def test_hold_leaves_no_trace_and_apply_is_the_plain_step(with_guard):
    n = N_ADAM
    hyper = _hyper()
    g0, g1, g2 = [x.cuda() for x in _vectors(n, 3, seed=11)]
    a = _Flat(n)
    a.guarded(g0, hyper)              # one real step first: t = 1, moments and guard[2..7] hold something to lose
    assert a.bits()[4][5] == 1        # (max_norm 3.0 is far below the norm of 70001 normal values: it was clipped)
    rec, acc, loss = _new_record(2), torch.full((n,), float("nan"), device="cuda"), _f32(1.0).cuda()
    before = a.bits()
    g = g1.clone()
    _accum(g, acc, n, 1, loss, rec)
    assert _read(rec)["apply"] == 0
    a.accum_forms(g, hyper, rec, with_guard)
    assert _same(before, a.bits())    # p, m, v, all 16 words of state, all 8 of the guard record
    assert torch.equal(g, g1)         # (a hold does not touch g either)
    g = g2.clone()
    _accum(g, acc, n, 3, loss, rec)
    assert _read(rec)["apply"] == 1
    assert torch.equal(g.cpu(), (g1.cpu() + 3 * g2.cpu()) / 4)
    b = a.twin()
    a.accum_forms(g, hyper, rec, with_guard)
    if with_guard:
        b.guarded(g, hyper)
    else:
        b.plain(g, hyper)
    assert _same(a.bits(), b.bits())
    assert float(a.state[0]) == 2.0 and not _same(before[:3], a.bits()[:3])
    if with_guard:
        assert int(a.bits()[4][5]) == 2      # clipped: once for the first step, once for the apply, none for the hold


# ---- through the step objects ----------------------------------------------------------------------------------------------
LR = 1e-3


def _graphs(name="cyl_cavity_b2"):
    return tuple(g.clone().to("cuda") for g in cases.make_graphs(name))


def _fresh_model(dataset_size):
    from FVMmodel.importer import NNmodel
    from gfv.params import default_params
    P = O.init_parameters(cases.WEIGHT_SEED)
    m = NNmodel(default_params(dataset_size=dataset_size))
    sd = m.state_dict()
    for k, v in P.items():
        sd[k].copy_(v)
    m.load_state_dict(sd)
    return m


@pytest.fixture(scope="module")
def frozen_sd():
    """Model state after the Normalizer's accumulation has ended (dataset_size = 3: two accumulating steps), computed once."""
    from gfv.trainer import TrainStep
    model = _fresh_model(3).cuda()
    ts = TrainStep(model, _graphs(), lr=LR, use_graph=False)
    for _ in range(3):
        ts.step()
    torch.cuda.synchronize()
    assert not model.node_norm.should_accumulate() and float(model.node_norm.acc_sum.abs().sum()) > 0.0
    return {k: v.detach().cpu().clone() for k, v in model.state_dict().items()}


def _model(sd):
    m = _fresh_model(3)
    m.load_state_dict(sd)
    m = m.cuda()
    assert not m.node_norm.should_accumulate()
    return m


def _named_bits(ts):
    """Parameters and moments of the named tensors (the alignment padding of the flat buffers is not state) + the Adam state."""
    torch.cuda.synchronize()
    ns = ts.named_state()
    return [torch.cat([v[j].reshape(-1) for v in ns.values()]).detach().cpu().view(torch.int32) for j in range(3)] + \
        [ts.adam_state.detach().cpu().view(torch.int32).clone()]


@pytest.mark.parametrize("mode", [False, "list", True], ids=["eager", "list", "hipgraph"])
def test_trainstep_two_micro_steps_of_one_batch_are_one_plain_step(frozen_sd, mode):
    """Fixed batch, B = 2: (2g + 2g) / 4 is g exactly, so 2m steps with accum_steps=2 are m plain steps bit for bit."""
    from gfv.trainer import TrainStep
    m = 4
    plain = TrainStep(_model(frozen_sd), _graphs(), lr=LR, use_graph=mode)
    for _ in range(m):
        plain.step()
    ts = TrainStep(_model(frozen_sd), _graphs(), lr=LR, use_graph=mode, accum_steps=2)
    assert ts.accum_steps == 2 and ts.accum_pending == 0
    for j in range(2 * m):
        before = _named_bits(ts)
        loss = ts.step()
        assert loss is ts.loss
        if j % 2 == 0:        # the first micro-step of every pair holds
            assert _same(before, _named_bits(ts)), j
            assert ts.accum_pending == 1
        else:
            assert not torch.equal(before[0], _named_bits(ts)[0]), j
            assert ts.accum_pending == 0
    assert _same(_named_bits(plain), _named_bits(ts))
    assert float(ts.adam_state[0]) == m
    st = ts.accum_stats()
    assert set(st) == {"micro", "graphs", "loss_mean", "closed"}
    assert st["micro"] == 0 and st["graphs"] == 0 and st["closed"] == m      # (a hipGraph warm-up counts nothing)
    assert st["loss_mean"] == float(ts.loss)                                  # (2 l + 2 l) / 4
    if mode == "list":
        assert len(ts._lists) >= 1
    assert set(ts.state_dict()) == set(plain.state_dict())                   # an open accumulation is not state


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


def _four_mesh_pool():
    from gfv.pool import DevicePool
    return DevicePool(*_meshes())


def _variant_pool():
    from gfv import meshgen
    from gfv.pool import DevicePool
    raw = meshgen.raw_tri_channel_cylinder(nx=30, ny=6, quad_fraction=0.0, seed=21)
    m = meshgen.finish_mesh(raw, U=0.15)
    pool = DevicePool([m], [meshgen.random_fields(m, seed=5)])
    for j in range(5):
        pool.add_variant(0, fields=meshgen.random_fields(m, seed=11 + j), U=0.12 + 0.04 * j, mu=1e-3 * (1 + j), dt=0.01 * (2 + j))
    return pool


def _two_size_pool():
    from gfv import meshgen
    from gfv.pool import DevicePool
    raws = [meshgen.raw_tri_channel_cylinder(nx=30, ny=6, seed=21), meshgen.raw_quad_cavity(n=7, jitter=0.1, tri_fraction=0.3, seed=13)]
    ms = [meshgen.finish_mesh(r, U=U) for r, U in zip(raws, (0.15, 1.0))]
    return DevicePool(ms, [meshgen.random_fields(m, seed=30 + i) for i, m in enumerate(ms)])


def test_pool_micro_batches_give_the_big_batch_gradient(frozen_sd):
    from gfv.pool import batch_signature
    from gfv.pool_trainer import PoolTrainStep
    big = PoolTrainStep(_model(frozen_sd), _four_mesh_pool(), max_graphs=4, lr=LR, use_graph=False)
    big.step([0, 1, 2, 3])
    torch.cuda.synchronize()
    ref = big.flat_g.detach().cpu().double()
    names = [n for n in big.G.off if n not in big.G.skip and big.G.numel(n) > 0]
    gscale = max(float(ref[big.G.off[n]:big.G.off[n] + big.G.numel(n)].abs().max()) for n in names)
    assert gscale > 0.0
    assert len({batch_signature(big.pool.sizes, [i]) for i in range(4)}) == 4
    for k, mg, seq in ((2, 2, ([0, 1], [2, 3])), (4, 1, ([0], [1], [2], [3]))):
        ts = PoolTrainStep(_model(frozen_sd), _four_mesh_pool(), max_graphs=mg, lr=LR, use_graph=False, accum_steps=k)
        for j, idx in enumerate(seq):
            assert ts.accum_pending == j
            ts.step(idx)
        st = ts.accum_stats()
        assert ts.accum_pending == 0 and st["graphs"] == 0 and st["micro"] == 0 and st["closed"] == 1
        got = ts.flat_g.detach().cpu().double()
        worst = 0.0
        for n in names:
            off, cnt = ts.G.off[n], ts.G.numel(n)
            assert off == big.G.off[n]
            err = float((got[off:off + cnt] - ref[off:off + cnt]).abs().max())
            bound = 1e-4 * float(ref[off:off + cnt].abs().max()) + 1e-6 * gscale
            worst = max(worst, err / bound)
            assert err < bound, (k, n, err, bound)
        print(f"micro against big batch, k={k}: worst error / bound {worst:.3f}")
        assert abs(st["loss_mean"] - float(big.loss)) <= 1e-5 * max(abs(float(big.loss)), 1.0)
        assert float(ts.adam_state[0]) == 1.0


def test_one_list_serves_every_phase(frozen_sd):
    """k = 3 and two signatures alternating: a signature meets every phase, a list recorded in one phase is replayed in the
    other two.  A phase baked into a list gives other parameters than the eager twin."""
    from gfv.pool_trainer import PoolTrainStep
    seq = [[k % 2] for k in range(18)]
    eager = PoolTrainStep(_model(frozen_sd), _two_size_pool(), max_graphs=1, lr=LR, use_graph=False, accum_steps=3)
    ts = PoolTrainStep(_model(frozen_sd), _two_size_pool(), max_graphs=1, lr=LR, use_graph="list", accum_steps=3)
    replayed_in = set()
    for j, idx in enumerate(seq):
        eager.step(idx)
        was = ts.stats()["replayed"]
        ts.step(idx)
        if ts.stats()["replayed"] > was:
            replayed_in.add(j % 3)
    assert _same(_named_bits(eager), _named_bits(ts))
    st = ts.stats()
    assert st["lists"] == 2 and st["recorded"] == 2 and st["replayed"] > 0, st
    assert replayed_in == {0, 1, 2}
    assert float(ts.adam_state[0]) == 6.0 and ts.accum_stats()["closed"] == 6


def _segment_norm(ts):
    """fp32 rounding of the float64 norm of flat_g over the guard's segments."""
    from gfv.guard import segments
    torch.cuda.synchronize()
    g = ts.flat_g.detach().cpu().double()
    parts = torch.cat([g[o:o + k] for o, k in segments(ts.G)])
    return np.float32(np.sqrt(float((parts * parts).sum())))


def test_the_guard_sees_the_finished_mean_gradient_once_per_optimiser_step(frozen_sd):
    from gfv.pool_trainer import PoolTrainStep
    ts = PoolTrainStep(_model(frozen_sd), _variant_pool(), max_graphs=1, lr=LR, use_graph="list", accum_steps=2, max_grad_norm=1e30)
    ts.step([0])
    assert ts.guard_stats()["norm"] == 0.0 and ts.guard_stats()["clipped"] == 0      # a hold: the record is as it was made
    ts.step([1])
    first = ts.guard_stats()
    assert first["norm"] > 0.0 and first["clipped"] == 0 and first["coef"] == 1.0
    ts.max_grad_norm = 0.01 * first["norm"]       # (well below: the norm moves from step to step, as in tests/test_grad_guard_gpu.py)
    clipped = 0
    for j in range(8):                            # warm-up, recording and replays of the one list
        before = ts.guard_stats()
        ts.step([(2 + j) % 6])
        st = ts.guard_stats()
        if j % 2 == 0:
            assert st == before, j                # hold: norm, coefficient, decision and counts untouched
        else:
            clipped += 1
            assert st["clipped"] == clipped and st["decision"] == CLIP and st["coef"] < 1.0, (j, st)
            want = _segment_norm(ts)
            got = np.float32(st["norm"])
            assert abs(float(got) - float(want)) <= float(np.spacing(want)), (got, want)
    assert clipped == 4 and ts.stats()["replayed"] > 0 and ts.stats()["lists"] == 1
    assert float(ts.adam_state[0]) == 5.0


def test_a_non_finite_micro_batch_leaves_the_whole_optimiser_step_out(frozen_sd):
    from gfv.pool_trainer import PoolTrainStep

    def make():
        pool = _variant_pool()
        return pool, PoolTrainStep(_model(frozen_sd), pool, max_graphs=1, lr=LR, use_graph="list", accum_steps=2, skip_nonfinite=True)
    (pool, ts), (_, twin) = make(), make()
    for t in (ts, twin):
        t.step([0])
        t.step([1])
    assert _same(_named_bits(ts), _named_bits(twin)) and float(ts.adam_state[0]) == 1.0
    before = _named_bits(ts)
    keep = pool.x[2].clone()
    pool.x[2][:, 0:3] = float("inf")
    ts.step([2])                                  # the bad micro-batch opens the accumulation ...
    pool.x[2].copy_(keep)
    ts.step([3])                                  # ... and a healthy one closes it: the mean is not finite
    st = ts.guard_stats()
    assert st["skipped_nonfinite"] == 1 and st["decision"] == SKIP_NONFINITE and not np.isfinite(st["norm"])
    assert _same(before, _named_bits(ts)) and float(ts.adam_state[0]) == 1.0
    assert ts.accum_stats()["closed"] == 2 and ts.accum_pending == 0
    for t in (ts, twin):                          # the next accumulation: as if the bad entry had never been seen
        t.step([4])
        t.step([2])
    assert _same(_named_bits(ts), _named_bits(twin)) and float(ts.adam_state[0]) == 2.0
    assert ts.guard_stats()["skipped_nonfinite"] == 1 and twin.guard_stats()["skipped_nonfinite"] == 0


def test_accum_steps_is_an_attribute_and_a_loaded_state_starts_a_new_accumulation(frozen_sd):
    from gfv.pool_trainer import PoolTrainStep
    model = _model(frozen_sd)
    ts = PoolTrainStep(model, _variant_pool(), max_graphs=1, lr=LR, use_graph="list", accum_steps=3)
    start = _named_bits(ts)
    ts.step([0])
    ts.step([1])
    st = ts.accum_stats()
    assert ts.accum_pending == 2 and st["micro"] == 2 and st["graphs"] == 2 and st["closed"] == 0
    ts.accum_steps = 2                            # mid-accumulation: the open one is dropped, host and device
    st = ts.accum_stats()
    assert ts.accum_steps == 2 and ts.accum_pending == 0 and st["micro"] == 0 and st["graphs"] == 0 and st["closed"] == 0
    assert _same(start, _named_bits(ts))
    ts.step([2])
    assert ts.accum_pending == 1 and _same(start, _named_bits(ts))
    ts.step([3])
    assert ts.accum_pending == 0 and ts.accum_stats()["closed"] == 1 and float(ts.adam_state[0]) == 1.0
    ts.step([4])
    assert ts.accum_pending == 1 and ts.accum_stats()["micro"] == 1
    ts.load_state_dict(ts.state_dict())           # a loaded state: no open accumulation
    assert ts.accum_pending == 0 and ts.accum_stats()["micro"] == 0 and ts.accum_stats()["graphs"] == 0
    ts.step([0])
    ts.step([1])
    assert ts.accum_stats()["closed"] == 2 and float(ts.adam_state[0]) == 2.0
    assert ts.stats()["lists"] == 1               # seven steps of one signature: recorded at the third
    with pytest.raises(ValueError, match="accum_steps"):
        ts.accum_steps = 0
    # 2 -> 1: the launch sequence changes, the lists go, and the step is the plain step again
    ts.accum_steps = 1
    assert ts.accum_steps == 1 and ts.stats()["lists"] == 0 and ts._accum is None and ts.accum_pending == 0
    ts.load_state_dict(ts.state_dict())           # (both twins form the bias corrections from the step count the same way)
    torch.cuda.synchronize()
    sd = {k: v.detach().cpu().clone() for k, v in model.state_dict().items()}
    plain = PoolTrainStep(_model(sd), _variant_pool(), max_graphs=1, lr=LR, use_graph=False)
    plain.load_state_dict(ts.state_dict())
    assert _same(_named_bits(ts), _named_bits(plain))
    for idx in ([5], [2]):
        ts.step(idx)
        plain.step(idx)
    assert _same(_named_bits(ts), _named_bits(plain)) and float(ts.adam_state[0]) == 4.0
    ts.accum_steps = 2                            # ... and back
    ts.step([0])
    assert ts.accum_pending == 1 and float(ts.adam_state[0]) == 4.0
