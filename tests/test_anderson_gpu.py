"""GPU: Anderson acceleration of the rollout on the device (csrc/anderson.hip, gfv/anderson.py).

Tests 1 - 5 drive the two launches + `gfv_rollout_advance` stand-alone through ctypes on ONE batch of three graphs of 37, 133 and
4161 nodes (a partial chunk; three chunks; 66 chunks, so that the last arriver's fold wraps past lane 63), chunk tables as
gfv/plan.py builds them, with G - the rank-3 linear contraction of tests/anderson_ref.py - evaluated by numpy on the host:

1. every step's depth and flags equal the numpy reference's (driven with the device's own (x_k, g_k)); gamma agrees with
   `numpy.linalg.solve` of the reference's regularised system within 64 eps64 cond || gamma ||; the new uvp_node is within one
   fp32 spacing of the reference mix evaluated with the device's gamma - m = 4, and m = 8 with beta = 0.5, 12 steps each;
2. AA(4) is below a relative residual of 1e-5 by step index 8 (the reference: 6, two steps of margin for the rounding of gamma);
   launches that decide depth 0 leave uvp_node's bits alone;
3. each graph run alone (B = 1) gives the bits it gives inside the batch: table, gamma, iterate;
4. rows whose g never changes keep their bits through 12 accelerated steps (beta = 1 and 0.5);
5. the decisions: GROWTH, NONFINITE (that graph only, no NaN in any gamma), a zero Gram matrix;
6. through `Rollout` on the small fixture model: anderson=0 is today's rollout bit for bit; step 1 of anderson=4 is the plain
   step 1; list mode equals eager mode over 10 steps; reset() reproduces; run(tol) stops on the table's ratio; Dirichlet values
   equal the plain rollout's.  (Of a wall or inflow node only u, v are Dirichlet values - the model's pressure there is free - so
   the whole row x_backup[:, 0:3] is compared on the pressure points, where all three are fixed, and u, v on the others.)
"""
import types

import numpy as np
import pytest
import torch

import anderson_ref as R
import cases
from oracle import fvgn_oracle as O

pytestmark = pytest.mark.gpu
EPS64 = float(np.finfo(np.float64).eps)
STEPS = 12


class Device:
    """The two Anderson launches and gfv_rollout_advance on buffers of its own, G on the host."""

    def __init__(self, sizes, m, beta=1.0, reg=1e-10, restart=10.0, start=0, max_steps=16):
        from gfv.anderson import AndersonState
        dev = torch.device("cuda")
        cb, ce, gcp = R.chunk_tables(sizes)
        self.N, self.B = int(sum(sizes)), len(sizes)
        assert int(ce.max()) <= self.N and int(cb.min()) >= 0 and int(gcp[-1]) == len(cb)
        t = lambda a: torch.from_numpy(a).to(dev)
        self.plan = types.SimpleNamespace(N=self.N, B=self.B, n_chunks=len(cb), chunk_beg=t(cb), chunk_end=t(ce), gchunk_ptr=t(gcp))
        self.aa = AndersonState(self.plan, dev, max_steps, m, beta, reg, restart, start)
        self.max_steps = max_steps
        self.x_backup = torch.zeros((self.N, 12), dtype=torch.float32, device=dev)
        self.x = torch.zeros_like(self.x_backup)
        self.uvp = torch.zeros((self.N, 3), dtype=torch.float32, device=dev)
        self.losses = torch.zeros((self.B, 4), dtype=torch.float32, device=dev)
        self.partial = torch.zeros((len(cb), 2), dtype=torch.float64, device=dev)
        self.history = torch.zeros((max_steps, self.B, 6), dtype=torch.float32, device=dev)
        self.state = torch.zeros(2, dtype=torch.int32, device=dev)
        self.k = 0

    def set_x(self, x):
        self.x_backup[:, 0:3] = torch.from_numpy(np.ascontiguousarray(x)).cuda()

    def get_x(self):
        return self.x_backup[:, 0:3].cpu().numpy().copy()

    def step(self, g):
        """One step with the model's output `g` [N,3] -> (the iterate advanced to, table row [B,4], gamma [B,8])."""
        from gfv import lib as L
        assert self.k < self.max_steps
        pl = self.plan
        self.uvp.copy_(torch.from_numpy(np.ascontiguousarray(g)))
        self.aa.launch(self.uvp, self.x_backup, self.state)
        L.check(L.load().gfv_rollout_advance(
            self.uvp.data_ptr(), self.x_backup.data_ptr(), self.x.data_ptr(), pl.N, pl.chunk_beg.data_ptr(), pl.chunk_end.data_ptr(),
            pl.gchunk_ptr.data_ptr(), pl.n_chunks, pl.B, self.losses.data_ptr(), self.partial.data_ptr(), self.history.data_ptr(),
            self.max_steps, self.state.data_ptr(), L.stream_ptr()), "gfv_rollout_advance")
        torch.cuda.synchronize()
        out = self.uvp.cpu().numpy().copy()
        row = self.aa.table[self.k].cpu().numpy().copy()
        gamma = self.aa.gamma.cpu().numpy().copy()
        self.k += 1
        assert self.state.tolist() == [self.k, 0] and int(self.aa.counter) == 0
        assert np.array_equal(self.get_x().view(np.int32), out.view(np.int32))
        return out, row, gamma


def _run(G, x0, sizes, m, steps=STEPS, **kw):
    """`steps` accelerated steps of G from x0 on the device -> per step (x_k, g_k, out, row, gamma), and the Device."""
    d = Device(sizes, m, **kw)
    d.set_x(x0)
    rec = []
    for _ in range(steps):
        x = d.get_x()
        g = G(x)
        rec.append((x, g) + d.step(g))
    return rec, d


@pytest.fixture(scope="module")
def problem():
    return R.BatchMap()


@pytest.fixture(scope="module")
def batch_run(problem):
    """AA(4), beta = 1 on the batch: shared by tests 1 - 3 (computed once, left unchanged)."""
    return _run(problem, problem.x0, R.SIZES, 4)


def _same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def _check_against_reference(rec, sizes, m, beta):
    ref = R.AndersonRef(sizes, m, beta=beta)
    worst_g = worst_u = 0.0
    depths = []
    for k, (x, g, out, row, gamma) in enumerate(rec):
        row_ref, _ = ref.gram(k, x, g)
        depths.append(row[:, 2].astype(int).tolist())
        assert row[:, 2].tolist() == row_ref[:, 2].tolist(), (k, "depth", row[:, 2], row_ref[:, 2])
        assert row[:, 3].tolist() == row_ref[:, 3].tolist(), (k, "flags", row[:, 3], row_ref[:, 3])
        # the norms: fp32 roundings of float64 sums that agree to ~1e-14 - one fp32 spacing
        assert np.all(np.abs(row[:, 0:2].astype(np.float64) - row_ref[:, 0:2]) <= np.spacing(row_ref[:, 0:2])), (k, row, row_ref)
        for b in range(len(sizes)):
            if row[b, 2] == 0:
                assert not gamma[b].any(), (k, b, gamma[b])
                continue
            slots, Areg, rhs = ref.systems[b]
            sol = np.linalg.solve(Areg, rhs)
            cond = float(np.linalg.cond(Areg))
            err = float(np.linalg.norm(gamma[b, slots] - sol))
            bound = 64 * EPS64 * cond * float(np.linalg.norm(sol))
            worst_g = max(worst_g, err / bound if bound > 0 else (0.0 if err == 0 else np.inf))
            print(f"m={m} beta={beta} step {k} graph {b}: depth {int(row[b, 2])} cond {cond:.2e} |gamma err| {err:.2e} bound {bound:.2e}")
            unused = [j for j in range(R.MAX_DEPTH) if j not in slots]
            assert not gamma[b, unused].any(), (k, b, gamma[b])
            assert err <= bound, (k, b, err, bound, cond)
        want = ref.mix(g, row, gamma)                 # the reference mix with the DEVICE's gamma
        gap = np.abs(out.astype(np.float64) - want.astype(np.float64))
        worst_u = max(worst_u, float((gap / np.spacing(np.abs(want))).max()))
        assert np.all(gap <= np.spacing(np.abs(want))), (k, float(gap.max()))
    print(f"m={m} beta={beta}: depths {depths}; worst gamma error / bound {worst_g:.3f}; worst iterate gap {worst_u:.2f} fp32 spacings")
    assert max(max(d) for d in depths) == m


def test_reference_agreement_m4(batch_run):
    _check_against_reference(batch_run[0], R.SIZES, 4, 1.0)


def test_reference_agreement_m8_beta_half(problem):
    rec, _ = _run(problem, problem.x0, R.SIZES, 8, beta=0.5)
    _check_against_reference(rec, R.SIZES, 8, 0.5)


def test_convergence_and_plain_steps_keep_their_bits(problem, batch_run):
    rec, d = batch_run
    table = np.stack([r[3] for r in rec])
    rel = table[:, :, 0].astype(np.float64) / table[:, :, 1]
    first = [int(np.argmax(rel[:, b] < 1e-5)) if (rel[:, b] < 1e-5).any() else -1 for b in range(3)]
    print("AA(4) on the device: first step index below 1e-5 per graph", first, "residuals at 8:", rel[8].tolist())
    assert all(0 <= f <= 8 for f in first), (first, rel[:9].tolist())
    assert d.aa.stats()["restarts"] == [0, 0, 0]
    # depth 0: step 0 of that run, and every step before `start`
    assert rec[0][3][:, 2].tolist() == [0, 0, 0] and _same_bits(rec[0][2], rec[0][1])
    late, dl = _run(problem, problem.x0, R.SIZES, 4, steps=5, start=3)
    for k, (x, g, out, row, gamma) in enumerate(late):
        if k < 3:
            assert row[:, 2].tolist() == [0, 0, 0] and row[:, 3].tolist() == [0, 0, 0] and _same_bits(out, g), k
            assert not gamma.any()
        else:
            assert row[:, 2].tolist() == [min(k, 4)] * 3, (k, row)          # the columns were kept while it waited
            assert not _same_bits(out, g)


def test_a_graph_alone_gives_the_bits_it_gives_in_the_batch(problem, batch_run):
    rec, _ = batch_run
    for b, n in enumerate(R.SIZES):
        sl = slice(problem.ptr[b], problem.ptr[b + 1])
        alone, _ = _run(problem.maps[b], problem.maps[b].x0, [n], 4)
        for k, ((x, g, out, row, gamma), (xa, ga, outa, rowa, gammaa)) in enumerate(zip(rec, alone)):
            assert _same_bits(x[sl], xa) and _same_bits(g[sl], ga), (b, k, "the inputs")
            assert _same_bits(row[b], rowa[0]), (b, k, "table", row[b], rowa[0])
            assert _same_bits(gamma[b], gammaa[0]), (b, k, "gamma", gamma[b], gammaa[0])
            assert _same_bits(out[sl], outa), (b, k, "iterate")


@pytest.mark.parametrize("beta", [1.0, 0.5])
def test_rows_with_a_constant_g_keep_their_bits(problem, beta):
    rng = np.random.default_rng(21)
    rows = np.concatenate([problem.ptr[b] + rng.choice(n, size=min(n, 9), replace=False) for b, n in enumerate(R.SIZES)])
    rows = np.unique(np.concatenate((rows, [0, 36, 37, 169, 170, problem.ptr[3] - 1])))   # + first / last rows of the graphs
    vals = rng.standard_normal((len(rows), 3)).astype(np.float32)
    vals[0] = (0.0, -0.0, 1e-30)

    def G(x):
        g = problem(x)
        g[rows] = vals
        return g
    x0 = problem.x0.copy()
    x0[rows] = vals
    rec, _ = _run(G, x0, R.SIZES, 4, beta=beta)
    used = 0
    for k, (x, g, out, row, gamma) in enumerate(rec):
        used += int((row[:, 2] > 0).sum())
        assert _same_bits(out[rows], vals), (k, beta)
    assert used >= 3 * (STEPS - 2), used          # the steps WERE accelerated


def test_decisions(problem):
    sizes = R.SIZES
    ptr = problem.ptr
    d, twin = Device(sizes, 4), Device(sizes, 4)
    for dev in (d, twin):
        dev.set_x(problem.x0)
    outs = []
    for k in range(3):
        x = d.get_x()
        g = problem(x)
        outs.append((x, g, d.step(g), twin.step(g)))
    assert outs[-1][2][1][:, 2].tolist() == [2, 2, 2]
    # NONFINITE: a NaN in g of graph 1 only; graphs 0 and 2 have the bits of the twin that saw no NaN
    x = d.get_x()
    g = problem(x)
    bad = g.copy()
    bad[ptr[1] + 70, 1] = np.nan
    out, row, gamma = d.step(bad)
    out_t, row_t, gamma_t = twin.step(g)
    assert row[:, 3].tolist() == [0, R.NONFINITE, 0] and row[:, 2].tolist() == [3, 0, 3], row
    assert not np.isnan(gamma).any() and not gamma[1].any()
    for b in (0, 2):
        sl = slice(ptr[b], ptr[b + 1])
        assert _same_bits(row[b], row_t[b]) and _same_bits(gamma[b], gamma_t[b]) and _same_bits(out[sl], out_t[sl]), b
    assert _same_bits(out[ptr[1]:ptr[2]], bad[ptr[1]:ptr[2]])                      # depth 0: the model's output as it is
    st = d.aa.stats()
    assert st["restarts"] == [0, 1, 0] and st["columns"] == [3, 0, 3] and st["has_prev"] == [1, 0, 1]
    # ... and graph 1 starts over: a pair, then a column
    x = d.get_x()
    x[ptr[1]:ptr[2]] = problem.x0[ptr[1]:ptr[2]]
    d.set_x(x)
    for want in (0, 1):
        x = d.get_x()
        out, row, gamma = d.step(problem(x))
        assert row[1, 2:].tolist() == [want, 0] and not np.isnan(gamma).any() and not np.isnan(out).any(), (want, row)
    # GROWTH: a residual 20 x the last one (restart = 10) in graph 0
    x = d.get_x()
    g = problem(x)
    f_last = outs[0][1] - outs[0][0]                    # (any direction; scaled to 20 x the last residual norm below)
    sl = slice(ptr[0], ptr[1])
    r_last = float(d.aa.r_prev[0])
    big = g.copy()
    big[sl] = x[sl] + (f_last[sl] * (20.0 * r_last / np.linalg.norm(f_last[sl].astype(np.float64)))).astype(np.float32)
    before = d.aa.stats()
    out, row, gamma = d.step(big)
    after = d.aa.stats()
    assert row[0, 2:].tolist() == [0, R.GROWTH], row
    assert after["columns"][0] == 0 and after["restarts"][0] == before["restarts"][0] + 1 and after["has_prev"][0] == 1
    assert _same_bits(out[sl], big[sl]) and not gamma[0].any()
    assert row[2, 3] == 0 and row[2, 2] == 4


def test_zero_gram_matrix_gives_no_nan(problem):
    d = Device(R.SIZES, 4)
    g = problem(problem.x0)
    d.set_x(g)
    seen = set()
    for k in range(6):                                   # x = g every step: f = 0, every column 0
        out, row, gamma = d.step(g)
        assert _same_bits(out, g), k
        assert not np.isnan(row).any() and not np.isnan(gamma).any() and not gamma.any()
        assert all(row[b, 2] == 0 and row[b, 3] in (0, R.SINGULAR) for b in range(3)), (k, row)
        assert row[:, 0].tolist() == [0, 0, 0]
        seen |= set(row[:, 3].astype(int).tolist())
    assert R.SINGULAR in seen
    assert d.aa.stats()["restarts"] == [5, 5, 5]         # every step with a (zero) column


# ---- 6. through Rollout ----------------------------------------------------------------------------------------------------
def _hip_model(P, dataset_size=1):
    from FVMmodel.importer import NNmodel
    from gfv.params import default_params
    m = NNmodel(default_params(dataset_size=dataset_size))
    sd = m.state_dict()
    for k, v in P.items():
        sd[k].copy_(v)
    m.load_state_dict(sd)
    return m.cuda()


def _to_gpu(graphs):
    hg = tuple(g.clone().to("cuda") for g in graphs)
    hg[0].norm_uvp, hg[0].norm_global = True, True
    return hg


def _tbits(a, b):
    a, b = a.detach().cpu().contiguous(), b.detach().cpu().contiguous()
    return a.shape == b.shape and a.dtype == b.dtype and bool(torch.equal(a.view(torch.int32), b.view(torch.int32)))


K = 10


@pytest.fixture(scope="module")
def fixture_model():
    graphs = cases.make_graphs("cyl_cavity_b2")
    return _hip_model(O.init_parameters(cases.WEIGHT_SEED)), graphs


def _steps(r, k=K):
    outs = []
    for _ in range(k):
        outs.append([t.clone() for t in r.step()])
    return outs


@pytest.fixture(scope="module")
def plain_run(fixture_model):
    from gfv.rollout import Rollout
    model, graphs = fixture_model
    r = Rollout(model, _to_gpu(graphs), max_steps=K)
    outs = _steps(r)
    return outs, r.history.cpu().clone(), r.x_backup.clone()


def test_rollout_anderson_off_is_the_rollout_of_today(fixture_model, plain_run):
    from gfv.rollout import Rollout
    model, graphs = fixture_model
    r = Rollout(model, _to_gpu(graphs), max_steps=K, anderson=0)
    assert r._aa is None and r.anderson == 0
    outs = _steps(r)
    for k in range(K):
        for a, b in zip(outs[k], plain_run[0][k]):
            assert _tbits(a, b), k
    assert _tbits(r.history, plain_run[1]) and _tbits(r.x_backup, plain_run[2]) and _tbits(r.x, plain_run[2])
    assert r._state.tolist() == [K, 0]
    with pytest.raises(RuntimeError, match="anderson=0"):
        r.anderson_history()


def test_rollout_anderson_list_eager_reset_tol_and_dirichlet(fixture_model, plain_run):
    from gfv.rollout import Rollout
    model, graphs = fixture_model
    r = Rollout(model, _to_gpu(graphs), max_steps=K, anderson=4)
    outs = _steps(r)
    hist, table, xb = r.history.cpu().clone(), r.anderson_history().clone(), r.x_backup.clone()
    assert r._lists, "the list should have been recorded"
    # step 1 is the plain step 1 (no pair yet: depth 0)
    for a, b in zip(outs[0], plain_run[0][0]):
        assert _tbits(a, b)
    assert _tbits(hist[0], plain_run[1][0]) and table[0, :, 2].tolist() == [0.0] * r.plan.B
    print("depths", table[:, :, 2].tolist(), "flags", table[:, :, 3].tolist(), "restarts", r.anderson_stats()["restarts"])
    assert float(table[:, :, 2].max()) > 0, "no step was accelerated"
    assert not _tbits(xb, plain_run[2])
    # the table against the fields: column 0 is || G(x) - x ||, known from the history only where the depth was 0
    plain_rows = table[:, :, 2] == 0
    assert torch.allclose(table[:, :, 0][plain_rows], hist[:, :, 4][plain_rows], rtol=1e-6, atol=0)
    # Dirichlet values against the plain rollout's
    nt = graphs[0].node_type.reshape(-1).cpu()
    press = nt == O.PRESS_POINT
    diri = press | (nt == O.WALL_BOUNDARY) | (nt == O.INFLOW) | (nt == O.IN_WALL)
    assert int(diri.sum()) > 0
    assert _tbits(xb.cpu()[diri][:, 0:2], plain_run[2].cpu()[diri][:, 0:2])
    if int(press.sum()):
        assert _tbits(xb.cpu()[press][:, 0:3], plain_run[2].cpu()[press][:, 0:3])
    assert _tbits(xb.cpu()[:, 3:], plain_run[2].cpu()[:, 3:])
    # reset() and the same steps again
    stats = r.anderson_stats()
    r.reset()
    assert r.steps_done == 0 and not bool(r._aa.table.any()) and not bool(r._aa.state.any()) and not bool(r._aa.dF.any())
    _steps(r)
    assert _tbits(r.history, hist) and _tbits(r.anderson_history(), table) and _tbits(r.x_backup, xb)
    assert r.anderson_stats() == stats
    # run(tol) stops on the table's ratio: a tolerance between two recorded values of it, from the middle of the strict record lows
    m = (table[:, :, 0] / table[:, :, 1]).max(dim=1).values.double()
    h = (hist[:, :, 4] / hist[:, :, 5]).max(dim=1).values.double()          # the accelerated update: NOT the criterion
    print("true residual ratio", m.tolist(), "| update ratio", h.tolist())
    lows = [k for k in range(1, K) if m[k] < m[:k].min()]
    assert lows, m.tolist()
    k_star = lows[len(lows) // 2]
    tol = float((m[k_star] + m[:k_star].min()) / 2)
    first = lambda v, t: next((k for k in range(K) if v[k] < t), None)
    assert first(m, tol) == k_star
    r.reset()
    out = r.run(steps=K, tol=tol, check_every=1)
    assert out.shape[0] == k_star + 1 == r.steps_done, (out.shape, k_star, m.tolist(), tol)
    assert _tbits(out, hist[:k_star + 1]) and _tbits(r.anderson_history(), table[:k_star + 1])
    # ... and a tolerance at which history columns 4 / 5 would stop a run at another step than the table does
    split = [(first(m, t), first(h, t), t) for t in (float((m[k] + h[k]) / 2) for k in range(1, K))]
    split = [s for s in split if s[0] is not None and s[1] is not None and s[0] != s[1]]
    assert split, "the two criteria never disagree on this run: nothing tells them apart"
    k_m, k_h, tol = split[0]
    r.reset()
    out = r.run(steps=K, tol=tol, check_every=1)
    print("tolerance", tol, ": the table stops after", k_m + 1, "steps, the update norm would after", k_h + 1)
    assert out.shape[0] == k_m + 1 == r.steps_done, (out.shape, k_m, k_h, tol)
    # list mode equals eager mode (built last: the rollouts share the model's engine)
    e = Rollout(model, _to_gpu(graphs), max_steps=K, launch_mode="eager", anderson=4)
    outs_e = _steps(e)
    assert _tbits(hist, e.history) and _tbits(table, e.anderson_history()) and _tbits(xb, e.x_backup)
    for k in range(K):
        for a, b in zip(outs[k], outs_e[k]):
            assert _tbits(a, b), k
