"""GPU: gfv.optim.LBFGS and the gfv_lbfgs_* launches under it (csrc/lbfgs.hip).

The search direction against the textbook two-loop recursion in float64, beside the same recursion in plain fp32 torch ops (what
torch.optim.LBFGS computes); padding that must not leak; bit-for-bit repeatability; a quadratic with a known answer and the
reference's closure on the drop-in model, both beside torch.optim.LBFGS; checkpoints both ways."""
import math

import numpy as np
import pytest
import torch

import cases
from oracle import fvgn_oracle as O

pytestmark = pytest.mark.gpu

MODEL_NUMEL = 1181539
SMALL_SHAPES = [(3,), (7, 5), (129,), (834,)]          # 1001 elements, 1008 with the padding of the flat layout
QUAD_SHAPES = [(3,), (7, 5), (129,), (64, 64), (1,)]


def _model_shapes():
    from FVMmodel.importer import NNmodel
    from gfv.params import default_params
    shapes = [tuple(p.shape) for p in NNmodel(default_params()).parameters()]
    assert sum(math.prod(s) for s in shapes) == MODEL_NUMEL
    return shapes


def _bare_optimizer(shapes, history_size, **kw):
    from gfv.optim import LBFGS
    params = [torch.nn.Parameter(torch.zeros(s, device="cuda")) for s in shapes]
    return LBFGS(params, history_size=history_size, **kw)


def _flat_with_padding(opt, v, fill):
    """The unpadded vector `v` in the optimiser's flat layout, the padding slots holding `fill`."""
    flat = torch.full((opt.n,), fill, dtype=torch.float32, device="cuda")
    flat[opt._idx] = v.to("cuda")
    return flat


def _push(opt, s, y, g, fill=0.0):
    """One direction launch sequence with (s, y) as the candidate pair and g as the gradient (the pair written where
    gfv_lbfgs_pair would write it; the gradient through the masked copy, its padding holding `fill`).  Returns the result block."""
    from gfv import lib as L
    ring = opt.ring.cpu()
    c = (int(ring[0]) + int(ring[1])) % opt.slots
    n = opt.n
    opt._padded(opt.S[c * n:(c + 1) * n], s)
    opt._padded(opt.Y[c * n:(c + 1) * n], y)
    opt._ingest(_flat_with_padding(opt, g, fill), opt._gcur)
    lib, st = L.load(), L.stream_ptr()
    gp = opt.gbuf[opt._gcur].data_ptr()
    L.check(lib.gfv_lbfgs_multidot(opt.S.data_ptr(), opt.Y.data_ptr(), opt.slots, n, opt.ring.data_ptr(), gp, opt.partial.data_ptr(),
                                   0, st), "multidot")
    L.check(lib.gfv_lbfgs_coef(opt.ring.data_ptr(), opt.M.data_ptr(), opt.partial.data_ptr(), opt.delta.data_ptr(), opt.res.data_ptr(),
                               opt.slots, n, 0, st), "coef")
    L.check(lib.gfv_lbfgs_combine(opt.S.data_ptr(), opt.Y.data_ptr(), opt.slots, n, opt.ring.data_ptr(), gp, opt.delta.data_ptr(),
                                  opt.d.data_ptr(), opt.res.data_ptr(), st), "combine")
    return opt.res.cpu()


def _history(n, pairs, seed):
    """A history from a convex quadratic, so that every pair is valid: s_i normal, y_i = D s_i with D diagonal and log-uniform in
    [0.1, 10] (rounded to fp32: the stored pair IS the input of every implementation), g normal."""
    gen = torch.Generator().manual_seed(seed)
    D = 10.0 ** (2.0 * torch.rand(n, generator=gen) - 1.0)
    S = [torch.randn(n, generator=gen) for _ in range(pairs)]
    Y = [D * s for s in S]
    g = torch.randn(n, generator=gen)
    return S, Y, g


def _two_loop(S, Y, g, dtype, device):
    """The textbook two-loop recursion (torch/optim/lbfgs.py:425-442, Nocedal & Wright alg. 7.4) in `dtype` on `device`:
    gamma = y.s / y.y of the newest pair.  Returns d and g.d."""
    S = [s.to(device=device, dtype=dtype) for s in S]
    Y = [y.to(device=device, dtype=dtype) for y in Y]
    g = g.to(device=device, dtype=dtype)
    k = len(S)
    ro = [1.0 / Y[i].dot(S[i]) for i in range(k)]
    H = Y[-1].dot(S[-1]) / Y[-1].dot(Y[-1])
    al = [None] * k
    q = g.neg()
    for i in range(k - 1, -1, -1):
        al[i] = S[i].dot(q) * ro[i]
        q.add_(Y[i], alpha=-al[i])
    r = torch.mul(q, H)
    for i in range(k):
        be = Y[i].dot(r) * ro[i]
        r.add_(S[i], alpha=al[i] - be)
    return r, g.dot(r)


def _relerr(d, d64):
    d = d.detach().double().cpu()
    return float((d - d64).norm() / d64.norm())


def _run_direction(shapes, m, pushes, seed, fill=0.0, reject_at=None, opt=None):
    """Push `pushes` pairs into a ring of `m`; `reject_at`: a candidate with y = 0 goes in before that pair, and must change
    nothing.  Returns (optimiser, unpadded d, result block, the pairs the ring must hold, g)."""
    opt = _bare_optimizer(shapes, m) if opt is None else opt
    n_u = int(opt._idx.numel())
    S, Y, g = _history(n_u, pushes, seed)
    for i in range(pushes):
        if reject_at == i:
            before = (opt.ring.cpu()[:2].clone(), float(opt.res[4]))
            res = _push(opt, S[i], torch.zeros(n_u), g, fill)
            assert res[3] == 0.0
            assert torch.equal(opt.ring.cpu()[:2], before[0]) and float(opt.res[4]) == before[1]
        res = _push(opt, S[i], Y[i], g, fill)
        assert res[3] == 1.0 and int(res[5]) == min(i + 1, m)
    torch.cuda.synchronize()
    return opt, opt.d[opt._idx].clone(), res, (S[-m:], Y[-m:]), g


CASES = [("small", 1), ("small", 3), ("small", 10), ("small", 100), ("model", 1), ("model", 3), ("model", 10), ("model", 100)]


@pytest.mark.parametrize("layout,m", CASES + [("small", "wrap"), ("model", "wrap")])
def test_direction_against_float64(layout, m):
    """err = ||d - d64|| / ||d64|| against the float64 recursion on the CPU: the launches (sums in double, rounded once) within
    1.5 x the error of the same recursion in fp32 torch ops on the GPU - and g.d from the coefficient launch within the same
    factor of the fp32 d.dot(g).  m = "wrap": 8 pairs into a ring of 5, a rejected candidate (y = 0) on the way."""
    shapes = SMALL_SHAPES if layout == "small" else _model_shapes()
    if m == "wrap":
        opt, d, res, (S, Y), g = _run_direction(shapes, 5, 8, seed=11, reject_at=6)
    else:
        opt, d, res, (S, Y), g = _run_direction(shapes, m, m, seed=100 + m)
    assert opt.n % 4 == 0 and opt.n > int(opt._idx.numel())            # the layout has padding
    d64, gtd64 = _two_loop(S, Y, g, torch.float64, "cpu")
    d32, gtd32 = _two_loop(S, Y, g, torch.float32, "cuda")
    err_hip, err_32 = _relerr(d, d64), _relerr(d32, d64)
    gerr_hip = abs(float(res[0]) - float(gtd64)) / abs(float(gtd64))
    gerr_32 = abs(float(gtd32) - float(gtd64)) / abs(float(gtd64))
    print(f"LBFGS-DIRECTION layout={layout} n={int(opt._idx.numel())} m={m} err_hip={err_hip:.3e} err_fp32={err_32:.3e} "
          f"gtd_err_hip={gerr_hip:.3e} gtd_err_fp32={gerr_32:.3e}")
    pad = torch.ones(opt.n, dtype=torch.bool, device="cuda")
    pad[opt._idx] = False
    assert bool((opt.d[pad] == 0).all())                                # d is zero in padding
    g64 = g.double()
    assert float(res[1]) == float(g.abs().max()) and abs(float(res[2]) - float(g64.abs().sum())) <= 1e-12 * float(g64.abs().sum())
    dmax = float(res[8:9].view(torch.float32)[0])
    assert dmax == float(d.abs().max())
    assert err_hip <= 1.5 * err_32
    assert gerr_hip <= 1.5 * gerr_32


@pytest.mark.parametrize("layout,m", [("small", 10), ("model", 3)])
def test_padding_does_not_leak(layout, m):
    """The gradient's padding slots holding 1e30, then NaN: direction, g.d, max|g| and sum|g| bit-equal to the zero-padded run."""
    shapes = SMALL_SHAPES if layout == "small" else _model_shapes()
    runs = [_run_direction(shapes, m, m, seed=7, fill=f) for f in (0.0, 1e30, float("nan"))]
    d0, r0 = runs[0][1], runs[0][2]
    assert torch.isfinite(d0).all() and float(d0.abs().max()) > 0
    for _, d, r, _, _ in runs[1:]:
        assert torch.equal(d, d0)
        assert torch.equal(r[:3], r0[:3]) and torch.equal(r[8:9], r0[8:9])
    for opt, _, _, _, _ in runs:
        assert torch.equal(opt.d, runs[0][0].d)                        # the padding of d included: zeros


def _quadratic(seed=0, n_eig=2, b_scale=1.0):
    """f = 1/2 sum d_i x_i^2 - b.x over QUAD_SHAPES, condition number 1e3, x0 = 0: d takes n_eig values log-spaced 1 .. 1e3,
    b = b_scale * standard normal."""
    gen = torch.Generator().manual_seed(seed)
    n = sum(math.prod(s) for s in QUAD_SHAPES)
    d = torch.logspace(0, 3, n_eig)[torch.arange(n) % n_eig][torch.randperm(n, generator=gen)]
    b = b_scale * torch.randn(n, generator=gen)
    return d.cuda(), b.cuda()


def _quad_params(x=None):
    ps, o = [], 0
    for s in QUAD_SHAPES:
        k = math.prod(s)
        v = torch.zeros(s, device="cuda") if x is None else x[o:o + k].reshape(s).clone()
        ps.append(torch.nn.Parameter(v))
        o += k
    return ps


def _quad_closure(opt, ps, d, b, hist, f64=False):
    """Plain torch on the GPU.  f64: the fp32 parameters are cast and f is summed in float64 (the gradients arrive in fp32 as
    ever): a loss without the rounding noise of an fp32 sum."""
    if f64:
        d, b = d.double(), b.double()

    def closure():
        opt.zero_grad()
        x = torch.cat([p.reshape(-1) for p in ps])
        x = x.double() if f64 else x
        f = 0.5 * (d * x * x).sum() - (b * x).sum()
        f.backward()
        hist.append(float(f.detach()))
        return f
    return closure


HARD = dict(n_eig=64, b_scale=1.0)   # a spectrum that keeps every iteration of a short run productive (no early convergence)
SHORT = dict(max_iter=3, max_eval=12, history_size=4, tolerance_grad=0.0, tolerance_change=0.0, line_search_fn="strong_wolfe")


def _run_quadratic(cls, steps=1, problem=None, f64=False, **kw):
    d, b = _quadratic(**(problem or {}))
    ps = _quad_params()
    opt = cls(ps, **kw)
    hist = []
    closure = _quad_closure(opt, ps, d, b, hist, f64)
    for _ in range(steps):
        opt.step(closure)
    torch.cuda.synchronize()
    return opt, ps, hist, d, b


@pytest.mark.parametrize("line_search_fn", [None, "strong_wolfe"])
def test_quadratic_with_a_known_answer_beside_torch(line_search_fn):
    """b standard normal, two eigenvalues 1 and 1e3 (the run to |g|_inf <= 1e-5 takes 15 iterations: the ring of 10 wraps), the
    loss summed in float64 inside the closure.  With the loss summed in fp32 the end of this run is decided by the rounding of f,
    for torch.optim.LBFGS as for this optimiser: f* is about -1057 (ulp 1.2e-4) while a step at |g| ~ 1e-4 lowers f by about
    1e-8, so the Armijo test compares noise.  Measured that way (strong_wolfe): n_iter 14 / func_evals 27 / |x - b/d|_inf 4.4e-4
    here, 15 / 19 for torch, the first ten losses equal to 1e-6.  A float64 sum gives both optimisers the same quiet f."""
    from gfv.optim import LBFGS
    kw = dict(lr=1, max_iter=100, tolerance_grad=1e-5, tolerance_change=0.0, history_size=10, line_search_fn=line_search_fn)
    ours, ps, hist, d, b = _run_quadratic(LBFGS, f64=True, **kw)
    theirs, pt, hist_t, _, _ = _run_quadratic(torch.optim.LBFGS, f64=True, **kw)
    so, st = ours.state[ps[0]], theirs.state[pt[0]]
    print(f"LBFGS-QUADRATIC {line_search_fn}: ours n_iter={so['n_iter']} func_evals={so['func_evals']}; torch n_iter={st['n_iter']} "
          f"func_evals={st['func_evals']}")
    x = torch.cat([p.detach().reshape(-1) for p in ps])
    err = float((x - b / d).abs().max())
    print(f"LBFGS-QUADRATIC {line_search_fn}: |x - b/d|_inf={err:.3e}; ours {hist[:10]}; torch {hist_t[:10]}")
    assert len(hist) >= 10 and len(hist_t) >= 10
    assert all(abs(a - c) <= 1e-5 * abs(c) for a, c in zip(hist[:10], hist_t[:10]))   # (x0 = 0: the first loss is 0 for both)
    assert so["n_iter"] == st["n_iter"] and so["func_evals"] == st["func_evals"]
    assert 10 < so["n_iter"] < 100                                      # the ring wrapped; ended by the gradient test
    assert err <= 1e-5 / float(d.min())


@pytest.mark.parametrize("line_search_fn", [None, "strong_wolfe"])
def test_dense_spectrum_twenty_iterations_beside_torch(line_search_fn):
    """64 distinct eigenvalues: nowhere near convergence after 20 iterations, every one of them works through a full, wrapped
    history of 10.  Same number of evaluations as torch.optim.LBFGS and the same first ten losses (1e-5, the bound of the run
    above).  Not run to the tolerance: that takes some 240 iterations here, over which the counts of any two differently
    rounded implementations part (every iteration amplifies the rounding difference of the directions)."""
    from gfv.optim import LBFGS
    kw = dict(lr=1, max_iter=20, max_eval=60, tolerance_grad=1e-5, tolerance_change=0.0, history_size=10, line_search_fn=line_search_fn)
    ours, ps, hist, _, _ = _run_quadratic(LBFGS, problem=HARD, f64=True, **kw)
    theirs, pt, hist_t, _, _ = _run_quadratic(torch.optim.LBFGS, problem=HARD, f64=True, **kw)
    so, st = ours.state[ps[0]], theirs.state[pt[0]]
    rel = max(abs(a - c) / abs(c) for a, c in list(zip(hist, hist_t))[1:])
    print(f"LBFGS-DENSE {line_search_fn}: ours {so['n_iter']}/{so['func_evals']} torch {st['n_iter']}/{st['func_evals']} "
          f"largest relative loss difference over the run {rel:.1e}")
    assert so["n_iter"] == st["n_iter"] == 20 and so["func_evals"] == st["func_evals"]
    assert all(abs(a - c) <= 1e-5 * abs(c) for a, c in zip(hist[:10], hist_t[:10]))
    assert hist[-1] < hist[0]


def test_run_to_run_determinism():
    """The m = 100 direction twice, and a 6-iteration optimiser run twice: the same bits."""
    a = _run_direction(SMALL_SHAPES, 100, 100, seed=200)
    b = _run_direction(SMALL_SHAPES, 100, 100, seed=200)
    assert torch.equal(a[1], b[1]) and torch.equal(a[2], b[2])
    shapes = _model_shapes()
    a = _run_direction(shapes, 100, 100, seed=200)
    da, ra = a[1].clone(), a[2].clone()
    del a
    torch.cuda.empty_cache()
    b = _run_direction(shapes, 100, 100, seed=200)
    assert torch.equal(da, b[1]) and torch.equal(ra, b[2])
    from gfv.optim import LBFGS
    kw = dict(max_iter=6, history_size=10, tolerance_grad=0.0, tolerance_change=0.0, line_search_fn="strong_wolfe")
    _, p1, h1, _, _ = _run_quadratic(LBFGS, problem=HARD, **kw)
    _, p2, h2, _, _ = _run_quadratic(LBFGS, problem=HARD, **kw)
    assert h1 == h2 and len(h1) >= 7
    assert all(torch.equal(x, y) for x, y in zip(p1, p2))


def test_parameter_padding_is_left_alone_and_gradient_padding_ignored_by_step():
    from gfv.optim import LBFGS
    kw = dict(max_iter=5, history_size=4, tolerance_grad=0.0, tolerance_change=0.0, line_search_fn="strong_wolfe")
    _, p_clean, h_clean, _, _ = _run_quadratic(LBFGS, problem=HARD, **kw)
    d, b = _quadratic(**HARD)
    ps = _quad_params()
    opt = LBFGS(ps, **kw)
    pad = torch.ones(opt.n, dtype=torch.bool, device="cuda")
    pad[opt._idx] = False
    assert int(pad.sum()) > 0
    opt.flat_p[pad] = 7.0
    opt.flat_g[pad] = float("nan")          # the gather of .grad leaves the padding of this buffer as it finds it
    hist = []
    opt.step(_quad_closure(opt, ps, d, b, hist))
    torch.cuda.synchronize()
    assert hist == h_clean and all(torch.equal(x, y) for x, y in zip(ps, p_clean))
    assert bool((opt.flat_p[pad] == 7.0).all())
    assert bool((opt.d[pad] == 0).all()) and bool((opt.g_prev[pad] == 0).all()) and bool((opt.S.view(opt.slots, -1)[:, pad] == 0).all())


def test_a_parameter_without_gradient_contributes_zeros():
    """torch's _gather_flat_grad: `.grad is None` counts as zeros - the parameter stays where it is."""
    from gfv.optim import LBFGS
    d, b = _quadratic()
    ps = _quad_params()
    extra = torch.nn.Parameter(torch.full((5,), 3.0, device="cuda"))
    opt = LBFGS(ps + [extra], max_iter=4, history_size=4, line_search_fn="strong_wolfe")
    hist = []
    opt.step(_quad_closure(opt, ps, d, b, hist))
    assert extra.grad is None and bool((extra == 3.0).all()) and hist[-1] < hist[0]


# ---- the reference's closure on the drop-in model ---------------------------------------------------------------------------
def _model_and_closure(opt_cls, kw, hidden=None):
    from FVMmodel.importer import NNmodel
    from gfv.params import default_params
    cpu_graphs = cases.make_graphs("cavity_mixed_b1")
    if hidden is None:
        params, P = default_params(dataset_size=1), O.init_parameters(cases.WEIGHT_SEED)
    else:
        params = default_params(dataset_size=1, hidden_size=hidden)
        P = O.init_parameters(cases.WEIGHT_SEED, {"hidden_size": hidden})
    model = NNmodel(params)
    sd = model.state_dict()
    for k, v in P.items():
        sd[k].copy_(v)
    model.load_state_dict(sd)
    model = model.cuda()
    graphs = tuple(g.clone().to("cuda") for g in cpu_graphs)
    gn = graphs[0]
    xg = gn.x.clone()
    hist = []
    opt = opt_cls(model.parameters(), **kw)

    def closure():
        opt.zero_grad()
        gn.x = xg.clone()
        gn.norm_uvp, gn.norm_global = params.norm_uvp, params.norm_global
        lc, lmx, lmy, lp, _, _ = model(*graphs)
        lb = params.loss_press * lp + params.loss_cont * lc + params.loss_mom * lmx + params.loss_mom * lmy
        loss = torch.mean(torch.log(torch.clamp(lb, min=1e-10, max=1e10)))
        loss.backward()
        hist.append(float(loss))
        return loss

    return model, opt, closure, hist


@pytest.mark.parametrize("hidden", [None, 64])
def test_reference_closure_on_the_drop_in_model_beside_torch(hidden):
    """cavity_mixed_b1, the weights, closure and arguments of test_lbfgs_loop_tracks_the_oracle_under_the_same_optimizer: the
    two optimisers on two copies of the same NNmodel see the same losses - the first to 1e-5, the next (up to five evaluations)
    to 1e-3, that test's own bounds - and the loss falls by more than 1e-3.  hidden = 64: FVMmodel/padding.py's padded parameters."""
    from gfv.optim import LBFGS
    kw = dict(max_iter=4, history_size=10, tolerance_grad=1e-9, tolerance_change=1e-12, line_search_fn="strong_wolfe")
    _, opt_t, closure_t, hist_t = _model_and_closure(torch.optim.LBFGS, kw, hidden)
    opt_t.step(closure_t)
    _, opt_o, closure_o, hist_o = _model_and_closure(LBFGS, kw, hidden)
    opt_o.step(closure_o)
    k = min(len(hist_o), len(hist_t), 5)
    rels = [abs(a - c) / abs(c) for a, c in zip(hist_o[:k], hist_t[:k])]
    print(f"LBFGS-MODEL hidden={hidden}: ours {hist_o}; torch {hist_t}; rel {['%.1e' % r for r in rels]}")
    assert k >= 3 and all(np.isfinite(hist_o))
    assert rels[0] < 1e-5
    assert all(r < 1e-3 for r in rels[1:])
    assert min(hist_o) < hist_o[0] - 1e-3


# ---- checkpoints -----------------------------------------------------------------------------------------------------------
def test_checkpoint_resumes_bit_for_bit():
    from gfv.optim import LBFGS
    kw = SHORT
    opt5, p5, h5, d, b = _run_quadratic(LBFGS, steps=5, problem=HARD, **kw)
    opt3, p3, h3, _, _ = _run_quadratic(LBFGS, steps=3, problem=HARD, **kw)
    sd = opt3.state_dict()
    keys = {"old_dirs", "old_stps", "ro", "H_diag", "d", "t", "prev_flat_grad", "prev_loss", "n_iter", "func_evals", "al"}
    assert set(sd["state"][0]) == keys
    n_u = sum(math.prod(s) for s in QUAD_SHAPES)
    assert all(v.shape == (n_u,) for v in sd["state"][0]["old_dirs"]) and sd["state"][0]["d"].shape == (n_u,)
    assert len(sd["state"][0]["old_dirs"]) == 4                          # the ring wrapped: oldest first, history_size of them
    ps = _quad_params(torch.cat([p.detach().reshape(-1) for p in p3]))
    opt = LBFGS(ps, **kw)
    opt.load_state_dict(sd)
    hist = []
    closure = _quad_closure(opt, ps, d, b, hist)
    for _ in range(2):
        opt.step(closure)
    torch.cuda.synchronize()
    assert h3 + hist == h5
    assert all(torch.equal(x, y) for x, y in zip(ps, p5))
    assert opt.state[ps[0]]["n_iter"] == opt5.state[p5[0]]["n_iter"] == 15
    assert opt.state[ps[0]]["func_evals"] == opt5.state[p5[0]]["func_evals"]


def _gram(opt):
    """The stored pairs' block of the dot-product matrix in logical order (s oldest .. newest, then y)."""
    ring = opt.ring.cpu()
    head, count = int(ring[0]), int(ring[1])
    slots = [(head + i) % opt.slots for i in range(count)]
    rows = torch.tensor(slots + [opt.slots + s for s in slots])
    M = opt.M.view(opt.R, opt.R).cpu()
    return M[rows][:, rows]


def test_checkpoint_at_the_models_size_through_save_checkpoint(tmp_path):
    """A wrapped history at the model's layout (289 column tiles) goes through NNmodel.save_checkpoint (`optimizer0`) and
    load_checkpoint into a fresh model and optimiser: the vectors, the rebuilt dot-product matrix and the next direction have
    the same bits."""
    from FVMmodel.importer import NNmodel
    from gfv.optim import LBFGS
    from gfv.params import default_params
    model = NNmodel(default_params()).cuda()
    opt = LBFGS(model.parameters(), history_size=3, line_search_fn="strong_wolfe")
    assert int(opt._idx.numel()) == MODEL_NUMEL
    _run_direction(None, 3, 5, seed=31, opt=opt)
    assert int(opt.ring.cpu()[0]) != 0                                   # the ring has turned
    opt.state[opt._params[0]].update(n_iter=5, func_evals=7, t=0.5, prev_loss=1.25)
    path = str(tmp_path / "ckpt.pth")
    model.save_checkpoint(path, optimizer=opt)
    assert "optimizer0" in torch.load(path, map_location="cpu", weights_only=False)
    model2 = NNmodel(default_params()).cuda()
    opt2 = LBFGS(model2.parameters(), history_size=3, line_search_fn="strong_wolfe")
    model2.load_checkpoint(optimizer=opt2, ckpdir=path, device="cuda")
    a, b = opt.state_dict()["state"][0], opt2.state_dict()["state"][0]
    assert (b["n_iter"], b["func_evals"], b["t"], b["prev_loss"]) == (5, 7, 0.5, 1.25)
    for key in ("old_dirs", "old_stps", "ro"):
        assert len(a[key]) == len(b[key]) == 3 and all(torch.equal(x, y) for x, y in zip(a[key], b[key])), key
    assert torch.equal(a["d"], b["d"]) and torch.equal(a["H_diag"], b["H_diag"])
    assert torch.equal(_gram(opt), _gram(opt2))
    S, Y, g = _history(MODEL_NUMEL, 1, seed=32)
    ra, rb = _push(opt, S[0], Y[0], g), _push(opt2, S[0], Y[0], g)
    assert torch.equal(opt.d, opt2.d) and torch.equal(ra[:6], rb[:6]) and torch.equal(ra[8:9], rb[8:9])


@pytest.mark.parametrize("direction", ["torch_to_gfv", "gfv_to_torch"])
def test_checkpoints_cross_load(direction):
    from gfv.optim import LBFGS
    kw = SHORT
    src_cls, dst_cls = (torch.optim.LBFGS, LBFGS) if direction == "torch_to_gfv" else (LBFGS, torch.optim.LBFGS)
    src, p_src, _, d, b = _run_quadratic(src_cls, steps=2, problem=HARD, **kw)
    x = torch.cat([p.detach().reshape(-1) for p in p_src])
    # the source goes on by itself: the reference for the step after the hand-over
    h_ref = []
    src_sd = src.state_dict()
    assert src_sd["state"][0]["n_iter"] == 6 and len(src_sd["state"][0]["old_dirs"]) == 4
    ps = _quad_params(x)
    dst = dst_cls(ps, **kw)
    dst.load_state_dict(src_sd)
    h_dst = []
    dst.step(_quad_closure(dst, ps, d, b, h_dst))
    src.step(_quad_closure(src, p_src, d, b, h_ref))
    print(f"LBFGS-CROSSLOAD {direction}: {h_dst[:3]} beside {h_ref[:3]}")
    assert abs(h_dst[0] - h_ref[0]) <= 1e-5 * abs(h_ref[0])          # the step's first loss
    assert abs(h_dst[1] - h_ref[1]) <= 1e-3 * abs(h_ref[1])          # the first trial point: the loaded history, d and t decide it
    assert dst.state[ps[0]]["n_iter"] == src.state[p_src[0]]["n_iter"] == 9          # (3 step() calls of 3 iterations)
    assert len(dst.state_dict()["state"][0]["old_dirs"]) == 4
