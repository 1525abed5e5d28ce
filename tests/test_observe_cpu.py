"""CPU: the observation term's reference (tests/obs_ref.py) and the host-only checks of gfv/observe.py.

1. the reference's g_dec increment and gloss against torch float64 autograd of the objective written directly from the formulas
   (tanh, boundary mask, scale, weighted mean, log of the sum), to 1e-12 relative;
2. a graph without an observed element: obs = 0, tot = the PDE part, no NaN; NaN targets under zero weights change nothing;
3. what the host refuses; 4. the new symbols are declared, and the entry points refuse bad arguments before touching a device."""
import ctypes as C

import numpy as np
import pytest
import torch

import obs_ref as R

f32, f64 = np.float32, np.float64
ROWS = (1, 65, 100)                       # three graphs, one chunk each
LW = (6e4, 5e4, 1.0)                      # w_cont, w_mom, w_press
W_OBS = 3.0


def _table(rows=ROWS):
    end = np.cumsum(rows)
    return (end - np.asarray(rows)).astype(np.int32), end.astype(np.int32), np.arange(len(rows) + 1, dtype=np.int32), \
        int(end[-1]), np.repeat(np.arange(len(rows)), rows)


def _inputs(seed, N, B, row_graph, zero_graph=None, nan_targets=True):
    rng = np.random.default_rng(seed)
    dec = rng.uniform(-10.0, 10.0, (N, 3))
    y = rng.uniform(-1.0, 1.0, (N, 2))
    node_type = rng.integers(0, 6, N)
    node_type[1:7] = np.arange(6)            # (every kind occurs; node 0, a graph of its own, stays as drawn)
    target = rng.standard_normal((N, 3)) * 3.0
    weight = rng.uniform(0.1, 2.0, (N, 3)) * (rng.uniform(0, 1, (N, 3)) > 1.0 / 3.0)
    if zero_graph is not None:
        weight[row_graph == zero_graph] = 0.0
    if nan_targets:
        target[weight == 0] = np.nan
    return dict(dec=dec, y=y, node_type=node_type, target=target, weight=weight,
                uvp_dim=rng.uniform(0.5, 2.0, (B, 3)), sigma=rng.uniform(0.5, 2.0, (B, 3)),
                losses=rng.uniform(1e-5, 1e-3, (B, 4)) * np.array([1.0, 1.0, 1.0, 1e3]))


def _phi3(dec, y, node_type):
    """BC(10 tanh(dec / 10)) in numpy float64."""
    phi = 10.0 * np.tanh(dec / 10.0)
    diri = np.isin(node_type, (R.WALL, R.INFLOW, R.PRESS, R.INWALL))
    phi[diri, 0:2] = y[diri]
    phi[node_type == R.PRESS, 2] = 0.0
    return phi


def _reference(d, row_graph, tab, exact):
    cb, ce, gcp, N, _ = tab
    phi3 = _phi3(d["dec"].copy(), d["y"], d["node_type"])
    e, _ = R.misfit(phi3, d["target"], d["weight"], d["uvp_dim"], d["sigma"], row_graph, dtype=f64)
    _, SW = R.sums(R.row_terms(e, d["weight"]), cb, ce, gcp, N)
    rec = R.record(SW, d["losses"], LW, W_OBS, exact=exact)
    inc, contributes = R.gdec_increment(rec, e, d["weight"], d["dec"], d["uvp_dim"], d["sigma"], row_graph, d["node_type"])
    return rec, inc, contributes


def _autograd(d, row_graph):
    """The same objective in torch float64, straight from the formulas."""
    t = lambda a: torch.from_numpy(np.asarray(a, dtype=f64))
    dec = t(d["dec"]).requires_grad_(True)
    losses = t(d["losses"]).requires_grad_(True)
    nt, rg = torch.from_numpy(d["node_type"]), torch.from_numpy(row_graph)
    phi = 10.0 * torch.tanh(dec / 10.0)
    diri = ((nt == R.WALL) | (nt == R.INFLOW) | (nt == R.PRESS) | (nt == R.INWALL))[:, None]
    uv = torch.where(diri, t(d["y"]), phi[:, 0:2])
    p = torch.where((nt == R.PRESS), torch.zeros((), dtype=torch.float64), phi[:, 2])
    pred = torch.cat((uv, p[:, None]), 1) * t(d["uvp_dim"])[rg] * t(d["sigma"])[rg]
    w = t(d["weight"])
    sq = torch.where(w != 0, w * (pred - torch.nan_to_num(t(d["target"]))) ** 2, torch.zeros((), dtype=torch.float64))
    B = d["losses"].shape[0]
    S = torch.zeros(B, dtype=torch.float64).index_add(0, rg, sq.sum(1))
    W = torch.zeros(B, dtype=torch.float64).index_add(0, rg, w.sum(1))
    obs = torch.where(W > 0, S / torch.where(W > 0, W, torch.ones_like(W)), torch.zeros_like(S))
    wc, wm, wp = LW
    tot = wp * losses[:, 3] + wc * losses[:, 0] + wm * losses[:, 1] + wm * losses[:, 2] + W_OBS * obs
    loss = torch.log(tot).mean()
    g_dec, g_losses = torch.autograd.grad(loss, [dec, losses])
    return float(loss.detach()), g_dec.numpy(), g_losses.numpy(), obs.detach().numpy()


def test_reference_gradient_equals_float64_autograd():
    tab = _table()
    row_graph = tab[4]
    d = _inputs(1, tab[3], len(ROWS), row_graph)
    rec, inc, contributes = _reference(d, row_graph, tab, exact=True)
    loss, g_dec, g_losses, obs = _autograd(d, row_graph)
    assert contributes.any() and not contributes.all() and (rec["W"] > 0).all()
    assert abs(rec["loss"] - loss) <= 1e-12 * abs(loss)
    assert np.abs(rec["obs"] - obs).max() <= 1e-12 * np.abs(obs).max()
    assert np.abs(rec["gloss"] - g_losses).max() <= 1e-12 * np.abs(g_losses).max()
    assert np.abs(inc - g_dec).max() <= 1e-12 * np.abs(g_dec).max()
    assert (g_dec[~contributes] == 0).all() and (inc[~contributes] == 0).all()


def test_an_unobserved_graph_and_nan_targets_under_zero_weights():
    tab = _table()
    row_graph = tab[4]
    d = _inputs(2, tab[3], len(ROWS), row_graph, zero_graph=1, nan_targets=True)
    rec, inc, _ = _reference(d, row_graph, tab, exact=False)
    assert rec["W"][1] == 0 and rec["obs"][1] == 0 and rec["tot"][1] == rec["pde"][1]
    assert rec["obs"][0] > 0 and rec["obs"][2] > 0
    for v in (rec["obs"], rec["tot"], rec["gobs"], rec["gloss"], inc, np.array(rec["loss"])):
        assert np.isfinite(v).all()
    assert (inc[row_graph == 1] == 0).all()
    clean = dict(d, target=np.where(d["weight"] == 0, 7.0, d["target"]))
    rec2, inc2, _ = _reference(clean, row_graph, tab, exact=False)
    for k in ("obs", "W", "tot", "gobs", "gloss"):
        assert np.array_equal(rec[k].view(np.int64), rec2[k].view(np.int64)), k
    assert np.array_equal(inc.view(np.int64), inc2.view(np.int64))
    # the kernels' precision: e in fp32 moves obs by a few fp32 roundings, nothing more
    phi3 = _phi3(d["dec"].copy(), d["y"], d["node_type"]).astype(f32)
    e32, observed = R.misfit(phi3, d["target"].astype(f32), d["weight"].astype(f32), d["uvp_dim"].astype(f32),
                             d["sigma"].astype(f32), row_graph)
    assert e32.dtype == f32 and np.isfinite(e32).all() and (e32[~observed] == 0).all()


def test_host_checks_refuse_what_the_kernels_do_not_define():
    from gfv import march
    from gfv.observe import ObservationTerm, check_observations, check_observe
    v, w = torch.zeros(5, 3), torch.ones(5, 3)
    assert check_observations(v, w, 2) == 2.0 and check_observations(v, w, 0.0, n=5) == 0.0
    assert check_observations(torch.full((5, 3), float("nan")), torch.zeros(5, 3)) == 1.0      # (unobserved values may be NaN)
    for bad in (-1.0, float("nan"), float("inf")):
        wb = w.clone()
        wb[2, 1] = bad
        with pytest.raises(ValueError, match="finite and >= 0"):
            check_observations(v, wb)
    for vv, ww in ((torch.zeros(5, 2), torch.ones(5, 2)), (torch.zeros(5), torch.ones(5)), (v, torch.ones(4, 3)),
                   (torch.zeros(5, 3, 1), torch.ones(5, 3, 1))):
        with pytest.raises(ValueError):
            check_observations(vv, ww)
    with pytest.raises(ValueError, match="rows"):
        check_observations(v, w, n=6)
    with pytest.raises(ValueError, match="float32"):
        check_observations(v.double(), w)
    with pytest.raises(ValueError, match="float32"):
        check_observations(v, w.to(torch.float16))
    with pytest.raises(ValueError, match="torch tensor"):
        check_observations(v.numpy(), w)
    for bad in (-1.0, float("nan"), float("inf"), "1", None, True):
        with pytest.raises(ValueError, match="weight"):
            check_observations(v, w, bad)
    with pytest.raises(ValueError, match="observations= is not supported"):
        march.check_step_args("list", {"observations": object()})
    march.check_step_args("list", {"observations": None})
    term = ObservationTerm(1.0)
    check_observe(None, object())
    check_observe(term, None)
    with pytest.raises(ValueError, match="balance= together with observations="):
        check_observe(term, object(), "TrainStep")
    with pytest.raises(TypeError):
        check_observe(object(), None)
    term._owner = object()
    with pytest.raises(ValueError, match="already attached"):
        check_observe(term, None)
    term.weight = 4
    assert term.weight == 4.0
    with pytest.raises(ValueError):
        term.weight = -1


def test_observations_on_the_cpu_are_refused():
    from gfv.observe import Observations
    with pytest.raises(RuntimeError, match="GPU"):
        Observations(torch.zeros(5, 3), torch.ones(5, 3))


def test_the_new_symbols_are_declared_and_refuse_bad_arguments_without_a_gpu():
    from gfv import lib
    names = {"gfv_obs_fwd", "gfv_obs_bwd", "gfv_obs_gather"}
    assert names <= set(lib.declared_symbols())
    h = lib.load()
    assert lib.OBS_RECORD == 4
    p = 4096                                   # a non-NULL, 16-byte aligned address that is never dereferenced: every call below is refused
    fwd = lambda **kw: h.gfv_obs_fwd(*[kw.get(k, d) for k, d in (
        ("phi", p), ("target", p), ("weight", p), ("N", 10), ("cb", p), ("ce", p), ("gcp", p), ("n_chunks", 1), ("B", 1), ("dim", p),
        ("sigma", p), ("losses", p), ("hyper", p), ("w_obs", p), ("partial", p), ("counter", p), ("rec", p), ("loss", p), ("gloss", p),
        ("stream", None))])
    for kw in (dict(phi=None), dict(target=None), dict(weight=None), dict(cb=None), dict(w_obs=None), dict(rec=None), dict(gloss=None),
               dict(B=0), dict(B=lib.POOL_MAX_GRAPHS + 1), dict(N=0), dict(N=-3), dict(n_chunks=0), dict(phi=p + 4), dict(rec=p + 8)):
        assert fwd(**kw) == -1, kw
    bwd = lambda **kw: h.gfv_obs_bwd(*[kw.get(k, d) for k, d in (
        ("rec", p), ("dec", p), ("phi", p), ("target", p), ("weight", p), ("batch", p), ("node_type", p), ("dim", p), ("sigma", p),
        ("N", 10), ("B", 1), ("g_dec", p), ("stream", None))])
    for kw in (dict(rec=None), dict(dec=None), dict(batch=None), dict(g_dec=None), dict(N=-1), dict(B=0), dict(B=lib.POOL_MAX_GRAPHS + 1),
               dict(phi=p + 4)):
        assert bwd(**kw) == -1, kw
    assert bwd(N=0) == 0                       # nothing to do, nothing launched
    vals, wts, rows = (C.c_void_p * 2)(p, None), (C.c_void_p * 2)(p, None), (C.c_int32 * 2)(3, 4)
    a = lambda x: C.addressof(x)
    gather = lambda v=a(vals), w=a(wts), r=a(rows), B=2, dv=p, dw=p, cap=7: h.gfv_obs_gather(v, w, r, B, dv, dw, cap, None)
    assert gather(v=None) == -1 and gather(r=None) == -1 and gather(dv=None) == -1 and gather(dw=None) == -1
    assert gather(B=0) == -1 and gather(B=lib.POOL_MAX_GRAPHS + 1) == -1 and gather(cap=6) == -1 and gather(cap=-1) == -1
    neg, half = (C.c_int32 * 2)(3, -1), (C.c_void_p * 2)(p, p)
    assert gather(r=a(neg)) == -1 and gather(w=a(half)) == -1
    empty = (C.c_int32 * 2)(0, 0)
    assert gather(r=a(empty)) == 0             # no rows: nothing launched
