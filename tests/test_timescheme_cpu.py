"""The time scheme (gfv/timescheme.py) without a GPU.

1. exactness in time, in float64: on node fields that are quadratic in t the momentum residual's time term with the BDF2
   substitution (u* = u_n + (u_n - u_{n-1}) / 3, dt / 1.5) is the exact derivative at the new level; the BDF1 form misses it by
   c dt - so the test can see the difference;
2. the numpy launch rule (tests/timescheme_ref.py) over the clock sequence 0, 0, 1, 1, 1, 2, 3;
3. argument checks and every refusal that needs no device."""
import types

import numpy as np
import pytest
import torch

import cases
import fvm_float64 as F
import timescheme_ref as R

f32 = np.float32
CLOCKS = (0, 0, 1, 1, 1, 2, 3)
ERR_ARG = -1          # GFV_ERR_ARG of include/gfv.h


def _poly():
    from test_config5_gpu import _small_polygon_graphs
    return _small_polygon_graphs()


# ---- 1. exactness in time -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("conserved", [True, False], ids=["conserved", "non-conserved"])
def test_bdf2_time_term_is_exact_on_fields_quadratic_in_time(conserved):
    graphs = F.distinct_coefficients(_poly(), 3)
    G = F.graph_tensors(graphs)
    nb = G["node_batch"]
    N = nb.shape[0]
    g = torch.Generator().manual_seed(5)
    a, b, c = (0.5 * torch.randn(N, 2, generator=g, dtype=torch.float64) for _ in range(3))
    dt = G["dt_graph"].reshape(-1)[nb].reshape(N, 1)
    # the Dirichlet rows of the new level are the targets y, whatever dec says: a field that passes through them at t = dt
    nt = G["node_type"]
    dirichlet = ((nt == 1) | (nt == 3) | (nt == 4) | (nt == 5)).reshape(N, 1)
    a = torch.where(dirichlet, G["y"] - b * dt - c * dt * dt, a)
    u = lambda t: a + b * t + c * t * t
    u_prev, u_n, u_new = u(-dt), u(0 * dt), u(dt)
    assert float(u_new.abs().max()) < 9.0
    dec = torch.cat((10.0 * torch.atanh(u_new / 10.0), torch.randn(N, 1, generator=g, dtype=torch.float64)), dim=1)
    theta0 = G["theta_PDE"][G["cell_batch"], 0:1]
    area = G["cells_area"].reshape(-1, 1)
    G0 = dict(G, theta_PDE=torch.cat((torch.zeros_like(G["theta_PDE"][:, 0:1]), G["theta_PDE"][:, 1:]), dim=1))
    dt_g = G["dt_graph"].reshape(-1)

    def time_term(uv_star, dt_eff):
        run = lambda GG: R.stages_ts(dec, u_n, uv_star, dt_eff, GG, conserved, "implicit")
        with_t, without = run(G), run(G0)
        assert float((with_t["phi"][:, 0:2] - u_new).abs().max()) < 1e-14          # dec reproduces u(dt) (free rows) / y (Dirichlet)
        return with_t["cres"][:, 1:3] - without["cres"][:, 1:3]

    def cellmean(field):
        # the section's own node -> cell interpolation (linear in the field): what channels 5,6 of phic hold of a baseline
        return R.stages_ts(dec, u_n, field, dt_g, G, conserved, "implicit")["phic"][:, 5:7]

    exact = theta0 * area * cellmean(b + 2.0 * c * dt)
    miss = theta0 * area * cellmean(c * dt)
    bound = 1e-12 * float(exact.abs().max())
    bdf2 = time_term(u_n + (u_n - u_prev) / 3.0, dt_g / 1.5)
    bdf1 = time_term(u_n, dt_g)
    e2, e1 = float((bdf2 - exact).abs().max()), float(((exact - bdf1) - miss).abs().max())
    print(f"time term: max |exact| {float(exact.abs().max()):.3e}, BDF2 off by {e2:.1e}, BDF1 off its c dt form by {e1:.1e}, "
          f"bound {bound:.1e}, max |miss| {float(miss.abs().max()):.3e}")
    assert e2 <= bound
    assert e1 <= bound
    assert float(miss.abs().max()) > 1e6 * bound            # the difference between the two schemes is far above the bound


# ---- 2. the launch rule -----------------------------------------------------------------------------------------------------------
def _rule_inputs():
    graphs = F.distinct_coefficients(cases.make_graphs("cyl_cavity_b2"), 7)
    gn, gi = graphs[0], graphs[4]
    batch = gn.batch.reshape(-1).numpy()
    g = np.random.default_rng(9)
    fields = [gn.x.numpy().astype(f32)]
    for _ in range(3):
        nxt = fields[-1].copy()
        nxt[:, 0:3] += (0.1 * g.standard_normal((nxt.shape[0], 3))).astype(f32)
        fields.append(nxt)
    return graphs, batch, gi.uvp_dim.numpy().astype(f32), gi.dt_graph.reshape(-1).numpy().astype(f32), fields


def _same(a, b):
    return np.asarray(a, dtype=f32).tobytes() == np.asarray(b, dtype=f32).tobytes()


def test_the_launch_rule_over_a_clock_sequence():
    graphs, batch, dim, dt, fields = _rule_inputs()
    k = R.LaunchRule(batch, dim, dt, R.BDF2)
    k.reset(0)
    seen, last = [], None
    for c in CLOCKS:
        before = k.state()
        active = k.launch(fields[c], c)
        seen.append(active)
        st = k.state()
        if c == last:
            assert all(_same(st[n], before[n]) for n in st), c           # a repeated clock changes nothing
        if not active:
            assert _same(st["dt_eff"], dt)
        else:
            assert _same(st["ustar"], R.ustar_of(fields[c], fields[c - 1], batch, dim))
            assert _same(st["dt_eff"], dt / f32(1.5)) and not _same(st["dt_eff"], dt)
        assert _same(st["ring"][c & 1], fields[c][:, 0:2])
        last = c
    assert seen == [False, False, True, True, True, True, True]
    # the inactive launch's baseline has the bits of the input preparation's uv_old
    k0 = R.LaunchRule(batch, dim, dt, R.BDF2)
    k0.reset(0)
    k0.launch(fields[0], 0)
    assert _same(k0.ustar, F.uv_old_of(graphs).numpy())
    # "bdf1" is never active
    k1 = R.LaunchRule(batch, dim, dt, R.BDF1)
    k1.reset(0)
    for c in CLOCKS:
        assert not k1.launch(fields[c], c)
        dimn = dim[batch][:, 0:2]
        assert _same(k1.ustar, fields[c][:, 0:2] / dimn) and _same(k1.dt_eff, dt)
    # previous= makes clock 0 active
    prev = fields[3][:, 0:3]
    kp = R.LaunchRule(batch, dim, dt, R.BDF2)
    kp.install_previous(prev, 0)
    assert kp.launch(fields[0], 0) and _same(kp.ustar, R.ustar_of(fields[0], prev, batch, dim))
    assert not _same(kp.ustar, k0.ustar)
    # reset makes the next launch inactive, the one behind the next advance active again
    kp.launch(fields[1], 1)
    kp.reset(1)
    assert not kp.launch(fields[1], 1) and _same(kp.dt_eff, dt)
    assert kp.launch(fields[2], 2) and _same(kp.ustar, R.ustar_of(fields[2], fields[1], batch, dim))


# ---- 3. argument checks and refusals ------------------------------------------------------------------------------------------------
def test_argument_checks_and_refusals_without_a_device():
    from gfv import timescheme as T
    from gfv.engine import _check_time_state
    from gfv.march import MarchStep
    from gfv.pool_trainer import PoolTrainStep
    assert T.TimeScheme().scheme == "bdf2" and T.TimeScheme("bdf1").scheme == "bdf1"
    for bad in ("bdf3", "BDF2", 2, None):
        with pytest.raises(ValueError, match="scheme must be one of"):
            T.TimeScheme(bad)
    for bad in (torch.zeros(5), torch.zeros(5, 1), torch.zeros(0, 2), [[0.0, 0.0]], torch.zeros(5, 2, 2)):
        with pytest.raises(ValueError, match="previous must be a"):
            T.TimeScheme("bdf2", previous=bad)
    with pytest.raises(ValueError, match="floating-point"):
        T.TimeScheme("bdf2", previous=torch.zeros(5, 2, dtype=torch.int32))
    with pytest.raises(ValueError, match="must live on the GPU"):
        T.TimeScheme("bdf2", previous=torch.zeros(5, 3))
    sch = T.TimeScheme("bdf2")
    for call in (sch.read, sch.reset, sch.launch, sch.tick, sch.state_dict, lambda: sch.load_state_dict({"scheme": "bdf2"})):
        with pytest.raises(RuntimeError, match="not attached"):
            call()
    # owners: the wrong type, a second owner, the pool trainer
    with pytest.raises(ValueError, match="gfv.timescheme.TimeScheme or None"):
        T.check_owner("bdf2")
    with pytest.raises(ValueError, match="gfv.timescheme.TimeScheme or None"):
        MarchStep(None, None, time_scheme="bdf2")
    T.check_owner(None)
    T.check_owner(sch)
    sch._owner = "MarchStep"
    with pytest.raises(ValueError, match="already attached to a MarchStep"):
        T.check_owner(sch)
    with pytest.raises(ValueError, match="already attached"):
        MarchStep(None, None, time_scheme=sch)
    with pytest.raises(ValueError, match="the pool owns the fields"):
        PoolTrainStep(None, None, time_scheme=T.TimeScheme())
    # the node state an owner hands over
    with pytest.raises(ValueError, match=r"\[7, 12\]"):
        T.check_field(torch.zeros(6, 12), 7)
    with pytest.raises(ValueError, match="contiguous float32"):
        T.check_field(torch.zeros(7, 12, dtype=torch.float64), 7)
    with pytest.raises(ValueError, match="must live on the GPU"):
        T.check_field(torch.zeros(7, 12), 7)
    # what the engine refuses of time_state=
    pl, dev = types.SimpleNamespace(N=7, B=2), torch.device("cpu")
    ok = (torch.zeros(7, 2), torch.zeros(2))
    assert _check_time_state(ok, pl, dev) == ok
    for bad in (None, 3, (ok[0],), (torch.zeros(7, 3), ok[1]), (ok[0], torch.zeros(3)), (ok[0].double(), ok[1]),
                (torch.zeros(2, 7).t(), ok[1])):
        with pytest.raises(ValueError, match="time_state"):
            _check_time_state(bad, pl, dev)
    with pytest.raises(ValueError, match="lives on"):
        _check_time_state(ok, pl, torch.device("meta"))


def test_the_library_declares_the_two_entry_points():
    from gfv import lib as L
    assert {"gfv_time_scheme_update", "gfv_phi_fwd_ts"} <= set(L.declared_symbols())
    assert (L.TIME_SCHEME_RECORD, L.TIME_SCHEME_BDF1, L.TIME_SCHEME_BDF2) == (4, R.BDF1, R.BDF2)
    lib = L.load(raw=True)
    # GFV_ERR_ARG before anything is launched: NULL pointers, N < 1, B < 1, a misaligned x_backup / ring
    a = 1 << 20
    good = [a, a, a, a, 5, 1, a, a, a, a, a, None]
    assert lib.gfv_time_scheme_update(*[None if i == 0 else v for i, v in enumerate(good)]) == ERR_ARG
    for i in (0, 1, 2, 3, 6, 7, 8, 9, 10):
        args = list(good)
        args[i] = None
        assert lib.gfv_time_scheme_update(*args) == ERR_ARG, i
    for i, v in ((4, 0), (5, 0), (0, a + 8), (8, a + 4), (9, a + 4)):
        args = list(good)
        args[i] = v
        assert lib.gfv_time_scheme_update(*args) == ERR_ARG, i
    assert lib.gfv_phi_fwd_ts(a, a, a, a, None, a, 5, 1, None) == ERR_ARG
