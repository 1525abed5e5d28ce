"""Pool renewal on the device (gfv.pool.DevicePool.renew, csrc/pool.hip gfv_pool_renew): ONE launch re-draws the boundary
conditions of many entries.  The yardstick for the two profile kinds `reset_env` knows is `reset_env` itself, bit for bit; for the
kinds it does not know, the reference's own init_env recorded in tests/golden/renew_small.npz (make_renew_golden.py), to the
project's round-off bound for a float64 profile rounded to fp32 (2e-7 x max|want|, tests/test_pool_gpu.py:167)."""
import os

import numpy as np
import pytest
import torch

import cases
import make_renew_golden as MG
from oracle import fvgn_oracle as O

pytestmark = pytest.mark.gpu

BOUND = 2e-7
LR = 1e-3


def _pool(U=(0.15, 1.0)):
    """Four entries: the channel, the cavity, a variant of each."""
    from gfv import meshgen
    from gfv.pool import DevicePool
    raws = MG.raws()
    pool = DevicePool([meshgen.finish_mesh(raws["channel"], U=U[0]), meshgen.finish_mesh(raws["cavity"], U=U[1])])
    assert pool.add_variant(0, U=0.2, mu=1.5e-3) == 2 and pool.add_variant(1, U=0.8, dt=0.05) == 3
    return pool


def _owned(pool, i):
    p = pool.plans[i]
    return dict(x=pool.x[i], y=p.y, theta=p.theta, dt=p.dt, uvp_dim=p.uvp_dim)


def _model():
    from FVMmodel.importer import NNmodel
    from gfv.params import default_params
    P = O.init_parameters(cases.WEIGHT_SEED)
    m = NNmodel(default_params(dataset_size=1))
    sd = m.state_dict()
    for k, v in P.items():
        sd[k].copy_(v)
    m.load_state_dict(sd)
    return m.cuda()


# 1 ---------------------------------------------------------------------------------------------------------------------
def test_one_launch_equals_one_by_one():
    """renew([2, 0, 1]) against three reset_env calls on a twin pool: every owned tensor of all four entries bit for bit - the
    parabolic entries too (the kernel keeps the operation order of reset_env's float64 expression, uncontracted) -, the entry that
    was not named unchanged although its parent was renewed, and the host-side bc records equal."""
    new = {2: dict(U=0.31, mu=2.0e-3, source=0.05, aoa=3.0, dt=0.02), 0: dict(U=0.27, rho=1.1, L=0.12),
           1: dict(U=1.3, mu=5e-3, source=0.2, aoa=-2.0, dt=0.07)}
    a, b = _pool(), _pool()
    before3 = {k: v.clone() for k, v in _owned(a, 3).items()}
    order = [2, 0, 1]
    a.renew(order, [new[i] for i in order])
    for i in order:
        b.reset_env(i, **new[i])
    torch.cuda.synchronize()
    assert a.bc == b.bc
    for i in range(4):
        for k, mine in _owned(a, i).items():
            want = _owned(b, i)[k]
            if not torch.equal(mine, want):
                print(i, k, "max |difference|", float((mine - want).abs().max()), "max |want|", float(want.abs().max()))
            assert torch.equal(mine, want), (i, k)
    for k, v in _owned(a, 3).items():
        assert torch.equal(v, before3[k]), k
    # the renewal did something: a parabolic profile on the channel's inlet, the new scales, distinct variants
    assert float(a.plans[0].y[:, 0].max()) > 1.0 and float(a.plans[2].uvp_dim[0, 0]) == float(np.float32(0.31))
    assert not torch.equal(a.x[0], a.x[2]) and float(a.x[1][:, 0].max()) == float(np.float32(1.3))
    # (shared structure stays shared: the launch wrote the entries' own tensors only)
    assert a.plans[2].es.data_ptr() == a.plans[0].es.data_ptr() and a.pos64[2] is a.pos64[0]
    assert len(a._yrange_row) == 2                     # one row of ranges per topology: a variant uses its parent's


# 2 ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def golden():
    return dict(np.load(os.path.join(cases.ROOT, "tests", "golden", "renew_small.npz")))


def test_new_kinds_against_the_reference(golden):
    """uniform_aoa at 3 degrees, Taylor_Green, and a parabolic inlet over a uniform initial field, on both meshes, in ONE launch per
    case (the cavity through its variant).  The reference's parabolic profile over the cavity's lid - every inlet node at one height
    - is 0 / 0: those rows must be NaN here too, everything else within the bound."""
    from gfv import meshgen
    raws = MG.raws()
    pool = _pool()
    for case, (inlet_type, init_type, aoa) in MG.CASES.items():
        entries = {"channel": 0, "cavity": 3}
        pool.renew(list(entries.values()), [dict(U=MG.MESHES[name][2], aoa=aoa, inlet_type=inlet_type, init_field_type=init_type)
                                            for name in entries])
        torch.cuda.synchronize()
        for name, i in entries.items():
            U, nt = MG.MESHES[name][2], raws[name]["node|node_type"]
            assert pool.bc[i]["inlet_type"] == inlet_type and pool.bc[i]["init_field_type"] == init_type
            for what, mine, want in (("uvp_node", pool.x[i][:, 0:3].cpu().numpy(), golden[f"{name}.{case}.uvp_node"]),
                                     ("target", pool.plans[i].y.cpu().numpy(), golden[f"{name}.{case}.target"])):
                nan = np.isnan(want)
                assert np.array_equal(np.isnan(mine), nan), (name, case, what)
                assert nan.any() == ((name, case) == ("cavity", "mixed"))
                err, top = np.abs(np.where(nan, 0, mine - want)).max(), np.abs(want[~nan]).max()
                print(name, case, what, "max error", err, "bound", BOUND * top)
                assert err <= BOUND * top, (name, case, what)
            x = pool.x[i].cpu().numpy()
            assert np.array_equal(x[:, 3:12], np.broadcast_to(pool.plans[i].theta.cpu().numpy(), (x.shape[0], 9)))
            iw, wall = nt == meshgen.IN_WALL, nt == meshgen.WALL
            assert iw.sum() >= 2 and not x[wall, 0:2].any()
            if case == "aoa":      # v is not zero, and IN_WALL rows hold half of (u, v)
                assert np.abs(x[:, 1]).max() > 0.05 * U and not x[:, 2].any()
                free = (nt == meshgen.NORMAL) | (nt == meshgen.INFLOW)
                assert np.array_equal(x[iw, 0:2] * 2, np.broadcast_to(x[free][0, 0:2], (int(iw.sum()), 2)))
            if case == "tg":       # v and p are not zero, and IN_WALL rows hold half of (u, v, p): all three columns
                assert np.abs(x[:, 1]).max() > 0.5 * U and np.abs(x[:, 2]).max() > 0.2 * U
                uv, p = meshgen.velocity_profile(raws[name]["node|pos"], U, "Taylor_Green", pressure=True)
                full = np.concatenate((uv, p[:, None]), axis=1).astype(np.float32)
                assert np.abs(full[iw, 2]).min() > 0
                for c in range(3):
                    assert np.abs(x[iw, c] - full[iw, c] / 2).max() <= BOUND * np.abs(full[:, c]).max(), c
                pp = (nt == meshgen.OUTFLOW) | (nt == meshgen.NORMAL)
                assert np.abs(x[pp, 2] - full[pp, 2]).max() <= BOUND * np.abs(full[:, 2]).max()


# 3 ---------------------------------------------------------------------------------------------------------------------
def test_renew_does_not_synchronise():
    """Under torch's sync debug mode a renewal over cached ranges raises nothing; the control - reset_env, which indexes with a
    boolean mask - does raise under the same mode, so the mode is honoured here."""
    pool = _pool()
    pool.renew([0, 1], [dict(U=0.3), dict(U=1.1)])          # the first renewal reduces the ranges of both topologies
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        pool.renew([2, 3, 0], [dict(U=0.25, mu=2e-3), dict(U=0.9, inlet_type="uniform_aoa", aoa=4.0), dict(U=0.2)])
        with pytest.raises(RuntimeError):
            pool.reset_env(1, U=0.7)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    torch.cuda.synchronize()
    assert float(pool.plans[2].uvp_dim[0, 0]) == float(np.float32(0.25)) and float(pool.x[3][:, 1].max()) > 0


# 4 ---------------------------------------------------------------------------------------------------------------------
def _cyl_pool():
    from gfv import meshgen
    from gfv.pool import DevicePool
    m = meshgen.finish_mesh(MG.raws()["channel"], U=0.15)
    pool = DevicePool([m], [meshgen.random_fields(m, seed=5)])
    for j in range(2):
        pool.add_variant(0, fields=meshgen.random_fields(m, seed=11 + j), U=0.12 + 0.04 * j, mu=1e-3 * (1 + j), dt=0.01 * (2 + j))
    return pool


STEPS = 6   # two eager steps, the recorded one, three replayed ones


def _train(change):
    from gfv.pool_trainer import PoolTrainStep
    pool = _cyl_pool()
    ts = PoolTrainStep(_model(), pool, max_graphs=1, lr=LR, use_graph="list")
    losses = []
    for k in range(STEPS):
        if k == STEPS - 1:
            assert ts.stats()["recorded"] == 1 and ts.stats()["replayed"] == 2       # (the first steps of a signature run eager)
            change(pool)
        losses.append(float(ts.step([k % 3])))
    assert ts.stats()["recorded"] == 1 and ts.stats()["replayed"] == 3
    return losses, ts.flat_p.clone()


def test_renew_reaches_a_replayed_step():
    """tests/test_pool_train_gpu.py::test_reset_env_reaches_a_replayed_step with the renewal between the second and the third
    REPLAYED step: the step after it equals the step of a twin that used reset_env, loss and parameters bit for bit."""
    last = (STEPS - 1) % 3
    new = {last: dict(U=0.31, mu=2e-3, dt=0.02), (last + 1) % 3: dict(U=0.22)}
    order = list(new)
    losses, params = _train(lambda pool: pool.renew(order, [new[i] for i in order]))
    ref_losses, ref_params = _train(lambda pool: [pool.reset_env(i, **new[i]) for i in order])
    assert losses == ref_losses and torch.equal(params, ref_params)
    unchanged, _ = _train(lambda pool: None)
    assert unchanged[:-1] == losses[:-1] and unchanged[-1] != losses[-1]     # the new boundary condition did change the step


# 5 ---------------------------------------------------------------------------------------------------------------------
def test_an_entry_without_inlet_nodes():
    """A cavity whose lid is retyped to WALL has no inlet node: the inlet profile is empty (Set_BC.py:24-25) - nothing comes from
    it, nothing divides by the (empty) inlet range - and the field is the initial-field kind over all nodes, zero on the walls."""
    from gfv import meshgen
    from gfv.pool import DevicePool
    raw = dict(MG.raws()["cavity"])
    nt = raw["node|node_type"].copy()
    nt[(nt == meshgen.INFLOW) | (nt == meshgen.IN_WALL) | (nt == meshgen.PRESS_POINT)] = meshgen.WALL
    raw["node|node_type"] = nt
    assert set(np.unique(nt)) == {meshgen.NORMAL, meshgen.WALL}
    m = meshgen.finish_mesh(raw, U=1.0)
    a, b = DevicePool([m]), DevicePool([m])
    a.renew([0], [dict(U=0.6, mu=3e-3)])
    b.reset_env(0, U=0.6, mu=3e-3)
    torch.cuda.synchronize()
    for k, mine in _owned(a, 0).items():
        assert torch.equal(mine, _owned(b, 0)[k]), k
    wall = torch.from_numpy(nt == meshgen.WALL).cuda()
    assert float(a.x[0][~wall, 0].min()) == float(np.float32(0.6)) and not bool(a.x[0][wall, 0:3].any())
    # a parabolic INLET over no inlet node under a Taylor-Green field: (0 - 0) / 0 is never formed
    a.renew([0], [dict(U=0.6, inlet_type="parabolic", init_field_type="Taylor_Green")])
    torch.cuda.synchronize()
    x, y = a.x[0].cpu().numpy(), a.plans[0].y.cpu().numpy()
    assert np.isfinite(x).all() and np.isfinite(y).all()
    uv, p = meshgen.velocity_profile(raw["node|pos"], 0.6, "Taylor_Green", pressure=True)
    want = np.concatenate((uv, p[:, None]), axis=1).astype(np.float32)
    want[nt == meshgen.WALL, 0:2] = 0
    for c in range(3):
        assert np.abs(x[:, c] - want[:, c]).max() <= BOUND * np.abs(want[:, c]).max(), c
    # and the parabolic field over all nodes, for which the range is the mesh's own
    a.renew([0], [dict(U=0.6, inlet_type="parabolic", init_field_type="parabolic")])
    torch.cuda.synchronize()
    x = a.x[0].cpu().numpy()
    want = meshgen.velocity_profile(raw["node|pos"], 0.6, "parabolic")[:, 0].astype(np.float32)
    want[nt == meshgen.WALL] = 0
    assert np.isfinite(x).all() and np.abs(x[:, 0] - want).max() <= BOUND * np.abs(want).max() and want.max() > 0.6
