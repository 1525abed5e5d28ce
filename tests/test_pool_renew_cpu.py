"""CPU: the host side of pool renewal (include/gfv.h gfv_pool_renew, gfv.pool.DevicePool.renew, gfv.meshgen.velocity_profile,
gfv.renew.PoolRenewal): every bad argument is refused before anything touches a device, the host profile meets the
reference-generated fixture tests/golden/renew_small.npz (make_renew_golden.py) for the new kinds and is bit for bit what it was
for the two old ones, and the renewal schedule is the reference's (pre_train_Adam.py:116-118, Graph_loader.py:154-229,389-396)."""
import ctypes as C
import os
import re
from math import ceil

import numpy as np
import pytest

import cases
import make_renew_golden as MG

BOUND = 2e-7   # x max|want|: the project's round-off bound for a float64 profile rounded to fp32 (tests/test_pool_gpu.py:167)


@pytest.fixture(scope="module")
def golden():
    return dict(np.load(os.path.join(cases.ROOT, "tests", "golden", "renew_small.npz")))


def _records(K=3):
    """K acceptable records over fake pointers (nothing is launched: the acceptable call itself needs a device)."""
    from gfv import lib
    recs = (lib.RenewRec * K)()
    for k, r in enumerate(recs):
        base = 0x1000000 * (k + 1)
        r.x, r.y, r.theta, r.dt, r.uvp_dim, r.node_type, r.pos, r.yrange = (base + 0x10000 * j for j in range(8))
        r.N, r.U, r.cos_aoa, r.sin_aoa = 100 + k, 0.3, 1.0, 0.0
        r.inlet_kind, r.init_kind = lib.RENEW_KINDS["parabolic"], lib.RENEW_KINDS["uniform"]
    return recs


def test_pool_renew_is_declared_exported_and_bound():
    from gfv import lib
    handle = lib.load()
    header = open(os.path.join(cases.ROOT, "include", "gfv.h")).read()
    assert "gfv_pool_renew" in set(re.findall(r"\b(gfv_[a-z0-9_]+)\s*\(", header))
    assert "gfv_pool_renew" in lib.declared_symbols() and handle.gfv_pool_renew.argtypes is not None
    assert handle.gfv_abi_version() == 3                                   # additive: the version stays
    assert handle.gfv_struct_size(10) == C.sizeof(lib.RenewRec) == 8 * 8 + 3 * 8 + 13 * 4 + 3 * 4
    names = re.search(r"enum \{ (GFV_RENEW_NONE[^}]*)\}", header).group(1)
    codes = {n.strip(): int(v) for n, v in (kv.split("=") for kv in names.split(","))}
    assert codes == {"GFV_RENEW_NONE": lib.RENEW_KINDS[None], "GFV_RENEW_PARABOLIC": lib.RENEW_KINDS["parabolic"],
                     "GFV_RENEW_UNIFORM": lib.RENEW_KINDS["uniform"], "GFV_RENEW_UNIFORM_AOA": lib.RENEW_KINDS["uniform_aoa"],
                     "GFV_RENEW_TAYLOR_GREEN": lib.RENEW_KINDS["Taylor_Green"]}


def test_pool_renew_refuses_bad_arguments_without_a_gpu():
    """Each case differs from an acceptable call in ONE argument."""
    from gfv import lib
    handle = lib.load()
    call = lambda recs, K: handle.gfv_pool_renew(C.addressof(recs), K, None)
    assert handle.gfv_pool_renew(None, 1, None) == -1                       # NULL records
    big = _records(lib.POOL_MAX_GRAPHS + 1)
    for K in (0, -2, lib.POOL_MAX_GRAPHS + 1):                              # K outside [1, POOL_MAX_GRAPHS]
        assert call(big, K) == -1, K
    for name in ("x", "y", "theta", "dt", "uvp_dim", "node_type", "pos", "yrange"):   # a NULL pointer inside a record
        for k in (0, 2):
            recs = _records()
            setattr(recs[k], name, None)
            assert call(recs, 3) == -1, (name, k)
    for n in (0, -5):                                                       # N < 1
        recs = _records()
        recs[1].N = n
        assert call(recs, 3) == -1, n
    for field in ("inlet_kind", "init_kind"):                               # an unknown kind code
        for code in (-1, 5, 99):
            recs = _records()
            setattr(recs[2], field, code)
            assert call(recs, 3) == -1, (field, code)
    for U in (0.0, -0.0, float("nan"), float("inf")):                       # U == 0 (and a U nothing can be divided by)
        recs = _records()
        recs[0].U = U
        assert call(recs, 3) == -1, U
    recs = _records()
    recs[2].x = recs[0].x                                                   # two records of one entry
    assert call(recs, 3) == -1


def _finished(name, case):
    from gfv import meshgen
    raw = dict(MG.raws()[name])
    inlet_type, init_type, aoa = MG.CASES[case]
    raw["bc"] = dict(raw["bc"], U=MG.MESHES[name][2], aoa=aoa, inlet_type=inlet_type, init_field_type=init_type)
    return meshgen.finish_mesh(raw)


@pytest.mark.parametrize("name", list(MG.MESHES))
@pytest.mark.parametrize("case", list(MG.CASES))
def test_host_profile_meets_the_reference_fixture(golden, name, case):
    """finish_mesh (velocity_profile for the initial field and the inlet targets, init_env's masks) against the reference's init_env.
    The reference's parabolic profile over the cavity's lid - all inlet nodes at one height - is 0 / 0: the NaN rows must be the
    same rows, everything else within the bound."""
    m = _finished(name, case)
    for mine, want in ((m["init_uvp"], golden[f"{name}.{case}.uvp_node"]), (m["target|uvp"], golden[f"{name}.{case}.target"])):
        assert mine.dtype == np.float32 and mine.shape == want.shape
        nan = np.isnan(want)
        assert np.array_equal(np.isnan(mine), nan)
        assert nan.any() == ((name, case) == ("cavity", "mixed"))
        err, top = np.abs(np.where(nan, 0, mine - want)).max(), np.abs(want[~nan]).max()
        print(name, case, "max error", err, "bound", BOUND * top)
        assert err <= BOUND * top


def test_old_kinds_are_bit_for_bit_what_they_were(golden):
    from gfv import meshgen
    for name, raw in MG.raws().items():
        pos, nt, U = raw["node|pos"], raw["node|node_type"], MG.MESHES[name][2]
        inlet = (nt == meshgen.INFLOW) | (nt == meshgen.IN_WALL) | (nt == meshgen.PRESS_POINT)
        for kind in ("parabolic", "uniform"):
            with np.errstate(invalid="ignore"):
                got_all, got_in = meshgen.velocity_profile(pos, U, kind), meshgen.velocity_profile(pos[inlet], U, kind)
            for got, key in ((got_all, f"{name}.old.{kind}.all"), (got_in, f"{name}.old.{kind}.inlet")):
                assert got.dtype == np.float64 and np.array_equal(got, golden[key], equal_nan=True), key
            uv, p = meshgen.velocity_profile(pos, U, kind, pressure=True)
            assert np.array_equal(uv, got_all, equal_nan=True) and not p.any()
    # a mesh finished with the key absent is what it was: p = 0, IN_WALL rows of u halved
    m = meshgen.finish_mesh(MG.raws()["channel"], U=0.31)
    assert "init_field_type" not in m["bc"] and not m["init_uvp"][:, 1:].any()
    empty = np.zeros((0, 2))
    for kind in ("parabolic", "uniform", "uniform_aoa", "Taylor_Green", None):
        uv, p = meshgen.velocity_profile(empty, 1.0, kind, pressure=True)       # no inlet node: an empty profile
        assert uv.shape == (0, 2) and p.shape == (0,)
    assert not meshgen.velocity_profile(MG.raws()["cavity"]["node|pos"], 1.0, None).any()
    for bad in ("wave", [0.0, 0.0, 0.0], "data.h5"):
        with pytest.raises(ValueError):
            meshgen.velocity_profile(MG.raws()["cavity"]["node|pos"], 1.0, bad)


def test_fixture_is_the_hard_path(golden):
    """Where `reset_env`'s shortcut (v = p = 0, only u halved) would be wrong: v and p are non-zero and IN_WALL rows are half of the
    profile in all three columns."""
    from gfv import meshgen
    for name, raw in MG.raws().items():
        pos, nt, U = raw["node|pos"], raw["node|node_type"], MG.MESHES[name][2]
        assert (nt == meshgen.IN_WALL).sum() >= 2
        aoa = golden[f"{name}.aoa.uvp_node"]
        assert np.abs(aoa[:, 1]).max() > 0.05 * U and not aoa[:, 2].any()
        tg = golden[f"{name}.tg.uvp_node"]
        assert np.abs(tg[:, 1]).max() > 0.5 * U and np.abs(tg[:, 2]).max() > 0.2 * U
        uv, p = meshgen.velocity_profile(pos, U, "Taylor_Green", pressure=True)
        full = np.concatenate((uv, p[:, None]), axis=1).astype(np.float32)
        iw = nt == meshgen.IN_WALL
        assert np.abs(full[iw, 2]).min() > 0
        for c in range(3):
            assert np.abs(tg[iw, c] - full[iw, c] / 2).max() <= BOUND * np.abs(tg[:, c]).max(), c


def test_renew_refuses_before_it_changes_anything():
    """DevicePool.renew on a pool kept on the host: every refusal comes before a device is touched or a `bc` record changed."""
    import copy
    from gfv import meshgen
    from gfv.pool import DevicePool
    raws = MG.raws()
    ms = [meshgen.finish_mesh(raws["channel"], U=0.15), meshgen.finish_mesh(raws["cavity"], U=1.0)]
    nobc = dict(ms[1])
    nobc.pop("bc")
    pool = DevicePool(ms + [nobc], device="cpu")
    before = copy.deepcopy(pool.bc)
    ok = dict(U=0.31, mu=2e-3)
    for indices, sampled in (([0, 2], [ok, ok]),                                           # an entry without its bc record
                             ([0, 1], [ok, dict(ok, inlet_type="wave")]),                   # unknown kinds
                             ([0, 1], [dict(ok, init_field_type="Taylor-Green"), ok]),
                             ([0, 1, 0], [ok, ok, ok]),                                     # a repeated index
                             ([1], [dict(ok, init_field_type=[0.1, 0.0, 0.0])]),            # the list-valued form
                             ([1], [dict(ok, init_field_type="data.vtu")]),                 # the file-valued forms
                             ([1], [dict(ok, init_field_type="field.h5")]),
                             ([0, 1], [ok]),                                                # one dict per index
                             ([5], [ok]),
                             ([0], [dict(ok, U=0.0)])):
        with pytest.raises(ValueError):
            pool.renew(indices, sampled)
        assert pool.bc == before


# the schedule ------------------------------------------------------------------------------------------------------------
class _FakePool:
    def __init__(self, n):
        self.n, self.calls = n, []

    def renew(self, indices, sampled):
        self.calls.append((list(indices), list(sampled)))


@pytest.mark.parametrize("dataset_size,asl", [(100, 20), (8, 20), (1, 1)])
def test_pool_renewal_schedule_is_the_reference_s(dataset_size, asl):
    from gfv.renew import PoolRenewal
    pool = _FakePool(dataset_size)
    draws = []

    def draw(i):
        draws.append(i)
        return dict(U=0.1 * (len(draws) + 1), tag=len(draws))
    sched = PoolRenewal(pool, draw, average_sequence_length=asl)             # dataset_size: the pool's
    # the reference's arithmetic, written out (pre_train_Adam.py:116-118; Data_Pool: pop(0) ... append, Graph_loader.py:163,229)
    period, rst_time = ceil(asl / dataset_size), ceil(dataset_size / asl)
    assert (period, rst_time) == {(100, 20): (1, 5), (8, 20): (3, 1), (1, 1): (1, 1)}[(dataset_size, asl)]
    assert (sched.period, sched.rst_time) == (period, rst_time)
    ref_pool, ref_flag, events = list(range(dataset_size)), False, 0
    for epoch in range(4 * period + 1):
        if epoch % period == 0:
            ref_flag = True
        assert sched.arm(epoch) == ref_flag
        for inner in range(2):                                               # two paybacks per epoch: only the first one renews
            want = []
            if ref_flag:
                for _ in range(rst_time):
                    old = ref_pool.pop(0)
                    want.append(old)
                    ref_pool.append(old)
                ref_flag = False
            n_calls = len(pool.calls)
            got = sched.after_payback()
            assert got == want and list(sched.age) == ref_pool
            if want:
                events += 1
                assert len(pool.calls) == n_calls + 1                        # ONE pool.renew call per renewal
                idx, sampled = pool.calls[-1]
                assert idx == want and [s["tag"] for s in sampled] == list(range(len(draws) - len(want) + 1, len(draws) + 1))
                assert draws[-len(want):] == want and list(sched.age)[-len(want):] == want   # renewed: the youngest
            else:
                assert len(pool.calls) == n_calls
    assert events == 5 and sched.renewed == 5 * rst_time
    if dataset_size == 100:                                                  # first in first out over several events
        assert [c[0] for c in pool.calls[:3]] == [[0, 1, 2, 3, 4], [5, 6, 7, 8, 9], [10, 11, 12, 13, 14]]
    if dataset_size == 8:
        assert [c[0] for c in pool.calls] == [[0], [1], [2], [3], [4]]
        assert [e for e in range(14) if e % sched.period == 0] == [0, 3, 6, 9, 12]


def test_pool_renewal_edges():
    from gfv.renew import PoolRenewal
    pool = _FakePool(3)
    sched = PoolRenewal(pool, lambda i: dict(U=1.0), dataset_size=3, average_sequence_length=2)
    assert (sched.period, sched.rst_time) == (1, 2)
    assert sched.after_payback() == [] and not pool.calls                   # not armed: nothing happens
    sched.arm(0)
    assert sched.after_payback() == [0, 1] and list(sched.age) == [2, 0, 1]
    pool.n = 4                                                               # an entry added since (add_variant): the youngest
    sched.arm(1)
    assert sched.after_payback() == [2, 0] and list(sched.age) == [1, 3, 2, 0]
    with pytest.raises(ValueError):
        PoolRenewal(pool, None, dataset_size=0)
    with pytest.raises(ValueError):
        PoolRenewal(pool, None, average_sequence_length=0)
    few = PoolRenewal(_FakePool(2), lambda i: {}, dataset_size=10, average_sequence_length=2)   # retires 5 of a pool of 2
    few.arm(0)
    with pytest.raises(ValueError):
        few.after_payback()
    assert few.armed and list(few.age) == [0, 1]
