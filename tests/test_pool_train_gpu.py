"""Pool training (gfv/pool_trainer.py, gfv.pool.BatchArena, csrc/pool.hip): a different batch of the device-resident pool every
step on the recorded launch path.  The bar between launch modes is bit identity, as in tests/test_pool_gpu.py: `==` on losses,
`torch.equal` on parameters - no tolerances, except the one test_reset_env_on_the_device_equals_host_transform_mesh already uses
for the float64 inlet profile rounded to fp32 (2e-7 relative)."""
import numpy as np
import pytest
import torch

import cases
from oracle import fvgn_oracle as O

pytestmark = pytest.mark.gpu

LR = 1e-3


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


def _plan_tensors(plan):
    return {k: v for k, v in vars(plan).items() if torch.is_tensor(v)}


def _reference_run(pool, seq, dataset_size=1, between=None, payback=False):
    """The existing changing-batch path: pool.batch + TrainStep(use_graph=False).set_batch + step."""
    from gfv.trainer import TrainStep
    model = _model(dataset_size)
    ts, losses = None, []
    for k, idx in enumerate(seq):
        if between is not None:
            between(k, pool)
        g, _ = pool.batch(idx)
        if ts is None:
            ts = TrainStep(model, g, lr=LR, use_graph=False)
        else:
            ts.set_batch(g)
        losses.append(float(ts.step()))
        if payback:
            pool.payback(idx, ts.uvp_node)
    return losses, ts, model


def _pool_run(pool, seq, dataset_size=1, between=None, payback=False, **kw):
    from gfv.pool_trainer import PoolTrainStep
    model = _model(dataset_size)
    ts = PoolTrainStep(model, pool, lr=LR, **kw)
    losses = []
    for k, idx in enumerate(seq):
        if between is not None:
            between(k, pool)
        losses.append(float(ts.step(idx, payback=payback)))
    return losses, ts, model


def _cyl_pool_with_variants():
    from gfv import meshgen
    from gfv.pool import DevicePool
    raw = meshgen.raw_tri_channel_cylinder(nx=30, ny=6, quad_fraction=0.0, seed=21)
    m = meshgen.finish_mesh(raw, U=0.15)
    pool = DevicePool([m], [meshgen.random_fields(m, seed=5)])
    for j in range(5):
        v = pool.add_variant(0, fields=meshgen.random_fields(m, seed=11 + j), U=0.12 + 0.04 * j, mu=1e-3 * (1 + j), dt=0.01 * (2 + j))
        assert v == j + 1
    return pool


# 1 ---------------------------------------------------------------------------------------------------------------------
def test_arena_assembly_equals_pool_batch():
    """Batches loaded one after the other into ONE arena (a smaller one follows a larger one) equal pool.batch tensor for tensor."""
    from gfv.pool import DevicePool
    ms, fs = _meshes()
    pool = DevicePool(ms, fs)
    arena = pool.arena(4)
    for indices in ([2, 0], [1], [3, 1, 0, 2], [0, 0]):
        graphs, plan = arena.load(indices)
        ref_graphs, ref = pool.batch(indices)
        torch.cuda.synchronize()
        assert torch.equal(graphs[0].x, ref_graphs[0].x)
        assert torch.equal(arena.x_raw(graphs), ref_graphs[0].x)
        checked = 0
        for k, v in vars(ref).items():
            if k.startswith("_"):
                continue                     # (pool.batch keeps its upload buffer alive on the plan: not a plan tensor)
            if torch.is_tensor(v):
                mine = getattr(plan, k)
                assert mine.shape == v.shape and mine.dtype == v.dtype, (k, mine.shape, v.shape)
                assert torch.equal(mine, v), (indices, k)
                checked += 1
            elif isinstance(v, int):
                assert getattr(plan, k) == v, k
        assert checked >= 45
        for a, b in zip(graphs[4].__dict__.items(), ref_graphs[4].__dict__.items()):
            assert a[0] == b[0] and (a[1] == b[1] if not torch.is_tensor(a[1]) else torch.equal(a[1], b[1])), a[0]
    with pytest.raises(ValueError):
        arena.load([0, 1, 2, 3, 0])


# 2 ---------------------------------------------------------------------------------------------------------------------
def test_equal_signatures_give_stable_pointers():
    pool = _cyl_pool_with_variants()
    arena = pool.arena(2)
    assert arena.signature([0, 3]) == arena.signature([4, 1]) != arena.signature([0])
    g1, p1 = arena.load([0, 3])
    ptr1 = {k: (v.data_ptr(), tuple(v.shape)) for k, v in _plan_tensors(p1).items()}
    x1 = (g1[0].x.data_ptr(), arena.x_raw(g1).data_ptr())
    arena.load([2])
    g2, p2 = arena.load([4, 1])
    ptr2 = {k: (v.data_ptr(), tuple(v.shape)) for k, v in _plan_tensors(p2).items()}
    assert len(ptr1) >= 45 and ptr1 == ptr2
    assert x1 == (g2[0].x.data_ptr(), arena.x_raw(g2).data_ptr())


# 3 ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B", [1, 2])
def test_replay_across_batches_of_one_signature(B):
    """Twelve steps, a different batch each (one cylinder mesh + five variants with other U, mu, dt and fields): the list recorded
    at the third step is replayed for the nine after it and gives the bits of the existing eager path."""
    seq = [[k % 6] for k in range(12)] if B == 1 else [[k % 6, (k + 2) % 6] for k in range(12)]
    ref_losses, ref_ts, _ = _reference_run(_cyl_pool_with_variants(), seq)
    losses, ts, _ = _pool_run(_cyl_pool_with_variants(), seq, max_graphs=2, use_graph="list")
    assert len(set(ref_losses)) > 6          # the batches do differ
    assert losses == ref_losses
    assert torch.equal(ts.flat_p, ref_ts.flat_p)
    st = ts.stats()
    assert st["replayed"] >= 9 and st["recorded"] == 1 and st["lists"] == 1 and st["list_bytes"] > 0, st


# 4 ---------------------------------------------------------------------------------------------------------------------
def _permuted(raw, seed):
    """The same mesh with its nodes renumbered: same sizes, other connectivity tables."""
    from gfv import meshgen
    rng = np.random.default_rng(seed)
    n = raw["node|pos"].shape[0]
    perm = rng.permutation(n)                                   # new id of old node i
    pos, nt = np.empty_like(raw["node|pos"]), np.empty_like(raw["node|node_type"])
    pos[perm], nt[perm] = raw["node|pos"], raw["node|node_type"]
    cn, cnt = perm[raw["cells_node"]], np.bincount(raw["cells_index"])
    blocks, start, c = [], 0, 0
    while c < len(cnt):
        c1 = c
        while c1 < len(cnt) and cnt[c1] == cnt[c]:
            c1 += 1
        k = int(cnt[c])
        blocks.append(cn[start:start + k * (c1 - c)].reshape(c1 - c, k))
        start += k * (c1 - c)
        c = c1
    return meshgen._assemble_raw(pos, blocks, nt, {"bc": dict(raw["bc"]), "case_name": raw["case_name"] + "_perm"})


def _same_size_pool():
    from gfv import meshgen
    from gfv.pool import DevicePool
    raws = [meshgen.raw_quad_cavity(n=7, jitter=0.1, tri_fraction=0.3, seed=s) for s in (13, 14, 15)]
    raws.append(_permuted(raws[0], seed=3))
    ms = [meshgen.finish_mesh(r, U=1.0) for r in raws]
    return DevicePool(ms, [meshgen.random_fields(m, seed=20 + i) for i, m in enumerate(ms)])


def test_same_sizes_other_geometry_and_other_connectivity():
    """Three jittered cavities of one size signature (other positions and moments) and a fourth with the nodes of the first
    renumbered (same signature, DIFFERENT index tables): steps alternating over them replay one list and match eager bit for
    bit - no host-side decision of the step depends on what the tables hold."""
    pool = _same_size_pool()
    arena = pool.arena(1)
    sigs = {arena.signature([i]) for i in range(4)}
    assert len(sigs) == 1 and next(iter(sigs))[0][:4] == (64, 126, 63, 224)
    assert not torch.equal(pool.plans[0].es, pool.plans[3].es) and not torch.equal(pool.plans[0].pos, pool.plans[1].pos)
    seq = [[k % 4] for k in range(12)]
    ref_losses, ref_ts, _ = _reference_run(_same_size_pool(), seq)
    losses, ts, _ = _pool_run(pool, seq, max_graphs=1, use_graph="list")
    assert losses == ref_losses and torch.equal(ts.flat_p, ref_ts.flat_p)
    assert ts.stats()["lists"] == 1 and ts.stats()["replayed"] == 9


# 5 ---------------------------------------------------------------------------------------------------------------------
def _three_size_pool():
    from gfv import meshgen
    from gfv.pool import DevicePool
    raws = [meshgen.raw_tri_channel_cylinder(nx=30, ny=6, seed=21), meshgen.raw_tri_channel_cylinder(nx=30, ny=6, seed=22),
            meshgen.raw_quad_cavity(n=7, jitter=0.1, tri_fraction=0.3, seed=13)]
    ms = [meshgen.finish_mesh(r, U=U) for r, U in zip(raws, (0.15, 0.2, 1.0))]
    return DevicePool(ms, [meshgen.random_fields(m, seed=30 + i) for i, m in enumerate(ms)])


def _alternating_sequence():
    # A, B, A, B, A, A, B, B, C, A twice over with single meshes, then the same with pairs (B = 2; [0, 1] and [1, 0] are different
    # ORDERED signatures of the same total size)
    single = dict(A=[0], B=[1], C=[2])
    pair = dict(A=[0, 1], B=[1, 0], C=[2, 2])
    letters = "ABABAABBCA" * 2
    return [single[c] for c in letters] + [pair[c] for c in letters]


def test_alternating_signatures_keep_one_list_each():
    pool = _three_size_pool()
    assert pool.sizes[0]["e"] == 574 and pool.sizes[1]["e"] == 573
    seq = _alternating_sequence()
    from gfv.pool import batch_signature
    distinct = len({batch_signature(pool.sizes, i) for i in seq})
    assert distinct == 6
    ref_losses, ref_ts, _ = _reference_run(_three_size_pool(), seq)
    from gfv.pool_trainer import PoolTrainStep
    ts = PoolTrainStep(_model(), pool, max_graphs=2, lr=LR, use_graph="list")
    losses = []
    for idx in seq:
        losses.append(float(ts.step(idx)))
        assert ts.stats()["lists"] <= distinct
    assert losses == ref_losses and torch.equal(ts.flat_p, ref_ts.flat_p)
    assert ts.stats()["replayed"] > 0
    # a byte budget below one list's size: everything runs eager
    losses0, ts0, _ = _pool_run(_three_size_pool(), seq, max_graphs=2, use_graph="list", max_list_bytes=1)
    assert losses0 == ref_losses and torch.equal(ts0.flat_p, ref_ts.flat_p)
    assert ts0.stats()["lists"] == 0 and ts0.stats()["replayed"] == 0
    losses00, ts00, _ = _pool_run(_three_size_pool(), seq[:12], max_graphs=2, use_graph="list", max_list_bytes=0)
    assert losses00 == ref_losses[:12] and ts00.stats()["eager"] == 12 and ts00.stats()["recorded"] == 0


def test_a_byte_budget_for_one_list_does_not_record_on_every_visit():
    """Two signatures alternate and the budget holds one list: least recently used goes out, and a key that lost its list twice
    stays eager instead of recording again on every visit - the other keeps its list and replays.  Results as eager throughout."""
    seq = [[0], [1]] * 10
    ref_losses, ref_ts, _ = _reference_run(_three_size_pool(), seq)
    probe_losses, probe, _ = _pool_run(_three_size_pool(), seq[:6], max_graphs=1, use_graph="list")
    one, two = sorted(e.bytes for e in probe._lists.values())
    losses, ts, _ = _pool_run(_three_size_pool(), seq, max_graphs=1, use_graph="list", max_list_bytes=two + one // 2)
    assert losses == ref_losses and torch.equal(ts.flat_p, ref_ts.flat_p)
    st = ts.stats()
    assert st["lists"] == 1 and st["list_bytes"] <= two + one // 2 and st["recorded"] <= 5 and st["replayed"] >= 5, st


# 6 ---------------------------------------------------------------------------------------------------------------------
def test_payback_and_advance_in_the_arena():
    from gfv.pool import DevicePool
    from gfv.pool_trainer import PoolTrainStep
    from gfv.trainer import TrainStep
    ms, fs = _meshes()
    idx = [2, 0, 2]                          # entry 2 twice: the later occurrence is the one that stays
    pool, ref_pool = DevicePool(ms, fs), DevicePool(ms, fs)
    before = [x.clone() for x in pool.x]
    room = {k: 3 * max(s[k] for s in pool.sizes) for k in ("n", "e", "c", "k", "s", "nchunk")}
    ts = PoolTrainStep(_model(), pool, max_graphs=3, max_sizes=room, lr=LR)
    loss = float(ts.step(idx, payback=True))
    g, _ = ref_pool.batch(idx)
    ref = TrainStep(_model(), g, lr=LR, use_graph=False)
    assert float(ref.step()) == loss
    ref_pool.payback(idx, ref.uvp_node)
    torch.cuda.synchronize()
    for i in range(4):
        assert torch.equal(pool.x[i], ref_pool.x[i]), i
        assert torch.equal(pool.x[i][:, 3:], before[i][:, 3:])
    assert torch.equal(pool.x[1], before[1]) and torch.equal(pool.x[3], before[3])
    n2, n0 = pool.x[2].shape[0], pool.x[0].shape[0]
    assert torch.equal(pool.x[2][:, 0:3], ts.uvp_node[n2 + n0:]) and not torch.equal(pool.x[2][:, 0:3], ts.uvp_node[:n2])
    # the advance-in-arena form: the next inner step of the same batch starts from the prediction (TrainStep.advance_time)
    loss = float(ts.step(idx, advance=True))
    ref.set_batch(ref_pool.batch(idx)[0])    # (the pool entries changed: the paid-back state is what the next batch holds)
    assert float(ref.step()) == loss
    ref.advance_time()
    torch.cuda.synchronize()
    assert torch.equal(ts.x_backup, ref.x_backup)
    with pytest.raises(ValueError):
        ts.arena.payback(idx, ts.uvp_node[:-1].contiguous())


# 7 ---------------------------------------------------------------------------------------------------------------------
def test_reset_env_reaches_a_replayed_step():
    seq = [[k % 6] for k in range(8)]

    def between(k, pool):
        if k == 5:
            pool.reset_env(1, U=0.31, mu=2e-3, dt=0.02)
    seq[5] = seq[7] = [1]
    ref_losses, ref_ts, _ = _reference_run(_cyl_pool_with_variants(), seq, between=between)
    from gfv.pool_trainer import PoolTrainStep
    pool = _cyl_pool_with_variants()
    ts = PoolTrainStep(_model(), pool, max_graphs=1, lr=LR, use_graph="list")
    losses = []
    for k, idx in enumerate(seq):
        if k == 5:
            assert ts.stats()["recorded"] == 1 and ts.stats()["replayed"] == 2
            between(k, pool)
        losses.append(float(ts.step(idx)))
    assert losses == ref_losses and torch.equal(ts.flat_p, ref_ts.flat_p)
    assert ts.stats()["recorded"] == 1 and ts.stats()["replayed"] == 5
    unchanged, _, _ = _reference_run(_cyl_pool_with_variants(), seq)
    assert unchanged[5] != ref_losses[5]     # the new boundary condition did change the step


# 8 ---------------------------------------------------------------------------------------------------------------------
def test_variants_share_topology_and_own_their_boundary_condition():
    from gfv import meshgen
    from gfv.graph import build_batch
    from gfv.plan import build_plan
    from gfv.pool import DevicePool, _VARIANT_OWNED
    raw = meshgen.raw_tri_channel_cylinder(nx=30, ny=6, quad_fraction=0.0, seed=21)
    m = meshgen.finish_mesh(raw, U=0.15)
    pool = DevicePool([m])
    new = dict(U=0.31, mu=2.0e-3, source=0.05, aoa=3.0, dt=0.02)
    v = pool.add_variant(0, **new)
    assert v == 1 and pool.n == 2
    graphs, plan = pool.arena(2).load([0, v])
    raw_v = dict(raw)
    raw_v["bc"] = dict(raw["bc"], **new)
    ref_graphs = build_batch([m, meshgen.finish_mesh(raw_v)], device="cuda")
    ref = build_plan(*ref_graphs)
    torch.cuda.synchronize()
    assert float(ref.theta[0, 6]) != float(ref.theta[1, 6])
    for k, t in vars(ref).items():
        if torch.is_tensor(t) and k != "y":
            assert torch.equal(getattr(plan, k), t), k
    assert torch.equal(graphs[0].x[:, 3:12], ref_graphs[0].x[:, 3:12])
    n0 = m["node|pos"].shape[0]
    assert torch.equal(graphs[0].x[:n0], ref_graphs[0].x[:n0]) and torch.equal(plan.y[:n0], ref.y[:n0])
    for mine, want in ((graphs[0].x[:, 0:3], ref_graphs[0].x[:, 0:3]), (plan.y, ref.y)):
        assert float((mine - want).abs().max()) <= 2e-7 * float(want.abs().max())
    # shared structure, own boundary condition
    shared = 0
    for k, t in vars(pool.plans[0]).items():
        if torch.is_tensor(t):
            same = getattr(pool.plans[v], k).data_ptr() == t.data_ptr()
            assert same == (k not in _VARIANT_OWNED), k
            shared += same
    assert shared >= 35 and pool.x[v].data_ptr() != pool.x[0].data_ptr()

    def owned(i):
        return [getattr(pool.plans[i], k).clone() for k in _VARIANT_OWNED] + [pool.x[i].clone()]
    keep_v, keep_0 = owned(v), owned(0)
    pool.reset_env(0, U=0.2, mu=5e-3, dt=0.05)
    assert all(torch.equal(a, b) for a, b in zip(owned(v), keep_v)) and pool.bc[v]["U"] == 0.31
    assert not torch.equal(pool.plans[0].theta, keep_0[1])
    keep_0 = owned(0)
    pool.reset_env(v, U=0.11, mu=1e-3, dt=0.01)
    assert all(torch.equal(a, b) for a, b in zip(owned(0), keep_0)) and pool.bc[0]["U"] == 0.2
    assert not torch.equal(pool.plans[v].theta, keep_v[1])


# 9 ---------------------------------------------------------------------------------------------------------------------
def test_a_list_is_never_replayed_against_moved_scratch():
    """A piece of the owned scratch re-allocated behind the object's back: the next step finds the recorded pointers stale,
    drops the list and runs eager (correct results); nothing stale is issued.  (The piece replaced is the input preparation's
    workspace: zero between launches, like a fresh one.  The weight-gradient workspaces are not interchangeable with fresh ones
    bit for bit - the padding slots of the flat gradient take what they held.)"""
    seq = [[k % 6] for k in range(10)]
    ref_losses, ref_ts, _ = _reference_run(_cyl_pool_with_variants(), seq)
    from gfv.pool_trainer import PoolTrainStep
    ts = PoolTrainStep(_model(), _cyl_pool_with_variants(), max_graphs=1, lr=LR, use_graph="list")
    losses = []
    for k, idx in enumerate(seq):
        if k == 5:
            assert ts.stats() == dict(ts.stats(), replayed=2, recorded=1, eager=2, lists=1)
            ts._scratch["_prep_ws"] = torch.zeros_like(ts._scratch["_prep_ws"])
        losses.append(float(ts.step(idx)))
        if k == 5:
            assert ts.stats() == dict(ts.stats(), replayed=2, recorded=1, eager=3, lists=0)
    assert losses == ref_losses and torch.equal(ts.flat_p, ref_ts.flat_p)
    # steps 5, 6 eager (the dropped key warms up again), 7 records against the new workspace, 8 and 9 replay
    assert ts.stats() == dict(ts.stats(), replayed=4, recorded=2, eager=4, lists=1)


# 10 --------------------------------------------------------------------------------------------------------------------
def test_normalizer_flip_uses_a_list_per_accumulate_value():
    """dataset_size = 6: the Normalizer accumulates during the first six steps and not after; the key carries `accumulate`, so the
    two phases use different lists, and losses, parameters and the Normalizer's buffers equal the eager path's."""
    seq = [[k % 6] for k in range(10)]
    ref_losses, ref_ts, ref_model = _reference_run(_cyl_pool_with_variants(), seq, dataset_size=6)
    losses, ts, model = _pool_run(_cyl_pool_with_variants(), seq, dataset_size=6, max_graphs=1, use_graph="list")
    assert losses == ref_losses and torch.equal(ts.flat_p, ref_ts.flat_p)
    for name in ("acc_count", "num_accumulations", "acc_sum", "acc_sum_squared"):
        assert torch.equal(getattr(model.node_norm, name), getattr(ref_model.node_norm, name)), name
    assert float(model.node_norm.num_accumulations) == 6.0
    st = ts.stats()
    assert st["lists"] == 2 and st["recorded"] == 2 and st["replayed"] == 4 and st["eager"] == 4, st
    assert sorted(k[1] for k in ts._lists) == [False, True]


def test_unsupported_modes_are_refused():
    from gfv.pool_trainer import PoolTrainStep
    pool = _cyl_pool_with_variants()
    with pytest.raises(ValueError):
        PoolTrainStep(_model(), pool, max_graphs=1, use_graph=True)
