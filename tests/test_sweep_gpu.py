"""GPU: `gfv.sweep.Sweep` (continuous batching of a parameter sweep over a device pool) and `gfv_sweep_advance` (csrc/sweep.hip).

The reference everywhere is the plain `gfv.rollout.Rollout` over `pool.batch(idx)`: its `x_backup[:, 0:3]` after every step and its
history.  Bit identity wherever the same launches run on the same values; `TOL = 1e-5` relative (tests/test_model_gpu.py) only
where the batch composition differs.  Tolerances of the latch tests are taken from the reference's own table of relative updates
(the midpoint between two adjacent distinct values), never from the code under test.

1. no swap, no latch: entries <= slots, both launch modes;
2. per-slot latch and freeze, run-ahead (`max_ahead`) changes nothing, queued steps behind a finished batch change nothing;
3. `patience` and `min_steps`;
4. continuous batching on one signature: one list, two swaps; with a latching tolerance against solo runs;
5. mixed topologies; a zero byte budget runs all-eager with the bits of list mode;
6. a narrow model (hidden 64: padded parameters);
7. a parameter change between two runs is refused until `refresh_weights()`.
"""
import numpy as np
import pytest
import torch

import cases
from oracle import fvgn_oracle as O
from test_pool_train_gpu import _cyl_pool_with_variants, _meshes

pytestmark = pytest.mark.gpu
TOL = 1e-5          # tests/test_model_gpu.py
K = 6


def rel_err(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return float((a - b).abs().max() / (b.abs().max() + 1e-30))


def _model(hidden=128):
    from FVMmodel.importer import NNmodel
    from gfv.params import default_params
    if hidden == 128:
        P, m = O.init_parameters(cases.WEIGHT_SEED), NNmodel(default_params(dataset_size=1))
    else:
        P = O.init_parameters(cases.WEIGHT_SEED, {"hidden_size": hidden})
        m = NNmodel(default_params(dataset_size=1, hidden_size=hidden))
    sd = m.state_dict()
    for k, v in P.items():
        sd[k].copy_(v)
    m.load_state_dict(sd)
    return m.cuda()


def _mesh_pool():
    from gfv.pool import DevicePool
    ms, fs = _meshes()
    return DevicePool(ms, fs)


_POOLS = {"cyl": _cyl_pool_with_variants, "mesh": _mesh_pool}
_REF = {}


def _reference(kind, idx, hidden=128):
    """The plain Rollout over pool.batch(idx) of a pool nothing has been written into, K steps -> (x_backup[:, 0:3] after every
    step, history [K, B, 6], node offsets of the graphs).  Computed once per (pool, batch, width) and left unchanged."""
    from gfv.rollout import Rollout
    key = (kind, tuple(idx), hidden)
    if key not in _REF:
        if ("pool", kind) not in _REF:
            _REF[("pool", kind)] = _POOLS[kind]()
        if ("model", hidden) not in _REF:
            _REF[("model", hidden)] = _model(hidden)
        pool = _REF[("pool", kind)]
        g, _ = pool.batch(idx)
        r = Rollout(_REF[("model", hidden)], g, max_steps=K, launch_mode="eager")
        states = []
        for _ in range(K):
            r.step()
            states.append(r.x_backup[:, 0:3].clone())
        offs = np.concatenate(([0], np.cumsum([pool.sizes[i]["n"] for i in idx])))
        _REF[key] = (states, r.history.cpu().clone(), offs)
    return _REF[key]


def _rel_table(hist):
    return hist[:, :, 4] / hist[:, :, 5]        # fp32 quotient of the two fp32 norms, as Rollout.run forms it


def _expect(col, tol, max_steps, min_steps=1, patience=1):
    """(steps, converged) of one graph from its column of the reference's table, by the rule of include/gfv.h."""
    streak = 0
    for k in range(max_steps):
        age = k + 1
        streak = streak + 1 if float(col[k]) < tol else 0
        if streak >= patience and age >= min_steps:
            return age, True
        if age >= max_steps:
            return age, False
    raise AssertionError


def _choose_tol(table, **kw):
    """The midpoint between two adjacent distinct values of the table at which graphs latch at different steps (two of them
    converged where the table allows it) -> (tol, [(steps, converged) per graph])."""
    vals = sorted({float(v) for v in table.flatten() if np.isfinite(float(v))})
    fallback = None
    for a, b in zip(vals, vals[1:]):
        tol = float(np.float32((a + b) / 2))
        if not a < tol < b:
            continue
        exp = [_expect(table[:, g], tol, table.shape[0], **kw) for g in range(table.shape[1])]
        conv = {s for s, c in exp if c}
        if len(conv) >= 2:
            return tol, exp
        if fallback is None and conv and len({s for s, _ in exp}) >= 2:
            fallback = (tol, exp)
    assert fallback is not None, ("no tolerance separates the graphs of this table", table)
    return fallback


def _fields(pool, idx):
    torch.cuda.synchronize()
    return [pool.x[i][:, 0:3].clone() for i in idx]


def _check_against(kind, idx, pool, results, expect, hidden=128):
    """Entry idx[b] holds the reference's state after its `steps`-th step and reports that step's losses."""
    states, hist, offs = _reference(kind, idx, hidden)
    for b, (i, r, (steps, conv)) in enumerate(zip(idx, results, expect)):
        assert (r.entry, r.steps, r.converged) == (i, steps, conv), (b, r, steps, conv)
        want = states[steps - 1][offs[b]:offs[b + 1]]
        got = pool.x[i][:, 0:3]
        assert torch.equal(got, want), (kind, idx, b, rel_err(got, want))
        assert torch.equal(torch.tensor(r.losses, dtype=torch.float32), hist[steps - 1, b, 0:4]), (b, r.losses)
        assert r.rel_update == float(hist[steps - 1, b, 4]) / float(hist[steps - 1, b, 5])


# 1 ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["cmd_list", "eager"])
def test_no_swap_no_latch_equals_rollout(mode):
    from gfv.sweep import Sweep
    idx = [0, 1, 2]
    pool = _cyl_pool_with_variants()
    untouched = _fields(pool, [3, 4, 5])
    sw = Sweep(_model(), pool, max_graphs=4, tol=-1, max_steps=K, launch_mode=mode)
    res = sw.run(idx)
    _check_against("cyl", idx, pool, res, [(K, False)] * 3)
    for a, b in zip(untouched, _fields(pool, [3, 4, 5])):
        assert torch.equal(a, b)
    st = sw.stats()
    assert st["steps"] == K and st["swaps"] == 0, st
    if mode == "cmd_list":
        assert (st["eager"], st["recorded"], st["replayed"], st["lists"]) == (2, 1, 3, 1) and st["list_bytes"] > 0, st
    else:
        assert (st["eager"], st["recorded"], st["replayed"], st["lists"]) == (K, 0, 0, 0), st


# 2 ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("idx", [[0, 1], [0, 1, 2]])
def test_per_slot_latch_and_freeze(idx):
    from gfv.sweep import Sweep
    _, hist, _ = _reference("cyl", idx)
    table = _rel_table(hist)
    tol, expect = _choose_tol(table)
    print(f"batch {idx}: rel table\n{table}\ntol {tol:.6e} -> expected (steps, converged) {expect}")
    assert len({s for s, _ in expect}) >= 2
    runs = []
    for ahead in (0, 4):
        pool = _cyl_pool_with_variants()
        sw = Sweep(_model(), pool, max_graphs=len(idx), tol=tol, max_steps=K, max_ahead=ahead)
        res = sw.run(idx)
        _check_against("cyl", idx, pool, res, expect)
        runs.append((res, _fields(pool, idx), sw))
    assert runs[0][0] == runs[1][0]
    for a, b in zip(runs[0][1], runs[1][1]):
        assert torch.equal(a, b)
    # every slot is done: steps queued behind that change nothing
    sw = runs[1][2]
    torch.cuda.synchronize()
    state3, slots, last = sw._state3.clone(), sw._slots.clone(), sw._last.clone()
    for _ in range(3):
        sw._step(*sw._current)
    torch.cuda.synchronize()
    assert torch.equal(sw._state3, state3) and torch.equal(sw._slots, slots) and torch.equal(sw._last, last)
    n = sum(runs[1][1][b].shape[0] for b in range(len(idx)))
    assert torch.equal(state3[:n], torch.cat(runs[1][1]))


# 3 ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("patience,min_steps", [(2, 1), (1, 3), (2, 3)])
def test_patience_and_min_steps(patience, min_steps):
    from gfv.sweep import Sweep
    idx = [0, 1, 2]
    _, hist, _ = _reference("cyl", idx)
    table = _rel_table(hist)
    tol_mid, _ = _choose_tol(table)
    for tol in (tol_mid, 1e30):      # (1e30: every step is below it - the streak grows by one per step)
        expect = [_expect(table[:, g], tol, K, min_steps=min_steps, patience=patience) for g in range(len(idx))]
        print(f"patience {patience} min_steps {min_steps} tol {tol:.6e}: expected {expect}")
        pool = _cyl_pool_with_variants()
        sw = Sweep(_model(), pool, max_graphs=3, tol=tol, max_steps=K, min_steps=min_steps, patience=patience, max_ahead=0)
        _check_against("cyl", idx, pool, sw.run(idx), expect)
    assert expect == [(max(patience, min_steps), True)] * 3


# 4 ---------------------------------------------------------------------------------------------------------------------
def test_continuous_batching_on_one_signature():
    from gfv.sweep import Sweep
    pool = _cyl_pool_with_variants()
    sw = Sweep(_model(), pool, max_graphs=2, tol=-1, max_steps=5, max_ahead=0)
    res = sw.run()
    assert [r.entry for r in res] == list(range(6))
    for pair in ([0, 1], [2, 3], [4, 5]):
        _check_against("cyl", pair, pool, [res[i] for i in pair], [(5, False)] * 2)
    st = sw.stats()
    assert st["lists"] == 1 and st["recorded"] == 1 and st["swaps"] == 2 and st["steps"] == 15, st
    assert st["eager"] == 2 and st["replayed"] == 12, st


def test_continuous_batching_with_a_latching_tolerance():
    """The slots retire at different steps: every entry's (steps, converged) is what its SOLO Rollout's table predicts, and its
    field is its solo run's at TOL - its neighbours in the batch change from swap to swap.
    Finding (MI355X): against the SOLO run (a batch of one) no slot of the batch of two is bit-identical - the fields differ by
    8e-9 .. 4e-8 relative, the first slot (same row offsets as solo) included - so a forward kernel does depend on the batch it
    runs in (its row count: a size-dependent kernel form, or a scale taken over all rows).  Every slot is therefore held to TOL
    here; against a Rollout of the SAME batch composition the fields are bit-identical (tests 1 - 4 above)."""
    from gfv.sweep import Sweep
    solo = [_reference("cyl", [i]) for i in range(6)]
    table = torch.cat([_rel_table(h) for _, h, _ in solo], dim=1)       # [K, 6]
    tol, expect = _choose_tol(table)
    print(f"solo rel table\n{table}\ntol {tol:.6e} -> expected {expect}")
    assert len({s for s, _ in expect}) >= 2
    pool = _cyl_pool_with_variants()
    sw = Sweep(_model(), pool, max_graphs=2, tol=tol, max_steps=K, max_ahead=0)
    res = sw.run()
    print(sw.stats())
    assert sw.stats()["lists"] == 1
    for i, r in enumerate(res):
        assert (r.entry, r.steps, r.converged) == (i, *expect[i]), (r, expect[i])
        want = solo[i][0][r.steps - 1]
        e = rel_err(pool.x[i][:, 0:3], want)
        print(f"entry {i}: steps {r.steps} converged {r.converged} field rel {e:.2e} bitwise {bool(torch.equal(pool.x[i][:, 0:3], want))}")
        assert e < TOL, (i, e)


# 5 ---------------------------------------------------------------------------------------------------------------------
def test_mixed_topologies():
    from gfv.sweep import Sweep
    runs = {}
    for budget in (16 << 30, 0):
        pool = _mesh_pool()
        sw = Sweep(_model(), pool, max_graphs=2, tol=-1, max_steps=K, max_ahead=0, max_list_bytes=budget)
        res = sw.run()
        runs[budget] = (res, _fields(pool, range(4)), sw.stats())
    res, fields, st = runs[16 << 30]
    assert sorted(r.entry for r in res) == [0, 1, 2, 3] and [r.entry for r in res] == [0, 1, 2, 3]
    assert all((r.steps, r.converged) == (K, False) for r in res)
    for i in range(4):
        states, hist, _ = _reference("mesh", [i])
        e = rel_err(fields[i], states[K - 1])
        print(f"mesh {i}: field against the solo Rollout rel {e:.2e}")
        assert e < TOL, (i, e)
        assert rel_err(torch.tensor(res[i].losses), hist[K - 1, 0, 0:4]) < TOL
    assert st["lists"] >= 2 and st["swaps"] == 1, st
    res0, fields0, st0 = runs[0]
    assert res0 == res and all(torch.equal(a, b) for a, b in zip(fields0, fields))
    assert st0["eager"] == st0["steps"] == st["steps"] and st0["recorded"] == 0 and st0["lists"] == 0, st0


# 6 ---------------------------------------------------------------------------------------------------------------------
def test_narrow_model():
    from gfv import lib as L
    from gfv.sweep import Sweep
    idx = [0, 1, 2]
    pool = _cyl_pool_with_variants()
    sw = Sweep(_model(64), pool, max_graphs=4, tol=-1, max_steps=K)
    res = sw.run(idx)
    assert L.load().gfv_hidden_size() == 128
    _check_against("cyl", idx, pool, res, [(K, False)] * 3, hidden=64)
    st = sw.stats()
    assert (st["eager"], st["recorded"], st["replayed"]) == (2, 1, 3), st


# 7 ---------------------------------------------------------------------------------------------------------------------
def test_refresh_weights_is_required_after_a_parameter_change():
    from gfv.sweep import Sweep
    model = _model()
    pool = _cyl_pool_with_variants()
    sw = Sweep(model, pool, max_graphs=2, tol=-1, max_steps=4)
    first = sw.run([0, 1])
    P2 = O.init_parameters(cases.WEIGHT_SEED + 1)
    sd = model.state_dict()
    for k, v in P2.items():
        sd[k].copy_(v)
    model.load_state_dict(sd)
    with pytest.raises(RuntimeError, match="refresh_weights"):
        sw.run([2, 3])
    sw.refresh_weights()
    res = sw.run([2, 3])
    other_pool = _cyl_pool_with_variants()
    fresh = Sweep(model, other_pool, max_graphs=2, tol=-1, max_steps=4, launch_mode="eager")
    want = fresh.run([2, 3])
    assert res == want and res[0].losses != first[0].losses
    for a, b in zip(_fields(pool, [2, 3]), _fields(other_pool, [2, 3])):
        assert torch.equal(a, b)
