"""GPU: `gfv.evaluate.Evaluate` (held-out losses and field errors over a device pool) and `gfv_eval_collect` (csrc/eval.hip).

The reference for losses is the plain `gfv.rollout.Rollout(model, pool.batch(idx)[0], launch_mode="eager").step()` over the same
batch composition - never `Evaluate` itself: bit identity wherever the same launches run on the same values, `TOL = 1e-5`
(tests/test_model_gpu.py) only where the composition differs.  Every norm is checked against numpy - difference in fp32, sum of
squares in float64, square root, rounded to fp32 - and may differ from it by at most one fp32 spacing: the two sides differ only in
the order of a double sum, which can move the fp32 rounding by one step and no more.

1. one batch, both launch modes; the pool is not written;
2. one signature, three batches: two warm-ups, one list, replays across `run()` calls; row i of the table is entry i;
3. a short last batch; a batch that does not fit is refused before anything is launched; a graph of more than 64 chunks;
4. targets: against numpy, exactly 0 for the prediction as its own target, NaN without one;
5. the weights move: refused until `refresh_weights()`, which rebuilds in place and keeps the lists;
6. a narrow model (hidden 64: padded parameters, refreshed with `copy_`);
7. training is untouched by an evaluation in between; the averaged weights through `ema_weights()`.
"""
import numpy as np
import pytest
import torch

import cases
from oracle import fvgn_oracle as O
from test_pool_train_gpu import LR, _cyl_pool_with_variants, _meshes
from test_sweep_gpu import _model

pytestmark = pytest.mark.gpu
TOL = 1e-5          # tests/test_model_gpu.py

_CACHE = {}


def _shared_model(hidden=128):
    """A model no test writes into (tests that change parameters build their own)."""
    if ("model", hidden) not in _CACHE:
        _CACHE[("model", hidden)] = _model(hidden)
    return _CACHE[("model", hidden)]


def _mesh_pool():
    from gfv.pool import DevicePool
    if "meshes" not in _CACHE:
        _CACHE["meshes"] = _meshes()
    ms, fs = _CACHE["meshes"]
    return DevicePool(ms, fs)


def _big_pool():
    """One cavity of more than 64 x 64 nodes: more chunks in one graph than the folding wave has lanes."""
    from gfv import meshgen
    from gfv.pool import DevicePool
    if "big" not in _CACHE:
        m = meshgen.finish_mesh(meshgen.raw_quad_cavity(n=66, jitter=0.1, tri_fraction=0.3, seed=17), U=1.0)
        _CACHE["big"] = (m, meshgen.random_fields(m, seed=9))
    m, f = _CACHE["big"]
    return DevicePool([m], [f])


_POOLS = {"cyl": _cyl_pool_with_variants, "mesh": _mesh_pool, "big": _big_pool}


def _reference(kind, idx, hidden=128):
    """One eager Rollout step over pool.batch(idx) of a pool nothing has been written into -> (losses [B,4], the prediction
    [N,3], the entries' own state [N,3], node offsets), on the host.  Computed once per (pool, batch, width), left unchanged."""
    from gfv.rollout import Rollout
    key = ("ref", kind, tuple(idx), hidden)
    if key not in _CACHE:
        if ("pool", kind) not in _CACHE:
            _CACHE[("pool", kind)] = _POOLS[kind]()
        pool = _CACHE[("pool", kind)]
        cur = torch.cat([pool.x[i][:, 0:3] for i in idx]).cpu().clone()
        losses, uvp_node, _ = Rollout(_shared_model(hidden), pool.batch(idx)[0], max_steps=1, launch_mode="eager").step()
        torch.cuda.synchronize()
        offs = np.concatenate(([0], np.cumsum([pool.sizes[i]["n"] for i in idx])))
        _CACHE[key] = (losses.cpu().clone(), uvp_node.cpu().clone(), cur, offs)
    return _CACHE[key]


def _bits(t):
    return t.detach().cpu().contiguous().view(torch.int32 if t.dtype == torch.float32 else torch.int64)


def _same_report(a, b):
    return (a.entries == b.entries and torch.equal(_bits(a.table), _bits(b.table)) and torch.equal(_bits(a.losses), _bits(b.losses))
            and torch.equal(_bits(a.loss_batch), _bits(b.loss_batch)) and torch.equal(_bits(a.rel_update), _bits(b.rel_update))
            and torch.equal(_bits(a.rel_error), _bits(b.rel_error))
            and np.float64(a.objective).tobytes() == np.float64(b.objective).tobytes() and a.nonfinite == b.nonfinite)


def _norm32(a, b=None):
    """|| a - b ||_2 per column as the kernel is specified: difference in fp32, squares and sum in float64, sqrt, fp32."""
    d = a if b is None else (a - b)
    assert d.dtype == np.float32
    return np.sqrt(np.sum(d.astype(np.float64) ** 2, axis=0)).astype(np.float32)


def _within_one_spacing(got, want, what):
    got, want = np.asarray(got, dtype=np.float32), np.asarray(want, dtype=np.float32)
    lo, hi = np.nextafter(want, np.float32(-np.inf)), np.nextafter(want, np.float32(np.inf))
    steps = (got.view(np.int32).astype(np.int64) - want.view(np.int32).astype(np.int64))
    print(f"{what}: got {got} want {want} fp32 steps apart {steps}")
    assert np.all((got == want) | (got == lo) | (got == hi)), (what, got, want)
    assert np.all(np.isfinite(got))


def _check_norms(rep, k, pred, cur, what):
    """Columns 4-9 of row k of the report's table against numpy over the graph's own nodes; rel_update is their float64 quotient."""
    row = rep.table[k].numpy()
    _within_one_spacing(row[4:7], _norm32(pred, cur), f"{what} ||pred - cur||")
    _within_one_spacing(row[7:10], _norm32(pred), f"{what} ||pred||")
    with np.errstate(divide="ignore", invalid="ignore"):      # (a channel the model predicts as exactly zero: inf, or NaN for 0 / 0)
        want = row[4:7].astype(np.float64) / row[7:10].astype(np.float64)
    assert np.array_equal(rep.rel_update[k].numpy(), want, equal_nan=True)


def _pool_bits(pool):
    torch.cuda.synchronize()
    return [x.detach().cpu().view(torch.int32).clone() for x in pool.x]


def _check_batches(rep, kind, batches, hidden=128):
    """Rows of the report, in order, against eager Rollouts of the same batches: losses bit for bit, norms against numpy."""
    k = 0
    for idx in batches:
        losses, pred, cur, offs = _reference(kind, idx, hidden)
        for b, i in enumerate(idx):
            assert rep.entries[k] == i
            assert torch.equal(_bits(rep.losses[k]), _bits(losses[b])), (kind, idx, b, rep.losses[k], losses[b])
            sl = slice(offs[b], offs[b + 1])
            _check_norms(rep, k, pred[sl].numpy(), cur[sl].numpy(), f"{kind} {idx} graph {b}")
            k += 1
    assert k == len(rep.entries)
    assert rep.nonfinite == 0 and np.isfinite(rep.objective)


# 1 ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["cmd_list", "eager"])
def test_one_batch_equals_rollout_and_leaves_the_pool_alone(mode):
    from gfv.evaluate import Evaluate
    idx = [2, 0, 3, 1]
    pool = _mesh_pool()
    before = _pool_bits(pool)
    ev = Evaluate(_shared_model(), pool, max_graphs=4, launch_mode=mode)
    reps = [ev.run(idx) for _ in range(4)]       # list mode: two warm-ups, the recording, one replay
    _check_batches(reps[0], "mesh", [idx])
    assert all(_same_report(reps[0], r) for r in reps[1:])
    assert all(torch.equal(a, b) for a, b in zip(before, _pool_bits(pool)))
    assert torch.isnan(reps[0].rel_error).all() and torch.isnan(reps[0].table[:, 10:16]).all()
    p = _shared_model().params
    want = [p.loss_press * float(r[3]) + p.loss_cont * float(r[0]) + p.loss_mom * (float(r[1]) + float(r[2])) for r in reps[0].losses]
    assert reps[0].loss_batch.tolist() == want
    st = ev.stats()
    assert set(st) == {"batches", "replayed", "recorded", "eager", "lists", "list_bytes"}
    if mode == "cmd_list":
        assert (st["batches"], st["eager"], st["recorded"], st["replayed"], st["lists"]) == (4, 2, 1, 1, 1) and st["list_bytes"] > 0, st
    else:
        assert (st["batches"], st["eager"], st["recorded"], st["replayed"], st["lists"]) == (4, 4, 0, 0, 0), st


# 2 ---------------------------------------------------------------------------------------------------------------------
def test_one_signature_three_batches_replays_across_runs():
    from gfv.evaluate import Evaluate
    idx = [4, 1, 5, 0, 3, 2]
    pool = _cyl_pool_with_variants()
    before = _pool_bits(pool)
    ev = Evaluate(_shared_model(), pool, max_graphs=2)
    first = ev.run(idx)
    st = ev.stats()
    assert (st["eager"], st["recorded"], st["replayed"], st["lists"]) == (2, 1, 0, 1), st
    second = ev.run(idx)
    st = ev.stats()
    assert (st["eager"], st["recorded"], st["replayed"], st["lists"]) == (2, 1, 3, 1), st
    eager = Evaluate(_shared_model(), pool, max_graphs=2, launch_mode="eager").run(idx)
    assert _same_report(first, second) and _same_report(first, eager)
    _check_batches(first, "cyl", [[4, 1], [5, 0], [3, 2]])
    # row i of the table belongs to entry i, whatever position of whatever batch it was evaluated in
    table = ev._table.cpu()
    for k, i in enumerate(idx):
        assert torch.equal(_bits(table[i]), _bits(first.table[k])), (k, i)
    assert all(torch.equal(a, b) for a, b in zip(before, _pool_bits(pool)))
    # a subset in another order: the batches differ, the signature - and with it the list - stays
    sub = ev.run([0, 5])
    assert ev.stats()["recorded"] == 1 and ev.stats()["replayed"] == 4
    _check_batches(sub, "cyl", [[0, 5]])


# 3 ---------------------------------------------------------------------------------------------------------------------
def test_short_last_batch():
    from gfv.evaluate import Evaluate
    from test_sweep_gpu import rel_err
    idx = [1, 3, 0]
    pool = _mesh_pool()
    rep = Evaluate(_shared_model(), pool, max_graphs=2).run(idx)
    _check_batches(rep, "mesh", [[1, 3], [0]])
    one = Evaluate(_shared_model(), pool, max_graphs=4).run(idx)
    _check_batches(one, "mesh", [idx])
    for k in range(3):                           # the composition differs: TOL, as tests/test_sweep_gpu.py holds such pairs
        e = rel_err(rep.losses[k], one.losses[k])
        print(f"entry {idx[k]}: losses {rep.losses[k].tolist()} against {one.losses[k].tolist()} rel {e:.2e}")
        assert e < TOL, (k, e)
    with pytest.raises(ValueError, match="more than once"):
        Evaluate(_shared_model(), pool, max_graphs=2).run([1, 3, 1])
    with pytest.raises(ValueError):
        Evaluate(_shared_model(), pool, max_graphs=2).run([])


def test_a_batch_that_does_not_fit_is_refused_before_anything_is_launched():
    from gfv.evaluate import Evaluate
    pool = _mesh_pool()
    small = pool.arena(1)                        # room for the largest single entry
    ev = Evaluate(_shared_model(), pool, max_graphs=2, arena=small)
    with pytest.raises(ValueError):
        ev.run([0, 1, 2])                        # ([0, 1]: two graphs in an arena of one)
    assert ev.stats()["batches"] == 0
    torch.cuda.synchronize()
    assert torch.isnan(ev._table).all()          # nothing was launched: the table is as it was created
    with pytest.raises(ValueError, match="another pool"):
        Evaluate(_shared_model(), _mesh_pool(), arena=small)


def test_a_graph_of_more_than_64_chunks():
    """The fold's second trip: lane l takes chunks l, l + 64, ... of a graph (SLICE_CHUNK = 64 nodes per chunk)."""
    from gfv import meshgen
    from gfv.evaluate import Evaluate
    pool = _big_pool()
    assert pool.plans[0].n_chunks > 64 and pool.sizes[0]["n"] % 64 != 0, (pool.plans[0].n_chunks, pool.sizes[0]["n"])
    losses, pred, cur, offs = _reference("big", [0])
    tgt = meshgen.random_fields(_CACHE["big"][0], seed=10)
    ev = Evaluate(_shared_model(), pool, max_graphs=1, launch_mode="eager")
    ev.set_target(0, tgt)
    rep = ev.run()
    _check_batches(rep, "big", [[0]])
    row = rep.table[0].numpy()
    _within_one_spacing(row[10:13], _norm32(pred.numpy(), tgt), "big ||pred - tgt||")
    _within_one_spacing(row[13:16], _norm32(tgt), "big ||tgt||")
    assert _same_report(rep, ev.run())


# 4 ---------------------------------------------------------------------------------------------------------------------
def test_targets():
    from gfv import meshgen
    from gfv.evaluate import Evaluate
    idx = [0, 1, 2, 3]
    pool = _mesh_pool()
    ms, _ = _CACHE["meshes"]
    losses, pred, cur, offs = _reference("mesh", idx)
    tgt1 = meshgen.random_fields(ms[1], seed=77)
    tgt2 = pred[offs[2]:offs[3]].numpy().copy()  # the Rollout's own prediction
    ev = Evaluate(_shared_model(), pool, max_graphs=4, launch_mode="eager")
    ev.set_target(1, tgt1)
    ev.set_target(2, torch.from_numpy(tgt2))
    with pytest.raises(ValueError):
        ev.set_target(0, tgt1)                   # another entry's node count
    rep = ev.run(idx)
    _check_batches(rep, "mesh", [idx])
    row = rep.table.numpy()
    p1 = pred[offs[1]:offs[2]].numpy()
    _within_one_spacing(row[1, 10:13], _norm32(p1, tgt1), "||pred - tgt|| entry 1")
    _within_one_spacing(row[1, 13:16], _norm32(tgt1), "||tgt|| entry 1")
    assert np.array_equal(rep.rel_error[1].numpy(), row[1, 10:13].astype(np.float64) / row[1, 13:16].astype(np.float64))
    assert bool((rep.rel_error[1] > 0).all())
    assert rep.rel_error[2].tolist() == [0.0, 0.0, 0.0]                    # exactly
    _within_one_spacing(row[2, 13:16], _norm32(tgt2), "||tgt|| entry 2")
    assert np.array_equal(row[2, 13:16].view(np.int32), row[2, 7:10].view(np.int32))      # the target IS the prediction
    assert torch.isnan(rep.rel_error[0]).all() and torch.isnan(rep.rel_error[3]).all()
    assert np.isnan(row[[0, 3], 10:16]).all()
    # the same through a list: the staging copies and the collect launch are issued behind the replay
    lst = Evaluate(_shared_model(), pool, max_graphs=4)
    lst.set_target(1, tgt1)
    lst.set_target(2, tgt2)
    again = [lst.run(idx) for _ in range(4)][-1]
    assert lst.stats()["replayed"] == 1 and _same_report(rep, again)
    ev.clear_targets()
    rep = ev.run(idx)
    assert torch.isnan(rep.rel_error).all() and torch.isnan(rep.table[:, 10:16]).all()
    assert torch.equal(_bits(rep.table[:, 0:10]), _bits(again.table[:, 0:10]))


# 5 ---------------------------------------------------------------------------------------------------------------------
def _scale_parameters(model, f):
    with torch.no_grad():
        for p in model.parameters():
            p.mul_(f)


def test_weights_move_refresh_in_place_keeps_the_lists():
    from gfv.evaluate import Evaluate
    model = _model()
    pool = _cyl_pool_with_variants()
    idx = [0, 1, 2, 3]
    ev = Evaluate(model, pool, max_graphs=2)
    old = [ev.run(idx) for _ in range(2)][-1]    # batches 1-2 eager, 3 recorded, 4 replayed
    st0 = ev.stats()
    assert (st0["eager"], st0["recorded"], st0["replayed"]) == (2, 1, 1), st0
    images = {k: v.data_ptr() for k, v in ev.engine._wi["fwd"].images.items()} if ev.engine._wi else {}
    _scale_parameters(model, 1.01)
    with pytest.raises(RuntimeError, match="refresh_weights"):
        ev.run(idx)
    ev.refresh_weights()
    rep = ev.run(idx)
    st1 = ev.stats()
    assert st1["recorded"] == st0["recorded"] and st1["replayed"] == st0["replayed"] + 2 and st1["eager"] == st0["eager"], st1
    fresh = Evaluate(model, _cyl_pool_with_variants(), max_graphs=2, launch_mode="eager").run(idx)
    assert _same_report(rep, fresh)
    assert not torch.equal(_bits(rep.losses), _bits(old.losses))            # (the new values were used: not the stale images)
    if ev.engine._wi:
        now = {k: v.data_ptr() for k, v in ev.engine._wi["fwd"].images.items()}
        assert now == images                                                # rebuilt where they were
    # ... and what is right for the new weights is what a Rollout of them says
    from gfv.rollout import Rollout
    ref_pool = _cyl_pool_with_variants()
    for pair, rows in (([0, 1], (0, 1)), ([2, 3], (2, 3))):
        losses, _, _ = Rollout(model, ref_pool.batch(pair)[0], max_steps=1, launch_mode="eager").step()
        for b, k in enumerate(rows):
            assert torch.equal(_bits(rep.losses[k]), _bits(losses[b].cpu()))


# 6 ---------------------------------------------------------------------------------------------------------------------
def test_narrow_model():
    from gfv import lib as L
    from gfv.evaluate import Evaluate
    idx = [0, 1, 2]
    pool = _cyl_pool_with_variants()
    rep = Evaluate(_shared_model(64), pool, max_graphs=4).run(idx)
    assert L.load().gfv_hidden_size() == 128
    _check_batches(rep, "cyl", [idx], hidden=64)
    # the padded copies are refreshed into the tensors that exist: the list stays
    model = _model(64)
    ev = Evaluate(model, pool, max_graphs=4)
    for _ in range(4):
        ev.run(idx)
    ptrs = {n: t.data_ptr() for n, t in ev.P.items()}
    assert any(ev.P[n].shape != t.shape for n, t in zip(*model.param_names_tensors()))     # (something IS padded)
    _scale_parameters(model, 1.01)
    with pytest.raises(RuntimeError, match="refresh_weights"):
        ev.run(idx)
    ev.refresh_weights()
    assert {n: t.data_ptr() for n, t in ev.P.items()} == ptrs
    got = ev.run(idx)
    st = ev.stats()
    assert (st["eager"], st["recorded"], st["replayed"]) == (2, 1, 2), st
    fresh = Evaluate(model, pool, max_graphs=4, launch_mode="eager").run(idx)
    assert _same_report(got, fresh) and not torch.equal(_bits(got.losses), _bits(rep.losses))
    assert L.load().gfv_hidden_size() == 128


# 7 ---------------------------------------------------------------------------------------------------------------------
SEQ = [[0, 1], [2, 3], [4, 5], [1, 0]]


def _flat_bits(pts):
    torch.cuda.synchronize()
    return [_bits(t).clone() for t in (pts.flat_p, pts.flat_m, pts.flat_v)]


def test_training_is_untouched_by_an_evaluation_in_between():
    from gfv.evaluate import Evaluate
    from gfv.pool_trainer import PoolTrainStep
    plain = PoolTrainStep(_model(), _cyl_pool_with_variants(), max_graphs=2, lr=LR)
    for idx in SEQ:
        plain.step(idx)
    want = _flat_bits(plain)
    model, pool = _model(), _cyl_pool_with_variants()
    pts = PoolTrainStep(model, pool, max_graphs=2, lr=LR)
    for idx in SEQ[:2]:
        pts.step(idx)
    ev = Evaluate(model, pool, max_graphs=2, arena=pts.arena)
    assert ev.arena is pts.arena
    before = _pool_bits(pool)
    rep = ev.run()
    assert rep.entries == list(range(6)) and rep.nonfinite == 0 and np.isfinite(rep.objective)
    assert all(torch.equal(a, b) for a, b in zip(before, _pool_bits(pool)))
    for idx in SEQ[2:]:
        pts.step(idx)
    got = _flat_bits(pts)
    assert all(torch.equal(a, b) for a, b in zip(want, got))
    ev.refresh_weights()                         # (the fused Adam writes through raw pointers: the caller's duty after training)
    again = ev.run()
    assert again.nonfinite == 0 and not torch.equal(_bits(again.losses), _bits(rep.losses))


def test_averaged_weights_through_the_swap():
    from FVMmodel.importer import NNmodel
    from gfv.evaluate import Evaluate
    from gfv.params import default_params
    from gfv.pool_trainer import PoolTrainStep
    model, pool = _model(), _cyl_pool_with_variants()
    pts = PoolTrainStep(model, pool, max_graphs=2, lr=LR, ema_decay=0.9)
    for idx in SEQ:
        pts.step(idx)
    torch.cuda.synchronize()
    held_out = [5, 2, 3]
    ev = Evaluate(model, pool, max_graphs=2, arena=pts.arena)
    it = ev.run(held_out)                        # the iterate
    names, tensors = model.param_names_tensors()
    iterate = [t.detach().cpu().clone() for t in tensors]
    avg = pts.ema_parameters()
    assert any(not torch.equal(avg[n], t) for n, t in zip(names, iterate))
    with pts.ema_weights():
        with pytest.raises(RuntimeError, match="refresh_weights"):
            ev.run(held_out)
        ev.refresh_weights()
        rep = ev.run(held_out)
    torch.cuda.synchronize()
    for t, want in zip(tensors, iterate):        # after the block the iterate is back
        assert torch.equal(t.detach().cpu(), want)
    with pytest.raises(RuntimeError, match="refresh_weights"):
        ev.run(held_out)
    # a second model loaded from the averaged parameters gives the same bits (same values -> same image bits)
    sd = {k: v.detach().cpu().clone() for k, v in model.state_dict().items()}
    for n in names:
        assert n in sd
        sd[n] = avg[n]
    other = NNmodel(default_params(dataset_size=1))
    other.load_state_dict(sd)
    other = other.cuda()
    want = Evaluate(other, _cyl_pool_with_variants(), max_graphs=2, launch_mode="eager").run(held_out)
    assert _same_report(rep, want)
    assert not torch.equal(_bits(rep.losses), _bits(it.losses))
    ev.refresh_weights()                         # ... and the iterate evaluates as before
    assert _same_report(ev.run(held_out), it)
    pts.step(SEQ[0])                             # training goes on
    assert pts.ema_stats()["updates"] == 5
