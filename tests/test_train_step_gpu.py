"""The one step skeleton of `TrainStep`, `PoolTrainStep` and `MarchStep` (gfv/trainer.py: `_step_head`, `_issue`, `_step_tail`) on the
smallest golden batch, `cyl_cavity_b2`.  Every comparison is bit for bit against an eager (`use_graph=False`) twin built from the
same seed and taken through the same sequence: an eager object reads every value at every launch and records nothing.

1. list mode: warm-up, recording, replay; a list whose engine signature moved is never issued and never kept;
2. a replay re-points `losses` / `uvp_node` / `uvp_cell` at the replayed list's own outputs, and `advance_time()` reads those;
3. `MarchStep`: the march record is the hold record of the optimiser's launches AND of the log, in eager, recorded and replayed steps.

The model's Normalizer has finished accumulating (dataset_size 1; the count starts at 1): every step has the key (False, False)."""
import numpy as np
import pytest
import torch

from test_march_gpu import _bits, _cpu_graphs, _model

pytestmark = pytest.mark.gpu

LR = 5e-5
STEADY = (False, False)


def _graphs():
    return tuple(g.clone().to("cuda") for g in _cpu_graphs("cyl_cavity_b2"))


def _pair(**kw):
    """A list-mode TrainStep and its eager twin."""
    from gfv.trainer import TrainStep
    ts = TrainStep(_model(), _graphs(), lr=LR, use_graph="list", **kw)
    twin = TrainStep(_model(), _graphs(), lr=LR, use_graph=False, **kw)
    assert ts.stats() == twin.stats() == dict(replayed=0, recorded=0, eager=0, lists=0, list_bytes=0) and not ts._lists.warm
    return ts, twin


def _kept(ts):
    """What a step moves for good: parameters and both moments by name (the alignment padding of the flat buffers is not state) and
    the step count."""
    return torch.cat([_bits(t).reshape(-1) for pmv in ts.named_state().values() for t in pmv] + [_bits(ts.adam_state[0:1])])


def _named(ts):
    """... and the step's own loss and residual terms."""
    return torch.cat([_kept(ts), _bits(ts.loss.reshape(-1)), _bits(ts.losses.reshape(-1))])


def _step_both(ts, twin, what):
    ts.step()
    twin.step()
    assert torch.equal(_named(ts), _named(twin)), what
    # once a step has returned no list recorded against another weight-image set or product form is left
    sig = ts.engine.capture_signature()
    assert all(e.engine_sig == sig for e in ts._lists.values()), what


def _took(ts, before):
    """Which launch path the step since `before` (a stats() dict) took."""
    now = ts.stats()
    moved = [k for k in ("eager", "recorded", "replayed") if now[k] != before[k]]
    assert len(moved) == 1 and now[moved[0]] == before[moved[0]] + 1, (before, now)
    return moved[0]


# ---- 1 ----------------------------------------------------------------------------------------------------------------------------
def test_a_list_whose_engine_signature_moved_is_dropped_and_recorded_again_behind_a_new_warm_up():
    from gfv import lib as L
    lib = L.load()
    ts, twin = _pair()
    took = []
    try:
        for k in range(4):
            before = ts.stats()
            _step_both(ts, twin, f"form 1, step {k}")
            took.append(_took(ts, before))
        assert took == ["eager", "eager", "recorded", "replayed"]
        assert list(ts._lists) == [STEADY]
        assert ts.stats() == dict(eager=2, recorded=1, replayed=1, lists=1, list_bytes=ts._lists[STEADY].bytes)
        first = ts._lists[STEADY]
        assert len(first.cl) > 100 and first.early is False and first.engine_sig == ts.engine.capture_signature()
        lib.gfv_set_f16split(2)                              # one fp16 x fp16 product per term: other launches, other images
        assert first.engine_sig != ts.engine.capture_signature()
        took = []
        for k in range(3):
            before = ts.stats()
            _step_both(ts, twin, f"form 2, step {k}")
            took.append(_took(ts, before))
            if k == 0:
                assert STEADY not in ts._lists and ts._lists.warm[STEADY] == 1     # the step that found it stale: warm-up 1
        assert took == ["eager", "eager", "recorded"]
        second = ts._lists[STEADY]
        assert second is not first and second.cl is not first.cl and ts.stats()["lists"] == 1
        before = ts.stats()
        _step_both(ts, twin, "form 2, the replay")
        assert _took(ts, before) == "replayed" and ts._lists[STEADY] is second
    finally:
        lib.gfv_set_f16split(1)
    # and the twin never recorded a thing
    assert twin.stats() == dict(replayed=0, recorded=0, eager=8, lists=0, list_bytes=0)


# ---- 2 ----------------------------------------------------------------------------------------------------------------------------
def test_a_replay_re_points_the_outputs_and_advance_time_reads_them():
    ts, twin = _pair()
    for k in range(3):
        _step_both(ts, twin, f"step {k}")
    ent = ts._lists[STEADY]
    assert ts.stats()["recorded"] == 1 and ts.stats()["replayed"] == 0
    assert ts.losses is ent.outs[0] and ts.uvp_node is ent.outs[1] and ts.uvp_cell is ent.outs[2]      # (the recording's own)
    # whatever the attributes name in between - here nothing - the replayed step's outputs are the replayed list's
    ts.losses = ts.uvp_node = ts.uvp_cell = None
    _step_both(ts, twin, "the replay")
    assert ts.stats()["replayed"] == 1 and ts._lists[STEADY] is ent
    assert ts.losses is ent.outs[0] and ts.uvp_node is ent.outs[1] and ts.uvp_cell is ent.outs[2]
    assert torch.equal(_bits(ts.uvp_node), _bits(twin.uvp_node)) and torch.equal(_bits(ts.uvp_cell), _bits(twin.uvp_cell))
    for t in (ts, twin):
        t.advance_time()
    assert torch.equal(_bits(ts.x_backup), _bits(twin.x_backup)) and torch.equal(_bits(ts.x), _bits(twin.x))
    assert torch.equal(_bits(ts.x_backup[:, 0:3]), _bits(twin.uvp_node))
    _step_both(ts, twin, "the step of the next time level")
    assert ts.stats()["replayed"] == 2 and ts.stats()["recorded"] == 1


# ---- 3 ----------------------------------------------------------------------------------------------------------------------------
def test_the_march_record_is_the_hold_record_of_the_optimiser_and_of_the_log():
    """max_inner = 2 and no tolerance: two levels are four applied steps - two warm-ups, the recording, a replay - and the two
    steps behind them are held and replayed.  `apply` is 1, 1, 1, 1, 0, 0 in the log (its reader of the record) and the
    parameters stop moving (the guard's and Adam's), as in the eager twin."""
    from gfv.march import MarchStep
    out = {}
    for mode in (False, "list"):
        ms = MarchStep(_model(), _graphs(), lr=LR, use_graph=mode, max_inner=2, tol=None, max_levels=4, log=16, max_grad_norm=1e-3)
        assert ms._hold_record() is ms._march and ms._accum is None
        rows = ms.run(levels=2, max_ahead=0)
        assert [(r["inner"], r["capped"]) for r in rows] == [(2, True), (2, True)]
        applied = _kept(ms)
        for _ in range(2):
            ms.step()
        torch.cuda.synchronize()
        assert torch.equal(_kept(ms), applied)                                 # (a held step moves its own loss and terms, no more)
        st, log = ms.stats(), ms.log.read()
        assert (st["seen"], st["held"], st["level"], st["apply"]) == (4, 2, 2, 0)
        assert ms.guard_stats()["clipped"] == 4 and float(ms.adam_state[0]) == 4.0
        if mode == "list":
            assert ms._lists.stats() == dict(replayed=3, recorded=1, eager=2, lists=1, list_bytes=ms._lists[STEADY].bytes)
        out[mode] = (_named(ms), log)
    for mode in out:
        assert out[mode][1].apply.tolist() == [1, 1, 1, 1, 0, 0] and out[mode][1].applied.tolist() == [1, 1, 1, 1, 0, 0]
    assert torch.equal(out[False][0], out["list"][0])
    a, b = out[False][1], out["list"][1]
    assert np.array_equal(a.apply, b.apply) and np.array_equal(a.adam_t, b.adam_t)
    assert np.array_equal(a.loss.view(np.int32), b.loss.view(np.int32))
    assert np.array_equal(a.grad_sumsq.view(np.int64), b.grad_sumsq.view(np.int64))
