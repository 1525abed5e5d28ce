"""GPU: `Rollout`, `Evaluate` and `Sweep` taking turns on ONE model and engine (gfv/static_forward.py, gfv/listcache.py).

Each of the three goes through warm-up, recording and replay while the other two run batches of other sizes through the same
engine in between.  The reference of each is its twin: the same object built on a model and engine of its own (same weights) and
run ALONE through the same calls.  The same launches on the same values: everything is compared bit for bit, and no tolerance
appears.  The engine's own scratch of the input preparation and of the finite-volume tail is the same pair of tensors after every
call as before it - the three work on scratch of their own and put the engine's back.

Pool: the generated meshes of tests/test_sweep_gpu.py (four sizes), two slots.  Both widths: hidden 128, and hidden 64, where the
parameters a list points at are padded copies that `refresh_weights()` refreshes in place - one set per engine, or the three
would name three parameter sets to it and each would find the image set of another.
"""
import pytest
import torch

from test_evaluate_gpu import _mesh_pool       # (the pool of test_sweep_gpu.py, its meshes generated once)
from test_sweep_gpu import _fields, _model

pytestmark = pytest.mark.gpu
ROUNDS = 6          # Evaluate meets each of its two batch signatures once per run(): two warm-ups, the recording, three replays
ROLLOUT_BATCH = [1, 3]


def _bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


def _same(a, b):
    return a.shape == b.shape and torch.equal(_bits(a), _bits(b))


def _plain(results):
    """SweepResults as exactly comparable values (NaN included)."""
    return [(r.entry, r.steps, r.converged, [float(v).hex() for v in (*r.losses, r.rel_update)]) for r in results]


class _Family:
    """What the test drives: `members` of (rollout, evaluate, sweep) or None, each with a pool of its own (the sweep writes into
    its pool: round k starts from what round k - 1 left there)."""

    def __init__(self, model, members):
        from gfv.evaluate import Evaluate
        from gfv.rollout import Rollout
        from gfv.sweep import Sweep
        self.engine = model.engine()
        self.rollout = self.evaluate = self.sweep = None
        if "rollout" in members:
            self.rollout = Rollout(model, _mesh_pool().batch(ROLLOUT_BATCH)[0], max_steps=ROUNDS + 1)
        if "evaluate" in members:
            self.evaluate = Evaluate(model, _mesh_pool(), max_graphs=2)
        if "sweep" in members:
            self.sweep_pool = _mesh_pool()
            self.sweep = Sweep(model, self.sweep_pool, max_graphs=2, tol=-1, max_steps=3, max_ahead=0)
        self.out = dict(rollout=[], evaluate=[], sweep=[])

    def _guarded(self, fn):
        before = (self.engine._prep_ws, self.engine._fvm_cnt)
        out = fn()
        assert self.engine._prep_ws is before[0] and self.engine._fvm_cnt is before[1], "the engine's own scratch was replaced"
        return out

    def round(self):
        if self.rollout is not None:
            self.out["rollout"].append([t.clone() for t in self._guarded(self.rollout.step)])
        if self.evaluate is not None:
            self.out["evaluate"].append(self._guarded(self.evaluate.run).table)
        if self.sweep is not None:
            res = self._guarded(self.sweep.run)
            self.out["sweep"].append((_plain(res), _fields(self.sweep_pool, range(4))))


def _compare(name, got, want, rounds):
    assert len(got.out[name]) == len(want.out[name]) == rounds
    for k, (a, b) in enumerate(zip(got.out[name], want.out[name])):
        if name == "rollout":
            assert all(_same(x, y) for x, y in zip(a, b)), (name, k)
        elif name == "evaluate":
            assert _same(a, b), (name, k)
        else:
            assert a[0] == b[0], (name, k, a[0], b[0])
            assert all(_same(x, y) for x, y in zip(a[1], b[1])), (name, k)
    if name == "rollout":
        torch.cuda.synchronize()
        assert got.rollout.steps_done == want.rollout.steps_done == rounds
        assert _same(got.rollout.history, want.rollout.history) and _same(got.rollout.x_backup, want.rollout.x_backup)


@pytest.mark.parametrize("hidden", [128, 64])
def test_three_forward_only_users_interleaved_on_one_engine_equal_their_twins_run_alone(hidden):
    together = _Family(_model(hidden), ("rollout", "evaluate", "sweep"))
    alone = {name: _Family(_model(hidden), (name,)) for name in ("rollout", "evaluate", "sweep")}
    for _ in range(ROUNDS):
        together.round()
    for twin in alone.values():
        for _ in range(ROUNDS):
            twin.round()
    for name, twin in alone.items():
        _compare(name, together, twin, ROUNDS)
    # every object warmed up, recorded and replayed, and did so exactly as its twin
    assert len(together.rollout._lists) == 1 and together.rollout._lists.stats() == alone["rollout"].rollout._lists.stats()
    assert together.rollout._lists.stats() == dict(together.rollout._lists.stats(), eager=2, recorded=1, replayed=ROUNDS - 3, lists=1)
    st = together.evaluate.stats()
    print(f"hidden {hidden}: evaluate {st}\nsweep {together.sweep.stats()}\nrollout {together.rollout._lists.stats()}")
    assert st == alone["evaluate"].evaluate.stats()
    assert st == dict(st, batches=2 * ROUNDS, eager=4, recorded=2, replayed=2 * (ROUNDS - 3), lists=2) and st["list_bytes"] > 0
    st = together.sweep.stats()
    assert st == alone["sweep"].sweep.stats()
    assert st == dict(st, steps=6 * ROUNDS, swaps=ROUNDS, eager=4, recorded=2, replayed=6 * ROUNDS - 6, lists=2) and st["list_bytes"] > 0
    # the weights rebuilt where they are (same values): Rollout and Sweep drop their lists, Evaluate keeps them; the next round of
    # each still has the bits of its twin's, which replays
    ptrs = {n: t.data_ptr() for n, t in together.rollout.P.items()}
    for obj in (together.rollout, together.evaluate, together.sweep):
        obj.refresh_weights()
    assert {n: t.data_ptr() for n, t in together.rollout.P.items()} == ptrs
    assert not together.rollout._lists and together.sweep.stats()["lists"] == 0 and together.evaluate.stats()["lists"] == 2
    together.round()
    for name, twin in alone.items():
        twin.round()
        _compare(name, together, twin, ROUNDS + 1)
    assert together.evaluate.stats()["replayed"] == 2 * (ROUNDS - 2) and together.sweep.stats()["recorded"] == 4
