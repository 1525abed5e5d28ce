"""Loss balancing on the device (gfv/balance.py, csrc/balance.hip; include/gfv.h gfv_loss_balance).

1. the kernel alone against tests/balance_ref.py, launch by launch through `observe()`: integer words exact; m, s, s_ref, lam, the
   running power and the record's w to relative 1e-12 (at most ~B float64 roundings in a sum - 2.2e-14 at B = 200 - and the device
   exp within a few units of the last place of libm's; the rest is margin), with an absolute floor of 1e-300 for values that are
   zero; hyper[5:8] within 4 fp32 spacings of float32(reference) (differences far below one fp32 spacing can still flip the final
   rounding); hyper[0:5] bit for bit what it was;
2. the launch lands BEHIND its step's Adam: a balanced run equals an unbalanced one that is given the same fp32 weights from the
   host in front of every step, bit for bit;
3. eager, recorded list and hipGraph: record, weights and parameters bit for bit;
4. accumulation: the weights move only behind applied steps;   5. PoolTrainStep on the recorded path with changing B;
6. a state dict continues a run bit for bit;   7. the balancer owns hyper[5:8]."""
import copy

import numpy as np
import pytest
import torch

import balance_ref as R
from test_march_gpu import LR, _assert_same, _bits, _graphs, _model

pytestmark = pytest.mark.gpu

f32 = np.float32
W0 = (6e4, 5e4, 1.0)
REL, ABS, SPACINGS = 1e-12, 1e-300, 4


def _spacings_apart(got, want):
    """fp32 steps between two arrays of finite fp32 values of one sign."""
    got, want = np.asarray(got, dtype=f32), np.asarray(want, dtype=f32)
    assert np.all(np.isfinite(got)) and np.all(np.isfinite(want)), (got, want)
    return np.abs(got.view(np.int32).astype(np.int64) - want.view(np.int32).astype(np.int64))


def _state(ts):
    """Parameters, moments and step count by name, the balancer's record and hyper, as CPU copies (synchronises).  The alignment
    padding between the tensors of the flat buffers is not state (its gradient slots take whatever the shared weight-gradient
    workspace held, which depends on warm-up passes and on the object's history): TrainStep.named_state() leaves it out."""
    torch.cuda.synchronize()
    out = {"named": torch.cat([t.reshape(-1) for pmv in ts.named_state().values() for t in pmv]).cpu(),
           "adam_t": ts.adam_state[0:1].cpu().clone(), "hyper": ts.hyper.cpu().clone()}
    if ts.balance is not None:
        out["rec"] = ts.balance.rec.cpu().clone()
    return out


def _read(rec):
    from gfv import balance as Bal
    return Bal.state_of(rec.cpu())


def _compare_record(rec, ref, what):
    got = _read(rec)
    assert {k: got[k] for k in ("n", "n_applied", "n_updates", "n_skipped")} == ref.words(), what
    want = dict(power=[ref.power], ema=ref.m, last=ref.s, s_ref=ref.s_ref, lam=ref.lam, weights=ref.w)
    worst = 0.0
    for key, vals in want.items():
        have = [got[key]] if key == "power" else got[key]
        for g, w in zip(have, vals):
            assert abs(g - w) <= REL * abs(w) + ABS, (what, key, g, w)
            worst = max(worst, abs(g - w) / abs(w) if w else 0.0)
    return worst


# ---- 1. the kernel alone -----------------------------------------------------------------------------------------------------------
HOLDS = [None, 1, 1, 0, None, 1, None, 1, 0, 1, 1, None]      # the hold word of each launch: absent, 1 or 0
NAN_AT, NEG_AT, ZERO_PRESS_AT = 4, 7, 9


def _script(B, seed):
    """12 launches of [B, 4] fp32 terms falling at different rates; one with a NaN term, one whose mom_x is negative on every graph
    (a negative statistic), one with press == 0 on every graph."""
    rng = np.random.default_rng(seed)
    out = []
    for i in range(len(HOLDS)):
        a = np.empty((B, 4), dtype=f32)
        a[:, 0] = 1e-3 * 0.8 ** i * rng.uniform(0.5, 1.5, B)
        a[:, 1] = 4e-3 * 0.95 ** i * rng.uniform(0.5, 1.5, B)
        a[:, 2] = 2e-3 * 0.9 ** i * rng.uniform(0.5, 1.5, B)
        a[:, 3] = 0.3 * 0.6 ** i * rng.uniform(0.5, 1.5, B)
        if i == NAN_AT:
            a[B // 2, 0] = np.nan
        if i == NEG_AT:
            a[:, 1] = -1.0
        if i == ZERO_PRESS_AT:
            a[:, 3] = 0.0
        out.append(a)
    return out


@pytest.mark.parametrize("decay", [0.0, 0.6])
@pytest.mark.parametrize("kind", ["inverse", "progress"])
@pytest.mark.parametrize("B", [1, 3, 64, 65, 200])
def test_the_kernel_alone_launch_by_launch(B, kind, decay):
    from gfv import balance as Bal
    if kind == "inverse":
        bal = Bal.Inverse(shares=(2, 1, 1), decay=decay, warmup=2, every=2)
        ref = R.Balance(R.INVERSE, W0, g=(2, 1, 1), decay=decay, warmup=2, every=2)
    else:
        bal = Bal.Progress(alpha=0.7, tau=0.5, decay=decay, warmup=2, every=2)
        ref = R.Balance(R.PROGRESS, W0, decay=decay, warmup=2, every=2, alpha=0.7, tau=0.5)
    bal.set_base(W0)
    bal.to("cuda")
    hyper0 = np.random.default_rng(B).uniform(0.5, 2.0, 8).astype(f32)
    hyper = torch.from_numpy(hyper0.copy()).cuda()
    ref_hyper = [float(v) for v in hyper0]
    hold = torch.zeros(1, dtype=torch.int32, device="cuda")
    publishes, floor_bound, worst, apart = [], False, 0.0, 0
    for i, (terms, h) in enumerate(zip(_script(B, 100 + B), HOLDS)):
        if h is not None:
            hold.fill_(h)
        bal.observe(torch.from_numpy(terms).cuda(), B, hyper=hyper, hold=None if h is None else hold)
        did = ref.observe(terms.tolist(), hold=h, hyper=ref_hyper)
        if did:
            publishes.append(i)
            floor_bound |= (ref.mh[2] if kind == "inverse" else ref.s_ref[2]) < ref.floor
        worst = max(worst, _compare_record(bal.rec, ref, (B, kind, i)))
        got = hyper.cpu().numpy()
        assert np.array_equal(got[:5].view(np.int32), hyper0[:5].view(np.int32)), i      # hyper[0:5]: bit for bit what it was
        steps = _spacings_apart(got[5:8], np.array(ref_hyper[5:8], dtype=np.float64).astype(f32))
        apart = max(apart, int(steps.max()))
        assert steps.max() <= SPACINGS, (B, kind, i, got[5:8], ref_hyper[5:8])
        if not publishes:
            assert np.array_equal(got[5:8].view(np.int32), hyper0[5:8].view(np.int32)), i
    print(f"B={B} {kind} decay={decay}: publishes at {publishes}, worst relative difference of a double {worst:.2e}, "
          f"hyper[5:8] at most {apart} fp32 spacings from the reference")
    assert publishes == [5, 9, 11] and ref.n_skipped == 2 and ref.n == 10 and ref.n_applied == 8
    assert bal.stats()["n_updates"] == 3 and bal.stats()["weights"] == _read(bal.rec)["weights"]
    if decay == 0.0:
        assert floor_bound                                                  # press == 0 met a publish: the floor was the divisor


def test_observe_without_an_owner_uses_its_own_hyper_and_reset_restores_it():
    from gfv import balance as Bal
    bal = Bal.Inverse(decay=0.0, warmup=0)
    bal.set_base((2.0, 3.0, 4.0))
    bal.to("cuda")
    assert bal.to("cuda") is bal and bal._own_hyper[5:8].cpu().tolist() == [2.0, 3.0, 4.0]
    ptr = bal.rec.data_ptr()
    terms = torch.tensor([[1.0, 0.5, 0.5, 4.0]], device="cuda")
    bal.observe(terms, 1)
    # R0 = 2 + 3 + 16 = 21, every class a third of it
    assert bal._own_hyper[5:8].cpu().tolist() == [7.0, 7.0, 1.75] and bal._own_hyper[:5].cpu().tolist() == [0.0] * 5
    assert bal.stats() == dict(n=1, n_applied=1, n_updates=1, n_skipped=0, weights=[7.0, 7.0, 1.75], ema=[1.0, 1.0, 4.0],
                               last=[1.0, 1.0, 4.0])
    bal.set_base((1.0, 1.0, 1.0))
    bal.reset()
    assert bal.rec.data_ptr() == ptr and bal._own_hyper[5:8].cpu().tolist() == [1.0, 1.0, 1.0]
    assert torch.equal(bal.rec.cpu().view(torch.int64), bal.pack().view(torch.int64))
    with pytest.raises(ValueError, match="contiguous float32 device tensor"):
        bal.observe(terms, 2)
    with pytest.raises(ValueError, match="int32 device tensor"):
        bal.observe(terms, 1, hold=torch.zeros(1, device="cuda"))


# ---- 2. timing of effect -------------------------------------------------------------------------------------------------------------
def _weights(ts):
    return ts.hyper[5:8].cpu().clone()


def _step_bits(ts):
    torch.cuda.synchronize()
    return {"loss": ts.loss.cpu().clone(), "losses": ts.losses.cpu().clone(), "flat_p": ts.flat_p.cpu().clone(),
            "named": torch.cat([t.reshape(-1) for pmv in ts.named_state().values() for t in pmv]).cpu()}


def test_the_launch_lands_behind_its_steps_adam():
    from gfv.balance import Inverse
    from gfv.trainer import TrainStep
    a = TrainStep(_model(), _graphs(), lr=LR, balance=Inverse(warmup=1, every=1, decay=0.5))
    assert a.balance is not None and a.loss_weights == W0
    used, outs = [], []
    for _ in range(6):
        used.append(_weights(a))                                           # what this step's loss reads
        a.step()
        outs.append(_step_bits(a))
    assert torch.equal(used[0], torch.tensor(W0, dtype=torch.float32)) and torch.equal(used[1], used[0])     # (warmup 1)
    assert all(not torch.equal(used[k], used[k - 1]) for k in range(2, 6))  # from the second observation on the weights move
    st = a.balance.stats()
    assert (st["n"], st["n_applied"], st["n_updates"], st["n_skipped"]) == (6, 6, 5, 0)
    b = TrainStep(_model(), _graphs(), lr=LR)
    for k in range(6):
        b.loss_weights = tuple(float(v) for v in used[k])                  # fp32 values: exactly representable
        b.step()
        _assert_same(_step_bits(b), outs[k], f"step {k}")


# ---- 3. launch modes -----------------------------------------------------------------------------------------------------------------
def test_launch_modes_are_bit_identical():
    from gfv.balance import Progress
    from gfv.trainer import TrainStep
    outs = []
    for mode in (False, "list", True):
        ts = TrainStep(_model(), _graphs(), lr=LR, use_graph=mode, balance=Progress(alpha=0.5, tau=0.05, warmup=1, decay=0.5))
        for _ in range(6):
            ts.step()
        outs.append(_state(ts))
        assert ts.balance.stats()["n_updates"] == 5
    assert not torch.equal(outs[0]["hyper"][5:8], torch.tensor(W0, dtype=torch.float32))
    _assert_same(outs[1], outs[0], "list against eager")
    _assert_same(outs[2], outs[0], "hipGraph against eager")


# ---- 4. accumulation -----------------------------------------------------------------------------------------------------------------
def test_under_accumulation_the_weights_move_only_behind_applied_steps():
    from gfv.balance import Inverse
    from gfv.trainer import TrainStep
    ts = TrainStep(_model(), _graphs(), lr=LR, use_graph="list", accum_steps=2, balance=Inverse(warmup=1, every=1, decay=0.5))
    seen = [_weights(ts)]
    for _ in range(8):
        ts.step()
        seen.append(_weights(ts))
    for i in range(8):
        moved = not torch.equal(seen[i + 1], seen[i])
        assert moved == (i % 2 == 1), (i, seen[i], seen[i + 1])           # micro-step i closes an accumulation iff i is odd
    st = ts.balance.stats()
    assert (st["n"], st["n_applied"], st["n_updates"], st["n_skipped"]) == (8, 4, 4, 0)
    assert ts.accum_stats()["closed"] == 4


# ---- 5. PoolTrainStep ----------------------------------------------------------------------------------------------------------------
def test_a_pool_step_with_changing_batches_follows_the_reference():
    from gfv.balance import Inverse
    from gfv.pool_trainer import PoolTrainStep
    from test_pool_train_gpu import _model as pool_model
    from test_pool_train_gpu import _three_size_pool
    ts = PoolTrainStep(pool_model(), _three_size_pool(), max_graphs=2, lr=1e-3, use_graph="list",
                       balance=Inverse(shares=(1, 2, 1), warmup=1, every=1, decay=0.5))
    ref = R.Balance(R.INVERSE, ts.loss_weights, g=(1, 2, 1), decay=0.5, warmup=1, every=1)
    ref_hyper = [0.0] * 5 + [R.f32(v) for v in ts.loss_weights]
    worst = 0
    for k in range(10):
        idx = [0] if k % 2 == 0 else [0, 1]
        ts.step(idx)
        terms = ts.losses.cpu().numpy().reshape(len(idx), 4)
        assert ref.observe(terms.tolist(), hyper=ref_hyper) == (k >= 1)
        steps = _spacings_apart(ts.hyper[5:8].cpu().numpy(), np.array(ref_hyper[5:8], dtype=np.float64).astype(f32))
        worst = max(worst, int(steps.max()))
        assert steps.max() <= SPACINGS, (k, steps)
    print("pool: hyper[5:8] at most", worst, "fp32 spacings from the reference; lists:", ts.stats())
    assert ts.stats()["replayed"] >= 2 and ts.stats()["lists"] == 2
    _compare_record(ts.balance.rec, ref, "pool")


# ---- 6. resume -----------------------------------------------------------------------------------------------------------------------
def test_a_state_dict_continues_a_balanced_run_bit_for_bit():
    from gfv.balance import Progress
    from gfv.trainer import TrainStep

    def make():
        return TrainStep(_model(), _graphs(), lr=LR, balance=Progress(alpha=0.5, tau=0.05, warmup=1, decay=0.5))
    whole = make()
    for _ in range(6):
        whole.step()
    want = _state(whole)
    first = make()
    for _ in range(3):
        first.step()
    sd, model_sd = copy.deepcopy(first.state_dict()), copy.deepcopy(first.model.state_dict())
    assert sd["gfv_balance"]["kind"] == "Progress" and sd["gfv_balance"]["n_updates"] == 2
    assert tuple(sd["gfv_loss_weights"]) == W0
    second = make()
    second.model.load_state_dict(model_sd)
    second.load_state_dict(sd)
    second.sync_from_model()
    assert torch.equal(_bits(second.hyper.cpu()), _bits(first.hyper.cpu()))
    assert torch.equal(_bits(second.balance.rec.cpu()), _bits(first.balance.rec.cpu()))
    for _ in range(3):
        second.step()
    _assert_same(_state(second), want, "resumed")
    plain = TrainStep(second.model, _graphs(), lr=LR)
    assert "gfv_balance" not in plain.state_dict() and plain.balance is None
    torch.optim.Adam(second.model.parameters()).load_state_dict(sd)       # (torch ignores the key, like the other gfv_* keys)
    with pytest.raises(ValueError, match="does not load into"):
        first.load_state_dict(dict(sd, gfv_balance=dict(sd["gfv_balance"], kind="Inverse")))


# ---- 7. who owns hyper[5:8] ----------------------------------------------------------------------------------------------------------
def test_the_balancer_owns_the_weight_words():
    from gfv.balance import Inverse
    from gfv.march import MarchStep
    from gfv.trainer import TrainStep
    model, graphs = _model(), _graphs()
    bal = Inverse(warmup=0, every=1, decay=0.5)
    ts = TrainStep(model, graphs, lr=LR, loss_weights=(3e4, 2e4, 2.0), balance=bal)
    assert ts.balance is bal and ts.loss_weights == (3e4, 2e4, 2.0) and ts.hyper[5:8].cpu().tolist() == [3e4, 2e4, 2.0]
    ts.step()
    before = ts.hyper.cpu().clone()
    assert before[5:8].tolist() != [3e4, 2e4, 2.0]                         # (warmup 0: the first step published)
    ts.betas = (0.8, 0.99)
    ts.eps = 1e-7
    after = ts.hyper.cpu().clone()
    assert torch.equal(_bits(after[5:8]), _bits(before[5:8])) and after[1:4].tolist() == [R.f32(0.8), R.f32(0.99), R.f32(1e-7)]
    with pytest.raises(RuntimeError, match="set_base"):
        ts.loss_weights = (1.0, 1.0, 1.0)
    assert torch.equal(_bits(ts.hyper.cpu()), _bits(after)) and ts.loss_weights == (3e4, 2e4, 2.0)
    ts.balance.set_base((1e4, 1e4, 1.0))
    assert ts.loss_weights == (1e4, 1e4, 1.0) and torch.equal(_bits(ts.hyper.cpu()), _bits(after))   # (the next publish follows)
    ts.step()
    assert _read(bal.rec)["w0"] == [1e4, 1e4, 1.0] and ts.balance.stats()["n_updates"] == 2
    with pytest.raises(ValueError, match="already attached"):
        TrainStep(model, graphs, lr=LR, balance=bal)
    with pytest.raises(ValueError, match="balance= is not supported"):
        MarchStep(model, graphs, lr=LR, balance=Inverse())
    with pytest.raises(ValueError, match="data parallelism"):
        TrainStep(model, graphs, lr=LR, distributed=True, balance=Inverse())
    with pytest.raises(TypeError):
        TrainStep(model, graphs, lr=LR, balance="inverse")
