"""Learning-rate schedules on the device (gfv/schedule.py, csrc/sched.hip; include/gfv.h gfv_lr_schedule).

1. the kernel alone, TICK by TICK from epoch 0 to past total_epoch, against the doubles recorded from the reference's classes
   (tests/golden/lr_schedules.json): hyper[0] within ONE fp32 spacing of float32(golden) - the device's double pow may differ
   from libm's in its last bits, and rounding to fp32 turns that into one step at most (the argument of test_march_gpu's
   _within_one_spacing); TABLE and PLATEAU bit for bit (no pow in either);
2. the group rows: float32(lr_double * scale_k), nothing else moves;   3. EVAL is idempotent, FOLLOW;
4. TrainStep(schedule=) against a TrainStep driven by `ts.lr = rate` from the host, bit for bit;
5. MarchStep(schedule=): one scheduler step per time level, independent of how far the host ran ahead;
6. state dicts and the refusals that need the device."""
import json
import math
import os

import numpy as np
import pytest
import torch

import cases
import sched_ref as R
from test_march_gpu import LR, TOL, _assert_same, _bits, _graphs, _model, _state, _within_one_spacing
from test_schedule_cpu import PLATEAU_ARGS, series32, torch_plateau

pytestmark = pytest.mark.gpu

f32 = np.float32
GOLDEN = json.load(open(os.path.join(cases.ROOT, "tests", "golden", "lr_schedules.json")))
ROWS = 34 * 8        # words of the group table: header, GFV_MAX_PARAM_GROUPS rows, the reserved row


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _launch(rec, mode, hyper, table=None, scales=None, n_groups=0, tab=None, metric=None, counter=None):
    from gfv import lib as L
    L.check(L.load().gfv_lr_schedule(rec.data_ptr(), mode, hyper.data_ptr(), None if table is None else table.data_ptr(),
                                     None if scales is None else scales.data_ptr(), n_groups,
                                     None if tab is None else tab.data_ptr(), 0 if tab is None else tab.numel(), metric, counter,
                                     L.stream_ptr()), "gfv_lr_schedule")


def _schedule(case):
    from gfv import schedule as S
    args = dict(case["args"])
    if case["kind"] == "stepexp":
        return S.StepExp(**args, base_lr=case["base_lr"])
    if case["kind"] == "exp":
        return S.Exp(**args, base_lr=case["base_lr"])
    return S.GradualStepExp(**args, base_lr=case["base_lr"])


def _record(rec):
    from gfv import schedule as S
    d = rec.cpu()
    w = d.view(torch.int32)
    return dict(epoch=int(w[S.W_EPOCH]), lr=float(d[S.D_LR]), best=float(d[S.D_BEST]), num_bad=int(w[S.W_NUM_BAD]),
                cooldown_left=int(w[S.W_COOLDOWN_LEFT]))


# ---- 1. the kernel alone -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(GOLDEN["cases"]))
def test_closed_forms_tick_by_tick_within_one_fp32_spacing(name):
    from gfv import lib as L
    case = GOLDEN["cases"][name]
    want = [float.fromhex(h) for h in case["rates"]]
    rec, hyper = _schedule(case).pack().cuda(), torch.zeros(8, device="cuda")
    got, dbl = [], []
    for e in range(len(want)):
        _launch(rec, L.SCHED_EVAL if e == 0 else L.SCHED_TICK, hyper)
        got.append(hyper[0:1].clone())
        dbl.append(rec[8:9].clone())
    got, dbl = torch.cat(got).cpu().numpy(), torch.cat(dbl).cpu().numpy()
    want32 = np.array(want, dtype=np.float64).astype(f32)
    print(f"{name}: {int((got == want32).sum())} of {len(want)} epochs exact in fp32, "
          f"{int((dbl == np.array(want)).sum())} exact in double")
    _within_one_spacing(got, want32, name)
    assert _record(rec)["epoch"] == len(want) - 1
    assert np.array_equal(dbl.astype(f32), got)                            # hyper[0] is the record's rate, rounded once
    if case["kind"] == "stepexp":                                          # in front of the decay no pow enters: the double itself
        flat = range(case["args"]["explr_milestone"])
        assert [float(dbl[e]).hex() for e in flat] == [want[e].hex() for e in flat]
    assert (hyper[1:].cpu() == 0).all()


def test_table_is_bit_for_bit_also_past_its_end():
    from gfv import lib as L
    from gfv import schedule as S
    vals = [3e-3, 1.0 / 3.0 * 1e-3, 7.77e-5, 1e-6, 2.5e-3]
    s = S.Table(vals)
    rec, hyper, tab = s.pack().cuda(), torch.zeros(8, device="cuda"), torch.tensor(vals, dtype=torch.float64).cuda()
    got = []
    for e in range(len(vals) + 3):
        _launch(rec, L.SCHED_EVAL if e == 0 else L.SCHED_TICK, hyper, tab=tab)
        got.append((float(hyper[0]), float(rec[S.D_LR])))
    want = [R.table(e, vals) for e in range(len(vals) + 3)]
    assert [g[1].hex() for g in got] == [w.hex() for w in want]
    assert [g[0] for g in got] == [R.f32(w) for w in want]
    assert _record(rec)["epoch"] == len(vals) + 2
    _launch(rec, L.SCHED_EVAL, hyper)                                      # without a table the rate stays
    assert float(rec[S.D_LR]) == vals[-1] and float(hyper[0]) == R.f32(vals[-1])


@pytest.mark.parametrize("args", PLATEAU_ARGS)
def test_plateau_is_torchs_class_bit_for_bit(args):
    from gfv import lib as L
    from gfv import schedule as S
    metrics = series32()
    want = torch_plateau(1e-3, args, metrics)
    ref = R.Plateau(1e-3, **args)
    rec, hyper = S.Plateau(base_lr=1e-3, **args).pack().cuda(), torch.zeros(8, device="cuda")
    m_dev = torch.tensor(metrics, dtype=torch.float32).cuda()
    _launch(rec, L.SCHED_EVAL, hyper)
    assert float(hyper[0]) == R.f32(1e-3)
    for i, m in enumerate(metrics):
        _launch(rec, L.SCHED_TICK, hyper, metric=m_dev.data_ptr() + 4 * i)
        ref.tick(m)
        got = _record(rec)
        assert got["lr"].hex() == want[i].hex() and float(hyper[0]) == R.f32(want[i]), (i, m)
        assert got == dict(epoch=ref.epoch, lr=ref.lr, best=ref.best, num_bad=ref.num_bad, cooldown_left=ref.cooldown_left), i
    before = rec.cpu().clone()
    _launch(rec, L.SCHED_TICK, hyper)                                      # a TICK without a metric observes nothing
    after = _record(rec)
    assert after["epoch"] == ref.epoch + 1 and {k: v for k, v in after.items() if k != "epoch"} == \
        {k: v for k, v in _record(before).items() if k != "epoch"}


@pytest.mark.parametrize("name", sorted(GOLDEN["warmup"]))
def test_warmup_and_handover_are_the_reference_class_bit_for_bit(name):
    from gfv import lib as L
    from gfv import schedule as S
    case = GOLDEN["warmup"][name]
    s = S.Plateau(base_lr=case["base_lr"], warmup_epochs=case["warmup"]["warmup_epochs"], multiplier=case["warmup"]["multiplier"],
                  **case["plateau"])
    rec, hyper = s.pack().cuda(), torch.zeros(8, device="cuda")
    m_dev = torch.tensor([float.fromhex(m) for m in case["metrics"]], dtype=torch.float32).cuda()
    _launch(rec, L.SCHED_EVAL, hyper)
    got = [float(rec[S.D_LR])]
    for i in range(m_dev.numel()):
        _launch(rec, L.SCHED_TICK, hyper, metric=m_dev.data_ptr() + 4 * i)
        got.append(float(rec[S.D_LR]))
        assert float(hyper[0]) == R.f32(got[-1])
    assert [g.hex() for g in got] == case["rates"]


# ---- 2. the group rows --------------------------------------------------------------------------------------------------------------
def _odd_pair():
    """(lr, scale) whose product rounds differently from float32(lr) * scale, found on the host."""
    rng = np.random.default_rng(5)
    for _ in range(10000):
        lr, scale = float(rng.uniform(1e-5, 1e-3)), float(rng.uniform(0.1, 3.0))
        if R.f32(lr * scale) != R.f32(R.f32(lr) * scale):
            return lr, scale
    raise AssertionError("no such pair")


@pytest.mark.parametrize("n_groups", [1, 3, 32])
def test_group_rows_take_the_double_product_and_nothing_else_moves(n_groups):
    from gfv import lib as L
    from gfv import schedule as S
    lr, odd = _odd_pair()
    scales = ([odd, 0.0, 1.0] * 11)[:n_groups]
    rng = np.random.default_rng(n_groups)
    table0 = rng.standard_normal(ROWS).astype(f32)
    hyper0 = rng.standard_normal(8).astype(f32)
    rec, tab = S.Table([lr]).pack().cuda(), torch.tensor([lr], dtype=torch.float64).cuda()
    table, hyper, sc = _dev(table0), _dev(hyper0), torch.tensor(scales + [9.0] * (32 - n_groups), dtype=torch.float64).cuda()
    _launch(rec, L.SCHED_EVAL, hyper, table=table, scales=sc, n_groups=n_groups, tab=tab)
    want_t, want_h = table0.copy(), hyper0.copy()
    for k, s in enumerate(scales):
        want_t[8 * (1 + k)] = R.group_word(lr, s)
    want_h[0] = R.f32(lr)
    assert np.array_equal(table.cpu().numpy().view(np.int32), want_t.view(np.int32))
    assert np.array_equal(hyper.cpu().numpy().view(np.int32), want_h.view(np.int32))
    assert float(want_t[8]) != R.f32(R.f32(lr) * odd)                                # the case exists: one rounding, not two
    # group_table NULL: only hyper[0] changes
    table2, hyper2 = _dev(table0), _dev(hyper0)
    _launch(rec, L.SCHED_EVAL, hyper2, table=None, scales=sc, n_groups=n_groups, tab=tab)
    assert np.array_equal(hyper2.cpu().numpy().view(np.int32), want_h.view(np.int32))
    assert np.array_equal(table2.cpu().numpy().view(np.int32), table0.view(np.int32))


# ---- 3. EVAL, FOLLOW ---------------------------------------------------------------------------------------------------------------
def test_eval_is_idempotent_and_follow_lands_where_ticks_would():
    from gfv import lib as L
    from gfv import schedule as S
    case = GOLDEN["cases"]["stepexp_gamma"]
    sched = _schedule(case)
    a, b, ha, hb = sched.pack().cuda(), sched.pack().cuda(), torch.zeros(8, device="cuda"), torch.zeros(8, device="cuda")
    counter = torch.zeros(4, dtype=torch.int32, device="cuda")
    for _ in range(8):
        _launch(a, L.SCHED_TICK, ha)                                       # epoch 8: inside the decay
    once = (a.cpu().clone(), ha.cpu().clone())
    _launch(a, L.SCHED_EVAL, ha)
    _launch(a, L.SCHED_EVAL, ha)
    assert torch.equal(_bits(a.cpu()), _bits(once[0])) and torch.equal(_bits(ha.cpu()), _bits(once[1]))
    # FOLLOW with an unchanged counter is EVAL
    counter[0] = 8
    _launch(a, L.SCHED_FOLLOW, ha, counter=counter.data_ptr())
    assert torch.equal(_bits(a.cpu()), _bits(once[0])) and torch.equal(_bits(ha.cpu()), _bits(once[1]))
    # ... and after a jump by 3 it lands where three ticks land
    counter[0] = 11
    _launch(a, L.SCHED_FOLLOW, ha, counter=counter.data_ptr())
    for _ in range(11):
        _launch(b, L.SCHED_TICK, hb)
    assert torch.equal(_bits(a.cpu()), _bits(b.cpu())) and torch.equal(_bits(ha.cpu()), _bits(hb.cpu()))
    assert _record(a)["epoch"] == 11
    _within_one_spacing([float(ha[0])], [R.f32(float.fromhex(case["rates"][11]))], "follow")
    # the cap: a counter beyond it sets the cap's epoch, and going back is followed too
    a.view(torch.int32)[S.W_FOLLOW_CAP:S.W_FOLLOW_CAP + 1].copy_(torch.tensor([9], dtype=torch.int32))
    counter[0] = 10
    _launch(a, L.SCHED_FOLLOW, ha, counter=counter.data_ptr())
    assert _record(a)["epoch"] == 9
    counter[0] = 2
    _launch(a, L.SCHED_FOLLOW, ha, counter=counter.data_ptr())
    assert _record(a)["epoch"] == 2 and float(ha[0]) == R.f32(float.fromhex(case["rates"][2]))


# ---- 4. the wiring is exact ---------------------------------------------------------------------------------------------------------
# epochs 0, 1, 2, 3: LR, LR / 2, then two rates inside the decay (a pow each) - four different rates
SE = dict(startlr=LR, steplr_milestone=1, steplr_gamma=0.5, explr_milestone=1, explr_gamma=1e-1, total_epoch=4, min_lr=1e-6)


def _rate(e):
    return R.stepexp(e, **SE)


@pytest.mark.parametrize("grouped", [False, True], ids=["plain", "groups-guard"])
def test_a_scheduled_trainstep_is_a_trainstep_driven_by_ts_lr(grouped):
    from gfv.schedule import StepExp
    from gfv.trainer import TrainStep
    kw = {}
    if grouped:
        # (lr_scale a power of two: float32(rate) * scale on the host and the device's product from the unrounded rate agree)
        kw = dict(param_groups=[dict(params=["simulator.decoder"], lr_scale=0.5), dict(params=["simulator.encoder"], frozen=True)],
                  max_grad_norm=1e-3)
    ts = TrainStep(_model(), _graphs(), lr=LR, use_graph="list", log=16, schedule=StepExp(**SE), **kw)
    assert ts.lr == LR
    for k in range(12):
        if k and k % 3 == 0:
            ts.schedule.tick()
        if grouped and k == 7:
            ts.loss_weights = (5e4, 4e4, 1.5)
            ts.set_group(0, lr_scale=0.25)
            lr2 = ts.schedule.current_lr()                                 # the record's double: epoch 2, inside the decay
            _within_one_spacing([R.f32(lr2)], [R.f32(_rate(2))], "epoch 2")
            assert float(ts.hyper[0]) == R.f32(lr2)                        # the scheduled rate is still in force
            rows = ts._pg.table.cpu()
            assert float(rows[8]) == R.group_word(lr2, 0.25) and float(rows[24]) == R.f32(lr2)
            assert float(rows[16]) == R.f32(lr2) and rows.view(torch.int32)[18] == 1   # (the frozen row: its rate, its flag)
            assert ts.hyper[5:8].cpu().tolist() == [5e4, 4e4, 1.5]
        ts.step()
    rates = ts.log.read().lr
    want = np.array([_rate(k // 3) for k in range(12)], dtype=np.float64).astype(f32)
    print("rates in the log:", rates, "fp32 steps from the host's:", rates.view(np.int32) - want.view(np.int32))
    _within_one_spacing(rates, want, "log rates")
    assert len({float(r) for r in rates}) == 4 and ts.schedule.epoch == 3
    ref = TrainStep(_model(), _graphs(), lr=LR, use_graph="list", **kw)
    for k in range(12):
        ref.lr = float(rates[k])
        if grouped and k == 7:
            ref.loss_weights = (5e4, 4e4, 1.5)
            ref.set_group(0, lr_scale=0.25)
        ref.step()
    _assert_same(_state(ts), _state(ref), "scheduled against host-driven")
    if grouped:
        assert torch.equal(_bits(ts._pg.table.cpu()), _bits(ref._pg.table.cpu()))
        assert ts.guard_stats() == ref.guard_stats() and ts.guard_stats()["clipped"] > 0
    assert torch.equal(_bits(ts.hyper.cpu()), _bits(ref.hyper.cpu()))


# ---- 5. the march -----------------------------------------------------------------------------------------------------------------
def _sched_march(**kw):
    from gfv.march import MarchStep
    return MarchStep(_model(), _graphs(), lr=LR, use_graph="list", tol=TOL, max_inner=5, max_levels=8, **kw)


def _sched_bits(ms):
    torch.cuda.synchronize()
    return {"rec": ms.schedule.rec.cpu().clone(), "hyper": ms.hyper.cpu().clone()}


def test_a_march_takes_one_scheduler_step_per_level_whatever_the_run_ahead():
    from gfv.schedule import StepExp
    outs = []
    for ahead in (32, 0):
        ms = _sched_march(schedule=StepExp(**SE), log=64)
        rows = ms.run(levels=3, max_ahead=ahead)
        st, log = ms.stats(), ms.log.read()
        outs.append((_state(ms), _sched_bits(ms), rows, st, log))
    (state, sbits, rows, st, log), other = outs[0], outs[1]
    inner = [r["inner"] for r in rows]
    print("inner iterations per level:", inner, "held:", st["held"], "rates:", log.lr)
    level_of = [lv for lv, k in enumerate(inner) for _ in range(k)]
    assert len(level_of) == st["seen"] and len(log.lr) == st["seen"] + st["held"]
    want = np.array([_rate(lv) for lv in level_of] + [_rate(2)] * st["held"], dtype=np.float64).astype(f32)
    _within_one_spacing(log.lr, want, "march log rates")
    assert len({float(v) for v in log.lr}) == 3                            # three levels, three rates
    # the rate changes exactly where a level begins: a level's last step still runs at that level's rate
    changes = [i for i in range(1, st["seen"]) if log.lr[i] != log.lr[i - 1]]
    assert changes == list(np.cumsum(inner)[:-1])
    # the same bits with a synchronisation per step
    assert other[3]["held"] == 0
    _assert_same(state, other[0], "run-ahead")
    _assert_same(sbits, other[1], "run-ahead: schedule")
    assert np.array_equal(log.lr[:st["seen"]].view(np.int32), other[4].lr.view(np.int32))
    # steps past the target leave the rate and the record untouched
    ms = _sched_march(schedule=StepExp(**SE))
    ms.run(levels=3, max_ahead=0)
    before = _sched_bits(ms)
    for _ in range(3):
        ms.step()
    assert ms.stats()["held"] == 3
    _assert_same(_sched_bits(ms), before, "held steps")
    assert ms.schedule.epoch == 2
    _assert_same(_state(ms), state, "held steps: state")
    # ... and a host that sets the rate per level, with a synchronisation per step, computes the same
    host = _sched_march()
    for lv in range(3):
        host.lr = float(log.lr[sum(inner[:lv])])                           # (the rate the device used, read from its log)
        host.run(levels=1, max_ahead=0)
    _assert_same(_state(host), state, "host-driven march")


def test_a_march_without_schedule_is_the_march_it_was():
    a, b = _sched_march(schedule=None), _sched_march()
    ra, rb = a.run(levels=2, max_ahead=8), b.run(levels=2, max_ahead=8)
    assert [r["inner"] for r in ra] == [r["inner"] for r in rb]
    _assert_same(_state(a), _state(b), "schedule=None")
    assert torch.equal(_bits(a.hyper.cpu()), _bits(b.hyper.cpu())) and a.schedule is None


# ---- 6. state dicts and refusals --------------------------------------------------------------------------------------------------
def test_state_dict_continues_a_stepexp_mid_decay():
    from gfv.schedule import StepExp
    from gfv.trainer import TrainStep
    ts = TrainStep(_model(), _graphs(), lr=LR, schedule=StepExp(**SE))
    for _ in range(3):
        ts.schedule.tick()
    ts.step()
    sd = ts.state_dict()
    assert sd["gfv_schedule"]["epoch"] == 3 and sd["gfv_schedule"]["kind"] == "StepExp" and sd["param_groups"][0]["lr"] == LR
    new = TrainStep(_model(), _graphs(), lr=LR, schedule=StepExp(**SE))
    new.load_state_dict(sd)
    assert torch.equal(_bits(new.hyper.cpu()), _bits(ts.hyper.cpu())) and new.schedule.epoch == 3
    for _ in range(3):
        ts.schedule.tick()
        new.schedule.tick()
        assert new.schedule.current_lr() == ts.schedule.current_lr() and float(new.hyper[0]) == float(ts.hyper[0])
    _within_one_spacing([float(new.hyper[0])], [R.f32(_rate(6))], "after the load")
    assert "gfv_schedule" not in TrainStep(new.model, _graphs(), lr=LR).state_dict()
    torch.optim.Adam(new.model.parameters()).load_state_dict(sd)          # (torch ignores the key, like the other gfv_* keys)
    with pytest.raises(ValueError, match="does not load into"):
        new.load_state_dict(dict(sd, gfv_schedule=dict(sd["gfv_schedule"], kind="Exp")))


def test_state_dict_continues_a_plateau_mid_cooldown():
    from gfv.schedule import Plateau
    args, metrics = PLATEAU_ARGS[0], series32()
    want = torch_plateau(1e-3, args, metrics)
    m_dev = torch.tensor(metrics, dtype=torch.float32).cuda()
    p = Plateau(base_lr=1e-3, **args).to("cuda")
    cut = None
    for i in range(len(metrics)):
        p.tick(m_dev[i:i + 1])
        sd = p.state_dict()
        assert sd["lr"] == want[i]
        if sd["cooldown_left"] > 0 and sd["cooldown_left"] < args["cooldown"]:
            cut = i + 1
            break
    assert cut is not None and 0 < sd["cooldown_left"] < args["cooldown"]  # mid-cooldown
    q = Plateau(base_lr=1e-3, **args).to("cuda")
    q.load_state_dict(sd)
    assert q.state_dict() == sd
    for i in range(cut, len(metrics)):
        q.tick(m_dev[i:i + 1])
        assert q.current_lr() == want[i], i
    assert q.epoch == len(metrics)


def test_refusals_that_need_the_device():
    from gfv.march import MarchStep
    from gfv.schedule import Plateau, StepExp
    from gfv.trainer import TrainStep
    model, graphs = _model(), _graphs()
    sched = StepExp(**SE)
    ts = TrainStep(model, graphs, lr=LR, schedule=sched)
    with pytest.raises(RuntimeError, match="owns the learning rate"):
        ts.lr = 1e-4
    with pytest.raises(RuntimeError, match="owns the learning rate"):
        ts.set_lr(1e-4)
    assert ts.lr == LR and float(ts.hyper[0]) == R.f32(LR)
    with pytest.raises(ValueError, match="already attached"):
        TrainStep(model, graphs, lr=LR, schedule=sched)
    with pytest.raises(ValueError, match="Plateau schedule is not supported"):
        MarchStep(model, graphs, lr=LR, schedule=Plateau())
    with pytest.raises(TypeError):
        TrainStep(model, graphs, lr=LR, schedule="StepExp")
    dp = TrainStep(model, graphs, lr=LR, distributed=True, schedule=Plateau(factor=0.5, patience=0))
    with pytest.raises(ValueError, match="rank-local"):
        dp.schedule.tick()
    shared = torch.full((1,), 2.0, device="cuda")
    dp.schedule.tick(shared)                                               # a metric every rank holds alike is taken
    dp.schedule.tick(shared)                                               # (no improvement, patience 0: the rate halves)
    assert dp.schedule.current_lr() == LR * 0.5 and float(dp.hyper[0]) == R.f32(LR * 0.5)
    with pytest.raises(ValueError, match="1-element float32 device tensor"):
        dp.schedule.tick(torch.zeros(1))
    # Plateau.tick() on a step object observes ts.loss
    pl = TrainStep(model, graphs, lr=LR, schedule=Plateau(factor=0.5, patience=0))
    pl.step()
    pl.schedule.tick()
    first = float(pl.loss)
    assert pl.schedule.state_dict()["best"] == first and not math.isnan(first)
