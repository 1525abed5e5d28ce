"""CPU: the host side of the device learning-rate schedules (gfv/schedule.py, csrc/sched.hip): the entry point is declared,
exported and bound and refuses bad arguments before anything touches a device; tests/sched_ref.py - the restatement the GPU tests
compare the kernel with - equals the doubles recorded from the reference's classes (tests/golden/lr_schedules.json) and torch's
ReduceLROnPlateau exactly; the record a new object packs; the constructor refusals; Table.from_torch.  Nothing here touches a GPU."""
import ctypes as C
import json
import math
import os
import re

import pytest
import torch

import cases
import sched_ref as R

GOLDEN = json.load(open(os.path.join(cases.ROOT, "tests", "golden", "lr_schedules.json")))
# the plateau series: improvements inside and outside the threshold, a run longer than patience, a cooldown, the min_lr floor, the
# eps cut-off and one NaN
SERIES = [1.0, 0.9, 0.8995, 0.8999, 0.91, 0.92, 0.93, 0.94, 0.5, 0.51, float("nan"), 0.52, 0.53, 0.54, 0.55, 0.4999, 0.56, 0.57,
          0.58, 0.59, 0.6, 0.61, 0.62, 0.63, 0.64, 0.65, 0.66, 0.67, 0.68, 0.69, 0.7, 0.71]
PLATEAU_ARGS = [dict(factor=0.1, patience=2, threshold=1e-3, cooldown=2, min_lr=3e-6, eps=1e-8),
                dict(factor=0.5, patience=0, threshold=1e-4, cooldown=0, min_lr=0.0, eps=2e-4),
                dict(factor=0.3, patience=1, threshold=0.2, cooldown=1, min_lr=1e-4, eps=0.0)]


def series32():
    return [R.f32(m) for m in SERIES]


def torch_plateau(base_lr, args, metrics):
    """The rates torch's class leaves in a CPU optimiser after each metric."""
    opt = torch.optim.SGD([torch.nn.Parameter(torch.zeros(1))], lr=base_lr)
    sch = torch.optim.lr_scheduler.ReduceLROnPlateau(opt, mode="min", threshold_mode="rel", **args)
    out = []
    for m in metrics:
        opt.step()
        sch.step(m)
        out.append(float(opt.param_groups[0]["lr"]))
    return out


def test_schedule_entry_point_is_declared_exported_and_bound():
    from gfv import cmdlist, lib
    from gfv import schedule as S
    handle = lib.load()
    header = open(os.path.join(cases.ROOT, "include", "gfv.h")).read()
    declared = set(re.findall(r"\b(gfv_[a-z0-9_]+)\s*\(", header))
    declared -= {"gfv_seg_t", "gfv_layer_t", "gfv_rowtile_args_t", "gfv_dw_tile_t", "gfv_wimg_desc_t", "gfv_reduce_piece_t"}
    name = "gfv_lr_schedule"
    assert name in declared and name in lib.declared_symbols() and hasattr(handle, name)
    assert len(getattr(handle, name).argtypes) == 11
    assert declared == set(lib.declared_symbols()), declared ^ set(lib.declared_symbols())
    assert handle.gfv_abi_version() == 3 and lib.ABI_VERSION == 3          # additive: the version stays
    assert name not in cmdlist._QUERIES                                    # it launches: part of a recorded list
    for macro, value in (("RECORD", lib.SCHED_RECORD), ("MAX_MILESTONES", lib.SCHED_MAX_MILESTONES), ("EVAL", lib.SCHED_EVAL),
                         ("TICK", lib.SCHED_TICK), ("FOLLOW", lib.SCHED_FOLLOW), ("STEPEXP", lib.SCHED_STEPEXP),
                         ("EXP", lib.SCHED_EXP), ("GRADUAL", lib.SCHED_GRADUAL), ("TABLE", lib.SCHED_TABLE),
                         ("PLATEAU", lib.SCHED_PLATEAU)):
        assert int(re.search(rf"#define GFV_SCHED_{macro} (\d+)", header).group(1)) == value, macro
    assert (R.EVAL, R.TICK, R.FOLLOW) == (lib.SCHED_EVAL, lib.SCHED_TICK, lib.SCHED_FOLLOW)
    # the words the header states, where gfv/schedule.py writes them
    for word, idx in (("kind", S.W_KIND), ("epoch", S.W_EPOCH), ("n_milestones", S.W_N_MILESTONES), ("num_bad", S.W_NUM_BAD),
                      ("cooldown_left", S.W_COOLDOWN_LEFT), ("patience", S.W_PATIENCE), ("cooldown", S.W_COOLDOWN),
                      ("warmup_epochs", S.W_WARMUP), ("steplr_milestone", S.W_STEP_MILESTONE),
                      ("explr_milestone", S.W_EXP_MILESTONE), ("total_epoch", S.W_TOTAL_EPOCH), ("follow_cap", S.W_FOLLOW_CAP)):
        assert re.search(rf"\bw\[{idx}\]\s+{word}\b", header), word
    for word, idx in (("lr", S.D_LR), ("base_lr", S.D_BASE_LR), ("min_lr", S.D_MIN_LR), ("gamma", S.D_GAMMA),
                      ("expgamma", S.D_EXPGAMMA), ("decay_steps", S.D_DECAY_STEPS), ("startlr", S.D_START_LR), ("best", S.D_BEST),
                      ("factor", S.D_FACTOR), ("threshold", S.D_THRESHOLD), ("eps", S.D_EPS), ("multiplier", S.D_MULTIPLIER)):
        assert re.search(rf"\bd\[{idx}\]\s+{word}\b", header), word
    assert S.W_MILESTONES == 40 and S.W_MILESTONES + lib.SCHED_MAX_MILESTONES <= 2 * lib.SCHED_RECORD


def test_lr_schedule_rejects_bad_arguments_before_touching_a_device():
    from gfv import lib as L
    lib = L.load(raw=True)
    buf = (C.c_double * 64)()          # host memory stands in for every device pointer: a refused call reads none of them
    p = C.cast(buf, C.c_void_p).value
    ok = dict(rec=p, mode=L.SCHED_FOLLOW, hyper=p, gt=p, scales=p, ng=3, table=p, tl=4, metric=p, counter=p)

    def call(**kw):
        a = {**ok, **kw}
        return lib.gfv_lr_schedule(a["rec"], a["mode"], a["hyper"], a["gt"], a["scales"], a["ng"], a["table"], a["tl"],
                                   a["metric"], a["counter"], None)
    assert call(rec=None) == -1 and call(hyper=None) == -1
    assert call(rec=p + 4) == -1                                           # not 8-byte aligned
    assert call(mode=3) == -1 and call(mode=-1) == -1
    assert call(counter=None) == -1                                        # FOLLOW without its counter
    assert call(ng=-1) == -1 and call(ng=L.MAX_PARAM_GROUPS + 1) == -1
    assert call(scales=None) == -1                                         # group rows without their scales
    assert call(tl=-1) == -1 and call(table=None) == -1                    # a table length without a table


@pytest.mark.parametrize("name", sorted(GOLDEN["cases"]))
def test_closed_forms_equal_the_reference_classes_exactly(name):
    case = GOLDEN["cases"][name]
    want = [float.fromhex(h) for h in case["rates"]]
    args = dict(case["args"])
    args.pop("multiplier", None)                                           # (acts in the plateau branch only)
    if case["kind"] != "stepexp" or case["base_lr"] != args["startlr"]:
        args["base_lr"] = case["base_lr"]
    got = [R.rate(case["kind"], args, e) for e in range(len(want))]
    assert [g.hex() for g in got] == [w.hex() for w in want]
    if case["kind"] != "exp":
        assert len(want) > args["total_epoch"] + 1                         # past total_epoch


def test_the_fixture_covers_what_the_gpu_test_steps_through():
    c = GOLDEN["cases"]
    assert c["stepexp_driver"]["args"] == dict(startlr=1e-3, steplr_milestone=2, steplr_gamma=1, explr_milestone=10,
                                               explr_gamma=1e-1, total_epoch=20, min_lr=1e-6)
    assert any(v["kind"] == "stepexp" and v["args"]["steplr_gamma"] != 1 for v in c.values())
    assert any(v["args"]["min_lr"] > v["base_lr"] for v in c.values() if v["kind"] == "stepexp")
    assert {len(v["args"]["milestone"]) for v in c.values() if v["kind"] == "gradual"} >= {0, 1, 8}


@pytest.mark.parametrize("name", sorted(GOLDEN["warmup"]))
def test_warmup_and_handover_equal_the_reference_class_exactly(name):
    case = GOLDEN["warmup"][name]
    p = R.Plateau(case["base_lr"], warmup_epochs=case["warmup"]["warmup_epochs"], multiplier=case["warmup"]["multiplier"],
                  **case["plateau"])
    got = [p.lr] + [p.tick(float.fromhex(m)) for m in case["metrics"]]
    assert [g.hex() for g in got] == case["rates"]


@pytest.mark.parametrize("args", PLATEAU_ARGS)
def test_plateau_rule_equals_torch_exactly(args):
    metrics = series32()
    want = torch_plateau(1e-3, args, metrics)
    p = R.Plateau(1e-3, **args)
    got = [p.tick(m) for m in metrics]
    assert [g.hex() for g in got] == [w.hex() for w in want]
    assert p.epoch == len(metrics)


def test_the_plateau_series_takes_every_branch():
    """What the series is said to contain, shown on the restatement's own state."""
    metrics = series32()
    assert sum(1 for m in metrics if math.isnan(m)) == 1
    seen = set()
    for args in PLATEAU_ARGS:
        p = R.Plateau(1e-3, **args)
        for m in metrics:
            before, best, cool = p.lr, p.best, p.cooldown_left
            p.tick(m)
            if not math.isnan(m) and m < best and p.best == best:
                seen.add("improvement inside the threshold")
            if p.best != best:
                seen.add("improvement")
            if cool > 0:
                seen.add("cooldown")
            if p.lr < before:
                seen.add("reduced")
                if p.lr == args["min_lr"]:
                    seen.add("floor")
            if p.lr == before and p.cooldown_left == args["cooldown"] and p.num_bad == 0 and cool == 0 and p.best == best \
                    and before - max(before * args["factor"], args["min_lr"]) <= args["eps"]:
                seen.add("eps cut-off")
    assert seen >= {"improvement inside the threshold", "improvement", "cooldown", "reduced", "floor", "eps cut-off"}, seen


def test_a_new_objects_record_is_what_the_header_states():
    from gfv import lib as L
    from gfv import schedule as S
    s = S.StepExp(1e-3, 2, 0.5, 10, 1e-1, 20, 1e-6)
    d = s.pack()
    w = d.view(torch.int32)
    assert d.numel() == L.SCHED_RECORD and d.dtype == torch.float64
    assert [int(w[i]) for i in range(12)] == [L.SCHED_STEPEXP, 0, 0, 0, 0, 0, 0, 0, 2, 10, 20, -1]
    assert [float(v) for v in d[8:16]] == [1e-3, 1e-3, 1e-6, 0.5, 1e-1, 10.0, 1e-3, math.inf]
    g = S.GradualStepExp(1.0, [5, 3, 3, 0], 0.1, 1e-2, 8, 12, base_lr=2e-3)
    w = g.pack().view(torch.int32)
    assert int(w[S.W_KIND]) == L.SCHED_GRADUAL and int(w[S.W_N_MILESTONES]) == 3          # (sorted, a repeated one counted once)
    assert [int(w[S.W_MILESTONES + i]) for i in range(4)] == [0, 3, 5, 0]
    p = S.Plateau(factor=0.5, patience=3, threshold=1e-3, cooldown=2, min_lr=1e-6, eps=1e-9, warmup_epochs=4, multiplier=2.0,
                  base_lr=1e-3)
    d = p.pack()
    w = d.view(torch.int32)
    assert [int(w[i]) for i in (S.W_KIND, S.W_EPOCH, S.W_PATIENCE, S.W_COOLDOWN, S.W_WARMUP)] == [L.SCHED_PLATEAU, 1, 3, 2, 4]
    assert float(d[S.D_LR]) == R.warmup(1, 1e-3, 2.0, 4) and float(d[S.D_BEST]) == math.inf
    assert [float(d[i]) for i in (S.D_FACTOR, S.D_THRESHOLD, S.D_EPS, S.D_MULTIPLIER)] == [0.5, 1e-3, 1e-9, 2.0]
    t = S.Table([3e-3, 2e-3, 1e-3])
    assert int(t.pack().view(torch.int32)[S.W_KIND]) == L.SCHED_TABLE and float(t.pack()[S.D_LR]) == 3e-3


def test_constructor_refusals():
    from gfv import schedule as S
    with pytest.raises(ValueError, match="milestone should be smaller than total_epoch"):
        S.GradualStepExp(1.0, [3, 9], 0.1, 1e-2, 8, 12)
    with pytest.raises(ValueError, match="multiplier should be greater"):
        S.GradualStepExp(0.5, [3], 0.1, 1e-2, 8, 12)
    with pytest.raises(ValueError, match="multiplier should be greater"):
        S.Plateau(multiplier=0.99)
    with pytest.raises(ValueError, match="at most 8"):
        S.GradualStepExp(1.0, list(range(9)), 0.1, 1e-2, 20, 12)
    with pytest.raises(ValueError, match="Factor should be < 1.0"):
        S.Plateau(factor=1.0)
    with pytest.raises(ValueError, match="must exceed explr_milestone"):
        S.StepExp(1e-3, 2, 1.0, 10, 1e-1, 10, 1e-6)
    for bad in (dict(startlr=float("nan")), dict(steplr_milestone=-1), dict(steplr_milestone=1.5), dict(explr_gamma=0.0),
                dict(min_lr=-1e-6), dict(total_epoch=True)):
        kw = dict(startlr=1e-3, steplr_milestone=2, steplr_gamma=1.0, explr_milestone=10, explr_gamma=1e-1, total_epoch=20,
                  min_lr=1e-6)
        kw.update(bad)
        with pytest.raises(ValueError):
            S.StepExp(**kw)
    with pytest.raises(ValueError):
        S.Exp(decay_steps=0)
    with pytest.raises(ValueError):
        S.Plateau(patience=-1)
    with pytest.raises(ValueError, match="at least one rate"):
        S.Table([])
    with pytest.raises(ValueError):
        S.Table([1e-3, float("inf")])
    with pytest.raises(ValueError, match="base_lr is not known"):
        S.Exp().pack()                                                     # (no owner, no base rate)
    with pytest.raises(ValueError, match="takes no metric"):
        S.Exp(base_lr=1e-3).tick(metric=torch.zeros(1))
    with pytest.raises(RuntimeError, match="no device record"):
        S.Exp(base_lr=1e-3).tick()
    with pytest.raises(TypeError):
        S.check_schedule(torch.optim.lr_scheduler.StepLR)
    with pytest.raises(ValueError, match="Plateau schedule is not supported"):
        from gfv.march import check_step_args
        check_step_args("list", dict(schedule=S.Plateau()))


def test_table_from_torch_is_the_scheduler_it_was_made_from():
    from gfv import schedule as S
    base, n = 3e-3, 25
    makers = [lambda o: torch.optim.lr_scheduler.CosineAnnealingLR(o, T_max=20, eta_min=1e-5),
              lambda o: torch.optim.lr_scheduler.LambdaLR(o, lambda e: 1.0 / (1.0 + 0.3 * e)),
              lambda o: torch.optim.lr_scheduler.MultiStepLR(o, [3, 7, 11], gamma=0.3)]
    for make in makers:
        t = S.Table.from_torch(make, base, n)
        opt = torch.optim.Adam([torch.nn.Parameter(torch.zeros(2))], lr=base)
        sch = make(opt)
        want = []
        for _ in range(n):
            want.append(float(opt.param_groups[0]["lr"]))
            opt.step()
            sch.step()
        assert [v.hex() for v in t.values] == [w.hex() for w in want]
        assert [R.table(e, t.values) for e in (0, 5, n - 1, n, n + 7)] == [want[0], want[5], want[-1], want[-1], want[-1]]
