"""CPU: the host side of the parameter groups (include/gfv.h gfv_adam_step_groups_dev, gfv/groups.py) - the
selectors, `no_decay_names`, the run table of a flat layout, the constructor checks of the step objects and of `gfv.optim`, the
new entry point's refusals, and the update formula itself: a float64 restatement kept here equals torch.optim.Adam and
torch.optim.AdamW."""
import ctypes as C
import inspect
import os
import re

import pytest
import torch

import cases


@pytest.fixture(scope="module")
def model():
    from FVMmodel.importer import NNmodel
    from gfv.params import default_params
    return NNmodel(default_params())


def _nt(model):
    return model.param_names_tensors()


# ---- the entry point ---------------------------------------------------------------------------------------------------------
def test_groups_symbol_is_declared_bound_and_exported():
    from gfv import lib
    handle = lib.load()
    header = open(os.path.join(cases.ROOT, "include", "gfv.h")).read()
    declared = set(re.findall(r"\b(gfv_[a-z0-9_]+)\s*\(", header))
    name = "gfv_adam_step_groups_dev"
    assert name in declared and name in lib.declared_symbols() and hasattr(handle, name)
    assert handle.gfv_abi_version() == lib.ABI_VERSION == 3     # an addition
    assert re.search(r"#define\s+GFV_MAX_PARAM_GROUPS\s+32\b", header) and lib.MAX_PARAM_GROUPS == 32
    assert re.search(r"GFV_GROUP_FROZEN\s*=\s*1\b", header) and lib.GROUP_FROZEN == 1


def test_groups_entry_point_rejects_bad_arguments_without_a_gpu():
    """Negative return codes, nothing launched: the pointers below are host memory no kernel may ever see."""
    from gfv import lib
    handle = lib.load()
    buf = (C.c_double * 512)()
    a = C.addressof(buf)
    e = a + 2048

    def adam(p=a, g=a, m=a, v=a, e=e, n=4, state=a, hyper=a, grd=a, acc=a, rec=a, rs=a, rg=a, runs=1, tab=a):
        return handle.gfv_adam_step_groups_dev(p, g, m, v, e, n, state, hyper, grd, acc, rec, rs, rg, runs, tab, None)
    for name in ("p", "g", "m", "v", "state", "hyper", "rs", "rg", "tab"):
        assert adam(**{name: None}) < 0, name
        assert adam(grd=None, acc=None, e=None, rec=None, **{name: None}) < 0, name
    assert adam(e=None) < 0 and adam(rec=None) < 0              # the average and its record come together
    assert adam(e=a) < 0 and adam(e=a + 4) < 0                  # e overlapping p[0, n)
    assert adam(n=0) < 0 and adam(n=-5) < 0
    assert adam(runs=0) < 0 and adam(runs=-1) < 0
    assert adam(runs=1025) < 0 and lib.MAX_PARAM_RUNS == 1024       # the run starts are staged in LDS: a longer table is refused


# ---- selectors ---------------------------------------------------------------------------------------------------------------
def test_a_string_selects_a_name_and_everything_below_it(model):
    from gfv.groups import select
    names, tensors = _nt(model)
    enc = select(names, tensors, ["simulator.encoder"])
    assert enc and enc == [n for n in names if n.startswith("simulator.encoder.")]
    one = select(names, tensors, ["simulator.encoder.eb_encoder.0.0.weight"])
    assert one == ["simulator.encoder.eb_encoder.0.0.weight"]
    # a prefix is a whole dotted component: "simulator.processpr_list.1" does not select "...processpr_list.10" or half a name
    assert select(names, tensors, ["simulator.processpr_list.1"]) == [n for n in names if n.startswith("simulator.processpr_list.1.")]
    with pytest.raises(ValueError, match="selects no parameter"):
        select(names, tensors, ["simulator.enc"])
    by_fn = select(names, tensors, lambda n, t: t.dim() >= 2)
    assert by_fn == [n for n, t in zip(names, tensors) if t.dim() >= 2]


def test_groups_overlap_empty_default_and_limit(model):
    from gfv.groups import MAX_GROUPS, check_groups
    names, tensors = _nt(model)
    with pytest.raises(ValueError, match="selected by groups 0 and 1"):
        check_groups(names, tensors, 0.0, True, [{"params": ["simulator.encoder"]}, {"params": ["simulator.encoder.nb_encoder"]}])
    with pytest.raises(ValueError, match="selects no parameter"):
        check_groups(names, tensors, 0.0, True, [{"params": ["nothing.here"]}])
    with pytest.raises(ValueError, match="unknown keys"):
        check_groups(names, tensors, 0.0, True, [{"params": ["simulator.encoder"], "lr": 1e-3}])
    for bad in (-0.1, float("nan"), float("inf"), True, "0.1"):
        with pytest.raises(ValueError, match="weight_decay"):
            check_groups(names, tensors, bad)
        with pytest.raises(ValueError, match="lr_scale"):
            check_groups(names, tensors, 0.0, True, [{"params": ["simulator.encoder"], "lr_scale": bad}])
    spec = check_groups(names, tensors, 0.05, True, [{"params": ["simulator.encoder"], "frozen": True},
                                                      {"params": ["simulator.decoder"], "lr_scale": 0.1, "weight_decay": 0.0}])
    assert len(spec.groups) == 3                                   # the two given + the default group behind them
    assert spec.groups[2]["names"] == [n for n in names if n.startswith("simulator.processpr_list.")]
    assert sorted(n for g in spec.groups for n in g["names"]) == sorted(names)
    assert spec.values(2e-3) == [(2e-3, 0.05, True), (2e-3 * 0.1, 0.0, False), (2e-3, 0.05, False)]
    assert spec.frozen_names() == set(spec.groups[0]["names"]) and not spec.trivial
    # set_group checks everything before it changes anything
    assert spec.set_group(1, frozen=True) is True
    with pytest.raises(ValueError, match="nothing left to optimise"):
        spec.set_group(2, lr_scale=0.5, frozen=True)
    with pytest.raises(ValueError, match="weight_decay"):
        spec.set_group(2, lr_scale=0.5, weight_decay=-1.0)
    assert spec.groups[2]["lr_scale"] == 1.0 and spec.groups[2]["frozen"] is False
    assert spec.set_group(1, frozen=False) is True and spec.set_group(1, frozen=False) is False
    assert check_groups(names, tensors).trivial and len(check_groups(names, tensors).groups) == 1
    assert not check_groups(names, tensors, 0.01).trivial
    # the limit counts the implicit default group
    one_each = [{"params": [n]} for n in names[:MAX_GROUPS]]
    with pytest.raises(ValueError, match="at most 32"):
        check_groups(names, tensors, 0.0, True, one_each)          # 32 given + the default group = 33
    assert len(check_groups(names, tensors, 0.0, True, one_each[:MAX_GROUPS - 1]).groups) == MAX_GROUPS


def test_no_decay_names_are_the_biases_and_the_vectors(model):
    from gfv.groups import no_decay_names
    got = no_decay_names(model)
    named = dict(model.named_parameters())
    assert len(got) == len(set(got)) and set(got) <= set(named)
    for n, p in named.items():
        long_axes = sum(1 for d in p.shape if d > 1)
        if n in got:
            assert n.endswith("bias") or long_axes <= 1, n
        else:
            assert p.dim() >= 2 and long_axes >= 2 and not n.endswith("bias"), n
    assert all(n in got for n in named if n.endswith(".bias") or ".ln_" in n or n.endswith("temperature"))
    assert any(n.endswith("temperature") for n in got)


# ---- the run table -----------------------------------------------------------------------------------------------------------
def test_build_runs_one_run_per_tensor_padding_inside(model):
    from gfv.engine import GradStore
    from gfv.functions import unused_param_names
    from gfv.groups import RESERVED, build_runs, check_groups
    names, tensors = _nt(model)
    skip = unused_param_names(names)
    assert skip
    store = GradStore(names, [t.shape for t in tensors], "cpu", skip=skip)
    spec = check_groups(names, tensors, 0.1, True, [{"params": ["simulator.encoder"]}, {"params": ["simulator.decoder"]}])
    starts, rows = build_runs(store, spec.group_of)
    assert len(rows) == len(names) and len(starts) == len(names) + 1
    assert starts[0] == 0 and starts[-1] == store.total and all(a <= b for a, b in zip(starts, starts[1:]))
    for r, (n, t) in enumerate(zip(names, tensors)):
        assert starts[r] == store.off[n]
        assert starts[r + 1] - starts[r] == (t.numel() + 3) // 4 * 4       # the alignment padding belongs to the tensor's run
        assert rows[r] == (RESERVED if n in skip else spec.group_of[n])
    assert any(starts[r + 1] - starts[r] > tensors[r].numel() for r in range(len(names)))
    # bare tensors of odd sizes, dealt round-robin
    sizes = [1, 3, 17, 511, 512, 513, 4101]
    store = GradStore([str(i) for i in range(len(sizes))], [(k,) for k in sizes], "cpu")
    starts, rows = build_runs(store, {str(i): i % 3 for i in range(len(sizes))})
    assert rows == [0, 1, 2, 0, 1, 2, 0] and starts == [0, 4, 8, 28, 540, 1052, 1568, 5672]
    with pytest.raises(ValueError):
        build_runs(store, {str(i): 33 for i in range(len(sizes))})
    from gfv.groups import ParamGroups
    many = GradStore([str(i) for i in range(1025)], [(1,)] * 1025, "cpu")
    with pytest.raises(ValueError, match="at most 1024 runs"):
        ParamGroups(many, "cpu", {str(i): 0 for i in range(1025)}, [(1e-3, 0.0, False)], True)


# ---- constructors ------------------------------------------------------------------------------------------------------------
def test_the_step_objects_take_the_three_arguments():
    from gfv.pool_trainer import PoolTrainStep
    from gfv.trainer import TrainStep
    for cls in (TrainStep, PoolTrainStep):
        params = inspect.signature(cls.__init__).parameters
        for name, default in (("weight_decay", 0.0), ("decoupled_weight_decay", True), ("param_groups", None)):
            assert params[name].default == default and params[name].kind is inspect.Parameter.KEYWORD_ONLY, name
    assert isinstance(TrainStep.weight_decay, property) and isinstance(TrainStep.param_groups, property)
    assert callable(PoolTrainStep.set_group)


def test_trainstep_refuses_bad_groups_before_anything_touches_a_device(model):
    from gfv.pool_trainer import PoolTrainStep
    from gfv.trainer import TrainStep
    for cls in (TrainStep, PoolTrainStep):
        with pytest.raises(ValueError, match="weight_decay"):
            cls(model, None, weight_decay=-1.0)
        with pytest.raises(ValueError, match="selects no parameter"):
            cls(model, None, param_groups=[{"params": ["no.such.block"]}])
        with pytest.raises(ValueError, match="selected by groups"):
            cls(model, None, param_groups=[{"params": ["simulator"]}, {"params": ["simulator.decoder"]}])


def test_optim_constructor_refusals():
    from gfv.optim import Adam, AdamW
    ps = [torch.nn.Parameter(torch.randn(5)) for _ in range(3)]
    with pytest.raises(NotImplementedError, match="amsgrad"):
        Adam(ps, amsgrad=True)
    with pytest.raises(NotImplementedError, match="maximize"):
        Adam(ps, maximize=True)
    with pytest.raises(NotImplementedError, match="amsgrad"):
        AdamW(ps, amsgrad=True)
    with pytest.raises(NotImplementedError, match="betas or eps"):
        Adam([{"params": ps[:1], "betas": (0.8, 0.9)}, {"params": ps[1:]}])
    with pytest.raises(NotImplementedError, match="betas or eps"):
        AdamW([{"params": ps[:1]}, {"params": ps[1:], "eps": 1e-6}])
    with pytest.raises(ValueError, match="weight_decay"):
        Adam(ps, weight_decay=-0.1)
    many = [torch.nn.Parameter(torch.randn(2)) for _ in range(33)]
    with pytest.raises(ValueError, match="at most 32"):
        Adam([{"params": [p]} for p in many])
    # what used to be refused - a decay, a second group, a frozen one - now gets as far as "these are CPU tensors"
    for build in (lambda: Adam(ps, weight_decay=0.1),
                  lambda: Adam(ps, weight_decay=0.1, decoupled_weight_decay=True),
                  lambda: AdamW(ps),
                  lambda: Adam([{"params": ps[:1], "lr": 3e-3}, {"params": ps[1:], "weight_decay": 0.5}]),
                  lambda: AdamW([{"params": ps[:2]}, {"params": ps[2:], "frozen": True}])):
        with pytest.raises(RuntimeError, match="fp32 parameters on the GPU"):
            build()
    sig = inspect.signature(AdamW.__init__).parameters
    assert sig["weight_decay"].default == 1e-2 and sig["lr"].default == 1e-3


# ---- the formula -------------------------------------------------------------------------------------------------------------
def restated_step(p, m, v, g, t, lr, wd, decoupled, b1=0.9, b2=0.999, eps=1e-8):
    """One step of the update as include/gfv.h states it, float64; t = the step count this step carries (1 for the first)."""
    if wd != 0 and not decoupled:
        g = g + wd * p
    if wd != 0 and decoupled:
        p = p * (1.0 - lr * wd)
    m = m * b1 + (1.0 - b1) * g
    v = v * b2 + (1.0 - b2) * g * g
    step_size = lr / (1.0 - b1 ** t)
    denom = v.sqrt() / (1.0 - b2 ** t) ** 0.5 + eps
    return p - step_size * (m / denom), m, v


@pytest.mark.parametrize("decoupled", [False, True], ids=["Adam", "AdamW"])
def test_the_restated_update_is_torchs(decoupled):
    gen = torch.Generator().manual_seed(5)
    sizes = [1, 3, 17, 511]
    groups = [(1e-3, 0.1), (3e-3, 0.0), (5e-4, 0.5)]
    start = [torch.randn(k, generator=gen, dtype=torch.float64) for k in sizes]
    ps = [torch.nn.Parameter(t.clone()) for t in start]
    no_grad = 2                                             # a parameter of the 0.5-decay group that never gets a gradient
    cls = torch.optim.AdamW if decoupled else torch.optim.Adam
    opt = cls([{"params": ps[k::3], "lr": lr, "weight_decay": wd} for k, (lr, wd) in enumerate(groups)])
    mine = [(t.clone(), torch.zeros_like(t), torch.zeros_like(t)) for t in start]
    for step in range(5):
        grads = [torch.randn(k, generator=gen, dtype=torch.float64) * (1 + step) for k in sizes]
        for i, p in enumerate(ps):
            p.grad = None if i == no_grad else grads[i].clone()
        opt.step()
        for i in range(len(sizes)):
            if i == no_grad:
                continue
            lr, wd = groups[i % 3]
            mine[i] = restated_step(*mine[i], grads[i], step + 1, lr, wd, decoupled)[0:3]
            mine[i] = (mine[i][0], mine[i][1], mine[i][2])
    for i, p in enumerate(ps):
        assert float((p.detach() - mine[i][0]).abs().max()) <= 1e-12, i
        if i != no_grad:
            st = opt.state[p]
            assert float((st["exp_avg"] - mine[i][1]).abs().max()) <= 1e-12
            assert float((st["exp_avg_sq"] - mine[i][2]).abs().max()) <= 1e-12
    assert torch.equal(ps[no_grad].detach(), start[no_grad]) and len(opt.state[ps[no_grad]]) == 0
