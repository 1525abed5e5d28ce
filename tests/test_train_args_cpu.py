"""CPU: the one constructor check of the step objects (`gfv.trainer.check_train_args`).  `TrainStep` and `PoolTrainStep` call it
before they touch a device, a batch or a pool, so every refusal below is raised by the CONSTRUCTORS with no GPU present.  The
message each must carry is the one the feature's own check (`check_policy`, `check_accum_steps`, `check_ema`, `check_groups`,
`check_schedule`, `check_balance`, `check_observe`, `timescheme.check_owner`) raises for the same arguments: those functions are
what the constructors called one by one before, so "the same message as before" is "the same as theirs"."""
import pytest
import torch

from gfv import balance as Bal
from gfv import schedule as S
from gfv import timescheme as T
from gfv.accum import check_accum_steps
from gfv.ema import check_ema
from gfv.groups import check_groups
from gfv.guard import check_policy
from gfv.observe import ObservationTerm, Observations, PoolObservations, check_observe
from gfv.pool_trainer import PoolTrainStep
from gfv.trainer import TrainStep, check_train_args


class _Model:
    """All the check reads of a model: names and tensors of its parameters."""
    NAMES, TENSORS = ["enc.weight", "dec.weight", "dec.bias"], [torch.zeros(4, 4), torch.zeros(4, 4), torch.zeros(4)]

    def param_names_tensors(self):
        return self.NAMES, self.TENSORS


class _Pool:
    """A pool nothing may be asked of before the arguments have been checked."""

    def arena(self, *a, **kw):
        raise AssertionError("the arena was asked for before the arguments were checked")


def _term(kind, owner=None, pool=None):
    term = kind.__new__(kind)                  # (Observations' own constructor wants device tensors)
    ObservationTerm.__init__(term, 1.0)
    term._owner, term.pool = owner, pool
    return term


def _taken(obj):
    obj._owner = "TrainStep"
    return obj


def _cases(who, kind, pool):
    """(constructor keywords, the feature's own check with the arguments the constructor gives it) per refusal."""
    names, tensors = _Model.NAMES, _Model.TENSORS
    junk, bal, sch = object(), Bal.Inverse(), S.Table([3e-3, 2e-3])
    term, other = _term(kind, pool=pool), _term(Observations if kind is PoolObservations else PoolObservations, pool=pool)
    groups = [{"params": ["no such parameter"]}]
    out = [
        (dict(max_grad_norm=-1.0), lambda: check_policy(-1.0, False, False)),
        (dict(max_grad_norm=float("nan")), lambda: check_policy(float("nan"), False, False)),
        (dict(skip_on_flag=True, distributed=True), lambda: check_policy(None, True, True)),
        (dict(accum_steps=0), lambda: check_accum_steps(0, False)),
        (dict(accum_steps=True), lambda: check_accum_steps(True, False)),
        (dict(accum_steps=2, distributed=True), lambda: check_accum_steps(2, True)),
        (dict(ema_decay=1.5), lambda: check_ema(1.5, True)),
        (dict(ema_decay=1.0, ema_warmup=False), lambda: check_ema(1.0, False)),
        (dict(weight_decay=-1.0), lambda: check_groups(names, tensors, -1.0, True, None)),
        (dict(param_groups=groups), lambda: check_groups(names, tensors, 0.0, True, groups)),
        (dict(param_groups=[{"params": ["dec"], "momentum": 0.9}]),
         lambda: check_groups(names, tensors, 0.0, True, [{"params": ["dec"], "momentum": 0.9}])),
        (dict(schedule=junk), lambda: S.check_schedule(junk)),
        (dict(schedule=_taken(S.Table([1e-3]))), lambda: S.check_schedule(_taken(S.Table([1e-3])))),
        (dict(balance=junk), lambda: Bal.check_balance(junk, False, 1, who)),
        (dict(balance=bal, distributed=True), lambda: Bal.check_balance(bal, True, 1, who)),
        (dict(balance=_taken(Bal.Inverse())), lambda: Bal.check_balance(_taken(Bal.Inverse()), False, 1, who)),
        (dict(observations=junk), lambda: check_observe(junk, None, who, kind)),
        (dict(observations=other), lambda: check_observe(other, None, who, kind)),
        (dict(observations=term, balance=bal), lambda: check_observe(term, bal, who, kind)),
        (dict(observations=_term(kind, "TrainStep", pool)), lambda: check_observe(_term(kind, "TrainStep", pool), None, who, kind)),
        # the order of the checks is part of what a caller sees: the first of two bad arguments is the one reported
        (dict(max_grad_norm=-1.0, accum_steps=0, ema_decay=1.5, schedule=sch), lambda: check_policy(-1.0, False, False)),
        (dict(ema_decay=1.5, weight_decay=-1.0, balance=junk), lambda: check_ema(1.5, True)),
        (dict(schedule=junk, balance=junk, observations=junk), lambda: S.check_schedule(junk)),
    ]
    if who == "TrainStep":
        out += [
            (dict(skip_on_flag=True, world_size=2), lambda: check_policy(None, True, True)),
            (dict(accum_steps=2, world_size=2), lambda: check_accum_steps(2, True)),
            (dict(balance=bal, world_size=2), lambda: Bal.check_balance(bal, True, 2, who)),
            (dict(balance=bal, world_size=2, distributed=False), lambda: Bal.check_balance(bal, False, 2, who)),
            (dict(time_scheme="bdf2"), lambda: T.check_owner("bdf2")),
            (dict(time_scheme=_taken(T.TimeScheme())), lambda: T.check_owner(_taken(T.TimeScheme()))),
        ]
    return out


def _refusal(fn):
    with pytest.raises((ValueError, TypeError)) as e:
        fn()
    return type(e.value), str(e.value)


def _same_but_for_addresses(got, want):
    """The messages that print an argument with `repr` name an object each side made for itself: compared up to the address."""
    import re
    strip = lambda s: re.sub(r"0x[0-9a-f]+", "0x", s)
    return got[0] is want[0] and strip(got[1]) == strip(want[1])


@pytest.mark.parametrize("cls,kind", [(TrainStep, Observations), (PoolTrainStep, PoolObservations)], ids=["TrainStep", "PoolTrainStep"])
def test_every_refusal_is_made_without_a_device_and_reads_as_before(cls, kind):
    who, pool = cls.__name__, _Pool()
    second = pool if cls is PoolTrainStep else None          # (TrainStep: graphs=None - nothing is asked of them either)
    cases = _cases(who, kind, pool)
    assert len(cases) >= 23
    for kw, own_check in cases:
        want = _refusal(own_check)
        assert _same_but_for_addresses(_refusal(lambda: check_train_args(who, kind, _Model(), **kw)), want), (kw, want)
        assert _same_but_for_addresses(_refusal(lambda: cls(_Model(), second, **kw)), want), (kw, want)
    # where a message names the object it names the class's own, not its parent's
    assert _refusal(lambda: cls(_Model(), second, balance=Bal.Inverse(), distributed=True))[1].startswith(who + ": balance=")


def test_what_the_check_returns_is_what_the_constructor_goes_on_with():
    dist_on, accum, ema, spec = check_train_args("TrainStep", Observations, _Model())
    assert (dist_on, accum, ema) == (False, 1, None) and spec.trivial
    dist_on, accum, ema, spec = check_train_args("TrainStep", Observations, _Model(), world_size=2, accum_steps=1, ema_decay=0.9,
                                                 param_groups=[{"params": ["dec"], "lr_scale": 0.5}], lr=1e-3, betas=(0.9, 0.99))
    assert dist_on is True and ema == check_ema(0.9, True) and not spec.trivial and len(spec.groups) == 2
    assert check_train_args("TrainStep", Observations, _Model(), world_size=2, distributed=False)[0] is False
    assert check_train_args("TrainStep", Observations, _Model(), distributed=True)[0] is True


def test_pool_train_step_keeps_its_own_refusals_and_makes_them_before_the_arena():
    pool = _Pool()
    with pytest.raises(ValueError, match=r'PoolTrainStep: use_graph must be False or "list" \(the hipGraph mode is bound to one batch\)'):
        PoolTrainStep(_Model(), pool, use_graph=True)
    with pytest.raises(ValueError, match="PoolTrainStep: time_scheme= is not supported .the pool owns the fields"):
        PoolTrainStep(_Model(), pool, time_scheme=T.TimeScheme())
    with pytest.raises(ValueError, match="PoolTrainStep: the PoolObservations were built on another pool than the one to train on"):
        PoolTrainStep(_Model(), pool, observations=PoolObservations(_Pool()))
    with pytest.raises(ValueError, match="max_grad_norm"):
        PoolTrainStep(_Model(), pool, max_grad_norm=-1.0)
    for unknown in ("world_size", "process_group", "momentum"):
        with pytest.raises(TypeError, match=unknown):
            PoolTrainStep(_Model(), pool, **{unknown: 1})
    with pytest.raises(TypeError, match="momentum"):
        TrainStep(_Model(), None, momentum=1)
    # ... and with nothing to refuse the arena is the next thing it asks for
    with pytest.raises(AssertionError, match="the arena was asked for"):
        PoolTrainStep(_Model(), pool, max_grad_norm=1.0, observations=PoolObservations(pool))
    import inspect
    params = inspect.signature(PoolTrainStep.__init__).parameters
    assert params["use_graph"].default == "list" and params["max_list_bytes"].default == 16 << 30
    ours = {k: v.default for k, v in inspect.signature(TrainStep.__init__).parameters.items()
            if k not in ("self", "model", "graphs", "world_size", "process_group", "use_graph")}
    assert all(params[k].default == v and params[k].kind is inspect.Parameter.KEYWORD_ONLY for k, v in ours.items())
