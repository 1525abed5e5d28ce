"""CPU: the host side of the averaged weights (include/gfv.h gfv_ema_init / gfv_adam_step_ema_dev, gfv/ema.py) - the new entry
points are declared, bound and exported, refuse bad arguments before anything touches a device, `check_ema` and `ema_weight`
say what the device record will hold, and the step objects take the two new arguments."""
import ctypes as C
import inspect
import math
import os
import re

import pytest

import cases

NEW = ("gfv_ema_init", "gfv_adam_step_ema_dev")


def test_ema_symbols_are_declared_bound_and_exported():
    from gfv import lib
    handle = lib.load()
    header = open(os.path.join(cases.ROOT, "include", "gfv.h")).read()
    declared = set(re.findall(r"\b(gfv_[a-z0-9_]+)\s*\(", header))
    for name in NEW:
        assert name in declared, name
        assert name in lib.declared_symbols(), name
        assert hasattr(handle, name), name
    assert handle.gfv_abi_version() == lib.ABI_VERSION == 3     # new entry points only


def test_ema_entry_points_reject_bad_arguments_without_a_gpu():
    """Negative return codes, nothing launched: the pointers below are host memory no kernel may ever see."""
    from gfv import lib
    handle = lib.load()
    buf = (C.c_double * 512)()      # 8-byte aligned stand-in for every pointer argument
    a = C.addressof(buf)
    e = a + 2048                    # the second half: 4 floats there do not overlap 4 floats at `a`

    def init(rec=a, decay=0.9, warmup=1, updates=0):
        return handle.gfv_ema_init(rec, decay, warmup, updates, None)
    assert init(rec=None) < 0
    for decay in (1.0, 1.5, -0.1, -1e-30, float("inf"), float("nan")):
        assert init(decay=decay) < 0, decay
        assert init(decay=decay, warmup=0) < 0, decay
    assert init(decay=0.99999999) < 0                          # 1.0f as the fp32 value the record would hold
    assert init(warmup=2) < 0 and init(warmup=-1) < 0
    assert init(updates=-1) < 0

    def adam(p=a, g=a, m=a, v=a, e=e, n=4, state=a, hyper=a, grd=a, acc=a, rec=a):
        return handle.gfv_adam_step_ema_dev(p, g, m, v, e, n, state, hyper, grd, acc, rec, None)
    for name in ("p", "g", "m", "v", "e", "state", "hyper", "rec"):
        assert adam(**{name: None}) < 0, name
        assert adam(grd=None, acc=None, **{name: None}) < 0, name   # (guard == NULL, accum == NULL alone: the plain form)
    assert adam(e=a) < 0 and adam(e=a, grd=None, acc=None) < 0      # e == p
    assert adam(e=a + 4) < 0 and adam(p=e, e=e - 8) < 0             # e overlapping p[0, n)
    assert adam(n=0) < 0 and adam(n=-5) < 0


@pytest.mark.parametrize("ok", [None, 0, 0.5, 0.999])
def test_check_ema_accepts(ok):
    from gfv.ema import check_ema
    got = check_ema(ok, True)
    assert got is None if ok is None else (isinstance(got, float) and got == ok)
    assert check_ema(ok, False) == got


@pytest.mark.parametrize("bad", [1, -0.1, float("nan"), True, "0.9"])
def test_bad_ema_decay_is_a_value_error(bad):
    from gfv.ema import check_ema
    from gfv.pool_trainer import PoolTrainStep
    from gfv.trainer import TrainStep
    with pytest.raises(ValueError, match="ema_decay"):
        check_ema(bad, True)
    # (the check sits beside check_policy in the constructors: no model, batch or GPU is needed to be told)
    with pytest.raises(ValueError, match="ema_decay"):
        TrainStep(None, None, ema_decay=bad)
    with pytest.raises(ValueError, match="ema_decay"):
        PoolTrainStep(None, None, ema_decay=bad)


def test_a_decay_that_is_one_in_fp32_is_a_value_error():
    from gfv.ema import check_ema
    with pytest.raises(ValueError, match="fp32"):
        check_ema(0.99999999, True)


@pytest.mark.parametrize("k", [0, 1, 8, 9, 10 ** 6])
def test_ema_weight_states_the_formula(k):
    from gfv.ema import ema_weight
    for d in (0.0, 0.5, 0.9, 0.999):
        assert ema_weight(d, False, k) == 1.0 - d
        ramp = (1.0 + k) / (10.0 + k)
        want = 1.0 - min(d, ramp)
        assert ema_weight(d, True, k) == want
        assert 0.0 < ema_weight(d, True, k) <= 1.0
    # the ramp by hand: 1/10, 2/11, 9/18, 10/19
    by_hand = {0: 0.9, 1: 9.0 / 11.0, 8: 0.5, 9: 9.0 / 19.0}
    if k in by_hand:
        assert math.isclose(ema_weight(0.999, True, k), by_hand[k], rel_tol=0, abs_tol=1e-15)
    else:
        assert math.isclose(ema_weight(0.999, True, k), 1.0 - 0.999, rel_tol=0, abs_tol=1e-15)   # the ramp is past the decay


def test_ema_weight_examples():
    """The first update of a warmed-up average weighs the parameters 0.9 whatever the decay (d_eff = min(decay, 1 / 10) = 0.1 for
    every decay >= 0.1), and a decay of 0.5 is reached when the ramp (1 + k) / (10 + k) is: at k = 8.
    (The issue behind this feature lists `ema_weight(0.5, True, 0) == 0.5` as an example.  Its own formula, the one the device
    evaluates, gives 1 - min(0.5, 0.1) = 0.9 there and 0.5 from k = 8 on; no formula gives both that example and its neighbour
    `ema_weight(0.999, True, 0) == 0.9` without contradicting the stated one.  The formula is what is asserted.)"""
    from gfv.ema import ema_weight
    assert ema_weight(0.999, True, 0) == 0.9
    assert ema_weight(0.5, True, 0) == 0.9
    assert ema_weight(0.5, False, 0) == 0.5
    assert all(ema_weight(0.5, True, k) == 0.5 for k in (8, 9, 10 ** 6))
    assert ema_weight(0.05, True, 0) == 0.95     # a decay below the ramp's start is not raised to it


def test_the_step_objects_take_the_two_arguments():
    from gfv.pool_trainer import PoolTrainStep
    from gfv.trainer import TrainStep
    for cls in (TrainStep, PoolTrainStep):
        params = inspect.signature(cls.__init__).parameters
        assert params["ema_decay"].default is None and params["ema_decay"].kind is inspect.Parameter.KEYWORD_ONLY
        assert params["ema_warmup"].default is True and params["ema_warmup"].kind is inspect.Parameter.KEYWORD_ONLY
    for name in ("ema_decay", "ema_warmup"):
        assert isinstance(getattr(TrainStep, name), property)
    for name in ("ema_reset", "ema_stats", "ema_parameters", "ema_weights"):
        assert callable(getattr(PoolTrainStep, name))
